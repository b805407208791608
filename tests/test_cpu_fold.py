"""The fold's host side without a GPU: the fixture (tests/golden/fold_chains.npz) still meets the conditions it was searched for under
the float64 oracle (tests/fold_oracle.py), the PDB writer round-trips through the project's own reader, and the oracle's restraint
counts equal a direct count from the maps."""
import json
import math

import numpy as np
import pytest

import fold_oracle as FO
from helpers import load_golden

KEYS = ("48", "96", "96cut", "132")
NAMES = ("dist", "omega", "theta", "phi")


@pytest.fixture(scope="module")
def gold():
    g = load_golden("fold_chains")
    g["meta"] = json.loads(str(g["meta"]))
    return g


def _maps(gold, key):
    return {nm: gold[f"{nm}_{key}"].astype(np.float64) for nm in NAMES}


def test_ideal_cb_constants():
    """The constexpr values the kernels are compiled with, read out of csrc/backbone_geom.h (fold.hip takes them from there), against the
    oracle's own derivation: |Cb - CA| and N-CA-Cb from the virtual-Cb identity at N-CA 1.458, CA-C 1.525, N-CA-C 111.0, to the six
    decimals they are written with.  The float twins the fp32 kernels use are the doubles rounded once, each held by a static_assert to
    the float literal of the same digits; no kernel file spells the identity's constants itself."""
    import glob
    import os
    import re
    csrc = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "text2protein_amd", "csrc")
    geom = open(os.path.join(csrc, "backbone_geom.h")).read()
    names = {"K1": "K1", "K2": "K2", "K3": "K3", "N_CA": "BOND_N_CA", "C_N": "BOND_C_N", "R_CB": "R_CB", "COS_NCACB": "COS_NCACB", "SIN_NCACB": "SIN_NCACB"}
    text = dict(re.findall(r"\b(K1|K2|K3|BOND_N_CA|BOND_C_N|R_CB|COS_NCACB|SIN_NCACB) = (-?\d+\.\d+)[,;]", geom))
    assert len(text) == 8, text
    found = {k: float(text[v]) for k, v in names.items()}
    want = {"K1": FO.K1, "K2": FO.K2, "K3": FO.K3, "N_CA": FO.N_CA, "C_N": FO.C_N, "R_CB": FO.R_CB, "COS_NCACB": math.cos(FO.A_NCACB),
            "SIN_NCACB": math.sin(FO.A_NCACB)}
    for k, v in want.items():
        assert abs(found[k] - v) <= (5.01e-7 if k in ("R_CB", "COS_NCACB", "SIN_NCACB") else 0.0), (k, found[k], v)
    fold_src = open(os.path.join(csrc, "fold.hip")).read()
    assert '#include "backbone_geom.h"' in fold_src and "using namespace geom;" in fold_src
    for v in names.values():                                   # the fp32 kernels' constants: (float) of the double, equal to the float literal
        assert f"{v}_F = (float){v}" in geom and f"{v}_F == {text[v]}f" in geom and f"{v}_F" in fold_src, v
    assert "cb_offset(bv, cv)" in fold_src                     # the score's double Cb: the header's one formula
    for path in glob.glob(os.path.join(csrc, "*.hip")):
        assert not re.search(r"0\.58273431|0\.56802827|0\.54067466", open(path).read()), path


@pytest.mark.parametrize("key", KEYS)
def test_oracle_meets_the_fixture_conditions(gold, key):
    xyz, maps, rep = gold[f"xyz_{key}"], _maps(gold, key), gold["meta"]["chains"][key]
    n = xyz.shape[0]
    assert n == rep["n"] == {"48": 48, "96": 96, "96cut": 37, "132": 132}[key]
    ca = xyz[:, 1]
    dca = np.linalg.norm(ca[:, None] - ca[None], axis=-1)
    assert dca[np.abs(np.arange(n)[:, None] - np.arange(n)[None]) >= 3].min() >= 4.0
    cb = FO.virtual_cb(xyz)
    dcb = np.linalg.norm(cb[:, None] - cb[None], axis=-1)
    off = ~np.eye(n, dtype=bool)
    assert min(np.abs(dcb[off] - v).min() for v in (12.0, 19.0, 20.0)) >= 1e-3
    near = off & (dcb <= 20.0)
    assert np.abs(maps["dist"] - np.where(near, dcb, 20.0))[off].max() < 1e-5          # the stored maps are this chain's
    d, known, nb = FO.pairs(maps["dist"])
    assert FO.geodesics(d, known)[1] == 0 and nb.sum(1).min() >= 4
    for i in range(n):
        e = cb[nb[i]] - cb[i]
        w = np.linalg.eigvalsh((e / np.linalg.norm(e, axis=1)[:, None]).T @ (e / np.linalg.norm(e, axis=1)[:, None]))
        assert w[0] >= 0.05 * w[-1]
    f = FO.fold(maps)
    rmsd = FO.kabsch_rmsd(f["xyz"][:, 1], ca)
    print(f"oracle on chain {key}: CA RMSD {rmsd:.4f}, all-atom {FO.kabsch_rmsd(f['xyz'].reshape(-1, 3), xyz.reshape(-1, 3)):.4f}, "
          f"closure {f['closure']}, hand {f['hand']}, stress rms {f['stress_rms']:.4f}, known pairs {f['known_fraction']:.2f}")
    # the fixture's figure was taken on the float64 maps, this one on their float32 copies (what a decode gives)
    assert f["status"] == 0 and f["placed"] == [] and rmsd < 0.5 and abs(rmsd - rep["oracle_ca_rmsd"]) < 1e-3
    assert abs(f["closure"][0] - f["closure"][1]) > 0.5 and f["hand"] == rep["hand"] == int(np.argmin(f["closure"]))
    assert f["axis_corr"].min() > 0.02
    mirrored = FO.kabsch_rmsd(f["xyz"][:, 1] * np.array([1.0, 1.0, -1.0]), ca)
    assert mirrored > 4 * rmsd                                                          # the hand matters: no reflection in the fit
    gap = gold[f"score_f32_gap_{key}"]
    assert gap.shape == (4,) and (gap > 0).all() and (gap < 1e-4 * f["score"]).all()   # float32 rounding, not an allowance


@pytest.mark.parametrize("key", KEYS)
def test_restraint_counts_equal_a_direct_count(gold, key):
    maps = _maps(gold, key)
    n = maps["dist"].shape[0]
    want = [0, 0, 0]
    for a in range(n):
        for b in range(n):
            if maps["dist"][a, b] > 12.0:               # filter_idx of load_constraints
                continue
            if a < b and maps["dist"][a, b] > 0:
                want[0] += 1
            if a < b and abs(maps["omega"][a, b]) > 0:
                want[1] += 1
            if a != b:
                want[2] += 1
    _, counts = FO.restraint_score(gold[f"xyz_{key}"], maps)
    assert counts.tolist() == want + [want[2]] == gold["meta"]["chains"][key]["counts"]


def test_pdb_round_trip(gold, tmp_path):
    from text2protein_amd.encode import read_backbone
    from text2protein_amd.fold import write_backbone_pdb
    xyz = gold["xyz_96cut"] * 7.3 - 40.0                # negative and three-digit coordinates
    for with_cb in (False, True):
        path = tmp_path / f"cb{int(with_cb)}.pdb"
        write_backbone_pdb(str(path), xyz, chain="B", resname="GLY", with_cb=with_cb)
        got, ok, n = read_backbone(str(path), chain="B")
        want = np.vectorize(lambda v: float(f"{v:.3f}"))(xyz)           # the format's own rounding to 3 decimals
        assert n == 37 and ok.all() and np.array_equal(got, want.astype(np.float32)) and np.abs(want - xyz).max() <= 5.0e-4 + 1e-12
        lines = path.read_text().splitlines()
        atoms = [l for l in lines if l.startswith("ATOM")]
        assert len(atoms) == 37 * (4 if with_cb else 3) and lines[-2].startswith("TER") and lines[-1] == "END"
        assert all(len(l) == 78 and l[17:20] == "GLY" and l[21] == "B" for l in atoms)
        assert [l[12:16] for l in atoms[:4]][:3] == [" N  ", " CA ", " C  "] and (not with_cb or atoms[3][12:16] == " CB ")
        if with_cb:
            cb = np.array([[float(l[30:38]), float(l[38:46]), float(l[46:54])] for l in atoms[3::4]])
            assert np.abs(cb - FO.virtual_cb(xyz)).max() <= 5.001e-4
    with pytest.raises(ValueError):
        read_backbone(str(path), chain="A")             # written as chain B
    with pytest.raises(ValueError):
        write_backbone_pdb(str(tmp_path / "x.pdb"), np.full((2, 3, 3), np.nan))
