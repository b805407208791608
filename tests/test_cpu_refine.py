"""The refinement's host side without a GPU: the float64 oracle (tests/refine_oracle.py) is checked against finite differences and
against fold_oracle's restraint score, reproduces its own recorded run (tests/golden/refine_cases.npz), and the constants, the C ABI
and the command line of the product agree with it."""
import json
import os
import re
import subprocess
import sys

import numpy as np
import pytest

import fold_oracle as FO
import refine_oracle as RO
from helpers import load_golden

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def fold_gold():
    return load_golden("fold_chains")


@pytest.fixture(scope="module")
def gold():
    g = load_golden("refine_cases")
    g["meta"] = json.loads(str(g["meta"]))
    return g


def _inputs(fold_gold, gold, case):
    maps = {k: v.astype(np.float64) for k, v in RO.case_maps(fold_gold, case).items()}
    return gold[f"start_{case}"].astype(np.float64), maps


@pytest.mark.parametrize("case", ["96cut", "96w8"])
def test_oracle_gradient_against_central_differences(fold_gold, gold, case):
    """Step 1e-5 A in float64: the truncation error is O(h^2) times a third derivative, the rounding error eps E / h, both far below
    the bound 1e-6 max(1, max|g|)."""
    x, maps = _inputs(fold_gold, gold, case)
    lists = RO.restraint_lists(maps)
    h = 1e-5
    for stage in RO.default_schedule():
        _, _, g = RO.energy(x, maps, stage, lists=lists)
        fd = np.zeros_like(g)
        for idx in np.ndindex(*x.shape):
            xp, xm = x.copy(), x.copy()
            xp[idx] += h
            xm[idx] -= h
            fd[idx] = (RO.energy(xp, maps, stage, lists=lists)[0] - RO.energy(xm, maps, stage, lists=lists)[0]) / (2 * h)
        err, bound = np.abs(g - fd).max(), 1e-6 * max(1.0, np.abs(g).max())
        print(f"gradient {case} stage {stage[:2]}: max|g| {np.abs(g).max():.4g}, max|g - g_fd| {err:.3e} (bound {bound:.3e})")
        assert err <= bound


@pytest.mark.parametrize("case", ["96cut", "132"])
def test_restraint_terms_equal_the_fold_oracles_score(fold_gold, gold, case):
    x, maps = _inputs(fold_gold, gold, case)
    want, counts = FO.restraint_score(x, maps)
    _, terms, _ = RO.energy(x, maps, (1, RO.SEP_ALL, 1.0, 1.0, 1.0), arm_min=0.0)
    assert np.allclose(terms[:4], want, rtol=1e-12, atol=0.0), (terms[:4], want)
    lists = RO.restraint_lists(maps, arm_min=0.0)
    assert [len(lists[k][0]) for k in ("dist", "omega", "theta", "phi")] == counts.tolist()
    filtered = RO.restraint_lists(maps)
    assert len(filtered["theta"][0]) < counts[2] and len(filtered["omega"][0]) < counts[1] and len(filtered["phi"][0]) == counts[3]
    phi = maps["phi"][filtered["theta"]]
    assert phi.min() >= np.deg2rad(RO.ARM_MIN) and phi.max() <= np.pi - np.deg2rad(RO.ARM_MIN)


def test_oracle_reproduces_the_recorded_run_and_never_raises_the_energy(fold_gold, gold):
    x, maps = _inputs(fold_gold, gold, "96cut")
    trace = []
    r = RO.refine(x, maps, trace=trace)
    sc = gold["scalars_96cut"]
    assert r["status"] == 0 and abs(r["e_end"] - sc[1]) <= 1e-9 * abs(sc[1]) and abs(r["e_start"] - sc[0]) <= 1e-9 * abs(sc[0])
    assert [r["iterations"], r["evaluations"]] == [int(sc[2]), int(sc[3])]
    assert np.abs(r["xyz"] - gold["xyz_96cut"]).max() <= 1e-9
    assert all(after is not None and after <= before for before, after, *_ in trace) and len(trace) == r["iterations"]
    assert r["e_end"] <= r["e_start"] and r["closure"] < 0.01
    rep = gold["meta"]["cases"]
    for case in RO.NOISY:
        assert rep[case]["refined_ca_rmsd"] < rep[case]["fold_ca_rmsd"], case
    assert sorted(rep) == sorted(RO.CASES)


def test_noisy_maps_are_reproducible_and_clipped(fold_gold):
    a, b = RO.case_maps(fold_gold, "48"), RO.case_maps(fold_gold, "48")
    clean = {k: fold_gold[f"{k}_48"] for k in a}
    for k in a:
        assert np.array_equal(a[k], b[k]) and a[k].dtype == np.float32
    known = (clean["dist"] > 0) & (clean["dist"] < 20)
    assert np.array_equal(a["dist"][~known], clean["dist"][~known]) and (a["dist"][known] != clean["dist"][known]).mean() > 0.99
    assert a["dist"][known].min() >= 0.5 and a["dist"][known].max() <= np.float32(19.99)
    assert a["phi"][known].min() >= np.float32(0.01) and a["phi"][known].max() <= np.float32(np.pi - 0.01)
    up = np.triu(known, 1)
    assert np.array_equal(a["dist"][up], a["dist"].T[up]) and np.array_equal(a["omega"][up], a["omega"].T[up])
    sd = (a["dist"].astype(np.float64) - clean["dist"])[up].std()
    assert 0.9 < sd < 1.1


def test_kernel_constants_equal_the_oracles():
    csrc = os.path.join(ROOT, "text2protein_amd", "csrc")
    geom = open(os.path.join(csrc, "backbone_geom.h")).read()                                          # the shared geometry: K1..K3, the ideal backbone, GUARD
    src = open(os.path.join(csrc, "refine.hip")).read()
    assert '#include "backbone_geom.h"' in src and "using namespace geom;" in src
    found = {k: float(v) for k, v in re.findall(r"\b([A-Z][A-Z0-9_]*) = (-?\d+(?:\.\d+)?(?:e-?\d+)?)[,;]", geom + src)}
    want = {"K1": RO.K1, "K2": RO.K2, "K3": RO.K3, "BOND_N_CA": RO.BOND_N_CA, "BOND_CA_C": RO.BOND_CA_C, "BOND_C_N": RO.BOND_C_N,
            "BOND_SIGMA": RO.BOND_SIGMA, "ANGLE_N_CA_C": RO.ANGLE_N_CA_C, "ANGLE_CA_C_N": RO.ANGLE_CA_C_N, "ANGLE_C_N_CA": RO.ANGLE_C_N_CA,
            "ANGLE_SIGMA": RO.ANGLE_SIGMA, "PEPT_SIGMA": RO.PEPT_SIGMA, "REP_RADIUS": RO.REP_RADIUS, "REP_MIN_SEP": RO.REP_MIN_SEP,
            "REFINE_HISTORY": RO.HISTORY, "REFINE_MAX_TRIALS": RO.MAX_TRIALS, "ARMIJO_C1": RO.ARMIJO_C1, "GRAD_TOL": RO.GRAD_TOL,
            "CURVATURE_EPS": RO.CURVATURE_EPS, "NEIGHBOUR": RO.NEIGHBOUR, "GUARD": RO.GUARD}
    for k, v in want.items():
        assert found.get(k) == v, (k, found.get(k), v)
    fold_src = open(os.path.join(csrc, "fold.hip")).read()
    for k in ("K1", "K2", "K3"):                                                                       # the same identity as the fold's: its float
        assert f"{k}_F == {want[k]:.8f}f" in geom and f"{k}_F = (float){k}" in geom and f"{k}_F" in fold_src, k      # twin, held to the literal
    hdr = open(os.path.join(ROOT, "text2protein_amd", "csrc", "t2p_kernels.h")).read()
    assert re.search(r"REFINE_MAX_L = 256, REFINE_MAX_STAGES = 8;", hdr)


def test_python_defaults_equal_the_oracles_and_the_references_bands():
    from text2protein_amd import refine as R
    assert R.default_schedule() == RO.default_schedule() and R.default_schedule(3) == RO.default_schedule(3)
    assert [(s[0], s[1]) for s in R.default_schedule(3)] == [(3, 12), (3, 24), (3, R.SEP_ALL)]       # add_rst 3-12, 12-24, 24-len, cumulative
    assert all(s[2:] == (3.0, 1.0, 3.0, 300) for s in R.default_schedule(3))                           # rosetta_min/run.py:5-7, run 0
    assert (R.DIST_STD, R.ANGLE_STD, R.ARM_MIN, R.TERM_NAMES) == (RO.DIST_STD, RO.ANGLE_STD, RO.ARM_MIN, RO.TERMS)
    assert R.REFINE_MAX_L == 256 and R.SEP_ALL > R.REFINE_MAX_L


def test_header_and_signatures_declare_the_entry_points():
    from text2protein_amd import _lib
    hdr = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "t2p.h")).read(), flags=re.S)
    for name, n_args in (("t2p_op_refine_ws", 2), ("t2p_op_refine_backbone", 16), ("t2p_op_restraint_energy", 14)):
        m = re.search(r"\b" + name + r"\s*\(([^)]*)\)", hdr)
        assert m and len(m.group(1).split(",")) == n_args == len(_lib.SIGNATURES[name][1]), name
    lib = _lib.load()
    assert lib.t2p_op_refine_ws(1, 257) == -1 and lib.t2p_op_refine_ws(1, 0) == -1 and lib.t2p_op_refine_ws(0, 8) == -1
    assert lib.t2p_op_refine_ws(32, 128) > 32 * 128 * 127 * 32                                         # every pair of every chain fits


def test_refine_has_no_cpu_path():
    import torch
    from text2protein_amd._lib import T2PError
    from text2protein_amd.refine import refine_backbone_batch
    with pytest.raises(T2PError, match="no CPU fallback"):
        refine_backbone_batch(torch.zeros(1, 8, 3, 3), torch.zeros(1, 4, 64), torch.tensor([8]))


def test_cli_help_shows_refine():
    r = subprocess.run([sys.executable, os.path.join(ROOT, "sampling_6d.py"), "--help"], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and "--refine" in r.stdout and "refined_<id>.pdb" in r.stdout
