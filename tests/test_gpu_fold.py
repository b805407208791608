"""The fold on the GPU (t2p_op_fold_6d / t2p_op_restraint_score, text2protein_amd/fold.py) on chains with known coordinates
(tests/golden/fold_chains.npz, written by tests/golden/make_golden_fold.py), against the truth and against the float64 oracle
(tests/fold_oracle.py).  The maps come from encode_6d_batch -> decode_6d_batch, so the whole device path runs; the oracle is given the
same decoded maps.

Bounds.  r_or = the oracle's own CA RMSD to the truth on the chain (0.12 to 0.25 A on the committed chains), computed here.
  * GPU CA RMSD to the truth (Kabsch, proper rotations only) <= 2 r_or and GPU to oracle CA RMSD <= r_or: the bounds the feature was
    specified with.  They are wide: they hold even when a stress step loses some of its pairs;
  * so, tighter: GPU to oracle CA RMSD <= 1e-4 A and |GPU stress rms - oracle stress rms| <= 1e-4 A on every chain.  The kernel does the
    oracle's arithmetic in float32: coordinates of up to 40 A carry 4e-6 A of rounding, the 300 stress steps are a contraction, and the
    3x3 frame solves amplify by at most the condition of the normal matrix (<= 20 on these chains): 1e-4 A leaves a factor of ten or so
    and is a hundred times below what a dropped pair does (0.02 A);
  * one chain of 8 residues (residues 11..18 of the 96-residue chain): a single chunk of eight in the stress step;
  * restraint scores against the oracle on the SAME coordinates and maps: per term 4 x score_f32_gap of the fixture (oracle in
    float32 against float64 -- the rule of test_gpu_encode.py); the counts equal.
The figures are printed before they are asserted; with T2P_FOLD_PARITY_OUT=<file> they are also written there as JSON
(profiles/fold_parity.json is such a file).
"""
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch
import yaml

import fold_oracle as FO
from helpers import GOLDEN, cfg_ckpt, load_golden

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CASES = {"48": ("48",), "96": ("96",), "132": ("132",), "96cut": ("96cut",), "96w8": ("96w8",), "ragged": ("96", "96cut", "48")}
SCORE_CASES = [c for c in CASES if c != "96w8"]          # the fixture records the float32 / float64 score gap of its own chains
TIGHT = 1e-4
NAMES = ("dist", "omega", "theta", "phi")
SEEN = {}


@pytest.fixture(scope="module")
def gold():
    g = load_golden("fold_chains")
    g["meta"] = json.loads(str(g["meta"]))
    g["xyz_96w8"] = g["xyz_96"][11:19]
    return g


def _fold_case(gold, keys):
    from text2protein_amd.encode import encode_6d_batch
    from text2protein_amd.fold import fold_6d_batch
    ns = [gold[f"xyz_{k}"].shape[0] for k in keys]
    L = max(ns)
    xyz = torch.full((len(keys), L, 3, 3), float("nan"))
    for b, k in enumerate(keys):
        xyz[b, :ns[b]] = torch.from_numpy(gold[f"xyz_{k}"]).float()
    enc = encode_6d_batch(xyz.cuda(), torch.tensor(ns, dtype=torch.int32))
    out = fold_6d_batch(enc["coords_6d"])
    torch.cuda.synchronize()
    return enc["coords_6d"], out


@pytest.fixture(scope="module")
def folded(gold):
    """Every case folded once and shared."""
    return {name: _fold_case(gold, keys) for name, keys in CASES.items()}


@pytest.fixture(scope="module")
def oracle(gold, folded):
    """The oracle on the decoded maps of every chain (taken from the case that holds the chain alone), once."""
    out = {}
    for key in ("48", "96", "132", "96cut", "96w8"):
        _, r = folded[key]
        n = int(r["lengths"][0])
        maps = {nm: r["absval"][0, c, :n * n].reshape(n, n).cpu().numpy().astype(np.float64) for c, nm in enumerate(NAMES)}
        o = FO.fold(maps)
        o["maps"] = maps
        o["r_or"] = FO.kabsch_rmsd(o["xyz"][:, 1], gold[f"xyz_{key}"][:, 1])
        out[key] = o
    return out


def _record(name, value):
    SEEN[name] = value
    path = os.environ.get("T2P_FOLD_PARITY_OUT")
    if path:
        with open(path, "w") as f:
            json.dump(SEEN, f, indent=1, sort_keys=True)


@pytest.mark.parametrize("case", list(CASES))
def test_fold_reconstructs_the_chain(gold, folded, oracle, case):
    _, r = folded[case]
    xyz = r["xyz"].cpu().numpy().astype(np.float64)
    assert np.isfinite(xyz).all()
    rows = []
    for b, key in enumerate(CASES[case]):
        o, d, n = oracle[key], r["chains"][b], gold[f"xyz_{key}"].shape[0]
        assert d["L"] == n and (xyz[b, n:] == 0).all()
        truth = FO.kabsch_rmsd(xyz[b, :n, 1], gold[f"xyz_{key}"][:, 1])
        all_atom = FO.kabsch_rmsd(xyz[b, :n].reshape(-1, 3), gold[f"xyz_{key}"].reshape(-1, 3))
        to_oracle = FO.kabsch_rmsd(xyz[b, :n, 1], o["xyz"][:, 1])
        rows.append(dict(chain=key, n=n, r_or=o["r_or"], gpu_ca_rmsd=truth, gpu_all_atom_rmsd=all_atom, gpu_to_oracle=to_oracle, hand=d["hand"],
                         oracle_hand=o["hand"], closure=d["closure"], oracle_closure=list(o["closure"]), stress_rms=d["stress_rms"],
                         oracle_stress_rms=o["stress_rms"], status=d["status"]))
        print(f"fold {case}/{key}: CA RMSD to truth {truth:.4f} (oracle {o['r_or']:.4f}, bound {2 * o['r_or']:.4f}), all-atom {all_atom:.4f}, "
              f"to oracle {to_oracle:.4f} (bound {o['r_or']:.4f}), hand {d['hand']} / {o['hand']}, closure {d['closure']}, status {d['status']}")
    _record(case, rows)
    for row, key in zip(rows, CASES[case]):
        assert row["r_or"] < 0.5
        assert row["gpu_ca_rmsd"] <= 2.0 * row["r_or"], row
        assert row["gpu_to_oracle"] <= row["r_or"], row
        assert row["gpu_to_oracle"] <= TIGHT and abs(row["stress_rms"] - row["oracle_stress_rms"]) <= TIGHT, row
        assert row["hand"] == row["oracle_hand"] and row["status"] == 0, row
    assert r["status"].cpu().tolist() == [0] * len(rows) and not r["placed"].any()


@pytest.mark.parametrize("case", SCORE_CASES)
def test_restraint_scores_match_the_oracle(gold, folded, oracle, case):
    from text2protein_amd.fold import restraint_score
    _, r = folded[case]
    xyz = r["xyz"].cpu().numpy()
    worst = []
    for b, key in enumerate(CASES[case]):
        n, d = gold[f"xyz_{key}"].shape[0], r["chains"][b]
        want, counts = FO.restraint_score(xyz[b, :n].astype(np.float64), oracle[key]["maps"])
        got = np.array([d["score"][nm] for nm in NAMES])
        bound = 4.0 * gold[f"score_f32_gap_{key}"]
        print(f"restraint score {case}/{key}: got {got}, oracle {want}, |difference| {np.abs(got - want)}, bounds {bound}, counts {counts}")
        worst.append((np.abs(got - want), bound, [d["count"][nm] for nm in NAMES], counts.tolist()))
    _record("score_" + case, [dict(chain=key, abs_difference=w[0].tolist(), bound=w[1].tolist(), counts=w[3]) for key, w in zip(CASES[case], worst)])
    for diff, bound, got_counts, counts in worst:
        assert got_counts == counts
        assert (diff <= bound).all(), (diff, bound)
    # the score on its own, for a backbone of the caller's: the same kernels, the same bits
    key = CASES[case][0]
    n = gold[f"xyz_{key}"].shape[0]
    dec = {"L": n, **{nm + "_abs": oracle[key]["maps"][nm].astype(np.float32) for nm in NAMES}}
    alone = restraint_score(xyz[0, :n], dec)
    assert alone["score"] == r["chains"][0]["score"] and alone["count"] == r["chains"][0]["count"]


def test_two_calls_give_the_same_bits(gold, folded):
    coords, first = folded["ragged"]
    from text2protein_amd.fold import fold_6d_batch
    again = fold_6d_batch(coords)
    for k in ("xyz", "status", "placed", "diag"):
        assert torch.equal(first[k], again[k]), k
    _, big = folded["132"]
    _, big2 = _fold_case(gold, CASES["132"])
    for k in ("xyz", "status", "placed", "diag"):
        assert torch.equal(big[k], big2[k]), k


def test_ragged_batch_equals_the_chains_alone(gold, folded):
    _, rag = folded["ragged"]
    for b, key in enumerate(CASES["ragged"]):
        _, one = folded[key]
        n = gold[f"xyz_{key}"].shape[0]
        assert torch.equal(rag["xyz"][b, :n], one["xyz"][0, :n]), key
        assert torch.equal(rag["diag"][b], one["diag"][0]), key
        assert not rag["xyz"][b, n:].any()


def test_improper_mask_and_isolated_residue(gold, folded):
    from text2protein_amd.fold import fold_6d, fold_6d_batch, fold_maps_batch
    coords, good = folded["48"]
    bad = torch.cat([coords, coords]).clone()
    bad[1, -1, 0, 1] = 0.0                                  # 48^2 - 1 ones: not a perfect square
    r = fold_6d_batch(bad)
    assert r["status"].cpu().tolist() == [0, -1] and r["lengths"].tolist() == [48, -1]
    assert torch.equal(r["xyz"][0], good["xyz"][0]) and not r["xyz"][1].any() and not r["diag"][1].any()
    with pytest.raises(ValueError, match="improper masking"):
        fold_6d(bad)
    one = fold_6d(coords)[0]
    assert one["xyz"].shape == (48, 3, 3) and one["status"] == 0
    # residue 20 beyond the cut-off of every other: its row and column say 20 A
    absval = good["absval"].clone()
    d = absval[0, 0].reshape(48, 48)
    d[20, :] = 20.0
    d[:, 20] = 20.0
    xyz, status, placed, diag = fold_maps_batch(absval, good["lengths"])
    assert status.cpu().tolist() == [1] and 20 in torch.nonzero(placed[0]).flatten().tolist()
    assert torch.isfinite(xyz).all() and torch.isfinite(diag).all() and diag[0, 12] > 0
    with pytest.raises(ValueError, match="FOLD_MAX_L"):            # the coordinate arrays kept in LDS bound the map side
        fold_maps_batch(torch.zeros(1, 4, 513 * 513, device="cuda"), torch.tensor([513]))


def test_random_weight_sample_stays_finite():
    """The last sample of a 1000-step run of a network with random weights: any status, finite coordinates."""
    from text2protein_amd.fold import fold_6d_batch
    s = torch.from_numpy(load_golden("run1000_cond_length")["sample"][-1:]).cuda()
    r = fold_6d_batch(s)
    print("random-weight sample:", r["chains"][0])
    assert r["status"].cpu().tolist()[0] in (-1, 0, 1)
    assert torch.isfinite(r["xyz"]).all() and torch.isfinite(r["diag"]).all()
    junk = torch.rand(2, 5, 40, 40, generator=torch.Generator().manual_seed(3)) * 2 - 1
    junk[:, -1] = 0
    junk[0, -1, :33, :33] = 1
    junk[1, -1, :2, :2] = 1
    r = fold_6d_batch(junk.cuda())
    print("uniform maps:", [(c["L"], c["status"], len(c["placed"])) for c in r["chains"]])
    assert r["lengths"].tolist() == [33, 2]
    assert torch.isfinite(r["xyz"]).all() and torch.isfinite(r["diag"]).all()


def test_cli_fold_writes_a_backbone_per_sample(tmp_path):
    from text2protein_amd.encode import read_backbone
    cfg = cfg_ckpt()
    cfg.training.sde = "vesde"
    cfg.model.condition = ["length"]
    cfg_path = tmp_path / "ckpt_length.yml"
    with open(cfg_path, "w") as f:
        yaml.safe_dump(yaml.safe_load(json.dumps(cfg)), f)
    out = tmp_path / "out"
    cmd = [sys.executable, os.path.join(ROOT, "sampling_6d.py"), str(cfg_path), os.path.join(GOLDEN, "tiny_checkpoint.pth"), "--batch_size", "2",
           "--context_tokens", "4", "--dtype", "f32", "--select_length", "1", "--length_index", "4", "--outdir", str(out), "--fold"]
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=600, cwd=str(tmp_path))
    assert r.returncode == 0, r.stdout + r.stderr
    assert sorted(os.listdir(out)) == sorted(f"{stem}_{i}.{ext}" for i in (0, 1) for stem, ext in
                                             (("sampled", "pkl"), ("decoded", "npz"), ("folded", "pdb"), ("fold", "json")))
    for i in (0, 1):
        xyz, ok, n = read_backbone(str(out / f"folded_{i}.pdb"))
        with open(out / f"fold_{i}.json") as f:
            d = json.load(f)
        assert n == 7 == d["L"] and ok.all() and np.isfinite(xyz).all() and d["status"] in (0, 1)
        assert (d["status"] != 0) == (f"sample {i}: fold status" in r.stdout)
