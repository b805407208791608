"""The refinement on the GPU (t2p_op_refine_backbone / t2p_op_restraint_energy, text2protein_amd/refine.py) against the float64 oracle
(tests/refine_oracle.py) and its recorded runs (tests/golden/refine_cases.npz, written by tests/golden/make_golden_refine.py).  The
maps of every case are rebuilt from fold_chains.npz by ``refine_oracle.case_maps`` (Philox noise, nothing noisy is committed); the GPU
and the oracle read the same float32 maps and start from the same float32 coordinates.

Bounds.
  * one evaluation, every case and stage: terms and total <= 1e-9 max(1, |value|), gradient <= 1e-9 max(1, max|g|).  Both sides are in
    double; reordering a few 10^4 terms costs about 1e-12, a float32 slip anywhere 1e-7;
  * 5 iterations per stage: coordinates <= 1e-4 A (the float32 rounding of input and output at 40 A, 4e-6, with room for 15 steps: the
    fold test's TIGHT); status, iteration and evaluation counts equal;
  * the default run: status 0, E_end <= E_start, closure < 0.01 A, and on every noisy case the refined CA RMSD to the truth below the
    start's;
  * the default run against the oracle's recorded one: nine hundred line-search decisions need not agree to the last one, so the two
    bounds are 4 x the largest gap recorded in profiles/refine_parity.json (ENERGY_REL_BOUND, RMSD_BOUND below), both far under the
    5 % / 0.05 A beyond which the issue asks for a statement instead.
The figures are printed before they are asserted; with T2P_REFINE_PARITY_OUT=<file> those of the default run are also written there as
JSON (profiles/refine_parity.json is such a file).
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
import refine_oracle as RO
from helpers import GOLDEN, cfg_ckpt, load_golden

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("dist", "omega", "theta", "phi")
CASES = list(RO.CASES)
TIGHT = 1e-4
ENERGY_REL_BOUND = 4 * 4.01e-3         # 4 x the largest |E_gpu - E_oracle| / E_oracle of profiles/refine_parity.json (chain 132, E = 0.028)
RMSD_BOUND = 4 * 2.18e-3               # 4 x the largest |CA RMSD_gpu - CA RMSD_oracle| (A) recorded there (chain 132)
SEEN = {}


def _record(name, value):
    SEEN[name] = value
    path = os.environ.get("T2P_REFINE_PARITY_OUT")
    if path:
        with open(path, "w") as f:
            json.dump(SEEN, f, indent=1, sort_keys=True)


@pytest.fixture(scope="module")
def fold_gold():
    return load_golden("fold_chains")


@pytest.fixture(scope="module")
def gold():
    g = load_golden("refine_cases")
    g["meta"] = json.loads(str(g["meta"]))
    return g


@pytest.fixture(scope="module")
def maps(fold_gold):
    return {name: RO.case_maps(fold_gold, name) for name in CASES}


def _pack(gold, maps, names, L=None, fill=float("nan")):
    """The start coordinates and maps of `names` as one batch padded to L; the padding is NaN: nothing past a chain's length is read."""
    ns = [gold[f"start_{k}"].shape[0] for k in names]
    L = L or max(ns)
    xyz = torch.full((len(names), L, 3, 3), fill)
    absval = torch.full((len(names), 4, L * L), fill)
    for b, k in enumerate(names):
        xyz[b, :ns[b]] = torch.from_numpy(gold[f"start_{k}"])
        for c, nm in enumerate(NAMES):
            absval[b, c, :ns[b] * ns[b]] = torch.from_numpy(maps[k][nm].reshape(-1))
    return xyz.cuda(), absval.cuda(), torch.tensor(ns, dtype=torch.int32)


@pytest.fixture(scope="module")
def full(gold, maps):
    """The default run of every case alone, once."""
    from text2protein_amd.refine import refine_backbone_batch
    out = {}
    for name in CASES:
        xyz, absval, n = _pack(gold, maps, [name])
        out[name] = refine_backbone_batch(xyz, absval, n)
    torch.cuda.synchronize()
    return out


@pytest.mark.parametrize("case", CASES)
def test_energy_operator_matches_the_oracle(gold, maps, case):
    from text2protein_amd.refine import restraint_energy
    xyz, absval, n = _pack(gold, maps, [case])
    m64 = {k: v.astype(np.float64) for k, v in maps[case].items()}
    x64 = gold[f"start_{case}"].astype(np.float64)
    for stage in RO.default_schedule():
        terms, grad = restraint_energy(xyz, absval, n, stage)
        terms, grad = terms.cpu().numpy()[0], grad.cpu().numpy()[0]
        e, t, g = RO.energy(x64, m64, stage)
        want = np.concatenate([t, [e]])
        rel = np.abs(terms - want) / np.maximum(1.0, np.abs(want))
        gerr = np.abs(grad - g).max() / max(1.0, np.abs(g).max())
        print(f"energy {case} stage {stage[:2]}: total {terms[8]:.9g} (oracle {e:.9g}), worst term gap {rel.max():.2e}, gradient gap {gerr:.2e}, "
              f"max|g| {np.abs(g).max():.4g}")
        assert (rel <= 1e-9).all(), (terms, want)
        assert gerr <= 1e-9
        assert np.abs(g).max() > 0 and e > 0


@pytest.mark.parametrize("case", CASES)
def test_short_run_follows_the_oracle(gold, maps, case):
    from text2protein_amd.refine import refine_backbone_batch
    xyz, absval, n = _pack(gold, maps, [case])
    out, status, diag = refine_backbone_batch(xyz, absval, n, RO.short_schedule(RO.SHORT_ITERS))
    got, d = out.cpu().numpy()[0].astype(np.float64), diag.cpu().numpy()[0]
    gap = np.abs(got - gold[f"short_xyz_{case}"]).max()
    counts = [int(status[0]), int(d[10]), int(d[11])]
    print(f"short run {case}: coordinates to oracle {gap:.2e} A, status / iterations / evaluations {counts} (oracle {gold[f'short_counts_{case}'].tolist()})")
    assert gap <= TIGHT
    assert counts == gold[f"short_counts_{case}"].tolist()
    assert d[14] == 3 and d[1] <= d[0]


@pytest.mark.parametrize("case", CASES)
def test_default_run(gold, fold_gold, full, case):
    out, status, diag = full[case]
    d = diag.cpu().numpy()[0]
    x = out.cpu().numpy()[0].astype(np.float64)
    truth = RO.case_truth(fold_gold, case)
    before = FO.kabsch_rmsd(gold[f"start_{case}"][:, 1], truth[:, 1])
    after = FO.kabsch_rmsd(x[:, 1], truth[:, 1])
    print(f"default run {case}: status {int(status[0])}, E {d[0]:.6g} -> {d[1]:.6g}, closure {d[13]:.2e}, CA RMSD {before:.4f} -> {after:.4f}, "
          f"iterations {int(d[10])}, evaluations {int(d[11])}, max|g| {d[12]:.3g}")
    assert int(status[0]) == 0 and np.isfinite(x).all() and np.isfinite(d).all()
    assert d[1] <= d[0] and d[13] < 0.01 and d[14] == 3
    assert abs(d[13] - FO.closure(x)) < 1e-5                    # the diagnostic is of the coordinates returned (float32 rounding)
    if case in RO.NOISY:
        assert after < before


def test_default_run_against_the_recorded_oracle(gold, fold_gold, full):
    rows, worst_e, worst_r = {}, 0.0, 0.0
    for case in CASES:
        out, status, diag = full[case]
        d = diag.cpu().numpy()[0]
        truth = RO.case_truth(fold_gold, case)
        sc = gold[f"scalars_{case}"]
        rmsd = FO.kabsch_rmsd(out.cpu().numpy()[0, :, 1].astype(np.float64), truth[:, 1])
        e_gap, r_gap = abs(d[1] - sc[1]) / abs(sc[1]), abs(rmsd - sc[7])
        rows[case] = dict(energy=float(d[1]), oracle_energy=float(sc[1]), energy_rel_gap=float(e_gap), ca_rmsd=rmsd, oracle_ca_rmsd=float(sc[7]),
                          ca_rmsd_gap=float(r_gap), iterations=int(d[10]), evaluations=int(d[11]), oracle_iterations=int(sc[2]),
                          oracle_evaluations=int(sc[3]), max_gradient=float(d[12]), closure=float(d[13]), fold_ca_rmsd=float(sc[6]))
        print(f"parity {case}: {rows[case]}")
        worst_e, worst_r = max(worst_e, e_gap), max(worst_r, r_gap)
    _record("default_run", dict(cases=rows, largest_energy_rel_gap=worst_e, largest_ca_rmsd_gap=worst_r))
    assert ENERGY_REL_BOUND <= 0.05 and RMSD_BOUND <= 0.05
    assert worst_e <= ENERGY_REL_BOUND and worst_r <= RMSD_BOUND


def test_two_calls_and_any_padding_give_the_same_bits(gold, maps, full):
    from text2protein_amd.refine import refine_backbone_batch
    ragged = ["96", "96cut", "48"]
    first = None
    for L in (96, 128, 256):                                  # 256: the largest map side, 98.9 KB of dynamic LDS
        xyz, absval, n = _pack(gold, maps, ragged, L)
        out, status, diag = refine_backbone_batch(xyz, absval, n)
        if first is None:
            first = (out, status, diag)
            again = refine_backbone_batch(xyz, absval, n)
            for a, b in zip(first, again):
                assert torch.equal(a, b)
        for b, name in enumerate(ragged):
            one, one_status, one_diag = full[name]
            k = int(n[b])
            assert torch.equal(out[b, :k], one[0, :k]), (L, name)
            assert not out[b, k:].any()
            assert torch.equal(diag[b], one_diag[0]) and int(status[b]) == int(one_status[0]), (L, name)


def test_the_largest_chain():
    """256 residues, REFINE_MAX_L (the 256-residue chain of tmalign_pairs.npz, exact maps from the device's own encode and decode,
    started from the device's fold): four rounds of 64 residues per evaluation, every vector at its full LDS size.  One evaluation
    against the oracle with the bound of the other cases; the run itself is held to what the algorithm guarantees, because the fold
    is not pinned on this chain: its start lies 7.85 A CA RMSD from the truth (E = 5.7e5), and the run ends with status 1 (a stage
    stopped on a failed line search) at E = 5.3e3 after 581 evaluations, closure 0.0012 A, CA RMSD 7.76 A."""
    from text2protein_amd.decode import decode_6d_batch
    from text2protein_amd.encode import encode_6d_batch
    from text2protein_amd.fold import fold_maps_batch
    from text2protein_amd.refine import refine_backbone_batch, restraint_energy
    truth = load_golden("tmalign_pairs")["xyz_256"].astype(np.float64)
    n = torch.tensor([256], dtype=torch.int32)
    coords = encode_6d_batch(torch.from_numpy(truth).float().unsqueeze(0).cuda(), n)["coords_6d"]
    lengths, _, absval = decode_6d_batch(coords)
    start = fold_maps_batch(absval, lengths)[0]
    m64 = {nm: absval[0, c].reshape(256, 256).cpu().numpy().astype(np.float64) for c, nm in enumerate(NAMES)}
    x64 = start.cpu().numpy()[0].astype(np.float64)
    stage = RO.default_schedule()[-1]
    terms, grad = restraint_energy(start, absval, lengths, stage)
    e, t, g = RO.energy(x64, m64, stage)
    want, got = np.concatenate([t, [e]]), terms.cpu().numpy()[0]
    rel = np.abs(got - want) / np.maximum(1.0, np.abs(want))
    gerr = np.abs(grad.cpu().numpy()[0] - g).max() / max(1.0, np.abs(g).max())
    out, status, diag = refine_backbone_batch(start, absval, lengths)
    d = diag.cpu().numpy()[0]
    before = FO.kabsch_rmsd(x64[:, 1], truth[:, 1])
    after = FO.kabsch_rmsd(out.cpu().numpy()[0, :, 1].astype(np.float64), truth[:, 1])
    print(f"256 residues: term gap {rel.max():.2e}, gradient gap {gerr:.2e}; status {int(status[0])}, E {d[0]:.6g} -> {d[1]:.6g}, "
          f"closure {d[13]:.2e}, CA RMSD {before:.4f} -> {after:.4f}, evaluations {int(d[11])}")
    assert (rel <= 1e-9).all() and gerr <= 1e-9
    assert int(status[0]) in (0, 1) and torch.isfinite(out).all() and np.isfinite(d).all()
    assert d[1] <= d[0] and d[0] == got[8] and d[14] == 3 and 0 < d[10] <= 900


def test_bad_inputs_give_a_status_and_zeros(gold, maps):
    from text2protein_amd.refine import refine_backbone_batch, restraint_energy
    xyz, absval, n = _pack(gold, maps, ["96w8"] * 4, L=8, fill=0.0)
    xyz[1, 3, 1, 2] = float("nan")
    n = torch.tensor([8, 8, -1, 1], dtype=torch.int32)
    out, status, diag = refine_backbone_batch(xyz, absval, n)
    assert status.cpu().tolist() == [0, 2, -1, -1]
    assert torch.isfinite(out).all() and torch.isfinite(diag).all()
    assert out[0].any() and not out[1:].any() and not diag[1:].any()          # diag[11] == 0: no evaluation was made
    assert diag[0, 11] > 0
    terms, grad = restraint_energy(xyz, absval, n)
    assert torch.isfinite(terms).all() and torch.isfinite(grad).all() and terms[0].any() and not terms[1:].any() and not grad[1:].any()


def test_more_than_256_residues_are_refused():
    from text2protein_amd import _lib
    from text2protein_amd.refine import refine_backbone_batch, restraint_energy
    lib = _lib.load()
    assert lib.t2p_op_refine_ws(1, 257) == -1 and lib.t2p_op_refine_ws(0, 8) == -1 and lib.t2p_op_refine_ws(2, 0) == -1
    assert lib.t2p_op_refine_ws(2, 256) > 0
    xyz, absval = torch.zeros(1, 257, 3, 3, device="cuda"), torch.zeros(1, 4, 257 * 257, device="cuda")
    for fn in (refine_backbone_batch, restraint_energy):
        with pytest.raises(ValueError, match="REFINE_MAX_L"):
            fn(xyz, absval, torch.tensor([257]))
    with pytest.raises(ValueError, match="stages"):
        refine_backbone_batch(xyz[:, :8], absval[:, :, :64], torch.tensor([8]), schedule=[(1, 12, 3, 1, 3, 5)] * 9)


def test_fold_with_refine_end_to_end(fold_gold):
    from text2protein_amd.encode import encode_6d_batch
    from text2protein_amd.fold import fold_6d, fold_6d_batch
    from text2protein_amd.tmalign import tm_align_batch
    keys = ("96", "48")
    ns = [fold_gold[f"xyz_{k}"].shape[0] for k in keys]
    xyz = torch.full((2, 96, 3, 3), float("nan"))
    for b, k in enumerate(keys):
        xyz[b, :ns[b]] = torch.from_numpy(fold_gold[f"xyz_{k}"]).float()
    coords = encode_6d_batch(xyz.cuda(), torch.tensor(ns, dtype=torch.int32))["coords_6d"]
    plain = fold_6d_batch(coords)
    r = fold_6d_batch(coords, refine=True)
    assert torch.equal(r["xyz_fold"], plain["xyz"]) and torch.equal(r["diag"], plain["diag"]) and r["chains"] == plain["chains"]
    assert "xyz_fold" not in plain and "refine" not in plain
    for b, k in enumerate(keys):
        truth = fold_gold[f"xyz_{k}"][:, 1]
        before = FO.kabsch_rmsd(plain["xyz"][b, :ns[b], 1].cpu().numpy(), truth)
        after = FO.kabsch_rmsd(r["xyz"][b, :ns[b], 1].cpu().numpy(), truth)
        print(f"end to end {k}: CA RMSD {before:.4f} -> {after:.4f}, {r['refine'][b]}")
        assert r["refine"][b]["status"] == 0 and r["refine"][b]["L"] == ns[b] and after < before
    n_dev = torch.tensor(ns, dtype=torch.int32, device="cuda")
    tm = tm_align_batch(r["xyz"], n_dev, plain["xyz"], n_dev, pairs=torch.tensor([[0, 0], [1, 1]], dtype=torch.int32, device="cuda"))
    assert tm["status"].cpu().tolist() == [0, 0] and (tm["tm_a"].cpu() > 0.9).all()
    one = fold_6d(coords[1:], refine=True)[0]
    assert one["xyz"].shape == (48, 3, 3) and one["xyz_fold"].shape == (48, 3, 3) and one["refine"]["status"] == 0


def test_a_stage_of_no_iterations_returns_the_start(gold, maps):
    from text2protein_amd.refine import refine_backbone_batch
    xyz, absval, n = _pack(gold, maps, ["96cut"])
    out, status, diag = refine_backbone_batch(xyz, absval, n, schedule=[(1, RO.SEP_ALL, 3.0, 1.0, 3.0, 0)])
    assert torch.equal(out, xyz) and int(status[0]) == 0
    assert diag[0, 0] == diag[0, 1] and diag[0, 10] == 0 and diag[0, 11] == 3 and diag[0, 14] == 1


def test_cli_refine_writes_a_refined_backbone_per_sample(tmp_path):
    """--refine alone implies --fold and --decode; the maps of a random-weight network are junk, so any status but finite files."""
    from text2protein_amd.encode import read_backbone
    cfg = cfg_ckpt()
    cfg.training.sde = "vesde"
    cfg.model.condition = ["length"]
    cfg_path = tmp_path / "ckpt_length.yml"
    with open(cfg_path, "w") as f:
        yaml.safe_dump(yaml.safe_load(json.dumps(cfg)), f)
    out = tmp_path / "out"
    cmd = [sys.executable, os.path.join(ROOT, "sampling_6d.py"), str(cfg_path), os.path.join(GOLDEN, "tiny_checkpoint.pth"), "--batch_size", "2",
           "--context_tokens", "4", "--dtype", "f32", "--select_length", "1", "--length_index", "4", "--outdir", str(out), "--refine"]
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=600, cwd=str(tmp_path))
    assert r.returncode == 0, r.stdout + r.stderr
    assert sorted(os.listdir(out)) == sorted(f"{stem}_{i}.{ext}" for i in (0, 1) for stem, ext in
                                             (("sampled", "pkl"), ("decoded", "npz"), ("folded", "pdb"), ("refined", "pdb"), ("fold", "json")))
    for i in (0, 1):
        xyz, ok, n = read_backbone(str(out / f"refined_{i}.pdb"))
        with open(out / f"fold_{i}.json") as f:
            d = json.load(f)
        rf = d["refine"]
        assert n == 7 == d["L"] == rf["L"] and ok.all() and np.isfinite(xyz).all()
        assert rf["status"] in (0, 1) and rf["energy"] <= rf["energy_start"] and rf["stages"] == 3 and sorted(rf["terms"]) == sorted(RO.TERMS)
        assert (rf["status"] != 0) == (f"sample {i}: refine status" in r.stdout)
