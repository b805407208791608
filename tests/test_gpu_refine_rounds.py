"""The refinement in rounds on the GPU (t2p_op_perturb_torsions / t2p_op_refine_rounds, text2protein_amd/refine.py) against
the float64 oracle (tests/refine_rounds_oracle.py), its recorded protocol run (tests/golden/refine_rounds.npz) and the composition of
the public operators the loop is made of.

Bounds.
  * the move: coordinates <= 1e-4 A (test_gpu_refine's TIGHT).  Both sides are double over the same float32 input; the float32 rounding
    of the output is 4e-6 A at 40 A.  Atoms 0..2 and a kept first candidate are bit-equal to the input;
  * the loop against its composition from perturb_torsions, refine_backbone_batch, restraint_energy and a host argmin: bit-equal --
    both sides run the same kernels on the same bits;
  * the loop against the recorded oracle: the kept indices equal (every recorded selection has a relative margin of 1e-3), final
    coordinates <= 1e-4 A, E_sel <= 1e-6 relative.
The figures are printed before they are asserted.
"""
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch
import yaml

import refine_oracle as RO
import refine_rounds_oracle as RR
from helpers import GOLDEN, cfg_ckpt, load_golden

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("dist", "omega", "theta", "phi")
TIGHT = 1e-4
P = RR.PROTOCOL


@pytest.fixture(scope="module")
def cases():
    return load_golden("refine_cases")


@pytest.fixture(scope="module")
def gold():
    g = load_golden("refine_rounds")
    g["meta"] = json.loads(str(g["meta"]))
    return g


@pytest.fixture(scope="module")
def maps():
    fold_gold = load_golden("fold_chains")
    return {name: RO.case_maps(fold_gold, name) for name in P["chains"]}


def _pack_xyz(chains, L):
    """Chains (n_i, 3, 3) float32 as one batch padded with NaN: nothing past a chain's length is read."""
    xyz = torch.full((len(chains), L, 3, 3), float("nan"))
    for b, c in enumerate(chains):
        xyz[b, :c.shape[0]] = torch.from_numpy(c)
    return xyz.cuda(), torch.tensor([c.shape[0] for c in chains], dtype=torch.int32)


def _pack_maps(maps, names, L):
    absval = torch.full((len(names), 4, L * L), float("nan"))
    for b, k in enumerate(names):
        n = maps[k]["dist"].shape[0]
        for c, nm in enumerate(NAMES):
            absval[b, c, :n * n] = torch.from_numpy(maps[k][nm].reshape(-1))
    return absval.cuda()


def _schedules():
    return [RR.round_schedule(r, P["iters"]) for r in range(P["rounds"])]


@pytest.fixture(scope="module")
def batch(cases, maps):
    xyz, n = _pack_xyz([cases[f"start_{k}"] for k in P["chains"]], 40)
    return xyz, _pack_maps(maps, P["chains"], 40), n


@pytest.fixture(scope="module")
def looped(batch, gold):
    """The protocol run of the fixture, once: (xyz, status, diag, trace)."""
    from text2protein_amd.refine import refine_rounds_batch
    xyz, absval, n = batch
    out = refine_rounds_batch(xyz, absval, n, P["rounds"], P["replicas"], P["amp"], int(gold["seed"]), P["stream_base"], list(P["chain_ids"]),
                              _schedules(), RR.SELECT_STAGE)
    torch.cuda.synchronize()
    return out


# ---------------------------------------------------------------------------------------------------------------------------------
MOVE_IDS, MOVE_SEED, MOVE_STREAM, MOVE_K = (5, 9, 2, 7), 1234, 40, 3


@pytest.fixture(scope="module")
def move_chains(cases):
    return [cases["start_96w8"], cases["start_96cut"], cases["start_96cut"][:2].copy(), cases["start_96cut"][5:8].copy()]


@pytest.mark.parametrize("L", [40, 256])
@pytest.mark.parametrize("keep_first", [False, True])
def test_move_against_the_oracle(move_chains, L, keep_first):
    from text2protein_amd.refine import perturb_torsions
    xyz, n = _pack_xyz(move_chains, L)
    out, status = perturb_torsions(xyz, n, RR.AMP, MOVE_SEED, MOVE_STREAM, MOVE_K, keep_first, MOVE_IDS)
    assert tuple(out.shape) == (4, MOVE_K, L, 3, 3) and not status.any() and torch.isfinite(out).all()
    got = out.cpu().numpy()
    for b, c in enumerate(move_chains):
        k = c.shape[0]
        want = RR.perturb(c.astype(np.float64), RR.AMP, MOVE_SEED, MOVE_STREAM, MOVE_K, keep_first, MOVE_IDS[b])
        gap = np.abs(got[b, :, :k].astype(np.float64) - want).max()
        moved = np.abs(got[b, -1, :k] - c).max()
        print(f"move L={L} keep_first={keep_first} chain {b} ({k} residues): gap to the oracle {gap:.2e} A, largest displacement {moved:.3f} A")
        assert gap <= TIGHT
        assert not got[b, :, k:].any()                                            # zero past the chain's length
        for q in range(MOVE_K):
            assert np.array_equal(got[b, q, 0], c[0])                             # atoms 0..2: bit-equal
        if keep_first:
            assert np.array_equal(got[b, 0, :k], c)
        assert moved > 1e-3                                                       # even two residues have a psi and a phi to move
        assert not np.array_equal(got[b, 1, :k], got[b, 2, :k])                   # every candidate its own stream


def test_move_does_not_depend_on_batch_position_padding_or_call(move_chains):
    from text2protein_amd.refine import perturb_torsions
    xyz, n = _pack_xyz(move_chains, 40)
    first, _ = perturb_torsions(xyz, n, RR.AMP, MOVE_SEED, MOVE_STREAM, MOVE_K, False, MOVE_IDS)
    again, _ = perturb_torsions(xyz, n, RR.AMP, MOVE_SEED, MOVE_STREAM, MOVE_K, False, MOVE_IDS)
    assert torch.equal(first, again)
    back, nb = _pack_xyz(move_chains[::-1], 256)
    rev, _ = perturb_torsions(back, nb, RR.AMP, MOVE_SEED, MOVE_STREAM, MOVE_K, False, MOVE_IDS[::-1])
    for b, c in enumerate(move_chains):
        k = c.shape[0]
        assert torch.equal(first[b, :, :k], rev[3 - b, :, :k]), b
    other, _ = perturb_torsions(xyz, n, RR.AMP, MOVE_SEED, MOVE_STREAM, MOVE_K, False, (6, 9, 2, 7))
    assert not torch.equal(first[0], other[0]) and torch.equal(first[1:], other[1:])      # the chain id is what names a chain
    default, _ = perturb_torsions(xyz, n, RR.AMP, MOVE_SEED, MOVE_STREAM, MOVE_K)
    ranged, _ = perturb_torsions(xyz, n, RR.AMP, MOVE_SEED, MOVE_STREAM, MOVE_K, False, (0, 1, 2, 3))
    assert torch.equal(default, ranged)
    shifted, _ = perturb_torsions(xyz, n, RR.AMP, MOVE_SEED, MOVE_STREAM + 1, MOVE_K - 1, False, MOVE_IDS)
    assert torch.equal(shifted, first[:, 1:])                                             # candidate k draws under stream + k


def test_move_gives_bad_inputs_a_status_and_zeros(move_chains):
    from text2protein_amd.refine import perturb_torsions
    xyz, n = _pack_xyz([move_chains[0]] * 4, 8)
    xyz[1, 3, 1, 2] = float("inf")
    n = torch.tensor([8, 8, 1, 9], dtype=torch.int32)
    out, status = perturb_torsions(xyz, n, replicas=2, keep_first=True)
    assert status.cpu().tolist() == [[0, 0], [2, 2], [-1, -1], [-1, -1]]
    assert torch.isfinite(out).all() and out[0].any() and not out[1:].any()
    line = np.zeros((1, 3, 3, 3), np.float32)
    line[0, :, :, 0] = np.arange(9).reshape(3, 3) * 1.4                                   # nine collinear atoms: the fallback frame
    got, st = perturb_torsions(torch.from_numpy(line).cuda(), torch.tensor([3]), seed=1)
    assert int(st[0, 0]) == 0 and torch.isfinite(got).all() and np.abs(got.cpu().numpy()[0] - line).max() <= TIGHT


# ---------------------------------------------------------------------------------------------------------------------------------
def _compose(batch, seed, rounds, K, schedules):
    """The loop from the public operators and an argmin on the host."""
    from text2protein_amd.refine import perturb_torsions, refine_backbone_batch, restraint_energy
    xyz, absval, n = batch
    B, L = xyz.shape[0], xyz.shape[1]
    abs_k, n_k = absval.repeat_interleave(K, 0), n.repeat_interleave(K)
    inc, e_inc = xyz.clone(), [float("inf")] * B
    status, diag = torch.zeros(B, dtype=torch.int32), torch.zeros(B, 16, dtype=torch.float64)
    trace = torch.zeros(B, rounds, K, 4, dtype=torch.float64)
    for r in range(rounds):
        cand, moved = perturb_torsions(inc, n, P["amp"], seed, P["stream_base"] + 16 * r, K, r == 0, list(P["chain_ids"]))
        assert not moved.any()
        rx, rst, rdg = refine_backbone_batch(cand.reshape(B * K, L, 3, 3), abs_k, n_k, schedules[r])
        terms, _ = restraint_energy(rx, abs_k, n_k, RR.SELECT_STAGE)
        esel, rst, rdg = terms[:, 8].cpu().reshape(B, K), rst.cpu().reshape(B, K), rdg.cpu().reshape(B, K, 16)
        for b in range(B):
            trace[b, r, :, 0], trace[b, r, :, 1], trace[b, r, :, 2] = esel[b], rst[b].double(), rdg[b, :, 11]
            valid = [k for k in range(K) if int(rst[b, k]) in (0, 1)]
            best = min(valid, key=lambda k: (float(esel[b, k]), k))
            if float(esel[b, best]) < e_inc[b]:
                e_inc[b] = float(esel[b, best])
                inc[b] = rx[b * K + best]
                status[b], diag[b] = rst[b, best], rdg[b, best]
                trace[b, r, best, 3] = 1.0
    return inc, status, diag, trace


def test_loop_is_bit_equal_to_its_composition_from_the_public_operators(batch, looped, gold):
    xyz, status, diag, trace = looped
    want = _compose(batch, int(gold["seed"]), P["rounds"], P["replicas"], _schedules())
    print("trace (E_sel, status, evaluations, kept):", trace.cpu().numpy().tolist())
    assert torch.equal(trace.cpu(), want[3])
    assert torch.equal(xyz, want[0]) and torch.equal(status.cpu(), want[1]) and torch.equal(diag.cpu(), want[2])


def test_loop_follows_the_recorded_oracle(looped, gold):
    xyz, status, diag, trace = looped
    tr = trace.cpu().numpy()
    kept = [[int(np.nonzero(tr[b, r, :, 3])[0][0]) if tr[b, r, :, 3].any() else -1 for r in range(P["rounds"])] for b in range(2)]
    e_gap = np.abs(tr[..., 0] - gold["esel"]) / np.abs(gold["esel"])
    gaps = []
    for b, name in enumerate(P["chains"]):
        k = gold[f"xyz_{name}"].shape[0]
        gaps.append(np.abs(xyz[b, :k].cpu().numpy().astype(np.float64) - gold[f"xyz_{name}"]).max())
    print(f"protocol: kept {kept} (oracle {gold['kept'].tolist()}), E_sel {tr[..., 0].tolist()} (oracle {gold['esel'].tolist()}), "
          f"largest relative E_sel gap {e_gap.max():.2e}, coordinates to the oracle {gaps} A, evaluations {tr[..., 2].tolist()} "
          f"(oracle {gold['evals'].tolist()})")
    assert kept == gold["kept"].tolist()
    assert max(gaps) <= TIGHT
    assert e_gap.max() <= 1e-6
    assert np.array_equal(tr[..., 1], gold["cstatus"]) and np.array_equal(tr[..., 2], gold["evals"])
    assert status.cpu().tolist() == gold["status"].tolist()


def test_one_round_of_one_candidate_is_refine_backbone(batch):
    from text2protein_amd.refine import refine_backbone_batch, refine_rounds_batch
    xyz, absval, n = batch
    want = refine_backbone_batch(xyz, absval, n)
    got = refine_rounds_batch(xyz, absval, n, rounds=1, replicas=1)
    for a, b in zip(got[:3], want):
        assert torch.equal(a, b)
    assert got[3].shape == (2, 1, 1, 4) and (got[3][:, 0, 0, 3] == 1).all() and torch.equal(got[3][:, 0, 0, 2], want[2][:, 11])


def test_what_the_protocol_guarantees(batch, looped):
    from text2protein_amd.refine import refine_rounds_batch
    xyz, absval, n = batch
    runs = [looped, refine_rounds_batch(xyz, absval, n, 4, 5, seed=3, stream_base=7, schedules=[RR.round_schedule(r, 3) for r in range(4)])]
    for out, status, diag, trace in runs:
        tr = trace.cpu().numpy()
        assert torch.isfinite(out).all() and torch.isfinite(diag).all() and np.isfinite(tr).all()
        for b in range(tr.shape[0]):
            e_inc, last, history = np.inf, None, []
            for r in range(tr.shape[1]):
                valid = np.isin(tr[b, r, :, 1], (0, 1))
                best = int(np.argmin(np.where(valid, tr[b, r, :, 0], np.inf)))
                kept = np.nonzero(tr[b, r, :, 3])[0]
                assert kept.size <= 1
                if tr[b, r, best, 0] < e_inc:                                     # the minimum over the valid candidates, when it is lower
                    assert kept.tolist() == [best]
                    e_inc, last = tr[b, r, best, 0], (r, best)
                else:
                    assert kept.size == 0
                history.append(e_inc)
            assert last is not None and int(status[b]) == int(tr[b, last[0], last[1], 1])
            assert float(diag[b, 11]) == tr[b, last[0], last[1], 2]               # the kept candidate's own row
            print(f"chain {b}: E_inc after every round {history}")
            assert (np.diff(history) <= 0).all()


def test_a_chain_without_a_valid_candidate_keeps_its_status(batch):
    from text2protein_amd.refine import refine_backbone_batch, refine_rounds_batch
    xyz, absval, n = batch
    xyz = xyz.clone()
    xyz[0, 2, 1, 0] = float("nan")
    n = torch.tensor([8, 1], dtype=torch.int32)
    out, status, diag, trace = refine_rounds_batch(xyz, absval, n, 2, 2, schedules=[RO.short_schedule(2)] * 2)
    want = refine_backbone_batch(xyz, absval, n, RO.short_schedule(2))
    assert status.cpu().tolist() == [2, -1] == want[1].cpu().tolist()
    assert not out.any() and not diag.any() and not trace[..., 0].any() and not trace[..., 2:].any()
    assert trace[0, :, :, 1].eq(2).all() and trace[1, :, :, 1].eq(-1).all()


def test_limits_are_refused():
    from text2protein_amd import _lib
    from text2protein_amd.refine import refine_rounds_batch
    ws = _lib.load().t2p_op_refine_rounds_ws
    assert ws(1, 257, 2, 2) == -1 and ws(1, 8, 9, 2) == -1 and ws(1, 8, 2, 17) == -1 and ws(1, 8, 2, 0) == -1 and ws(1, 8, 2, 2) > 0
    n = torch.tensor([8])
    small = (torch.zeros(1, 8, 3, 3, device="cuda"), torch.zeros(1, 4, 64, device="cuda"), n)
    big = (torch.zeros(1, 257, 3, 3, device="cuda"), torch.zeros(1, 4, 257 * 257, device="cuda"), torch.tensor([257]))
    with pytest.raises(ValueError, match="REFINE_MAX_L"):
        refine_rounds_batch(*big, rounds=2, replicas=2)
    for kw in (dict(rounds=9), dict(replicas=17), dict(replicas=0)):
        with pytest.raises(ValueError):
            refine_rounds_batch(*small, **kw)


def test_fold_with_rounds_end_to_end():
    from text2protein_amd.encode import encode_6d_batch
    from text2protein_amd.fold import fold_6d_batch
    fold_gold = load_golden("fold_chains")
    truth = fold_gold["xyz_48"]
    coords = encode_6d_batch(torch.from_numpy(truth).float().unsqueeze(0).cuda(), torch.tensor([48], dtype=torch.int32))["coords_6d"]
    single = fold_6d_batch(coords, refine=True)
    same = fold_6d_batch(coords, refine=True, refine_rounds=1, refine_replicas=1)
    assert torch.equal(single["xyz"], same["xyz"]) and "refine_rounds" not in same
    r = fold_6d_batch(coords, refine=True, refine_rounds=2, refine_replicas=2, refine_seed=4)
    assert torch.equal(r["xyz_fold"], single["xyz_fold"]) and len(r["refine_rounds"][0]) == 2 and len(r["refine_rounds"][0][0]["candidates"]) == 2
    assert r["refine_rounds"][0][0]["kept"] is not None and r["refine"][0]["status"] in (0, 1) and torch.isfinite(r["xyz"]).all()


def test_cli_rounds_write_the_kept_chain_and_a_rounds_block(tmp_path):
    from text2protein_amd.encode import read_backbone
    cfg = cfg_ckpt()
    cfg.training.sde = "vesde"
    cfg.model.condition = ["length"]
    cfg_path = tmp_path / "ckpt_length.yml"
    with open(cfg_path, "w") as f:
        yaml.safe_dump(yaml.safe_load(json.dumps(cfg)), f)
    out = tmp_path / "out"
    cmd = [sys.executable, os.path.join(ROOT, "sampling_6d.py"), str(cfg_path), os.path.join(GOLDEN, "tiny_checkpoint.pth"), "--batch_size", "2",
           "--context_tokens", "4", "--dtype", "f32", "--select_length", "1", "--length_index", "4", "--outdir", str(out),
           "--refine_rounds", "2", "--refine_replicas", "2"]
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=600, cwd=str(tmp_path))
    assert r.returncode == 0, r.stdout + r.stderr
    for i in (0, 1):
        xyz, ok, n = read_backbone(str(out / f"refined_{i}.pdb"))
        with open(out / f"fold_{i}.json") as f:
            d = json.load(f)
        rounds = d["refine"]["rounds"]
        assert n == 7 == d["L"] and ok.all() and np.isfinite(xyz).all()
        assert len(rounds) == 2 and all(len(rd["candidates"]) == 2 for rd in rounds)
        assert rounds[0]["kept"] in (0, 1) and all(sorted(c) == ["e_sel", "evaluations", "status"] for rd in rounds for c in rd["candidates"])
        assert d["refine"]["status"] in (0, 1)
