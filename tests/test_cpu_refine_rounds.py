"""The refinement in rounds without a GPU: the float64 oracle's phi / psi move (tests/refine_rounds_oracle.py) keeps what the move must
keep and changes what it must change, its recorded protocol run (tests/golden/refine_rounds.npz) has a margin at every selection, and
the constants, the C ABI and the command line of the product agree with the description."""
import json
import os
import re
import subprocess
import sys

import numpy as np
import pytest

import refine_oracle as RO
import refine_rounds_oracle as RR
from helpers import load_golden
from oracle import philox

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CHAINS = ("96w8", "96cut")


@pytest.fixture(scope="module")
def starts():
    g = load_golden("refine_cases")
    return {c: g[f"start_{c}"].astype(np.float64) for c in CHAINS}


@pytest.fixture(scope="module")
def gold():
    g = load_golden("refine_rounds")
    g["meta"] = json.loads(str(g["meta"]))
    return g


@pytest.mark.parametrize("case", CHAINS)
def test_oracle_move_keeps_bonds_and_angles_and_moves_only_phi_and_psi(starts, case):
    x = starts[case]
    n = x.shape[0]
    dphi, dpsi = RR.draws(seed=5, stream=3, chain_id=7, n=n)
    assert np.abs(dphi).max() <= RR.AMP and np.abs(dpsi).max() <= RR.AMP and np.abs(dphi).max() > 0.5 * RR.AMP
    d = RR.torsion_deltas(n, dphi, dpsi)
    y = RR.rebuild(x, d)
    b0, t0, u0 = RR.internals(x)
    b1, t1, u1 = RR.internals(y)
    gap_b, gap_t = np.abs(b1 - b0).max(), np.abs(t1 - t0).max()
    gap_u = np.abs(RO._wrap(u1 - u0 - d)).max()
    print(f"{case}: bond gap {gap_b:.2e}, angle gap {gap_t:.2e}, torsion gap {gap_u:.2e}")
    assert gap_b <= 1e-12 and gap_t <= 1e-12 and gap_u <= 1e-12
    k = np.arange(3, 3 * n)
    omega, phi, psi = k[k % 3 == 1], k[k % 3 == 2], k[k % 3 == 0]
    assert (d[omega] == 0).all() and np.abs(RO._wrap(u1 - u0)[omega]).max() <= 1e-12                   # omega not at all
    assert np.array_equal(d[phi], np.deg2rad(dphi[1:])) and np.array_equal(d[psi], np.deg2rad(dpsi[:n - 1]))
    assert np.array_equal(y.reshape(-1, 3)[:3], x.reshape(-1, 3)[:3])
    assert np.abs(y - x).max() > 0.1                                                                    # and it is a move


@pytest.mark.parametrize("case", CHAINS)
def test_oracle_move_with_zero_draws_returns_the_input(starts, case):
    x = starts[case]
    gap = np.abs(RR.rebuild(x, np.zeros(3 * x.shape[0])) - x).max()
    print(f"{case}: zero-draw gap {gap:.2e}")
    assert gap <= 1e-12
    assert np.array_equal(RR.perturb(x, replicas=2, keep_first=True)[0], x)


def test_oracle_move_is_finite_on_collinear_atoms():
    x = np.zeros((3, 3, 3))
    x[:, :, 0] = np.arange(9).reshape(3, 3) * 1.4                                                       # nine atoms on a line
    y = RR.perturb(x, seed=1, replicas=2)
    assert np.isfinite(y).all() and np.allclose(y, x, atol=1e-9)                                        # tau cannot bend a straight chain
    assert np.isfinite(RR.perturb(np.zeros((3, 3, 3)), seed=1)).all()                                   # coincident atoms


def test_draws_follow_the_training_layout():
    n, seed, stream, cid = 6, (9 << 32) + 5, (1 << 33) + 4, 11
    c = np.array([[i, cid, stream & 0xFFFFFFFF, stream >> 32] for i in range(n)], dtype=np.uint64)
    w = philox.philox4x32_10(c, np.array([seed & 0xFFFFFFFF, seed >> 32], dtype=np.uint64))
    u = philox.uniform24(w).astype(np.float64)
    dphi, dpsi = RR.draws(seed, stream, cid, n, amp=10.0)
    assert np.array_equal(dphi, 10.0 * (2.0 * u[:, 0] - 1.0)) and np.array_equal(dpsi, 10.0 * (2.0 * u[:, 1] - 1.0))
    other = RR.draws(seed, stream, cid + 1, n)[0]
    assert not np.array_equal(other, dphi)


def test_reference_rounds_and_select_stage_equal_the_references_tables():
    from text2protein_amd import refine as R
    rounds = R.reference_rounds()
    assert len(rounds) == 5 and all(len(s) == 3 for s in rounds)
    assert [s[0][4] for s in rounds] == [3.0, 5.0, 10.0, 10.0, 10.0]                                    # vdw_weight
    assert [s[0][2] for s in rounds] == [3.0, 2.0, 1.0, 1.0, 1.0]                                       # rsr_dist_weight
    assert [s[0][3] for s in rounds] == [1.0, 1.0, 0.5, 0.5, 0.5]                                       # rsr_orient_weight
    for r, sched in enumerate(rounds):
        assert [(s[0], s[1]) for s in sched] == [(1, 12), (1, 24), (1, R.SEP_ALL)]
        assert all(s[2:5] == sched[0][2:5] and s[5] == 300 for s in sched)
        assert sched == RR.round_schedule(r)
    assert rounds[0] == R.default_schedule()                                                            # run 0 is today's schedule
    assert [s[0] for s in R.reference_rounds(2, sep_lo=3)[1]] == [3, 3, 3]
    assert R.SELECT_STAGE == (1, R.SEP_ALL, 1.0, 0.5, 5.0, 0) == RR.SELECT_STAGE                        # scorefxn_cart.wts
    assert (R.MAX_ROUNDS, R.MAX_REPLICAS, R.STREAM_STRIDE, R.AMP_DEG) == (8, 16, 16, 10.0)


def test_header_signatures_and_sources_declare_the_entry_points():
    from text2protein_amd import _lib, build
    assert "refine_rounds.hip" in build.SOURCES and os.path.exists(os.path.join(build.CSRC, "refine_rounds.hip"))
    hdr = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "t2p.h")).read(), flags=re.S)
    for name, n_args in (("t2p_op_perturb_torsions", 13), ("t2p_op_refine_rounds_ws", 4), ("t2p_op_refine_rounds", 24),
                         ("t2p_op_refine_backbone", 16)):
        m = re.search(r"\b" + name + r"\s*\(([^)]*)\)", hdr)
        assert m and len(m.group(1).split(",")) == n_args == len(_lib.SIGNATURES[name][1]), name
    assert hdr.index("t2p_op_restraint_energy") < hdr.index("t2p_op_perturb_torsions") < hdr.index("t2p_op_refine_rounds_ws")
    kh = open(os.path.join(build.CSRC, "t2p_kernels.h")).read()
    assert "REFINE_MAX_ROUNDS = 8, REFINE_MAX_REPLICAS = 16, REFINE_STREAM_STRIDE = 16;" in kh
    assert "t2p_op_perturb_torsions" in open(os.path.join(build.CSRC, "philox.h")).read()
    lib = _lib.load()
    ws = lib.t2p_op_refine_rounds_ws
    assert ws(2, 257, 2, 2) == -1 and ws(2, 40, 9, 2) == -1 and ws(2, 40, 2, 17) == -1 and ws(2, 40, 2, 0) == -1 and ws(2, 40, 0, 2) == -1
    assert ws(0, 40, 2, 2) == -1 and ws(2, 0, 2, 2) == -1
    assert ws(2, 40, 2, 3) > lib.t2p_op_refine_ws(6, 40) and ws(2, 40, 8, 3) == ws(2, 40, 1, 3)


def test_rounds_have_no_cpu_path_and_refuse_bad_limits():
    import torch
    from text2protein_amd._lib import T2PError
    from text2protein_amd.refine import perturb_torsions, refine_rounds_batch
    x, a, n = torch.zeros(1, 8, 3, 3), torch.zeros(1, 4, 64), torch.tensor([8])
    with pytest.raises(T2PError, match="no CPU fallback"):
        perturb_torsions(x, n)
    with pytest.raises(T2PError, match="no CPU fallback"):
        refine_rounds_batch(x, a, n, rounds=2, replicas=2)
    for kw in (dict(rounds=9), dict(replicas=17), dict(replicas=0), dict(rounds=0)):
        with pytest.raises(ValueError):
            refine_rounds_batch(x, a, n, **kw)


def test_cli_help_shows_the_rounds_options():
    r = subprocess.run([sys.executable, os.path.join(ROOT, "sampling_6d.py"), "--help"], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and "--refine_rounds" in r.stdout and "--refine_replicas" in r.stdout


def test_recorded_protocol_has_a_margin_at_every_selection(gold):
    P = gold["meta"]["protocol"]
    assert tuple(P["chains"]) == RR.PROTOCOL["chains"] and (P["rounds"], P["replicas"], P["iters"]) == (2, 3, RO.SHORT_ITERS)
    assert gold["esel"].shape == (2, 2, 3) and gold["kept"].shape == (2, 2)
    for b, name in enumerate(P["chains"]):
        gaps = RR.selection_gaps(gold["esel"][b], gold["cstatus"][b])
        print(f"{name}: E_sel {gold['esel'][b].tolist()}, kept {gold['kept'][b].tolist()}, gaps {gaps.tolist()}")
        assert (gaps >= RR.MIN_GAP).all()
        e_inc = np.inf                                                  # the kept indices are what the recorded energies imply
        for r in range(P["rounds"]):
            k = int(np.argmin(gold["esel"][b, r]))
            want = k if gold["esel"][b, r, k] < e_inc else -1
            assert gold["kept"][b, r] == want
            e_inc = min(e_inc, gold["esel"][b, r, k])
    assert (gold["kept"] > 0).any()                                     # a perturbed candidate wins somewhere: the selection is exercised


def test_oracle_reproduces_the_recorded_short_chain(gold):
    fold_gold, cases = load_golden("fold_chains"), load_golden("refine_cases")
    P = RR.PROTOCOL
    schedules = [RR.round_schedule(r, P["iters"]) for r in range(P["rounds"])]
    res = RR.rounds(cases["start_96w8"], RO.case_maps(fold_gold, "96w8"), schedules, RR.SELECT_STAGE, P["replicas"], P["amp"],
                    int(gold["seed"]), P["stream_base"], P["chain_ids"][0])
    assert res["kept"] == gold["kept"][0].tolist() and np.array_equal(res["evals"], gold["evals"][0])
    assert np.allclose(res["esel"], gold["esel"][0], rtol=1e-9, atol=0) and np.abs(res["xyz"] - gold["xyz_96w8"]).max() <= 1e-6
    assert (np.diff(res["e_inc"]) <= 0).all()
