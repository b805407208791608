"""The random inpainting mask of training on the GPU: the operator (t2p_op_inpaint_mask_draw), the trainer's request
(t2p_train_set_inpaint_draw) and the Python mirror (HipTrainModel.set_inpaint_draw, get_step_fn(..., inpaint_mask_draw=...)).

Oracles: tests/inpaint_cases.device_draw, the numpy restatement of the device draw on oracle/philox.py (bit for bit: the draw is integer
arithmetic); tests/golden/inpaint_masks.npz, the masks the reference's own ``random_mask_batch`` (utils.py:15-60) drew under recorded
seeds; tests/golden/train_tinyB_inpaintdraw_{rand,contig}.npz, autograd through the reference UNetModel on train_tinyB's inputs with two
of those masks (tests/golden/make_golden_train_inpaint.py).  Architecture and inputs are train_tinyB's and only the mask differs, so the
fp32 tolerances are the ones test_gpu_train_ss.py uses.  Everything runs at L = 16 (one L = 15 operator case takes the byte-store path).

Bitwise comparisons of whole trainer states run in f16, the mode in which two identical steps are bitwise equal at all (fixed-order
reductions; the f32 step sums its weight gradients with atomics).  A loss is compared with ``==`` in either mode: the forward pass is
deterministic and the scalar is a double sum rounded to float once.
"""
import ctypes as C
import random

import numpy as np
import pytest
import torch

from helpers import TRAIN_CASES, check_step_against_fixture, load_golden, train_inputs
from inpaint_cases import (INPAINT_STREAM, INPAINT_TRAIN_CASES, INPAINTING, LENGTHS, MODE_CONTIGUOUS, MODE_NONE, MODE_RANDOM, cfg_inpaint,
                           device_draw, device_mode, len_lo_hi)
from sde_train_cases import make_sde
from test_gpu_train import GRAD_TOL, LOSS_TOL, PARAM_TOL
from test_gpu_train_sde import _all_state, _batch, _masks, _state

pytestmark = pytest.mark.gpu

PR, PC = INPAINTING["random_mask_prob"], INPAINTING["contiguous_mask_prob"]
REFUSAL = "the inpainting condition needs batch.mask_inpaint"
CASE = dict(TRAIN_CASES["train_tinyB"], sde="ve")
L = 16


def _trainer_seed():
    """The smallest trainer seed whose first loss call draws a random mask and whose second draws a contiguous one (from the numpy
    restatement: the tests below then see two different, non-trivial masks on consecutive calls)."""
    for s in range(1000):
        if device_mode(s, INPAINT_STREAM, PR, PC) == MODE_RANDOM and device_mode(s, 4096 + INPAINT_STREAM, PR, PC) == MODE_CONTIGUOUS:
            return s
    raise AssertionError("no such seed below 1000")


SEED = _trainer_seed()


def _setup(dtype="f32", seed=SEED, case=CASE):
    from text2protein_amd import synth
    from text2protein_amd.losses import HipTrainModel
    cfg = cfg_inpaint()
    cfg.device = "cuda:0"
    inp = train_inputs(cfg, case)
    model = HipTrainModel(cfg, device="cuda:0", seed=seed, dtype=dtype)
    model.load_state_dict(synth.synth_state_dict(cfg, case["seed"]))
    model.set_dropout_masks(_masks(case, cfg, model))
    return cfg, inp, model


def _fns(cfg, **kw):
    from text2protein_amd import losses, sde_lib
    sde = make_sde(sde_lib, cfg, CASE)
    return (losses.get_step_fn(sde, train=True, optimize_fn=losses.optimization_manager(cfg), **kw), losses.get_step_fn(sde, train=False, **kw))


def _nomask(inp):
    """train_tinyB's batch WITHOUT mask_inpaint, with the residue counts the draw needs."""
    b = {k: v for k, v in _batch(inp).items() if k != "mask_inpaint"}
    b["lengths"] = torch.tensor(LENGTHS)
    return b


def _op(llh, Lx=L, pr=PR, pc=PC, seed=0, stream_id=0, force_mode=-1, flags=None, pair=None, B=None):
    """t2p_op_inpaint_mask_draw; returns (status, flags, pair, mode)."""
    from text2protein_amd import _lib
    lib = _lib.load()
    arr = np.ascontiguousarray(np.asarray(llh, dtype=np.int32).reshape(-1, 3))
    n = arr.shape[0] if B is None else B
    if flags is None:
        flags = torch.full((max(n, 1), Lx), 9, dtype=torch.uint8, device="cuda")
    if pair is None:
        pair = torch.full((max(n, 1), Lx, Lx), 9, dtype=torch.uint8, device="cuda")
    mode = C.c_int(-7)
    rc = lib.t2p_op_inpaint_mask_draw(C.c_void_p(arr.ctypes.data), n, Lx, float(pr), float(pc), seed, stream_id, force_mode, _lib.ptr(flags),
                                      _lib.ptr(pair), C.byref(mode), _lib.stream_ptr())
    torch.cuda.synchronize()
    return rc, flags, pair, mode.value


def _device_mask(seed, calls):
    """The (B, L, L) bool mask the trainer of ``seed`` draws in its loss call number ``calls`` (stream 4096 calls + 3), from the operator."""
    rc, _, pair, mode = _op(len_lo_hi(LENGTHS), seed=seed, stream_id=4096 * calls + INPAINT_STREAM)
    assert rc == 0
    return pair.bool(), mode


# ---- 1. the operator ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("Lx", [16, 15])
def test_operator_equals_the_numpy_restatement(Lx):
    """B = 64 samples of 2 .. Lx residues; each forced mode and the drawn mode under 8 stream ids: flags, pair mask and mode equal the numpy
    restatement bit for bit, pair = flags OR flags^T, padding columns are 0 except in mode none.  L = 16 stores four pixels at a time,
    L = 15 byte by byte."""
    lengths = [2 + k % (Lx - 1) for k in range(64)]
    assert min(lengths) == 2 and max(lengths) == Lx
    llh = len_lo_hi(lengths)
    runs = [(fm, 4096 * 3 + INPAINT_STREAM) for fm in (MODE_NONE, MODE_RANDOM, MODE_CONTIGUOUS)] + [(-1, 4096 * k + INPAINT_STREAM) for k in range(8)]
    seen = set()
    for fm, stream in runs:
        rc, flags, pair, mode = _op(llh, Lx, seed=77, stream_id=stream, force_mode=fm)
        assert rc == 0
        f, p = flags.cpu().numpy(), pair.cpu().numpy()
        wf, wp, wmode, r, _ = device_draw(llh, Lx, PR, PC, 77, stream, fm)
        assert mode == wmode and (fm < 0 or mode == fm)
        assert np.array_equal(f, wf) and np.array_equal(p, wp), (fm, stream)
        assert np.array_equal(p, f[:, :, None] | f[:, None, :]) and set(np.unique(f).tolist()) <= {0, 1}
        if mode == MODE_NONE:
            assert f.all()
        else:
            assert np.array_equal(f.sum(1), r)
            assert all(not f[b, l:].any() for b, l in enumerate(lengths))
        seen.add(mode)
    assert seen == {MODE_NONE, MODE_RANDOM, MODE_CONTIGUOUS}
    assert {device_mode(77, 4096 * k + INPAINT_STREAM, PR, PC) for k in range(8)} == seen      # the drawn runs alone reach all three


def test_operator_edges():
    """lo = 0 with hi = 1 (r = 0: nothing flagged), hi - lo = 1 away from zero (r = lo exactly), l = L, l = 2; another seed or stream gives
    other draws; and every refusal returns an error and leaves the outputs untouched."""
    from text2protein_amd import _lib
    lib = _lib.load()
    llh = np.array([(16, 0, 1), (16, 5, 6), (16, 0, 15), (2, 0, 1), (16, 15, 16), (9, 8, 9)], dtype=np.int32)
    for fm in (MODE_RANDOM, MODE_CONTIGUOUS):
        rc, flags, pair, mode = _op(llh, seed=5, stream_id=INPAINT_STREAM, force_mode=fm)
        assert rc == 0 and mode == fm
        f, p = flags.cpu().numpy(), pair.cpu().numpy()
        wf, wp, _, r, start = device_draw(llh, L, PR, PC, 5, INPAINT_STREAM, fm)
        assert np.array_equal(f, wf) and np.array_equal(p, wp)
        assert list(f.sum(1))[:2] == [0, 5] and f.sum(1)[3] == 0 and f.sum(1)[4] == 15 and f.sum(1)[5] == 8
        assert not p[0].any() and not p[3].any()                   # r = 0: an all-False mask, num_elem = 0 downstream
        assert not f[5, 9:].any() and not f[3, 2:].any()
        if fm == MODE_CONTIGUOUS:
            assert start[4] == 0 and f[4, :15].all() and not f[4, 15]       # l - r = 1: the only window
    a = _op(llh, seed=5, stream_id=INPAINT_STREAM, force_mode=MODE_RANDOM)[1]
    assert torch.equal(a, _op(llh, seed=5, stream_id=INPAINT_STREAM, force_mode=MODE_RANDOM)[1])
    assert not torch.equal(a, _op(llh, seed=6, stream_id=INPAINT_STREAM, force_mode=MODE_RANDOM)[1])
    assert not torch.equal(a, _op(llh, seed=5, stream_id=4096 + INPAINT_STREAM, force_mode=MODE_RANDOM)[1])
    # refusals
    flags = torch.full((3, L), 7, dtype=torch.uint8, device="cuda")
    pair = torch.full((3, L, L), 7, dtype=torch.uint8, device="cuda")
    ok = [(16, 0, 15), (11, 0, 10), (6, 0, 5)]
    for rows, kw, what in ((ok, dict(pr=1.2), "[0, 1]"), (ok, dict(pr=-0.1), "[0, 1]"), (ok, dict(pc=1.5), "[0, 1]"), (ok, dict(pc=-1e-3), "[0, 1]"),
                           (ok, dict(pr=0.6, pc=0.5), "exceed 1"),
                           ([(16, 0, 15), (-1, 0, 1), (6, 0, 5)], {}, "outside"), ([(16, 0, 15), (17, 0, 16), (6, 0, 5)], {}, "outside"),
                           ([(16, 0, 15), (1, 0, 0), (6, 0, 5)], {}, "range"), ([(16, 4, 3), (11, 0, 10), (6, 0, 5)], {}, "range"),
                           ([(16, 0, 15), (11, 0, 12), (6, 0, 5)], {}, "range"), ([(16, -1, 15), (11, 0, 10), (6, 0, 5)], {}, "range"),
                           (ok, dict(force_mode=3), "force_mode"), (ok, dict(force_mode=-2), "force_mode"), (ok, dict(B=0), "arguments"),
                           (ok, dict(Lx=257), "256")):
        if kw.get("Lx"):
            rows = [(257, 0, 200)] * 3              # valid for L = 257, whose outputs would not fit: refused before anything is written
        rc, _, _, mode = _op(rows, flags=flags, pair=pair, **kw)
        assert rc != 0 and what in lib.t2p_last_error().decode(), (what, lib.t2p_last_error())
        assert mode == -7
    assert (flags == 7).all() and (pair == 7).all()


# ---- 2. supplied masks and the host route against the reference -------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(INPAINT_TRAIN_CASES))
def test_training_step_vs_reference(name):
    """ONE fp32 step on train_tinyB's inputs with the reference's random mask of one seed: the fixture's mask passed as mask_inpaint for
    the loss, the score and every gradient; then the step through get_step_fn(inpaint_mask_draw="host") on a batch WITHOUT a mask under
    the fixture's random.seed / torch.manual_seed, and the post-step state -- all at test_gpu_train_ss.py's fp32 tolerances."""
    g = load_golden(name)
    case = INPAINT_TRAIN_CASES[name]
    masks = load_golden("inpaint_masks")
    assert np.array_equal(g["mask_inpaint"], masks["masks"][case["mask_seed"]]) and int(masks["modes"][case["mask_seed"]]) == case["mask_mode"]
    cfg, inp, model = _setup(case=case)
    inp = dict(inp, mask_inpaint=torch.from_numpy(g["mask_inpaint"]))
    step_fn, _ = _fns(cfg, inpaint_mask_draw="host")
    from text2protein_amd import sde_lib
    model.set_sde(make_sde(sde_lib, cfg, case))

    def seed_host():
        random.seed(case["mask_seed"])
        torch.manual_seed(case["mask_seed"])

    base_loss = float(load_golden(case["base"])["loss"])
    assert abs(float(g["loss"]) - base_loss) > 100 * LOSS_TOL * abs(base_loss)        # the fixture tells train_tinyB's own mask apart
    check_step_against_fixture(name, g, case, cfg, inp, model, step_fn, _batch(inp), loss_tol=LOSS_TOL, score_tol=1e-5, grad_tol=GRAD_TOL,
                               param_tol=PARAM_TOL, delta_tol=None, before_step=seed_host, step_batch=_nomask(inp))


@pytest.mark.parametrize("seed", [1, 0, 5])
def test_host_route_equals_the_supplied_mask_bitwise(seed):
    """get_step_fn(..., inpaint_mask_draw="host") under a fixture seed (random, contiguous, none) gives the loss of the step that is handed
    the fixture's mask, bitwise (t and z given, Dropout_0 by given keep-masks); train and eval alike."""
    mask = torch.from_numpy(load_golden("inpaint_masks")["masks"][seed])
    out = {}
    for how in ("supplied", "host"):
        cfg, inp, model = _setup()
        step_fn, eval_fn = _fns(cfg, inpaint_mask_draw="host")
        batch = dict(_nomask(inp), mask_inpaint=mask) if how == "supplied" else _nomask(inp)
        state = _state(model, cfg, CASE["step0"])
        random.seed(seed)
        torch.manual_seed(seed)
        e = eval_fn(state, batch, condition=cfg.model.condition, t=inp["t"], z=inp["z"])
        random.seed(seed)
        torch.manual_seed(seed)
        l = step_fn(state, batch, condition=cfg.model.condition, t=inp["t"], z=inp["z"])
        assert "mask_inpaint" not in batch or how == "supplied"       # the caller's batch is not written to
        out[how] = (e, l)
        del model
    print(f"seed {seed}: eval / train loss, supplied {out['supplied']}, host route {out['host']}")
    assert out["host"] == out["supplied"] and np.isfinite(out["host"]).all()


# ---- 3. the device route ------------------------------------------------------------------------------------------------------------------
def test_device_route_equals_the_operator_mask_bitwise():
    """Two consecutive f16 steps with inpaint_mask_draw="device" on a batch without a mask, against two steps on a second trainer of the
    same seed that is handed the masks t2p_op_inpaint_mask_draw returns for (seed, 4096 calls + 3), calls = 0, 1: the losses and the
    whole state (parameters, gradients, EMA, both moments) are bitwise equal after each step, and the two masks differ."""
    m0, mode0 = _device_mask(SEED, 0)
    m1, mode1 = _device_mask(SEED, 1)
    assert (mode0, mode1) == (MODE_RANDOM, MODE_CONTIGUOUS) and not torch.equal(m0, m1) and m0.any() and m1.any()
    runs = {}
    for how in ("device", "supplied"):
        cfg, inp, model = _setup("f16")
        step_fn, _ = _fns(cfg, **({"inpaint_mask_draw": "device"} if how == "device" else {}))
        state = _state(model, cfg, CASE["step0"])
        seq = []
        for m in (m0, m1):
            batch = _nomask(inp) if how == "device" else dict(_nomask(inp), mask_inpaint=m)
            loss = step_fn(state, batch, condition=cfg.model.condition, t=inp["t"], z=inp["z"])
            seq.append((loss, _all_state(model), model.get_step()))
        runs[how] = seq
        del model
    print("device route losses:", [s[0] for s in runs["device"]], "supplied:", [s[0] for s in runs["supplied"]])
    assert runs["device"][0][0] != runs["device"][1][0]
    for a, b in zip(runs["device"], runs["supplied"]):
        assert a[0] == b[0] and a[2] == b[2] and np.isfinite(a[0])
        for w in a[1]:
            for n in a[1][w]:
                assert torch.equal(a[1][w][n], b[1][w][n]), (w, n)


def test_request_is_consumed_and_a_supplied_mask_wins():
    """One pass consumes the request: it computes the loss of the operator's mask, and the next pass without a mask gets the refusal that
    a trainer without a request gives.  A pass whose batch supplies a mask computes with that mask and clears the request too."""
    from text2protein_amd._lib import T2PError
    cfg, inp, model = _setup()
    nomask, own = _nomask(inp), _batch(inp)                            # own: train_tinyB's mask_info mask
    with pytest.raises(T2PError) as e0:
        model.loss(nomask, t=inp["t"], z=inp["z"])
    assert REFUSAL in str(e0.value)
    # (the refused pass above counted as loss call 0: the trainer's next draw is call 1's)
    m1, _ = _device_mask(SEED, 1)
    model.set_inpaint_draw(LENGTHS, cfg.model.inpainting)
    l_draw = model.loss(nomask, t=inp["t"], z=inp["z"])
    with pytest.raises(T2PError) as e1:
        model.loss(nomask, t=inp["t"], z=inp["z"])
    assert str(e1.value) == str(e0.value)
    l_m1 = model.loss(dict(nomask, mask_inpaint=m1), t=inp["t"], z=inp["z"])
    l_own = model.loss(own, t=inp["t"], z=inp["z"])
    assert l_draw == l_m1 and l_draw != l_own
    model.set_inpaint_draw(LENGTHS, cfg.model.inpainting)
    assert model.loss(own, t=inp["t"], z=inp["z"]) == l_own            # the supplied mask wins ...
    with pytest.raises(T2PError) as e2:
        model.loss(nomask, t=inp["t"], z=inp["z"])                     # ... and the request is gone
    assert str(e2.value) == str(e0.value)
    model.set_inpaint_draw(LENGTHS, cfg.model.inpainting)
    model.set_inpaint_draw([], None)                                   # cleared by hand
    with pytest.raises(T2PError, match=REFUSAL):
        model.loss(nomask, t=inp["t"], z=inp["z"])


def test_eval_loss_takes_the_request():
    """train.py draws before the eval step too (:193): eval_loss after set_inpaint_draw equals eval_loss with the operator's mask supplied,
    consumes the request, and goes through the step function with train=False."""
    from text2protein_amd._lib import T2PError
    m0, _ = _device_mask(SEED, 0)
    cfg, inp, model = _setup()
    model.set_inpaint_draw(LENGTHS, cfg.model.inpainting)
    e_draw = model.eval_loss(_nomask(inp), t=inp["t"], z=inp["z"])
    with pytest.raises(T2PError, match=REFUSAL):
        model.eval_loss(_nomask(inp), t=inp["t"], z=inp["z"])
    e_m0 = model.eval_loss(dict(_nomask(inp), mask_inpaint=m0), t=inp["t"], z=inp["z"])
    e_own = model.eval_loss(_batch(inp), t=inp["t"], z=inp["z"])
    cfg2, inp2, fresh = _setup()
    _, eval_fn = _fns(cfg2, inpaint_mask_draw="device")
    e_fn = eval_fn(_state(fresh, cfg2, CASE["step0"]), _nomask(inp2), condition=cfg2.model.condition, t=inp2["t"], z=inp2["z"])
    print(f"eval_loss: drawn {e_draw}, operator's mask {e_m0}, through the step function {e_fn}, train_tinyB's own mask {e_own}")
    assert e_draw == e_m0 == e_fn and e_draw != e_own


# ---- 4. refusals --------------------------------------------------------------------------------------------------------------------------
def test_wrong_batch_size_fails_the_pass_and_changes_nothing():
    """A request for 2 samples meets a batch of 3: the step raises, parameters, gradients, moments, EMA and counters are what they were,
    and the request is cleared."""
    from text2protein_amd._lib import T2PError
    cfg, inp, model = _setup()
    model.loss(_batch(inp), t=inp["t"], z=inp["z"], backward=True)     # a gradient buffer worth keeping
    model.set_step(CASE["step0"], 3, 3)
    before, steps = _all_state(model), model.get_step()
    step_fn, _ = _fns(cfg)
    state = _state(model, cfg, CASE["step0"])
    model.set_inpaint_draw(LENGTHS[:2], cfg.model.inpainting)
    with pytest.raises(T2PError, match="inpaint draw: the request holds 2 samples, the batch 3"):
        step_fn(state, _nomask(inp), condition=cfg.model.condition, t=inp["t"], z=inp["z"])
    after = _all_state(model)
    for w in before:
        for n in before[w]:
            assert torch.equal(before[w][n], after[w][n]), (w, n)
    assert model.get_step() == steps and state["step"] == CASE["step0"]
    with pytest.raises(T2PError, match=REFUSAL):
        model.loss(_nomask(inp), t=inp["t"], z=inp["z"])
    # through the step function: a batch without residue counts, and an empty range, are refused before any native pass
    dev_fn, _ = _fns(cfg, inpaint_mask_draw="device")
    no_len = {k: v for k, v in _nomask(inp).items() if k != "lengths"}
    with pytest.raises(T2PError, match="residue counts"):
        dev_fn(state, no_len, condition=cfg.model.condition, t=inp["t"], z=inp["z"])
    with pytest.raises(T2PError, match="range"):
        dev_fn(state, dict(no_len, lengths=[16, 1, 6]), condition=cfg.model.condition, t=inp["t"], z=inp["z"])
    assert model.get_step() == steps and state["step"] == CASE["step0"]


def test_setter_refusals():
    """A trainer created without the inpainting condition refuses the setter (clearing stays allowed); bad arguments on a trainer with
    the condition leave the request that was set before them in place."""
    from text2protein_amd._lib import T2PError
    from text2protein_amd.config import AttrDict
    from test_gpu_train_sde import _model
    plain_case = TRAIN_CASES["train_tiny"]
    plain_cfg = plain_case["config"]()
    assert "inpainting" not in plain_cfg.model.condition
    plain = _model(plain_case, plain_cfg)
    with pytest.raises(T2PError, match="inpainting condition"):
        plain.set_inpaint_draw([12, 9], AttrDict(INPAINTING))
    plain.set_inpaint_draw([], None)
    pin = train_inputs(plain_cfg, plain_case)
    assert np.isfinite(plain.loss(_batch(pin), t=pin["t"], z=pin["z"]))
    cfg, inp, model = _setup()
    m0, _ = _device_mask(SEED, 0)
    model.set_inpaint_draw(LENGTHS, cfg.model.inpainting)
    for lengths, over, what in ((LENGTHS, dict(random_mask_prob=1.5), r"\[0, 1\]"), (LENGTHS, dict(contiguous_mask_prob=-0.2), r"\[0, 1\]"),
                                (LENGTHS, dict(random_mask_prob=0.7, contiguous_mask_prob=0.4), "exceed 1"), ([16, 17, 6], {}, "outside"),
                                ([16, -1, 6], {}, "outside"), ([16, 1, 6], {}, "range"), (LENGTHS, dict(mask_min_len=0.9, mask_max_len=0.1), "range"),
                                (LENGTHS, dict(mask_max_len=1.5), "range")):
        with pytest.raises(T2PError, match=what):
            model.set_inpaint_draw(lengths, AttrDict(dict(INPAINTING, **over)))
    l_draw = model.loss(_nomask(inp), t=inp["t"], z=inp["z"])         # the request set first is still there
    assert l_draw == model.loss(dict(_nomask(inp), mask_inpaint=m0), t=inp["t"], z=inp["z"])


# ---- 5. the num_elem = 0 sample ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dt", ["f32", "f16"])
def test_sample_without_masked_residues_stays_finite(dt):
    """Seed 7's random mask leaves sample 0 without a masked residue: num_elem = 0, its loss term 0 / 1e-8 = 0.  Loss and every gradient
    are finite, and a step goes through."""
    from text2protein_amd import losses
    g = load_golden("inpaint_masks")
    mask = torch.from_numpy(g["masks"][7])
    assert int(g["modes"][7]) == MODE_RANDOM and not mask[0].any() and mask[1].any() and mask[2].any()
    cfg, inp, model = _setup(dt)
    batch = dict(_nomask(inp), mask_inpaint=mask)
    loss = model.loss(batch, t=inp["t"], z=inp["z"], backward=True)
    grads = model.read(losses.GRAD)
    assert np.isfinite(loss) and loss > 0 and all(bool(torch.isfinite(v).all()) for v in grads.values())
    assert any(float(v.abs().max()) > 0 for v in grads.values())
    model.set_step(CASE["step0"])
    assert np.isfinite(model.step(batch, t=inp["t"], z=inp["z"]))
    assert all(bool(torch.isfinite(v).all()) for v in model.read(losses.PARAM).values())
