"""Text-context dropout on the GPU (training for classifier-free guidance): the operator (t2p_op_context_drop: the kernels
context_drop_draw and zero_sample_rows alone), the trainer's request (t2p_train_set_context_drop) and the Python mirror
(HipTrainModel.set_context_drop, get_step_fn(context_dropout=...)).

Oracle: tests/golden/train_tinyB_ctxdrop.npz -- autograd through the reference UNetModel on train_tinyB's inputs with the context rows of
samples 0 and 2 set to zero (tests/golden/make_golden_train_ctxdrop.py).  Architecture and inputs are train_tinyB's and only zeros differ,
so the fp32 tolerances are test_gpu_train.py's own (the argument test_gpu_train_ss.py makes).  The device draw is checked bit for bit
against ctxdrop_cases.device_decisions (oracle/philox.py).
"""
import ctypes as C
import random

import numpy as np
import pytest
import torch

from ctxdrop_cases import CTXDROP_CASES, DECISIONS, DRAW_PAIRS, device_decisions, zeroed_context
from helpers import check_step_against_fixture, load_golden, train_inputs
from sde_train_cases import SDE_TRAIN_CASES, make_sde
from test_gpu_train import GRAD_TOL, LOSS_TOL, PARAM_TOL
from test_gpu_train_sde import _all_state, _batch, _masks, _state

pytestmark = pytest.mark.gpu

NAME = "train_tinyB_ctxdrop"
SENTINEL = 64            # floats on either side of the operator's buffer


def _case(name):
    return CTXDROP_CASES[name] if name in CTXDROP_CASES else SDE_TRAIN_CASES[name]


def _setup(name=NAME, dtype="f32", seed=11):
    """A trainer ready for its first pass: the case's weights, SDE and Dropout_0 keep-masks; ``seed`` is the trainer seed (the Philox key)."""
    from text2protein_amd import losses, sde_lib, synth
    case = _case(name)
    cfg = case["config"]()
    cfg.device = "cuda:0"
    inp = train_inputs(cfg, case)
    model = losses.HipTrainModel(cfg, device="cuda:0", seed=seed, dtype=dtype)
    model.load_state_dict(synth.synth_state_dict(cfg, case["seed"]))
    model.set_dropout_masks(_masks(case, cfg, model))
    model.set_sde(make_sde(sde_lib, cfg, case))
    return case, cfg, inp, model


def _fns(cfg, case, **kw):
    from text2protein_amd import losses, sde_lib
    sde = make_sde(sde_lib, cfg, case)
    return (losses.get_step_fn(sde, train=True, optimize_fn=losses.optimization_manager(cfg), **kw), losses.get_step_fn(sde, train=False, **kw))


def _assert_same_state(a, b):
    for w in a:
        for n in a[w]:
            assert torch.equal(a[w][n], b[w][n]), (w, n)


def _bits(t):
    return t.contiguous().view(torch.int32)


def _op(x_host, drop=None, p=0.5, seed=0, stream_id=0, want_decisions=False, batch=None, row_floats=None):
    """t2p_op_context_drop on x_host [B][n] placed between two sentinel blocks; returns (status, the whole allocation read back, the
    allocation as uploaded, the decisions used or None)."""
    from text2protein_amd import _lib
    lib = _lib.load()
    B, n = x_host.shape
    gen = torch.Generator().manual_seed(17)
    whole = torch.cat([torch.rand(SENTINEL, generator=gen) + 1.0, x_host.reshape(-1), torch.rand(SENTINEL, generator=gen) + 1.0])
    dev = whole.cuda()
    d = None if drop is None else np.ascontiguousarray(np.asarray(drop, dtype=np.uint8))
    used = torch.full((B,), 9, dtype=torch.uint8, device="cuda") if want_decisions else None
    rc = lib.t2p_op_context_drop(C.c_void_p(dev.data_ptr() + 4 * SENTINEL), B if batch is None else batch, n if row_floats is None else row_floats,
                                 None if d is None else C.c_void_p(d.ctypes.data), float(p), seed, stream_id, _lib.ptr(used), _lib.stream_ptr())
    torch.cuda.synchronize()
    return rc, dev.cpu(), whole, None if used is None else used.cpu()


def _patterns(B):
    return {"none": [0] * B, "all": [1] * B, "first only": [1] + [0] * (B - 1), "last only": [0] * (B - 1) + [1],
            "alternating": [(b + 1) % 2 for b in range(B)]}


# ---- 1. the operator ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("B", [1, 3, 5])
def test_operator_zeroes_the_dropped_rows_and_nothing_else(B):
    """row_floats 4 (one vector), 24 (less than a wavefront), 160 (train_tinyB's K row), 513 * 64 (no multiple of the workgroup's chunk):
    the whole allocation, sentinels included, is bit-equal to torch.where(drop[:, None], 0, x); an Inf and a NaN in a dropped row read
    back as +0, in a kept row they are untouched."""
    gen = torch.Generator().manual_seed(B)
    for n in (4, 24, 160, 513 * 64):
        x = torch.rand(B, n, generator=gen) + 0.5                    # no zero in the input: every zero in the output was written
        x[0, 1], x[0, n - 1] = float("inf"), float("nan")            # first and last row: dropped in some patterns, kept in others
        x[B - 1, 0], x[B - 1, n - 2] = float("nan"), float("-inf")
        for what, drop in _patterns(B).items():
            rc, got, whole, _ = _op(x, drop)
            assert rc == 0, (n, what)
            d = torch.tensor(drop, dtype=torch.bool)
            want = whole.clone()
            want[SENTINEL:SENTINEL + B * n] = torch.where(d[:, None], torch.zeros(()), x).reshape(-1)
            assert torch.equal(_bits(got), _bits(want)), (n, what)
            body = got[SENTINEL:SENTINEL + B * n].reshape(B, n)
            assert (_bits(body[d]) == 0).all() and torch.equal(_bits(body[~d]), _bits(x[~d])), (n, what)      # +0.0f; Inf / NaN kept where kept
            assert torch.equal(got[:SENTINEL], whole[:SENTINEL]) and torch.equal(got[-SENTINEL:], whole[-SENTINEL:]), (n, what)


def test_operator_refusals_leave_x_untouched():
    from text2protein_amd import _lib
    lib = _lib.load()
    x = torch.rand(3, 24, generator=torch.Generator().manual_seed(8)) + 0.5
    for kw, what in ((dict(row_floats=6), "multiple of 4"), (dict(p=1.5, drop=None), "[0, 1]"), (dict(p=-0.1, drop=None), "[0, 1]"),
                     (dict(batch=0), "arguments"), (dict(row_floats=0), "arguments"), (dict(p=float("nan"), drop=None), "[0, 1]")):
        kw.setdefault("drop", [1, 1, 1])
        rc, got, whole, _ = _op(x, **kw)
        assert rc != 0 and what in lib.t2p_last_error().decode(), (kw, lib.t2p_last_error())
        assert torch.equal(got, whole), kw


# ---- 2. the device draw -------------------------------------------------------------------------------------------------------------------
def test_device_draw_is_the_restated_philox_draw():
    """4096 decisions through drop_out_device, bit-equal to ctxdrop_cases.device_decisions for the three (seed, stream) pairs; the rows
    zeroed are those decisions'; p = 0 drops none, p = 1 all."""
    n = 4096
    x = torch.rand(n, 4, generator=torch.Generator().manual_seed(2)) + 0.5
    for seed, stream in DRAW_PAIRS:
        rc, got, whole, used = _op(x, None, p=0.1, seed=seed, stream_id=stream, want_decisions=True)
        want = torch.from_numpy(device_decisions(seed, stream, n, 0.1))
        print(f"seed {seed}, stream {stream}: {int(used.sum())} of {n} dropped on the device, {int(want.sum())} restated")
        assert rc == 0 and set(used.tolist()) == {0, 1} and torch.equal(used.bool(), want)
        body = got[SENTINEL:SENTINEL + 4 * n].reshape(n, 4)
        assert torch.equal(body, torch.where(want[:, None], torch.zeros(()), x))
    rc, got, whole, used = _op(x, None, p=0.0, seed=11, stream_id=7, want_decisions=True)
    assert rc == 0 and int(used.sum()) == 0 and torch.equal(got, whole)
    rc, got, whole, used = _op(x, None, p=1.0, seed=11, stream_id=7, want_decisions=True)
    assert rc == 0 and int(used.sum()) == n and (got[SENTINEL:SENTINEL + 4 * n] == 0).all()


# ---- 3. the f32 step against the reference fixture ------------------------------------------------------------------------------------------
def test_training_step_vs_reference():
    """ONE fp32 step with samples 0 and 2 dropped against autograd through the reference UNetModel on the context zeroed beforehand:
    loss, score, every gradient, then the parameters, the EMA and both Adam moments, at test_gpu_train.py's tolerances.  The loss pass
    takes explicit decisions; the step goes through get_step_fn(context_dropout=0.5, context_dropout_draw="host") under random.seed(3).
    The update's rel-L2 over whole tensors is reported only, for test_gpu_train_ss.py's reason: Adam's first step moves an element whose
    gradient is within rounding of zero by anything in [-lr, lr], and a dropped sample adds exact zeros to such gradients."""
    g = load_golden(NAME)
    case, cfg, inp, model = _setup()
    batch = _batch(inp)
    context_before = batch["context"].clone()
    base_loss = float(load_golden(case["base"])["loss"])
    assert abs(float(g["loss"]) - base_loss) > 100 * LOSS_TOL * abs(base_loss)      # the fixture tells a step without the dropout apart
    step_fn, _ = _fns(cfg, case, context_dropout=case["p"], context_dropout_draw="host")

    def after(ctx):
        assert torch.equal(batch["context"], context_before) and torch.equal(inp["context"], context_before)

    check_step_against_fixture(NAME, g, case, cfg, inp, model, step_fn, batch, loss_tol=LOSS_TOL, score_tol=1e-5, grad_tol=GRAD_TOL,
                               param_tol=PARAM_TOL, delta_tol=None, before_loss=lambda m: m.set_context_drop(3, drop=DECISIONS),
                               before_step=lambda: random.seed(case["py_seed"]), after=after)


# ---- 4. the drop equals a context zeroed beforehand ------------------------------------------------------------------------------------------
def _pass_and_step(name, dtype, dropped):
    """loss + backward, then one step, on a fresh trainer: with the drop request (dropped=True) or on the context zeroed on the host."""
    from text2protein_amd import losses
    case, cfg, inp, model = _setup(name, dtype)
    batch = _batch(inp)
    if not dropped:
        batch = dict(batch, context=zeroed_context(inp["context"], DECISIONS))
    if dropped:
        model.set_context_drop(3, drop=DECISIONS)
    loss, score = model.loss(batch, t=inp["t"], z=inp["z"], backward=True, return_score=True)
    grads = model.read(losses.GRAD)
    model.set_step(case["step0"])
    if dropped:
        model.set_context_drop(3, drop=DECISIONS)
    loss1 = model.step(batch, t=inp["t"], z=inp["z"])
    return loss, score.cpu(), grads, loss1, _all_state(model)


def test_drop_equals_zeroed_context_f32():
    case, cfg, inp, model = _setup()
    batch = _batch(inp)
    model.set_context_drop(3, drop=DECISIONS)
    l_drop, s_drop = model.loss(batch, t=inp["t"], z=inp["z"], return_score=True)
    l_zero, s_zero = model.loss(dict(batch, context=zeroed_context(inp["context"], DECISIONS)), t=inp["t"], z=inp["z"], return_score=True)
    l_plain, s_plain = model.loss(batch, t=inp["t"], z=inp["z"], return_score=True)
    print(f"f32 losses: dropped {l_drop:.7f}, context zeroed beforehand {l_zero:.7f}, plain {l_plain:.7f}")
    assert abs(l_drop - l_zero) <= 1e-6 * abs(l_zero) and torch.equal(s_drop, s_zero)
    assert torch.equal(s_drop[1], s_plain[1]) and not torch.equal(s_drop[0], s_plain[0]) and not torch.equal(s_drop[2], s_plain[2])


@pytest.mark.parametrize("name,dtype", [(NAME, "f16"), (NAME, "bf16"), ("train_tinyB_vp", "f16")])
def test_drop_equals_zeroed_context_16bit_bitwise(name, dtype):
    """The 16-bit step is the mode in which two identical steps are bitwise equal at all (fixed-order reductions): the loss, the score,
    every gradient and all post-step state of a step with the request equal those of a step on the zeroed context."""
    a = _pass_and_step(name, dtype, True)
    b = _pass_and_step(name, dtype, False)
    print(f"{name} {dtype}: loss {a[0]:.7f} / {b[0]:.7f}, step loss {a[3]:.7f} / {b[3]:.7f}")
    assert a[0] == b[0] and a[3] == b[3] and torch.equal(a[1], b[1])
    for n in a[2]:
        assert torch.equal(a[2][n], b[2][n]), n
    _assert_same_state(a[4], b[4])


# ---- 5. all dropped; nothing dropped ----------------------------------------------------------------------------------------------------------
def test_all_dropped_leaves_the_context_projections_alone():
    """to_k and to_v of every cross-attention see only zeros: their gradients are exactly 0, and after the step the parameters, their EMA
    and both moments are bitwise what they were."""
    from text2protein_amd import losses
    case, cfg, inp, model = _setup()
    names = [n for n, _ in model.param_table() if n.endswith("attn2.to_k.weight") or n.endswith("attn2.to_v.weight")]
    assert len(names) >= 4
    before = _all_state(model)
    model.set_step(case["step0"])
    model.set_context_drop(3, drop=[1, 1, 1])
    model.step(_batch(inp), t=inp["t"], z=inp["z"])
    after = _all_state(model)
    for n in names:
        assert int((_bits(after[losses.GRAD][n]) & 0x7FFFFFFF).ne(0).sum()) == 0, n
        for w in (losses.PARAM, losses.EMA, losses.EXP_AVG, losses.EXP_AVG_SQ):
            assert torch.equal(_bits(before[w][n]), _bits(after[w][n])), (w, n)
    moved = [n for n in after[losses.PARAM] if not torch.equal(after[losses.PARAM][n], before[losses.PARAM][n])]
    assert len(moved) > len(after[losses.PARAM]) // 2 and not set(moved) & set(names)          # the step itself happened


def test_step_without_a_request_is_the_step_as_it_was():
    """drop = [0, 0, 0], a request set and cleared again, and a trainer that never heard of the feature: bitwise-equal f16 steps."""
    runs = []
    for how in ("never", "none dropped", "cleared"):
        case, cfg, inp, model = _setup(dtype="f16")
        if how == "none dropped":
            model.set_context_drop(3, drop=[0, 0, 0])
        elif how == "cleared":
            model.set_context_drop(3, drop=DECISIONS)
            model.set_context_drop(0)
        model.set_step(case["step0"])
        loss = model.step(_batch(inp), t=inp["t"], z=inp["z"])
        runs.append((loss, _all_state(model), model.get_step()))
        del model
    for other in runs[1:]:
        assert other[0] == runs[0][0] and other[2] == runs[0][2]
        _assert_same_state(runs[0][1], other[1])


# ---- 6. consumed by one pass ------------------------------------------------------------------------------------------------------------------
def test_request_is_consumed_by_one_pass_and_eval_honours_it():
    g, base = load_golden(NAME), load_golden("train_tinyB")
    case, cfg, inp, model = _setup()
    batch = _batch(inp)
    zeroed = dict(batch, context=zeroed_context(inp["context"], DECISIONS))
    model.set_context_drop(3, drop=DECISIONS)
    l1 = model.loss(batch, t=inp["t"], z=inp["z"])
    l2 = model.loss(batch, t=inp["t"], z=inp["z"])
    print(f"losses: with the request {l1:.6f} (fixture {float(g['loss']):.6f}), next pass {l2:.6f} (train_tinyB {float(base['loss']):.6f})")
    assert abs(l1 - float(g["loss"])) <= LOSS_TOL * abs(float(g["loss"]))
    assert abs(l2 - float(base["loss"])) <= LOSS_TOL * abs(float(base["loss"])) and l1 != l2
    e_plain = model.eval_loss(batch, t=inp["t"], z=inp["z"])
    model.set_context_drop(3, drop=DECISIONS)
    e_drop = model.eval_loss(batch, t=inp["t"], z=inp["z"])
    e_after = model.eval_loss(batch, t=inp["t"], z=inp["z"])
    e_pre = model.eval_loss(zeroed, t=inp["t"], z=inp["z"])
    print(f"eval_loss: plain {e_plain:.6f}, with the request {e_drop:.6f}, after it {e_after:.6f}, context zeroed beforehand {e_pre:.6f}")
    assert abs(e_drop - e_pre) <= 1e-6 * abs(e_pre) and abs(e_after - e_plain) <= 1e-6 * abs(e_plain)
    assert abs(e_drop - e_plain) > 1e-6 * abs(e_plain)                  # beyond the tolerance of the two equalities: it differs
    # train=False never drops: the evaluation loss stays the conditional one
    _, eval_fn = _fns(cfg, case, context_dropout=1.0)
    e_fn = eval_fn(_state(model, cfg, case["step0"]), batch, condition=cfg.model.condition, t=inp["t"], z=inp["z"])
    assert abs(e_fn - e_plain) <= 1e-6 * abs(e_plain)


# ---- 7. refusals ------------------------------------------------------------------------------------------------------------------------------
def test_request_of_another_batch_size_fails_the_pass_and_changes_nothing():
    from text2protein_amd._lib import T2PError
    base = load_golden("train_tinyB")
    case, cfg, inp, model = _setup()
    batch = _batch(inp)
    model.loss(batch, t=inp["t"], z=inp["z"], backward=True)          # a gradient buffer worth keeping
    model.set_step(case["step0"], 3, 3)
    before, steps = _all_state(model), model.get_step()
    step_fn, _ = _fns(cfg, case)
    state = _state(model, cfg, case["step0"])
    model.set_context_drop(2, drop=[1, 0])
    with pytest.raises(T2PError, match="context dropout: the request holds 2 samples, the batch 3"):
        step_fn(state, batch, condition=cfg.model.condition, t=inp["t"], z=inp["z"])
    _assert_same_state(before, _all_state(model))
    assert model.get_step() == steps and state["step"] == case["step0"]
    loss = model.loss(batch, t=inp["t"], z=inp["z"])                  # the request is cleared
    assert abs(loss - float(base["loss"])) <= LOSS_TOL * abs(float(base["loss"]))


def test_setter_refusals_keep_the_stored_request():
    from text2protein_amd._lib import T2PError
    g = load_golden(NAME)
    case, cfg, inp, model = _setup()
    model.set_context_drop(3, drop=DECISIONS)
    for args, kw, what in (((3,), dict(p=1.5), r"\[0, 1\]"), ((3,), dict(p=-0.1), r"\[0, 1\]"), ((3,), dict(p=float("nan")), r"\[0, 1\]"),
                           ((3,), dict(drop=[1, 0]), "decisions"), ((3,), dict(drop=[1, 0, 1, 1]), "decisions"), ((-3,), dict(), "negative")):
        with pytest.raises(T2PError, match=what):
            model.set_context_drop(*args, **kw)
    loss = model.loss(_batch(inp), t=inp["t"], z=inp["z"])
    assert abs(loss - float(g["loss"])) <= LOSS_TOL * abs(float(g["loss"]))


# ---- 8. through get_step_fn with the device draw ------------------------------------------------------------------------------------------------
def _steps16(seed, n_steps, kw=None, explicit=None):
    """n_steps f16 steps on a fresh trainer seeded ``seed``: through get_step_fn(**kw), or with explicit decisions per step."""
    case, cfg, inp, model = _setup(dtype="f16", seed=seed)
    step_fn, _ = _fns(cfg, case, **(kw or {}))
    state = _state(model, cfg, case["step0"])
    losses_ = []
    for i in range(n_steps):
        if explicit is not None:
            model.set_context_drop(3, drop=explicit[i])
        losses_.append(step_fn(state, _batch(inp), condition=cfg.model.condition, t=inp["t"], z=inp["z"]))
    return losses_, _all_state(model)


def test_step_fn_device_draw_at_one_and_zero():
    """p = 1 equals the explicit all-dropped step, p = 0 equals the plain step (f16: bitwise)."""
    one = _steps16(11, 1, dict(context_dropout=1.0, context_dropout_draw="device"))
    every = _steps16(11, 1, explicit=[[1, 1, 1]])
    zero = _steps16(11, 1, dict(context_dropout=0.0, context_dropout_draw="device"))
    plain = _steps16(11, 1)
    print(f"p = 1: {one[0][0]:.7f} (explicit {every[0][0]:.7f}); p = 0: {zero[0][0]:.7f} (plain {plain[0][0]:.7f})")
    assert one[0] == every[0] and zero[0] == plain[0] and one[0] != plain[0]
    _assert_same_state(one[1], every[1])
    _assert_same_state(zero[1], plain[1])


def test_step_fn_device_draw_uses_the_restated_decisions():
    """Two steps at p = 0.5 on a trainer seeded 12: the decisions of loss call c are device_decisions(12, 4096 c + 4, 3, 0.5) -- the
    same steps with those decisions given explicitly are bitwise equal (f16), the same seed gives the same losses again, and the steps
    with the other call's decisions do not."""
    seed, p = 12, 0.5
    want = [device_decisions(seed, 4096 * c + 4, 3, p).astype(int).tolist() for c in range(2)]
    print("restated decisions of calls 0 and 1:", want)
    assert all(0 < sum(d) < 3 for d in want) and want[0] != want[1]           # mixed, and the call index matters
    a = _steps16(seed, 2, dict(context_dropout=p, context_dropout_draw="device"))
    b = _steps16(seed, 2, dict(context_dropout=p, context_dropout_draw="device"))
    given = _steps16(seed, 2, explicit=want)
    swapped = _steps16(seed, 2, explicit=want[::-1])
    assert a[0] == b[0] == given[0] and a[0][0] != swapped[0][0]
    _assert_same_state(a[1], b[1])
    _assert_same_state(a[1], given[1])
