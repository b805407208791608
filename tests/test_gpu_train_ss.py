"""Secondary-structure block dropout on the GPU: the operator (t2p_op_ss_block_dropout), the trainer's block list
(t2p_train_set_ss_blocks) and the Python mirror (HipTrainModel.set_ss_blocks, get_step_fn with batch["ss_indices"]).

Oracle: tests/golden/train_tinyB_ssdrop.npz / train_tinyB_ssdrop_vp.npz -- the reference's own ``block_dropout`` (losses.py:54-64) under a
recorded ``random.seed``, then autograd through the reference UNetModel on the dropped coordinates
(tests/golden/make_golden_train_ss.py).  Architecture and inputs are train_tinyB's and only zeros differ, so the fp32 tolerances are
test_gpu_train.py's own; the 16-bit bounds are about twice the values measured against the fp32 fixture.
"""
import ctypes as C
import random

import numpy as np
import pytest
import torch

from helpers import TRAIN_CASES, check_step_against_fixture, load_golden, projection, rel_l2, train_inputs
from sde_train_cases import make_sde
from ss_train_cases import BLOCK_DROPOUT, SS_TRAIN_CASES, dropped_coords, ss_record
from test_gpu_train import GRAD_TOL, LOSS_TOL, PARAM_TOL
from test_gpu_train_sde import _all_state, _batch, _masks, _model, _state

pytestmark = pytest.mark.gpu

# 16-bit step on train_tinyB_ssdrop against the fp32 reference fixture: about 2x the measured values ("Block
# dropout": measured on an MI355X; the 16-bit step is bitwise reproducible, so the figures do not move from run to run)
STEP16_TOL = {
    "f16": dict(loss=2.4e-4, score=7.8e-3, grad_norm=2.6e-2, grad_proj=5.8e-2, grad=5.2e-2, post=3.6e-4, post_norm=1.3e-3),
    "bf16": dict(loss=2e-4, score=4.6e-2, grad_norm=0.22, grad_proj=0.42, grad=0.44, post=4e-3, post_norm=3.2e-3),
}


def _setup(name, dtype="f32"):
    case = SS_TRAIN_CASES[name]
    cfg = case["config"]()
    inp = train_inputs(cfg, case)
    model = _model(case, cfg, dtype)
    model.set_dropout_masks(_masks(case, cfg, model))
    return case, cfg, inp, model


def _fns(cfg, case, **kw):
    from text2protein_amd import losses, sde_lib
    sde = make_sde(sde_lib, cfg, case)
    return (sde, losses.get_step_fn(sde, train=True, optimize_fn=losses.optimization_manager(cfg), **kw),
            losses.get_step_fn(sde, train=False, **kw))


def _op(x, blocks, drop=None, p=BLOCK_DROPOUT, seed=0, stream_id=0, out=None, drop_out=None, C_=None):
    """t2p_op_ss_block_dropout; returns (status, out)."""
    from text2protein_amd import _lib
    lib = _lib.load()
    B, Cx, L = x.shape[0], x.shape[1], x.shape[2]
    if out is None:
        out = torch.empty_like(x)
    arr = np.ascontiguousarray(np.asarray(blocks, dtype=np.int32).reshape(-1, 3))
    d = None if drop is None else np.ascontiguousarray(np.asarray(drop, dtype=np.uint8))
    rc = lib.t2p_op_ss_block_dropout(_lib.ptr(x), _lib.ptr(out), B, Cx if C_ is None else C_, L, C.c_void_p(arr.ctypes.data) if len(arr) else None,
                                     len(arr), None if d is None else C.c_void_p(d.ctypes.data), float(p), seed, stream_id, _lib.ptr(drop_out),
                                     _lib.stream_ptr())
    torch.cuda.synchronize()
    return rc, out


def _torch_dropout(x, blocks, drop):
    """block_dropout's two assignments (losses.py:61-62) for the dropped blocks, on a clone."""
    y = x.clone()
    for (b, start, end), d in zip(blocks, drop):
        if d:
            y[b, 4:7, :, start:end] = 0
            y[b, 4:7, start:end, :] = 0
    return y


# ---- 1. the operator ----------------------------------------------------------------------------------------------------------------------
def test_operator_reproduces_the_reference_block_dropout():
    """B = 3, C = 8, L = 16, the fixture's blocks and decisions: bit-equal to what the reference's block_dropout returned, out of place
    (x untouched) and in place."""
    rec = ss_record(load_golden("train_tinyB_ssdrop"))
    case = SS_TRAIN_CASES["train_tinyB_ssdrop"]
    x_host = train_inputs(case["config"](), case)["coords_6d"]
    assert tuple(x_host.shape) == (3, 8, 16, 16)
    want = dropped_coords(x_host, rec)                    # the reference's tensor, rebuilt and checked against the fixture's SHA-256
    x = x_host.cuda()
    rc, out = _op(x, rec["blocks"], rec["decisions"])
    assert rc == 0 and torch.equal(out.cpu(), want)
    assert torch.equal(x.cpu(), x_host) and not torch.equal(out.cpu(), x_host)
    rc, same = _op(x, rec["blocks"], rec["decisions"], out=x)
    assert rc == 0 and same is x and torch.equal(x.cpu(), want)


def test_operator_edges():
    """B = 2, C = 8, L = 20: Python slice semantics (end clamped, start >= end empty, overlaps), a whole-axis block, the untouched
    channels, and the refusals."""
    from text2protein_amd import _lib
    lib = _lib.load()
    B, Cx, L = 2, 8, 20
    gen = torch.Generator().manual_seed(3)
    x_host = torch.rand(B, Cx, L, L, generator=gen) + 0.5          # no zero in the input: every zero in the output was written
    x = x_host.cuda()
    cases = {
        "end past L": [(0, 15, 27)],
        "start == end": [(1, 5, 5)],
        "start > end": [(1, 9, 4)],
        "start past L": [(0, 25, 30)],
        "overlapping": [(1, 2, 8), (1, 6, 11)],
        "whole axis": [(0, 0, L)],
        "kept and dropped": [(0, 1, 3), (0, 4, 9), (1, 0, 20), (1, 3, 4)],
        "none": [],
    }
    for what, blocks in cases.items():
        drop = [1] * len(blocks) if what != "kept and dropped" else [0, 1, 0, 1]
        rc, out = _op(x, blocks, drop)
        assert rc == 0, (what, lib.t2p_last_error())
        got = out.cpu()
        assert torch.equal(got, _torch_dropout(x_host, blocks, drop)), what
        assert torch.equal(got[:, :4], x_host[:, :4]) and torch.equal(got[:, 7], x_host[:, 7]), what
        if what in ("start == end", "start > end", "start past L", "none"):
            assert torch.equal(got, x_host), what
        if what == "end past L":
            assert (got[0, 4:7, 15:, :] == 0).all() and (got[0, 4:7, :, 15:] == 0).all() and torch.equal(got[0, 4:7, :15, :15], x_host[0, 4:7, :15, :15])
        if what == "whole axis":
            assert (got[0, 4:7] == 0).all() and torch.equal(got[1], x_host[1])
    assert torch.equal(x.cpu(), x_host)
    # refusals: nothing is written
    out = torch.full_like(x, 7.0)
    x5 = x[:, :5].contiguous()
    for args, kw, what in (((x5, [(0, 1, 3)], [1]), dict(out=out[:, :5].contiguous()), "C >= 7"),
                           ((x, [(0, -2, 3)], [1]), dict(out=out), "negative"), ((x, [(0, 2, -1)], [1]), dict(out=out), "negative"),
                           ((x, [(-1, 2, 3)], [1]), dict(out=out), "outside the batch"), ((x, [(B, 2, 3)], [1]), dict(out=out), "outside the batch"),
                           ((x, [(0, 2, 3)], None), dict(out=out, p=1.5), "[0, 1]"), ((x, [(0, 2, 3)], None), dict(out=out, p=-0.1), "[0, 1]")):
        rc, _ = _op(*args, **kw)
        assert rc != 0 and what in lib.t2p_last_error().decode(), (what, lib.t2p_last_error())
    assert (out == 7.0).all()


def test_operator_device_draws():
    """4096 blocks drawn on the device at p = 0.2: the same (seed, stream) gives the same decisions, another stream other ones; the
    dropped fraction lies within 0.2 +- 0.025 (derived: the binomial sd is sqrt(0.2 0.8 / 4096) = 0.00625, the bound is 4 sd); p = 0
    drops none, p = 1 all; and the output is the zeroing by the decisions reported."""
    n, L = 4096, 16
    gen = torch.Generator().manual_seed(4)
    x_host = torch.rand(1, 8, L, L, generator=gen) + 0.5
    x = x_host.cuda()
    blocks = [(0, k % L, k % L + 1) for k in range(n)]

    def draw(p, seed, stream_id):
        d = torch.full((n,), 9, dtype=torch.uint8, device="cuda")
        rc, out = _op(x, blocks, None, p=p, seed=seed, stream_id=stream_id, drop_out=d)
        assert rc == 0
        return d.cpu(), out.cpu()

    d0, out0 = draw(0.2, 11, 4096 * 5 + 2)
    d1, _ = draw(0.2, 11, 4096 * 5 + 2)
    d2, _ = draw(0.2, 11, 4096 * 6 + 2)
    d3, _ = draw(0.2, 12, 4096 * 5 + 2)
    assert set(d0.tolist()) == {0, 1}
    assert torch.equal(d0, d1) and not torch.equal(d0, d2) and not torch.equal(d0, d3)
    frac = float(d0.float().mean())
    print(f"device draws: {int(d0.sum())} of {n} blocks dropped at p = 0.2 ({frac:.4f})")
    assert abs(frac - 0.2) <= 0.025
    assert torch.equal(out0, _torch_dropout(x_host, blocks, d0.tolist()))
    none, out_none = draw(0.0, 11, 7)
    every, out_all = draw(1.0, 11, 7)
    assert int(none.sum()) == 0 and torch.equal(out_none, x_host)
    assert int(every.sum()) == n and (out_all[0, 4:7] == 0).all()


# ---- 2. the training step against the reference, f32 ----------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(SS_TRAIN_CASES))
def test_training_step_vs_reference(name):
    """ONE fp32 step with the fixture's blocks and decisions against autograd through the reference UNetModel on the coordinates the
    reference's block_dropout produced: loss, every gradient, then the parameters, the EMA and both Adam moments after the update, at
    test_gpu_train.py's tolerances.  The step itself goes through get_step_fn with batch["ss_indices"] under the fixture's random.seed."""
    g = load_golden(name)
    case, cfg, inp, model = _setup(name)
    assert "t" not in g or np.array_equal(inp["t"].numpy(), g["t"])
    sde, step_fn, _ = _fns(cfg, case)
    model.set_sde(sde)
    check_ss_step_against_fixture(name, g, case, cfg, inp, model, step_fn)


def check_ss_step_against_fixture(name, g, case, cfg, inp, model, step_fn, label=None):
    """helpers.check_step_against_fixture for a block-dropout fixture, with what only these fixtures need: the fixture's blocks and
    decisions for the loss, the strings and the reference's own draws (random.seed) for the step through the Python mirror; the fixture
    tells a step without the dropout apart; the caller's coords_6d is not modified; the update element by element where it is determined."""
    rec = ss_record(g)
    batch = _batch(inp)
    coords_before = batch["coords_6d"].clone()
    base_loss = float(load_golden(case["base"])["loss"])
    assert abs(float(g["loss"]) - base_loss) > 100 * LOSS_TOL * abs(base_loss)      # the fixture tells a step without the dropout apart

    def update_where_determined(ctx):
        # The update itself.  Its rel-L2 over a whole tensor is only reported (measured 5.8e-3 VE / 6.3e-3 VP, on tensors with elements whose
        # gradient is within rounding of zero: Adam's first step moves an element by lr g / (|g| + eps), so such an element may land
        # anywhere between -lr and +lr on either side and no gradient tolerance bounds the difference).  Asserted is the update of every
        # element whose gradient is FAR from zero, where it is determined: with c = the clipping factor and |c g| >= 1000 eps the step is
        # sign(g) lr to within 1e-3 lr, and an element with |g| > 2 GRAD_TOL ||g|| cannot have another sign here than in the reference (the
        # element error is at most the tensor's, asserted above).  Bound: 2e-3 lr + 4 ulp of the parameter.
        assert torch.equal(batch["coords_6d"], coords_before)                 # the caller's coords_6d is not modified
        post, sd, T = ctx["post"], ctx["sd"], ctx["T"]
        lr = cfg.optim.lr * min(case["step0"] / cfg.optim.warmup, 1.0)
        clip = min(1.0, cfg.optim.grad_clip / (T + 1e-6)) if cfg.optim.grad_clip >= 0 else 1.0
        assert cfg.optim.weight_decay == 0 and cfg.optim.eps == 1e-8
        checked = 0
        for n in ctx["full"]:
            gref = torch.from_numpy(g["grad:" + n]).double()
            sel = (gref.abs() > 2 * GRAD_TOL * float(gref.norm())) & (gref.abs() * clip >= 1000 * cfg.optim.eps)
            got_d, ref_d = (post["post"][n] - sd[n])[sel], (torch.from_numpy(g["post:" + n]) - sd[n])[sel]
            bound = 2e-3 * lr + 4 * 6e-8 * sd[n][sel].abs()
            assert ((got_d - ref_d).abs() <= bound).all(), (n, float((got_d - ref_d).abs().max()), lr)
            assert ((got_d + lr * torch.sign(gref[sel]).float()).abs() <= bound).all(), n       # and it is -lr sign(g)
            checked += int(sel.sum())
        print(f"{name}: loss without block dropout {base_loss:.6f}; update checked element by element on {checked} elements with a gradient far "
              f"from zero (lr {lr:.1e}, clip factor {clip:.3g})")
        assert checked > 1000

    return check_step_against_fixture(label or name, g, case, cfg, inp, model, step_fn, batch, loss_tol=LOSS_TOL, score_tol=1e-5,
                                      grad_tol=GRAD_TOL, param_tol=PARAM_TOL, delta_tol=None,
                                      before_loss=lambda m: m.set_ss_blocks(rec["blocks"], drop=rec["decisions"]),
                                      before_step=lambda: random.seed(case["py_seed"]),
                                      step_batch=dict(batch, ss_indices=case["ss_indices"]), after=update_where_determined)


# ---- 3. f16 / bf16 ----------------------------------------------------------------------------------------------------------------------
def _step16(dt):
    from text2protein_amd import losses
    name = "train_tinyB_ssdrop"
    g = load_golden(name)
    rec = ss_record(g)
    case, cfg, inp, model = _setup(name, dt)
    batch = _batch(inp)
    sde, step_fn, _ = _fns(cfg, case)
    model.set_sde(sde)
    model.set_ss_blocks(rec["blocks"], drop=rec["decisions"])
    loss0, score = model.loss(batch, t=inp["t"], z=inp["z"], backward=True, return_score=True)
    grads = model.read(losses.GRAD)
    state = _state(model, cfg, case["step0"])
    random.seed(case["py_seed"])
    loss1 = step_fn(state, dict(batch, ss_indices=case["ss_indices"]), condition=cfg.model.condition, t=inp["t"], z=inp["z"])
    assert abs(loss1 - loss0) <= 1e-6 * abs(loss0) and model.get_step() == (case["step0"] + 1, 1, 1)
    return g, loss0, score.cpu(), grads, _all_state(model)


@pytest.mark.parametrize("dt", ["f16", "bf16"])
def test_training_step16_vs_reference(dt):
    """ONE 16-bit step with block dropout against the fp32 reference fixture, in the assertion forms of test_gpu_train16; a second run
    from a fresh trainer is bitwise equal in the gradients and in all post-step state."""
    from text2protein_amd import losses
    g, loss0, score, grads, state = _step16(dt)
    names = [str(n) for n in g["names"]]
    tol = STEP16_TOL[dt]
    e_score = rel_l2(score, g["score"])
    e_loss = abs(loss0 - float(g["loss"])) / abs(float(g["loss"]))
    T = float(g["grad_total_norm"])
    pcache = {}
    e_norm = e_proj = 0.0
    for i, n in enumerate(names):
        scale = max(float(g["grads_norm"][i]), 1e-3 * T, 1e-30)
        e_norm = max(e_norm, abs(float(grads[n].double().norm()) - float(g["grads_norm"][i])) / scale)
        e_proj = max(e_proj, abs(projection(n, grads[n], cache=pcache) - float(g["grads_proj"][i])) / scale)
    full = [k[5:] for k in g if k.startswith("grad:")]
    e_grad, worst_n = max((rel_l2(grads[n], g["grad:" + n]), n) for n in full)
    post, ema = state[losses.PARAM], state[losses.EMA]
    e_post = max(rel_l2(post[n], g["post:" + n]) for n in full)
    e_post_norm = 0.0
    for key, got in (("post", post), ("ema", ema)):
        for i, n in enumerate(names):
            e_post_norm = max(e_post_norm, abs(float(got[n].double().norm()) - float(g[key + "_norm"][i])) / max(float(g[key + "_norm"][i]), 1e-30))
    print(f"{dt} train_tinyB_ssdrop: loss rel {e_loss:.1e}, score rel-L2 {e_score:.1e}, gradient norm {e_norm:.1e} / projection {e_proj:.1e} "
          f"(of max(norm, 1e-3 total)), stored gradients rel-L2 {e_grad:.1e} over {len(full)} tensors ({worst_n}), post-step parameters rel-L2 "
          f"{e_post:.1e}, post-step parameter / EMA norms {e_post_norm:.1e}")
    assert e_loss < tol["loss"] and e_score < tol["score"]
    assert e_norm < tol["grad_norm"] and e_proj < tol["grad_proj"] and e_grad < tol["grad"]
    assert e_post < tol["post"] and e_post_norm < tol["post_norm"]
    _, loss_b, score_b, grads_b, state_b = _step16(dt)
    assert abs(loss_b - loss0) <= 1e-6 * abs(loss0) and torch.equal(score, score_b)      # (the scalar loss sums with double atomics)
    for n in grads:
        assert torch.equal(grads[n], grads_b[n]), n
    for w in (losses.PARAM, losses.EMA, losses.EXP_AVG, losses.EXP_AVG_SQ):
        for n in state[w]:
            assert torch.equal(state[w][n], state_b[w][n]), (w, n)


# ---- 4. behaviour around the list ------------------------------------------------------------------------------------------------------------
def test_block_list_is_consumed_by_one_pass():
    """The pass after set_ss_blocks computes the fixture's loss; the next pass on the same trainer, without a new list, computes
    train_tinyB's own.  The block list gives what the same pass gives on coordinates zeroed beforehand."""
    g = load_golden("train_tinyB_ssdrop")
    rec = ss_record(g)
    base = load_golden("train_tinyB")
    case, cfg, inp, model = _setup("train_tinyB_ssdrop")
    batch = _batch(inp)
    model.set_ss_blocks(rec["blocks"], drop=rec["decisions"])
    l1, s1 = model.loss(batch, t=inp["t"], z=inp["z"], return_score=True)
    l2 = model.loss(batch, t=inp["t"], z=inp["z"])
    l3, s3 = model.loss(dict(batch, coords_6d=dropped_coords(inp["coords_6d"], rec)), t=inp["t"], z=inp["z"], return_score=True)
    print(f"losses: with the list {l1:.6f}, next pass {l2:.6f}, coordinates zeroed beforehand {l3:.6f}")
    assert abs(l1 - float(g["loss"])) <= LOSS_TOL * abs(float(g["loss"]))
    assert abs(l2 - float(base["loss"])) <= LOSS_TOL * abs(float(base["loss"])) and l1 != l2
    assert abs(l3 - l1) <= 1e-6 * abs(l1) and torch.equal(s1, s3)


def test_step_without_blocks_equals_step_with_an_empty_list():
    """A step on a trainer that never heard of blocks and one after set_ss_blocks([]) -- and one after a list was set and cleared again:
    bitwise equal in the loss, every parameter, the EMA and both moments.  Run in f16, the mode in which two identical steps are bitwise
    equal at all (fixed-order reductions; the f32 step sums its weight gradients with atomics)."""
    g = load_golden("train_tinyB_ssdrop")
    rec = ss_record(g)
    runs = []
    for how in ("never", "empty", "cleared"):
        case, cfg, inp, model = _setup("train_tinyB_ssdrop", "f16")
        if how == "empty":
            model.set_ss_blocks([])
        elif how == "cleared":
            model.set_ss_blocks(rec["blocks"], drop=rec["decisions"])
            model.set_ss_blocks([], drop=[])
        model.set_step(case["step0"])
        loss = model.step(_batch(inp), t=inp["t"], z=inp["z"])
        runs.append((loss, _all_state(model), model.get_step()))
        del model
    for other in runs[1:]:
        assert other[0] == runs[0][0] and other[2] == runs[0][2]
        for w in runs[0][1]:
            for n in runs[0][1][w]:
                assert torch.equal(runs[0][1][w][n], other[1][w][n]), (w, n)


def test_eval_loss_takes_the_blocks():
    """The reference applies block_dropout with train=False too: eval_loss (the EMA weights, dropout off) after set_ss_blocks equals
    eval_loss on coordinates zeroed beforehand, differs from eval_loss without the list, and consumes the list."""
    g = load_golden("train_tinyB_ssdrop")
    rec = ss_record(g)
    case, cfg, inp, model = _setup("train_tinyB_ssdrop")
    batch = _batch(inp)
    e_plain = model.eval_loss(batch, t=inp["t"], z=inp["z"])
    model.set_ss_blocks(rec["blocks"], drop=rec["decisions"])
    e_drop = model.eval_loss(batch, t=inp["t"], z=inp["z"])
    e_after = model.eval_loss(batch, t=inp["t"], z=inp["z"])
    e_pre = model.eval_loss(dict(batch, coords_6d=dropped_coords(inp["coords_6d"], rec)), t=inp["t"], z=inp["z"])
    print(f"eval_loss: plain {e_plain:.6f}, with the list {e_drop:.6f}, after it {e_after:.6f}, coordinates zeroed beforehand {e_pre:.6f}")
    assert abs(e_drop - e_pre) <= 1e-6 * abs(e_pre) and abs(e_after - e_plain) <= 1e-6 * abs(e_plain)
    assert abs(e_drop - e_plain) > 100 * LOSS_TOL * abs(e_plain)
    # through the step function with train=False
    _, _, eval_fn = _fns(cfg, case)
    random.seed(case["py_seed"])
    e_fn = eval_fn(_state(model, cfg, case["step0"]), dict(batch, ss_indices=case["ss_indices"]), condition=cfg.model.condition, t=inp["t"],
                   z=inp["z"])
    assert abs(e_fn - e_drop) <= 1e-6 * abs(e_drop)


# ---- 5. refusals --------------------------------------------------------------------------------------------------------------------------
def test_setter_refusals_change_nothing():
    from text2protein_amd._lib import T2PError
    g = load_golden("train_tinyB_ssdrop")
    rec = ss_record(g)
    # a trainer without the ss flag
    plain_case = TRAIN_CASES["train_tiny"]
    plain_cfg = plain_case["config"]()
    assert "ss" not in plain_cfg.model.condition
    plain = _model(plain_case, plain_cfg)
    with pytest.raises(T2PError, match="ss condition"):
        plain.set_ss_blocks([(0, 1, 3)], drop=[1])
    plain.set_ss_blocks([])                                           # clearing is always allowed
    pin = train_inputs(plain_cfg, plain_case)
    fresh = _model(plain_case, plain_cfg)
    assert plain.loss(_batch(pin), t=pin["t"], z=pin["z"]) == fresh.loss(_batch(pin), t=pin["t"], z=pin["z"])
    # bad arguments on a trainer with the flag: the list set before them stays as it was
    case, cfg, inp, model = _setup("train_tinyB_ssdrop")
    model.set_ss_blocks(rec["blocks"], drop=rec["decisions"])
    for blocks, kw, what in (([(0, 1, 3)], dict(p=1.01), r"\[0, 1\]"), ([(0, 1, 3)], dict(p=-0.5), r"\[0, 1\]"),
                             ([(0, -1, 3)], dict(drop=[1]), "negative"), ([(0, 1, -3)], dict(drop=[1]), "negative"),
                             ([(0, 1, 3), (-1, 1, 3)], dict(drop=[1, 1]), "negative sample"), ([(0, 1, 3)], dict(drop=[1, 0]), "decisions")):
        with pytest.raises(T2PError, match=what):
            model.set_ss_blocks(blocks, **kw)
    loss = model.loss(_batch(inp), t=inp["t"], z=inp["z"])
    assert abs(loss - float(g["loss"])) <= LOSS_TOL * abs(float(g["loss"]))


def test_sample_outside_the_batch_fails_the_pass_and_changes_nothing():
    """sample >= batch is detected at the pass: the step raises, parameters, gradients, moments, EMA and counters are what they were, the
    list is cleared (the next pass computes train_tinyB's loss)."""
    from text2protein_amd import losses
    from text2protein_amd._lib import T2PError
    base = load_golden("train_tinyB")
    case, cfg, inp, model = _setup("train_tinyB_ssdrop")
    batch = _batch(inp)
    model.loss(batch, t=inp["t"], z=inp["z"], backward=True)          # a gradient buffer worth keeping
    model.set_step(case["step0"], 3, 3)
    before, steps = _all_state(model), model.get_step()
    _, step_fn, _ = _fns(cfg, case)
    state = _state(model, cfg, case["step0"])
    model.set_ss_blocks([(0, 1, 3), (case["B"], 2, 5)], drop=[1, 1])
    with pytest.raises(T2PError, match="sample index"):
        step_fn(state, batch, condition=cfg.model.condition, t=inp["t"], z=inp["z"])
    after = _all_state(model)
    for w in before:
        for n in before[w]:
            assert torch.equal(before[w][n], after[w][n]), (w, n)
    assert model.get_step() == steps and state["step"] == case["step0"]
    loss = model.loss(batch, t=inp["t"], z=inp["z"])
    assert abs(loss - float(base["loss"])) <= LOSS_TOL * abs(float(base["loss"]))
    # the Python mirror refuses a batch whose ss_indices has another length before any native call
    with pytest.raises(T2PError, match="3 samples"):
        step_fn(state, dict(batch, ss_indices=["1:2"]), condition=cfg.model.condition, t=inp["t"], z=inp["z"])
    with pytest.raises(T2PError, match="two integers"):
        step_fn(state, dict(batch, ss_indices=["1:2", "x", ""]), condition=cfg.model.condition, t=inp["t"], z=inp["z"])
    assert model.get_step() == steps and state["step"] == case["step0"]
    assert all(torch.equal(before[losses.PARAM][n], v) for n, v in model.read(losses.PARAM).items())


# ---- 6. through get_step_fn -----------------------------------------------------------------------------------------------------------------
def test_step_fn_draws_on_the_device():
    """block_dropout_draw="device": reproducible for a fixed trainer seed and call index, p = 1 equals the explicit all-dropped list and
    differs from the loss without dropout, p = 0 equals the loss without dropout; a batch without ss_indices has nothing dropped."""
    base = load_golden("train_tinyB")
    out = {}
    for key, kw in (("a", dict(block_dropout=0.5, block_dropout_draw="device")), ("b", dict(block_dropout=0.5, block_dropout_draw="device")),
                    ("one", dict(block_dropout=1.0, block_dropout_draw="device")), ("zero", dict(block_dropout=0.0, block_dropout_draw="device")),
                    ("host_one", dict(block_dropout=1.0)), ("absent", dict(block_dropout=1.0, block_dropout_draw="device"))):
        case, cfg, inp, model = _setup("train_tinyB_ssdrop")
        _, step_fn, _ = _fns(cfg, case, **kw)
        batch = _batch(inp) if key == "absent" else dict(_batch(inp), ss_indices=case["ss_indices"])
        state = _state(model, cfg, case["step0"])
        out[key] = step_fn(state, batch, condition=cfg.model.condition, t=inp["t"], z=inp["z"])
        del model
    print("device-drawn block dropout:", {k: round(v, 6) for k, v in out.items()}, f"(train_tinyB: {float(base['loss']):.6f})")
    b = float(base["loss"])
    assert abs(out["a"] - out["b"]) <= 1e-6 * abs(out["a"])
    assert abs(out["one"] - out["host_one"]) <= 1e-6 * abs(out["one"]) and abs(out["one"] - b) > 100 * LOSS_TOL * b
    assert abs(out["zero"] - b) <= LOSS_TOL * b and abs(out["absent"] - b) <= LOSS_TOL * b
