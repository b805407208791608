"""The 16-bit training step's plumbing on exact products (plan switch 48, tools/README.md).

A trainer created while the switch is set uses everything the f16 / bf16 step uses except the products: the fixed-order reductions
(GroupNorm / LayerNorm parameter gradients, bias column sums, the gradient norm), the scaled backward seed (the host power of two under
VE, seed_scale / scale_dev on the device under VP and sub-VP, divided out of the flat gradient buffer afterwards) and the overflow guard
of apply().  tg and conv3x3 stay on the f32 kernels, so the reference fixtures apply at their fp32 tolerances (test_gpu_train.py,
test_gpu_train_sde.py, test_gpu_train_ss.py), which the 16-bit products themselves can never meet.
"""
import contextlib
import os

import pytest
import torch

from helpers import TRAIN_CASES, check_step_against_fixture, load_golden, train_inputs
from sde_train_cases import SDE_TRAIN_CASES, make_sde
from ss_train_cases import SS_TRAIN_CASES
from test_gpu_train import GRAD_TOL, LOSS_TOL, PARAM_TOL
from test_gpu_train_sde import SCORE_TOL, _all_state, _batch, _masks, _model

pytestmark = pytest.mark.gpu

PLUMBING_SWITCH = 48


@contextlib.contextmanager
def plumbing16():
    """Trainers created inside run the 16-bit step's plumbing; the switch is read at creation and restored on the way out."""
    from text2protein_amd import _lib
    lib = _lib.load()
    _lib.check(lib.t2p_debug_set(PLUMBING_SWITCH, 1))
    try:
        yield
    finally:
        lib.t2p_debug_set(PLUMBING_SWITCH, 0)


def _case(name):
    for table in (TRAIN_CASES, SDE_TRAIN_CASES, SS_TRAIN_CASES):
        if name in table:
            return dict(table[name])
    raise KeyError(name)


def _setup(name):
    """An f32 trainer with the plumbing on (call inside plumbing16()), the fixture's weights and dropout masks, and its step function."""
    from text2protein_amd import losses, sde_lib
    case = _case(name)
    case.setdefault("sde", "ve")
    cfg = case["config"]()
    inp = train_inputs(cfg, case)
    model = _model(case, cfg, "f32")
    model.set_dropout_masks(_masks(case, cfg, model))
    sde = make_sde(sde_lib, cfg, case)
    model.set_sde(sde)
    step_fn = losses.get_step_fn(sde, train=True, optimize_fn=losses.optimization_manager(cfg))
    return case, cfg, inp, model, step_fn


# (parameter tolerance, bound on the update's rel-L2) as the fp32 test of each fixture holds them: test_gpu_train (VE),
# test_gpu_train_sde (train_tinyB_vp: 2e-5, one sample at t = 0.99 stepping at the full rate); the ss fixture goes through test_gpu_train_ss's own
_PARAM = {"train_tinyB_vp": (2e-5, 5e-3), "train_cond_length": (1e-4, 2e-2)}


@pytest.mark.parametrize("name", ["train_tiny", "train_tinyB", "train_tiny_vp", "train_tinyB_vp", "train_tiny_subvp", "train_tinyB_ssdrop",
                                  pytest.param("train_cond_length", marks=pytest.mark.skipif(os.environ.get("T2P_LONG_TESTS") != "1",
                                               reason="the real-size model (75 M parameters through host-side norms and projections): "
                                                      "T2P_LONG_TESTS=1 runs it; the tiny cases carry the check"))])
def test_plumbing_step_vs_reference(name):
    """ONE step with exact products and the 16-bit step's reductions, seed scale and guard against autograd through the reference
    UNetModel, by the fp32 procedure at the fp32 tolerances: train_tiny / train_tinyB (dropout masks, up / down blocks, all three
    conditions; host seed scale), the VP and sub-VP fixtures (device-chosen seed scale), one ss fixture with block dropout."""
    g = load_golden(name)
    label = name + " (plumbing of the 16-bit step, f32 products)"
    with plumbing16():
        case, cfg, inp, model, step_fn = _setup(name)
        if "ss_indices" in case:                   # the whole procedure of test_gpu_train_ss, its element-by-element update check included
            from test_gpu_train_ss import check_ss_step_against_fixture
            out = check_ss_step_against_fixture(name, g, case, cfg, inp, model, step_fn, label=label)
        else:
            ptol, dtol = _PARAM.get(name, (PARAM_TOL, 5e-3))
            out = check_step_against_fixture(label, g, case, cfg, inp, model, step_fn, _batch(inp), loss_tol=LOSS_TOL, score_tol=SCORE_TOL,
                                             grad_tol=GRAD_TOL, param_tol=ptol, delta_tol=dtol)
    from test_gpu_baseline import _record
    _record(f"train_plumbing_{name}", out)


def test_plumbing_bias_and_norm_gradients_are_bitwise_reproducible():
    """Two fresh trainers under the switch: every one-dimensional parameter (biases, GroupNorm / LayerNorm weights) gets its gradient
    only from fixed-order reductions of fp32 data, so those are bit-identical.  (The weight gradients still pass through tgemm's fp32
    atomics and are not asserted bitwise.)"""
    from text2protein_amd import losses
    runs = []
    with plumbing16():
        for _ in range(2):
            case, cfg, inp, model, _ = _setup("train_tinyB")
            model.loss(_batch(inp), t=inp["t"], z=inp["z"], backward=True)
            runs.append(model.read(losses.GRAD))
            del model
    one_d = [n for n, v in runs[0].items() if v.dim() == 1]
    nonzero = [n for n in one_d if float(runs[0][n].abs().max()) > 0]
    print(f"{len(one_d)} one-dimensional parameters of {len(runs[0])}, {len(nonzero)} with a non-zero gradient")
    assert len(one_d) > 50 and len(nonzero) > 0.8 * len(one_d)        # (an AttnBlockpp's key bias has a zero gradient in exact arithmetic)
    for n in one_d:
        assert torch.equal(runs[0][n], runs[1][n]), n


def test_plumbing_overflow_guard_leaves_state_unchanged():
    """After a completed backward pass one inf is written into the gradient buffer: apply() refuses and the parameters, both moments,
    the EMA and the step counters read back exactly as before; with the gradient restored the same apply() goes through.  A trainer
    created without the switch has no guard (test_training16_overflow_guard_leaves_state_unchanged: fp32 mode runs as it always has)."""
    from text2protein_amd import losses
    from text2protein_amd._lib import T2PError
    with plumbing16():
        case, cfg, inp, model, _ = _setup("train_tiny")
    # (the switch is read at creation: it is off again from here on)
    model.set_step(case["step0"])
    model.loss(_batch(inp), t=inp["t"], z=inp["z"], backward=True)
    before, steps = _all_state(model), model.get_step()
    name = next(iter(before[losses.GRAD]))
    bad = before[losses.GRAD][name].clone()
    bad.view(-1)[0] = float("inf")
    model.write(losses.GRAD, {name: bad})
    with pytest.raises(T2PError, match="not finite"):
        model.apply()
    after = _all_state(model)
    for w in (losses.PARAM, losses.EMA, losses.EXP_AVG, losses.EXP_AVG_SQ):
        for n in before[w]:
            assert torch.equal(before[w][n], after[w][n]), (w, n)
    assert model.get_step() == steps
    model.write(losses.GRAD, {name: before[losses.GRAD][name]})
    model.apply()
    assert model.get_step() == (steps[0] + 1, steps[1] + 1, steps[2] + 1)
    moved = model.read(losses.PARAM)
    assert any(not torch.equal(moved[n], before[losses.PARAM][n]) for n in moved)
