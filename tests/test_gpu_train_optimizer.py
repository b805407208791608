"""Optimizer and EMA paths that no whole-step fixture reaches, on the GPU through t2p_train_write / t2p_train_set_step / t2p_train_apply:
the matrix of tests/optimizer_cases.py (weight decay 0 / 1e-2; Adam update 1 / 2 / 1000; clipping off / inactive / active; warm-up off /
running / over; EMA updates 0 / 5 / 10 000), once on a plain f32 trainer (atomic sum of squares) and once under plan switch 48 (the
16-bit step's fixed-order sum of squares and overflow guard inside apply).  Reference: the oracle's formulas in float64 on the same fp32
inputs; bounds: 4x the float32 oracle's own error (optimizer_cases.BOUND, re-measured by tests/test_cpu_optimizer.py)."""
import contextlib

import pytest
import torch

import optimizer_cases as OC
from helpers import rel_l2, train_inputs
from test_gpu_train_plumbing import plumbing16

pytestmark = pytest.mark.gpu

_WHICH = {}


def _trainer(cfg, plumbing):
    """The smallest trainer; under the switch with one completed backward pass behind it (the guard of apply() requires one)."""
    from text2protein_amd import losses, synth
    cfg.device = "cuda:0"
    with plumbing16() if plumbing else contextlib.nullcontext():
        model = losses.HipTrainModel(cfg, device="cuda:0", seed=11)
    model.load_state_dict(synth.synth_state_dict(cfg, 0))
    if plumbing:
        case = dict(seed=2, B=1, T=2, lengths=[8], mask_info=None)
        inp = train_inputs(cfg, case)
        loss = model.loss({k: inp[k] for k in ("coords_6d", "mask_pair", "context")}, t=inp["t"], z=inp["z"], backward=True)
        assert loss == loss and abs(loss) < float("inf")
    return model


def _run(model, st, step, k, ema_updates):
    from text2protein_amd import losses
    if not _WHICH:
        _WHICH.update(p=losses.PARAM, g=losses.GRAD, m=losses.EXP_AVG, v=losses.EXP_AVG_SQ, e=losses.EMA)
    for key, which in _WHICH.items():
        model.write(which, st[key])
    model.set_step(step, adam_updates=k - 1, ema_updates=ema_updates)
    model.apply()
    assert model.get_step() == (step + 1, k, ema_updates + 1)
    got = {q: model.read(_WHICH[w]) for q, w in (("g", "g"), ("p", "p"), ("m", "m"), ("v", "v"), ("ema", "e"))}
    got["update"] = {n: got["p"][n] - st["p"][n] for n in st["p"]}
    return got


_ORACLE = {}        # the float64 reference of a case: computed by the first of the two trainer kinds to reach it, dropped by the second


def _reference(cfg, st, wd, clip, warmup, step, k, ema_updates):
    key = (wd, clip, warmup, step, k, ema_updates)
    if key in _ORACLE:
        return _ORACLE.pop(key)
    ref = OC.oracle_apply(cfg, st, step, k, ema_updates, torch.float64)
    if len(_ORACLE) < 18:              # (one test's worth: the two kinds of a case run back to back; never more than that is kept)
        _ORACLE[key] = ref
    return ref


@pytest.mark.parametrize("plumbing", [False, True], ids=["f32", "plumbing16"])
@pytest.mark.parametrize("warmup,step", OC.WARMUP, ids=["warmup_off", "warmup_running", "warmup_over"])
@pytest.mark.parametrize("clip", OC.CLIP)
def test_optimizer_matrix(clip, warmup, step, plumbing):
    worst = {q: 0.0 for q in OC.QUANTITIES}
    st = None
    clipped = {}                           # (k, ema updates) -> the gradient read back without weight decay
    for wd in OC.WEIGHT_DECAY:
        cfg = OC.cfg_optimizer(wd, clip, warmup)
        model = _trainer(cfg, plumbing)
        if st is None:
            st = OC.draw_state(model.param_table(), clip)
            norm = OC.grad_norm(st)
            assert (norm < 1.0) if clip == "below" else (norm > 1.0), norm
        for k in OC.ADAM_K:
            for ema_updates in OC.EMA_UPDATES:
                got = _run(model, st, step, k, ema_updates)
                e = OC.worst_errors(got, _reference(cfg, st, wd, clip, warmup, step, k, ema_updates))
                for q in OC.QUANTITIES:
                    worst[q] = max(worst[q], e[q])
                    assert e[q] < OC.BOUND[q], (q, e[q], OC.BOUND[q], dict(weight_decay=wd, clip=clip, warmup=warmup, step=step, k=k,
                                                                         ema_updates=ema_updates, plumbing=plumbing))
                # the gradient read back is the clipped one, the same whether or not weight decay is on
                if wd == 0.0:
                    clipped[(k, ema_updates)] = got["g"]
                else:
                    assert max(rel_l2(got["g"][n], clipped[(k, ema_updates)][n]) for n in got["g"]) < OC.BOUND["g"], (k, ema_updates)
                if clip != "above":
                    assert all(torch.equal(got["g"][n], st["g"][n]) for n in st["g"])      # (nothing to clip: written back unchanged)
        del model
    tag = f"{clip}_warmup{int(warmup)}_step{step}_{'plumbing16' if plumbing else 'f32'}"
    print(f"optimizer matrix {tag}: worst rel-L2 per tensor " + ", ".join(f"{q} {v:.1e} (bound {OC.BOUND[q]:.1e})" for q, v in worst.items()))
    from test_gpu_baseline import _record
    _record(f"train_optimizer_{tag}", worst)
