"""Mixed-precision training step (compute_dtype f16 / bf16) on the GPU: the 16-bit strided GEMM (t2p_op_tgemm16) and the whole step.

Oracles: for the op, an fp64 product of the operands AFTER rounding them to the 16-bit type (so the check pins the kernel to
fp32-accumulation level, not merely "close to fp32"); for the step, the same reference-autograd fixtures (tests/golden/train_*.npz,
fp32) the fp32 step is held to, with tolerances set from measured 16-bit errors.
"""
import ctypes as C

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from helpers import TRAIN_CASES, CounterDropout, load_golden, projection, rel_l2, train_inputs

pytestmark = pytest.mark.gpu

DT = {"f16": (2, torch.float16), "bf16": (1, torch.bfloat16)}
OP_TOL = 1e-5           # rel-L2 against the fp64 product of the rounded operands

# whole step against the fp32 reference fixtures: about 2x the measured error, capped at the planned ceilings
# (f16: loss 2e-3, score 3e-3, gradient norm / projection 1e-2 / 3e-2 of max(norm, 1e-3 total), stored gradients 1e-2, post-step 2e-4;
# bf16: 8x).  train_tinyB measures above those ceilings and carries its own row; DESIGN.md section 7 records why that is rounding
# (errors scale with the unit roundoff: bf16 / f16 = 8.4, median over 644 tensors) amplified through the network in dY itself
# (weight and bias gradients of the same layers are equally far off), not range loss or cancellation in the bias column sums.
STEP_TOL = {
    "f16": dict(loss=1e-4, score=2e-3, grad_norm=3e-3, grad_proj=1e-2, grad=1e-2, post=2e-4, post_norm=2e-4),
    "bf16": dict(loss=3e-4, score=6e-3, grad_norm=2.2e-2, grad_proj=6e-2, grad=5.5e-2, post=4e-4, post_norm=5e-4),
    ("f16", "train_tinyB"): dict(loss=1e-4, score=6e-3, grad_norm=2.2e-2, grad_proj=6e-2, grad=3.5e-2, post=4e-4, post_norm=1.1e-3),
    ("bf16", "train_tinyB"): dict(loss=2e-4, score=4e-2, grad_norm=0.22, grad_proj=0.44, grad=0.36, post=4e-3, post_norm=3e-3),
}


@pytest.fixture(scope="module")
def lib():
    from text2protein_amd import _lib
    return _lib.load()


_KEEP = []


def dev(t):
    d = t.contiguous().to("cuda")
    _KEEP.append(d)
    return d


@pytest.fixture(autouse=True)
def _release_device_tensors():
    yield
    torch.cuda.synchronize()
    _KEEP.clear()


def P(t):
    return None if t is None else C.c_void_p(t.data_ptr())


def check(lib, rc):
    assert rc == 0, lib.t2p_last_error().decode()


def rounded(t, dt):
    return t.to(DT[dt][1]).double()


# ---- the 16-bit strided GEMM ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dt", ["f16", "bf16"])
def test_tgemm16_views_and_bias(lib, dt):
    """C = alpha A B + bias + beta C, A / B as row- or column-major views, at the shapes of test_tgemm_views."""
    worst = 0.0
    for M, N, K in [(64, 64, 16), (70, 33, 19), (256, 300, 129), (5, 288, 1000), (1000, 5, 77), (384, 256, 512)]:
        for ta in (0, 1):
            for tb in (0, 1):
                g = torch.Generator().manual_seed(M * 31 + N * 7 + K + ta * 2 + tb)
                a = torch.randn(M, K, generator=g)
                b = torch.randn(K, N, generator=g) / K ** 0.5
                bias = torch.randn(N, generator=g)
                c0 = torch.randn(M, N, generator=g)
                ref = 0.7 * (rounded(a, dt) @ rounded(b, dt)) + bias.double() + 0.5 * c0.double()
                da, db, out = dev(a.T.contiguous() if ta else a), dev(b.T.contiguous() if tb else b), dev(c0.clone())
                sAm, sAk = (1, M) if ta else (K, 1)
                sBk, sBn = (1, K) if tb else (N, 1)
                check(lib, lib.t2p_op_tgemm16(DT[dt][0], P(da), sAm, sAk, P(db), sBk, sBn, P(out), N, M, N, K, 1, 0, 0, 0, 0.7, 0.5,
                                              P(dev(bias)), 1, 0, 0, 0, 0, None))
                e = rel_l2(out.cpu(), ref)
                worst = max(worst, e)
                assert e < OP_TOL, (M, N, K, ta, tb, e)
    print(f"tgemm16 {dt}: views worst rel-L2 {worst:.1e}")


@pytest.mark.parametrize("dt", ["f16", "bf16"])
def test_tgemm16_split_k_heads_and_magnitudes(lib, dt):
    """Forced split-K (2, 7) into an initialised C; the library's own split on a long K; a batch of heads; operands near 1e4 and 1e-4
    (products pass through unscaled and unflushed)."""
    g = torch.Generator().manual_seed(5)
    code = DT[dt][0]
    M, N, K = 96, 160, 20000
    dy, x = torch.randn(K, M, generator=g), torch.randn(K, N, generator=g)
    c0 = torch.randn(M, N, generator=g)
    ref = c0.double() + rounded(dy, dt).T @ rounded(x, dt)
    errs = []
    for ks in (2, 7, 0):
        out = dev(c0.clone())
        check(lib, lib.t2p_op_tgemm16(code, P(dev(dy)), 1, M, P(dev(x)), N, 1, P(out), N, M, N, K, 1, 0, 0, 0, 1.0, 1.0, None, ks, 0, 0, 0, 0, None))
        errs.append(rel_l2(out.cpu(), ref))
    B, n, h, d = 3, 50, 4, 24
    q, k = torch.randn(B, n, h * d, generator=g), torch.randn(B, n, h * d, generator=g)
    S = dev(torch.zeros(B, h, n, n))
    dq, dk = dev(q), dev(k)
    for hh in range(h):
        check(lib, lib.t2p_op_tgemm16(code, C.c_void_p(dq.data_ptr() + 4 * hh * d), h * d, 1, C.c_void_p(dk.data_ptr() + 4 * hh * d), 1, h * d,
                                      C.c_void_p(S.data_ptr() + 4 * hh * n * n), n, n, n, d, B, n * h * d, n * h * d, h * n * n, 1.0, 0.0, None, 1,
                                      0, 0, 0, 0, None))
    ref_h = torch.einsum("bihd,bjhd->bhij", rounded(q, dt).reshape(B, n, h, d), rounded(k, dt).reshape(B, n, h, d))
    errs.append(rel_l2(S.cpu(), ref_h))
    sign = lambda t: torch.where(t >= 0, 1.0, -1.0)
    a = 1e4 * (1 + 0.5 * torch.rand(200, 300, generator=g)) * sign(torch.randn(200, 300, generator=g))
    b = 1e-4 * (1 + 0.5 * torch.rand(300, 120, generator=g)) * sign(torch.randn(300, 120, generator=g))
    out = dev(torch.zeros(200, 120))
    check(lib, lib.t2p_op_tgemm16(code, P(dev(a)), 300, 1, P(dev(b)), 120, 1, P(out), 120, 200, 120, 300, 1, 0, 0, 0, 1.0, 0.0, None, 1,
                                  0, 0, 0, 0, None))
    errs.append(rel_l2(out.cpu(), rounded(a, dt) @ rounded(b, dt)))
    print(f"tgemm16 {dt}: split-K 2 / 7 / auto, heads, magnitudes 1e4 x 1e-4: rel-L2 " + " ".join(f"{e:.1e}" for e in errs))
    assert max(errs) < OP_TOL


@pytest.mark.parametrize("dt", ["f16", "bf16"])
@pytest.mark.parametrize("B,H,W,Ci,Co", [(2, 8, 8, 32, 64), (3, 16, 16, 8, 32), (1, 12, 20, 40, 5)])
def test_tgemm16_convolution_weight_gradient(lib, dt, B, H, W, Ci, Co):
    """dW[co][tap][ci] = sum_pixels dY[pixel][co] X[pixel + tap][ci] (the 3x3 window gather) against conv2d's weight gradient on the
    rounded operands."""
    g = torch.Generator().manual_seed(B + H + Ci)
    x = torch.randn(B, Ci, H, W, generator=g, dtype=torch.float64)
    w = torch.randn(Co, Ci, 3, 3, generator=g, dtype=torch.float64, requires_grad=True)
    dy = torch.randn(B, Co, H, W, generator=g, dtype=torch.float64)
    xr, dyr = rounded(x.float(), dt), rounded(dy.float(), dt)
    F.conv2d(xr, w, padding=1).backward(dyr)
    ref = w.grad.permute(0, 2, 3, 1).reshape(Co, 9 * Ci)
    xn = dev(x.float().permute(0, 2, 3, 1).contiguous())
    dyn = dev(dy.float().permute(0, 2, 3, 1).contiguous())
    out = dev(torch.zeros(Co, 9 * Ci))
    check(lib, lib.t2p_op_tgemm16(DT[dt][0], P(dyn), 1, Co, P(xn), 0, 0, P(out), 9 * Ci, Co, 9 * Ci, B * H * W, 1, 0, Ci, 0, 1.0, 1.0, None, 0,
                                  1, H, W, Ci, None))
    e = rel_l2(out.cpu(), ref)
    print(f"tgemm16 {dt}: convolution weight gradient {B}x{H}x{W} {Ci}->{Co}: rel-L2 {e:.1e}")
    assert e < OP_TOL


def test_tgemm16_split_k_is_bitwise_reproducible(lib):
    g = torch.Generator().manual_seed(9)
    M, N, K = 128, 1152, 65536
    dy, x = dev(torch.randn(K, M, generator=g)), dev(torch.randn(K, N, generator=g))
    outs = []
    for _ in range(2):
        out = dev(torch.zeros(M, N))
        check(lib, lib.t2p_op_tgemm16(2, P(dy), 1, M, P(x), N, 1, P(out), N, M, N, K, 1, 0, 0, 0, 1.0, 1.0, None, 0, 0, 0, 0, 0, None))
        outs.append(out.cpu())
    assert torch.equal(outs[0], outs[1])


# ---- the whole step -----------------------------------------------------------------------------------------------------------------
def _model(case, cfg, dtype, scale=1.0):
    from text2protein_amd import synth
    from text2protein_amd.losses import HipTrainModel
    cfg.device = "cuda:0"
    m = HipTrainModel(cfg, device="cuda:0", seed=11, dtype=dtype)
    sd = synth.synth_state_dict(cfg, case["seed"])
    m.load_state_dict({k: v * scale for k, v in sd.items()} if scale != 1.0 else sd)
    return m


def _dropout_masks(case, cfg, model):
    if cfg.model.dropout <= 0:
        return []
    from oracle import t2p_oracle as O
    drop = CounterDropout(case["seed"], cfg.model.dropout)
    inputs, mid, outs = O.unet_plan(cfg)
    L, B = cfg.data.max_res_num, case["B"]
    table = dict(model.param_table())
    masks, k, side = [], 0, L
    for stage in inputs + [mid] + outs:
        for kind, prefix, up, down in stage:
            if kind != "res":
                continue
            side = side * 2 if up else side // 2 if down else side
            co = table[prefix + ".Conv_1.weight"][0]
            masks.append(drop.mask(k, (B, co, side, side)).permute(0, 2, 3, 1).contiguous().to(torch.uint8))
            k += 1
    return masks


def _state(model, cfg, step):
    from text2protein_amd import losses
    return dict(model=model, optimizer=losses.get_optimizer(cfg, model.parameters()),
                ema=losses.ExponentialMovingAverage(model.parameters(), decay=cfg.model.ema_rate), step=step)


def _fns(cfg):
    from text2protein_amd import losses, sde_lib
    sde = sde_lib.VESDE(sigma_min=cfg.model.sigma_min, sigma_max=cfg.model.sigma_max, N=cfg.model.num_scales)
    return losses.get_step_fn(sde, train=True, optimize_fn=losses.optimization_manager(cfg)), losses.get_step_fn(sde, train=False)


def _batch(inp):
    return {k: inp[k] for k in ("coords_6d", "mask_pair", "context", "mask_inpaint") if k in inp}


@pytest.mark.parametrize("dt,name", [("f16", "train_tiny"), ("f16", "train_tinyB"), ("f16", "train_cond_length"),
                                     ("bf16", "train_tiny"), ("bf16", "train_tinyB")])
def test_training_step16_vs_reference(dt, name):
    """ONE 16-bit training step against the fp32 reference autograd (the procedure of test_training_step_vs_reference): loss, score,
    every gradient through its norm and projection, the stored whole tensors, then the post-step parameters and EMA."""
    from text2protein_amd import losses
    g = load_golden(name)
    case = TRAIN_CASES[name]
    cfg = case["config"]()
    inp = train_inputs(cfg, case)
    model = _model(case, cfg, dt)
    names = [str(n) for n in g["names"]]
    assert [n for n, _ in model.param_table()] == names
    model.set_dropout_masks(_dropout_masks(case, cfg, model))
    assert len(model._keep) == int(g["n_dropout_calls"])
    batch = _batch(inp)
    tol = STEP_TOL.get((dt, name), STEP_TOL[dt])
    loss0, score = model.loss(batch, t=inp["t"], z=inp["z"], backward=True, return_score=True)
    e_score = rel_l2(score.cpu()[:, :, ::8, ::8] if case.get("full_size") else score.cpu(), g["score"])
    e_loss = abs(loss0 - float(g["loss"])) / abs(float(g["loss"]))
    grads = model.read(losses.GRAD)
    T = float(g["grad_total_norm"])
    pcache = {}
    e_norm = e_proj = 0.0
    for i, n in enumerate(names):
        scale = max(float(g["grads_norm"][i]), 1e-3 * T, 1e-30)
        e_norm = max(e_norm, abs(float(grads[n].double().norm()) - float(g["grads_norm"][i])) / scale)
        e_proj = max(e_proj, abs(projection(n, grads[n], cache=pcache) - float(g["grads_proj"][i])) / scale)
    full = [k[5:] for k in g if k.startswith("grad:")]
    e_grad, worst_n = max((rel_l2(grads[n], g["grad:" + n]), n) for n in full)
    step_fn, _ = _fns(cfg)
    state = _state(model, cfg, case["step0"])
    loss1 = step_fn(state, batch, condition=cfg.model.condition, t=inp["t"], z=inp["z"])
    assert abs(loss1 - loss0) <= 1e-6 * abs(loss0) and model.get_step() == (case["step0"] + 1, 1, 1)
    post, ema = model.read(losses.PARAM), model.read(losses.EMA)
    e_post = max(rel_l2(post[n], g["post:" + n]) for n in full)
    e_post_norm = 0.0
    for key, got in (("post", post), ("ema", ema)):
        for i, n in enumerate(names):
            scale = max(float(g[key + "_norm"][i]), 1e-30)
            e_post_norm = max(e_post_norm, abs(float(got[n].double().norm()) - float(g[key + "_norm"][i])) / scale)
    print(f"{dt} {name}: loss rel {e_loss:.1e}, score rel-L2 {e_score:.1e}, gradient norm {e_norm:.1e} / projection {e_proj:.1e} "
          f"(of max(norm, 1e-3 total)), stored gradients rel-L2 {e_grad:.1e} over {len(full)} tensors ({worst_n}), post-step parameters rel-L2 "
          f"{e_post:.1e}, post-step parameter / EMA norms {e_post_norm:.1e}")
    assert e_loss < tol["loss"] and e_score < tol["score"]
    assert e_norm < tol["grad_norm"] and e_proj < tol["grad_proj"] and e_grad < tol["grad"]
    assert e_post < tol["post"] and e_post_norm < tol["post_norm"]


def _all_state(model):
    from text2protein_amd import losses
    return {w: model.read(w) for w in (losses.PARAM, losses.GRAD, losses.EMA, losses.EXP_AVG, losses.EXP_AVG_SQ)}


def test_training_step16_is_bitwise_reproducible():
    """Two fresh f16 trainers, same seed and weights, two steps each with the fixture's masks: every buffer bitwise equal."""
    case = TRAIN_CASES["train_tinyB"]
    cfg = case["config"]()
    inp = train_inputs(cfg, case)
    runs = []
    for _ in range(2):
        model = _model(case, cfg, "f16")
        model.set_dropout_masks(_dropout_masks(case, cfg, model))
        step_fn, _ = _fns(cfg)
        state = _state(model, cfg, case["step0"])
        losses_seq = [step_fn(state, _batch(inp), condition=cfg.model.condition, t=inp["t"], z=inp["z"]) for _ in range(2)]
        runs.append((losses_seq, _all_state(model), model.get_step()))
        del model
    assert runs[0][2] == runs[1][2] and np.allclose(runs[0][0], runs[1][0], rtol=1e-6, atol=0)   # (the scalar loss sums with double atomics)
    for w in runs[0][1]:
        for n in runs[0][1][w]:
            assert torch.equal(runs[0][1][w][n], runs[1][1][w][n]), (w, n)


def test_training16_loss_falls_and_tracks_fp32():
    """12 f16 steps and 12 f32 steps on one batch from the same start (dropout masks fixed): the f16 loss falls, its first step matches
    f32, its last is within 5 % of f32's; eval_loss runs on the EMA; state_dict() loads unchanged into an f32 trainer."""
    from text2protein_amd import losses
    case = dict(TRAIN_CASES["train_tinyB"], step0=5000)
    cfg = case["config"]()
    inp = train_inputs(cfg, case)
    seqs, evals, models = {}, {}, {}
    for dt in ("f32", "f16"):
        model = _model(case, cfg, dt)
        model.set_dropout_masks(_dropout_masks(case, cfg, model))
        step_fn, eval_fn = _fns(cfg)
        state = _state(model, cfg, 5000)
        e0 = eval_fn(state, _batch(inp), condition=cfg.model.condition, t=inp["t"], z=inp["z"])
        seqs[dt] = [step_fn(state, _batch(inp), condition=cfg.model.condition, t=inp["t"], z=inp["z"]) for _ in range(12)]
        evals[dt] = (e0, eval_fn(state, _batch(inp), condition=cfg.model.condition, t=inp["t"], z=inp["z"]))
        models[dt] = model
    a, b = seqs["f16"], seqs["f32"]
    first, last = abs(a[0] - b[0]) / abs(b[0]), abs(a[-1] - b[-1]) / abs(b[-1])
    print("f16 loss over 12 steps:", " ".join(f"{v:.4f}" for v in a), f"| f32 last {b[-1]:.4f}; step 0 rel {first:.1e}, last rel {last:.1e}; "
          f"f16 EMA loss {evals['f16'][0]:.4f} -> {evals['f16'][1]:.4f}")
    assert all(np.isfinite(a)) and a[-1] < a[0]
    assert first < STEP_TOL["f16"]["loss"] and last < 0.05
    e0, e1 = evals["f16"]
    assert e1 < e0 and e1 > a[-1]                                       # the EMA follows, behind the live weights
    sd = models["f16"].state_dict()
    f32 = losses.HipTrainModel(cfg, device="cuda:0", seed=11)
    f32.load_state_dict(sd)
    back = f32.state_dict()
    assert list(back) == list(sd) and all(torch.equal(back[n], sd[n]) for n in sd)


def test_training16_overflow_guard_leaves_state_unchanged():
    """Weights scaled by 1e5 overflow f16: the step raises T2PError and the parameters, both moments, the EMA and the step counters
    read back exactly as before."""
    from text2protein_amd._lib import T2PError
    case = TRAIN_CASES["train_tiny"]
    cfg = case["config"]()
    inp = train_inputs(cfg, case)
    model = _model(case, cfg, "f16", scale=1e5)
    step_fn, _ = _fns(cfg)
    state = _state(model, cfg, case["step0"])
    before, steps = _all_state(model), model.get_step()
    with pytest.raises(T2PError, match="not finite"):
        step_fn(state, _batch(inp), condition=cfg.model.condition, t=inp["t"], z=inp["z"])
    after = _all_state(model)
    from text2protein_amd import losses
    for w in (losses.PARAM, losses.EMA, losses.EXP_AVG, losses.EXP_AVG_SQ):
        for n in before[w]:
            assert torch.equal(before[w][n], after[w][n]), (w, n)
    assert model.get_step() == steps
    f32 = _model(case, cfg, "f32", scale=1e5)                           # fp32 mode: no guard, the step runs as it always has
    step_fn(_state(f32, cfg, case["step0"]), _batch(inp), condition=cfg.model.condition, t=inp["t"], z=inp["z"])


def test_train_model_dtype_surface():
    from text2protein_amd import losses
    cfg = TRAIN_CASES["train_tiny"]["config"]()
    cfg.device = "cuda:0"
    with pytest.raises(ValueError):
        losses.HipTrainModel(cfg, device="cuda:0", dtype="f64")
    assert losses.HipTrainModel(cfg, device="cuda:0")._mc.compute_dtype == 0
    assert losses.get_train_model(cfg, dtype="bf16")._mc.compute_dtype == 1
