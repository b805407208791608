"""The DDIM sampler's own training objective on the GPU: t2p_train_set_ploss, t2p_op_ploss_draw_t, DiffusionSampler.p_loss / forward and
losses.get_ploss_step_fn.

Oracle: tests/golden/train_*_ploss_*.npz -- loss, pred_noise, gradients and post-step state produced by autograd through the REFERENCE
UNetModel with the reference's own DiffusionSampler.p_loss (tests/golden/make_golden_train_ploss.py; the masked cases write the masked form
out next to the reference's tables).  The fp32 tolerances are those of the VE step (tests/test_gpu_train.py: the network and the backward
pass are shared); the 16-bit bounds are about twice the values measured against the same fp32 fixtures.

Not covered here: two data-parallel ranks.  The rank body of test_gpu_train.py's data-parallel test (tests/dist_worker.py) builds its own
VE step function and cannot be pointed at another objective without editing it; the data-parallel branch is get_step_fn's own, shared
through one body (losses._run_step), and the per-sample normalisation that makes equal shards reproduce the whole batch is pinned on the
CPU (tests/test_cpu_train_ploss.py) and by the masked fixtures.
"""
import ctypes as C

import numpy as np
import pytest
import torch

import ploss_oracle as PO
from helpers import check_step_against_fixture, load_golden, projection, rel_l2
from ploss_cases import PLOSS_CASES, make_betas, ploss_batch, ploss_inputs

pytestmark = pytest.mark.gpu

LOSS_TOL = 1e-5      # the VE step's tolerances (tests/test_gpu_train.py)
SCORE_TOL = 1e-5
GRAD_TOL = 1e-4
PARAM_TOL = 1e-5

# 16-bit step against the fp32 reference fixtures: about 2x the measured values ("Parity, 16-bit, p_loss": every row
# measured on an MI355X).  The 16-bit step is bitwise reproducible (fixed-order reductions), so the measured figures do not move.
STEP16_TOL = {
    ("f16", "train_tiny_ploss_l2"): dict(loss=5e-4, score=2.3e-3, grad_norm=9.4e-3, grad_proj=2e-2, grad=9.6e-3, post=7.2e-4, post_norm=4.4e-4),
    ("bf16", "train_tiny_ploss_l2"): dict(loss=8.5e-4, score=1.7e-2, grad_norm=4.6e-2, grad_proj=8.1e-2, grad=5.3e-2, post=7.2e-4, post_norm=7.5e-4),
    ("f16", "train_tiny_ploss_l1"): dict(loss=3e-4, score=2.3e-3, grad_norm=8.3e-3, grad_proj=2.2e-2, grad=1.3e-2, post=1e-4, post_norm=2.2e-4),
    ("bf16", "train_tiny_ploss_l1"): dict(loss=2.7e-4, score=1.7e-2, grad_norm=8.3e-2, grad_proj=0.14, grad=0.2, post=7.2e-4, post_norm=9.1e-4),
    ("f16", "train_tinyB_ploss_l2m"): dict(loss=8.7e-5, score=3.8e-3, grad_norm=3.4e-2, grad_proj=4.8e-2, grad=4.1e-2, post=1.8e-3, post_norm=1.4e-3),
    ("f16", "train_tinyB_ploss_l1m"): dict(loss=1.5e-4, score=3.8e-3, grad_norm=4.5e-2, grad_proj=6.3e-2, grad=4.3e-2, post=1.7e-3, post_norm=1.7e-3),
}


def _model(case, cfg, dtype="f32", seed=11):
    from text2protein_amd import synth
    from text2protein_amd.losses import HipTrainModel
    cfg.device = "cuda:0"
    m = HipTrainModel(cfg, device="cuda:0", seed=seed, dtype=dtype)
    m.load_state_dict(synth.synth_state_dict(cfg, case["seed"]))
    return m


def _sampler(model, case, cfg, **kw):
    from text2protein_amd.ddim import DiffusionSampler
    betas = make_betas(case, cfg)
    return DiffusionSampler(model, timesteps=betas.numel(), betas=betas, loss_type=case["loss_type"], **kw)


def _setup(name, dtype="f32", set_objective=True, **case_over):
    from test_gpu_train16 import _dropout_masks
    case = dict(PLOSS_CASES[name], **case_over)
    cfg = case["config"]()
    inp = ploss_inputs(cfg, case)
    model = _model(case, cfg, dtype)
    model.set_dropout_masks(_dropout_masks(case, cfg, model))
    ds = _sampler(model, case, cfg)
    if set_objective:
        model.set_ploss(ds)
    return case, cfg, inp, model, ds


def _fns(ds, cfg, case, **kw):
    from text2protein_amd import losses
    return (losses.get_ploss_step_fn(ds, train=True, optimize_fn=losses.optimization_manager(cfg), masked=case["masked"], **kw),
            losses.get_ploss_step_fn(ds, train=False, masked=case["masked"]))


def _state(model, cfg, step):
    from text2protein_amd import losses
    return dict(model=model, optimizer=losses.get_optimizer(cfg, model.parameters()),
                ema=losses.ExponentialMovingAverage(model.parameters(), decay=cfg.model.ema_rate), step=step)


def _all_state(model):
    from text2protein_amd import losses
    return {w: model.read(w) for w in (losses.PARAM, losses.GRAD, losses.EMA, losses.EXP_AVG, losses.EXP_AVG_SQ)}


def _masked_kw(inp, case):
    """p_loss's `batch` argument for a case."""
    return dict(batch={k: inp[k] for k in ("mask_pair", "mask_inpaint") if k in inp}) if case["masked"] else {}


# ---- 1. reference parity, f32 --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(PLOSS_CASES))
def test_training_step_vs_reference(name):
    """ONE fp32 training step under p_loss against autograd through the reference UNetModel and the reference's DiffusionSampler, with the
    assertions and the tolerances of the VE step.  The two tinyB cases step at the full learning rate (step0 >= warmup) with one sample at
    the last timestep, the situation for which test_gpu_train_sde.py gives train_tinyB_vp 2e-5 on the post-step parameters (a sign-like
    first Adam update at the full rate); they take the same."""
    g = load_golden(name)
    case, cfg, inp, model, ds = _setup(name)
    assert np.array_equal(inp["t"].numpy(), g["t"])
    assert PO.tables_close(ds.sqrt_alpha_cumprod, ds.sqrt_one_minus_alphas_cumprod, g["sqrt_alpha_cumprod"], g["sqrt_one_minus_alphas_cumprod"])
    step_fn, _ = _fns(ds, cfg, case)
    check_step_against_fixture(name, g, case, cfg, inp, model, step_fn, ploss_batch(inp, case), loss_tol=LOSS_TOL, score_tol=SCORE_TOL,
                               grad_tol=GRAD_TOL, param_tol=2e-5 if name.startswith("train_tinyB") else PARAM_TOL, delta_tol=5e-3)


# ---- 2. the perturbed input and the label -------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["train_tiny_ploss_l2", "train_tinyB_ploss_l2m"])
def test_perturbed_input_and_label_per_sample(name):
    """pred_noise against the reference's, sample by sample: a_b and s_b enter through x_noisy, the label through the embedding.  A t moved
    by one table entry fails the same bound in the sample it was moved in, so the bound tells neighbouring entries apart."""
    g = load_golden(name)
    case, cfg, inp, model, ds = _setup(name)
    ref = torch.from_numpy(g["score"])
    x, ctx, z = inp["coords_6d"], inp["context"], inp["z"]
    _, pred = ds.p_loss(x, ctx, inp["t"], z, return_pred=True, **_masked_kw(inp, case))
    per_sample = [rel_l2(pred.cpu()[b], ref[b]) for b in range(case["B"])]
    print(f"{name}: pred_noise rel-L2 per sample " + " ".join(f"{e:.1e}" for e in per_sample) + f"; t {g['t'].tolist()}, a {g['a'].tolist()}, "
          f"s {g['s'].tolist()}")
    assert max(per_sample) < SCORE_TOL
    for b in range(case["B"]):
        t2 = inp["t"].clone()
        t2[b] += 1 if int(t2[b]) + 1 < ds.timesteps else -1
        _, p2 = ds.p_loss(x, ctx, t2, z, return_pred=True, **_masked_kw(inp, case))
        errs = [rel_l2(p2.cpu()[k], ref[k]) for k in range(case["B"])]
        print(f"{name}: t[{b}] {int(inp['t'][b])} -> {int(t2[b])}: per sample " + " ".join(f"{e:.1e}" for e in errs))
        assert errs[b] > 10 * SCORE_TOL and all(errs[k] < SCORE_TOL for k in range(case["B"]) if k != b)


@pytest.mark.parametrize("name", list(PLOSS_CASES))
def test_zero_head_weights_make_the_loss_a_function_of_the_noise(name):
    """With an all-zero head convolution the prediction is a constant per sample and channel, and the loss is the restated loss of that
    constant against the noise: the mask, the normalisation and l1 / l2 alone, without the network."""
    from text2protein_amd import losses
    case, cfg, inp, model, ds = _setup(name)
    head = [n for n, _ in model.param_table() if n.endswith(".weight")][-1]
    model.write(losses.PARAM, {head: torch.zeros_like(model.read(losses.PARAM, head))})
    loss, pred = ds.p_loss(inp["coords_6d"], inp["context"], inp["t"], inp["z"], return_pred=True, **_masked_kw(inp, case))
    pred = pred.cpu()
    assert torch.equal(pred, pred[:, :, :1, :1].expand_as(pred))
    mask = PO.conditional_mask(tuple(pred.shape), cfg.model.condition, inp["mask_pair"], inp.get("mask_inpaint")) if case["masked"] else None
    want = float(PO.loss(pred.double(), inp["z"].double(), case["loss_type"], mask))
    assert abs(loss - want) <= 1e-6 * abs(want), (loss, want)


# ---- 3. the integer draw --------------------------------------------------------------------------------------------------------------
def _draw_op(seed, stream, B, T):
    from text2protein_amd import _lib
    from text2protein_amd._lib import check, ptr, stream_ptr
    out = torch.full((B,), -1, dtype=torch.int32, device="cuda")
    check(_lib.load().t2p_op_ploss_draw_t(seed, stream, B, T, ptr(out), stream_ptr()))
    torch.cuda.synchronize()
    return out.cpu()


@pytest.mark.parametrize("T", [1, 7, 1000])
def test_draw_t_op(T):
    got = _draw_op(11, 4096 * 2 + 5, 4096, T)
    assert np.array_equal(got.numpy().astype(np.int64), PO.draw_t(11, 4096 * 2 + 5, 4096, T))
    assert int(got.min()) >= 0 and int(got.max()) < T


def test_draw_t_op_refusals():
    from text2protein_amd import _lib
    lib = _lib.load()
    out = torch.zeros(4, dtype=torch.int32, device="cuda")
    for args in ((1, 5, 0, 10, C.c_void_p(out.data_ptr())), (1, 5, 4, 0, C.c_void_p(out.data_ptr())),
                 (1, 5, 4, (1 << 24) + 1, C.c_void_p(out.data_ptr())), (1, 5, 4, 10, None)):
        assert lib.t2p_op_ploss_draw_t(*args, None) != 0, args


def test_device_drawn_pass_equals_the_pass_given_the_draws():
    """t = None, z = None on a fresh trainer (loss_calls = 0: t on stream 5, z on stream 1 under the trainer seed 11) against a fresh
    trainer given the operator's t and t2p_op_philox_normal's z: the same loss and the same pred_noise, bit for bit."""
    from text2protein_amd import _lib
    from text2protein_amd._lib import check, ptr, stream_ptr
    case, cfg, inp, model, ds = _setup("train_tiny_ploss_l2")
    x, ctx = inp["coords_6d"], inp["context"]
    l_dev, p_dev = ds(x, ctx, return_pred=True)
    t = _draw_op(11, 5, case["B"], ds.timesteps).long()
    z = torch.empty(x.shape, device="cuda")
    check(_lib.load().t2p_op_philox_normal(ptr(z), z.numel(), 11, 1, stream_ptr()))
    case2, cfg2, inp2, model2, ds2 = _setup("train_tiny_ploss_l2")
    l_given, p_given = ds2.p_loss(x, ctx, t, z, return_pred=True)
    print(f"device-drawn t {t.tolist()}: loss {l_dev!r} / given the draws {l_given!r}")
    assert l_dev == l_given and torch.equal(p_dev, p_given)
    l_next = ds(x, ctx)                                   # the next call draws on other streams
    assert np.isfinite(l_next) and l_next != l_dev


# ---- 4. the unmasked loss is torch's -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["train_tiny_ploss_l2", "train_tiny_ploss_l1", "train_tinyB_ploss_l2m", "train_tinyB_ploss_l1m"])
def test_unmasked_loss_equals_torch(name):
    """p_loss without `batch` is the reference's definition: mse_loss / abs().mean() of the returned pred_noise and the supplied noise over
    every element -- also on a trainer whose configuration carries conditions (they are ignored)."""
    case, cfg, inp, model, ds = _setup(name)
    loss, pred = ds.p_loss(inp["coords_6d"], inp["context"], inp["t"], inp["z"], return_pred=True)
    p, z = pred.cpu().double(), inp["z"].double()
    want = float(torch.nn.functional.mse_loss(p, z)) if case["loss_type"] == "l2" else float((p - z).abs().mean())
    print(f"{name}: unmasked loss {loss:.7f}, torch {want:.7f}")
    assert abs(loss - want) <= 1e-6 * abs(want)
    if not case["masked"]:
        g = load_golden(name)
        assert abs(loss - float(g["loss"])) <= LOSS_TOL * abs(float(g["loss"]))


# ---- 5. f16 / bf16 ----------------------------------------------------------------------------------------------------------------------
def _step16_figures(dt, name):
    from text2protein_amd import losses
    g = load_golden(name)
    case, cfg, inp, model, ds = _setup(name, dt)
    names = [str(n) for n in g["names"]]
    batch = ploss_batch(inp, case)
    step_fn, _ = _fns(ds, cfg, case)
    loss0, score = model.loss(batch, t=inp["t"], z=inp["z"], backward=True, return_score=True)
    out = dict(score=rel_l2(score.cpu(), g["score"]), loss=abs(loss0 - float(g["loss"])) / abs(float(g["loss"])))
    grads = model.read(losses.GRAD)
    T = float(g["grad_total_norm"])
    pcache = {}
    out["grad_norm"] = out["grad_proj"] = 0.0
    for i, n in enumerate(names):
        scale = max(float(g["grads_norm"][i]), 1e-3 * T, 1e-30)
        out["grad_norm"] = max(out["grad_norm"], abs(float(grads[n].double().norm()) - float(g["grads_norm"][i])) / scale)
        out["grad_proj"] = max(out["grad_proj"], abs(projection(n, grads[n], cache=pcache) - float(g["grads_proj"][i])) / scale)
    full = [k[5:] for k in g if k.startswith("grad:")]
    out["grad"] = max(rel_l2(grads[n], g["grad:" + n]) for n in full)
    state = _state(model, cfg, case["step0"])
    loss1 = step_fn(state, batch, condition=cfg.model.condition, t=inp["t"], z=inp["z"])
    assert abs(loss1 - loss0) <= 1e-6 * abs(loss0) and model.get_step() == (case["step0"] + 1, 1, 1)
    post, ema = model.read(losses.PARAM), model.read(losses.EMA)
    out["post"] = max(rel_l2(post[n], g["post:" + n]) for n in full)
    out["post_norm"] = 0.0
    for key, got in (("post", post), ("ema", ema)):
        for i, n in enumerate(names):
            scale = max(float(g[key + "_norm"][i]), 1e-30)
            out["post_norm"] = max(out["post_norm"], abs(float(got[n].double().norm()) - float(g[key + "_norm"][i])) / scale)
    print(f"{dt} {name}: " + ", ".join(f"{k}={v:.2e}" for k, v in out.items()))
    return out


@pytest.mark.parametrize("dt,name", list(STEP16_TOL))
def test_training_step16_vs_reference(dt, name):
    """ONE 16-bit p_loss step against the fp32 reference autograd, in the assertion forms of test_gpu_train_sde."""
    out = _step16_figures(dt, name)
    tol = STEP16_TOL[(dt, name)]
    for k, v in tol.items():
        assert out[k] < v, (k, out[k], v)


@pytest.mark.parametrize("name", ["train_tiny_ploss_l1", "train_tinyB_ploss_l2m"])
def test_training_step16_is_bitwise_reproducible(name):
    """Two fresh f16 trainers, the same backward pass and step: identical gradient bits and post-step state."""
    runs = []
    for _ in range(2):
        case, cfg, inp, model, ds = _setup(name, "f16")
        step_fn, _ = _fns(ds, cfg, case)
        batch = ploss_batch(inp, case)
        model.loss(batch, t=inp["t"], z=inp["z"], backward=True)
        from text2protein_amd import losses
        grads = model.read(losses.GRAD)
        step_fn(_state(model, cfg, case["step0"]), batch, condition=cfg.model.condition, t=inp["t"], z=inp["z"])
        runs.append((grads, _all_state(model)))
        del model
    for n in runs[0][0]:
        assert torch.equal(runs[0][0][n], runs[1][0][n]), n
    for w in runs[0][1]:
        for n in runs[0][1][w]:
            assert torch.equal(runs[0][1][w][n], runs[1][1][w][n]), (w, n)


# ---- 6. per-batch data ------------------------------------------------------------------------------------------------------------------
def test_ss_blocks_equal_channels_zeroed_on_the_host():
    """The masked f16 step with two dropped ss blocks against the step on a batch whose channels 4:7 were zeroed on those rows and columns
    beforehand: bitwise (the 16-bit step has a fixed order throughout)."""
    blocks = [(0, 2, 5), (2, 0, 3), (1, 4, 6)]
    drop = [1, 1, 0]
    runs = []
    for on_device in (True, False):
        case, cfg, inp, model, ds = _setup("train_tinyB_ploss_l2m", "f16")
        batch = ploss_batch(inp, case)
        if on_device:
            model.set_ss_blocks(blocks, drop=drop)
        else:
            x = batch["coords_6d"].clone()
            for (b, s, e), d in zip(blocks, drop):
                if d:
                    x[b, 4:7, s:e, :] = 0
                    x[b, 4:7, :, s:e] = 0
            assert not torch.equal(x, batch["coords_6d"])
            batch = dict(batch, coords_6d=x)
        model.set_step(case["step0"])
        loss = model.step(batch, t=inp["t"], z=inp["z"])
        runs.append((loss, _all_state(model)))
    assert runs[0][0] == runs[1][0]
    for w in runs[0][1]:
        for n in runs[0][1][w]:
            assert torch.equal(runs[0][1][w][n], runs[1][1][w][n]), (w, n)


def test_context_dropout_of_every_sample_equals_a_zero_context():
    """All-ones decisions against a zero context, at test_gpu_train_ctxdrop.py's f32 tolerance: the loss to 1e-6, pred_noise bitwise."""
    case, cfg, inp, model, ds = _setup("train_tinyB_ploss_l1m")
    x, ctx, t, z = inp["coords_6d"], inp["context"], inp["t"], inp["z"]
    kw = _masked_kw(inp, case)
    model.set_context_drop(case["B"], drop=[1] * case["B"])
    l_drop, p_drop = ds.p_loss(x, ctx, t, z, return_pred=True, **kw)
    l_zero, p_zero = ds.p_loss(x, ctx * 0, t, z, return_pred=True, **kw)
    l_plain, p_plain = ds.p_loss(x, ctx, t, z, return_pred=True, **kw)
    assert abs(l_drop - l_zero) <= 1e-6 * abs(l_zero) and torch.equal(p_drop, p_zero)
    assert not torch.equal(p_drop, p_plain)


def test_unmasked_pass_refuses_pending_ss_blocks_and_clears_them():
    from text2protein_amd import losses
    from text2protein_amd._lib import T2PError
    case, cfg, inp, model, ds = _setup("train_tinyB_ploss_l2m")
    x, ctx, t, z = inp["coords_6d"], inp["context"], inp["t"], inp["z"]
    kw = _masked_kw(inp, case)
    l0, p0 = ds.p_loss(x, ctx, t, z, backward=True, return_pred=True, **kw)
    before = _all_state(model)
    model.set_ss_blocks([(0, 2, 5)], drop=[1])
    with pytest.raises(T2PError, match="unmasked"):
        ds.p_loss(x, ctx, t, z, backward=True)
    after = _all_state(model)
    for w in before:
        for n in before[w]:
            assert torch.equal(before[w][n], after[w][n]), (w, n)
    l1, p1 = ds.p_loss(x, ctx, t, z, return_pred=True, **kw)      # the list is gone: the masked pass is the one of before
    assert abs(l1 - l0) <= 1e-6 * abs(l0) and torch.equal(p0, p1)


# ---- 7. refusals ------------------------------------------------------------------------------------------------------------------------
def test_objective_refusals_leave_the_trainer_usable():
    from text2protein_amd import sde_lib
    from text2protein_amd._lib import T2PError
    name = "train_tiny_ploss_l2"
    # after a pass
    case, cfg, inp, model, ds = _setup(name, set_objective=False)
    batch = {k: inp[k] for k in ("coords_6d", "mask_pair", "context")}
    tf = torch.tensor([0.3, 0.7])
    l0, s0 = model.loss(batch, t=tf, z=inp["z"], return_score=True)
    with pytest.raises(T2PError, match="a pass has run"):
        ds.p_loss(inp["coords_6d"], inp["context"], inp["t"], inp["z"])
    l1, s1 = model.loss(batch, t=tf, z=inp["z"], return_score=True)
    assert l0 == l1 and torch.equal(s0, s1)
    # after set_sde to VP: at the C ABI and at the Python surface
    case, cfg, inp, model, ds = _setup(name, set_objective=False)
    vp = sde_lib.VPSDE(cfg.model.beta_min, cfg.model.beta_max, cfg.model.num_scales)
    model.set_sde(vp)
    a = ds.sqrt_alpha_cumprod.contiguous()
    s = ds.sqrt_one_minus_alphas_cumprod.contiguous()
    pa, ps = C.c_void_p(a.data_ptr()), C.c_void_p(s.data_ptr())
    assert model.lib.t2p_train_set_ploss(model._h, 2, 40, pa, ps) != 0 and b"VP or sub-VP" in model.lib.t2p_last_error()
    with pytest.raises(T2PError, match="cannot switch"):
        ds.p_loss(inp["coords_6d"], inp["context"], inp["t"], inp["z"])
    assert np.isfinite(model.loss(batch, t=tf, z=inp["z"]))                      # still the VP trainer
    # the C ABI's argument checks, on a fresh trainer, change nothing: it still takes the objective afterwards
    case, cfg, inp, model, ds = _setup(name, set_objective=False)
    lib = model.lib
    for args, what in (((0, 40, pa, ps), "loss_type"), ((3, 40, pa, ps), "loss_type"), ((2, 0, pa, ps), "timesteps"),
                       ((2, (1 << 24) + 1, pa, ps), "timesteps"), ((2, 40, None, ps), "tables"), ((2, 40, pa, None), "tables"),
                       ((2, cfg.model.num_scales + 1, pa, ps), "num_scales")):
        assert lib.t2p_train_set_ploss(model._h, *args) != 0, args
        assert what in lib.t2p_last_error().decode(), (args, lib.t2p_last_error())
    g = load_golden(name)
    loss = ds.p_loss(inp["coords_6d"], inp["context"], inp["t"], inp["z"])
    assert abs(loss - float(g["loss"])) <= LOSS_TOL * abs(float(g["loss"]))
    # set_sde after set_ploss, a second call, a second, different schedule
    assert lib.t2p_train_set_sde(model._h, 0, 0.1, 20.0, None) != 0 and b"keeps it" in lib.t2p_last_error()
    assert lib.t2p_train_set_ploss(model._h, 2, 40, pa, ps) != 0 and b"keeps it" in lib.t2p_last_error()
    for sde in (vp, sde_lib.VESDE(sigma_min=cfg.model.sigma_min, sigma_max=cfg.model.sigma_max, N=cfg.model.num_scales)):
        with pytest.raises(T2PError, match="cannot switch"):
            model.set_sde(sde)
    from text2protein_amd.ddim import DiffusionSampler
    for other in (DiffusionSampler(model, timesteps=40, betas=torch.linspace(0.01, 0.1, 40)),
                  DiffusionSampler(model, timesteps=30, betas=torch.linspace(0.01, 0.2, 30)),
                  DiffusionSampler(model, timesteps=40, betas=torch.linspace(0.01, 0.2, 40), loss_type="l1")):
        with pytest.raises(T2PError, match="cannot switch"):
            other.p_loss(inp["coords_6d"], inp["context"], inp["t"].clamp(max=29), inp["z"])
    same = DiffusionSampler(model, timesteps=40, betas=torch.linspace(0.01, 0.2, 40))     # the same schedule again is no switch
    l2 = same.p_loss(inp["coords_6d"], inp["context"], inp["t"], inp["z"])
    assert l2 == loss


# ---- 8. one object trains and samples ------------------------------------------------------------------------------------------------
def test_train_then_sample_with_one_object():
    from text2protein_amd import losses
    from text2protein_amd.ddim import DiffusionSampler
    case, cfg, inp, model, _ = _setup("train_tiny_ploss_l2", set_objective=False, masked=True)
    ds = DiffusionSampler(model, timesteps=40, betas=torch.linspace(0.01, 0.2, 40), sampling_steps=5, w=0.7)
    step_fn = losses.get_ploss_step_fn(ds, train=True, optimize_fn=losses.optimization_manager(cfg), context_dropout=0.5)
    eval_fn = losses.get_ploss_step_fn(ds, train=False)
    state = _state(model, cfg, 5000)
    batch = {k: inp[k] for k in ("coords_6d", "mask_pair", "context")}
    t, z = torch.tensor([12, 30]), inp["z"]
    e0 = eval_fn(state, batch, condition=cfg.model.condition, t=t, z=z)
    seq = [step_fn(state, batch, condition=cfg.model.condition, t=t, z=z) for _ in range(30)]
    print("p_loss over 30 steps on one batch (context dropout 0.5):", " ".join(f"{v:.3f}" for v in seq))
    assert all(np.isfinite(seq)) and np.mean(seq[-5:]) < np.mean(seq[:5])
    assert state["step"] == 5030 and model.get_step() == (5030, 30, 30)
    before = model.read(losses.PARAM)
    e1 = eval_fn(state, batch, condition=cfg.model.condition, t=t, z=z)
    assert all(torch.equal(before[n], v) for n, v in model.read(losses.PARAM).items())
    other = _model(case, cfg)                          # the evaluation loss is the loss under the EMA weights (no dropout in this config)
    other.load_state_dict(model.read(losses.EMA))
    want = DiffusionSampler(other, timesteps=40, betas=torch.linspace(0.01, 0.2, 40)).p_loss(
        batch["coords_6d"], batch["context"], t, z, batch=batch)
    print(f"EMA loss {e0:.4f} -> {e1:.4f} (a trainer holding the EMA: {want:.4f})")
    assert cfg.model.dropout == 0.0 and abs(e1 - want) <= 1e-6 * abs(want) and e1 < e0
    # train.py:198-215 with the same object
    ema = state["ema"]
    shape = (2, cfg.data.num_channels, cfg.data.max_res_num, cfg.data.max_res_num)
    ema.store(model.parameters())
    ema.copy_to(model.parameters())
    sample = ds.ddim_sample(shape, inp["context"])
    ema.restore(model.parameters())
    torch.cuda.synchronize()
    assert tuple(sample.shape) == shape and bool(torch.isfinite(sample).all()) and float(sample.abs().max()) <= 1.0
    assert all(torch.equal(before[n], v) for n, v in model.read(losses.PARAM).items())
    assert np.isfinite(step_fn(state, batch, condition=cfg.model.condition, t=t, z=z)) and state["step"] == 5031
    assert np.isfinite(ds(batch["coords_6d"], batch["context"]))         # forward: t and the noise drawn on the device
