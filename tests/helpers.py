"""Shared helpers for the parity tests."""
import os

import numpy as np
import torch

from text2protein_amd.config import tiny_config

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


def load_golden(name):
    return dict(np.load(os.path.join(GOLDEN, name + ".npz")))


def cfg_tiny():
    return tiny_config()


def cfg_tinyB():
    return tiny_config(**{"model.ch_mult": [1, 1, 2], "model.num_res_blocks": 2, "data.num_channels": 8,
                          "model.attn_resolutions": [4, 8], "model.n_heads": 2, "model.context_dim": 24,
                          "model.nf": 32})


def rel_l2(a, b):
    a = torch.as_tensor(a).double()
    b = torch.as_tensor(b).double()
    return float((a - b).norm() / b.norm().clamp_min(1e-30))


# The float32 schedule tables of tables.npz are the reference's arithmetic on the host that wrote them.  exp, log and linspace
# round differently in the last bits on other hosts (vector width, libm); the product is held to the reference arithmetic bit for bit
# on the host the test runs on (against the oracle), and to the stored tables within this relative bound (about 8 ulp).
F32_HOST_RTOL = 1e-6


def ve_g_rtol(N, sigma_min=0.01, sigma_max=100.0):
    """G = sqrt(sigma_k^2 - sigma_{k-1}^2) magnifies a relative error of the sigmas by 1 / (1 - (sigma_{k-1} / sigma_k)^2)."""
    return F32_HOST_RTOL / (1.0 - (sigma_min / sigma_max) ** (2.0 / (N - 1)))


def assert_table_close(got, want, rtol=F32_HOST_RTOL):
    got, want = np.asarray(got, np.float64), np.asarray(want, np.float64)
    assert got.shape == want.shape and np.all(want != 0)
    err = float(np.max(np.abs(got - want) / np.abs(want)))
    assert err <= rtol, f"max relative difference {err:.3e} > {rtol:.3e}"


def cfg_smallC():
    """Wide enough (64/128 channels, 32x32 maps) for the LDS-DMA GEMM kernel to be selected."""
    return tiny_config(**{"model.nf": 64, "model.ch_mult": [1, 2], "model.num_res_blocks": 1, "data.max_res_num": 32,
                          "model.attn_resolutions": [16], "model.n_heads": 4, "model.context_dim": 64,
                          "model.num_scales": 10})


# ---- BASELINE-size fixtures (tests/golden/make_golden_full.py writes them, the GPU tests read them) ----------------
# stem -> (YAML, L, N, batch of the fixture, text tokens, chains per GPU of the benchmark), BASELINE.md section 5
FULL = {
    "test_config": ("test_config.yml", 128, 1000, 2, 512, 32),
    "cond_length": ("cond_length.yml", 128, 1000, 2, 512, 32),
    "cond_length_inpainting": ("cond_length_inpainting.yml", 128, 1000, 2, 512, 16),
    "test_config_large": ("test_config_large.yml", 256, 1000, 1, 512, 16),
}
FULL_LABELS = [3, 700]     # time labels of the fixture's samples (sigma ~ 97 and ~ 0.16)


def full_inputs(cfg, B, T, seed=0):
    """x, labels and text context of the full-size fixtures: regenerated on both sides from the counter-hash
    generator, so only the score is stored."""
    from text2protein_amd import synth
    C, L = cfg.data.num_channels, cfg.data.max_res_num
    x = torch.from_numpy(synth.normal(seed, "full_x", B * C * L * L).reshape(B, C, L, L))
    labels = torch.tensor(FULL_LABELS[:B]).long()
    sig = torch.from_numpy(np.exp(np.linspace(np.log(cfg.model.sigma_max), np.log(cfg.model.sigma_min), cfg.model.num_scales)))
    x = x * sig[labels].float()[:, None, None, None]          # a state of the right magnitude for its noise level
    ctx = synth.synth_context(B, T, cfg.model.context_dim, seed + 17)
    return x, labels, ctx


class CounterNoise:
    """Stand-in for torch.randn / torch.randn_like: draw k = synth.normal(seed, "draw<k>", n).  Patched over the
    reference's draws when the 100-step fixture is made, injected through ``noise_fn`` on the HIP side."""

    def __init__(self, seed):
        self.seed, self.k = int(seed), 0

    def draw(self, shape):
        from text2protein_amd import synth
        n = int(np.prod(shape))
        z = torch.from_numpy(synth.normal(self.seed, f"draw{self.k}", n).reshape(tuple(shape)))
        self.k += 1
        return z

    def randn(self, *shape, **kw):
        if len(shape) == 1 and not isinstance(shape[0], int):
            shape = tuple(shape[0])
        return self.draw(shape)

    def randn_like(self, x, **kw):
        return self.draw(tuple(x.shape)).to(x.device)


def cfg_ss():
    return tiny_config(**{"data.num_channels": 8, "model.condition": ["length", "ss"]})


def cfg_ckpt():
    """Small enough for a committed .pth (about 1 MB with the EMA copy)."""
    return tiny_config(**{"model.nf": 8, "model.ch_mult": [4], "model.attn_resolutions": [], "data.max_res_num": 8,
                          "model.n_heads": 2, "model.context_dim": 16, "model.num_scales": 10})


# ---- training-step fixtures (tests/golden/make_golden_train.py writes them) ------------------------------------------
def cfg_train_tiny():
    """The tiny configuration in training trim: `length` condition, no dropout (the gradient check proper)."""
    return tiny_config(**{"model.condition": ["length"], "model.dropout": 0.0, "model.num_scales": 50})


def cfg_train_tinyB():
    """Up / down blocks, two attention levels, C = 8, all three conditions, Dropout_0 active with counter-based keep-masks."""
    return tiny_config(**{"model.ch_mult": [1, 1, 2], "model.num_res_blocks": 2, "data.num_channels": 8,
                          "model.attn_resolutions": [4, 8], "model.n_heads": 2, "model.context_dim": 24, "model.nf": 32,
                          "model.condition": ["length", "ss", "inpainting"], "model.dropout": 0.1, "model.num_scales": 50})


def cfg_train_cond_length():
    """BASELINE configs[2]'s model at its real size: configs/cond_length.yml, L = 128 (75.0 M parameters), dropout as shipped (0.1)."""
    from text2protein_amd.config import load_config
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    return load_config(os.path.join(root, "configs", "cond_length.yml"), **{"data.max_res_num": 128, "model.num_scales": 1000})


def cfg_train_test_config():
    """BASELINE configs[1]'s model at its real WIDTH (configs/test_config.yml: nf 256, channel multipliers up to 2, 8 heads, AttnBlockpp and
    SpatialTransformer at three resolutions, 379.5 M parameters) on L = 64 maps (six levels down to 2 x 2), dropout as shipped (0.1), no condition."""
    from text2protein_amd.config import load_config
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    return load_config(os.path.join(root, "configs", "test_config.yml"), **{"data.max_res_num": 64, "model.num_scales": 1000})


TRAIN_CASES = {   # name -> what the fixture script and the tests share; step0 = state['step'] before the update (warm-up factor step0 / 5000)
    "train_tiny": dict(config=cfg_train_tiny, seed=3, B=2, T=3, lengths=[12, 9], step0=2000, mask_info=None),
    "train_tinyB": dict(config=cfg_train_tinyB, seed=4, B=3, T=5, lengths=[16, 11, 6], step0=7000, mask_info="1:3,6:8"),
    # full size (round 4): norms + projections of all 622 tensors, whole tensors for the small ones only (the file stays ~1 MB)
    "train_cond_length": dict(config=cfg_train_cond_length, seed=5, B=1, T=16, lengths=[100], step0=9000, mask_info=None, full_size=True),
    # the other architecture family at its real width (C = 256 / 512, attention at three resolutions)
    "train_test_config": dict(config=cfg_train_test_config, seed=6, B=1, T=8, lengths=[50], step0=3000, mask_info=None, full_size=True,
                              yaml="test_config.yml"),
}


def train_inputs(cfg, case):
    """coords_6d ~ U(-1, 1) with the padding channel = the pair mask, pair masks of the given lengths, t ~ U(eps, 1), z ~ N(0, 1),
    text context: all from the counter-hash generator, regenerated identically on both sides."""
    from text2protein_amd import synth
    B, T, seed = case["B"], case["T"], case["seed"]
    C, L = cfg.data.num_channels, cfg.data.max_res_num
    x = torch.from_numpy(synth.uniform_pm1(seed, "train_coords", B * C * L * L).reshape(B, C, L, L))
    mp = torch.zeros(B, L, L).bool()
    for b, n in enumerate(case["lengths"]):
        mp[b, :n, :n] = True
    x = x * mp.unsqueeze(1)
    x[:, -1] = mp.float()
    u = torch.from_numpy((synth.uniform_pm1(seed, "train_t", B).astype(np.float64) + 1.0) / 2.0).float()
    t = u * (1.0 - 1e-5) + 1e-5                               # losses.py:106 with sde.T = 1, eps = 1e-5
    z = torch.from_numpy(synth.normal(seed, "train_z", B * C * L * L).reshape(B, C, L, L))
    out = dict(coords_6d=x, mask_pair=mp, t=t, z=z, context=synth.synth_context(B, T, cfg.model.context_dim, seed + 31))
    if case.get("mask_info"):
        m = torch.zeros(B, L)
        for r in case["mask_info"].split(","):
            a, b = r.split(":")
            m[:, int(a):int(b) + 1] = 1
        out["mask_inpaint"] = torch.logical_or(m.unsqueeze(-1), m.unsqueeze(1)).bool()
    return out


class CounterDropout:
    """Dropout_0 keep-masks from the counter-hash generator: call k keeps element i iff uniform_pm1(seed, "drop<k>", n)[i] >= 2p - 1
    (row-major over the NCHW tensor).  ``functional`` is patched over torch.nn.functional.dropout when the fixture is made
    (calls with p == 0 or in eval mode pass through uncounted: FeedForward / CrossAttention hold Dropout(0.)); ``module`` is the
    oracle's hook; ``mask(k, shape)`` gives the test the same mask to upload."""

    def __init__(self, seed, p):
        self.seed, self.p, self.k = int(seed), float(p), 0

    def mask(self, k, shape):
        from text2protein_amd import synth
        n = int(np.prod(shape))
        u = torch.from_numpy(synth.uniform_pm1(self.seed, f"drop{k}", n).reshape(tuple(shape)))
        return u >= (2.0 * self.p - 1.0)

    def module(self, h):
        keep = self.mask(self.k, h.shape)
        self.k += 1
        return h * keep / (1.0 - self.p)

    def functional(self, input, p=0.5, training=True, inplace=False):
        if not training or p == 0.0:
            return input
        assert abs(p - self.p) < 1e-12
        return self.module(input)


def projection(name, tensor, seed=99, cache=None):
    """<tensor, r> with r ~ U(-1, 1) keyed by the tensor's name: pins every element of a tensor with one stored number.
    ``cache`` (a dict) keeps r between calls: the full-size fixture projects five buffers of 75 M elements on the same vectors."""
    from text2protein_amd import synth
    v = torch.as_tensor(tensor).detach().double().reshape(-1)
    r = cache.get(name) if cache is not None else None
    if r is None:
        r = torch.from_numpy(synth.uniform_pm1(seed, name + ":proj", v.numel()))
        if cache is not None:
            cache[name] = r
    return float((v * r.double()).sum())


def check_step_against_fixture(name, g, case, cfg, inp, model, step_fn, batch, *, loss_tol, score_tol, grad_tol, param_tol, delta_tol,
                               step_batch=None, before_loss=None, before_step=None, after=None):
    """The fp32 procedure of the whole-step tests (test_gpu_train / test_gpu_train_sde / test_gpu_train_ss: test_training_step_vs_reference)
    on a model that is ready for its first pass: the loss and the score; every gradient through its norm and a random projection against
    max(norm, zero-gradient floor), the total norm, the stored tensors element by element; then ONE step through ``step_fn`` and the
    parameters, the EMA and both Adam moments the same way, the stored post-step parameters and the parameter UPDATE.  Every figure is
    printed before anything is asserted and returned.  ``delta_tol`` None: the update's rel-L2 is reported only (the ss fixtures, where
    test_gpu_train_ss explains why).  ``before_loss(model)`` / ``before_step()`` run just before the two passes; ``step_batch`` replaces
    ``batch`` in the step (the ss cases hand the reference's strings to the Python mirror there); ``after(ctx)`` runs last with the tensors
    read back (ctx: names, full, T, sd, grads, post), for checks only one fixture family makes."""
    from text2protein_amd import losses, synth
    names = [str(n) for n in g["names"]]
    assert [n for n, _ in model.param_table()] == names and len(model._keep) == int(g["n_dropout_calls"])
    if before_loss:
        before_loss(model)
    loss0, score = model.loss(batch, t=inp["t"], z=inp["z"], backward=True, return_score=True)
    out = {"score_rel_l2": rel_l2(score.cpu()[:, :, ::8, ::8] if case.get("full_size") else score.cpu(), g["score"]),
           "loss_rel": abs(loss0 - float(g["loss"])) / abs(float(g["loss"]))}
    grads = model.read(losses.GRAD)
    T = float(g["grad_total_norm"])
    got_T = float(torch.sqrt(sum((v.double() ** 2).sum() for v in grads.values())))
    floor = {"grads": 3e-5 * T, "m": 3e-6 * T, "v": 1e-12 * T * T, "post": 0.0, "ema": 0.0}
    pcache = {}

    def norms_and_projections(key, got):
        wn = wp = 0.0
        for i, n in enumerate(names):
            scale = max(float(g[key + "_norm"][i]), floor[key], 1e-30)
            wn = max(wn, abs(float(got[n].double().norm()) - float(g[key + "_norm"][i])) / scale)
            wp = max(wp, abs(projection(n, got[n], cache=pcache) - float(g[key + "_proj"][i])) / scale)
        return wn, wp

    out["grad_norm"], out["grad_proj"] = norms_and_projections("grads", grads)
    out["grad_total_rel"] = abs(got_T - T) / T
    full = [k[5:] for k in g if k.startswith("grad:")]
    out["grad_rel_l2"] = max(rel_l2(grads[n], g["grad:" + n]) for n in full)
    print(f"{name}: loss {loss0:.6f} (reference {float(g['loss']):.6f}, rel {out['loss_rel']:.1e}), score rel-L2 {out['score_rel_l2']:.1e}, "
          f"gradient norms {out['grad_norm']:.1e} / projections {out['grad_proj']:.1e} of max(norm, floor), total norm rel "
          f"{out['grad_total_rel']:.1e}, worst stored gradient rel-L2 {out['grad_rel_l2']:.1e} over {len(full)} tensors")
    assert out["loss_rel"] < loss_tol and out["score_rel_l2"] < score_tol and out["grad_rel_l2"] < grad_tol
    assert out["grad_norm"] <= grad_tol and out["grad_proj"] <= 10 * grad_tol and out["grad_total_rel"] <= grad_tol
    # the step itself
    if before_step:
        before_step()
    state = dict(model=model, optimizer=losses.get_optimizer(cfg, model.parameters()),
                 ema=losses.ExponentialMovingAverage(model.parameters(), decay=cfg.model.ema_rate), step=case["step0"])
    loss1 = step_fn(state, batch if step_batch is None else step_batch, condition=cfg.model.condition, t=inp["t"], z=inp["z"])
    assert abs(loss1 - loss0) <= 1e-6 * abs(loss0) and state["step"] == case["step0"] + 1
    assert model.get_step() == (case["step0"] + 1, 1, 1)
    post = {"post": model.read(losses.PARAM), "ema": model.read(losses.EMA), "m": model.read(losses.EXP_AVG), "v": model.read(losses.EXP_AVG_SQ)}
    worst = {}
    for key, tol in (("post", param_tol), ("ema", param_tol), ("m", grad_tol), ("v", 2 * grad_tol)):
        worst[key] = norms_and_projections(key, post[key]) + (tol,)
        out[key + "_norm"], out[key + "_proj"] = worst[key][:2]
    sd = synth.synth_state_dict(cfg, case["seed"])
    out["post_rel_l2"] = max(rel_l2(post["post"][n], g["post:" + n]) for n in full)
    out["update_rel_l2"] = max(rel_l2(post["post"][n] - sd[n], torch.from_numpy(g["post:" + n]) - sd[n]) for n in full)
    print(f"{name}: post-step parameters worst rel-L2 {out['post_rel_l2']:.1e}, parameter UPDATE worst rel-L2 {out['update_rel_l2']:.1e}; worst "
          "norm / projection error of max(norm, floor): " + ", ".join(f"{k} {wn:.1e} / {wp:.1e}" for k, (wn, wp, _) in worst.items()))
    assert all(wn <= tol and wp <= 10 * tol for wn, wp, tol in worst.values()), worst
    assert out["post_rel_l2"] < param_tol and (delta_tol is None or out["update_rel_l2"] < delta_tol)
    if after:
        after(dict(names=names, full=full, T=T, sd=sd, grads=grads, post=post))
    return out
