"""What the sampler's element-wise tail computes, as a dict of arrays: the norm sums of the two Langevin-norm operators, short
predictor-corrector runs of the tiny f32 model (VE / VP, plain / guided, with and without a length mask, one and two corrector steps),
one whole VP run of t2p_sampler_run and two fused DDIM runs.  tests/golden/make_golden_pc_parent.py stores compute() at the commit
before the guided and plain update kernels were folded into one set (pc_update_parent.npz); tests/test_gpu_pc_parent.py holds the
current build to those bits.

Operator inputs come from a closed-form integer hash (splitmix64 of the element index, the top 24 bits as a float32 in [-1, 1)):
integer arithmetic only, so no library's random stream or libm enters and only outputs are stored.  The runs draw their noise on the
device (Philox, seed 5) and start from _device_randn_like(., 9, 0) times the SDE's prior scale."""
import itertools

import numpy as np
import torch

F32 = np.float32
NORM_B = (1, 2, 5)
NORM_PER_SAMPLE = (7, 1280, 16385)     # element-by-element tail; 16-byte path; every partial block busy and a second trip
NORM_SCALES = (1.0, -1.7)
W, W1 = float(F32(0.7)), float(F32(1 - 0.7))
SHAPE = (2, 5, 16, 16)
L_MASK = 8                             # residues the length mask leaves free (of 16)
SEED, X_SEED, STEPS = 5, 9, 4
# name -> (sde, n_steps_each, length mask, guidance weight)
PC_RUNS = {
    "ve_n2_length": ("ve", 2, True, None),
    "vp_n1": ("vp", 1, False, None),
    "vp_n2_length": ("vp", 2, True, None),
    "ve_guided_w07": ("ve", 1, False, 0.7),
    "vp_guided_w2_length": ("vp", 1, True, 2.0),
}
EPS = {"ve": 1e-5, "vp": 1e-3}


def hash_uniform(n, salt):
    """n float32 values in [-1, 1), element i = the top 24 bits of splitmix64(i + salt * 2^32)."""
    with np.errstate(over="ignore"):
        z = np.arange(n, dtype=np.uint64) + np.uint64(salt << 32)
        z = (z + np.uint64(0x9E3779B97F4A7C15))
        z = (z ^ (z >> np.uint64(30))) * np.uint64(0xBF58476D1CE4E5B9)
        z = (z ^ (z >> np.uint64(27))) * np.uint64(0x94D049BB133111EB)
        z = z ^ (z >> np.uint64(31))
    return ((z >> np.uint64(40)).astype(np.int64) - (1 << 23)).astype(F32) / F32(1 << 23)


def norm_inputs(B, per_sample):
    n = B * per_sample
    oc = hash_uniform(n, 1) * F32(0.02)
    ou = oc + hash_uniform(n, 2) * F32(0.005)
    z = hash_uniform(n, 3) * F32(1.7)
    return [torch.from_numpy(a.reshape(B, per_sample)).cuda() for a in (oc, ou, z)]


def norm_sums(out):
    from text2protein_amd import _lib
    from text2protein_amd._lib import check, ptr, stream_ptr
    lib = _lib.load()
    for B, per_sample in itertools.product(NORM_B, NORM_PER_SAMPLE):
        oc, ou, z = norm_inputs(B, per_sample)
        ws, sums = torch.empty(B * 128, device="cuda"), torch.zeros(2, device="cuda")
        check(lib.t2p_op_langevin_norms(ptr(oc), ptr(z), B, per_sample, ptr(ws), ptr(sums), stream_ptr()))
        out[f"norms_plain_B{B}_n{per_sample}"] = sums.cpu().numpy()
        for guided, scale in itertools.product((True, False), NORM_SCALES):
            sums = torch.zeros(2, device="cuda")
            check(lib.t2p_op_guided_langevin_norms(ptr(oc), ptr(ou) if guided else None, ptr(z), B, per_sample, W, W1, scale, ptr(ws),
                                                   ptr(sums), stream_ptr()))
            out[f"norms_guided_B{B}_n{per_sample}_ou{int(guided)}_scale{scale}"] = sums.cpu().numpy()


def _model(vp, **over):
    from text2protein_amd import sde_lib, synth
    from text2protein_amd.config import tiny_config
    from text2protein_amd.model import HipScoreModel
    cfg = tiny_config(**{"model.num_scales": 40, "training.sde": "vpsde", **over}) if vp else tiny_config()
    cfg.device = "cuda"
    model = HipScoreModel(cfg, dtype="f32")
    model.load_state_dict(synth.synth_state_dict(cfg, 0))
    m = cfg.model
    sde = (sde_lib.VPSDE(beta_min=m.beta_min, beta_max=m.beta_max, N=m.num_scales) if vp
           else sde_lib.VESDE(sigma_min=m.sigma_min, sigma_max=m.sigma_max, N=m.num_scales))
    ctx = synth.synth_context(SHAPE[0], 3, m.context_dim, 0).cuda()
    return cfg, model, sde, ctx


def _start(sde, length):
    """The state the runs start from and, under the length mask, the stepper's condition."""
    from text2protein_amd import sampling
    x = sampling._device_randn_like(torch.empty(SHAPE, device="cuda"), X_SEED, 0) * sde.prior_scale()
    if not length:
        return x.contiguous(), None, None
    m = torch.zeros(SHAPE[0], SHAPE[2], SHAPE[3], device="cuda").bool()
    m[:, :L_MASK, :L_MASK] = True
    x, cmask = sampling.apply_conditions(x, {"length": m})
    x = x.float().contiguous()
    return x, cmask.to(torch.uint8).contiguous(), x.clone()


def pc_runs(out, dispatches=None):
    from text2protein_amd import sampling
    from text2protein_amd._lib import check, ptr, stream_ptr
    B = SHAPE[0]
    models = {}
    for name, (kind, n_each, length, w) in PC_RUNS.items():
        if kind not in models:
            models[kind] = _model(kind == "vp")
        cfg, model, sde, ctx = models[kind]
        st = sampling.PCStepper(model, sde, B, cfg.sampling.snr, n_each, eps=EPS[kind], seed=SEED, guidance_w=w)
        (st.set_context if w is not None else model.set_context)(ctx)
        x, mask, xi = _start(sde, length)
        st.set_condition(mask, xi)
        buf = x
        if st.guided:
            buf = torch.full((2 * B, *SHAPE[1:]), float("nan"), device="cuda")
            buf[:B] = x
        xm = torch.empty(SHAPE, device="cuda")
        st.reset(0)
        for _ in range(STEPS):
            st.step(buf, xm)
        torch.cuda.synchronize()
        out[f"pc_{name}_x"] = buf[:B].cpu().numpy()
        out[f"pc_{name}_x_mean"] = xm.cpu().numpy()
        if dispatches is not None:
            dispatches[name] = st.count_dispatches(buf, xm)
    # one whole VP run: the prior drawn on the device, x_mean of the last step returned (denoise)
    cfg, model, sde, ctx = models["vp"]
    st = sampling.PCStepper(model, sde, B, cfg.sampling.snr, eps=EPS["vp"], seed=SEED)
    model.set_context(ctx)
    x, res = torch.empty(SHAPE, device="cuda"), torch.empty(SHAPE, device="cuda")
    check(st.lib.t2p_sampler_run(st._h, ptr(x), ptr(res), 0, 0, stream_ptr()))
    torch.cuda.synchronize()
    out["vp_run"] = res.cpu().numpy()


def ddim_runs(out):
    """The fused DDIM route on the configuration of the fixture ddim_tiny_a (8 of 40 steps, eta 1, static clipping), device noise."""
    from helpers import load_golden
    from text2protein_amd import sde_lib
    from text2protein_amd.ddim import DiffusionSampler
    g = load_golden("ddim_tiny_a")
    cfg, model, _, _ = _model(True, **{"model.scale_by_sigma": bool(g["scale_by_sigma"])})
    for tag, w in (("guided", float(g["w"])), ("w1", 1.0)):
        ds = DiffusionSampler.from_sde(model, sde_lib.VPSDE(0.1, 20, 40), sampling_steps=int(g["steps"]), ddim_eta=float(g["eta"]),
                                       w=w, seed=11)
        res = ds.ddim_sample(SHAPE, torch.from_numpy(g["context"]), call_index=0)
        torch.cuda.synchronize()
        out[f"ddim_{tag}"] = res.cpu().numpy()


def compute(dispatches=None):
    out = {}
    norm_sums(out)
    pc_runs(out, dispatches)
    ddim_runs(out)
    return out
