"""DDIM sampling with classifier-free guidance on the GPU (csrc/ddim.hip, text2protein_amd/ddim.py): the update kernel against its
formula, whole runs against the reference's own DiffusionSampler, device noise, conditions, refusals and the command line."""
import ctypes as C
import itertools
import os
import pickle
import subprocess
import sys

import numpy as np
import pytest
import torch
import yaml

from helpers import GOLDEN, cfg_ckpt, cfg_ss, load_golden, rel_l2

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
U = 2.0 ** -24
SHAPE = (2, 5, 16, 16)


def f32(v):
    return float(np.float32(v))


def bits(t):
    return t.detach().cpu().contiguous().view(torch.int32)


# ---- (a) the operator against the formula ---------------------------------------------------------------------------------
def _rows():
    """A middle and the last row of the VP schedule the run fixtures use (40 timesteps, 8 steps), for eta 0 and 1."""
    from text2protein_amd import sde_lib
    from text2protein_amd.ddim import DiffusionSampler
    out = {}
    for eta in (0.0, 1.0):
        tab = DiffusionSampler.from_sde(None, sde_lib.VPSDE(0.1, 20, 40), sampling_steps=8, ddim_eta=eta).step_table()
        for name, i in (("mid", 4), ("last", 7)):
            out[(name, eta)] = {k: f32(tab[k][i]) for k in ("sqrt_recip", "sqrt_recipm1", "sqrt_an", "c", "sigma")}
            assert tab["last"][i] == (name == "last")
    assert out[("mid", 1.0)]["sigma"] > 0.1 and out[("mid", 0.0)]["sigma"] == 0.0
    return out


@pytest.mark.parametrize("n", [1, 3, 4, 45, 1023, 1024, 1025, 2053])
def test_update_operator_against_the_formula(n):
    """t2p_op_ddim_update on every combination of {middle, last} x eta {0, 1} x clip x mask x {one, two destinations} x {eps_u,
    none} against the formula in float64 from the same float32 inputs and scalars, within
    8 * 2^-24 * (|sqrt_recip x| + |sqrt_recipm1 eps| + |x0 sqrt_an| + |c eps| + |sigma z|) per element (a few roundings of each
    term).  The bound has no term for cancellation inside the guidance sum w eps_c + (1 - w) eps_u, so eps_u is eps_c plus a
    quarter-size perturbation -- the two predictions of a guided run differ by the text's influence, they do not cancel -- and
    w = 0.7 then keeps |w eps_c| + |(1 - w) eps_u| within 1.3 |eps|.  n sits below, at and across the vector width (4) and the
    block (256 threads x 4); an odd n makes the second destination, which starts at element n of the same allocation, unaligned."""
    from text2protein_amd import _lib
    from text2protein_amd._lib import check, ptr, stream_ptr
    lib = _lib.load()
    gen = torch.Generator().manual_seed(100 + n)
    x, ec, z = (torch.randn(n, generator=gen) for _ in range(3))
    eu = ec + 0.25 * torch.randn(n, generator=gen)
    x = x * 0.6                                      # about a third of the clean-sample predictions land on the clamp
    xi = torch.randn(n, generator=gen)
    mask = (torch.rand(n, generator=gen) < 0.6).to(torch.uint8)
    if n > 1:
        mask[0], mask[-1] = 0, 1
    w, w1 = f32(0.7), f32(1 - 0.7)
    dev = {k: v.cuda() for k, v in dict(x=x, ec=ec, eu=eu, z=z, xi=xi, mask=mask).items()}
    znan = torch.full((n,), float("nan"), device="cuda")
    rows = _rows()
    worst = 0.0
    SENT = 12345.0
    for (step, eta), clip, use_mask, two, guided in itertools.product(rows, (1, 0), (False, True), (False, True), (True, False)):
        r, last = rows[(step, eta)], step == "last"
        buf = torch.full((2 * n + 8,), SENT, device="cuda")
        x0o = torch.full((n + 8,), SENT, device="cuda")
        check(lib.t2p_op_ddim_update(ptr(dev["x"]), ptr(dev["ec"]), ptr(dev["eu"]) if guided else None, ptr(znan if last else dev["z"]),
                                     ptr(dev["mask"]) if use_mask else None, ptr(dev["xi"]) if use_mask else None, ptr(buf),
                                     ptr(buf[n:]) if two else None, ptr(x0o), n, w, w1, r["sqrt_recip"], r["sqrt_recipm1"],
                                     r["sqrt_an"], r["c"], r["sigma"], clip, int(last), 0, 0, stream_ptr()))
        got, got0 = buf.cpu().double(), x0o.cpu().double()
        X, EC, EU, Z = x.double(), ec.double(), eu.double(), z.double()
        eps = w * EC + w1 * EU if guided else EC
        x0 = r["sqrt_recip"] * X - r["sqrt_recipm1"] * eps
        if clip:
            x0 = x0.clamp(-1, 1)
        want = x0 if last else x0 * r["sqrt_an"] + r["c"] * eps + r["sigma"] * Z
        bound0 = 8 * U * ((r["sqrt_recip"] * X).abs() + (r["sqrt_recipm1"] * eps).abs())
        bound = bound0 + (0 if last else 8 * U * ((x0 * r["sqrt_an"]).abs() + (r["c"] * eps).abs() + (r["sigma"] * Z).abs()))
        free = mask.bool() if use_mask else torch.ones(n, dtype=torch.bool)
        tag = (n, step, eta, clip, use_mask, two, guided)
        assert torch.isfinite(got[:n]).all(), tag                      # the last step reads no z: a buffer of NaNs leaves no trace
        ratio = ((got[:n] - want).abs() / bound.clamp_min(1e-300))[free]
        worst = max(worst, float(ratio.max()) if ratio.numel() else 0.0)
        assert bool(((got[:n] - want).abs() <= bound)[free].all()), (tag, float(ratio.max()))
        assert bool(((got0[:n] - x0).abs() <= bound0).all()), tag      # the clean-sample prediction, masked or not
        if use_mask:                                                   # frozen entries: x_initial bit for bit
            assert torch.equal(bits(buf[:n])[~free], bits(xi)[~free]), tag
        if two:
            assert torch.equal(bits(buf[n:2 * n]), bits(buf[:n])), tag
        assert bool((buf[2 * n if two else n:] == SENT).all()) and bool((x0o[n:] == SENT).all()), tag      # nothing past the end
    print(f"n = {n}: worst |got - want| / bound over {len(rows) * 16} launches = {worst:.3f}")
    # in place (x_out == x) and at w = 2 (fixture b's weight; w and 1 - w exact)
    xin = dev["x"].clone()
    r = rows[("mid", 1.0)]
    check(lib.t2p_op_ddim_update(ptr(xin), ptr(dev["ec"]), ptr(dev["eu"]), ptr(dev["z"]), None, None, ptr(xin), None, None, n, 2.0, -1.0,
                                 r["sqrt_recip"], r["sqrt_recipm1"], r["sqrt_an"], r["c"], r["sigma"], 1, 0, 0, 0, stream_ptr()))
    eps = 2.0 * ec.double() - eu.double()
    x0 = (r["sqrt_recip"] * x.double() - r["sqrt_recipm1"] * eps).clamp(-1, 1)
    want = x0 * r["sqrt_an"] + r["c"] * eps + r["sigma"] * z.double()
    bound = 8 * U * ((r["sqrt_recip"] * x.double()).abs() + (r["sqrt_recipm1"] * eps).abs() + (x0 * r["sqrt_an"]).abs()
                     + (r["c"] * eps).abs() + (r["sigma"] * z.double()).abs())
    assert bool(((xin.cpu().double() - want).abs() <= bound).all())


def test_update_operator_refuses_bad_arguments():
    from text2protein_amd import _lib
    from text2protein_amd._lib import T2PError, check, ptr, stream_ptr
    lib = _lib.load()
    a = torch.zeros(8, device="cuda")
    m = torch.ones(8, dtype=torch.uint8, device="cuda")
    for args in ((None, ptr(a), 8, 1, 0, None), (ptr(a), None, 8, 1, 0, None), (ptr(a), ptr(a), 0, 1, 0, None),
                 (ptr(a), ptr(a), 8, 2, 0, None), (ptr(a), ptr(a), 8, 1, 3, None), (ptr(a), ptr(a), 8, 1, 0, ptr(m))):
        x, e, n, clip, last, mask = args
        with pytest.raises(T2PError):
            check(lib.t2p_op_ddim_update(x, e, None, None, mask, None, ptr(a), None, None, n, 1.0, 0.0, 1.0, 0.0, 1.0, 0.0, 0.0,
                                         clip, last, 0, 0, stream_ptr()))


# ---- (b), (c) whole runs against the reference ---------------------------------------------------------------------------------
def _fixture_model(g, dtype="f32"):
    from text2protein_amd import synth
    from text2protein_amd.config import tiny_config
    from text2protein_amd.model import HipScoreModel
    cfg = tiny_config(**{"model.num_scales": 40, "training.sde": "vpsde", "model.scale_by_sigma": bool(g["scale_by_sigma"])})
    cfg.device = "cuda"
    model = HipScoreModel(cfg, dtype=dtype)
    model.load_state_dict(synth.synth_state_dict(cfg, 0))
    return cfg, model


def _sampler(g, model, **kw):
    from text2protein_amd import sde_lib
    from text2protein_amd.ddim import DiffusionSampler
    return DiffusionSampler.from_sde(model, sde_lib.VPSDE(0.1, 20, 40), sampling_steps=int(g["steps"]), ddim_eta=float(g["eta"]),
                                     w=float(g["w"]), **kw)


def _run(g, ds, **kw):
    it = iter([torch.from_numpy(z) for z in g["noise"]])
    trace = []
    out = ds.ddim_sample(SHAPE, torch.from_numpy(g["context"]), noise_fn=lambda shp: next(it), trace=trace, **kw)
    torch.cuda.synchronize()
    assert next(it, None) is None                       # the prior and one draw per step but the last: all consumed
    return out.cpu(), [t.cpu() for t in trace]


@pytest.mark.parametrize("name", ["ddim_tiny_a", "ddim_tiny_b", "ddim_tiny_c", "ddim_tiny_sbs"])
def test_runs_match_the_reference_through_both_routes(name):
    """The reference's own DiffusionSampler on the CPU (tests/golden/make_golden_ddim.py) against the f32 engine on the same noise:
    final rel-L2 <= 1e-4 -- what the 40-step f32 VP run is held to in test_vp_sde_route_matches_reference_run -- for a fixture whose
    stored sensitivity (rel-L2 change of the sample per relative change of the network output) is <= 10, scaled linearly with
    the sensitivity above that (the error of a run is proportional to it).  The clean-sample prediction of step k is
    sqrt_recip x - sqrt_recipm1 eps: evaluation error enters it times sqrt_recipm1[t_k] (148 at t = 39), so it is held to the
    same bound times max(1, sqrt_recipm1[t_k]); a wrong coefficient or time label misses that by orders of magnitude and the
    printed line says at which step.  The fused route (one evaluation at 2B) and the ops route (two at B) agree within the bound.
    Measured on an MI355X: see DESIGN.md, 'DDIM sampling with classifier-free guidance'."""
    g = load_golden(name)
    bound = 1e-4 * max(1.0, float(g["sensitivity"]) / 10.0)
    cfg, model = _fixture_model(g)
    ds = _sampler(g, model)
    srm1 = ds.step_table()["sqrt_recipm1"]
    outs, ok = {}, True
    for route, force in (("fused", False), ("ops", True)):
        out, trace = _run(g, ds, force_ops=force)
        outs[route] = out
        assert len(trace) == int(g["steps"]) and model.pool_reclaimed() == 0
        e = rel_l2(out, g["sample"])
        e0 = [rel_l2(t, g["x0"][k]) for k, t in enumerate(trace)]
        print(f"{name} ({route}): final rel-L2 vs reference {e:.3e} (bound {bound:.2e}, sensitivity {float(g['sensitivity']):.3g}); "
              "x0 per step " + " ".join(f"{v:.1e}" for v in e0))
        ok = ok and e <= bound and all(v <= bound * max(1.0, srm1[k]) for k, v in enumerate(e0))
        assert torch.equal(trace[-1], out)              # the last step returns the clean sample
        assert float(out.abs().max()) <= 1.0
    between = rel_l2(outs["fused"], outs["ops"])
    print(f"{name}: fused vs ops rel-L2 {between:.3e}")
    assert ok and between <= bound


# rel-L2 of the final sample against the reference fixture a, measured on an MI355X on the first GPU run of this test (gfx950,
# ROCm 7.2; recorded in DESIGN.md, 'DDIM sampling with classifier-free guidance'); the kernels are deterministic, the factor 2
# below only covers compiler and library drift
MEASURED_16BIT = {"f16": 1.572e-3, "bf16": 1.043e-2}


@pytest.mark.parametrize("dtype", ["f16", "bf16"])
def test_16bit_engines_on_fixture_a(dtype):
    g = load_golden("ddim_tiny_a")
    cfg, model = _fixture_model(g, dtype)
    out, trace = _run(g, _sampler(g, model))
    e = rel_l2(out, g["sample"])
    print(f"ddim_tiny_a on the {dtype} engine: final rel-L2 vs reference {e:.3e} (measured figure {MEASURED_16BIT[dtype]})")
    assert torch.isfinite(out).all() and float(out.abs().max()) <= 1.0          # the last step clips
    assert all(torch.isfinite(t).all() and float(t.abs().max()) <= 1.0 for t in trace)
    assert e <= 2 * MEASURED_16BIT[dtype]


# ---- (d) device noise ----------------------------------------------------------------------------------------------------------
def test_device_noise_is_reproducible_and_keyed_by_the_call():
    g = load_golden("ddim_tiny_a")
    cfg, model = _fixture_model(g)
    ds = _sampler(g, model, seed=11)
    ctx = torch.from_numpy(g["context"])
    a = ds.ddim_sample(SHAPE, ctx, call_index=0)
    b = ds.ddim_sample(SHAPE, ctx, call_index=0)
    c = ds.ddim_sample(SHAPE, ctx, call_index=1)
    d = ds.ddim_sample(SHAPE, ctx)                       # the sampler's own counter: the first un-pinned call is call 0
    o = ds.ddim_sample(SHAPE, ctx, call_index=0, force_ops=True)
    assert torch.isfinite(a).all() and torch.equal(bits(a), bits(b)) and torch.equal(bits(a), bits(d))
    assert not torch.equal(a, c) and rel_l2(a.cpu(), c.cpu()) > 1e-2
    assert rel_l2(o.cpu(), a.cpu()) <= 1e-4              # the same Philox draws through the ops route


def test_fused_step_with_device_noise_equals_the_operator_fed_philox():
    """One fused step (the draw made inside the update kernel) against t2p_op_ddim_update on the same network outputs with
    z = t2p_op_philox_normal(seed, draw index): bit for bit, for the first step (draw 1) and a later one (draw 3)."""
    from text2protein_amd import _lib
    from text2protein_amd._lib import check, ptr, stream_ptr
    from text2protein_amd.ddim import DDIMStepper
    lib = _lib.load()
    g = load_golden("ddim_tiny_a")
    cfg, model = _fixture_model(g)
    ds = _sampler(g, model)
    tab = ds.step_table()
    B, n, seed = SHAPE[0], int(np.prod(SHAPE)), 987654321
    ctx = torch.from_numpy(g["context"]).cuda()
    prior = torch.from_numpy(g["noise"][0]).cuda()
    st = DDIMStepper(model, ds, B, True, seed)
    w = float(g["w"])
    for k in (0, 2):
        st.set_context(ctx)
        st.reset(k)
        x = torch.cat([prior, torch.zeros_like(prior)]).contiguous()         # the step itself fills the second half
        x0 = torch.empty_like(prior)
        st.step(x, x0)
        # the same evaluation through the model: [x ; x] under [ctx ; 0] at batch 2B
        eps = model(torch.cat([prior, prior]), torch.full((2 * B,), tab["t"][k], dtype=torch.long), torch.cat([ctx, ctx * 0]))
        z = torch.empty_like(prior)
        check(lib.t2p_op_philox_normal(ptr(z), n, seed, k + 1, stream_ptr()))
        want, want0 = torch.empty_like(prior), torch.empty_like(prior)
        check(lib.t2p_op_ddim_update(ptr(prior), ptr(eps[:B]), ptr(eps[B:]), ptr(z), None, None, ptr(want), None, ptr(want0), n,
                                     w, 1 - w, tab["sqrt_recip"][k], tab["sqrt_recipm1"][k], tab["sqrt_an"][k], tab["c"][k],
                                     tab["sigma"][k], 1, 0, 0, 0, stream_ptr()))
        assert tab["sigma"][k] > 0 and torch.isfinite(want).all()
        assert torch.equal(bits(x[:B]), bits(want)) and torch.equal(bits(x[B:]), bits(want)) and torch.equal(bits(x0), bits(want0))


# ---- (e) conditions ------------------------------------------------------------------------------------------------------------
def test_length_condition_freezes_its_entries_bit_for_bit():
    from text2protein_amd import sde_lib, synth
    from text2protein_amd.config import tiny_config
    from text2protein_amd.ddim import DiffusionSampler
    from text2protein_amd.model import HipScoreModel
    from text2protein_amd.sampling import apply_conditions
    base = cfg_ss()
    cfg = tiny_config(**{"data.num_channels": base.data.num_channels, "model.condition": list(base.model.condition),
                         "model.num_scales": 40, "training.sde": "vpsde"})
    cfg.device = "cuda"
    model = HipScoreModel(cfg, dtype="f32")
    model.load_state_dict(synth.synth_state_dict(cfg, 1))
    B, Cn, L = 2, cfg.data.num_channels, cfg.data.max_res_num
    shape = (B, Cn, L, L)
    m = torch.zeros(B, L, L).bool()
    m[0, :12, :12] = True
    m[1, :7, :7] = True
    ctx = synth.synth_context(B, 3, cfg.model.context_dim, 1)
    gen = torch.Generator().manual_seed(5)
    draws = [torch.randn(shape, generator=gen) for _ in range(6)]
    x_init, cmask = apply_conditions(draws[0].clone(), {"length": m})
    frozen = ~cmask
    assert 0.3 < float(frozen.float().mean()) < 0.9
    ds = DiffusionSampler.from_sde(model, sde_lib.VPSDE(0.1, 20, 40), sampling_steps=6, ddim_eta=1.0, w=0.7)
    for force in (False, True):
        it = iter(draws)
        trace = []
        out = ds.ddim_sample(shape, ctx, condition={"length": m.cuda()}, noise_fn=lambda s: next(it), force_ops=force, trace=trace).cpu()
        assert torch.isfinite(out).all()
        assert torch.equal(bits(out)[frozen], bits(x_init)[frozen])
        assert torch.equal(out[:, -1], m.float())                         # the padding channel carries the length mask
        assert not torch.equal(out[cmask], x_init[cmask])


def test_all_ones_mask_reproduces_the_unconditioned_run():
    g = load_golden("ddim_tiny_a")
    cfg, model = _fixture_model(g)
    ds = _sampler(g, model)
    ones = {"inpainting": {"mask_inpaint": torch.ones(SHAPE[0], 16, 16).bool(), "coords_6d": torch.full(SHAPE, 7.0)}}
    for force in (False, True):
        plain, _ = _run(g, ds, force_ops=force)
        cond, _ = _run(g, ds, force_ops=force, condition=ones)
        assert torch.equal(bits(plain), bits(cond))


# ---- (f) refusals --------------------------------------------------------------------------------------------------------------
def test_refusals_change_nothing():
    from text2protein_amd import _lib, synth
    from text2protein_amd._lib import DdimConfig, DdimStepRow, T2PError, check
    from text2protein_amd.config import tiny_config
    from text2protein_amd.ddim import DDIMStepper
    from text2protein_amd.model import HipScoreModel
    g = load_golden("ddim_tiny_a")
    cfg, model = _fixture_model(g)
    ds = _sampler(g, model)
    B, S = SHAPE[0], int(g["steps"])
    ctx = torch.from_numpy(g["context"]).cuda()
    st = DDIMStepper(model, ds, B)
    x = torch.randn(2 * B, *SHAPE[1:], device="cuda")
    with pytest.raises(T2PError, match="set_context"):
        st.step(x)                                        # no context yet
    with pytest.raises(T2PError, match="cfg.batch"):
        st.set_context(torch.cat([ctx, ctx[:1]]))         # batch 3 on a sampler made for 2
    with pytest.raises(T2PError, match="set_context"):
        st.step(x)                                        # ... and the refused call set nothing
    st.set_context(ctx)
    for bad in (-1, S):
        with pytest.raises(T2PError, match="step out of range"):
            st.reset(bad)
    # a complete run through t2p_ddim_run, then one step more
    out = torch.empty(SHAPE, device="cuda")
    st.run(x, out)
    torch.cuda.synchronize()
    assert model.pool_reclaimed() == 0 and torch.isfinite(out).all() and torch.equal(out, x[:B])
    before = x.clone()
    with pytest.raises(T2PError, match="beyond the step table"):
        st.step(x)
    torch.cuda.synchronize()
    assert torch.equal(bits(x), bits(before))
    # t2p_ddim_run draws its own prior (draw 0 of the seed) when none is given: equal to the Python route on device noise
    st.set_seed(77)
    st.run(x, out, prior_given=False)
    ds77 = _sampler(g, model, seed=77)
    assert torch.equal(bits(out), bits(ds77.ddim_sample(SHAPE, ctx, call_index=0)))
    # refused at creation
    lib = _lib.load()
    tab = ds.step_table()

    def create(engine, eta=1.0, steps=S, t0=None, timesteps=40, batch=B):
        rows = (DdimStepRow * max(steps, 1))()
        for i in range(max(steps, 1)):
            for k in ("t", "sqrt_recip", "sqrt_recipm1", "sqrt_an", "c", "sigma", "last"):
                setattr(rows[i], k, tab[k][min(i, S - 1)])
        if t0 is not None:
            rows[0].t = t0
        c = DdimConfig()
        c.timesteps, c.sampling_steps, c.eta, c.w, c.clip, c.batch, c.seed = timesteps, steps, eta, 0.7, 1, batch, 0
        h = C.c_void_p()
        check(lib.t2p_ddim_create(engine, C.byref(c), rows, C.byref(h)))
        lib.t2p_ddim_destroy(h)

    create(model._h)                                      # the good one is accepted
    for kw in (dict(eta=-0.1), dict(eta=1.5), dict(eta=float("nan")), dict(steps=0), dict(t0=-1), dict(t0=40), dict(timesteps=41),
               dict(batch=0)):
        with pytest.raises(T2PError):
            create(model._h, **kw)
    raw = HipScoreModel(cfg, dtype="f32")                 # weights not loaded: the engine is not finalized
    with pytest.raises(T2PError, match="finalize"):
        create(raw._h)
    # the engine still evaluates after all of that
    out2, _ = _run(g, ds)
    assert rel_l2(out2, g["sample"]) <= 1e-4


# ---- (g) command line ----------------------------------------------------------------------------------------------------------
def _cli(tmp_path, sde, tag, *flags):
    cfg = cfg_ckpt()
    cfg.training.sde = sde
    cfg.model.beta_max = 5.0                  # 10 scales: beta_max / N must stay below 1 for the VP schedule
    cfg_path = tmp_path / f"ckpt_{sde}.yml"
    with open(cfg_path, "w") as f:
        yaml.safe_dump(yaml.safe_load(__import__("json").dumps(cfg)), f)
    out = tmp_path / tag
    cmd = [sys.executable, os.path.join(ROOT, "sampling_6d.py"), str(cfg_path), os.path.join(GOLDEN, "tiny_checkpoint.pth"),
           "--batch_size", "2", "--context_tokens", "4", "--outdir", str(out), *flags]
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=600, cwd=str(tmp_path))
    assert r.returncode == 0, r.stdout + r.stderr
    samples = {}
    for name in sorted(os.listdir(out)):
        with open(out / name, "rb") as f:
            samples[name] = pickle.load(f)
    return samples, r.stdout


def test_cli_ddim_writes_the_same_files_as_the_pc_route(tmp_path):
    ddim, log = _cli(tmp_path, "vpsde", "ddim", "--dtype", "f32", "--sampler", "ddim", "--ddim_steps", "4", "--guidance_w", "0.7")
    pc, _ = _cli(tmp_path, "vpsde", "pc", "--dtype", "f32")
    assert sorted(ddim) == sorted(pc) == ["sampled_0.pkl", "sampled_1.pkl"]
    for k in ddim:
        assert isinstance(ddim[k], torch.Tensor) and ddim[k].shape == pc[k].shape == (1, 5, 8, 8) and ddim[k].dtype == pc[k].dtype
        assert torch.isfinite(ddim[k]).all() and float(ddim[k].abs().max()) <= 1.0
    assert "(8 score evaluations per chain)" in log       # 4 steps, guided: two per step


def test_cli_default_route_is_unchanged(tmp_path):
    """Without --sampler the command runs the PC loop as before: its samples equal, bit for bit, the ones the commit before the
    DDIM sampler wrote for the same command on an MI355X (tests/golden/cli_default_parent.npz), and --sampler pc is the same."""
    g = load_golden("cli_default_parent")
    default, _ = _cli(tmp_path, "vesde", "default", "--dtype", "f32")
    named, _ = _cli(tmp_path, "vesde", "named", "--dtype", "f32", "--sampler", "pc")
    assert sorted(default) == sorted(named) == ["sampled_0.pkl", "sampled_1.pkl"]
    for k in default:
        assert torch.equal(bits(default[k]), bits(named[k]))
        assert torch.equal(bits(default[k]), bits(torch.from_numpy(g[k])))
