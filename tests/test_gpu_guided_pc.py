"""Classifier-free guidance in the predictor-corrector sampler on the GPU: the three guided kernels against their formula, whole
runs against the reference's own pc_sampler on a guidance wrapper (tests/golden/make_golden_guided_pc.py), device noise, weight edge
cases, conditions, graph replay, the norm all-reduce hook, refusals and the command line."""
import ctypes as C
import itertools
import os
import pickle
import subprocess
import sys
import threading

import numpy as np
import pytest
import torch
import yaml

import guided_oracle as GO
from helpers import GOLDEN, cfg_ckpt, load_golden, rel_l2
from oracle import philox

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F32 = np.float32
SENT = 12345.0
# rel-L2 of the final sample per compute dtype: SAMPLE_TOL of test_gpu_sampler.py (the unguided tiny runs)
SAMPLE_TOL = {"f32": 1e-5, "f16": 1e-3, "bf16": 1e-2}


def bits(t):
    return t.detach().cpu().contiguous().view(torch.int32)


# ---- the float32 formula on the host --------------------------------------------------------------------------------------
def fma32(a, b, c):
    """fmaf(a, b, c) of float32 arrays, exactly: the product is exact in float64, the sum is rounded to odd there (TwoSum gives
    its error), and a round-to-odd 53-bit value rounds to 24 bits as the exact one does."""
    p = a.astype(np.float64) * b.astype(np.float64)
    c = np.broadcast_to(np.asarray(c, np.float64), p.shape)
    s = p + c
    bb = s - p
    err = (p - (s - bb)) + (c - bb)
    raw = s.view(np.int64).copy()
    fix = (err != 0) & ((raw & 1) == 0)
    away = (err > 0) == (s > 0)                      # the exact sum lies further from zero than s
    raw = np.where(fix, np.where(away, raw + 1, raw - 1), raw)
    return raw.view(np.float64).astype(F32)


def guided_s(oc, ou, w, w1, scale):
    """s = scale (w o_c + w1 o_u), each product and sum rounded to float32 in this order (numpy float32 arithmetic rounds each)."""
    o = oc if ou is None else F32(w) * oc + F32(w1) * ou
    return (o * F32(scale)).astype(F32)


def langevin_formula(x, s, z, sums, batch_total, snr, alpha):
    gn, nn = F32(sums[0]) / F32(batch_total), F32(sums[1]) / F32(batch_total)
    r = F32(snr) * nn / gn
    step = r * r * F32(2) * F32(alpha)
    nscale = np.sqrt(step * F32(2))
    assert step.dtype == F32 and nscale.dtype == F32
    xm = fma32(np.full_like(s, step), s, x)
    return fma32(np.full_like(z, nscale), z, xm), xm


def predictor_formula(x, s, z, G, x_coef, pf):
    G = F32(G)
    g2 = G * G * F32(0.5 if pf else 1.0)
    gz = F32(0.0) if pf else G
    xm = F32(x_coef) * x + g2 * s                      # two rounded products, one rounded sum
    return fma32(np.full_like(z, gz), z, xm), xm


def test_the_host_fma_is_exact():
    """fma32 against rational arithmetic on values built to sit on float64 and float32 rounding ties."""
    from fractions import Fraction
    rng = np.random.default_rng(3)
    a = rng.standard_normal(400).astype(F32)
    b = rng.standard_normal(400).astype(F32)
    c = (rng.standard_normal(400) * 2.0 ** rng.integers(-30, 30, 400)).astype(F32)
    c[:50] = (-(a[:50].astype(np.float64) * b[:50].astype(np.float64))).astype(F32)          # heavy cancellation
    got = fma32(a, b, c)
    for i in range(400):
        exact = Fraction(float(a[i])) * Fraction(float(b[i])) + Fraction(float(c[i]))
        lo = np.nextafter(got[i], F32(-np.inf))
        hi = np.nextafter(got[i], F32(np.inf))
        d = abs(Fraction(float(got[i])) - exact)
        assert d <= abs(Fraction(float(lo)) - exact) and d <= abs(Fraction(float(hi)) - exact), i


# ---- 1. operators against the formula ---------------------------------------------------------------------------------------
def _op_inputs(n):
    gen = torch.Generator().manual_seed(300 + n)
    x, oc, z, xi = (torch.randn(n, generator=gen) for _ in range(4))
    x = x * 30
    ou = oc + 0.25 * torch.randn(n, generator=gen)
    mask = (torch.rand(n, generator=gen) < 0.6).to(torch.uint8)
    if n > 1:
        mask[0], mask[-1] = 0, 1
    return dict(x=x, oc=oc, ou=ou, z=z, xi=xi, mask=mask)


@pytest.mark.parametrize("n", [1, 3, 4, 45, 1023, 1024, 1025, 2053])
def test_update_operators_are_the_formula_bit_for_bit(n):
    """t2p_op_guided_langevin_update / t2p_op_guided_predictor over {o_u, none} x mask x {one, two destinations} x VP scalars
    (scale, alpha, x_coef) on and off x probability_flow, bit for bit against the float32 formula evaluated on the host in the
    stated rounding order.  n sits below, at and across the access width (4) and the block (256 threads x 4); an odd n makes the
    second destination, which starts at element n of the same allocation, unaligned (the element-by-element branch).  Then x_out
    aliasing x, o_u NULL against t2p_op_langevin_update / t2p_op_predictor, and those two (the same kernels since the plain and
    guided families became one) against the formula with s = o_c."""
    from text2protein_amd import _lib
    from text2protein_amd._lib import check, ptr, stream_ptr
    lib = _lib.load()
    host = _op_inputs(n)
    dev = {k: v.cuda() for k, v in host.items()}
    h = {k: v.numpy() for k, v in host.items()}
    w, w1 = float(F32(0.7)), float(F32(1 - 0.7))
    sums = torch.tensor([3.25, 71.5], device="cuda")
    snr, bt = 0.17, 2.0
    free = h["mask"].astype(bool)
    for guided, use_mask, two, vp in itertools.product((True, False), (False, True), (False, True), (False, True)):
        scale, alpha, xc = (-1.7, 0.93, 1.031) if vp else (1.0, 1.0, 1.0)
        s = guided_s(h["oc"], h["ou"] if guided else None, w, w1, scale)
        launches = [("langevin", None, langevin_formula(h["x"], s, h["z"], [3.25, 71.5], bt, snr, alpha))]
        launches += [("predictor", pf, predictor_formula(h["x"], s, h["z"], 3.7, xc, pf)) for pf in (0, 1)]
        for kind, pf, (want, want_m) in launches:
            buf = torch.full((2 * n + 8,), SENT, device="cuda")
            xmo = torch.full((n + 8,), SENT, device="cuda")
            common = (ptr(dev["x"]), ptr(dev["oc"]), ptr(dev["ou"]) if guided else None, ptr(dev["z"]),
                      ptr(dev["mask"]) if use_mask else None, ptr(dev["xi"]) if use_mask else None, ptr(buf),
                      ptr(buf[n:]) if two else None, ptr(xmo), n, w, w1, scale)
            if kind == "langevin":
                check(lib.t2p_op_guided_langevin_update(*common, ptr(sums), bt, snr, alpha, stream_ptr()))
            else:
                check(lib.t2p_op_guided_predictor(*common, 3.7, xc, pf, stream_ptr()))
            tag = (n, kind, pf, guided, use_mask, two, vp)
            want = np.where(free, want, h["xi"]) if use_mask else want
            assert torch.equal(bits(buf[:n]), bits(torch.from_numpy(want))), tag
            assert torch.equal(bits(xmo[:n]), bits(torch.from_numpy(want_m))), tag          # x_mean is not masked
            if two:
                assert torch.equal(bits(buf[n:2 * n]), bits(buf[:n])), tag
            assert bool((buf[2 * n if two else n:] == SENT).all()) and bool((xmo[n:] == SENT).all()), tag      # nothing past the end
    # x_out aliasing x, x_mean_out optional
    s = guided_s(h["oc"], h["ou"], w, w1, 1.0)
    for kind in ("langevin", "predictor"):
        xin = dev["x"].clone()
        common = (ptr(xin), ptr(dev["oc"]), ptr(dev["ou"]), ptr(dev["z"]), None, None, ptr(xin), None, None, n, w, w1, 1.0)
        if kind == "langevin":
            check(lib.t2p_op_guided_langevin_update(*common, ptr(sums), bt, snr, 1.0, stream_ptr()))
            want = langevin_formula(h["x"], s, h["z"], [3.25, 71.5], bt, snr, 1.0)[0]
        else:
            check(lib.t2p_op_guided_predictor(*common, 3.7, 1.0, 0, stream_ptr()))
            want = predictor_formula(h["x"], s, h["z"], 3.7, 1.0, 0)[0]
        assert torch.equal(bits(xin), bits(torch.from_numpy(want))), (n, kind, "in place")
    # o_u NULL: the existing operators, bit for bit
    for use_mask in (False, True):
        m, xi = (ptr(dev["mask"]), ptr(dev["xi"])) if use_mask else (None, None)
        a, am, b, bm = (torch.empty(n, device="cuda") for _ in range(4))
        check(lib.t2p_op_guided_langevin_update(ptr(dev["x"]), ptr(dev["oc"]), None, ptr(dev["z"]), m, xi, ptr(a), None, ptr(am), n, w, w1,
                                                1.0, ptr(sums), bt, snr, 0.93, stream_ptr()))
        check(lib.t2p_op_langevin_update(ptr(dev["x"]), ptr(dev["oc"]), ptr(dev["z"]), m, xi, ptr(b), ptr(bm), n, ptr(sums), bt, snr, 0.93,
                                         stream_ptr()))
        assert torch.equal(bits(a), bits(b)) and torch.equal(bits(am), bits(bm)), (n, use_mask)
        for pf in (0, 1):
            check(lib.t2p_op_guided_predictor(ptr(dev["x"]), ptr(dev["oc"]), None, ptr(dev["z"]), m, xi, ptr(a), None, ptr(am), n, w, w1,
                                              1.0, 3.7, 1.0, pf, stream_ptr()))
            check(lib.t2p_op_predictor(ptr(dev["x"]), ptr(dev["oc"]), ptr(dev["z"]), m, xi, ptr(b), ptr(bm), n, 3.7, pf, stream_ptr()))
            assert torch.equal(bits(a), bits(b)) and torch.equal(bits(am), bits(bm)), (n, use_mask, pf)
    # ... which now compares one kernel with itself: t2p_op_langevin_update / t2p_op_predictor against the formula with s = o_c,
    # with and without the mask, and x_initial without a mask (accepted and ignored: the no-mask result)
    plain = [("langevin", None, langevin_formula(h["x"], h["oc"], h["z"], [3.25, 71.5], bt, snr, 0.93))]
    plain += [("predictor", pf, predictor_formula(h["x"], h["oc"], h["z"], 3.7, 1.0, pf)) for pf in (0, 1)]
    for (kind, pf, (want, want_m)), (use_mask, use_xi) in itertools.product(plain, ((False, False), (True, True), (False, True))):
        m, xi = ptr(dev["mask"]) if use_mask else None, ptr(dev["xi"]) if use_xi else None
        b, bm = torch.full((n + 8,), SENT, device="cuda"), torch.full((n + 8,), SENT, device="cuda")
        if kind == "langevin":
            check(lib.t2p_op_langevin_update(ptr(dev["x"]), ptr(dev["oc"]), ptr(dev["z"]), m, xi, ptr(b), ptr(bm), n, ptr(sums), bt, snr, 0.93,
                                             stream_ptr()))
        else:
            check(lib.t2p_op_predictor(ptr(dev["x"]), ptr(dev["oc"]), ptr(dev["z"]), m, xi, ptr(b), ptr(bm), n, 3.7, pf, stream_ptr()))
        tag = (n, kind, pf, use_mask, use_xi)
        want = np.where(free, want, h["xi"]) if use_mask else want
        assert torch.equal(bits(b[:n]), bits(torch.from_numpy(want))), tag
        assert torch.equal(bits(bm[:n]), bits(torch.from_numpy(want_m))), tag
        assert bool((b[n:] == SENT).all()) and bool((bm[n:] == SENT).all()), tag


@pytest.mark.parametrize("per_sample", [7, 1280, 16385])
@pytest.mark.parametrize("B", [1, 2, 5])
def test_norm_operator_against_a_float64_sum(B, per_sample):
    """t2p_op_guided_langevin_norms: sum_b ||s_b|| and sum_b ||z_b|| with s formed in float32 as stated, the sums in float64 on the
    host.  The tolerance is what test_langevin_and_predictor (test_gpu_ops.py) allows t2p_op_langevin's norm sums: a relative 1e-6
    (its bound on the noise sum; its bound on the score sum, 1e-4 absolute on a sum of about 2, is wider).  per_sample 7 and 16385
    take the element-by-element branch (not a multiple of 4), 1280 the 16-byte one; 16385 gives every one of the 64 partial
    blocks work and the first a second trip."""
    from text2protein_amd import _lib
    from text2protein_amd._lib import check, ptr, stream_ptr
    lib = _lib.load()
    gen = torch.Generator().manual_seed(17 * B + per_sample)
    oc = torch.randn(B, per_sample, generator=gen) * 0.02
    ou = oc + 0.005 * torch.randn(B, per_sample, generator=gen)
    z = torch.randn(B, per_sample, generator=gen)
    w, w1 = float(F32(0.7)), float(F32(1 - 0.7))
    ws = torch.empty(B * 128, device="cuda")
    d_oc, d_ou, d_z = oc.cuda(), ou.cuda(), z.cuda()
    for guided, scale in itertools.product((True, False), (1.0, -1.7)):
        sums = torch.zeros(2, device="cuda")
        check(lib.t2p_op_guided_langevin_norms(ptr(d_oc), ptr(d_ou) if guided else None, ptr(d_z), B, per_sample, w, w1,
                                               scale, ptr(ws), ptr(sums), stream_ptr()))
        s = guided_s(oc.numpy(), ou.numpy() if guided else None, w, w1, scale).astype(np.float64)
        want = [np.sqrt((s ** 2).sum(-1)).sum(), np.sqrt((z.numpy().astype(np.float64) ** 2).sum(-1)).sum()]
        got = sums.cpu().double().numpy()
        err = [abs(got[i] / want[i] - 1) for i in range(2)]
        print(f"B {B}, per_sample {per_sample}, guided {guided}, scale {scale}: relative error {err[0]:.2e} / {err[1]:.2e}")
        assert max(err) < 1e-6, (B, per_sample, guided, scale)


# ---- 2. whole runs against the reference -------------------------------------------------------------------------------------
def _fixture(name, dtype="f32", model_cls=None):
    from text2protein_amd import sde_lib, synth
    from text2protein_amd.model import HipScoreModel
    case = GO.CASES[name]
    g = load_golden(name)
    cfg = GO.case_config(case)
    cfg.device = "cuda"
    model = (model_cls or HipScoreModel)(cfg, dtype=dtype)
    model.load_state_dict(synth.synth_state_dict(cfg, GO.SEED))
    m = cfg.model
    sde = (sde_lib.VESDE(sigma_min=m.sigma_min, sigma_max=m.sigma_max, N=m.num_scales) if case["sde"] == "vesde"
           else sde_lib.VPSDE(beta_min=m.beta_min, beta_max=m.beta_max, N=m.num_scales))
    shape = (GO.B, cfg.data.num_channels, cfg.data.max_res_num, cfg.data.max_res_num)
    return case, g, cfg, model, sde, shape


def _sampler(case, cfg, sde, shape, **kw):
    from text2protein_amd import sampling
    return sampling.get_sampling_fn(cfg, sde, shape, GO.EPS[case["sde"]], **kw)


def _fused_steps(case, g, cfg, model, sde, shape, w):
    """The fused route driven step by step (PCStepper) on the recorded draws -> (x after every step, x_mean of the last, x buffer)."""
    from text2protein_amd import sampling
    noise = torch.from_numpy(g["noise"]).cuda()
    st = sampling.PCStepper(model, sde, shape[0], cfg.sampling.snr, case["n_steps_each"], eps=GO.EPS[case["sde"]], guidance_w=w)
    x, cmask = sampling.apply_conditions(noise[0] * sde.prior_scale(), GO.case_condition(case, shape[-1]))
    x = x.float().contiguous()
    cond = bool(case["length"])
    keep = (cmask.to(torch.uint8).contiguous(), x.clone())
    st.set_context(torch.from_numpy(g["context"]))
    st.set_condition(*(keep if cond else (None, None)))
    st.reset(0)
    buf = torch.full((2 * shape[0], *shape[1:]), float("nan"), device="cuda") if st.guided else torch.empty(shape, device="cuda")
    buf[:shape[0]] = x
    xm = torch.empty(shape, device="cuda")
    assert case["n_steps_each"] == 1                   # injected corrector noise: one Langevin step per level
    xs = []
    for i in range(sde.N):
        st.step(buf, xm, noise[1 + 2 * i], noise[2 + 2 * i])
        xs.append(buf[:shape[0]].clone())
    if cond:
        xm = torch.where(cmask, xm, keep[1])
    return xs, xm, buf


@pytest.mark.parametrize("name", [n for n, c in GO.CASES.items() if c["n_steps_each"] == 1])
def test_guided_runs_match_the_reference(name):
    """Fused route (step by step) and predictor / corrector classes on the recorded draws against the reference's guided run: the
    final sample and x after every step within the float32 bound of the unguided tiny runs (1e-5 VE, 1e-4 VP), fused against
    classes within the same bound -- and the unguided run of the same build on the same draws misses it (a test an unguided run
    passes shows nothing; the stored unguided reference run is what it lands on instead)."""
    from text2protein_amd.model import HipScoreModel

    class Recording(HipScoreModel):                    # the state the classes route hands to every evaluation
        seen = None

        def __call__(self, x, labels, context=None):
            if self.seen is not None:
                self.seen.append(x[:GO.B].detach().clone())
            return super().__call__(x, labels, context)

    case, g, cfg, model, sde, shape = _fixture(name, model_cls=Recording)
    tol, w = GO.F32_TOL[case["sde"]], case["w"]
    steps = load_golden(name + "_steps")
    ctx = torch.from_numpy(g["context"])
    N = sde.N
    # fused
    xs, xm, buf = _fused_steps(case, g, cfg, model, sde, shape, w)
    torch.cuda.synchronize()
    assert model.pool_reclaimed() == 0
    e_final = rel_l2(xm.cpu(), g["sample"])
    e_steps = max(rel_l2(xs[i].cpu(), steps["x"][i]) for i in range(N))
    assert torch.equal(bits(buf[GO.B:]), bits(buf[:GO.B]))                      # the sampler's copy of the state
    # classes
    fn = _sampler(case, cfg, sde, shape, force_classes=True, guidance_w=w)
    it = iter(torch.from_numpy(g["noise"]))
    model.seen = []
    out_c, nfe = fn(model, condition=GO.case_condition(case, shape[-1]), context=ctx, noise_fn=lambda shp: next(it))
    torch.cuda.synchronize()
    seen, model.seen = model.seen, None
    assert model.pool_reclaimed() == 0
    assert nfe == int(g["nfe"]) == N * 2 and len(seen) == 2 * N                 # ONE evaluation (at batch 2B) per score
    c_final = rel_l2(out_c.cpu(), g["sample"])
    c_steps = max(rel_l2(seen[2 * (i + 1)].cpu(), steps["x"][i]) for i in range(N - 1))
    # the fused route through the public sampler: what the step-by-step drive gave
    fn_f = _sampler(case, cfg, sde, shape, guidance_w=w)
    it = iter(torch.from_numpy(g["noise"]))
    out_f, nfe_f = fn_f(model, condition=GO.case_condition(case, shape[-1]), context=ctx, noise_fn=lambda shp: next(it))
    assert nfe_f == nfe and out_f.shape == tuple(shape) and torch.equal(bits(out_f), bits(xm))
    assert model.pool_reclaimed() == 0
    f_vs_c = rel_l2(out_f.cpu(), out_c.cpu())
    # unguided, same build, same draws
    fn_u = _sampler(case, cfg, sde, shape)
    it = iter(torch.from_numpy(g["noise"]))
    out_u, _ = fn_u(model, condition=GO.case_condition(case, shape[-1]), context=ctx, noise_fn=lambda shp: next(it))
    u_vs_guided, u_vs_unguided = rel_l2(out_u.cpu(), g["sample"]), rel_l2(out_u.cpu(), g["unguided"])
    print(f"{name}: fused final {e_final:.2e}, worst step {e_steps:.2e}; classes final {c_final:.2e}, worst step {c_steps:.2e}; "
          f"fused vs classes {f_vs_c:.2e}; unguided run vs guided reference {u_vs_guided:.2e}, vs unguided reference "
          f"{u_vs_unguided:.2e} (bound {tol:.0e})")
    assert e_final < tol and e_steps < tol and c_final < tol and c_steps < tol and f_vs_c < tol
    assert u_vs_guided > tol and u_vs_unguided < tol


def test_two_corrector_steps_guided():
    """n_steps_each = 2 on the fixture's draws (the reference draws the second Langevin noise of a level in float64; the stored
    draws are its float32 roundings, through the classes route; the fused loop takes injected corrector noise for one Langevin step
    only, so it runs on device noise against the classes route on the same device noise)."""
    name = "guided_pc_ve_w3_n2"
    case, g, cfg, model, sde, shape = _fixture(name)
    ctx = torch.from_numpy(g["context"])
    fn = _sampler(case, cfg, sde, shape, force_classes=True, guidance_w=case["w"])
    it = iter(torch.from_numpy(g["noise"]))
    out, nfe = fn(model, context=ctx, noise_fn=lambda shp: next(it))
    e = rel_l2(out.cpu(), g["sample"])
    assert nfe == int(g["nfe"]) == 3 * sde.N
    fn_f = _sampler(case, cfg, sde, shape, guidance_w=case["w"], seed=11)
    a, _ = fn_f(model, context=ctx, call_index=0)
    assert model.pool_reclaimed() == 0
    # the classes route draws stream k for its k-th draw; the fused loop draws (stream, step word): feed the fused loop's draws
    n = int(np.prod(shape))
    order = [(0, 0)] + [(s, i) for i in range(sde.N) for s in (2, 4, 1)]
    draws = iter([torch.from_numpy(philox.normals(11, s, i, n).astype(F32)).reshape(shape) for s, i in order])
    b, _ = fn(model, context=ctx, noise_fn=lambda shp: next(draws))
    e_fc = rel_l2(a.cpu(), b.cpu())
    print(f"{name}: classes vs reference {e:.2e}; fused on device noise vs classes on the restatement's draws {e_fc:.2e}")
    assert e < SAMPLE_TOL["f32"] and e_fc < SAMPLE_TOL["f32"] and torch.isfinite(a).all()


# ---- 3. 16-bit engines -------------------------------------------------------------------------------------------------------
# rel-L2 of the final sample against the reference on guided_pc_ve_w3_length, measured on an MI355X on the first GPU run of this
# test (gfx950; recorded in DESIGN.md, 'Classifier-free guidance in the predictor-corrector sampler'); the kernels are
# deterministic, the factor 2 below only covers compiler and library drift.  (A dtype without a figure would be held to
# SAMPLE_TOL[dtype] (|w| + |1 - w|), the unguided 16-bit bound scaled by the weights of the guidance sum: 5e-3 / 5e-2 here.)
MEASURED_16BIT = {"f16": 4.166e-4, "bf16": 2.597e-3}


@pytest.mark.parametrize("dtype", ["f16", "bf16"])
def test_16bit_engines_on_the_w3_fixture(dtype):
    name = "guided_pc_ve_w3_length"
    case, g, cfg, model, sde, shape = _fixture(name, dtype)
    fn = _sampler(case, cfg, sde, shape, guidance_w=case["w"])
    it = iter(torch.from_numpy(g["noise"]))
    out, _ = fn(model, condition=GO.case_condition(case, shape[-1]), context=torch.from_numpy(g["context"]), noise_fn=lambda shp: next(it))
    e = rel_l2(out.cpu(), g["sample"])
    w = case["w"]
    bound = 2 * MEASURED_16BIT[dtype] if MEASURED_16BIT.get(dtype) is not None else SAMPLE_TOL[dtype] * (abs(w) + abs(1 - w))
    print(f"{name} on the {dtype} engine: final rel-L2 vs reference {e:.3e} (bound {bound:.3e})")
    assert torch.isfinite(out).all() and e <= bound


# ---- 4. device noise ---------------------------------------------------------------------------------------------------------
def _guided_step_from_operators(model, sde, eps, snr, x, ctx2, i, w, zc, zp, mask=None, xi=None):
    """One guided VE step at loop step i from the operator ABI: the evaluation of [x ; x] under [ctx ; 0] and the three guided
    operators on its two halves -> (x, x_mean)."""
    from text2protein_amd import _lib
    from text2protein_amd._lib import check, ptr, stream_ptr
    lib = _lib.load()
    B, n = x.shape[0], x.numel()
    label = torch.full((2 * B,), int(sde.label_table(eps)[i]), dtype=torch.long, device="cuda")
    G = float(sde.g_table(eps)[i])
    w_, w1 = float(F32(w)), float(F32(1 - w))
    ws, sums = torch.empty(B * 128, device="cuda"), torch.empty(2, device="cuda")
    x = x.clone()
    out = model(torch.cat([x, x]), label, ctx2)
    check(lib.t2p_op_guided_langevin_norms(ptr(out[:B]), ptr(out[B:]), ptr(zc), B, n // B, w_, w1, 1.0, ptr(ws), ptr(sums), stream_ptr()))
    check(lib.t2p_op_guided_langevin_update(ptr(x), ptr(out[:B]), ptr(out[B:]), ptr(zc), ptr(mask), ptr(xi), ptr(x), None, None, n, w_, w1,
                                            1.0, ptr(sums), float(B), snr, 1.0, stream_ptr()))
    out = model(torch.cat([x, x]), label, ctx2)
    xm = torch.empty_like(x)
    check(lib.t2p_op_guided_predictor(ptr(x), ptr(out[:B]), ptr(out[B:]), ptr(zp), ptr(mask), ptr(xi), ptr(x), None, ptr(xm), n, w_, w1, 1.0,
                                      G, 1.0, 0, stream_ptr()))
    return x, xm


def test_fused_step_with_device_noise_against_the_operators():
    """The fused guided step against the guided operators.  Loop step 0: device noise against the operators fed
    t2p_op_philox_normal(seed, stream 2 / 1) -- the documented keys, whose step word is the loop step, 0 here -- bit for bit.  Loop
    step 2: t2p_op_philox_normal cannot draw under step word 2, so (a) with noise injected on both sides the step is bit for bit
    (the step's label and G), and (b) the device draw is held to the restatement's noise at step word 2 within 1e-5, the bound of
    test_the_step_word_of_the_fused_pc_loop.  The second block of x equals the first every time."""
    from text2protein_amd import sampling
    from text2protein_amd._lib import check, ptr, stream_ptr
    case, g, cfg, model, sde, shape = _fixture("guided_pc_ve_w07")
    eps, w, seed, B = GO.EPS["vesde"], case["w"], 5, shape[0]
    n = int(np.prod(shape))
    ctx = torch.from_numpy(g["context"]).cuda()
    ctx2 = torch.cat([ctx, ctx * 0]).contiguous()
    st = sampling.PCStepper(model, sde, B, cfg.sampling.snr, eps=eps, seed=seed, guidance_w=w)
    x0 = sampling._device_randn_like(torch.empty(shape, device="cuda"), 9, 0) * 100.0

    def fused(i, zc=None, zp=None):
        st.set_context(ctx)
        buf = torch.full((2 * B, *shape[1:]), float("nan"), device="cuda")
        buf[:B] = x0
        xm = torch.empty(shape, device="cuda")
        st.reset(i)
        st.step(buf, xm, zc, zp)
        torch.cuda.synchronize()
        assert torch.equal(bits(buf[B:]), bits(buf[:B]))
        return buf[:B].clone(), xm

    def op_noise(stream):
        z = torch.empty(shape, device="cuda")
        check(model.lib.t2p_op_philox_normal(ptr(z), n, seed, stream, stream_ptr()))
        return z

    got = fused(0)
    want = _guided_step_from_operators(model, sde, eps, cfg.sampling.snr, x0, ctx2, 0, w, op_noise(2), op_noise(1))
    assert torch.equal(bits(got[0]), bits(want[0])) and torch.equal(bits(got[1]), bits(want[1]))
    assert not torch.equal(got[0], x0)
    zc, zp = (torch.from_numpy(philox.normals(seed, s, 2, n).astype(F32)).reshape(shape).cuda() for s in (2, 1))
    got = fused(2, zc, zp)
    want = _guided_step_from_operators(model, sde, eps, cfg.sampling.snr, x0, ctx2, 2, w, zc, zp)
    assert torch.equal(bits(got[0]), bits(want[0])) and torch.equal(bits(got[1]), bits(want[1]))
    drawn = fused(2)
    e_x, e_xm = rel_l2(drawn[0].cpu(), got[0].cpu()), rel_l2(drawn[1].cpu(), got[1].cpu())
    print(f"guided step at loop step 2, device noise vs the restatement's: x {e_x:.2e}, x_mean {e_xm:.2e}")
    assert e_x <= 1e-5 and e_xm <= 1e-5
    assert model.pool_reclaimed() == 0


# ---- 5. weight edge cases ----------------------------------------------------------------------------------------------------
def test_weight_one_is_the_plain_sampler_at_batch_b():
    from text2protein_amd import sampling
    case, g, cfg, model, sde, shape = _fixture("guided_pc_ve_w07")
    ctx = torch.from_numpy(g["context"])
    outs = []
    for w in (None, 1.0):
        it = iter(torch.from_numpy(g["noise"]))
        out, _ = _sampler(case, cfg, sde, shape, guidance_w=w)(model, context=ctx, noise_fn=lambda shp: next(it), n_iter=6)
        outs.append(out.clone())
    assert torch.equal(bits(outs[0]), bits(outs[1]))
    counts = []
    for w in (None, 1.0):
        st = sampling.PCStepper(model, sde, shape[0], cfg.sampling.snr, seed=5, guidance_w=w)
        assert not st.guided
        (st.set_context if w is not None else model.set_context)(ctx.cuda())
        x = sampling._device_randn_like(torch.empty(shape, device="cuda"), 9, 0) * 100.0          # room for B samples only
        xm = torch.empty_like(x)
        st.reset(0)
        st.step(x, xm)
        counts.append(st.count_dispatches(x, xm))
    assert counts[0] == counts[1]


def test_no_guidance_reproduces_the_unguided_fixture():
    """guidance_w=None is the path of test_sampler_f32_matches_reference_run: tiny_sampler_none within its bound, and the same bits
    whether the keyword is given or not."""
    from helpers import cfg_tiny
    from text2protein_amd import sampling, sde_lib, synth
    from text2protein_amd.model import HipScoreModel
    g = load_golden("tiny_sampler_none")
    cfg = cfg_tiny()
    cfg.device = "cuda"
    model = HipScoreModel(cfg, dtype="f32")
    model.load_state_dict(synth.synth_state_dict(cfg, int(g["seed"])))
    sde = sde_lib.VESDE(sigma_min=cfg.model.sigma_min, sigma_max=cfg.model.sigma_max, N=cfg.model.num_scales)
    shape = (2, cfg.data.num_channels, cfg.data.max_res_num, cfg.data.max_res_num)
    outs = []
    for kw in ({}, {"guidance_w": None}):
        for force in (False, True):
            it = iter(torch.from_numpy(g["noise"]))
            fn = sampling.get_sampling_fn(cfg, sde, shape, 1e-5, force_classes=force, **kw)
            out, nfe = fn(model, condition={}, context=torch.from_numpy(g["context"]), noise_fn=lambda shp: next(it))
            assert nfe == int(g["nfe"]) and rel_l2(out.cpu(), g["sample"]) < SAMPLE_TOL["f32"]
            outs.append(out.clone())
    assert torch.equal(bits(outs[0]), bits(outs[2])) and torch.equal(bits(outs[1]), bits(outs[3]))


def test_weight_zero_is_the_unguided_run_under_a_zero_context():
    case, g, cfg, model, sde, shape = _fixture("guided_pc_ve_w07")
    ctx = torch.from_numpy(g["context"])
    it = iter(torch.from_numpy(g["noise"]))
    a, _ = _sampler(case, cfg, sde, shape, guidance_w=0.0)(model, context=ctx, noise_fn=lambda shp: next(it))
    it = iter(torch.from_numpy(g["noise"]))
    b, _ = _sampler(case, cfg, sde, shape)(model, context=ctx * 0, noise_fn=lambda shp: next(it))
    e = rel_l2(a.cpu(), b.cpu())
    print(f"w = 0 vs the unguided run under a zero context: {e:.2e}")
    assert e < SAMPLE_TOL["f32"] and rel_l2(a.cpu(), g["unguided"]) > SAMPLE_TOL["f32"]


# ---- 6. frozen entries -------------------------------------------------------------------------------------------------------
def test_length_condition_freezes_its_entries_in_both_halves():
    from text2protein_amd import sampling
    name = "guided_pc_ve_w3_length"
    case, g, cfg, model, sde, shape = _fixture(name)
    xs, xm, buf = _fused_steps(case, g, cfg, model, sde, shape, case["w"])
    x0, cmask = sampling.apply_conditions(torch.from_numpy(g["noise"][0]).cuda() * sde.prior_scale(), GO.case_condition(case, shape[-1]))
    frozen = ~cmask
    assert int(frozen.sum()) > 0
    for half in (buf[:GO.B], buf[GO.B:]):
        assert torch.equal(bits(half[frozen]), bits(x0.float()[frozen]))
    assert torch.equal(bits(xm[frozen]), bits(x0.float()[frozen]))
    # an all-ones mask is the unconditioned guided run
    case, g, cfg, model, sde, shape = _fixture("guided_pc_ve_w07")
    plain, _, _ = _fused_steps(case, g, cfg, model, sde, shape, case["w"])
    st = sampling.PCStepper(model, sde, GO.B, cfg.sampling.snr, eps=GO.EPS["vesde"], guidance_w=case["w"])
    st.set_context(torch.from_numpy(g["context"]))
    noise = torch.from_numpy(g["noise"]).cuda()
    buf = torch.cat([noise[0] * sde.prior_scale()] * 2).contiguous()
    ones, xi = torch.ones(shape, dtype=torch.uint8, device="cuda"), torch.full(shape, float("nan"), device="cuda")
    st.set_condition(ones, xi)
    st.reset(0)
    xm = torch.empty(shape, device="cuda")
    for i in range(3):
        st.step(buf, xm, noise[1 + 2 * i], noise[2 + 2 * i])
    assert torch.equal(bits(buf[:GO.B]), bits(plain[2])) and torch.equal(bits(buf[GO.B:]), bits(plain[2]))


# ---- 7. graph replay and the dispatch count ----------------------------------------------------------------------------------
def test_graph_replay_and_dispatch_count_guided():
    from text2protein_amd import sampling
    case, g, cfg, model, sde, shape = _fixture("guided_pc_ve_w07", "f16")
    ctx = torch.from_numpy(g["context"]).cuda()
    B = shape[0]
    outs = []
    for use_graph in (False, True):
        st = sampling.PCStepper(model, sde, B, cfg.sampling.snr, eps=GO.EPS["vesde"], seed=5, guidance_w=case["w"])
        st.set_context(ctx)
        x = torch.zeros(2 * B, *shape[1:], device="cuda")
        x[:B] = sampling._device_randn_like(torch.empty(shape, device="cuda"), 9, 0) * 100.0
        xm = torch.empty(shape, device="cuda")
        st.reset(0)
        side = torch.cuda.Stream()
        side.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(side):
            for _ in range(4):
                (st.step_graph if use_graph else st.step)(x, xm)
        torch.cuda.synchronize()
        outs.append((x.clone(), xm.clone()))
    assert torch.isfinite(outs[0][0]).all() and torch.equal(bits(outs[0][0][:B]), bits(outs[0][0][B:]))
    assert torch.equal(bits(outs[0][0]), bits(outs[1][0])) and torch.equal(bits(outs[0][1]), bits(outs[1][1]))
    # the dispatch count: the guided step enqueues what the plain step does (the guidance sum rides in the same kernels), plus at
    # most the mirror launch of the first step after a reset
    before = x.clone()
    guided = st.count_dispatches(x, xm)
    st.reset(4)
    first = st.count_dispatches(x, xm)
    torch.cuda.synchronize()
    assert torch.equal(bits(x), bits(before))          # nothing executed
    plain_st = sampling.PCStepper(model, sde, B, cfg.sampling.snr, eps=GO.EPS["vesde"], seed=5)
    model.set_context(ctx)
    xb = before[:B].clone()
    plain_st.reset(0)
    plain_st.step(xb, xm)
    plain = plain_st.count_dispatches(xb, xm)
    print(f"dispatches per step: plain {plain}, guided {guided}, first guided step after a reset {first}")
    assert guided == plain and first == plain + 1
    st.set_context(ctx)                                # (the plain stepper's context at batch B replaced [ctx ; 0])
    st.step(x, xm)                                     # the counted mirror launch was not run and is not skipped now
    torch.cuda.synchronize()
    assert torch.equal(bits(x[:B]), bits(x[B:]))


# ---- 8. the norm all-reduce hook ---------------------------------------------------------------------------------------------
def test_global_batch_norm_two_steppers_equal_one_process():
    """A guided run with global_batch = 2 split over two steppers of one chain each (two engines, two threads, the hook summing
    the two 2-float buffers between them) equals the one-process run on both chains within 1e-5, the bound of
    test_global_batch_norm_two_ranks_equal_one_process."""
    from text2protein_amd import sampling, synth
    from text2protein_amd.model import HipScoreModel
    case, g, cfg, model, sde, shape = _fixture("guided_pc_ve_w07")
    n_iter = 6
    ctx = torch.from_numpy(g["context"])
    noise = torch.from_numpy(g["noise"])
    it = iter(noise)
    want, _ = _sampler(case, cfg, sde, shape, guidance_w=case["w"])(model, context=ctx, noise_fn=lambda shp: next(it), n_iter=n_iter)
    barrier = threading.Barrier(2, timeout=60)
    slots, outs, errors = [None, None], [None, None], []

    def rank(r):
        try:
            torch.cuda.set_device(0)
            m = HipScoreModel(cfg, dtype="f32")
            m.load_state_dict(synth.synth_state_dict(cfg, GO.SEED))

            def all_reduce(t):
                torch.cuda.current_stream().synchronize()
                slots[r] = t.clone()
                barrier.wait()
                t.add_(slots[1 - r])
                torch.cuda.current_stream().synchronize()
                barrier.wait()

            fn = _sampler(case, cfg, sde, (1, *shape[1:]), guidance_w=case["w"], global_batch=2, all_reduce=all_reduce)
            draws = iter(noise)
            outs[r], _ = fn(m, context=ctx[r:r + 1], noise_fn=lambda shp: next(draws)[r:r + 1], n_iter=n_iter)
            torch.cuda.synchronize()
        except Exception as e:  # noqa: BLE001
            errors.append(e)
            barrier.abort()

    threads = [threading.Thread(target=rank, args=(r,)) for r in range(2)]
    for t in threads:
        t.start()
    for t in threads:
        t.join(120)
    assert not errors, errors
    e = rel_l2(torch.cat(outs).cpu(), want.cpu())
    it = iter(noise)
    alone, _ = _sampler(case, cfg, sde, (1, *shape[1:]), guidance_w=case["w"])(model, context=ctx[:1], noise_fn=lambda shp: next(it)[:1],
                                                                              n_iter=n_iter)
    print(f"guided, 2 steppers x 1 chain with the global-batch hook vs 1 stepper x 2 chains: rel-L2 = {e:.3e}")
    assert e < 1e-5
    assert rel_l2(alone.cpu(), want[:1].cpu()) > 1e-5          # the per-stepper mean is another number: the hook really ran


# ---- 9. refusals change nothing ----------------------------------------------------------------------------------------------
def test_refusals_change_nothing():
    from text2protein_amd import sampling
    from text2protein_amd._lib import T2PError
    case, g, cfg, model, sde, shape = _fixture("guided_pc_ve_w07")
    B = shape[0]
    ctx = torch.from_numpy(g["context"]).cuda()
    st = sampling.PCStepper(model, sde, B, cfg.sampling.snr, eps=GO.EPS["vesde"], seed=5, guidance_w=case["w"])
    x = torch.zeros(2 * B, *shape[1:], device="cuda")
    x[:B] = sampling._device_randn_like(torch.empty(shape, device="cuda"), 9, 0) * 100.0
    xm = torch.full(shape, SENT, device="cuda")
    before = x.clone()

    def untouched():
        torch.cuda.synchronize()
        return torch.equal(bits(x), bits(before)) and bool((xm == SENT).all())

    st.reset(0)
    with pytest.raises(T2PError, match="set_context"):                 # a guided step before the context
        st.step(x, xm)
    assert untouched()
    with pytest.raises(T2PError, match="batch"):                       # a context of another batch
        st.set_context(torch.cat([ctx, ctx]))
    with pytest.raises(T2PError, match="set_context"):
        st.step(x, xm)
    assert untouched()
    st.set_context(ctx)
    for bad in (float("nan"), float("inf"), -float("inf")):            # a non-finite weight: the sampler keeps w = 0.7
        with pytest.raises(T2PError, match="finite"):
            st.set_guidance(bad)
        with pytest.raises(T2PError, match="finite"):
            sampling.get_pc_sampler(sde, shape, sampling.ReverseDiffusionPredictor, sampling.LangevinCorrector, 0.17, guidance_w=bad)
    assert st.guided
    st.step(x, xm)
    torch.cuda.synchronize()
    ref = sampling.PCStepper(model, sde, B, cfg.sampling.snr, eps=GO.EPS["vesde"], seed=5, guidance_w=case["w"])
    ref.set_context(ctx)
    y, ym = before.clone(), torch.empty_like(xm)
    ref.reset(0)
    ref.step(y, ym)
    assert torch.equal(bits(x), bits(y)) and torch.equal(bits(xm), bits(ym))
    st.set_context(ctx)
    st.reset(sde.N - 1)                                                # a step past N
    st.step(x, xm)
    torch.cuda.synchronize()
    before, kept = x.clone(), xm.clone()
    with pytest.raises(T2PError, match="beyond sde.N"):
        st.step(x, xm)
    torch.cuda.synchronize()
    assert torch.equal(bits(x), bits(before)) and torch.equal(bits(xm), bits(kept))
    with pytest.raises(T2PError, match="context"):                     # guidance without a context
        _sampler(case, cfg, sde, shape, guidance_w=0.7)(model, context=None)


def test_cli_refuses_pc_guidance_with_ddim():
    """--pc_guidance_w with --sampler ddim exits before touching a device (no visible device in the child)."""
    env = dict(os.environ, HIP_VISIBLE_DEVICES="", ROCR_VISIBLE_DEVICES="")
    r = subprocess.run([sys.executable, os.path.join(ROOT, "sampling_6d.py"), "no_such_config.yml", "synthetic", "--sampler", "ddim",
                        "--pc_guidance_w", "0.7"], capture_output=True, text=True, timeout=120, env=env)
    assert r.returncode != 0 and "--pc_guidance_w" in r.stderr and "Traceback" not in r.stderr


# ---- 10. the command line ----------------------------------------------------------------------------------------------------
def test_cli_pc_guidance(tmp_path):
    """--pc_guidance_w 0.7 on a synthetic VE checkpoint writes the files of the default route with other contents; the default route
    still writes what the parent commit wrote (cli_default_parent.npz, the fixture of test_gpu_ddim.py's CLI test)."""
    cfg = cfg_ckpt()
    cfg.training.sde = "vesde"
    cfg.model.beta_max = 5.0                  # the configuration test_cli_default_route_is_unchanged (test_gpu_ddim.py) writes
    cfg_path = tmp_path / "ckpt_vesde.yml"
    with open(cfg_path, "w") as f:
        yaml.safe_dump(yaml.safe_load(__import__("json").dumps(cfg)), f)
    base = [sys.executable, os.path.join(ROOT, "sampling_6d.py"), str(cfg_path), os.path.join(GOLDEN, "tiny_checkpoint.pth"),
            "--batch_size", "2", "--context_tokens", "4", "--dtype", "f32"]
    files = {}
    for tag, extra in (("default", []), ("guided", ["--pc_guidance_w", "0.7"])):
        out = tmp_path / tag
        r = subprocess.run(base + ["--outdir", str(out)] + extra, capture_output=True, text=True, timeout=600, cwd=str(tmp_path))
        assert r.returncode == 0, r.stdout + r.stderr
        files[tag] = {p.name: pickle.load(open(p, "rb")) for p in sorted(out.iterdir())}
    assert sorted(files["default"]) == sorted(files["guided"]) == ["sampled_0.pkl", "sampled_1.pkl"]
    parent = load_golden("cli_default_parent")
    for k in files["default"]:
        d, gd = files["default"][k], files["guided"][k]
        assert d.shape == gd.shape == (1, 5, 8, 8) and d.dtype == gd.dtype and torch.isfinite(gd).all() and not torch.equal(d, gd)
        assert torch.equal(bits(d), bits(torch.from_numpy(parent[k])))
