"""Replacement inpainting in the fused predictor-corrector loop on the GPU (score_sde_pytorch/inpainting.py, get_pc_inpainter): the
update operators with the replacement against their formula, whole runs against the reference's own pc_inpainter body
(tests/golden/make_golden_inpaint_replace.py), device draws, identities, precedence under a condition, graph replay and the
dispatch count, 16-bit engines, the Python interface and the command line, refusals."""
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

import inpaint_replace_oracle as IO
from helpers import GOLDEN, assert_table_close, cfg_ckpt, rel_l2
from oracle import philox
from test_gpu_guided_pc import SAMPLE_TOL, SENT, bits, guided_s, langevin_formula, predictor_formula

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F32 = np.float32
STREAM_C, STREAM_P = 0x80000000, 0x80000001          # csrc/philox.h: the draw after the corrector / after the predictor


def _replace(lib_struct, known, data, noise=None, tables=None, step=0, a=1.0, s=0.0, seed=0, stream=0):
    from text2protein_amd._lib import ptr
    r = lib_struct()
    r.known, r.data, r.noise = ptr(known), ptr(data), ptr(noise)
    if tables is not None:
        r.mean_table, r.std_table, r.n_table = ptr(tables[0]), ptr(tables[1]), tables[0].numel()
    r.step, r.mean_coef, r.std, r.seed, r.stream_id = step, a, s, seed, stream
    return r


def replace_formula(xn, d, kn, free, a, s, z):
    """x'' and m'' from the (already condition-masked) update result xn: r = fl(fl(a d) + fl(z s)), each rounded (numpy float32)."""
    ad = (F32(a) * d).astype(F32)
    r = (ad + (z * F32(s)).astype(F32)).astype(F32)
    rep = kn.astype(bool) & free
    x2 = np.where(rep, r, xn)
    return x2, np.where(rep, ad, x2)


# ---- 1. operators against the formula ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [1, 3, 4, 5, 4 * 64 * 3 + 2])
def test_replace_operators_are_the_formula(n):
    """t2p_op_inpaint_langevin_update / t2p_op_inpaint_predictor by value (==, so -0 == +0) against the float32 formula on the
    host: {plain, guided (two destinations)} x condition mask x {a = 1 and s by value, VP-like device tables read at step 3} x
    known {all 0, all 1, mixed within every quad} x pointers {16-byte aligned, offset by one float and the byte masks by one byte:
    the element-by-element path}.  n below, at and across the quad, and more than one block with a tail."""
    from text2protein_amd import _lib
    from text2protein_amd._lib import check, ptr, stream_ptr
    lib = _lib.load()
    gen = torch.Generator().manual_seed(900 + n)
    w, w1 = float(F32(0.7)), float(F32(1 - 0.7))
    sums_h = [3.25, 71.5]
    sums = torch.tensor(sums_h, device="cuda")
    snr, bt = 0.17, 2.0
    tabs_h = (torch.tensor([0.1, 0.2, 0.3, 0.8125, 0.9]), torch.tensor([0.9, 0.8, 0.7, 0.5831, 0.1]))
    tabs = tuple(t.cuda() for t in tabs_h)
    for off in (0, 1):
        def dev(t):                                    # a device copy that starts `off` elements into its allocation
            buf = torch.zeros(t.numel() + off, dtype=t.dtype, device="cuda")
            buf[off:] = t
            return buf[off:]
        x, oc, z, xi, d, rz = (torch.randn(n, generator=gen) for _ in range(6))
        x = x * 30
        ou = oc + 0.25 * torch.randn(n, generator=gen)
        mask = (torch.rand(n, generator=gen) < 0.6).to(torch.uint8)
        mixed = (torch.arange(n) % 4 == 1) | (torch.arange(n) % 4 == 2) if n > 1 else torch.ones(1, dtype=torch.bool)
        knowns = {"none": torch.zeros(n, dtype=torch.uint8), "all": torch.ones(n, dtype=torch.uint8), "mixed": mixed.to(torch.uint8)}
        h = {k: v.numpy() for k, v in dict(x=x, oc=oc, ou=ou, z=z, xi=xi, d=d, rz=rz, mask=mask).items()}
        D = {k: dev(v) for k, v in dict(x=x, oc=oc, ou=ou, z=z, xi=xi, d=d, rz=rz, mask=mask).items()}
        for (kname, kn), guided, use_mask, use_tab in itertools.product(knowns.items(), (False, True), (False, True), (False, True)):
            d_kn = dev(kn)
            free = h["mask"].astype(bool) if use_mask else np.ones(n, bool)
            a, s = (float(tabs_h[0][3]), float(tabs_h[1][3])) if use_tab else (1.0, 0.37)
            scale, alpha, xc = (-1.7, 0.93, 1.031) if use_tab else (1.0, 1.0, 1.0)
            sc = guided_s(h["oc"], h["ou"] if guided else None, w, w1, scale)
            launches = [("langevin", 0, langevin_formula(h["x"], sc, h["z"], sums_h, bt, snr, alpha)[0]),
                        ("predictor", 0, predictor_formula(h["x"], sc, h["z"], 3.7, xc, 0)[0]),
                        ("predictor", 1, predictor_formula(h["x"], sc, h["z"], 3.7, xc, 1)[0])]
            for kind, pf, upd in launches:
                xn = np.where(free, upd, h["xi"])
                want, want_m = replace_formula(xn, h["d"], kn.numpy(), free, a, s, h["rz"])
                out = torch.full((2 * n + 8 + off,), SENT, device="cuda")[off:]
                xmo = torch.full((n + 8 + off,), SENT, device="cuda")[off:]
                r = _replace(_lib.InpaintReplace, d_kn, D["d"], D["rz"], tabs if use_tab else None, 3 if use_tab else 0, a if not use_tab else 7.0,
                             s if not use_tab else 7.0)
                common = (ptr(D["x"]), ptr(D["oc"]), ptr(D["ou"]) if guided else None, ptr(D["z"]), ptr(D["mask"]) if use_mask else None,
                          ptr(D["xi"]) if use_mask else None, ptr(out), ptr(out[n:]) if guided else None, ptr(xmo), n, w, w1, scale)
                if kind == "langevin":
                    check(lib.t2p_op_inpaint_langevin_update(*common, ptr(sums), bt, snr, alpha, C.byref(r), stream_ptr()))
                else:
                    check(lib.t2p_op_inpaint_predictor(*common, 3.7, xc, pf, C.byref(r), stream_ptr()))
                tag = (n, off, kname, guided, use_mask, use_tab, kind, pf)
                got, got_m = out[:n].cpu().numpy(), xmo[:n].cpu().numpy()
                assert np.array_equal(got, want), tag
                assert np.array_equal(got_m, want_m), tag
                if guided:
                    assert torch.equal(bits(out[n:2 * n]), bits(out[:n])), tag
                assert bool((out[2 * n if guided else n:] == SENT).all()) and bool((xmo[n:] == SENT).all()), tag
                if kname == "none":                    # nothing known: the update itself, x_mean = the new x
                    assert np.array_equal(got, xn) and np.array_equal(got_m, xn), tag


def test_operator_draws_are_the_documented_philox_draws():
    """noise NULL: the operator draws z = normals(seed, stream, step word) for the quad, the numbers t2p_op_philox_normal gives
    for step word 0 bit for bit and oracle/philox.py within the bound of test_the_step_word_of_the_fused_pc_loop (1e-5) at step
    word 3; aligned and unaligned pointers draw the same numbers."""
    from text2protein_amd import _lib
    from text2protein_amd._lib import check, ptr, stream_ptr
    lib = _lib.load()
    n, seed = 4 * 300 + 3, 77
    zero = torch.zeros(n + 1, device="cuda")
    ones_u8 = torch.ones(n + 1, dtype=torch.uint8, device="cuda")
    for step, off in itertools.product((0, 3), (0, 1)):
        out, xm = torch.empty(n + 1, device="cuda")[off:], torch.empty(n + 1, device="cuda")[off:]
        r = _replace(_lib.InpaintReplace, ones_u8[off:], zero[off:], None, None, step, 1.0, 1.0, seed, STREAM_P)
        check(lib.t2p_op_inpaint_predictor(ptr(zero[off:]), ptr(zero[off:]), None, ptr(zero[off:]), None, None, ptr(out), None, ptr(xm), n,
                                           1.0, 0.0, 1.0, 0.0, 1.0, 0, C.byref(r), stream_ptr()))
        want = philox.normals(seed, STREAM_P, step, n).astype(F32)
        assert rel_l2(out[:n].cpu(), want) <= 1e-5 and bool((xm[:n] == 0).all()), (step, off)
        if step == 0:
            z = torch.empty(n + 1, device="cuda")
            check(lib.t2p_op_philox_normal(ptr(z), n, seed, STREAM_P, stream_ptr()))
            assert torch.equal(bits(out[:n]), bits(z[:n])), off


# ---- 2. whole runs against the reference ------------------------------------------------------------------------------------
def _fixture(name, dtype="f32"):
    from text2protein_amd import sde_lib, synth
    from text2protein_amd.model import HipScoreModel
    case = IO.CASES[name]
    g, steps = IO.load(name, GOLDEN)
    cfg = IO.case_config(case)
    cfg.device = "cuda"
    model = HipScoreModel(cfg, dtype=dtype)
    model.load_state_dict(synth.synth_state_dict(cfg, IO.SEED))
    m = cfg.model
    sde = (sde_lib.VESDE(sigma_min=m.sigma_min, sigma_max=m.sigma_max, N=m.num_scales) if case["sde"] == "vesde"
           else sde_lib.VPSDE(beta_min=m.beta_min, beta_max=m.beta_max, N=m.num_scales))
    shape = (IO.B, cfg.data.num_channels, cfg.data.max_res_num, cfg.data.max_res_num)
    return case, g, steps, cfg, model, sde, shape


def _stepper(case, g, cfg, model, sde, shape, w="case", known=None, seed=0, inpaint=True):
    """A PCStepper on the fixture's context, condition, data and known mask -> (stepper, x buffer holding the start, x_mean,
    (condition mask, x_initial))."""
    from text2protein_amd import sampling
    w = case["w"] if w == "case" else w
    eps = IO.EPS[case["sde"]]
    st = sampling.PCStepper(model, sde, shape[0], cfg.sampling.snr, case["n_steps_each"], eps=eps, seed=seed, guidance_w=w)
    data = torch.from_numpy(g["data"]).cuda()
    kn = torch.from_numpy(g["known"]).cuda() if known is None else known
    x = torch.from_numpy(g["noise"][0]).cuda() * sde.prior_scale()
    x = torch.where(kn.bool(), data, x) if inpaint else x
    x, cmask = sampling.apply_conditions(x, IO.case_condition(case, shape[-1]))
    x = x.float().contiguous()
    cond = (cmask.to(torch.uint8).contiguous(), x.clone())
    (st.set_context if w is not None else model.set_context)(torch.from_numpy(g["context"]).cuda())
    st.set_condition(*(cond if case["length"] else (None, None)))
    if inpaint:
        st.set_inpaint(kn.contiguous(), data, *sde.inpaint_tables(eps))
    st.reset(0)
    buf = torch.full((2 * shape[0], *shape[1:]), float("nan"), device="cuda") if st.guided else torch.empty(shape, device="cuda")
    buf[:shape[0]] = x
    return st, buf, torch.empty(shape, device="cuda"), cond


_REPLAYS = {}


def _replay(name, dtype="f32"):
    """The fused loop step by step on the fixture's draws (cached per case) -> (x after every step, x_mean after every step, the
    x buffer, (condition mask, x_initial))."""
    if (name, dtype) not in _REPLAYS:
        case, g, steps, cfg, model, sde, shape = _fixture(name, dtype)
        assert case["n_steps_each"] == 1
        st, buf, xm, cond = _stepper(case, g, cfg, model, sde, shape)
        noise = torch.from_numpy(g["noise"]).cuda()
        xs, xms = [], []
        for i in range(sde.N):
            st.set_inpaint_noise(noise[2 + 4 * i], noise[4 + 4 * i])
            st.step(buf, xm, noise[1 + 4 * i], noise[3 + 4 * i])
            xs.append(buf[:shape[0]].clone())
            xms.append(xm.clone())
        torch.cuda.synchronize()
        assert model.pool_reclaimed() == 0
        _REPLAYS[(name, dtype)] = (xs, xms, buf.clone(), cond)
    return _REPLAYS[(name, dtype)]


@pytest.mark.parametrize("name", [n for n, c in IO.CASES.items() if c["n_steps_each"] == 1])
def test_replay_matches_the_reference(name):
    """Injected draws through t2p_sampler_step: the final sample and x after every step within the float32 bound of the tiny runs
    (guided_oracle.F32_TOL: 1e-5 VE, 1e-4 VP); the known region of every per-step x_mean is fl(a_i d) exactly; and a plain run of
    the same build on the same update draws misses the bound (a test the plain loop passes shows nothing)."""
    case, g, steps, cfg, model, sde, shape = _fixture(name)
    tol = IO.F32_TOL[case["sde"]]
    xs, xms, buf, cond = _replay(name)
    final = torch.where(cond[0].bool(), xms[-1], cond[1]) if case["length"] else xms[-1]
    e_final = rel_l2(final.cpu(), g["sample"])
    e_steps = max(rel_l2(xs[i].cpu(), steps["x"][i]) for i in range(sde.N))
    print(f"{name}: final {e_final:.2e}, worst per-step x {e_steps:.2e} (bound {tol:.0e})")
    assert e_final < tol and e_steps < tol
    kn = g["known"].astype(bool)
    a = sde.inpaint_tables(IO.EPS[case["sde"]])[0].numpy()      # the float32 values torch computes on this host (helpers.F32_HOST_RTOL)
    assert_table_close(a, g["mean_coef"])
    for i in range(sde.N):
        assert np.array_equal(xms[i].cpu().numpy()[kn], (a[i] * g["data"])[kn]), i
    if buf.shape[0] == 2 * shape[0]:
        assert torch.equal(bits(buf[shape[0]:]), bits(buf[:shape[0]]))
    st, pbuf, pxm, _ = _stepper(case, g, cfg, model, sde, shape, inpaint=False)
    noise = torch.from_numpy(g["noise"]).cuda()
    for i in range(sde.N):
        st.step(pbuf, pxm, noise[1 + 4 * i], noise[3 + 4 * i])
    assert rel_l2(pxm.cpu(), g["sample"]) > tol


def test_two_corrector_steps_from_the_operators():
    """n_steps_each = 2: the fused loop takes injected corrector noise for one Langevin step only, so the fixture's draws run
    through the kernels of the loop as operators (the replacement rides in the last inner Langevin update), within the VE bound;
    and the fused loop on device noise replaces after the last inner step only: its known x_mean is fl(a d), its sample finite."""
    from text2protein_amd import _lib
    from text2protein_amd._lib import check, ptr, stream_ptr
    name = "inpaint_replace_ve_n2"
    case, g, steps, cfg, model, sde, shape = _fixture(name)
    lib = _lib.load()
    eps, B, n = IO.EPS["vesde"], shape[0], int(np.prod(shape))
    noise = torch.from_numpy(g["noise"]).cuda()
    data, kn = torch.from_numpy(g["data"]).cuda(), torch.from_numpy(g["known"]).cuda()
    ctx = torch.from_numpy(g["context"]).cuda()
    a_t, s_t = sde.inpaint_tables(eps)
    labels, G = sde.label_table(eps), sde.g_table(eps)
    x = torch.where(kn.bool(), data, noise[0] * sde.prior_scale()).contiguous()
    xm = torch.empty_like(x)
    ws, sums = torch.empty(B * 128, device="cuda"), torch.empty(2, device="cuda")
    worst = 0.0
    for i in range(sde.N):
        lab = torch.full((B,), int(labels[i]), dtype=torch.long, device="cuda")
        z = noise[1 + 5 * i: 6 + 5 * i]
        for k in range(2):
            out = model(x, lab, ctx)
            check(lib.t2p_op_langevin_norms(ptr(out), ptr(z[k]), B, n // B, ptr(ws), ptr(sums), stream_ptr()))
            if k == 0:
                check(lib.t2p_op_langevin_update(ptr(x), ptr(out), ptr(z[k]), None, None, ptr(x), None, n, ptr(sums), float(B), cfg.sampling.snr,
                                                 1.0, stream_ptr()))
            else:
                r = _replace(_lib.InpaintReplace, kn, data, z[2], None, i, float(a_t[i]), float(s_t[i]))
                check(lib.t2p_op_inpaint_langevin_update(ptr(x), ptr(out), None, ptr(z[k]), None, None, ptr(x), None, None, n, 1.0, 0.0, 1.0,
                                                         ptr(sums), float(B), cfg.sampling.snr, 1.0, C.byref(r), stream_ptr()))
        out = model(x, lab, ctx)
        r = _replace(_lib.InpaintReplace, kn, data, z[4], None, i, float(a_t[i]), float(s_t[i]))
        check(lib.t2p_op_inpaint_predictor(ptr(x), ptr(out), None, ptr(z[3]), None, None, ptr(x), None, ptr(xm), n, 1.0, 0.0, 1.0, float(G[i]), 1.0,
                                           0, C.byref(r), stream_ptr()))
        worst = max(worst, rel_l2(x.cpu(), steps["x"][i]))
    e = rel_l2(xm.cpu(), g["sample"])
    print(f"{name} through the operators: final {e:.2e}, worst per-step x {worst:.2e}")
    assert e < IO.F32_TOL["vesde"] and worst < IO.F32_TOL["vesde"]
    st, buf, fxm, _ = _stepper(case, g, cfg, model, sde, shape, seed=4)
    for _ in range(3):
        st.step(buf, fxm)
    torch.cuda.synchronize()
    k = g["known"].astype(bool)
    assert np.array_equal(fxm.cpu().numpy()[k], g["data"][k]) and bool(torch.isfinite(buf).all())
    from text2protein_amd._lib import T2PError
    with pytest.raises(T2PError, match="n_steps_each == 1"):
        st.set_inpaint_noise(noise[1], None)
    st.set_inpaint_noise(None, noise[1])               # the predictor side has one draw per level: accepted


# ---- 3. device draws ---------------------------------------------------------------------------------------------------------
def _step_from_operators(model, sde, cfg, eps, x, ctx, i, zc, zp, kn, data, rc, rp):
    """One plain VE step with replacement at loop step i from the operator ABI; rc / rp: (noise or None, seed) of the two draws."""
    from text2protein_amd import _lib
    from text2protein_amd._lib import check, ptr, stream_ptr
    lib = _lib.load()
    B, n = x.shape[0], x.numel()
    a_t, s_t = sde.inpaint_tables(eps)
    lab = torch.full((B,), int(sde.label_table(eps)[i]), dtype=torch.long, device="cuda")
    ws, sums = torch.empty(B * 128, device="cuda"), torch.empty(2, device="cuda")
    x, xm = x.clone(), torch.empty_like(x)
    out = model(x, lab, ctx)
    check(lib.t2p_op_langevin_norms(ptr(out), ptr(zc), B, n // B, ptr(ws), ptr(sums), stream_ptr()))
    r = _replace(_lib.InpaintReplace, kn, data, rc[0], None, i, float(a_t[i]), float(s_t[i]), rc[1], STREAM_C)
    check(lib.t2p_op_inpaint_langevin_update(ptr(x), ptr(out), None, ptr(zc), None, None, ptr(x), None, None, n, 1.0, 0.0, 1.0, ptr(sums),
                                             float(B), cfg.sampling.snr, 1.0, C.byref(r), stream_ptr()))
    out = model(x, lab, ctx)
    r = _replace(_lib.InpaintReplace, kn, data, rp[0], None, i, float(a_t[i]), float(s_t[i]), rp[1], STREAM_P)
    check(lib.t2p_op_inpaint_predictor(ptr(x), ptr(out), None, ptr(zp), None, None, ptr(x), None, ptr(xm), n, 1.0, 0.0, 1.0,
                                       float(sde.g_table(eps)[i]), 1.0, 0, C.byref(r), stream_ptr()))
    return x, xm


@pytest.mark.parametrize("i", [0, 3])
def test_fused_step_draws_the_two_new_streams(i):
    """One fused step at loop step i with the update noise injected and the replacement noise drawn on the device, against the
    operators: bit for bit when they draw (seed, stream 0x80000000 / 0x80000001, step word i) themselves, and within 1e-5 (the bound
    of the restatement's draws, test_the_step_word_of_the_fused_pc_loop) when fed oracle/philox.py's normals for those keys."""
    case, g, steps, cfg, model, sde, shape = _fixture("inpaint_replace_ve")
    eps, seed, n = IO.EPS["vesde"], 21, int(np.prod(shape))
    st, buf, xm, _ = _stepper(case, g, cfg, model, sde, shape, seed=seed)
    x0 = buf.clone()
    noise = torch.from_numpy(g["noise"]).cuda()
    zc, zp = noise[1], noise[3]
    st.reset(i)
    st.step(buf, xm, zc, zp)
    torch.cuda.synchronize()
    data, kn, ctx = torch.from_numpy(g["data"]).cuda(), torch.from_numpy(g["known"]).cuda(), torch.from_numpy(g["context"]).cuda()
    model.set_context(ctx)
    want = _step_from_operators(model, sde, cfg, eps, x0, ctx, i, zc, zp, kn, data, (None, seed), (None, seed))
    assert torch.equal(bits(buf), bits(want[0])) and torch.equal(bits(xm), bits(want[1]))
    fed = [torch.from_numpy(philox.normals(seed, s, i, n).astype(F32)).reshape(shape).cuda() for s in (STREAM_C, STREAM_P)]
    near = _step_from_operators(model, sde, cfg, eps, x0, ctx, i, zc, zp, kn, data, (fed[0], 0), (fed[1], 0))
    e_x, e_m = rel_l2(buf.cpu(), near[0].cpu()), rel_l2(xm.cpu(), near[1].cpu())
    print(f"loop step {i}: device draws vs oracle/philox.py normals: x {e_x:.2e}, x_mean {e_m:.2e}")
    assert e_x <= 1e-5 and e_m <= 1e-5
    other = _step_from_operators(model, sde, cfg, eps, x0, ctx, i, zc, zp, kn, data, (None, seed + 1), (None, seed + 1))
    assert not torch.equal(bits(other[0]), bits(want[0]))            # the draws are really read


# ---- 4. identities -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("w", [None, 3.0])
def test_nothing_known_is_the_plain_run_bit_for_bit(w):
    """known all zeros, 'never set' and 'set, then cleared' all reproduce the state of the plain loop bit for bit (x and, under
    guidance, the sampler's copy).  x_mean: never set and cleared give the plain loop's bit for bit; with an all-zero mask set, the
    replacement runs and x_mean is the NEW x everywhere, as the reference has it off the known region (inpainting.py:46).  known all
    ones gives x_mean == fl(a d) everywhere (VP tables, a != 1)."""
    runs = {}
    case, g, steps, cfg, model, sde, shape = _fixture("inpaint_replace_vp")
    zeros = torch.zeros(shape, dtype=torch.uint8, device="cuda")
    for tag in ("never", "zeros", "cleared"):
        st, buf, xm, _ = _stepper(case, g, cfg, model, sde, shape, w=w, known=zeros, seed=6, inpaint=tag != "never")
        buf[:shape[0]] = torch.from_numpy(g["noise"][0]).cuda()
        if tag == "cleared":
            st.set_inpaint()
        for _ in range(3):
            st.step(buf, xm)
        torch.cuda.synchronize()
        runs[tag] = (buf.clone(), xm.clone())
    for tag in ("zeros", "cleared"):
        assert torch.equal(bits(runs[tag][0]), bits(runs["never"][0])), tag
    assert torch.equal(bits(runs["cleared"][1]), bits(runs["never"][1]))
    assert torch.equal(bits(runs["zeros"][1]), bits(runs["zeros"][0][:shape[0]]))      # inpainting.py:46: x_mean = x * (1 - mask) + ...
    assert not torch.equal(bits(runs["never"][1]), bits(runs["never"][0][:shape[0]]))
    assert bool(torch.isfinite(runs["never"][0]).all())
    ones = torch.ones(shape, dtype=torch.uint8, device="cuda")
    st, buf, xm, _ = _stepper(case, g, cfg, model, sde, shape, w=w, known=ones, seed=6)
    for _ in range(3):
        st.step(buf, xm)
    a = sde.inpaint_tables(IO.EPS["vpsde"])[0]
    assert float(a[2]) != 1.0
    assert np.array_equal(xm.cpu().numpy(), (a[2].numpy() * g["data"]).astype(F32))
    assert not torch.equal(bits(buf[:shape[0]]), bits(runs["never"][0][:shape[0]]))


# ---- 5. precedence -----------------------------------------------------------------------------------------------------------
def test_frozen_entries_win_over_known_ones():
    """inpaint_replace_ve_length under guidance, with a known mask that also covers entries the length condition freezes: those stay
    x_initial bitwise in both halves of the state and in x_mean; known entries the condition leaves free are replaced."""
    case, g, steps, cfg, model, sde, shape = _fixture("inpaint_replace_ve_length")
    B = shape[0]
    kn = torch.from_numpy(g["known"]).cuda().clone()
    kn[:, :, 10:14, :] = 1                               # rows 12, 13 and the last channel are frozen by the length condition
    st, buf, xm, cond = _stepper(case, g, cfg, model, sde, shape, w=3.0, known=kn, seed=8)
    for _ in range(3):
        st.step(buf, xm)
    torch.cuda.synchronize()
    frozen, x_initial = ~cond[0].bool(), cond[1]
    assert int((frozen & kn.bool()).sum()) > 0
    for half in (buf[:B], buf[B:]):
        assert torch.equal(bits(half[frozen]), bits(x_initial[frozen]))
    assert torch.equal(bits(xm[frozen]), bits(x_initial[frozen]))
    rep = kn.bool() & ~frozen
    data = torch.from_numpy(g["data"]).cuda()
    assert torch.equal(xm[rep], data[rep]) and not torch.equal(buf[:B][rep], data[rep])
    # the stored run: frozen entries of every replayed state
    xs, xms, _, cond = _replay("inpaint_replace_ve_length")
    assert all(torch.equal(bits(x[~cond[0].bool()]), bits(cond[1][~cond[0].bool()])) for x in xs)


# ---- 6. graph replay and the dispatch count ---------------------------------------------------------------------------------
def test_graph_replay_recapture_and_dispatch_count():
    case, g, steps, cfg, model, sde, shape = _fixture("inpaint_replace_ve", "f16")
    kn2 = torch.from_numpy(g["known"]).cuda().flip(0).contiguous()
    outs = {}
    for use_graph in (False, True):
        st, buf, xm, _ = _stepper(case, g, cfg, model, sde, shape, seed=5)
        side = torch.cuda.Stream()
        side.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(side):
            for _ in range(4):
                (st.step_graph if use_graph else st.step)(buf, xm)
            torch.cuda.synchronize()
            first = (buf.clone(), xm.clone())
            # other known / data pointers: the captured step is dropped and captured again
            data2 = torch.from_numpy(g["data"]).cuda().flip(0).contiguous()
            st.set_inpaint(kn2, data2, *sde.inpaint_tables(IO.EPS["vesde"]))
            for _ in range(2):
                (st.step_graph if use_graph else st.step)(buf, xm)
        torch.cuda.synchronize()
        outs[use_graph] = (first, (buf.clone(), xm.clone()))
        if use_graph:
            from text2protein_amd._lib import T2PError
            st.set_inpaint_noise(None, torch.zeros(shape, device="cuda"))
            with pytest.raises(T2PError, match="set_inpaint_noise"):
                with torch.cuda.stream(side):
                    st.step_graph(buf, xm)
            st.set_inpaint_noise()
            on = st.count_dispatches(buf, xm)
            st.set_inpaint()
            off = st.count_dispatches(buf, xm)
            print(f"dispatches per step: replacement on {on}, off {off}")
            assert on == off
    for part in (0, 1):
        for t in (0, 1):
            assert torch.equal(bits(outs[False][part][t]), bits(outs[True][part][t])), (part, t)
    k2 = kn2.bool().cpu().numpy()
    assert np.array_equal(outs[True][1][1].cpu().numpy()[k2], np.flip(g["data"], 0)[k2])       # the re-captured step reads the new pointers
    assert bool(torch.isfinite(outs[True][1][0]).all())


# ---- 7. 16-bit engines ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", ["f16", "bf16"])
def test_16bit_engines_on_the_ve_fixture(dtype):
    """The replay of inpaint_replace_ve on a 16-bit engine against the reference within SAMPLE_TOL of test_gpu_sampler.py (the
    fixture's stored sensitivity is at most 10)."""
    name = "inpaint_replace_ve"
    g, _ = IO.load(name, GOLDEN)
    assert float(g["sensitivity"]) <= 10
    xs, xms, _, _ = _replay(name, dtype)
    e = rel_l2(xms[-1].cpu(), g["sample"])
    print(f"{name} on the {dtype} engine: final rel-L2 vs reference {e:.3e} (bound {SAMPLE_TOL[dtype]:.0e})")
    assert bool(torch.isfinite(xms[-1]).all()) and e <= SAMPLE_TOL[dtype]


# ---- 8. end to end -----------------------------------------------------------------------------------------------------------
def test_pc_inpainter_on_a_trainer_is_reproducible():
    """get_pc_inpainter with a HipTrainModel (its current parameters through sampling_model) and the prior drawn on the device
    (t2p_sampler_run): two calls with the same call index are identical, another index differs, known entries of the denoised
    VE sample are the data, and guidance / a condition compose."""
    from text2protein_amd import inpainting, losses, sampling, sde_lib, synth
    case = IO.CASES["inpaint_replace_ve_length"]
    cfg = IO.case_config(case)
    cfg.device = "cuda"
    g, _ = IO.load("inpaint_replace_ve_length", GOLDEN)
    trainer = losses.HipTrainModel(cfg, device="cuda:0", seed=11)
    trainer.load_state_dict(synth.synth_state_dict(cfg, IO.SEED))
    m = cfg.model
    sde = sde_lib.VESDE(sigma_min=m.sigma_min, sigma_max=m.sigma_max, N=m.num_scales)
    data, known, ctx = torch.from_numpy(g["data"]), torch.from_numpy(g["known"]), torch.from_numpy(g["context"])
    cond = IO.case_condition(case, cfg.data.max_res_num)
    for w in (None, 3.0):
        fn = inpainting.get_pc_inpainter(sde, sampling.ReverseDiffusionPredictor, sampling.LangevinCorrector, cfg.sampling.snr,
                                         eps=IO.EPS["vesde"], seed=3, guidance_w=w)
        a, nfe = fn(trainer, data, known, context=ctx, condition=cond, call_index=0, train_dtype="f32")
        b, _ = fn(trainer, data, known, context=ctx, condition=cond, call_index=0, train_dtype="f32")
        c, _ = fn(trainer, data, known, context=ctx, condition=cond, call_index=1, train_dtype="f32")
        assert nfe == 2 * sde.N and a.shape == data.shape and bool(torch.isfinite(a).all())
        assert torch.equal(bits(a), bits(b)) and not torch.equal(bits(a), bits(c))
        k = known.bool()
        assert torch.equal(a.cpu()[k], data[k])
        _, free = sampling.apply_conditions(torch.zeros_like(data), cond)
        x_init, _ = sampling.apply_conditions(torch.zeros_like(data), cond)
        assert torch.equal(a.cpu()[~free], x_init[~free])
        assert not torch.equal(a.cpu()[free & ~k], data[free & ~k])


def test_cli_replace_mode_holds_the_known_maps(tmp_path):
    """sampling_6d.py --inpaint_mode replace --pdb on a config WITHOUT the inpainting condition (length only), the tiny
    checkpoint: the known entries of the written (denoised, VE: a = 1) samples are the encoded maps of the chain, the residues of
    --mask_info are not; the default mode on the same command line does not hold them."""
    from text2protein_amd import encode
    from text2protein_amd.conditions import pair_mask, parse_mask_info
    cfg = cfg_ckpt()
    cfg.training.sde = "vesde"
    cfg.model.condition = ["length"]
    cfg_path = tmp_path / "ckpt_length.yml"
    with open(cfg_path, "w") as f:
        yaml.safe_dump(yaml.safe_load(__import__("json").dumps(cfg)), f)
    pdb = os.path.join(GOLDEN, "encode_chain.pdb")
    L, Cn = cfg.data.max_res_num, cfg.data.num_channels
    base = [sys.executable, os.path.join(ROOT, "sampling_6d.py"), str(cfg_path), os.path.join(GOLDEN, "tiny_checkpoint.pth"), "--batch_size", "2",
            "--context_tokens", "4", "--dtype", "f32", "--pdb", pdb, "--chain", "A", "--mask_info", "1:2,5"]
    files = {}
    for tag, extra in (("replace", ["--inpaint_mode", "replace"]), ("condition", [])):
        out = tmp_path / tag
        r = subprocess.run(base + ["--outdir", str(out)] + extra, capture_output=True, text=True, timeout=600, cwd=str(tmp_path))
        assert r.returncode == 0, r.stdout + r.stderr
        files[tag] = [pickle.load(open(out / f"sampled_{i}.pkl", "rb"))[0] for i in range(2)]
    xyz, atom_ok, nres = encode.read_backbone(pdb, "A")
    x = torch.zeros(1, L, 3, 3)
    ok = torch.zeros(1, L, 3, dtype=torch.uint8)
    x[0, :nres], ok[0, :nres] = torch.from_numpy(xyz), torch.from_numpy(atom_ok)
    enc = encode.encode_6d_batch(x.cuda(), torch.tensor([nres]), atom_ok=ok.cuda(), num_channels=Cn)["coords_6d"][0].cpu()
    inside = torch.arange(L) < nres
    redo = pair_mask(parse_mask_info("1:2,5", 1, L))[0]
    known = (~redo & inside[:, None] & inside[None, :])[None].expand(Cn, L, L).clone()
    known[-1] = False                                    # the length condition's channel
    assert int(known.sum()) > 0 and int((~known[:-1]).sum()) > 0
    for t in files["replace"]:
        assert t.shape == (Cn, L, L) and bool(torch.isfinite(t).all())
        assert torch.equal(t[known], enc[known])
        assert not torch.equal(t[:-1][~known[:-1] & (inside[:, None] & inside[None, :])[None].expand(Cn - 1, L, L)],
                               enc[:-1][~known[:-1] & (inside[:, None] & inside[None, :])[None].expand(Cn - 1, L, L)])
    assert not torch.equal(files["condition"][0][known], enc[known])


# ---- 9. refusals change nothing ---------------------------------------------------------------------------------------------
def test_refusals_change_nothing():
    from text2protein_amd import _lib, sampling
    from text2protein_amd._lib import T2PError, check, ptr, stream_ptr
    case, g, steps, cfg, model, sde, shape = _fixture("inpaint_replace_ve")
    eps = IO.EPS["vesde"]
    st, buf, xm, _ = _stepper(case, g, cfg, model, sde, shape, seed=5)
    start = buf.clone()
    a, s = sde.inpaint_tables(eps)
    data, kn = torch.from_numpy(g["data"]).cuda(), torch.from_numpy(g["known"]).cuda()
    lib = st.lib
    for args in ((None, None, a, s), (kn, data, None, None), (kn, None, a, s), (kn, data, a, None)):
        rc = lib.t2p_sampler_set_inpaint(st._h, ptr(args[0]), ptr(args[1]), ptr(args[2]), ptr(args[3]))
        assert rc != 0 and b"go together" in lib.t2p_last_error()
    with pytest.raises(T2PError, match="float32 CPU"):
        st.set_inpaint(kn, data, a[:-1].contiguous(), s)
    # the replacement set before is still the one that runs
    st.step(buf, xm)
    torch.cuda.synchronize()
    ref, rbuf, rxm, _ = _stepper(case, g, cfg, model, sde, shape, seed=5)
    ref.step(rbuf, rxm)
    torch.cuda.synchronize()
    assert torch.equal(bits(buf), bits(rbuf)) and torch.equal(bits(xm), bits(rxm)) and not torch.equal(bits(buf), bits(start))
    # injected replacement noise without a replacement
    st.set_inpaint()
    with pytest.raises(T2PError, match="set_inpaint first"):
        st.set_inpaint_noise(torch.zeros(shape, device="cuda"), None)
    # operators: a replacement without known / data, tables without a valid step
    n = int(np.prod(shape))
    out = torch.full((n,), SENT, device="cuda")
    z = torch.zeros(n, device="cuda")
    tabs = (a.cuda(), s.cuda())
    bad = [_replace(_lib.InpaintReplace, None, data), _replace(_lib.InpaintReplace, kn, None),
           _replace(_lib.InpaintReplace, kn, data, None, tabs, sde.N), _replace(_lib.InpaintReplace, kn, data, None, tabs, -1)]
    for r in bad:
        rc = lib.t2p_op_inpaint_predictor(ptr(z), ptr(z), None, ptr(z), None, None, ptr(out), None, None, n, 1.0, 0.0, 1.0, 1.0, 1.0, 0,
                                          C.byref(r), stream_ptr())
        torch.cuda.synchronize()
        assert rc != 0 and bool((out == SENT).all())
    rc = lib.t2p_op_inpaint_predictor(ptr(z), ptr(z), None, ptr(z), None, None, ptr(out), None, None, n, 1.0, 0.0, 1.0, 1.0, 1.0, 0, None,
                                      stream_ptr())
    assert rc != 0 and bool((out == SENT).all())
    from text2protein_amd import inpainting
    fn = inpainting.get_pc_inpainter(sde, sampling.ReverseDiffusionPredictor, sampling.LangevinCorrector, cfg.sampling.snr, eps=eps)
    with pytest.raises(T2PError, match="does not match the model"):
        fn(model, torch.zeros(2, 5, 8, 8), torch.zeros(2, 5, 8, 8), context=torch.from_numpy(g["context"]))
