"""The 3x3 convolution of the TRAINING step at the plans the benchmark batch sizes take (t2p_op_train_conv3x3), and the whole step at
batch 16 against its sixteen samples taken one at a time.

The trainer launches the engine's implicit GEMM in a form the sampler never uses: fp32 output on the 16-bit kernels, the per-sample
time-embedding bias on an fp32 output, N < ldc, and for the data gradient an in-place residual (dX += conv3x3(dY, wd), p.R == p.C).
Which kernel runs depends on M = B H W: up to the batch sizes of the other training tests everything is the 128 x 128 geometry; batch
16 takes the 512 x 128 dx-shared-stage kernel at 128 x 128 maps and the 256 x 128 tile at 64 x 64.  t2p_op_train_conv3x3 runs the
trainer's own code (train.h: train_conv3x3_forward / _backward) on explicit buffers; here every geometry is forced on it (plan switch
2, switch 47 for the dx-shared-stage kernel), the kernel that ran is read back from the profile hooks, and the results are held to
torch autograd in float64.

Oracle: F.conv2d(x, w, b, padding=1) + tbias in float64, dx / dw / dbias / dtbias from autograd.  In the 16-bit modes the operands of
each product are rounded to the 16-bit type first (x and w for y, dy and w for dx, dy and x for dw: conv2d is bilinear, so one autograd
pass over the rounded leaves gives exactly that), the oracle of tests/test_gpu_train16.py: the kernels are held to fp32-accumulation
level.  Bias, time-embedding bias and the column sums stay fp32.  Tolerances are the project's: exact-f32 path 2e-6 forward (TOL[0]
of test_gpu_ops.py), 3e-6 dx / dw (test_tgemm_convolution_weight_gradient), 2e-5 column sums (the norm backward tests); 16-bit
OP_TOL = 1e-5 (test_gpu_train16.py).
"""
import ctypes as C
import functools

import pytest
import torch
import torch.nn.functional as F

from helpers import cfg_smallC, rel_l2
from text2protein_amd.config import tiny_config
from test_gpu_train16 import OP_TOL, STEP_TOL

pytestmark = pytest.mark.gpu

TDT = {0: torch.float32, 1: torch.bfloat16, 2: torch.float16}
TC_NAME = {1: "bf16_t", 2: "f16_t"}
F32_TOL = dict(y=2e-6, dx=3e-6, dw=3e-6, colsum=2e-5)
TOL16 = dict(y=OP_TOL, dx=OP_TOL, dw=OP_TOL, colsum=2e-5)
GEOM_SWITCH = {(256, 128): 1, (128, 128): 2, (256, 256): 3, (512, 128): 4}      # plan switch 2 (plan.h: dma_geom)
PAD_SENTINEL = 12345.0


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


def profiled(lib, fn):
    """fn() between t2p_profile_begin / _end: the convolution launches it made, by kernel.  `dma`: {(kernel name, M, N, K): launches}
    on the LDS-DMA kernels; `reg`: {(M, N, K): launches} on the register-staged kernel (kind 2 of t2p_profile_shapes)."""
    check(lib, lib.t2p_profile_begin())
    try:
        fn()
    finally:
        o9 = (C.c_double * 9)()
        check(lib, lib.t2p_profile_end(o9))
    buf = C.create_string_buffer(1 << 16)
    check(lib, lib.t2p_profile_conv_kernels(buf, len(buf)))
    dma = {}
    for line in buf.value.decode().splitlines()[1:]:
        name, M, N, K, n = line.split(";")
        dma[(name, int(M), int(N), int(K))] = int(n)
    check(lib, lib.t2p_profile_shapes(buf, len(buf)))
    reg = {}
    for line in buf.value.decode().splitlines()[1:]:
        f = line.split(",")
        if f[0] == "2" and abs(int(f[4])) == 9:
            reg[(int(f[1]), int(f[2]), int(f[3]))] = int(f[6])
    assert sum(dma.values()) == int(o9[2]) and sum(reg.values()) == int(o9[8])
    return dma, reg


def dma_name(kernel, dt, BM, BN):
    """The prefix of an LDS-DMA instantiation's name: gemm_dxs_kernel<TC, BM, BN, ...> or gemm_dma_kernel<TC, BM, BN, ..., MODE = 1 ...>."""
    return f"{kernel}<{TC_NAME[dt]}, {BM}, {BN}, "


def nhwc(t, Cp, pad=0.0):
    """[B][C][H][W] -> [B][H][W][Cp] fp32, the pad columns = pad"""
    B, Cc, H, W = t.shape
    out = torch.full((B, H, W, Cp), float(pad))
    out[..., :Cc] = t.permute(0, 2, 3, 1)
    return out


@functools.lru_cache(maxsize=None)
def case_data(dt, B, H, W, Ci, Co, with_tbias, ref_samples=None):
    """Inputs without a zero border and the float64 reference of one case, computed once and shared by every plan the case runs under
    (never modified).  ref_samples: y / dx are referenced on these samples only (the batch-16 case); dw and the sums always in full."""
    g = torch.Generator().manual_seed(B * 1000003 + H * 1009 + Ci * 31 + Co + 7 * dt)
    x = torch.randn(B, Ci, H, W, generator=g) + 0.25
    w = torch.randn(Co, Ci, 3, 3, generator=g) / (9 * Ci) ** 0.5
    bias = torch.randn(Co, generator=g)
    tbias = torch.randn(B, Co, generator=g) if with_tbias else None
    dy = torch.randn(B, Co, H, W, generator=g) * 0.5 - 0.1
    rd = (lambda t: t.to(TDT[dt]).double()) if dt else (lambda t: t.double())
    sel = list(range(B)) if ref_samples is None else list(ref_samples)
    xr, wr, dyr = rd(x), rd(w).requires_grad_(True), rd(dy)
    xs = xr[sel].clone().requires_grad_(True)
    y = F.conv2d(xs, wr, bias.double(), padding=1)
    y.backward(dyr[sel])
    ref = dict(dx=xs.grad, dbias=dy.double().sum((0, 2, 3)), sel=sel)
    ref["y"] = y.detach() + (tbias.double()[sel][:, :, None, None] if with_tbias else 0.0)
    if with_tbias:
        ref["dtbias"] = dy.double().sum((2, 3))
    if ref_samples is None:
        ref["dw"] = wr.grad
    else:
        # conv2d's weight gradient as one product per sample over the unfolded windows (dW[co][ci, ky, kx] = sum_p dY[co][p] X[ci][p + k]);
        # the same sum as autograd's, checked against autograd on the referenced samples
        dw = torch.zeros(Co, Ci * 9, dtype=torch.float64)
        part = torch.zeros_like(dw)
        for b in range(B):
            d = dyr[b].reshape(Co, H * W) @ F.unfold(xr[b:b + 1], 3, padding=1)[0].T
            dw += d
            if b in sel:
                part += d
        assert rel_l2(part.reshape(Co, Ci, 3, 3), wr.grad) < 1e-12
        ref["dw"] = dw.reshape(Co, Ci, 3, 3)
    return dict(x=x, w=w, bias=bias, tbias=tbias, dy=dy, ref=ref)


def run_conv(lib, dt, d, Cip, Cop, fixed_order, backward=True, want_dx=True, seed=0):
    """One call of t2p_op_train_conv3x3 on the case's inputs.  dx / dw / dbias / dtbias start from random contents, y from NaN, the pad
    columns of dx from a sentinel and those of dy hold one too (they must not be read: wd is zero there).  Returns what the call wrote
    and what it ADDED to the gradients, after checking the pad columns."""
    x, w, dy = d["x"], d["w"], d["dy"]
    B, Ci, H, W = x.shape
    Co = w.shape[0]
    g = torch.Generator().manual_seed(991 + seed)
    y = torch.full((B, H, W, Cop), float("nan"), device="cuda")
    dx0 = nhwc(torch.randn(B, Ci, H, W, generator=g), Cip, PAD_SENTINEL)
    dw0, db0 = torch.randn(Co, Ci, 3, 3, generator=g), torch.randn(Co, generator=g)
    dtb0 = torch.randn(B, Co, generator=g) if d["tbias"] is not None else None
    dx = dev(dx0.clone()) if (backward and want_dx) else None
    dw, db = (dev(dw0.clone()), dev(db0.clone())) if backward else (None, None)
    dtb = dev(dtb0.clone()) if (backward and dtb0 is not None) else None
    check(lib, lib.t2p_op_train_conv3x3(dt, P(dev(nhwc(x, Cip))), P(dev(w)), P(dev(d["bias"])), P(dev(d["tbias"])) if dtb0 is not None else None,
                                        B, H, W, Ci, Co, Cip, Cop, P(y), P(dev(nhwc(dy, Cop, PAD_SENTINEL))) if backward else None,
                                        P(dx), P(dw), P(db), P(dtb), int(fixed_order), None))
    torch.cuda.synchronize()
    out = dict(y=y.cpu())
    assert torch.isfinite(out["y"]).all() and (out["y"][..., Co:] == 0).all() and not out["y"][..., Co:].signbit().any()
    if backward:
        out.update(dw=dw.cpu() - dw0, dbias=db.cpu() - db0, dw_raw=dw.cpu(), dbias_raw=db.cpu())
        if dx is not None:
            got = dx.cpu()
            assert torch.equal(got[..., Ci:], dx0[..., Ci:])                  # the pad columns of dx: untouched, bit for bit
            out.update(dx=got[..., :Ci] - dx0[..., :Ci], dx_raw=got)
        if dtb is not None:
            out.update(dtbias=dtb.cpu() - dtb0, dtbias_raw=dtb.cpu())
    return out


def errors(out, d):
    ref, Co = d["ref"], d["w"].shape[0]
    sel = ref["sel"]
    e = dict(y=rel_l2(out["y"][sel][..., :Co], ref["y"].permute(0, 2, 3, 1)))
    if "dw" in out:
        e.update(dw=rel_l2(out["dw"], ref["dw"]), dbias=rel_l2(out["dbias"], ref["dbias"]))
    if "dx" in out:
        e["dx"] = rel_l2(out["dx"][sel], ref["dx"].permute(0, 2, 3, 1))
    if "dtbias" in out:
        e["dtbias"] = rel_l2(out["dtbias"], ref["dtbias"])
    return e


def assert_errors(e, tol, what):
    print(f"{what}: " + ", ".join(f"{k} {v:.1e}" for k, v in e.items()))
    for k, v in e.items():
        assert v < tol["colsum" if k in ("dbias", "dtbias") else k], (what, k, v)


def same_bits(a, b, keys):
    return all(torch.equal(a[k], b[k]) for k in keys if k in a)


def conv16_under_plan(lib, dt, shape, geom, dxs, expect, fixed_order=1, ref_samples=None):
    """A 16-bit case twice under one forced plan (geom: the (BM, BN) of plan switch 2 or None = the library's choice; dxs: plan switch
    47): the kernel that ran is `expect` = (kernel, BM, BN) for the forward AND the data gradient, the two runs agree bit for bit in
    y and dx (and in dw, dbias, dtbias: fixed-order reductions), and the first is within OP_TOL of the rounded-operand oracle."""
    B, H, W, Ci, Co = shape
    d = case_data(dt, B, H, W, Ci, Co, True, ref_samples)
    outs = []
    try:
        check(lib, lib.t2p_debug_set(2, GEOM_SWITCH[geom] if geom else 0))
        check(lib, lib.t2p_debug_set(47, int(dxs)))
        for _ in range(2):
            dma, reg = profiled(lib, lambda: outs.append(run_conv(lib, dt, d, Ci, Co, fixed_order)))
            M = B * H * W
            want = {(M, Co, Ci): 1, (M, Ci, Co): 1} if Ci != Co else {(M, Co, Ci): 2}
            if expect[0] == "reg":                                      # the register-staged kernel (launch_tile)
                assert not dma and reg == want, (dma, reg)
            else:
                pre = dma_name(*((expect[0], dt) + expect[1:]))
                assert not reg and {k[1:]: n for k, n in dma.items()} == want and all(k[0].startswith(pre) for k in dma), (pre, dma, reg)
    finally:
        lib.t2p_debug_set(2, 0)
        lib.t2p_debug_set(47, 1)
    what = f"{TC_NAME[dt]} {shape} on {expect}"
    assert same_bits(outs[0], outs[1], ("y", "dx_raw")), what + ": y / dx differ between two runs"
    if fixed_order:
        assert same_bits(outs[0], outs[1], ("dw_raw", "dbias_raw", "dtbias_raw")), what + ": dw / sums differ between two runs"
    assert_errors(errors(outs[0], d), TOL16, what)
    return outs[0]


# ---- the tall and the square tile on power-of-two rows: the dx-shared-stage kernel and the kernel it replaces ---------------------
@pytest.mark.parametrize("dt", [2, 1])
@pytest.mark.parametrize("shape,geom", [((2, 64, 64, 64, 128), (512, 128)), ((2, 64, 64, 64, 256), (256, 256))])
def test_train_conv_tall_and_square_tiles(lib, dt, shape, geom):
    """gemm_dxs_kernel<.., 512, 128, ..> / <.., 256, 256, ..> forced on the training parameterisation: fp32 output + bias + the per-sample
    time-embedding bias (forward) and the in-place residual (dx), N = Ci = 64 < BN for dx.  Then the same with plan switch 47 off:
    gemm_dma_kernel on the same tile, bit-identical to the dxs run (same K order, same MFMA order, same epilogue)."""
    a = conv16_under_plan(lib, dt, shape, geom, True, ("gemm_dxs_kernel",) + geom)
    b = conv16_under_plan(lib, dt, shape, geom, False, ("gemm_dma_kernel",) + geom)
    assert same_bits(a, b, ("y", "dx_raw", "dw_raw", "dbias_raw", "dtbias_raw"))


# ---- rows that are no power of two: tiles that span two samples (the two_b bias edge), every geometry ------------------------------
@pytest.mark.parametrize("dt", [2, 1])
@pytest.mark.parametrize("geom", [(256, 128), (256, 256), (512, 128), (128, 128)])
def test_train_conv_tiles_spanning_two_samples(lib, dt, geom):
    """W = 24 (never the dxs kernel), samples of 576 rows: every tile geometry has tiles that hold the end of one sample and the start
    of the next (the time-embedding bias changes inside the tile), M = 1728 is no multiple of any tile (rows past M are dropped)."""
    conv16_under_plan(lib, dt, (3, 24, 24, 128, 128), geom, True, ("gemm_dma_kernel",) + geom)


@pytest.mark.parametrize("dt", [2, 1])
@pytest.mark.parametrize("geom", [None, (256, 256)])
def test_train_conv_samples_shorter_than_a_tile(lib, dt, geom):
    """8 x 8 maps, 9 samples: rows_per_batch = 64 < BM with the time-embedding bias and the in-place residual.  The library's own choice
    here is the 128 x 128 geometry: the generic loop of the LDS-staged epilogue (a sample index per row).  256 x 256 tiles hold four
    samples each: the register epilogue's sample index per 16-row tile."""
    conv16_under_plan(lib, dt, (9, 8, 8, 256, 256), geom, True, ("gemm_dma_kernel",) + (geom or (128, 128)))


@pytest.mark.parametrize("dt", [2, 1])
def test_train_conv_register_staged_16bit(lib, dt):
    """Channels that are no multiple of 64 (16 -> 24): the register-staged 16-bit kernel on a 16-bit A operand (a_f32 = 0)."""
    conv16_under_plan(lib, dt, (3, 12, 12, 16, 24), None, True, ("reg",))


@pytest.mark.parametrize("dt", [2, 1])
def test_train_conv_batch16_plan_at_64x64(lib, dt):
    """The plan batch 16 really takes at the 64 x 64 level (nothing forced): M = 65536, the 256 x 128 tile for the forward and the data
    gradient; K = 65536 rows for the gathered weight gradient with the library's split-K.  y / dx against float64 on samples 0, 7, 15;
    dw, dbias, dtbias in full."""
    conv16_under_plan(lib, dt, (16, 64, 64, 64, 128), None, True, ("gemm_dma_kernel", 256, 128), ref_samples=(0, 7, 15))


# ---- the exact-f32 kernels: the input and head convolutions in every mode, everything in the f32 step ------------------------------
@pytest.mark.parametrize("shape,Cip,Cop,tbias,want_dx", [
    ((1, 128, 128, 64, 128), 64, 128, True, True),       # launch_tile: 128 x 128 tiles (128 of them)
    ((2, 12, 12, 24, 40), 24, 40, True, True),           # launch_tile: 64 x 64 tiles
    ((2, 16, 16, 64, 5), 64, 8, False, True),            # the head: N = 5 < ldc = 8, wd padded to Cop
    ((2, 16, 16, 5, 64), 8, 64, False, False),           # the input convolution: Ci = 5 < Cip = 8 (wf padded), x needs no gradient
])
@pytest.mark.parametrize("fixed_order", [0, 1])
def test_train_conv_f32(lib, shape, Cip, Cop, tbias, want_dx, fixed_order):
    B, H, W, Ci, Co = shape
    d = case_data(0, B, H, W, Ci, Co, tbias)
    outs = []
    dma, reg = profiled(lib, lambda: outs.append(run_conv(lib, 0, d, Cip, Cop, fixed_order, want_dx=want_dx)))
    M = B * H * W
    want = {(M, Co, Cip): 1}
    if want_dx:
        want[(M, Ci, Cop)] = want.get((M, Ci, Cop), 0) + 1
    assert not dma and reg == want, (dma, reg)
    assert ("dx" in outs[0]) == want_dx
    assert_errors(errors(outs[0], d), F32_TOL, f"f32 {shape} Cip {Cip} Cop {Cop} fixed_order {fixed_order} on the register-staged kernel")


# ---- layouts alone --------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dt", [0, 2, 1])
def test_train_conv_weight_layouts_name_one_tap(lib, dt):
    """conv_w_prep (wf, the flipped transposed wd, the padding for Cip > Ci and Cop > Co) and conv_w_grad_fold through the op, with
    integer weights that are all different and one-hot x and dy: every entry of y and dx is ONE weight, dw is ONE tap -- exact in every
    dtype, so a flip or a transposition slip (8 - t, ky <-> kx, co <-> ci) fails by itself and not inside a tolerance.  The pixel of
    dy sits at (+1, -1) from the pixel of x: the tap it names is (ky, kx) = (0, 2), which no symmetry maps to itself."""
    B, H, W, Ci, Co, Cip, Cop = 2, 6, 5, 3, 5, 8, 8
    w = (torch.randperm(Co * Ci * 9, generator=torch.Generator().manual_seed(3)) + 1).float().reshape(Co, Ci, 3, 3)
    x = torch.zeros(B, Ci, H, W)
    dy = torch.zeros(B, Co, H, W)
    x[1, 2, 2, 3] = 1.0
    dy[1, 3, 3, 2] = 1.0
    xr, wr = x.double().requires_grad_(True), w.double().requires_grad_(True)
    y = F.conv2d(xr, wr, padding=1)
    y.backward(dy.double())
    assert int((wr.grad != 0).sum()) == 1 and wr.grad[3, 2, 0, 2] == 1
    d = dict(x=x, w=w, bias=torch.zeros(Co), tbias=None, dy=dy)
    g = run_conv(lib, dt, d, Cip, Cop, 1)
    assert torch.equal(g["y"][..., :Co].double(), y.detach().permute(0, 2, 3, 1))
    # (dx and dw were accumulated into random fp32 contents: the added part is exact up to the rounding of that sum)
    assert (g["dx"].double() - xr.grad.permute(0, 2, 3, 1)).abs().max() < 1e-4 and (g["dw"].double() - wr.grad).abs().max() < 1e-6
    assert (g["dbias"].double() - dy.double().sum((0, 2, 3))).abs().max() < 1e-6


# ---- the whole step: a batch of 16 equals its samples taken one at a time ---------------------------------------------------------
def cfg_batch16():
    """cfg_smallC grown to the levels of cond_length.yml: 128 x 128 maps, nf = 64, four levels (128, 64, 32, 16), one residual block
    each, attention at 16 x 16 only, `length` condition, dropout 0.1 (masks injected)."""
    base = cfg_smallC()
    cfg = tiny_config(**{"model.nf": 64, "model.ch_mult": [1, 1, 2, 2], "model.num_res_blocks": 1, "data.max_res_num": 128,
                         "model.attn_resolutions": [16], "model.n_heads": base.model.n_heads, "model.context_dim": base.model.context_dim,
                         "model.condition": ["length"], "model.dropout": 0.1, "model.num_scales": 100})
    cfg.device = "cuda:0"
    return cfg


def batch16_inputs(cfg, B):
    from text2protein_amd import synth
    import numpy as np
    Cc, L, seed = cfg.data.num_channels, cfg.data.max_res_num, 21
    lengths = [40 + (88 * b) // (B - 1) for b in range(B)]                 # 40 .. 128
    x = torch.from_numpy(synth.uniform_pm1(seed, "train_coords", B * Cc * L * L).reshape(B, Cc, L, L))
    mp = torch.zeros(B, L, L).bool()
    for b, n in enumerate(lengths):
        mp[b, :n, :n] = True
    x = x * mp.unsqueeze(1)
    x[:, -1] = mp.float()
    # t spread over (eps, 1), not sorted by length: sigma from 0.01 to 100, per-sample gradient magnitudes orders apart
    t = torch.tensor([1e-5 + (1.0 - 1e-5) * ((5 * b + 3) % B + 0.5) / B for b in range(B)], dtype=torch.float32)
    z = torch.from_numpy(synth.normal(seed, "train_z", B * Cc * L * L).reshape(B, Cc, L, L))
    ctx = synth.synth_context(B, 6, cfg.model.context_dim, seed + 31)
    return dict(coords_6d=x, mask_pair=mp, context=ctx), t, z


def batch16_masks(cfg, model, B):
    """One keep-mask per residual block in forward order, NHWC uint8 [B][side][side][co] (p = dropout)."""
    from oracle import t2p_oracle as O
    inputs, mid, outs = O.unet_plan(cfg)
    table = dict(model.param_table())
    g = torch.Generator().manual_seed(77)
    masks, side = [], cfg.data.max_res_num
    for stage in inputs + [mid] + outs:
        for kind, prefix, up, down in stage:
            if kind != "res":
                continue
            side = side * 2 if up else side // 2 if down else side
            co = table[prefix + ".Conv_1.weight"][0]
            masks.append((torch.rand(B, side, side, co, generator=g) >= cfg.model.dropout).to(torch.uint8))
    return masks


# The distance between the two sides.  f32: the bounds of test_gpu_train.py (LOSS_TOL, the score bound, GRAD_TOL).  16-bit: about 2x the
# deviation measured on the MI355X (the docstring of the test), far below the 16-bit step's own distance from the fp32 reference
# (STEP_TOL of test_gpu_train16.py, the ceiling).  The measured score deviation is zero, so the scores are held bit for bit (score = 0.0
# means torch.equal).  The loss is ONE float32 on each side: the batch side rounds a double sum once, the single side is the double mean
# of sixteen rounded float32 -- at most one float32 spacing apart (1.2e-7 relative; measured 1.5e-8), asserted at two.
BATCH16_TOL = {
    "f32": dict(loss=1e-5, score=1e-5, grad=1e-4),
    "f16": dict(loss=2.4e-7, score=0.0, grad=1e-6),
    "bf16": dict(loss=2.4e-7, score=0.0, grad=1e-6),
}
assert all(BATCH16_TOL[d][k] <= STEP_TOL[d][k] for d in ("f16", "bf16") for k in ("loss", "score", "grad"))


@pytest.mark.parametrize("dtype", ["f32", "f16", "bf16"])
def test_training_step_batch16_equals_its_samples(lib, dtype):
    """loss(B = 16) = mean_b loss(sample b), grad(B = 16) = 1/16 sum_b grad(sample b), score(B = 16)[b] = score(sample b) for given t, z and
    dropout masks: the loss is a mean over the batch and no operator of the forward couples samples (GroupNorm statistics, attention
    and the time-embedding bias are per sample).  The single-sample side runs the plans train_cond_length pins to the reference's
    autograd (128 x 128 tiles everywhere); the batch side runs the benchmark's: the profile hooks must show gemm_dxs_kernel<.., 512,
    128, ..> for its 128 x 128 maps and the 256 x 128 tile for its 64 x 64 maps in the 16-bit modes, and neither on the single side.
    Gradients per tensor against max(|tensor|, 3e-5 of the whole gradient's norm), the measure of test_gpu_train.py.

    Measured on the MI355X (loss rel / worst per-sample score rel-L2 / worst gradient rel-L2 over 384 tensors):
    f32 1.9e-8 / 0 / 3.1e-6, f16 1.5e-8 / 0 / 4.8e-7, bf16 7.5e-9 / 0 / 5.0e-7.  The forward pass is bit-identical between the plans in
    every mode (each output element sums its K products in the same order on every tile geometry); the gradients differ only by the
    order of the sums over pixels and samples (f32: atomics; 16-bit: fixed order, but another split of the rows).  The backward seed
    scale of the VE loss is a host power of two, 2^round(log2(B C L L)): at B = 16 exactly 16 times the single-sample one, which cancels
    the 1 / B of the seed, so each sample's backward pass starts from the same values on both sides."""
    from text2protein_amd import losses, synth
    from text2protein_amd.losses import HipTrainModel
    B = 16
    cfg = cfg_batch16()
    batch, t, z = batch16_inputs(cfg, B)
    model = HipTrainModel(cfg, device="cuda:0", seed=11, dtype=dtype)
    model.load_state_dict(synth.synth_state_dict(cfg, 9))
    masks = batch16_masks(cfg, model, B)
    L, nf = cfg.data.max_res_num, cfg.model.nf
    dt = {"f32": 0, "bf16": 1, "f16": 2}[dtype]

    def one_pass(sl):
        model.set_dropout_masks([m[sl] for m in masks])
        res = []
        dma, reg = profiled(lib, lambda: res.append(model.loss({k: v[sl] for k, v in batch.items()}, t=t[sl], z=z[sl], backward=True,
                                                               return_score=True)))
        return res[0][0], res[0][1].cpu(), {n: v.double() for n, v in model.read(losses.GRAD).items()}, dma, reg

    loss_b, score_b, grad_b, dma_b, reg_b = one_pass(slice(0, B))
    tall = dma_name("gemm_dxs_kernel", dt, 512, 128) if dt else None
    mid = dma_name("gemm_dma_kernel", dt, 256, 128) if dt else None
    if dt:
        at128 = {k: n for k, n in dma_b.items() if k[1] == B * L * L}
        at64 = {k: n for k, n in dma_b.items() if k[1] == B * L * L // 4}
        assert at128 and all(k[0].startswith(tall) for k in at128), at128
        assert at64 and all(k[0].startswith(mid) for k in at64), at64
        print(f"{dtype} batch 16: " + "; ".join(f"{n} x {k[0]} M {k[1]} N {k[2]} K {k[3]}" for k, n in sorted(dma_b.items())))
    else:
        assert not dma_b and any(k[0] == B * L * L for k in reg_b)
    loss_s, grad_s = 0.0, None
    score_s = torch.empty_like(score_b)
    for b in range(B):
        l1, s1, g1, dma_1, reg_1 = one_pass(slice(b, b + 1))
        if dt:
            assert dma_1 and not any(k[0].startswith(tall) or k[0].startswith(mid) for k in dma_1), dma_1
        loss_s += l1 / B
        score_s[b] = s1[0]
        grad_s = g1 if grad_s is None else {n: grad_s[n] + g1[n] for n in g1}
    grad_s = {n: v / B for n, v in grad_s.items()}
    T = float(torch.sqrt(sum((v ** 2).sum() for v in grad_s.values())))
    # the scores are real ones: non-zero, different from sample to sample, orders of magnitude apart (t spread over (eps, 1))
    rms = score_s.double().pow(2).mean((1, 2, 3)).sqrt()
    assert float(rms.min()) > 0 and float(rms.max() / rms.min()) > 100
    e_loss = abs(loss_b - loss_s) / abs(loss_s)
    e_score = max(rel_l2(score_b[b], score_s[b]) for b in range(B))
    e_grad, worst = max((float((grad_b[n] - grad_s[n]).norm()) / max(float(grad_s[n].norm()), 3e-5 * T), n) for n in grad_s)
    print(f"{dtype} batch 16 against its 16 samples: loss {loss_b:.6f} vs {loss_s:.6f} (rel {e_loss:.1e}), worst per-sample score rel-L2 "
          f"{e_score:.1e}, worst gradient rel-L2 {e_grad:.1e} over {len(grad_s)} tensors ({worst})")
    tol = BATCH16_TOL[dtype]
    assert e_loss < tol["loss"] and e_grad < tol["grad"]
    assert e_score < tol["score"] or (tol["score"] == 0.0 and torch.equal(score_b, score_s))
