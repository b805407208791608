"""The reductions and the seed scale that only the 16-bit training step uses, one operator at a time through the C ABI
(t2p_op_groupnorm_backward_form, t2p_op_layernorm_backward_form, t2p_op_colsum, t2p_op_sumsq, t2p_op_seed_scale).

They are fp32 (sumsq: double) arithmetic whatever the product type, so each is held to a float64 reference on the CPU -- torch autograd
for the norms, plain sums otherwise -- at the tolerance its atomic form already meets (GroupNorm 2e-5, LayerNorm 1e-5, test_gpu_train.py;
column sums OP_TOL = 1e-5, test_gpu_train16.py; sumsq 1e-12: double accumulation of squares that are exact in double, n 2^-53 at most),
at the smallest shapes that cross each kernel's internal boundaries (row chunks of 256, 64-column blocks, 4 row lanes, 64-pixel
GroupNorm chunks, the 1024-block grid of sumsq).  Every output is pre-filled, so accumulate and overwrite are both checked; each fixed
form is called twice (bit-identical) and against the atomic form of the same call.
"""
import ctypes as C
import math

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import test_gpu_train as TG
from helpers import rel_l2
from test_gpu_train import GN_BWD_SHAPES, P, check, dev, groupnorm_backward_case
from test_gpu_train16 import OP_TOL

pytestmark = pytest.mark.gpu

GN_TOL = 2e-5        # test_gpu_train.test_groupnorm_backward
LN_TOL = 1e-5        # test_gpu_train.test_layernorm_backward
SUMSQ_TOL = 1e-12

_WORST = {}


@pytest.fixture(scope="module")
def lib():
    from text2protein_amd import _lib
    return _lib.load()


@pytest.fixture(autouse=True)
def _release_device_tensors():
    yield
    torch.cuda.synchronize()
    TG._KEEP.clear()


@pytest.fixture(scope="module", autouse=True)
def _record_worst():
    """The measured worst errors of this module, next to the suite's other parity figures."""
    yield
    if _WORST:
        from test_gpu_baseline import _record
        _record("train_reductions", dict(_WORST))


def _note(key, value):
    _WORST[key] = max(_WORST.get(key, 0.0), float(value))


# ---- GroupNorm backward: gn_bwd_finalize_kernel<false> + gn_bwd_param_sum_kernel ------------------------------------------------------------
# test_groupnorm_backward's list, then: B = 1 and 3; HW = 16 (one short 64-pixel chunk) and 100 (a ragged second chunk); C = 512 (the c0
# loop of the partial kernel); C = 96 (C < 256 with 256 % C != 0: no pixel lanes)
GN_FORM_SHAPES = GN_BWD_SHAPES + [(1, 100, 96, 24, 1), (3, 16, 96, 24, 0), (3, 100, 512, 32, 1), (1, 16, 32, 8, 0), (3, 100, 32, 8, 1)]


@pytest.mark.parametrize("B,HW,Cc,G,silu", GN_FORM_SHAPES)
def test_groupnorm_backward_forms(lib, B, HW, Cc, G, silu):
    fixed, e_fixed = groupnorm_backward_case(lib, B, HW, Cc, G, silu, fixed_order=1)
    again, _ = groupnorm_backward_case(lib, B, HW, Cc, G, silu, fixed_order=1)
    atomic, e_atomic = groupnorm_backward_case(lib, B, HW, Cc, G, silu, fixed_order=0)
    e_forms = [rel_l2(a, b) for a, b in zip(fixed, atomic)]
    print(f"GroupNorm backward B {B} HW {HW} C {Cc}: fixed order dx / dgamma / dbeta " + " / ".join(f"{e:.1e}" for e in e_fixed) +
          "; atomic " + " / ".join(f"{e:.1e}" for e in e_atomic) + "; fixed vs atomic " + " / ".join(f"{e:.1e}" for e in e_forms))
    _note("groupnorm_backward_fixed", max(e_fixed))
    assert max(e_fixed) < GN_TOL and max(e_atomic) < GN_TOL and max(e_forms) < GN_TOL
    assert all(torch.equal(a, b) for a, b in zip(fixed, again))


# ---- LayerNorm backward: ln_bwd_rows_kernel / ln_bwd_cols_kernel / ln_bwd_cols_finish_kernel ------------------------------------------------
def _layernorm_backward(lib, rows, Cc, fixed_order):
    g = torch.Generator().manual_seed(rows * 7 + Cc)
    x = (torch.randn(rows, Cc, generator=g) * 1.5 - 0.2).double().requires_grad_(True)
    gamma = (1 + 0.2 * torch.randn(Cc, generator=g)).double().requires_grad_(True)
    beta = torch.zeros(Cc).double().requires_grad_(True)
    dy = torch.randn(rows, Cc, generator=g).double()
    F.layer_norm(x, (Cc,), gamma, beta, eps=1e-5).backward(dy)
    dx0, dg0, db0 = torch.randn(rows, Cc, generator=g), torch.randn(Cc, generator=g), torch.randn(Cc, generator=g)   # accumulated into
    dx, dg, db = dev(dx0.clone()), dev(dg0.clone()), dev(db0.clone())
    check(lib, lib.t2p_op_layernorm_backward_form(P(dev(x.detach().float())), P(dev(dy.float())), P(dev(gamma.detach().float())), rows, Cc,
                                                 1e-5, P(dx), P(dg), P(db), fixed_order, None))
    torch.cuda.synchronize()
    got = (dx.cpu() - dx0, dg.cpu() - dg0, db.cpu() - db0)
    return got, (rel_l2(got[0], x.grad), rel_l2(got[1], gamma.grad), rel_l2(got[2], beta.grad))


@pytest.mark.parametrize("Cc", [32, 96, 256, 1000, 1024])
@pytest.mark.parametrize("rows", [1, 3, 255, 257, 600])
def test_layernorm_backward_forms(lib, rows, Cc):
    """One wave per row, 256-row column chunks, 256-channel blocks: rows below, at and past one chunk (600: two full chunks and a ragged
    third), channel counts below a wave's 64 lanes, off the block size and over several blocks."""
    fixed, e_fixed = _layernorm_backward(lib, rows, Cc, 1)
    again, _ = _layernorm_backward(lib, rows, Cc, 1)
    atomic, e_atomic = _layernorm_backward(lib, rows, Cc, 0)
    e_forms = [rel_l2(a, b) for a, b in zip(fixed, atomic)]
    print(f"LayerNorm backward {rows} x {Cc}: fixed order dx / dgamma / dbeta " + " / ".join(f"{e:.1e}" for e in e_fixed) +
          "; atomic " + " / ".join(f"{e:.1e}" for e in e_atomic) + "; fixed vs atomic " + " / ".join(f"{e:.1e}" for e in e_forms))
    _note("layernorm_backward_fixed", max(e_fixed))
    assert max(e_fixed) < LN_TOL and max(e_atomic) < LN_TOL and max(e_forms) < LN_TOL
    assert all(torch.equal(a, b) for a, b in zip(fixed, again))


# ---- column sums: colsum_partial_kernel / colsum_finish_kernel -----------------------------------------------------------------------------
def _colsum_case(lib, nz, rows, N, ld):
    """Both forms, overwrite and accumulate, out rows of N + 2 floats pre-filled (columns N.. must come back untouched).  dy has mean
    0.25, so that no column sum is a cancellation to near zero that a relative bound could not hold in fp32."""
    g = torch.Generator().manual_seed(nz * 100003 + rows * 131 + N * 7 + ld)
    ld_out = N + 2
    dy = torch.randn(nz * rows, ld, generator=g) + 0.25
    out0 = torch.randn(nz, ld_out, generator=g)
    sums = dy.double().reshape(nz, rows, ld)[:, :, :N].sum(1)
    d_dy = dev(dy)
    got = {}
    for fixed in (1, 0):
        for acc in (0, 1):
            want = out0.double().clone()
            want[:, :N] = sums + (out0[:, :N].double() if acc else 0.0)
            runs = []
            for _ in range(2 if fixed else 1):
                out = dev(out0.clone())
                check(lib, lib.t2p_op_colsum(P(d_dy), nz, rows, N, ld, P(out), ld_out, acc, fixed, None))
                torch.cuda.synchronize()
                runs.append(out.cpu())
            o = runs[0]
            assert torch.equal(o[:, N:], out0[:, N:]), (fixed, acc, "columns N.. of out were written")
            e = rel_l2(o[:, :N], want[:, :N])
            _note("colsum_fixed" if fixed else "colsum_atomic", e)
            assert e < OP_TOL, (fixed, acc, e)
            assert all(torch.equal(o, r) for r in runs[1:]), (acc, "the fixed-order form differs between two calls")
            got[(fixed, acc)] = o
    for acc in (0, 1):
        assert rel_l2(got[(1, acc)][:, :N], got[(0, acc)][:, :N]) < OP_TOL


@pytest.mark.parametrize("nz", [1, 3])
@pytest.mark.parametrize("N", [1, 5, 64, 65, 130])
@pytest.mark.parametrize("rows", [1, 3, 255, 256, 257, 700])
def test_colsum_forms(lib, rows, N, nz):
    """256 rows per chunk, 64 columns per block, 4 row lanes: fewer rows than lanes, one row short of / exactly / one row past a chunk,
    two chunks and a ragged third; columns below, at and past one block and past two; one sample (bias gradients) and three (the
    per-sample time-embedding bias); dy rows of N + 3 floats."""
    _colsum_case(lib, nz, rows, N, N + 3)


@pytest.mark.parametrize("rows", [257, 700])
def test_colsum_head_convolution_layout(lib, rows):
    """The head convolution's dY: 5 of 8 columns."""
    _colsum_case(lib, 1, rows, 5, 8)


# ---- sum of squares: sumsq_partial_kernel / sumsq_finish_kernel -------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [1, 255, 256 * 1024 + 1, 1_000_003])
def test_sumsq_forms(lib, n):
    """One element, less than a block, one element past one pass of the 1024-block grid, and several passes with a ragged end; |g| from
    1e-6 to 1e3.  The reference is the correctly rounded sum (math.fsum) of the squares, which are exact in double."""
    g = torch.Generator().manual_seed(n)
    mag = 10.0 ** (torch.rand(n, generator=g, dtype=torch.float64) * 9.0 - 6.0)
    x = (mag * torch.where(torch.rand(n, generator=g) < 0.5, -1.0, 1.0)).float()
    want = math.fsum((x.double() ** 2).tolist())
    d = dev(x)
    res = {}
    for fixed in (1, 0):
        vals = []
        for _ in range(2 if fixed else 1):
            out = C.c_double(-1.0)
            check(lib, lib.t2p_op_sumsq(P(d), n, fixed, C.byref(out), None))
            vals.append(out.value)
        res[fixed] = vals[0]
        e = abs(vals[0] - want) / want
        print(f"sumsq n {n} {'fixed order' if fixed else 'atomic'}: {vals[0]!r} against {want!r}, rel {e:.1e}")
        _note("sumsq_fixed" if fixed else "sumsq_atomic", e)
        assert e < SUMSQ_TOL, (fixed, e)
        assert all(v == vals[0] for v in vals), "the fixed-order form differs between two calls"
    assert abs(res[1] - res[0]) <= SUMSQ_TOL * want


# ---- the device-chosen seed scale: absmax_kernel + seed_scale_kernel --------------------------------------------------------------------------
def _f32(v):
    return float(np.float32(v))


def _expected_scale(m, target):
    """S = 2^e, e the largest integer with 2^e m <= target, clamped to [-60, 60]; from the operands' own exponents (math.frexp), no quotient."""
    if not (m > 0.0 and math.isfinite(m)):
        return 1.0
    fm, em = math.frexp(m)
    ft, et = math.frexp(target)
    e = et - em - (1 if ft < fm else 0)
    if -60 <= e <= 60:                      # the contract proper, checked exactly (a power of two times a float32 is exact in double)
        assert math.ldexp(m, e) <= target < math.ldexp(m, e + 1)
    return math.ldexp(1.0, min(max(e, -60), 60))


def _seed_scale(lib, x, target):
    out = (C.c_float * 2)(-1.0, -1.0)
    check(lib, lib.t2p_op_seed_scale(P(dev(x)), x.numel(), target, out, None))
    return float(out[0]), float(out[1])


_UP = lambda v: _f32(np.nextafter(np.float32(v), np.float32(np.inf)))
_DOWN = lambda v: _f32(np.nextafter(np.float32(v), np.float32(0.0)))


@pytest.mark.parametrize("target", [64.0, 48.0])
@pytest.mark.parametrize("what", ["1.0", "0.75", "target", "above target", "below target", "1.5 * 2^-40", "1.25 * 2^30", "1e-30", "subnormal", "1e30"])
def test_seed_scale_maximum(lib, what, target):
    """max|x| at the values where a power of two can come out wrong by one: at, just above and just below the target (64, what the trainer
    passes, and 48, whose mantissa is not 1), far from it but inside the clamp (1.5 * 2^-40 and 1.25 * 2^30: the unclamped exponent, 45 and -25 for 64), and far outside, where
    the exponent is clamped to +-60 (a subnormal maximum overflows target / max to infinity, so the exponent must come from max itself)."""
    m = {"1.0": 1.0, "0.75": 0.75, "target": target, "above target": _UP(target), "below target": _DOWN(target), "1.5 * 2^-40": 1.5 * 2.0 ** -40,
         "1.25 * 2^30": 1.25 * 2.0 ** 30, "1e-30": _f32(1e-30),
         "subnormal": _f32(3e-39), "1e30": _f32(1e30)}[what]
    assert what != "subnormal" or 0.0 < m < _f32(np.finfo(np.float32).tiny)
    g = torch.Generator().manual_seed(5)
    for sign in (1.0, -1.0):                 # the maximum carried by a positive and by a negative element
        x = (torch.rand(1000, generator=g, dtype=torch.float64) - 0.5) * m        # |.| <= m / 2
        x[123] = sign * m
        x = x.float()
        assert float(x.abs().max()) == m
        S, inv = _seed_scale(lib, x, target)
        want = _expected_scale(m, target)
        print(f"seed scale: max|x| {m!r} ({what}, sign {sign:+.0f}), target {target}: S {S!r}, 1 / S {inv!r}, expected {want!r}")
        assert S == want and inv == 1.0 / want, (what, sign, S, inv, want)


def test_seed_scale_last_element_zeros_and_non_finite(lib):
    n = 256 * 1024 + 1                       # one element past one pass of absmax_kernel's 1024-block grid
    g = torch.Generator().manual_seed(6)
    x = (torch.rand(n, generator=g) - 0.5) * 1e-3
    x[-1] = -3.0
    assert _seed_scale(lib, x, 64.0) == (16.0, 1.0 / 16.0) == (_expected_scale(3.0, 64.0), 1.0 / 16.0)
    assert _seed_scale(lib, torch.zeros(1000), 64.0) == (1.0, 1.0)
    for bad in (float("inf"), float("-inf"), float("nan")):
        y = x[:1000].clone()
        y[17] = bad
        assert _seed_scale(lib, y, 64.0) == (1.0, 1.0), bad
