"""The row-resident K = 512 GEMM (rowgemm.hip, plan switch 49) against the 256 x 256 16x16x32 kernel it replaces at the 32 x 32 level.

Every case runs one launch twice, with the switch at 0 (the LDS-DMA kernel) and at 2 (the row-resident kernel wherever it is
eligible), and asserts that the two outputs are the same bits -- the same MFMA, the same assignment of k to fragment positions, the
same K order and the same epilogue arithmetic -- and that the key-0 result agrees with an fp64 product as test_gemm asks.

The tile geometry is pinned to 256 x 256 (development key 2 = 3) for both runs: that is the plan the products take at the sizes the
planner gives the new kernel (M >= 16384).  Left alone, the planner runs these small test shapes on 128 x 128 tiles with the
32x32x16 MFMA, which sums the 64 k of a K-tile in four steps of 16 instead of two of 32 and so rounds differently: not the kernel the
new one stands in for.  t2p_debug_rowres_launches tells which kernel a launch took."""
import ctypes as C

import pytest
import torch

from helpers import rel_l2

pytestmark = pytest.mark.gpu

TOL = {1: 6e-3, 2: 8e-4}              # rel-L2 of one rounding to bf16 / fp16 (test_gpu_ops.TOL)
TDT = {1: torch.bfloat16, 2: torch.float16}
PAD = 8                                # extra columns of a padded ldc (rows stay 16-byte aligned)


@pytest.fixture(scope="module")
def lib():
    from text2protein_amd import _lib
    return _lib.load()


def P(t):
    return C.c_void_p(t.data_ptr())


def check(lib, rc):
    assert rc == 0, lib.t2p_last_error().decode()


def both(lib, launch, expect_new):
    """launch(out) with the switch at 0 and at 2 -> the two outputs; expect_new: the second run takes the new kernel"""
    outs = []
    try:
        check(lib, lib.t2p_debug_set(2, 3))
        for key in (0, 2):
            check(lib, lib.t2p_debug_set(49, key))
            n0 = lib.t2p_debug_rowres_launches()
            out = launch()
            torch.cuda.synchronize()
            assert lib.t2p_debug_rowres_launches() - n0 == (1 if key == 2 and expect_new else 0)
            outs.append(out.cpu())
    finally:
        lib.t2p_debug_set(49, 1)
        lib.t2p_debug_set(2, 0)
    return outs


def operands(dt, M, N, K, seed):
    g = torch.Generator().manual_seed(seed)
    a = torch.randn(M, K, generator=g).to(TDT[dt])
    w = (torch.randn(N, K, generator=g) / K ** 0.5).to(TDT[dt])
    bias = torch.randn(N, generator=g)
    res = torch.randn(M, N, generator=g).to(TDT[dt])
    return a, w, bias, res


@pytest.mark.parametrize("dt", [1, 2])
@pytest.mark.parametrize("M,N", [(128, 64),        # one slice: seven waves without one
                                 (256, 576),       # nine slices: wave 0 has two, N is no multiple of 512
                                 (384, 1536)])     # three slices per wave, three workgroups
def test_plain(lib, dt, M, N):
    K, ldc = 512, N + PAD
    a, w, _, _ = operands(dt, M, N, K, M + N)
    da, dw = a.cuda(), w.cuda()
    sentinel = torch.full((M, ldc), 3.0, dtype=TDT[dt])

    def launch():
        out = sentinel.cuda()
        check(lib, lib.t2p_op_gemm(dt, P(da), 0, P(dw), P(out), 0, M, N, K, K, K, ldc, None, None, 1.0, None))
        return out

    old, new = both(lib, launch, True)
    assert torch.equal(old, new)
    assert torch.equal(new[:, N:], sentinel[:, N:])                      # the padding of a wide ldc is not written
    assert rel_l2(old[:, :N].float(), a.double() @ w.double().T) < 2 * TOL[dt]


@pytest.mark.parametrize("dt", [1, 2])
def test_bias_residual_in_place(lib, dt):
    """attn*.to_out: bias, the 16-bit residual and the output in the same buffer, alpha != 1"""
    M, N, K, ldc = 256, 512, 512, 512 + PAD
    a, w, bias, res = operands(dt, M, N, K, 7)
    da, dw, db = a.cuda(), w.cuda(), bias.cuda()
    start = torch.full((M, ldc), 3.0, dtype=TDT[dt])
    start[:, :N] = res

    def launch():
        out = start.cuda()
        check(lib, lib.t2p_op_gemm_r16(dt, P(da), 0, P(dw), P(out), 0, M, N, K, K, K, ldc, P(db), P(out), 0.5, None))
        return out

    old, new = both(lib, launch, True)
    assert torch.equal(old, new)
    assert torch.equal(new[:, N:], start[:, N:])
    ref = (a.double() @ w.double().T + bias.double() + res.double()) * 0.5
    assert rel_l2(old[:, :N].float(), ref) < 2 * TOL[dt]


@pytest.mark.parametrize("dt", [1, 2])
def test_geglu(lib, dt):
    """ff.net.0: rows of W interleaved (value_j, gate_j); out[:, j] = value * gelu_erf(gate), N / 2 columns"""
    M, N, K = 256, 1024, 512
    ldc = N // 2 + PAD
    a, w, bias, _ = operands(dt, M, N, K, 11)
    da, dw, db = a.cuda(), w.cuda(), bias.cuda()
    sentinel = torch.full((M, ldc), 3.0, dtype=TDT[dt])

    def launch():
        out = sentinel.cuda()
        check(lib, lib.t2p_op_gemm_geglu(dt, P(da), P(dw), P(out), M, N, K, ldc, P(db), None))
        return out

    old, new = both(lib, launch, True)
    assert torch.equal(old, new)
    assert torch.equal(new[:, N // 2:], sentinel[:, N // 2:])
    u = a.double() @ w.double().T + bias.double()
    ref = u[:, 0::2] * torch.nn.functional.gelu(u[:, 1::2])
    assert rel_l2(old[:, :N // 2].float(), ref) < 2 * TOL[dt]


@pytest.mark.parametrize("dt", [1, 2])
@pytest.mark.parametrize("M,N,K,c_f32", [(256, 128, 256, 0),      # K != 512
                                         (200, 128, 512, 0),      # M % 128 != 0
                                         (256, 128, 512, 1)])     # fp32 output
def test_ineligible_launches_keep_their_plan(lib, dt, M, N, K, c_f32):
    a, w, bias, _ = operands(dt, M, N, K, M + K + c_f32)
    da, dw, db = a.cuda(), w.cuda(), bias.cuda()

    def launch():
        out = torch.full((M, N), float("nan"), device="cuda", dtype=torch.float32 if c_f32 else TDT[dt])
        check(lib, lib.t2p_op_gemm(dt, P(da), 0, P(dw), P(out), c_f32, M, N, K, K, K, N, P(db), None, 1.0, None))
        return out

    old, new = both(lib, launch, False)
    assert torch.equal(old, new)
    assert rel_l2(old.float(), a.double() @ w.double().T + bias.double()) < (3e-6 if c_f32 else 2 * TOL[dt])


def test_planner_takes_it_from_128_workgroups(lib):
    """the default (switch at 1): the new kernel from M / 128 >= 128 workgroups on where the planner's tile is 256 x 256 (here it
    is: 64 x 4 tiles), the LDS-DMA kernel below -- same bits"""
    dt, N, K = 2, 1024, 512
    for M, expect in ((128 * 128, 1), (128 * 127, 0)):
        a, w, _, _ = operands(dt, M, N, K, M)
        da, dw = a.cuda(), w.cuda()
        outs = []
        try:
            for key in (0, 1):
                check(lib, lib.t2p_debug_set(49, key))
                n0 = lib.t2p_debug_rowres_launches()
                out = torch.full((M, N), float("nan"), device="cuda", dtype=TDT[dt])
                check(lib, lib.t2p_op_gemm(dt, P(da), 0, P(dw), P(out), 0, M, N, K, K, K, N, None, None, 1.0, None))
                torch.cuda.synchronize()
                assert lib.t2p_debug_rowres_launches() - n0 == (expect if key else 0)
                outs.append(out.cpu())
        finally:
            lib.t2p_debug_set(49, 1)
        assert torch.equal(outs[0], outs[1])
