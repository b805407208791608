"""The launch-profiling records (t2p_profile_begin / _end / _shapes / _attention) of every launch kind the operators reach.

One launch of each kind between begin and end, at the smallest shape the tests of that operator use: the register-staged fp32
product, an LDS-DMA f16 product, the row-resident K = 512 product (plan switch 49 at 2), a dx-shared-stage convolution, a fused
attention launch, and the thin-output head convolution inside one f16 score evaluation of cfg_smallC.  Each must leave ONE record
with its kind, M, N, K, taps and batch, the flops of the launch site's formula and a positive time.
"""
import ctypes as C

import pytest
import torch

from helpers import cfg_smallC

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def lib():
    from text2protein_amd import _lib
    return _lib.load()


def P(t):
    return None if t is None else C.c_void_p(t.data_ptr())


def check(lib, rc):
    assert rc == 0, lib.t2p_last_error().decode()


def profiled(lib, fn):
    """fn() between t2p_profile_begin / _end -> (out[kind] = (ms, flops, launches), {(kind, M, N, K, taps, batch): (launches, ms, flops)},
    (ms, flops, launches) of the fused-attention launches)"""
    check(lib, lib.t2p_profile_begin())
    try:
        fn()
        torch.cuda.synchronize()
    finally:
        o9 = (C.c_double * 9)()
        check(lib, lib.t2p_profile_end(o9))
    buf = C.create_string_buffer(1 << 16)
    check(lib, lib.t2p_profile_shapes(buf, len(buf)))
    lines = buf.value.decode().splitlines()
    assert lines[0] == "kind,M,N,K,taps,batch,launches,ms,flops"
    shapes = {}
    for line in lines[1:]:
        f = line.split(",")
        shapes[(int(f[0]), int(f[1]), int(f[2]), f[3], int(f[4]), int(f[5]))] = (int(f[6]), float(f[7]), float(f[8]))
    att = (C.c_double * 3)()
    check(lib, lib.t2p_profile_attention(att))
    return [tuple(o9[3 * k:3 * k + 3]) for k in range(3)], shapes, tuple(att)


def one_record(kinds, shapes, key, flops):
    """the region holds exactly one GEMM record: `key`, with the site's flops and a positive time"""
    assert list(shapes) == [key], shapes
    launches, ms, fl = shapes[key]
    assert launches == 1 and ms > 0
    assert fl == float(f"{flops:.6g}")                      # (the line prints six significant digits)
    for k in range(3):
        assert kinds[k][2] == (1 if k == key[0] else 0)
    assert kinds[key[0]][1] == flops and kinds[key[0]][0] > 0


def operands(M, N, K, td, seed):
    g = torch.Generator().manual_seed(seed)
    return torch.randn(M, K, generator=g).to(td).cuda(), (torch.randn(N, K, generator=g) / K ** 0.5).to(td).cuda()


def test_register_staged_fp32_product(lib):
    M, N, K = 7, 130, 8                                     # test_gpu_ops.test_gemm
    a, w = operands(M, N, K, torch.float32, 1)
    out = torch.empty(M, N, device="cuda")
    kinds, shapes, att = profiled(lib, lambda: check(lib, lib.t2p_op_gemm(0, P(a), 1, P(w), P(out), 1, M, N, K, K, K, N, None, None, 1.0, None)))
    one_record(kinds, shapes, (1, M, N, str(K), 1, 1), 2.0 * M * N * K)
    assert att[2] == 0


def test_lds_dma_f16_product(lib):
    M, N, K = 256, 128, 64                                  # test_gpu_ops.test_gemm, operands in the compute dtype
    a, w = operands(M, N, K, torch.float16, 2)
    out = torch.empty(M, N, device="cuda", dtype=torch.float16)
    kinds, shapes, att = profiled(lib, lambda: check(lib, lib.t2p_op_gemm(2, P(a), 0, P(w), P(out), 0, M, N, K, K, K, N, None, None, 1.0, None)))
    one_record(kinds, shapes, (1, M, N, str(K), 1, 1), 2.0 * M * N * K)
    assert att[2] == 0


def test_row_resident_product(lib):
    M, N, K = 128, 64, 512                                  # test_gpu_rowgemm.test_plain
    a, w = operands(M, N, K, torch.float16, 3)
    out = torch.empty(M, N, device="cuda", dtype=torch.float16)
    try:
        check(lib, lib.t2p_debug_set(49, 2))
        n0 = lib.t2p_debug_rowres_launches()
        kinds, shapes, att = profiled(lib, lambda: check(lib, lib.t2p_op_gemm(2, P(a), 0, P(w), P(out), 0, M, N, K, K, K, N, None, None, 1.0, None)))
        assert lib.t2p_debug_rowres_launches() - n0 == 1
    finally:
        lib.t2p_debug_set(49, 1)
    one_record(kinds, shapes, (1, M, N, str(K), 1, 1), 2.0 * M * N * K)
    assert att[2] == 0


def test_dx_shared_stage_convolution(lib):
    B, H, W, Cin, Cout = 8, 128, 128, 64, 128               # test_gpu_ops.test_dx_shared_stage_convolution_is_bit_identical
    g = torch.Generator().manual_seed(4)
    x = torch.randn(B, H, W, Cin, generator=g).to(torch.float16).cuda()
    w = (torch.randn(Cout, 9 * Cin, generator=g) / (9 * Cin) ** 0.5).to(torch.float16).cuda()
    bias = torch.randn(Cout, generator=g).cuda()
    out = torch.empty(B, H, W, Cout, device="cuda", dtype=torch.float16)
    kinds, shapes, att = profiled(lib, lambda: check(lib, lib.t2p_op_conv3x3_shortcut(
        2, P(x), P(w), P(bias), None, 0, None, 0, C.c_float(0.5), P(out), 0, B, H, W, Cin, Cout, None)))
    M = B * H * W
    one_record(kinds, shapes, (0, M, Cout, str(Cin), 9, 1), 2.0 * M * Cout * 9.0 * Cin)
    dom, name = (C.c_double * 4)(), C.create_string_buffer(256)
    check(lib, lib.t2p_profile_dominant(dom, name, 256))
    assert name.value.decode().startswith("gemm_dxs_kernel<f16_t, ") and dom[2] == 1
    assert att[2] == 0


def test_fused_attention_launch(lib):
    B, heads, nq, nk, d = 2, 2, 4, 3, 32                    # test_gpu_ops.test_attention
    g = torch.Generator().manual_seed(5)
    C_, nkp = heads * d, 8
    q = torch.randn(B, nq, C_, generator=g).to(torch.float16).cuda()
    k = torch.randn(B, nk, C_, generator=g).to(torch.float16).cuda()
    vt = torch.zeros(B, C_, nkp)
    vt[:, :, :nk] = torch.randn(B, C_, nk, generator=g)
    vt = vt.to(torch.float16).cuda()
    ws = torch.empty(lib.t2p_op_attention_ws(2, B, heads, nq, nk), dtype=torch.uint8, device="cuda")
    out = torch.empty(B, nq, C_, device="cuda", dtype=torch.float16)
    kinds, shapes, att = profiled(lib, lambda: check(lib, lib.t2p_op_attention(
        2, P(q), C_, P(k), C_, P(vt), nkp, P(out), B, heads, nq, nk, d, d ** -0.5, P(ws), None)))
    assert shapes == {} and all(k[2] == 0 for k in kinds)    # the fused kernel: no GEMM launch
    assert att[2] == 1 and att[1] == 4.0 * nq * nk * d * heads * B and att[0] > 0


def test_thin_output_head_in_a_score_evaluation(lib):
    from text2protein_amd import synth
    from text2protein_amd.model import HipScoreModel
    cfg = cfg_smallC()
    m = HipScoreModel(cfg, dtype="f16")
    m.load_state_dict(synth.synth_state_dict(cfg, 5))
    B, L, nc, nf = 3, cfg.data.max_res_num, cfg.data.num_channels, cfg.model.nf
    x = (torch.from_numpy(synth.normal(8, "x", B * nc * L * L).reshape(B, nc, L, L)) * 10.0).cuda()
    ctx = synth.synth_context(B, 7, cfg.model.context_dim, 2).cuda()
    labels = torch.tensor([0, 4, 9]).cuda()
    kinds, shapes, att = profiled(lib, lambda: m(x, labels, ctx))
    M = B * L * L
    launches, ms, fl = shapes[(2, M, nc, str(nf), 9, 1)]
    assert launches == 1 and ms > 0 and fl == float(f"{2.0 * M * nc * 9.0 * nf:.6g}")
    assert sum(v[0] for v in shapes.values()) == sum(k[2] for k in kinds)


def test_empty_region_reports_nothing(lib):
    a, w = operands(7, 130, 8, torch.float32, 1)
    out = torch.empty(7, 130, device="cuda")
    profiled(lib, lambda: check(lib, lib.t2p_op_gemm(0, P(a), 1, P(w), P(out), 1, 7, 130, 8, 8, 8, 130, None, None, 1.0, None)))
    kinds, shapes, att = profiled(lib, lambda: None)
    assert shapes == {} and all(k == (0.0, 0.0, 0.0) for k in kinds) and att == (0.0, 0.0, 0.0)
