"""numpy restatement of the weight packings (``t2p_op_weight_pack``, include/t2p.h), written from their formulas, and the cases
the CPU and GPU tests share.

Each ``pack_*`` returns the float32 block a packing writes; ``to_dtype`` rounds it to the stored type (nearest even).  The two
products are formed the way the engine's host load path forms them: one float32 accumulator from 0, terms in ascending k, every
product and every add rounded to float32 (``np.float32`` arithmetic, no fused multiply-add); the double-accumulated bias likewise in
``np.float64``.
"""
import numpy as np
import torch

COPY, ROWS, CONV3, CONV3_T, NIN, GEGLU, UP4, ADD, PRODUCT, DOT64 = range(10)
DTYPES = {"f32": 0, "bf16": 1, "f16": 2}


def values(seed, *shape):
    """Deterministic float32 values with full mantissas in about (-1, 1), some exactly representable, some tiny."""
    rng = np.random.RandomState(seed)
    v = rng.standard_normal(int(np.prod(shape))).astype(np.float32) * np.float32(0.37)
    v[::7] = np.float32(0.5)
    v[3::11] = np.float32(1e-6)
    return v.reshape(shape)


def to_dtype(block, dtype):
    """float32 block -> the bit pattern stored for ``dtype`` (uint32 for f32, uint16 for the 16-bit types)."""
    t = torch.from_numpy(np.ascontiguousarray(block, dtype=np.float32))
    if dtype == "f32":
        return t.numpy().view(np.uint32)
    return t.to(torch.float16 if dtype == "f16" else torch.bfloat16).view(torch.int16).numpy().view(np.uint16)


def pack_copy(*srcs):
    return np.concatenate([s.reshape(-1) for s in srcs])


def pack_rows(src, ld, fill):
    """(rows, rowlen) at pitch ld; ``fill`` stands where the packing writes nothing."""
    rows, rl = src.shape
    out = np.full((rows, ld), fill, np.float32)
    out[:, :rl] = src
    return out


def pack_conv3(w, cin_pad=0, ld=0, fill=0.0):
    """(N, Ci, 3, 3) -> [N][tap = kh * 3 + kw][cin_pad], channels past Ci zero; rows at pitch ld."""
    N, ci = w.shape[:2]
    cp = cin_pad or ci
    ld = ld or 9 * cp
    out = np.full((N, ld), fill, np.float32)
    blk = np.zeros((N, 9, cp), np.float32)
    for n in range(N):
        for c in range(ci):
            for tap in range(9):
                blk[n, tap, c] = w[n, c, tap // 3, tap % 3]
    out[:, :9 * cp] = blk.reshape(N, 9 * cp)
    return out


def pack_conv3_t(w):
    """(N, C, 3, 3) -> [tap][C][N]."""
    N, C = w.shape[:2]
    out = np.zeros((9, C, N), np.float32)
    for n in range(N):
        for c in range(C):
            for tap in range(9):
                out[tap, c, n] = w[n, c, tap // 3, tap % 3]
    return out


def pack_nin(*ws):
    """one or two (K, N) -> [nsrc * N][K]."""
    return np.concatenate([np.array([[w[k, n] for k in range(w.shape[0])] for n in range(w.shape[1])], np.float32) for w in ws])


def pack_geglu(w):
    """(2 inner, rowlen): row 2 j = source row j (value), row 2 j + 1 = source row inner + j (gate)."""
    inner = w.shape[0] // 2
    out = np.empty_like(w)
    for j in range(inner):
        out[2 * j] = w[j]
        out[2 * j + 1] = w[inner + j]
    return out


def pack_up4(w):
    """conv0 of an up block on the 2x nearest-up-sampled map as four 2 x 2 phase convolutions on the source map: output phase
    (py, px) and kernel row kh read source row offset floor((py + kh - 1) / 2); the taps that meet in one source pixel are
    summed in float32 in (kh, kw) order from 0.  -> [phase][co][ty * 2 + tx][ci]."""
    co, ci = w.shape[:2]
    out = np.zeros((4, co, 4, ci), np.float32)
    for py in range(2):
        for px in range(2):
            for kh in range(3):
                for kw in range(3):
                    ty = (py + kh - 1) // 2 + 1 - py         # Python's // is the floor
                    tx = (px + kw - 1) // 2 + 1 - px
                    out[py * 2 + px, :, ty * 2 + tx, :] = out[py * 2 + px, :, ty * 2 + tx, :] + w[:, :, kh, kw]
    return out


def pack_add(a, b):
    return (a + b).astype(np.float32)


def pack_product(A, B, addv=None, transposed=False, ld=0, fill=0.0):
    """sum_k A[m][k] B[k][n] (+ addv[n]) in float32: multiply, round, add, round, ascending k."""
    M, K = A.shape
    N = B.shape[1]
    acc = np.zeros((M, N), np.float32)
    for k in range(K):
        acc = acc + (A[:, k:k + 1] * B[k:k + 1, :]).astype(np.float32)     # float32 * float32 and float32 + float32: each rounded once
    if addv is not None:
        acc = acc + addv[None, :]
    blk = acc.T if transposed else acc
    out = np.full((blk.shape[0], ld or blk.shape[1]), fill, np.float32)
    out[:, :blk.shape[1]] = blk
    return out


def pack_dot64(W, v, b0):
    """(float32)(b0[n] + sum_j float64(W[n][j]) * float64(v[j])), ascending j."""
    acc = b0.astype(np.float64)
    W64, v64 = W.astype(np.float64), v.astype(np.float64)
    for j in range(W.shape[1]):
        acc = acc + W64[:, j] * v64[j]
    return acc.astype(np.float32)


FILL = np.float32(-77.0)       # what the tests put into a destination before a packing with a pitch: gaps keep it


def cases():
    """name -> (kind, sources, dims, expected float32 block with FILL in the gaps of pitched rows).  Sizes: no multiple of a tile
    (256 channels, 64 x 64, 32 x 32) or of the vector width; one below a tile, one across a tile boundary where the kernel has one."""
    c = {}
    a, b, d = values(1, 1000), values(2, 24), values(3, 7)
    c["copy_one_vec4"] = (COPY, [a], [1000], pack_copy(a))
    c["copy_one_odd"] = (COPY, [a[:999]], [999], pack_copy(a[:999]))
    c["copy_three"] = (COPY, [a[:333], b, d], [333, 24, 7], pack_copy(a[:333], b, d))
    r = values(4, 24, 40)
    c["rows_pitched"] = (ROWS, [r], [24, 40, 51], pack_rows(r, 51, FILL))
    w = values(5, 24, 5, 3, 3)
    c["conv3_ci5_pad8"] = (CONV3, [w], [24, 5, 8, 0], pack_conv3(w, 8))
    w = values(6, 24, 40, 3, 3)
    c["conv3_ci40"] = (CONV3, [w], [24, 40, 0, 0], pack_conv3(w))
    c["conv3_ci40_pitched"] = (CONV3, [w], [24, 40, 40, 9 * 40 + 13], pack_conv3(w, 40, 9 * 40 + 13, FILL))
    w = values(7, 3, 264, 3, 3)
    c["conv3_ci264_two_tiles"] = (CONV3, [w], [3, 264, 0, 0], pack_conv3(w))
    w = values(8, 40, 5, 3, 3)
    c["conv3_t_n40_c5"] = (CONV3_T, [w], [40, 5], pack_conv3_t(w))
    w = values(9, 24, 8, 3, 3)
    c["conv3_t_n24_c8"] = (CONV3_T, [w], [24, 8], pack_conv3_t(w))
    w0, w1 = values(10, 24, 40), values(11, 24, 40)
    c["nin_24x40"] = (NIN, [w0], [24, 40, 1], pack_nin(w0))
    c["nin_24x40_stacked"] = (NIN, [w0, w1], [24, 40, 2], pack_nin(w0, w1))
    w0 = values(12, 72, 70)
    c["nin_72x70_two_tiles"] = (NIN, [w0], [72, 70, 1], pack_nin(w0))
    w = values(13, 8 * 24, 24)
    c["geglu_ci24"] = (GEGLU, [w], [4 * 24, 24], pack_geglu(w))
    c["geglu_bias_ci24"] = (GEGLU, [w[:, 0].copy()], [4 * 24, 1], pack_geglu(w[:, :1].copy()))
    w = values(14, 24, 40, 3, 3)
    c["up4_co24_ci40"] = (UP4, [w], [24, 40], pack_up4(w))
    w = values(15, 2, 260, 3, 3)
    c["up4_ci260_two_tiles"] = (UP4, [w], [2, 260], pack_up4(w))
    c["add_24"] = (ADD, [b, values(16, 24)], [24], pack_add(b, values(16, 24)))
    A, B = values(17, 24, 40), values(18, 40, 72)
    c["product_24x40x72"] = (PRODUCT, [A, B], [24, 40, 72, 0, 0], pack_product(A, B))
    c["product_24x40x72_transposed"] = (PRODUCT, [A, B], [24, 40, 72, 1, 0], pack_product(A, B, transposed=True))
    c["product_24x40x72_pitched"] = (PRODUCT, [A, B], [24, 40, 72, 0, 72 + 24], pack_product(A, B, ld=96, fill=FILL))
    A1, B1 = values(19, 24, 1), values(20, 1, 72)
    c["product_k1"] = (PRODUCT, [A1, B1], [24, 1, 72, 0, 0], pack_product(A1, B1))
    bv, addv = values(21, 1, 40), values(22, 72)
    c["product_bias_row"] = (PRODUCT, [bv, B, addv], [1, 40, 72, 0, 0], pack_product(bv, B, addv))
    W, v, b0 = values(23, 24, 40), values(24, 40), values(25, 24)
    c["dot64_24x40"] = (DOT64, [W, v, b0], [24, 40], pack_dot64(W, v, b0))
    return c
