"""Philox4x32-10 as the device draws it (text2protein_amd/csrc/philox.h), restated in numpy: test infrastructure only.

Integer parts are exact (uint64 arrays masked to 32 bits).  The normals follow the device's float32 arithmetic up to the
arguments of the transcendentals -- u1 from a float32 add (which rounds above 2^23), the angle a float32 product -- and
evaluate log, sqrt, sin and cos in float64, so they differ from the device's logf / sqrtf / sincosf by rounding only.
"""
import numpy as np

M32 = np.uint64(0xFFFFFFFF)
_S32 = np.uint64(32)
_MUL0, _MUL1 = np.uint64(0xD2511F53), np.uint64(0xCD9E8D57)
_W0, _W1 = np.uint64(0x9E3779B9), np.uint64(0xBB67AE85)
_2POW_M24 = np.float32(1.0 / 16777216.0)
_TWO_PI = np.float32(6.283185307179586)


def philox4x32_10(counter_words, key_words):
    """Ten rounds on counters [..., 4] under keys [..., 2] (or one key [2]); uint64 arrays holding 32-bit words.  Returns [..., 4]."""
    c = np.asarray(counter_words, dtype=np.uint64) & M32
    k = np.asarray(key_words, dtype=np.uint64) & M32
    c0, c1, c2, c3 = (c[..., i] for i in range(4))
    k0, k1 = k[..., 0], k[..., 1]
    for _ in range(10):
        p0, p1 = _MUL0 * c0, _MUL1 * c2                    # 32 x 32 -> 64 bits: no overflow in uint64
        c0, c1, c2, c3 = (p1 >> _S32) ^ c1 ^ k0, p1 & M32, (p0 >> _S32) ^ c3 ^ k1, p0 & M32
        k0, k1 = (k0 + _W0) & M32, (k1 + _W1) & M32
    return np.stack([c0, c1, c2, c3], axis=-1)


def uniform24(w):
    """(w >> 8) 2^-24 in [0, 1) as float32: exact (24 bits)."""
    return (np.asarray(w, dtype=np.uint64) >> np.uint64(8)).astype(np.float32) * _2POW_M24


def _key(seed):
    seed = int(seed) & 0xFFFFFFFFFFFFFFFF
    return np.array([seed & 0xFFFFFFFF, seed >> 32], dtype=np.uint64)


def normals(seed, stream, step, n):
    """The n standard normals of t2p_op_philox_normal(seed, stream) at step word `step` (sampling layout: counter
    {q lo, q hi, (uint32) stream, step} for quad q), float64."""
    q = np.arange((int(n) + 3) // 4, dtype=np.uint64)
    c = np.stack([q & M32, q >> _S32, np.full_like(q, int(stream) & 0xFFFFFFFF), np.full_like(q, int(step) & 0xFFFFFFFF)], axis=-1)
    w = philox4x32_10(c, _key(seed)) >> np.uint64(8)
    u1 = (w[:, 0::2].astype(np.float32) + np.float32(0.5)) * _2POW_M24          # (0, 1]: the float32 add rounds above 2^23
    angle = (_TWO_PI * (w[:, 1::2].astype(np.float32) * _2POW_M24)).astype(np.float64)
    rad = np.sqrt(-2.0 * np.log(u1.astype(np.float64)))
    z = np.stack([rad * np.cos(angle), rad * np.sin(angle)], axis=-1)            # [nq][pair][cos, sin] = z0 z1 z2 z3
    return z.reshape(-1)[:int(n)]


def train_uniforms(seed, stream, index):
    """The four float32 uniforms of the training layout's counter {i lo, i hi, stream lo, stream hi} for every i of `index`:
    [..., 4].  The diffusion times and the block decisions read word 0; the keep-masks read all four (element 4 i + j)."""
    i = np.asarray(index, dtype=np.uint64)
    s = int(stream) & 0xFFFFFFFFFFFFFFFF
    c = np.stack([i & M32, i >> _S32, np.full_like(i, s & 0xFFFFFFFF), np.full_like(i, s >> 32)], axis=-1)
    return uniform24(philox4x32_10(c, _key(seed)))
