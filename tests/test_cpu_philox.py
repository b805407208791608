"""The numpy restatement of the device generator (oracle/philox.py) against the Random123 known-answer vectors for philox4x32-10."""
import numpy as np

from oracle import philox

KAT = [  # counter, key, words
    ("00000000 00000000 00000000 00000000", "00000000 00000000", "6627e8d5 e169c58d bc57ac4c 9b00dbd8"),
    ("ffffffff ffffffff ffffffff ffffffff", "ffffffff ffffffff", "408f276d 41c83b0e a20bc7c6 6d5451fd"),
    ("243f6a88 85a308d3 13198a2e 03707344", "a4093822 299f31d0", "d16cfe09 94fdcceb 5001e420 24126ea1"),
]


def _words(text):
    return np.array([int(w, 16) for w in text.split()], dtype=np.uint64)


def test_known_answer_vectors():
    for counter, key, want in KAT:
        assert np.array_equal(philox.philox4x32_10(_words(counter), _words(key)), _words(want)), counter
    # and as one batch under per-row keys
    got = philox.philox4x32_10(np.stack([_words(c) for c, _, _ in KAT]), np.stack([_words(k) for _, k, _ in KAT]))
    assert np.array_equal(got, np.stack([_words(w) for _, _, w in KAT]))


def test_uniform24_and_the_layouts():
    """uniform24 keeps the top 24 bits; the sampling layout truncates the stream to 32 bits and carries the step word, the training
    layout carries all 64 bits of the stream; both key with (seed lo, seed hi)."""
    assert philox.uniform24(0xFFFFFFFF) == np.float32(1.0) - np.float32(2.0 ** -24) and philox.uniform24(0xFF) == 0
    seed, stream = 0x0123456789ABCDEF, 0x500000003
    key = np.array([0x89ABCDEF, 0x01234567], dtype=np.uint64)
    w = philox.philox4x32_10(np.array([[1, 0, 3, 5]], dtype=np.uint64), key)
    assert np.array_equal(philox.train_uniforms(seed, stream, [1]), philox.uniform24(w))
    z = philox.normals(seed, stream, 7, 6)
    assert z.shape == (6,) and z.dtype == np.float64
    assert np.array_equal(z, philox.normals(seed, 3, 7, 8)[:6]) and not np.array_equal(z, philox.normals(seed, 3, 0, 6))
    w = philox.philox4x32_10(np.array([0, 0, 3, 7], dtype=np.uint64), key) >> np.uint64(8)
    u1, u2 = (float(w[0]) + 0.5) / 2 ** 24, float(w[1]) / 2 ** 24
    want = np.sqrt(-2 * np.log(u1)) * np.cos(float(np.float32(6.283185307179586) * np.float32(u2)))
    assert abs(z[0] - want) <= 1e-6
