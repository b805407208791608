"""The random inpainting mask of training (reference utils.py:15-60, ``random_mask_batch``): what the fixture generator
(tests/golden/make_golden_train_inpaint.py) and the tests (test_cpu_train_inpaint.py, test_gpu_train_inpaint.py) share, and a numpy
restatement of the DEVICE draw (t2p_op_inpaint_mask_draw, csrc/train_kernels.hip: inpaint_mask_draw_kernel) built on oracle/philox.py.

Geometry: train_tinyB's (helpers.TRAIN_CASES: B = 3, N = 16, pair masks of 16 / 11 / 6 residues, C = 8, conditions length + ss +
inpainting) with the shipped ``model.inpainting`` of configs/cond_length_inpainting.yml.  The host fixture holds the reference's masks
for ``random.seed(s); torch.manual_seed(s)``, s = 0 .. 11.

The device draw, all in integers (training layout of philox.h, key = seed, stream = stream_id):
  counter 0                      word 0 -> u0 = (w >> 8) 2^-24: random when u0 < float32(random_p), contiguous when
                                 u0 > float32(1.0 - contiguous_p) (the subtraction in double), else none
  counter (b + 1) 2^32           word 0 -> r = lo + (((w >> 8) (hi - lo)) >> 24), word 1 -> start = ((w >> 8) (l - r)) >> 24
  counter (b + 1) 2^32 + 1 + j   word 0 -> the key of residue j < l; j is masked iff fewer than r keys sort before (key_j, j)
"""
import numpy as np

from helpers import TRAIN_CASES, cfg_train_tinyB
from oracle.philox import M32, _key, philox4x32_10, train_uniforms

INPAINTING = dict(random_mask_prob=0.33, contiguous_mask_prob=0.33, mask_min_len=0.05, mask_max_len=0.95)   # the shipped values
SEEDS = list(range(12))
LENGTHS = list(TRAIN_CASES["train_tinyB"]["lengths"])          # 16, 11, 6
MODE_NONE, MODE_RANDOM, MODE_CONTIGUOUS = 0, 1, 2
INPAINT_STREAM = 3                                            # Trainer::rng_inpaint() = 4096 loss_calls + 3

# the two end-to-end fixtures: train_tinyB's inputs with the reference's mask of one random and one contiguous seed (the generator
# asserts the modes)
INPAINT_TRAIN_CASES = {
    "train_tinyB_inpaintdraw_rand": dict(TRAIN_CASES["train_tinyB"], sde="ve", base="train_tinyB", mask_seed=1, mask_mode=MODE_RANDOM),
    "train_tinyB_inpaintdraw_contig": dict(TRAIN_CASES["train_tinyB"], sde="ve", base="train_tinyB", mask_seed=0, mask_mode=MODE_CONTIGUOUS),
}


def cfg_inpaint():
    """train_tinyB's configuration with the shipped ``model.inpainting`` block."""
    cfg = cfg_train_tinyB()
    cfg.model.inpainting = dict(INPAINTING)
    return cfg


def len_lo_hi(lengths, inpainting=INPAINTING):
    """int32 [B][3] = (l, int(mask_min_len l), int(mask_max_len l)): the products in double, truncated, as Python forms them."""
    return np.array([(l, int(inpainting["mask_min_len"] * l), int(inpainting["mask_max_len"] * l)) for l in lengths], dtype=np.int32)


def _words(seed, stream, index):
    """The four 32-bit words of the training layout's counter {i lo, i hi, stream lo, stream hi} for every i of ``index``."""
    i = np.asarray(index, dtype=np.uint64)
    s = int(stream) & 0xFFFFFFFFFFFFFFFF
    c = np.stack([i & M32, i >> np.uint64(32), np.full_like(i, s & 0xFFFFFFFF), np.full_like(i, s >> 32)], axis=-1)
    return philox4x32_10(c, _key(seed))


def device_mode(seed, stream, random_p, contiguous_p):
    u0 = train_uniforms(seed, stream, [0])[0, 0]               # float32, exact
    if u0 < np.float32(random_p):
        return MODE_RANDOM
    if u0 > np.float32(1.0 - contiguous_p):
        return MODE_CONTIGUOUS
    return MODE_NONE


def device_draw(llh, L, random_p, contiguous_p, seed, stream, force_mode=-1):
    """(flags [B][L] uint8, pair [B][L][L] uint8, mode, r [B], start [B]) as the device draws them."""
    llh = np.asarray(llh, dtype=np.int64).reshape(-1, 3)
    B = llh.shape[0]
    mode = device_mode(seed, stream, random_p, contiguous_p) if force_mode < 0 else int(force_mode)
    flags = np.zeros((B, L), np.uint8)
    rs, starts = np.zeros(B, np.int64), np.zeros(B, np.int64)
    for b in range(B):
        l, lo, hi = (int(v) for v in llh[b])
        base = (b + 1) << 32
        w = _words(seed, stream, [base])[0]
        r = lo + ((int(w[0] >> np.uint64(8)) * (hi - lo)) >> 24)
        start = (int(w[1] >> np.uint64(8)) * (l - r)) >> 24
        rs[b], starts[b] = r, start
        if mode == MODE_NONE:
            flags[b, :] = 1
        elif mode == MODE_CONTIGUOUS:
            flags[b, start:start + r] = 1
        elif l > 0:
            keys = _words(seed, stream, base + 1 + np.arange(l, dtype=np.uint64))[:, 0]
            order = np.lexsort((np.arange(l), keys))            # by key, ties to the lower index
            flags[b, order[:r]] = 1
    pair = flags[:, :, None] | flags[:, None, :]
    return flags, pair, mode, rs, starts
