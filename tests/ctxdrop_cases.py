"""Text-context dropout (training for classifier-free guidance): what tests/golden/make_golden_train_ctxdrop.py,
tests/test_cpu_train_ctxdrop.py and tests/test_gpu_train_ctxdrop.py share.

The case is train_tinyB's -- configuration, seed and inputs (B = 3, T = 5, context_dim = 24, L = 16, VE) -- with the text context of the
dropped samples replaced by zeros.  ``py_seed`` = 3 is chosen so that three ``random.random() < 0.5`` give [1, 0, 1]: a dropped sample on
either side of a kept one (the tests assert the decisions, not the seed).

``device_decisions`` restates the device draw (csrc/train_kernels.hip: context_drop_draw) on oracle/philox.py."""
import json

import numpy as np

from helpers import TRAIN_CASES

CONTEXT_DROPOUT = 0.5
PY_SEED = 3
DECISIONS = [1, 0, 1]
CTXDROP_STREAM = 4        # Trainer::rng_ctx() = 4096 loss_calls + 4 (csrc/philox.h)

CTXDROP_CASES = {
    "train_tinyB_ctxdrop": dict(TRAIN_CASES["train_tinyB"], sde="ve", base="train_tinyB", p=CONTEXT_DROPOUT, py_seed=PY_SEED,
                                decisions=DECISIONS),
}

# the three (seed, stream) pairs of the draw tests: call 5 and call 6 of a trainer seeded 11, call 5 of one seeded 12
DRAW_PAIRS = [(11, 4096 * 5 + CTXDROP_STREAM), (11, 4096 * 6 + CTXDROP_STREAM), (12, 4096 * 5 + CTXDROP_STREAM)]


def ctxdrop_record(g):
    """The record of a fixture: p, py_seed, decisions and the generator's two measured conditions."""
    return json.loads(str(g["ctxdrop"]))


def device_decisions(seed, stream, B, p):
    """Sample b is dropped iff philox_uniform24(word 0) < (float)p: training layout, counter b, the given stream, key = seed."""
    from oracle.philox import train_uniforms
    return train_uniforms(seed, stream, np.arange(int(B)))[..., 0] < np.float32(p)


def zeroed_context(context, decisions):
    """A copy of ``context`` (B, T, D) with the rows of the dropped samples zeroed: what a dropped sample trains on."""
    out = context.clone()
    for b, d in enumerate(decisions):
        if d:
            out[b] = 0
    return out
