"""Training-step fixtures with secondary-structure block dropout (tests/golden/make_golden_train_ss.py writes them;
tests/test_gpu_train_ss.py and tests/test_cpu_train_ss.py read them).  Configuration, seed and inputs are train_tinyB's (helpers.TRAIN_CASES /
sde_train_cases.SDE_TRAIN_CASES: C = 8, conditions length + ss + inpainting, pair masks of 16, 11 and 6 residues on L = 16); added are the
reference's ``batch["ss_indices"]`` strings and the ``random.seed`` under which its ``block_dropout`` (losses.py:54-64) ran.

The strings: sample 0 has three blocks, the last one reaching past L (Python clamps the slice), sample 1 has no annotation (''), sample 2
has two, the second reaching past its 6 valid residues.  ``py_seed`` = 22 is chosen so that under p = 0.2 blocks 6:10 and 12:20 of sample 0
and 4:9 of sample 2 are dropped and 0:4 / 1:3 are kept: dropped and kept blocks in both annotated samples, every dropped block inside a
valid region (the generator asserts the properties, not the seed)."""
import hashlib
import json

import numpy as np

from helpers import TRAIN_CASES
from sde_train_cases import SDE_TRAIN_CASES

SS_INDICES = ["0:4,6:10,12:20", "", "1:3,4:9"]
BLOCK_DROPOUT = 0.2      # the reference's default (losses.py:54)

SS_TRAIN_CASES = {
    "train_tinyB_ssdrop": dict(TRAIN_CASES["train_tinyB"], sde="ve", base="train_tinyB", ss_indices=SS_INDICES, py_seed=22),
    "train_tinyB_ssdrop_vp": dict(SDE_TRAIN_CASES["train_tinyB_vp"], base="train_tinyB_vp", ss_indices=SS_INDICES, py_seed=22),
}


def ss_record(g):
    """The block-dropout record of a fixture: ss_indices, py_seed, block_dropout, blocks, decisions, changed, sha256."""
    return json.loads(str(g["ss"]))


def dropped_coords(coords_6d, rec):
    """The coords_6d the reference's block_dropout returned: the (regenerated) input with channels 4:7 zeroed on the rows and columns of
    the dropped blocks (losses.py:61-62), checked bit for bit against the fixture -- the SHA-256 of its bytes and the number of elements
    whose bits changed."""
    x = coords_6d.clone()
    for (b, start, end), d in zip(rec["blocks"], rec["decisions"]):
        if d:
            x[b, 4:7, :, start:end] = 0
            x[b, 4:7, start:end, :] = 0
    assert hashlib.sha256(x.numpy().tobytes()).hexdigest() == rec["sha256"], "the rebuilt dropped coords_6d differs from the reference's"
    assert int((x.numpy().view(np.int32) != coords_6d.numpy().view(np.int32)).sum()) == rec["changed"] > 0
    return x
