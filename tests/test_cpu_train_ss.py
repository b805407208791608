"""Host side of secondary-structure block dropout (losses.py:54-64 of the reference): the parser of ``batch["ss_indices"]`` and the host
draws of text2protein_amd.losses against the block list, the decisions and the dropped coords_6d the reference's own ``block_dropout``
produced when the fixtures were made (tests/golden/make_golden_train_ss.py), and the two new C-ABI symbols.  No GPU."""
import inspect
import os
import random
import re

import numpy as np
import pytest
import torch

from helpers import load_golden, train_inputs
from ss_train_cases import BLOCK_DROPOUT, SS_TRAIN_CASES, dropped_coords, ss_record

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.parametrize("name", list(SS_TRAIN_CASES))
def test_parser_and_host_draws_reproduce_the_reference(name):
    """parse_ss_indices + draw_block_decisions under the fixture's random.seed give the fixture's block list and decisions exactly (the
    reference's draw order: samples in order, blocks in string order, no draw for ''), and zeroing by them in torch gives the
    reference's dropped coords_6d bit for bit (stored as its SHA-256 and the count of changed elements)."""
    from text2protein_amd import losses
    g = load_golden(name)
    case = SS_TRAIN_CASES[name]
    cfg = case["config"]()
    rec = ss_record(g)
    assert rec["ss_indices"] == case["ss_indices"] and rec["py_seed"] == case["py_seed"] and rec["block_dropout"] == BLOCK_DROPOUT
    blocks = losses.parse_ss_indices(rec["ss_indices"], case["B"])
    assert [list(b) for b in blocks] == rec["blocks"]
    random.seed(case["py_seed"])
    drop = losses.draw_block_decisions(blocks, BLOCK_DROPOUT)
    assert drop == rec["decisions"] and 0 < sum(drop) < len(drop)
    # zeroing by the parser's blocks and the host draws gives the tensor the reference's block_dropout returned: its SHA-256 and the
    # number of changed elements are the fixture's (dropped_coords asserts both)
    x = train_inputs(cfg, case)["coords_6d"]
    want = dropped_coords(x, dict(rec, blocks=[list(b) for b in blocks], decisions=drop))
    assert want.dtype == torch.float32 and not torch.equal(want, x)
    other = dict(rec, decisions=[1 - d for d in drop])           # the check can fail: other decisions give another tensor
    with pytest.raises(AssertionError):
        dropped_coords(x, other)
    base = load_golden(case["base"])
    assert float(g["loss"]) != float(base["loss"])


def test_parser_forms():
    from text2protein_amd.losses import parse_ss_indices
    assert parse_ss_indices(["", ""]) == []
    assert parse_ss_indices(["3:7"]) == [(0, 3, 7)]
    assert parse_ss_indices(["", "0:2,5:5,9:4", "", "1:30"], 4) == [(1, 0, 2), (1, 5, 5), (1, 9, 4), (3, 1, 30)]
    assert parse_ss_indices(("2:3",), 1) == [(0, 2, 3)]


@pytest.mark.parametrize("bad", [["1:2,"], ["1"], ["1:2:3"], ["a:b"], ["1:"], [":4"], ["1.5:4"], ["1:2;3:4"], [","], ["-3:5"], ["2:-1"],
                                 [None], [5], "1:2", 7])
def test_malformed_ss_indices_raise(bad):
    from text2protein_amd._lib import T2PError
    from text2protein_amd.losses import parse_ss_indices
    with pytest.raises(T2PError):
        parse_ss_indices(bad)


def test_ss_indices_length_is_checked_against_the_batch():
    from text2protein_amd._lib import T2PError
    from text2protein_amd.losses import parse_ss_indices
    with pytest.raises(T2PError, match="3 samples"):
        parse_ss_indices(["1:2", ""], 3)


def test_no_draw_without_blocks_and_one_per_block():
    """'' consumes no random number; every block consumes exactly one, dropped or not."""
    from text2protein_amd.losses import draw_block_decisions, parse_ss_indices
    blocks = parse_ss_indices(["", "1:2,3:4", "", "5:6"])
    random.seed(5)
    want = [random.random() for _ in range(4)]
    random.seed(5)
    got = draw_block_decisions(blocks, 0.5)
    assert got == [int(u < 0.5) for u in want[:3]] and random.random() == want[3]
    assert draw_block_decisions(blocks, 0.0) == [0, 0, 0] and draw_block_decisions(blocks, 1.0) == [1, 1, 1]


def test_step_functions_take_the_block_dropout_arguments():
    from text2protein_amd import losses, sde_lib
    sde = sde_lib.VESDE(sigma_min=0.01, sigma_max=100.0, N=10)
    for fn in (losses.get_sde_loss_fn, losses.get_step_fn):
        sig = inspect.signature(fn)
        assert sig.parameters["block_dropout"].default == 0.2 and sig.parameters["block_dropout_draw"].default == "host"
        fn(sde, train=True, block_dropout=0.3, block_dropout_draw="device")
        with pytest.raises(ValueError, match="block_dropout_draw"):
            fn(sde, train=True, block_dropout_draw="gpu")
    assert callable(losses.HipTrainModel.set_ss_blocks)


def test_header_declares_and_lib_binds_the_new_symbols():
    from text2protein_amd import _lib
    hdr = open(os.path.join(ROOT, "include", "t2p.h")).read()
    code = re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)
    for sym, nargs in (("t2p_train_set_ss_blocks", 5), ("t2p_op_ss_block_dropout", 13)):
        m = re.search(r"\bint\s+" + sym + r"\s*\(([^)]*)\)\s*;", code)
        assert m, sym
        assert len(m.group(1).split(",")) == nargs
        assert sym in _lib.SIGNATURES and len(_lib.SIGNATURES[sym][1]) == nargs
        assert hasattr(_lib.load(), sym)
    assert "losses.py:54-64" in hdr and ":106-107" in hdr
