"""Host side of the random inpainting mask of training (reference utils.py:15-60, ``random_mask_batch``):
text2protein_amd.conditions.random_mask_batch against the masks the reference's own function drew when the fixture was made
(tests/golden/make_golden_train_inpaint.py), the two new C-ABI symbols, and the properties of the numpy restatement of the DEVICE draw
(tests/inpaint_cases.py) that the GPU tests compare the kernel with.  No GPU."""
import inspect
import os
import random
import re

import numpy as np
import pytest
import torch

from helpers import load_golden
from inpaint_cases import (INPAINTING, LENGTHS, MODE_CONTIGUOUS, MODE_NONE, MODE_RANDOM, SEEDS, cfg_inpaint, device_draw, device_mode,
                           len_lo_hi)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
N = 16


def _batch(form="lengths", lengths=LENGTHS):
    b = {"coords_6d": torch.zeros(len(lengths), 8, N, N)}
    if form == "lengths":
        b["lengths"] = torch.tensor(lengths)
    else:
        b["aa_str"] = ["A" * l + "_" * (N - l) for l in lengths]
    return b


def test_fixture_holds_what_the_issue_describes():
    g = load_golden("inpaint_masks")
    assert g["masks"].shape == (len(SEEDS), 3, N, N) and g["masks"].dtype == np.bool_
    assert list(g["seeds"]) == SEEDS and list(g["lengths"]) == LENGTHS
    assert set(g["modes"].tolist()) == {MODE_NONE, MODE_RANDOM, MODE_CONTIGUOUS}
    empty = [(int(s), b) for s, m, mode in zip(g["seeds"], g["masks"], g["modes"]) if mode != MODE_NONE for b in range(3) if not m[b].any()]
    assert empty, "one sample without a masked residue (num_elem = 0)"


@pytest.mark.parametrize("form", ["lengths", "aa_str"])
@pytest.mark.parametrize("seed", SEEDS)
def test_host_draw_reproduces_the_reference(seed, form):
    """After the same random.seed / torch.manual_seed the mask is the reference's bit for bit, from ``lengths`` and from ``aa_str``
    alike, and exactly one random.random() was consumed."""
    from text2protein_amd import conditions
    g = load_golden("inpaint_masks")
    if str(g["torch_version"]).split("+")[0] != torch.__version__.split("+")[0]:
        print(f"fixture drawn by torch {g['torch_version']}, running {torch.__version__}")
    cfg = cfg_inpaint()
    random.seed(seed)
    random.random()
    second = random.random()
    random.seed(seed)
    torch.manual_seed(seed)
    batch = _batch(form)
    out = conditions.random_mask_batch(batch, cfg)
    assert out is batch and out["mask_inpaint"].dtype == torch.bool and tuple(out["mask_inpaint"].shape) == (3, N, N)
    assert np.array_equal(out["mask_inpaint"].numpy(), g["masks"][seed]), (seed, int(g["modes"][seed]))
    assert random.random() == second


def test_no_draw_without_the_condition():
    from text2protein_amd import conditions
    cfg = cfg_inpaint()
    cfg.model.condition = ["length"]
    random.seed(3)
    first = random.random()
    random.seed(3)
    state = torch.get_rng_state()
    out = conditions.random_mask_batch(_batch(), cfg)
    assert out["mask_inpaint"] is None
    assert random.random() == first and torch.equal(torch.get_rng_state(), state)


def test_empty_count_range_is_refused_before_any_draw():
    """l = 1: int(0.05) = int(0.95) = 0, torch.randint(0, 0) raises in the reference; here a T2PError, and no random number is consumed."""
    from text2protein_amd import conditions
    from text2protein_amd._lib import T2PError
    cfg = cfg_inpaint()
    random.seed(4)
    first = random.random()
    random.seed(4)
    state = torch.get_rng_state()
    for form in ("lengths", "aa_str"):
        with pytest.raises(T2PError, match="range"):
            conditions.random_mask_batch(_batch(form, [16, 1, 6]), cfg)
    with pytest.raises(T2PError, match="residue counts"):
        conditions.random_mask_batch({"coords_6d": torch.zeros(3, 8, N, N)}, cfg)
    with pytest.raises(T2PError, match="outside"):
        conditions.random_mask_batch(_batch("lengths", [16, 17, 6]), cfg)
    assert random.random() == first and torch.equal(torch.get_rng_state(), state)


def test_get_condition_from_batch_draws_without_mask_info():
    from text2protein_amd import conditions
    g = load_golden("inpaint_masks")
    cfg = cfg_inpaint()
    coords = torch.rand(3, 8, N, N)
    batch = dict(_batch(), coords_6d=coords)
    random.seed(1)
    torch.manual_seed(1)
    c = conditions.get_condition_from_batch(cfg, batch)
    assert list(c) == ["length", "ss", "inpainting"]
    assert np.array_equal(c["inpainting"]["mask_inpaint"].numpy(), g["masks"][1]) and c["inpainting"]["coords_6d"] is coords
    assert "mask_inpaint" not in batch                             # the caller's batch is not written to
    # with mask_info: as before, nothing drawn
    random.seed(1)
    first = random.random()
    random.seed(1)
    c2 = conditions.get_condition_from_batch(cfg, batch, mask_info="1:3,6:8")
    assert torch.equal(c2["inpainting"]["mask_inpaint"], conditions.pair_mask(conditions.parse_mask_info("1:3,6:8", 3, N)))
    assert random.random() == first


def test_header_declares_and_lib_binds_the_new_symbols():
    from text2protein_amd import _lib
    hdr = open(os.path.join(ROOT, "include", "t2p.h")).read()
    code = re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)
    for sym, nargs in (("t2p_train_set_inpaint_draw", 5), ("t2p_op_inpaint_mask_draw", 12)):
        m = re.search(r"\bint\s+" + sym + r"\s*\(([^)]*)\)\s*;", code)
        assert m, sym
        assert len(m.group(1).split(",")) == nargs
        assert sym in _lib.SIGNATURES and len(_lib.SIGNATURES[sym][1]) == nargs
        assert hasattr(_lib.load(), sym)
    assert "utils.py:15-60" in hdr and "train.py:176" in hdr


def test_step_functions_take_the_inpaint_mask_draw_argument():
    from text2protein_amd import losses, sde_lib
    sde = sde_lib.VESDE(sigma_min=0.01, sigma_max=100.0, N=10)
    for fn in (losses.get_sde_loss_fn, losses.get_step_fn):
        assert inspect.signature(fn).parameters["inpaint_mask_draw"].default is None
        for ok in (None, "host", "device"):
            fn(sde, train=True, inpaint_mask_draw=ok)
        with pytest.raises(ValueError, match="inpaint_mask_draw"):
            fn(sde, train=True, inpaint_mask_draw="gpu")
    assert callable(losses.HipTrainModel.set_inpaint_draw)


# ---- the numpy restatement of the device draw ---------------------------------------------------------------------------------------------
N_DRAWS = 4096


def _many(force_mode):
    """4096 draws at l = L = 16 under the shipped bounds (lo = 0, hi = 15): one stream id each, sample 0."""
    llh = len_lo_hi([16])
    out = [device_draw(llh, 16, INPAINTING["random_mask_prob"], INPAINTING["contiguous_mask_prob"], 11, 4096 * k + 3, force_mode)
           for k in range(N_DRAWS)]
    flags = np.stack([o[0][0] for o in out])
    return llh[0], flags, np.array([o[3][0] for o in out]), np.array([o[4][0] for o in out]), out


def test_restatement_random_mode_properties():
    """Exactly r residues set with lo <= r < hi; every r of the range occurs; the per-residue inclusion frequency lies within 5 standard
    errors of E[r] / l.  (r is uniform on [lo, hi) up to 2^-24, so E[r] = (lo + hi - 1) / 2; given r a residue is included with
    probability r / l; the variance of the indicator is p (1 - p) with p = E[r] / l.)"""
    (l, lo, hi), flags, r, _, out = _many(MODE_RANDOM)
    assert np.array_equal(flags.sum(1), r) and r.min() >= lo and r.max() < hi
    assert set(r.tolist()) == set(range(lo, hi))
    p = (lo + hi - 1) / 2 / l
    se = np.sqrt(p * (1 - p) / N_DRAWS)
    freq = flags.mean(0)
    print(f"random mode: E[r] / l = {p:.4f}, inclusion frequencies {freq.min():.4f} .. {freq.max():.4f}, 5 se = {5 * se:.4f}")
    assert np.all(np.abs(freq - p) <= 5 * se)
    for o in out[:64]:
        assert np.array_equal(o[1], o[0][:, :, None] | o[0][:, None, :]) and o[2] == MODE_RANDOM


def test_restatement_contiguous_mode_properties():
    """A window of r residues, lo <= r < hi, inside [0, l), with start in [0, l - r) as torch.randint(0, l - r) gives it (so the window
    never holds the last residue, as in the reference); for r = 1 both ends of that range occur."""
    (l, lo, hi), flags, r, start, _ = _many(MODE_CONTIGUOUS)
    assert r.min() >= lo and r.max() < hi and start.min() >= 0 and np.all(start < l - r)
    for k in range(N_DRAWS):
        want = np.zeros(16, np.uint8)
        want[start[k]:start[k] + r[k]] = 1
        assert np.array_equal(flags[k], want)
    assert start[r == 1].max() == l - 2 and start[r == 1].min() == 0


def test_restatement_mode_frequencies_and_none():
    """The drawn mode over 4096 stream ids: each within 5 standard errors of 0.33 / 0.33 / 0.34; mode none flags every residue, the padding
    included; r = 0 (lo = 0) flags nothing; a short sample never has a padding residue flagged."""
    pr, pc = INPAINTING["random_mask_prob"], INPAINTING["contiguous_mask_prob"]
    modes = np.array([device_mode(11, 4096 * k + 3, pr, pc) for k in range(N_DRAWS)])
    for m, p in ((MODE_RANDOM, pr), (MODE_CONTIGUOUS, pc), (MODE_NONE, 1 - pr - pc)):
        assert abs((modes == m).mean() - p) <= 5 * np.sqrt(p * (1 - p) / N_DRAWS), m
    llh = len_lo_hi(LENGTHS)
    f, pair, mode, _, _ = device_draw(llh, N, pr, pc, 5, 3, MODE_NONE)
    assert mode == MODE_NONE and f.all() and pair.all()
    zero = 0
    for k in range(256):
        for fm in (MODE_RANDOM, MODE_CONTIGUOUS):
            f, pair, _, r, _ = device_draw(llh, N, pr, pc, 5, 4096 * k + 3, fm)
            assert np.array_equal(f.sum(1), r)
            assert not f[1, 11:].any() and not f[2, 6:].any()
            zero += int((r == 0).sum())
    assert zero > 0
