"""Condition builders of the sampling path: the pure-tensor parts of reference ``utils.py``.

  get_mask_all_lengths     utils.py:139-148   (n_lengths, B, L, L) bool; the driver indexes it with
                                              ``length_index - 1`` (sampling_6d.py:145)
  selected_mask_batch      utils.py:62-81     "1:5,10:15" -> (B, L, L) bool, inclusive 0-based ranges
  random_mask_batch        utils.py:15-60     the random inpainting mask train.py draws before every train and eval step
  get_condition_from_batch utils.py:84-106    {"length" | "ss" | "inpainting"} from a batch of 6D maps
  get_conditions_from_pdb  utils.py:122-137   the same from one chain of a PDB file, featurised on the device
                                              (text2protein_amd/encode.py: dataset.py:114-168, :200-239, :396-450)
The reference's builder goes through biotite and calls ``ProteinDataset`` with a signature it does not have (SURVEY.md section 2,
row 10); here the chain is read by ``encode.read_backbone`` and encoded by ``t2p_op_encode_6d``.  The secondary-structure letters
of the 8-channel layout (biotite's P-SEA in the reference) are an input, or ``sse="psea"`` computes them on the device
(``t2p_op_annotate_sse``).  ``get_conditions_random`` (utils.py:108-120) draws from a
dataset directory and stays out of scope.
"""
from __future__ import annotations

import random

import numpy as np
import torch


def get_mask_all_lengths(config, batch_size=16):
    """(n_lengths, B, L, L) bool: entry k masks the top-left square of ``min_res_num + k`` residues (utils.py:139-148)."""
    L = config.data.max_res_num
    lengths = torch.arange(config.data.min_res_num, L + 1)
    inside = torch.arange(L)[None, :] < lengths[:, None]                      # (n_lengths, L)
    square = inside[:, :, None] & inside[:, None, :]                          # (n_lengths, L, L)
    return square[:, None].expand(-1, batch_size, -1, -1).clone()


def parse_mask_info(mask_info: str, batch: int, n: int) -> torch.Tensor:
    """(B, N) 0/1 residue mask from ``"a:b,c"``: comma separated 0-based entries, ``a:b`` inclusive (utils.py:69-76).
    Indices follow tensor slicing semantics (negative values count from the end), as in the reference."""
    row = torch.zeros(n)
    for item in mask_info.split(","):
        lo, _, hi = item.partition(":")
        if hi:
            row[int(lo):int(hi) + 1] = 1
        else:
            row[int(lo)] = 1
    return row.expand(batch, n).clone()


def pair_mask(residue_mask: torch.Tensor) -> torch.Tensor:
    """(B, N) -> (B, N, N) bool: a pixel (i, j) is selected when residue i OR residue j is (utils.py:78)."""
    m = residue_mask.bool()
    return m[:, :, None] | m[:, None, :]


def selected_mask_batch(batch, mask_info, config):
    """utils.py:62-81 on a ``{"coords_6d": (B,C,N,N)}`` batch; adds ``mask_inpaint`` (B,N,N) bool."""
    if "inpainting" not in config.model.condition:
        batch["mask_inpaint"] = None
        return batch
    B, _, N, _ = batch["coords_6d"].shape
    batch["mask_inpaint"] = pair_mask(parse_mask_info(mask_info, B, N))
    return batch


def batch_lengths(batch):
    """The valid residues per sample as Python ints: ``batch["lengths"]`` (what ``encode_6d_batch`` returns) or the reference's
    ``batch["aa_str"]`` (padded with "_", utils.py:27)."""
    if "lengths" in batch:
        return [int(v) for v in torch.as_tensor(batch["lengths"]).reshape(-1).tolist()]
    if "aa_str" in batch:
        return [sum(ch != "_" for ch in s) for s in batch["aa_str"]]
    from ._lib import T2PError
    raise T2PError("the random inpainting mask needs the residue counts: batch['lengths'] or batch['aa_str']")


def mask_count_range(length, inpainting_cfg, max_res_num=None):
    """``(lo, hi)`` = ``(int(mask_min_len * l), int(mask_max_len * l))``, the bounds of ``torch.randint`` at utils.py:34 / :46.  An empty
    range (``l = 1`` under the shipped 0.05 / 0.95) makes ``torch.randint`` raise in the reference; here it is a ``T2PError``."""
    from ._lib import T2PError
    l = int(length)
    lo, hi = int(inpainting_cfg.mask_min_len * l), int(inpainting_cfg.mask_max_len * l)
    if l < 0 or (max_res_num is not None and l > max_res_num):
        raise T2PError(f"a sample of {l} residues lies outside [0, {max_res_num}]")
    if not 0 <= lo < hi <= l:
        raise T2PError(f"a sample of {l} residues has the empty or misplaced range [{lo}, {hi}) for its number of masked residues "
                       f"(mask_min_len = {inpainting_cfg.mask_min_len}, mask_max_len = {inpainting_cfg.mask_max_len})")
    return lo, hi


def random_mask_batch(batch, config):
    """utils.py:15-60, which train.py calls before every train and eval step (train.py:176, :193): adds ``mask_inpaint`` (B, N, N) bool
    on ``config.device``; None when ``inpainting`` is not in the condition.

    The calls into ``random`` and ``torch`` are the reference's, in its order, on the CPU default generator: one ``random.random()`` per
    batch picks random / contiguous / no masking, then per sample ``torch.randint(int(min l), int(max l), (1,))`` and
    ``torch.randperm(l)`` (random) or ``torch.randint(0, l - r, (1,))`` (contiguous).  After the same ``random.seed`` and
    ``torch.manual_seed`` the mask is the reference's bit for bit.  Every range is checked before the first draw, so a refused batch
    (``T2PError``) consumes no random number."""
    if "inpainting" not in config.model.condition:
        batch["mask_inpaint"] = None
        return batch
    cfg = config.model.get("inpainting")
    if cfg is None:
        raise ValueError("the inpainting condition needs mask_info (residue ranges such as '1:5,10:15') or, for a random mask, "
                         "config.model.inpainting (random_mask_prob, contiguous_mask_prob, mask_min_len, mask_max_len)")
    B, _, N, _ = batch["coords_6d"].shape
    lengths = batch_lengths(batch)
    if len(lengths) != B:
        from ._lib import T2PError
        raise T2PError(f"{len(lengths)} residue counts for a batch of {B} samples")
    ranges = [mask_count_range(l, cfg, N) for l in lengths]
    prob = random.random()
    if prob < cfg.random_mask_prob:
        mask = torch.zeros(B, N)
        for b, (l, (lo, hi)) in enumerate(zip(lengths, ranges)):
            r = torch.randint(lo, hi, (1,))[0]
            mask[b, torch.randperm(l)[:r]] = 1
    elif prob > 1 - cfg.contiguous_mask_prob:
        mask = torch.zeros(B, N)
        for b, (l, (lo, hi)) in enumerate(zip(lengths, ranges)):
            r = int(torch.randint(lo, hi, (1,))[0])
            start = int(torch.randint(0, l - r, (1,))[0])
            mask[b, start:start + r] = 1
    else:
        mask = torch.ones(B, N)                       # the padding too: mask_pair removes it in the loss
    batch["mask_inpaint"] = pair_mask(mask).to(device=config.device)
    return batch


def get_condition_from_batch(config, batch, mask_info=None):
    """utils.py:84-106 for a tensor batch: one entry per name in ``config.model.condition``.

    ``batch`` holds ``coords_6d`` (B, C, L, L) and the residue counts either as ``lengths`` (B ints) or as the
    reference's ``aa_str`` (padded with "_").  ``inpainting`` takes ``mask_info``; without it the mask is drawn by
    ``random_mask_batch`` (utils.py:99-100), which needs ``config.model.inpainting``."""
    coords = batch["coords_6d"]
    B, L = coords.shape[0], config.data.max_res_num
    out = {}
    for name in config.model.condition:
        if name == "length":
            if "lengths" in batch:
                lengths = torch.as_tensor(batch["lengths"]).long()
            else:
                lengths = torch.tensor([sum(ch != "_" for ch in s) for s in batch["aa_str"]])
            inside = torch.arange(L)[None, :] < lengths[:, None]
            out[name] = inside[:, :, None] & inside[:, None, :]
        elif name == "ss":
            out[name] = coords[:, 4:7]
        elif name == "inpainting":
            if mask_info is None:
                out[name] = {"coords_6d": coords, "mask_inpaint": random_mask_batch(dict(batch), config)["mask_inpaint"]}
            else:
                out[name] = {"coords_6d": coords, "mask_inpaint": pair_mask(parse_mask_info(mask_info, B, L))}
        else:
            raise ValueError(f"unknown condition {name!r}")
    return out


def get_conditions_from_pdb(pdb, config, chain="A", mask_info=None, batch_size=8, sse=None, with_batch=False):
    """utils.py:122-137: chain ``chain`` of the file ``pdb``, featurised (dataset.py:311-325) and padded to ``max_res_num``
    (PaddingCollate), repeated over the batch, then ``get_condition_from_batch``; every tensor on ``config.device``, which must be a
    GPU.  ``sse``: one of a / b / c per residue (P-SEA letters), required by the 8-channel layout, or the word ``"psea"``: the letters
    are then computed from the chain's CA trace on the device (``encode.annotate_sse_batch``).  ``with_batch`` adds the
    featurised batch itself under ``"_batch"`` (replacement inpainting reads the maps and the residue counts from it).  A chain outside
    ``[min_res_num, max_res_num]`` is refused (the reference's dataset drops it, dataset.py:282-284)."""
    from .encode import encode_6d_batch, read_backbone
    xyz, atom_ok, nres = read_backbone(pdb, chain)
    lo, hi, C = config.data.min_res_num, config.data.max_res_num, config.data.num_channels
    if nres < lo or nres > hi:
        raise ValueError(f"chain {chain!r} of {pdb} has {nres} residues, outside [{lo}, {hi}] (data.min_res_num, data.max_res_num)")
    if C == 8:
        if sse is None:
            raise ValueError("an 8-channel model needs the chain's secondary-structure letters (a / b / c per residue): pass --sse")
        if sse != "psea" and len(sse) != nres:
            raise ValueError(f"--sse holds {len(sse)} letters, chain {chain!r} of {pdb} has {nres} residues")
    elif sse is not None:
        raise ValueError("--sse applies to 8-channel models only (data.num_channels)")
    device = torch.device(config.device if str(config.device) != "cuda" else "cuda:0")
    x = torch.zeros(1, hi, 3, 3)
    ok = torch.zeros(1, hi, 3, dtype=torch.uint8)
    x[0, :nres], ok[0, :nres] = torch.from_numpy(xyz), torch.from_numpy(atom_ok)
    one = encode_6d_batch(x.to(device), torch.tensor([nres]), atom_ok=ok.to(device), sse=sse if sse in (None, "psea") else [sse], num_channels=C)
    batch = {"coords_6d": one["coords_6d"].repeat(batch_size, 1, 1, 1), "mask_pair": one["mask_pair"].repeat(batch_size, 1, 1),
             "lengths": one["lengths"].repeat(batch_size), "ss_indices": one["ss_indices"] * batch_size}
    cond = get_condition_from_batch(config, batch, mask_info=mask_info)
    out = {k: {kk: vv.to(device) for kk, vv in v.items()} if isinstance(v, dict) else v.to(device) for k, v in cond.items()}
    if with_batch:
        out["_batch"] = {"coords_6d": batch["coords_6d"], "lengths": batch["lengths"]}
    return out


def synthetic_condition(config, batch, kind, device, length=100, mask_info="1:5,10:15", seed=0):
    """Benchmark conditions: a length mask for `length` residues and, for
    inpainting, the reference's default ``--mask_info`` with coords_6d ~ U(-1, 1)."""
    from . import synth
    L, C = config.data.max_res_num, config.data.num_channels
    cond = {}
    if "length" in kind:
        idx = length - config.data.min_res_num            # == length_index - 1 of the driver
        cond["length"] = get_mask_all_lengths(config, batch)[idx].to(device)
    if "inpainting" in kind:
        coords = torch.from_numpy(synth.uniform_pm1(seed, "coords_6d", batch * C * L * L).reshape(batch, C, L, L))
        cond["inpainting"] = {"coords_6d": coords.to(device),
                              "mask_inpaint": pair_mask(parse_mask_info(mask_info, batch, L)).to(device)}
    return cond
