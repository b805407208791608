"""6D encode of backbones on the device -- the featuriser the reference's PDB-driven conditions and its training batches come from.

Mirrors ``dataset.py``: ``get_coords6d`` (:396-450: virtual Cb, Cb-Cb distances within 20 A, the omega / theta dihedrals and the phi
angle, normalised to [-1, 1]), the residue / pair masks and the padding channel (:200-239), ``get_coarse_constraints`` (:114-168: helix,
beta and block-adjacency channels of the 8-channel layout) and ``PaddingCollate`` (:452-506).  One call of ``t2p_op_encode_6d`` encodes a
whole padded batch; there is no CPU path.  The secondary-structure letters (the reference asks biotite's P-SEA for them,
dataset.py:121-123) are one of ``a`` / ``b`` / ``c`` per residue: supplied by the caller, or computed from the CA trace on the device by
``annotate_sse_batch`` (``t2p_op_annotate_sse``; ``sse="psea"``).  ``read_backbone`` is a small PDB text reader of the
three backbone atoms.
"""
from __future__ import annotations

import ctypes as C

import numpy as np
import torch

from . import _lib
from ._lib import T2PError, check, ptr, stream_ptr

HELIX, BETA = 0, 1
MIN_BLOCK = 4          # runs shorter than this are no block (dataset.py:138-139)
PSEA = "psea"          # the value of ``sse`` that asks for the annotation on the device
SSE_MAX_L = 512        # csrc/t2p_kernels.h: the trace t2p_op_annotate_sse keeps in LDS (the fold's limit)
COUNT_NAMES = ("a", "b", "c", "a_blocks", "b_blocks", "target_a", "target_a_hit", "target_b", "target_b_hit", "no_ca")


def sse_blocks(sse: str):
    """Runs of ``'a'`` (helix) and of ``'b'`` (strand) of at least four residues in a string of P-SEA letters, the helices first, each
    kind in chain order (dataset.py:131-153).  Returns ``(blocks, ss_indices)``: ``blocks`` = ``[(start, last, kind), ...]`` with ``last``
    the run's last residue, and the reference's ``"start:last,..."`` string (dataset.py:167), which ``batch["ss_indices"]`` takes as it is."""
    bad = set(sse) - set("abc")
    if bad:
        raise ValueError(f"secondary-structure letters must be a, b or c; found {sorted(bad)}")
    blocks = []
    for letter, kind in (("a", HELIX), ("b", BETA)):
        start = None
        for i, ch in enumerate(sse + "c"):
            if ch == letter and start is None:
                start = i
            elif ch != letter and start is not None:
                if i - start >= MIN_BLOCK:
                    blocks.append((start, i - 1, kind))
                start = None
    return blocks, ",".join(f"{s}:{l}" for s, l, _ in blocks)


def _letter_rows(target, B, L, dev):
    """(B, L) uint8 device tensor of letters from a tensor of that shape or from B strings (padded with 0)."""
    if isinstance(target, torch.Tensor):
        t = target.to(dev, torch.uint8).contiguous()
    else:
        if isinstance(target, str) or len(target) != B:
            raise ValueError(f"target must hold {B} strings, one per chain")
        rows = np.zeros((B, L), np.uint8)
        for b, letters in enumerate(target):
            if set(letters) - set("abc") or len(letters) > L:
                raise ValueError(f"target[{b}] must hold at most {L} letters a, b or c")
            rows[b, :len(letters)] = np.frombuffer(letters.encode(), np.uint8)
        t = torch.from_numpy(rows).to(dev)
    if tuple(t.shape) != (B, L):
        raise ValueError(f"target must be ({B}, {L})")
    return t


def annotate_sse_batch(xyz, nres, atom_ok=None, target=None):
    """Secondary structure of a batch of chains from their CA traces, on the device: P-SEA as DESIGN.md 8i states it
    (``t2p_op_annotate_sse``; there is no CPU path).  ``xyz`` (B, L, 3, 3) N / CA / C per residue, of which CA is read, or (B, L, 3) a
    bare CA trace; ``nres`` (B,) residue counts; ``atom_ok`` (B, L, 3) (or (B, L) for a CA trace) presence flags or None; ``target``
    B letter strings or a (B, L) uint8 tensor of letters, to count the agreement with, or None.  Returns ``letters`` (one string per
    chain; empty for a chain whose count lies outside [1, L]), ``letters_dev`` (B, L) uint8 and ``counts`` (B, 12) int32 on the device
    (the order of ``COUNT_NAMES``, two spare zeros) and ``status`` (B,) int32 on the device: 0, 1 when a CA that should be there was
    not finite or beyond 1e6 (it counts as absent), -1 for a residue count outside [1, L].  A residue without a CA is ``c``."""
    if not isinstance(xyz, torch.Tensor) or not (xyz.dim() == 4 and tuple(xyz.shape[2:]) == (3, 3) or xyz.dim() == 3 and xyz.shape[2] == 3):
        raise ValueError("xyz must be a (B, L, 3, 3) tensor (N / CA / C) or a (B, L, 3) tensor (a CA trace)")
    B, L, atoms = xyz.shape[0], xyz.shape[1], 3 if xyz.dim() == 4 else 1
    if B < 1 or not 1 <= L <= SSE_MAX_L:
        raise ValueError(f"annotate_sse takes at least one chain, padded to between 1 and {SSE_MAX_L} residues (SSE_MAX_L), not {B} of {L}")
    if xyz.device.type != "cuda":
        raise T2PError("annotate_sse needs the coordinates on a GPU device (there is no CPU fallback)")
    lib = _lib.load()
    dev = xyz.device
    x = xyz.to(torch.float32).contiguous()
    n = torch.as_tensor(nres).to(dev, torch.int32).contiguous()
    if tuple(n.shape) != (B,):
        raise ValueError(f"nres must hold {B} residue counts")
    ok = None
    if atom_ok is not None:
        ok = torch.as_tensor(atom_ok).to(dev).ne(0).to(torch.uint8).contiguous()
        if ok.numel() != B * L * atoms or ok.shape[:2] != (B, L):
            raise ValueError(f"atom_ok must be ({B}, {L}, {atoms})")
    t = None if target is None else _letter_rows(target, B, L, dev)
    letters = torch.empty(B, L, device=dev, dtype=torch.uint8)
    counts = torch.empty(B, 12, device=dev, dtype=torch.int32)
    status = torch.empty(B, device=dev, dtype=torch.int32)
    with torch.cuda.device(dev):
        check(lib.t2p_op_annotate_sse(ptr(x), ptr(n), ptr(ok), B, L, atoms, ptr(t), ptr(letters), ptr(counts), ptr(status), stream_ptr()))
    host = letters.cpu().numpy()
    return {"letters": [bytes(row[row != 0]).decode() for row in host], "letters_dev": letters, "counts": counts, "status": status}


def sse_target(coords_6d):
    """Per-residue target letters of an 8-channel condition, one string per sample: ``a`` where the diagonal of channel 4 (helix)
    rounds to 1, ``b`` where the diagonal of channel 5 (beta) does, else ``c``, up to the last residue the padding channel keeps (a
    residue the pair mask removes is ``c``; removed residues at the chain's end cannot be told from padding and are left out).  The
    channels hold the reference's half-open ``[start:last]`` blocks (dataset.py:141-151), so a block's last residue is ``c`` here."""
    x = torch.as_tensor(coords_6d)
    if x.dim() == 3:
        x = x.unsqueeze(0)
    if x.dim() != 4 or x.shape[1] != 8:
        raise ValueError("sse_target needs 8-channel maps (B, 8, L, L)")
    diag = torch.diagonal(x[:, [4, 5, 7]].detach().float(), dim1=-2, dim2=-1).round().cpu().numpy()       # (B, 3, L)
    out = []
    for helix, beta, inside in diag:
        row = np.where(helix == 1, "a", np.where(beta == 1, "b", "c"))
        kept = np.nonzero(inside == 1)[0]
        out.append("".join(row[:int(kept[-1]) + 1 if kept.size else 0]))
    return out


def encode_6d_batch(xyz, nres, atom_ok=None, sse=None, num_channels=5):
    """``xyz`` (B, L, 3, 3) float32 device tensor (N, CA, C per residue, padded to L), ``nres`` (B,) residue counts, ``atom_ok``
    (B, L, 3) presence flags or None (all present), ``sse`` one letter string per sample (8 channels only; ``None`` or ``''`` = no
    blocks) or the word ``"psea"``: the letters are then computed from the CA trace on the device (``annotate_sse_batch``) and go through
    ``sse_blocks`` exactly as supplied ones do.  Returns the batch the condition builders and the training step take: ``coords_6d``
    (B, C, L, L) float32 and ``mask_pair`` (B, L, L) bool on the device, ``lengths`` (B,) int64 on the host, ``ss_indices`` one string per sample."""
    if not isinstance(xyz, torch.Tensor) or xyz.dim() != 4 or tuple(xyz.shape[2:]) != (3, 3):
        raise ValueError("xyz must be a (B, L, 3, 3) tensor")
    if xyz.device.type != "cuda":
        raise T2PError("encode_6d needs the coordinates on a GPU device (there is no CPU fallback)")
    if num_channels not in (5, 8):
        raise ValueError(f"num_channels must be 5 or 8, not {num_channels}")
    lib = _lib.load()
    dev = xyz.device
    x = xyz.to(torch.float32).contiguous()
    B, L = x.shape[0], x.shape[1]
    n = torch.as_tensor(nres).to(dev, torch.int32).contiguous()
    if tuple(n.shape) != (B,):
        raise ValueError(f"nres must hold {B} residue counts")
    ok = None
    if atom_ok is not None:
        ok = torch.as_tensor(atom_ok).to(dev).ne(0).to(torch.uint8).contiguous()
        if tuple(ok.shape) != (B, L, 3):
            raise ValueError(f"atom_ok must be ({B}, {L}, 3)")
    lengths = n.cpu().long()
    quads, strings = [], [""] * B
    if sse is not None:
        if num_channels != 8:
            raise ValueError("secondary-structure letters need the 8-channel layout (num_channels=8)")
        if isinstance(sse, str) and sse == PSEA:
            sse = annotate_sse_batch(x, n, atom_ok=ok)["letters"]
        if isinstance(sse, str) or len(sse) != B:
            raise ValueError(f"sse must hold {B} strings, one per sample")
        for b, letters in enumerate(sse):
            if not letters:
                continue
            if len(letters) != int(lengths[b]):
                raise ValueError(f"sse[{b}] holds {len(letters)} letters, the sample has {int(lengths[b])} residues")
            blocks, strings[b] = sse_blocks(letters)
            quads += [(b, s, l, k) for s, l, k in blocks]
    arr = np.ascontiguousarray(np.asarray(quads, dtype=np.int32).reshape(-1, 4))
    coords = torch.empty(B, num_channels, L, L, device=dev, dtype=torch.float32)
    mask = torch.empty(B, L, L, device=dev, dtype=torch.uint8)
    with torch.cuda.device(dev):
        check(lib.t2p_op_encode_6d(ptr(x), ptr(n), ptr(ok), B, num_channels, L, C.c_void_p(arr.ctypes.data) if len(quads) else None,
                                   len(quads), ptr(coords), ptr(mask), stream_ptr()))
    return {"coords_6d": coords, "mask_pair": mask.bool(), "lengths": lengths, "ss_indices": strings}


def read_backbone(path, chain="A"):
    """N, CA and C of one chain of a PDB file: ``(xyz, atom_ok, nres)`` with ``xyz`` (nres, 3, 3) float32 (a missing atom is (0, 0, 0),
    dataset.py:219), ``atom_ok`` (nres, 3) uint8.  Fixed columns of ATOM / HETATM records; a residue is a run of records with one
    (residue number, insertion code), in file order; of each atom name the first occurrence counts (so of alternate locations the
    first).  An ATOM residue without backbone atoms stays in the chain with its flags cleared; a HETATM residue counts only when it
    carries all three (a modified amino acid, not a ligand, an ion or water).  Records are grouped by residue number and insertion code
    alone: a HETATM record that repeats those of the ATOM residue just before it is read as part of that residue.  A file with more
    than one MODEL is refused, as the reference skips it (dataset.py:180-182)."""
    names = {"N": 0, "CA": 1, "C": 2}
    residues, key, models = [], None, 0
    with open(path) as f:
        for line in f:
            rec = line[:6].strip()
            if rec == "MODEL":
                models += 1
                if models > 1:
                    raise ValueError(f"{path}: more than one MODEL (the reference skips such files)")
                key = None
                continue
            if rec == "TER":
                key = None
                continue
            if rec not in ("ATOM", "HETATM") or len(line) < 54 or line[21] != chain:
                continue
            k = (line[22:26], line[26])
            if k != key:
                key = k
                residues.append({"het": rec == "HETATM", "atoms": {}})
            a = names.get(line[12:16].strip())
            if a is not None and a not in residues[-1]["atoms"]:
                residues[-1]["atoms"][a] = (float(line[30:38]), float(line[38:46]), float(line[46:54]))
    residues = [r for r in residues if not r["het"] or len(r["atoms"]) == 3]
    nres = len(residues)
    if nres == 0:
        raise ValueError(f"{path}: no residues in chain {chain!r}")
    xyz = np.zeros((nres, 3, 3), np.float32)
    atom_ok = np.zeros((nres, 3), np.uint8)
    for i, r in enumerate(residues):
        for a, pos in r["atoms"].items():
            xyz[i, a] = pos
            atom_ok[i, a] = 1
    return xyz, atom_ok, nres
