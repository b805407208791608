"""6D encode of backbones on the device -- the featuriser the reference's PDB-driven conditions and its training batches come from.

Mirrors ``dataset.py``: ``get_coords6d`` (:396-450: virtual Cb, Cb-Cb distances within 20 A, the omega / theta dihedrals and the phi
angle, normalised to [-1, 1]), the residue / pair masks and the padding channel (:200-239), ``get_coarse_constraints`` (:114-168: helix,
beta and block-adjacency channels of the 8-channel layout) and ``PaddingCollate`` (:452-506).  One call of ``t2p_op_encode_6d`` encodes a
whole padded batch; there is no CPU path.  The secondary-structure letters themselves (the reference asks biotite's P-SEA for them) are
an input here: one of ``a`` / ``b`` / ``c`` per residue.  ``read_backbone`` is a small PDB text reader of the three backbone atoms.
"""
from __future__ import annotations

import ctypes as C

import numpy as np
import torch

from . import _lib
from ._lib import T2PError, check, ptr, stream_ptr

HELIX, BETA = 0, 1
MIN_BLOCK = 4          # runs shorter than this are no block (dataset.py:138-139)


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


def encode_6d_batch(xyz, nres, atom_ok=None, sse=None, num_channels=5):
    """``xyz`` (B, L, 3, 3) float32 device tensor (N, CA, C per residue, padded to L), ``nres`` (B,) residue counts, ``atom_ok``
    (B, L, 3) presence flags or None (all present), ``sse`` one letter string per sample (8 channels only; ``None`` or ``''`` = no
    blocks).  Returns the batch the condition builders and the training step take: ``coords_6d`` (B, C, L, L) float32 and ``mask_pair``
    (B, L, L) bool on the device, ``lengths`` (B,) int64 on the host, ``ss_indices`` one string per sample."""
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
