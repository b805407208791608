"""Backbones from sampled 6D maps on the device -- the stage the reference hands to PyRosetta (``sampling_rosetta.py:98-160``,
``rosetta_min/``), without the energy function.

The four decoded maps determine an N / CA / C backbone directly: Cb-Cb distances under ``known_below`` are completed to
all pairs by shortest paths, embedded by classical MDS and refined by ``stress_steps`` gradient steps on the known pairs; phi gives every
residue's CA - Cb direction, theta the azimuth of N about it and the featuriser's virtual-Cb identity then gives C; of the two mirror
images the one whose consecutive C and N close the chain is kept.  ``t2p_op_fold_6d`` does all of it for a whole batch in five launches;
there is no CPU path.  Rosetta's minimisation, relax / design and side chains are not here; the reference's restraint set
(``load_constraints``, rosetta_min/utils.py:119-206) is scored on the result with the harmonic forms Rosetta applies, so chains can be
ranked the way ``sampling_rosetta.py`` ranks its runs.  A minimisation against that restraint set -- a Cartesian L-BFGS, not Rosetta's
energy -- is ``text2protein_amd/refine.py`` (``fold_6d_batch(..., refine=True)``).  TM-align, which the reference runs on the backbones
next, is ``text2protein_amd/tmalign.py``: it takes the ``xyz`` this module leaves on the device.

``known_below`` defaults to 19.0 A (an encoded far pair decodes to exactly 20).  No trained checkpoint exists in this repository, so
the best value for SAMPLED maps is not measured; the default is only known to work on maps encoded from real geometry.
"""
from __future__ import annotations

import ctypes as C

import numpy as np
import torch

from . import _lib
from ._lib import T2PError, check, ptr, stream_ptr
from .decode import decode_6d_batch

SCORE_NAMES = ("dist", "omega", "theta", "phi")
CB_ATOM = (-0.58273431, 0.56802827, -0.54067466)          # the featuriser's virtual Cb (dataset.py:409)


def _workspace(lib, B, L, dev):
    if B < 1 or L < 1:
        raise ValueError(f"fold_6d needs at least one chain and one residue, not a batch of {B} maps of side {L}")
    nbytes = lib.t2p_op_fold_ws(B, L)
    if nbytes < 0:
        raise ValueError(f"fold_6d: maps of side {L} exceed FOLD_MAX_L (csrc/t2p_kernels.h: the coordinate arrays the kernel keeps in LDS)")
    return torch.empty(max(int(nbytes), 1), device=dev, dtype=torch.uint8), int(nbytes)


def diagnostics(status, placed, diag, lengths):
    """Host view of one call's outputs: one dict per chain."""
    st, pl, dg = status.cpu().tolist(), placed.cpu().numpy(), diag.cpu().numpy()
    out = []
    for b, n in enumerate(lengths.tolist()):
        d = dg[b]
        out.append({"L": int(n), "status": int(st[b]), "placed": np.nonzero(pl[b])[0].tolist(), "hand": int(d[0]),
                    "closure": [float(d[1]), float(d[2])], "stress_rms": float(d[3]),
                    "score": {nm: float(d[4 + k]) for k, nm in enumerate(SCORE_NAMES)},
                    "count": {nm: int(d[8 + k]) for k, nm in enumerate(SCORE_NAMES)},
                    "unreachable_pairs": int(d[12]), "eigenvalues": [float(v) for v in d[13:16]]})
    return out


def fold_maps_batch(absval, lengths, known_below=19.0, stress_steps=300, dist_std=2.0, angle_std=10.0):
    """The fold proper on what ``decode_6d_batch`` returns: ``absval`` (B, 4, L*L) float32 on the device, ``lengths`` (B,) on the host or
    the device (-1 = improper mask).  Returns ``xyz`` (B, L, 3, 3) float32, ``status`` (B,) int32, ``placed`` (B, L) uint8 and ``diag``
    (B, 16) float64 device tensors; nothing is read back."""
    if not isinstance(absval, torch.Tensor) or absval.dim() != 3 or absval.shape[1] != 4:
        raise ValueError("absval must be a (B, 4, L*L) tensor")
    if absval.device.type != "cuda":
        raise T2PError("fold_6d needs the maps on a GPU device (there is no CPU fallback)")
    lib = _lib.load()
    dev = absval.device
    a = absval.to(torch.float32).contiguous()
    B, L = a.shape[0], int(round(a.shape[2] ** 0.5))
    if L * L != a.shape[2]:
        raise ValueError("absval must hold square maps")
    n = torch.as_tensor(lengths).to(dev, torch.int32).contiguous()
    if tuple(n.shape) != (B,):
        raise ValueError(f"lengths must hold {B} entries")
    ws, nbytes = _workspace(lib, B, L, dev)
    xyz = torch.empty(B, L, 3, 3, device=dev, dtype=torch.float32)
    status = torch.empty(B, device=dev, dtype=torch.int32)
    placed = torch.empty(B, L, device=dev, dtype=torch.uint8)
    diag = torch.empty(B, 16, device=dev, dtype=torch.float64)
    with torch.cuda.device(dev):
        check(lib.t2p_op_fold_6d(ptr(a), ptr(n), B, L, float(known_below), int(stress_steps), float(dist_std), float(angle_std), ptr(xyz),
                                 ptr(status), ptr(placed), ptr(diag), ptr(ws), nbytes, stream_ptr()))
    return xyz, status, placed, diag


def fold_6d_batch(samples, known_below=19.0, stress_steps=300, dist_std=2.0, angle_std=10.0, refine=False, schedule=None, arm_min=None,
                  refine_rounds=1, refine_replicas=1, refine_seed=0, refine_stream=0, chain_ids=None):
    """``samples``: (B, C, L, L) float32 on the device, as the samplers return them.  Decodes and folds.  Returns a dict: ``xyz``
    (B, L, 3, 3), ``status`` (B,), ``placed`` (B, L), ``diag`` (B, 16) device tensors, ``absval`` (the decoded maps the fold read,
    (B, 4, L*L) on the device), ``lengths`` (B,) int32 on the host and
    ``chains``, the host diagnostics (one dict per chain: status, residues placed without a frame, hand kept, both closure errors,
    stress rms, the four restraint scores and their counts).

    ``refine=True`` then minimises every chain against the restraint set (text2protein_amd/refine.py; ``schedule`` and ``arm_min`` as
    there, at most 256 residues): ``xyz`` is the refined backbone, ``xyz_fold`` the fold's own, ``refine`` the per-chain diagnostics
    of the minimisation and ``refine_status`` / ``refine_diag`` its device tensors.  ``status``, ``diag`` and ``chains`` stay the fold's.
    With ``refine_rounds`` or ``refine_replicas`` above 1 the minimisation runs in rounds (``refine.refine_rounds_batch``: the
    reference's schedules, ``refine_seed`` / ``refine_stream`` / ``chain_ids`` for its draws; ``schedule`` is not used) and the dict
    gains ``refine_trace`` and ``refine_rounds`` (``refine.rounds_diagnostics``); with both at 1 the route and the bits are those of
    ``refine_backbone_batch``."""
    lengths, _, absval = decode_6d_batch(samples)
    xyz, status, placed, diag = fold_maps_batch(absval, lengths, known_below, stress_steps, dist_std, angle_std)
    out = {"xyz": xyz, "status": status, "placed": placed, "diag": diag, "lengths": lengths, "absval": absval,
           "chains": diagnostics(status, placed, diag, lengths)}
    if refine:
        from . import refine as R
        arm = R.ARM_MIN if arm_min is None else arm_min
        if int(refine_rounds) == 1 and int(refine_replicas) == 1:
            rx, rstatus, rdiag = R.refine_backbone_batch(xyz, absval, lengths, schedule, dist_std, angle_std, arm)
        else:
            rx, rstatus, rdiag, trace = R.refine_rounds_batch(xyz, absval, lengths, refine_rounds, refine_replicas, seed=refine_seed,
                                                              stream_base=refine_stream, chain_ids=chain_ids, dist_std=dist_std,
                                                              angle_std=angle_std, arm_min=arm)
            out.update(refine_trace=trace, refine_rounds=R.rounds_diagnostics(trace))
        out.update(xyz=rx, xyz_fold=xyz, refine_status=rstatus, refine_diag=rdiag, refine=R.diagnostics(rstatus, rdiag, lengths))
    return out


def fold_6d(samples, **kw):
    """One dict per chain, like ``decode_6d``: the diagnostics plus ``xyz`` (L, 3, 3) float32 numpy.  An improper mask raises
    ``ValueError`` with the reference's message (sampling_rosetta.py:72-73).  With ``refine=True`` ``xyz`` is the refined backbone and
    every dict gains ``xyz_fold`` and ``refine`` (that chain's minimisation diagnostics)."""
    if samples.dim() == 3:
        samples = samples.unsqueeze(0)
    r = fold_6d_batch(samples, **kw)
    xyz = r["xyz"].cpu().numpy()
    out = []
    for b, d in enumerate(r["chains"]):
        if d["status"] < 0:
            raise ValueError("Terminated due to improper masking channel...")
        one = dict(d, xyz=xyz[b, :d["L"]].copy())
        if "refine" in r:
            one.update(xyz_fold=r["xyz_fold"][b, :d["L"]].cpu().numpy(), refine=r["refine"][b])
        out.append(one)
    return out


def restraint_score(xyz, decoded, dist_std=2.0, angle_std=10.0):
    """The reference's restraint set scored on a backbone of the caller's.  ``xyz``: (L, 3, 3) or (B, L, 3, 3), N / CA / C per residue;
    ``decoded``: one dict of ``decode_6d`` (or a list of B), whose ``*_abs`` maps give the restraints.  Returns per chain
    ``{"score": {dist, omega, theta, phi}, "count": {...}}`` (a list when a batch was given).  Runs on the device."""
    single = isinstance(decoded, dict)
    decs = [decoded] if single else list(decoded)
    x = torch.as_tensor(np.asarray(xyz) if not isinstance(xyz, torch.Tensor) else xyz).to(torch.float32)
    if x.dim() == 3:
        x = x.unsqueeze(0)
    if x.dim() != 4 or tuple(x.shape[2:]) != (3, 3) or x.shape[0] != len(decs):
        raise ValueError("xyz must be (L, 3, 3) or (B, L, 3, 3) with one decoded dict per chain")
    if not torch.cuda.is_available():
        raise T2PError("restraint_score needs a GPU device (there is no CPU fallback)")
    dev = x.device if x.device.type == "cuda" else torch.device("cuda")
    lib = _lib.load()
    B, L = x.shape[0], x.shape[1]
    absval = torch.zeros(B, 4, L * L, dtype=torch.float32)
    lengths = []
    for b, d in enumerate(decs):
        n = int(d["L"])
        if n < 1 or n > L:
            raise ValueError(f"chain {b}: {n} residues do not fit xyz of {L}")
        for k, nm in enumerate(SCORE_NAMES):
            absval[b, k, :n * n] = torch.as_tensor(np.asarray(d[nm + "_abs"], np.float32)).reshape(-1)
        lengths.append(n)
    absval, x = absval.to(dev), x.to(dev).contiguous()
    n_dev = torch.tensor(lengths, dtype=torch.int32, device=dev)
    ws, nbytes = _workspace(lib, B, L, dev)
    out = torch.empty(B, 8, device=dev, dtype=torch.float64)
    with torch.cuda.device(dev):
        check(lib.t2p_op_restraint_score(ptr(x), ptr(absval), ptr(n_dev), B, L, float(dist_std), float(angle_std), ptr(out), ptr(ws), nbytes,
                                         stream_ptr()))
    o = out.cpu().numpy()
    res = [{"score": {nm: float(o[b, k]) for k, nm in enumerate(SCORE_NAMES)}, "count": {nm: int(o[b, 4 + k]) for k, nm in enumerate(SCORE_NAMES)}}
           for b in range(B)]
    return res[0] if single else res


def ss_agreement(xyz, lengths, target=None):
    """Does a folded (or refined) chain have its helices and strands where the ``ss`` condition put them?  ``xyz`` (B, L, 3, 3) or
    (B, L, 3) on the device, ``lengths`` (B,), ``target`` one letter string per chain (``encode.sse_target`` of the condition) or None.
    The chains are annotated on the device (``encode.annotate_sse_batch``, P-SEA).  Returns one dict per chain:
    ``letters``, ``counts`` (``encode.COUNT_NAMES``), ``status`` and, with a target, ``target``, ``helix_agreement`` = target-``a``
    residues labelled ``a`` / target-``a`` residues and ``strand_agreement`` likewise; each is None when its target is empty.  A chain
    whose length lies outside [1, L] (an improper mask: -1) has empty letters and zero counts."""
    from .encode import COUNT_NAMES, annotate_sse_batch
    r = annotate_sse_batch(xyz, lengths, target=target)
    counts, status = r["counts"].cpu().tolist(), r["status"].cpu().tolist()
    out = []
    for b, c in enumerate(counts):
        d = {"letters": r["letters"][b], "counts": dict(zip(COUNT_NAMES, c)), "status": status[b]}
        if target is not None:
            d.update(target=target[b], helix_agreement=c[6] / c[5] if c[5] else None, strand_agreement=c[8] / c[7] if c[7] else None)
        out.append(d)
    return out


def write_backbone_pdb(path, xyz, chain="A", resname="ALA", with_cb=False):
    """N / CA / C of one chain as fixed-column ATOM records (3 decimals), ``TER`` and ``END``; ``with_cb`` adds the virtual CB the
    featuriser builds from the three.  ``encode.read_backbone`` reads the file back."""
    x = np.asarray(xyz.detach().cpu() if isinstance(xyz, torch.Tensor) else xyz, dtype=np.float64)
    if x.ndim != 3 or x.shape[1:] != (3, 3) or x.shape[0] < 1:
        raise ValueError("xyz must be (L, 3, 3) with at least one residue")
    if x.shape[0] > 9999 or len(chain) != 1 or not 1 <= len(resname) <= 3:
        raise ValueError("at most 9999 residues, a one-letter chain and a residue name of up to three letters fit the PDB columns")
    if not np.isfinite(x).all() or np.abs(x).max() >= 9999.9995:
        raise ValueError("coordinates must be finite and fit the PDB format's %8.3f columns")
    atoms = [(" N  ", "N"), (" CA ", "C"), (" C  ", "C")] + ([(" CB ", "C")] if with_cb else [])
    lines, serial = ["REMARK   1 backbone folded from 6D maps (text2protein_amd.fold); N / CA / C only" + (", CB virtual" if with_cb else "")], 1
    for r in range(x.shape[0]):
        pos = list(x[r])
        if with_cb:
            b, c = x[r, 1] - x[r, 0], x[r, 2] - x[r, 1]
            pos.append(CB_ATOM[0] * np.cross(b, c) + CB_ATOM[1] * b + CB_ATOM[2] * c + x[r, 1])
        for (name, elem), p in zip(atoms, pos):
            lines.append(f"ATOM  {serial:5d} {name} {resname:>3s} {chain}{r + 1:4d}    {p[0]:8.3f}{p[1]:8.3f}{p[2]:8.3f}{1.0:6.2f}{0.0:6.2f}          {elem:>2s}")
            serial += 1
    lines += [f"TER   {serial:5d}      {resname:>3s} {chain}{x.shape[0]:4d}", "END"]
    with open(path, "w") as f:
        f.write("\n".join(lines) + "\n")
