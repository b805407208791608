"""Refinement of folded backbones against the reference's restraint set on the device -- the minimisation the reference runs between
its decoded maps and TM-align (``rosetta_min/run.py``), without Rosetta.

``t2p_op_refine_backbone`` minimises, per chain and in double, the restraint terms ``restraint_score`` sums (``load_constraints``'
sets with the forms Rosetta applies) plus ideal-geometry terms (bonds, angles, peptide planarity, a CA-CA repulsion) over the N / CA / C
coordinates, by a staged L-BFGS that one persistent workgroup runs without host round trips.  The stages follow the
reference's ``add_rst`` order -- sequence separations below 12, below 24, all -- with its run-0 weights.  There is no ``ref2015``, no
centroid term, no relax / design, no side chain and no torsion-space move here, and there is no CPU path.

``sep_lo`` defaults to 1, not the reference's 3: with no Ramachandran or centroid term the |i - j| < 3 restraints are what fixes the
local geometry.  ``default_schedule(3)`` gives the reference's sets.  ``arm_min`` (degrees) drops the theta / omega restraints whose
dihedral arm is nearly collinear with its axis at the target; whether 15 is the best cut has not been measured, nor has the behaviour
on maps sampled from a trained checkpoint (none exists in this repository).
"""
from __future__ import annotations

import numpy as np
import torch

from . import _lib
from ._lib import T2PError, check, ptr, stream_ptr

REFINE_MAX_L = 256
MAX_STAGES = 8
SEP_ALL = 1 << 20                     # "up to the chain's end"
TERM_NAMES = ("dist", "omega", "theta", "phi", "bond", "angle", "pept", "rep")
W_DIST, W_ANG, W_REP, STAGE_ITERS = 3.0, 1.0, 3.0, 300          # rsr_dist_weight[0], rsr_orient_weight[0], vdw_weight[0] (rosetta_min/run.py:5-7)
DIST_STD, ANGLE_STD, ARM_MIN = 2.0, 10.0, 15.0


def default_schedule(sep_lo=1):
    """One tuple per stage: ``(sep_lo, sep_hi, w_dist, w_ang, w_rep, max_iter)``; restraints count for ``sep_lo <= |i - j| < sep_hi``."""
    return [(int(sep_lo), hi, W_DIST, W_ANG, W_REP, STAGE_ITERS) for hi in (12, 24, SEP_ALL)]


def _schedule_array(schedule):
    s = np.ascontiguousarray(np.asarray(default_schedule() if schedule is None else schedule, dtype=np.float64))
    if s.ndim != 2 or s.shape[1] != 6 or not 1 <= s.shape[0] <= MAX_STAGES:
        raise ValueError(f"a schedule is 1 to {MAX_STAGES} stages of (sep_lo, sep_hi, w_dist, w_ang, w_rep, max_iter)")
    if not np.isfinite(s).all() or (s < 0).any():
        raise ValueError("the entries of a schedule must be finite and not negative")
    return s


def _inputs(xyz, absval, lengths, what):
    if not isinstance(xyz, torch.Tensor) or xyz.dim() != 4 or tuple(xyz.shape[2:]) != (3, 3):
        raise ValueError("xyz must be a (B, L, 3, 3) tensor")
    if not isinstance(absval, torch.Tensor) or absval.dim() != 3 or absval.shape[1] != 4:
        raise ValueError("absval must be a (B, 4, L*L) tensor")
    if xyz.device.type != "cuda" or absval.device != xyz.device:
        raise T2PError(f"{what} needs the coordinates and the maps on one GPU device (there is no CPU fallback)")
    B, L = xyz.shape[0], xyz.shape[1]
    if B < 1 or L < 1 or absval.shape[0] != B or absval.shape[2] != L * L:
        raise ValueError(f"xyz of {tuple(xyz.shape)} and absval of {tuple(absval.shape)} do not describe the same chains")
    if L > REFINE_MAX_L:
        raise ValueError(f"{what}: {L} residues exceed REFINE_MAX_L = {REFINE_MAX_L} (csrc/t2p_kernels.h: the vectors the kernel keeps in LDS)")
    dev = xyz.device
    n = torch.as_tensor(lengths).to(dev, torch.int32).contiguous()
    if tuple(n.shape) != (B,):
        raise ValueError(f"lengths must hold {B} entries")
    lib = _lib.load()
    nbytes = int(lib.t2p_op_refine_ws(B, L))
    if nbytes < 0:
        raise ValueError(f"{what}: {L} residues exceed REFINE_MAX_L = {REFINE_MAX_L}")
    ws = torch.empty(max(nbytes, 1), device=dev, dtype=torch.uint8)
    return lib, xyz.to(torch.float32).contiguous(), absval.to(torch.float32).contiguous(), n, ws, nbytes, B, L


def refine_backbone_batch(xyz, absval, lengths, schedule=None, dist_std=DIST_STD, angle_std=ANGLE_STD, arm_min=ARM_MIN):
    """``xyz`` (B, L, 3, 3) float32 and ``absval`` (B, 4, L*L) float32 on the device, ``lengths`` (B,) as ``fold_maps_batch`` takes and
    returns them.  Returns ``xyz`` (B, L, 3, 3) float32, ``status`` (B,) int32 (0 ok, 1 a stage ended on a failed line search, 2 a start
    coordinate not finite, -1 fewer than 2 residues or an improper mask) and ``diag`` (B, 16) float64 device tensors; nothing is read
    back."""
    lib, x, a, n, ws, nbytes, B, L = _inputs(xyz, absval, lengths, "refine_backbone")
    sched = _schedule_array(schedule)
    out = torch.empty_like(x)
    status = torch.empty(B, device=x.device, dtype=torch.int32)
    diag = torch.empty(B, 16, device=x.device, dtype=torch.float64)
    with torch.cuda.device(x.device):
        check(lib.t2p_op_refine_backbone(ptr(x), ptr(a), ptr(n), B, L, sched.ctypes.data, sched.shape[0], float(dist_std), float(angle_std),
                                         float(arm_min), ptr(out), ptr(status), ptr(diag), ptr(ws), nbytes, stream_ptr()))
    return out, status, diag


def restraint_energy(xyz, absval, lengths, stage=None, dist_std=DIST_STD, angle_std=ANGLE_STD, arm_min=ARM_MIN):
    """One evaluation of the refinement's energy under one stage's parameters (default: the last default stage), by the device
    functions the minimiser calls.  Returns ``terms`` (B, 9) float64 -- the eight unweighted terms of ``TERM_NAMES``, then the weighted
    total -- and ``grad`` (B, L, 3, 3) float64, device tensors."""
    lib, x, a, n, ws, nbytes, B, L = _inputs(xyz, absval, lengths, "restraint_energy")
    st = _schedule_array([default_schedule()[-1] if stage is None else tuple(stage) + (0,) * (6 - len(stage))])
    terms = torch.empty(B, 9, device=x.device, dtype=torch.float64)
    grad = torch.empty(B, L, 3, 3, device=x.device, dtype=torch.float64)
    with torch.cuda.device(x.device):
        check(lib.t2p_op_restraint_energy(ptr(x), ptr(a), ptr(n), B, L, st.ctypes.data, float(dist_std), float(angle_std), float(arm_min),
                                          ptr(terms), ptr(grad), ptr(ws), nbytes, stream_ptr()))
    return terms, grad


def diagnostics(status, diag, lengths):
    """Host view of one call's outputs: one dict per chain."""
    st, dg = status.cpu().tolist(), diag.cpu().numpy()
    return [{"L": int(n), "status": int(st[b]), "energy_start": float(dg[b, 0]), "energy": float(dg[b, 1]),
             "terms": {nm: float(dg[b, 2 + k]) for k, nm in enumerate(TERM_NAMES)}, "iterations": int(dg[b, 10]),
             "evaluations": int(dg[b, 11]), "max_gradient": float(dg[b, 12]), "closure": float(dg[b, 13]), "stages": int(dg[b, 14])}
            for b, n in enumerate(torch.as_tensor(lengths).tolist())]
