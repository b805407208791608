"""Refinement of folded backbones against the reference's restraint set on the device -- the minimisation the reference runs between
its decoded maps and TM-align (``rosetta_min/run.py``), without Rosetta.

``t2p_op_refine_backbone`` minimises, per chain and in double, the restraint terms ``restraint_score`` sums (``load_constraints``'
sets with the forms Rosetta applies) plus ideal-geometry terms (bonds, angles, peptide planarity, a CA-CA repulsion) over the N / CA / C
coordinates, by a staged L-BFGS that one persistent workgroup runs without host round trips.  The stages follow the
reference's ``add_rst`` order -- sequence separations below 12, below 24, all -- with its run-0 weights.  There is no ``ref2015``, no
centroid term, no relax / design and no side chain here, and there is no CPU path.

``refine_rounds_batch`` is the reference's loop around that minimisation (``run.py:88-151``): five runs, each from the best
structure so far with every phi and psi moved by up to 10 degrees (``perturb_torsions``, the only torsion-space step here), each with
its run's weights (``reference_rounds``), a result kept only when it scores lower under ``SELECT_STAGE``.  ``replicas`` candidates per
round are minimised side by side -- one workgroup each -- and the lowest is the round's result; the reference makes one.

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


# ---- refinement in rounds (csrc/refine_rounds.hip) ----------------------------------------------------------------------
MAX_ROUNDS, MAX_REPLICAS, STREAM_STRIDE = 8, 16, 16
AMP_DEG = 10.0                                        # "diversify backbone": uniform in +-10 degrees on every phi and psi (run.py:104-109)
# per run, as run.py's setdefault really yields them from vdw_weight, rsr_dist_weight and rsr_orient_weight (key 2 is missing from the last two)
W_REP_ROUNDS = (3.0, 5.0, 10.0, 10.0, 10.0)
W_DIST_ROUNDS = (3.0, 2.0, 1.0, 1.0, 1.0)
W_ANG_ROUNDS = (1.0, 1.0, 0.5, 0.5, 0.5)
# what a run's result is scored with before it may replace the best so far: the constraint and vdw weights of scorefxn_cart.wts
SELECT_STAGE = (1, SEP_ALL, 1.0, 0.5, 5.0, 0)


def reference_rounds(rounds=5, sep_lo=1):
    """One schedule per round: the three separation stages with that round's weights, ``STAGE_ITERS`` iterations each.  Rounds past the
    fifth keep the fifth's weights."""
    out = []
    for r in range(int(rounds)):
        k = min(r, len(W_REP_ROUNDS) - 1)
        out.append([(int(sep_lo), hi, W_DIST_ROUNDS[k], W_ANG_ROUNDS[k], W_REP_ROUNDS[k], STAGE_ITERS) for hi in (12, 24, SEP_ALL)])
    return out


def _chain_ids(chain_ids, B, dev):
    ids = torch.arange(B, dtype=torch.int32) if chain_ids is None else torch.as_tensor(chain_ids)
    if tuple(ids.shape) != (B,):
        raise ValueError(f"chain_ids must hold {B} entries")
    return ids.to(dev, torch.int32).contiguous()


def _rounds_limits(L, rounds, replicas, what):
    if L > REFINE_MAX_L:
        raise ValueError(f"{what}: {L} residues exceed REFINE_MAX_L = {REFINE_MAX_L}")
    if not 1 <= int(rounds) <= MAX_ROUNDS:
        raise ValueError(f"{what}: rounds must lie in 1..{MAX_ROUNDS}, not {rounds}")
    if not 1 <= int(replicas) <= MAX_REPLICAS:
        raise ValueError(f"{what}: replicas must lie in 1..{MAX_REPLICAS}, not {replicas}")


def perturb_torsions(xyz, lengths, amp=AMP_DEG, seed=0, stream=0, replicas=1, keep_first=False, chain_ids=None):
    """The reference's phi / psi move on ``xyz`` (B, L, 3, 3) float32 on the device: every phi and psi of every chain moves by a uniform
    draw in +-``amp`` degrees, bond lengths, bond angles and omega stay as they are.  Candidate ``k`` of ``replicas`` draws under
    ``stream + k``; with ``keep_first`` candidate 0 is the input itself.  ``chain_ids`` (default 0 .. B - 1) name the chains to the
    generator, so a chain's move does not depend on where in a batch it sits.  Returns ``xyz`` (B, replicas, L, 3, 3) float32 and
    ``status`` (B, replicas) int32 (0 ok, 2 a coordinate not finite, -1 fewer than 2 residues), device tensors."""
    if not isinstance(xyz, torch.Tensor) or xyz.dim() != 4 or tuple(xyz.shape[2:]) != (3, 3):
        raise ValueError("xyz must be a (B, L, 3, 3) tensor")
    if xyz.device.type != "cuda":
        raise T2PError("perturb_torsions needs the coordinates on a GPU device (there is no CPU fallback)")
    B, L = xyz.shape[0], xyz.shape[1]
    if B < 1 or L < 1:
        raise ValueError(f"xyz of {tuple(xyz.shape)} holds no chain")
    _rounds_limits(L, 1, replicas, "perturb_torsions")
    if not (np.isfinite(amp) and amp >= 0):
        raise ValueError("amp (degrees) must be finite and not negative")
    dev = xyz.device
    n = torch.as_tensor(lengths).to(dev, torch.int32).contiguous()
    if tuple(n.shape) != (B,):
        raise ValueError(f"lengths must hold {B} entries")
    ids = _chain_ids(chain_ids, B, dev)
    x = xyz.to(torch.float32).contiguous()
    K = int(replicas)
    out = torch.empty(B, K, L, 3, 3, device=dev, dtype=torch.float32)
    status = torch.empty(B, K, device=dev, dtype=torch.int32)
    mask = (1 << 64) - 1
    with torch.cuda.device(dev):
        check(_lib.load().t2p_op_perturb_torsions(ptr(x), ptr(n), ptr(ids), B, L, K, float(amp), int(seed) & mask, int(stream) & mask,
                                                  int(bool(keep_first)), ptr(out), ptr(status), stream_ptr()))
    return out, status


def refine_rounds_batch(xyz, absval, lengths, rounds=5, replicas=1, amp=AMP_DEG, seed=0, stream_base=0, chain_ids=None, schedules=None,
                        select_stage=SELECT_STAGE, dist_std=DIST_STD, angle_std=ANGLE_STD, arm_min=ARM_MIN):
    """The reference's loop over runs on the device: every round perturbs the best chain so far into ``replicas``
    candidates (``perturb_torsions``; round 0 keeps the input as candidate 0), minimises each as ``refine_backbone_batch`` does under
    ``schedules[r]`` (default ``reference_rounds(rounds)``) and keeps the one of lowest ``restraint_energy`` total under
    ``select_stage`` when that is lower than the best so far.  Inputs as ``refine_backbone_batch``.  Returns ``xyz`` (B, L, 3, 3),
    ``status`` (B,), ``diag`` (B, 16) -- the kept candidate's, as ``refine_backbone_batch`` gives them -- and ``trace``
    (B, rounds, replicas, 4) float64: E_sel, status, evaluations, 1 where the candidate became the best so far.  Nothing is read back."""
    if isinstance(xyz, torch.Tensor) and xyz.dim() == 4:
        _rounds_limits(xyz.shape[1], rounds, replicas, "refine_rounds")
    lib, x, a, n, _, _, B, L = _inputs(xyz, absval, lengths, "refine_rounds")
    R, K = int(rounds), int(replicas)
    sched = np.ascontiguousarray(np.stack([_schedule_array(s) for s in (reference_rounds(R) if schedules is None else schedules)]))
    if sched.shape[0] != R:
        raise ValueError(f"{sched.shape[0]} schedules for {R} rounds")
    sel = _schedule_array([tuple(select_stage) + (0,) * (6 - len(select_stage))])
    nbytes = int(lib.t2p_op_refine_rounds_ws(B, L, R, K))
    if nbytes < 0:
        raise ValueError(f"refine_rounds: {B} chains x {K} replicas of {L} residues are out of range")
    ids = _chain_ids(chain_ids, B, x.device)
    ws = torch.empty(max(nbytes, 1), device=x.device, dtype=torch.uint8)
    out = torch.empty_like(x)
    status = torch.empty(B, device=x.device, dtype=torch.int32)
    diag = torch.empty(B, 16, device=x.device, dtype=torch.float64)
    trace = torch.empty(B, R, K, 4, device=x.device, dtype=torch.float64)
    mask = (1 << 64) - 1
    with torch.cuda.device(x.device):
        check(lib.t2p_op_refine_rounds(ptr(x), ptr(a), ptr(n), ptr(ids), B, L, sched.ctypes.data, R, sched.shape[1], K, sel.ctypes.data,
                                       float(amp), int(seed) & mask, int(stream_base) & mask, float(dist_std), float(angle_std),
                                       float(arm_min), ptr(out), ptr(status), ptr(diag), ptr(trace), ptr(ws), nbytes, stream_ptr()))
    return out, status, diag, trace


def rounds_diagnostics(trace):
    """Host view of a ``trace``: per chain a list of rounds, each ``{"candidates": [{"e_sel", "status", "evaluations"}, ...], "kept": k
    or None}``."""
    tr = trace.cpu().numpy()
    out = []
    for b in range(tr.shape[0]):
        rounds = []
        for r in range(tr.shape[1]):
            kept = np.nonzero(tr[b, r, :, 3] != 0)[0]
            rounds.append({"candidates": [{"e_sel": float(c[0]), "status": int(c[1]), "evaluations": int(c[2])} for c in tr[b, r]],
                           "kept": int(kept[0]) if kept.size else None})
        out.append(rounds)
    return out


def diagnostics(status, diag, lengths):
    """Host view of one call's outputs: one dict per chain."""
    st, dg = status.cpu().tolist(), diag.cpu().numpy()
    return [{"L": int(n), "status": int(st[b]), "energy_start": float(dg[b, 0]), "energy": float(dg[b, 1]),
             "terms": {nm: float(dg[b, 2 + k]) for k, nm in enumerate(TERM_NAMES)}, "iterations": int(dg[b, 10]),
             "evaluations": int(dg[b, 11]), "max_gradient": float(dg[b, 12]), "closure": float(dg[b, 13]), "stages": int(dg[b, 14])}
            for b, n in enumerate(torch.as_tensor(lengths).tolist())]
