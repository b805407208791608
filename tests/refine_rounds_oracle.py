"""Float64 numpy restatement of the refinement in rounds (text2protein_amd/refine.py, csrc/refine_rounds.hip): the phi / psi
move on an N / CA / C chain held in Cartesian coordinates, its Philox draws (oracle/philox.py) and the protocol -- perturb, minimise,
select -- over ``refine_oracle.refine`` / ``refine_oracle.energy``.  Written from the description, independently of the kernel.  Test
infrastructure only.

``internals(xyz)`` -> bond, theta, tau per atom; ``rebuild(xyz, dtau)`` -> the chain with ``dtau`` (rad, per atom) added to its torsions;
``draws(seed, stream, chain_id, n, amp)`` -> dphi, dpsi in degrees; ``perturb(xyz, ...)`` -> the K candidates of one chain;
``rounds(xyz0, maps, schedules, ...)`` -> dict.
"""
import numpy as np

import geom_oracle as GO
import refine_oracle as RO
from oracle import philox

GUARD = RO.GUARD
AMP = 10.0
SELECT_STAGE = (1, RO.SEP_ALL, 1.0, 0.5, 5.0, 0)          # scorefxn_cart.wts: atom_pair_constraint 1, dihedral / angle_constraint 0.5, vdw 5
# rosetta_min/run.py:5-7 as run.py reads them (setdefault(run, last listed value)): vdw_weight, rsr_dist_weight, rsr_orient_weight
W_REP_ROUNDS = (3.0, 5.0, 10.0, 10.0, 10.0)
W_DIST_ROUNDS = (3.0, 2.0, 1.0, 1.0, 1.0)
W_ANG_ROUNDS = (1.0, 1.0, 0.5, 0.5, 0.5)


# the recorded protocol run (tests/golden/make_golden_refine_rounds.py -> refine_rounds.npz): both chains in one batch, the short schedule
# per round with the round's weights; the seed is the first for which every selection has a margin (MIN_GAP) and is stored in the fixture
PROTOCOL = dict(chains=("96w8", "96cut"), chain_ids=(0, 1), rounds=2, replicas=3, iters=RO.SHORT_ITERS, stream_base=0, amp=AMP)
MIN_GAP = 1e-3


def selection_gaps(esel, cstatus):
    """Per round the relative gap between the two lowest E_sel among the valid candidates and the incumbent: (rounds,) array."""
    gaps, e_inc = [], np.inf
    for r in range(esel.shape[0]):
        pool = sorted([e for e, s in zip(esel[r], cstatus[r]) if s in (0, 1)] + ([e_inc] if np.isfinite(e_inc) else []))
        gaps.append((pool[1] - pool[0]) / abs(pool[1]) if len(pool) > 1 else np.inf)
        e_inc = min(e_inc, pool[0]) if pool else e_inc
    return np.array(gaps)


def round_schedule(r, iters=RO.STAGE_ITERS, sep_lo=1):
    r = min(r, len(W_REP_ROUNDS) - 1)
    return [(sep_lo, hi, W_DIST_ROUNDS[r], W_ANG_ROUNDS[r], W_REP_ROUNDS[r], iters) for hi in (12, 24, RO.SEP_ALL)]


def internals(xyz):
    """bond[k] = |a_k - a_k-1|, theta[k] = the angle at a_k-1, tau[k] = dihedral(a_k-3, a_k-2, a_k-1, a_k) for k >= 3 (zero before)."""
    a = np.asarray(xyz, np.float64).reshape(-1, 3)
    m = a.shape[0]
    bond, theta, tau = np.zeros(m), np.zeros(m), np.zeros(m)
    if m > 3:
        p0, p1, p2, p3 = a[:-3], a[1:-2], a[2:-1], a[3:]
        bond[3:] = np.linalg.norm(p3 - p2, axis=-1)
        theta[3:] = GO.angle(p1, p2, p3)
        tau[3:] = GO.dihedral_cross(p0, p1, p2, p3)
    return bond, theta, tau


def _frame(a, b, c):
    """The unit vectors (bc, n, m) atom d is placed in; the fallback where a, b and c are collinear or b and c coincide: bc = x when
    |c - b|^2 < GUARD, n = bc x e (e the coordinate axis on which bc is shortest) when |(b - a) x bc|^2 < GUARD."""
    bc = c - b
    l2 = bc @ bc
    bc = bc / np.sqrt(l2) if l2 >= GUARD else np.array([1.0, 0.0, 0.0])
    n = np.cross(b - a, bc)
    if n @ n < GUARD:
        e = np.zeros(3)
        e[np.argmin(np.abs(bc))] = 1.0
        n = np.cross(bc, e)
    n = n / np.sqrt(n @ n)
    return bc, n, np.cross(n, bc)


def rebuild(xyz, dtau):
    """NeRF: atoms 0..2 kept, every later atom placed from the three rebuilt atoms before it with the measured bond and angle and the
    measured torsion plus dtau[k]."""
    a = np.asarray(xyz, np.float64).reshape(-1, 3)
    bond, theta, tau = internals(a)
    out = a.copy()
    for k in range(3, a.shape[0]):
        bc, n, m = _frame(out[k - 3], out[k - 2], out[k - 1])
        t = tau[k] + dtau[k]
        out[k] = out[k - 1] + bond[k] * (-np.cos(theta[k]) * bc + np.sin(theta[k]) * (np.cos(t) * m + np.sin(t) * n))
    return out.reshape(np.asarray(xyz).shape)


def torsion_deltas(n, dphi_deg, dpsi_deg):
    """Per-atom torsion changes (rad): tau[3 i + 2] (places C_i) is phi_i, i >= 1; tau[3 i + 3] (places N_i+1) is psi_i, i <= n - 2."""
    d = np.zeros(3 * n)
    i = np.arange(1, n)
    d[3 * i + 2] = np.deg2rad(np.asarray(dphi_deg, np.float64)[1:])
    i = np.arange(0, n - 1)
    d[3 * i + 3] = np.deg2rad(np.asarray(dpsi_deg, np.float64)[:n - 1])
    return d


def draws(seed, stream, chain_id, n, amp=AMP):
    """dphi_i = amp (2 u(word 0) - 1), dpsi_i = amp (2 u(word 1) - 1), degrees: the training layout's counter {i, chain_id, stream lo,
    stream hi} under the key `seed`."""
    u = philox.train_uniforms(seed, stream, np.arange(n, dtype=np.uint64) + (np.uint64(int(chain_id) & 0xFFFFFFFF) << np.uint64(32)))
    u = u.astype(np.float64)
    return amp * (2.0 * u[:, 0] - 1.0), amp * (2.0 * u[:, 1] - 1.0)


def perturb(xyz, amp=AMP, seed=0, stream=0, replicas=1, keep_first=False, chain_id=0):
    """(K, n, 3, 3) float64 (not rounded): candidate k draws under stream + k; with keep_first candidate 0 is the input."""
    x = np.asarray(xyz, np.float64)
    n = x.shape[0]
    out = []
    for k in range(replicas):
        if k == 0 and keep_first:
            out.append(x.copy())
            continue
        out.append(rebuild(x, torsion_deltas(n, *draws(seed, stream + k, chain_id, n, amp))))
    return np.stack(out)


def rounds(xyz0, maps, schedules, select_stage=SELECT_STAGE, replicas=1, amp=AMP, seed=0, stream_base=0, chain_id=0):
    """The protocol of one chain.  Coordinates pass through float32 where the device's do: the candidates the move writes and the chains
    the minimiser writes.  Returns xyz (float32), status, kept (per round: the candidate that became the incumbent, or -1), esel /
    cstatus / evals (rounds, replicas), e_inc (per round, after it) and the kept candidate's refine dict."""
    m64 = {k: np.asarray(v, np.float64) for k, v in maps.items()}
    inc = np.asarray(xyz0, np.float32)
    e_inc, status, kept_run = np.inf, None, None
    R = len(schedules)
    esel, cstatus, evals = np.zeros((R, replicas)), np.zeros((R, replicas), int), np.zeros((R, replicas), int)
    kept, e_after = [], []
    for r, schedule in enumerate(schedules):
        cands = perturb(inc, amp, seed, stream_base + 16 * r, replicas, r == 0, chain_id).astype(np.float32)
        best, runs = -1, []
        for k in range(replicas):
            run = RO.refine(cands[k].astype(np.float64), m64, schedule)
            run["xyz32"] = run["xyz"].astype(np.float32)
            runs.append(run)
            esel[r, k] = RO.energy(run["xyz32"].astype(np.float64), m64, select_stage)[0]
            cstatus[r, k], evals[r, k] = run["status"], run["evaluations"]
            if run["status"] in (0, 1) and (best < 0 or esel[r, k] < esel[r, best]):
                best = k
        if best >= 0 and esel[r, best] < e_inc:
            inc, e_inc, status, kept_run = runs[best]["xyz32"], esel[r, best], runs[best]["status"], runs[best]
            kept.append(best)
        else:
            kept.append(-1)
        e_after.append(e_inc)
    return dict(xyz=inc, status=status, kept=kept, esel=esel, cstatus=cstatus, evals=evals, e_inc=np.array(e_after), run=kept_run)
