"""Float64 numpy restatement of the restraint refinement (text2protein_amd/refine.py, csrc/refine.hip): the energy over
N / CA / C with its own analytic gradient, and the staged L-BFGS.  Written from the description, independently of the kernel: the
gradient is scattered term by term with ``numpy.add.at`` where the kernel gathers per residue.  Test infrastructure only.

``energy(xyz, maps, stage)`` -> (total, terms (8,), gradient (n, 3, 3)); ``refine(xyz0, maps, schedule)`` -> dict;
``noisy_maps(clean, sd_dist, sd_ang, seed)`` -> reproducible noisy copies of a chain's four maps (oracle/philox.py).
"""
import numpy as np

import fold_oracle as FO
import geom_oracle as GO
from oracle import philox

K1, K2, K3 = GO.K1, GO.K2, GO.K3
NEIGHBOUR = FO.NEIGHBOUR
DIST_STD, ANGLE_STD, ARM_MIN = 2.0, 10.0, 15.0
BOND_SIGMA, ANGLE_SIGMA, PEPT_SIGMA = 0.02, 3.0, 6.0                     # A, degrees, degrees
BOND_N_CA, BOND_CA_C, BOND_C_N = 1.458, 1.525, 1.329
ANGLE_N_CA_C, ANGLE_CA_C_N, ANGLE_C_N_CA = 111.0, 116.2, 121.7
REP_RADIUS, REP_MIN_SEP = 3.8, 2
HISTORY, ARMIJO_C1, MAX_TRIALS, GRAD_TOL, CURVATURE_EPS = 8, 1e-4, 20, 1e-3, 1e-10
W_DIST, W_ANG, W_REP, STAGE_ITERS = 3.0, 1.0, 3.0, 300
SEP_ALL = 1 << 20                                                         # "up to the chain's end"
GUARD = GO.GUARD                                                          # floor of every denominator
TERMS = ("dist", "omega", "theta", "phi", "bond", "angle", "pept", "rep")


def default_schedule(sep_lo=1):
    """(sep_lo, sep_hi, w_dist, w_ang, w_rep, max_iter) per stage: the reference's add_rst order, its run-0 weights."""
    return [(sep_lo, hi, W_DIST, W_ANG, W_REP, STAGE_ITERS) for hi in (12, 24, SEP_ALL)]


def short_schedule(iters, sep_lo=1):
    return [s[:5] + (iters,) for s in default_schedule(sep_lo)]


# ---------------------------------------------------------------------------------------------------------------------------------
def restraint_lists(maps, arm_min=ARM_MIN):
    """Index arrays of the four sets (fold_oracle.restraint_sets) after the arm_min filter: a theta restraint goes when its target
    phi_ij is within arm_min degrees of 0 or 180, an omega restraint when phi_ij or phi_ji is."""
    sd, so, sa = FO.restraint_sets(maps)
    phi = np.asarray(maps["phi"], np.float64)
    a = np.deg2rad(arm_min)
    flat = (phi < a) | (phi > np.pi - a)
    return dict(dist=np.nonzero(sd), omega=np.nonzero(so & ~flat & ~flat.T), theta=np.nonzero(sa & ~flat), phi=np.nonzero(sa))


_wrap = GO.wrap


def _dot(a, b):
    return (a * b).sum(-1)


def _dihedral(p0, p1, p2, p3):
    """Value (geom_oracle.dihedral_cross) and the four gradients of the dihedral p0-p1-p2-p3, rows of points."""
    val = GO.dihedral_cross(p0, p1, p2, p3)
    f, g, h = p0 - p1, p1 - p2, p3 - p2
    a, b = np.cross(f, g), np.cross(h, g)
    gl = np.sqrt(np.maximum(_dot(g, g), GUARD))
    aa, bb = np.maximum(_dot(a, a), GUARD), np.maximum(_dot(b, b), GUARD)
    d0 = (-gl / aa)[:, None] * a
    d3 = (gl / bb)[:, None] * b
    fa, hb = (_dot(f, g) / (aa * gl))[:, None] * a, (_dot(h, g) / (bb * gl))[:, None] * b
    return val, d0, -d0 + fa - hb, -d3 - fa + hb, d3


def _angle(pa, pb, pc):
    """Value (geom_oracle.angle) and the three gradients of the angle at pb."""
    val = GO.angle(pa, pb, pc)
    v, w = pa - pb, pc - pb
    cr = np.cross(v, w)
    sn = np.sqrt(_dot(cr, cr))
    ga = np.cross(v, cr) / np.maximum(_dot(v, v) * sn, GUARD)[:, None]
    gc = -np.cross(w, cr) / np.maximum(_dot(w, w) * sn, GUARD)[:, None]
    return val, ga, -ga - gc, gc


def energy(xyz, maps, stage, dist_std=DIST_STD, angle_std=ANGLE_STD, arm_min=ARM_MIN, lists=None):
    x = np.asarray(xyz, np.float64)
    n = x.shape[0]
    sep_lo, sep_hi, w_dist, w_ang, w_rep = stage[:5]
    lists = lists or restraint_lists(maps, arm_min)
    N, CA, C = x[:, 0], x[:, 1], x[:, 2]
    bv, cv = CA - N, C - CA
    CB = GO.virtual_cb(N, CA, C)
    gN, gCA, gC, gCB = (np.zeros((n, 3)) for _ in range(4))
    terms = np.zeros(8)
    astd = np.deg2rad(angle_std)

    def band(ij):
        i, j = ij
        s = np.abs(i - j)
        k = (s >= sep_lo) & (s < sep_hi)
        return i[k], j[k]

    def scatter(w, res, parts):                       # res (m,), parts: [(gradient array, index, dvalue)]
        for arr, idx, dv in parts:
            np.add.at(arr, idx, (w * res)[:, None] * dv)

    # dist
    i, j = band(lists["dist"])
    dv = CB[i] - CB[j]
    r = np.sqrt(_dot(dv, dv))
    res = (r - maps["dist"][i, j]) / dist_std
    terms[0] = (res * res).sum()
    u = dv / np.maximum(r, GUARD)[:, None]
    scatter(w_dist * 2.0 / dist_std, res, [(gCB, i, u), (gCB, j, -u)])
    # omega: CA_i Cb_i Cb_j CA_j
    i, j = band(lists["omega"])
    val, d0, d1, d2, d3 = _dihedral(CA[i], CB[i], CB[j], CA[j])
    res = _wrap(val - maps["omega"][i, j]) / astd
    terms[1] = (res * res).sum()
    scatter(w_ang * 2.0 / astd, res, [(gCA, i, d0), (gCB, i, d1), (gCB, j, d2), (gCA, j, d3)])
    # theta: N_i CA_i Cb_i Cb_j
    i, j = band(lists["theta"])
    val, d0, d1, d2, d3 = _dihedral(N[i], CA[i], CB[i], CB[j])
    res = _wrap(val - maps["theta"][i, j]) / astd
    terms[2] = (res * res).sum()
    scatter(w_ang * 2.0 / astd, res, [(gN, i, d0), (gCA, i, d1), (gCB, i, d2), (gCB, j, d3)])
    # phi: CA_i Cb_i Cb_j
    i, j = band(lists["phi"])
    val, da, db, dc = _angle(CA[i], CB[i], CB[j])
    res = (val - maps["phi"][i, j]) / astd
    terms[3] = (res * res).sum()
    scatter(w_ang * 2.0 / astd, res, [(gCA, i, da), (gCB, i, db), (gCB, j, dc)])
    # bonds
    k = np.arange(n)
    k1 = np.arange(n - 1)
    for (pa, ia, ga), (pb, ib, gb), b0 in (((N, k, gN), (CA, k, gCA), BOND_N_CA), ((CA, k, gCA), (C, k, gC), BOND_CA_C),
                                           ((C, k1, gC), (N, k1 + 1, gN), BOND_C_N)):
        dv = pa[ia] - pb[ib]
        r = np.sqrt(_dot(dv, dv))
        res = (r - b0) / BOND_SIGMA
        terms[4] += (res * res).sum()
        u = dv / np.maximum(r, GUARD)[:, None]
        scatter(2.0 / BOND_SIGMA, res, [(ga, ia, u), (gb, ib, -u)])
    # angles
    asig = np.deg2rad(ANGLE_SIGMA)
    for (pa, ia, ga), (pb, ib, gb), (pc, ic, gc), a0 in (((N, k, gN), (CA, k, gCA), (C, k, gC), ANGLE_N_CA_C),
                                                         ((CA, k1, gCA), (C, k1, gC), (N, k1 + 1, gN), ANGLE_CA_C_N),
                                                         ((C, k1, gC), (N, k1 + 1, gN), (CA, k1 + 1, gCA), ANGLE_C_N_CA)):
        val, da, db, dc = _angle(pa[ia], pb[ib], pc[ic])
        res = (val - np.deg2rad(a0)) / asig
        terms[5] += (res * res).sum()
        scatter(2.0 / asig, res, [(ga, ia, da), (gb, ib, db), (gc, ic, dc)])
    # peptide planarity: CA_i C_i N_i+1 CA_i+1 about 180
    psig = np.deg2rad(PEPT_SIGMA)
    val, d0, d1, d2, d3 = _dihedral(CA[k1], C[k1], N[k1 + 1], CA[k1 + 1])
    res = _wrap(val - np.pi) / psig
    terms[6] = (res * res).sum()
    scatter(2.0 / psig, res, [(gCA, k1, d0), (gC, k1, d1), (gN, k1 + 1, d2), (gCA, k1 + 1, d3)])
    # repulsion
    i, j = np.nonzero(np.triu(np.ones((n, n), bool), REP_MIN_SEP))
    dv = CA[i] - CA[j]
    r = np.sqrt(_dot(dv, dv))
    res = np.maximum(0.0, REP_RADIUS - r)
    terms[7] = (res * res).sum()
    u = dv / np.maximum(r, GUARD)[:, None]
    scatter(-2.0 * w_rep, res, [(gCA, i, u), (gCA, j, -u)])
    # through the virtual Cb: Cb = CA + K1 (b x c) + K2 b + K3 c
    gb = K1 * np.cross(cv, gCB) + K2 * gCB
    gc = K1 * np.cross(gCB, bv) + K3 * gCB
    grad = np.stack([gN - gb, gCA + gCB + gb - gc, gC + gc], axis=1)
    total = w_dist * terms[0] + w_ang * (terms[1] + terms[2] + terms[3]) + terms[4] + terms[5] + terms[6] + w_rep * terms[7]
    return float(total), terms, grad


# ---------------------------------------------------------------------------------------------------------------------------------
def refine(xyz0, maps, schedule=None, dist_std=DIST_STD, angle_std=ANGLE_STD, arm_min=ARM_MIN, trace=None):
    """The staged L-BFGS.  Evaluations counted: one at the start (last stage's weights), one at the start of every stage, one per
    line-search trial, one at the end.  Iterations counted: line searches run."""
    schedule = schedule or default_schedule()
    maps = {k: np.asarray(v, np.float64) for k, v in maps.items()}
    lists = restraint_lists(maps, arm_min)
    x = np.asarray(xyz0, np.float64).copy()
    shape = x.shape
    evals = iters = status = 0

    def ev(y, stage):
        nonlocal evals
        evals += 1
        e, t, g = energy(y.reshape(shape), maps, stage, dist_std, angle_std, arm_min, lists)
        return e, t, g.reshape(-1)

    x = x.reshape(-1)
    e_start = ev(x, schedule[-1])[0]
    stages_done = 0
    for stage in schedule:
        e, _, g = ev(x, stage)
        hist = []                                      # (s, y, 1 / s.y), oldest first
        for _ in range(int(stage[5])):
            if np.abs(g).max() < GRAD_TOL:
                break
            d = None
            if hist:
                q = g.copy()
                alpha = []
                for s, y, rho in reversed(hist):
                    a = rho * (s @ q)
                    alpha.append(a)
                    q -= a * y
                s, y, _ = hist[-1]
                q *= (s @ y) / (y @ y)
                for (s, y, rho), a in zip(hist, reversed(alpha)):
                    q += (a - rho * (y @ q)) * s
                d = -q
                if not (g @ d < 0.0):
                    d, hist = None, []
            steepest = d is None
            if steepest:
                d = -g
            gd = g @ d
            t = 1.0 / max(np.sqrt(g @ g), 1.0) if steepest else 1.0
            iters += 1
            ok = False
            for _ in range(MAX_TRIALS):
                xt = x + t * d
                et, _, gt = ev(xt, stage)
                if np.isfinite(et) and et <= e + ARMIJO_C1 * t * gd:
                    ok = True
                    break
                t *= 0.5
            if trace is not None:
                trace.append((e, et if ok else None, t, steepest, len(hist)))
            if not ok:
                if steepest:
                    status |= 1
                    break
                hist = []
                continue
            s, y = xt - x, gt - g
            sy = s @ y
            if sy > CURVATURE_EPS * np.sqrt(s @ s) * np.sqrt(y @ y):
                hist = (hist + [(s, y, 1.0 / sy)])[-HISTORY:]
            x, e, g = xt, et, gt
        stages_done += 1
    e_end, terms, g = ev(x, schedule[-1])
    xyz = x.reshape(shape)
    return dict(xyz=xyz, status=status, e_start=e_start, e_end=e_end, terms=terms, iterations=iters, evaluations=evals,
                gmax=float(np.abs(g).max()), closure=FO.closure(xyz), stages=stages_done)


# ---------------------------------------------------------------------------------------------------------------------------------
def noisy_maps(clean, sd_dist, sd_ang, seed):
    """Gaussian noise on the known distances (A) and on the angles (rad) of pairs with 0 < d < 20: symmetric for dist and omega, per
    ordered pair for theta and phi; dist clipped to [0.5, 19.99], phi to [0.01, pi - 0.01].  Returned as float32, what a decode gives."""
    d = np.asarray(clean["dist"], np.float64)
    n = d.shape[0]
    z = philox.normals(seed, 0, 0, 4 * n * n).reshape(4, n, n)
    sym = lambda a: np.triu(a, 1) + np.triu(a, 1).T
    known = (d > 0) & (d < FO.DMAX)
    out = {}
    out["dist"] = np.where(known, np.clip(d + sd_dist * sym(z[0]), 0.5, 19.99), d)
    om = np.asarray(clean["omega"], np.float64)
    out["omega"] = np.where(known, GO.wrap(om + sd_ang * sym(z[1])), om)
    out["theta"] = np.where(known, GO.wrap(np.asarray(clean["theta"], np.float64) + sd_ang * z[2]), clean["theta"])
    out["phi"] = np.where(known, np.clip(np.asarray(clean["phi"], np.float64) + sd_ang * z[3], 0.01, np.pi - 0.01), clean["phi"])
    return {k: v.astype(np.float32) for k, v in out.items()}


def maps_of(xyz):
    """The four absolute maps of a backbone whose Cb pairs all lie under 20 A (the 8-residue window): float32, zero diagonal."""
    x = np.asarray(xyz, np.float64)
    n = x.shape[0]
    cb = FO.virtual_cb(x)
    i, j = np.nonzero(~np.eye(n, dtype=bool))
    out = {k: np.zeros((n, n)) for k in ("dist", "omega", "theta", "phi")}
    out["dist"][i, j] = np.linalg.norm(cb[i] - cb[j], axis=-1)
    assert out["dist"].max() < FO.DMAX
    out["omega"][i, j] = _dihedral(x[i, 1], cb[i], cb[j], x[j, 1])[0]
    out["theta"][i, j] = _dihedral(x[i, 0], x[i, 1], cb[i], cb[j])[0]
    out["phi"][i, j] = _angle(x[i, 1], cb[i], cb[j])[0]
    return {k: v.astype(np.float32) for k, v in out.items()}


# the fixture's cases (tests/golden/make_golden_refine.py): chain of fold_chains.npz, noise on dist (A) and on the angles (rad), seed
CASES = {"96cut": ("96cut", 1.0, 0.1, 11), "48": ("48", 1.0, 0.1, 12), "96": ("96", 0.5, 0.05, 13), "132": ("132", 0.0, 0.0, 0),
         "96w8": ("96w8", 0.0, 0.0, 0)}
NOISY = ("96cut", "48", "96")
SHORT_ITERS = 5


def case_truth(fold_gold, name):
    return fold_gold["xyz_96"][11:19] if name == "96w8" else fold_gold[f"xyz_{CASES[name][0]}"]


def case_maps(fold_gold, name):
    """The float32 maps of a case, rebuilt from fold_chains.npz (nothing noisy is committed)."""
    key, sd_dist, sd_ang, seed = CASES[name]
    if name == "96w8":
        return maps_of(case_truth(fold_gold, name))
    clean = {k: fold_gold[f"{k}_{key}"] for k in ("dist", "omega", "theta", "phi")}
    return noisy_maps(clean, sd_dist, sd_ang, seed) if sd_dist > 0 else {k: np.asarray(v, np.float32) for k, v in clean.items()}
