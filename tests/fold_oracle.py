"""Float64 numpy restatement of the restraint-free fold (text2protein_amd/fold.py, csrc/fold.hip): decoded 6D maps ->
N / CA / C.  Written from the algorithm's description, independently of the kernels, with ``numpy.linalg.eigh`` where the kernel
iterates.  Test infrastructure only: nothing in the package imports it and there is no CPU path in the product.

``fold(maps)`` takes the four absolute maps (dist in A, omega / theta / phi in rad, each (n, n)) and returns a dict; ``dtype`` runs the
restraint score (and only it) in another precision, which is how the fixture's float32 / float64 gap is made.
"""
import numpy as np

import geom_oracle as GO

K1, K2, K3 = GO.K1, GO.K2, GO.K3                            # the featuriser's virtual-Cb identity (dataset.py:409)
N_CA, CA_C, N_CA_C, C_N = 1.458, 1.525, 111.0, 1.329
DMAX, NEIGHBOUR = 20.0, 12.0


def ideal_cb():
    """|Cb - CA| and the N-CA-Cb angle that the identity gives at ideal N-CA, CA-C and N-CA-C."""
    b = np.array([N_CA, 0.0, 0.0])                                        # CA - N
    t = np.deg2rad(N_CA_C)
    c = CA_C * np.array([-np.cos(t), np.sin(t), 0.0])                     # C - CA: angle between -b and c is N-CA-C
    off = K1 * np.cross(b, c) + K2 * b + K3 * c
    r = np.linalg.norm(off)
    return float(r), float(np.arccos(-(b @ off) / (N_CA * r)))


R_CB, A_NCACB = ideal_cb()


def pairs(dist, known_below=19.0):
    """Symmetric distances from the upper triangle, the known-pair and the neighbour masks."""
    du = np.triu(np.asarray(dist, np.float64), 1)
    d = du + du.T
    off = ~np.eye(d.shape[0], dtype=bool)
    known = off & (d < known_below)
    return d, known, known & (d <= NEIGHBOUR)


def geodesics(d, known):
    g = np.where(known, d, np.inf)
    np.fill_diagonal(g, 0.0)
    for k in range(g.shape[0]):
        g = np.minimum(g, g[:, k:k + 1] + g[k:k + 1, :])
    unreachable = np.isinf(g)
    if unreachable.any():
        finite = g[~unreachable]
        g[unreachable] = (finite.max() if finite.size else 0.0) + DMAX
    return g, int(unreachable.sum())


def classical_mds(g):
    n = g.shape[0]
    d2 = g * g
    b = -0.5 * (d2 - d2.mean(0, keepdims=True) - d2.mean(1, keepdims=True) + d2.mean())
    w, v = np.linalg.eigh(b)
    w, v = w[::-1][:3], v[:, ::-1][:, :3]
    if v.shape[1] < 3:
        v = np.concatenate([v, np.zeros((n, 3 - v.shape[1]))], 1)
        w = np.concatenate([w, np.zeros(3 - w.shape[0])])
    ramp = np.arange(n) - (n - 1) / 2.0
    corr = ramp @ v                                                       # sign convention: every axis rises along the chain
    v = v * np.where(corr < 0, -1.0, 1.0)
    denom = np.linalg.norm(ramp) if n > 1 else 1.0
    return v * np.sqrt(np.maximum(w, 1e-12)), w, np.abs(corr) / max(denom, 1e-30)


def stress_refine(x, d, known, steps):
    n = x.shape[0]
    off = ~np.eye(n, dtype=bool)
    deg = np.maximum(known.sum(1), 1)
    for _ in range(steps):
        diff = x[:, None] - x[None]
        r = np.sqrt((diff * diff).sum(-1))
        coef = np.where(known, r - d, np.where(off & ~known & (r < DMAX), r - DMAX, 0.0))
        x = x - 0.5 * ((coef / np.maximum(r, 1e-6))[:, :, None] * diff).sum(1) / deg[:, None]
    r = np.linalg.norm(x[:, None] - x[None], axis=-1)
    rms = float(np.sqrt(((r - d)[known] ** 2).mean())) if known.any() else 0.0
    return x, rms


def frames(cb, nb, theta, phi):
    """N / CA / C about given Cb positions; returns (xyz (n, 3, 3), bad (n,) bool)."""
    n = cb.shape[0]
    xyz, bad = np.zeros((n, 3, 3)), np.zeros(n, bool)
    for i in range(n):
        js = np.nonzero(nb[i])[0]
        if len(js) < 3:
            bad[i] = True
            continue
        e = cb[js] - cb[i]
        e = e / np.maximum(np.linalg.norm(e, axis=1), 1e-6)[:, None]
        a_mat = e.T @ e
        if np.linalg.det(a_mat) < 1e-4 * (np.trace(a_mat) / 3.0) ** 3:
            bad[i] = True
            continue
        u = np.linalg.solve(a_mat, e.T @ np.cos(phi[i, js]))
        if np.linalg.norm(u) < 1e-3:
            bad[i] = True
            continue
        u = u / np.linalg.norm(u)
        ax = -u                                                            # CA -> Cb
        ca = cb[i] + R_CB * u
        w = e - (e @ ax)[:, None] * ax
        wn = np.linalg.norm(w, axis=1)
        ok = wn >= 1e-3
        w = w[ok] / wn[ok][:, None]
        th = theta[i, js][ok]
        v = (w * np.cos(th)[:, None] - np.cross(ax, w) * np.sin(th)[:, None]).sum(0)
        if np.linalg.norm(v) < 1e-3:
            bad[i] = True
            continue
        p = v / np.linalg.norm(v)
        nn = ca + N_CA * (np.cos(A_NCACB) * ax + np.sin(A_NCACB) * p)
        b = ca - nn
        bx = np.array([[0, -b[2], b[1]], [b[2], 0, -b[0]], [-b[1], b[0], 0]])
        c = np.linalg.solve(K3 * np.eye(3) + K1 * bx, (cb[i] - ca) - K2 * b)
        xyz[i] = nn, ca, ca + c
    place_bad(xyz, cb, bad)
    return xyz, bad


def place_bad(xyz, cb, bad):
    """A residue without a frame takes the offsets (atom - Cb) of the nearest framed residue before it, else after it, else fixed ones."""
    n = cb.shape[0]
    good = np.nonzero(~bad)[0]
    for i in np.nonzero(bad)[0]:
        before, after = good[good < i], good[good > i]
        if before.size:
            k = before[-1]
        elif after.size:
            k = after[0]
        else:
            xyz[i] = cb[i] + np.array([[-1.2, -0.9, 0.0], [0.0, -R_CB, 0.0], [1.25, -0.9, 0.0]])
            continue
        xyz[i] = cb[i] + (xyz[k] - cb[k])


def closure(xyz):
    if xyz.shape[0] < 2:
        return 0.0
    return float(np.abs(np.linalg.norm(xyz[:-1, 2] - xyz[1:, 0], axis=1) - C_N).mean())


def virtual_cb(xyz):
    return GO.virtual_cb(xyz[:, 0], xyz[:, 1], xyz[:, 2])


def restraint_sets(maps):
    """The index sets of load_constraints (rosetta_min/utils.py:119-206): (dist, omega) over i < j, (theta, phi) over ordered pairs."""
    dist, omega = np.asarray(maps["dist"]), np.asarray(maps["omega"])
    n = dist.shape[0]
    near = dist <= NEIGHBOUR                                               # not in filter_idx (dist > 12)
    up = np.triu(np.ones((n, n), bool), 1)
    off = ~np.eye(n, dtype=bool)
    return up & (dist > 0) & near, up & (omega != 0) & near, off & near


def restraint_score(xyz, maps, dist_std=2.0, angle_std=10.0, dtype=np.float64):
    """The four harmonic sums and their counts for a backbone (n, 3, 3): ((dist, omega, theta, phi), (counts))."""
    x = np.asarray(xyz, dtype)
    m = {k: np.asarray(maps[k], dtype) for k in ("dist", "omega", "theta", "phi")}
    sd, so, sa = restraint_sets(m)
    cb, ca, nn = virtual_cb(x).astype(dtype), x[:, 1], x[:, 0]
    astd = dtype(np.deg2rad(angle_std))
    out = []
    i, j = np.nonzero(sd)
    out.append((((np.linalg.norm(cb[i] - cb[j], axis=-1) - m["dist"][i, j]) / dtype(dist_std)) ** 2).sum(dtype=dtype))
    i, j = np.nonzero(so)
    out.append(((GO.wrap(GO.dihedral_projection(ca[i], cb[i], cb[j], ca[j]) - m["omega"][i, j], dtype) / astd) ** 2).sum(dtype=dtype))
    i, j = np.nonzero(sa)
    out.append(((GO.wrap(GO.dihedral_projection(nn[i], ca[i], cb[i], cb[j]) - m["theta"][i, j], dtype) / astd) ** 2).sum(dtype=dtype))
    out.append((((GO.angle(ca[i], cb[i], cb[j]) - m["phi"][i, j]) / astd) ** 2).sum(dtype=dtype))
    return np.array([float(v) for v in out]), np.array([int(sd.sum()), int(so.sum()), int(sa.sum()), int(sa.sum())])


def fold(maps, known_below=19.0, stress_steps=300, dist_std=2.0, angle_std=10.0):
    dist = np.asarray(maps["dist"], np.float64)
    theta, phi = np.asarray(maps["theta"], np.float64), np.asarray(maps["phi"], np.float64)
    d, known, nb = pairs(dist, known_below)
    g, unreachable = geodesics(d, known)
    x0, eig, axis_corr = classical_mds(g)
    cb, rms = stress_refine(x0, d, known, stress_steps)
    hands = []
    for h in (0, 1):
        c = cb * np.array([1.0, 1.0, -1.0 if h else 1.0])
        xyz, bad = frames(c, nb, theta, phi)
        hands.append((xyz, bad, closure(xyz)))
    hand = 0 if hands[0][2] <= hands[1][2] else 1
    xyz, bad, _ = hands[hand]
    score, counts = restraint_score(xyz, maps, dist_std, angle_std)
    return dict(xyz=xyz, cb=cb, hand=hand, closure=(hands[0][2], hands[1][2]), stress_rms=rms, status=int(unreachable > 0 or bad.any()),
                placed=np.nonzero(bad)[0].tolist(), unreachable=unreachable, score=score, counts=counts, eig=eig, axis_corr=axis_corr,
                known_fraction=float(known.sum()) / max(known.size - known.shape[0], 1))


def kabsch_rmsd(p, q):
    """RMSD of p onto q after the best proper rotation (no reflection) and translation."""
    p, q = np.asarray(p, np.float64), np.asarray(q, np.float64)
    p, q = p - p.mean(0), q - q.mean(0)
    u, s, vt = np.linalg.svd(p.T @ q)
    sign = np.sign(np.linalg.det(u @ vt))
    s[-1] *= sign
    e = (p * p).sum() + (q * q).sum() - 2.0 * s.sum()
    return float(np.sqrt(max(e, 0.0) / p.shape[0]))
