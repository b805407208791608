"""Float64 numpy restatement of the secondary-structure annotation t2p_op_annotate_sse computes (include/t2p.h): P-SEA
(Labesse et al. 1997) with its published thresholds, on a CA trace.  Written from the specification, one residue at a time, so that
every rule can be read off; the GPU test demands the kernel's letters, counts and status equal these exactly.

Quantities of residue i, from the CA positions p (indices inside [0, n), every residue named must have a CA, else the quantity is
undefined -- NaN here -- and every test on it is false):
    d2 = |p[i-1] - p[i+1]|     d3 = |p[i-1] - p[i+2]|     d4 = |p[i-1] - p[i+3]|
    r  = angle at p[i] between p[i-1] and p[i+1], degrees
    a  = dihedral of p[i-1], p[i], p[i+1], p[i+2], degrees in (-180, 180]; a right-handed alpha helix gives about +50
d2, d3 and d4 of residue i do not name p[i]: they stay defined when residue i itself has no CA.  Such a residue may so lie inside a
run; its own letter is 'c' whatever the run says.

``annotate`` also returns ``margin``: the smallest distance of any defined quantity from any of ITS thresholds (A or degrees), the
contact distances |p[i] - p[j]|, i != j, against 4.2 and 5.2 included.  A fixture whose margin is well above what rounding can move a
quantity has no label on an edge.
"""
import numpy as np

D3_HELIX, D4_HELIX, R_HELIX, A_HELIX = (4.8, 5.8), (5.8, 7.0), (77.0, 101.0), (30.0, 70.0)
D2_STRAND, D3_STRAND, D4_STRAND, R_STRAND = (6.1, 7.3), (9.0, 10.8), (11.3, 13.5), (110.0, 138.0)
A_STRAND = ((-180.0, -125.0), (145.0, 180.0))
CONTACT = (4.2, 5.2)
MIN_CORE, SHORT_CORE, MIN_CONTACTS = 5, 3, 5
MAX_COORD = 1e6
THRESHOLDS = {"d2": D2_STRAND, "d3": D3_HELIX + D3_STRAND, "d4": D4_HELIX + D4_STRAND, "r": R_HELIX + R_STRAND,
              "a": A_HELIX + A_STRAND[0] + A_STRAND[1]}


def _in(v, lo_hi):
    return bool(v >= lo_hi[0]) and bool(v <= lo_hi[1])          # False for NaN


def quantities(p, has):
    """(n, 5) float64: d2, d3, d4, r, a per residue; NaN where undefined."""
    n = p.shape[0]
    q = np.full((n, 5), np.nan)

    def ok(*idx):
        return all(0 <= k < n and has[k] for k in idx)

    with np.errstate(invalid="ignore", divide="ignore"):
        for i in range(n):
            for col, off in ((0, 1), (1, 2), (2, 3)):
                if ok(i - 1, i + off):
                    q[i, col] = np.sqrt(((p[i - 1] - p[i + off]) ** 2).sum())
            if ok(i - 1, i, i + 1):
                u, v = p[i - 1] - p[i], p[i + 1] - p[i]
                c = (u * v).sum() / (np.sqrt((u * u).sum()) * np.sqrt((v * v).sum()))
                q[i, 3] = np.degrees(np.arccos(min(1.0, max(-1.0, c)))) if c == c else np.nan
            if ok(i - 1, i, i + 1, i + 2):
                b0, b1, b2 = p[i] - p[i - 1], p[i + 1] - p[i], p[i + 2] - p[i + 1]
                n1, n2 = np.cross(b0, b1), np.cross(b1, b2)
                q[i, 4] = np.degrees(np.arctan2((np.cross(n1, n2) * b1).sum() / np.sqrt((b1 * b1).sum()), (n1 * n2).sum()))
    return q


def runs(flags):
    """Maximal runs of true entries: [(start, last), ...]."""
    out, start = [], None
    for i, f in enumerate(list(flags) + [False]):
        if f and start is None:
            start = i
        elif not f and start is not None:
            out.append((start, i - 1))
            start = None
    return out


def annotate(xyz, atom_ok=None, target=None):
    """``xyz``: (n, 3) CA trace or (n, 3, 3) N / CA / C (atom 1 is read), any float dtype, taken to float64; ``atom_ok``: (n,) or
    (n, atoms) presence flags or None; ``target``: n letters or None.  Returns a dict: ``letters`` (str), ``counts`` (12 ints, the order
    of include/t2p.h), ``status`` (0, or 1 when a present CA was not finite or beyond 1e6 and so counted as absent), ``margin``,
    ``q`` (the quantities), ``potential_helix`` / ``potential_strand`` (bool arrays) and ``contacts`` (per residue)."""
    x = np.asarray(xyz, dtype=np.float64)
    p = x[:, 1] if x.ndim == 3 else x
    n = p.shape[0]
    has = np.ones(n, bool)
    if atom_ok is not None:
        k = np.asarray(atom_ok)
        has = (k[:, 1] if k.ndim == 2 and k.shape[1] == 3 else k.reshape(n)) != 0
    with np.errstate(invalid="ignore"):
        bad = has & ~(np.abs(p) <= MAX_COORD).all(axis=1)
    status = int(bad.any())
    has = has & ~bad
    p = np.where(has[:, None], p, 0.0)
    q = quantities(p, has)
    d2, d3, d4, r, a = q.T
    ph = np.array([(_in(d3[i], D3_HELIX) and _in(d4[i], D4_HELIX)) or (_in(r[i], R_HELIX) and _in(a[i], A_HELIX)) for i in range(n)], bool)
    ps = np.array([(_in(d2[i], D2_STRAND) and _in(d3[i], D3_STRAND) and _in(d4[i], D4_STRAND))
                   or (_in(r[i], R_STRAND) and (_in(a[i], A_STRAND[0]) or _in(a[i], A_STRAND[1]))) for i in range(n)], bool)
    dist = np.sqrt(((p[:, None] - p[None]) ** 2).sum(-1))
    pair = has[:, None] & has[None] & ~np.eye(n, dtype=bool)
    contacts = (pair & (dist >= CONTACT[0]) & (dist <= CONTACT[1])).sum(1)

    helix, strand = np.zeros(n, bool), np.zeros(n, bool)
    for s, e in runs(ph):
        if e - s + 1 >= MIN_CORE:
            helix[s:e + 1] = True
            for k in (s - 1, e + 1):                    # one residue per end, judged against the cores: no cascade
                if 0 <= k < n and (_in(d3[k], D3_HELIX) or _in(r[k], R_HELIX)):
                    helix[k] = True
    for s, e in runs(ps):
        m = e - s + 1
        if m >= MIN_CORE or (m >= SHORT_CORE and int(contacts[s:e + 1].sum()) >= MIN_CONTACTS):
            strand[s:e + 1] = True
            for k in (s - 1, e + 1):
                if 0 <= k < n and _in(d3[k], D3_STRAND):
                    strand[k] = True
    lt = np.full(n, "c")
    lt[helix] = "a"
    lt[strand] = "b"                                    # the strand wins an overlap
    lt[~has] = "c"
    letters = "".join(lt)

    counts = [letters.count("a"), letters.count("b"), letters.count("c"),
              sum(e - s + 1 >= 4 for s, e in runs(lt == "a")), sum(e - s + 1 >= 4 for s, e in runs(lt == "b")), 0, 0, 0, 0, int((~has).sum()), 0, 0]
    if target is not None:
        t = np.array(list(target)) if isinstance(target, str) else np.asarray(target)
        if t.dtype.kind in "iu":
            t = np.array([chr(v) for v in t])
        assert t.shape == (n,)
        counts[5:9] = [int((t == "a").sum()), int(((t == "a") & (lt == "a")).sum()), int((t == "b").sum()), int(((t == "b") & (lt == "b")).sum())]

    margin = np.inf
    for col, name in enumerate(("d2", "d3", "d4", "r", "a")):
        v = q[:, col][~np.isnan(q[:, col])]
        for th in THRESHOLDS[name]:
            if v.size:
                margin = min(margin, float(np.abs(v - th).min()))
    if pair.any():
        margin = min(margin, min(float(np.abs(dist[pair] - th).min()) for th in CONTACT))
    return {"letters": letters, "counts": counts, "status": status, "margin": margin, "q": q, "potential_helix": ph, "potential_strand": ps,
            "contacts": contacts, "has": has}
