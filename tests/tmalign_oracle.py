"""Float64 numpy restatement of TM-align's default path (the reference's ``tm/TMalign.cpp``), test infrastructure only.

``tm_align(x, y)`` takes two CA traces, (n, 3) each: ``x`` is Chain_1 (superimposed), ``y`` is Chain_2.  It follows
``TMalign_main`` (TMalign.cpp:3923): ``parameter_set4search``, the five seeds -- ``get_initial`` (gapless threading), ``get_initial_ss``
(DP on ``make_sec`` strings), ``get_initial5`` (local superposition + DP), ``get_initial_ssplus`` and ``get_initial_fgt`` (fragment
threading after ``find_max_frag``) -- each followed by ``detailed_search`` and ``DP_iter``; then ``detailed_search_standard`` at
``simplify_step = 1``, the ``d <= score_d8`` cut and the two final ``TMscore8_search`` calls under ``parameter_set4final``.

The Kabsch fit is the reference's closed-form cubic (TMalign.cpp:983) statement by statement, so that a degenerate fit takes the same
branch; sums run in numpy's order, not the reference's, which moves a score by some 1e-14.  Tie rules are the reference's: the
threading loops keep the last maximum, ``get_initial5`` and ``TMscore8_search`` the first, ``NWDP_TM`` prefers the diagonal on
``d >= h and d >= v`` and its traceback ``j--`` on ``v >= h``.  The DP runs over anti-diagonals, which changes no cell.

``seeds`` switches seeds off (tests pin that seeds 3 to 5 matter).  Python loops: 0.1 s to tens of seconds per pair.
"""
import math

import numpy as np

SEEDS = ("gl", "ss", "i5", "ssp", "fgt")


def kabsch(x, y, mode=1):
    """TMalign.cpp:983.  x, y (n, 3).  Returns rms (mode 0 / 2 only, else 0), t (3,), u (3, 3)."""
    n = len(x)
    t = [0.0, 0.0, 0.0]
    u = [[1.0, 0.0, 0.0], [0.0, 1.0, 0.0], [0.0, 0.0, 1.0]]
    a = [[1.0, 0.0, 0.0], [0.0, 1.0, 0.0], [0.0, 0.0, 1.0]]
    b = [[0.0] * 3 for _ in range(3)]
    if n < 1:
        return 0.0, np.array(t), np.array(u)
    x = np.asarray(x, np.float64)
    y = np.asarray(y, np.float64)
    s1 = x.sum(0).tolist()
    s2 = y.sum(0).tolist()
    sxyz = (x.T @ y).tolist()                                   # sx = sxyz[0], sy = sxyz[1], sz = sxyz[2]
    xc = [v / n for v in s1]
    yc = [v / n for v in s2]
    e0 = 0.0
    if mode in (0, 2):
        e0 = float(((x - np.array(xc)) ** 2).sum() + ((y - np.array(yc)) ** 2).sum())
    r = [[sxyz[c][j] - s1[c] * s2[j] / n for c in range(3)] for j in range(3)]
    det = (r[0][0] * (r[1][1] * r[2][2] - r[1][2] * r[2][1]) - r[0][1] * (r[1][0] * r[2][2] - r[1][2] * r[2][0])
           + r[0][2] * (r[1][0] * r[2][1] - r[1][1] * r[2][0]))
    sigma = det
    rr = []
    for j in range(3):
        for i in range(j + 1):
            rr.append(r[0][i] * r[0][j] + r[1][i] * r[1][j] + r[2][i] * r[2][j])
    spur = (rr[0] + rr[2] + rr[5]) / 3.0
    cof = (((((rr[2] * rr[5] - rr[4] * rr[4]) + rr[0] * rr[5]) - rr[3] * rr[3]) + rr[0] * rr[2]) - rr[1] * rr[1]) / 3.0
    det = det * det
    e = [spur, spur, spur]
    eps, tol, sqrt3 = 0.00000001, 0.01, 1.73205080756888
    ip = (0, 1, 3, 1, 2, 4, 3, 4, 5)
    ip2312 = (1, 2, 0, 1)
    a_failed = b_failed = False
    if spur > 0:
        d = spur * spur
        h = d - cof
        g = (spur * cof - det) / 2.0 - spur * h
        if h > 0:
            sqrth = math.sqrt(h)
            d = h * h * h - g * g
            if d < 0.0:
                d = 0.0
            d = math.atan2(math.sqrt(d), -g) / 3.0
            cth = sqrth * math.cos(d)
            sth = sqrth * sqrt3 * math.sin(d)
            e = [(spur + cth) + cth, (spur - cth) + sth, (spur - cth) - sth]
            if mode != 0:
                j = 0
                for l in (0, 2):
                    d = e[l]
                    ss = [(d - rr[2]) * (d - rr[5]) - rr[4] * rr[4], (d - rr[5]) * rr[1] + rr[3] * rr[4],
                          (d - rr[0]) * (d - rr[5]) - rr[3] * rr[3], (d - rr[2]) * rr[3] + rr[1] * rr[4],
                          (d - rr[0]) * rr[4] + rr[1] * rr[3], (d - rr[0]) * (d - rr[2]) - rr[1] * rr[1]]
                    ss = [0.0 if abs(v) <= eps else v for v in ss]
                    if abs(ss[0]) >= abs(ss[2]):
                        j = 2 if abs(ss[0]) < abs(ss[5]) else 0
                    elif abs(ss[2]) >= abs(ss[5]):
                        j = 1
                    else:
                        j = 2
                    d = 0.0
                    j = 3 * j
                    for i in range(3):
                        k = ip[i + j]
                        a[i][l] = ss[k]
                        d = d + ss[k] * ss[k]
                    d = 1.0 / math.sqrt(d) if d > eps else 0.0
                    for i in range(3):
                        a[i][l] = a[i][l] * d
                d = a[0][0] * a[0][2] + a[1][0] * a[1][2] + a[2][0] * a[2][2]
                m1, m = (2, 0) if (e[0] - e[1]) > (e[1] - e[2]) else (0, 2)
                p = 0.0
                for i in range(3):
                    a[i][m1] = a[i][m1] - d * a[i][m]
                    p = p + a[i][m1] * a[i][m1]
                if p <= tol:
                    p = 1.0
                    for i in range(3):
                        if p < abs(a[i][m]):
                            continue
                        p = abs(a[i][m])
                        j = i
                    k, l = ip2312[j], ip2312[j + 1]
                    p = math.sqrt(a[k][m] * a[k][m] + a[l][m] * a[l][m])
                    if p > tol:
                        a[j][m1] = 0.0
                        a[k][m1] = -a[l][m] / p
                        a[l][m1] = a[k][m] / p
                    else:
                        a_failed = True
                else:
                    p = 1.0 / math.sqrt(p)
                    for i in range(3):
                        a[i][m1] = a[i][m1] * p
                if not a_failed:
                    a[0][1] = a[1][2] * a[2][0] - a[1][0] * a[2][2]
                    a[1][1] = a[2][2] * a[0][0] - a[2][0] * a[0][2]
                    a[2][1] = a[0][2] * a[1][0] - a[0][0] * a[1][2]
        if mode != 0 and not a_failed:
            for l in range(2):
                d = 0.0
                for i in range(3):
                    b[i][l] = r[i][0] * a[0][l] + r[i][1] * a[1][l] + r[i][2] * a[2][l]
                    d = d + b[i][l] * b[i][l]
                d = 1.0 / math.sqrt(d) if d > eps else 0.0
                for i in range(3):
                    b[i][l] = b[i][l] * d
            d = b[0][0] * b[0][1] + b[1][0] * b[1][1] + b[2][0] * b[2][1]
            p = 0.0
            for i in range(3):
                b[i][1] = b[i][1] - d * b[i][0]
                p += b[i][1] * b[i][1]
            if p <= tol:
                p = 1.0
                j = 0
                for i in range(3):
                    if p < abs(b[i][0]):
                        continue
                    p = abs(b[i][0])
                    j = i
                k, l = ip2312[j], ip2312[j + 1]
                p = math.sqrt(b[k][0] * b[k][0] + b[l][0] * b[l][0])
                if p > tol:
                    b[j][1] = 0.0
                    b[k][1] = -b[l][0] / p
                    b[l][1] = b[k][0] / p
                else:
                    b_failed = True
            else:
                p = 1.0 / math.sqrt(p)
                for i in range(3):
                    b[i][1] = b[i][1] * p
            if not b_failed:
                b[0][2] = b[1][0] * b[2][1] - b[1][1] * b[2][0]
                b[1][2] = b[2][0] * b[0][1] - b[2][1] * b[0][0]
                b[2][2] = b[0][0] * b[1][1] - b[0][1] * b[1][0]
                for i in range(3):
                    for j in range(3):
                        u[i][j] = b[i][0] * a[j][0] + b[i][1] * a[j][1] + b[i][2] * a[j][2]
            for i in range(3):
                t[i] = ((yc[i] - u[i][0] * xc[0]) - u[i][1] * xc[1]) - u[i][2] * xc[2]
    else:
        for i in range(3):
            t[i] = ((yc[i] - u[i][0] * xc[0]) - u[i][1] * xc[1]) - u[i][2] * xc[2]
    e = [math.sqrt(max(v, 0.0)) for v in e]
    d = e[2]
    if sigma < 0.0:
        d = -d
    d = (d + e[1]) + e[0]
    rms = 0.0
    if mode in (0, 2):
        rms = max((e0 - d) - d, 0.0)
    return rms, np.array(t), np.array(u)


def rotate(x, t, u):
    return x @ u.T + t


def dist2(a, b):
    return ((a - b) ** 2).sum(-1)


def score_fun8(xt, y, d, method8, norm, d8, d0):
    """TMalign.cpp:1719 / 1762: the selected set (bool mask) and the score."""
    di = dist2(xt, y)
    n = len(di)
    inc = 0
    dt = d * d
    while True:
        sel = di < dt
        if sel.sum() < 3 and n > 3:
            inc += 1
            dt = (d + inc * 0.5) ** 2
        else:
            break
    s = 1.0 / (1.0 + di / (d0 * d0))
    if method8:
        s = s[di <= d8 * d8]
    return sel, float(s.sum()) / norm


def tmscore8_search(x, y, step, method8, d0s, norm, d8, d0):
    """TMalign.cpp:1807 (and 1962, whose score is normalised by the pair count: pass ``norm=None``).  x, y: the aligned pairs."""
    n = len(x)
    if norm is None:
        norm = n
    lmin = min(4, n)
    frags = []
    for i in range(5):
        L = int(n / 2.0 ** i)
        if L <= lmin:
            frags.append(lmin)
            break
        frags.append(L)
    else:
        frags.append(lmin)
    best, bt, bu = -1.0, np.zeros(3), np.eye(3)
    for L in frags:
        imax, i = n - L, 0
        while True:
            _, t, u = kabsch(x[i:i + L], y[i:i + L])
            sel, s = score_fun8(rotate(x, t, u), y, d0s - 1, method8, norm, d8, d0) if n else (np.zeros(0, bool), 0.0)
            if s > best:
                best, bt, bu = s, t, u
            for _ in range(20):
                ka = sel
                _, t, u = kabsch(x[sel], y[sel])
                sel, s = score_fun8(rotate(x, t, u), y, d0s + 1, method8, norm, d8, d0) if n else (sel, 0.0)
                if s > best:
                    best, bt, bu = s, t, u
                if np.array_equal(sel, ka):
                    break
            if i < imax:
                i = min(i + step, imax)
            else:
                break
    return best, bt, bu


def nwdp(score, gap):
    """TMalign.cpp:1321 on score (n, m); cells of one anti-diagonal are independent.  Returns j2i (m,)."""
    n, m = score.shape
    val = np.zeros((n + 1, m + 1))
    path = np.zeros((n + 1, m + 1), bool)
    direc = np.zeros((n + 1, m + 1), bool)
    for s in range(2, n + m + 1):
        i = np.arange(max(1, s - m), min(n, s - 1) + 1)
        j = s - i
        d = val[i - 1, j - 1] + score[i - 1, j - 1]
        h = val[i - 1, j] + np.where(path[i - 1, j], gap, 0.0)
        v = val[i, j - 1] + np.where(path[i, j - 1], gap, 0.0)
        dg = (d >= h) & (d >= v)
        path[i, j] = dg
        direc[i, j] = v >= h
        val[i, j] = np.where(dg, d, np.where(v >= h, v, h))
    inv = -np.ones(m, np.int64)
    i, j = n, m
    while i > 0 and j > 0:
        if path[i, j]:
            inv[j - 1] = i - 1
            i -= 1
            j -= 1
        elif direc[i, j]:
            j -= 1
        else:
            i -= 1
    return inv


def pairs(x, y, inv):
    j = np.nonzero(inv >= 0)[0]
    return x[inv[j]], y[j]


def make_sec(x):
    """TMalign.cpp:2436-2491: 1 coil, 2 helix, 3 turn, 4 strand."""
    n = len(x)
    s = np.ones(n, np.int64)
    D = lambda a, b: math.sqrt(float(dist2(x[a], x[b])))           # noqa: E731
    for i in range(2, n - 2):
        d13, d14, d15, d24, d25, d35 = D(i - 2, i), D(i - 2, i + 1), D(i - 2, i + 2), D(i - 1, i + 1), D(i - 1, i + 2), D(i, i + 2)
        if all(abs(a - b) < 2.1 for a, b in ((d15, 6.37), (d14, 5.18), (d25, 5.18), (d13, 5.45), (d24, 5.45), (d35, 5.45))):
            s[i] = 2
        elif all(abs(a - b) < 1.42 for a, b in ((d15, 13.0), (d14, 10.4), (d25, 10.4), (d13, 6.1), (d24, 6.1), (d35, 6.1))):
            s[i] = 4
        elif d15 < 8:
            s[i] = 3
    return s


def get_score_fast(x, y, inv, d0, d0s):
    """TMalign.cpp:2194."""
    a, b = pairs(x, y, inv)
    n = len(a)
    _, t, u = kabsch(a, b)
    di = dist2(rotate(a, t, u), b)
    tm = float((1.0 / (1.0 + di / (d0 * d0))).sum())
    d2 = d0s * d0s
    while True:
        sel = di <= d2
        if sel.sum() < 3 and n > 3:
            d2 += 0.5
        else:
            break
    if sel.sum() == n:
        return tm
    _, t, u = kabsch(a[sel], b[sel])
    di = dist2(rotate(a, t, u), b)
    tm1 = float((1.0 / (1.0 + di / (d0 * d0))).sum())
    d2 = d0s * d0s + 1
    while True:
        sel = di <= d2
        if sel.sum() < 3 and n > 3:
            d2 += 0.5
        else:
            break
    _, t, u = kabsch(a[sel], b[sel])
    di = dist2(rotate(a, t, u), b)
    tm2 = float((1.0 / (1.0 + di / (d0 * d0))).sum())
    return max(tm, tm1, tm2)


def find_max_frag(x, dcu0=4.25):
    """TMalign.cpp:2678: the longest run without a CA-CA step of dcu0 or more (start, end inclusive)."""
    n = len(x)
    r_min = min(int(n / 3.0), 4)
    step = dist2(x[1:], x[:-1])
    inc, cut = 0, dcu0 * dcu0
    lmax, smax, emax = 0, 0, 0
    while lmax < r_min:
        lmax, j, start = 0, 1, 0
        for i in range(1, n):
            if step[i - 1] < cut:
                j += 1
                if i == n - 1:
                    if j > lmax:
                        lmax, smax, emax = j, start, i
                    j = 1
            else:
                if j > lmax:
                    lmax, smax, emax = j, start, i - 1
                j = 1
                start = i
        if lmax < r_min:
            inc += 1
            cut = (1.1 ** inc * dcu0) ** 2
    return smax, emax


def _thread_x(x, y, ifr, d0, d0s, best):
    xl, yl, L1 = len(x), len(y), len(ifr)
    ma = max(3, int(min(L1, yl) / 2.5))
    j = np.arange(yl)
    for k in range(-yl + ma, L1 - ma + 1):
        i = j + k
        ok = (i >= 0) & (i < L1)
        inv = np.where(ok, ifr[np.clip(i, 0, L1 - 1)], -1)
        s = get_score_fast(x, y, inv, d0, d0s)
        if s >= best[0]:
            best = (s, inv)
    return best


def _thread_y(x, y, ifr, d0, d0s, best):
    xl, yl, L2 = len(x), len(y), len(ifr)
    ma = max(3, int(min(xl, L2) / 2.5))
    j = np.arange(L2)
    for k in range(-L2 + ma, xl - ma + 1):
        inv = -np.ones(yl, np.int64)
        i = j + k
        ok = (i >= 0) & (i < xl)
        inv[ifr[ok]] = i[ok]
        s = get_score_fast(x, y, inv, d0, d0s)
        if s >= best[0]:
            best = (s, inv)
    return best


def _trim(ifr, L0):
    if len(ifr) == L0:
        return ifr[int(L0 * 0.1):int(L0 * 0.89) + 1]
    return ifr


def get_initial_fgt(x, y, d0, d0s):
    """TMalign.cpp:2744."""
    xl, yl = len(x), len(y)
    xs, xe = find_max_frag(x)
    ys, ye = find_max_frag(y)
    Lx, Ly = xe - xs + 1, ye - ys + 1
    Lfr = min(Lx, Ly)
    fx, fy = xs + np.arange(Lfr), ys + np.arange(Lfr)
    best = (-1.0, None)
    if Lx < Ly or (Lx == Ly and xl < yl):
        return _thread_x(x, y, _trim(fx, min(xl, yl)), d0, d0s, best)[1]
    if Lx > Ly or (Lx == Ly and xl > yl):
        return _thread_y(x, y, _trim(fy, min(xl, yl)), d0, d0s, best)[1]
    best = _thread_x(x, y, _trim(fx, xl), d0, d0s, best)
    return _thread_y(x, y, _trim(fy, xl), d0, d0s, best)[1]


def d0_final(L):
    """parameter_set4final (TMalign.cpp:1687): d0 and d0_search."""
    d0 = 0.5 if L <= 21 else 1.24 * (L - 15.0) ** (1.0 / 3) - 1.8
    d0 = max(d0, 0.5)
    return d0, min(8.0, max(4.5, d0))


def tm_align(x, y, seeds=SEEDS):
    """Returns a dict: tm_a, tm_b (normalised by len(x), len(y)), rmsd, n_ali8, d0_a, d0_b, tm_max, seed (index into SEEDS of the seed
    that produced the final alignment), b2a (len(y),) and t (3,), u (3, 3) of the superposition of x onto y for tm_b."""
    x = np.asarray(x, np.float64)
    y = np.asarray(y, np.float64)
    xl, yl = len(x), len(y)
    Ln = min(xl, yl)
    d0 = (0.168 if Ln <= 19 else 1.24 * (Ln - 15.0) ** (1.0 / 3) - 1.8) + 0.8
    D0_MIN = d0
    d0s = min(8.0, max(4.5, d0))
    d8 = 1.5 * Ln ** 0.3 + 3.5
    ddcc = 0.1 if Ln <= 40 else 0.4

    def detailed(inv):
        a, b = pairs(x, y, inv)
        return tmscore8_search(a, b, 40, True, d0s, Ln, d8, d0)

    def dp_iter(t, u, g1, g2, itmax):
        best, binv, old = -1.0, None, 0.0
        for gap in (-0.6, 0.0)[g1:g2]:
            for it in range(itmax):
                xt = rotate(x, t, u)
                S = 1.0 / (1.0 + dist2(xt[:, None], y[None]) / (d0 * d0))
                inv = nwdp(S, gap)
                a, b = pairs(x, y, inv)
                tm, t, u = tmscore8_search(a, b, 40, True, d0s, Ln, d8, d0)
                if tm > best:
                    best, binv = tm, inv
                if it > 0 and abs(old - tm) < 0.000001:
                    break
                old = tm
        return best, binv

    sx, sy = make_sec(x), make_sec(y)
    eq = (sx[:, None] == sy[None])
    TMmax, inv0, seed0 = -1.0, -np.ones(yl, np.int64), 0
    for si, sd in enumerate(SEEDS):
        if sd not in seeds:
            continue
        if sd == "gl":
            ma = max(5, Ln // 2)
            bs, inv = -1.0, None
            j = np.arange(yl)
            for k in range(-yl + ma, xl - ma + 1):
                i = j + k
                cand = np.where((i >= 0) & (i < xl), i, -1)
                s = get_score_fast(x, y, cand, d0, d0s)
                if s >= bs:
                    bs, inv = s, cand
        elif sd == "ss":
            inv = nwdp(eq.astype(np.float64), -1.0)
        elif sd == "i5":
            d01 = max(d0 + 1.5, D0_MIN)
            jump = lambda n: min(45 if n > 250 else 35 if n > 200 else 25 if n > 150 else 15, n // 3)        # noqa: E731
            j1, j2 = jump(xl), jump(yl)
            glmax, inv = 0.0, None
            for nf in (min(20, Ln // 3), min(100, Ln // 2)):
                for i in range(0, xl - nf + 1, j1):
                    for j in range(0, yl - nf + 1, j2):
                        _, t, u = kabsch(x[i:i + nf], y[j:j + nf])
                        S = 1.0 / (1.0 + dist2(rotate(x, t, u)[:, None], y[None]) / (d01 * d01))
                        cand = nwdp(S, 0.0)
                        gl = get_score_fast(x, y, cand, d0, d0s)
                        if gl > glmax:
                            glmax, inv = gl, cand
            if inv is None:
                continue
        elif sd == "ssp":
            d01 = max(d0 + 1.5, D0_MIN)
            a, b = pairs(x, y, inv0)
            _, t, u = kabsch(a, b)
            S = 1.0 / (1.0 + dist2(rotate(x, t, u)[:, None], y[None]) / (d01 * d01)) + np.where(eq, 0.5, 0.0)
            inv = nwdp(S, -1.0)
        else:
            inv = get_initial_fgt(x, y, d0, d0s)
        tm, t, u = detailed(inv)
        if tm > TMmax:
            TMmax, inv0, seed0 = tm, inv, si
        if sd == "gl" or tm > TMmax * (0.2 if sd == "ss" else ddcc):
            tm, inv = dp_iter(t, u, 1 if sd == "fgt" else 0, 2, 2 if sd in ("i5", "fgt") else 30)
            if tm > TMmax:
                TMmax, inv0, seed0 = tm, inv, si
    a, b = pairs(x, y, inv0)
    _, t, u = tmscore8_search(a, b, 1, True, d0s, None, d8, d0)
    jj = np.nonzero(inv0 >= 0)[0]
    xt = rotate(x, t, u)
    keep = np.sqrt(dist2(xt[inv0[jj]], y[jj])) <= d8
    jj = jj[keep]
    b2a = -np.ones(yl, np.int64)
    b2a[jj] = inv0[jj]
    n8 = len(jj)
    # rmsd0 (TMalign.cpp:4381) is Kabsch mode 0's e0 - 2 (sum of singular values), which cancels to ~1e-7 A of noise for coinciding
    # chains; the same minimum is taken here as the residual under the optimal rotation (the kernel does the same)
    _, tz, uz = kabsch(xt[inv0[jj]], y[jj])
    rmsd = math.sqrt(float(dist2(rotate(xt[inv0[jj]], tz, uz), y[jj]).sum()) / n8)
    a, b = x[inv0[jj]], y[jj]
    d0b, d0sb = d0_final(yl)
    tm_b, t0, u0 = tmscore8_search(a, b, 1, False, d0sb, yl, d8, d0b)
    d0a, d0sa = d0_final(xl)
    tm_a, _, _ = tmscore8_search(a, b, 1, False, d0sa, xl, d8, d0a)
    return dict(tm_a=tm_a, tm_b=tm_b, rmsd=rmsd, n_ali8=n8, d0_a=d0a, d0_b=d0b, tm_max=TMmax, seed=seed0, b2a=b2a, t=t0, u=u0)
