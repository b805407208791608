"""Golden fixtures of the secondary-structure annotation (t2p_op_annotate_sse, text2protein_amd/encode.py annotate_sse_batch): chains
of our own with the letters the float64 oracle (tests/sse_oracle.py) gives them.  Only data is written: sse_chains.npz.

    python tests/golden/make_golden_sse.py

Two kinds of chain, everything rounded to 3 decimals:
  * N / CA / C backbones built by NeRF from ideal geometry (the constants of make_golden_fold.py) and torsions drawn around the
    helix / strand / PPII / left-handed basins, +- 10 degrees;
  * CA-level traces built from per-residue internal coordinates: the CA - CA bond 3.8 A, the angle r[i] at residue i and the
    dihedral a[i] of residues i-1 .. i+2 -- the very quantities the annotation thresholds, so a run of potential residues can be
    made exactly as long as wanted.  "helix" is r = 91, a = 50; "strand" r = 124, a = -168 (twisted: a flat zigzag has a = +-180
    exactly, on a threshold); "coil" r = 105, a = 100, which no rule accepts.  Every value is jittered by the seed.

The fixtures (``meta["chains"][key]`` records n, letters, counts, blocks = the reference's "start:last" string, margin, seed and
what the chain is there for):
  hlh        N / CA / C, helix - loop - hairpin: both a and b runs
  near, far  a CA-level strand followed by a second, short piece laid alongside it whose potential-strand run is exactly 3 long:
             b through the contact rule (near); the same piece moved 15 A further away: c (far)
  run5, run4 exactly 5 / exactly 4 potential-helix residues in coil: a core / nothing
  ext        a helix core whose neighbour before it is taken in (r in range, not potential itself) and whose neighbour after it is not
  hole       N / CA / C helix with the CA of one residue missing (atom_ok): that residue is c
  n1 .. n4   the first 1 .. 4 residues of `hole`'s chain: all c
  n512       N / CA / C, 512 residues of mixed runs
Seeds are searched until every fixture's ``margin`` (tests/sse_oracle.py: the smallest distance of any defined quantity from any of
its thresholds, contact distances included) is at least 1e-4 A or degrees -- a hundred times what fp32 rounding of the inputs can
move a quantity -- and the chain shows what it is there for (the assertions in ``purpose``).
"""
import json
import math
import os
import re
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
import sse_oracle as S                                                  # noqa: E402  (tests/)

MARGIN = 1e-4
BOND = {"N_CA": 1.458, "CA_C": 1.525, "C_N": 1.329}
ANGLE = {"N_CA_C": 111.0, "CA_C_N": 116.2, "C_N_CA": 121.7}
HELIX, STRAND, PPII, LEFT = (-61.0, -41.0), (-125.0, 130.0), (-72.0, 145.0), (57.0, 39.0)
CA_BOND = 3.8
CA_HELIX, CA_STRAND, CA_COIL = (91.0, 50.0), (124.0, -168.0), (105.0, 100.0)


def place(a, b, c, bond, angle, torsion):
    """NeRF: the point at `bond` from c, `angle` (deg) at c to b, `torsion` (deg) about b-c from a."""
    t, p = math.radians(angle), math.radians(torsion)
    bc = (c - b) / np.linalg.norm(c - b)
    n = np.cross(b - a, bc)
    n = n / np.linalg.norm(n)
    m = np.cross(n, bc)
    d = np.array([-bond * math.cos(t), bond * math.sin(t) * math.cos(p), bond * math.sin(t) * math.sin(p)])
    return c + d[0] * bc + d[1] * m + d[2] * n


def backbone(torsions):
    """(n, 3, 3) N / CA / C from [(phi, psi), ...], omega = 180, ideal geometry."""
    t = math.radians(ANGLE["N_CA_C"])
    first = np.zeros((3, 3))
    first[1] = (BOND["N_CA"], 0.0, 0.0)
    first[2] = first[1] + BOND["CA_C"] * np.array([-math.cos(t), math.sin(t), 0.0])
    out, psi_prev = [first], torsions[0][1]
    for phi, psi in torsions[1:]:
        p = out[-1]
        r = np.zeros((3, 3))
        r[0] = place(p[0], p[1], p[2], BOND["C_N"], ANGLE["CA_C_N"], psi_prev)
        r[1] = place(p[1], p[2], r[0], BOND["N_CA"], ANGLE["C_N_CA"], 180.0)
        r[2] = place(p[2], r[0], r[1], BOND["CA_C"], ANGLE["N_CA_C"], phi)
        out.append(r)
        psi_prev = psi
    return np.round(np.array(out), 3)


def jitter(rng, basin, k, width=10.0):
    return [(basin[0] + rng.uniform(-width, width), basin[1] + rng.uniform(-width, width)) for _ in range(k)]


def ca_trace(kinds, rng, width=3.0):
    """(n, 3) CA trace from per-residue (r, a) pairs: residue j >= 3 is placed with the angle of residue j-1 and the dihedral of
    residue j-2, so r[i] and a[i] of the finished trace are kinds[i] (plus the jitter) wherever they are defined."""
    n = len(kinds)
    r = [k[0] + rng.uniform(-width, width) for k in kinds]
    a = [k[1] + rng.uniform(-width, width) for k in kinds]
    p = [np.zeros(3), np.array([CA_BOND, 0.0, 0.0])]
    t = math.radians(r[1])
    p.append(p[1] + CA_BOND * np.array([-math.cos(t), math.sin(t), 0.0]))
    for j in range(3, n):
        p.append(place(p[j - 3], p[j - 2], p[j - 1], CA_BOND, r[j - 1], a[j - 2]))
    return np.round(np.array(p[:n]), 3)


def blocks(letters):
    """The reference's "start:last" string (dataset.py:131-167): runs of at least 4, the helices first."""
    return ",".join(f"{m.start()}:{m.end() - 1}" for ch in "ab" for m in re.finditer(ch + "{4,}", letters))


# ---- one builder per fixture: seed -> {key: (xyz, atom_ok or None, check)}; check(oracle result) -> None or the reason it fails ----
def build_hlh(rng):
    tors = (jitter(rng, PPII, 3) + jitter(rng, HELIX, 16) + jitter(rng, PPII, 2) + jitter(rng, LEFT, 1) + jitter(rng, PPII, 2)
            + jitter(rng, STRAND, 9) + [(60.0 + rng.uniform(-5, 5), 30.0 + rng.uniform(-5, 5)), (90.0 + rng.uniform(-5, 5), rng.uniform(-5, 5))]
            + jitter(rng, STRAND, 9) + jitter(rng, PPII, 3))

    def check(o):
        c = o["counts"]
        return None if c[3] >= 1 and c[4] >= 2 else f"blocks {c[3]} helix, {c[4]} strand"
    return {"hlh": (backbone(tors), None, check)}


def build_contact(rng):
    long_piece, short_piece = 9, 6
    s = ca_trace([CA_STRAND] * long_piece, rng)
    t0 = ca_trace([CA_STRAND] * short_piece, rng)
    # the short piece runs back along the long one: same frame, reversed, its centre over the long piece's, then pushed sideways
    t0 = t0[::-1] - t0.mean(0) + s[2:8].mean(0)
    axis = (s[-1] - s[0]) / np.linalg.norm(s[-1] - s[0])
    side = np.cross(axis, rng.normal(size=3))
    side /= np.linalg.norm(side)
    shift = side * rng.uniform(4.3, 5.1) + axis * rng.uniform(-1.7, 1.7)
    near = np.round(np.concatenate([s, t0 + shift]), 3)
    far = np.round(np.concatenate([s, t0 + shift + 15.0 * side]), 3)
    run = [long_piece + 1, long_piece + 2, long_piece + 3]

    def check_for(want):
        def check(o):
            ps = o["potential_strand"]
            if [i for i in range(long_piece, long_piece + short_piece) if ps[i]] != run:
                return "the short piece's potential-strand run is not the three residues meant"
            got = o["letters"][run[0]:run[-1] + 1]
            if got != want * 3 or "bbbbb" not in o["letters"][:long_piece]:
                return f"letters {o['letters']}"
            total = int(o["contacts"][run].sum())
            return None if (total >= 5) == (want == "b") else f"{total} contacts"
        return check
    return {"near": (near, None, check_for("b")), "far": (far, None, check_for("c"))}


def build_run(k):
    def build(rng):
        kinds = [CA_COIL] * 6 + [CA_HELIX] * k + [CA_COIL] * 6
        want = "a" if k >= 5 else "c"

        def check(o):
            if np.nonzero(o["potential_helix"])[0].tolist() != list(range(6, 6 + k)) or o["potential_strand"].any():
                return "potential residues " + "".join("h" if f else "." for f in o["potential_helix"])
            return None if o["letters"][6:6 + k] == want * k else f"letters {o['letters']}"
        return {f"run{k}": (ca_trace(kinds, rng), None, check)}
    return build


def build_ext(rng):
    # residue 5: the helix angle with a coil dihedral (taken in by r, not potential itself); residue 12: coil in both
    kinds = [CA_COIL] * 5 + [(CA_HELIX[0], CA_COIL[1])] + [CA_HELIX] * 6 + [CA_COIL] * 6

    def check(o):
        q, ph = o["q"], o["potential_helix"]
        if np.nonzero(ph)[0].tolist() != list(range(6, 12)):
            return "potential residues " + "".join("h" if f else "." for f in ph)
        if not (S._in(q[5, 3], S.R_HELIX) and not S._in(q[5, 1], S.D3_HELIX)):
            return "residue 5 is not taken in by its angle alone"
        if S._in(q[12, 3], S.R_HELIX) or S._in(q[12, 1], S.D3_HELIX):
            return "residue 12 is taken in"
        return None if o["letters"] == "ccccc" + "a" * 7 + "cccccc" else f"letters {o['letters']}"
    return {"ext": (ca_trace(kinds, rng), None, check)}


def build_hole(rng):
    xyz = backbone(jitter(rng, PPII, 3) + jitter(rng, HELIX, 14) + jitter(rng, PPII, 3))
    ok = np.ones((20, 3), np.uint8)
    ok[9, 1] = 0
    whole = S.annotate(xyz)["letters"]

    def check(o):
        lt = o["letters"]
        if whole[5:14] != "a" * 9 or lt[9] != "c" or o["counts"][9] != 1 or lt == whole:
            return f"letters {lt} (whole chain {whole})"
        return None if "a" in lt[:9] or "a" in lt[10:] else f"no helix left: {lt}"
    out = {"hole": (xyz, ok, check)}
    for k in (1, 2, 3, 4):
        out[f"n{k}"] = (xyz[:k].copy(), None, lambda o, k=k: None if o["letters"] == "c" * k else f"letters {o['letters']}")
    return out


def build_n512(rng):
    tors = []
    while len(tors) < 512:
        basin = (HELIX, STRAND, PPII, LEFT)[rng.integers(4)]
        tors += jitter(rng, basin, int(rng.integers(4, 13)))

    def check(o):
        c = o["counts"]
        return None if c[3] >= 5 and c[4] >= 5 else f"blocks {c[3]} helix, {c[4]} strand"
    return {"n512": (backbone(tors[:512]), None, check)}


BUILDERS = (("hlh", build_hlh, 100), ("contact", build_contact, 200), ("run5", build_run(5), 300), ("run4", build_run(4), 400),
            ("ext", build_ext, 500), ("hole", build_hole, 600), ("n512", build_n512, 700))


def search(name, build, first_seed, tries=4000):
    for seed in range(first_seed, first_seed + tries):
        found = {}
        for key, (xyz, ok, check) in build(np.random.default_rng(seed)).items():
            o = S.annotate(xyz, ok)
            assert S.annotate(xyz.astype(np.float32), ok)["letters"] == o["letters"] or o["margin"] < MARGIN
            why = f"margin {o['margin']:.1e}" if o["margin"] < MARGIN and xyz.shape[0] > 1 else check(o)
            if why:
                print(f"rejected: {name} seed {seed}, chain {key}: {why}", flush=True)
                break
            found[key] = (xyz, ok, o, seed)
        else:
            return found
    raise SystemExit(f"no seed satisfies the conditions of {name}")


if __name__ == "__main__":
    out, report = {}, {}
    for name, build, first in BUILDERS:
        for key, (xyz, ok, o, seed) in search(name, build, first).items():
            out[f"xyz_{key}"] = xyz
            if ok is not None:
                out[f"atom_ok_{key}"] = ok
            report[key] = dict(n=int(xyz.shape[0]), atoms=3 if xyz.ndim == 3 else 1, letters=o["letters"], counts=[int(v) for v in o["counts"]],
                               blocks=blocks(o["letters"]), margin=None if o["margin"] == np.inf else o["margin"], seed=seed,
                               potential_helix=np.nonzero(o["potential_helix"])[0].tolist(),
                               potential_strand=np.nonzero(o["potential_strand"])[0].tolist())
            print(key, json.dumps(report[key]), flush=True)
    out["meta"] = np.array(json.dumps(dict(chains=report, keys=list(report), margin=MARGIN)))
    path = os.path.join(HERE, "sse_chains.npz")
    np.savez_compressed(path, **out)
    print("wrote sse_chains.npz,", os.path.getsize(path), "bytes")
