"""Backbone geometry shared by the numpy oracles (fold_oracle, refine_oracle, refine_rounds_oracle) and the encode tests: the test-side
twin of csrc/backbone_geom.h.  Float64 numpy for float64 input; every function keeps the dtype it is given, which is how
fold_oracle.restraint_score runs in float32.  Points are single vectors or rows of vectors.  Test infrastructure only.
"""
import numpy as np

K1, K2, K3 = -0.58273431, 0.56802827, -0.54067466          # the featuriser's virtual-Cb identity (dataset.py:409)
GUARD = 1e-12                                               # floor of a denominator


def _dot(a, b):
    return (a * b).sum(-1)


def virtual_cb(n, ca, c):
    """Cb = K1 (b x c) + K2 b + K3 c + CA with b = CA - N, c = C - CA."""
    b, c = ca - n, c - ca
    return K1 * np.cross(b, c) + K2 * b + K3 * c + ca


def wrap(x, dtype=np.float64):
    """x brought into [-pi, pi] by a multiple of 2 pi (held in `dtype`)."""
    two_pi = dtype(2.0 * np.pi)
    return x - two_pi * np.round(x / two_pi)


def angle(pa, pb, pc):
    """The angle at pb: atan2(|v x w|, v . w)."""
    v, w = pa - pb, pc - pb
    cr = np.cross(v, w)
    return np.arctan2(np.sqrt(_dot(cr, cr)), _dot(v, w))


def dihedral_projection(a, b, c, d):
    """Dihedral a-b-c-d, projection form (get_dihedrals, dataset.py:364-380): the arms projected off the unit axis.  The form of the
    restraint score and of the 6D encode (backbone_geom.h's dihedral_or_zero); a zero axis is NaN here, where the kernels write 0."""
    b0, b1, b2 = a - b, c - b, d - c
    b1 = b1 / np.linalg.norm(b1, axis=-1, keepdims=True)
    v = b0 - _dot(b0, b1)[..., None] * b1
    w = b2 - _dot(b2, b1)[..., None] * b1
    return np.arctan2(_dot(np.cross(b1, v), w), _dot(v, w))


def dihedral_cross(p0, p1, p2, p3):
    """Dihedral p0-p1-p2-p3, cross-product form with |p1 - p2|^2 floored by GUARD: the minimiser's value and the move's measurement
    (backbone_geom.h's dihedral_guarded).  The same sign as dihedral_projection."""
    f, g, h = p0 - p1, p1 - p2, p3 - p2
    a, b = np.cross(f, g), np.cross(h, g)
    gl = np.sqrt(np.maximum(_dot(g, g), GUARD))
    return np.arctan2(_dot(np.cross(b, a), g) / gl, _dot(a, b))
