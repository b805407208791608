"""TM-align on the device: what the reference does with its backbones after the fold (``tm/TMalign.py:36-160``, ``utils.py:150-158``,
``play.py:49-61``), as one batched call on the coordinates ``fold_6d_batch`` leaves on the GPU.

``t2p_op_tm_align`` runs the default path of the reference's ``tm/TMalign.cpp`` for a batch of pairs of CA traces, one workgroup per
pair, in double: all five seeds, the iterated DP, the final searches at ``simplify_step = 1``.  Chain ``a`` is TM-align's
Chain_1 (the one superimposed), chain ``b`` its Chain_2.  Chains of 5 to ``TM_MAX_L`` = 256 residues; a pair with a chain outside that
range, or with a coordinate inside its length that is not finite (or beyond 1e6), comes back with ``status`` 1 and zero scores.  There is no CPU path.  Sequence input, ``-fast``, ``-i`` / ``-I``, circular
permutation, RNA, ``TMcut`` and the ``-a`` / ``-u`` / ``-d`` normalisations are not here.
"""
from __future__ import annotations

import numpy as np
import torch

from . import _lib
from ._lib import T2PError, check, ptr, stream_ptr

TM_MAX_L = 256
TM_MIN_L = 5
SEED_NAMES = ("get_initial", "get_initial_ss", "get_initial5", "get_initial_ssplus", "get_initial_fgt")
OUT_NAMES = ("tm_a", "tm_b", "rmsd", "n_ali8", "d0_a", "d0_b", "tm_max", "seed")


def _chains(xyz, lengths, name):
    """(n, L, atoms, 3) float32 on a GPU and (n,) int32 next to it; a (n, L, 3) CA trace is taken as atoms = 1."""
    if not isinstance(xyz, torch.Tensor):
        raise ValueError(f"xyz_{name} must be a torch tensor on a GPU device")
    if xyz.dim() == 3 and xyz.shape[-1] == 3:
        xyz = xyz.unsqueeze(2)
    if xyz.dim() != 4 or xyz.shape[3] != 3 or xyz.shape[2] not in (1, 3):
        raise ValueError(f"xyz_{name} must be (n, L, 3, 3) N / CA / C backbones or (n, L, 3) / (n, L, 1, 3) CA traces, not {tuple(xyz.shape)}")
    if not xyz.is_floating_point():
        raise ValueError(f"xyz_{name} must be a floating-point tensor, not {xyz.dtype}")
    if xyz.shape[0] < 1 or xyz.shape[1] < 1:
        raise ValueError(f"xyz_{name} needs at least one chain and one residue")
    if xyz.shape[1] > TM_MAX_L:
        raise ValueError(f"xyz_{name}: {xyz.shape[1]} residues exceed TM_MAX_L = {TM_MAX_L} (csrc/t2p_kernels.h)")
    if xyz.device.type != "cuda":
        raise T2PError("tm_align needs the coordinates on a GPU device (there is no CPU fallback)")
    n = torch.as_tensor(lengths)
    if n.is_floating_point() or tuple(n.shape) != (xyz.shape[0],):
        raise ValueError(f"len_{name} must hold {xyz.shape[0]} integers")
    return xyz.to(torch.float32).contiguous(), n.to(xyz.device, torch.int32).contiguous()


def tm_align_batch(xyz_a, len_a, xyz_b, len_b, pairs=None, with_map=False, with_rot=False):
    """TM-align of chains ``a`` (superimposed, Chain_1) onto chains ``b`` (Chain_2).  ``pairs``: (n_pairs, 2) integers (index into a,
    index into b), or None for all ``n_a * n_b`` pairs in row-major order.  Returns a dict of device tensors: ``tm_a``, ``tm_b`` (the
    TM-score normalised by the length of a, of b), ``rmsd``, ``n_ali8``, ``d0_a``, ``d0_b``, ``tm_max``, ``seed`` (all (n_pairs,)
    float64), ``out8`` (n_pairs, 8), ``status`` (n_pairs,) int32 (1 = a chain shorter than 5, longer than 256 or with a non-finite
    coordinate: scores zero) and, when
    asked for, ``b2a`` (n_pairs, Lb) int32 (the printed alignment, -1 = unaligned) and ``rot`` (n_pairs, 12) float64 (t then u of the
    superposition of a onto b behind ``tm_b``).  A pair index outside its set raises ``T2PError``."""
    a, na = _chains(xyz_a, len_a, "a")
    b, nb = _chains(xyz_b, len_b, "b")
    if a.device != b.device:
        raise ValueError("xyz_a and xyz_b must be on the same device")
    dev = a.device
    if pairs is None:
        pr, n_pairs = None, a.shape[0] * b.shape[0]
    else:
        pr = torch.as_tensor(pairs)
        if pr.is_floating_point() or pr.dim() != 2 or pr.shape[1] != 2 or pr.shape[0] < 1:
            raise ValueError("pairs must be (n_pairs, 2) integers with at least one pair")
        pr = pr.to(dev, torch.int32).contiguous()
        n_pairs = pr.shape[0]
    lib = _lib.load()
    La, Lb = a.shape[1], b.shape[1]
    nbytes = int(lib.t2p_op_tm_align_ws(n_pairs, La, Lb))
    if nbytes < 0:
        raise ValueError(f"tm_align: {La} / {Lb} residues exceed TM_MAX_L = {TM_MAX_L}")
    ws = torch.empty(nbytes, device=dev, dtype=torch.uint8)
    out8 = torch.empty(n_pairs, 8, device=dev, dtype=torch.float64)
    status = torch.empty(n_pairs, device=dev, dtype=torch.int32)
    b2a = torch.empty(n_pairs, Lb, device=dev, dtype=torch.int32) if with_map else None
    rot = torch.empty(n_pairs, 12, device=dev, dtype=torch.float64) if with_rot else None
    with torch.cuda.device(dev):
        check(lib.t2p_op_tm_align(ptr(a), ptr(na), a.shape[0], La, a.shape[2], ptr(b), ptr(nb), b.shape[0], Lb, b.shape[2], ptr(pr), n_pairs,
                                  ptr(out8), ptr(b2a), ptr(rot), ptr(status), ptr(ws), nbytes, stream_ptr()))
    if pr is not None and int(ws[:4].view(torch.int32).item()) != 0:
        raise T2PError(f"tm_align: a pair index lies outside [0, {a.shape[0]}) x [0, {b.shape[0]})")
    res = {nm: out8[:, k] for k, nm in enumerate(OUT_NAMES)}
    res.update(out8=out8, status=status)
    if with_map:
        res["b2a"] = b2a
    if with_rot:
        res["rot"] = rot
    return res


def tm_matrix(xyz_a, len_a, xyz_b, len_b):
    """(n_a, n_b, 2) float64 on the device: [..., 0] normalised by the chain of a, [..., 1] by the chain of b."""
    r = tm_align_batch(xyz_a, len_a, xyz_b, len_b)
    return r["out8"][:, :2].reshape(xyz_a.shape[0], xyz_b.shape[0], 2)


def pairwise_tm(xyz, lengths):
    """The samples against each other: ``(matrix, mean)`` with ``matrix`` (n, n) float64 on the device, symmetric, unit diagonal, entry
    (i, j) = max(TM normalised by i, by j) of the one alignment of i onto j (i < j); ``mean`` is the mean over the pairs i < j that
    ``play.calculate_sctm_score`` forms (a 0-dim device tensor; NaN for a single chain)."""
    x, n = _chains(xyz, lengths, "a")
    m = x.shape[0]
    mat = torch.eye(m, device=x.device, dtype=torch.float64)
    if m < 2:
        return mat, torch.full((), float("nan"), device=x.device, dtype=torch.float64)
    iu = torch.triu_indices(m, m, offset=1, device=x.device)
    r = tm_align_batch(x, n, x, n, pairs=iu.t().contiguous())
    best = torch.maximum(r["tm_a"], r["tm_b"])
    mat[iu[0], iu[1]] = best
    mat[iu[1], iu[0]] = best
    return mat, best.mean()


def _summary(tm, ok, names):
    """One sample's row against the references that were scored (``ok``): tm (R, 2), normalised by the sample / by the reference."""
    v = tm[ok, 1]
    k = int(np.argmax(np.where(ok, tm[:, 1], -np.inf)))
    return {"sample_min": float(v.min()), "sample_max": float(v.max()), "sample_avg": float(v.mean()), "sample_std": float(np.std(v)),
            "closest": names[k] if names is not None else k, "tm_by_sample": float(tm[k, 0]), "tm_by_reference": float(tm[k, 1])}


def novelty(xyz, lengths, ref_xyz, ref_lengths, names=None):
    """``train_gen_tm_compare`` (tm/TMalign.py:63-160) for samples already on the device: every sample (Chain_1) against every reference
    (Chain_2), scored as ``tm_score`` does -- normalised by the reference chain.  Returns ``(samples, overall)``: per sample a dict
    ``sample_min / sample_max / sample_avg / sample_std`` (np.std, as the reference), ``closest`` (the name, or index, of the reference
    of the maximum), ``tm_by_sample`` / ``tm_by_reference`` (both normalisations of that closest alignment); ``overall`` holds ``tm_max /
    tm_min / tm_avg / tm_std / reference_count / target_count``.  A refused pair (``status`` 1) raises ``ValueError``."""
    r = tm_align_batch(xyz, lengths, ref_xyz, ref_lengths)
    if int(r["status"].max()) != 0:
        raise ValueError(f"tm_align: a chain outside {TM_MIN_L} to {TM_MAX_L} residues or with a non-finite coordinate")
    m = r["out8"][:, :2].reshape(xyz.shape[0], ref_xyz.shape[0], 2).cpu().numpy()
    if names is not None and len(names) != m.shape[1]:
        raise ValueError(f"names must hold {m.shape[1]} entries")
    ok = np.ones(m.shape[1], bool)
    samples = [_summary(row, ok, names) for row in m]
    s = m[:, :, 1]
    overall = {"tm_max": float(s.max()), "tm_min": float(s.min()), "tm_avg": float(s.mean()), "tm_std": float(np.std(s)),
               "reference_count": int(m.shape[1]), "target_count": int(m.shape[0])}
    return samples, overall


def reference_files(paths):
    """``--tm_ref``: every PATH is a ``.pdb`` file or a directory of them (sorted by name).  Host only; raises ``ValueError`` for a path
    that does not exist, a file of another kind or a directory without a ``.pdb`` file."""
    import os
    files = []
    for p in paths:
        p = str(p)
        if os.path.isdir(p):
            found = sorted(os.path.join(p, f) for f in os.listdir(p) if f.lower().endswith(".pdb"))
            if not found:
                raise ValueError(f"--tm_ref {p}: the directory holds no .pdb file")
            files += found
        elif os.path.isfile(p):
            if not p.lower().endswith(".pdb"):
                raise ValueError(f"--tm_ref {p}: not a .pdb file")
            files.append(p)
        else:
            raise ValueError(f"--tm_ref {p}: no such file or directory")
    return files


def score_samples(xyz, lengths, ids, ref_xyz, ref_lengths, ref_names):
    """What ``sampling_6d.py --tm_ref`` writes as ``tm_scores.json``: ``xyz`` / ``lengths`` are the folded chains to score (device), ``ids``
    their names.  One ``tm_align_batch`` call against the references, one ``pairwise_tm`` call among the samples.  A sample that no
    reference could be aligned with is listed with ``"scored": false`` and ``"why"``: ``"sample"`` when its own length lies outside 5 to
    256 residues, else ``"references"`` (none of them usable: their lengths, or a non-finite coordinate)."""
    m = tm_align_batch(xyz, lengths, ref_xyz, ref_lengths)
    st = m["status"].reshape(len(ids), -1).cpu().numpy()
    tm = m["out8"][:, :2].reshape(len(ids), -1, 2).cpu().numpy()
    samples = {}
    for k, sid in enumerate(ids):
        ok, n = st[k] == 0, int(lengths[k])
        if ok.any():
            samples[str(sid)] = dict(_summary(tm[k], ok, ref_names), scored=True, L=n)
        else:
            samples[str(sid)] = {"scored": False, "L": n, "why": "sample" if not TM_MIN_L <= n <= TM_MAX_L else "references"}
    scored = [k for k, sid in enumerate(ids) if samples[str(sid)]["scored"]]
    out = {"references": list(ref_names), "references_scored": [bool(v) for v in (st == 0).any(0)], "samples": samples,
           "pairwise_ids": [str(ids[k]) for k in scored], "pairwise": [], "pairwise_mean": None}
    if scored:
        idx = torch.as_tensor(scored, device=xyz.device)
        mat, mean = pairwise_tm(xyz[idx], torch.as_tensor(lengths)[torch.as_tensor(scored)])
        out["pairwise"] = mat.cpu().tolist()
        out["pairwise_mean"] = float(mean) if len(scored) > 1 else None
    return out


# ---- the reference's surface (paths in, floats out) ----
def read_chains(paths, chain="A"):
    """The chains of PDB files as one padded device batch: ``(xyz (n, L, 3, 3) float32, NaN past each length, lengths (n,) int32)``."""
    from .encode import read_backbone
    if not torch.cuda.is_available():
        raise T2PError("tm_align needs a GPU device (there is no CPU fallback)")
    chains = [read_backbone(str(p), chain) for p in paths]
    L = max(c[2] for c in chains)
    if L > TM_MAX_L:
        raise ValueError(f"a chain of {L} residues exceeds TM_MAX_L = {TM_MAX_L}")
    xyz = np.full((len(chains), L, 3, 3), np.nan, np.float32)
    for k, (x, ok, n) in enumerate(chains):
        if not ok[:, 1].all():
            raise ValueError(f"{paths[k]}: a residue without a CA atom")
        xyz[k, :n] = x
    return torch.from_numpy(xyz).cuda(), torch.tensor([c[2] for c in chains], dtype=torch.int32).cuda()


def _pair(path1, path2, chain):
    xa, na = read_chains([path1], chain)
    xb, nb = read_chains([path2], chain)
    r = tm_align_batch(xa, na, xb, nb)
    if int(r["status"][0]) != 0:
        raise ValueError(f"tm_align: chains of {int(na[0])} and {int(nb[0])} residues; {TM_MIN_L} to {TM_MAX_L} are supported")
    return r


def tm_score(target_path, reference_path, chain="A"):
    """tm/TMalign.py:36-49: the TM-score of target onto reference, normalised by the reference (second) chain."""
    return float(_pair(target_path, reference_path, chain)["tm_b"][0])


def run_tmalign(path1, path2, chain="A"):
    """utils.py:150-158: the first ``TM-score=`` line TM-align prints, i.e. normalised by the FIRST chain."""
    return float(_pair(path1, path2, chain)["tm_a"][0])


def max_min_avg_tm_score(target_list, reference_list, chain="A"):
    """tm/TMalign.py:52-61: every target against every reference (one call); ``(tm_max, tm_min, tm_avg)``."""
    xa, na = read_chains(list(target_list), chain)
    xb, nb = read_chains(list(reference_list), chain)
    r = tm_align_batch(xa, na, xb, nb)
    if int(r["status"].max()) != 0:
        raise ValueError(f"tm_align: a chain outside {TM_MIN_L} to {TM_MAX_L} residues")
    s = r["tm_b"]
    return float(s.max()), float(s.min()), float(s.mean())
