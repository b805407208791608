"""t2p_op_tm_align on the GPU against tests/golden/tmalign_pairs.npz (tests/golden/make_golden_tmalign.py).

Every fixture pair is aligned once, in one call, and shared.  Two references, each with its own bound:
  * what the reference's own TM-align printed for the pair: both TM-scores within 1e-5 (one unit of the last digit it prints; its
    rounding is 5e-6, the float32 input rounding about 1e-7), n_ali8 and the b -> a map equal, RMSD within 5e-3 (printed to two
    decimals), the ``-m`` matrix within 1e-4 (printed to ten decimals, driven by coordinates exact to 1e-6 A);
  * the float64 oracle (tests/tmalign_oracle.py) on the same float32-widened coordinates: TM-scores, TMmax and RMSD within 1e-9, seed
    index and map equal.  Both sides sum at most 256 terms of at most 1 in double (3e-14 per score) and nothing accumulates across
    iterations because every fit starts from the coordinates; 1e-9 leaves four orders over that and lies four under the print
    resolution.  Only a discrete decision on a knife edge could exceed it.
The figures are printed before they are asserted.
"""
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch
import yaml

from helpers import GOLDEN, cfg_ckpt, load_golden

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def gold():
    g = load_golden("tmalign_pairs")
    g["meta"] = json.loads(str(g["meta"]))
    return g


def _batch(gold, names, L=None, atoms=3):
    ns = [gold["xyz_" + k].shape[0] for k in names]
    L = L or max(ns)
    xyz = torch.full((len(names), L, 3, 3), float("nan"))
    for b, k in enumerate(names):
        xyz[b, :ns[b]] = torch.from_numpy(gold["xyz_" + k])
    if atoms == 1:
        xyz = xyz[:, :, 1].contiguous()
    return xyz.cuda(), torch.tensor(ns, dtype=torch.int32)


@pytest.fixture(scope="module")
def aligned(gold):
    """All chains of the fixture in one padded batch (NaN past the lengths), every fixture pair aligned in one call."""
    from text2protein_amd.tmalign import tm_align_batch
    names = gold["meta"]["chains"]
    xyz, n = _batch(gold, names)
    pairs = torch.tensor([[names.index(p["a"]), names.index(p["b"])] for p in gold["meta"]["pairs"]])
    r = tm_align_batch(xyz, n, xyz, n, pairs=pairs, with_map=True, with_rot=True)
    torch.cuda.synchronize()
    return dict(names=names, xyz=xyz, n=n, pairs=pairs, r={k: v.cpu().numpy() for k, v in r.items()})


def _same(r1, r2, rows1=None, rows2=None):
    for k in ("out8", "status", "b2a", "rot"):
        if k in r1 and k in r2:
            a = r1[k].cpu().numpy() if isinstance(r1[k], torch.Tensor) else r1[k]
            b = r2[k].cpu().numpy() if isinstance(r2[k], torch.Tensor) else r2[k]
            a = a if rows1 is None else a[rows1]
            b = b if rows2 is None else b[rows2]
            if k == "b2a":                                      # padded to different widths: equal where both exist, -1 beyond
                w = min(a.shape[1], b.shape[1])
                assert (a[:, w:] == -1).all() and (b[:, w:] == -1).all()
                a, b = a[:, :w], b[:, :w]
            assert a.tobytes() == b.tobytes(), k


def test_against_recorded_tm_align(gold, aligned):
    r = aligned["r"]
    assert (r["status"] == 0).all() and np.isfinite(r["out8"]).all()
    worst = np.zeros(4)
    for p, pair in enumerate(gold["meta"]["pairs"]):
        tm_a, tm_b, rmsd, n8 = gold[f"ref_scalars_{p}"]
        o = r["out8"][p]
        d = np.array([abs(o[0] - tm_a), abs(o[1] - tm_b), abs(o[2] - rmsd), np.abs(r["rot"][p] - gold[f"ref_rot_{p}"]).max()])
        worst = np.maximum(worst, d)
        print(f"{pair['a']:>9s} {pair['b']:>9s}  TM {o[0]:.6f} {o[1]:.6f} ({tm_a:.5f} {tm_b:.5f})  n {int(o[3])} ({int(n8)})  rmsd {o[2]:.4f} "
              f"({rmsd:.2f})  seed {int(o[7])}  |d| TM {d[0]:.1e} {d[1]:.1e} rmsd {d[2]:.1e} matrix {d[3]:.1e}")
        assert d[0] <= 1e-5 and d[1] <= 1e-5
        assert int(o[3]) == int(n8) and np.array_equal(r["b2a"][p, :pair["len_b"]], gold[f"ref_b2a_{p}"])
        assert (r["b2a"][p, pair["len_b"]:] == -1).all()
        assert d[2] <= 5e-3 and d[3] <= 1e-4
    print("worst: TM", worst[0], worst[1], "rmsd", worst[2], "matrix", worst[3])


def test_against_the_oracle(gold, aligned):
    r = aligned["r"]
    worst = 0.0
    for p, pair in enumerate(gold["meta"]["pairs"]):
        want, got = gold[f"orc_out8_{p}"], r["out8"][p]
        d = np.abs(got - want)
        worst = max(worst, d[[0, 1, 2, 6]].max())
        print(f"{pair['a']:>9s} {pair['b']:>9s}  |gpu - oracle|  TM {d[0]:.1e} {d[1]:.1e}  rmsd {d[2]:.1e}  TMmax {d[6]:.1e}  d0 {d[4]:.1e} {d[5]:.1e}  "
              f"seed {int(got[7])} ({int(want[7])})")
        assert d[[0, 1, 2, 6]].max() <= 1e-9 and d[[4, 5]].max() <= 1e-12
        assert int(got[3]) == int(want[3]) and int(got[7]) == int(want[7])
        assert np.array_equal(r["b2a"][p, :pair["len_b"]], gold[f"orc_b2a_{p}"])
        assert np.abs(r["rot"][p] - gold[f"orc_rot_{p}"]).max() <= 1e-9
    print("worst |gpu - oracle| over TM, rmsd, TMmax:", worst)


def test_order_padding_and_layout_change_no_bit(gold, aligned):
    from text2protein_amd.tmalign import tm_align_batch
    base, pairs = aligned["r"], aligned["pairs"]
    # two calls agree
    again = tm_align_batch(aligned["xyz"], aligned["n"], aligned["xyz"], aligned["n"], pairs=pairs, with_map=True, with_rot=True)
    _same(again, base)
    # the same pairs at other positions of the list, some of them twice
    perm = torch.tensor([5, 0, 16, 3, 3, 9, 12, 0])
    r = tm_align_batch(aligned["xyz"], aligned["n"], aligned["xyz"], aligned["n"], pairs=pairs[perm], with_map=True, with_rot=True)
    _same(r, base, None, perm.numpy())
    # pairs = None against the explicit list; tight arrays (four wavefronts at 132 residues) against the 256-wide batch (three); a CA trace
    # (atoms = 1) against N / CA / C
    names = aligned["names"]
    a_set, b_set = ["96cut", "48"], ["96", "132"]
    xa, na = _batch(gold, a_set)
    xb, nb = _batch(gold, b_set)
    full = tm_align_batch(xa, na, xb, nb, with_map=True, with_rot=True)
    explicit = tm_align_batch(xa, na, xb, nb, pairs=torch.tensor([[0, 0], [0, 1], [1, 0], [1, 1]]), with_map=True, with_rot=True)
    _same(full, explicit)
    wide = tm_align_batch(aligned["xyz"], aligned["n"], aligned["xyz"], aligned["n"],
                          pairs=torch.tensor([[names.index(a), names.index(b)] for a in a_set for b in b_set]), with_map=True, with_rot=True)
    _same(full, wide)
    xa1, _ = _batch(gold, a_set, atoms=1)
    xb1, _ = _batch(gold, b_set, L=200, atoms=1)
    _same(full, tm_align_batch(xa1, na, xb1, nb, with_map=True, with_rot=True))
    rows = {(p["a"], p["b"]): k for k, p in enumerate(gold["meta"]["pairs"])}
    _same(full, base, [0, 2, 3], [rows[("96cut", "96")], rows[("48", "96")], rows[("48", "132")]])


def test_refusals(gold, aligned):
    from text2protein_amd import _lib
    from text2protein_amd._lib import T2PError, ptr, stream_ptr
    from text2protein_amd.tmalign import tm_align_batch
    names = ["48", "96", "256", "96cut"]
    x, n = _batch(gold, names)
    n_bad = n.clone()
    n_bad[1], n_bad[2] = 4, 257                                  # below TM-align's usable floor; above TM_MAX_L (and the array)
    good = tm_align_batch(x, n, x, n, with_map=True, with_rot=True)
    r = tm_align_batch(x, n_bad, x, n, with_map=True, with_rot=True)
    st = r["status"].reshape(4, 4).cpu().numpy()
    assert (st[[1, 2]] == 1).all() and (st[[0, 3]] == 0).all()
    bad_rows = [4, 5, 6, 7, 8, 9, 10, 11]
    assert (r["out8"][bad_rows] == 0).all() and (r["rot"][bad_rows] == 0).all() and (r["b2a"][bad_rows] == -1).all()
    ok_rows = [0, 1, 2, 3, 12, 13, 14, 15]
    _same(r, good, ok_rows, ok_rows)                             # the neighbours are untouched
    r = tm_align_batch(x, n, x, n_bad)
    assert (r["status"].reshape(4, 4).cpu().numpy()[:, [1, 2]] == 1).all() and int(r["status"].sum()) == 8
    # a coordinate inside the length that is not finite, or absurdly large: the pair is refused, not aligned (every distance would be
    # NaN); the other pairs of the call are untouched
    xn = x.clone()
    xn[0, 17, 1, 2] = float("nan")
    xn[3, 0, 1, 0] = float("inf")
    xn[1, 95, 1, 1] = 3.0e6
    xn[2, 40, 0, 0] = float("nan")                               # N of a residue: not read, chain 2 stays usable
    r = tm_align_batch(xn, n, x, n, with_map=True, with_rot=True)
    st = r["status"].reshape(4, 4).cpu().numpy()
    assert (st[[0, 1, 3]] == 1).all() and (st[2] == 0).all()
    rows = [0, 1, 2, 3, 4, 5, 6, 7, 12, 13, 14, 15]
    assert (r["out8"][rows] == 0).all() and (r["rot"][rows] == 0).all() and (r["b2a"][rows] == -1).all()
    _same(r, good, [8, 9, 10, 11], [8, 9, 10, 11])
    r = tm_align_batch(x, n, xn, n)                              # and as chain b
    assert (r["status"].reshape(4, 4).cpu().numpy() == np.array([1, 1, 0, 1])[None]).all()
    # a pair index outside its set
    for bad in ([[0, 4]], [[-1, 0]], [[0, 0], [4, 1]]):
        with pytest.raises(T2PError, match="pair index"):
            tm_align_batch(x, n, x, n, pairs=torch.tensor(bad))
    # refused before launch: a short workspace, atoms other than 1 or 3, non-positive counts
    lib = _lib.load()
    nd = n.cuda()
    out8 = torch.full((16, 8), -7.0, dtype=torch.float64, device="cuda")
    status = torch.full((16,), -7, dtype=torch.int32, device="cuda")
    ws = torch.zeros(int(lib.t2p_op_tm_align_ws(16, 256, 256)), dtype=torch.uint8, device="cuda")
    assert lib.t2p_op_tm_align_ws(16, 257, 256) == -1 and lib.t2p_op_tm_align_ws(16, 256, 257) == -1

    def call(atoms=3, n_pairs=16, nbytes=ws.numel()):
        return lib.t2p_op_tm_align(ptr(x), ptr(nd), 4, 256, atoms, ptr(x), ptr(nd), 4, 256, 3, None, n_pairs, ptr(out8), None, None, ptr(status),
                                   ptr(ws), nbytes, stream_ptr())
    for kw, what in ((dict(nbytes=ws.numel() - 1), "workspace"), (dict(atoms=2), "atoms_a"), (dict(n_pairs=0), "positive")):
        assert call(**kw) != 0
        assert what in lib.t2p_last_error().decode(), lib.t2p_last_error()
    torch.cuda.synchronize()
    assert (out8 == -7.0).all() and (status == -7).all()         # nothing was launched
    assert call() == 0


def test_reference_surface_on_written_files(gold, aligned, tmp_path):
    from text2protein_amd import tmalign as T
    from text2protein_amd.fold import write_backbone_pdb
    for k in ("96cut", "96", "48"):
        write_backbone_pdb(tmp_path / f"{k}.pdb", gold["xyz_" + k])
    rows = {(p["a"], p["b"]): k for k, p in enumerate(gold["meta"]["pairs"])}
    o = aligned["r"]["out8"]
    p1, p2 = rows[("96cut", "96")], rows[("48", "96")]
    assert T.tm_score(tmp_path / "96cut.pdb", tmp_path / "96.pdb") == o[p1, 1]           # normalised by the second chain
    assert T.run_tmalign(tmp_path / "96cut.pdb", tmp_path / "96.pdb") == o[p1, 0]        # by the first
    mx, mn, avg = T.max_min_avg_tm_score([tmp_path / "96cut.pdb", tmp_path / "48.pdb"], [tmp_path / "96.pdb"])
    assert mx == max(o[p1, 1], o[p2, 1]) and mn == min(o[p1, 1], o[p2, 1]) and abs(avg - (o[p1, 1] + o[p2, 1]) / 2) < 1e-15
    x, n = _batch(gold, ["48", "96", "96cut"])
    mat, mean = T.pairwise_tm(x, n)
    m = mat.cpu().numpy()
    assert m.shape == (3, 3) and (m == m.T).all() and (np.diag(m) == 1.0).all()
    assert m[0, 1] == max(o[p2, 0], o[p2, 1]) and m[1, 2] == 1.0 and abs(float(mean) - m[np.triu_indices(3, 1)].mean()) < 1e-15
    tm = T.tm_matrix(x, n, x[:2], n[:2])
    assert tuple(tm.shape) == (3, 2, 2) and tm[0, 1, 0] == o[p2, 0] and tm[0, 1, 1] == o[p2, 1]
    samples, overall = T.novelty(x, n, x[:2], n[:2], names=["ref48", "ref96"])
    assert [s["closest"] for s in samples[:2]] == ["ref48", "ref96"] and samples[2]["sample_max"] >= o[p1, 1]
    assert all(s["sample_min"] <= s["sample_avg"] <= s["sample_max"] and s["sample_std"] >= 0 for s in samples)
    assert overall["reference_count"] == 2 and overall["target_count"] == 3 and overall["tm_max"] == 1.0


def test_cli_tm_ref_scores_every_folded_chain(gold, tmp_path):
    from text2protein_amd.fold import write_backbone_pdb
    refs = tmp_path / "refs"
    refs.mkdir()
    write_backbone_pdb(refs / "r48.pdb", gold["xyz_48"])
    write_backbone_pdb(refs / "w8.pdb", gold["xyz_w8"])
    write_backbone_pdb(tmp_path / "r96cut.pdb", gold["xyz_96cut"])
    cfg = cfg_ckpt()
    cfg.training.sde = "vesde"
    cfg.model.condition = ["length"]
    cfg_path = tmp_path / "ckpt_length.yml"
    with open(cfg_path, "w") as f:
        yaml.safe_dump(yaml.safe_load(json.dumps(cfg)), f)
    out = tmp_path / "out"
    cmd = [sys.executable, os.path.join(ROOT, "sampling_6d.py"), str(cfg_path), os.path.join(GOLDEN, "tiny_checkpoint.pth"), "--batch_size", "2",
           "--context_tokens", "4", "--dtype", "f32", "--select_length", "1", "--length_index", "4", "--outdir", str(out), "--tm_ref", str(refs),
           "--tm_ref", str(tmp_path / "r96cut.pdb")]
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=600, cwd=str(tmp_path))
    assert r.returncode == 0, r.stdout + r.stderr
    assert sorted(os.listdir(out)) == sorted([f"{stem}_{i}.{ext}" for i in (0, 1) for stem, ext in
                                              (("sampled", "pkl"), ("decoded", "npz"), ("folded", "pdb"), ("fold", "json"))] + ["tm_scores.json"])
    with open(out / "tm_scores.json") as f:
        tm = json.load(f)
    assert tm["references"] == ["r48.pdb", "w8.pdb", "r96cut.pdb"] and tm["pairwise_ids"] == ["0", "1"]
    for i in ("0", "1"):
        s = tm["samples"][i]
        assert s["scored"] and s["L"] == 7 and s["closest"] in tm["references"]
        vals = [s[k] for k in ("sample_min", "sample_max", "sample_avg", "sample_std", "tm_by_sample", "tm_by_reference")]
        assert np.isfinite(vals).all() and 0.0 < s["sample_min"] <= s["sample_avg"] <= s["sample_max"] <= 1.0
        assert f"sample {i}: TM to 3 references" in r.stdout
    m = np.array(tm["pairwise"])
    assert m.shape == (2, 2) and (m == m.T).all() and (np.diag(m) == 1.0).all() and np.isfinite(m).all()
    assert abs(tm["pairwise_mean"] - m[0, 1]) < 1e-15


def test_kernel_uses_no_scratch():
    """The occupancy facts DESIGN.md 8g states, from the loaded code object: no scratch, LDS under the 64 KB a workgroup gets without
    opting in at every padded length up to TM_MAX_L."""
    import ctypes as C
    from text2protein_amd import _lib
    lib = _lib.load()
    info = (C.c_int32 * 4)()
    for La, Lb, waves, lds in ((128, 128, 4, 39424), (192, 256, 4, 61120), (193, 256, 3, None), (256, 256, 3, 60800)):
        _lib.check(lib.t2p_debug_tm_align_info(La, Lb, C.cast(info, C.c_void_p)))
        print(La, Lb, list(info))
        assert info[0] == waves and info[1] <= 65536 and (lds is None or info[1] == lds)
        assert info[3] == 0, f"tm_align_kernel spills {info[3]} bytes per lane to scratch"
