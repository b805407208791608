"""Secondary structure on the GPU (t2p_op_annotate_sse, text2protein_amd/encode.py annotate_sse_batch) against the float64 oracle
(tests/sse_oracle.py) on the recorded chains (tests/golden/sse_chains.npz, tests/golden/make_golden_sse.py) and on the four chains of
tests/golden/fold_chains.npz, then the layers on top: sse="psea" in the encoder and the condition builder, the agreement of a folded
chain with a target, and the command line.

The comparison is EXACT: letters, counts and status.  Every fixture's margin (the smallest distance of any quantity from any of its
thresholds) is at least 1e-4 A or degrees, the kernel computes in double from the same fp32 coordinates, and its sqrt / acos / atan2
differ from numpy's by a few units in the last place (1e-13 at these magnitudes): no label can move.  The end-to-end test runs the
oracle on the GPU's own fp32 backbone and first asserts that margin there is at least 1e-9 -- a condition on that input, reported as
such -- before it asks for equality.
"""
import ctypes as C
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch
import yaml

import sse_oracle as S
from helpers import GOLDEN, load_golden

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PDB = os.path.join(GOLDEN, "encode_chain.pdb")
FOLD_KEYS = ("48", "96", "96cut", "132")
CASES = {"L512": 512, "L64": 64}


@pytest.fixture(scope="module")
def chains():
    """key -> (xyz float32 (n, 3, 3) or (n, 3), atom_ok or None, the oracle's result on those float32 coordinates), computed once."""
    g = load_golden("sse_chains")
    meta = json.loads(str(g["meta"]))
    out = {}
    for key in meta["keys"]:
        x, ok = g[f"xyz_{key}"].astype(np.float32), g.get(f"atom_ok_{key}")
        out[key] = (x, ok, S.annotate(x, ok))
        assert out[key][2]["letters"] == meta["chains"][key]["letters"]
    f = load_golden("fold_chains")
    for key in FOLD_KEYS:
        x = f[f"xyz_{key}"].astype(np.float32)
        out["fold" + key] = (x, None, S.annotate(x))
        assert out["fold" + key][2]["margin"] >= 1e-4
    return out


def _batch(chains, keys, L, atoms):
    """The padded batch.  Padding rows, and the N and C of a chain that is a CA trace, hold NaN; a missing atom holds a large number:
    none of them may be read."""
    B = len(keys)
    xyz = torch.full((B, L, atoms, 3), float("nan"))
    ok = torch.zeros(B, L, atoms, dtype=torch.uint8)
    for b, k in enumerate(keys):
        x, a, _ = chains[k]
        n = x.shape[0]
        ca = torch.from_numpy(x[:, 1] if x.ndim == 3 else x)
        present = torch.ones(n, dtype=torch.uint8) if a is None else torch.from_numpy(a[:, 1])
        ca = torch.where(present[:, None] != 0, ca, torch.full_like(ca, 999.0))
        if atoms == 1:
            xyz[b, :n, 0], ok[b, :n, 0] = ca, present
        elif x.ndim == 3:
            xyz[b, :n], ok[b, :n] = torch.from_numpy(x), 1 if a is None else torch.from_numpy(a)
            xyz[b, :n, 1] = ca
        else:
            xyz[b, :n, 1], ok[b, :n, 1] = ca, present
    nres = torch.tensor([chains[k][0].shape[0] for k in keys], dtype=torch.int32)
    return (xyz[:, :, 0] if atoms == 1 else xyz).cuda(), nres.cuda(), (ok[:, :, 0] if atoms == 1 else ok).cuda()


@pytest.fixture(scope="module")
def annotated(chains):
    """Every (case, atoms) annotated once and shared."""
    from text2protein_amd.encode import annotate_sse_batch
    out = {}
    for name, L in CASES.items():
        keys = [k for k, (x, _, _) in chains.items() if x.shape[0] <= L]
        for atoms in (1, 3):
            xyz, nres, ok = _batch(chains, keys, L, atoms)
            out[name, atoms] = (keys, annotate_sse_batch(xyz, nres, atom_ok=ok), (xyz, nres, ok))
    torch.cuda.synchronize()
    return out


@pytest.mark.parametrize("atoms", [3, 1])
@pytest.mark.parametrize("case", list(CASES))
def test_letters_counts_and_status_equal_the_oracle(chains, annotated, case, atoms):
    keys, got, _ = annotated[case, atoms]
    L = CASES[case]
    assert ("n512" in keys) == (L == 512) and {"hlh", "near", "far", "run5", "run4", "ext", "hole", "n1", "n4", "fold48"} <= set(keys)
    dev, counts, status = got["letters_dev"].cpu().numpy(), got["counts"].cpu().numpy(), got["status"].cpu().tolist()
    assert dev.shape == (len(keys), L) and dev.dtype == np.uint8 and counts.shape == (len(keys), 12) and counts.dtype == np.int32
    for b, k in enumerate(keys):
        o = chains[k][2]
        n = len(o["letters"])
        print(f"{case} atoms {atoms} {k}: margin {o['margin']:.2e}, counts {counts[b].tolist()}")
        assert got["letters"][b] == o["letters"], k
        assert bytes(dev[b, :n]).decode() == o["letters"] and (dev[b, n:] == 0).all(), k       # 0 past the length
        assert counts[b].tolist() == o["counts"] and status[b] == o["status"] == 0, k


def test_both_layouts_and_both_paddings_agree(annotated):
    for case in CASES:
        (k3, g3, _), (k1, g1, _) = annotated[case, 3], annotated[case, 1]
        assert k3 == k1 and g3["letters"] == g1["letters"]
        assert torch.equal(g3["letters_dev"], g1["letters_dev"]) and torch.equal(g3["counts"], g1["counts"]) and torch.equal(g3["status"], g1["status"])
    small, big = annotated["L64", 3], annotated["L512", 3]
    for b, k in enumerate(small[0]):
        j = big[0].index(k)
        assert small[1]["letters"][b] == big[1]["letters"][j] and torch.equal(small[1]["counts"][b], big[1]["counts"][j]), k


def test_two_calls_give_the_same_bits(annotated):
    from text2protein_amd.encode import annotate_sse_batch
    _, first, (xyz, nres, ok) = annotated["L512", 3]
    again = annotate_sse_batch(xyz, nres, atom_ok=ok)
    for name in ("letters_dev", "counts", "status"):
        assert torch.equal(first[name], again[name]), name


def test_holes_and_unusable_coordinates(chains):
    """atom_ok is honoured; a CA that should be there but is NaN, infinite or beyond 1e6 counts as absent and sets status 1."""
    from text2protein_amd.encode import annotate_sse_batch
    x, ok, o = chains["hole"]
    n = x.shape[0]
    whole = S.annotate(x)
    assert whole["letters"] != o["letters"]
    xyz = torch.from_numpy(x)[None].repeat(6, 1, 1, 1)
    flags = torch.ones(6, n, 3, dtype=torch.uint8)
    flags[1] = torch.from_numpy(ok)
    xyz[2, 9, 1, 0] = float("nan")
    xyz[3, 9, 1, 2] = float("inf")
    xyz[4, 9, 1, 1] = -1.0e7
    xyz[5, 9, 1, 1] = 1.0e6                                  # not beyond: the residue stays, far from everything
    xyz[1, 9, 1] = float("nan")                               # marked absent: whatever it holds is not looked at
    xyz[:, :, 0] = xyz[:, :, 2] = float("nan")                # N and C are not read
    got = annotate_sse_batch(xyz.cuda(), torch.full((6,), n), atom_ok=flags.cuda())
    far = x.copy()
    far[9, 1, 1] = 1.0e6
    want = [whole, o, o, o, o, S.annotate(far)]
    assert got["status"].cpu().tolist() == [0, 0, 1, 1, 1, 0]
    for b in range(6):
        assert got["letters"][b] == want[b]["letters"] and got["counts"][b].cpu().tolist() == want[b]["counts"], b
    assert got["counts"][:, 9].cpu().tolist() == [0, 1, 1, 1, 1, 0]
    # a hole in a bare CA trace, flags given as (B, L)
    ca = torch.from_numpy(np.ascontiguousarray(x[:, 1]))[None].cuda()
    got = annotate_sse_batch(ca, torch.tensor([n]), atom_ok=torch.from_numpy(np.ascontiguousarray(ok[:, 1]))[None])
    assert got["letters"] == [o["letters"]]


def test_lengths_out_of_range_and_guarded_buffers(chains):
    """len = 0 and len > L give status -1, zero letters and zero counts, and leave the other chains alone; every output element is
    written and nothing next to the outputs is: the three outputs lie inside larger buffers filled with a sentinel."""
    from text2protein_amd import _lib
    lib = _lib.load()
    keys, L, G = ["hlh", "hole", "run5", "n1"], 50, 64
    xyz, nres, ok = _batch(chains, keys + ["hlh", "hlh"], L, 3)
    nres[4], nres[5] = 0, L + 1
    B = 6
    target = torch.full((B, L), ord("a"), dtype=torch.uint8).cuda()
    letters = torch.full((B * L + 2 * G,), 0xAB, dtype=torch.uint8).cuda()
    counts = torch.full((B * 12 + 2 * G,), -77, dtype=torch.int32).cuda()
    status = torch.full((B + 2 * G,), -77, dtype=torch.int32).cuda()
    rc = lib.t2p_op_annotate_sse(_lib.ptr(xyz), _lib.ptr(nres), _lib.ptr(ok), B, L, 3, _lib.ptr(target), _lib.ptr(letters[G:]), _lib.ptr(counts[G:]),
                                 _lib.ptr(status[G:]), _lib.stream_ptr())
    torch.cuda.synchronize()
    assert rc == 0, lib.t2p_last_error()
    lt, ct, st = letters.cpu().numpy(), counts.cpu().numpy(), status.cpu().numpy()
    for buf, size, fill in ((lt, B * L, 0xAB), (ct, B * 12, -77), (st, B, -77)):
        assert (buf[:G] == fill).all() and (buf[G + size:] == fill).all()
    lt, ct, st = lt[G:G + B * L].reshape(B, L), ct[G:G + B * 12].reshape(B, 12), st[G:G + B]
    assert st.tolist() == [0, 0, 0, 0, -1, -1]
    assert (lt[4:] == 0).all() and (ct[4:] == 0).all()
    for b, k in enumerate(keys):
        o = chains[k][2]
        n = len(o["letters"])
        assert bytes(lt[b, :n]).decode() == o["letters"] and (lt[b, n:] == 0).all(), k
        na = o["letters"].count("a")
        assert ct[b].tolist() == o["counts"][:5] + [n, na, 0, 0] + o["counts"][9:], k          # the target is all a


def test_agreement_counts_equal_numpys(chains):
    """A target that differs from the annotation: the chain's own letters moved by three residues, and every b run turned into a."""
    from text2protein_amd.encode import annotate_sse_batch
    from text2protein_amd.fold import ss_agreement
    keys = ["hlh", "n512", "near", "fold96"]
    xyz, nres, _ = _batch(chains, keys, 512, 1)
    targets = []
    for k in keys:
        lt = chains[k][2]["letters"]
        targets.append(("ccc" + lt)[:len(lt)] if k != "near" else lt.replace("b", "a"))
    got = annotate_sse_batch(xyz, nres, target=targets)
    rows = ss_agreement(xyz, nres, targets)
    for b, k in enumerate(keys):
        lt, t = np.array(list(chains[k][2]["letters"])), np.array(list(targets[b]))
        want = [int((t == "a").sum()), int(((t == "a") & (lt == "a")).sum()), int((t == "b").sum()), int(((t == "b") & (lt == "b")).sum())]
        assert want == S.annotate(chains[k][0], target=targets[b])["counts"][5:9]
        c = got["counts"][b].cpu().tolist()
        print(f"{k}: target a {want[0]} hit {want[1]}, target b {want[2]} hit {want[3]}")
        assert c[5:9] == want and c[:5] + c[9:] == chains[k][2]["counts"][:5] + chains[k][2]["counts"][9:], k
        r = rows[b]
        assert r["letters"] == "".join(lt) and r["target"] == targets[b] and r["counts"]["target_a_hit"] == want[1]
        assert r["helix_agreement"] == (want[1] / want[0] if want[0] else None)
        assert r["strand_agreement"] == (want[3] / want[2] if want[2] else None)
    assert rows[2]["strand_agreement"] is None and rows[2]["helix_agreement"] == 0.0 and rows[3]["strand_agreement"] is None
    assert 0.0 < rows[0]["helix_agreement"] < 1.0 and 0.0 < rows[0]["strand_agreement"] < 1.0
    # a target given as a tensor of letters is the same thing
    t = torch.zeros(4, 512, dtype=torch.uint8)
    for b, s in enumerate(targets):
        t[b, :len(s)] = torch.from_numpy(np.frombuffer(s.encode(), np.uint8).copy())
    assert torch.equal(annotate_sse_batch(xyz, nres, target=t.cuda())["counts"], got["counts"])


def test_encode_with_psea_equals_encode_with_the_oracles_letters(chains):
    from text2protein_amd.encode import encode_6d_batch, sse_blocks, sse_target
    keys = ["hlh", "hole", "fold48", "n4"]
    xyz, nres, ok = _batch(chains, keys, 64, 3)
    xyz = torch.nan_to_num(xyz, nan=0.0)                     # the encoder reads all three atoms; the padding stays zero
    letters = [chains[k][2]["letters"] for k in keys]
    a = encode_6d_batch(xyz, nres, atom_ok=ok, sse="psea", num_channels=8)
    b = encode_6d_batch(xyz, nres, atom_ok=ok, sse=letters, num_channels=8)
    assert torch.equal(a["coords_6d"], b["coords_6d"]) and torch.equal(a["mask_pair"], b["mask_pair"])
    assert a["ss_indices"] == b["ss_indices"] == [sse_blocks(s)[1] for s in letters] and a["ss_indices"][0].count(":") >= 3
    assert a["coords_6d"][:, 4:7].abs().sum() > 0
    # the target read back from the channels: the blocks, half-open, c at a residue the pair mask removes
    t = sse_target(a["coords_6d"])
    want = list("c" * len(letters[0]))
    for s, l, kind in sse_blocks(letters[0])[0]:
        want[s:l] = "ab"[kind] * (l - s)
    assert t[0] == "".join(want) and [len(s) for s in t] == [len(s) for s in letters]
    assert t[1][8:11] == "ccc" and "aaa" in t[1]           # the residue without a CA and its two neighbours are masked out
    with pytest.raises(ValueError, match="one per sample"):
        encode_6d_batch(xyz, nres, atom_ok=ok, sse="pse", num_channels=8)
    with pytest.raises(ValueError, match="8-channel"):
        encode_6d_batch(xyz, nres, atom_ok=ok, sse="psea", num_channels=5)


def test_conditions_from_pdb_with_psea(chains, tmp_path):
    """The repository's test PDB (8 residues, all c), and the helix-loop-hairpin fixture written out as a PDB file."""
    from text2protein_amd.conditions import get_conditions_from_pdb
    from text2protein_amd.config import tiny_config
    from text2protein_amd.encode import read_backbone
    from text2protein_amd.fold import write_backbone_pdb
    write_backbone_pdb(tmp_path / "hlh.pdb", chains["hlh"][0])
    for path, L in ((PDB, 16), (str(tmp_path / "hlh.pdb"), 64)):
        cfg = tiny_config(**{"model.condition": ["length", "ss", "inpainting"], "data.num_channels": 8, "data.max_res_num": L})
        cfg.device = "cuda:0"
        xyz, ok, n = read_backbone(path)
        o = S.annotate(xyz, ok)
        print(os.path.basename(path), o["letters"], "margin", o["margin"])
        assert o["margin"] >= 1e-4 and (L == 16 or o["letters"] == chains["hlh"][2]["letters"])
        a = get_conditions_from_pdb(path, cfg, mask_info="1:5", batch_size=2, sse="psea", with_batch=True)
        b = get_conditions_from_pdb(path, cfg, mask_info="1:5", batch_size=2, sse=o["letters"], with_batch=True)
        assert set(a) == set(b) == {"length", "ss", "inpainting", "_batch"}
        assert torch.equal(a["ss"], b["ss"]) and torch.equal(a["length"], b["length"]) and (L == 16) == (float(a["ss"].abs().sum()) == 0)
        assert torch.equal(a["inpainting"]["coords_6d"], b["inpainting"]["coords_6d"]) and torch.equal(a["_batch"]["coords_6d"], b["_batch"]["coords_6d"])
        with pytest.raises(ValueError, match="--sse"):        # no letters and no request for them: today's refusal
            get_conditions_from_pdb(path, cfg, sse=None)


def test_folded_chain_end_to_end(chains):
    """Exact maps of a fixture chain -> fold -> annotate the GPU's backbone; the oracle runs on that same fp32 backbone."""
    from text2protein_amd.encode import annotate_sse_batch, encode_6d_batch
    from text2protein_amd.fold import fold_6d_batch, ss_agreement
    keys = ["fold48", "fold96cut"]
    xyz, nres, _ = _batch(chains, keys, 48, 3)
    r = fold_6d_batch(encode_6d_batch(xyz, nres)["coords_6d"])
    assert r["status"].cpu().tolist() == [0, 0] and r["lengths"].tolist() == [48, 37]
    got = annotate_sse_batch(r["xyz"], r["lengths"])
    back = r["xyz"].cpu().numpy()
    truth = [chains[k][2]["letters"] for k in keys]
    rows = ss_agreement(r["xyz"], r["lengths"], truth)
    for b, k in enumerate(keys):
        n = int(r["lengths"][b])
        o = S.annotate(back[b, :n])
        print(f"{k} folded: margin of the oracle on the GPU's backbone {o['margin']:.3e}; letters {o['letters']} (true chain {truth[b]}), "
              f"helix agreement {rows[b]['helix_agreement']}")
        assert o["margin"] >= 1e-9, "a condition on the input: a quantity of the folded backbone lies on a threshold"
        assert got["letters"][b] == o["letters"] and got["counts"][b].cpu().tolist() == o["counts"] and int(got["status"][b]) == 0
        assert rows[b]["letters"] == o["letters"] and rows[b]["strand_agreement"] is None


def _cli_cfg(tmp_path):
    from text2protein_amd.config import tiny_config
    cfg = tiny_config(**{"model.num_scales": 4, "model.condition": ["length", "ss", "inpainting"], "data.num_channels": 8})
    path = tmp_path / "tiny_ss.yml"
    with open(path, "w") as f:
        yaml.safe_dump(yaml.safe_load(json.dumps(cfg)), f)
    return [sys.executable, os.path.join(ROOT, "sampling_6d.py"), str(path), "synthetic", "--batch_size", "2", "--dtype", "f32", "--context_tokens", "4",
            "--seed", "5", "--pdb", PDB, "--sse", "psea", "--mask_info", "1:5", "--outdir", str(tmp_path / "out")]


def test_cli_ss_check_writes_the_sse_block(tmp_path):
    """--pdb with --sse psea builds the 8-channel condition with no letters supplied; --ss_check (which implies --fold) reports."""
    from text2protein_amd.encode import COUNT_NAMES
    r = subprocess.run(_cli_cfg(tmp_path) + ["--ss_check", "--refine"], capture_output=True, text=True, timeout=600, cwd=str(tmp_path))
    assert r.returncode == 0, r.stdout + r.stderr
    for i in (0, 1):
        with open(tmp_path / "out" / f"fold_{i}.json") as f:
            d = json.load(f)
        assert d["L"] == 8 and set(d["sse"]) == {"folded", "refined"} and "refine" in d
        for row in d["sse"].values():
            assert len(row["letters"]) == 8 == len(row["target"]) and set(row["letters"]) <= set("abc") and row["status"] in (0, 1)
            assert tuple(row["counts"]) == COUNT_NAMES and sum(row["counts"][k] for k in "abc") == 8
            assert row["counts"]["target_a"] == row["target"].count("a") and row["counts"]["target_b"] == row["target"].count("b")
            assert (row["helix_agreement"] is None) == (row["counts"]["target_a"] == 0)
            assert (row["strand_agreement"] is None) == (row["counts"]["target_b"] == 0)
        assert f"sample {i}: secondary structure folded:" in r.stdout


def test_cli_without_ss_check_writes_no_sse_block(tmp_path):
    r = subprocess.run(_cli_cfg(tmp_path) + ["--fold"], capture_output=True, text=True, timeout=600, cwd=str(tmp_path))
    assert r.returncode == 0, r.stdout + r.stderr
    for i in (0, 1):
        with open(tmp_path / "out" / f"fold_{i}.json") as f:
            d = json.load(f)
        assert d["L"] == 8 and "sse" not in d
    assert "secondary structure" not in r.stdout
