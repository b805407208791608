"""Host half of the secondary-structure annotation (t2p_op_annotate_sse, text2protein_amd/encode.py): the float64 oracle
(tests/sse_oracle.py) against the recorded fixtures (tests/golden/sse_chains.npz, written by tests/golden/make_golden_sse.py), the
properties the GPU test relies on, the declaration of the entry point and the refusals that need no GPU."""
import ctypes as C
import json
import os
import re

import numpy as np
import pytest
import torch

import sse_oracle as S
from helpers import GOLDEN, load_golden

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PDB = os.path.join(GOLDEN, "encode_chain.pdb")
# what a prototype of the specification gave for two chains of tests/golden/fold_chains.npz (read there, not copied)
FOLD_CHAINS = {"48": "ccccccccccccccccccccaaaaaaaccccccccccccccccccccc", "96cut": "caaaaaaaaacccccccccccaaaaaaaaaaaaaacc"}


@pytest.fixture(scope="module")
def gold():
    g = load_golden("sse_chains")
    g["meta"] = json.loads(str(g["meta"]))
    return g


@pytest.fixture(scope="module")
def annotated(gold):
    return {k: S.annotate(gold[f"xyz_{k}"], gold.get(f"atom_ok_{k}")) for k in gold["meta"]["keys"]}


def test_oracle_reproduces_the_recorded_letters(gold, annotated):
    meta = gold["meta"]
    assert set(meta["keys"]) >= {"hlh", "near", "far", "run5", "run4", "ext", "hole", "n1", "n2", "n3", "n4", "n512"} and meta["margin"] == 1e-4
    for key, rep in meta["chains"].items():
        xyz, o = gold[f"xyz_{key}"], annotated[key]
        assert xyz.shape[0] == rep["n"] == len(rep["letters"]) and np.array_equal(np.round(xyz, 3), xyz), key
        assert o["letters"] == rep["letters"] and o["counts"] == rep["counts"] and o["status"] == 0, key
        assert sum(rep["counts"][:3]) == rep["n"] and rep["counts"][5:9] == [0, 0, 0, 0] and rep["counts"][10:] == [0, 0], key
        assert rep["n"] == 1 or o["margin"] >= 1e-4, (key, o["margin"])           # no label sits on an edge
        # fp32 rounding of the inputs moves no label
        assert S.annotate(xyz.astype(np.float32), gold.get(f"atom_ok_{key}"))["letters"] == rep["letters"], key
    ch = meta["chains"]
    assert "aaaa" in ch["hlh"]["letters"] and "bbbb" in ch["hlh"]["letters"] and 40 <= ch["hlh"]["n"] <= 60
    assert ch["n512"]["n"] == 512 and ch["n512"]["counts"][3] >= 5 and ch["n512"]["counts"][4] >= 5
    assert all(ch[f"n{k}"]["letters"] == "c" * k for k in (1, 2, 3, 4))


def test_fixtures_show_each_rule(gold, annotated):
    ch = gold["meta"]["chains"]
    # the contact rule: the same 3-residue potential run is b beside the strand and c 15 A further away
    near, far = annotated["near"], annotated["far"]
    run = [10, 11, 12]
    for o in (near, far):
        ps = o["potential_strand"]
        assert ps[run].all() and not ps[9] and not ps[13:].any()
    assert near["letters"][10:13] == "bbb" and far["letters"][10:13] == "ccc"
    assert int(near["contacts"][run].sum()) >= 5 > int(far["contacts"][run].sum())
    assert np.array_equal(gold["xyz_near"][:9], gold["xyz_far"][:9])
    moved = np.linalg.norm(gold["xyz_far"][9:] - gold["xyz_near"][9:], axis=1)
    assert np.abs(moved - 15.0).max() < 2e-3
    # exactly 5 potential-helix residues are a core, exactly 4 are not
    assert ch["run5"]["potential_helix"] == [6, 7, 8, 9, 10] and ch["run5"]["letters"] == "cccccc" + "aaaaa" + "cccccc"
    assert ch["run4"]["potential_helix"] == [6, 7, 8, 9] and set(ch["run4"]["letters"]) == {"c"}
    # one residue per end: taken in before the core (r in range, not potential itself), refused after it
    o = annotated["ext"]
    assert ch["ext"]["potential_helix"] == list(range(6, 12)) and o["letters"][4:14] == "c" + "a" * 7 + "cc"
    assert S.R_HELIX[0] <= o["q"][5, 3] <= S.R_HELIX[1] and not S.R_HELIX[0] <= o["q"][12, 3] <= S.R_HELIX[1]
    # a residue without a CA is c, and takes the quantities that name it with it
    o, whole = annotated["hole"], S.annotate(gold["xyz_hole"])
    assert gold["atom_ok_hole"][9, 1] == 0 and gold["atom_ok_hole"].sum() == 59
    assert whole["letters"][5:14] == "a" * 9 and o["letters"][9] == "c" and o["counts"][9] == 1 and "aaaa" in o["letters"]
    assert np.isnan(o["q"][9, 3]) and np.isnan(o["q"][10]).all() and not np.isnan(o["q"][9, 1])      # d3[9] names residues 8 and 11 only
    junk = gold["xyz_hole"].copy()
    junk[9, 1] = 999.0                                       # whatever the coordinates of the missing atom hold
    assert S.annotate(junk, gold["atom_ok_hole"])["letters"] == o["letters"]


def test_oracle_gives_the_prototypes_letters_on_the_fold_chains():
    g = load_golden("fold_chains")
    for key, letters in FOLD_CHAINS.items():
        for dtype in (np.float64, np.float32):
            o = S.annotate(g[f"xyz_{key}"].astype(dtype))
            assert o["letters"] == letters and o["margin"] >= 1e-4, key
    for key in ("96", "132"):
        o = S.annotate(g[f"xyz_{key}"])
        assert o["margin"] >= 1e-4 and "b" not in o["letters"] and "aaaa" in o["letters"]


def test_oracle_is_invariant_under_a_rigid_motion(gold, annotated):
    rng = np.random.default_rng(5)
    q, _ = np.linalg.qr(rng.normal(size=(3, 3)))
    if np.linalg.det(q) < 0:
        q[:, 0] = -q[:, 0]                                  # a proper rotation: a mirror image would flip the dihedral's sign
    for key in ("hlh", "near", "far", "ext", "hole", "n512"):
        moved = gold[f"xyz_{key}"] @ q.T + np.array([11.0, -7.0, 23.0])
        o = S.annotate(moved, gold.get(f"atom_ok_{key}"))
        assert o["letters"] == annotated[key]["letters"] and o["counts"] == annotated[key]["counts"], key
        assert abs(o["margin"] - annotated[key]["margin"]) < 1e-9
    mirror = S.annotate(gold["xyz_run5"] * np.array([1.0, 1.0, -1.0]))
    assert "a" not in mirror["letters"]                      # a left-handed helix has a near -50


def test_ideal_helix_and_strand_traces():
    i = np.arange(24)
    helix = np.stack([2.3 * np.cos(np.radians(100.0) * i), 2.3 * np.sin(np.radians(100.0) * i), 1.5 * i], axis=1)
    o = S.annotate(helix)
    a = o["q"][1:-2, 4]
    print("ideal alpha helix: dihedral", a.min(), "to", a.max(), "angle", o["q"][1:-1, 3].mean(), "d3", o["q"][1:-2, 1].mean(), "d4", o["q"][1:-3, 2].mean())
    assert np.abs(a - 50.0).max() < 3.0 and o["letters"] == "c" + "a" * 22 + "c"
    # a twisted strand: 3.3 A rise per residue, alternating sides, a slow turn about the axis
    strand = np.stack([0.9 * np.cos(np.radians(175.0) * i), 0.9 * np.sin(np.radians(175.0) * i), 3.3 * i], axis=1)
    o = S.annotate(strand)
    # a strand end is taken in on d3 alone, which the last two residues do not have
    assert o["letters"] == "c" + "b" * 21 + "cc" and o["counts"][4] == 1
    # a target: the agreement counts
    t = "c" + "a" * 10 + "b" * 5 + "c" * 8
    o = S.annotate(helix, target=t)
    assert o["counts"][5:9] == [10, 10, 5, 0]


def test_blocks_of_the_oracles_letters(gold, annotated):
    from text2protein_amd.encode import sse_blocks
    for key, rep in gold["meta"]["chains"].items():
        blocks, text = sse_blocks(annotated[key]["letters"])
        assert text == rep["blocks"], key
        assert sum(k == 0 for _, _, k in blocks) == rep["counts"][3] and sum(k == 1 for _, _, k in blocks) == rep["counts"][4], key
    assert gold["meta"]["chains"]["hlh"]["blocks"].count(":") >= 3


def test_symbol_is_declared_and_bound():
    from text2protein_amd import _lib, build, encode
    hdr = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "t2p.h")).read(), flags=re.S)
    m = re.search(r"^int t2p_op_annotate_sse\(([^;]*)\);", hdr, re.M)
    assert m and len(m.group(1).split(",")) == 11 == len(_lib.SIGNATURES["t2p_op_annotate_sse"][1])
    assert hdr.index("t2p_op_encode_6d(") < hdr.index("t2p_op_annotate_sse(") < hdr.index("t2p_op_fold_ws(")
    assert "sse.hip" in build.SOURCES and hasattr(_lib.load(), "t2p_op_annotate_sse")
    src = open(os.path.join(ROOT, "text2protein_amd", "csrc", "t2p_kernels.h")).read()
    assert "constexpr int SSE_MAX_L = FOLD_MAX_L;" in src and "FOLD_MAX_L = 512;" in src and encode.SSE_MAX_L == 512


def test_refusals_come_before_the_device_is_touched():
    """Every argument check of the entry point precedes its only launch; the pointers below are never followed."""
    from text2protein_amd import _lib
    lib = _lib.load()
    buf = (C.c_uint8 * 64)()
    p = C.cast(buf, C.c_void_p)
    good = dict(xyz=p, len=p, atom_ok=None, batch=1, L=8, atoms=3, target=None, letters=p, counts=p, status=p, stream=None)
    cases = [({"L": 0}, r"\[1, 512\]"), ({"L": 513}, r"\[1, 512\]"), ({"atoms": 2}, "atoms must be 1"), ({"atoms": 0}, "atoms must be 1"),
             ({"batch": 0}, "batch"), ({"batch": -3}, "batch")] + [({k: None}, "null") for k in ("xyz", "len", "letters", "counts", "status")]
    for change, message in cases:
        args = dict(good, **change)
        assert lib.t2p_op_annotate_sse(*args.values()) == 1, change
        assert re.search(message, lib.t2p_last_error().decode()), (change, lib.t2p_last_error())


def test_python_refusals_need_no_gpu():
    from text2protein_amd._lib import T2PError
    from text2protein_amd.conditions import get_conditions_from_pdb
    from text2protein_amd.config import tiny_config
    from text2protein_amd.encode import annotate_sse_batch, encode_6d_batch, sse_target
    with pytest.raises(T2PError, match="no CPU fallback"):
        annotate_sse_batch(torch.zeros(1, 8, 3, 3), torch.tensor([8]))
    with pytest.raises(T2PError, match="no CPU fallback"):
        annotate_sse_batch(torch.zeros(1, 8, 3), torch.tensor([8]))
    with pytest.raises(ValueError, match="SSE_MAX_L"):
        annotate_sse_batch(torch.zeros(1, 513, 3), torch.tensor([513]))
    for shape in ((1, 8, 2, 3), (1, 8, 4), (8, 3)):
        with pytest.raises(ValueError, match="CA trace"):
            annotate_sse_batch(torch.zeros(*shape), torch.tensor([8]))
    # "psea" on a 5-channel model is refused like any other letters; any other bare string keeps its ValueError
    with pytest.raises(ValueError, match="8-channel"):
        get_conditions_from_pdb(PDB, tiny_config(), sse="psea")
    with pytest.raises(ValueError, match="--sse"):
        get_conditions_from_pdb(PDB, tiny_config(**{"data.num_channels": 8}))
    with pytest.raises(T2PError, match="no CPU fallback"):
        encode_6d_batch(torch.zeros(1, 8, 3, 3), torch.tensor([8]), sse="psea", num_channels=8)
    # the target letters of an 8-channel condition: half-open blocks, so a block's last residue is c
    x = torch.zeros(2, 8, 12, 12)
    x[0, 7, :10, :10] = 1
    x[0, 4, 1:5, 1:5] = 1
    x[0, 5, 6:9, 6:9] = 0.9
    x[1, 7, :3, :3] = 1
    assert sse_target(x) == ["caaaacbbbc", "ccc"] and sse_target(x[0]) == ["caaaacbbbc"]
    with pytest.raises(ValueError, match="8-channel"):
        sse_target(torch.zeros(1, 5, 4, 4))
