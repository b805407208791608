"""Host half of the 6D encode (text2protein_amd/encode.py): the block finder, the PDB backbone reader and the refusals that need no
GPU, against tests/golden/encode_6d.npz / encode_chain.pdb (tests/golden/make_golden_encode.py: the reference's own featuriser)."""
import json
import os

import numpy as np
import pytest

import geom_oracle as GO
from helpers import GOLDEN, load_golden

PDB = os.path.join(GOLDEN, "encode_chain.pdb")


@pytest.fixture(scope="module")
def gold():
    g = load_golden("encode_6d")
    g["meta"] = json.loads(str(g["meta"]))
    return g


def test_sse_blocks_give_the_references_strings(gold):
    from text2protein_amd.encode import BETA, HELIX, sse_blocks
    for key, rep in gold["meta"]["chains"].items():
        blocks, text = sse_blocks(rep["sse"])
        assert text == rep["ss_indices"], key
        assert [k for _, _, k in blocks] == sorted(k for _, _, k in blocks)          # helices first
        assert all(rep["sse"][s:l + 1] == ("a" if k == HELIX else "b") * (l - s + 1) and l - s + 1 >= 4 for s, l, k in blocks)
    # a 3-long run is no block; a block may end at the last residue; an empty annotation gives the empty string
    assert sse_blocks("cbbbccaaaa") == ([(6, 9, HELIX)], "6:9")
    assert sse_blocks("bbbbcaaa") == ([(0, 3, BETA)], "0:3")
    assert sse_blocks("aaaabbbbaaaa") == ([(0, 3, HELIX), (8, 11, HELIX), (4, 7, BETA)], "0:3,8:11,4:7")
    assert sse_blocks("cccc") == ([], "") and sse_blocks("") == ([], "")
    assert any(rep["sse"].endswith("aaaa") or rep["sse"].endswith("bbbb") for rep in gold["meta"]["chains"].values())
    assert "cbbbc" in gold["meta"]["chains"]["19"]["sse"] and "4:" not in gold["meta"]["chains"]["19"]["ss_indices"].split(",")[-1]
    with pytest.raises(ValueError):
        sse_blocks("aaaaH")


def test_read_backbone_returns_the_fixture_chain(gold, tmp_path):
    from text2protein_amd.encode import read_backbone
    want = gold["xyz_8"].astype(np.float32)
    xyz, ok, n = read_backbone(PDB)
    assert n == 8 and xyz.dtype == np.float32 and ok.dtype == np.uint8
    assert np.array_equal(xyz, want) and ok.all()
    lines = open(PDB).read().splitlines()
    atoms = [i for i, l in enumerate(lines) if l.startswith("ATOM")]
    # one CA line removed: the residue stays, its flag is cleared, its coordinates are the origin
    ca = [i for i in atoms if lines[i][12:16] == " CA " and int(lines[i][22:26]) == 4][0]
    p = tmp_path / "no_ca.pdb"
    p.write_text("\n".join(lines[:ca] + lines[ca + 1:]) + "\n")
    xyz2, ok2, n2 = read_backbone(str(p))
    w2, k2 = want.copy(), np.ones((8, 3), np.uint8)
    w2[3, 1], k2[3, 1] = 0, 0
    assert n2 == 8 and np.array_equal(xyz2, w2) and np.array_equal(ok2, k2)
    # a second chain, hetero records of a ligand and of water, an alternate location: all filtered out
    extra = [l[:21] + "B" + l[22:] for l in (lines[i] for i in atoms[:6])]
    extra += ["HETATM  900 CA    CA A 101       1.000   2.000   3.000  1.00  0.00          CA",
              "HETATM  901  O   HOH A 102       4.000   5.000   6.000  1.00  0.00           O"]
    alt = lines[atoms[1]][:16] + "B" + lines[atoms[1]][17:30] + "   9.000   9.000   9.000" + lines[atoms[1]][54:]
    p = tmp_path / "two_chains.pdb"
    p.write_text("\n".join(lines[:atoms[1] + 1] + [alt] + lines[atoms[1] + 1:atoms[-1] + 1] + extra + ["END"]) + "\n")
    xyz3, ok3, n3 = read_backbone(str(p), chain="A")
    assert n3 == 8 and np.array_equal(xyz3, want) and ok3.all()
    xyz4, _, n4 = read_backbone(str(p), chain="B")
    assert n4 == 2 and np.array_equal(xyz4, want[:2])
    # two MODELs: refused, as the reference skips such a file
    p = tmp_path / "two_models.pdb"
    body = [lines[i] for i in atoms]
    p.write_text("\n".join(["MODEL        1"] + body + ["ENDMDL", "MODEL        2"] + body + ["ENDMDL", "END"]) + "\n")
    with pytest.raises(ValueError, match="MODEL"):
        read_backbone(str(p))
    p = tmp_path / "one_model.pdb"
    p.write_text("\n".join(["MODEL        1"] + body + ["ENDMDL", "END"]) + "\n")
    assert np.array_equal(read_backbone(str(p))[0], want)
    with pytest.raises(ValueError, match="no residues"):
        read_backbone(PDB, chain="Z")


def test_conditions_from_pdb_refusals_need_no_gpu():
    """The checks that come before the device is touched: chain length against the configuration, --sse with 8 channels."""
    from text2protein_amd.conditions import get_conditions_from_pdb
    from text2protein_amd.config import tiny_config
    with pytest.raises(ValueError, match="min_res_num"):
        get_conditions_from_pdb(PDB, tiny_config(**{"data.min_res_num": 9}))
    with pytest.raises(ValueError, match="max_res_num"):
        get_conditions_from_pdb(PDB, tiny_config(**{"data.max_res_num": 7}))
    with pytest.raises(ValueError, match="--sse"):
        get_conditions_from_pdb(PDB, tiny_config(**{"data.num_channels": 8}))
    with pytest.raises(ValueError, match="8 residues"):
        get_conditions_from_pdb(PDB, tiny_config(**{"data.num_channels": 8}), sse="caaaa")


def test_encode_has_no_cpu_path():
    import torch
    from text2protein_amd._lib import T2PError
    from text2protein_amd.encode import encode_6d_batch
    with pytest.raises(T2PError, match="no CPU fallback"):
        encode_6d_batch(torch.zeros(1, 8, 3, 3), torch.tensor([8]))


def test_fixture_conditions_hold(gold):
    """What the GPU test relies on to compare every pixel, re-derived from the stored float64 arrays."""
    meta = gold["meta"]
    assert set(meta["keys"]) == {"8", "19", "40", "64", "40cut", "64cut"} and meta["cut"] == 37
    gap = gold["ref_f32_gap"]
    assert gap.shape == (4,) and (gap > 0).all() and (gap < 1e-4).all()
    ones = zeros = 0
    for key in meta["keys"]:
        xyz, ok, c, mp = gold[f"xyz_{key}"], gold[f"atom_ok_{key}"], gold[f"coords_6d_{key}"], gold[f"mask_pair_{key}"]
        rep = meta["chains"][key]
        n = xyz.shape[0]
        assert c.shape == (8, n, n) and mp.shape == (n, n) and np.array_equal(np.round(xyz, 3), xyz) and len(rep["sse"]) == n
        assert rep["cut_margin"] >= 1e-3 and rep["adj_margin"] >= 1e-3 and rep["shortest_projection"] >= 1e-2
        bb = xyz * ok[:, :, None]
        cb = GO.virtual_cb(bb[:, 0], bb[:, 1], bb[:, 2])
        d = np.linalg.norm(cb[:, None] - cb[None, :], axis=-1)
        off = ~np.eye(n, dtype=bool)
        assert np.abs(d[off] - 20.0).min() >= 1e-3
        m = mp != 0
        assert np.array_equal(c[7], mp) and (c[:, ~m] == 0).all()
        far = m & ((d > 20.0) | ~off)
        assert (c[0][far] == 1).all() and (c[1][far] == 0).all() and (c[2][far] == 0).all() and (c[3][far] == -1).all()
        near = m & ~far
        assert np.abs((c[0][near] + 1) * 10 - d[near]).max() < 1e-9
        assert set(np.unique(c[4:7])) <= {0.0, 1.0}
        ones += int(c[6].sum())
        zeros += sum(v > 5.0 for v in rep["adjacency_minima"])
    assert ones > 0 and zeros > 0                       # the adjacency channel holds both
    k19 = gold["atom_ok_19"]
    assert k19[0, 0] == 0 and k19[9, 1] == 0 and k19[18, 2] == 0 and k19.sum() == 19 * 3 - 3
    res = np.ones(19, bool)
    res[[0, 1, 8, 9, 10, 17, 18]] = False               # the rolling mask of dataset.py:209-218
    assert np.array_equal(gold["mask_pair_19"] != 0, res[:, None] & res[None, :])
