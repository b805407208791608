"""TM-align's host side without a GPU: the float64 oracle (tests/tmalign_oracle.py) against what the reference's own TM-align printed
for every pair of tests/golden/tmalign_pairs.npz, at the bounds the GPU test holds the kernel to; that the seeds after the second
matter; what the fixture was built to contain; the checks tmalign.py makes before the native call; ``--tm_ref``'s argument handling."""
import json
import os
import re
import subprocess
import sys

import numpy as np
import pytest
import torch

import tmalign_oracle as O
from helpers import load_golden

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
N_PAIRS = 17


@pytest.fixture(scope="module")
def gold():
    g = load_golden("tmalign_pairs")
    g["meta"] = json.loads(str(g["meta"]))
    return g


def _ca(gold, name):
    return gold["xyz_" + name][:, 1].astype(np.float64)          # float32 widened: what the GPU gets


def test_fixture_holds_what_it_was_built_for(gold):
    m = gold["meta"]
    pairs = m["pairs"]
    assert len(pairs) == m["kept"] == N_PAIRS and m["candidates"] == m["kept"] + len(m["rejected"])
    assert 10 * len(m["rejected"]) <= m["candidates"]
    lens = [(p["len_a"], p["len_b"]) for p in pairs]
    assert any(a == b for a, b in lens), "a pair of equal lengths (the symmetric branch of get_initial_fgt)"
    assert any(min(a, b) == 8 for a, b in lens) and any(max(a, b) > 3 * min(a, b) for a, b in lens)
    assert {160, 210, 256} <= {n for ab in lens for n in ab}
    assert {p["seed"] for p in pairs} >= {0, 2, 3, 4}, "final alignments from the seeds past the second"
    # the chain break of the copy with a deletion: wider than find_max_frag's 4.25 A, so its longest fragment is not the chain
    x = _ca(gold, "132del")
    assert np.linalg.norm(x[1:] - x[:-1], axis=1).max() > 4.25
    s, e = O.find_max_frag(x)
    assert e - s + 1 < len(x)
    for name in m["chains"]:                       # rounded to 3 decimals, then to float32: the PDB text describes the same chain
        v = gold["xyz_" + name]
        assert v.dtype == np.float32
        assert (np.abs(v.astype(np.float64) - np.round(v.astype(np.float64), 3)) <= 0.5 * np.spacing(np.abs(v)).astype(np.float64)).all()


@pytest.mark.parametrize("p", range(N_PAIRS))
def test_oracle_reproduces_tm_align(gold, p):
    pair = gold["meta"]["pairs"][p]
    o = O.tm_align(_ca(gold, pair["a"]), _ca(gold, pair["b"]))
    tm_a, tm_b, rmsd, n8 = gold[f"ref_scalars_{p}"]
    print(pair["a"], pair["b"], "oracle", o["tm_a"], o["tm_b"], o["rmsd"], o["n_ali8"], "TM-align", tm_a, tm_b, rmsd, n8)
    assert abs(o["tm_a"] - tm_a) <= 1e-5 and abs(o["tm_b"] - tm_b) <= 1e-5
    assert o["n_ali8"] == int(n8) and np.array_equal(o["b2a"], gold[f"ref_b2a_{p}"])
    assert abs(o["rmsd"] - rmsd) <= 5e-3
    assert np.abs(np.concatenate([o["t"], o["u"].reshape(-1)]) - gold[f"ref_rot_{p}"]).max() <= 1e-4
    # and the record of the oracle the GPU test compares with is this oracle's
    got = np.array([o["tm_a"], o["tm_b"], o["rmsd"], o["n_ali8"], o["d0_a"], o["d0_b"], o["tm_max"], o["seed"]])
    assert np.abs(got - gold[f"orc_out8_{p}"]).max() <= 1e-9 and np.array_equal(o["b2a"], gold[f"orc_b2a_{p}"])


def test_the_later_seeds_matter(gold):
    """With get_initial5, get_initial_ssplus and get_initial_fgt switched off the score falls short of TM-align's on a pair whose final
    alignment came from one of them."""
    short = []
    for p, pair in enumerate(gold["meta"]["pairs"]):
        if (pair["a"], pair["b"]) in (("160", "132"), ("96", "256")):
            o = O.tm_align(_ca(gold, pair["a"]), _ca(gold, pair["b"]), seeds=("gl", "ss"))
            short.append(float(gold[f"ref_scalars_{p}"][1]) - o["tm_b"])
    print("TM-align minus the two-seed oracle:", short)
    assert len(short) == 2 and max(short) > 1e-3


def test_kabsch_is_a_rotation():
    rng = np.random.default_rng(0)
    x = rng.normal(0, 10, (20, 3))
    R = np.linalg.qr(rng.normal(size=(3, 3)))[0]
    R *= np.sign(np.linalg.det(R))
    y = x @ R.T + np.array([1.0, -2.0, 3.0])
    _, t, u = O.kabsch(x, y)
    assert np.abs(u - R).max() < 1e-9 and np.abs(x @ u.T + t - y).max() < 1e-8
    assert O.kabsch(x, y, mode=0)[0] < 1e-6


# ---- the host side of text2protein_amd/tmalign.py ----
def test_symbols_are_declared():
    from text2protein_amd import _lib
    header = open(os.path.join(ROOT, "include", "t2p.h")).read()
    for name, nargs in (("t2p_op_tm_align_ws", 3), ("t2p_op_tm_align", 19)):
        assert name in _lib.SIGNATURES and len(_lib.SIGNATURES[name][1]) == nargs
        decl = re.search(r"^int(?:64_t)? " + name + r"\(([^;]*)\);", header, re.M)
        assert decl and decl.group(1).count(",") == nargs - 1
    src = open(os.path.join(ROOT, "text2protein_amd", "csrc", "t2p_kernels.h")).read()
    assert re.search(r"constexpr int TM_MAX_L = 256;", src)
    from text2protein_amd import build, tmalign
    assert "tmalign.hip" in build.SOURCES and tmalign.TM_MAX_L == 256


def test_unusable_coordinates_are_refused_by_the_kernel_and_its_loops_are_bounded():
    """A non-finite coordinate makes every distance NaN, which no cut of TM-align's relaxation loops admits.  The kernel refuses such a
    pair as it loads the traces (one workgroup-wide vote) and caps the three loops besides; the header says so.  Read from the source:
    the GPU test feeds such input to the kernel only because both are in place."""
    src = open(os.path.join(ROOT, "text2protein_amd", "csrc", "tmalign.hip")).read()
    assert src.count("if (!(fabsf(v) <= TM_MAX_COORD)) usable = 0;") == 2 and "if (!__syncthreads_and(usable)) {" in src
    assert "while (true)" not in src.replace("while (true) {                                         // score_fun8's relaxation of the cut", "")
    for cap in ("relax < TM_CAP_FAST", "inc < TM_CAP_FUN8", "inc <= TM_CAP_FRAG"):
        assert cap in src, cap
    header = open(os.path.join(ROOT, "include", "t2p.h")).read()
    assert "is not finite or exceeds" in header and "t2p_debug_tm_align_info" in header and "t2p_op_tm_align_info" not in header


def test_host_checks_raise_before_the_native_call():
    from text2protein_amd import tmalign as T
    from text2protein_amd._lib import T2PError
    x = torch.zeros(2, 10, 3, 3)
    n = torch.tensor([10, 10])
    with pytest.raises(ValueError, match="torch tensor"):
        T.tm_align_batch(np.zeros((2, 10, 3, 3)), n, x, n)
    with pytest.raises(ValueError, match="N / CA / C"):
        T.tm_align_batch(torch.zeros(2, 10, 2, 3), n, x, n)
    with pytest.raises(ValueError, match="N / CA / C"):
        T.tm_align_batch(torch.zeros(2, 10, 3, 4), n, x, n)
    with pytest.raises(ValueError, match="floating-point"):
        T.tm_align_batch(torch.zeros(2, 10, 3, 3, dtype=torch.int32), n, x, n)
    with pytest.raises(ValueError, match="TM_MAX_L"):
        T.tm_align_batch(torch.zeros(1, 257, 3), torch.tensor([257]), x, n)
    with pytest.raises(T2PError, match="GPU"):                     # a tensor off the device is refused, not copied or scored on the CPU
        T.tm_align_batch(x, n, x, n)
    with pytest.raises(T2PError, match="GPU"):
        T.pairwise_tm(x, n)


def test_reference_files(tmp_path):
    from text2protein_amd.tmalign import reference_files
    d = tmp_path / "refs"
    d.mkdir()
    for name in ("b.pdb", "a.PDB", "notes.txt"):
        (d / name).write_text("END\n")
    one = tmp_path / "one.pdb"
    one.write_text("END\n")
    assert reference_files([str(one), str(d)]) == [str(one), str(d / "a.PDB"), str(d / "b.pdb")]
    empty = tmp_path / "empty"
    empty.mkdir()
    for bad, what in ((str(tmp_path / "none.pdb"), "no such file"), (str(empty), "no .pdb file"), (str(d / "notes.txt"), "not a .pdb file")):
        with pytest.raises(ValueError, match=what):
            reference_files([bad])


def test_cli_refuses_a_missing_reference_before_the_device(tmp_path):
    cmd = [sys.executable, os.path.join(ROOT, "sampling_6d.py"), os.path.join(ROOT, "configs", "cond_length.yml"), "synthetic", "--tm_ref",
           str(tmp_path / "missing.pdb")]
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=300, cwd=str(tmp_path))
    assert r.returncode != 0 and "--tm_ref" in r.stderr and "no such file or directory" in r.stderr, r.stdout + r.stderr
    assert not os.listdir(tmp_path)
