"""Golden fixtures of the RANDOM INPAINTING MASK of training, produced by the reference's own ``random_mask_batch`` (utils.py:15-60;
build container only).

    python tests/golden/make_golden_train_inpaint.py

The reference's ``utils.py`` is imported with empty stand-in modules registered under the names it imports at module level and never
uses in the function taken here (``biotite*``, ``dataset``: the route make_golden_encode.py takes).  ``random_mask_batch`` is CALLED,
not restated, on train_tinyB's geometry (tests/inpaint_cases.py: B = 3, N = 16, 16 / 11 / 6 valid residues, the shipped
probabilities) after ``random.seed(s); torch.manual_seed(s)`` for s = 0 .. 11.  The seed is replayed to record which branch the single
``random.random()`` took.

Written:
  inpaint_masks.npz                        the twelve (B, N, N) bool masks, the mode of each (0 none, 1 random, 2 contiguous), the seeds,
                                           the lengths and the torch version that drew them
  train_tinyB_inpaintdraw_rand.npz         the reference's loss, score, gradients and post-step state on train_tinyB's inputs with the
  train_tinyB_inpaintdraw_contig.npz       mask of one random / one contiguous seed in place of train_tinyB's mask_info mask: the step
                                           body of make_golden_train_sde.reference_step, stored the way make_golden_train_ss.py stores
Asserted: all three modes occur, one sample of one random mask has no masked residue (num_elem = 0), every mask is the OR of a
residue mask with itself.  The seeds are not asserted.  Only data is written; no reference source text goes into the repo.
"""
import io
import json
import os
import random
import sys
import types
import zipfile

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, HERE)
sys.path.insert(0, "/root/reference")

from helpers import load_golden, train_inputs, projection                                              # noqa: E402
from inpaint_cases import (INPAINT_TRAIN_CASES, INPAINTING, LENGTHS, MODE_CONTIGUOUS, MODE_NONE, MODE_RANDOM, SEEDS,   # noqa: E402
                           cfg_inpaint)
from make_golden_train import FULL_TENSORS                                                             # noqa: E402
from make_golden_train_sde import reference_step                                                       # noqa: E402

for _name in ("biotite", "biotite.structure", "biotite.structure.io", "dataset"):
    if _name not in sys.modules:
        sys.modules[_name] = types.ModuleType(_name)
sys.modules["biotite"].structure = sys.modules["biotite.structure"]
sys.modules["biotite.structure"].io = sys.modules["biotite.structure.io"]
for _attr in ("load_structure", "save_structure"):
    if not hasattr(sys.modules["biotite.structure.io"], _attr):
        setattr(sys.modules["biotite.structure.io"], _attr, None)
for _attr in ("ProteinDataset", "PaddingCollate"):
    if not hasattr(sys.modules["dataset"], _attr):
        setattr(sys.modules["dataset"], _attr, None)
import utils as ref_utils                                                                               # noqa: E402  (reference)


def reference_mask(seed):
    """(mask (B, N, N) bool, mode) of the reference's random_mask_batch under random.seed(seed); torch.manual_seed(seed)."""
    cfg = cfg_inpaint()
    cfg.device = "cpu"
    N = cfg.data.max_res_num
    batch = {"coords_6d": torch.zeros(len(LENGTHS), cfg.data.num_channels, N, N), "aa_str": ["A" * l + "_" * (N - l) for l in LENGTHS]}
    random.seed(seed)
    torch.manual_seed(seed)
    out = ref_utils.random_mask_batch(batch, cfg)
    assert out is batch and out["mask_inpaint"].dtype == torch.bool and tuple(out["mask_inpaint"].shape) == (len(LENGTHS), N, N)
    random.seed(seed)
    prob = random.random()                                   # the replay: which branch utils.py:30 / :42 took
    mode = MODE_RANDOM if prob < INPAINTING["random_mask_prob"] else MODE_CONTIGUOUS if prob > 1 - INPAINTING["contiguous_mask_prob"] else MODE_NONE
    return out["mask_inpaint"], mode


def write_npz(path, g):
    # the .npz container member by member at the highest deflate level (np.savez_compressed's level is fixed at the default)
    with zipfile.ZipFile(path, "w", zipfile.ZIP_DEFLATED, compresslevel=9) as zf:
        for key, val in g.items():
            buf = io.BytesIO()
            np.lib.format.write_array(buf, np.asanyarray(val), allow_pickle=False)
            zf.writestr(key + ".npy", buf.getvalue())


def masks_fixture():
    masks, modes = [], []
    for s in SEEDS:
        m, mode = reference_mask(s)
        res = torch.diagonal(m, dim1=1, dim2=2)                      # m[b, i, i] = the residue flag
        assert torch.equal(m, res[:, :, None] | res[:, None, :])
        if mode == MODE_NONE:
            assert bool(m.all())
        else:
            assert all(not bool(res[b, l:].any()) for b, l in enumerate(LENGTHS))      # no padding residue is ever drawn
        masks.append(m.numpy())
        modes.append(mode)
        print(f"seed {s}: mode {mode}, masked residues per sample {[int(v) for v in res.sum(1)]}", flush=True)
    assert set(modes) == {MODE_NONE, MODE_RANDOM, MODE_CONTIGUOUS}, "all three modes must occur: extend SEEDS"
    empty = [(s, b) for s, m, mode in zip(SEEDS, masks, modes) if mode != MODE_NONE for b in range(len(LENGTHS)) if not m[b].any()]
    assert empty, "no sample without a masked residue (the num_elem = 0 edge): extend SEEDS"
    print("samples without a masked residue (seed, sample):", empty)
    write_npz(os.path.join(HERE, "inpaint_masks.npz"),
              {"masks": np.stack(masks), "modes": np.array(modes, dtype=np.int64), "seeds": np.array(SEEDS, dtype=np.int64),
               "lengths": np.array(LENGTHS, dtype=np.int64), "inpainting": np.array(json.dumps(INPAINTING)),
               "torch_version": np.array(torch.__version__)})
    return dict(zip(SEEDS, zip(masks, modes)))


def step_fixture(name, drawn):
    case = INPAINT_TRAIN_CASES[name]
    cfg = case["config"]()
    inp = train_inputs(cfg, case)
    mask, mode = drawn[case["mask_seed"]]
    assert mode == case["mask_mode"], f"seed {case['mask_seed']} draws mode {mode}: choose another mask_seed for {name}"
    mask = torch.from_numpy(mask)
    assert not torch.equal(mask, inp["mask_inpaint"]) and all(bool(mask[b].any()) for b in range(case["B"]))
    r = reference_step(cfg, case, dict(inp, mask_inpaint=mask))
    base = load_golden(case["base"])
    print(f"[{name}] mask of seed {case['mask_seed']} (mode {mode}); loss {float(r['loss']):.6g} (train_tinyB's own mask: {float(base['loss']):.6g})",
          flush=True)
    assert float(r["loss"]) != float(base["loss"]) and np.isfinite(float(r["loss"]))
    names = r["names"]
    full = [n for n in FULL_TENSORS if n in r["grads"]]
    g = {"loss": np.float64(r["loss"]), "score": r["score"].float().numpy(), "names": np.array(names), "n_dropout_calls": np.int64(r["n_drop"]),
         "mask_inpaint": mask.numpy(), "mask_seed": np.int64(case["mask_seed"]), "mask_mode": np.int64(mode)}
    for key in ("grads", "post", "ema", "m", "v"):
        g[key + "_norm"] = np.array([float(r[key][n].double().norm()) for n in names])
        g[key + "_proj"] = np.array([projection(n, r[key][n]) for n in names])
    for n in full:
        g["grad:" + n] = r["grads"][n].numpy()
        g["post:" + n] = r["post"][n].numpy()
    g["grad_total_norm"] = np.float64(float(torch.sqrt(sum((v.double() ** 2).sum() for v in r["grads"].values()))))
    write_npz(os.path.join(HERE, name + ".npz"), g)


if __name__ == "__main__":
    torch.set_num_threads(int(os.environ.get("T2P_GOLDEN_THREADS", "2")))
    drawn = masks_fixture()
    for nm in (sys.argv[1:] or list(INPAINT_TRAIN_CASES)):
        step_fixture(nm, drawn)
