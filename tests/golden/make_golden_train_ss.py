"""Golden fixtures of the TRAINING STEP under the `ss` condition WITH secondary-structure block dropout, produced by the reference's own
`block_dropout` and autograd through the REFERENCE UNetModel (build container only).

    python tests/golden/make_golden_train_ss.py

The cases (tests/ss_train_cases.py) are train_tinyB / train_tinyB_vp -- configuration, seed, inputs -- plus `batch["ss_indices"]`.  The
reference's `losses.block_dropout` (losses.py:54-64) is CALLED, not restated: score_sde_pytorch/losses.py imports `biotite.structure` at
module level and never uses it in the functions taken here, so an empty stand-in module is registered under that name for the import
when the package is not installed.  Procedure: `random.seed(py_seed)`, `block_dropout` on a clone of coords_6d (it zeroes its argument
in place, :61-62); the seed is replayed to record the per-block decisions in the reference's draw order (:55-58); then the step body of
make_golden_train_sde.reference_step (losses.py:105-134, :41-49 as written there) runs on the dropped coordinates.  Stored: what the
train_tinyB* fixtures store, plus one JSON record: the strings, the Python seed, the block list, the decisions and the dropped coords_6d
as the count of changed elements and the SHA-256 of its bytes (it is rebuilt from the regenerated input, the blocks and the decisions).
Only data is written; no reference source text goes into the repo.
"""
import hashlib
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

from helpers import load_golden, train_inputs, projection              # noqa: E402
from ss_train_cases import BLOCK_DROPOUT, SS_TRAIN_CASES               # noqa: E402
from make_golden_train import FULL_TENSORS                             # noqa: E402
from make_golden_train_sde import T_MIN, reference_step                # noqa: E402

try:
    import biotite.structure                                           # noqa: F401
except ImportError:                  # the import line of the reference's losses.py only: nothing taken from it below touches biotite
    _pkg, _sub = types.ModuleType("biotite"), types.ModuleType("biotite.structure")
    _pkg.structure = _sub
    sys.modules["biotite"], sys.modules["biotite.structure"] = _pkg, _sub
from score_sde_pytorch import losses as ref_losses                     # noqa: E402  (reference)


def fixture(name):
    case = SS_TRAIN_CASES[name]
    cfg = case["config"]()
    assert "ss" in cfg.model.condition
    inp = train_inputs(cfg, case)
    assert float(inp["t"].min()) >= T_MIN
    ss, seed = case["ss_indices"], case["py_seed"]
    assert len(ss) == case["B"] and "" in ss
    # ---- the reference's own block_dropout, on a clone (it mutates its argument) -----------------------------------------
    dropped = inp["coords_6d"].clone()
    random.seed(seed)
    out = ref_losses.block_dropout(dropped, ss)
    assert out is dropped
    # ---- replay of the seed: one random.random() per block, samples in order, blocks in string order, none for '' ---------
    random.seed(seed)
    blocks, decisions = [], []
    for idx in range(len(ss)):
        if ss[idx] == "":
            continue
        for rng in ss[idx].split(","):
            a, b = [int(v) for v in rng.split(":")]
            blocks.append((idx, a, b))
            decisions.append(random.random() < BLOCK_DROPOUT)
    # the replay is the reference's sequence: zeroing by the recorded decisions gives the tensor block_dropout returned
    again = inp["coords_6d"].clone()
    for (idx, a, b), d in zip(blocks, decisions):
        if d:
            again[idx, 4:7, :, a:b] = 0
            again[idx, 4:7, a:b, :] = 0
    assert torch.equal(again, dropped)
    assert any(decisions) and not all(decisions), "choose a py_seed that drops some blocks and keeps some"
    lengths = case["lengths"]
    assert any(d and a < lengths[idx] for (idx, a, b), d in zip(blocks, decisions)), "no dropped block overlaps mask_pair's valid region"
    assert not torch.equal(dropped, inp["coords_6d"])
    r = reference_step(cfg, case, dict(inp, coords_6d=dropped))
    base = load_golden(case["base"])
    print(f"[{name}] blocks {blocks}, dropped {[int(d) for d in decisions]}; loss {float(r['loss']):.6g} (without block dropout: "
          f"{float(base['loss']):.6g}); {int((dropped != inp['coords_6d']).sum())} elements zeroed", flush=True)
    assert float(r["loss"]) != float(base["loss"]) and np.isfinite(float(r["loss"]))
    names = r["names"]
    full = [n for n in FULL_TENSORS if n in r["grads"]]
    # the dropped coords_6d is stored sparsely: it is the input with the dropped blocks zeroed, so the record holds the blocks, the
    # decisions, how many elements changed their bits and the SHA-256 of the tensor's bytes (ss_train_cases.dropped_coords rebuilds it
    # and checks both)
    changed = int((dropped.numpy().view(np.int32) != inp["coords_6d"].numpy().view(np.int32)).sum())
    record = dict(ss_indices=list(ss), py_seed=int(seed), block_dropout=BLOCK_DROPOUT, blocks=[list(b) for b in blocks],
                  decisions=[int(d) for d in decisions], changed=changed, sha256=hashlib.sha256(dropped.numpy().tobytes()).hexdigest())
    g = {"loss": np.float64(r["loss"]), "score": r["score"].float().numpy(), "names": np.array(names), "n_dropout_calls": np.int64(r["n_drop"]),
         "ss": np.array(json.dumps(record))}
    if case["sde"] == "vp":          # what train_tinyB_vp.npz holds besides
        g.update({"t": r["t"].numpy(), "labels": r["labels"].numpy(), "mean_coef": r["mean_coef"].float().numpy(), "std": r["std"].float().numpy(),
                  "score_std": r["score_std"].float().numpy(), "sqrt_1m_alphas_cumprod": r["sde"].sqrt_1m_alphas_cumprod.float().numpy()})
    for key in ("grads", "post", "ema", "m", "v"):
        g[key + "_norm"] = np.array([float(r[key][n].double().norm()) for n in names])
        g[key + "_proj"] = np.array([projection(n, r[key][n]) for n in names])
    for n in full:
        g["grad:" + n] = r["grads"][n].numpy()
        g["post:" + n] = r["post"][n].numpy()
    g["grad_total_norm"] = np.float64(float(torch.sqrt(sum((v.double() ** 2).sum() for v in r["grads"].values()))))
    # the .npz container written member by member at the highest deflate level (np.savez_compressed's level is fixed at the default)
    with zipfile.ZipFile(os.path.join(HERE, name + ".npz"), "w", zipfile.ZIP_DEFLATED, compresslevel=9) as zf:
        for key, val in g.items():
            buf = io.BytesIO()
            np.lib.format.write_array(buf, np.asanyarray(val), allow_pickle=False)
            zf.writestr(key + ".npy", buf.getvalue())


if __name__ == "__main__":
    torch.set_num_threads(int(os.environ.get("T2P_GOLDEN_THREADS", "2")))
    for nm in (sys.argv[1:] or list(SS_TRAIN_CASES)):
        fixture(nm)
