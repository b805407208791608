"""Golden fixture of the TRAINING STEP with text-context dropout, produced by autograd through the REFERENCE UNetModel (build container
only).

    python tests/golden/make_golden_train_ctxdrop.py

The reference's loss has no context dropout; what a dropped sample must compute is defined by the guided samplers, which evaluate the
network on ``context * 0``.  So the fixture is the reference's own step (make_golden_train_sde.reference_step: losses.py:105-134, :41-49
as written there) on train_tinyB's configuration, seed and inputs with the context rows of the dropped samples set to zero
(tests/ctxdrop_cases.py: decisions [1, 0, 1], what ``random.seed(3)`` gives for three ``random.random() < 0.5``).  Stored: what
train_tinyB.npz stores, plus one JSON record with p, the Python seed, the decisions and the two measured conditions below.

The generator refuses to write unless the fixture can tell the feature from its absence:
  * the loss differs from train_tinyB's by more than 100 LOSS_TOL relative;
  * the score of sample 1 (kept) is bit-equal to train_tinyB's and the score of sample 0 (dropped) is not.
Only data is written; no reference source text goes into the repo.
"""
import io
import json
import os
import random
import sys
import zipfile

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, HERE)

from helpers import load_golden, train_inputs, projection               # noqa: E402
from ctxdrop_cases import CTXDROP_CASES, zeroed_context                 # noqa: E402
from make_golden_train import FULL_TENSORS                              # noqa: E402
from make_golden_train_sde import reference_step                        # noqa: E402  (imports the reference)

LOSS_TOL = 1e-5          # test_gpu_train.py's


def fixture(name):
    case = CTXDROP_CASES[name]
    cfg = case["config"]()
    inp = train_inputs(cfg, case)
    p, seed, decisions = case["p"], case["py_seed"], case["decisions"]
    random.seed(seed)
    assert [int(random.random() < p) for _ in range(case["B"])] == decisions, "py_seed does not give the case's decisions"
    assert any(decisions) and not all(decisions)
    ctx = zeroed_context(inp["context"], decisions)
    assert not torch.equal(ctx, inp["context"])
    r = reference_step(cfg, case, dict(inp, context=ctx))
    base = load_golden(case["base"])
    loss, base_loss = float(r["loss"]), float(base["loss"])
    loss_rel = abs(loss - base_loss) / abs(base_loss)
    score, base_score = r["score"].float().numpy(), base["score"]
    kept = [b for b, d in enumerate(decisions) if not d]
    dropped = [b for b, d in enumerate(decisions) if d]
    kept_diff = max(float(np.abs(score[b] - base_score[b]).max()) for b in kept)
    kept_bits = all(np.array_equal(score[b].view(np.int32), base_score[b].view(np.int32)) for b in kept)
    dropped_diff = min(float(np.abs(score[b] - base_score[b]).max()) for b in dropped)
    print(f"[{name}] decisions {decisions}; loss {loss:.6g} (train_tinyB: {base_loss:.6g}, rel {loss_rel:.3e}, bound {100 * LOSS_TOL:.0e}); score: "
          f"kept samples max |diff| {kept_diff:.3g} (bit-equal: {kept_bits}), dropped samples' smallest max |diff| {dropped_diff:.3g}", flush=True)
    assert np.isfinite(loss) and loss_rel > 100 * LOSS_TOL, "the loss does not tell a step without the dropout apart"
    assert kept_bits and dropped_diff > 0, "kept samples must score as in train_tinyB, dropped ones must not"
    names = r["names"]
    full = [n for n in FULL_TENSORS if n in r["grads"]]
    record = dict(p=p, py_seed=int(seed), decisions=[int(d) for d in decisions], loss_rel_to_base=loss_rel, kept_score_max_diff=kept_diff,
                  dropped_score_max_diff=dropped_diff)
    g = {"loss": np.float64(r["loss"]), "score": score, "names": np.array(names), "n_dropout_calls": np.int64(r["n_drop"]),
         "ctxdrop": np.array(json.dumps(record))}
    for key in ("grads", "post", "ema", "m", "v"):
        g[key + "_norm"] = np.array([float(r[key][n].double().norm()) for n in names])
        g[key + "_proj"] = np.array([projection(n, r[key][n]) for n in names])
    for n in full:
        g["grad:" + n] = r["grads"][n].numpy()
        g["post:" + n] = r["post"][n].numpy()
    g["grad_total_norm"] = np.float64(float(torch.sqrt(sum((v.double() ** 2).sum() for v in r["grads"].values()))))
    with zipfile.ZipFile(os.path.join(HERE, name + ".npz"), "w", zipfile.ZIP_DEFLATED, compresslevel=9) as zf:
        for key, val in g.items():
            buf = io.BytesIO()
            np.lib.format.write_array(buf, np.asanyarray(val), allow_pickle=False)
            zf.writestr(key + ".npy", buf.getvalue())


if __name__ == "__main__":
    torch.set_num_threads(int(os.environ.get("T2P_GOLDEN_THREADS", "2")))
    for nm in (sys.argv[1:] or list(CTXDROP_CASES)):
        fixture(nm)
