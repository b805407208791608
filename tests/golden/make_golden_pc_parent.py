"""Record what the sampler's element-wise tail computes, bit for bit, at the commit before the plain and the guided update kernels
(and the DDIM update's quad loop) were folded into one set.

    python tests/golden/make_golden_pc_parent.py <commit hash> [output.npz]

Needs a GPU and the library built from that commit; reads no reference code.  Writes tests/golden/pc_update_parent.npz: every entry
of tests/pc_parent_cases.py's compute() -- the norm sums of t2p_op_langevin_norms / t2p_op_guided_langevin_norms, x and x_mean of
five short PCStepper runs, one t2p_sampler_run under the VP SDE and two fused DDIM runs -- and the commit hash.  The inputs are
regenerated on both sides (an integer hash, device Philox noise), so only outputs are stored.  Also prints the dispatches one PC step
of each run enqueues.
"""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]

import pc_parent_cases as P                                 # noqa: E402


def main():
    commit = sys.argv[1]
    path = sys.argv[2] if len(sys.argv) > 2 else os.path.join(HERE, "pc_update_parent.npz")
    dispatches = {}
    out = P.compute(dispatches)
    for k, v in out.items():
        assert np.isfinite(v).all(), k
        print(f"{k}: shape {v.shape}, |max| {float(np.abs(v).max()):.6g}")
    for k, n in dispatches.items():
        print(f"dispatches per PC step, {k}: {n}")
    np.savez_compressed(path, commit=np.array(commit), **out)
    print(f"wrote {path} ({os.path.getsize(path)} bytes, {len(out)} entries) at commit {commit}")


if __name__ == "__main__":
    main()
