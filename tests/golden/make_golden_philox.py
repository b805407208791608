"""Record what t2p_op_philox_normal draws, bit for bit, at the commit before the generator moved into csrc/philox.h.

    python tests/golden/make_golden_philox.py <commit hash> [output.npz]

Needs a GPU and the library built from that commit.  Writes tests/golden/philox_parent.npz: the n = 4099 normals of the three
(seed, stream) cases of tests/test_gpu_philox.py (step word 0), their seeds and streams, and the commit hash.  Also prints the
largest difference from the numpy restatement (oracle/philox.py), the measurement behind that test's bound.
"""
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)

from oracle import philox                                   # noqa: E402
from text2protein_amd import _lib                           # noqa: E402

N = 4099                   # not a multiple of 4 (the scalar tail runs), more than one workgroup of 256 quads
CASES = {                  # name -> (seed, stream)
    "small": (1234, 1),
    "high_seed": (0xC0FFEE1234567890, 7),
    "wrapped_stream": (42, 5),           # the test also draws stream 5 + 2^32: the same bits (the stream word is 32 bits wide)
}


def draw(seed, stream, n=N):
    out = torch.empty(n, device="cuda", dtype=torch.float32)
    _lib.check(_lib.load().t2p_op_philox_normal(_lib.ptr(out), n, seed, stream, None))
    torch.cuda.synchronize()
    return out.cpu().numpy()


def main():
    commit = sys.argv[1]
    path = sys.argv[2] if len(sys.argv) > 2 else os.path.join(HERE, "philox_parent.npz")
    out = {"commit": np.array(commit), "n": np.int64(N)}
    for name, (seed, stream) in CASES.items():
        z = draw(seed, stream)
        err = float(np.abs(z.astype(np.float64) - philox.normals(seed, stream, 0, N)).max())
        print(f"[{name}] seed {seed:#x} stream {stream}: max |device - restatement| = {err:.3e}, mean {z.mean():+.4f}, std {z.std():.4f}")
        out[name] = z
        out[name + "_seed"] = np.uint64(seed)
        out[name + "_stream"] = np.uint64(stream)
    np.savez_compressed(path, **out)
    print(f"wrote {path} ({os.path.getsize(path)} bytes) at commit {commit}")


if __name__ == "__main__":
    main()
