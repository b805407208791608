#!/usr/bin/env python3
"""ms per secondary-structure annotation (t2p_op_annotate_sse, text2protein_amd/encode.py) next to the ms of the fold call, same process.

    python tools/bench_sse.py [--runs 5] [--out profiles/sse_cond_length.json]

Two shapes: 32 chains at L = 128 (copies of the committed 132-residue chain of tests/golden/fold_chains.npz cut to 128 residues -- the
chains tools/bench_fold.py folds) and one batch of 32 chains at L = 512 (copies of the 512-residue chain of tests/golden/sse_chains.npz).
Timed between device events, median of --runs calls after one untimed call: ``sse`` = t2p_op_annotate_sse alone on outputs allocated
beforehand (one launch, nothing read back), ``sse_with_letters`` = annotate_sse_batch (allocations, the launch, the letters read back to
strings), ``fold`` = t2p_op_fold_6d on the L = 128 batch (fold_maps_batch, as in bench_fold.py).  One workgroup per chain: 32 workgroups on
256 compute units, so the annotation is bound by the latency of one workgroup's five phases, not by throughput.  There is
no pass mark.  One JSON line; bench.py is not touched.
"""
import argparse
import json
import os
import statistics
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--runs", type=int, default=5)
    ap.add_argument("--batch", type=int, default=32)
    ap.add_argument("--out", default="")
    args = ap.parse_args()

    from text2protein_amd import _lib
    from text2protein_amd.decode import decode_6d_batch
    from text2protein_amd.encode import annotate_sse_batch, encode_6d_batch
    from text2protein_amd.fold import fold_maps_batch

    dev = torch.device("cuda:0")
    torch.cuda.set_device(dev)
    lib = _lib.load()
    B = args.batch
    golden = os.path.join(ROOT, "tests", "golden")
    chains = {128: np.load(os.path.join(golden, "fold_chains.npz"))["xyz_132"][:128], 512: np.load(os.path.join(golden, "sse_chains.npz"))["xyz_n512"]}
    ev0, ev1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)

    def timed(fn):
        fn()
        torch.cuda.synchronize()
        ms = []
        for _ in range(args.runs):
            ev0.record()
            out = fn()
            ev1.record()
            torch.cuda.synchronize()
            ms.append(ev0.elapsed_time(ev1))
        return ms, out

    out = {"what": "ms per secondary-structure annotation (P-SEA, one workgroup per chain) next to ms per fold call, same process",
           "chains": B, "device": torch.cuda.get_device_name(0), "runs": args.runs}
    for L, truth in chains.items():
        xyz = torch.from_numpy(truth).float().unsqueeze(0).repeat(B, 1, 1, 1).to(dev).contiguous()
        n = torch.full((B,), L, dtype=torch.int32, device=dev)
        letters = torch.empty(B, L, device=dev, dtype=torch.uint8)
        counts = torch.empty(B, 12, device=dev, dtype=torch.int32)
        status = torch.empty(B, device=dev, dtype=torch.int32)

        def op():
            _lib.check(lib.t2p_op_annotate_sse(_lib.ptr(xyz), _lib.ptr(n), None, B, L, 3, None, _lib.ptr(letters), _lib.ptr(counts), _lib.ptr(status),
                                               _lib.stream_ptr()))

        op_ms, _ = timed(op)
        whole_ms, r = timed(lambda: annotate_sse_batch(xyz, n))
        c = counts[0].cpu().tolist()
        out[f"L{L}"] = {"sse_ms": round(statistics.median(op_ms), 4), "sse_ms_runs": [round(v, 4) for v in op_ms],
                        "sse_with_letters_ms": round(statistics.median(whole_ms), 4), "sse_with_letters_ms_runs": [round(v, 4) for v in whole_ms],
                        "residues_a_b_c": c[:3], "blocks_a_b": c[3:5], "status": sorted(set(status.cpu().tolist())),
                        "same_letters": bool(torch.equal(r["letters_dev"], letters) and len(set(r["letters"])) == 1)}
        if L == 128:
            samples = encode_6d_batch(xyz, n)["coords_6d"]
            lengths, _, absval = decode_6d_batch(samples)
            fold_ms, _ = timed(lambda: fold_maps_batch(absval, lengths))
            out["fold_ms"] = round(statistics.median(fold_ms), 4)
            out["fold_ms_runs"] = [round(v, 4) for v in fold_ms]
            out["sse_over_fold"] = round(statistics.median(op_ms) / statistics.median(fold_ms), 4)
    print(json.dumps(out), flush=True)
    if args.out:
        with open(args.out, "w") as f:
            json.dump(out, f, indent=1)
            f.write("\n")


if __name__ == "__main__":
    main()
