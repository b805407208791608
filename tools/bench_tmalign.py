#!/usr/bin/env python3
"""ms per TM-align call (text2protein_amd/tmalign.py) for the scoring a 32-chain run asks for, next to one PC step and to the
reference's own TM-align on CPU cores.

    python tools/bench_tmalign.py [--runs 5] [--pc_steps 10] [--out profiles/tmalign_cond_length.json]

Workload: 32 folded synthetic chains of 128 residues against 100 reference chains of 40 to 128 residues (3200 pairs, one
``tm_align_batch`` call) plus the 496 alignments of the chains against each other (one ``pairwise_tm`` call).  The chains are windows of
the committed compact synthetic chains (tests/golden/tmalign_pairs.npz: 132, 160, 210 and 256 residues); the 32 samples are encoded
and folded on the device first, so they are what ``fold_6d_batch`` leaves there.  Timed between device events, median of --runs calls
after one untimed call, with the range.

The bar is the reference's one-process-per-pair TM-align on 16 CPU cores: tmalign_pairs.npz records the binary's
wall time per fixture pair (g++ -O3, process start included) on the CPU-only build machine; a least-squares line ms = c0 + c1 La Lb
through those pairs gives the time of each pair of this workload, their sum is divided by 16.  The two figures come from different
machines.  The PC step is the one bench.py measures for configs/cond_length.yml, in the same process.  One JSON line; bench.py is not
touched.
"""
import argparse
import ctypes as C
import json
import os
import statistics
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def windows(gold, rng, count, lo, hi):
    """`count` windows of lo..hi residues cut from the fixture's long chains."""
    out = []
    names = ("132", "160", "210", "256")
    for k in range(count):
        x = gold["xyz_" + names[k % len(names)]]
        n = int(rng.integers(lo, hi + 1))
        at = int(rng.integers(0, x.shape[0] - n + 1))
        out.append(x[at:at + n])
    return out


def padded(chains, L, dev):
    xyz = torch.full((len(chains), L, 3, 3), float("nan"))
    for b, x in enumerate(chains):
        xyz[b, :len(x)] = torch.from_numpy(np.ascontiguousarray(x))
    return xyz.to(dev), torch.tensor([len(x) for x in chains], dtype=torch.int32)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--runs", type=int, default=5)
    ap.add_argument("--pc_steps", type=int, default=10)
    ap.add_argument("--dtype", default="f16", choices=["f32", "bf16", "f16"])
    ap.add_argument("--cpu_cores", type=int, default=16)
    ap.add_argument("--out", default="")
    args = ap.parse_args()

    from text2protein_amd import _lib, sampling, sde_lib, synth
    from text2protein_amd.conditions import synthetic_condition
    from text2protein_amd.config import load_config
    from text2protein_amd.encode import encode_6d_batch
    from text2protein_amd.fold import fold_6d_batch
    from text2protein_amd.model import HipScoreModel
    from text2protein_amd.tmalign import pairwise_tm, tm_align_batch

    dev = torch.device("cuda:0")
    torch.cuda.set_device(dev)
    B, L, R = 32, 128, 100
    gold = dict(np.load(os.path.join(ROOT, "tests", "golden", "tmalign_pairs.npz")))
    meta = json.loads(str(gold["meta"]))
    rng = np.random.default_rng(0)
    truth, n_truth = padded(windows(gold, rng, B, L, L), L, dev)
    folded = fold_6d_batch(encode_6d_batch(truth, n_truth)["coords_6d"])
    sx, sn = folded["xyz"], torch.as_tensor(folded["lengths"], dtype=torch.int32)
    refs = windows(gold, rng, R, 40, 128)
    rx, rn = padded(refs, L, dev)
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

    ref_ms, r = timed(lambda: tm_align_batch(sx, sn, rx, rn))
    pair_ms, (mat, mean) = timed(lambda: pairwise_tm(sx, sn))
    both = [a + b for a, b in zip(ref_ms, pair_ms)]
    n_pairs = B * R + B * (B - 1) // 2
    # the fold's chains against the chains they were folded from: what the numbers mean
    back = tm_align_batch(sx, sn, truth, n_truth, pairs=torch.arange(B).repeat(2, 1).t().contiguous())

    # the reference's TM-align on CPU cores, scaled from the fixture's recorded wall times
    fx = np.array([[1.0, p["len_a"] * p["len_b"]] for p in meta["pairs"]])
    fy = np.array([p["binary_ms"] for p in meta["pairs"]])
    coef, *_ = np.linalg.lstsq(fx, fy, rcond=None)
    la = sn.numpy().astype(np.float64)
    lb = rn.numpy().astype(np.float64)
    iu = np.triu_indices(B, 1)
    cpu_ms = float((coef[0] + coef[1] * la[:, None] * lb[None]).sum() + (coef[0] + coef[1] * la[iu[0]] * la[iu[1]]).sum())
    fit_resid = float(np.abs(fx @ coef - fy).max())

    info = (C.c_int32 * 4)()
    _lib.check(_lib.load().t2p_debug_tm_align_info(L, L, C.cast(info, C.c_void_p)))
    if info[3] != 0:
        raise SystemExit(f"tm_align_kernel spills {info[3]} bytes per lane to scratch: the figures below would not be the design's")

    cfg = load_config(os.path.join(ROOT, "configs", "cond_length.yml"), **{"data.max_res_num": L, "model.num_scales": 1000})
    cfg.device = str(dev)
    model = HipScoreModel(cfg, dtype=args.dtype, device=str(dev))
    model.load_state_dict(synth.synth_state_dict(cfg, seed=0))
    ctx = synth.synth_context(B, 512, cfg.model.context_dim, seed=1000).to(dev)
    cond = synthetic_condition(cfg, B, "length", dev)
    ve = sde_lib.VESDE(sigma_min=cfg.model.sigma_min, sigma_max=cfg.model.sigma_max, N=cfg.model.num_scales)
    c = cfg.sampling
    pc = sampling.PCStepper(model, ve, B, c.snr, c.n_steps_each, c.probability_flow, c.noise_removal, 1e-5, seed=0)
    x = sampling._device_randn_like(torch.empty(B, cfg.data.num_channels, L, L, device=dev), 12345, 0) * ve.prior_scale()
    x, mask = sampling.apply_conditions(x, cond)
    x = x.float().contiguous()
    pc.set_condition(mask.to(torch.uint8).contiguous(), x.clone())
    mean_x = torch.empty_like(x)
    model.set_context(ctx)
    pc.reset(0)
    for _ in range(3):
        pc.step(x, mean_x)
    torch.cuda.synchronize()
    ev0.record()
    for _ in range(args.pc_steps):
        pc.step(x, mean_x)
    ev1.record()
    torch.cuda.synchronize()
    pc_ms = ev0.elapsed_time(ev1) / args.pc_steps

    gpu_ms = statistics.median(both)
    tm_ref = r["tm_b"].cpu().numpy()
    out = {"what": "ms per TM-align scoring of a 32-chain run (3200 sample-reference pairs + 496 pairwise), next to one PC step (same process) "
                   "and to the reference's TM-align on 16 CPU cores (another machine: scaled from the fixture's recorded wall times)",
           "config": "cond_length.yml", "L": L, "samples": B, "references": R, "reference_lengths": [int(rn.min()), int(rn.max())],
           "pairs": n_pairs, "device": torch.cuda.get_device_name(0), "runs": args.runs,
           "gpu_ms": round(gpu_ms, 3), "gpu_ms_range": [round(min(both), 3), round(max(both), 3)],
           "against_references_ms": round(statistics.median(ref_ms), 3), "against_references_ms_runs": [round(v, 3) for v in ref_ms],
           "pairwise_ms": round(statistics.median(pair_ms), 3), "pairwise_ms_runs": [round(v, 3) for v in pair_ms],
           "pairs_per_second": round(n_pairs / (gpu_ms * 1e-3), 1),
           "pc_step_ms": round(pc_ms, 4), "pc_steps_timed": args.pc_steps, "gpu_ms_over_1000_pc_steps": round(gpu_ms / (1000.0 * pc_ms), 6),
           "cpu_reference": {"fit_ms": {"per_pair": round(float(coef[0]), 4), "per_residue_pair": round(float(coef[1]), 8)},
                             "fit_worst_residual_ms": round(fit_resid, 3), "fixture_pairs": len(fy), "one_core_ms": round(cpu_ms, 1),
                             "cores": args.cpu_cores, "ms": round(cpu_ms / args.cpu_cores, 1),
                             "machine": "the CPU-only build machine (g++ -O3, one process per pair, process start included)"},
           "cpu_over_gpu": round(cpu_ms / args.cpu_cores / gpu_ms, 2),
           "kernel": {"wavefronts": int(info[0]), "lds_bytes": int(info[1]), "registers_per_lane": int(info[2]), "scratch_bytes_per_lane": int(info[3])},
           "status": sorted(set(r["status"].cpu().tolist())), "fold_status": sorted(set(folded["status"].cpu().tolist())),
           "tm_to_references": {"min": round(float(tm_ref.min()), 4), "mean": round(float(tm_ref.mean()), 4), "max": round(float(tm_ref.max()), 4)},
           "tm_fold_to_truth_mean": round(float(torch.maximum(back["tm_a"], back["tm_b"]).mean()), 4),
           "pairwise_mean": round(float(mean), 4),
           "finite": bool(torch.isfinite(r["out8"]).all() and torch.isfinite(mat).all())}
    print(json.dumps(out), flush=True)
    if args.out:
        with open(args.out, "w") as f:
            json.dump(out, f, indent=1)
            f.write("\n")


if __name__ == "__main__":
    main()
