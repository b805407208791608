#!/usr/bin/env python3
"""ms per fold call (text2protein_amd/fold.py) for 32 chains at L = 128, next to the ms of one PC step of the same shapes, same process.

    python tools/bench_fold.py [--runs 5] [--pc_steps 10] [--out profiles/fold_cond_length.json]

The chains are 32 copies of the committed 132-residue compact synthetic chain (tests/golden/fold_chains.npz) cut to 128 residues,
encoded on the device; the fold's run time does not depend on which chain it is given beyond the share of known pairs.  Timed between
device events, median of --runs calls after one untimed call: ``fold`` = t2p_op_fold_6d alone (the five launches), ``decode_and_fold`` =
fold_6d_batch (decode, the lengths' trip to the host and back, fold, diagnostics read back).  The PC step is the one bench.py measures for
configs/cond_length.yml (VE, fused stepper, f16 engine, 512 text tokens, length condition), --pc_steps steps after 3 untimed ones.
There is no pass mark: a 1000-step run is 1000 PC steps, the fold runs once after it.  One JSON line; bench.py is not touched.
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
    ap.add_argument("--pc_steps", type=int, default=10)
    ap.add_argument("--dtype", default="f16", choices=["f32", "bf16", "f16"])
    ap.add_argument("--out", default="")
    args = ap.parse_args()

    from text2protein_amd import sampling, sde_lib, synth
    from text2protein_amd.conditions import synthetic_condition
    from text2protein_amd.config import load_config
    from text2protein_amd.decode import decode_6d_batch
    from text2protein_amd.encode import encode_6d_batch
    from text2protein_amd.fold import fold_6d_batch, fold_maps_batch
    from text2protein_amd.model import HipScoreModel

    dev = torch.device("cuda:0")
    torch.cuda.set_device(dev)
    B, L = args.batch, 128
    truth = np.load(os.path.join(ROOT, "tests", "golden", "fold_chains.npz"))["xyz_132"][:L]
    xyz = torch.from_numpy(truth).float().unsqueeze(0).repeat(B, 1, 1, 1).to(dev)
    samples = encode_6d_batch(xyz, torch.full((B,), L, dtype=torch.int32))["coords_6d"]
    lengths, _, absval = decode_6d_batch(samples)
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

    fold_ms, (fxyz, status, _, diag) = timed(lambda: fold_maps_batch(absval, lengths))
    whole_ms, _ = timed(lambda: fold_6d_batch(samples))
    got = fxyz[0].cpu().numpy().astype(np.float64)
    p, q = got[:, 1] - got[:, 1].mean(0), truth[:, 1] - truth[:, 1].mean(0)
    u, s, vt = np.linalg.svd(p.T @ q)
    s[-1] *= np.sign(np.linalg.det(u @ vt))
    rmsd = float(np.sqrt(max((p * p).sum() + (q * q).sum() - 2 * s.sum(), 0.0) / L))

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
    mean = torch.empty_like(x)
    model.set_context(ctx)
    pc.reset(0)
    for _ in range(3):
        pc.step(x, mean)
    torch.cuda.synchronize()
    ev0.record()
    for _ in range(args.pc_steps):
        pc.step(x, mean)
    ev1.record()
    torch.cuda.synchronize()
    pc_ms = ev0.elapsed_time(ev1) / args.pc_steps

    out = {"what": "ms per fold call (32 chains, L = 128, known_below 19, 300 stress steps) next to ms per PC step, same process",
           "config": "cond_length.yml", "L": L, "chains": B, "dtype": args.dtype, "device": torch.cuda.get_device_name(0), "runs": args.runs,
           "fold_ms": round(statistics.median(fold_ms), 4), "fold_ms_runs": [round(v, 4) for v in fold_ms],
           "decode_and_fold_ms": round(statistics.median(whole_ms), 4), "decode_and_fold_ms_runs": [round(v, 4) for v in whole_ms],
           "pc_step_ms": round(pc_ms, 4), "pc_steps_timed": args.pc_steps,
           "fold_over_1000_pc_steps": round(statistics.median(fold_ms) / (1000.0 * pc_ms), 6),
           "status": sorted(set(status.cpu().tolist())), "ca_rmsd_to_truth": round(rmsd, 4),
           "finite": bool(torch.isfinite(fxyz).all() and torch.isfinite(diag).all() and torch.isfinite(x).all())}
    print(json.dumps(out), flush=True)
    if args.out:
        with open(args.out, "w") as f:
            json.dump(out, f, indent=1)
            f.write("\n")


if __name__ == "__main__":
    main()
