#!/usr/bin/env python3
"""ms per refinement call (text2protein_amd/refine.py) for 32 chains at L = 128, next to the ms of the fold call that feeds it and of
one PC step of the same shapes, same process.

    python tools/bench_refine.py [--runs 5] [--pc_steps 10] [--out profiles/refine_cond_length.json]

The chains are 32 copies of the committed 132-residue compact synthetic chain (tests/golden/fold_chains.npz) cut to 128 residues,
encoded, decoded and folded on the device.  ``refine`` = t2p_op_refine_backbone alone (one launch, one workgroup per chain, the default
schedule of three stages of at most 300 iterations) on the exact maps; ``refine_noisy`` = the same call on maps with Gaussian noise of
1.0 A / 0.1 rad on the known pairs (drawn once with a fixed torch seed), started from the fold of those maps -- what a sampled map
looks like to the minimiser.  Timed between device events, median of --runs calls after one untimed call.  The PC step is the one
bench.py measures for configs/cond_length.yml (VE, fused stepper, f16 engine, 512 text tokens, length condition), --pc_steps steps
after 3 untimed ones.  There is no pass mark: a 1000-step run is 1000 PC steps, fold and refinement run once after it.  One JSON line;
bench.py is not touched.
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


def ca_rmsd(got, truth):
    p, q = got - got.mean(0), truth - truth.mean(0)
    u, s, vt = np.linalg.svd(p.T @ q)
    s[-1] *= np.sign(np.linalg.det(u @ vt))
    return float(np.sqrt(max((p * p).sum() + (q * q).sum() - 2 * s.sum(), 0.0) / p.shape[0]))


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
    from text2protein_amd.fold import fold_maps_batch
    from text2protein_amd.model import HipScoreModel
    from text2protein_amd.refine import diagnostics, refine_backbone_batch

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

    # the noisy maps: symmetric noise on dist and omega (only the upper triangle is read), per ordered pair on theta and phi
    g = torch.Generator(device="cpu").manual_seed(20240)
    z = torch.randn(B, 4, L, L, generator=g).to(dev)
    m = absval.reshape(B, 4, L, L)
    known = (m[:, 0] > 0) & (m[:, 0] < 20.0)
    noisy = m.clone()
    noisy[:, 0] = torch.where(known, (m[:, 0] + 1.0 * z[:, 0]).clamp(0.5, 19.99), m[:, 0])
    for c in (1, 2):
        a = m[:, c] + 0.1 * z[:, c]
        noisy[:, c] = torch.where(known, a - 2 * np.pi * torch.round(a / (2 * np.pi)), m[:, c])
    noisy[:, 3] = torch.where(known, (m[:, 3] + 0.1 * z[:, 3]).clamp(0.01, np.pi - 0.01), m[:, 3])
    noisy = noisy.reshape(B, 4, L * L).contiguous()

    fold_ms, (fxyz, fstatus, _, _) = timed(lambda: fold_maps_batch(absval, lengths))
    refine_ms, (rxyz, rstatus, rdiag) = timed(lambda: refine_backbone_batch(fxyz, absval, lengths))
    nxyz = fold_maps_batch(noisy, lengths)[0]
    noisy_ms, (nrxyz, nstatus, ndiag) = timed(lambda: refine_backbone_batch(nxyz, noisy, lengths))
    rep, nrep = diagnostics(rstatus, rdiag, lengths), diagnostics(nstatus, ndiag, lengths)
    rm = lambda x, b: ca_rmsd(x[b, :, 1].cpu().numpy().astype(np.float64), truth[:, 1])

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

    med = statistics.median
    out = {"what": "ms per refinement call (32 chains, L = 128, default schedule) next to ms per fold call and per PC step, same process",
           "config": "cond_length.yml", "L": L, "chains": B, "dtype": args.dtype, "device": torch.cuda.get_device_name(0), "runs": args.runs,
           "refine_ms": round(med(refine_ms), 4), "refine_ms_runs": [round(v, 4) for v in refine_ms],
           "refine_noisy_ms": round(med(noisy_ms), 4), "refine_noisy_ms_runs": [round(v, 4) for v in noisy_ms],
           "fold_ms": round(med(fold_ms), 4), "fold_ms_runs": [round(v, 4) for v in fold_ms],
           "pc_step_ms": round(pc_ms, 4), "pc_steps_timed": args.pc_steps,
           "refine_over_1000_pc_steps": round(med(refine_ms) / (1000.0 * pc_ms), 6),
           "refine_noisy_over_1000_pc_steps": round(med(noisy_ms) / (1000.0 * pc_ms), 6),
           "exact": {"status": sorted(set(rstatus.cpu().tolist())), "evaluations": rep[0]["evaluations"], "iterations": rep[0]["iterations"],
                     "fold_ca_rmsd": round(rm(fxyz, 0), 4), "refined_ca_rmsd": round(rm(rxyz, 0), 4), "closure": rep[0]["closure"]},
           "noisy": {"status": sorted(set(nstatus.cpu().tolist())), "noise": [1.0, 0.1],
                     "evaluations": [min(r["evaluations"] for r in nrep), max(r["evaluations"] for r in nrep)],
                     "fold_ca_rmsd_mean": round(float(np.mean([rm(nxyz, b) for b in range(B)])), 4),
                     "refined_ca_rmsd_mean": round(float(np.mean([rm(nrxyz, b) for b in range(B)])), 4),
                     "closure_max": max(r["closure"] for r in nrep)},
           "finite": bool(torch.isfinite(rxyz).all() and torch.isfinite(rdiag).all() and torch.isfinite(nrxyz).all() and torch.isfinite(x).all())}
    print(json.dumps(out), flush=True)
    if args.out:
        with open(args.out, "w") as f:
            json.dump(out, f, indent=1)
            f.write("\n")


if __name__ == "__main__":
    main()
