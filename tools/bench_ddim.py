#!/usr/bin/env python3
"""ms per DDIM step (guided, w = 0.7, and unguided, w = 1) next to ms per PC step, same model, same process, same device.

    python tools/bench_ddim.py [--steps 20] [--warmup 3] [--rounds 3] [--out profiles/ddim_cond_length.json]

The model is configs/cond_length.yml at L = 128 with synthetic weights, 32 chains, 512 text tokens, the f16 engine and the
length condition (bench.py's cfg3).  A guided DDIM step is ONE evaluation at batch 2B plus one elementwise pass; a PC step is
two evaluations at batch B plus two updates and the norm reductions; with w = 1 a DDIM step is one evaluation at batch B.
The PC step is measured as bench.py measures it (the VE loop of the shipped config, fused stepper); the DDIM steps run under
training.sde = vpsde.  The three variants alternate, --rounds times each, every window `--steps` steps between device events after
`--warmup` untimed steps; the medians and every window are printed as one JSON line.  bench.py is not touched.
"""
import argparse
import json
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--batch", type=int, default=32)
    ap.add_argument("--dtype", default="f16", choices=["f32", "bf16", "f16"])
    ap.add_argument("--ddim_steps", type=int, default=50)
    ap.add_argument("--out", default="")
    args = ap.parse_args()
    if args.steps + args.warmup >= args.ddim_steps:
        raise SystemExit("--steps + --warmup must stay below --ddim_steps: the last step of a run does less work")

    from text2protein_amd import sampling, sde_lib, synth
    from text2protein_amd.conditions import synthetic_condition
    from text2protein_amd.config import load_config
    from text2protein_amd.ddim import DDIMStepper, DiffusionSampler
    from text2protein_amd.model import HipScoreModel

    dev = torch.device("cuda:0")
    torch.cuda.set_device(dev)
    cfg = load_config(os.path.join(ROOT, "configs", "cond_length.yml"),
                      **{"data.max_res_num": 128, "model.num_scales": 1000, "training.sde": "vpsde"})
    cfg.device = str(dev)
    B, T, Cn, L = args.batch, 512, cfg.data.num_channels, cfg.data.max_res_num
    model = HipScoreModel(cfg, dtype=args.dtype, device=str(dev))
    model.load_state_dict(synth.synth_state_dict(cfg, seed=0))
    ctx = synth.synth_context(B, T, cfg.model.context_dim, seed=1000).to(dev)
    cond = synthetic_condition(cfg, B, "length", dev)
    ev0, ev1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)

    def window(step_fn, rewind):
        rewind()
        for _ in range(args.warmup):
            step_fn()
        torch.cuda.synchronize()
        ev0.record()
        for _ in range(args.steps):
            step_fn()
        ev1.record()
        torch.cuda.synchronize()
        return ev0.elapsed_time(ev1) / args.steps

    def conditioned(scale, rows):
        x = sampling._device_randn_like(torch.empty(B, Cn, L, L, device=dev), 12345, 0) * scale
        x, mask = sampling.apply_conditions(x, cond)
        x = x.float().contiguous()
        state = torch.empty((rows,) + tuple(x.shape[1:]), device=dev)
        state[:B] = x
        return state, mask.to(torch.uint8).contiguous(), x.clone()

    # the PC step of the shipped configuration (VE), as bench.py --workload cfg3 runs it
    ve = sde_lib.VESDE(sigma_min=cfg.model.sigma_min, sigma_max=cfg.model.sigma_max, N=cfg.model.num_scales)
    c = cfg.sampling
    pc = sampling.PCStepper(model, ve, B, c.snr, c.n_steps_each, c.probability_flow, c.noise_removal, 1e-5, seed=0)
    pc_x, pc_mask, pc_init = conditioned(ve.prior_scale(), B)
    pc.set_condition(pc_mask, pc_init)
    pc_mean = torch.empty_like(pc_x)

    def pc_rewind():
        model.set_context(ctx)
        pc.reset(0)

    variants = {"pc": (lambda: pc.step(pc_x, pc_mean), pc_rewind)}
    vp = sde_lib.VPSDE(beta_min=cfg.model.beta_min, beta_max=cfg.model.beta_max, N=cfg.model.num_scales)
    keep = []
    for name, w in (("ddim_w0.7", 0.7), ("ddim_w1", 1.0)):
        ds = DiffusionSampler.from_sde(model, vp, sampling_steps=args.ddim_steps, ddim_eta=1.0, w=w)
        st = DDIMStepper(model, ds, B, True, seed=0)
        x, mask, init = conditioned(1.0, 2 * B if w != 1.0 else B)
        st.set_condition(mask, init)
        keep.append((ds, st, x, mask, init))

        def rewind(st=st):
            st.set_context(ctx)
            st.reset(0)

        variants[name] = ((lambda st=st, x=x: st.step(x)), rewind)

    times = {k: [] for k in variants}
    for _ in range(args.rounds):
        for name, (fn, rewind) in variants.items():
            times[name].append(window(fn, rewind))
    finite = all(bool(torch.isfinite(t).all()) for t in [pc_x] + [k[2] for k in keep])
    med = {k: statistics.median(v) for k, v in times.items()}
    out = {"what": "ms per step: one PC step (2 evaluations at B, VE, fused stepper) vs one DDIM step (guided: 1 evaluation at 2B; w = 1: "
                   "1 evaluation at B), same model and process",
           "config": "cond_length.yml", "L": L, "chains": B, "text_tokens": T, "dtype": args.dtype, "condition": "length",
           "steps_per_window": args.steps, "warmup": args.warmup, "rounds": args.rounds, "device": torch.cuda.get_device_name(0),
           "ms_per_step": {k: round(v, 4) for k, v in med.items()},
           "windows_ms_per_step": {k: [round(t, 4) for t in v] for k, v in times.items()},
           "guided_over_pc": round(med["ddim_w0.7"] / med["pc"], 4), "guided_over_pc_expected_at_most": 1.05,
           "w1_over_pc": round(med["ddim_w1"] / med["pc"], 4), "w1_over_pc_expected_at_most": 0.55,
           "finite": finite}
    print(json.dumps(out), flush=True)
    if args.out:
        with open(args.out, "w") as f:
            json.dump(out, f, indent=1)
            f.write("\n")


if __name__ == "__main__":
    main()
