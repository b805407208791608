#!/usr/bin/env python3
"""ms per guided PC step (w = 0.7) next to the plain PC step at the same and at twice the batch: same model, process and device.

    python tools/bench_guided_pc.py [--steps 10] [--warmup 2] [--rounds 5] [--out profiles/guided_pc_cond_length.json]

The model is configs/cond_length.yml at L = 128 with synthetic weights, 32 chains, 512 text tokens, the f16 engine and the length
condition (bench.py's cfg3), the VE loop of the shipped config on the fused stepper.  A guided step at B does the network work of a
plain step at 2B (two evaluations of [x ; x] under [ctx ; 0]) and less elementwise work: noise and norms cover B samples, and the
guidance sum rides in the norm and update kernels.  So the criterion is guided at B <= plain at 2B, within the pass-to-pass spread
this tool reports; the ratio to a plain step at B is reported as well.  The three variants alternate, --rounds passes each, every
window `--steps` steps between device events after `--warmup` untimed steps; medians, every window and the spread are printed as
one JSON line.  bench.py is not touched.
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
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--batch", type=int, default=32)
    ap.add_argument("--dtype", default="f16", choices=["f32", "bf16", "f16"])
    ap.add_argument("--w", type=float, default=0.7)
    ap.add_argument("--out", default="")
    args = ap.parse_args()

    from text2protein_amd import sampling, sde_lib, synth
    from text2protein_amd.conditions import synthetic_condition
    from text2protein_amd.config import load_config
    from text2protein_amd.model import HipScoreModel

    dev = torch.device("cuda:0")
    torch.cuda.set_device(dev)
    cfg = load_config(os.path.join(ROOT, "configs", "cond_length.yml"), **{"data.max_res_num": 128, "model.num_scales": 1000})
    cfg.device = str(dev)
    B, T, Cn, L = args.batch, 512, cfg.data.num_channels, cfg.data.max_res_num
    model = HipScoreModel(cfg, dtype=args.dtype, device=str(dev))
    model.load_state_dict(synth.synth_state_dict(cfg, seed=0))
    sde = sde_lib.VESDE(sigma_min=cfg.model.sigma_min, sigma_max=cfg.model.sigma_max, N=cfg.model.num_scales)
    c = cfg.sampling
    ev0, ev1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)

    def variant(chains, w):
        """-> (step, rewind, state) of a fused stepper over `chains` chains, guided with weight w (None: plain)"""
        ctx = synth.synth_context(chains, T, cfg.model.context_dim, seed=1000).to(dev)
        cond = synthetic_condition(cfg, chains, "length", dev)
        st = sampling.PCStepper(model, sde, chains, c.snr, c.n_steps_each, c.probability_flow, c.noise_removal, 1e-5, seed=0, guidance_w=w)
        x = sampling._device_randn_like(torch.empty(chains, Cn, L, L, device=dev), 12345, 0) * sde.prior_scale()
        x, mask = sampling.apply_conditions(x, cond)
        x = x.float().contiguous()
        state = torch.empty(((2 if st.guided else 1) * chains,) + tuple(x.shape[1:]), device=dev)
        state[:chains] = x
        mask, init = mask.to(torch.uint8).contiguous(), x.clone()
        st.set_condition(mask, init)
        mean = torch.empty_like(x)

        def rewind():
            if w is None:
                model.set_context(ctx)
            else:
                st.set_context(ctx)
            st.reset(0)

        return (lambda: st.step(state, mean)), rewind, (st, state, mask, init, mean, ctx)

    variants = {"guided_B": variant(B, args.w), "plain_B": variant(B, None), "plain_2B": variant(2 * B, None)}

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

    times = {k: [] for k in variants}
    for _ in range(args.rounds):
        for name, (fn, rewind, _) in variants.items():
            times[name].append(window(fn, rewind))
    finite = all(bool(torch.isfinite(v[2][1]).all()) for v in variants.values())
    med = {k: statistics.median(v) for k, v in times.items()}
    spread = {k: (max(v) - min(v)) / med[k] for k, v in times.items()}
    margin = max(spread["guided_B"], spread["plain_2B"])
    out = {"what": "ms per PC step (VE, fused stepper): guided at B (2 evaluations at 2B, guidance sum inside the norm / update kernels) vs "
                   "plain at B and plain at 2B, same model and process",
           "config": "cond_length.yml", "L": L, "chains": B, "text_tokens": T, "dtype": args.dtype, "condition": "length", "w": args.w,
           "steps_per_window": args.steps, "warmup": args.warmup, "rounds": args.rounds, "device": torch.cuda.get_device_name(0),
           "ms_per_step": {k: round(v, 4) for k, v in med.items()},
           "windows_ms_per_step": {k: [round(t, 4) for t in v] for k, v in times.items()},
           "pass_to_pass_spread": {k: round(v, 4) for k, v in spread.items()},
           "guided_over_plain_2B": round(med["guided_B"] / med["plain_2B"], 4),
           "criterion_guided_B_at_most_plain_2B_within_spread": bool(med["guided_B"] <= med["plain_2B"] * (1 + margin)),
           "guided_over_plain_B": round(med["guided_B"] / med["plain_B"], 4),
           "finite": finite}
    print(json.dumps(out), flush=True)
    if args.out:
        with open(args.out, "w") as f:
            json.dump(out, f, indent=1)
            f.write("\n")


if __name__ == "__main__":
    main()
