#!/usr/bin/env python3
"""ms per PC step with replacement inpainting next to the plain PC step of the SAME sampler: same model, process and device.

    python tools/bench_inpaint_replace.py [--steps 10] [--warmup 2] [--rounds 5] [--out profiles/inpaint_replace_cond_length.json]

The model is configs/cond_length.yml at L = 128 with synthetic weights, 32 chains, 512 text tokens, the f16 engine and the length
condition (bench.py's cfg3), the VE loop of the shipped config on the fused stepper.  The replacement adds 5 bytes of reads per
element (the known byte and the data) and one Philox draw per quad with a known element to the Langevin and the predictor update
kernels, and no launch: the dispatch counts of both steps are reported.  One stepper serves both variants (t2p_sampler_set_inpaint
on / off between windows); the two alternate, --rounds passes each, every window `--steps` steps between device events after
`--warmup` untimed steps.  Medians with min..max, every window, the spreads and the criterion -- the difference of the medians
lies inside the plain windows' own min..max spread -- are printed as one JSON line.  The known region is everything inside the
100-residue square off residues 1:5 and 10:15 (the driver's default --mask_info).  bench.py is not touched.
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
    ap.add_argument("--out", default="")
    args = ap.parse_args()

    from text2protein_amd import sampling, sde_lib, synth
    from text2protein_amd.conditions import synthetic_condition
    from text2protein_amd.config import load_config
    from text2protein_amd.inpainting import known_from_mask_info
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
    eps = 1e-5
    ev0, ev1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)

    ctx = synth.synth_context(B, T, cfg.model.context_dim, seed=1000).to(dev)
    cond = synthetic_condition(cfg, B, "length", dev)
    st = sampling.PCStepper(model, sde, B, c.snr, c.n_steps_each, c.probability_flow, c.noise_removal, eps, seed=0)
    coords = torch.from_numpy(synth.uniform_pm1(0, "coords_6d", B * Cn * L * L).reshape(B, Cn, L, L)).to(dev)
    data, known = known_from_mask_info(cfg, {"coords_6d": coords, "lengths": [100] * B}, "1:5,10:15", cond)
    data, known_u8 = data.contiguous(), known.to(torch.uint8).contiguous()
    tables = sde.inpaint_tables(eps)
    prior = sampling._device_randn_like(torch.empty(B, Cn, L, L, device=dev), 12345, 0) * sde.prior_scale()
    x0, mask = sampling.apply_conditions(torch.where(known, data, prior), cond)
    x0 = x0.float().contiguous()
    mask, init = mask.to(torch.uint8).contiguous(), x0.clone()
    st.set_condition(mask, init)
    model.set_context(ctx)
    state, mean = x0.clone(), torch.empty_like(x0)

    def window(replace):
        st.set_inpaint(*((known_u8, data) + tuple(tables) if replace else ()))
        state.copy_(x0)
        st.reset(0)
        for _ in range(args.warmup):
            st.step(state, mean)
        torch.cuda.synchronize()
        ev0.record()
        for _ in range(args.steps):
            st.step(state, mean)
        ev1.record()
        torch.cuda.synchronize()
        return ev0.elapsed_time(ev1) / args.steps

    times = {"plain": [], "replace": []}
    for _ in range(args.rounds):
        for name in times:
            times[name].append(window(name == "replace"))
    finite = bool(torch.isfinite(state).all())
    held = bool(torch.equal(mean[known], data[known]))          # the last window replaced: x_mean of the known region is the data
    dispatches = {}
    for name in times:
        st.set_inpaint(*((known_u8, data) + tuple(tables) if name == "replace" else ()))
        st.reset(0)
        dispatches[name] = st.count_dispatches(state, mean)
    med = {k: statistics.median(v) for k, v in times.items()}
    spread = {k: (max(v) - min(v)) / med[k] for k, v in times.items()}
    diff = med["replace"] - med["plain"]
    parent_plain = 15.0184                                       # profiles/guided_pc_cond_length.json, plain_B, before the branch existed
    out = {"what": "ms per PC step (VE, fused stepper, one sampler): replacement inpainting on vs off; the replacement rides in the "
                   "Langevin and predictor update kernels",
           "config": "cond_length.yml", "L": L, "chains": B, "text_tokens": T, "dtype": args.dtype, "condition": "length",
           "known_fraction": round(float(known.float().mean()), 4),
           "steps_per_window": args.steps, "warmup": args.warmup, "rounds": args.rounds, "device": torch.cuda.get_device_name(0),
           "ms_per_step": {k: round(v, 4) for k, v in med.items()},
           "min_max_ms_per_step": {k: [round(min(v), 4), round(max(v), 4)] for k, v in times.items()},
           "windows_ms_per_step": {k: [round(t, 4) for t in v] for k, v in times.items()},
           "pass_to_pass_spread": {k: round(v, 4) for k, v in spread.items()},
           "replace_minus_plain_ms": round(diff, 4),
           "replace_over_plain": round(med["replace"] / med["plain"], 4),
           "criterion_difference_inside_plain_spread": bool(abs(diff) <= max(times["plain"]) - min(times["plain"])),
           "dispatches_per_step": dispatches,
           "extra_bytes_read_per_step": 2 * 5 * B * Cn * L * L,
           "plain_vs_parent": {"parent_plain_ms": parent_plain, "parent_spread": 0.0196, "ratio": round(med["plain"] / parent_plain, 4)},
           "finite": finite, "known_region_held": held}
    print(json.dumps(out), flush=True)
    if args.out:
        with open(args.out, "w") as f:
            json.dump(out, f, indent=1)
            f.write("\n")


if __name__ == "__main__":
    main()
