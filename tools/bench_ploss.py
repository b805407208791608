"""Time the training step under the DDIM sampler's p_loss against the VP SDE step, in one process.

    python tools/bench_ploss.py [--config cond_length.yml] [--batch 16] [--steps 10] [--warmup 2] [--rounds 5] [--dtypes f32,f16]

Per compute dtype two trainers of the same configuration and weights live in the process: one under the VP SDE loss
(get_step_fn(VPSDE)), one under p_loss (get_ploss_step_fn on DiffusionSampler.from_sde of the same VPSDE: l2, masked).  After --warmup
steps of each, --rounds rounds of --steps VP steps and --steps p_loss steps alternate; t, z and the Dropout_0 masks are drawn on the
device in both.  The two steps differ in the per-sample preparation kernel and in the element-wise loss kernel only.

Prints one JSON line: per dtype every round of both (ms per step), the medians, the ranges, the spreads (max - min) and whether the
difference of the medians lies inside the VP rounds' own spread.  Measurement tool, not part of the product path or of bench.py's
headline."""
import argparse
import json
import os
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--config", default="cond_length.yml")
    ap.add_argument("--batch", type=int, default=16)
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--tokens", type=int, default=512)
    ap.add_argument("--L", type=int, default=128)
    ap.add_argument("--dtypes", default="f32,f16")
    a = ap.parse_args()
    from text2protein_amd import losses, sde_lib, synth
    from text2protein_amd.config import load_config
    from text2protein_amd.ddim import DiffusionSampler
    cfg = load_config(os.path.join(ROOT, "configs", a.config), **{"data.max_res_num": a.L})
    cfg.device = "cuda:0"
    if "optim" not in cfg:
        cfg.optim = dict(optimizer="Adam", lr=1e-4, beta1=0.9, eps=1e-8, weight_decay=0, warmup=5000, grad_clip=1.0)
    cfg.model.setdefault("ema_rate", 0.999)
    cfg.model.setdefault("dropout", 0.1)
    B, C, L = a.batch, cfg.data.num_channels, cfg.data.max_res_num
    x = torch.from_numpy(synth.uniform_pm1(1, "bench_train_x", B * C * L * L).reshape(B, C, L, L))
    mp = torch.zeros(B, L, L).bool()
    mp[:, :100, :100] = True
    x = x * mp.unsqueeze(1)
    x[:, -1] = mp.float()
    batch = dict(coords_6d=x.cuda(), mask_pair=mp.cuda(), context=synth.synth_context(B, a.tokens, cfg.model.context_dim, 3).cuda())
    if "inpainting" in (cfg.model.condition or []):
        batch["mask_inpaint"] = mp.cuda()
    vp = sde_lib.VPSDE(beta_min=cfg.model.beta_min, beta_max=cfg.model.beta_max, N=cfg.model.num_scales)
    sd = synth.synth_state_dict(cfg, 0)
    med = lambda v: sorted(v)[len(v) // 2]     # noqa: E731
    rows = {}
    for dt in a.dtypes.split(","):
        kinds = {}
        for kind in ("vp", "ploss"):
            model = losses.HipTrainModel(cfg, device="cuda:0", seed=1, dtype=dt)
            model.load_state_dict(sd)
            if kind == "vp":
                fn = losses.get_step_fn(vp, train=True, optimize_fn=losses.optimization_manager(cfg))
            else:
                fn = losses.get_ploss_step_fn(DiffusionSampler.from_sde(model, vp, loss_type="l2"), train=True,
                                              optimize_fn=losses.optimization_manager(cfg), masked=True)
            state = dict(model=model, optimizer=losses.get_optimizer(cfg, model.parameters()),
                         ema=losses.ExponentialMovingAverage(model.parameters(), decay=cfg.model.ema_rate), step=5000)
            kinds[kind] = (fn, state)

        def timed(kind):
            fn, state = kinds[kind]
            torch.cuda.synchronize()
            t0 = time.time()
            out = [fn(state, batch, condition=cfg.model.condition) for _ in range(a.steps)]
            torch.cuda.synchronize()
            return (time.time() - t0) / a.steps * 1e3, out

        seq = {"vp": [], "ploss": []}
        for kind in kinds:
            fn, state = kinds[kind]
            seq[kind] += [fn(state, batch, condition=cfg.model.condition) for _ in range(a.warmup)]
        ms = {"vp": [], "ploss": []}
        for _ in range(a.rounds):
            for kind in ("vp", "ploss"):
                d, out = timed(kind)
                ms[kind].append(d)
                seq[kind] += out
        row = {}
        for kind in ms:
            v = ms[kind]
            row[kind] = {"ms_rounds": v, "median_ms": med(v), "min_ms": min(v), "max_ms": max(v), "spread_ms": max(v) - min(v),
                         "losses": [round(s, 5) for s in seq[kind]], "device_GiB": kinds[kind][1]["model"].device_bytes() / 2 ** 30}
        diff = row["ploss"]["median_ms"] - row["vp"]["median_ms"]
        row["median_ploss_minus_vp_ms"] = diff
        row["difference_inside_vp_spread"] = abs(diff) <= row["vp"]["spread_ms"]
        rows[dt] = row
        kinds.clear()
        torch.cuda.empty_cache()
    print(json.dumps({"what": "training step under the VP SDE loss and under the DDIM sampler's p_loss (l2, masked), alternating rounds in one "
                              "process, ms per step", "config": a.config, "batch": B, "L": L, "tokens": a.tokens, "steps_per_round": a.steps,
                      "warmup": a.warmup, "rounds": a.rounds, "dropout": float(cfg.model.dropout), "condition": list(cfg.model.condition or []),
                      "timesteps": int(vp.N), "rows": rows}))


if __name__ == "__main__":
    main()
