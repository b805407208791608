"""Time the training step (t2p_train_step: loss + backward + Adam + EMA) at a BASELINE model size.

    python tools/bench_train.py --config cond_length.yml --batch 8 --steps 5 [--tokens 64] [--dropout 0.1] [--dtype f32|f16|bf16] [--sde ve|vp|subvp]
                                [--condition length,ss [--ss-blocks 64]] [--inpaint_draw host|device [--rounds 5]]
                                [--context-dropout 0.1 [--rounds 5]]

--ss-blocks N: N synthetic secondary-structure blocks per step (8 residues each, spread over the samples and the 100 valid residues),
dropped on the device at the reference's p = 0.2; needs the `ss` condition, which needs an 8-channel configuration
(cond_length_inpainting.yml with --condition length,ss).

--inpaint_draw host|device: the batch carries NO mask_inpaint; the random mask of the reference's training loop (utils.random_mask_batch,
from config.model.inpainting and 100 valid residues per sample) is drawn before every step, on the host in the reference's order or on the
device from the trainer's Philox; needs the `inpainting` condition (cond_length_inpainting.yml).  With --rounds R the same process times R
rounds of --steps steps WITH A SUPPLIED MASK and R rounds with the drawn one, alternating, and reports every round of both
(`supplied_ms_rounds`, `drawn_ms_rounds`); `ms_per_step` is then the median drawn round.

--context-dropout P: text-context dropout (training for classifier-free guidance), every sample dropped on the device with probability P
before every step (get_step_fn(context_dropout=P)).  With --rounds R the same process times R rounds of --steps PLAIN steps and R rounds of
dropout steps, alternating, and reports every round of both (`plain_ms_rounds`, `ctxdrop_ms_rounds`) with their medians and spreads
(max - min); `ms_per_step` is then the median dropout round.

Prints one JSON line: ms per step, samples/s, the loss sequence, device memory, and the achieved matrix rate against the peak of the
compute dtype's MFMA (157.3 TFLOP/s f32, 2500 TFLOP/s f16 / bf16), counting a step as 3 x the forward pass AS EXECUTED (the text K / V projections are inside a training
step: the context changes with every batch).  Measurement tool, not part of the product path or of bench.py's headline."""
import argparse
import json
import os
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

PEAK_TFLOPS = {"f32": 157.3, "f16": 2500.0, "bf16": 2500.0}
FWD_GFLOP = {"test_config.yml": 714.0, "cond_length.yml": 151.2, "cond_length_inpainting.yml": 151.4, "test_config_large.yml": 3099.6}   # SURVEY 8(d), L = 128 / 256, T = 512


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--config", default="cond_length.yml")
    ap.add_argument("--batch", type=int, default=8)
    ap.add_argument("--steps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--tokens", type=int, default=512)
    ap.add_argument("--L", type=int, default=0)
    ap.add_argument("--dropout", type=float, default=-1.0)
    ap.add_argument("--dtype", default="f32", choices=sorted(PEAK_TFLOPS))
    ap.add_argument("--sde", default="ve", choices=["ve", "vp", "subvp"], help="the SDE of the loss")
    ap.add_argument("--condition", default="", help="override model.condition, comma-separated (e.g. length,ss)")
    ap.add_argument("--ss-blocks", type=int, default=0, help="synthetic secondary-structure blocks per step, drawn on the device")
    ap.add_argument("--inpaint_draw", default=None, choices=["host", "device"], help="draw the random inpainting mask before every step")
    ap.add_argument("--rounds", type=int, default=1, help="with --inpaint_draw: rounds of supplied-mask steps and drawn-mask steps, alternating; "
                                                          "with --context-dropout: rounds of plain steps and dropout steps, alternating")
    ap.add_argument("--context-dropout", type=float, default=0.0, help="drop every sample's text context with this probability, on the device")
    a = ap.parse_args()
    from text2protein_amd import losses, sde_lib, synth
    from text2protein_amd.config import load_config
    over = {"data.max_res_num": a.L or (256 if "large" in a.config else 128)}
    if a.dropout >= 0:
        over["model.dropout"] = a.dropout
    if a.condition:
        over["model.condition"] = a.condition.split(",")
    cfg = load_config(os.path.join(ROOT, "configs", a.config), **over)
    cfg.device = "cuda:0"
    if "optim" not in cfg:
        cfg.optim = dict(optimizer="Adam", lr=1e-4, beta1=0.9, eps=1e-8, weight_decay=0, warmup=5000, grad_clip=1.0)
    cfg.model.setdefault("ema_rate", 0.999)
    cfg.model.setdefault("dropout", 0.1)
    model = losses.HipTrainModel(cfg, device="cuda:0", seed=1, dtype=a.dtype)
    model.load_state_dict(synth.synth_state_dict(cfg, 0))
    B, C, L = a.batch, cfg.data.num_channels, cfg.data.max_res_num
    x = torch.from_numpy(synth.uniform_pm1(1, "bench_train_x", B * C * L * L).reshape(B, C, L, L))
    mp = torch.zeros(B, L, L).bool()
    mp[:, :100, :100] = True
    x = x * mp.unsqueeze(1)
    x[:, -1] = mp.float()
    batch = dict(coords_6d=x.cuda(), mask_pair=mp.cuda(), context=synth.synth_context(B, a.tokens, cfg.model.context_dim, 3).cuda())
    if "inpainting" in (cfg.model.condition or []):
        batch["mask_inpaint"] = mp.cuda()
    if a.sde == "ve":
        sde = sde_lib.VESDE(sigma_min=cfg.model.sigma_min, sigma_max=cfg.model.sigma_max, N=cfg.model.num_scales)
    else:
        sde = (sde_lib.VPSDE if a.sde == "vp" else sde_lib.subVPSDE)(beta_min=cfg.model.beta_min, beta_max=cfg.model.beta_max, N=cfg.model.num_scales)
    if a.inpaint_draw and "inpainting" not in (cfg.model.condition or []):
        raise SystemExit("--inpaint_draw needs the inpainting condition (cond_length_inpainting.yml)")
    if a.inpaint_draw and a.context_dropout > 0 and a.rounds > 1:
        raise SystemExit("--rounds compares one pair of variants: --inpaint_draw or --context-dropout, not both")
    step_fn = losses.get_step_fn(sde, train=True, optimize_fn=losses.optimization_manager(cfg), inpaint_mask_draw=a.inpaint_draw)
    ctxdrop_fn = losses.get_step_fn(sde, train=True, optimize_fn=losses.optimization_manager(cfg), inpaint_mask_draw=a.inpaint_draw,
                                    context_dropout=a.context_dropout, context_dropout_draw="device")
    drawn_batch = dict({k: v for k, v in batch.items() if k != "mask_inpaint"}, lengths=[100] * B)      # no mask: the step draws it
    state = dict(model=model, optimizer=losses.get_optimizer(cfg, model.parameters()),
                 ema=losses.ExponentialMovingAverage(model.parameters(), decay=cfg.model.ema_rate), step=5000)
    blocks = [(k % B, (8 * (k // B)) % 96, (8 * (k // B)) % 96 + 8) for k in range(a.ss_blocks)]
    if blocks and "ss" not in (cfg.model.condition or []):
        raise SystemExit("--ss-blocks needs the ss condition (--condition length,ss on an 8-channel configuration)")

    def one_step():
        if blocks:
            model.set_ss_blocks(blocks, drop=None, p=0.2)       # per-batch data: set before every step, consumed by it
        return (ctxdrop_fn if a.context_dropout > 0 else step_fn)(state, drawn_batch if a.inpaint_draw else batch, condition=cfg.model.condition)

    def timed(fn):
        torch.cuda.synchronize()
        t0 = time.time()
        out = [fn() for _ in range(a.steps)]
        torch.cuda.synchronize()
        return (time.time() - t0) / a.steps, out

    seq = []
    for _ in range(a.warmup):
        seq.append(one_step())
    extra = {}
    if a.inpaint_draw and a.rounds > 1:
        for _ in range(a.warmup):
            step_fn(state, batch, condition=cfg.model.condition)
        supplied, drawn = [], []
        for _ in range(a.rounds):
            supplied.append(timed(lambda: step_fn(state, batch, condition=cfg.model.condition))[0] * 1e3)
            d, out = timed(one_step)
            drawn.append(d * 1e3)
            seq += out
        dt = sorted(drawn)[len(drawn) // 2] / 1e3
        extra = {"supplied_ms_rounds": supplied, "drawn_ms_rounds": drawn, "supplied_median_ms": sorted(supplied)[len(supplied) // 2]}
    elif a.context_dropout > 0 and a.rounds > 1:
        for _ in range(a.warmup):
            step_fn(state, batch, condition=cfg.model.condition)
        plain, dropped = [], []
        for _ in range(a.rounds):
            plain.append(timed(lambda: step_fn(state, batch, condition=cfg.model.condition))[0] * 1e3)
            d, out = timed(one_step)
            dropped.append(d * 1e3)
            seq += out
        med = lambda v: sorted(v)[len(v) // 2]     # noqa: E731
        dt = med(dropped) / 1e3
        extra = {"plain_ms_rounds": plain, "ctxdrop_ms_rounds": dropped, "plain_median_ms": med(plain), "ctxdrop_median_ms": med(dropped),
                 "plain_spread_ms": max(plain) - min(plain), "ctxdrop_spread_ms": max(dropped) - min(dropped)}
    else:
        dt, out = timed(one_step)
        seq += out
    gf = FWD_GFLOP.get(a.config, 0.0) * 3 * B
    out = {"metric": f"training step ({'fp32' if a.dtype == 'f32' else a.dtype})", "dtype": a.dtype, "sde": a.sde, "config": a.config, "batch": B, "L": L,
           "tokens": a.tokens, "ms_per_step": dt * 1e3, "samples_per_s": B / dt, "losses": [round(v, 5) for v in seq],
           "device_GiB": model.device_bytes() / 2 ** 30, "channels": C, "condition": list(cfg.model.condition or []), "ss_blocks": len(blocks),
           "inpaint_draw": a.inpaint_draw, "context_dropout": a.context_dropout, **extra}
    tf = gf / dt / 1e3
    if a.dtype == "f32":
        out.update(tflops_f32=tf, frac_of_f32_peak=tf / PEAK_TFLOPS["f32"])
    out.update(tflops=tf, peak_tflops=PEAK_TFLOPS[a.dtype], frac_of_peak=tf / PEAK_TFLOPS[a.dtype], dropout=float(cfg.model.dropout))
    print(json.dumps(out))


if __name__ == "__main__":
    main()
