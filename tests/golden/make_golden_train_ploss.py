"""Golden fixtures of the TRAINING STEP under the DDIM sampler's own objective, produced by autograd through the REFERENCE UNetModel and the
REFERENCE DiffusionSampler (build container only).

    python tests/golden/make_golden_train_ploss.py

Same procedure and stored form as make_golden_train_sde.py: the reference `UNetModel` in train mode with `synth.synth_state_dict`, the
counter-based Dropout_0 keep-masks, `torch.optim.Adam`, `clip_grad_norm_` and the reference's `ExponentialMovingAverage`; inputs from
`helpers.train_inputs`, whose float t is ignored in favour of the case's integer timesteps.  The loss of the unmasked cases is the reference's
own `DiffusionSampler.p_loss` (model/diffusion_sampler.py:150-163; that file calls `model(x_noisy, t, context)`, UNetModel.forward's order)
on a sampler built with the case's betas (passed explicitly: with betas=None the reference moves its schedule to 'cuda').  For the masked
cases the masked form is written out here next to the reference's tables: its `q_sample`, the `torch.where` and the normalisation of
losses.py:115-134.  Stored besides what the VE fixtures hold: t, a = sqrt_alpha_cumprod[t], s = sqrt_one_minus_alphas_cumprod[t], the two
tables and the betas.  `score` holds pred_noise.  Only data is written; no reference source text goes into the repo.
"""
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, "/root/reference")

from helpers import CounterDropout, projection             # noqa: E402
from ploss_cases import L1_MIN_RESIDUAL, PLOSS_CASES, make_betas, ploss_inputs     # noqa: E402
from text2protein_amd import synth                         # noqa: E402

from score_sde_pytorch.models import ncsnpp                # noqa: E402  (reference)
from score_sde_pytorch.models.ema import ExponentialMovingAverage   # noqa: E402  (reference)
from model.diffusion_sampler import DiffusionSampler       # noqa: E402  (reference)

from make_golden_train import FULL_TENSORS                 # noqa: E402


def reference_step(cfg, case, inp):
    """One training step on the reference model: step_fn (losses.py:165-176) with p_loss as the loss and optimize_fn (:41-49)."""
    torch.manual_seed(0)
    model = ncsnpp.UNetModel(cfg)
    sd = synth.synth_state_dict(cfg, case["seed"])
    missing, unexpected = model.load_state_dict(sd, strict=False)
    assert (list(missing) == ["sigmas"] or not missing) and not unexpected
    o = cfg.optim
    optimizer = torch.optim.Adam(model.parameters(), lr=o.lr, betas=(o.beta1, 0.999), eps=o.eps, weight_decay=o.weight_decay)
    ema = ExponentialMovingAverage(model.parameters(), decay=cfg.model.ema_rate)
    betas = make_betas(case, cfg)
    ds = DiffusionSampler(model, timesteps=betas.numel(), betas=betas, loss_type=case["loss_type"])
    state = dict(optimizer=optimizer, model=model, ema=ema, step=case["step0"])
    x, t, z, ctx = inp["coords_6d"], inp["t"], inp["z"], inp["context"]
    seen = {}
    hook = model.register_forward_hook(lambda mod, args, out: seen.update(labels=args[1].detach().clone(), x_noisy=args[0].detach().clone(),
                                                                          pred=out.detach().clone()))
    drop = CounterDropout(case["seed"], cfg.model.dropout)
    real = torch.nn.functional.dropout
    torch.nn.functional.dropout = drop.functional
    # UNetModel.forward divides by its float64 `sigmas` buffer, so pred_noise is float64 and p_loss's mse_loss(pred_noise, noise) promotes the
    # float32 noise; this torch computes that forward but refuses its backward ("Found dtype Float but expected Double").  The promotion is
    # made explicit for the call: the same values, a backward that runs
    real_mse = torch.nn.functional.mse_loss
    torch.nn.functional.mse_loss = lambda input, target, *a, **k: real_mse(input, target.to(input.dtype), *a, **k)
    mask = None
    try:
        optimizer.zero_grad()
        if not case["masked"]:
            loss = ds.p_loss(x, t, ctx, noise=z)             # the reference's loss as written
        else:
            conditional_mask = torch.ones_like(x).bool()
            for c in cfg.model.condition:
                if c == "length":
                    conditional_mask[:, -1] = False
                elif c == "ss":
                    conditional_mask[:, 4:7] = False
                elif c == "inpainting":
                    conditional_mask = conditional_mask * inp["mask_inpaint"].unsqueeze(1)
            mask = inp["mask_pair"].unsqueeze(1) * conditional_mask
            num_elem = mask.reshape(mask.shape[0], -1).sum(dim=-1)
            x_noisy = torch.where(mask, ds.q_sample(x, t, z), x)
            pred = model(x_noisy, t, ctx)
            e = torch.abs(pred - z) if case["loss_type"] == "l1" else torch.square(pred - z)
            losses = torch.sum((e * mask).reshape(e.shape[0], -1), dim=-1) / (num_elem + 1e-8)
            loss = torch.mean(losses)
        loss.backward()
    finally:
        torch.nn.functional.dropout = real
        torch.nn.functional.mse_loss = real_mse
        hook.remove()
    n_drop = drop.k
    grads = {n: p.grad.detach().clone() for n, p in model.named_parameters()}
    if o.warmup > 0:
        for g in optimizer.param_groups:
            g["lr"] = o.lr * np.minimum(state["step"] / o.warmup, 1.0)
    if o.grad_clip >= 0:
        torch.nn.utils.clip_grad_norm_(model.parameters(), max_norm=o.grad_clip)
    optimizer.step()
    state["step"] += 1
    state["ema"].update(model.parameters())
    names = [n for n, _ in model.named_parameters()]
    post = {n: p.detach().clone() for n, p in model.named_parameters()}
    shadow = dict(zip(names, [s.detach().clone() for s in ema.shadow_params]))
    st = optimizer.state
    m = {n: st[p]["exp_avg"].clone() for n, p in model.named_parameters()}
    v = {n: st[p]["exp_avg_sq"].clone() for n, p in model.named_parameters()}
    counted = torch.ones_like(x).bool() if mask is None else mask
    return dict(loss=loss.detach(), score=seen["pred"], grads=grads, post=post, ema=shadow, m=m, v=v, names=names, sd=sd, n_drop=n_drop,
                labels=seen["labels"], x_noisy=seen["x_noisy"], a=ds.sqrt_alpha_cumprod[t], s=ds.sqrt_one_minus_alphas_cumprod[t], ds=ds,
                betas=betas, min_residual=float((seen["pred"] - z).abs()[counted].min()))


def fixture(name):
    case = PLOSS_CASES[name]
    cfg = case["config"]()
    inp = ploss_inputs(cfg, case)
    r = reference_step(cfg, case, inp)
    names = r["names"]
    full = [n for n in FULL_TENSORS + case.get("extra_full", []) if n in r["grads"]]
    moved = max(float((r["post"][n] - r["sd"][n]).abs().max()) for n in names)
    print(f"[{name}] loss {float(r['loss']):.6g} ({r['n_drop']} dropout calls); t {inp['t'].tolist()}, a {r['a'].tolist()}, s {r['s'].tolist()}; "
          f"min |pred - noise| over the counted elements {r['min_residual']:.3e}; largest parameter move {moved:.3e}", flush=True)
    assert moved > 0 and np.isfinite(float(r["loss"])) and torch.equal(r["labels"], inp["t"])
    if case["loss_type"] == "l1":
        assert r["min_residual"] > L1_MIN_RESIDUAL, "an l1 residual is within 1e-4 of zero: choose another seed for this case"
    out = {"loss": np.float64(r["loss"]), "score": r["score"].float().numpy(), "names": np.array(names), "n_dropout_calls": np.int64(r["n_drop"]),
           "t": inp["t"].numpy(), "a": r["a"].float().numpy(), "s": r["s"].float().numpy(), "betas": r["betas"].float().numpy(),
           "sqrt_alpha_cumprod": r["ds"].sqrt_alpha_cumprod.float().numpy(),
           "sqrt_one_minus_alphas_cumprod": r["ds"].sqrt_one_minus_alphas_cumprod.float().numpy()}
    for key in ("grads", "post", "ema", "m", "v"):
        out[key + "_norm"] = np.array([float(r[key][n].double().norm()) for n in names])
        out[key + "_proj"] = np.array([projection(n, r[key][n]) for n in names])
    for n in full:
        out["grad:" + n] = r["grads"][n].numpy()
        out["post:" + n] = r["post"][n].numpy()
    total = float(torch.sqrt(sum((g.double() ** 2).sum() for g in r["grads"].values())))
    out["grad_total_norm"] = np.float64(total)
    np.savez_compressed(os.path.join(HERE, name + ".npz"), **out)


if __name__ == "__main__":
    torch.set_num_threads(int(os.environ.get("T2P_GOLDEN_THREADS", "2")))
    for nm in (sys.argv[1:] or list(PLOSS_CASES)):
        fixture(nm)
