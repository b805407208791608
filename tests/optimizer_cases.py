"""The optimizer / EMA matrix that no whole-step fixture reaches (tests/test_gpu_train_optimizer.py runs it on the GPU,
tests/test_cpu_optimizer.py pins its oracle and its bounds): weight decay, Adam update counts past the first, clipping off / inactive /
active, warm-up off / running / over, the early EMA decay.  No forward pass: random state is written into the smallest trainer
(helpers.cfg_ckpt, 136 405 parameters in 102 tensors), t2p_train_apply runs, everything is read back and compared with
oracle.adam_update / clip_coef / warmup_lr / ema_decay evaluated in float64 on the same fp32 inputs.
"""
import torch

from helpers import cfg_ckpt, rel_l2

WEIGHT_DECAY = (0.0, 1e-2)
ADAM_K = (1, 2, 1000)                     # the update about to be made: the bias corrections 1 - beta^k
CLIP = ("off", "below", "above")          # grad_clip -1; 1.0 with the gradient norm below it; 1.0 with the norm above it
WARMUP = ((0.0, 3000), (5000.0, 2000), (5000.0, 7000))      # (optim.warmup, state['step'] before the update): off, running, over
EMA_UPDATES = (0, 5, 10_000)              # ema.num_updates before the update: min(ema_rate = 0.999, (1 + k) / (10 + k)) = 0.18 / 0.4375 / 0.999 (0.99910 is past it)

QUANTITIES = ("g", "update", "m", "v", "ema")
# Bounds (rel-L2 per tensor against the float64 oracle): 4x the worst rel-L2 of the SAME oracle formulas evaluated in float32 on the CPU
# against float64 over the whole matrix on these inputs -- the kernel uses the same handful of fp32 operations in a possibly different
# association.  Measured, with the case (weight decay, clip, warm-up, step, k, EMA updates) that gave it (tests/test_cpu_optimizer.py
# re-measures these cases and an eighth of the matrix and holds the constants to it):
#   g (the clipped gradient read back)  4.09e-8   update (p_after - p_before)  3.23e-4 (*)   m  7.77e-8   v  7.42e-8   ema  1.25e-7
# (*) the update is lr-sized (4e-5 while the warm-up runs) on parameters of size 0.1, whose fp32 spacing is 7e-9: rounding p_after alone
# is 1e-4 of the update.  m and v are what pins the arithmetic of the update to 1e-7; this row pins its size, sign and bias corrections.
MEASURED = {"g": 4.09e-8, "update": 3.23e-4, "m": 7.77e-8, "v": 7.42e-8, "ema": 1.25e-7}
WORST_CASES = {"g": (0.0, "above", 0.0, 3000, 1, 0), "update": (0.01, "below", 5000.0, 2000, 2, 0), "m": (0.01, "above", 0.0, 3000, 1, 0),
               "v": (0.0, "off", 0.0, 3000, 1, 0), "ema": (0.0, "off", 5000.0, 2000, 2, 0)}
BOUND = {q: 4.0 * v for q, v in MEASURED.items()}


def cfg_optimizer(weight_decay, clip, warmup):
    cfg = cfg_ckpt()
    cfg.model.dropout = 0.0
    cfg.optim.weight_decay = weight_decay
    cfg.optim.grad_clip = -1.0 if clip == "off" else 1.0
    cfg.optim.warmup = warmup
    return cfg


def draw_state(table, clip, seed=0):
    """name -> fp32 tensor for the five buffers.  |g| lies in [1e-3, 1] (log-uniform; with clip == "below" uniform in [1e-3, 2e-3], which
    puts the total norm of 136 405 elements at 0.56 < 1), random signs: no element in the sign-like regime |g| ~ eps that the
    whole-step tests have to excuse.  Parameters ~ 0.1 N(0, 1), EMA shadow 0.1 away from them, both moments as after earlier updates
    (m ~ 0.1 N(0, 1), v in [1e-4, 1e-2])."""
    gen = torch.Generator().manual_seed(1234 + seed)
    st = {k: {} for k in ("p", "g", "m", "v", "e")}
    for name, shape in table:
        u = torch.rand(shape, generator=gen, dtype=torch.float64)
        mag = 1e-3 * (1.0 + u) if clip == "below" else 10.0 ** (-3.0 * u)
        st["g"][name] = (mag * torch.where(torch.rand(shape, generator=gen) < 0.5, -1.0, 1.0)).float()
        st["p"][name] = 0.1 * torch.randn(shape, generator=gen)
        st["e"][name] = st["p"][name] + 0.1 * torch.randn(shape, generator=gen)
        st["m"][name] = 0.1 * torch.randn(shape, generator=gen)
        st["v"][name] = 1e-4 + (1e-2 - 1e-4) * torch.rand(shape, generator=gen)
    return st


def grad_norm(st):
    return float(torch.sqrt(sum((g.double() ** 2).sum() for g in st["g"].values())))


def oracle_apply(cfg, st, step, adam_k, ema_updates, dtype):
    """optimize_fn + ema.update (oracle.train_step's tail) on copies of ``st`` in ``dtype``: ``adam_k`` is the number of the update made
    here, ``step`` / ``ema_updates`` the counters before it.  Returns name -> tensor for g (as clip_grad_norm_ leaves it), p, m, v, ema
    and the update p_after - p_before."""
    from oracle import t2p_oracle as O
    o = cfg.optim
    names = list(st["p"])
    c = {k: {n: st[k][n].to(dtype).clone() for n in names} for k in st}
    lr = O.warmup_lr(cfg, step)
    if o.grad_clip >= 0:
        coef, _ = O.clip_coef([c["g"][n] for n in names], o.grad_clip)
        for n in names:
            c["g"][n].mul_(coef.to(dtype))
    for n in names:
        O.adam_update(c["p"][n], c["g"][n], c["m"][n], c["v"][n], adam_k, lr, o.beta1, 0.999, o.eps, o.weight_decay)
    d = O.ema_decay(cfg.model.ema_rate, ema_updates + 1)
    for n in names:
        c["e"][n].sub_((1.0 - d) * (c["e"][n] - c["p"][n]))
    return {"g": c["g"], "p": c["p"], "m": c["m"], "v": c["v"], "ema": c["e"],
            "update": {n: c["p"][n] - st["p"][n].to(dtype) for n in names}}


def worst_errors(got, ref):
    """Worst rel-L2 over the tensors, per quantity of QUANTITIES; ``got`` / ``ref``: quantity -> name -> tensor."""
    return {q: max(rel_l2(got[q][n], ref[q][n]) for n in ref[q]) for q in QUANTITIES}


def matrix():
    for wd in WEIGHT_DECAY:
        for clip in CLIP:
            for warmup, step in WARMUP:
                for k in ADAM_K:
                    for ema_updates in EMA_UPDATES:
                        yield wd, clip, warmup, step, k, ema_updates
