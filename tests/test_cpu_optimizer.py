"""The optimizer oracle away from the fixtures' single update, on the CPU: oracle.adam_update with weight decay and update counts
past the first against torch.optim.Adam itself, as the reference's get_optimizer constructs it (losses.py:26-36) and optimize_fn drives
it (:41-49); and the float32-against-float64 error of the oracle formulas that tests/optimizer_cases.py turns into the bounds of the
GPU optimizer matrix (tests/test_gpu_train_optimizer.py)."""
import pytest
import torch

import optimizer_cases as OC
from helpers import rel_l2


@pytest.mark.parametrize("weight_decay", [0.0, 1e-2])
@pytest.mark.parametrize("dtype,tol", [(torch.float64, 1e-13), (torch.float32, 1e-6)])
def test_oracle_adam_update_is_torch_adam_over_three_updates(weight_decay, dtype, tol):
    """Three consecutive updates (k = 1, 2, 3) with a fresh gradient and the warm-up's learning rate each time.  float64: the two agree
    to rounding (1e-13); float32: to a few ulp of the parameters (torch's Adam folds the same formula with lerp / addcdiv)."""
    from oracle import t2p_oracle as O
    cfg = OC.cfg_optimizer(weight_decay, "off", 5000.0)
    o = cfg.optim
    gen = torch.Generator().manual_seed(3)
    shapes = [(7, 5), (33,), (4, 3, 3, 3)]
    p0 = [0.1 * torch.randn(s, generator=gen, dtype=torch.float64).to(dtype) for s in shapes]
    params = [torch.nn.Parameter(p.clone()) for p in p0]
    opt = torch.optim.Adam(params, lr=o.lr, betas=(o.beta1, 0.999), eps=o.eps, weight_decay=o.weight_decay)      # get_optimizer
    mine = [p.clone() for p in p0]
    m = [torch.zeros_like(p) for p in p0]
    v = [torch.zeros_like(p) for p in p0]
    for k, step in ((1, 1000), (2, 1001), (3, 6000)):
        grads = [(10.0 ** (-3.0 * torch.rand(s, generator=gen, dtype=torch.float64)) *
                  torch.where(torch.rand(s, generator=gen) < 0.5, -1.0, 1.0)).to(dtype) for s in shapes]
        lr = O.warmup_lr(cfg, step)
        for grp in opt.param_groups:                                      # optimize_fn, losses.py:44-46
            grp["lr"] = lr
        for p, g in zip(params, grads):
            p.grad = g.clone()
        opt.step()
        for i, g in enumerate(grads):
            O.adam_update(mine[i], g, m[i], v[i], k, lr, o.beta1, 0.999, o.eps, o.weight_decay)
        for i, p in enumerate(params):
            st = opt.state[p]
            assert int(st["step"]) == k
            assert rel_l2(mine[i], p.detach()) < tol and rel_l2(mine[i] - p0[i], p.detach() - p0[i]) < (tol if dtype == torch.float64 else 1e-3)
            assert rel_l2(m[i], st["exp_avg"]) < tol and rel_l2(v[i], st["exp_avg_sq"]) < tol
    if weight_decay:                                                      # the branch is live: without it the moments differ at 1e-3
        g0, m0, v0, q = grads[0], torch.zeros_like(p0[0]), torch.zeros_like(p0[0]), p0[0].clone()
        O.adam_update(q, g0, m0, v0, 1, o.lr, o.beta1, 0.999, o.eps, 0.0)
        m1, v1, q1 = torch.zeros_like(p0[0]), torch.zeros_like(p0[0]), p0[0].clone()
        O.adam_update(q1, g0, m1, v1, 1, o.lr, o.beta1, 0.999, o.eps, weight_decay)
        assert rel_l2(m1, m0) > 1e-4


def test_oracle_schedule_pieces():
    from oracle import t2p_oracle as O
    assert O.ema_decay(0.999, 1) == 2 / 11 and O.ema_decay(0.999, 6) == 7 / 16 and O.ema_decay(0.999, 10_001) == 0.999
    assert O.ema_decay(0.9999, 10_001) == 10_002 / 10_011
    cfg = OC.cfg_optimizer(0.0, "above", 5000.0)
    assert O.warmup_lr(cfg, 2000) == cfg.optim.lr * 0.4 and O.warmup_lr(cfg, 7000) == cfg.optim.lr
    assert O.warmup_lr(OC.cfg_optimizer(0.0, "above", 0.0), 3000) == cfg.optim.lr
    g = [torch.full((4,), 3.0), torch.full((9,), -4.0 / 3.0)]           # norm sqrt(36 + 16) = 7.2111
    c, total = O.clip_coef(g, 1.0)
    assert abs(float(total) - 52 ** 0.5) < 1e-6 and abs(float(c) - 1 / (52 ** 0.5 + 1e-6)) < 1e-7
    assert float(O.clip_coef(g, 10.0)[0]) == 1.0


def test_gpu_matrix_bounds_cover_the_float32_oracle_error():
    """Re-measures what optimizer_cases.MEASURED records (the recorded worst case of every quantity and an eighth of the matrix): no case
    exceeds the recorded figure (5 % slack: the inputs pass through pow and randn, which may differ in the last bit between hosts), so
    the GPU bounds, 4x MEASURED, stay at least 3.8x what the float32 oracle shows on the host that runs this."""
    from text2protein_amd.arch import param_specs
    table = None
    states = {}
    cases = list(OC.matrix())[::8] + list(OC.WORST_CASES.values())
    seen = {q: 0.0 for q in OC.QUANTITIES}
    for case in cases:
        wd, clip, warmup, step, k, eu = case
        cfg = OC.cfg_optimizer(wd, clip, warmup)
        if table is None:
            table = [(s.name, tuple(s.shape)) for s in param_specs(cfg)]
            assert sum(int(torch.Size(s).numel()) for _, s in table) == 136405
        if clip not in states:
            states[clip] = OC.draw_state(table, clip)
            norm = OC.grad_norm(states[clip])
            assert (norm < 1.0) if clip == "below" else (norm > 1.0), (clip, norm)
            assert all(1e-3 * (1 - 1e-6) <= float(g.abs().min()) and float(g.abs().max()) <= 1.0 for g in states[clip]["g"].values())
        e = OC.worst_errors(OC.oracle_apply(cfg, states[clip], step, k, eu, torch.float32),
                            OC.oracle_apply(cfg, states[clip], step, k, eu, torch.float64))
        for q in OC.QUANTITIES:
            seen[q] = max(seen[q], e[q])
    print("float32 oracle against float64, worst rel-L2 per tensor:", {q: f"{v:.2e}" for q, v in seen.items()})
    for q in OC.QUANTITIES:
        assert 0.0 < seen[q] <= 1.05 * OC.MEASURED[q], (q, seen[q], OC.MEASURED[q])
