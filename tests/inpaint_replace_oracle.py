"""CPU restatement of a replacement-inpainting run (reference score_sde_pytorch/inpainting.py, get_pc_inpainter), for the fixtures
of tests/golden/make_golden_inpaint_replace.py and the tests that read them.  Built from the untouched pieces of
``oracle.t2p_oracle`` (``unet_forward`` through its score functions, ``langevin_update``, ``reverse_diffusion_update``,
``vp_tables``, ``timesteps``); guidance enters as in tests/guided_oracle.py.  The loop, for an update U (the whole corrector, then
the predictor) at level i:

    x, x_mean = U(x, t_i)
    r      = a_i d + z s_i            (a_i d, s_i) = sde.marginal_prob(d, t_i); z: one fresh draw per U
    x      = known ? r : x
    x_mean = known ? a_i d : x        (the NEW x off the known region: inpainting.py:46)

from ``x = known ? d : prior``.  Extension: under a condition, an element it freezes stays x_initial; known applies to the rest.
"""
import numpy as np
import torch

import guided_oracle as GO
from oracle import t2p_oracle as O
from text2protein_amd import synth
from text2protein_amd.config import tiny_config

B, T_CTX, SEED = GO.B, GO.T_CTX, GO.SEED
# name -> the run.  20 noise levels at 4 draws per level (16 at 5 for the two-corrector-step run): 80 stored draws and the prior,
# the count of the guided fixtures, which keeps each file within the size limit of a committed file.
CASES = {
    "inpaint_replace_ve": dict(sde="vesde", w=None, length=False, n_steps_each=1, num_scales=20),
    "inpaint_replace_vp": dict(sde="vpsde", w=None, length=False, n_steps_each=1, num_scales=20),
    "inpaint_replace_ve_length": dict(sde="vesde", w=None, length=True, n_steps_each=1, num_scales=20),
    "inpaint_replace_ve_n2": dict(sde="vesde", w=None, length=False, n_steps_each=2, num_scales=16),
    "inpaint_replace_ve_w3": dict(sde="vesde", w=3.0, length=False, n_steps_each=1, num_scales=20),
}
F32_TOL, EPS = GO.F32_TOL, GO.EPS
case_config, case_condition = GO.case_config, GO.case_condition


def case_data(case, config):
    """(data, known) of a case: U(-1, 1) maps and a block of known entries per sample whose edges (columns 3 / 10 and 5 / 11) cut
    through quads of four consecutive elements; under the length condition the block lies inside the 12 x 12 free square and off
    the last channel, which that condition freezes."""
    C, L = config.data.num_channels, config.data.max_res_num
    data = torch.from_numpy(synth.uniform_pm1(SEED, "inpaint_replace_data", B * C * L * L).reshape(B, C, L, L)).float()
    known = torch.zeros(B, C, L, L, dtype=torch.bool)
    chans = slice(0, C - 1) if case["length"] else slice(0, C)
    known[0, chans, 2:9, 3:10] = True
    known[1, chans, 1:7, 5:11] = True
    return data, known


def marginal_tables(config, eps):
    """(mean_coef, std), float32[N]: sde.marginal_prob at t_i = linspace(T, eps, N)[i] (sde_lib.py:134-138, :224-227)."""
    m = config.model
    ts = O.timesteps(m.num_scales, eps)
    if config.training.sde == "vesde":
        return torch.ones(m.num_scales), O.ve_marginal_std(ts, m.sigma_min, m.sigma_max)
    lmc = -0.25 * ts ** 2 * (m.beta_max - m.beta_min) - 0.5 * ts * m.beta_min
    return torch.exp(lmc), torch.sqrt(1. - torch.exp(2. * lmc))


def replace(x, data, known, free, a, s, z):
    """The replacement after an update -> (x, x_mean); ``free``: the condition's mask (1 = the chain evolves)."""
    mean = a * data
    r = mean + z * s
    rep = known & free
    x = torch.where(rep, r, x)
    return x, torch.where(rep, mean, x)


def inpaint_run(sd, config, shape, context, data, known, w=None, condition=None, noise_fn=None, trace=None, n_steps_limit=None):
    """-> (sample, nfe).  ``noise_fn(shape)`` hands out the draws in the reference's order: prior, then per level the corrector's
    Langevin draws, the replacement after it, the predictor's draw, the replacement after it."""
    m, s = config.model, config.sampling
    kind, N = config.training.sde, config.model.num_scales
    eps = EPS[kind]
    ts = O.timesteps(N, eps)
    a_tab, s_tab = marginal_tables(config, eps)
    vp = O.vp_tables(m.beta_min, m.beta_max, N) if kind == "vpsde" else None
    dsig = O.ve_discrete_sigmas(m.sigma_min, m.sigma_max, N)

    def score_fn(x, t):
        if kind == "vesde":
            return O.score_fn_ve(sd, config, x, t, context)
        labels = t * (N - 1)
        out = O.unet_forward(sd, config, x, labels, context)
        return -out / vp["sqrt_1m_alphas_cumprod"][labels.long()][:, None, None, None]

    with torch.no_grad(), GO.guided_network(w):
        x = noise_fn(shape) * (m.sigma_max if kind == "vesde" else 1.0)
        x = torch.where(known, data, x)
        x, free = O.apply_conditions(x, condition)
        x_initial = x.detach().clone()
        x_mean = x
        for i in range(N if n_steps_limit is None else n_steps_limit):
            vec_t = torch.ones(shape[0]) * ts[i]
            k = (vec_t * (N - 1)).long()
            alpha = vp["alphas"][k][0] if vp else 1.0
            for _ in range(s.n_steps_each):
                grad = score_fn(x, vec_t)
                x, x_mean = O.langevin_update(x, grad, noise_fn(tuple(x.shape)), s.snr, alpha)
            x = torch.where(free, x, x_initial).float()
            x, x_mean = replace(x, data, known, free, a_tab[i], s_tab[i], noise_fn(tuple(x.shape)))
            score = score_fn(x, vec_t)
            z = noise_fn(tuple(x.shape))
            if vp:
                f = torch.sqrt(vp["alphas"][k])[:, None, None, None] * x - x
                x, x_mean = O.reverse_diffusion_update(x, score, z, torch.sqrt(vp["discrete_betas"][k]), s.probability_flow, f=f)
            else:
                x, x_mean = O.reverse_diffusion_update(x, score, z, O.ve_discretize_G(vec_t, dsig, N), s.probability_flow)
            x = torch.where(free, x, x_initial).float()
            x, x_mean = replace(x, data, known, free, a_tab[i], s_tab[i], noise_fn(tuple(x.shape)))
            if trace is not None:
                trace.append((x.clone(), x_mean.clone()))
        return (x_mean if s.noise_removal else x), N * (s.n_steps_each + 1)


replay = GO.replay


def load(name, golden_dir):
    """The two fixture files of a case as dicts of numpy arrays."""
    import os
    with np.load(os.path.join(golden_dir, name + ".npz")) as f, np.load(os.path.join(golden_dir, name + "_steps.npz")) as g:
        return {k: f[k] for k in f.files}, {k: g[k] for k in g.files}
