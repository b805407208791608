"""CPU restatement of a guided predictor-corrector run, for the fixtures of tests/golden/make_golden_guided_pc.py and the tests that
read them.  The loops are those of ``oracle.t2p_oracle`` (``pc_sampler_ve`` / ``pc_sampler_vp``), untouched: for the length of a
run their network, ``unet_forward``, is replaced by the guidance expression of the reference's sampler/diffusion_sampler.py:128
on that same function,

    w * unet_forward(x, labels, context) + (1 - w) * unet_forward(x, labels, context * 0)
"""
import contextlib

import torch

from oracle import t2p_oracle as O
from text2protein_amd.config import tiny_config

B, T_CTX, SEED = 2, 3, 0
# name -> the run: SDE, guidance weight, the 12 x 12 length condition, Langevin steps per level, noise levels.  40 levels: the 5 of
# the tiny_sampler_* fixtures move a w = 0.7 run only 4e-4 away from the unguided one.  (The two-corrector-step run has 3 draws per
# level: 24 levels keep its file within the size limit of a committed file.)
CASES = {
    "guided_pc_ve_w07": dict(sde="vesde", w=0.7, length=False, n_steps_each=1, num_scales=40),
    "guided_pc_ve_w3_length": dict(sde="vesde", w=3.0, length=True, n_steps_each=1, num_scales=40),
    "guided_pc_ve_wm1": dict(sde="vesde", w=-1.0, length=False, n_steps_each=1, num_scales=40),
    "guided_pc_vp_w07": dict(sde="vpsde", w=0.7, length=False, n_steps_each=1, num_scales=40),
    "guided_pc_vp_w2_length": dict(sde="vpsde", w=2.0, length=True, n_steps_each=1, num_scales=40),
    "guided_pc_ve_w3_n2": dict(sde="vesde", w=3.0, length=False, n_steps_each=2, num_scales=24),
}
# the bound of the unguided tiny runs in float32: relative L2 of the sample (SAMPLE_TOL["f32"] of test_gpu_sampler; the VP run of
# test_vp_sde_route_matches_reference_run)
F32_TOL = {"vesde": 1e-5, "vpsde": 1e-4}
EPS = {"vesde": 1e-5, "vpsde": 1e-3}


def case_config(case):
    return tiny_config(**{"model.num_scales": case["num_scales"], "training.sde": case["sde"], "sampling.n_steps_each": case["n_steps_each"]})


def case_condition(case, L):
    if not case["length"]:
        return {}
    m = torch.zeros(B, L, L).bool()
    m[:, :12, :12] = True
    return {"length": m}


@contextlib.contextmanager
def guided_network(w):
    """``oracle.t2p_oracle.unet_forward`` gives the guided output while the block runs (``w`` None: unchanged)."""
    plain = O.unet_forward

    def guided(P, config, x, labels, context, *a, **k):
        return w * plain(P, config, x, labels, context, *a, **k) + (1 - w) * plain(P, config, x, labels, context * 0, *a, **k)

    if w is not None:
        O.unet_forward = guided
    try:
        yield
    finally:
        O.unet_forward = plain


def guided_pc_run(sd, config, shape, context, w, condition=None, noise_fn=None, trace=None, n_steps_limit=None):
    """-> (sample, nfe) of the oracle's PC loop for ``config.training.sde`` under guidance weight ``w`` (None: the plain run)."""
    kind = config.training.sde
    run = O.pc_sampler_ve if kind == "vesde" else O.pc_sampler_vp
    with guided_network(w):
        return run(sd, config, shape, context, condition=condition, eps=EPS[kind], noise_fn=noise_fn, trace=trace,
                   n_steps_limit=n_steps_limit)


def replay(noise):
    """``noise_fn`` handing out the stored draws in order."""
    it = iter(torch.as_tensor(noise))
    return lambda shape: next(it).reshape(tuple(shape)).clone()
