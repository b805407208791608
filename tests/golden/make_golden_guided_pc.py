"""Generate the guided predictor-corrector fixtures by running the REFERENCE's own pc_sampler (build container only).

    python tests/golden/make_golden_guided_pc.py [case ...]

The guidance expression of the reference's second sampler, ``w * model(x, cond, t) + (1 - w) * model(x, cond * 0, t)``
(sampler/diffusion_sampler.py:128), is a property of the network output; the reference's ``get_pc_sampler`` takes any module, so a
guided PC run of the reference is its own ``sampling.get_sampling_fn(...)`` on a wrapper module with that forward, in the
``(x, labels, context)`` order of ``UNetModel.forward``.  This script loads the repo's synthetic weights into the reference
``UNetModel``, wraps it, runs the cases of tests/guided_oracle.py on the CPU with the draws recorded, and writes only data:
``guided_pc_*.npz`` (context, draws, the final sample, the unguided run on the same draws, the run's sensitivity to evaluation
error) and ``guided_pc_*_steps.npz`` (x / x_mean after every step).  It fails when a case would show nothing: the guided and the unguided sample must differ by at
least 20 times the float32 bound the tests hold the product to, and the sensitivity must stay below 10.  The GPU box never runs
this script.
"""
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, "/root/reference")

from text2protein_amd import synth                         # noqa: E402
import guided_oracle as GO                                 # noqa: E402

from score_sde_pytorch.models import ncsnpp                # noqa: E402  (reference)
from score_sde_pytorch import sde_lib, sampling            # noqa: E402  (reference)


class Guided(torch.nn.Module):
    """diffusion_sampler.py:128 as a module; ``bump`` scales every network output by (1 + bump) (the sensitivity run)."""

    def __init__(self, net, w, bump=None):
        super().__init__()
        self.net, self.w, self.bump, self.inputs = net, w, bump, []

    def one(self, x, labels, context):
        out = self.net(x, labels, context)
        return out if self.bump is None else out * (1 + self.bump)

    def forward(self, x, labels, context):
        self.inputs.append(x.detach().clone())
        if self.w is None:
            return self.one(x, labels, context)
        return self.w * self.one(x, labels, context) + (1 - self.w) * self.one(x, labels, context * 0)


def rel(a, b):
    return float((a.double() - b.double()).norm() / b.double().norm())


def run_fixture(name, case):
    cfg = GO.case_config(case)
    kind, w, k_each = case["sde"], case["w"], case["n_steps_each"]
    torch.manual_seed(0)
    net = ncsnpp.UNetModel(cfg)
    sd = synth.synth_state_dict(cfg, GO.SEED)
    missing, unexpected = net.load_state_dict(sd, strict=False)
    assert (list(missing) == ["sigmas"] or not missing) and not unexpected
    net.eval()
    N, L = cfg.model.num_scales, cfg.data.max_res_num
    shape = (GO.B, cfg.data.num_channels, L, L)
    ctx = synth.synth_context(GO.B, GO.T_CTX, cfg.model.context_dim, GO.SEED)
    if kind == "vesde":
        sde = sde_lib.VESDE(sigma_min=cfg.model.sigma_min, sigma_max=cfg.model.sigma_max, N=N)
    else:
        sde = sde_lib.VPSDE(beta_min=cfg.model.beta_min, beta_max=cfg.model.beta_max, N=N)
    fn = sampling.get_sampling_fn(cfg, sde, shape, GO.EPS[kind])
    pattern = torch.from_numpy(np.sign(synth.uniform_pm1(GO.SEED, "guided_pc_sens", int(np.prod(shape)))).reshape(shape)).float()
    seed = 2468 + int(round(10 * w)) + 100 * k_each

    draws = []

    def keep(fn_):                         # the run's own draws, in its own order and dtype
        def wrapped(*a, **k):
            z = fn_(*a, **k)
            draws.append(z.clone())
            return z
        return wrapped

    def run(module, record=False):
        torch.manual_seed(seed)
        randn, randn_like = torch.randn, torch.randn_like
        if record:
            torch.randn, torch.randn_like = keep(randn), keep(randn_like)
        try:
            with torch.no_grad():
                return fn(module, condition=GO.case_condition(case, L), context=ctx)
        finally:
            torch.randn, torch.randn_like = randn, randn_like

    wrapper = Guided(net, w)
    ref, nfe = run(wrapper, record=True)
    # (the second Langevin draw of a level is randn_like of a float64 state: another stream than float32 draws from the same seed)
    noise = torch.stack([d.float() for d in draws])
    assert nfe == N * (k_each + 1) == len(wrapper.inputs) and bool(torch.isfinite(ref).all())
    unguided, _ = run(Guided(net, None))
    bumped, _ = run(Guided(net, w, 1e-6 * pattern))
    sens = rel(bumped, ref) / 1e-6
    diff = rel(ref, unguided)
    # the same draws (as stored: float32) through the oracle's loop under the same expression, recording the state after every step
    trace = []
    got, nfe2 = GO.guided_pc_run(sd, cfg, shape, ctx, w, condition=GO.case_condition(case, L), noise_fn=GO.replay(noise), trace=trace)
    err = rel(got, ref)
    # the state the reference's own run handed to the first evaluation of step i + 1 is the oracle's x after step i
    per = k_each + 1
    step_err = max(rel(trace[i][0], wrapper.inputs[(i + 1) * per]) for i in range(N - 1))
    print(f"[{name}] guided vs unguided rel-L2 {diff:.3g} (needs {20 * GO.F32_TOL[kind]:.0e}), sensitivity {sens:.3g}, "
          f"oracle vs reference: sample {err:.2e}, worst per-step x {step_err:.2e}, nfe {nfe}")
    assert err < 1e-5 and step_err < 1e-5 and nfe2 == nfe and len(draws) == 1 + N * per
    assert diff >= 20 * GO.F32_TOL[kind], "the guided run is too close to the unguided one to be told apart"
    assert sens <= 10, "the run amplifies evaluation error too much to bound a float32 product"
    np.savez_compressed(os.path.join(HERE, name + ".npz"), context=ctx.numpy(), noise=noise.numpy(), sample=ref.numpy(),
                        unguided=unguided.numpy(), sensitivity=np.float64(sens), difference=np.float64(diff), w=np.float64(w),
                        nfe=np.int64(nfe))
    # (a file of its own: draws and states together pass the size limit of a committed file)
    np.savez_compressed(os.path.join(HERE, name + "_steps.npz"), x=torch.stack([t[0] for t in trace]).numpy().astype(np.float32),
                        x_mean=torch.stack([t[1] for t in trace]).numpy().astype(np.float32))


def main():
    torch.set_num_threads(8)
    for name, case in GO.CASES.items():
        if len(sys.argv) < 2 or name in sys.argv[1:]:     # (names on the command line: only those cases)
            run_fixture(name, case)


if __name__ == "__main__":
    main()
