"""Generate the replacement-inpainting fixtures by running the REFERENCE's own pc_inpainter body (build container only).

    python tests/golden/make_golden_inpaint_replace.py [case ...]

The reference's ``score_sde_pytorch/inpainting.py::get_pc_inpainter`` cannot run as shipped: it passes ``continuous=`` to
``shared_predictor_update_fn`` / ``shared_corrector_update_fn``, which do not take it, and no ``context``.  Its body is built from
pieces the reference does run, so this script imports the module and replaces those two names *in the imported module* with
adapters that drop ``continuous``, bind the context and call the reference's own ``sampling.shared_*_update_fn``; everything else
(the replacement, the initial state, the loop, the draws) is the reference's code.  Guidance wraps the network as
make_golden_guided_pc.py does.  For the case under a length condition the adapters re-mask after each update and the prior is
conditioned, as the reference's pc_sampler does (sampling.py:259-285); the known block lies inside the free region.

Written: only data.  ``inpaint_replace_*.npz`` (context, data, known, the draws in order, the sample, the plain PC run on the same
seed, the run's sensitivity to evaluation error, the mean_coef / std tables of the reference's ``marginal_prob``, a probe of the host's exp) and
``inpaint_replace_*_steps.npz`` (x / x_mean after every step, from the oracle helper on the same draws).  It fails when a case
would show nothing: the replaced and the plain sample must differ by at least 20 times the float32 bound the tests hold the
product to, the sensitivity must stay below 10, and tests/inpaint_replace_oracle.py must agree with the reference to 1e-5 after
every step and at the end.  The GPU box never runs this script.
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
import inpaint_replace_oracle as IO                        # noqa: E402
from oracle import t2p_oracle as O                         # noqa: E402

from score_sde_pytorch.models import ncsnpp                # noqa: E402  (reference)
from score_sde_pytorch import sde_lib, sampling            # noqa: E402  (reference)
from score_sde_pytorch import inpainting as ref_inpainting  # noqa: E402  (reference)
from make_golden_guided_pc import Guided, rel              # noqa: E402


def run_fixture(name, case):
    cfg = IO.case_config(case)
    kind, w, k_each = case["sde"], case["w"], case["n_steps_each"]
    torch.manual_seed(0)
    net = ncsnpp.UNetModel(cfg)
    sd = synth.synth_state_dict(cfg, IO.SEED)
    missing, unexpected = net.load_state_dict(sd, strict=False)
    assert (list(missing) == ["sigmas"] or not missing) and not unexpected
    net.eval()
    N, L = cfg.model.num_scales, cfg.data.max_res_num
    shape = (IO.B, cfg.data.num_channels, L, L)
    ctx = synth.synth_context(IO.B, IO.T_CTX, cfg.model.context_dim, IO.SEED)
    data, known = IO.case_data(case, cfg)
    condition = IO.case_condition(case, L)
    if kind == "vesde":
        sde = sde_lib.VESDE(sigma_min=cfg.model.sigma_min, sigma_max=cfg.model.sigma_max, N=N)
    else:
        sde = sde_lib.VPSDE(beta_min=cfg.model.beta_min, beta_max=cfg.model.beta_max, N=N)
    eps = IO.EPS[kind]
    _, free = O.apply_conditions(torch.zeros(shape), condition)
    x_initial, _ = O.apply_conditions(torch.zeros(shape), condition)

    def remask(xs):                        # sampling.py:283,285 (an identity without a condition)
        x, x_mean = xs
        return torch.where(free, x, x_initial).to(x.dtype), x_mean

    def predictor_adapter(x, t, model, sde, predictor, probability_flow, continuous):
        return remask(sampling.shared_predictor_update_fn(x, t, ctx, sde, model, predictor, probability_flow))

    def corrector_adapter(x, t, model, sde, corrector, continuous, snr, n_steps):
        return remask(sampling.shared_corrector_update_fn(x, t, ctx, sde, model, corrector, snr, n_steps))

    ref_inpainting.shared_predictor_update_fn = predictor_adapter
    ref_inpainting.shared_corrector_update_fn = corrector_adapter
    inpainter = ref_inpainting.get_pc_inpainter(sde, sampling.get_predictor(cfg.sampling.predictor.lower()),
                                                sampling.get_corrector(cfg.sampling.corrector.lower()), cfg.sampling.snr,
                                                n_steps=k_each, probability_flow=cfg.sampling.probability_flow, continuous=False,
                                                denoise=cfg.sampling.noise_removal, eps=eps)
    plain_fn = sampling.get_sampling_fn(cfg, sde, shape, eps)
    pattern = torch.from_numpy(np.sign(synth.uniform_pm1(IO.SEED, "inpaint_replace_sens", int(np.prod(shape)))).reshape(shape)).float()
    seed = 1357 + int(round(10 * (w or 0))) + 100 * k_each

    draws = []

    def keep(fn_):
        def wrapped(*a, **k):
            z = fn_(*a, **k)
            draws.append(z.clone())
            return z
        return wrapped

    prior_sampling = sde.prior_sampling

    def conditioned_prior(shp):            # sampling.py:253-277: the prior goes through the condition before the loop
        return O.apply_conditions(prior_sampling(shp), condition)[0]

    def run(module, record=False, inpaint=True):
        torch.manual_seed(seed)
        randn, randn_like = torch.randn, torch.randn_like
        if record:
            torch.randn, torch.randn_like = keep(randn), keep(randn_like)
        sde.prior_sampling = conditioned_prior
        try:
            with torch.no_grad():
                if inpaint:
                    return inpainter(module, data, known.float())
                return plain_fn(module, condition=condition, context=ctx)[0]
        finally:
            torch.randn, torch.randn_like = randn, randn_like
            sde.prior_sampling = prior_sampling

    wrapper = Guided(net, w)
    ref = run(wrapper, record=True)
    noise = torch.stack([d.float() for d in draws])
    per = k_each + 1
    nfe = N * per
    assert nfe == len(wrapper.inputs) and bool(torch.isfinite(ref).all()) and len(draws) == 1 + N * (per + 2)
    sde.prior_sampling = prior_sampling
    plain = run(Guided(net, w), inpaint=False)
    bumped = run(Guided(net, w, 1e-6 * pattern))
    sens = rel(bumped, ref) / 1e-6
    diff = rel(ref, plain)
    trace = []
    got, nfe2 = IO.inpaint_run(sd, cfg, shape, ctx, data, known, w=w, condition=condition, noise_fn=IO.replay(noise), trace=trace)
    err = rel(got, ref)
    step_err = max(rel(trace[i][0], wrapper.inputs[(i + 1) * per]) for i in range(N - 1))
    # the tables of the reference's marginal_prob, per level, on a unit "image"
    ts = torch.linspace(sde.T, eps, N)
    one = torch.ones(1, 1, 1, 1)
    pairs = [sde.marginal_prob(one, torch.ones(1) * t) for t in ts]
    mean_coef = torch.stack([p[0].reshape(()) for p in pairs]).float()
    std = torch.stack([p[1].reshape(()) for p in pairs]).float()
    a_tab, s_tab = IO.marginal_tables(cfg, eps)
    assert torch.equal(a_tab.float(), mean_coef) and torch.equal(s_tab.float(), std), "the oracle's tables are not the reference's"
    print(f"[{name}] replaced vs plain rel-L2 {diff:.3g} (needs {20 * IO.F32_TOL[kind]:.0e}), sensitivity {sens:.3g}, "
          f"oracle vs reference: sample {err:.2e}, worst per-step x {step_err:.2e}, nfe {nfe}, draws {len(draws)}")
    assert err < 1e-5 and step_err < 1e-5 and nfe2 == nfe
    assert diff >= 20 * IO.F32_TOL[kind], "the replaced run is too close to the plain one to be told apart"
    assert sens <= 10, "the run amplifies evaluation error too much to bound a float32 product"
    np.savez_compressed(os.path.join(HERE, name + ".npz"), context=ctx.numpy(), data=data.numpy(), known=known.numpy().astype(np.uint8),
                        noise=noise.numpy(), sample=ref.numpy(), plain=plain.numpy(), sensitivity=np.float64(sens),
                        difference=np.float64(diff), w=np.float64(np.nan if w is None else w), nfe=np.int64(nfe),
                        mean_coef=mean_coef.numpy(), std=std.numpy(),
                        # exp on this host, for a reader to tell whether its own float32 exp rounds as the writer's did
                        exp_probe=torch.exp(torch.linspace(-3, 0, 20)).numpy())
    np.savez_compressed(os.path.join(HERE, name + "_steps.npz"), x=torch.stack([t[0] for t in trace]).numpy().astype(np.float32),
                        x_mean=torch.stack([t[1] for t in trace]).numpy().astype(np.float32))


def main():
    torch.set_num_threads(8)
    for name, case in IO.CASES.items():
        if len(sys.argv) < 2 or name in sys.argv[1:]:
            run_fixture(name, case)


if __name__ == "__main__":
    main()
