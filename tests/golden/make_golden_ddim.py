"""Generate the DDIM fixtures by running the REFERENCE's own DiffusionSampler (build container only).

    python tests/golden/make_golden_ddim.py

Loads this repo's synthetic weights into the reference ``UNetModel`` and runs ``model/diffusion_sampler.py`` (the copy that calls
``model(x, t, context)``, ``UNetModel.forward``'s order) on the CPU; ``betas=`` is passed so that its ``.to('cuda')`` is never
reached.  Only data is written: ``ddim_tiny_*.npz`` (context, noise draws, final sample, the clean-sample prediction of every
step, the run's sensitivity to evaluation error, the constructor's signature as names and defaults) and ``ddim_tables.npz`` (the
loop's per-step schedule for several lengths, strides and eta).  The GPU box never runs this script.
"""
import inspect
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)
sys.path.insert(0, "/root/reference")

from text2protein_amd.config import tiny_config            # noqa: E402
from text2protein_amd import synth                         # noqa: E402

from score_sde_pytorch.models import ncsnpp                # noqa: E402  (reference)
from score_sde_pytorch import sde_lib                      # noqa: E402  (reference)
from model.diffusion_sampler import DiffusionSampler       # noqa: E402  (reference)

B, T_CTX, SEED = 2, 3, 0
CASES = {  # name -> (sampling_steps, eta, w, scale_by_sigma)
    "ddim_tiny_a": (8, 1.0, 0.7, False),
    "ddim_tiny_b": (5, 0.5, 2.0, False),
    "ddim_tiny_c": (8, 0.0, 1.0, False),
    "ddim_tiny_sbs": (8, 1.0, 0.7, True),
}


def base_config(scale_by_sigma):
    return tiny_config(**{"model.num_scales": 40, "training.sde": "vpsde", "model.scale_by_sigma": scale_by_sigma})


def reference_model(cfg):
    torch.manual_seed(0)
    model = ncsnpp.UNetModel(cfg)
    missing, unexpected = model.load_state_dict(synth.synth_state_dict(cfg, SEED), strict=False)
    assert (list(missing) == ["sigmas"] or not missing) and not unexpected
    return model.eval()


def run_fixture(name, steps, eta, w, sbs):
    cfg = base_config(sbs)
    model = reference_model(cfg)
    shape = (B, cfg.data.num_channels, cfg.data.max_res_num, cfg.data.max_res_num)
    ctx = synth.synth_context(B, T_CTX, cfg.model.context_dim, SEED)
    betas = sde_lib.VPSDE(0.1, 20, 40).discrete_betas
    pattern = torch.from_numpy(np.sign(synth.uniform_pm1(SEED, "ddim_sens", int(np.prod(shape)))).reshape(shape)).float()

    def run(net):
        ds = DiffusionSampler(net, timesteps=40, betas=betas, sampling_steps=steps, ddim_eta=eta, w=w)
        x0s, draws, inner = [], [], ds.model_predictions

        def recording(*a, **k):
            pred, x_start = inner(*a, **k)
            x0s.append(x_start.detach().clone())
            return pred, x_start

        def keep(fn):                      # the run's own draws, in its own order and dtype
            def wrapped(*a, **k):
                z = fn(*a, **k)
                draws.append(z.clone())
                return z
            return wrapped

        ds.model_predictions = recording
        randn, randn_like = torch.randn, torch.randn_like
        torch.manual_seed(777 + steps)
        torch.randn, torch.randn_like = keep(randn), keep(randn_like)
        try:
            with torch.no_grad():
                out = ds.ddim_sample(shape, ctx)
        finally:
            torch.randn, torch.randn_like = randn, randn_like
        return out, x0s, draws

    out, x0s, draws = run(model)
    assert len(x0s) == steps and len(draws) == steps and bool(torch.isfinite(out).all())
    # seeding before the run and replaying the generator gives the same stream: the prior, then one draw per step but the last
    torch.manual_seed(777 + steps)
    replay = [torch.randn(shape)] + [torch.randn(shape, dtype=d.dtype) for d in draws[1:]]
    assert all(torch.equal(a, b) for a, b in zip(draws, replay))
    draws = [d.float() for d in draws]
    bumped, _, _ = run(lambda x, t, c: model(x, t, c) * (1 + 1e-6 * pattern))
    sens = float((bumped.double() - out.double()).norm() / out.double().norm()) / 1e-6
    on_clamp = float((out.abs() == 1).double().mean())
    print(f"[{name}] dtype {out.dtype}, |sample| rms {float(out.double().pow(2).mean().sqrt()):.4f}, on the clamp {on_clamp:.1%}, "
          f"sensitivity {sens:.3g}")
    sig = inspect.signature(DiffusionSampler.__init__)
    names = [p for p in sig.parameters if p != "self"]
    defaults = ["<required>" if sig.parameters[p].default is inspect.Parameter.empty else repr(sig.parameters[p].default)
                for p in names]
    np.savez_compressed(os.path.join(HERE, name + ".npz"), context=ctx.numpy(), noise=torch.stack(draws).numpy(),
                        sample=out.numpy(), x0=torch.stack(x0s).numpy(), sensitivity=np.float64(sens), steps=np.int64(steps),
                        eta=np.float64(eta), w=np.float64(w), scale_by_sigma=np.bool_(sbs), betas=betas.numpy(),
                        signature_names=np.array(names), signature_defaults=np.array(defaults))


class Probe(torch.nn.Module):
    """Stands in for the network: records the time label of every call."""

    def __init__(self):
        super().__init__()
        self.t = []

    def forward(self, x, t, c):
        self.t.append(int(t[0]))
        return torch.zeros_like(x)


def tables_fixture():
    out = {}
    for timesteps, steps in ((40, 8), (40, 7), (10, 10), (10, 15), (1000, 50), (1000, 1000)):     # (10, 15): repeated times
        for kind, betas in (("linear", torch.linspace(0.01, 0.2, timesteps)),
                            ("vpsde", sde_lib.VPSDE(0.1, 20, timesteps).discrete_betas)):
            for eta in (0.0, 0.5, 1.0):
                probe = Probe()
                ds = DiffusionSampler(probe, timesteps=timesteps, betas=betas, sampling_steps=steps, ddim_eta=eta, w=1.0)
                with torch.no_grad():
                    ds.ddim_sample((1, 1, 1, 1), torch.zeros(1, 1, 1))
                ts = probe.t[::2]                      # two calls per step
                assert len(ts) == steps
                t_next = ts[1:] + [-1]
                rows = {k: [] for k in ("alpha_bar", "alpha_next_bar", "sigma", "c", "sqrt_recip", "sqrt_recipm1")}
                for t, tn in zip(ts, t_next):
                    ab = ds.alphas_cumprod[t]
                    an = sg = c = torch.zeros(())
                    if tn >= 0:                        # the loop's own expressions on the sampler's own buffers
                        an = ds.alphas_cumprod[tn]
                        sg = torch.sqrt(eta * ((1 - ab / an) * (1 - an) / (1 - ab)))
                        c = torch.sqrt(1 - an - sg ** 2)
                    for k, v in (("alpha_bar", ab), ("alpha_next_bar", an), ("sigma", sg), ("c", c),
                                 ("sqrt_recip", ds.sqrt_recip_alphas_cumprod[t]), ("sqrt_recipm1", ds.sqrt_recipm1_alphas_cumprod[t])):
                        rows[k].append(float(v))
                key = f"{kind}_{timesteps}_{steps}_eta{eta}_"
                out[key + "t"] = np.array(ts, np.int64)
                out[key + "t_next"] = np.array(t_next, np.int64)
                for k, v in rows.items():
                    out[key + k] = np.array(v, np.float32)
    np.savez_compressed(os.path.join(HERE, "ddim_tables.npz"), **out)
    print(f"[ddim_tables] {len(out)} arrays written")


def main():
    torch.set_num_threads(8)
    for name, (steps, eta, w, sbs) in CASES.items():
        run_fixture(name, steps, eta, w, sbs)
    tables_fixture()


if __name__ == "__main__":
    main()
