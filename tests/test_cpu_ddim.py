"""The DDIM sampler's host side (text2protein_amd/ddim.py, sampling_6d.py --sampler ddim): schedule tables against the
reference's, the constructor's surface, refusals, the C ABI's declarations.  No GPU."""
import inspect
import os
import re
import subprocess
import sys

import numpy as np
import pytest
import torch
import yaml

from helpers import F32_HOST_RTOL, assert_table_close, load_golden

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FLOAT_KEYS = ("alpha_bar", "alpha_next_bar", "sigma", "c", "sqrt_recip", "sqrt_recipm1")


def _betas(kind, timesteps):
    from text2protein_amd import sde_lib
    return None if kind == "linear" else sde_lib.VPSDE(0.1, 20, timesteps).discrete_betas


@pytest.mark.parametrize("timesteps,steps", [(40, 8), (40, 7), (10, 10), (10, 15), (1000, 50), (1000, 1000)])
@pytest.mark.parametrize("kind", ["linear", "vpsde"])
def test_step_tables_match_the_reference(timesteps, steps, kind):
    from text2protein_amd.ddim import DiffusionSampler
    g = load_golden("ddim_tables")
    for eta in (0.0, 0.5, 1.0):
        key = f"{kind}_{timesteps}_{steps}_eta{eta}_"
        ds = DiffusionSampler(None, timesteps=timesteps, betas=_betas(kind, timesteps), sampling_steps=steps, ddim_eta=eta)
        tab = ds.step_table()
        # integers exactly: the truncated linspace, its duplicates and the closing t_next = -1
        assert tab["t"] == g[key + "t"].tolist() and tab["t_next"] == g[key + "t_next"].tolist()
        assert tab["t_next"][-1] == -1 and tab["last"] == [0] * (steps - 1) + [1] and tab["t"][0] == timesteps - 1
        for k in FLOAT_KEYS:
            got, want = np.asarray(tab[k], np.float64), g[key + k].astype(np.float64)
            # compared as they are: zeros (eta = 0, a repeated time, the unused entries of the last row) and what the reference's
            # float32 schedule turns into inf / NaN once alphas_cumprod underflows (the default betas over 1000 steps)
            exact = (want == 0) | ~np.isfinite(want)
            assert np.array_equal(got[exact], want[exact], equal_nan=True), k
            if (~exact).any():
                assert_table_close(got[~exact], want[~exact], F32_HOST_RTOL)
        an = g[key + "alpha_next_bar"].astype(np.float64)
        live = (np.asarray(tab["t_next"]) >= 0) & (an > 1e-30)
        assert_table_close(np.asarray(tab["sqrt_an"])[live] ** 2, an[live], 4 * F32_HOST_RTOL)


def test_duplicate_times_when_steps_exceed_the_stride():
    from text2protein_amd.ddim import DiffusionSampler
    g = load_golden("ddim_tables")
    t = g["linear_10_15_eta1.0_t"].tolist()
    assert len(t) == 15 and len(set(t)) < 15               # the fixture really holds repeated times
    tab = DiffusionSampler(None, timesteps=10, sampling_steps=15).step_table()
    assert tab["t"] == t
    rep = [i for i in range(14) if tab["t"][i] == tab["t_next"][i]]
    assert rep and all(tab["sigma"][i] == 0.0 for i in rep)       # alpha_bar / alpha_next_bar == 1: no noise on a repeated time


def test_default_schedule_is_linear_whatever_beta_schedule_says():
    from text2protein_amd.ddim import DiffusionSampler
    a = DiffusionSampler(None, timesteps=50)
    b = DiffusionSampler(None, timesteps=50, beta_schedule="cosine")
    assert torch.equal(a.betas, torch.linspace(0.01, 0.2, 50)) and torch.equal(a.betas, b.betas)
    for name in ("betas", "alphas", "alphas_cumprod", "alphas_cumprod_prev", "sqrt_alpha_cumprod", "sqrt_one_minus_alphas_cumprod",
                 "log_one_minus_alphas_cumprod", "sqrt_recip_alphas_cumprod", "sqrt_recipm1_alphas_cumprod"):
        buf = getattr(a, name)
        assert buf.dtype == torch.float32 and buf.device.type == "cpu" and buf.shape == (50,), name
    assert float(a.alphas_cumprod_prev[0]) == 1.0 and torch.equal(a.alphas_cumprod_prev[1:], a.alphas_cumprod[:-1])


def test_constructor_signature_equals_the_reference():
    from text2protein_amd.ddim import DiffusionSampler
    g = load_golden("ddim_tiny_a")
    names = [str(n) for n in g["signature_names"]]
    defaults = [str(d) for d in g["signature_defaults"]]
    sig = inspect.signature(DiffusionSampler.__init__)
    params = [p for p in sig.parameters.values() if p.name != "self"]
    positional = [p for p in params if p.kind == p.POSITIONAL_OR_KEYWORD]
    assert [p.name for p in positional] == names
    assert ["<required>" if p.default is p.empty else repr(p.default) for p in positional] == defaults
    extra = [p for p in params if p.kind != p.POSITIONAL_OR_KEYWORD]
    assert [(p.name, p.kind, p.default) for p in extra] == [("seed", inspect.Parameter.KEYWORD_ONLY, 0)]


def test_from_sde_takes_the_discrete_betas():
    from text2protein_amd import sde_lib
    from text2protein_amd.ddim import DiffusionSampler
    sde = sde_lib.VPSDE(0.1, 20, 40)
    ds = DiffusionSampler.from_sde(None, sde, sampling_steps=8, ddim_eta=0.5, w=2.0, seed=5)
    assert ds.timesteps == 40 and torch.equal(ds.betas, sde.discrete_betas) and torch.equal(ds.alphas_cumprod, sde.alphas_cumprod)
    assert (ds.sampling_steps, ds.ddim_eta, ds.w, ds.seed) == (8, 0.5, 2.0, 5)
    assert torch.equal(ds.betas, torch.from_numpy(load_golden("ddim_tiny_a")["betas"]))


def test_refusals_on_the_host():
    from text2protein_amd._lib import T2PError
    from text2protein_amd.ddim import DiffusionSampler
    for eta in (-0.01, 1.01, float("nan")):
        with pytest.raises(T2PError, match="ddim_eta"):
            DiffusionSampler(None, timesteps=10, ddim_eta=eta)
    for steps in (0, -3):
        with pytest.raises(T2PError, match="sampling_steps"):
            DiffusionSampler(None, timesteps=10, sampling_steps=steps)
    ds = DiffusionSampler(None, timesteps=10, sampling_steps=5)
    with pytest.raises(T2PError, match="cond is required"):
        ds.ddim_sample((1, 5, 16, 16), None)
    with pytest.raises(T2PError, match="cond is required"):
        ds.denoise_sample_from_pure_noise((1, 5, 16, 16))
    with pytest.raises(T2PError, match="clip_scheme"):
        ds.ddim_sample((1, 5, 16, 16), torch.zeros(1, 2, 32), clip_scheme="none")
    for call in (lambda: ds.p_loss(None, None, None), lambda: ds.forward(None), lambda: ds(None)):
        with pytest.raises(T2PError, match=r"losses"):
            call()
    with pytest.raises(T2PError, match="betas"):
        DiffusionSampler(None, timesteps=10, betas=torch.linspace(0.01, 0.2, 9))


def test_q_sample_and_predict_start_invert_each_other():
    from text2protein_amd.ddim import DiffusionSampler
    ds = DiffusionSampler(None, timesteps=40, betas=_betas("vpsde", 40))
    gen = torch.Generator().manual_seed(0)
    x0, eps = torch.rand(3, 2, 4, 4, generator=gen) * 2 - 1, torch.randn(3, 2, 4, 4, generator=gen)
    t = torch.tensor([0, 17, 39])
    xt = ds.q_sample(x0, t, eps)
    want = ds.sqrt_alpha_cumprod[t].view(3, 1, 1, 1) * x0 + ds.sqrt_one_minus_alphas_cumprod[t].view(3, 1, 1, 1) * eps
    assert torch.equal(xt, want)
    back = ds.predict_start_from_noise(xt, t, eps)
    assert float((back - x0).abs().max()) < 1e-4 * float(ds.sqrt_recip_alphas_cumprod[39])


def test_header_declares_and_lib_binds_the_ddim_symbols():
    from text2protein_amd import _lib
    hdr = open(os.path.join(ROOT, "include", "t2p.h")).read()
    code = re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)
    for sym, nargs, ret in (("t2p_ddim_create", 4, "int"), ("t2p_ddim_destroy", 1, "void"), ("t2p_ddim_set_seed", 2, "int"),
                            ("t2p_ddim_set_condition", 3, "int"), ("t2p_ddim_set_context", 5, "int"), ("t2p_ddim_reset", 3, "int"),
                            ("t2p_ddim_step", 5, "int"), ("t2p_ddim_run", 6, "int"), ("t2p_op_ddim_update", 22, "int")):
        m = re.search(r"\b" + ret + r"\s+" + sym + r"\s*\(([^)]*)\)\s*;", code)
        assert m, sym
        assert len(m.group(1).split(",")) == nargs, sym
        assert sym in _lib.SIGNATURES and len(_lib.SIGNATURES[sym][1]) == nargs, sym
        assert hasattr(_lib.load(), sym)
    for field in ("timesteps", "sampling_steps", "eta", "w", "clip", "batch", "seed"):
        assert re.search(r"\b" + field + r"\s*;", code.split("t2p_ddim_config {")[1].split("}")[0]), field
    assert [f for f, _ in _lib.DdimConfig._fields_] == ["timesteps", "sampling_steps", "eta", "w", "clip", "batch", "seed"]
    assert [f for f, _ in _lib.DdimStepRow._fields_] == ["t", "sqrt_recip", "sqrt_recipm1", "sqrt_an", "c", "sigma", "last"]
    assert "diffusion_sampler.py" in hdr and "w == 1" in hdr
    from text2protein_amd import build
    assert "ddim.hip" in build.SOURCES and "ddim.h" in build.HEADERS


def _run_cli(tmp_path, sde, *flags):
    from text2protein_amd.config import tiny_config
    cfg = tiny_config(**{"model.num_scales": 40, "training.sde": sde})
    cfg_path = tmp_path / f"tiny_{sde}.yml"
    with open(cfg_path, "w") as f:
        yaml.safe_dump(yaml.safe_load(__import__("json").dumps(cfg)), f)
    cmd = [sys.executable, os.path.join(ROOT, "sampling_6d.py"), str(cfg_path), "synthetic", "--outdir", str(tmp_path / "out"), *flags]
    return subprocess.run(cmd, capture_output=True, text=True, timeout=120, cwd=str(tmp_path))


def test_cli_refuses_ddim_on_a_ve_config_before_touching_a_device(tmp_path):
    r = _run_cli(tmp_path, "vesde", "--sampler", "ddim", "--ddim_steps", "4", "--ddim_eta", "0.5", "--guidance_w", "0.7")
    assert r.returncode != 0
    assert "--sampler ddim needs a noise-prediction network: training.sde must be vpsde" in r.stderr and "vesde" in r.stderr
    assert not (tmp_path / "out").exists() or not os.listdir(tmp_path / "out")


def test_cli_parses_the_new_flags(tmp_path):
    r = _run_cli(tmp_path, "vesde", "--sampler", "euler")
    assert r.returncode == 2 and "--sampler" in r.stderr and "'pc', 'ddim'" in r.stderr
    r = _run_cli(tmp_path, "vesde", "--sampler", "ddim", "--ddim_steps", "x")
    assert r.returncode == 2 and "--ddim_steps" in r.stderr
    r = _run_cli(tmp_path, "vesde", "--sampler", "ddim", "--guidance_w", "x")
    assert r.returncode == 2 and "--guidance_w" in r.stderr
    r = _run_cli(tmp_path, "vesde", "--sampler", "ddim", "--ddim_eta", "x")
    assert r.returncode == 2 and "--ddim_eta" in r.stderr
    src = open(os.path.join(ROOT, "sampling_6d.py")).read()
    assert 'default="pc"' in src
