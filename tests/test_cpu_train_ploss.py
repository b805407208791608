"""The DDIM sampler's training objective without a GPU: the torch restatement (tests/ploss_oracle.py) against the reference fixtures
(tests/golden/train_*_ploss_*.npz, written by make_golden_train_ploss.py from the reference's DiffusionSampler.p_loss) and against
autograd, the host-side refusals of DiffusionSampler.p_loss, the two new C symbols, and the integer timestep draw restated with
oracle/philox.py."""
import os
import re

import numpy as np
import pytest
import torch

import ploss_oracle as PO
from helpers import load_golden
from ploss_cases import L1_MIN_RESIDUAL, PLOSS_CASES, make_betas, ploss_inputs

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _mask(case, cfg, inp):
    if not case["masked"]:
        return None
    return PO.conditional_mask(tuple(inp["coords_6d"].shape), cfg.model.condition, inp["mask_pair"], inp.get("mask_inpaint"))


@pytest.mark.parametrize("name", list(PLOSS_CASES))
def test_oracle_loss_matches_the_fixture(name):
    """Given the fixture's pred_noise, the restated loss equals the reference's to 1e-6 relative, in float64 and in float32; the tables
    restated from the betas equal the reference's float32 tables up to float32 rounding (ploss_oracle.tables_close states the bound), and
    a / s are the tables' entries at t."""
    g = load_golden(name)
    case = PLOSS_CASES[name]
    cfg = case["config"]()
    inp = ploss_inputs(cfg, case)
    assert np.array_equal(g["t"], np.array(case["t"]))
    betas = make_betas(case, cfg)
    assert np.allclose(betas.numpy(), g["betas"], rtol=2.0 ** -21, atol=0)          # (a few float32 roundings; the host's vector width)
    a_tab, s_tab = PO.tables(betas)
    assert PO.tables_close(a_tab, s_tab, g["sqrt_alpha_cumprod"], g["sqrt_one_minus_alphas_cumprod"])
    # from the fixture's own betas the restatement is the reference's table up to the same roundings, and a / s are its entries at t
    a_fix, s_fix = PO.tables(torch.from_numpy(g["betas"]))
    assert PO.tables_close(a_fix, s_fix, g["sqrt_alpha_cumprod"], g["sqrt_one_minus_alphas_cumprod"])
    assert np.array_equal(g["sqrt_alpha_cumprod"][g["t"]], g["a"]) and np.array_equal(g["sqrt_one_minus_alphas_cumprod"][g["t"]], g["s"])
    a64, s64 = PO.tables(betas.double(), torch.float64)
    assert np.allclose(a64.numpy(), g["sqrt_alpha_cumprod"], rtol=1e-6, atol=0)
    # float32's 1 - alphas_cumprod cancels near t = 0: quantised to 6e-8 absolute, i.e. 6e-8 / (1 - acp) relative, halved by the root
    var = (s64 * s64).numpy()
    assert (np.abs(s64.numpy() - g["sqrt_one_minus_alphas_cumprod"]) <= (1e-6 + 1.2e-7 / var) * s64.numpy()).all()
    pred = torch.from_numpy(g["score"])
    mask = _mask(case, cfg, inp)
    for dt in (torch.float64, torch.float32):
        got = float(PO.loss(pred.to(dt), inp["z"].to(dt), case["loss_type"], mask))
        tol = 1e-6
        assert abs(got - float(g["loss"])) <= tol * abs(float(g["loss"])), (dt, got, float(g["loss"]))
    if case["loss_type"] == "l1":
        counted = torch.ones_like(pred).bool() if mask is None else mask
        assert float((pred - inp["z"]).abs()[counted].min()) > L1_MIN_RESIDUAL


@pytest.mark.parametrize("loss_type", ["l1", "l2"])
@pytest.mark.parametrize("masked", [False, True])
def test_oracle_gradient_matches_autograd(loss_type, masked):
    case = PLOSS_CASES["train_tinyB_ploss_l2m"]
    cfg = case["config"]()
    inp = ploss_inputs(cfg, case)
    mask = PO.conditional_mask(tuple(inp["coords_6d"].shape), cfg.model.condition, inp["mask_pair"], inp["mask_inpaint"]) if masked else None
    g = torch.Generator().manual_seed(5)
    pred = torch.randn(inp["z"].shape, generator=g, dtype=torch.float64).requires_grad_(True)
    z = inp["z"].double()
    PO.loss(pred, z, loss_type, mask).backward()
    want = PO.d_pred(pred.detach(), z, loss_type, mask)
    assert torch.allclose(pred.grad, want, rtol=1e-12, atol=1e-18)
    assert mask is None or float(pred.grad[~mask].abs().max()) == 0.0


def test_q_sample_freezes_what_the_mask_leaves_out():
    case = PLOSS_CASES["train_tinyB_ploss_l2m"]
    cfg = case["config"]()
    inp = ploss_inputs(cfg, case)
    mask = PO.conditional_mask(tuple(inp["coords_6d"].shape), cfg.model.condition, inp["mask_pair"], inp["mask_inpaint"])
    a, s = PO.tables(make_betas(case, cfg))
    x = inp["coords_6d"]
    xn = PO.q_sample(x, inp["t"], inp["z"], a, s, mask)
    assert torch.equal(xn[~mask], x[~mask]) and not torch.equal(xn[mask], x[mask])
    from text2protein_amd.ddim import DiffusionSampler
    ds = DiffusionSampler(None, timesteps=50, betas=make_betas(case, cfg))
    assert torch.equal(PO.q_sample(x, inp["t"], inp["z"], a, s), ds.q_sample(x, inp["t"], inp["z"]))


def _host_only_trainer(cfg):
    """A HipTrainModel shell with a config and no native object: enough for the checks p_loss makes before any native call."""
    from text2protein_amd import losses
    m = object.__new__(losses.HipTrainModel)
    m.config = cfg
    return m


def test_host_refusals():
    from text2protein_amd._lib import T2PError
    from text2protein_amd.ddim import DiffusionSampler
    from text2protein_amd import losses
    case = PLOSS_CASES["train_tiny_ploss_l2"]
    cfg = case["config"]()
    inp = ploss_inputs(cfg, case)
    x, ctx = inp["coords_6d"], inp["context"]
    ds = DiffusionSampler(_host_only_trainer(cfg), timesteps=40)
    for t, what in ((torch.tensor([0, 40]), r"outside \[0, 40\)"), (torch.tensor([-1, 3]), r"outside \[0, 40\)"),
                    (torch.tensor([0.0, 3.0]), "integer tensor"), ([0, 3], "integer tensor"), (torch.tensor([1, 2, 3]), "shape")):
        with pytest.raises(T2PError, match=what):
            ds.p_loss(x, ctx, t)
    with pytest.raises(T2PError, match="x_start"):
        ds.p_loss(x[:, :-1], ctx, inp["t"])
    with pytest.raises(T2PError, match="cond is required"):
        ds.p_loss(x, None, inp["t"])
    with pytest.raises(T2PError, match="cond is required"):
        ds(x)
    with pytest.raises(T2PError, match="mask_pair"):
        ds.p_loss(x, ctx, inp["t"], batch={})
    bad = DiffusionSampler(_host_only_trainer(cfg), timesteps=40, loss_type="huber")
    with pytest.raises(NotImplementedError, match='Loss type "huber" not implemented'):
        bad.p_loss(x, ctx, inp["t"])
    with pytest.raises(NotImplementedError, match='Loss type "huber" not implemented'):
        losses.get_ploss_step_fn(bad, train=True)
    with pytest.raises(T2PError, match=r"outside \[0, 40\)"):
        losses.get_ploss_step_fn(ds, train=True)({}, dict(coords_6d=x, context=ctx), t=torch.tensor([0, 40]))
    # a model that is not a trainer: the refusal of before, pointing at losses
    for model in (None, lambda x, t, c: x):
        other = DiffusionSampler(model, timesteps=40)
        for call in (lambda: other.p_loss(x, ctx, inp["t"]), lambda: other.forward(x, ctx), lambda: other(x, ctx)):
            with pytest.raises(T2PError, match=r"losses.*get_train_model.*get_ploss_step_fn"):
                call()


def test_symbols_in_header_and_signature_table():
    from text2protein_amd import _lib
    with open(os.path.join(ROOT, "include", "t2p.h")) as f:
        header = f.read()
    for name, nargs in (("t2p_train_set_ploss", 5), ("t2p_op_ploss_draw_t", 6)):
        m = re.search(r"\bint\s+" + name + r"\s*\(([^;]*?)\)\s*;", header, re.S)
        assert m, name
        assert len(m.group(1).split(",")) == nargs
        assert name in _lib.SIGNATURES and len(_lib.SIGNATURES[name][1]) == nargs


def test_integer_draw_restated():
    """((w >> 8) T) >> 24: T = 1 gives zeros only; T = 7 over 4096 samples hits every value and nothing outside; T = 2^24 stays inside."""
    assert not PO.draw_t(11, 5, 4096, 1).any()
    t7 = PO.draw_t(11, 4096 * 3 + 5, 4096, 7)
    assert set(t7.tolist()) == set(range(7))
    counts = np.bincount(t7, minlength=7)
    assert counts.min() > 4096 / 7 * 0.8 and counts.max() < 4096 / 7 * 1.2      # (binomial sd is 22 of 585)
    big = PO.draw_t(11, 5, 4096, 1 << 24)
    assert big.min() >= 0 and big.max() < (1 << 24)
    assert not np.array_equal(PO.draw_t(11, 5, 64, 1000), PO.draw_t(11, 4096 + 5, 64, 1000))
    # the uniform the other training draws form from the same word is this draw's source: t = floor(u T)
    from oracle import philox
    u = philox.train_uniforms(11, 5, np.arange(4096))[:, 0].astype(np.float64)
    assert np.array_equal(PO.draw_t(11, 5, 4096, 1000), np.floor(u * 1000).astype(np.int64))
