"""Host side of the VP / sub-VP training step: sde_lib's marginal_prob and the discrete std table against the values the reference
used when the fixtures were made (tests/golden/make_golden_train_sde.py), and the SDE surface of text2protein_amd.losses that needs
no GPU."""
import numpy as np
import pytest
import torch

from helpers import load_golden
from sde_train_cases import SDE_TRAIN_CASES, make_sde


@pytest.mark.parametrize("name", list(SDE_TRAIN_CASES))
def test_marginal_prob_and_std_table_match_the_reference(name):
    from text2protein_amd import sde_lib
    g = load_golden(name)
    case = SDE_TRAIN_CASES[name]
    cfg = case["config"]()
    sde = make_sde(sde_lib, cfg, case)
    t = torch.from_numpy(g["t"])
    B = t.shape[0]
    x = torch.from_numpy(np.linspace(-1.0, 1.0, B * 2 * 3 * 3, dtype=np.float32).reshape(B, 2, 3, 3))
    mean, std = sde.marginal_prob(x, t)
    assert mean.shape == x.shape and std.shape == (B,)
    coef = sde.marginal_prob(torch.ones(B, 1, 1, 1), t)[0].reshape(-1)
    assert np.allclose(coef.numpy(), g["mean_coef"], rtol=1e-6, atol=0)
    assert np.allclose(std.numpy(), g["std"], rtol=1e-6, atol=0)
    assert np.allclose(mean.numpy(), g["mean_coef"][:, None, None, None] * x.numpy(), rtol=2e-6, atol=0)
    assert np.allclose(sde.marginal_prob_std(t).numpy(), std.numpy(), rtol=0, atol=0)
    if case["sde"] == "vp":
        table = sde.sqrt_1m_alphas_cumprod
        assert table.dtype == torch.float32 and np.array_equal(table.numpy(), g["sqrt_1m_alphas_cumprod"])
        label = t * (sde.N - 1)
        assert np.array_equal(label.numpy(), g["labels"])
        assert np.array_equal(table[label.long()].numpy(), g["score_std"])
        assert sde.vp_tables(1e-3)[1].shape == (sde.N,)          # the sampler's score scale comes from the same table
    else:
        assert np.array_equal((t * 999).numpy(), g["labels"]) and np.array_equal(g["score_std"], g["std"])


def test_ve_marginal_prob():
    from text2protein_amd import sde_lib
    sde = sde_lib.VESDE(sigma_min=0.01, sigma_max=100.0, N=50)
    t = torch.tensor([0.0, 0.5, 1.0])
    x = torch.ones(3, 1, 2, 2)
    mean, std = sde.marginal_prob(x, t)
    assert torch.equal(mean, x) and np.allclose(std.numpy(), [0.01, 1.0, 100.0], rtol=1e-6)


def test_loss_functions_refuse_an_unknown_sde():
    from text2protein_amd import _lib, losses

    class Other:
        N = 10

    for make in (lambda: losses.get_sde_loss_fn(Other(), train=True), lambda: losses.get_sde_loss_fn(Other(), train=False),
                 lambda: losses.get_step_fn(Other(), train=True)):
        with pytest.raises(NotImplementedError, match="Other"):
            make()
    assert (_lib.SDE_VE, _lib.SDE_VP, _lib.SDE_SUBVP) == (0, 1, 2)
    assert "t2p_train_set_sde" in _lib.SIGNATURES
