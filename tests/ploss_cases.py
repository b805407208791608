"""Training-step fixtures under the DDIM sampler's own objective, ``DiffusionSampler.p_loss`` (tests/golden/make_golden_train_ploss.py
writes them; tests/test_gpu_train_ploss.py and tests/test_cpu_train_ploss.py read them).  Same inputs and form as helpers.TRAIN_CASES;
on top: ``loss_type``, ``masked`` (the masked form of the loss, an extension; False = the reference's loss as written), ``betas`` and the
integer timestep ``t`` of every sample (the float ``t`` of ``helpers.train_inputs`` is not used).

The seeds of the l1 cases are chosen so that min |pred_noise - noise| over the counted elements is above 1e-4 (the generator asserts it):
the l1 gradient is sign(pred - noise), and no sign may hang on rounding."""
import torch

from helpers import cfg_train_tiny, cfg_train_tinyB, train_inputs

L1_MIN_RESIDUAL = 1e-4

PLOSS_CASES = {
    # betas = linspace(0.01, 0.2, 40): DiffusionSampler's default schedule, not any VPSDE's; both ends of the table
    "train_tiny_ploss_l2": dict(config=cfg_train_tiny, seed=3, B=2, T=3, lengths=[12, 9], step0=2000, mask_info=None, loss_type="l2",
                                masked=False, betas="linear40", t=[0, 39]),
    "train_tiny_ploss_l1": dict(config=cfg_train_tiny, seed=3, B=2, T=3, lengths=[12, 9], step0=2000, mask_info=None, loss_type="l1",
                                masked=False, betas="linear40", t=[0, 39]),
    # all three conditions, Dropout_0 at 0.1, the schedule of a VPSDE with N = 50
    "train_tinyB_ploss_l2m": dict(config=cfg_train_tinyB, seed=4, B=3, T=5, lengths=[16, 11, 6], step0=7000, mask_info="1:3,6:8",
                                  loss_type="l2", masked=True, betas="vpsde50", t=[49, 0, 17]),
    "train_tinyB_ploss_l1m": dict(config=cfg_train_tinyB, seed=4, B=3, T=5, lengths=[16, 11, 6], step0=7000, mask_info="1:3,6:8",
                                  loss_type="l1", masked=True, betas="vpsde50", t=[49, 0, 17]),
}


def make_betas(case, cfg):
    """The float32 betas of a case: DiffusionSampler's default ``linspace(0.01, 0.2, 40)``, or a VPSDE's ``discrete_betas`` with N = 50."""
    if case["betas"] == "linear40":
        return torch.linspace(0.01, 0.2, 40)
    assert case["betas"] == "vpsde50"
    from text2protein_amd import sde_lib
    return sde_lib.VPSDE(beta_min=cfg.model.beta_min, beta_max=cfg.model.beta_max, N=50).discrete_betas.float()


def ploss_inputs(cfg, case):
    """``helpers.train_inputs`` with the float t replaced by the case's integer timesteps (torch.long)."""
    inp = train_inputs(cfg, case)
    inp["t"] = torch.tensor(case["t"], dtype=torch.long)
    return inp


def ploss_batch(inp, case):
    """The batch a pass takes: without the masks for an unmasked case (that selects the reference's loss)."""
    keys = ("coords_6d", "context") + (("mask_pair", "mask_inpaint") if case["masked"] else ())
    return {k: inp[k] for k in keys if k in inp}
