"""Training-step fixtures under the VP and sub-VP SDEs (tests/golden/make_golden_train_sde.py writes them; tests/test_gpu_train_sde.py and
tests/test_cpu_train_sde.py read them).  Same inputs and form as helpers.TRAIN_CASES; ``sde`` names the SDE of the loss.  The seeds are
chosen so that every drawn t is >= 0.02 (the generator asserts it): below that the reference's fp32 ``1 - exp(2 lmc)`` is quantised to
more than 1e-4 relative and the comparison would measure that cancellation, not the product."""
from helpers import cfg_train_cond_length, cfg_train_tiny, cfg_train_tinyB


def cfg_train_tiny_subvp():
    """num_scales = 1000: the reference's sub-VP label is t * 999 whatever N is (models/utils.py:147) and indexes the sigma table."""
    cfg = cfg_train_tiny()
    cfg.model.num_scales = 1000
    return cfg


SDE_TRAIN_CASES = {
    "train_tiny_vp": dict(config=cfg_train_tiny, sde="vp", seed=7, B=2, T=3, lengths=[12, 9], step0=2000, mask_info=None),
    "train_tinyB_vp": dict(config=cfg_train_tinyB, sde="vp", seed=4, B=3, T=5, lengths=[16, 11, 6], step0=7000, mask_info="1:3,6:8"),
    "train_tiny_subvp": dict(config=cfg_train_tiny_subvp, sde="subvp", seed=6, B=2, T=3, lengths=[12, 9], step0=2000, mask_info=None),
    # full size: norms + projections of all 622 tensors, whole tensors for the small ones only
    "train_cond_length_vp": dict(config=cfg_train_cond_length, sde="vp", seed=5, B=1, T=16, lengths=[100], step0=9000, mask_info=None,
                                 full_size=True),
}


def make_sde(sde_lib, cfg, case):
    """The SDE object of a case from ``sde_lib`` (the product's module or the reference's: same constructors)."""
    m = cfg.model
    if case["sde"] == "vp":
        return sde_lib.VPSDE(beta_min=m.beta_min, beta_max=m.beta_max, N=m.num_scales)
    if case["sde"] == "subvp":
        return sde_lib.subVPSDE(beta_min=m.beta_min, beta_max=m.beta_max, N=m.num_scales)
    return sde_lib.VESDE(sigma_min=m.sigma_min, sigma_max=m.sigma_max, N=m.num_scales)
