"""Replacement inpainting on the fused predictor-corrector loop: mirror of ``score_sde_pytorch/inpainting.py``.

  get_pc_inpainter(sde, predictor, corrector, snr, n_steps=1, probability_flow=False, continuous=False, denoise=True, eps=1e-5)
      -> pc_inpainter(model, data, mask)                                                     inpainting.py:6-78

After every corrector and predictor update the known region (``mask == 1``, the reference's convention) is overwritten with the
data noised to the current level, ``mean(data, t) + std(t) z`` (Song et al.): the unknown region is denoised next to a known
region of matching noise.  Unlike the ``inpainting`` *condition* (sampling.apply_conditions), which freezes clean entries and
needs a network trained to see them, this works with every checkpoint.

The reference's function cannot run as shipped (it passes ``continuous=`` to update functions that do not take it, and no
context); its body is well defined and is what runs here, inside the update kernels of the fused loop (csrc/update_loop.h):

    x, x_mean = update(x, t_i)                      the whole corrector (all n_steps inner steps), then the predictor
    r      = mean_coef_i data + z std_i             z: a fresh N(0, 1) draw per update
    x      = mask ? r : x
    x_mean = mask ? mean_coef_i data : x            off the known region this is the NEW x (inpainting.py:46), reproduced

starting from ``mask ? data : prior`` and returning the last predictor's ``x_mean`` (``denoise``) or ``x``.

Beyond the reference: ``context`` (the network needs one), ``condition`` (an existing condition still applies; per element:
frozen by the condition -> x_initial, else known -> replaced, else the update), ``guidance_w``, ``seed``, and the rank sharding of
``get_pc_sampler`` (``global_batch`` / ``all_reduce``).
"""
from __future__ import annotations

import math

import torch

from . import sde_lib
from ._lib import T2PError
from .sampling import LangevinCorrector, PCStepper, ReverseDiffusionPredictor, apply_conditions, call_seed


def known_from_mask_info(config, batch, mask_info, condition=None):
    """``(data, known)`` of a replacement run from a batch of 6D maps and ``--mask_info``: ``known`` (B, C, L, L) bool is the
    complement of ``mask_inpaint`` (the residues ``mask_info`` selects are the ones to design), inside the length mask of the
    batch's residue counts, on every channel ``condition`` leaves free."""
    from .conditions import batch_lengths, pair_mask, parse_mask_info
    data = batch["coords_6d"].float()
    B, C, L, _ = data.shape
    redo = pair_mask(parse_mask_info(mask_info, B, L)).to(data.device)
    lengths = torch.as_tensor(batch_lengths(batch), device=data.device)
    inside = torch.arange(L, device=data.device)[None, :] < lengths[:, None]
    known = (~redo & inside[:, :, None] & inside[:, None, :])[:, None].expand(B, C, L, L)
    _, free = apply_conditions(torch.zeros_like(data), condition)
    return data, known & free.to(data.device)


def get_pc_inpainter(sde, predictor, corrector, snr, n_steps=1, probability_flow=False, continuous=False, denoise=True, eps=1e-5,
                     *, seed=0, guidance_w=None, global_batch=None, all_reduce=None):
    """Create an inpainting function that uses the PC sampler (inpainting.py:6-78), on the fused ``PCStepper``.

    Refused with ``T2PError``: ``continuous=True`` (the fused loop runs the discrete schedules), the sub-VP SDE, any predictor /
    corrector other than ``ReverseDiffusionPredictor`` / ``LangevinCorrector`` (the DDIM sampler among them: it has no
    corrector to replace after), a non-finite guidance weight.

    The returned ``pc_inpainter(model, data, mask, context=None, condition=None, call_index=None, train_dtype="f16")`` takes a
    ``HipScoreModel`` or a ``HipTrainModel`` (its current parameters, as ``get_pc_sampler`` does), ``data`` (B, C, L, L) and
    ``mask`` of the same shape, 1 = known; returns ``(sample, number of function evaluations)``.  The prior and both replacement
    draws come from the device generator (csrc/philox.h); call k of one inpainter uses ``call_seed(seed, k)``."""
    from .ddim import DiffusionSampler
    if continuous:
        raise T2PError("replacement inpainting runs the discrete schedules of the fused loop: continuous=True is not supported")
    if any(isinstance(o, DiffusionSampler) or o is DiffusionSampler for o in (sde, predictor, corrector)):
        raise T2PError("replacement inpainting belongs to the predictor-corrector loop: the DDIM sampler has no corrector / "
                       "predictor pair to replace after")
    if isinstance(sde, sde_lib.subVPSDE):
        raise T2PError("replacement inpainting covers the VE and VP SDEs (sub-VP cannot be sampled, sde_lib.subVPSDE)")
    if not isinstance(sde, (sde_lib.VESDE, sde_lib.VPSDE)):
        raise T2PError(f"replacement inpainting covers the VE and VP SDEs, not {type(sde).__name__}")
    if predictor is not ReverseDiffusionPredictor or corrector is not LangevinCorrector:
        raise T2PError("replacement inpainting runs on the fused loop: ReverseDiffusionPredictor with LangevinCorrector")
    if guidance_w is not None and not math.isfinite(float(guidance_w)):
        raise T2PError("the guidance weight must be finite")
    state = {"sampler": None, "model": None, "batch": None, "calls": 0}
    mean_coef, std = sde.inpaint_tables(eps)

    def pc_inpainter(model, data, mask, context=None, condition=None, call_index=None, train_dtype="f16"):
        """PC sampler for inpainting (inpainting.py:54-76) -> (inpainted samples, number of function evaluations)."""
        if context is None:
            raise T2PError("pc_inpainter needs the text context the score network was trained with (context=)")
        if data.dim() != 4:
            raise T2PError(f"data must be (B, C, L, L), got {tuple(data.shape)}")
        if tuple(mask.shape) != tuple(data.shape):
            raise T2PError(f"mask {tuple(mask.shape)} must have the shape of data {tuple(data.shape)} (1 = known)")
        if context.shape[0] != data.shape[0]:
            raise T2PError(f"context batch {context.shape[0]} != data batch {data.shape[0]}")
        if hasattr(model, "sampling_model"):
            model = model.sampling_model(train_dtype)
        cfg = model.config
        want = (cfg.data.num_channels, cfg.data.max_res_num, cfg.data.max_res_num)
        if tuple(data.shape[1:]) != want:
            raise T2PError(f"data {tuple(data.shape)} does not match the model's (B, {want[0]}, {want[1]}, {want[2]})")
        device = model.device
        torch.cuda.set_device(device)
        B = data.shape[0]
        if call_index is None:
            call_index = state["calls"]
            state["calls"] += 1
        run_seed = call_seed(seed, call_index)
        with torch.no_grad():
            if state["sampler"] is None or state["model"] is not model or state["batch"] != B:
                state["sampler"] = PCStepper(model, sde, B, snr, n_steps, probability_flow, denoise, eps, seed,
                                             global_batch=global_batch, all_reduce=all_reduce, guidance_w=guidance_w)
                state["model"], state["batch"] = model, B
            stepper = state["sampler"]
            data = data.to(device, torch.float32).contiguous()
            known = (mask.to(device) != 0).to(torch.uint8).contiguous()
            context = context.to(device, torch.float32).contiguous()
            if stepper.guided or guidance_w is not None:
                stepper.set_context(context)
            else:
                model.set_context(context)
            # the frozen entries of a condition do not depend on the prior (zeros / the length channel / given maps)
            x_initial, free = apply_conditions(torch.zeros_like(data), condition)
            conditioned = bool(condition)
            stepper.set_condition(free.to(torch.uint8).contiguous() if conditioned else None,
                                  x_initial.float().contiguous() if conditioned else None)
            stepper.set_inpaint(known, data, mean_coef, std)
            stepper.set_seed(run_seed)
            x = torch.empty((2 if stepper.guided else 1) * B, *data.shape[1:], device=device, dtype=torch.float32)
            out = torch.empty_like(data)
            try:
                stepper.run(x, out, prior_given=False)
            finally:
                stepper.set_inpaint()
                stepper.set_condition()
            return out, sde.N * (n_steps + 1)

    return pc_inpainter
