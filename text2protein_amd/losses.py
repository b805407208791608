"""Training step on MI355X: Python mirror of the reference's ``score_sde_pytorch/losses.py`` over the C ABI
(``t2p_train_*``, include/t2p.h).  SURVEY.md 8(f)4, under the VE, VP or sub-VP SDE: exact-f32 products, or (``dtype="f16"`` / ``"bf16"``) 16-bit
products with fp32 accumulation and fp32 parameters, gradients, optimizer state, EMA and loss.

The reference keeps four objects in ``state`` -- ``model`` (DataParallel(UNetModel)), ``optimizer`` (torch Adam),
``ema`` (ExponentialMovingAverage) and ``step`` (train.py:118-124) -- and ``step_fn`` (losses.py:165-176) drives them:
zero_grad, loss_fn, backward, optimize_fn (warm-up, clip, Adam), ``step += 1``, ``ema.update``.  Here the parameters, their
gradients, both Adam moments and the EMA shadow live in ONE native object (flat device buffers in ``parameters()`` order) and
one call runs the whole step on the GPU; the classes below are views of that object with the reference's names and call
signatures, so a training script reads the same:

    model = get_train_model(config)                  # utils.get_model(config)
    optimizer = get_optimizer(config, model.parameters())
    ema = ExponentialMovingAverage(model.parameters(), decay=config.model.ema_rate)
    state = dict(optimizer=optimizer, model=model, ema=ema, step=0)
    step_fn = get_step_fn(sde, train=True, optimize_fn=optimization_manager(config))
    loss = step_fn(state, batch, condition=config.model.condition)

The DDIM sampler's own objective (``DiffusionSampler.p_loss``, sampler/diffusion_sampler.py:144-167) is a second objective of the same
step: ``get_ploss_step_fn(diffusion, train, ...)`` in place of ``get_step_fn(sde, train, ...)``, or ``diffusion.p_loss`` /
``diffusion(x, cond)`` on a ``DiffusionSampler`` built on the model (``HipTrainModel.set_ploss``).

There is no CPU fallback: without a HIP device ``HipTrainModel`` raises.
"""
from __future__ import annotations

import ctypes as C
import random
from collections import OrderedDict

import numpy as np
import torch

from . import _lib
from ._lib import T2PError, TrainBatch, TrainConfig, check, ptr, stream_ptr
from .arch import param_specs
from .model import _model_config
from .sde_lib import VESDE, VPSDE, subVPSDE

_COND_FLAGS = {"length": 1, "ss": 2, "inpainting": 4}
PARAM, GRAD, EMA, EXP_AVG, EXP_AVG_SQ = 0, 1, 2, 3, 4
STASH = 5          # t2p_train_copy only: where ema.store keeps the parameters


def condition_flags(condition) -> int:
    flags = 0
    for c in (condition or []):
        if c not in _COND_FLAGS:
            raise ValueError(f"unknown condition {c!r}")       # the reference ignores unknown names silently (losses.py:115-123)
        flags |= _COND_FLAGS[c]
    return flags


def parse_ss_indices(ss_indices, batch_size=None):
    """``batch["ss_indices"]`` (one string per sample, ``"a:b,c:d"``; ``''`` = no secondary-structure annotation, losses.py:56) as the
    block list of ``t2p_train_set_ss_blocks``: ``[(sample, start, end), ...]``, samples in order, blocks in string order -- the order in
    which the reference draws its ``random.random()`` per block (losses.py:55-58).  Raises ``T2PError`` on a list of the wrong length,
    on a range that is not two integers and on a negative index (Python would wrap it; the dataset never writes one, so it is refused
    rather than guessed at)."""
    if isinstance(ss_indices, str) or not hasattr(ss_indices, "__len__"):
        raise T2PError("ss_indices must be a sequence of strings, one per sample")
    if batch_size is not None and len(ss_indices) != int(batch_size):
        raise T2PError(f"ss_indices holds {len(ss_indices)} entries, the batch has {int(batch_size)} samples")
    blocks = []
    for b, text in enumerate(ss_indices):
        if not isinstance(text, str):
            raise T2PError(f"ss_indices[{b}] is not a string: {text!r}")
        if text == "":
            continue
        for rng in text.split(","):
            parts = rng.split(":")
            try:
                if len(parts) != 2:
                    raise ValueError(rng)
                start, end = int(parts[0]), int(parts[1])
            except ValueError:
                raise T2PError(f"ss_indices[{b}]: {rng!r} is not a range 'start:end' of two integers") from None
            if start < 0 or end < 0:
                raise T2PError(f"ss_indices[{b}]: negative index in {rng!r}")
            blocks.append((b, start, end))
    return blocks


def draw_block_decisions(blocks, block_dropout=0.2):
    """One ``random.random() < block_dropout`` per block in list order (losses.py:58): after the same ``random.seed`` the same blocks are
    dropped as in the reference."""
    return [1 if random.random() < block_dropout else 0 for _ in blocks]


def _set_batch_ss_blocks(model, batch, condition, block_dropout, draw):
    """losses.py:106-107: under the ``ss`` condition the blocks of ``batch["ss_indices"]`` go to the next pass.  A batch WITHOUT the key
    runs as before this existed -- nothing is set, nothing is dropped -- where the reference would raise ``KeyError``."""
    if "ss" not in (condition or []) or "ss_indices" not in batch:
        return
    blocks = parse_ss_indices(batch["ss_indices"], batch["coords_6d"].shape[0])
    model.set_ss_blocks(blocks, drop=draw_block_decisions(blocks, block_dropout) if draw == "host" else None, p=block_dropout)


def _check_draw(draw):
    if draw not in ("host", "device"):
        raise ValueError(f"block_dropout_draw must be 'host' or 'device', not {draw!r}")


def _check_inpaint_draw(draw):
    if draw not in (None, "host", "device"):
        raise ValueError(f"inpaint_mask_draw must be None, 'host' or 'device', not {draw!r}")


def _check_context_dropout(p, draw):
    try:
        ok = 0.0 <= float(p) <= 1.0            # (a NaN fails the comparison)
    except (TypeError, ValueError):
        ok = False
    if not ok:
        raise ValueError(f"context_dropout must be a probability in [0, 1], not {p!r}")
    if draw not in ("host", "device"):
        raise ValueError(f"context_dropout_draw must be 'host' or 'device', not {draw!r}")


def draw_context_decisions(n, context_dropout):
    """One ``random.random() < context_dropout`` per sample in sample order."""
    return [1 if random.random() < context_dropout else 0 for _ in range(int(n))]


def _request_context_drop(model, batch, p, draw):
    """Training for classifier-free guidance: every sample of the batch loses its text context with probability ``p`` in the pass that
    follows.  ``p == 0``: no native call and no ``random`` draw.  Comes after the block-dropout and inpainting-mask draws, so one
    ``random.seed`` reproduces a step; a failure here clears those two requests, as no pass follows."""
    if p <= 0.0:
        return
    try:
        n = batch["coords_6d"].shape[0]
        model.set_context_drop(n, drop=draw_context_decisions(n, p) if draw == "host" else None, p=p)
    except Exception:
        model.set_ss_blocks([])
        model.set_inpaint_draw(None, None)
        raise


def _draw_batch_inpaint_mask(model, batch, condition, draw):
    """train.py:176 / :193: under the ``inpainting`` condition a batch WITHOUT ``mask_inpaint`` gets the reference's random mask --
    ``"host"``: ``conditions.random_mask_batch`` on a copy of the batch (the reference's draws in its order); ``"device"``: the request of
    ``set_inpaint_draw``, consumed by the pass that follows.  ``None``, another condition or a supplied mask: the batch as it is."""
    if draw is None or "inpainting" not in (condition or []) or batch.get("mask_inpaint") is not None:
        return batch
    from . import conditions
    try:
        if draw == "host":
            return conditions.random_mask_batch(dict(batch), model.config)
        model.set_inpaint_draw(conditions.batch_lengths(batch), model.config.model.get("inpainting"))
    except Exception:
        model.set_ss_blocks([])                # no pass follows: a block list set for this batch must not reach the next one
        raise
    return batch


class HipTrainModel:
    """The score network in training form: ``UNetModel`` + its optimizer state + its EMA, resident on one GPU.

    ``dtype`` ("f32" | "f16" | "bf16", the names of ``HipScoreModel``) is the compute dtype of the products.  Whatever it is, the
    parameters, gradients, Adam moments, EMA and checkpoints are fp32 and laid out identically.  In the 16-bit modes a step whose
    loss or gradient norm is not finite raises ``T2PError`` and changes nothing (mixed-precision training's skipped step)."""

    def __init__(self, config, device="cuda:0", seed=0, dtype="f32"):
        if not isinstance(dtype, str) or dtype not in _lib.DTYPE_NAMES:
            raise ValueError(f"unknown compute dtype {dtype!r}: one of {sorted(_lib.DTYPE_NAMES)}")
        self.config = config
        self.dtype = dtype
        self.device = torch.device(device)
        if self.device.type != "cuda":
            raise T2PError("HipTrainModel needs a GPU device (there is no CPU fallback)")
        self.lib = _lib.load()
        torch.cuda.set_device(self.device)
        self._mc = _model_config(config, dtype)
        o, m = config.optim, config.model
        if o.optimizer != "Adam":
            raise NotImplementedError(f"Optimizer {o.optimizer} not supported yet!")          # losses.py:32-34
        tc = TrainConfig()
        tc.lr, tc.beta1, tc.eps, tc.weight_decay = float(o.lr), float(o.beta1), float(o.eps), float(o.weight_decay)
        tc.warmup, tc.grad_clip = float(o.warmup), float(o.grad_clip)
        tc.ema_rate, tc.dropout, tc.t_eps = float(m.ema_rate), float(m.dropout), 1e-5
        tc.cond_flags = condition_flags(m.condition)
        tc.seed = int(seed)
        self._tc = tc
        h = C.c_void_p()
        check(self.lib.t2p_train_create(C.byref(self._mc), C.byref(tc), C.byref(h)))
        self._h = h
        self._specs = param_specs(config)
        if self.lib.t2p_train_num_params(self._h) != len(self._specs):
            raise T2PError("parameter table mismatch between the trainer and arch.param_specs")
        self._loaded = False
        self.training = True
        self._keep = []
        self._sde = None          # (kind, parameters) once set_sde ran; the native default is VE with the model's sigmas
        self._samplers = {}       # compute dtype -> HipScoreModel fed from this trainer's buffers (sampling_model)

    # -- nn.Module-like surface ----------------------------------------------------------------------------------------
    def train(self, mode=True):
        self.training = bool(mode)
        return self

    def eval(self):
        return self.train(False)

    def to(self, *_a, **_k):
        return self

    def parameters(self):
        """Handle the optimizer / EMA views are built from (the tensors themselves stay on the device)."""
        return _ParamHandle(self)

    def sampling_model(self, dtype="f16"):
        """A ``HipScoreModel`` of compute dtype ``dtype`` on this trainer's GPU holding the trainer's CURRENT parameters (after
        ``ema.copy_to(model.parameters())`` those are the EMA): created at the first call for each dtype, refreshed on the device
        by every call (``HipScoreModel.load_from``).  What the samplers evaluate when they are handed this model: the trainer's own
        forward pass keeps every activation for the backward pass and is an order of magnitude slower per evaluation."""
        from .model import HipScoreModel
        m = self._samplers.get(dtype)
        if m is None:
            m = self._samplers[dtype] = HipScoreModel(self.config, dtype=dtype, device=self.device)
        return m.load_from(self, "param")

    def copy_buffer(self, dst, src):
        """Device-to-device copy between the flat buffers (``t2p_train_copy``): 5 <- 0 store, 0 <- 2 copy_to, 0 <- 5 restore."""
        torch.cuda.set_device(self.device)
        check(self.lib.t2p_train_copy(self._h, int(dst), int(src), stream_ptr()))

    def param_table(self):
        out = []
        name, shape, nd = C.c_char_p(), (C.c_int64 * 4)(), C.c_int()
        for i in range(self.lib.t2p_train_num_params(self._h)):
            check(self.lib.t2p_train_param_info(self._h, i, C.byref(name), shape, C.byref(nd)))
            out.append((name.value.decode(), tuple(shape[k] for k in range(nd.value))))
        return out

    def load_state_dict(self, state_dict, strict=True):
        seen = set()
        for k, v in state_dict.items():
            name = k[7:] if k.startswith("module.") else k
            if name == "sigmas":
                continue
            t = torch.as_tensor(v).detach().to("cpu", torch.float32).contiguous()
            shape = (C.c_int64 * max(t.dim(), 1))(*t.shape)
            check(self.lib.t2p_train_load_param(self._h, name.encode(), C.c_void_p(t.data_ptr()), shape, t.dim()))
            seen.add(name)
        missing = [s.name for s in self._specs if s.name not in seen]
        if missing and strict:
            raise T2PError(f"missing parameters: {missing[:5]}{'...' if len(missing) > 5 else ''}")
        self._loaded = not missing
        return missing

    def read(self, which, name=None):
        """One tensor (``name``) or all of them (OrderedDict in ``parameters()`` order) of buffer ``which``
        (PARAM / GRAD / EMA / EXP_AVG / EXP_AVG_SQ) as CPU float32 tensors."""
        specs = [s for s in self._specs if name is None or s.name == name]
        out = OrderedDict()
        for s in specs:
            t = torch.empty(tuple(s.shape), dtype=torch.float32)
            check(self.lib.t2p_train_read(self._h, which, s.name.encode(), C.c_void_p(t.data_ptr())))
            out[s.name] = t
        return out[name] if name is not None else out

    def write(self, which, tensors):
        for k, v in tensors.items():
            t = torch.as_tensor(v).detach().to("cpu", torch.float32).contiguous()
            check(self.lib.t2p_train_write(self._h, which, k.encode(), C.c_void_p(t.data_ptr())))

    def state_dict(self):
        return self.read(PARAM)

    def set_step(self, step, adam_updates=None, ema_updates=None):
        cur = self.get_step()
        check(self.lib.t2p_train_set_step(self._h, int(step), int(cur[1] if adam_updates is None else adam_updates),
                                          int(cur[2] if ema_updates is None else ema_updates)))

    def get_step(self):
        out = (C.c_int64 * 3)()
        check(self.lib.t2p_train_get_step(self._h, out))
        return tuple(int(v) for v in out)

    def set_sde(self, sde):
        """The SDE of the loss (``get_sde_loss_fn``'s ``sde``): an ``sde_lib.VESDE``, ``VPSDE`` or ``subVPSDE`` whose ``N`` is
        ``model.num_scales``.  ``get_sde_loss_fn`` / ``get_step_fn`` call this on first use; a model stays with the SDE it was given."""
        key = _sde_key(sde)
        if int(sde.N) != int(self.config.model.num_scales):
            raise T2PError(f"sde.N = {sde.N} differs from model.num_scales = {self.config.model.num_scales}")
        if self._sde is not None:
            if self._sde != key:
                raise T2PError(f"this model trains under {self._sde[0]}{self._sde[1:]}; it cannot switch to {key[0]}{key[1:]}")
            return
        m = self.config.model
        if key[0] == "VESDE":
            if (float(m.sigma_min), float(m.sigma_max)) != key[1:3]:
                raise T2PError("the VESDE's sigma_min / sigma_max differ from model.sigma_min / sigma_max")
            check(self.lib.t2p_train_set_sde(self._h, _lib.SDE_VE, 0.1, 20.0, None))       # (the betas are unused under VE)
        elif key[0] == "VPSDE":
            table = sde.sqrt_1m_alphas_cumprod.detach().to("cpu", torch.float32).contiguous()     # the reference's float32 table
            check(self.lib.t2p_train_set_sde(self._h, _lib.SDE_VP, key[1], key[2], C.c_void_p(table.data_ptr())))
        else:
            check(self.lib.t2p_train_set_sde(self._h, _lib.SDE_SUBVP, key[1], key[2], None))
        self._sde = key

    def set_ploss(self, diffusion):
        """The DDIM sampler's own objective (``DiffusionSampler.p_loss``, diffusion_sampler.py:144-167) instead of an SDE loss: integer
        timesteps in ``[0, diffusion.timesteps)``, the sampler's ``sqrt_alpha_cumprod`` / ``sqrt_one_minus_alphas_cumprod`` tables (float32,
        from whatever ``betas`` it was built with; ``timesteps`` is not tied to ``model.num_scales``) and ``diffusion.loss_type`` ('l1' or
        'l2').  ``DiffusionSampler.p_loss`` / ``get_ploss_step_fn`` call this on first use; a model stays with the objective it was given."""
        key = _ploss_key(diffusion)
        if self._sde is not None:
            if self._sde != key:
                raise T2PError(f"this model trains under {self._sde[0]}{self._sde[1:]}; it cannot switch to {key[0]}{key[1:]}")
            return
        a = diffusion.sqrt_alpha_cumprod.detach().to("cpu", torch.float32).contiguous()
        s = diffusion.sqrt_one_minus_alphas_cumprod.detach().to("cpu", torch.float32).contiguous()
        check(self.lib.t2p_train_set_ploss(self._h, key[1], key[2], C.c_void_p(a.data_ptr()), C.c_void_p(s.data_ptr())))
        self._sde = key

    def set_dropout_masks(self, masks):
        """Parity runs: NHWC uint8 keep-masks (device tensors), one per residual block in forward order; None / [] = Philox."""
        masks = [m.to(self.device, torch.uint8).contiguous() for m in (masks or [])]
        self._keep = masks
        arr = (C.c_void_p * max(len(masks), 1))(*[m.data_ptr() for m in masks])
        check(self.lib.t2p_train_set_dropout_masks(self._h, arr, len(masks)))

    def set_ss_blocks(self, blocks, drop=None, p=0.2):
        """``block_dropout`` (losses.py:54-64) for the NEXT ``loss`` / ``step`` / ``eval_loss``, which consumes the list: ``blocks`` =
        ``(sample, start, end)`` triples (``parse_ss_indices``), ``drop`` = one decision per block or None = drawn on the device at
        probability ``p``.  ``batch["coords_6d"]`` is not modified (the reference zeroes it in place).  ``[]`` clears the list."""
        arr = np.ascontiguousarray(np.asarray(blocks, dtype=np.int64).reshape(-1, 3))
        if arr.size and (np.abs(arr) > 2 ** 31 - 1).any():
            raise T2PError("ss block index out of the int32 range")
        arr = arr.astype(np.int32)
        n = arr.shape[0]
        d = None
        if drop is not None:
            d = np.ascontiguousarray(np.asarray(drop).reshape(-1) != 0, dtype=np.uint8)
            if d.shape[0] != n:
                raise T2PError(f"{d.shape[0]} block decisions for {n} blocks")
        check(self.lib.t2p_train_set_ss_blocks(self._h, C.c_void_p(arr.ctypes.data) if n else None, n,
                                               C.c_void_p(d.ctypes.data) if d is not None and n else None, float(p)))

    def set_inpaint_draw(self, lengths, inpainting_cfg):
        """``random_mask_batch`` (utils.py:15-60) on the device for the NEXT ``loss`` / ``step`` / ``eval_loss`` whose batch carries no
        ``mask_inpaint``; that pass consumes the request.  ``lengths``: the valid residues per sample; ``inpainting_cfg``:
        ``config.model.inpainting`` (random_mask_prob, contiguous_mask_prob, mask_min_len, mask_max_len).  The number of masked residues
        lies in ``[int(mask_min_len l), int(mask_max_len l))`` as in the reference; an empty range (``l = 1``) raises ``T2PError``.  The
        draws come from the trainer's Philox, not from torch.  ``None`` / ``[]`` clears the request."""
        from .conditions import mask_count_range
        lengths = [] if lengths is None else [int(v) for v in torch.as_tensor(lengths).reshape(-1).tolist()]
        if not lengths:
            check(self.lib.t2p_train_set_inpaint_draw(self._h, None, 0, 0.0, 0.0))
            return
        if inpainting_cfg is None:
            raise T2PError("set_inpaint_draw needs config.model.inpainting (random_mask_prob, contiguous_mask_prob, mask_min_len, mask_max_len)")
        if max(abs(l) for l in lengths) > 2 ** 31 - 1:
            raise T2PError("residue count out of the int32 range")
        L = int(self.config.data.max_res_num)
        arr = np.ascontiguousarray([(l,) + mask_count_range(l, inpainting_cfg, L) for l in lengths], dtype=np.int32)
        check(self.lib.t2p_train_set_inpaint_draw(self._h, C.c_void_p(arr.ctypes.data), arr.shape[0], float(inpainting_cfg.random_mask_prob),
                                                  float(inpainting_cfg.contiguous_mask_prob)))

    def set_context_drop(self, n, drop=None, p=0.1):
        """Text-context dropout (training for classifier-free guidance) for the NEXT ``loss`` / ``step`` / ``eval_loss``, which consumes
        the request: ``n`` = the batch size, ``drop`` = one decision per sample or None = drawn on the device at probability ``p`` from
        the trainer's Philox.  A dropped sample trains exactly as if ``batch["context"][b]`` were all zeros -- the ``context * 0`` of
        the guided samplers; ``batch["context"]`` itself is not modified.  ``n`` = 0 / None clears the request."""
        n = int(n or 0)
        if n == 0:
            check(self.lib.t2p_train_set_context_drop(self._h, None, 0, 0.0))
            return
        d = None
        if drop is not None:
            d = np.ascontiguousarray(np.asarray(drop).reshape(-1) != 0, dtype=np.uint8)
            if d.shape[0] != n:
                raise T2PError(f"{d.shape[0]} context-dropout decisions for {n} samples")
        check(self.lib.t2p_train_set_context_drop(self._h, C.c_void_p(d.ctypes.data) if d is not None else None, n, float(p)))

    def _batch(self, batch, t=None, z=None):
        dev = self.device
        # under the p_loss objective a batch without mask_pair is the reference's unmasked loss (and its mask_inpaint is not passed on)
        unmasked = self._sde is not None and self._sde[0] == "p_loss" and batch.get("mask_pair") is None
        hold = [batch["coords_6d"].to(dev, torch.float32).contiguous(),
                None if unmasked else batch["mask_pair"].to(dev, torch.uint8).contiguous(),
                batch["context"].to(dev, torch.float32).contiguous()]
        tb = TrainBatch()
        tb.coords_6d, tb.mask_pair, tb.context = hold[0].data_ptr(), None if unmasked else hold[1].data_ptr(), hold[2].data_ptr()
        tb.batch, tb.tokens = hold[0].shape[0], hold[2].shape[1]
        if hold[2].shape[2] != self.config.model.context_dim:
            raise T2PError("context width differs from model.context_dim")
        for key, val, dt in (("mask_inpaint", None if unmasked else batch.get("mask_inpaint"), torch.uint8), ("t", t, torch.float32),
                             ("z", z, torch.float32)):
            if val is not None:
                v = val.to(dev, dt).contiguous()
                hold.append(v)
                setattr(tb, key, v.data_ptr())
        return tb, hold

    def _pass_inputs(self, batch, t, z, need_weights=True):
        """``_batch`` for a pass.  A pass that fails here never reaches the library, so a block list (``set_ss_blocks``), a random-mask
        request (``set_inpaint_draw``) or a context-dropout request (``set_context_drop``) set for it is cleared: it is this batch's
        data and must not reach whichever pass comes next."""
        try:
            if need_weights and not self._loaded:
                raise T2PError("load weights before training")
            return self._batch(batch, t, z)
        except Exception:
            self.lib.t2p_train_set_ss_blocks(self._h, None, 0, None, 0.0)
            self.lib.t2p_train_set_inpaint_draw(self._h, None, 0, 0.0, 0.0)
            self.lib.t2p_train_set_context_drop(self._h, None, 0, 0.0)
            raise

    def loss(self, batch, t=None, z=None, backward=False, return_score=False):
        """``loss_fn`` (losses.py:105-134); ``t`` / ``z`` = the draws of :106-107 (None: drawn on the device)."""
        tb, hold = self._pass_inputs(batch, t, z)
        out = C.c_float()
        score = torch.empty_like(hold[0]) if return_score else None
        check(self.lib.t2p_train_loss(self._h, C.byref(tb), int(backward), C.byref(out), ptr(score), stream_ptr()))
        return (float(out.value), score) if return_score else float(out.value)

    def step(self, batch, t=None, z=None):
        """``step_fn`` with train=True (losses.py:165-176) in one call."""
        tb, hold = self._pass_inputs(batch, t, z)
        out = C.c_float()
        check(self.lib.t2p_train_step(self._h, C.byref(tb), C.byref(out), stream_ptr()))
        return float(out.value)

    def apply(self):
        """optimize_fn + ``step += 1`` + ``ema.update`` (losses.py:41-49, 174-176; ema.py:32-49) on the gradient buffer as it stands."""
        check(self.lib.t2p_train_apply(self._h, stream_ptr()))

    def grad_view(self):
        """The flat fp32 gradient buffer (every tensor in ``parameters()`` order) as a torch tensor sharing the trainer's device memory:
        what data-parallel training all-reduces between ``loss(..., backward=True)`` and ``apply()``."""
        p, n = C.c_void_p(), C.c_int64()
        check(self.lib.t2p_train_grad_buffer(self._h, C.byref(p), C.byref(n)))

        class _Buf:          # CUDA array interface: torch wraps the memory without copying
            __cuda_array_interface__ = {"shape": (int(n.value),), "typestr": "<f4", "data": (int(p.value), False), "version": 2}

        keep = _Buf()
        t = torch.as_tensor(keep, device=self.device)
        t._t2p_owner = (self, keep)
        return t

    def eval_loss(self, batch, t=None, z=None):
        """``step_fn`` with train=False (losses.py:177-183): the loss under the EMA weights."""
        tb, hold = self._pass_inputs(batch, t, z, need_weights=False)
        out = C.c_float()
        check(self.lib.t2p_train_eval_loss(self._h, C.byref(tb), C.byref(out), stream_ptr()))
        return float(out.value)

    def device_bytes(self):
        return int(self.lib.t2p_train_device_bytes(self._h))

    def __del__(self):
        try:
            if getattr(self, "_h", None):
                self.lib.t2p_train_destroy(self._h)
                self._h = None
        except Exception:  # noqa: BLE001
            pass


def _sde_key(sde):
    """(class name, parameters, N) of a supported SDE; any other class raises the reference's error (models/utils.py:173-174)."""
    if isinstance(sde, VESDE):
        return ("VESDE", float(sde.sigma_min), float(sde.sigma_max), int(sde.N))
    if isinstance(sde, VPSDE):
        return ("VPSDE", float(sde.beta_0), float(sde.beta_1), int(sde.N))
    if isinstance(sde, subVPSDE):
        return ("subVPSDE", float(sde.beta_0), float(sde.beta_1), int(sde.N))
    raise NotImplementedError(f"SDE class {sde.__class__.__name__} not yet supported.")


_PLOSS_TYPES = {"l1": 1, "l2": 2}


def _ploss_key(diffusion):
    """("p_loss", loss type, timesteps, a checksum of the two tables) of a ``DiffusionSampler``; a ``loss_type`` other than 'l1' / 'l2'
    raises the reference's error (diffusion_sampler.py:160-161)."""
    import zlib
    if diffusion.loss_type not in _PLOSS_TYPES:
        raise NotImplementedError(f'Loss type "{diffusion.loss_type}" not implemented')
    tabs = torch.stack([diffusion.sqrt_alpha_cumprod, diffusion.sqrt_one_minus_alphas_cumprod]).detach().to("cpu", torch.float32).contiguous()
    if tabs.shape[1] != int(diffusion.timesteps):
        raise T2PError(f"the sampler's tables hold {tabs.shape[1]} entries, timesteps is {diffusion.timesteps}")
    return ("p_loss", _PLOSS_TYPES[diffusion.loss_type], int(diffusion.timesteps), zlib.crc32(tabs.numpy().tobytes()))


def check_ploss_t(t, timesteps, batch_size=None):
    """``t`` of ``p_loss``: None (drawn on the device) or an integer tensor [B] inside ``[0, timesteps)``; anything else raises ``T2PError``
    before any native call (the kernel clamps the table index; range and integrality are checked here)."""
    if t is None:
        return None
    if not torch.is_tensor(t) or t.dtype not in (torch.int8, torch.uint8, torch.int16, torch.int32, torch.int64):
        raise T2PError("p_loss: t must be an integer tensor of timesteps (torch.long), one per sample")
    if t.dim() != 1 or (batch_size is not None and t.shape[0] != int(batch_size)):
        raise T2PError(f"p_loss: t must have shape ({batch_size},), got {tuple(t.shape)}")
    if t.numel() and (int(t.min()) < 0 or int(t.max()) >= int(timesteps)):
        raise T2PError(f"p_loss: t outside [0, {int(timesteps)}): min {int(t.min())}, max {int(t.max())}")
    return t


class _ParamHandle:
    """What ``model.parameters()`` returns: the optimizer and the EMA are views of the model's native state."""

    def __init__(self, model):
        self.model = model


def get_train_model(config, seed=0, dtype="f32"):
    """``utils.get_model(config)`` (score_sde_pytorch/utils.py:4-9) for training: no DataParallel, one process per GPU."""
    return HipTrainModel(config, device=config.device if str(config.device) != "cuda" else "cuda:0", seed=seed, dtype=dtype)


class AdamView:
    """``get_optimizer``'s return value: hyper-parameters are those of the config the model was created from."""

    def __init__(self, model, lr, betas, eps, weight_decay):
        self.model = model
        self.param_groups = [dict(lr=lr, betas=betas, eps=eps, weight_decay=weight_decay)]

    def zero_grad(self):
        pass            # the native step zeroes the gradient buffer itself

    def state_dict(self):
        """``torch.optim.Adam.state_dict()`` layout (what the reference's save_checkpoint stores, score_sde_pytorch/utils.py:19-26):
        ``state`` = {parameter index: {step, exp_avg, exp_avg_sq}} in ``parameters()`` order (empty before the first update),
        ``param_groups`` = one group listing every index."""
        k = self.model.get_step()[1]
        names = [s.name for s in self.model._specs]
        state = {}
        if k > 0:
            m, v = self.model.read(EXP_AVG), self.model.read(EXP_AVG_SQ)
            state = {i: {"step": torch.tensor(float(k)), "exp_avg": m[n], "exp_avg_sq": v[n]} for i, n in enumerate(names)}
        g = dict(self.param_groups[0])
        group = dict(lr=g["lr"], betas=tuple(g["betas"]), eps=g["eps"], weight_decay=g["weight_decay"], amsgrad=False, maximize=False,
                     foreach=None, capturable=False, differentiable=False, fused=None, decoupled_weight_decay=False,
                     params=list(range(len(names))))
        return dict(state=state, param_groups=[group])

    def load_state_dict(self, sd):
        names = [s.name for s in self.model._specs]
        st = sd.get("state", {})
        cur = self.model.get_step()
        if not st:
            self.model.set_step(cur[0], adam_updates=0)
            return
        if len(st) != len(names):
            raise T2PError(f"optimizer state holds {len(st)} tensors, the model has {len(names)}")
        self.model.write(EXP_AVG, {n: st[i]["exp_avg"] for i, n in enumerate(names)})
        self.model.write(EXP_AVG_SQ, {n: st[i]["exp_avg_sq"] for i, n in enumerate(names)})
        steps = {int(torch.as_tensor(st[i]["step"]).item()) for i in range(len(names))}
        if len(steps) != 1:
            raise T2PError("per-parameter Adam step counts differ: not a state this trainer can continue from")
        self.model.set_step(cur[0], adam_updates=steps.pop())


def get_optimizer(config, params):
    """losses.py:26-36."""
    if config.optim.optimizer != "Adam":
        raise NotImplementedError(f"Optimizer {config.optim.optimizer} not supported yet!")
    if not isinstance(params, _ParamHandle):
        raise TypeError("get_optimizer takes model.parameters() of a HipTrainModel")
    o = config.optim
    return AdamView(params.model, o.lr, (o.beta1, 0.999), o.eps, o.weight_decay)


def optimization_manager(config):
    """losses.py:38-51.  The returned function only checks that its arguments are the ones the native step was built with
    (the warm-up, the clipping and the Adam update themselves run inside ``t2p_train_step``)."""
    o = config.optim

    def optimize_fn(optimizer, params, step, lr=o.lr, warmup=o.warmup, grad_clip=o.grad_clip):
        tc = optimizer.model._tc
        if (float(lr), float(warmup), float(grad_clip)) != (tc.lr, tc.warmup, tc.grad_clip):
            raise T2PError("optimize_fn arguments differ from the configuration the model was created with")

    return optimize_fn


class ExponentialMovingAverage:
    """models/ema.py:8-93 as a view of the model's EMA buffer."""

    def __init__(self, parameters, decay, use_num_updates=True):
        if decay < 0.0 or decay > 1.0:
            raise ValueError("Decay must be between 0 and 1")                                # ema.py:24-25
        if not isinstance(parameters, _ParamHandle):
            raise TypeError("ExponentialMovingAverage takes model.parameters() of a HipTrainModel")
        self.model = parameters.model
        if abs(decay - self.model._tc.ema_rate) > 1e-12 or not use_num_updates:
            raise T2PError("the EMA of a HipTrainModel runs with model.ema_rate and use_num_updates=True")
        self.decay = decay

    @property
    def num_updates(self):
        return self.model.get_step()[2]

    @property
    def shadow_params(self):
        return list(self.model.read(EMA).values())

    def _same_model(self, parameters):
        if not isinstance(parameters, _ParamHandle) or parameters.model is not self.model:
            raise TypeError("takes model.parameters() of the HipTrainModel this EMA was created from")

    def store(self, parameters):
        """ema.py:72-78: save the current parameters for ``restore`` (a device-to-device copy into the trainer's stash)."""
        self._same_model(parameters)
        self.model.copy_buffer(STASH, PARAM)

    def copy_to(self, parameters):
        """ema.py:51-62: the parameters become the EMA shadow (device-to-device)."""
        self._same_model(parameters)
        self.model.copy_buffer(PARAM, EMA)

    def restore(self, parameters):
        """ema.py:80-84 (and :64-70): the parameters saved by ``store`` come back; raises before any ``store``."""
        self._same_model(parameters)
        self.model.copy_buffer(PARAM, STASH)

    def state_dict(self):
        return dict(decay=self.decay, num_updates=self.num_updates, shadow_params=self.shadow_params)      # ema.py:86-88

    def load_state_dict(self, state_dict):
        names = [s.name for s in self.model._specs]
        self.model.write(EMA, dict(zip(names, state_dict["shadow_params"])))
        cur = self.model.get_step()
        self.model.set_step(cur[0], ema_updates=int(state_dict["num_updates"]))


def get_sde_loss_fn(sde, train, eps=1e-5, block_dropout=0.2, block_dropout_draw="host", inpaint_mask_draw=None, context_dropout=0.0,
                    context_dropout_draw="device"):
    """losses.py:66-136 for ``sde`` = VESDE, VPSDE or subVPSDE (the model takes the SDE on first use and keeps it).  ``batch["context"]`` holds the caption embedding (B, T, context_dim); with raw captions pass
    ``llm_components`` = a callable ``captions -> embedding`` (text2protein_amd.text_context.TextContextProducer).

    With ``"ss"`` in ``condition`` and ``batch["ss_indices"]`` present, every block is dropped with probability ``block_dropout``
    (losses.py:54-64, :106-107; train and eval alike).  ``block_dropout_draw="host"``: ``random.random()`` once per block in the
    reference's order, so the same ``random.seed`` drops the same blocks; ``"device"``: drawn on the GPU from the trainer seed.  A batch
    without ``ss_indices`` has nothing dropped (the reference would raise ``KeyError``).

    ``inpaint_mask_draw``: with ``"inpainting"`` in ``condition`` and no ``batch["mask_inpaint"]``, the random mask that train.py draws
    before every train and eval step (``utils.random_mask_batch``, train.py:176, :193) from ``config.model.inpainting`` and the residue
    counts ``batch["lengths"]`` / ``batch["aa_str"]``.  ``"host"``: ``conditions.random_mask_batch``, the reference's ``random`` / ``torch``
    draws in its order (the same seeds give its mask); ``"device"``: drawn on the GPU from the trainer seed
    (``HipTrainModel.set_inpaint_draw``).  None (the default): no mask is drawn and such a batch is refused.

    ``context_dropout``: training for classifier-free guidance.  With ``train=True`` and a probability above 0, every sample of every
    batch loses its text context with that probability and trains exactly as if ``batch["context"][b]`` were all zeros -- the
    ``context * 0`` that ``--guidance_w`` / ``guidance_w=`` evaluate (``HipTrainModel.set_context_drop``; the reference's loss has no
    counterpart).  ``context_dropout_draw="device"``: drawn on the GPU from the trainer seed; ``"host"``: ``random.random()`` once per
    sample in sample order, after the block-dropout and inpainting-mask host draws, so one ``random.seed`` reproduces a step.
    ``train=False`` never drops: the evaluation loss stays the conditional one.  At 0.0 (the default) nothing is requested and no
    ``random`` draw is consumed.  A probability outside [0, 1] or an unknown draw mode raises ``ValueError`` here."""
    _sde_key(sde)
    _check_draw(block_dropout_draw)
    _check_inpaint_draw(inpaint_mask_draw)
    _check_context_dropout(context_dropout, context_dropout_draw)
    context_dropout = float(context_dropout)

    def loss_fn(model, batch, condition=None, llm_components=None, t=None, z=None):
        model.set_sde(sde)
        if condition_flags(condition) != model._tc.cond_flags:
            raise T2PError("`condition` differs from the model.condition the model was created with")
        if "context" not in batch:
            if llm_components is None:
                raise T2PError("the batch holds no `context`; pass llm_components=TextContextProducer(...)")
            batch = dict(batch, context=llm_components(batch["caption"]))
        _set_batch_ss_blocks(model, batch, condition, block_dropout, block_dropout_draw)
        batch = _draw_batch_inpaint_mask(model, batch, condition, inpaint_mask_draw)
        if train:
            _request_context_drop(model, batch, context_dropout, context_dropout_draw)
            return model.loss(batch, t=t, z=z, backward=False)
        return model.eval_loss(batch, t=t, z=z)

    return loss_fn


def _run_step(state, batch, condition, t, z, set_objective, train, optimize_fn, dist, world, block_dropout, block_dropout_draw,
              inpaint_mask_draw, context_dropout, context_dropout_draw):
    """The body of ``step_fn`` (losses.py:165-186) whatever the objective: ``set_objective(model)`` gives the model its SDE
    (``get_step_fn``) or the DDIM sampler's p_loss (``get_ploss_step_fn``) on first use; everything after it is the same."""
    model = state["model"]
    set_objective(model)
    if condition_flags(condition) != model._tc.cond_flags:
        raise T2PError("`condition` differs from the model.condition the model was created with")
    if "context" not in batch:
        producer = state.get("llm")
        if producer is None:
            raise T2PError("the batch holds no `context`; put a TextContextProducer under state['llm']")
        batch = dict(batch, context=producer(batch["caption"]))
    if train:
        if optimize_fn is not None:
            optimize_fn(state["optimizer"], model.parameters(), step=state["step"])
        _set_batch_ss_blocks(model, batch, condition, block_dropout, block_dropout_draw)
        batch = _draw_batch_inpaint_mask(model, batch, condition, inpaint_mask_draw)
        _request_context_drop(model, batch, context_dropout, context_dropout_draw)
        prev = model.get_step()
        model.set_step(state["step"])
        if world == 1:
            try:
                loss = model.step(batch, t=t, z=z)            # zero_grad, loss, backward, optimize_fn, ema.update
            except T2PError:
                model.set_step(*prev)                         # a refused 16-bit step leaves the counters as they were
                raise
        else:
            from . import distributed as D
            try:
                loss = model.loss(batch, t=t, z=z, backward=True)
            except T2PError:
                model.set_step(*prev)                         # a refused pass (a block outside the batch) changes nothing
                raise
            D.allreduce_mean_(model.grad_view(), dist)        # one collective over the whole gradient
            loss = D.mean_over_ranks(loss, dist, model.device)
            try:
                model.apply()
            except T2PError:
                model.set_step(*prev)                         # as above: a refused 16-bit step leaves the counters as they were
                raise
        state["step"] += 1
        return loss
    _set_batch_ss_blocks(model, batch, condition, block_dropout, block_dropout_draw)
    batch = _draw_batch_inpaint_mask(model, batch, condition, inpaint_mask_draw)
    return model.eval_loss(batch, t=t, z=z)                  # ema.store / copy_to / loss / restore (losses.py:177-183)


def get_step_fn(sde, train, optimize_fn=None, dist=None, block_dropout=0.2, block_dropout_draw="host", inpaint_mask_draw=None,
                context_dropout=0.0, context_dropout_draw="device"):
    """losses.py:140-186.  ``block_dropout`` / ``block_dropout_draw`` / ``inpaint_mask_draw``: as in ``get_sde_loss_fn`` (each rank drops the blocks and draws the mask of its shard).  ``dist`` (an initialised ``torch.distributed`` module, text2protein_amd.distributed.init_process_group):
    data-parallel training, one process per GPU -- each rank takes its shard of the batch, the flat gradient buffer is averaged over
    the ranks with ONE all-reduce (RCCL over xGMI) and every rank applies the same update; the returned loss is the mean over the
    ranks.  With equal shards this is the reference's DataParallel step on the concatenated batch (the loss is a mean of per-sample
    terms, losses.py:128-131).

    ``context_dropout`` / ``context_dropout_draw``: as in ``get_sde_loss_fn`` (train steps only).  Under ``dist`` each rank decides for
    its own shard; the device draw is keyed by the trainer seed and the sample's index WITHIN the shard, so ranks need different
    trainer seeds (``get_train_model(config, seed=base + rank)``) to drop different patterns."""
    _sde_key(sde)
    _check_draw(block_dropout_draw)
    _check_inpaint_draw(inpaint_mask_draw)
    _check_context_dropout(context_dropout, context_dropout_draw)
    context_dropout = float(context_dropout)
    world = dist.get_world_size() if dist is not None and dist.is_initialized() else 1

    def step_fn(state, batch, condition=None, t=None, z=None):
        return _run_step(state, batch, condition, t, z, lambda model: model.set_sde(sde), train, optimize_fn, dist, world, block_dropout,
                         block_dropout_draw, inpaint_mask_draw, context_dropout, context_dropout_draw)

    return step_fn


def get_ploss_step_fn(diffusion, train, optimize_fn=None, dist=None, masked=True, block_dropout=0.2, block_dropout_draw="host",
                      inpaint_mask_draw=None, context_dropout=0.0, context_dropout_draw="device"):
    """``get_step_fn`` for the DDIM sampler's own objective (``DiffusionSampler.p_loss``, diffusion_sampler.py:144-167): ``diffusion`` is the
    ``text2protein_amd.ddim.DiffusionSampler`` whose tables and ``loss_type`` the model takes on first use (``HipTrainModel.set_ploss``).
    ``step_fn(state, batch, condition=None, t=None, z=None)``: ``t`` = integer timesteps in ``[0, diffusion.timesteps)`` or None = drawn
    on the device, ``z`` = the noise or None.  Everything else -- optimize_fn, the per-batch requests, data-parallel training under
    ``dist``, the evaluation loss under the EMA with ``train=False`` -- is ``get_step_fn``'s, through the same body.

    ``masked=True`` (the default): the mask of the SDE loss (``batch["mask_pair"]`` x the conditional mask of ``condition``); frozen entries
    reach the network clean, as ``ddim_sample(condition=...)`` re-imposes them.  ``masked=False``: the reference's loss as written, every
    element counts; ``mask_pair`` / ``mask_inpaint`` are not passed on, and no block list or inpainting mask is requested."""
    _ploss_key(diffusion)
    _check_draw(block_dropout_draw)
    _check_inpaint_draw(inpaint_mask_draw)
    _check_context_dropout(context_dropout, context_dropout_draw)
    context_dropout = float(context_dropout)
    world = dist.get_world_size() if dist is not None and dist.is_initialized() else 1

    def step_fn(state, batch, condition=None, t=None, z=None):
        check_ploss_t(t, diffusion.timesteps, batch["coords_6d"].shape[0])
        if not masked:
            batch = {k: v for k, v in batch.items() if k not in ("mask_pair", "mask_inpaint", "ss_indices")}
        return _run_step(state, batch, condition, t, z, lambda model: model.set_ploss(diffusion), train, optimize_fn, dist, world, block_dropout,
                         block_dropout_draw, None if not masked else inpaint_mask_draw, context_dropout, context_dropout_draw)

    return step_fn
