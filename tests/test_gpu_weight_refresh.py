"""On-device weight refresh: a trainer's parameters or EMA into the score engine without leaving the GPU (``HipScoreModel.load_from``,
``t2p_engine_load_flat``), the EMA verbs on ``t2p_train_copy`` and the snapshot block of the reference's training loop
(train.py:198-215).  The yardstick is always the host load path (``load_state_dict`` / ``load_ema_shadow``) fed the same numbers;
every comparison is ``torch.equal``.

Paths of ``Engine::pack_weights`` the three configurations of the first test open (read off its gates):
  tinyB   (32 / 32 / 64 channels, C = 8): up and down blocks (the four-phase conv0 in 16-bit), AttnBlockpp + SpatialTransformer at 64
          and 32 channels (both weight products), the split input convolution, the fused shortcut of the 128 -> 64 out blocks;
  smallC  (64 / 128 channels): the fused shortcut and the feed-forward / proj_out product at two widths;
  wide256 (128 / 256 channels, attention at 256): every ``ci == 256`` fragment-major copy (fm_qk, fm_v3, fm_in .. fm_ff1, fm_ffpo).
          The configuration the issue proposes takes these paths as it stands; it was not adjusted.
"""
import ctypes as C
import functools

import pytest
import torch

from helpers import cfg_smallC, cfg_tinyB, cfg_train_tiny, train_inputs

pytestmark = pytest.mark.gpu

PARAM, EMA = 0, 2


def cfg_wide256():
    from text2protein_amd.config import tiny_config
    return tiny_config(**{"model.nf": 128, "model.ch_mult": [1, 2], "model.num_res_blocks": 1, "data.max_res_num": 16,
                          "model.attn_resolutions": [8], "model.n_heads": 4, "model.context_dim": 64, "model.num_scales": 10})


CONFIGS = {"tinyB": cfg_tinyB, "smallC": cfg_smallC, "wide256": cfg_wide256}


@functools.lru_cache(maxsize=None)
def _weights(name, seed):
    from text2protein_amd import synth
    return synth.synth_state_dict(_cfg(name), seed)


def _cfg(name):
    cfg = (CONFIGS.get(name) or {"train_tiny": cfg_train_tiny}[name])()
    cfg.device = "cuda:0"
    return cfg


def _engine(cfg, dtype, state_dict=None):
    from text2protein_amd.model import HipScoreModel
    m = HipScoreModel(cfg, dtype=dtype, device="cuda:0")
    if state_dict is not None:
        m.load_state_dict(state_dict)
    return m


def _trainer(cfg, dtype, state_dict, seed=11):
    from text2protein_amd.losses import HipTrainModel
    t = HipTrainModel(cfg, device="cuda:0", seed=seed, dtype=dtype)
    t.load_state_dict(state_dict)
    return t


def _inputs(cfg, seed=0):
    from text2protein_amd import synth
    Cx, L, N = cfg.data.num_channels, cfg.data.max_res_num, cfg.model.num_scales
    x = torch.from_numpy(synth.normal(seed, "refresh_x", 2 * Cx * L * L).reshape(2, Cx, L, L)).cuda()
    return x, torch.tensor([0, N - 1]).cuda(), synth.synth_context(2, 5, cfg.model.context_dim, seed + 3).cuda()


def _score(model, cfg, seed=0):
    x, labels, ctx = _inputs(cfg, seed)
    out = model(x, labels, ctx)
    torch.cuda.synchronize()
    return out.cpu()


def _train_batch(cfg, B=2):
    case = dict(B=B, T=5, seed=4, lengths=[cfg.data.max_res_num, 11][:B])
    inp = train_inputs(cfg, case)
    return {k: inp[k] for k in ("coords_6d", "mask_pair", "context")}, inp


def _two_steps(trainer, cfg):
    batch, inp = _train_batch(cfg)
    trainer.set_step(2000)              # inside the warm-up ramp: a learning rate above 0, so the parameters move
    for _ in range(2):
        trainer.step(batch, t=inp["t"], z=inp["z"])


@pytest.mark.parametrize("dtype", ["f32", "f16", "bf16"])
@pytest.mark.parametrize("name", ["tinyB", "smallC", "wide256"])
def test_refresh_equals_host_load(name, dtype):
    cfg = _cfg(name)
    W = _weights(name, 1)
    a = _engine(cfg, dtype, W)
    trainer = _trainer(cfg, dtype, W)
    b = _engine(cfg, dtype).load_from(trainer, "param")
    assert b.device_bytes() == a.device_bytes()           # the same persistent buffers, nothing else
    want, got = _score(a, cfg), _score(b, cfg)
    assert torch.isfinite(want).all() and torch.equal(got, want)
    assert b.pool_reclaimed() == 0


def test_refresh_across_compute_dtypes():
    """A bf16 trainer feeds an f16 engine: the flat buffers are fp32 whatever the trainer computes in."""
    cfg = _cfg("tinyB")
    W = _weights("tinyB", 1)
    b = _engine(cfg, "f16").load_from(_trainer(cfg, "bf16", W), "ema")      # a loaded trainer's EMA is a clone of its parameters
    assert torch.equal(_score(b, cfg), _score(_engine(cfg, "f16", W), cfg))


def test_refresh_in_place():
    from text2protein_amd import losses
    cfg = _cfg("tinyB")
    trainer = _trainer(cfg, "f16", _weights("tinyB", 1))
    b = _engine(cfg, "f16").load_from(trainer, "param")
    first = _score(b, cfg)                                # also builds the lazily made fragment-major convolution copies
    bytes_before = b.device_bytes()
    _two_steps(trainer, cfg)
    ema = trainer.read(losses.EMA)
    assert not torch.equal(ema["pre_conv.weight"], trainer.read(losses.PARAM, "pre_conv.weight"))
    b.load_from(trainer, "ema")
    fresh = _engine(cfg, "f16", ema)
    want, got = _score(fresh, cfg), _score(b, cfg)
    assert torch.equal(got, want) and not torch.equal(got, first)
    assert b.device_bytes() == bytes_before and b.pool_reclaimed() == 0
    b.load_from(trainer, "ema")
    assert b.device_bytes() == bytes_before
    # and over a host-loaded engine: whichever way the engine was first loaded
    a = _engine(cfg, "f16", _weights("tinyB", 1))
    assert torch.equal(_score(a, cfg), first)
    n = a.device_bytes()
    a.load_from(trainer, "ema")
    assert torch.equal(_score(a, cfg), want) and a.device_bytes() == n


def test_stale_context_is_refused():
    from text2protein_amd._lib import ptr, stream_ptr
    cfg = _cfg("tinyB")
    trainer = _trainer(cfg, "f16", _weights("tinyB", 1))
    b = _engine(cfg, "f16").load_from(trainer, "param")
    before = _score(b, cfg)
    ctx_key = b._ctx_key
    assert ctx_key is not None
    _two_steps(trainer, cfg)
    b.load_from(trainer, "param")
    assert b._ctx_key is None
    x, labels, ctx = _inputs(cfg)
    out = torch.full_like(x, -5.0)
    labels32 = labels.to(torch.int32)
    rc = b.lib.t2p_engine_score(b._h, ptr(x), ptr(labels32), ptr(out), 2, stream_ptr())
    torch.cuda.synchronize()
    assert rc != 0 and b"set_context must be called" in b.lib.t2p_last_error()
    assert bool((out == -5.0).all())
    got = b(x, labels, ctx)                                # the Python call re-projects its context
    fresh = _engine(cfg, "f16", trainer.read(PARAM))
    assert torch.equal(got.cpu(), _score(fresh, cfg)) and not torch.equal(got.cpu(), before)
    assert b.pool_reclaimed() == 0


def test_refusals_change_nothing():
    from text2protein_amd._lib import T2PError, stream_ptr
    from text2protein_amd.config import tiny_config
    cfg = _cfg("tinyB")
    W = _weights("tinyB", 1)
    trainer = _trainer(cfg, "f16", W)
    b = _engine(cfg, "f16").load_from(trainer, "param")
    before = _score(b, cfg)

    def still_scores():
        assert torch.equal(_score(b, cfg), before)

    other = _cfg("train_tiny")                             # another block list: the parameter count differs
    with pytest.raises(T2PError, match="parameter tensors"):
        b.load_from(_trainer(other, "f16", _weights("train_tiny", 2)), "param")
    still_scores()
    # the same block list at another context width: the count and the names agree, a shape differs
    wider = tiny_config(**{"model.ch_mult": [1, 1, 2], "model.num_res_blocks": 2, "data.num_channels": 8, "model.attn_resolutions": [4, 8],
                           "model.n_heads": 2, "model.context_dim": 32, "model.nf": 32})
    wider.device = "cuda:0"
    from text2protein_amd import synth
    with pytest.raises(T2PError, match="shape of .* differs"):
        b.load_from(_trainer(wider, "f16", synth.synth_state_dict(wider, 1)), "param")
    still_scores()
    for which in (1, 3, 4):
        with pytest.raises(T2PError, match="which is 0 .parameters. or 2 .EMA shadow."):
            b.load_from(trainer, which)
        still_scores()
    with pytest.raises(ValueError):
        b.load_from(trainer, "shadow")
    p, n = C.c_void_p(), C.c_int64()
    assert b.lib.t2p_train_buffer(trainer._h, PARAM, C.byref(p), C.byref(n)) == 0
    assert n.value == sum(v.numel() for v in W.values())
    for bad in (n.value - 1, n.value + 1):
        assert b.lib.t2p_engine_load_flat(b._h, p, bad, stream_ptr()) != 0
        assert b"element count" in b.lib.t2p_last_error()
        still_scores()
    assert b.lib.t2p_train_buffer(trainer._h, 1, C.byref(p), C.byref(n)) != 0
    assert b.lib.t2p_engine_load_flat(b._h, p, n.value, stream_ptr()) == 0       # the right n loads
    still_scores()


def test_ema_verbs():
    from text2protein_amd import losses
    from text2protein_amd._lib import T2PError
    cfg = _cfg("tinyB")
    W = _weights("tinyB", 1)
    t1, t2 = _trainer(cfg, "f16", W), _trainer(cfg, "f16", W)
    batch, inp = _train_batch(cfg)
    for t in (t1, t2):
        t.set_step(2000)
        t.step(batch, t=inp["t"], z=inp["z"])
    ema = losses.ExponentialMovingAverage(t1.parameters(), decay=cfg.model.ema_rate)
    with pytest.raises(T2PError, match="restore .* before any store"):
        ema.restore(t1.parameters())
    with pytest.raises(TypeError):
        ema.store(t2.parameters())
    params = t1.read(losses.PARAM)
    shadow = t1.read(losses.EMA)
    assert any(not torch.equal(params[k], shadow[k]) for k in params)
    bytes_before = t1.device_bytes()
    ema.store(t1.parameters())
    stash = t1.device_bytes() - bytes_before
    n_bytes = 4 * sum(v.numel() for v in W.values())
    assert n_bytes <= stash < n_bytes + 4096               # the stash, counted (the pool rounds an allocation up to its granule)
    ema.copy_to(t1.parameters())
    now = t1.read(losses.PARAM)
    assert all(torch.equal(now[k], shadow[k]) for k in shadow)
    ema.restore(t1.parameters())
    now = t1.read(losses.PARAM)
    assert all(torch.equal(now[k], params[k]) for k in params)
    ema.store(t1.parameters())
    assert t1.device_bytes() == bytes_before + stash       # allocated once
    # nothing the trainer derives from its parameters is left stale: the next step matches a twin that never cycled
    for t in (t1, t2):
        t.step(batch, t=inp["t"], z=inp["z"])
    a, b = t1.read(losses.PARAM), t2.read(losses.PARAM)
    assert all(torch.equal(a[k], b[k]) for k in a)
    a, b = t1.read(losses.EMA), t2.read(losses.EMA)
    assert all(torch.equal(a[k], b[k]) for k in a)


def _pc_sampling_fn(cfg, shape):
    from text2protein_amd import sampling, sde_lib
    sde = sde_lib.VESDE(sigma_min=cfg.model.sigma_min, sigma_max=cfg.model.sigma_max, N=cfg.model.num_scales)
    fn = sampling.get_sampling_fn(cfg, sde, shape, 1e-5, seed=3)
    return lambda model, condition, context: fn(model, condition, context, n_iter=3, call_index=0)[0]


def _ddim_sampling_fn(cfg, shape):
    from text2protein_amd import sde_lib
    from text2protein_amd.ddim import DiffusionSampler
    vp = sde_lib.VPSDE(beta_min=cfg.model.beta_min, beta_max=cfg.model.beta_max, N=cfg.model.num_scales)
    return lambda model, condition, context: DiffusionSampler.from_sde(model, vp, sampling_steps=3, ddim_eta=1.0, w=0.5, seed=3).ddim_sample(
        shape, context, condition=condition, call_index=0)


@pytest.mark.parametrize("route", ["pc", "ddim"])
def test_snapshot_block_as_the_training_loop_writes_it(route):
    from text2protein_amd import losses
    cfg = _cfg("train_tiny")
    train_model = _trainer(cfg, "f16", _weights("train_tiny", 2))
    ema = losses.ExponentialMovingAverage(train_model.parameters(), decay=cfg.model.ema_rate)
    _two_steps(train_model, cfg)
    B, Cx, L = 2, cfg.data.num_channels, cfg.data.max_res_num
    shape = (B, Cx, L, L)
    mask = torch.zeros(B, L, L)
    mask[0, :12, :12] = 1
    mask[1, :9, :9] = 1
    condition = {"length": mask.cuda()}
    from text2protein_amd import synth
    context = synth.synth_context(B, 4, cfg.model.context_dim, 8).cuda()
    sampling_fn = (_pc_sampling_fn if route == "pc" else _ddim_sampling_fn)(cfg, shape)
    before = train_model.read(losses.PARAM)
    shadow = train_model.read(losses.EMA)
    # train.py:198-215
    ema.store(train_model.parameters())
    ema.copy_to(train_model.parameters())
    sample = sampling_fn(train_model, condition, context)
    ema.restore(train_model.parameters())
    torch.cuda.synchronize()
    after = train_model.read(losses.PARAM)
    assert all(torch.equal(after[k], before[k]) for k in before)
    ref_model = _engine(cfg, "f16")
    ref_model.load_ema_shadow(list(shadow.values()))
    want = sampling_fn(ref_model, condition, context)
    torch.cuda.synchronize()
    assert torch.isfinite(want).all() and torch.equal(sample.cpu(), want.cpu())
    # a second snapshot after more training reuses the trainer's sampling model and sees the new weights
    _two_steps(train_model, cfg)
    ema.store(train_model.parameters())
    ema.copy_to(train_model.parameters())
    again = sampling_fn(train_model, condition, context)
    ema.restore(train_model.parameters())
    assert len(train_model._samplers) == 1 and not torch.equal(again.cpu(), want.cpu())


def test_captured_step_graph_survives_a_refresh():
    from text2protein_amd import sampling, sde_lib, synth
    cfg = _cfg("train_tiny")
    trainer = _trainer(cfg, "f16", _weights("train_tiny", 2))
    model = _engine(cfg, "f16").load_from(trainer, "param")
    sde = sde_lib.VESDE(sigma_min=cfg.model.sigma_min, sigma_max=cfg.model.sigma_max, N=cfg.model.num_scales)
    ctx = synth.synth_context(2, 3, cfg.model.context_dim, 0).cuda()
    shape = (2, cfg.data.num_channels, cfg.data.max_res_num, cfg.data.max_res_num)
    x0 = sampling._device_randn_like(torch.empty(shape, device="cuda"), 9, 0) * 100.0
    model.set_context(ctx)
    st = sampling.PCStepper(model, sde, 2, cfg.sampling.snr, seed=5)
    x, xm = x0.clone(), torch.empty_like(x0)
    side = torch.cuda.Stream()
    st.reset(0)
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        for _ in range(3):                                 # one eager step, the capture, one more replay
            st.step_graph(x, xm)
    torch.cuda.synchronize()
    old = xm.clone()
    _two_steps(trainer, cfg)
    torch.cuda.synchronize()
    with torch.cuda.stream(side):
        model.load_from(trainer, "ema")
        model.set_context(ctx)
        x.copy_(x0)
        st.reset(0)
        for _ in range(2):
            st.step_graph(x, xm)                           # the graph captured before the refresh
    torch.cuda.synchronize()
    fresh = _engine(cfg, "f16", trainer.read(EMA))
    fresh.set_context(ctx)
    st2 = sampling.PCStepper(fresh, sde, 2, cfg.sampling.snr, seed=5)
    x2, xm2 = x0.clone(), torch.empty_like(x0)
    st2.reset(0)
    with torch.cuda.stream(side):
        for _ in range(2):
            st2.step(x2, xm2)
    torch.cuda.synchronize()
    assert torch.isfinite(x2).all() and torch.equal(x, x2) and torch.equal(xm, xm2)
    assert not torch.equal(xm, old)
