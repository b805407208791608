"""Every device draw against an independent statement of the generator (oracle/philox.py) and, for the normals, against the bits
the library drew before the generator moved into csrc/philox.h (tests/golden/philox_parent.npz, tests/golden/make_golden_philox.py).

The (key, stream, step, counter) of every draw is tabulated at the top of text2protein_amd/csrc/philox.h.
"""
import sys

import numpy as np
import pytest
import torch

from helpers import GOLDEN, TRAIN_CASES, cfg_tiny, load_golden, rel_l2, train_inputs
from oracle import philox

sys.path.insert(0, GOLDEN)
from make_golden_philox import CASES, N, draw          # noqa: E402

pytestmark = pytest.mark.gpu

# max |device - restatement| over the three cases, measured on an MI355X at the commit the fixture names (logf / sqrtf / sincosf
# and the float32 result against float64): 4.701e-7, 3.771e-7, 3.787e-7
MEASURED_MAX_ERR = 4.701e-7


def test_normals_against_the_restatement():
    """t2p_op_philox_normal, n = 4099 (a scalar tail, 5 workgroups), three (seed, stream) cases, every element against
    oracle.philox.normals.  The device's logf and sincosf are not float64, so the bound is a measurement: the largest difference at
    the parent commit was 4.701e-7 (|z| reaches 3.85 there: one float32 ulp at that size is 2.4e-7); asserted is four times that (another box's
    libdevice may round differently), and never more than 1e-5.  A wrong word, pairing or counter gives differences of order 1."""
    bound = 4 * MEASURED_MAX_ERR
    assert bound <= 1e-5
    for name, (seed, stream) in CASES.items():
        z = draw(seed, stream)
        want = philox.normals(seed, stream, 0, N)
        err = float(np.abs(z.astype(np.float64) - want).max())
        print(f"[{name}] max |device - restatement| = {err:.3e} (bound {bound:.1e}), max |z| = {np.abs(z).max():.3f}")
        assert z.shape == want.shape == (N,) and err <= bound, name
    seed, stream = CASES["wrapped_stream"]
    # the recorded wart (philox.h): the sampling layout keeps the low 32 bits of the stream id, so s and s + 2^32 draw the same bits
    assert np.array_equal(draw(seed, stream + 2 ** 32), draw(seed, stream))
    assert np.array_equal(philox.normals(seed, stream + 2 ** 32, 0, N), philox.normals(seed, stream, 0, N))


def test_normals_equal_the_parent_bit_for_bit():
    g = load_golden("philox_parent")
    assert int(g["n"]) == N and len(str(g["commit"])) == 40
    for name, (seed, stream) in CASES.items():
        assert (int(g[name + "_seed"]), int(g[name + "_stream"])) == (seed, stream)
        assert torch.equal(torch.from_numpy(draw(seed, stream)), torch.from_numpy(g[name])), name
    seed, stream = CASES["wrapped_stream"]
    assert torch.equal(torch.from_numpy(draw(seed, stream + 2 ** 32)), torch.from_numpy(g["wrapped_stream"]))


def test_the_step_word_of_the_fused_pc_loop():
    """Only the fused PC loop draws under a nonzero step word.  One step at loop step 2 with device noise against the same step with
    the restatement's noise injected (corrector: stream 2, predictor: stream 1, step word 2): rel-L2 <= 1e-5, smoke()'s bound."""
    from text2protein_amd import sampling, sde_lib, synth
    from text2protein_amd.model import HipScoreModel
    cfg = cfg_tiny()
    cfg.device = "cuda"
    seed, B = 5, 2
    model = HipScoreModel(cfg, dtype="f32")
    model.load_state_dict(synth.synth_state_dict(cfg, 0))
    model.set_context(synth.synth_context(B, 3, cfg.model.context_dim, 0).cuda())
    sde = sde_lib.VESDE(sigma_min=cfg.model.sigma_min, sigma_max=cfg.model.sigma_max, N=cfg.model.num_scales)
    st = sampling.PCStepper(model, sde, B, cfg.sampling.snr, n_steps=1, seed=seed)
    x0 = sampling._device_randn_like(torch.empty(B, cfg.data.num_channels, 16, 16, device="cuda"), 9, 0) * 100.0
    n = x0.numel()
    runs = []
    for inject in (False, True):
        x, xm = x0.clone(), torch.empty_like(x0)
        noise = [None, None]
        if inject:
            noise = [torch.from_numpy(philox.normals(seed, s, 2, n).astype(np.float32)).reshape(x0.shape).cuda() for s in (2, 1)]
        st.reset(2)
        st.step(x, xm, noise_corrector=noise[0], noise_predictor=noise[1])
        torch.cuda.synchronize()
        runs.append((x.cpu(), xm.cpu()))
    e_x, e_xm = rel_l2(runs[0][0], runs[1][0]), rel_l2(runs[0][1], runs[1][1])
    # another step word is another draw: the restatement's noise at step word 0 is not what the loop drew at step 2
    assert not np.array_equal(philox.normals(seed, 1, 0, 8), philox.normals(seed, 1, 2, 8))
    print(f"PC step at loop step 2, device noise vs injected restatement: x {e_x:.2e}, x_mean {e_xm:.2e}")
    assert e_x <= 1e-5 and e_xm <= 1e-5 and not torch.equal(runs[0][0], x0.cpu())


def test_block_decisions_are_the_restatement_exactly():
    """t2p_op_ss_block_dropout with the 4096 blocks, seed and stream of test_operator_device_draws at p = 0.2: drop_out[k] is
    uniform24(word 0 of counter k) < float32(0.2), element for element (integer-exact: 24-bit uniforms, one float32 comparison)."""
    from test_gpu_train_ss import _op
    n, L, seed, stream = 4096, 16, 11, 4096 * 5 + 2
    x = torch.ones(1, 8, L, L, device="cuda")
    d = torch.full((n,), 9, dtype=torch.uint8, device="cuda")
    rc, _ = _op(x, [(0, k % L, k % L + 1) for k in range(n)], None, p=0.2, seed=seed, stream_id=stream, drop_out=d)
    assert rc == 0
    want = philox.train_uniforms(seed, stream, np.arange(n))[:, 0] < np.float32(0.2)
    assert np.array_equal(d.cpu().numpy(), want.astype(np.uint8)) and 0 < int(want.sum()) < n


def test_device_drawn_times_and_keep_masks_are_the_restatement():
    """train_tinyB (Dropout_0 at p = 0.1, f32): the first loss of a trainer with device-drawn t, z and keep-masks against the first
    loss of a fresh trainer of the same seed given the same draws explicitly -- t = eps + (1 - eps) u and the keep-masks u >= p from
    the restatement, z from t2p_op_philox_normal -- under the stream ids of train.h at loss_calls_ = 0 (Trainer::loss increments it
    after the pass): rng_t 0, rng_z 1, rng_dropout(k) 16 + k.  Bound: test_gpu_train.py's LOSS_TOL (a contracted FMA moves t by
    one ulp; a wrong counter moves the loss by order 1)."""
    from test_gpu_train import LOSS_TOL, _dropout_masks, _model_for
    case = TRAIN_CASES["train_tinyB"]
    cfg = case["config"]()
    inp = train_inputs(cfg, case)
    batch = {k: inp[k] for k in ("coords_6d", "mask_pair", "context", "mask_inpaint")}
    seed, p, eps = 11, np.float32(cfg.model.dropout), np.float32(1e-5)      # _model_for's trainer seed; HipTrainModel's t_eps
    drawn = _model_for(case, cfg)
    assert drawn._tc.seed == seed and p > 0
    loss_drawn = drawn.loss(batch)
    given = _model_for(case, cfg)
    u = philox.train_uniforms(seed, 0, np.arange(case["B"]))[:, 0]
    t = torch.from_numpy(u * (np.float32(1) - eps) + eps)
    z = torch.from_numpy(draw(seed, 1, inp["coords_6d"].numel())).reshape(inp["coords_6d"].shape)
    masks = []
    for k, like in enumerate(_dropout_masks(case, cfg, given)):            # its shapes: one NHWC mask per residual block
        n = like.numel()
        keep = philox.train_uniforms(seed, 16 + k, np.arange((n + 3) // 4)).reshape(-1)[:n] >= p
        masks.append(torch.from_numpy(keep.astype(np.uint8)).reshape(like.shape))
    given.set_dropout_masks(masks)
    loss_given = given.loss(batch, t=t, z=z)
    kept = sum(int(m.sum()) for m in masks) / sum(m.numel() for m in masks)
    print(f"loss with device draws {loss_drawn:.7f}, with the restatement's draws {loss_given:.7f}; t = {t.tolist()}, "
          f"{len(masks)} masks keep {kept:.4f}")
    assert len(masks) > 0 and abs(loss_drawn - loss_given) <= LOSS_TOL * abs(loss_given)
    assert abs(drawn.loss(batch) - loss_given) > 100 * LOSS_TOL * abs(loss_given)      # the second call draws under other streams
