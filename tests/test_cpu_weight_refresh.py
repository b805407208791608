"""The surface of the on-device weight refresh that needs no GPU: the new names and their signatures, and the numpy restatement of
the packings (tests/weightpack_cases.py, the yardstick of test_gpu_weight_pack_ops) against torch re-layouts of the reference's
tensor shapes."""
import ctypes as C
import inspect
import os
import re

import numpy as np
import torch

import weightpack_cases as wp

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_new_entry_points_and_signatures():
    from text2protein_amd import _lib
    i, i64, vp = C.c_int, C.c_int64, C.c_void_p
    want = {
        "t2p_engine_load_flat": (i, [vp, vp, i64, vp]),
        "t2p_train_buffer": (i, [vp, i, C.POINTER(vp), C.POINTER(i64)]),
        "t2p_engine_load_from_trainer": (i, [vp, vp, i, vp]),
        "t2p_train_copy": (i, [vp, i, i, vp]),
        "t2p_op_weight_pack": (i, [i, vp, vp, vp, vp, C.POINTER(i64), i, i, vp]),
    }
    lib = _lib.load()
    for name, (res, args) in want.items():
        assert name in _lib.SIGNATURES, name
        assert _lib.SIGNATURES[name][0] is res and list(_lib.SIGNATURES[name][1]) == args, name
        assert hasattr(lib, name), name
    assert "t2p_train_grad_buffer" in _lib.SIGNATURES          # stays
    hdr = open(os.path.join(ROOT, "include", "t2p.h")).read()
    hdr = re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)
    for decl in ("int t2p_engine_load_flat(t2p_engine* e, const float* device_flat, int64_t n, void* stream);",
                 "int t2p_train_buffer(t2p_trainer* t, int which, float** device_ptr, int64_t* n);",
                 "int t2p_engine_load_from_trainer(t2p_engine* e, t2p_trainer* t, int which, void* stream);",
                 "int t2p_train_copy(t2p_trainer* t, int dst, int src, void* stream);"):
        assert decl in hdr, decl


def test_python_surface():
    from text2protein_amd import ddim, losses, model, sampling
    assert list(inspect.signature(model.HipScoreModel.load_from).parameters) == ["self", "train_model", "which"]
    assert inspect.signature(model.HipScoreModel.load_from).parameters["which"].default == "ema"
    assert inspect.signature(losses.HipTrainModel.sampling_model).parameters["dtype"].default == "f16"
    for verb in ("store", "copy_to", "restore"):
        assert list(inspect.signature(getattr(losses.ExponentialMovingAverage, verb)).parameters) == ["self", "parameters"]
    assert inspect.signature(ddim.DiffusionSampler.ddim_sample).parameters["train_dtype"].default == "f16"
    src = inspect.getsource(sampling.get_pc_sampler)
    assert 'train_dtype="f16"' in src


def test_ema_verbs_refuse_foreign_parameters():
    """The verbs take model.parameters() of the model the EMA views; anything else is refused before the library is reached."""
    from text2protein_amd import losses

    class _Model:
        pass

    ema = losses.ExponentialMovingAverage.__new__(losses.ExponentialMovingAverage)
    ema.model = _Model()
    for verb in (ema.store, ema.copy_to, ema.restore):
        for bad in ([torch.zeros(2)], losses._ParamHandle(_Model()), None):
            try:
                verb(bad)
            except TypeError:
                continue
            raise AssertionError(f"{verb.__name__} accepted {bad!r}")


def test_restatement_matches_torch_relayouts():
    w = wp.values(31, 6, 5, 3, 3)
    t = torch.from_numpy(w)
    # 3x3 convolution (N, Ci, 3, 3) -> [N][tap][Cin_pad]
    assert np.array_equal(wp.pack_conv3(w), t.permute(0, 2, 3, 1).reshape(6, 45).numpy())
    padded = torch.zeros(6, 3, 3, 8)
    padded[..., :5] = t.permute(0, 2, 3, 1)
    assert np.array_equal(wp.pack_conv3(w, 8), padded.reshape(6, 72).numpy())
    assert np.array_equal(wp.pack_conv3_t(w), t.permute(2, 3, 1, 0).reshape(9, 5, 6).numpy())
    # NIN (K, N) -> [N][K], stacked
    a, b = wp.values(32, 7, 9), wp.values(33, 7, 9)
    assert np.array_equal(wp.pack_nin(a), torch.from_numpy(a).t().contiguous().numpy())
    assert np.array_equal(wp.pack_nin(a, b), torch.cat([torch.from_numpy(a).t(), torch.from_numpy(b).t()]).numpy())
    # stacks and the fused shortcut
    q, k, v = (wp.values(s, 4, 6) for s in (34, 35, 36))
    assert np.array_equal(wp.pack_copy(q, k, v).reshape(12, 6), torch.cat([torch.from_numpy(x) for x in (q, k, v)]).numpy())
    w1, w2 = wp.values(37, 4, 4, 3, 3), wp.values(38, 4, 6)
    fused = np.concatenate([wp.pack_conv3(w1), w2], axis=1)
    blk = wp.pack_conv3(w1, 4, 36 + 6, wp.FILL)
    blk[:, 36:] = wp.pack_rows(w2, 6, wp.FILL)
    assert np.array_equal(blk, fused)
    # GEGLU: rows interleaved (value_j, gate_j), written with indexing
    g = wp.values(39, 16, 3)
    tg = torch.from_numpy(g)
    inter = torch.empty_like(tg)
    inter[0::2], inter[1::2] = tg[:8], tg[8:]
    assert np.array_equal(wp.pack_geglu(g), inter.numpy())
    # the four-phase form of an up block's conv0 reproduces the 3x3 convolution of the up-sampled map
    up = wp.values(40, 3, 2, 3, 3).astype(np.float64)
    x = torch.from_numpy(wp.values(41, 1, 2, 4, 4).astype(np.float64))
    full = torch.nn.functional.conv2d(torch.nn.functional.interpolate(x, scale_factor=2, mode="nearest"), torch.from_numpy(up), padding=1)
    w4 = torch.from_numpy(wp.pack_up4(up.astype(np.float32)).astype(np.float64))          # [ph][co][ty * 2 + tx][ci]
    xp = torch.nn.functional.pad(x, (1, 1, 1, 1))
    for py in range(2):
        for px in range(2):
            k2 = w4[py * 2 + px].reshape(3, 2, 2, 2).permute(0, 3, 1, 2)                   # (co, ci, ty, tx)
            y = torch.nn.functional.conv2d(xp[:, :, py:py + 5, px:px + 5], k2)
            assert torch.allclose(y, full[:, :, py::2, px::2], atol=1e-6), (py, px)
    # products: the ordered float32 sum stays within the forward error bound of the float64 product
    A, B = wp.values(42, 5, 40), wp.values(43, 40, 7)
    ref = A.astype(np.float64) @ B.astype(np.float64)
    bound = 40 * 2.0 ** -24 * (np.abs(A).astype(np.float64) @ np.abs(B).astype(np.float64))
    assert np.all(np.abs(wp.pack_product(A, B) - ref) <= bound)
    assert np.array_equal(wp.pack_product(A, B, transposed=True), wp.pack_product(A, B).T)
    W, v, b0 = wp.values(44, 5, 40), wp.values(45, 40), wp.values(46, 5)
    terms = np.concatenate([b0.astype(np.float64)[:, None], W.astype(np.float64) * v.astype(np.float64)], axis=1)
    assert np.array_equal(wp.pack_dot64(W, v, b0), np.cumsum(terms, axis=1)[:, -1].astype(np.float32))     # cumsum adds left to right


def test_to_dtype_rounds_to_nearest_even():
    x = np.array([1.0 + 2.0 ** -11, 1.0 + 3 * 2.0 ** -11, 1.0 + 2.0 ** -8, 1.0 + 3 * 2.0 ** -8, 1e-6], np.float32)
    assert list(wp.to_dtype(x, "f16")[:2]) == [0x3C00, 0x3C02]           # ties go to the even mantissa
    assert list(wp.to_dtype(x, "bf16")[2:4]) == [0x3F80, 0x3F82]
    assert wp.to_dtype(x, "f16")[4] == 0x0011                              # 1e-6 is a subnormal half: 16.78 units of 2^-24
