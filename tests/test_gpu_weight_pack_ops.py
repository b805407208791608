"""The weight-packing kernels (csrc/weightpack.hip) one kind at a time through ``t2p_op_weight_pack``, against the numpy restatement of
their formulas (tests/weightpack_cases.py): equal bits in f32, f16 and bf16, at sizes that are no multiple of a tile or of the vector
width, with a guard band behind every destination and the gaps of pitched rows left as they were."""
import ctypes as C

import numpy as np
import pytest
import torch

import weightpack_cases as wp

pytestmark = pytest.mark.gpu

GUARD = 64
_CASES = wp.cases()


@pytest.fixture(scope="module")
def lib():
    from text2protein_amd import _lib
    return _lib.load()


def _run(lib, kind, srcs, dims, expect, dtype):
    from text2protein_amd._lib import check, ptr, stream_ptr
    dev = torch.device("cuda:0")
    tdt = {"f32": torch.float32, "f16": torch.float16, "bf16": torch.bfloat16}[dtype]
    n = expect.size
    dst = torch.full((n + GUARD,), float(wp.FILL), device=dev, dtype=tdt)
    d_src = [torch.from_numpy(np.ascontiguousarray(s)).to(dev) for s in srcs] + [None] * (3 - len(srcs))
    arr = (C.c_int64 * len(dims))(*dims)
    check(lib.t2p_op_weight_pack(kind, ptr(d_src[0]), ptr(d_src[1]), ptr(d_src[2]), ptr(dst), arr, len(dims), wp.DTYPES[dtype], stream_ptr()))
    torch.cuda.synchronize()
    got = dst.cpu()
    bits = got.view(torch.int32 if dtype == "f32" else torch.int16).numpy().view(np.uint32 if dtype == "f32" else np.uint16)
    return bits[:n], bits[n:]


@pytest.mark.parametrize("dtype", ["f32", "f16", "bf16"])
@pytest.mark.parametrize("name", sorted(_CASES))
def test_weight_pack_bits(lib, name, dtype):
    kind, srcs, dims, expect = _CASES[name]
    want = wp.to_dtype(expect.reshape(-1), dtype)
    got, guard = _run(lib, kind, srcs, dims, expect, dtype)
    fill = wp.to_dtype(np.full(1, wp.FILL, np.float32), dtype)[0]
    assert np.all(guard == fill), f"{name} {dtype}: wrote past the destination"
    bad = np.nonzero(got != want)[0]
    assert bad.size == 0, f"{name} {dtype}: {bad.size} of {want.size} elements differ, first at {bad[:5]}"


def test_weight_pack_refuses_bad_arguments(lib):
    from text2protein_amd._lib import ptr, stream_ptr
    x = torch.zeros(64, device="cuda:0")
    for kind, dims in ((99, [4]), (wp.COPY, [0]), (wp.ROWS, [4, 8, 7]), (wp.CONV3, [4, 5, 4, 0]), (wp.NIN, [4, 4, 3]), (wp.PRODUCT, [4, 4, 4, 2, 0])):
        arr = (C.c_int64 * len(dims))(*dims)
        assert lib.t2p_op_weight_pack(kind, ptr(x), ptr(x), ptr(x), ptr(x), arr, len(dims), 0, stream_ptr()) != 0, (kind, dims)
    arr = (C.c_int64 * 1)(4)
    assert lib.t2p_op_weight_pack(wp.COPY, None, None, None, ptr(x), arr, 1, 0, stream_ptr()) != 0
    assert lib.t2p_op_weight_pack(wp.COPY, ptr(x), None, None, ptr(x), arr, 1, 7, stream_ptr()) != 0
