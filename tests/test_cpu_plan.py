"""The plan switches of libt2p_hip.so (csrc/plan.h, the key table next to t2p_debug_set): defaults, set / get round trips, the
per-key rules and the names.  Host state only: no HIP call is made."""
import ctypes as C

import pytest

from text2protein_amd import _lib

BOOLS = [0, 3, 4, 5, 6, 7, 9, 12, 13, 14, 15, 17, 20, 21, 22, 23, 25, 26, 27, 28, 29, 32, 33, 34, 36, 38, 39, 40, 41, 42, 45, 46, 47, 48]
DEFAULTS = {k: 1 for k in BOOLS}
DEFAULTS.update({12: 0, 48: 0})
DEFAULTS.update({1: 0, 2: 0, 8: 2, 10: 0, 11: 0, 30: 192, 31: 256, 43: 4096, 49: 1})
# a legal value other than the default for every int key (bools: the other state)
OTHER = {1: 128, 2: 3, 8: 1, 10: 64, 11: 2, 30: 100, 31: 300, 43: 8192, 49: 2}
OTHER.update({k: 1 - DEFAULTS[k] for k in BOOLS})
UNKNOWN = [16, 18, 19, 24, 35, 37, 44, -1, 50, 1000]
OK, INVALID = 0, 1


@pytest.fixture()
def lib():
    lib = _lib.load()
    try:
        yield lib
    finally:
        for k, v in DEFAULTS.items():
            assert lib.t2p_debug_set(k, v) == OK, k


def get(lib, key):
    v = C.c_int(-12345)
    assert lib.t2p_debug_get(key, C.byref(v)) == OK, key
    return v.value


def test_table_covers_the_43_keys():
    assert len(DEFAULTS) == 43 and set(OTHER) == set(DEFAULTS)


def test_defaults(lib):
    assert {k: get(lib, k) for k in DEFAULTS} == DEFAULTS


def test_set_get_round_trip_for_every_key(lib):
    for k, d in DEFAULTS.items():
        assert OTHER[k] != d
        assert lib.t2p_debug_set(k, OTHER[k]) == OK, k
        assert get(lib, k) == OTHER[k], k
        assert lib.t2p_debug_set(k, d) == OK, k
        assert get(lib, k) == d, k
    assert {k: get(lib, k) for k in DEFAULTS} == DEFAULTS      # no key wrote into another one's state


def test_bools_store_value_not_equal_zero(lib):
    for k in BOOLS:
        assert lib.t2p_debug_set(k, 0) == OK and get(lib, k) == 0, k
        assert lib.t2p_debug_set(k, 7) == OK and get(lib, k) == 1, k
        assert lib.t2p_debug_set(k, 0) == OK and lib.t2p_debug_set(k, -1) == OK and get(lib, k) == 1, k


def test_plain_ints_are_stored_as_given(lib):
    for k in (2, 8, 11, 43, 10):
        for v in (5, -3, 0):
            assert lib.t2p_debug_set(k, v) == OK and get(lib, k) == v, (k, v)


def test_split_constants_ignore_values_that_are_not_positive(lib):
    for k in (30, 31):
        for v in (0, -5):
            assert lib.t2p_debug_set(k, v) == OK, (k, v)
            assert get(lib, k) == DEFAULTS[k], (k, v)
        assert lib.t2p_debug_set(k, 1) == OK and get(lib, k) == 1
        assert lib.t2p_debug_set(k, 0) == OK and get(lib, k) == 1


def test_rowres_takes_0_to_2_only(lib):
    for v in (0, 1, 2):
        assert lib.t2p_debug_set(49, v) == OK and get(lib, 49) == v
    for v in (-1, 3):
        assert lib.t2p_debug_set(49, v) == INVALID, v
        assert get(lib, 49) == 2, v
        assert lib.t2p_last_error(), v


def test_ablation_mask(lib):
    assert lib.t2p_debug_set(1, 12672) == OK and get(lib, 1) == 12672 == 128 | 256 | 4096 | 8192
    if lib.t2p_built_with_ablation() == 0:
        for v in (1, 12672 | 2, -1):
            assert lib.t2p_debug_set(1, v) == INVALID, v
            assert get(lib, 1) == 12672, v
            assert lib.t2p_last_error(), v
    else:
        assert lib.t2p_debug_set(1, 1) == OK and get(lib, 1) == 1


def test_unknown_keys_are_refused(lib):
    v = C.c_int(-12345)
    for k in UNKNOWN:
        assert lib.t2p_debug_set(k, 1) == INVALID, k
        assert lib.t2p_debug_get(k, C.byref(v)) == INVALID and v.value == -12345, k
        assert lib.t2p_debug_key_name(k) is None, k
    assert lib.t2p_debug_get(0, None) == INVALID
    assert {k: get(lib, k) for k in DEFAULTS} == DEFAULTS


def test_names_are_unique_and_non_empty(lib):
    names = {k: lib.t2p_debug_key_name(k) for k in DEFAULTS}
    assert all(names.values()), names
    assert len(set(names.values())) == len(names), names
    assert all(n.decode().islower() and n.decode().replace("_", "").isalnum() for n in names.values()), names
    assert names[12] == b"midsplit" and names[48] == b"train_plumbing16"
    assert {k for k in range(-8, 1100) if lib.t2p_debug_key_name(k) is not None} == set(DEFAULTS)


def test_set_plan_switches_takes_names_and_numbers(lib):
    name = lib.t2p_debug_key_name(39).decode()
    _lib.set_plan_switches(f"{name}=0")
    assert get(lib, 39) == 0
    assert lib.t2p_debug_set(39, 1) == OK
    _lib.set_plan_switches("39=0")
    assert get(lib, 39) == 0
    _lib.set_plan_switches(f"{name}=1,8=1,{lib.t2p_debug_key_name(49).decode()}=2")
    assert (get(lib, 39), get(lib, 8), get(lib, 49)) == (1, 1, 2)
    with pytest.raises(_lib.T2PError):
        _lib.set_plan_switches("no_such_switch=1")
    with pytest.raises(_lib.T2PError):
        _lib.set_plan_switches("49=3")
    with pytest.raises(_lib.T2PError):
        _lib.set_plan_switches("44=1")
