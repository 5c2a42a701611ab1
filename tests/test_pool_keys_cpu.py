"""The host-only surface of the device pool's per-client key calls (hipbfv_Pool_*Keys, hipbfv_Pool_SetKeyCacheBytes): exports
and signatures, argument checks that need no device, and the per-chunk key table (hipbfv_debug_pool_keyplan) against a
Python model.  The GPU behaviour is tests/test_gpu_pool_keys.py."""
import ctypes as C
import os
import re

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
KEY_CALLS = (
    "hipbfv_Pool_MultiplyRelinKeys",
    "hipbfv_Pool_RotateRowsKeys",
    "hipbfv_Pool_RotateColumnsKeys",
    "hipbfv_Pool_ProgramRunKeys",
    "hipbfv_Pool_SetKeyCacheBytes",
    "hipbfv_debug_pool_keyplan",
)
U32P = C.POINTER(C.c_uint32)


def _hr(x):
    return x & 0xFFFFFFFF


def test_key_calls_are_exported_and_match_the_header():
    from sunscreen_amd import _lib

    header = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "hipbfv.h")).read(), flags=re.S)
    for name in KEY_CALLS:
        m = re.search(rf"^long\s+{name}\s*\((.*?)\);", header, flags=re.M | re.S)
        assert m, f"{name} is not declared in include/hipbfv.h"
        assert name in _lib._SIGNATURES, name
        assert len(_lib._SIGNATURES[name]) == len(m.group(1).split(",")), name
        assert hasattr(_lib.load(), name), f"{name} is not exported"
    # the argument order of the single-device _keys forms, minus evaluator (kept: the pool) and stream (dropped)
    for pool_name, single in (
        ("hipbfv_Pool_MultiplyRelinKeys", "hipbfv_batch_multiply_relin_keys"),
        ("hipbfv_Pool_RotateRowsKeys", "hipbfv_batch_rotate_rows_keys"),
        ("hipbfv_Pool_RotateColumnsKeys", "hipbfv_batch_rotate_columns_keys"),
        ("hipbfv_Pool_ProgramRunKeys", "hipbfv_Program_RunKeys"),
    ):
        want = list(_lib._SIGNATURES[single][:-1])
        if single == "hipbfv_Program_RunKeys":
            del want[1]  # (program, evaluator, ...) -> (pool, program, ...)
            want.insert(0, _lib.vp)
        assert _lib._SIGNATURES[pool_name] == want, pool_name
    assert _lib._SIGNATURES["hipbfv_Pool_SetKeyCacheBytes"] == [_lib.vp, _lib.u64]


def test_python_surface():
    from sunscreen_amd import pool
    from sunscreen_amd.pool import DevicePool

    for name in ("multiply_relin_keys", "rotate_rows_keys", "rotate_columns_keys", "rotate_rows", "rotate_columns", "set_key_cache_bytes", "run"):
        assert callable(getattr(DevicePool, name)), name
    assert callable(pool.keyplan)


def test_arguments_are_checked_without_a_device():
    from sunscreen_amd import _lib

    L = _lib.load()
    E_POINTER = _lib.E_POINTER
    sets = (C.c_void_p * 1)(None)
    idx = (C.c_uint32 * 1)(0)
    buf = (C.c_uint64 * 4)()
    kinds = (C.c_uint32 * 1)(0)
    ptrs = (C.c_void_p * 1)(C.addressof(buf))
    strides = (C.c_uint64 * 1)(0)
    # no pool
    assert _hr(L.hipbfv_Pool_MultiplyRelinKeys(None, buf, buf, sets, 1, idx, buf, 1)) == E_POINTER
    assert _hr(L.hipbfv_Pool_RotateRowsKeys(None, buf, 1, sets, 1, idx, buf, 1)) == E_POINTER
    assert _hr(L.hipbfv_Pool_RotateColumnsKeys(None, buf, sets, 1, idx, buf, 1)) == E_POINTER
    assert _hr(L.hipbfv_Pool_ProgramRunKeys(None, None, 1, 1, kinds, ptrs, strides, 1, sets, sets, idx, 1, ptrs)) == E_POINTER
    assert _hr(L.hipbfv_Pool_SetKeyCacheBytes(None, 0)) == E_POINTER
    # a handle of another kind is not a pool
    prog = C.c_void_p()
    assert L.hipbfv_Program_Create(C.byref(prog)) == 0
    try:
        assert _hr(L.hipbfv_Pool_SetKeyCacheBytes(prog, 1 << 20)) == E_POINTER
        assert _hr(L.hipbfv_Pool_MultiplyRelinKeys(prog, buf, buf, sets, 1, idx, buf, 1)) == E_POINTER
        assert _hr(L.hipbfv_Pool_RotateRowsKeys(prog, buf, 1, sets, 1, idx, buf, 1)) == E_POINTER
        assert _hr(L.hipbfv_Pool_RotateColumnsKeys(prog, buf, sets, 1, idx, buf, 1)) == E_POINTER
        assert _hr(L.hipbfv_Pool_ProgramRunKeys(prog, prog, 1, 1, kinds, ptrs, strides, 1, sets, sets, idx, 1, ptrs)) == E_POINTER
        # the per-key run needs key_index and at least one key set, whatever the pool
        assert _hr(L.hipbfv_Pool_ProgramRunKeys(prog, prog, 1, 1, kinds, ptrs, strides, 1, sets, sets, None, 1, ptrs)) == E_POINTER
        assert _hr(L.hipbfv_Pool_ProgramRunKeys(prog, prog, 1, 1, kinds, ptrs, strides, 0, sets, sets, idx, 1, ptrs)) == E_POINTER
    finally:
        assert L.hipbfv_Program_Destroy(prog) == 0
    # the diagnostic's required pointers
    local, remapped = (C.c_uint32 * 4)(), (C.c_uint32 * 4)()
    nl, nc = C.c_uint64(), C.c_uint64()
    assert _hr(L.hipbfv_debug_pool_keyplan(None, 1, 1, 1, 0, 1, 0, local, C.byref(nl), remapped, C.byref(nc))) == E_POINTER
    assert _hr(L.hipbfv_debug_pool_keyplan(idx, 1, 1, 1, 0, 1, 0, None, C.byref(nl), remapped, C.byref(nc))) == E_POINTER
    assert _hr(L.hipbfv_debug_pool_keyplan(idx, 1, 1, 1, 0, 1, 0, local, None, remapped, C.byref(nc))) == E_POINTER
    assert _hr(L.hipbfv_debug_pool_keyplan(idx, 1, 1, 1, 0, 1, 0, local, C.byref(nl), None, C.byref(nc))) == E_POINTER
    assert _hr(L.hipbfv_debug_pool_keyplan(idx, 1, 1, 1, 0, 1, 0, local, C.byref(nl), remapped, None)) == E_POINTER


def _model(key_index, members, member, chunk, chunk_no):
    """The chunk's distinct sets in ascending order of the caller's index, and its key_index remapped onto them."""
    from sunscreen_amd.dist import shard_range

    lo, hi = shard_range(len(key_index), member, members)
    sets = min(chunk, hi - lo)  # a chunk is never larger than the shard
    first = lo + chunk_no * sets
    part = [int(k) for k in key_index[first : min(first + sets, hi)]]
    local = sorted(set(part))
    where = {k: i for i, k in enumerate(local)}
    return local, [where[k] for k in part], (hi - lo + sets - 1) // sets if sets else 0


def _key_indices(batch, nsets, rng):
    yield "sorted", np.sort(rng.integers(0, nsets, batch))
    yield "shuffled", rng.integers(0, nsets, batch)
    yield "constant", np.full(batch, nsets - 1)


@pytest.mark.parametrize("members", [1, 2, 3, 8])
@pytest.mark.parametrize("chunk", [1, 7, 256])
def test_keyplan_follows_the_model(members, chunk):
    from sunscreen_amd.pool import keyplan

    rng = np.random.default_rng(members * 1000 + chunk)
    for batch in (24, 25, 1000, 1023):  # with and without remainders for 1, 2, 3 and 8 members
        cases = list(_key_indices(batch, 9, rng)) + [("one set per item", rng.permutation(batch))]
        for label, key_index in cases:
            nsets = int(key_index.max()) + 1
            for member in range(members):
                nch = _model(key_index, members, member, chunk, 0)[2]
                picks = sorted({0, nch // 2, nch - 1}) if chunk == 1 else range(nch)  # chunk 1: the ends and the middle
                for j in picks:
                    want_local, want_map, _ = _model(key_index, members, member, chunk, j)
                    local, remapped = keyplan(key_index, nsets, members, member, chunk, j)
                    assert local == want_local, (label, batch, member, j)
                    assert remapped == want_map, (label, batch, member, j)
                    assert [local[r] for r in remapped] == [int(k) for k in key_index[_first(batch, members, member, chunk, j) :][: len(remapped)]]


def _first(batch, members, member, chunk, chunk_no):
    from sunscreen_amd.dist import shard_range

    lo, hi = shard_range(batch, member, members)
    return lo + chunk_no * min(chunk, hi - lo)


def test_keyplan_refuses_what_is_out_of_range():
    from sunscreen_amd import _lib

    L = _lib.load()
    idx = (C.c_uint32 * 10)(*([0, 1, 2, 3, 4] * 2))
    local, remapped = (C.c_uint32 * 8)(), (C.c_uint32 * 16)()
    nl, nc = C.c_uint64(), C.c_uint64()

    def plan(batch, nsets, members, member, chunk, chunk_no):
        return _hr(L.hipbfv_debug_pool_keyplan(idx, batch, nsets, members, member, chunk, chunk_no, local, C.byref(nl), remapped, C.byref(nc)))

    assert plan(10, 5, 3, 0, 2, 0) == 0 and (nl.value, nc.value) == (2, 2)
    assert plan(10, 5, 3, 3, 2, 0) == _lib.E_INVALIDARG  # member outside the pool
    assert plan(10, 5, 0, 0, 2, 0) == _lib.E_INVALIDARG  # no members
    assert plan(10, 5, 3, 0, 2, 2) == _lib.E_INVALIDARG  # member 0 holds 4 input sets: chunks 0 and 1
    assert plan(10, 5, 3, 0, 2, 1) == 0
    assert plan(10, 5, 3, 0, 0, 0) == _lib.E_INVALIDARG  # an empty chunk
    assert plan(10, 4, 3, 0, 2, 0) == _lib.E_INVALIDARG  # key_index names set 4 of 4
    assert plan(2, 5, 3, 2, 2, 0) == _lib.E_INVALIDARG  # an empty shard has no chunk
