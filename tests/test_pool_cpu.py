"""The device pool's host-only surface: its shard rule against dist.shard_range, its bindings, and argument checks that
need no device (the GPU behaviour is tests/test_gpu_pool.py)."""
import ctypes as C
import os
import re

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
POOL_CALLS = (
    "hipbfv_Pool_Create",
    "hipbfv_Pool_Destroy",
    "hipbfv_Pool_SetChunk",
    "hipbfv_Pool_Describe",
    "hipbfv_Pool_MultiplyRelin",
    "hipbfv_Pool_ProgramRun",
    "hipbfv_debug_pool_shard",
)


@pytest.mark.parametrize("members", [1, 2, 3, 4, 7, 8])
def test_shards_follow_dist_shard_range(members):
    from sunscreen_amd.dist import shard_range
    from sunscreen_amd.pool import shard

    for batch in [0, 1, 2, 3, 5, 7, 8, 9, 255, 256, 257, 1000, 1023, 4096, 65537]:
        spans = [shard(batch, members, r) for r in range(members)]
        assert spans == [shard_range(batch, r, members) for r in range(members)], (batch, members)
        assert spans[0][0] == 0 and spans[-1][1] == batch
        assert all(a[1] == b[0] for a, b in zip(spans, spans[1:]))  # contiguous, in member order
        sizes = [hi - lo for lo, hi in spans]
        assert max(sizes) - min(sizes) <= 1


def test_shard_rule_refuses_a_member_outside_the_pool():
    from sunscreen_amd import _lib

    lo, hi = C.c_uint64(), C.c_uint64()
    L = _lib.load()
    assert L.hipbfv_debug_pool_shard(10, 0, 0, C.byref(lo), C.byref(hi)) & 0xFFFFFFFF == _lib.E_INVALIDARG
    assert L.hipbfv_debug_pool_shard(10, 3, 3, C.byref(lo), C.byref(hi)) & 0xFFFFFFFF == _lib.E_INVALIDARG
    assert L.hipbfv_debug_pool_shard(10, 3, 0, None, C.byref(hi)) & 0xFFFFFFFF == _lib.E_POINTER


def test_pool_signatures_match_the_header():
    from sunscreen_amd import _lib

    header = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "hipbfv.h")).read(), flags=re.S)
    for name in POOL_CALLS:
        m = re.search(rf"^long\s+{name}\s*\((.*?)\);", header, flags=re.M | re.S)
        assert m, f"{name} is not declared in include/hipbfv.h"
        assert name in _lib._SIGNATURES, name
        assert len(_lib._SIGNATURES[name]) == len(m.group(1).split(",")), name
        assert hasattr(_lib.load(), name), f"{name} is not exported"
    assert _lib._SIGNATURES["hipbfv_Pool_ProgramRun"][2:4] == [_lib.u64, _lib.u64]  # batch, num_inputs
    assert _lib._SIGNATURES["hipbfv_Pool_MultiplyRelin"][-1] is _lib.u64


def test_pool_arguments_are_checked_without_a_device():
    from sunscreen_amd import _lib

    L = _lib.load()
    E_POINTER = _lib.E_POINTER
    h = C.c_void_p()
    devs = (C.c_int * 1)(0)
    assert L.hipbfv_Pool_Create(None, devs, 1, C.byref(h)) & 0xFFFFFFFF == E_POINTER
    assert h.value is None
    assert L.hipbfv_Pool_Destroy(None) & 0xFFFFFFFF == E_POINTER
    assert L.hipbfv_Pool_SetChunk(None, 0) & 0xFFFFFFFF == E_POINTER
    need = C.c_uint64()
    assert L.hipbfv_Pool_Describe(None, None, 0, C.byref(need)) & 0xFFFFFFFF == E_POINTER
    assert L.hipbfv_Pool_MultiplyRelin(None, None, None, None, None, 0) & 0xFFFFFFFF == E_POINTER
    kinds = (C.c_uint32 * 1)(0)
    assert L.hipbfv_Pool_ProgramRun(None, None, 0, 1, kinds, None, None, None, None, 0, None) & 0xFFFFFFFF == E_POINTER
    # a handle of another kind is not a pool
    prog = C.c_void_p()
    assert L.hipbfv_Program_Create(C.byref(prog)) == 0
    try:
        assert L.hipbfv_Pool_SetChunk(prog, 0) & 0xFFFFFFFF == E_POINTER
        assert L.hipbfv_Pool_Destroy(prog) & 0xFFFFFFFF == E_POINTER
    finally:
        assert L.hipbfv_Program_Destroy(prog) == 0


def test_device_pool_is_exported():
    import sunscreen_amd
    from sunscreen_amd.pool import DevicePool

    assert sunscreen_amd.DevicePool is DevicePool
    for name in ("multiply_relin", "run", "describe", "set_chunk"):
        assert callable(getattr(DevicePool, name))
