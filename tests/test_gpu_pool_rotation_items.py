"""Mixed-step rotation batches with one key set per client through the device pool (hipbfv_Pool_RotateRowsItemsKeys): the 13-item,
3-client batch of tests/test_gpu_rotation_items_keys.py over a pool of 2 members on device 0 in chunks of 2, word for word against
the one-device call -- itself held there to the single-item calls -- for pinned and pageable host memory, two client orders and a
key-cache bound that forces evictions; what a member copied is read from hipbfv_Pool_Describe."""
import re

import numpy as np
import pytest

from tests.test_gpu_rotation_items_keys import A, B, C, DIRECT_OF, E_INVALIDARG, H, N, _Foreign, _WORLDS, main_world

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module", autouse=True)
def _shared_worlds():
    yield
    _WORLDS.clear()


def _field(pool, name):
    return [int(x) for x in re.findall(rf"{name}=(\d+)", pool.describe())]


def _pool(w, chunk=2):
    from sunscreen_amd import DevicePool

    p = DevicePool(w.ctx, [0, 0])
    p.set_chunk(chunk)
    return p


def _naf(step):
    neg, v, parts, i = step < 0, abs(step), [], 0
    while v:
        z = 2 - (v & 3) if v & 1 else 0
        v = (v - z) >> 1
        if z:
            parts.append((-z if neg else z) * (1 << i))
        i += 1
    return parts


def _elt(step):
    return pow(3, step if step > 0 else H - abs(step), 2 * N)


def _reads(step, client):
    """The (client, element) key buffers one item reads: its direct key where the client holds it, else its chain's."""
    if step == 0:
        return set()
    pow2 = {_elt(s * (1 << i)) for i in range(H.bit_length() - 1) for s in (1, -1)}
    held = pow2 | {_elt(s) for s in DIRECT_OF[client]}
    if _elt(step) in held:
        return {(client, _elt(step))}
    return {(client, _elt(p)) for p in _naf(step) if abs(p) != H}


def _one_device(w, order):
    from sunscreen_amd.batch import to_host
    import torch

    idx = torch.from_numpy(order).cuda()
    out = w.ev.rotate_rows_items_keys(w.dev[idx].contiguous(), [w.steps[p] for p in order], w.sets, w.key_index[order])
    return to_host(out)


@pytest.mark.parametrize("order_kind", ["as given", "by client"])
def test_the_pool_gives_the_words_of_the_one_device_call(order_kind):
    """Members 0 and 1 get 7 and 6 items in chunks of 2 (a short last chunk each).  Sorted by client, member 0 sees A and B only and
    member 1 sees B and C only: neither may copy a key of the client it never meets, and each copies exactly the (client, element)
    buffers its own items read."""
    import torch
    from sunscreen_amd.batch import to_host

    w = main_world()
    count = len(w.steps)
    order = np.arange(count) if order_kind == "as given" else np.argsort(w.key_index, kind="stable")
    steps, key_index = [w.steps[p] for p in order], w.key_index[order]
    ct = np.ascontiguousarray(to_host(w.dev)[order])
    ref = _one_device(w, order)
    pool = _pool(w)
    try:
        out = pool.rotate_rows_items_keys(ct, steps, w.sets, key_index)
        assert (out == ref).all(), np.nonzero((out != ref).any(axis=(1, 2, 3)))[0]
        want = []
        for lo, hi in ((0, 7), (7, 13)):
            reads = set().union(*[_reads(steps[i], int(key_index[i])) for i in range(lo, hi)])
            want.append(len(reads))
            if order_kind == "by client":
                assert {k for k, _ in reads} == ({A, B} if lo == 0 else {B, C})
        assert _field(pool, "key_copies") == want, pool.describe()
        # pinned memory, and in place
        pinned_in = torch.from_numpy(ct.view(np.int64)).pin_memory()
        pinned_out = torch.empty_like(pinned_in).pin_memory()
        pool.rotate_rows_items_keys(pinned_in, steps, w.sets, key_index, out=pinned_out)
        assert (pinned_out.numpy().view(np.uint64) == ref).all()
        inplace = ct.copy()
        pool.rotate_rows_items_keys(inplace, steps, w.sets, key_index, out=inplace)
        assert (inplace == ref).all()
        assert _field(pool, "key_copies") == want, "a second call copied keys again"
        # a bound of four key buffers: a chunk of two items reads at most four, a member's shard reads more
        key_bytes = _field(pool, "key_bytes")
        per_key = key_bytes[0] // want[0]
        assert all(b == per_key * c for b, c in zip(key_bytes, want)) and min(want) > 4
        pool.set_key_cache_bytes(4 * per_key)
        bounded = pool.rotate_rows_items_keys(ct, steps, w.sets, key_index)
        assert (bounded == ref).all()
        assert all(e > 0 for e in _field(pool, "key_evictions")) and all(b <= 4 * per_key for b in _field(pool, "key_bytes")), pool.describe()
    finally:
        pool.close()


def test_one_chunk_per_member_and_unreferenced_sets():
    """The library's default chunk (the whole shard in one chunk) and a handle array with NULL and foreign entries that only
    copied items name."""
    from sunscreen_amd.batch import to_host

    w = main_world()
    ct = to_host(w.dev)
    ref = _one_device(w, np.arange(len(w.steps)))
    sets = [w.sets[A], None, _Foreign(), w.sets[B], w.sets[C]]
    key_index = np.array([{A: 0, B: 3, C: 4}[int(k)] for k in w.key_index], dtype=np.uint32)
    zeros = [i for i, s in enumerate(w.steps) if s == 0]
    key_index[zeros[0]], key_index[zeros[1]] = 1, 2
    pool = _pool(w, chunk=0)
    try:
        assert (pool.rotate_rows_items_keys(ct, w.steps, sets, key_index) == ref).all()
    finally:
        pool.close()


@pytest.mark.parametrize("case", ["step", "key_index", "null set", "chain key missing"])
def test_refusals_copy_nothing_and_write_nothing(case):
    from sunscreen_amd import HipBfvError
    from sunscreen_amd.batch import to_host
    from sunscreen_amd.seal import KeyGenerator

    w = main_world()
    ct = to_host(w.dev)
    steps, sets, key_index = list(w.steps), list(w.sets), w.key_index.copy()
    if case == "step":
        item, k = 12, A  # in the second member's shard: decided over the whole batch all the same
        steps[item] = -H
    elif case == "key_index":
        item, k = 11, 5
        key_index[item] = 5
    elif case == "null set":
        item, k = 3, C
        sets[C] = None
    else:
        item, k = 1, B
        sets[B] = KeyGenerator(w.ctx, seed=6).create_galois_keys(steps=[1, -1, 2, -2])
    out = np.full_like(ct, 0xA5A5A5A5A5A5A5A5)
    pool = _pool(w)
    try:
        with pytest.raises(HipBfvError) as e:
            pool.rotate_rows_items_keys(ct, steps, sets, key_index, out=out)
        assert e.value.hresult & 0xFFFFFFFF == E_INVALIDARG and f"item {item}: key set {k}: " in str(e.value), str(e.value)
        assert (out == 0xA5A5A5A5A5A5A5A5).all()
        assert _field(pool, "key_copies") == [0, 0] and _field(pool, "keys_cached") == [0, 0], pool.describe()
        # the pool stays usable
        assert (pool.rotate_rows_items_keys(ct, w.steps, w.sets, w.key_index) == _one_device(w, np.arange(len(w.steps)))).all()
    finally:
        pool.close()
