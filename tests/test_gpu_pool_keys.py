"""Per-client key sets through the device pool (hipbfv_Pool_MultiplyRelinKeys / RotateRowsKeys / RotateColumnsKeys /
ProgramRunKeys / SetKeyCacheBytes): every result word for word against the single-device per-key calls on the whole batch
and, for a subset, against the CPU oracle run with that input set's own client's keys -- never against the pool itself.
One GPU: the members [0, 0, 0] share it."""
import ctypes as C
import functools
import re

import numpy as np
import pytest

from oracle import bfv_oracle as O
from tests.bfv_helpers import oracle_for, params
from tests.oracle_program import run_program

pytestmark = pytest.mark.gpu

E_INVALIDARG = 0x80070057
E_OUTOFMEMORY = 0x8007000E
COR_E_INVALIDOPERATION = 0x80131509


def _random_cts(name, count, seed):
    """Ciphertext-shaped residues, uniform below each data prime (bit-exactness needs no valid encryption)."""
    n, primes, _ = params(name)
    K = len(primes) - 1
    rng = np.random.default_rng(seed)
    out = np.empty((count, 2, K, n), dtype=np.uint64)
    for k in range(K):
        out[:, :, k, :] = rng.integers(0, primes[k], (count, 2, n), dtype=np.uint64)
    return out


@functools.lru_cache(maxsize=None)
def _context(name):
    from sunscreen_amd import Context
    from sunscreen_amd.batch import BatchEvaluator

    n, primes, t = params(name)
    ctx = Context.from_raw(n, primes, t)
    return oracle_for(name), ctx, BatchEvaluator(ctx)


@functools.lru_cache(maxsize=None)
def _relin_clients(name, nclients, seed=400):
    from sunscreen_amd import RelinearizationKeys

    o, ctx, ev = _context(name)
    out = []
    for k in range(nclients):
        O.seed(seed + k)
        sk, pk, rk, _ = o.keygen()
        out.append({"sk": sk, "pk": pk, "rk": rk, "rkd": RelinearizationKeys.from_array(ctx, rk)})
    return out


DIRECT_STEPS = (3, -5)  # the D clients hold these rotations' own keys; the P clients reach them over the NAF chain
POW2_STEPS = (1, -1, 4, -4)  # 3 = 4 - 1, -5 = -4 - 1


@functools.lru_cache(maxsize=None)
def _galois_clients(name, nclients, seed=500):
    """Client k even: D (the power-of-two keys, the column key and the direct keys of 3 and -5); odd: P (no direct keys)."""
    from sunscreen_amd import GaloisKeys

    o, ctx, ev = _context(name)
    pow2 = [o.galois_elt_from_step(s) for s in POW2_STEPS] + [2 * o.n - 1]
    direct = [o.galois_elt_from_step(s) for s in DIRECT_STEPS]
    out = []
    for k in range(nclients):
        O.seed(seed + k)
        sk, pk, _, gk = o.keygen(relin=False, galois_elts=pow2 + (direct if k % 2 == 0 else []))
        out.append({"sk": sk, "pk": pk, "gk": gk, "gkd": GaloisKeys.from_arrays(ctx, gk), "direct": k % 2 == 0})
    return out


def _pool(ctx, members, chunk=0):
    from sunscreen_amd import DevicePool

    p = DevicePool(ctx, members)
    p.set_chunk(chunk)
    return p


def _field(pool, name):
    return [int(x) for x in re.findall(rf"{name}=(\d+)", pool.describe())]


def _hr(e):
    return e.value.hresult & 0xFFFFFFFF


def _shuffled_index(nclients, batch, seed):
    rng = np.random.default_rng(seed)
    key_index = rng.integers(0, nclients, batch).astype(np.uint32)
    key_index[:nclients] = rng.permutation(nclients)  # every client appears
    return key_index


def _spread(key_index, count):
    """`count` input sets spread over the batch that cover every client."""
    batch = len(key_index)
    picks = set(np.linspace(0, batch - 1, count).astype(int).tolist())
    for k in set(int(x) for x in key_index):
        picks.add(int(np.nonzero(key_index == k)[0][0]))
    return sorted(picks)


class _Foreign:
    """A live handle that is no key object."""

    def __init__(self):
        from sunscreen_amd.program import FheProgram

        self._p = FheProgram()

    def get_handle(self):
        return self._p._h


# ---- 4: multiply + relinearize ----
@pytest.mark.parametrize("name,batch", [("default_8192_17", 200), ("default_16384_17", 100)])
def test_multiply_relin_keys_matches_the_batched_call_and_the_oracle(name, batch):
    from sunscreen_amd.batch import to_device, to_host

    o, ctx, ev = _context(name)
    clients = _relin_clients(name, 6)
    sets = [c["rkd"] for c in clients]
    key_index = _shuffled_index(len(clients), batch, 41)
    assert batch % 3 != 0
    a = _random_cts(name, batch, 12)
    b = np.ascontiguousarray(np.roll(a, 1, axis=0)[:, ::-1])
    ref = to_host(ev.multiply_relin_keys(to_device(a), to_device(b), sets, key_index))
    pool = _pool(ctx, [0, 0, 0], chunk=7)  # chunks of 7 shuffled input sets: every chunk straddles clients
    try:
        out = pool.multiply_relin_keys(a, b, sets, key_index)
        bad = np.nonzero((out != ref).any(axis=(1, 2, 3)))[0]
        assert bad.size == 0, bad[:8]
        # the order of clients in the batch does not matter: the same pairs sorted by client give the same words
        order = np.argsort(key_index, kind="stable")
        out_sorted = pool.multiply_relin_keys(np.ascontiguousarray(a[order]), np.ascontiguousarray(b[order]), sets, key_index[order])
        assert (out_sorted == ref[order]).all()
        pool.set_chunk(0)
        inplace = a.copy()
        assert pool.multiply_relin_keys(inplace, b, sets, key_index, out=inplace) is not None
        assert (inplace == ref).all()
    finally:
        pool.close()
    picks = _spread(key_index, 64)
    assert len(picks) >= 64
    for i in picks:
        k = int(key_index[i])
        assert (ref[i] == o.relinearize(o.multiply(a[i], b[i]), clients[k]["rk"])).all(), (i, k)


# ---- 5: rotations ----
def test_rotations_match_the_batched_calls_and_the_oracle():
    from sunscreen_amd import HipBfvError
    from sunscreen_amd.batch import to_device, to_host

    name, batch = "default_8192_17", 50
    o, ctx, ev = _context(name)
    clients = _galois_clients(name, 6)
    sets = [c["gkd"] for c in clients]
    key_index = _shuffled_index(len(clients), batch, 52)
    ct = _random_cts(name, batch, 13)
    dct = to_device(ct)
    picks = _spread(key_index, 6)
    pool = _pool(ctx, [0, 0, 0], chunk=5)  # 5 shuffled input sets of 6 clients: direct and chain sets meet in the chunks
    try:
        for steps in DIRECT_STEPS + (1, 0):
            ref = to_host(ev.rotate_rows_keys(dct, steps, sets, key_index))
            out = pool.rotate_rows_keys(ct, steps, sets, key_index)
            assert (out == ref).all(), steps
            for i in picks:
                gk = clients[int(key_index[i])]["gk"]
                assert (ref[i] == (o.rotate_rows(ct[i], steps, gk) if steps else ct[i])).all(), (steps, i)
            inplace = ct.copy()
            pool.rotate_rows_keys(inplace, steps, sets, key_index, out=inplace)
            assert (inplace == ref).all(), steps
        ref = to_host(ev.rotate_columns_keys(dct, sets, key_index))
        assert (pool.rotate_columns_keys(ct, sets, key_index) == ref).all()
        for i in picks:
            assert (ref[i] == o.rotate_columns(ct[i], clients[int(key_index[i])]["gk"])).all(), i
        inplace = ct.copy()
        pool.rotate_columns_keys(inplace, sets, key_index, out=inplace)
        assert (inplace == ref).all()
        # one shared key set: the num_key_sets = 1, all-zero key_index case
        one = to_host(ev.rotate_rows_keys(dct, 3, [sets[1]], np.zeros(batch, dtype=np.uint32)))
        assert (pool.rotate_rows(ct, 3, sets[1]) == one).all()
        assert (pool.rotate_columns(ct, sets[1]) == to_host(ev.rotate_columns_keys(dct, [sets[1]], np.zeros(batch, dtype=np.uint32)))).all()
        # an output shifted by one input set overlaps its input other than exactly: refused before anything runs
        buf = np.concatenate([ct, ct[:1]])
        before = buf.copy()
        for call in (lambda: pool.rotate_rows_keys(buf[:batch], 3, sets, key_index, out=buf[1:]),
                     lambda: pool.rotate_columns_keys(buf[:batch], sets, key_index, out=buf[1:])):
            with pytest.raises(HipBfvError) as ei:
                call()
            assert _hr(ei) == E_INVALIDARG
            assert (buf == before).all()
    finally:
        pool.close()


# ---- 6: programs ----
def test_program_run_keys_matches_program_run_keys_and_the_oracle():
    from sunscreen_amd import GaloisKeys, RelinearizationKeys
    from sunscreen_amd.batch import to_device, to_host
    from sunscreen_amd.workloads import chi_sq_optimized, dot_product

    name = "default_4096_16"
    o, ctx, ev = _context(name)
    clients = []
    for k in range(4):  # clients 2 and 3 hold one Galois element more than clients 0 and 1: two kinds of key sets in one batch
        O.seed(600 + k)
        sk, pk, rk, gk = o.keygen(galois_elts="all")
        if k >= 2:
            extra = o.galois_elt_from_step(3)
            gk = dict(gk)
            gk[extra] = o.keygen(relin=False, galois_elts=[extra])[3][extra]  # (of a fresh secret: the graph never reads it)
        clients.append({"pk": pk, "rk": rk, "gk": gk, "rkd": RelinearizationKeys.from_array(ctx, rk), "gkd": GaloisKeys.from_arrays(ctx, gk)})
    rks, gks = [c["rkd"] for c in clients], [c["gkd"] for c in clients]
    batch = 11
    key_index = _shuffled_index(4, batch, 63)
    rng = np.random.default_rng(6)

    def enc(hi):
        vals = rng.integers(0, hi, (batch, o.n)).astype(np.uint64)
        return np.stack([o.encrypt(clients[int(k)]["pk"], o.batch_encode(v)) for v, k in zip(vals, key_index)])

    prog = dot_product(o.n // 2)
    ca, cb = enc(4), enc(4)
    (ref,) = [to_host(t) for t in prog.run(ev, [to_device(ca), to_device(cb)], rks, gks, key_index=key_index)]
    pool = _pool(ctx, [0, 0, 0], chunk=2)
    try:
        (out,) = pool.run(prog, [ca, cb], rks, gks, key_index=key_index)
        assert (out == ref).all()
        for i in _spread(key_index, 3):
            c = clients[int(key_index[i])]
            (oref,) = run_program(o, prog.nodes, prog.edges, [ca[i], cb[i]], c["rk"], c["gk"])
            assert (ref[i] == oref).all(), i
        prog = chi_sq_optimized()
        cts = [enc(7) for _ in range(3)]
        refs = [to_host(t) for t in prog.run(ev, [to_device(c) for c in cts], rks, None, key_index=key_index)]
        outs = pool.run(prog, cts, rks, None, key_index=key_index)
        assert len(outs) == 4
        for j in range(4):
            assert (outs[j] == refs[j]).all(), j
        for i in _spread(key_index, 3):
            oref = run_program(o, prog.nodes, prog.edges, [c[i] for c in cts], clients[int(key_index[i])]["rk"])
            for j in range(4):
                assert (refs[j][i] == oref[j]).all(), (i, j)
    finally:
        pool.close()


# ---- 7: what counts is what key_index names ----
def test_only_referenced_sets_count_and_bad_ones_fail_before_anything_runs():
    from sunscreen_amd import Context, GaloisKeys, HipBfvError, RelinearizationKeys, _lib
    from sunscreen_amd.batch import to_device, to_host

    name = "default_8192_17"
    o, ctx, ev = _context(name)
    clients = _relin_clients(name, 6)
    gclients = _galois_clients(name, 6)
    n, primes, t = params(name)
    other = Context.from_raw(n, primes, 65537 if t != 65537 else 40961)
    other_params = RelinearizationKeys.from_array(other, clients[0]["rk"])
    empty = RelinearizationKeys()
    foreign = _Foreign()
    batch = 10
    a = _random_cts(name, batch, 14)
    b = np.ascontiguousarray(a[::-1])
    good = [clients[0]["rkd"], None, clients[2]["rkd"], foreign, empty, other_params]
    key_index = np.array([0, 2, 2, 0, 2, 0, 0, 2, 0, 2], dtype=np.uint32)
    ref = to_host(ev.multiply_relin_keys(to_device(a), to_device(b), [clients[0]["rkd"], None, clients[2]["rkd"]], key_index))
    pool = _pool(ctx, [0, 0, 0], chunk=2)
    try:
        # unreferenced entries NULL, foreign, empty or of other parameters: the call succeeds
        assert (pool.multiply_relin_keys(a, b, good, key_index) == ref).all()
        copies = _field(pool, "key_copies")
        assert copies == [2, 2, 2]
        out = np.full((batch, 2, ctx.K, o.n), 7, dtype=np.uint64)
        for bad_set in (1, 3, 4, 5):  # referenced once, in the LAST member's shard: NULL, foreign, empty, other parameters
            ki = key_index.copy()
            ki[8] = bad_set
            with pytest.raises(HipBfvError, match=rf"key set {bad_set} ") as ei:
                pool.multiply_relin_keys(a, b, good, ki, out=out)
            assert _hr(ei) == E_INVALIDARG, bad_set
            assert (out == 7).all() and _field(pool, "key_copies") == copies
        ki = key_index.copy()
        ki[9] = 6
        with pytest.raises(HipBfvError, match=r"key set 6\b") as ei:
            pool.multiply_relin_keys(a, b, good, ki, out=out)
        assert _hr(ei) == E_INVALIDARG
        assert (out == 7).all() and _field(pool, "key_copies") == copies
        # a Galois set without the key of the rotation: step 2 has neither a direct key nor a chain (a power of two)
        gsets = [c["gkd"] for c in gclients]
        gi = (np.arange(batch) % 2 * 3).astype(np.uint32)  # sets 0 and 3
        with pytest.raises(HipBfvError, match=r"key set 0 ") as ei:
            pool.rotate_rows_keys(a, 2, gsets, gi, out=out)
        assert _hr(ei) == E_INVALIDARG
        # step -5: client 3 (a P client) lacks the direct key but has the chain; a P client without its -4 key has neither
        lacking = {e: k for e, k in gclients[1]["gk"].items() if e != o.galois_elt_from_step(-4)}
        gsets2 = [gsets[0], gsets[3], GaloisKeys.from_arrays(ctx, lacking)]
        with pytest.raises(HipBfvError, match=r"key set 2 ") as ei:
            pool.rotate_rows_keys(a, -5, gsets2, np.array([0, 1] * 4 + [2, 0], dtype=np.uint32), out=out)
        assert _hr(ei) == E_INVALIDARG
        with pytest.raises(HipBfvError, match=r"key set 1 ") as ei:
            pool.rotate_columns_keys(a, [gsets[0], clients[0]["rkd"]], np.array([0] * 9 + [1], dtype=np.uint32), out=out)  # a relin set has no column key
        assert _hr(ei) == E_INVALIDARG
        assert (out == 7).all() and _field(pool, "key_copies") == copies
        # device pointers stay refused
        L = _lib.load()
        da = to_device(a)
        hs = (C.c_void_p * 1)(clients[0]["rkd"].get_handle())
        zeros = np.zeros(batch, dtype=np.uint32)
        hr = L.hipbfv_Pool_MultiplyRelinKeys(pool.get_handle(), da.data_ptr(), b.ctypes.data, hs, 1, zeros.ctypes.data_as(C.POINTER(C.c_uint32)),
                                             out.ctypes.data, batch)
        assert hr & 0xFFFFFFFF == E_INVALIDARG
        assert (out == 7).all()
        # and the pool is still usable
        assert (pool.multiply_relin_keys(a, b, good, key_index, out=out) == ref).all()
        assert _field(pool, "key_copies") == copies
    finally:
        pool.close()


# ---- 8: a member copies what its shard names and the call needs ----
def test_a_member_copies_only_the_keys_its_shard_uses():
    from sunscreen_amd.dist import shard_range

    name, batch, steps = "default_8192_17", 50, 3
    o, ctx, ev = _context(name)
    clients = _galois_clients(name, 6)
    sets = [c["gkd"] for c in clients]
    # every member meets a different mix: clients 0..1, 2..3, 4..5 plus one stray input set of client 5 / client 0
    key_index = np.repeat(np.arange(6, dtype=np.uint32), 9)[:batch]
    key_index[3], key_index[48] = 5, 0
    ct = _random_cts(name, batch, 15)
    members = [0, 0, 0]
    expected = []
    for r in range(3):
        lo, hi = shard_range(batch, r, 3)
        named = set(int(k) for k in key_index[lo:hi])
        expected.append(sum(1 if clients[k]["direct"] else 2 for k in named))  # the direct key, or the chain's -1 and 4
    assert len(set(expected)) > 1 and sum(expected) < 3 * sum(len(c["gk"]) for c in clients)
    pool = _pool(ctx, members, chunk=4)
    try:
        first = pool.rotate_rows_keys(ct, steps, sets, key_index)
        assert _field(pool, "key_copies") == expected
        assert _field(pool, "keys_cached") == expected
        key_bytes = 8 * ctx.K * 2 * ctx.KK * o.n
        assert _field(pool, "key_bytes") == [e * key_bytes for e in expected]
        assert (pool.rotate_rows_keys(ct, steps, sets, key_index) == first).all()
        assert _field(pool, "key_copies") == expected  # a second identical call copies nothing
        # the column rotation needs one more element of every set a shard names, and nothing else
        pool.rotate_columns_keys(ct, sets, key_index)
        more = [len(set(int(k) for k in key_index[slice(*shard_range(batch, r, 3))])) for r in range(3)]
        assert _field(pool, "key_copies") == [e + m for e, m in zip(expected, more)]
        assert _field(pool, "key_evictions") == [0, 0, 0]
    finally:
        pool.close()


# ---- 9: the key-cache bound ----
def test_the_key_cache_bound_evicts_and_keeps_the_bits():
    from sunscreen_amd import HipBfvError
    from sunscreen_amd.batch import to_device, to_host

    name, batch = "default_8192_17", 50
    o, ctx, ev = _context(name)
    clients = _relin_clients(name, 6)[:5]
    sets = [c["rkd"] for c in clients]
    key_index = np.repeat(np.arange(5, dtype=np.uint32), 10)  # client after client
    a = _random_cts(name, batch, 16)
    b = np.ascontiguousarray(np.roll(a, 3, axis=0))
    ref = to_host(ev.multiply_relin_keys(to_device(a), to_device(b), sets, key_index))
    key_bytes = 8 * ctx.K * 2 * ctx.KK * o.n
    bound = 2 * key_bytes + 4096  # room for two relinearisation keys
    pool = _pool(ctx, [0, 0], chunk=5)  # shards [0, 25), [25, 50): clients 0-2 and 2-4, three keys each
    try:
        unbounded = pool.multiply_relin_keys(a, b, sets, key_index)
        assert (unbounded == ref).all()
        assert _field(pool, "key_bytes") == [3 * key_bytes] * 2 and _field(pool, "key_evictions") == [0, 0]
        pool.set_key_cache_bytes(bound)
        for _ in range(2):
            assert (pool.multiply_relin_keys(a, b, sets, key_index) == ref).all()
            assert all(kb <= bound for kb in _field(pool, "key_bytes"))
        evictions = _field(pool, "key_evictions")
        assert all(e > 0 for e in evictions), evictions
        # a chunk that names two clients under a bound of one key
        pool.set_key_cache_bytes(key_bytes + 4096)
        pool.set_chunk(20)
        out = np.full_like(a, 7)
        with pytest.raises(HipBfvError, match=rf"{2 * key_bytes} bytes.*{key_bytes + 4096} bytes") as ei:
            pool.multiply_relin_keys(a, b, sets, key_index, out=out)
        assert _hr(ei) == E_OUTOFMEMORY
        pool.set_chunk(5)  # one client per chunk fits
        assert (pool.multiply_relin_keys(a, b, sets, key_index) == ref).all()
        assert all(kb <= key_bytes + 4096 for kb in _field(pool, "key_bytes"))
        # back to no bound: nothing is dropped any more
        pool.set_key_cache_bytes(0)
        before = _field(pool, "key_evictions")
        for _ in range(2):
            assert (pool.multiply_relin_keys(a, b, sets, key_index) == ref).all()
        assert _field(pool, "key_evictions") == before
        assert _field(pool, "key_bytes") == [3 * key_bytes] * 2
    finally:
        pool.close()


# ---- 10: transparent results ----
def test_a_transparent_result_names_its_input_set_in_the_whole_batch():
    from sunscreen_amd import HipBfvError
    from sunscreen_amd.batch import to_device, to_host

    name, batch = "default_8192_17", 10  # members [0, 0, 0]: shards [0, 4), [4, 7), [7, 10)
    o, ctx, ev = _context(name)
    clients = _relin_clients(name, 6)
    sets = [c["rkd"] for c in clients]
    key_index = _shuffled_index(6, batch, 71)
    a = _random_cts(name, batch, 17)
    b = np.ascontiguousarray(a[::-1])
    pool = _pool(ctx, [0, 0, 0], chunk=2)
    try:
        za = a.copy()
        za[8] = 0  # 0 * b = 0: transparent, in the last member's shard
        with pytest.raises(HipBfvError, match="input set 8 ") as ei:
            pool.multiply_relin_keys(za, b, sets, key_index)
        assert _hr(ei) == COR_E_INVALIDOPERATION
        ref = to_host(ev.multiply_relin_keys(to_device(a), to_device(b), sets, key_index))
        assert (pool.multiply_relin_keys(a, b, sets, key_index) == ref).all()
    finally:
        pool.close()


# ---- 11: pinned and pageable host memory ----
def test_pinned_and_pageable_host_memory_give_the_same_bits():
    import torch
    from sunscreen_amd.batch import to_device, to_host

    name, batch = "default_8192_17", 50
    o, ctx, ev = _context(name)
    clients = _galois_clients(name, 6)
    sets = [c["gkd"] for c in clients]
    key_index = _shuffled_index(6, batch, 82)
    ct = _random_cts(name, batch, 18)
    ref = to_host(ev.rotate_rows_keys(to_device(ct), -5, sets, key_index))
    pin = torch.empty(ct.shape, dtype=torch.int64, pin_memory=True)
    pout = torch.empty(ct.shape, dtype=torch.int64, pin_memory=True)
    pin.numpy()[:] = ct.view(np.int64)
    pool = _pool(ctx, [0, 0], chunk=8)
    try:
        assert (pool.rotate_rows_keys(pin, -5, sets, key_index, out=pout) == ref).all()
        assert "bounce_words=0" in pool.describe()  # pinned both ways: nothing was staged
        assert (pool.rotate_rows_keys(ct, -5, sets, key_index) == ref).all()
        assert (pool.rotate_rows_keys(pin, -5, sets, key_index) == ref).all()  # pinned in, pageable out
        assert "bounce_words=0 " not in pool.describe()
    finally:
        pool.close()
