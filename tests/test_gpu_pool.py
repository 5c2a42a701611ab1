"""DevicePool (hipbfv_Pool_*): host-fed batches sharded over pool members, bit for bit against the single-device calls
(BatchEvaluator.multiply_relin, FheProgram.run) and the oracle.  One GPU: members [0], [0, 0], [0, 0, 0] share it."""
import ctypes as C
import functools
import gc
import threading

import numpy as np
import pytest

from oracle import bfv_oracle as O
from tests.bfv_helpers import oracle_for, params
from tests.oracle_program import run_program

pytestmark = pytest.mark.gpu

MEMBERS = ([0], [0, 0], [0, 0, 0])
BATCHES = (1, 2, 5, 257, 1000)


def _random_cts(n, primes, K, count, seed):
    """Ciphertext-shaped residues, uniform below each data prime (bit-exactness needs no valid encryption)."""
    rng = np.random.default_rng(seed)
    out = np.empty((count, 2, K, n), dtype=np.uint64)
    for k in range(K):
        out[:, :, k, :] = rng.integers(0, primes[k], (count, 2, n), dtype=np.uint64)
    return out


@functools.lru_cache(maxsize=None)
def _setup(name, galois=None, seed=5):
    from sunscreen_amd import Context, GaloisKeys, RelinearizationKeys
    from sunscreen_amd.batch import BatchEvaluator

    n, primes, t = params(name)
    o = oracle_for(name)
    O.seed(seed)
    sk, pk, rk, gk = o.keygen(galois_elts=list(galois) if isinstance(galois, tuple) else galois)
    ctx = Context.from_raw(n, primes, t)
    ev = BatchEvaluator(ctx)
    rkd = RelinearizationKeys.from_array(ctx, rk)
    gkd = GaloisKeys.from_arrays(ctx, gk) if gk else None
    return o, sk, pk, rk, gk, ctx, ev, rkd, gkd


@functools.lru_cache(maxsize=None)
def _mulrelin_data(name):
    from sunscreen_amd.batch import to_device, to_host

    o, sk, pk, rk, gk, ctx, ev, rkd, gkd = _setup(name)
    a = _random_cts(o.n, params(name)[1], ctx.K, max(BATCHES), 11)
    b = np.ascontiguousarray(np.roll(a, 1, axis=0)[:, ::-1])  # other sets, polynomials swapped
    ref = to_host(ev.multiply_relin(to_device(a), to_device(b), rkd))
    return a, b, ref


def _pool(ctx, members, chunk=0):
    from sunscreen_amd import DevicePool

    p = DevicePool(ctx, members)
    p.set_chunk(chunk)
    return p


def _hr(e):
    return e.value.hresult & 0xFFFFFFFF


def _key_copies(pool):
    return [int(x) for x in __import__("re").findall(r"key_copies=(\d+)", pool.describe())]


@pytest.mark.parametrize("name", ["default_8192_17", "default_16384_17"])
def test_multiply_relin_matches_the_batched_call_and_the_oracle(name):
    o, sk, pk, rk, gk, ctx, ev, rkd, gkd = _setup(name)
    a, b, ref = _mulrelin_data(name)
    # several chunks per member, the library's choice, one chunk larger than any shard (bounded at N = 16384: its buffers)
    chunks = (7, 0, 200 if o.n == 16384 else 4096)
    for mi, members in enumerate(MEMBERS):
        pool = _pool(ctx, members)
        try:
            for bi, batch in enumerate(BATCHES):
                pool.set_chunk(chunks[(mi + bi) % len(chunks)])
                out = pool.multiply_relin(a[:batch], b[:batch], rkd)
                assert out.shape == (batch, 2, ctx.K, o.n)
                bad = np.nonzero((out != ref[:batch]).any(axis=(1, 2, 3)))[0]
                assert bad.size == 0, (members, batch, bad[:8])
        finally:
            pool.close()
    for i in (0, 499, 999):
        assert (ref[i] == o.relinearize(o.multiply(a[i], b[i]), rk)).all(), i


def test_batch_zero_and_a_batch_smaller_than_the_pool():
    o, sk, pk, rk, gk, ctx, ev, rkd, gkd = _setup("default_8192_17")
    a, b, ref = _mulrelin_data("default_8192_17")
    pool = _pool(ctx, [0, 0, 0])
    try:
        out = pool.multiply_relin(a[:0], b[:0], rkd)
        assert out.shape[0] == 0
        assert (pool.multiply_relin(a[:2], b[:2], rkd) == ref[:2]).all()  # the third member's shard is empty
        lines = pool.describe().strip().splitlines()
        assert len(lines) == 3 and all(f"member={i} device=0" in lines[i] for i in range(3))
        assert "slot_words=0" in lines[2]  # it launched nothing and allocated nothing
    finally:
        pool.close()


def test_pinned_and_pageable_host_memory_give_the_same_bits():
    import torch

    o, sk, pk, rk, gk, ctx, ev, rkd, gkd = _setup("default_8192_17")
    a, b, ref = _mulrelin_data("default_8192_17")
    batch = 300
    pa = torch.empty((batch, 2, ctx.K, o.n), dtype=torch.int64, pin_memory=True)
    pb = torch.empty((batch, 2, ctx.K, o.n), dtype=torch.int64, pin_memory=True)
    po = torch.empty((batch, 2, ctx.K, o.n), dtype=torch.int64, pin_memory=True)
    pa.numpy()[:] = a[:batch].view(np.int64)
    pb.numpy()[:] = b[:batch].view(np.int64)
    pool = _pool(ctx, [0, 0], chunk=64)
    try:
        pinned = pool.multiply_relin(pa, pb, rkd, out=po)
        assert (pinned == ref[:batch]).all()
        pageable = pool.multiply_relin(a[:batch], b[:batch], rkd)
        assert (pageable == ref[:batch]).all()
        mixed = pool.multiply_relin(pa, b[:batch], rkd)  # one pinned, one pageable operand
        assert (mixed == ref[:batch]).all()
        assert "bounce_words=0" not in pool.describe()  # the pageable calls staged through the bounce buffers
    finally:
        pool.close()


def _chi_sq_inputs(o, pk, batch, seed):
    rng = np.random.default_rng(seed)
    vals = rng.integers(0, 7, (3, batch, o.n)).astype(np.uint64)
    return vals, [np.stack([o.encrypt(pk, o.batch_encode(vals[k, i])) for i in range(batch)]) for k in range(3)]


def test_program_run_chi_sq_matches_program_run_and_the_oracle():
    from sunscreen_amd.batch import to_device, to_host
    from sunscreen_amd.workloads import chi_sq_optimized

    o, sk, pk, rk, gk, ctx, ev, rkd, gkd = _setup("default_8192_17")
    prog = chi_sq_optimized()
    batch = 13
    vals, cts = _chi_sq_inputs(o, pk, batch, 3)
    ref = [to_host(t) for t in prog.run(ev, [to_device(c) for c in cts], rkd)]
    for members, chunk in (([0], 0), ([0, 0], 3), ([0, 0, 0], 100)):
        pool = _pool(ctx, members, chunk)
        try:
            outs = pool.run(prog, cts, rkd)
        finally:
            pool.close()
        assert len(outs) == 4
        for k in range(4):
            assert (outs[k] == ref[k]).all(), (members, k)
    for i in (0, batch - 1):
        oref = run_program(o, prog.nodes, prog.edges, [c[i] for c in cts], rk)
        for k in range(4):
            assert (ref[k][i] == oref[k]).all()


def test_program_run_dot_product_with_rotations():
    from sunscreen_amd.batch import to_device, to_host
    from sunscreen_amd.workloads import dot_product

    o, sk, pk, rk, gk, ctx, ev, rkd, gkd = _setup("default_4096_16", galois="all")
    prog = dot_product(o.n // 2)
    batch = 7
    rng = np.random.default_rng(2)
    va = rng.integers(0, 4, (batch, o.n)).astype(np.uint64)
    vb = rng.integers(0, 4, (batch, o.n)).astype(np.uint64)
    ca = np.stack([o.encrypt(pk, o.batch_encode(v)) for v in va])
    cb = np.stack([o.encrypt(pk, o.batch_encode(v)) for v in vb])
    (ref,) = [to_host(t) for t in prog.run(ev, [to_device(ca), to_device(cb)], rkd, gkd)]
    pool = _pool(ctx, [0, 0], chunk=2)
    try:
        (out,) = pool.run(prog, [ca, cb], rkd, gkd)
    finally:
        pool.close()
    assert (out == ref).all()
    (oref,) = run_program(o, prog.nodes, prog.edges, [ca[batch - 1], cb[batch - 1]], rk, gk)
    assert (ref[batch - 1] == oref).all()
    dot = int((va[0].astype(np.int64) * vb[0].astype(np.int64)).sum()) % o.t
    assert (o.batch_decode(o.decrypt(out[0], sk)) == dot).all()


def _plain_graph():
    """out = x * p_shared + p_item  (argument 1: ONE plaintext for every set, stride 0; argument 2: per-set plaintexts)"""
    from sunscreen_amd.program import FheProgram

    p = FheProgram()
    x = p.append_input_ciphertext(0)
    ps = p.append_input_plaintext(1)
    pi = p.append_input_plaintext(2)
    p.append_output_ciphertext(p.append_add_plaintext(p.append_multiply_plaintext(x, ps), pi))
    return p


def _item_graph():
    """out = x * p_item"""
    from sunscreen_amd.program import FheProgram

    p = FheProgram()
    x = p.append_input_ciphertext(0)
    p.append_output_ciphertext(p.append_multiply_plaintext(x, p.append_input_plaintext(1)))
    return p


def test_program_run_with_a_shared_plaintext():
    from sunscreen_amd.batch import to_device, to_host

    o, sk, pk, rk, gk, ctx, ev, rkd, gkd = _setup("default_8192_17")
    prog = _plain_graph()
    batch = 11
    rng = np.random.default_rng(9)
    cts = _random_cts(o.n, params("default_8192_17")[1], ctx.K, batch, 4)
    shared = rng.integers(1, o.t, o.n).astype(np.uint64)
    item = rng.integers(0, o.t, (batch, o.n)).astype(np.uint64)
    (ref,) = [to_host(t) for t in prog.run(ev, [to_device(cts), to_device(shared), to_device(item)], rkd)]
    for members, chunk in (([0], 4), ([0, 0, 0], 2)):
        pool = _pool(ctx, members, chunk)
        try:
            (out,) = pool.run(prog, [cts, shared, item])
        finally:
            pool.close()
        assert (out == ref).all(), members
    (oref,) = run_program(o, prog.nodes, prog.edges, [cts[5], shared, item[5]], rk)
    assert (ref[5] == oref).all()


def test_a_transparent_result_names_its_global_input_set_and_the_pool_stays_usable():
    from sunscreen_amd import HipBfvError, _lib
    from sunscreen_amd.batch import to_device, to_host

    o, sk, pk, rk, gk, ctx, ev, rkd, gkd = _setup("default_8192_17")
    a, b, ref = _mulrelin_data("default_8192_17")
    batch = 10  # members [0, 0, 0]: shards [0, 4), [4, 7), [7, 10)
    pool = _pool(ctx, [0, 0, 0], chunk=2)
    try:
        za = a[:batch].copy()
        za[8] = 0  # 0 * b = 0: transparent, in the last member's shard
        with pytest.raises(HipBfvError, match="input set 8 ") as ei:
            pool.multiply_relin(za, b[:batch], rkd)
        assert _hr(ei) == _lib.COR_E_INVALIDOPERATION
        assert (pool.multiply_relin(a[:batch], b[:batch], rkd) == ref[:batch]).all()

        prog = _item_graph()
        cts = a[:batch]
        item = np.zeros((batch, o.n), dtype=np.uint64)
        item[:, 0] = 1 + np.arange(batch, dtype=np.uint64)
        item[9] = 0  # x * 0: transparent at set 9 only, in the last member's shard
        with pytest.raises(HipBfvError, match="input set 9 ") as ei:
            pool.run(prog, [cts, item])
        assert _hr(ei) == _lib.COR_E_INVALIDOPERATION
        item[9, 0] = 10
        (ok,) = pool.run(prog, [cts, item])
        (ref1,) = prog.run(ev, [to_device(cts), to_device(item)])
        assert (ok == to_host(ref1)).all()
    finally:
        pool.close()


def test_missing_and_foreign_keys_fail_before_anything_is_launched():
    from sunscreen_amd import Context, HipBfvError, RelinearizationKeys, _lib
    from sunscreen_amd.batch import to_device
    from sunscreen_amd.program import FheProgram
    from sunscreen_amd.workloads import chi_sq_optimized, dot_product

    o, sk, pk, rk, gk, ctx, ev, rkd, gkd = _setup("default_4096_16", galois="all")
    prog = dot_product(o.n // 2)
    cts = _random_cts(o.n, params("default_4096_16")[1], ctx.K, 3, 8)
    with pytest.raises(HipBfvError) as single:
        prog.run(ev, [to_device(cts), to_device(cts)], rkd, None)
    pool = _pool(ctx, [0, 0])
    try:
        out = np.full((3, 2, ctx.K, o.n), 7, dtype=np.uint64)
        with pytest.raises(HipBfvError) as ei:
            pool.run(prog, [cts, cts], rkd, None, outputs=[out])
        assert _hr(ei) == _hr(single) == _lib.E_INVALIDARG
        assert (out == 7).all()  # nothing was written
        assert _key_copies(pool) == [0, 0]  # nor copied
        # keys of a context with other parameters count as absent; keys of another context with the same parameters are fine
        n, primes, t = params("default_4096_16")
        other = Context.from_raw(n, primes, 65537 if t != 65537 else 40961)
        _, _, rk_o, _ = oracle_for("default_4096_16").keygen()
        with pytest.raises(HipBfvError) as ei:
            pool.multiply_relin(cts, cts, RelinearizationKeys.from_array(other, rk_o))
        assert _hr(ei) == _lib.E_INVALIDARG
        with pytest.raises(HipBfvError) as ei:
            pool.run(chi_sq_optimized(), [cts, cts, cts], RelinearizationKeys.from_array(other, rk_o))
        assert _hr(ei) == _lib.E_INVALIDARG
        twin = Context.from_raw(n, primes, t)
        same = pool.multiply_relin(cts, cts, RelinearizationKeys.from_array(twin, rk))
        assert (same == pool.multiply_relin(cts, cts, rkd)).all()

        # kind 2 inputs, null pointers, unknown kinds: refused by the C ABI itself
        L = _lib.load()
        p = FheProgram()
        x = p.append_input_ciphertext(0)
        p.append_output_ciphertext(p.append_multiply_plaintext(x, p.append_input_plaintext(1)))
        plain = np.ones((3, ctx.K, o.n), dtype=np.uint64)
        kinds = (C.c_uint32 * 2)(0, 2)
        ptrs = (C.c_void_p * 2)(cts.ctypes.data, plain.ctypes.data)
        strides = (C.c_uint64 * 2)(0, ctx.K * o.n)
        optrs = (C.c_void_p * 1)(out.ctypes.data)
        assert L.hipbfv_Pool_ProgramRun(pool.get_handle(), p._h, 3, 2, kinds, ptrs, strides, rkd.get_handle(), None, 1, optrs) & 0xFFFFFFFF == _lib.E_INVALIDARG
        assert "kind 2" in _lib.last_error()
        kinds[1] = 7
        assert L.hipbfv_Pool_ProgramRun(pool.get_handle(), p._h, 3, 2, kinds, ptrs, strides, rkd.get_handle(), None, 1, optrs) & 0xFFFFFFFF == _lib.E_INVALIDARG
        kinds[1] = 1
        strides[1] = o.n
        ptrs[1] = None
        assert L.hipbfv_Pool_ProgramRun(pool.get_handle(), p._h, 3, 2, kinds, ptrs, strides, rkd.get_handle(), None, 1, optrs) & 0xFFFFFFFF == _lib.E_POINTER
        assert L.hipbfv_Pool_ProgramRun(pool.get_handle(), p._h, 3, 2, kinds, None, strides, rkd.get_handle(), None, 1, optrs) & 0xFFFFFFFF == _lib.E_POINTER
        assert L.hipbfv_Pool_MultiplyRelin(pool.get_handle(), cts.ctypes.data, None, rkd.get_handle(), out.ctypes.data, 3) & 0xFFFFFFFF == _lib.E_POINTER
        assert (out == 7).all()
        (good,) = pool.run(prog, [cts, cts], rkd, gkd)  # still usable
        assert good.shape == (3, 2, ctx.K, o.n)
    finally:
        pool.close()


def test_the_key_cache_copies_once_and_follows_the_key_buffer():
    from sunscreen_amd import RelinearizationKeys
    from sunscreen_amd.batch import to_device, to_host

    name = "default_8192_17"
    o, sk, pk, rk, gk, ctx, ev, rkd, gkd = _setup(name)
    a, b, ref = _mulrelin_data(name)
    batch = 40
    pool = _pool(ctx, [0, 0], chunk=8)
    try:
        O.seed(101)
        _, _, rk_a, _ = o.keygen()
        keys_a = RelinearizationKeys.from_array(ctx, rk_a)
        out_a = pool.multiply_relin(a[:batch], b[:batch], keys_a)
        assert _key_copies(pool) == [1, 1]
        assert (pool.multiply_relin(a[:batch], b[:batch], keys_a) == out_a).all()
        assert _key_copies(pool) == [1, 1]  # the second call copies nothing
        assert (out_a == to_host(ev.multiply_relin(to_device(a[:batch]), to_device(b[:batch]), keys_a))).all()
        del keys_a
        gc.collect()
        O.seed(202)
        _, _, rk_b, _ = o.keygen()
        keys_b = RelinearizationKeys.from_array(ctx, rk_b)  # very likely the block keys A just gave back
        out_b = pool.multiply_relin(a[:batch], b[:batch], keys_b)
        assert (out_b == to_host(ev.multiply_relin(to_device(a[:batch]), to_device(b[:batch]), keys_b))).all()
        assert not (out_b == out_a).all()
        assert _key_copies(pool) == [2, 2]
        assert "keys_cached=1" in pool.describe()  # A's copies went with A
    finally:
        pool.close()


def test_two_pools_on_two_threads_give_the_bits_of_a_serial_run():
    o, sk, pk, rk, gk, ctx, ev, rkd, gkd = _setup("default_8192_17")
    a, b, ref = _mulrelin_data("default_8192_17")
    pools = [_pool(ctx, [0], chunk=32), _pool(ctx, [0, 0], chunk=16)]
    results, errors = [None, None], []

    def work(k):
        try:
            lo = 300 * k
            results[k] = [pools[k].multiply_relin(a[lo : lo + 300], b[lo : lo + 300], rkd) for _ in range(3)]
        except Exception as e:  # pragma: no cover - reported below
            errors.append(e)

    try:
        threads = [threading.Thread(target=work, args=(k,)) for k in range(2)]
        for t in threads:
            t.start()
        for t in threads:
            t.join()
    finally:
        for p in pools:
            p.close()
    assert not errors, errors
    for k in range(2):
        for r in results[k]:
            assert (r == ref[300 * k : 300 * k + 300]).all(), k


def test_pools_leave_the_device_and_the_handle_level_evaluators_alone():
    from sunscreen_amd import BFVEvaluator, Ciphertext, _lib

    o, sk, pk, rk, gk, ctx, ev, rkd, gkd = _setup("default_8192_17")
    a, b, ref = _mulrelin_data("default_8192_17")
    L = _lib.load()
    for members in ([0], [0, 0, 0]):
        pool = _pool(ctx, members)
        assert (pool.multiply_relin(a[:3], b[:3], rkd) == ref[:3]).all()
        pool.close()
    assert L.hipbfv_set_device(0) == 0
    hev = BFVEvaluator(ctx)
    x = Ciphertext.from_array(ctx, a[0])
    y = Ciphertext.from_array(ctx, b[0])
    z = hev.relinearize(hev.multiply(x, y), rkd)
    assert (z.to_array() == ref[0]).all()
    pool = _pool(ctx, [0])
    try:
        z2 = hev.relinearize(hev.multiply(x, y), rkd)  # while a pool lives
        assert (z2.to_array() == ref[0]).all()
    finally:
        pool.close()
