"""Sums of rotations: hipbfv_batch_rotate_rows_sum / hipbfv_batch_apply_galois_sum give out[g] = sum_t rotate(source of item
g * terms + t, steps[t]) with every term finished and added inside the key switch's last kernel (ks_tail_sum).  Every result is
judged word for word against the CPU oracle -- o.rotate_rows / o.apply_galois per term, folded with o.add -- and by its decoded
slots, which must be the sum of the sources' rows rolled by the terms' steps, mod t.

The first group shares the world of tests/test_gpu_rotation_steps.py (n = 4096, K = 2: holdings P, D and M over 20 ciphertexts).
The second group runs one small case through each kernel body: the integer-policy (MIXED) head and summing tail, the 8-prime form
that sums through the output rows behind the per-row packed head, and the staging-and-fold route below n = 4096."""
import ctypes as C

import numpy as np
import pytest

from oracle import bfv_oracle as O
from tests.bfv_helpers import params
from tests.test_gpu_rotation_steps import COUNT, E_INVALIDARG, H, SENTINEL, _hr, _rolled, _slots, _World

pytestmark = pytest.mark.gpu

E_POINTER = 0x80004003
GROUPS, TERMS = 5, 4
DIRECT_STEPS = [1, -13, 0, 2045]  # under D: three keys of their own and the identity
CHAIN_STEPS = [11, 1707, 1, 2045]  # under P: three NAF chains and one direct key
assert GROUPS * TERMS == COUNT

_WORLD = []


@pytest.fixture(scope="module", autouse=True)
def _shared_world():
    yield
    while _WORLD:
        _WORLD.pop().close()


def _world() -> _World:
    if not _WORLD:
        _WORLD.append(_World())
    return _WORLD[0]


def _profiled(ev, call):
    """The result of call() and the kernels it launched: {name: launches}."""
    import torch

    ev.profile(True)
    ev.profile_reset()
    try:
        out = call()
        torch.cuda.synchronize()
        seen = {k: v["launches"] for k, v in ev.profile_read().items()}
    finally:
        ev.profile(False)
    return out, seen


def _source(groups, terms, src_index):
    return [i if src_index is None else src_index[i % len(src_index)] for i in range(groups * terms)]


def _oracle_sums(o, cts, gk, steps, groups, src_index, galois=False, cache=None):
    """out[g] = the oracle's rotations of the group's terms, folded with o.add (every (source, step) rotated once)."""
    cache = {} if cache is None else cache
    src = _source(groups, len(steps), src_index)
    out = []
    for g in range(groups):
        acc = None
        for t, step in enumerate(steps):
            s = src[g * len(steps) + t]
            if (s, step) not in cache:
                if galois:
                    cache[(s, step)] = cts[s] if step == 1 else o.apply_galois(cts[s], step, gk)
                else:
                    cache[(s, step)] = o.rotate_rows(cts[s], step, gk) if step else cts[s]
            acc = cache[(s, step)] if acc is None else o.add(acc, cache[(s, step)])
        out.append(acc)
    return np.stack(out)


def _check_sums(o, sk, got, ref, vals, row_steps, groups, src_index, what):
    """Word for word against the oracle's fold; the decoded slots against the sum of the rolled rows mod t.  row_steps: the row
    rotation of every term (None: that term swaps the rows -- the column element)."""
    src = _source(groups, len(row_steps), src_index)
    t = np.uint64(o.t)
    for g in range(groups):
        assert (got[g] == ref[g]).all(), (what, g)
        assert o.noise_budget(ref[g], sk) > 0, (what, g)
        want = np.zeros_like(vals[0])
        for k, step in enumerate(row_steps):
            v = vals[src[g * len(row_steps) + k]]
            v = np.concatenate([v[v.size // 2:], v[: v.size // 2]]) if step is None else _rolled(v, step)
            want = (want + v) % t
        assert (o.batch_decode(o.decrypt(got[g], sk)) == want).all(), (what, g)


_CASE1 = {}


def _case1(w):
    """The bits of case 1 at the default chunk (computed once): every other route to the same sums is compared with them."""
    import torch

    if "out" not in _CASE1:
        ev = w.ev("split")
        da = w.dev.clone()
        out, seen = _profiled(ev, lambda: ev.rotate_rows_sum(da, DIRECT_STEPS, w.gkd["D"]))
        assert torch.equal(da, w.dev), "the input changed"
        ev.check()
        _CASE1["out"], _CASE1["seen"] = out, seen
        _CASE1["ref"] = _oracle_sums(w.o, w.cts, w.gk["D"], DIRECT_STEPS, GROUPS, None)
    return _CASE1


# ---- first group: n = 4096 -----------------------------------------------------------------------------------------------
def test_direct_and_identity_terms_run_one_summing_sequence():
    """5 groups x 4 terms of distinct ciphertexts, three direct keys and the identity: ONE ks_head, ks_mid and ks_tail_sum; no tail of
    single items, no rotated copy, no whole-polynomial key switch and no element-wise add."""
    from sunscreen_amd.batch import to_host

    w = _world()
    c = _case1(w)
    seen = c["seen"]
    assert seen.get("ks_head") == 1 and seen.get("ks_mid") == 1 and seen.get("ks_tail_sum") == 1, seen
    assert not {"ks_tail", "galois", "ks_mac", "eltwise"} & set(seen), seen
    _check_sums(w.o, w.sk, to_host(c["out"]), c["ref"], w.vals, DIRECT_STEPS, GROUPS, None, "default chunk")


@pytest.mark.parametrize("chunk,sequences", [(7, 5), (3, 10)])
def test_chunks_and_slices_give_the_same_bits(chunk, sequences):
    """chunk 7: one group per sequence, five sequences.  chunk 3: every group in two slices, 3 + 1 terms, the second accumulating."""
    import torch
    from sunscreen_amd.batch import BatchEvaluator, multiply_sum_plan

    w = _world()
    plan = multiply_sum_plan(GROUPS, TERMS, chunk)
    assert len(plan) == sequences
    if chunk == 3:
        assert plan[:2] == [(0, 1, 0, 3, False), (0, 1, 3, 1, True)], plan[:2]
    ev = BatchEvaluator(w.ctx)
    ev.set_chunk_ops(chunk)
    out, seen = _profiled(ev, lambda: ev.rotate_rows_sum(w.dev, DIRECT_STEPS, w.gkd["D"]))
    assert seen.get("ks_tail_sum") == sequences and seen.get("ks_head") == sequences and seen.get("ks_mid") == sequences, seen
    assert not {"ks_tail", "galois", "ks_mac", "eltwise"} & set(seen), seen
    assert torch.equal(out, _case1(w)["out"]), chunk
    ev.check()


def test_source_indexing():
    """One ciphertext per group by four steps; one set of four ciphertexts shared by all groups; the same (source, step) twice."""
    import torch
    from sunscreen_amd.batch import to_host

    w = _world()
    o, ev, gk = w.o, w.ev("split"), w.gk["D"]
    cache = {}
    # src_index[i] = g: sources = 5
    idx = [i // TERMS for i in range(COUNT)]
    got = to_host(ev.rotate_rows_sum(w.dev[:GROUPS], DIRECT_STEPS, w.gkd["D"], src_index=idx))
    _check_sums(o, w.sk, got, _oracle_sums(o, w.cts, gk, DIRECT_STEPS, GROUPS, idx, cache=cache), w.vals, DIRECT_STEPS, GROUPS, idx, "one per group")
    # {0, 1, 2, 3} shared by 5 groups: sources = 4
    idx = [0, 1, 2, 3]
    out = ev.rotate_rows_sum(w.dev[:TERMS], DIRECT_STEPS, w.gkd["D"], groups=GROUPS, src_index=idx)
    got = to_host(out)
    _check_sums(o, w.sk, got, _oracle_sums(o, w.cts, gk, DIRECT_STEPS, GROUPS, idx, cache=cache), w.vals, DIRECT_STEPS, GROUPS, idx, "shared")
    for g in range(1, GROUPS):
        assert torch.equal(out[g], out[0]), g
    # the same (source, step) listed twice contributes twice
    steps, idx = [2045, 2045], [3, 3]
    got = to_host(ev.rotate_rows_sum(w.dev[:4], steps, w.gkd["D"], groups=1, src_index=idx))
    r = o.rotate_rows(w.cts[3], 2045, gk)
    assert (got[0] == o.add(r, r)).all()
    _check_sums(o, w.sk, got, np.stack([o.add(r, r)]), w.vals, steps, 1, idx, "twice")
    ev.check()


def test_eight_groups_take_the_xcd_row_order():
    """8 groups x 2 terms: the summing tail's grid has 2 * 8 (polynomial, group) rows, a multiple of 8 -- the XCD row order, which
    five groups never take."""
    from sunscreen_amd.batch import to_host

    w = _world()
    steps = [2045, -13]
    ev = w.ev("split")
    out, seen = _profiled(ev, lambda: ev.rotate_rows_sum(w.dev[:16], steps, w.gkd["D"]))
    assert seen.get("ks_tail_sum") == 1 and "eltwise" not in seen, seen
    _check_sums(w.o, w.sk, to_host(out), _oracle_sums(w.o, w.cts, w.gk["D"], steps, 8, None), w.vals, steps, 8, None, "8 groups")
    ev.check()


def test_chain_terms_are_rotated_beforehand_and_summed_as_identity_terms():
    """Holding P: 11, 1707 and 2045 walk their NAF chains, 1 has its key.  Against the oracle and against rotate_rows_items + add."""
    import torch
    from sunscreen_amd.batch import to_host

    w = _world()
    for kind in ("split", "chunk7"):
        ev = w.ev(kind)
        out, seen = _profiled(ev, lambda: ev.rotate_rows_sum(w.dev, CHAIN_STEPS, w.gkd["P"]))
        assert seen.get("ks_tail_sum") == (1 if kind == "split" else GROUPS) and "eltwise" not in seen, seen
        ref = _oracle_sums(w.o, w.cts, w.gk["P"], CHAIN_STEPS, GROUPS, None)
        _check_sums(w.o, w.sk, to_host(out), ref, w.vals, CHAIN_STEPS, GROUPS, None, kind)
        items = ev.rotate_rows_items(w.dev, CHAIN_STEPS * GROUPS, w.gkd["P"]).reshape(GROUPS, TERMS, 2, w.ctx.K, -1)
        hand = items[:, 0].contiguous()
        for t in range(1, TERMS):
            hand = ev.add(hand, items[:, t].contiguous())
        assert torch.equal(out, hand), kind
        ev.check()


def test_one_term_equals_rotate_rows_items():
    import torch

    w = _world()
    for kind in ("split", "chunk7"):
        ev = w.ev(kind)
        for step, holding in ((2045, "D"), (0, "D"), (1707, "P"), (-1, "P")):
            got = ev.rotate_rows_sum(w.dev, [step], w.gkd[holding])
            assert torch.equal(got, ev.rotate_rows_items(w.dev, [step] * COUNT, w.gkd[holding])), (kind, step, holding)
        ev.check()


def test_apply_galois_sum():
    """The identity, the column element 2N - 1 and two row elements under D, against the oracle."""
    from sunscreen_amd.batch import to_host

    w = _world()
    o = w.o
    elts = [1, 2 * o.n - 1, o.galois_elt_from_step(1), o.galois_elt_from_step(2045)]
    ev = w.ev("split")
    out, seen = _profiled(ev, lambda: ev.apply_galois_sum(w.dev, elts, w.gkd["D"]))
    assert seen.get("ks_head") == 1 and seen.get("ks_tail_sum") == 1 and not {"ks_tail", "galois", "eltwise"} & set(seen), seen
    ref = _oracle_sums(o, w.cts, w.gk["D"], elts, GROUPS, None, galois=True)
    _check_sums(o, w.sk, to_host(out), ref, w.vals, [0, None, 1, 2045], GROUPS, None, "galois")
    ev.check()


def _raw(ev, ct, sources, src_index, index_len, steps, gk, out, groups, terms):
    """The C entry point itself: the arguments a mirror would refuse on its own."""
    import torch
    from sunscreen_amd import _lib
    from sunscreen_amd.seal import _check

    idx = None if src_index is None else (C.c_uint32 * max(1, len(src_index)))(*src_index)
    st = None if steps is None else (C.c_int32 * max(1, len(steps)))(*steps)
    _check(_lib.load().hipbfv_batch_rotate_rows_sum(ev._h, C.c_void_p(ct.data_ptr()), sources, idx, index_len, st, gk.get_handle() if gk is not None else None,
                                                    C.c_void_p(out.data_ptr()), groups, terms, C.c_void_p(torch.cuda.current_stream().cuda_stream)))


def _refusals():
    one = [i // TERMS for i in range(COUNT)]
    # name, holding, (sources, src_index, index_len, steps, groups, terms), HRESULT, words of the message
    return [
        ("a step of n/2", "D", (COUNT, None, 0, [1, -13, H, 2045], GROUPS, TERMS), E_INVALIDARG, ("term 2:", "step count")),
        ("a missing chain key", "M", (COUNT, None, 0, [1, 0, 2, -11], GROUPS, TERMS), E_INVALIDARG, ("term 3:", "key")),
        ("an index equal to sources", "D", (GROUPS, one[:7] + [GROUPS] + one[8:], COUNT, DIRECT_STEPS, GROUPS, TERMS), E_INVALIDARG, ("item 7:",)),
        ("an empty index table", "D", (GROUPS, one, 0, DIRECT_STEPS, GROUPS, TERMS), E_INVALIDARG, ("index",)),
        ("no table and too few sources", "D", (COUNT - 1, None, 0, DIRECT_STEPS, GROUPS, TERMS), E_INVALIDARG, ("sources",)),
        ("no terms", "D", (COUNT, None, 0, DIRECT_STEPS, GROUPS, 0), E_INVALIDARG, ("term",)),
        ("no steps", "D", (COUNT, None, 0, None, GROUPS, TERMS), E_POINTER, ()),
    ]


@pytest.mark.parametrize("what,holding,args,hresult,words", _refusals(), ids=[r[0] for r in _refusals()])
def test_refusals_launch_nothing_and_write_nothing(what, holding, args, hresult, words):
    import torch

    w = _world()
    ev = w.ev("split")
    sources, src_index, index_len, steps, groups, terms = args
    da = w.dev.clone()
    out = torch.full((GROUPS, 2, w.ctx.K, w.ctx.poly_modulus_degree), SENTINEL, dtype=torch.int64, device=da.device)
    (hr, msg), seen = _profiled(ev, lambda: _hr(lambda: _raw(ev, da, sources, src_index, index_len, steps, w.gkd[holding], out, groups, terms)))
    assert hr == hresult and all(word in msg for word in words), (what, hex(hr), msg)
    assert seen == {}, (what, seen)
    assert bool((out == SENTINEL).all()) and torch.equal(da, w.dev), what


def test_overlapping_output_is_refused_and_no_groups_is_ok():
    import torch

    w = _world()
    ev = w.ev("split")
    buf = torch.cat([w.dev, torch.full_like(w.dev[:GROUPS], SENTINEL)])
    before = buf.clone()
    calls = {
        "out2 == ct2": lambda: _raw(ev, buf, COUNT, None, 0, DIRECT_STEPS, w.gkd["D"], buf, GROUPS, TERMS),
        "one item of overlap": lambda: _raw(ev, buf, COUNT, None, 0, DIRECT_STEPS, w.gkd["D"], buf[COUNT - 1:], GROUPS, TERMS),
    }
    for what in ("out2 == ct2", "one item of overlap"):
        (hr, msg), seen = _profiled(ev, lambda: _hr(calls[what]))
        assert hr == E_INVALIDARG and "overlap" in msg and seen == {}, (what, hex(hr), msg, seen)
    (hr, msg), seen = _profiled(ev, lambda: _hr(lambda: _raw(ev, buf, COUNT, None, 0, DIRECT_STEPS, None, buf[COUNT:], GROUPS, TERMS)))
    assert hr == E_POINTER and seen == {}, (hex(hr), msg, seen)
    (hr, msg), seen = _profiled(ev, lambda: _hr(lambda: _raw(ev, buf, 0, None, 0, DIRECT_STEPS, w.gkd["D"], buf[COUNT:], 0, TERMS)))
    assert hr == 0 and seen == {}, (hex(hr), msg, seen)
    torch.cuda.synchronize()
    assert torch.equal(buf, before)


def test_the_grouped_route_at_the_same_degree(monkeypatch):
    """HIPBFV_NO_FUSED_GALOIS=1 (read when an evaluator is made): the terms are rotated into a stage and folded by the element-wise
    add -- the bits of case 1."""
    import torch
    from sunscreen_amd.batch import BatchEvaluator

    w = _world()
    monkeypatch.setenv("HIPBFV_NO_FUSED_GALOIS", "1")
    ev = BatchEvaluator(w.ctx)
    out, seen = _profiled(ev, lambda: ev.rotate_rows_sum(w.dev, DIRECT_STEPS, w.gkd["D"]))
    assert "ks_tail_sum" not in seen and seen.get("eltwise") == GROUPS * (TERMS - 1), seen
    assert torch.equal(out, _case1(w)["out"])
    ev.check()


# ---- second group: one small case per kernel body -----------------------------------------------------------------------
def _small_case(n, primes, t, steps, groups, seed, monkeypatch):
    """Fresh keys for exactly the steps' elements, one encryption per item, an evaluator whose pipelines are chosen by the
    parameters alone; judged against the oracle by bits and by decoded slots.  Returns the context and the kernels launched."""
    from sunscreen_amd import Context, GaloisKeys
    from sunscreen_amd.batch import BatchEvaluator, to_device, to_host

    o = O.Oracle(n, primes, t)
    O.seed(seed)
    elts = sorted({o.galois_elt_from_step(s) for s in steps if s})
    sk, pk, _, gk = o.keygen(relin=False, galois_elts=elts)
    ctx = Context.from_raw(n, primes, t)
    vals = [_slots(n, t, j) for j in range(groups * len(steps))]
    cts = np.stack([o.encrypt(pk, o.batch_encode(v)) for v in vals])
    monkeypatch.setenv("HIPBFV_NO_SMALL_BATCH", "1")
    ev = BatchEvaluator(ctx)
    gkd = GaloisKeys.from_arrays(ctx, gk)
    dev = to_device(cts)
    out, seen = _profiled(ev, lambda: ev.rotate_rows_sum(dev, steps, gkd))
    _check_sums(o, sk, to_host(out), _oracle_sums(o, cts, gk, steps, groups, None), vals, steps, groups, None, n)
    ev.check()
    return ctx, seen


def test_integer_policy_bodies_of_the_head_and_the_summing_tail(monkeypatch):
    """The 3 x 54-bit data primes with a 56-bit special prime at n = 8192: every key prime takes the integer policy (MIXED)."""
    n = 8192
    primes = O.coeff_modulus_create(n, [54, 54, 54, 56])
    ctx, seen = _small_case(n, primes, O.plain_batching(n, 17), [1, -2, 0], 2, 5402, monkeypatch)
    assert ctx.K == 3 and ctx.KK == 4
    assert seen.get("ks_head") == 1 and seen.get("ks_tail_sum") == 1 and not {"ks_tail", "galois", "ks_mac", "eltwise"} & set(seen), seen


def test_eight_primes_sum_through_the_output_rows_behind_the_packed_head(monkeypatch):
    """SEAL's default primes at n = 16384 (K = 8): the summing tail adds every term onto the group's rows in out; the rows of T are
    packed per key prime (the PACK = 2 head)."""
    n, primes, t = params("default_16384")
    ctx, seen = _small_case(n, primes, t, [1, -1, 4], 2, 16385, monkeypatch)
    assert ctx.K == 8
    assert seen.get("ks_head") == 1 and seen.get("ks_tail_sum") == 1 and not {"ks_tail", "galois", "ks_mac", "eltwise"} & set(seen), seen


def test_below_the_split_kernels_the_terms_are_staged_and_folded(monkeypatch):
    """n = 1024 with the bit sizes of the reference's unit-test set: the whole-polynomial key switch and the element-wise add."""
    n = 1024
    primes = O.coeff_modulus_create(n, [50, 30, 30, 50, 50])
    ctx, seen = _small_case(n, primes, O.plain_batching(n, 20), [1, -1, 0], 2, 1025, monkeypatch)
    assert "ks_head" not in seen and "ks_tail_sum" not in seen and seen.get("ks_mac") and seen.get("eltwise") == 2 * 2, seen
