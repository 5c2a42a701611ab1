"""Mixed-step rotation batches: hipbfv_batch_rotate_rows_items / hipbfv_batch_apply_galois_items rotate item i by its own step or
Galois element, the items with a key of their own in ONE head / middle / tail sequence whose kernels take the automorphism and
the key per item.  Every result is judged word for word against the CPU oracle's rotation of that item alone (and, where a step
runs its NAF chain, against the uniform batch call of that step); the decoded slots must be the rows rolled by the item's step.

The first group shares the world of tests/test_gpu_rotation_steps.py (n = 4096: every +-2^i key, the column key, direct keys
of 2045, 1365 and -13 in holding D, holding M without the key of +4).  The second group runs one small case through each
kernel body the per-item table touches: the integer-policy (MIXED) head and tail, the per-row packed head, and the
whole-polynomial route below n = 4096, where the items are grouped by element instead."""
import numpy as np
import pytest

from oracle import bfv_oracle as O
from tests.bfv_helpers import oracle_for, params
from tests.test_gpu_rotation_steps import COUNT, E_INVALIDARG, H, INT_MIN, SENTINEL, _hr, _rolled, _slots, _World

pytestmark = pytest.mark.gpu

# every step twice at least, equal steps never neighbours
DIRECT_STEPS = [1, -1, 2, 1024, -1024, 2045, 1365, -13, 0, 1, -1, 2, 1024, -1024, 2045, 1365, -13, 0, 1, 2045]
# under P (no direct keys) 2045, 1365, -13, 11 and 1707 walk their chains; 2047 is one hop through the key of -1
CHAIN_STEPS = [1, 11, -1, 1707, 2, 2047, 1024, 2045, -1024, 1365, 0, -13, 11, 1, 1707, 2047, 2045, 0, 1365, -13]
assert len(DIRECT_STEPS) == len(CHAIN_STEPS) == COUNT
assert all(a != b for s in (DIRECT_STEPS, CHAIN_STEPS) for a, b in zip(s, s[1:]))
assert all(DIRECT_STEPS.count(s) >= 2 for s in set(DIRECT_STEPS))


class _ItemsWorld(_World):
    def item_ref(self, item, step, holding):
        """The oracle's rotation of ONE item by its own step (computed once)."""
        key = ("item", item, step, holding)
        if key not in self._refs:
            self._refs[key] = self.o.rotate_rows(self.cts[item], step, self.gk[holding]) if step else self.cts[item]
        return self._refs[key]

    def items_ref(self, steps, holding):
        return np.stack([self.item_ref(i, s, holding) for i, s in enumerate(steps)])


_WORLD = []


@pytest.fixture(scope="module", autouse=True)
def _shared_world():
    yield
    while _WORLD:
        _WORLD.pop().close()


def _world() -> _ItemsWorld:
    if not _WORLD:
        _WORLD.append(_ItemsWorld())
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


def _check_items(w, got, steps, holding, what):
    """Word for word against the oracle per item, and the decoded slots against the roll by the item's own step."""
    ref = w.items_ref(steps, holding)
    for i, step in enumerate(steps):
        assert (got[i] == ref[i]).all(), (what, i, step)
        assert (w.o.batch_decode(w.o.decrypt(got[i], w.sk)) == _rolled(w.vals[i], step)).all(), (what, i, step)


# ---- first group: n = 4096 -----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind,launches", [("split", 1), ("chunk7", 3)])
def test_mixed_steps_with_direct_keys_run_in_one_launch_sequence_per_chunk(kind, launches):
    """20 items, 8 distinct direct steps and the identity, interleaved.  At the default chunk the head and tail grids have
    2 * 20 = 40 (polynomial, item) rows, a multiple of 8: the XCD row order is taken.  In chunks of 7 (7, 7, 6) it is not, and
    the last chunk is short.  Either way: one head / middle / tail sequence per chunk and no rotated copy."""
    import torch
    from sunscreen_amd.batch import to_host

    w = _world()
    ev = w.ev(kind)
    assert w.ctx.K == 2  # 2 * COUNT rows in the head as in the tail
    da = w.dev.clone()
    out, seen = _profiled(ev, lambda: ev.rotate_rows_items(da, DIRECT_STEPS, w.gkd["D"]))
    assert torch.equal(da, w.dev), "the input of an out-of-place call changed"
    assert seen.get("ks_head") == launches and seen.get("ks_tail") == launches and seen.get("ks_mid") == launches, seen
    assert "galois" not in seen and "ks_mac" not in seen, seen
    _check_items(w, to_host(out), DIRECT_STEPS, "D", kind)
    ev.check()


def test_direct_and_chain_steps_in_one_call():
    """Holding P: the power-of-two steps and 2047 rotate through their keys in the mixed launch, the others walk their NAF chains
    grouped by step.  Every item is the oracle's NAF result and the item of the uniform batch call with its step."""
    import torch
    from sunscreen_amd.batch import to_host

    w = _world()
    for kind in ("split", "chunk7"):
        ev = w.ev(kind)
        out = ev.rotate_rows_items(w.dev, CHAIN_STEPS, w.gkd["P"])
        torch.cuda.synchronize()
        _check_items(w, to_host(out), CHAIN_STEPS, "P", kind)
        for step in sorted(set(CHAIN_STEPS)):
            uniform = ev.rotate_rows(w.dev, step, w.gkd["P"])
            for i in [i for i, s in enumerate(CHAIN_STEPS) if s == step]:
                assert torch.equal(out[i], uniform[i]), (kind, step, i)
        ev.check()


def test_per_item_galois_elements():
    """apply_galois_items: the identity (a copy), the column element 2N - 1 and row elements, D's direct ones included."""
    import torch
    from sunscreen_amd.batch import to_host

    w = _world()
    o, n = w.o, w.o.n
    pick = [1, 2 * n - 1, o.galois_elt_from_step(1), o.galois_elt_from_step(-1), 2 * n - 1, o.galois_elt_from_step(2045), 1,
            o.galois_elt_from_step(1024), o.galois_elt_from_step(1365), o.galois_elt_from_step(1)]
    elts = (pick * 2)[:COUNT]
    assert all(a != b for a, b in zip(elts, elts[1:]))
    for kind in ("split", "chunk7"):
        ev = w.ev(kind)
        got = to_host(ev.apply_galois_items(w.dev, elts, w.gkd["D"]))
        torch.cuda.synchronize()
        for i, e in enumerate(elts):
            ref = w.cts[i] if e == 1 else o.apply_galois(w.cts[i], e, w.gk["D"])
            assert (got[i] == ref).all(), (kind, i, e)
        ev.check()


def _refusals():
    n = 2 * H
    return [
        ("a step of n/2", "rotate", "P", lambda good: good[:3] + [H] + good[4:7] + [-H] + good[8:], 3, "step count"),
        ("INT_MIN", "rotate", "P", lambda good: good[:5] + [INT_MIN] + good[6:], 5, "step count"),
        ("an even element", "galois", "P", lambda good: good[:2] + [4] + good[3:], 2, "odd"),
        ("an element of 2N", "galois", "P", lambda good: good[:4] + [2 * n] + good[5:6] + [2 * n + 1] + good[7:], 4, "below"),
        ("a missing chain key", "rotate", "M", lambda good: good[:6] + [-11] + good[7:], 6, "key"),
    ]


@pytest.mark.parametrize("what,call,holding,spoil,item,word", _refusals(), ids=[r[0] for r in _refusals()])
def test_refusals_launch_nothing(what, call, holding, spoil, item, word):
    """One bad item among good ones (direct keys, a chain, a copy): E_INVALIDARG, the message names the first bad item, every
    output word keeps its sentinel, the input its words -- and the same call without the bad item then succeeds."""
    import torch
    from sunscreen_amd.batch import to_host

    w = _world()
    ev = w.ev("chunk7")
    count = 9
    da = w.dev[:count].clone()
    if call == "rotate":
        good = [1, 0, 11, -1, 1024, 2, 0, 11, -1024]
        fn = lambda args, out: ev.rotate_rows_items(da, args, w.gkd[holding], out=out)  # noqa: E731
    else:
        e = w.o.galois_elt_from_step
        good = [e(1), 1, e(-1), 2 * w.o.n - 1, e(2), 1, e(1024), e(1), 2 * w.o.n - 1]
        fn = lambda args, out: ev.apply_galois_items(da, args, w.gkd[holding], out=out)  # noqa: E731
    out = torch.full_like(da, SENTINEL)
    hr, msg = _hr(lambda: fn(spoil(good), out))
    torch.cuda.synchronize()
    assert hr == E_INVALIDARG and f"item {item}:" in msg and word in msg, (what, hex(hr), msg)
    assert bool((out == SENTINEL).all()) and torch.equal(da, w.dev[:count]), what
    hr, msg = _hr(lambda: fn(spoil(good), da))  # in place: refused alike, nothing written
    torch.cuda.synchronize()
    assert hr == E_INVALIDARG and f"item {item}:" in msg, (what, "in place", hex(hr), msg)
    assert torch.equal(da, w.dev[:count]), what
    got = to_host(fn(good, out))
    torch.cuda.synchronize()
    for i, g in enumerate(good):
        if call == "rotate":
            ref = w.item_ref(i, g, holding)
        else:
            ref = w.cts[i] if g == 1 else w.o.apply_galois(w.cts[i], g, w.gk[holding])
        assert (got[i] == ref).all(), (what, "the accepted call", i, g)
    ev.check()


def test_in_place_gives_the_oracles_bits_and_a_partial_overlap_is_refused():
    """out2 == ct2 exactly: the items are grouped by element and staged (the fused key switch cannot gather from what it
    overwrites).  An output shifted by one item against the input is refused before anything is written."""
    import torch
    from sunscreen_amd.batch import to_host

    w = _world()
    steps = [1, 2045, 0, 11, 1, -13, 2045, 0, 11, -1024, 1365, 1, -13, 2045, 1365, 0, -1, 11, -1, 1]
    for kind in ("split", "chunk7"):
        ev = w.ev(kind)
        da = w.dev.clone()
        got, seen = _profiled(ev, lambda: ev.rotate_rows_items(da, steps, w.gkd["D"], out=da))
        assert got.data_ptr() == da.data_ptr()
        assert seen.get("galois"), seen  # the rotated copy of the grouped route
        _check_items(w, to_host(da), steps, "D", ("in place", kind))
        ev.check()
    ev = w.ev("split")
    buf = torch.cat([w.dev, w.dev[:1]])
    before = buf.clone()
    for call in (lambda: ev.rotate_rows_items(buf[:-1], steps, w.gkd["D"], out=buf[1:]),
                 lambda: ev.rotate_rows_items(buf[1:], steps, w.gkd["D"], out=buf[:-1]),
                 lambda: ev.apply_galois_items(buf[:-1], [1] * COUNT, w.gkd["D"], out=buf[1:])):
        hr, msg = _hr(call)
        assert hr == E_INVALIDARG and "overlap" in msg, (hex(hr), msg)
    torch.cuda.synchronize()
    assert torch.equal(buf, before)


def test_one_item_and_one_distinct_step_equal_the_uniform_call():
    import torch
    from sunscreen_amd.batch import to_host

    w = _world()
    for kind in ("default", "split", "chunk7"):
        ev = w.ev(kind)
        for step, holding in ((1365, "D"), (1365, "P"), (0, "P"), (-1, "P")):
            one = ev.rotate_rows_items(w.dev[3:4], [step], w.gkd[holding])
            torch.cuda.synchronize()
            assert (to_host(one)[0] == w.item_ref(3, step, holding)).all(), (kind, step, holding)
            assert torch.equal(one, ev.rotate_rows(w.dev[3:4], step, w.gkd[holding])), (kind, step, holding)
        if kind == "default":
            continue
        for step, holding in ((2045, "D"), (2, "P"), (1707, "P")):
            got = ev.rotate_rows_items(w.dev, [step] * COUNT, w.gkd[holding])
            uniform = ev.rotate_rows(w.dev, step, w.gkd[holding])
            torch.cuda.synchronize()
            assert torch.equal(got, uniform), (kind, step, holding)
            for i in (0, COUNT - 1):
                assert (to_host(got[i]) == w.item_ref(i, step, holding)).all(), (kind, step, holding, i)
        ev.check()


def test_the_grouped_route_at_the_same_degree(monkeypatch):
    """HIPBFV_NO_FUSED_GALOIS=1 (read when an evaluator is made) sends an out-of-place call through the per-element groups: the
    same bits as the oracle, hence as the mixed launch."""
    import torch
    from sunscreen_amd.batch import BatchEvaluator, to_host

    w = _world()
    monkeypatch.setenv("HIPBFV_NO_FUSED_GALOIS", "1")
    ev = BatchEvaluator(w.ctx)
    ev.set_chunk_ops(7)
    out, seen = _profiled(ev, lambda: ev.rotate_rows_items(w.dev, DIRECT_STEPS, w.gkd["D"]))
    assert seen.get("galois") and seen.get("ks_head", 0) > 1, seen
    _check_items(w, to_host(out), DIRECT_STEPS, "D", "grouped")
    assert torch.equal(out, w.ev("split").rotate_rows_items(w.dev, DIRECT_STEPS, w.gkd["D"]))
    ev.check()


# ---- second group: one small case per kernel body -----------------------------------------------------------------------
def _small_case(n, primes, t, steps, seed, monkeypatch):
    """Fresh keys for exactly the steps' elements, one encryption per item, an evaluator whose pipelines are chosen by the
    parameters alone; returns what the checks need and the kernels the call launched."""
    from sunscreen_amd import Context, GaloisKeys
    from sunscreen_amd.batch import BatchEvaluator, to_device, to_host

    o = O.Oracle(n, primes, t)
    O.seed(seed)
    elts = sorted({o.galois_elt_from_step(s) for s in steps if s})
    sk, pk, _, gk = o.keygen(relin=False, galois_elts=elts)
    ctx = Context.from_raw(n, primes, t)
    vals = [_slots(n, t, j) for j in range(len(steps))]
    cts = np.stack([o.encrypt(pk, o.batch_encode(v)) for v in vals])
    monkeypatch.setenv("HIPBFV_NO_SMALL_BATCH", "1")
    ev = BatchEvaluator(ctx)
    gkd = GaloisKeys.from_arrays(ctx, gk)
    dev = to_device(cts)
    out, seen = _profiled(ev, lambda: ev.rotate_rows_items(dev, steps, gkd))
    got = to_host(out)
    for i, step in enumerate(steps):
        ref = o.rotate_rows(cts[i], step, gk) if step else cts[i]
        assert (got[i] == ref).all(), (n, i, step)
        assert (o.batch_decode(o.decrypt(got[i], sk)) == _rolled(vals[i], step)).all(), (n, i, step)
    ev.check()
    return ctx, seen


def test_integer_policy_head_and_tail_take_the_table(monkeypatch):
    """The 3 x 54-bit data primes with a 56-bit special prime at n = 8192: every key prime takes the integer policy, the MIXED
    bodies of the head and the tail read the per-item table."""
    n = 8192
    primes = O.coeff_modulus_create(n, [54, 54, 54, 56])
    assert primes[:3] == [0x3FFFFFFFE7C001, 0x3FFFFFFFEB8001, 0x3FFFFFFFEF8001]
    ctx, seen = _small_case(n, primes, O.plain_batching(n, 17), [1, -2, 1, 0], 5401, monkeypatch)
    assert ctx.K == 3 and ctx.KK == 4
    assert seen.get("ks_head") == 1 and seen.get("ks_tail") == 1 and "galois" not in seen and "ks_mac" not in seen, seen


def test_per_row_packed_head_takes_the_table(monkeypatch):
    """SEAL's default primes at n = 16384: the rows of T are packed per key prime (the PACK = 2 head)."""
    n, primes, t = params("default_16384")
    ctx, seen = _small_case(n, primes, t, [1, -1, 4], 16384, monkeypatch)
    assert seen.get("ks_head") == 1 and seen.get("ks_tail") == 1 and "galois" not in seen and "ks_mac" not in seen, seen


def test_below_the_split_kernels_the_items_are_grouped_by_element(monkeypatch):
    """n = 1024 with the bit sizes of the reference's unit-test set: the whole-polynomial key switch, no table -- two groups."""
    n = 1024
    primes = O.coeff_modulus_create(n, [50, 30, 30, 50, 50])
    ctx, seen = _small_case(n, primes, O.plain_batching(n, 20), [1, -1, 1], 1024, monkeypatch)
    assert seen.get("galois") == 2 and seen.get("ks_mac") == 2 and "ks_head" not in seen, seen
