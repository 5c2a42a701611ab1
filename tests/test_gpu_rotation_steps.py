"""Row rotations at the edges of the step range through every caller of SEAL's rotate_internal.

A rotation whose own Galois key is absent is decomposed into power-of-two rotations: the non-adjacent form (NAF) of the step,
low digit first, a part of exactly n/2 rows skipped.  The library decides that once (plan_row_rotation) for six callers (the
handle-level call, the batch call, the per-key batch call with its split into a direct and a chain group, the two program
executors, the device pool's walk over the keys a member copies).  Every caller is run here on the steps where the chain can go
wrong -- chains of up to six
hops (the first hop of an out-of-place chain reads the automorphism through the key switch, every later hop rotates its own
output in place through the rotated copy), mixed signs, the skipped n/2 part, steps that must be refused -- and judged three
ways: word for word against the CPU oracle, word for word against the other callers, and by the decoded slots (both rows of
the slot matrix rolled by the step), which no NAF code has a say in (tests/test_oracle_rotation_steps_cpu.py holds the oracle
itself to that and to a hop order derived another way).

Which steps reach the skip.  A step of n/2 - 2^k has the Galois element of step -2^k, so under the power-of-two keys
2047 and 2046 (n = 4096) are ONE hop through the keys of -1 and -2 and never walk their NAF [-2^k, +n/2]; a direct key "of
step 2047" IS the key of step -1.  The skipped part is reached by the other steps above n/3: 2045 = [+1, -4, +n/2],
1707 = [-1, -4, -16, -64, -256, +n/2].  Both kinds are here.  Likewise a chain reads the keys of its own signs:
11 = [-1, -4, +16] does not need the key of +4, -11 = [+1, +4, -16] does.
"""
import ctypes as C
import functools
import os
import re

import numpy as np
import pytest

from oracle import bfv_oracle as O
from tests.bfv_helpers import oracle_for, params

pytestmark = pytest.mark.gpu

E_INVALIDARG = 0x80070057
INT_MAX, INT_MIN = 2**31 - 1, -(2**31)
SENTINEL = -0x5A5A5A5A5A5A5A5B

NAME = "default_4096_16"
H = 2048  # n / 2
COUNT = 20  # above every small-batch limit; three chunks of 7 with a short last one
# accepted steps (NAF parts): 2047 [-1, n/2] and 2046 [-2, n/2] (one hop: the element of -1 / -2), 2045 [1, -4, n/2 skipped],
# 1707 [-1, -4, -16, -64, -256, n/2 skipped], 1025 [1, 1024], 1365 [1, 4, 16, 64, 256, 1024], -683 [1, 4, 16, 64, 256, -1024]
# (the element of 1365: D rotates it through that key),
# 11 [-1, -4, 16], -13 [-1, 4, -16], powers of two, the identity
ACCEPTED = (2047, -2047, 2046, 2045, -2045, 1707, 1025, 1365, -683, 11, -13, 1024, -1024, 1, -1, 0)
REFUSED = (2048, -2048, 2049, -2049, INT_MAX, INT_MIN)
DIRECT = (2045, 1365, -13)  # D holds these steps' own keys (and "the key of 2047": the key of -1, which P holds too)
MIX = np.array([0, 1, 1, 0, 1, 0, 0, 0, 1, 1, 1, 0, 1, 0, 0, 1, 0, 1, 1, 0], dtype=np.uint32)  # D = 0, P = 1: runs and singles, both in each half


def _slots(n, t, item):
    """Two rows that differ and are not periodic, another vector per item: a wrong step, a swapped row or a neighbour's
    result cannot decode to the expected roll."""
    return ((3 * np.arange(n, dtype=np.uint64) + 1 + 5 * item) % np.uint64(t)).astype(np.uint64)


def _rolled(v, step):
    h = v.size // 2
    return np.concatenate([np.roll(v[:h], -step), np.roll(v[h:], -step)])


class _World:
    """One oracle keygen at n = 4096 and three holdings of its Galois keys -- P: every +-2^i key and the column key ("all");
    D: P plus the direct keys of DIRECT; M: P without the key of step +4 -- over COUNT fresh encryptions under the one
    public key, so the same ciphertexts serve every holding.  Evaluators, the pool and the oracle's results per
    (step, holding) are made on first use and shared by the tests of this module."""

    def __init__(self):
        from sunscreen_amd import Context, GaloisKeys
        from sunscreen_amd.batch import to_device

        n, primes, t = params(NAME)
        self.o = o = oracle_for(NAME)
        assert n // 2 == H
        self.ctx = Context.from_raw(n, primes, t)
        O.seed(7101)
        pow2 = [o.galois_elt_from_step(s * (1 << i)) for i in range(H.bit_length() - 1) for s in (1, -1)] + [2 * n - 1]
        direct = [o.galois_elt_from_step(s) for s in DIRECT]
        assert not set(direct) & set(pow2)
        self.sk, self.pk, _, gk = o.keygen(relin=False, galois_elts=sorted(set(pow2)) + direct)
        self.gk = {
            "P": {e: gk[e] for e in pow2},
            "D": dict(gk),
            "M": {e: gk[e] for e in pow2 if e != o.galois_elt_from_step(4)},
        }
        self.gkd = {h: GaloisKeys.from_arrays(self.ctx, d) for h, d in self.gk.items()}
        self.vals = [_slots(n, t, j) for j in range(COUNT)]
        self.cts = np.stack([o.encrypt(self.pk, o.batch_encode(v)) for v in self.vals])
        self.dev = to_device(self.cts)
        self._refs, self._ref_dev, self._evs, self._pool = {}, {}, {}, None

    def direct(self, step):
        """Whether D rotates `step` through a key of its own that P lacks.  By Galois element, not by step: steps that differ
        by n/2 share their element, so D's key of 1365 is also the key of -683 (and 2045's that of -3)."""
        elt = self.o.galois_elt_from_step(step) if step else 0
        return elt in self.gk["D"] and elt not in self.gk["P"]

    def ref(self, step, holding, count=COUNT):
        """o.rotate_rows of the first `count` ciphertexts with that holding's dictionary.  D differs from P by the direct keys
        alone, which only the steps of those elements look up (a chain's hops are powers of two): the others share P's result."""
        if holding == "D" and not self.direct(step):
            holding = "P"
        have = self._refs.get((step, holding))
        if have is None or have.shape[0] < count:
            done = 0 if have is None else have.shape[0]
            more = [self.o.rotate_rows(self.cts[i], step, self.gk[holding]) if step else self.cts[i] for i in range(done, count)]
            have = np.stack(more) if have is None else np.concatenate([have, np.stack(more)])
            self._refs[(step, holding)] = have
            self._ref_dev.pop((step, holding), None)
        return have[:count]

    def ref_dev(self, step, holding, count=COUNT):
        from sunscreen_amd.batch import to_device

        if holding == "D" and not self.direct(step):
            holding = "P"
        self.ref(step, holding, count)
        full = self._refs[(step, holding)]
        if (step, holding) not in self._ref_dev:
            self._ref_dev[(step, holding)] = to_device(full)
        return self._ref_dev[(step, holding)][:count]

    def ref_mixed_dev(self, step, count=COUNT):
        """Item i with the holding MIX names."""
        import torch

        d, p = self.ref_dev(step, "D", count), self.ref_dev(step, "P", count)
        is_d = torch.from_numpy((MIX[:count] == 0)).to(d.device)
        return torch.where(is_d[:, None, None, None], d, p)

    def ev(self, kind):
        """Batch evaluators, made inside a test so that the suite's pipeline selection is in force: "split" (the selection as
        the suite pins it), "chunk7" (the same in chunks of 7), "default" (made with HIPBFV_NO_SMALL_BATCH unset: a few
        ciphertexts take the whole-polynomial pipelines at the degrees that have them)."""
        from sunscreen_amd.batch import BatchEvaluator

        if kind not in self._evs:
            saved = os.environ.get("HIPBFV_NO_SMALL_BATCH")
            if kind == "default":
                os.environ.pop("HIPBFV_NO_SMALL_BATCH", None)
            try:
                self._evs[kind] = BatchEvaluator(self.ctx)
            finally:
                if saved is not None:
                    os.environ["HIPBFV_NO_SMALL_BATCH"] = saved
            if kind == "chunk7":
                self._evs[kind].set_chunk_ops(7)
        return self._evs[kind]

    def hev(self):
        from sunscreen_amd import BFVEvaluator

        if "handle" not in self._evs:
            self._evs["handle"] = BFVEvaluator(self.ctx)
        return self._evs["handle"]

    def pool(self):
        if self._pool is None:
            self._pool = _new_pool(self.ctx, 3)
        return self._pool

    def close(self):
        if self._pool is not None:
            self._pool.close()
            self._pool = None


def _new_pool(ctx, chunk):
    from sunscreen_amd import DevicePool

    p = DevicePool(ctx, [0, 0])  # shards [0, 10) and [10, 20): MIX puts D and P on both sides of the boundary
    p.set_chunk(chunk)
    return p


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


def _hr(call):
    """(HRESULT, message) of a call through the Python mirror; (0, "") when it succeeds."""
    from sunscreen_amd.seal import HipBfvError

    try:
        call()
    except HipBfvError as e:
        return e.hresult & 0xFFFFFFFF, str(e)
    return 0, ""


def _means(w, ct, item, step):
    """Decrypted and decoded with the oracle's secret key: both rows of item's slot vector rolled by the step."""
    return bool((w.o.batch_decode(w.o.decrypt(ct, w.sk)) == _rolled(w.vals[item], step)).all())


# ---- the callers --------------------------------------------------------------------------------------------------------
def _handle(w, step, holding, item, inplace):
    """Evaluator_RotateRows on handles: to a fresh destination (the input stays as it was) or in place."""
    from sunscreen_amd import Ciphertext

    a = Ciphertext.from_array(w.ctx, w.cts[item])
    if inplace:
        w.hev().rotate_rows_inplace(a, step, w.gkd[holding])
        return a.to_array()
    r = w.hev().rotate_rows(a, step, w.gkd[holding])
    assert (a.to_array() == w.cts[item]).all(), (step, holding, "the input of an out-of-place rotation changed")
    return r.to_array()


def _batch(w, ev, step, holding, count, inplace):
    """hipbfv_batch_rotate_rows on the first `count` ciphertexts."""
    import torch

    da = w.dev[:count].clone()
    if inplace:
        return ev.rotate_rows(da, step, w.gkd[holding], out=da)
    out = ev.rotate_rows(da, step, w.gkd[holding])
    assert torch.equal(da, w.dev[:count]), (step, holding, "the input of an out-of-place rotation changed")
    return out


def _per_key(w, ev, step, key_index, count, inplace):
    """hipbfv_batch_rotate_rows_keys with the sets [D, P]."""
    import torch

    da = w.dev[:count].clone()
    sets = [w.gkd["D"], w.gkd["P"]]
    if inplace:
        return ev.rotate_rows_keys(da, step, sets, key_index[:count], out=da)
    out = ev.rotate_rows_keys(da, step, sets, key_index[:count])
    assert torch.equal(da, w.dev[:count]), (step, "the input of an out-of-place rotation changed")
    return out


@functools.lru_cache(maxsize=None)
def _program(step):
    """input -> rotate_left by a literal (rotate_right by -step for a negative step) -> output"""
    from sunscreen_amd.program import FheProgram

    p = FheProgram()
    a = p.append_input_ciphertext(0)
    r = p.append_rotate_left(a, p.append_input_literal(step)) if step >= 0 else p.append_rotate_right(a, p.append_input_literal(-step))
    p.append_output_ciphertext(r)
    return p


def _executors(monkeypatch):
    """Both program executors, selected as test_scheduled_and_node_by_node_executors_agree selects them."""
    for serial in (False, True):
        if serial:
            monkeypatch.setenv("HIPBFV_PROGRAM_SERIAL", "1")
        else:
            monkeypatch.delenv("HIPBFV_PROGRAM_SERIAL", raising=False)
        yield "node_by_node" if serial else "scheduled"
    monkeypatch.delenv("HIPBFV_PROGRAM_SERIAL", raising=False)


def _program_raw(prog, ev, dct, galois, key_index, out):
    """hipbfv_Program_Run (galois: one key object) / hipbfv_Program_RunKeys (galois: a list, with key_index) into the caller's
    own output tensor; returns (HRESULT, message)."""
    from sunscreen_amd import _lib
    from sunscreen_amd.batch import _ptr, _stream

    L = _lib.load()
    batch = dct.shape[0]
    kinds, ptrs, strides = (C.c_uint32 * 1)(0), (C.c_void_p * 1)(_ptr(dct)), (C.c_uint64 * 1)(0)
    optrs = (C.c_void_p * 1)(_ptr(out))
    if key_index is None:
        hr = L.hipbfv_Program_Run(prog._h, ev._h, batch, 1, kinds, ptrs, strides, None, galois.get_handle(), 1, optrs, _stream())
    else:
        idx = np.ascontiguousarray(key_index, dtype=np.uint32)
        gks = (C.c_void_p * len(galois))(*[g.get_handle() for g in galois])
        rks = (C.c_void_p * len(galois))()
        hr = L.hipbfv_Program_RunKeys(prog._h, ev._h, batch, 1, kinds, ptrs, strides, len(galois), rks, gks,
                                      idx.ctypes.data_as(C.POINTER(C.c_uint32)), 1, optrs, _stream())
    return hr & 0xFFFFFFFF, _lib.last_error() if hr else ""


# ---- accepted steps: oracle bits, cross-caller bits, meaning -------------------------------------------------------------
def _run_every_caller(w, step, monkeypatch, count=COUNT, callers=(1, 2, 3, 4, 5)):
    """`step` through the callers named, every result against the oracle with the holding the items ran with; returns what the
    callers gave for item 0 on holding P, one entry per copy of the loop, for the cross-caller and meaning checks."""
    import torch
    from sunscreen_amd.batch import to_device, to_host

    holdings = ("P", "D") if w.direct(step) else ("P",)
    refP = w.ref_dev(step, "P", count)
    mixed = w.ref_mixed_dev(step, count)
    first = {}  # copy of the loop -> item 0 rotated with P's keys (host words)
    if 1 in callers:
        for holding in holdings:
            for item in (0, count - 1):
                for inplace in (False, True):
                    got = _handle(w, step, holding, item, inplace)
                    assert (got == w.ref(step, holding, count)[item]).all(), ("handle", step, holding, item, inplace)
                    if holding == "P" and item == 0:
                        first["handle"] = got
    if 2 in callers:
        shapes = (("default", 1), ("split", count), ("chunk7", count))  # one ciphertext; the split kernels; chunks of 7
        for kind, c in shapes:
            for holding in holdings:
                for inplace in (False, True):
                    got = _batch(w, w.ev(kind), step, holding, c, inplace)
                    torch.cuda.synchronize()
                    assert torch.equal(got, w.ref_dev(step, holding, count)[:c]), ("batch", step, holding, kind, c, inplace)
                    if holding == "P" and kind == "split":
                        first["batch"] = to_host(got[0])
    if 3 in callers:
        ev = w.ev("split")
        for what, ki, ref in (("all P", np.ones(count, dtype=np.uint32), refP), ("all D", np.zeros(count, dtype=np.uint32), w.ref_dev(step, "D", count)),
                              ("D and P interleaved", MIX, mixed)):
            for inplace in (False, True):
                got = _per_key(w, ev, step, ki, count, inplace)
                torch.cuda.synchronize()
                assert torch.equal(got, ref), ("per-key", step, what, inplace)
                if what == "all P":
                    first["per-key"] = to_host(got[0])
        got = _per_key(w, w.ev("chunk7"), step, MIX, count, False)  # the direct / chain split inside chunks of 7
        assert torch.equal(got, mixed), ("per-key", step, "chunks of 7")
    if 4 in callers:
        prog, ev = _program(step), w.ev("split")
        c = min(count, 9)
        dct = w.dev[:c].contiguous()
        for executor in _executors(monkeypatch):
            for holding in holdings:
                (got,) = prog.run(ev, [dct], None, w.gkd[holding])
                torch.cuda.synchronize()
                assert torch.equal(got, w.ref_dev(step, holding, count)[:c]), ("program", executor, step, holding)
                if holding == "P":
                    first[executor] = to_host(got[0])
            (got,) = prog.run(ev, [dct], None, [w.gkd["D"], w.gkd["P"]], key_index=MIX[:c])
            torch.cuda.synchronize()
            assert torch.equal(got, mixed[:c]), ("program keys", executor, step)
        assert torch.equal(dct, w.dev[:c])
    if 5 in callers:
        pool = w.pool()
        sets = [w.gkd["D"], w.gkd["P"]]
        host_mixed = to_host(mixed)
        got = pool.rotate_rows_keys(w.cts[:count], step, sets, MIX[:count])
        assert (got == host_mixed).all(), ("pool", step)
        inplace = w.cts[:count].copy()
        pool.rotate_rows_keys(inplace, step, sets, MIX[:count], out=inplace)
        assert (inplace == host_mixed).all(), ("pool in place", step)
        first["pool"] = pool.rotate_rows_keys(w.cts[:count], step, [w.gkd["P"]], np.zeros(count, dtype=np.uint32))[0]
    for kind in ("split", "chunk7", "default"):
        if kind in w._evs:
            w.ev(kind).check()
    return first


def _check_first(w, step, first, copies):
    """One (step, holding): every copy's bits are the same words, and each decodes to the rolled rows."""
    assert set(first) == set(copies), (step, sorted(first))
    ref = w.ref(step, "P", 1)[0]
    for copy, got in first.items():
        assert (got == ref).all(), (copy, step)  # hence every caller equals every other
        assert _means(w, got, 0, step), (copy, step)


@pytest.mark.parametrize("step", ACCEPTED)
def test_every_caller_gives_the_oracles_bits_and_the_rolled_rows(step, monkeypatch):
    """Each accepted step through the six copies (handles; the batch call at one ciphertext, at 20 and at 20 in chunks of 7;
    the per-key call on P, on D and on D and P interleaved; a program through both executors with one key set and with
    interleaved sets; the pool with D and P across the shard boundary), out of place and in place."""
    w = _world()
    first = _run_every_caller(w, step, monkeypatch)
    _check_first(w, step, first, ("handle", "batch", "per-key", "scheduled", "node_by_node", "pool"))
    # an item that ran with D's keys decodes alike (the interleaved results above are D's on MIX == 0)
    last_d = int(np.nonzero(MIX == 0)[0][-1])
    assert _means(w, w.ref(step, "D")[last_d], last_d, step), step


def test_a_direct_key_and_the_chain_give_other_bits_and_the_same_slots():
    """D's own keys of 2045, 1365 and -13 are used, not the chain: the oracle's bits with D differ from P's (every caller above
    equals the oracle with the holding it ran with) and both decode to the rolled rows.  Step 2047 has no key of its own to
    hold: its Galois element is that of step -1, so D and P rotate it through the same key and give the same words."""
    w = _world()
    o = w.o
    assert o.galois_elt_from_step(-683) == o.galois_elt_from_step(1365)  # -683 = 1365 - n/2
    for step in DIRECT + (-683,):
        assert w.direct(step), step
        d, p = w.ref(step, "D", 2), w.ref(step, "P", 2)
        for i in range(2):
            assert not (d[i] == p[i]).all(), (step, i)
            assert _means(w, d[i], i, step) and _means(w, p[i], i, step), (step, i)
    assert o.galois_elt_from_step(H - 1) == o.galois_elt_from_step(-1) and o.galois_elt_from_step(H - 2) == o.galois_elt_from_step(-2)
    assert o.galois_elt_from_step(H - 1) in w.gk["P"]
    assert (o.rotate_rows(w.cts[0], H - 1, w.gk["D"]) == o.rotate_rows(w.cts[0], -1, w.gk["P"])).all()
    for step in (2045, 1707):  # the steps that do walk a NAF with the n/2 part in it
        assert o.galois_elt_from_step(step) not in w.gk["P"]


# ---- refused steps -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("step", REFUSED)
def test_every_caller_refuses_a_step_of_half_the_degree_or_more(step, monkeypatch):
    """|step| >= n/2 (INT_MIN included, whose negation does not exist): E_INVALIDARG from every caller, the output keeps its
    sentinel, the input its words, and the next accepted call on the same evaluator or pool gives the oracle's bits."""
    import torch
    from sunscreen_amd import Ciphertext
    from sunscreen_amd.batch import to_host

    w = _world()
    count = 6
    da = w.dev[:count].clone()
    sets = [w.gkd["D"], w.gkd["P"]]
    ki = MIX[:count]
    # 1: handles -- a destination that holds another ciphertext keeps it; in place the ciphertext keeps its words
    a, d = Ciphertext.from_array(w.ctx, w.cts[0]), Ciphertext.from_array(w.ctx, w.cts[1])
    from sunscreen_amd import _lib

    L = _lib.load()
    hr = L.Evaluator_RotateRows(w.hev()._h, a._h, step, w.gkd["P"]._h, d._h, None) & 0xFFFFFFFF
    assert hr == E_INVALIDARG, ("handle", step, hex(hr))
    assert (d.to_array() == w.cts[1]).all() and (a.to_array() == w.cts[0]).all(), ("handle", step)
    assert _hr(lambda: w.hev().rotate_rows_inplace(a, step, w.gkd["P"]))[0] == E_INVALIDARG
    assert (a.to_array() == w.cts[0]).all(), ("handle in place", step)
    # 2, 3: the batch calls, out of place into a sentinel and in place
    for kind in ("split", "chunk7", "default"):
        ev = w.ev(kind)
        for what, call in (("batch", lambda x, out: ev.rotate_rows(x, step, w.gkd["P"], out=out)),
                           ("per-key", lambda x, out: ev.rotate_rows_keys(x, step, sets, ki, out=out))):
            out = torch.full_like(da, SENTINEL)
            assert _hr(lambda: call(da, out))[0] == E_INVALIDARG, (what, kind, step)
            assert _hr(lambda: call(da, da))[0] == E_INVALIDARG, (what, kind, step, "in place")
            torch.cuda.synchronize()
            assert bool((out == SENTINEL).all()) and torch.equal(da, w.dev[:count]), (what, kind, step)
        ev.check()
    # 4: programs -- the literal is a u64 the executors read as SEAL's int (run.rs: `v as i32`); rotate_right negates it
    if step == INT_MIN:
        left_literal, right_literal = 2**31, None  # (int)2^31 = INT_MIN; its negation is not a step
    else:
        left_literal, right_literal = (step, None) if step > 0 else (None, -step)
    from sunscreen_amd.program import FheProgram

    prog = FheProgram()
    x = prog.append_input_ciphertext(0)
    lit = prog.append_input_literal(left_literal if left_literal is not None else right_literal)
    prog.append_output_ciphertext(prog.append_rotate_left(x, lit) if left_literal is not None else prog.append_rotate_right(x, lit))
    ev = w.ev("split")
    for executor in _executors(monkeypatch):
        for galois, index in ((w.gkd["P"], None), (sets, ki)):
            out = torch.full_like(da, SENTINEL)
            hr, msg = _program_raw(prog, ev, da, galois, index, out)
            torch.cuda.synchronize()
            assert hr == E_INVALIDARG, ("program", executor, step, hex(hr), msg)
            assert bool((out == SENTINEL).all()) and torch.equal(da, w.dev[:count]), ("program", executor, step)
    # 5: the pool
    pool = w.pool()
    host_out = np.full((count, 2, w.o.K, w.o.n), 7, dtype=np.uint64)
    host_in = w.cts[:count].copy()
    assert _hr(lambda: pool.rotate_rows_keys(host_in, step, sets, ki, out=host_out))[0] == E_INVALIDARG, ("pool", step)
    assert _hr(lambda: pool.rotate_rows_keys(host_in, step, sets, ki, out=host_in))[0] == E_INVALIDARG, ("pool in place", step)
    assert (host_out == 7).all() and (host_in == w.cts[:count]).all(), ("pool", step)
    # the next accepted call on each of them
    good = 1707
    assert (_handle(w, good, "P", 0, False) == w.ref(good, "P", count)[0]).all()
    for kind in ("split", "chunk7", "default"):
        assert torch.equal(_batch(w, w.ev(kind), good, "P", count, False), w.ref_dev(good, "P", count)), kind
        assert torch.equal(_per_key(w, w.ev(kind), good, MIX, count, False), w.ref_mixed_dev(good, count)), kind
    for executor in _executors(monkeypatch):
        (got,) = _program(good).run(ev, [da], None, sets, key_index=ki)
        assert torch.equal(got, w.ref_mixed_dev(good, count)), executor
    assert (pool.rotate_rows_keys(host_in, good, sets, ki) == to_host(w.ref_mixed_dev(good, count))).all()


# ---- a chain key that is missing -----------------------------------------------------------------------------------------
def test_a_missing_chain_key_fails_the_chains_that_read_it_and_no_other():
    """Holding M lacks the key of step +4.  1365 = [1, 4, 16, ...] and -11 = [1, 4, -16] read it: the per-key call and the pool
    fail before anything runs (the output keeps its sentinel, the error names the set), and so do the single-key batch call
    (its output keeps its sentinel too) and the handle call, with the missing-key error: a refused rotation launches nothing;
    the input keeps its words.  11 = [-1, -4, 16] reads the key of -4, not of +4, and succeeds, as do 2047 (the key of -1),
    1025 and 2045."""
    import torch
    from sunscreen_amd import Ciphertext
    from sunscreen_amd.batch import to_host

    w = _world()
    count = 6
    da = w.dev[:count].clone()
    ev, pool = w.ev("split"), w.pool()
    sets = [w.gkd["P"], w.gkd["D"], w.gkd["M"]]
    ki = np.array([0, 1, 0, 2, 1, 0], dtype=np.uint32)
    who = ["P", "D", "M"]
    host_in = w.cts[:count].copy()
    for step in (1365, -11):
        out = torch.full_like(da, SENTINEL)
        hr, msg = _hr(lambda: ev.rotate_rows_keys(da, step, sets, ki, out=out))
        assert hr == E_INVALIDARG and "key set 2" in msg, (step, hex(hr), msg)
        torch.cuda.synchronize()
        assert bool((out == SENTINEL).all()) and torch.equal(da, w.dev[:count]), step
        host_out = np.full((count, 2, w.o.K, w.o.n), 7, dtype=np.uint64)
        hr, msg = _hr(lambda: pool.rotate_rows_keys(host_in, step, sets, ki, out=host_out))
        assert hr == E_INVALIDARG and re.search(r"key set 2\b", msg), (step, hex(hr), msg)
        assert (host_out == 7).all() and (host_in == w.cts[:count]).all(), step
        scratch_out = torch.full_like(da, SENTINEL)
        hr, msg = _hr(lambda: ev.rotate_rows(da, step, w.gkd["M"], out=scratch_out))
        assert hr == E_INVALIDARG and "key" in msg and "step count" not in msg, (step, hex(hr), msg)
        torch.cuda.synchronize()
        assert bool((scratch_out == SENTINEL).all()) and torch.equal(da, w.dev[:count]), step
        a = Ciphertext.from_array(w.ctx, w.cts[0])
        hr, msg = _hr(lambda: w.hev().rotate_rows(a, step, w.gkd["M"]))
        assert hr == E_INVALIDARG and "key" in msg and "step count" not in msg, (step, hex(hr), msg)
        assert (a.to_array() == w.cts[0]).all(), step
    ev.check()
    for step in (2047, 1025, 11, 2045):
        refs = np.stack([w.o.rotate_rows(w.cts[i], step, w.gk[who[k]]) for i, k in enumerate(ki)])
        assert (to_host(ev.rotate_rows_keys(da, step, sets, ki)) == refs).all(), step
        assert (pool.rotate_rows_keys(host_in, step, sets, ki) == refs).all(), step
        assert (to_host(ev.rotate_rows(da, step, w.gkd["M"])) == w.ref(step, "P", count)).all(), step
        assert (_handle(w, step, "M", 3, False) == refs[3]).all(), step
    ev.check()


# ---- what a pool member copies -------------------------------------------------------------------------------------------
@pytest.mark.parametrize(
    "step,hops",
    [
        (2047, [-1]),  # the key of -1 alone: no key "of n/2" is looked up or copied
        (2045, [1, -4]),  # [+1, -4, +n/2]: the skipped part costs no lookup and no copy
        (1707, [-1, -4, -16, -64, -256]),  # ... +n/2
        (1365, [1, 4, 16, 64, 256, 1024]),
    ],
)
def test_a_pool_member_copies_the_keys_of_the_hops_and_nothing_for_the_skipped_part(step, hops):
    """Fresh pools, a batch on P: every member copies exactly the keys of the chain's hops (Pool_Describe's key_bytes)."""
    w = _world()
    key_bytes = 8 * w.ctx.K * 2 * w.ctx.KK * w.o.n
    pool = _new_pool(w.ctx, 4)
    try:
        got = pool.rotate_rows_keys(w.cts, step, [w.gkd["P"]], np.zeros(COUNT, dtype=np.uint32))
        text = pool.describe()
        assert [int(x) for x in re.findall(r"key_bytes=(\d+)", text)] == [len(hops) * key_bytes] * 2, (step, text)
        assert [int(x) for x in re.findall(r"key_copies=(\d+)", text)] == [len(hops)] * 2, (step, text)
        assert (got == w.ref(step, "P")).all(), step
    finally:
        pool.close()


# ---- larger degrees ------------------------------------------------------------------------------------------------------
def _hop_elts(o, steps):
    """The Galois elements the chains of `steps` read under power-of-two keys: written out per step below, checked against
    the sum."""
    elts = set()
    for step, hops in steps.items():
        assert sum(hops) in (step, step - o.n // 2, step + o.n // 2), (step, hops)
        elts |= {o.galois_elt_from_step(p) for p in hops}
    return sorted(elts)


def _larger(name, steps, count):
    from sunscreen_amd import Context, GaloisKeys
    from sunscreen_amd.batch import BatchEvaluator, to_device

    n, primes, t = params(name)
    o = oracle_for(name)
    O.seed(n)
    sk, pk, _, gk = o.keygen(relin=False, galois_elts=_hop_elts(o, steps))  # only the keys these steps read
    ctx = Context.from_raw(n, primes, t)
    vals = [_slots(n, t, j) for j in range(count)]
    cts = np.stack([o.encrypt(pk, o.batch_encode(v)) for v in vals])
    return o, sk, gk, ctx, BatchEvaluator(ctx), GaloisKeys.from_arrays(ctx, gk), vals, cts, to_device(cts)


@pytest.mark.parametrize(
    "name,count,steps",
    [
        ("default_8192_17", 20, {4095: [-1], 1365: [1, 4, 16, 64, 256, 1024], 4093: [1, -4]}),
        ("default_16384_17", 12, {8191: [-1], -2731: [1, 4, 16, 64, 256, 1024, -4096], 8189: [1, -4]}),
        ("default_32768_17", 3, {16383: [-1]}),  # the key of step -1 alone ("all" at this degree is gigabytes)
    ],
)
def test_edge_steps_at_larger_degrees(name, count, steps):
    """The batch call and the per-key call at n = 8192, 16384 (seven hops) and 32768: the first and the last item against the
    oracle and the rolled rows, every item of the two callers and of the in-place forms against each other."""
    import torch
    from sunscreen_amd.batch import to_host

    o, sk, gk, ctx, ev, gkd, vals, cts, dev = _larger(name, steps, count)
    if name == "default_16384_17" and os.environ.get("HIPBFV_NO_SPLIT_KS", "0")[:1] != "1":
        # this count takes the split key switch under either pipeline selection (a few ciphertexts, <= 4, would not)
        ev.profile(True)
        ev.profile_reset()
        ev.rotate_rows(dev, 8191, gkd)
        torch.cuda.synchronize()
        seen = ev.profile_read()
        ev.profile(False)
        assert "ks_mid" in seen and "ks_mac" not in seen, sorted(seen)
    ki = np.zeros(count, dtype=np.uint32)
    for step in steps:
        got = ev.rotate_rows(dev, step, gkd)
        keys = ev.rotate_rows_keys(dev, step, [gkd], ki)
        inplace = dev.clone()
        ev.rotate_rows(inplace, step, gkd, out=inplace)
        inplace_keys = dev.clone()
        ev.rotate_rows_keys(inplace_keys, step, [gkd], ki, out=inplace_keys)
        torch.cuda.synchronize()
        assert torch.equal(got, keys) and torch.equal(got, inplace) and torch.equal(got, inplace_keys), (name, step)
        host = to_host(got)
        for i in (0, count - 1):
            assert (host[i] == o.rotate_rows(cts[i], step, gk)).all(), (name, step, i)
            assert (o.batch_decode(o.decrypt(host[i], sk)) == _rolled(vals[i], step)).all(), (name, step, i)
    if len(gk) == 1:  # no chain without the other keys
        for call in (lambda: ev.rotate_rows(dev, 5, gkd), lambda: ev.rotate_rows_keys(dev, 5, [gkd], ki)):
            hr, msg = _hr(call)
            assert hr == E_INVALIDARG and "key" in msg and "step count" not in msg, (name, hex(hr), msg)
    ev.check()


# ---- random steps --------------------------------------------------------------------------------------------------------
def _random_trials():
    # HIPBFV_FUZZ_ROTATION_STEPS="lo:hi": extended campaigns; the suite's own are 0:8
    lo, hi = (int(x) for x in os.environ.get("HIPBFV_FUZZ_ROTATION_STEPS", "0:8").split(":"))
    return range(lo, hi)


@pytest.mark.parametrize("trial", _random_trials())
def test_random_steps_through_the_batch_the_per_key_and_the_program_callers(trial, monkeypatch):
    """A step drawn uniformly from (-n/2, n/2), seeded by the trial: oracle bits, cross-caller bits and the rolled rows."""
    w = _world()
    step = int(np.random.default_rng(7700 + trial).integers(-H + 1, H))
    first = _run_every_caller(w, step, monkeypatch, count=9, callers=(2, 3, 4))
    _check_first(w, step, first, ("batch", "per-key", "scheduled", "node_by_node"))
