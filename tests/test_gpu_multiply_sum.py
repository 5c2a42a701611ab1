"""Sums of products with one relinearization per group: hipbfv_batch_multiply_sum / _relin / _relin_keys.

out3[g] = sum_t a[g][t] * b[g][t] must be, word for word, the CPU oracle's `multiply` of every term folded with `add`, and out2[g]
the oracle's `relinearize` of that sum; decrypted and decoded, every group must give sum_t a_t * b_t mod t slot for slot.  Where the
multiply runs through the split kernels the summing tail (`mul_tail_sum` in the profiler) replaces `mul_tail`; elsewhere the terms
are multiplied into a staging buffer and folded.  Every parameter set here is one on which the oracle's own sequence decodes with
noise budget left (5 terms at n = 4096 with two 36-bit data primes leave 19 bits)."""
import ctypes as C
import os
import subprocess
import sys
import tempfile

import numpy as np
import pytest

from oracle import bfv_oracle as O
from tests.bfv_helpers import params

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
E_INVALIDARG = 0x80070057
E_POINTER = 0x80004003
COR_E_INVALIDOPERATION = 0x80131509
SENTINEL = -0x5A5A5A5A5A5A5A5B
BITS54 = (8192, tuple(O.coeff_modulus_create(8192, [54, 54, 54, 56])), O.plain_batching(8192, 17))
UNIT1024 = (1024, tuple(O.coeff_modulus_create(1024, [50, 30, 30, 50, 50])), O.plain_batching(1024, 20))


class _Case:
    """One parameter set, one key pair, groups x terms fresh encryptions of small slot vectors for each operand, and the oracle's
    results -- computed once and shared by the tests that name the same case."""

    def __init__(self, spec, groups, terms, seed):
        n, primes, t = params(spec) if isinstance(spec, str) else spec
        self.n, self.primes, self.t = n, list(primes), t
        self.groups, self.terms = groups, terms
        self.o = O.Oracle(n, self.primes, t)
        O.seed(seed)
        self.sk, self.pk, self.rk, _ = self.o.keygen()
        rng = np.random.default_rng(seed)
        self.va = rng.integers(0, 40, (groups, terms, n)).astype(np.uint64)
        self.vb = rng.integers(0, 40, (groups, terms, n)).astype(np.uint64)
        try:
            self.o.batch_encode(self.va[0, 0])
            self.encode, self.decode = self.o.batch_encode, self.o.batch_decode
        except ValueError:
            # a plain modulus without batching (simple_multiply: t = 2^18): constant polynomials, whose products are constants
            self.va[..., 1:] = 0
            self.vb[..., 1:] = 0
            self.encode = self.decode = lambda v: np.ascontiguousarray(v, dtype=np.uint64)
        enc = lambda v: self.o.encrypt(self.pk, self.encode(v))  # noqa: E731
        self.a = np.stack([np.stack([enc(self.va[g, j]) for j in range(terms)]) for g in range(groups)])
        self.b = np.stack([np.stack([enc(self.vb[g, j]) for j in range(terms)]) for g in range(groups)])
        self._refs = {}

    def sums(self, b=None, vb=None):
        """(ref3, ref2, slots): the oracle's size-3 sums, their relinearizations and the expected decoded slots, per group."""
        key = "ab" if b is None else "aa"
        if key not in self._refs:
            b = self.b if b is None else b
            vb = self.vb if vb is None else vb
            ref3, ref2, slots = [], [], []
            for g in range(self.groups):
                acc = self.o.multiply(self.a[g, 0], b[g, 0])
                for j in range(1, self.terms):
                    acc = self.o.add(acc, self.o.multiply(self.a[g, j], b[g, j]))
                ref3.append(acc)
                ref2.append(self.o.relinearize(acc, self.rk))
                slots.append((self.va[g].astype(object) * vb[g].astype(object)).sum(axis=0) % self.t)
            self._refs[key] = (np.stack(ref3), np.stack(ref2), np.stack(slots).astype(np.uint64))
        return self._refs[key]

    def squares(self):
        return self.sums(self.a, self.va)

    def check(self, out3, out2, refs, what):
        ref3, ref2, slots = refs
        for g in range(self.groups):
            if out3 is not None:
                assert (out3[g] == ref3[g]).all(), (what, "size 3", g)
            if out2 is not None:
                assert (out2[g] == ref2[g]).all(), (what, "relinearized", g)
                assert (self.decode(self.o.decrypt(out2[g], self.sk)) == slots[g]).all(), (what, "slots", g)
        if out3 is not None and out2 is None:
            for g in range(self.groups):  # the size-3 sum decrypts too (the oracle evaluates c0 + c1 s + c2 s^2)
                assert (self.decode(self.o.decrypt(out3[g], self.sk)) == slots[g]).all(), (what, "slots of the size-3 sum", g)


_CASES = {}


def _case(spec, groups, terms, seed=4096):
    key = (spec, groups, terms, seed)
    if key not in _CASES:
        _CASES[key] = _Case(spec, groups, terms, seed)
    return _CASES[key]


@pytest.fixture(scope="module", autouse=True)
def _drop_cases():
    yield
    _CASES.clear()


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


def _hr(call):
    from sunscreen_amd.seal import HipBfvError

    try:
        call()
    except HipBfvError as e:
        return e.hresult & 0xFFFFFFFF, str(e)
    return 0, ""


def _device(c, monkeypatch=None, env=None, small_batch=False):
    """Context, evaluator, device keys and operands of a case; the evaluator's pipelines chosen by the parameters alone unless
    small_batch (HIPBFV_NO_SMALL_BATCH is read when an evaluator is made, the other switches when a context is)."""
    from sunscreen_amd import Context, RelinearizationKeys
    from sunscreen_amd.batch import BatchEvaluator, to_device

    for k, v in (env or {}).items():
        monkeypatch.setenv(k, v)
    if not small_batch:
        monkeypatch.setenv("HIPBFV_NO_SMALL_BATCH", "1")
    ctx = Context.from_raw(c.n, c.primes, c.t)
    ev = BatchEvaluator(ctx)
    return ctx, ev, RelinearizationKeys.from_array(ctx, c.rk), to_device(c.a), to_device(c.b)


def _run_both(c, ev, rkd, da, db, refs, what):
    """multiply_sum and multiply_sum_relin of one case, checked; the kernels both calls launched."""
    from sunscreen_amd.batch import to_host

    out3, seen3 = _profiled(ev, lambda: ev.multiply_sum(da, db))
    out2, seen2 = _profiled(ev, lambda: ev.multiply_sum_relin(da, db, rkd))
    c.check(to_host(out3), None, refs, what)
    c.check(None, to_host(out2), refs, what)
    ev.check()
    return seen3, seen2


# ---- 1: chunk boundaries ----------------------------------------------------------------------------------------------------
def test_chunks_whole_groups_and_slices_give_the_same_bits(monkeypatch):
    """default_4096 (K = 2), 3 groups x 5 terms: one launch at the default chunk, one group per chunk at 7 items, slices of 2, 2
    and 1 terms at 2 items (the accumulate arm).  The summing tail runs 1, 3 and 9 times and the plain tail never."""
    import torch
    from sunscreen_amd.batch import to_host

    c = _case("default_4096", 3, 5)
    ctx, ev, rkd, da, db = _device(c, monkeypatch)
    assert ctx.K == 2
    refs = c.sums()
    first = None
    for chunk, launches in ((None, 1), (7, 3), (2, 9)):
        if chunk:
            ev.set_chunk_ops(chunk)
        before = (da.clone(), db.clone())
        out3, seen = _profiled(ev, lambda: ev.multiply_sum(da, db))
        assert seen.get("mul_tail_sum") == launches and "mul_tail" not in seen and "eltwise" not in seen, (chunk, seen)
        assert seen.get("mul_head") == launches and seen.get("mul_mid", 0) >= launches, (chunk, seen)
        out2, seen = _profiled(ev, lambda: ev.multiply_sum_relin(da, db, rkd))
        assert seen.get("mul_tail_sum") == launches and "mul_tail" not in seen, (chunk, seen)
        assert torch.equal(da, before[0]) and torch.equal(db, before[1]), "an operand changed"
        c.check(to_host(out3), to_host(out2), refs, chunk)
        if first is None:
            first = (out3, out2)
        assert torch.equal(out3, first[0]) and torch.equal(out2, first[1]), chunk
        ev.check()


# ---- 2: one term ------------------------------------------------------------------------------------------------------------
def test_one_term_is_the_plain_multiply(monkeypatch):
    import torch
    from sunscreen_amd.batch import to_host

    c = _case("simple_multiply", 3, 1)
    ctx, ev, rkd, da, db = _device(c, monkeypatch)
    out3, seen = _profiled(ev, lambda: ev.multiply_sum(da, db))
    assert seen.get("mul_tail_sum") == 1, seen
    out2 = ev.multiply_sum_relin(da, db, rkd)
    assert torch.equal(out3, ev.multiply(da[:, 0].contiguous(), db[:, 0].contiguous()))
    assert torch.equal(out2, ev.multiply_relin(da[:, 0].contiguous(), db[:, 0].contiguous(), rkd))
    c.check(to_host(out3), to_host(out2), c.sums(), "one term")
    ev.check()


# ---- 3: squares -------------------------------------------------------------------------------------------------------------
def test_squares_through_the_same_pointer_equal_the_call_with_a_copy(monkeypatch):
    import torch
    from sunscreen_amd.batch import to_host

    c = _case("default_4096", 2, 3)
    ctx, ev, rkd, da, _ = _device(c, monkeypatch)
    copy = da.clone()
    sq3, seen = _profiled(ev, lambda: ev.multiply_sum(da, da))
    assert seen.get("mul_tail_sum") == 1 and "mul_tail" not in seen, seen
    sq2 = ev.multiply_sum_relin(da, da, rkd)
    assert torch.equal(sq3, ev.multiply_sum(da, copy)) and torch.equal(sq2, ev.multiply_sum_relin(da, copy, rkd))
    c.check(to_host(sq3), to_host(sq2), c.squares(), "squares")
    ev.check()


# ---- 4: one small case per kernel body ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,spec,groups,env", [
    ("packed FP64, 4 primes", "default_8192", 2, {}),
    ("unit-test set", "seal_fhe_unit", 2, {}),
    ("mixed base", BITS54, 2, {}),
    ("8 primes, per-row packing", "default_16384", 1, {}),
    ("8 primes, 8-byte rows", "default_16384", 1, {"HIPBFV_PACK_ROWS": "0"}),
    ("integer base", "default_4096", 2, {"HIPBFV_NO_F64": "1"}),
])
def test_every_body_of_the_summing_tail(name, spec, groups, env, monkeypatch):
    c = _case(spec, groups, 3)
    ctx, ev, rkd, da, db = _device(c, monkeypatch, env)
    seen3, seen2 = _run_both(c, ev, rkd, da, db, c.sums(), name)
    for seen in (seen3, seen2):
        assert seen.get("mul_tail_sum") == 1 and "mul_tail" not in seen and "behz_floor_sk" not in seen, (name, seen)


def test_the_lane_split_geometry_build_gives_the_same_bits():
    """libhipbfv_geom8.so (`make variants`: the N/8-block geometry of n = 16384) in a process of its own, as
    tests/test_gpu_properties.py loads it: the words of the default build's case above, hence the oracle's."""
    lib = os.path.join(ROOT, "sunscreen_amd", "lib", "variants", "libhipbfv_geom8.so")
    assert os.path.exists(lib), "build the variant library first: make -C sunscreen_amd/csrc variants (build() does)"
    c = _case("default_16384", 1, 3)
    script = r"""
import sys, numpy as np, torch
sys.path.insert(0, %r)
from sunscreen_amd import Context, RelinearizationKeys
from sunscreen_amd.batch import BatchEvaluator, to_device, to_host
z = np.load(sys.argv[1])
ctx = Context.from_raw(int(z["n"]), [int(p) for p in z["primes"]], int(z["t"]))
ev = BatchEvaluator(ctx)
ev.profile(True)
a, b = to_device(z["a"]), to_device(z["b"])
out3 = ev.multiply_sum(a, b)
out2 = ev.multiply_sum_relin(a, b, RelinearizationKeys.from_array(ctx, z["rk"]))
torch.cuda.synchronize()
seen = ev.profile_read()
assert seen["mul_tail_sum"]["launches"] == 2 and "mul_tail" not in seen, seen
ev.check()
np.savez(sys.argv[2], out3=to_host(out3), out2=to_host(out2))
""" % ROOT
    with tempfile.TemporaryDirectory() as td:
        src, dst = os.path.join(td, "in.npz"), os.path.join(td, "out.npz")
        np.savez(src, n=c.n, primes=np.array(c.primes, dtype=np.uint64), t=c.t, a=c.a, b=c.b, rk=c.rk)
        subprocess.check_call([sys.executable, "-c", script, src, dst], env=dict(os.environ, HIPBFV_LIB=lib, HIPBFV_NO_SMALL_BATCH="1"))
        got = np.load(dst)
        c.check(got["out3"], got["out2"], c.sums(), "geom8")


# ---- 5: the non-split path --------------------------------------------------------------------------------------------------
def test_below_the_split_kernels_the_terms_are_folded(monkeypatch):
    c = _case(UNIT1024, 2, 3)
    ctx, ev, rkd, da, db = _device(c, monkeypatch)
    seen3, seen2 = _run_both(c, ev, rkd, da, db, c.sums(), "n = 1024")
    for seen in (seen3, seen2):
        assert "mul_tail_sum" not in seen and seen.get("behz_floor_sk") == 1 and seen.get("eltwise") == 2 * (3 - 1), seen


def test_a_few_items_take_the_whole_polynomial_multiply(monkeypatch):
    """default_8192, 2 x 3 = 6 items, at most the few-operations threshold, WITHOUT HIPBFV_NO_SMALL_BATCH: the same bits as the
    split path's case above (both are the oracle's)."""
    monkeypatch.delenv("HIPBFV_NO_SMALL_BATCH", raising=False)
    c = _case("default_8192", 2, 3)
    ctx, ev, rkd, da, db = _device(c, monkeypatch, small_batch=True)
    seen3, seen2 = _run_both(c, ev, rkd, da, db, c.sums(), "few items")
    for seen in (seen3, seen2):
        assert "mul_tail_sum" not in seen and "mul_tail" not in seen and seen.get("eltwise") == 4, seen


def test_the_folded_path_slices_a_long_group_too(monkeypatch):
    """n = 1024 with a chunk of 2 items: slices of 2 and 1 terms per group, the later slice added onto the first one's sums."""
    from sunscreen_amd.batch import to_host

    c = _case(UNIT1024, 2, 3)
    ctx, ev, rkd, da, db = _device(c, monkeypatch)
    ev.set_chunk_ops(2)
    out3, seen = _profiled(ev, lambda: ev.multiply_sum(da, db))
    assert seen.get("behz_floor_sk") == 4 and seen.get("eltwise") == 4 and "mul_tail_sum" not in seen, seen
    c.check(to_host(out3), None, c.sums(), "folded slices")
    ev.check()


# ---- 6: one key set per group -----------------------------------------------------------------------------------------------
def test_every_group_through_its_own_key_set(monkeypatch):
    import torch
    from sunscreen_amd import RelinearizationKeys
    from sunscreen_amd.batch import to_host

    c = _case("default_4096", 3, 5)
    ctx, ev, rkd_a, da, db = _device(c, monkeypatch)
    # a second client's relinearization key for the same secret would give the same plaintexts and other words: made from the
    # oracle under another seed (the key's randomness differs, the secret key does not matter for the word-for-word comparison)
    O.seed(77)
    rk_b = c.o.keygen()[2]
    rkd_b = RelinearizationKeys.from_array(ctx, rk_b)
    assert not (rk_b == c.rk).all()
    sets, index = [rkd_a, rkd_b, None], [1, 0, 1]
    out, seen = _profiled(ev, lambda: ev.multiply_sum_relin_keys(da, db, sets, index))
    assert seen.get("mul_tail_sum") == 1, seen
    single = {0: ev.multiply_sum_relin(da, db, rkd_a), 1: ev.multiply_sum_relin(da, db, rkd_b)}
    ref3 = c.sums()[0]
    host = to_host(out)
    for g, k in enumerate(index):
        assert torch.equal(out[g], single[k][g]), (g, k)
        assert (host[g] == c.o.relinearize(ref3[g], [c.rk, rk_b][k])).all(), (g, k)
    ev.set_chunk_ops(7)  # one group per chunk: the key selection follows the groups
    assert torch.equal(ev.multiply_sum_relin_keys(da, db, sets, index), out)
    ev.check()
    sentinel = torch.full_like(out, SENTINEL)
    hr, msg = _hr(lambda: ev.multiply_sum_relin_keys(da, db, sets, [2, 0, 1], out=sentinel))
    assert hr == E_INVALIDARG and "key set 2" in msg, (hex(hr), msg)
    torch.cuda.synchronize()
    assert (sentinel == SENTINEL).all()


# ---- 7: refusals launch nothing ---------------------------------------------------------------------------------------------
def test_refusals_come_before_any_launch_or_write(monkeypatch):
    import torch
    from sunscreen_amd import RelinearizationKeys, _lib
    from sunscreen_amd.batch import _ptr, _stream

    c = _case("default_4096", 3, 5)
    ctx, ev, rkd, da, db = _device(c, monkeypatch)
    L = _lib.load()
    h = ev._h
    K, n = ctx.K, c.n
    item = 2 * K * n
    # the operands inside one allocation with room after them, so that outputs can be laid over them
    buf = torch.full((3 * 5 * item + 3 * 3 * K * n + item,), SENTINEL, dtype=torch.int64, device="cuda")
    buf[: 15 * item] = da.reshape(-1)
    a_in = buf[: 15 * item].view(3, 5, 2, K, n)
    out3 = torch.full((3, 3, K, n), SENTINEL, dtype=torch.int64, device="cuda")
    out2 = torch.full((3, 2, K, n), SENTINEL, dtype=torch.int64, device="cuda")
    idx = (C.c_uint32 * 3)(0, 0, 3)
    hs = (C.c_void_p * 1)(rkd.get_handle())
    over_start = buf[: 9 * K * n].view(3, 3, K, n)
    over_shift = buf[item: item + 9 * K * n].view(3, 3, K, n)
    over_tail2 = buf[14 * item: 14 * item + 6 * K * n].view(3, 2, K, n)
    empty = RelinearizationKeys()  # a key object that holds no key: what hipbfv_batch_relinearize answers is the status to expect
    no_key = _hr(lambda: ev.relinearize(torch.zeros_like(out3), empty))[0]
    assert no_key != 0
    calls = [
        ("terms = 0", lambda: L.hipbfv_batch_multiply_sum(h, _ptr(da), _ptr(db), _ptr(out3), 3, 0, _stream()), E_INVALIDARG),
        ("terms = 0, relin", lambda: L.hipbfv_batch_multiply_sum_relin(h, _ptr(da), _ptr(db), rkd.get_handle(), _ptr(out2), 3, 0, _stream()), E_INVALIDARG),
        ("out over a", lambda: L.hipbfv_batch_multiply_sum(h, _ptr(a_in), _ptr(db), _ptr(over_start), 3, 5, _stream()), E_INVALIDARG),
        ("out over a + 1 item", lambda: L.hipbfv_batch_multiply_sum(h, _ptr(a_in), _ptr(db), _ptr(over_shift), 3, 5, _stream()), E_INVALIDARG),
        ("out over b", lambda: L.hipbfv_batch_multiply_sum(h, _ptr(db), _ptr(a_in), _ptr(over_shift), 3, 5, _stream()), E_INVALIDARG),
        ("out2 over a's last item", lambda: L.hipbfv_batch_multiply_sum_relin(h, _ptr(a_in), _ptr(db), rkd.get_handle(), _ptr(over_tail2), 3, 5, _stream()),
         E_INVALIDARG),
        ("NULL b", lambda: L.hipbfv_batch_multiply_sum(h, _ptr(da), None, _ptr(out3), 3, 5, _stream()), E_POINTER),
        ("NULL b, relin", lambda: L.hipbfv_batch_multiply_sum_relin(h, _ptr(da), None, rkd.get_handle(), _ptr(out2), 3, 5, _stream()), E_POINTER),
        ("NULL out", lambda: L.hipbfv_batch_multiply_sum(h, _ptr(da), _ptr(db), None, 3, 5, _stream()), E_POINTER),
        ("no relin key", lambda: L.hipbfv_batch_multiply_sum_relin(h, _ptr(da), _ptr(db), empty.get_handle(), _ptr(out2), 3, 5, _stream()), no_key),
        ("NULL key object", lambda: L.hipbfv_batch_multiply_sum_relin(h, _ptr(da), _ptr(db), None, _ptr(out2), 3, 5, _stream()), no_key),
        ("key_index out of range", lambda: L.hipbfv_batch_multiply_sum_relin_keys(h, _ptr(da), _ptr(db), hs, 1, idx, _ptr(out2), 3, 5, _stream()), E_INVALIDARG),
        ("NULL key table", lambda: L.hipbfv_batch_multiply_sum_relin_keys(h, _ptr(da), _ptr(db), None, 1, idx, _ptr(out2), 3, 5, _stream()), E_POINTER),
    ]
    before = buf.clone()
    ev.profile(True)
    ev.profile_reset()
    try:
        for what, call, want in calls:
            got = call() & 0xFFFFFFFF
            assert got == want, (what, hex(got), hex(want))
        # an empty call is accepted and launches nothing either
        assert L.hipbfv_batch_multiply_sum(h, _ptr(da), _ptr(db), _ptr(out3), 0, 5, _stream()) == 0
        assert L.hipbfv_batch_multiply_sum_relin(h, _ptr(da), _ptr(db), rkd.get_handle(), _ptr(out2), 0, 5, _stream()) == 0
        torch.cuda.synchronize()
        assert ev.profile_read() == {}, ev.profile_read()
    finally:
        ev.profile(False)
    assert torch.equal(buf, before) and (out3 == SENTINEL).all() and (out2 == SENTINEL).all()
    assert torch.equal(da, a_in)
    ev.check()


# ---- 8: transparent results -------------------------------------------------------------------------------------------------
def test_a_transparent_sum_is_reported_under_its_group_number(monkeypatch):
    """Every term of group 1 is a product of two transparent ciphertexts (c1 = 0 in both factors), so the group's sum has c1 = c2 = 0:
    hipbfv_batch_status names item 1, for the size-3 sum and for its relinearization.  A clean call reports nothing."""
    from sunscreen_amd import _lib
    from sunscreen_amd.batch import _stream

    c = _case("default_4096", 3, 5)
    ctx, ev, rkd, da, db = _device(c, monkeypatch)
    ta, tb = da.clone(), db.clone()
    ta[1, :, 1] = 0
    tb[1, :, 1] = 0
    L = _lib.load()
    first = C.c_uint64(123)
    for call in (lambda: ev.multiply_sum(ta, tb), lambda: ev.multiply_sum_relin(ta, tb, rkd)):
        call()
        hr, msg = _hr(ev.check)
        assert hr == COR_E_INVALIDOPERATION and "item 1)" in msg, (hex(hr), msg)
        ev.check()  # (the read above reset the word: clean again)
        call()
        assert L.hipbfv_batch_status(ev._h, C.byref(first), _stream()) & 0xFFFFFFFF == COR_E_INVALIDOPERATION and first.value == 1
    ev.multiply_sum(da, db)
    ev.multiply_sum_relin(da, db, rkd)
    assert L.hipbfv_batch_status(ev._h, C.byref(first), _stream()) == 0 and first.value == 2**64 - 1
