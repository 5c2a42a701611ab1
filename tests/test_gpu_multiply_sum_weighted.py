"""Weighted sums of products with one relinearization per group: hipbfv_batch_multiply_sum_weighted / _relin / _relin_keys.

out3[g] = sum_t w_t (.) multiply(a[g][t], b[g][t]), where w (.) c multiplies every word of residue row i by (w mod q_i), canonical,
mod q_i.  The reference is the CPU oracle's `multiply` of every term, each row scaled in Python integers, folded with the oracle's
`add` and relinearized by the oracle; for |w| <= 3 the scaling is also asserted to be the oracle's own repeated `add` after `negate`,
which pins the definition to the oracle.  Decoded slots are checked against sum_t w_t * va_t * vb_t mod t for small weights only, on
sets where the oracle's own sequence keeps noise budget (`noise_budget` of the reference result, measured on the CPU: 18 bits for
(1, -1, 3, -2, 1) over 5 terms at default_4096, 18 for the squares with (2, -1, 1), 120 for the determinant at default_8192, and for
(1, -1, 2): 19 at default_4096, 75 at seal_fhe_unit, 104 at n = 1024, 107 at 3 x 54 bits, 119 at default_8192, 334 at default_16384)."""
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
INT32_MIN = -(2**31)


class _Case:
    """One parameter set, one key pair, groups x terms fresh encryptions of small slot vectors per operand, the oracle's product of
    every term (computed once) and, per weight vector, the reference sums -- shared by the tests that name the same case."""

    def __init__(self, spec, groups, terms, seed):
        n, primes, t = params(spec) if isinstance(spec, str) else spec
        self.n, self.primes, self.t = n, list(primes), t
        self.K = len(self.primes) - 1
        self.groups, self.terms = groups, terms
        self.o = O.Oracle(n, self.primes, t)
        O.seed(seed)
        self.sk, self.pk, self.rk, _ = self.o.keygen()
        rng = np.random.default_rng(seed)
        self.va = rng.integers(0, 40, (groups, terms, n)).astype(np.uint64)
        self.vb = rng.integers(0, 40, (groups, terms, n)).astype(np.uint64)
        enc = lambda v: self.o.encrypt(self.pk, self.o.batch_encode(v))  # noqa: E731
        self.a = np.stack([np.stack([enc(self.va[g, j]) for j in range(terms)]) for g in range(groups)])
        self.b = np.stack([np.stack([enc(self.vb[g, j]) for j in range(terms)]) for g in range(groups)])
        self._products, self._refs = {}, {}

    def _product(self, key, b, g, j):
        if (key, g, j) not in self._products:
            self._products[(key, g, j)] = self.o.multiply(self.a[g, j], b[g, j])
        return self._products[(key, g, j)]

    def scale(self, ct, w):
        """w (.) ct in Python integers: row i of every polynomial times (w mod q_i) mod q_i."""
        out = np.empty_like(ct)
        for i in range(self.K):
            q = self.primes[i]
            out[:, i] = ((ct[:, i].astype(object) * (w % q)) % q).astype(np.uint64)
        return out

    def _scaled(self, prod, w):
        s = self.scale(prod, w)
        if 0 < abs(w) <= 3:  # the definition, pinned to the oracle: |w| additions of the (negated) product
            base = self.o.negate(prod) if w < 0 else prod
            rep = base
            for _ in range(abs(w) - 1):
                rep = self.o.add(rep, base)
            assert (rep == s).all(), ("scaling differs from the oracle's repeated add", w)
        return s

    def sums(self, weights, squares=False):
        """(ref3, ref2, slots): the reference size-3 sums, the oracle's relinearizations of them and the expected slots, per group."""
        key = ("aa" if squares else "ab", tuple(weights))
        if key not in self._refs:
            b, vb = (self.a, self.va) if squares else (self.b, self.vb)
            ref3, ref2, slots = [], [], []
            for g in range(self.groups):
                acc = None
                for j, w in enumerate(weights):
                    s = self._scaled(self._product(key[0], b, g, j), w)
                    acc = s if acc is None else self.o.add(acc, s)
                ref3.append(acc)
                ref2.append(self.o.relinearize(acc, self.rk))
                wv = np.array([int(w) for w in weights], dtype=object)[:, None]
                slots.append((wv * self.va[g].astype(object) * vb[g].astype(object)).sum(axis=0) % self.t)
            self._refs[key] = (np.stack(ref3), np.stack(ref2), np.stack(slots).astype(np.uint64))
        return self._refs[key]

    def check(self, out3, out2, refs, what, decode=True):
        ref3, ref2, slots = refs
        for g in range(self.groups):
            if out3 is not None:
                assert (out3[g] == ref3[g]).all(), (what, "size 3", g)
            if out2 is not None:
                assert (out2[g] == ref2[g]).all(), (what, "relinearized", g)
                if decode:
                    assert (self.o.batch_decode(self.o.decrypt(out2[g], self.sk)) == slots[g]).all(), (what, "slots", g)


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


def _device(c, monkeypatch, env=None, small_batch=False):
    from sunscreen_amd import Context, RelinearizationKeys
    from sunscreen_amd.batch import BatchEvaluator, to_device

    for k, v in (env or {}).items():
        monkeypatch.setenv(k, v)
    if not small_batch:
        monkeypatch.setenv("HIPBFV_NO_SMALL_BATCH", "1")
    ctx = Context.from_raw(c.n, c.primes, c.t)
    ev = BatchEvaluator(ctx)
    return ctx, ev, RelinearizationKeys.from_array(ctx, c.rk), to_device(c.a), to_device(c.b)


def _run_both(c, ev, rkd, da, db, weights, what, decode=True, squares=False):
    """multiply_sum_weighted and its relinearizing form of one case, checked; the kernels both calls launched."""
    from sunscreen_amd.batch import to_host

    refs = c.sums(weights, squares)
    out3, seen3 = _profiled(ev, lambda: ev.multiply_sum_weighted(da, db, weights))
    out2, seen2 = _profiled(ev, lambda: ev.multiply_sum_weighted_relin(da, db, weights, rkd))
    c.check(to_host(out3), to_host(out2), refs, what, decode)
    ev.check()
    return seen3, seen2


# ---- 1: chunks and slices ---------------------------------------------------------------------------------------------------
def test_chunks_whole_groups_and_slices_give_the_same_bits(monkeypatch):
    """default_4096, 3 groups x 5 terms, weights (1, -1, 3, -2, 1): one launch at the default chunk, one group per chunk at 7 items,
    slices of 2, 2 and 1 terms at 2 items -- a slice that starts at term0 reads the weight table from row term0."""
    import torch
    from sunscreen_amd.batch import to_host

    weights = (1, -1, 3, -2, 1)
    c = _case("default_4096", 3, 5)
    ctx, ev, rkd, da, db = _device(c, monkeypatch)
    refs = c.sums(weights)
    first = None
    for chunk, launches in ((None, 1), (7, 3), (2, 9)):
        if chunk:
            ev.set_chunk_ops(chunk)
        before = (da.clone(), db.clone())
        out3, seen = _profiled(ev, lambda: ev.multiply_sum_weighted(da, db, weights))
        assert seen.get("mul_tail_sum") == launches and "mul_tail" not in seen and "eltwise" not in seen, (chunk, seen)
        assert seen.get("mul_head") == launches, (chunk, seen)
        out2, seen = _profiled(ev, lambda: ev.multiply_sum_weighted_relin(da, db, weights, rkd))
        assert seen.get("mul_tail_sum") == launches and "mul_tail" not in seen and "eltwise" not in seen, (chunk, seen)
        assert torch.equal(da, before[0]) and torch.equal(db, before[1]), "an operand changed"
        c.check(to_host(out3), to_host(out2), refs, chunk)
        if first is None:
            first = (out3, out2)
        assert torch.equal(out3, first[0]) and torch.equal(out2, first[1]), chunk
        ev.check()


# ---- 2: all weights 1 -------------------------------------------------------------------------------------------------------
def test_all_weights_one_is_the_unweighted_call(monkeypatch):
    import torch

    c = _case("default_4096", 3, 5)
    ctx, ev, rkd, da, db = _device(c, monkeypatch)
    ones = [1] * 5
    for weighted, plain in ((lambda: ev.multiply_sum_weighted(da, db, ones), lambda: ev.multiply_sum(da, db)),
                            (lambda: ev.multiply_sum_weighted_relin(da, db, ones, rkd), lambda: ev.multiply_sum_relin(da, db, rkd))):
        got, seen_w = _profiled(ev, weighted)
        want, seen_p = _profiled(ev, plain)
        assert torch.equal(got, want) and seen_w == seen_p, (seen_w, seen_p)
    a1, b1 = da[:, :1].contiguous(), db[:, :1].contiguous()
    assert torch.equal(ev.multiply_sum_weighted(a1, b1, [1]), ev.multiply(a1[:, 0].contiguous(), b1[:, 0].contiguous()))
    assert torch.equal(ev.multiply_sum_weighted_relin(a1, b1, [1], rkd), ev.multiply_relin(a1[:, 0].contiguous(), b1[:, 0].contiguous(), rkd))
    ev.check()


# ---- 3: extreme weights -----------------------------------------------------------------------------------------------------
def test_extreme_weights_give_the_reference_words(monkeypatch):
    """(2^31 - 1, INT32_MIN, 0): words only -- such weights multiply the noise past the budget, nothing decodes."""
    c = _case("default_4096", 2, 3)
    ctx, ev, rkd, da, db = _device(c, monkeypatch)
    seen3, seen2 = _run_both(c, ev, rkd, da, db, (2**31 - 1, INT32_MIN, 0), "extreme", decode=False)
    assert seen3.get("mul_tail_sum") == 1 and seen2.get("mul_tail_sum") == 1, (seen3, seen2)


# ---- 4: signs only ----------------------------------------------------------------------------------------------------------
def test_a_determinant_at_8192(monkeypatch):
    """ad - bc: 2 groups x 2 terms, weights (1, -1), words and slots."""
    c = _case("default_8192", 2, 2)
    ctx, ev, rkd, da, db = _device(c, monkeypatch)
    seen3, seen2 = _run_both(c, ev, rkd, da, db, (1, -1), "determinant")
    for seen in (seen3, seen2):
        assert seen.get("mul_tail_sum") == 1 and "mul_tail" not in seen and "eltwise" not in seen, seen


# ---- 5: squares -------------------------------------------------------------------------------------------------------------
def test_weighted_squares_through_the_same_pointer_equal_the_call_with_a_copy(monkeypatch):
    import torch
    from sunscreen_amd.batch import to_host

    weights = (2, -1, 1)
    c = _case("default_4096", 2, 3)
    ctx, ev, rkd, da, _ = _device(c, monkeypatch)
    copy = da.clone()
    sq3, seen = _profiled(ev, lambda: ev.multiply_sum_weighted(da, da, weights))
    assert seen.get("mul_tail_sum") == 1 and "mul_tail" not in seen, seen
    sq2 = ev.multiply_sum_weighted_relin(da, da, weights, rkd)
    assert torch.equal(sq3, ev.multiply_sum_weighted(da, copy, weights)) and torch.equal(sq2, ev.multiply_sum_weighted_relin(da, copy, weights, rkd))
    c.check(to_host(sq3), to_host(sq2), c.sums(weights, squares=True), "squares")
    ev.check()


# ---- 6: one small case per kernel body --------------------------------------------------------------------------------------
BODY_WEIGHTS = (1, -1, 2)


@pytest.mark.parametrize("name,spec,groups,env", [
    ("packed FP64, 4 primes", "default_8192", 2, {}),
    ("unit-test set", "seal_fhe_unit", 2, {}),
    ("mixed base", BITS54, 2, {}),
    ("8 primes, per-row packing", "default_16384", 1, {}),
    ("8 primes, 8-byte rows", "default_16384", 1, {"HIPBFV_PACK_ROWS": "0"}),
    ("integer base", "default_4096", 2, {"HIPBFV_NO_F64": "1"}),
])
def test_every_body_of_the_weighted_summing_tail(name, spec, groups, env, monkeypatch):
    c = _case(spec, groups, 3)
    ctx, ev, rkd, da, db = _device(c, monkeypatch, env)
    seen3, seen2 = _run_both(c, ev, rkd, da, db, BODY_WEIGHTS, name)
    for seen in (seen3, seen2):
        assert seen.get("mul_tail_sum") == 1 and "mul_tail" not in seen and "behz_floor_sk" not in seen and "eltwise" not in seen, (name, seen)


# ---- 7: the lane-split geometry build ---------------------------------------------------------------------------------------
def test_the_lane_split_geometry_build_gives_the_same_bits():
    """libhipbfv_geom8.so in a process of its own: the words of case 6's default_16384."""
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
a, b, w = to_device(z["a"]), to_device(z["b"]), [int(x) for x in z["w"]]
out3 = ev.multiply_sum_weighted(a, b, w)
out2 = ev.multiply_sum_weighted_relin(a, b, w, RelinearizationKeys.from_array(ctx, z["rk"]))
torch.cuda.synchronize()
seen = ev.profile_read()
assert seen["mul_tail_sum"]["launches"] == 2 and "mul_tail" not in seen and "eltwise" not in seen, seen
ev.check()
np.savez(sys.argv[2], out3=to_host(out3), out2=to_host(out2))
""" % ROOT
    with tempfile.TemporaryDirectory() as td:
        src, dst = os.path.join(td, "in.npz"), os.path.join(td, "out.npz")
        np.savez(src, n=c.n, primes=np.array(c.primes, dtype=np.uint64), t=c.t, a=c.a, b=c.b, rk=c.rk, w=np.array(BODY_WEIGHTS, dtype=np.int64))
        subprocess.check_call([sys.executable, "-c", script, src, dst], env=dict(os.environ, HIPBFV_LIB=lib, HIPBFV_NO_SMALL_BATCH="1"))
        got = np.load(dst)
        c.check(got["out3"], got["out2"], c.sums(BODY_WEIGHTS), "geom8")


# ---- 8: the folded path -----------------------------------------------------------------------------------------------------
def test_below_the_split_kernels_the_terms_are_folded_with_their_weights(monkeypatch):
    c = _case(UNIT1024, 2, 3)
    ctx, ev, rkd, da, db = _device(c, monkeypatch)
    seen3, seen2 = _run_both(c, ev, rkd, da, db, BODY_WEIGHTS, "n = 1024")
    for seen in (seen3, seen2):
        # one scaled accumulate per term and group (the unweighted fold adds terms - 1 times: its first term needs no pass)
        assert "mul_tail_sum" not in seen and seen.get("behz_floor_sk") == 1 and seen.get("eltwise") == 2 * 3, seen


def test_a_few_items_take_the_whole_polynomial_multiply(monkeypatch):
    monkeypatch.delenv("HIPBFV_NO_SMALL_BATCH", raising=False)
    c = _case("default_8192", 2, 3)
    ctx, ev, rkd, da, db = _device(c, monkeypatch, small_batch=True)
    seen3, seen2 = _run_both(c, ev, rkd, da, db, BODY_WEIGHTS, "few items")
    for seen in (seen3, seen2):
        assert "mul_tail_sum" not in seen and "mul_tail" not in seen and seen.get("eltwise") == 6, seen


def test_the_folded_path_slices_a_long_group_too(monkeypatch):
    """n = 1024 with a chunk of 2 items: slices of 2 and 1 terms per group; the later slice reads the table from row 2 and adds on."""
    from sunscreen_amd.batch import to_host

    c = _case(UNIT1024, 2, 3)
    ctx, ev, rkd, da, db = _device(c, monkeypatch)
    ev.set_chunk_ops(2)
    out3, seen = _profiled(ev, lambda: ev.multiply_sum_weighted(da, db, BODY_WEIGHTS))
    assert seen.get("behz_floor_sk") == 4 and seen.get("eltwise") == 6 and "mul_tail_sum" not in seen, seen
    out2 = ev.multiply_sum_weighted_relin(da, db, BODY_WEIGHTS, rkd)
    c.check(to_host(out3), to_host(out2), c.sums(BODY_WEIGHTS), "folded slices")
    ev.check()


# ---- 9: one key set per group -----------------------------------------------------------------------------------------------
def test_every_group_through_its_own_key_set(monkeypatch):
    import torch
    from sunscreen_amd import RelinearizationKeys
    from sunscreen_amd.batch import to_host

    weights = (1, -1, 3, -2, 1)
    c = _case("default_4096", 3, 5)
    ctx, ev, rkd_a, da, db = _device(c, monkeypatch)
    O.seed(77)
    rk_b = c.o.keygen()[2]
    rkd_b = RelinearizationKeys.from_array(ctx, rk_b)
    assert not (rk_b == c.rk).all()
    sets, index = [rkd_a, rkd_b, None], [1, 0, 1]
    out, seen = _profiled(ev, lambda: ev.multiply_sum_weighted_relin_keys(da, db, weights, sets, index))
    assert seen.get("mul_tail_sum") == 1, seen
    single = {0: ev.multiply_sum_weighted_relin(da, db, weights, rkd_a), 1: ev.multiply_sum_weighted_relin(da, db, weights, rkd_b)}
    ref3 = c.sums(weights)[0]
    host = to_host(out)
    for g, k in enumerate(index):
        assert torch.equal(out[g], single[k][g]), (g, k)
        assert (host[g] == c.o.relinearize(ref3[g], [c.rk, rk_b][k])).all(), (g, k)
    ev.set_chunk_ops(7)  # one group per chunk: the key selection follows the groups, the weight table is staged once
    assert torch.equal(ev.multiply_sum_weighted_relin_keys(da, db, weights, sets, index), out)
    ev.check()


# ---- 10: refusals launch nothing --------------------------------------------------------------------------------------------
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
    buf = torch.full((3 * 5 * item + 3 * 3 * K * n + item,), SENTINEL, dtype=torch.int64, device="cuda")
    buf[: 15 * item] = da.reshape(-1)
    a_in = buf[: 15 * item].view(3, 5, 2, K, n)
    out3 = torch.full((3, 3, K, n), SENTINEL, dtype=torch.int64, device="cuda")
    out2 = torch.full((3, 2, K, n), SENTINEL, dtype=torch.int64, device="cuda")
    w = (C.c_int32 * 5)(1, -1, 3, -2, 1)
    idx = (C.c_uint32 * 3)(0, 0, 3)
    ok_idx = (C.c_uint32 * 3)(0, 0, 0)
    hs = (C.c_void_p * 1)(rkd.get_handle())
    none = (C.c_void_p * 1)(None)
    over_start = buf[: 9 * K * n].view(3, 3, K, n)
    over_shift = buf[item: item + 9 * K * n].view(3, 3, K, n)
    over_tail2 = buf[14 * item: 14 * item + 6 * K * n].view(3, 2, K, n)
    empty = RelinearizationKeys()
    no_key = _hr(lambda: ev.relinearize(torch.zeros_like(out3), empty))[0]
    assert no_key != 0
    S, SR, SK = L.hipbfv_batch_multiply_sum_weighted, L.hipbfv_batch_multiply_sum_weighted_relin, L.hipbfv_batch_multiply_sum_weighted_relin_keys
    calls = [
        ("NULL weights", lambda: S(h, _ptr(da), _ptr(db), None, _ptr(out3), 3, 5, _stream()), E_POINTER),
        ("NULL weights, relin", lambda: SR(h, _ptr(da), _ptr(db), None, rkd.get_handle(), _ptr(out2), 3, 5, _stream()), E_POINTER),
        ("NULL weights, keys", lambda: SK(h, _ptr(da), _ptr(db), None, hs, 1, ok_idx, _ptr(out2), 3, 5, _stream()), E_POINTER),
        ("terms = 0", lambda: S(h, _ptr(da), _ptr(db), w, _ptr(out3), 3, 0, _stream()), E_INVALIDARG),
        ("terms = 0, relin", lambda: SR(h, _ptr(da), _ptr(db), w, rkd.get_handle(), _ptr(out2), 3, 0, _stream()), E_INVALIDARG),
        ("out over a", lambda: S(h, _ptr(a_in), _ptr(db), w, _ptr(over_start), 3, 5, _stream()), E_INVALIDARG),
        ("out over a + 1 item", lambda: S(h, _ptr(a_in), _ptr(db), w, _ptr(over_shift), 3, 5, _stream()), E_INVALIDARG),
        ("out over b", lambda: S(h, _ptr(db), _ptr(a_in), w, _ptr(over_shift), 3, 5, _stream()), E_INVALIDARG),
        ("out2 over a's last item", lambda: SR(h, _ptr(a_in), _ptr(db), w, rkd.get_handle(), _ptr(over_tail2), 3, 5, _stream()), E_INVALIDARG),
        ("NULL b", lambda: S(h, _ptr(da), None, w, _ptr(out3), 3, 5, _stream()), E_POINTER),
        ("NULL out", lambda: S(h, _ptr(da), _ptr(db), w, None, 3, 5, _stream()), E_POINTER),
        ("no relin key", lambda: SR(h, _ptr(da), _ptr(db), w, empty.get_handle(), _ptr(out2), 3, 5, _stream()), no_key),
        ("NULL key object", lambda: SR(h, _ptr(da), _ptr(db), w, None, _ptr(out2), 3, 5, _stream()), no_key),
        ("key_index out of range", lambda: SK(h, _ptr(da), _ptr(db), w, hs, 1, idx, _ptr(out2), 3, 5, _stream()), E_INVALIDARG),
        ("a referenced key set is missing", lambda: SK(h, _ptr(da), _ptr(db), w, none, 1, ok_idx, _ptr(out2), 3, 5, _stream()), None),
        ("NULL key table", lambda: SK(h, _ptr(da), _ptr(db), w, None, 1, idx, _ptr(out2), 3, 5, _stream()), E_POINTER),
    ]
    before = buf.clone()
    ev.profile(True)
    ev.profile_reset()
    try:
        for what, call, want in calls:
            got = call() & 0xFFFFFFFF
            if want is None:  # the status of the unweighted call for the same missing set
                want = L.hipbfv_batch_multiply_sum_relin_keys(h, _ptr(da), _ptr(db), none, 1, ok_idx, _ptr(out2), 3, 5, _stream()) & 0xFFFFFFFF
                assert want != 0
            assert got == want, (what, hex(got), hex(want))
        assert S(h, _ptr(da), _ptr(db), w, _ptr(out3), 0, 5, _stream()) == 0
        assert SR(h, _ptr(da), _ptr(db), w, rkd.get_handle(), _ptr(out2), 0, 5, _stream()) == 0
        torch.cuda.synchronize()
        assert ev.profile_read() == {}, ev.profile_read()
    finally:
        ev.profile(False)
    assert torch.equal(buf, before) and (out3 == SENTINEL).all() and (out2 == SENTINEL).all()
    assert torch.equal(da, a_in)
    ev.check()


# ---- 11: transparent results ------------------------------------------------------------------------------------------------
def test_weights_that_cancel_equal_terms_are_reported_under_the_group_number(monkeypatch):
    """Group 1 holds the same term twice; weights (1, -1) cancel it to the all-zero ciphertext, whose c1 = c2 = 0: hipbfv_batch_status
    names item 1 for the size-3 sum and for its relinearization.  The other groups differ in their terms and report nothing."""
    from sunscreen_amd import _lib
    from sunscreen_amd.batch import _stream

    c = _case("default_8192", 2, 2)
    ctx, ev, rkd, da, db = _device(c, monkeypatch)
    ta, tb = da.clone(), db.clone()
    ta[1, 1] = ta[1, 0]
    tb[1, 1] = tb[1, 0]
    L = _lib.load()
    first = C.c_uint64(123)
    for call in (lambda: ev.multiply_sum_weighted(ta, tb, (1, -1)), lambda: ev.multiply_sum_weighted_relin(ta, tb, (1, -1), rkd)):
        out = call()
        assert not out[1].any() and out[0].any()
        hr, msg = _hr(ev.check)
        assert hr == COR_E_INVALIDOPERATION and "item 1)" in msg, (hex(hr), msg)
        ev.check()
        call()
        assert L.hipbfv_batch_status(ev._h, C.byref(first), _stream()) & 0xFFFFFFFF == COR_E_INVALIDOPERATION and first.value == 1
    ev.multiply_sum_weighted(ta, tb, (0, 0))  # all-zero weights: every group is transparent, the first one is named
    assert L.hipbfv_batch_status(ev._h, C.byref(first), _stream()) & 0xFFFFFFFF == COR_E_INVALIDOPERATION and first.value == 0
    ev.multiply_sum_weighted(da, db, (1, -1))
    ev.multiply_sum_weighted_relin(da, db, (1, -1), rkd)
    assert L.hipbfv_batch_status(ev._h, C.byref(first), _stream()) == 0 and first.value == 2**64 - 1
