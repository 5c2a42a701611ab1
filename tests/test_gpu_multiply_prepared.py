"""Products of two prepared operands: hipbfv_batch_multiply_prepared / _relin_prepared / _sum_prepared / _sum_relin_prepared.

Item i multiplies prepared ciphertext a_index[i % index_len] of one object by b_index[i % index_len] of another (i = g * terms + t in the
sum forms; the two objects may be one).  Every output must be, word for word, the CPU oracle's `multiply` (folded with `add`, then
`relinearize`) of the two named ciphertexts, and equal the library's own counterpart call on the two gathered arrays; decrypted and
decoded it must give the slot products.  On the split path there is no head at all -- one `mul_mid` launch reads both operands' rows --
elsewhere both operands are gathered from the objects' copies.  The parameter sets are those of test_gpu_multiply_shared.py, on which
three terms are established to leave noise budget; each oracle product and sum is asserted to decode before the GPU is compared with it."""
import ctypes as C
import os
import subprocess
import sys
import tempfile

import numpy as np
import pytest

from oracle import bfv_oracle as O
from tests.bfv_helpers import params
from tests.test_gpu_multiply_shared import _profiled
from tests.test_gpu_multiply_sum import BITS54, COR_E_INVALIDOPERATION, E_INVALIDARG, E_POINTER, SENTINEL, UNIT1024, _hr

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
AIDX = [0, 1, 2, 2, 0, 1]
BIDX = [0, 1, 0, 1, 1, 0]


class _Case:
    """One parameter set, one key pair, `na` fresh encryptions for the first object and `nb` for the second, and the oracle's products --
    each computed once and shared by the tests that name the same case."""

    def __init__(self, spec, na, nb, seed=8209):
        n, primes, t = params(spec) if isinstance(spec, str) else spec
        self.n, self.primes, self.t = n, list(primes), t
        self.o = O.Oracle(n, self.primes, t)
        O.seed(seed)
        self.sk, self.pk, self.rk, _ = self.o.keygen()
        rng = np.random.default_rng(seed)
        self.va = rng.integers(0, 40, (na, n)).astype(np.uint64)
        self.vb = rng.integers(0, 40, (nb, n)).astype(np.uint64)
        enc = lambda v: self.o.encrypt(self.pk, self.o.batch_encode(v))  # noqa: E731
        self.a = np.stack([enc(v) for v in self.va])
        self.b = np.stack([enc(v) for v in self.vb])
        self._prod = {}

    def slots(self, ct):
        return self.o.batch_decode(self.o.decrypt(ct, self.sk))

    def prod(self, ia, ib, gram=False):
        """(the oracle's a[ia] * b[ib], its slots) -- gram: a[ia] * a[ib]; the product must decode on its own before anything is compared
        with it"""
        key = (int(ia), int(ib), gram)
        if key not in self._prod:
            y, vy = (self.a, self.va) if gram else (self.b, self.vb)
            want = ((self.va[key[0]].astype(object) * vy[key[1]].astype(object)) % self.t).astype(np.uint64)
            p = self.o.multiply(self.a[key[0]], y[key[1]])
            assert (self.slots(p) == want).all(), ("the oracle's product does not decode", key)
            self._prod[key] = (p, want)
        return self._prod[key]

    def check_items(self, out3, out2, ai, bi, count, what, gram=False):
        for i in range(count):
            p, want = self.prod(ai[i % len(ai)], bi[i % len(bi)], gram)
            if out3 is not None:
                assert (out3[i] == p).all() and (self.slots(out3[i]) == want).all(), (what, "size 3", i)
            if out2 is not None:
                assert (out2[i] == self.o.relinearize(p, self.rk)).all() and (self.slots(out2[i]) == want).all(), (what, "relinearized", i)

    def check_sums(self, sum3, sum2, ai, bi, groups, terms, what):
        for g in range(groups):
            acc, want = None, 0
            for i in range(g * terms, (g + 1) * terms):
                p, w = self.prod(ai[i % len(ai)], bi[i % len(bi)])
                acc, want = p if acc is None else self.o.add(acc, p), want + w.astype(object)
            want = (want % self.t).astype(np.uint64)
            assert (self.slots(acc) == want).all(), ("the oracle's sum does not decode", what, g)
            if sum3 is not None:
                assert (sum3[g] == acc).all() and (self.slots(sum3[g]) == want).all(), (what, "size-3 sum", g)
            if sum2 is not None:
                assert (sum2[g] == self.o.relinearize(acc, self.rk)).all() and (self.slots(sum2[g]) == want).all(), (what, "relinearized sum", g)


_CASES = {}


def _case(spec, na=3, nb=2):
    key = (spec, na, nb)
    if key not in _CASES:
        _CASES[key] = _Case(spec, na, nb)
    return _CASES[key]


@pytest.fixture(scope="module", autouse=True)
def _drop_cases():
    yield
    _CASES.clear()


def _device(c, monkeypatch, env=None, small_batch=False):
    """Context, evaluator, device keys and the two arrays to prepare; the evaluator's pipelines chosen by the parameters alone unless
    small_batch (HIPBFV_NO_SMALL_BATCH is read when an evaluator is made, the other switches when a context is)."""
    from sunscreen_amd import Context, RelinearizationKeys
    from sunscreen_amd.batch import BatchEvaluator, to_device

    for k, v in (env or {}).items():
        monkeypatch.setenv(k, v)
    if small_batch:
        monkeypatch.delenv("HIPBFV_NO_SMALL_BATCH", raising=False)
    else:
        monkeypatch.setenv("HIPBFV_NO_SMALL_BATCH", "1")
    ctx = Context.from_raw(c.n, c.primes, c.t)
    return ctx, BatchEvaluator(ctx), RelinearizationKeys.from_array(ctx, c.rk), to_device(c.a), to_device(c.b)


def _gathered(d, index, count):
    import torch

    return d.index_select(0, torch.tensor([int(index[i % len(index)]) for i in range(count)], dtype=torch.int64, device=d.device)).contiguous()


def _four_calls(ev, rkd, ma, mb, groups, terms, ai=AIDX, bi=BIDX):
    """The four calls over two prepared objects: their outputs and what each launched."""
    count = groups * terms
    calls = {"mul": lambda: ev.multiply_prepared(ma, ai, mb, bi, count), "relin": lambda: ev.multiply_relin_prepared(ma, ai, mb, bi, rkd, count),
             "sum": lambda: ev.multiply_sum_prepared(ma, ai, mb, bi, groups, terms),
             "sum_relin": lambda: ev.multiply_sum_relin_prepared(ma, ai, mb, bi, rkd, groups, terms)}
    res = {k: _profiled(ev, f) for k, f in calls.items()}
    return {k: v[0] for k, v in res.items()}, {k: v[1] for k, v in res.items()}


def _check_all(c, ev, rkd, da, db, outs, groups, terms, what, ai=AIDX, bi=BIDX):
    """Against the oracle, and against the library's counterparts on the two gathered arrays."""
    import torch
    from sunscreen_amd.batch import to_host

    count = groups * terms
    ga, gb = _gathered(da, ai, count), _gathered(db, bi, count)
    sa, sb = ga.reshape((groups, terms) + tuple(ga.shape[1:])), gb.reshape((groups, terms) + tuple(gb.shape[1:]))
    own = {"mul": ev.multiply(ga, gb), "relin": ev.multiply_relin(ga, gb, rkd), "sum": ev.multiply_sum(sa, sb), "sum_relin": ev.multiply_sum_relin(sa, sb, rkd)}
    for call in outs:
        assert torch.equal(outs[call], own[call]), (what, call, "differs from the counterpart on the gathered arrays")
    c.check_items(to_host(outs["mul"]), to_host(outs["relin"]), ai, bi, count, what)
    c.check_sums(to_host(outs["sum"]), to_host(outs["sum_relin"]), ai, bi, groups, terms, what)


# ---- 1: every body of the new middle kernel, all four calls -----------------------------------------------------------------------
@pytest.mark.parametrize("name,spec,groups,env", [
    ("FP64, 2 primes", "default_4096", 2, {}),
    ("packed FP64, three exchange regions", "default_8192", 2, {}),
    ("unit-test set", "seal_fhe_unit", 2, {}),
    ("integer rows, mixed fused pair", BITS54, 2, {}),
    ("8 primes, per-row packing", "default_16384", 1, {}),  # 3 items: the slice-major order pads them to 8
    ("8 primes, 8-byte rows", "default_16384", 1, {"HIPBFV_PACK_ROWS": "0"}),
    ("integer base", "default_4096", 2, {"HIPBFV_NO_F64": "1"}),
])
def test_every_body_of_the_pair_middle_kernel(name, spec, groups, env, monkeypatch):
    import torch

    c = _case(spec)
    ctx, ev, rkd, da, db = _device(c, monkeypatch, env)
    count = groups * 3
    before = (da.clone(), db.clone())
    ma, mb = ev.prepare(da), ev.prepare(db)
    assert ma.count == 3 and mb.count == 2
    outs, seen = _four_calls(ev, rkd, ma, mb, groups, 3)
    for call, s in seen.items():
        assert "mul_head" not in s and "mul_prep" not in s and "behz_extend" not in s and "tensor" not in s, (name, call, s)
        assert s["mul_mid"]["launches"] == 1 and s["mul_mid"]["units"] == count, (name, call, s)
    assert "mul_tail" in seen["mul"] and "mul_tail_sum" in seen["sum"] and "mul_tail_sum" in seen["sum_relin"], (name, seen)
    _check_all(c, ev, rkd, da, db, outs, groups, 3, name)
    assert torch.equal(da, before[0]) and torch.equal(db, before[1]), "an operand changed"
    ev.check()
    ma.close()
    mb.close()


# ---- 2: the matrix product ---------------------------------------------------------------------------------------------------------
def test_matrix_product_under_every_chunk(monkeypatch):
    """default_4096, A 2 x 3 and B 3 x 2 through workloads.matrix_product: 4 groups x 3 terms.  One launch sequence at the default chunk,
    one group per sequence at 7 items, slices of 2 and 1 terms at 2 -- the same bits under all three, the oracle's words, and decoded
    the integer matrix product of the slot vectors mod t."""
    import torch
    from sunscreen_amd.batch import multiply_sum_plan, to_host
    from sunscreen_amd.workloads import matrix_product, matrix_product_index

    c = _case("default_4096", 6, 6)
    ctx, ev, rkd, da, db = _device(c, monkeypatch)
    ma, mb = ev.prepare(da), ev.prepare(db)
    ai, bi = matrix_product_index(2, 3, 2)
    first = None
    for chunk in (None, 7, 2):
        if chunk:
            ev.set_chunk_ops(chunk)
        launches = len(multiply_sum_plan(4, 3, chunk or 4096))
        out3, s3 = _profiled(ev, lambda: matrix_product(ev, ma, mb, 2, 3, 2))
        out2, s2 = _profiled(ev, lambda: matrix_product(ev, ma, mb, 2, 3, 2, rkd))
        for s in (s3, s2):
            assert s["mul_mid"]["launches"] == launches and s["mul_tail_sum"]["launches"] == launches and "mul_head" not in s, (chunk, s)
            assert s["mul_mid"]["units"] == 12, (chunk, s)
        if first is None:
            first = (out3, out2)
            assert tuple(out3.shape) == (4, 3, ctx.K, c.n) and tuple(out2.shape) == (4, 2, ctx.K, c.n)
            h3, h2 = to_host(out3), to_host(out2)
            c.check_sums(h3, h2, ai, bi, 4, 3, "matrix product")
            for i in range(2):
                for j in range(2):
                    want = sum(c.va[i * 3 + t].astype(object) * c.vb[t * 2 + j].astype(object) for t in range(3)) % c.t
                    assert (c.slots(h3[i * 2 + j]) == want.astype(np.uint64)).all() and (c.slots(h2[i * 2 + j]) == want.astype(np.uint64)).all(), (i, j)
        assert torch.equal(out3, first[0]) and torch.equal(out2, first[1]), chunk
    ev.check()
    ma.close()
    mb.close()


# ---- 3: one object on both sides ---------------------------------------------------------------------------------------------------
def test_a_gram_matrix_over_one_object(monkeypatch):
    """ma is mb: all 9 pairs (i, j) of 3 prepared ciphertexts, the three with i == j among them -- those have the words of the oracle's
    multiply(x, x)."""
    import torch
    from sunscreen_amd.batch import to_host

    c = _case("default_4096")
    ctx, ev, rkd, da, _db = _device(c, monkeypatch)
    m = ev.prepare(da)
    ai, bi = [i for i in range(3) for _ in range(3)], [j for _ in range(3) for j in range(3)]
    (out3, out2), seen = _profiled(ev, lambda: (ev.multiply_prepared(m, ai, m, bi), ev.multiply_relin_prepared(m, ai, m, bi, rkd)))
    assert seen["mul_mid"]["launches"] == 2 and seen["mul_mid"]["units"] == 18 and "mul_head" not in seen, seen
    ga, gb = _gathered(da, ai, 9), _gathered(da, bi, 9)
    assert torch.equal(out3, ev.multiply(ga, gb)) and torch.equal(out2, ev.multiply_relin(ga, gb, rkd))
    h3, h2 = to_host(out3), to_host(out2)
    c.check_items(h3, h2, ai, bi, 9, "gram", gram=True)
    for i in range(3):
        assert (h3[4 * i] == c.o.multiply(c.a[i], c.a[i])).all(), i
    ev.check()
    m.close()


# ---- 4: the other paths ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,spec,env,small_batch", [
    ("n = 1024", UNIT1024, {}, False),
    ("a few items", "default_8192", {}, True),
    ("no split multiply", "default_4096", {"HIPBFV_NO_SPLIT_MUL": "1"}, False),
])
def test_off_the_split_path_both_operands_are_gathered(name, spec, env, small_batch, monkeypatch):
    c = _case(spec)
    ctx, ev, rkd, da, db = _device(c, monkeypatch, env, small_batch)
    ma, mb = ev.prepare(da), ev.prepare(db)
    outs, seen = _four_calls(ev, rkd, ma, mb, 2, 3)
    for call, s in seen.items():
        assert "mul_prep" not in s and "mul_mid" not in s and "mul_head" not in s and s.get("behz_floor_sk"), (name, call, s)
    _check_all(c, ev, rkd, da, db, outs, 2, 3, name)
    ev.check()
    ma.close()
    mb.close()


def test_one_pair_of_objects_serves_the_whole_polynomial_and_the_split_path(monkeypatch):
    """default_8192 without HIPBFV_NO_SMALL_BATCH: 6 items take the whole-polynomial kernels (both copies are gathered), 40 items the
    split kernels (both objects' rows are read) -- the same objects, the same evaluator, the oracle's words both times."""
    import torch
    from sunscreen_amd.batch import to_host

    c = _case("default_8192")
    ctx, ev, rkd, da, db = _device(c, monkeypatch, small_batch=True)
    ma, mb = ev.prepare(da), ev.prepare(db)
    few, seen = _profiled(ev, lambda: ev.multiply_prepared(ma, AIDX, mb, BIDX))
    assert "mul_mid" not in seen and seen.get("behz_floor_sk"), seen
    c.check_items(to_host(few), None, AIDX, BIDX, 6, "6 items")
    many, seen = _profiled(ev, lambda: ev.multiply_prepared(ma, AIDX, mb, BIDX, 40))  # item i is item i % 6
    assert seen["mul_mid"]["launches"] == 1 and seen["mul_mid"]["units"] == 40 and "mul_head" not in seen and "behz_floor_sk" not in seen, seen
    for i in range(40):
        assert torch.equal(many[i], few[i % 6]), i
    ev.check()
    ma.close()
    mb.close()


# ---- 5: the lane-split geometry build ----------------------------------------------------------------------------------------------
def test_the_lane_split_geometry_build_gives_the_same_bits():
    """libhipbfv_geom8.so in a process of its own: both operands' rows written and read in that build's register order, the words of
    the default build's case above, hence the oracle's."""
    lib = os.path.join(ROOT, "sunscreen_amd", "lib", "variants", "libhipbfv_geom8.so")
    assert os.path.exists(lib), "build the variant library first: make -C sunscreen_amd/csrc variants (build() does)"
    c = _case("default_16384")
    script = r"""
import sys, numpy as np, torch
sys.path.insert(0, %r)
from sunscreen_amd import Context, RelinearizationKeys
from sunscreen_amd.batch import BatchEvaluator, to_device, to_host
z = np.load(sys.argv[1])
ctx = Context.from_raw(int(z["n"]), [int(p) for p in z["primes"]], int(z["t"]))
ev = BatchEvaluator(ctx)
ev.profile(True)
rk = RelinearizationKeys.from_array(ctx, z["rk"])
ma, mb = ev.prepare(to_device(z["a"])), ev.prepare(to_device(z["b"]))
ai, bi = [int(i) for i in z["ai"]], [int(i) for i in z["bi"]]
out = dict(mul=ev.multiply_prepared(ma, ai, mb, bi, 3), relin=ev.multiply_relin_prepared(ma, ai, mb, bi, rk, 3),
           sum3=ev.multiply_sum_prepared(ma, ai, mb, bi, 1, 3), sum2=ev.multiply_sum_relin_prepared(ma, ai, mb, bi, rk, 1, 3))
torch.cuda.synchronize()
seen = ev.profile_read()
assert seen["mul_prep"]["launches"] == 2 and seen["mul_mid"]["launches"] == 4 and seen["mul_head"]["units"] == 2 * 3 + 2 * 2, seen
ev.check()
np.savez(sys.argv[2], **{k: to_host(v) for k, v in out.items()})
""" % ROOT
    with tempfile.TemporaryDirectory() as td:
        src, dst = os.path.join(td, "in.npz"), os.path.join(td, "out.npz")
        np.savez(src, n=c.n, primes=np.array(c.primes, dtype=np.uint64), t=c.t, a=c.a, b=c.b, rk=c.rk, ai=np.array(AIDX), bi=np.array(BIDX))
        subprocess.check_call([sys.executable, "-c", script, src, dst], env=dict(os.environ, HIPBFV_LIB=lib, HIPBFV_NO_SMALL_BATCH="1"))
        got = np.load(dst)
        c.check_items(got["mul"], got["relin"], AIDX, BIDX, 3, "geom8")
        c.check_sums(got["sum3"], got["sum2"], AIDX, BIDX, 1, 3, "geom8")


# ---- 6: refusals launch nothing ----------------------------------------------------------------------------------------------------
def test_refusals_come_before_any_launch_or_write(monkeypatch):
    import torch
    from sunscreen_amd import Context, RelinearizationKeys, _lib
    from sunscreen_amd.batch import BatchEvaluator, _ptr, _stream

    c = _case("default_4096")
    ctx, ev, rkd, da, db = _device(c, monkeypatch)
    L, h, K, n = _lib.load(), ev._h, ctx.K, c.n
    ma, mb = ev.prepare(da), ev.prepare(db)
    ev2 = BatchEvaluator(Context.from_raw(c.n, c.primes, c.t))  # the same parameters, another context object
    oa, ob = ev2.prepare(da), ev2.prepare(db)
    out3 = torch.full((6, 3, K, n), SENTINEL, dtype=torch.int64, device="cuda")
    out2 = torch.full((6, 2, K, n), SENTINEL, dtype=torch.int64, device="cuda")
    u32x6 = C.c_uint32 * 6
    ai, bi = u32x6(*AIDX), u32x6(*BIDX)
    bad_a, bad_b = u32x6(0, 1, 2, 3, 0, 1), u32x6(0, 1, 0, 1, 2, 0)  # item 3 names ciphertext 3 of 3 / item 4 names ciphertext 2 of 2
    empty = RelinearizationKeys()
    no_key = _hr(lambda: ev.relinearize(torch.zeros((1, 3, K, n), dtype=torch.int64, device="cuda"), empty))[0]
    assert no_key != 0
    ok = dict(h=h, ma=ma.get_handle(), ai=ai, mb=mb.get_handle(), bi=bi, n=6, rk=rkd.get_handle(), o3=_ptr(out3), o2=_ptr(out2), terms=3)

    def run(which, **kw):  # the four calls on 6 items / 2 groups x 3 terms with the given arguments replaced
        p = dict(ok, **kw)
        head = (p["h"], p["ma"], p["ai"], p["mb"], p["bi"], p["n"])
        if which == "mul":
            return L.hipbfv_batch_multiply_prepared(*head, p["o3"], p.get("count", 6), _stream())
        if which == "relin":
            return L.hipbfv_batch_multiply_relin_prepared(*head, p["rk"], p["o2"], p.get("count", 6), _stream())
        if which == "sum":
            return L.hipbfv_batch_multiply_sum_prepared(*head, p["o3"], p.get("count", 2), p["terms"], _stream())
        return L.hipbfv_batch_multiply_sum_relin_prepared(*head, p["rk"], p["o2"], p.get("count", 2), p["terms"], _stream())

    ALL = ("mul", "relin", "sum", "sum_relin")
    refused = [(w, kw, E_POINTER) for w in ALL for kw in (dict(h=None), dict(ma=None), dict(mb=None), dict(ai=None), dict(bi=None), dict(o3=None, o2=None))]
    refused += [(w, kw, E_POINTER) for w in ALL for kw in (dict(ma=rkd.get_handle()), dict(mb=rkd.get_handle()))]  # a key object is no multiplicand
    refused += [(w, kw, E_INVALIDARG) for w in ALL for kw in (dict(n=0), dict(ai=bad_a), dict(bi=bad_b), dict(ma=oa.get_handle()), dict(mb=ob.get_handle()))]
    refused += [(w, dict(terms=0), E_INVALIDARG) for w in ("sum", "sum_relin")]
    refused += [(w, dict(rk=k), no_key) for w in ("relin", "sum_relin") for k in (empty.get_handle(), None)]
    ev.profile(True)
    ev.profile_reset()
    try:
        for which, kw, want in refused:
            got = run(which, **kw) & 0xFFFFFFFF
            assert got == want, (which, sorted(kw), hex(got), hex(want))
        msg = _hr(lambda: ev.multiply_prepared(ma, [0, 1, 2, 3, 0, 1], mb, BIDX))[1]
        assert "item 3" in msg and "a_index" in msg, msg
        msg = _hr(lambda: ev.multiply_sum_relin_prepared(ma, AIDX, mb, [0, 1, 0, 1, 2, 0], rkd, 2, 3))[1]
        assert "item 4" in msg and "b_index" in msg, msg
        msg = _hr(lambda: ev.multiply_sum_prepared(ma, [3, 1, 2, 2, 0, 1], mb, [2, 1, 0, 1, 1, 0], 2, 3))[1]  # both at item 0: a is named
        assert "item 0" in msg and "a_index" in msg, msg
        for which in ALL:  # empty calls are accepted and launch nothing either
            assert run(which, count=0) == 0, which
        torch.cuda.synchronize()
        assert ev.profile_read() == {}, ev.profile_read()
    finally:
        ev.profile(False)
    assert (out3 == SENTINEL).all() and (out2 == SENTINEL).all()
    ev.check()
    for m in (ma, mb, oa, ob):
        m.close()


# ---- 7: transparent results --------------------------------------------------------------------------------------------------------
def test_transparent_results_are_reported_as_in_the_counterparts(monkeypatch):
    """The second object's ciphertext 1 is all zero.  The item forms over b_index {0, 1, 0, 1, 1, 0}: item 1's product is the first
    transparent one and is named, as hipbfv_batch_multiply names it.  In a sum it is seen only when the whole group's sum is transparent:
    that index per group reports nothing, an index that gives group 1 the zero ciphertext in every term reports group 1."""
    from sunscreen_amd import _lib
    from sunscreen_amd.batch import _stream

    c = _case("default_4096")
    ctx, ev, rkd, da, db = _device(c, monkeypatch)
    zb = db.clone()
    zb[1] = 0
    ma, mb = ev.prepare(da), ev.prepare(zb)
    first = C.c_uint64(123)
    status = lambda: (_lib.load().hipbfv_batch_status(ev._h, C.byref(first), _stream()) & 0xFFFFFFFF, first.value)  # noqa: E731
    ev.multiply(_gathered(da, AIDX, 6), _gathered(zb, BIDX, 6))
    assert status() == (COR_E_INVALIDOPERATION, 1)
    for call in (lambda: ev.multiply_prepared(ma, AIDX, mb, BIDX), lambda: ev.multiply_relin_prepared(ma, AIDX, mb, BIDX, rkd)):
        call()
        hr, msg = _hr(ev.check)
        assert hr == COR_E_INVALIDOPERATION and "item 1)" in msg, (hex(hr), msg)
        call()
        assert status() == (COR_E_INVALIDOPERATION, 1)
    for call in (lambda bi: ev.multiply_sum_prepared(ma, AIDX, mb, bi, 2, 3), lambda bi: ev.multiply_sum_relin_prepared(ma, AIDX, mb, bi, rkd, 2, 3)):
        call(BIDX)
        assert status() == (0, 2**64 - 1)
        call([0, 0, 0, 1, 1, 1])
        assert status() == (COR_E_INVALIDOPERATION, 1)
    ma.close()
    mb.close()


# ---- 8: streams --------------------------------------------------------------------------------------------------------------------
def test_a_product_on_another_stream_waits_for_both_preparations(monkeypatch):
    """Both prepare() calls are queued on one stream behind other work, the products at once on another, with no host synchronisation
    in between: the objects' events order them."""
    import torch
    from sunscreen_amd.batch import to_host

    c = _case("default_4096")
    ctx, ev, rkd, da, db = _device(c, monkeypatch)
    torch.cuda.synchronize()
    s1, s2 = torch.cuda.Stream(), torch.cuda.Stream()
    with torch.cuda.stream(s1):
        x = torch.ones((2048, 2048), device="cuda")
        for _ in range(40):  # the preparations start well after the products below have been queued
            x = (x @ x) * 1e-4
        ma, mb = ev.prepare(da), ev.prepare(db)
    with torch.cuda.stream(s2):
        out3 = ev.multiply_prepared(ma, AIDX, mb, BIDX)
        out2 = ev.multiply_sum_relin_prepared(ma, AIDX, mb, BIDX, rkd, 2, 3)
    torch.cuda.synchronize()
    c.check_items(to_host(out3), None, AIDX, BIDX, 6, "two streams")
    c.check_sums(None, to_host(out2), AIDX, BIDX, 2, 3, "two streams")
    ev.check()
    ma.close()
    mb.close()
