"""Prepared multiplicands: hipbfv_Multiplicand_Create and hipbfv_batch_multiply_shared / _relin_shared / _sum_shared / _sum_relin_shared.

Item i multiplies a[i] by prepared ciphertext b_index[i % index_len] (i = g * terms + t in the sum forms).  Every output must be, word
for word, the CPU oracle's `multiply` (folded with `add`, then `relinearize`) on the replicated operand, and equal the library's own
counterpart call on a replicated array; decrypted and decoded it must give the slot products.  On the split path the head extends two
polynomials per item instead of four and `mul_prep` runs in `prepare` alone; elsewhere the multiplicands are gathered from the
object's copy.  Every parameter set here is one on which the oracle's own sequence decodes with noise budget left (3 terms; 5 terms at
n = 4096 with two 36-bit data primes leave 19 bits), and that is asserted before the GPU is compared with it."""
import ctypes as C
import os
import subprocess
import sys
import tempfile

import numpy as np
import pytest

from oracle import bfv_oracle as O
from tests.bfv_helpers import params
from tests.test_gpu_multiply_sum import BITS54, COR_E_INVALIDOPERATION, E_INVALIDARG, E_POINTER, SENTINEL, UNIT1024, _hr

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
IDX = [0, 1, 0]


class _Case:
    """One parameter set, one key pair, groups x terms fresh encryptions `a`, `nprep` fresh encryptions `m` to prepare, and the oracle's
    products -- each computed once and shared by the tests that name the same case."""

    def __init__(self, spec, groups, terms, nprep, seed=4097):
        n, primes, t = params(spec) if isinstance(spec, str) else spec
        self.n, self.primes, self.t, self.groups, self.terms = n, list(primes), t, groups, terms
        self.o = O.Oracle(n, self.primes, t)
        O.seed(seed)
        self.sk, self.pk, self.rk, _ = self.o.keygen()
        rng = np.random.default_rng(seed)
        self.va = rng.integers(0, 40, (groups, terms, n)).astype(np.uint64)
        self.vm = rng.integers(0, 40, (nprep, n)).astype(np.uint64)
        enc = lambda v: self.o.encrypt(self.pk, self.o.batch_encode(v))  # noqa: E731
        self.a = np.stack([np.stack([enc(self.va[g, j]) for j in range(terms)]) for g in range(groups)])
        self.m = np.stack([enc(self.vm[k]) for k in range(nprep)])
        self._prod = {}

    def slots(self, ct):
        return self.o.batch_decode(self.o.decrypt(ct, self.sk))

    def prod(self, i, index):
        """(the oracle's a[i] * m[index[i % len]], its slots); the product must decode on its own before anything is compared with it"""
        key = (i, int(index[i % len(index)]))
        if key not in self._prod:
            g, t = divmod(i, self.terms)
            want = ((self.va[g, t].astype(object) * self.vm[key[1]].astype(object)) % self.t).astype(np.uint64)
            p = self.o.multiply(self.a[g, t], self.m[key[1]])
            assert (self.slots(p) == want).all(), ("the oracle's product does not decode", key)
            self._prod[key] = (p, want)
        return self._prod[key]

    def check_items(self, out3, out2, index, what):
        for i in range(self.groups * self.terms):
            p, want = self.prod(i, index)
            if out3 is not None:
                assert (out3[i] == p).all() and (self.slots(out3[i]) == want).all(), (what, "size 3", i)
            if out2 is not None:
                assert (out2[i] == self.o.relinearize(p, self.rk)).all() and (self.slots(out2[i]) == want).all(), (what, "relinearized", i)

    def check_sums(self, sum3, sum2, index, what):
        T = self.terms
        for g in range(self.groups):
            acc, want = self.prod(g * T, index)
            want = want.astype(object)
            for i in range(g * T + 1, (g + 1) * T):
                acc, want = self.o.add(acc, self.prod(i, index)[0]), want + self.prod(i, index)[1].astype(object)
            want = (want % self.t).astype(np.uint64)
            assert (self.slots(acc) == want).all(), ("the oracle's sum does not decode", what, g)
            if sum3 is not None:
                assert (sum3[g] == acc).all() and (self.slots(sum3[g]) == want).all(), (what, "size-3 sum", g)
            if sum2 is not None:
                assert (sum2[g] == self.o.relinearize(acc, self.rk)).all() and (self.slots(sum2[g]) == want).all(), (what, "relinearized sum", g)


_CASES = {}


def _case(spec, groups, terms, nprep=2):
    key = (spec, groups, terms, nprep)
    if key not in _CASES:
        _CASES[key] = _Case(spec, groups, terms, nprep)
    return _CASES[key]


@pytest.fixture(scope="module", autouse=True)
def _drop_cases():
    yield
    _CASES.clear()


def _profiled(ev, call):
    """The result of call() and the kernels it launched: {name: {"launches", "units", "ms"}}."""
    import torch

    ev.profile(True)
    ev.profile_reset()
    try:
        out = call()
        torch.cuda.synchronize()
        return out, ev.profile_read()
    finally:
        ev.profile(False)


def _device(c, monkeypatch, env=None, small_batch=False):
    """Context, evaluator, device keys, `a` and the ciphertexts to prepare; the evaluator's pipelines chosen by the parameters alone
    unless small_batch (HIPBFV_NO_SMALL_BATCH is read when an evaluator is made, the other switches when a context is)."""
    from sunscreen_amd import Context, RelinearizationKeys
    from sunscreen_amd.batch import BatchEvaluator, to_device

    for k, v in (env or {}).items():
        monkeypatch.setenv(k, v)
    if small_batch:
        monkeypatch.delenv("HIPBFV_NO_SMALL_BATCH", raising=False)
    else:
        monkeypatch.setenv("HIPBFV_NO_SMALL_BATCH", "1")
    ctx = Context.from_raw(c.n, c.primes, c.t)
    return ctx, BatchEvaluator(ctx), RelinearizationKeys.from_array(ctx, c.rk), to_device(c.a), to_device(c.m)


def _flat(da):
    return da.reshape(-1, 2, da.shape[3], da.shape[4])


def _replicated(dm, index, count):
    import torch

    return dm.index_select(0, torch.tensor([int(index[i % len(index)]) for i in range(count)], dtype=torch.int64, device=dm.device)).contiguous()


def _four_calls(ev, rkd, da, m, index):
    """The four calls over a prepared multiplicand: their outputs and what each launched."""
    calls = {"mul": lambda: ev.multiply_shared(_flat(da), m, index), "relin": lambda: ev.multiply_relin_shared(_flat(da), m, index, rkd),
             "sum": lambda: ev.multiply_sum_shared(da, m, index), "sum_relin": lambda: ev.multiply_sum_relin_shared(da, m, index, rkd)}
    res = {k: _profiled(ev, f) for k, f in calls.items()}
    return {k: v[0] for k, v in res.items()}, {k: v[1] for k, v in res.items()}


def _check_all(c, ev, rkd, da, dm, outs, index, what):
    """Against the oracle, and against the library's counterparts on the replicated operand."""
    import torch
    from sunscreen_amd.batch import to_host

    db = _replicated(dm, index, c.groups * c.terms)
    own = {"mul": ev.multiply(_flat(da), db), "relin": ev.multiply_relin(_flat(da), db, rkd), "sum": ev.multiply_sum(da, db.reshape(da.shape)),
           "sum_relin": ev.multiply_sum_relin(da, db.reshape(da.shape), rkd)}
    for call in outs:
        assert torch.equal(outs[call], own[call]), (what, call, "differs from the counterpart on the replicated operand")
    c.check_items(to_host(outs["mul"]), to_host(outs["relin"]), index, what)
    c.check_sums(to_host(outs["sum"]), to_host(outs["sum_relin"]), index, what)


# ---- 1: every middle-kernel body, all four calls ---------------------------------------------------------------------------------
@pytest.mark.parametrize("name,spec,groups,env", [
    ("FP64, 2 primes", "default_4096", 2, {}),
    ("packed FP64, three exchange regions", "default_8192", 2, {}),
    ("unit-test set", "seal_fhe_unit", 2, {}),
    ("integer rows, mixed fused pair", BITS54, 2, {}),
    ("8 primes, per-row packing", "default_16384", 1, {}),  # 3 items: the slice-major order pads them to 8
    ("8 primes, 8-byte rows", "default_16384", 1, {"HIPBFV_PACK_ROWS": "0"}),
    ("integer base", "default_4096", 2, {"HIPBFV_NO_F64": "1"}),
])
def test_every_body_of_the_shared_middle_kernel(name, spec, groups, env, monkeypatch):
    import torch

    c = _case(spec, groups, 3)
    ctx, ev, rkd, da, dm = _device(c, monkeypatch, env)
    count = groups * 3
    before = (da.clone(), dm.clone())
    m, prep = _profiled(ev, lambda: ev.prepare(dm))
    assert prep["mul_prep"]["launches"] == 1 and prep["mul_prep"]["units"] == 2 and prep["mul_head"]["units"] == 2 * 2, (name, prep)
    assert m.count == 2 and m.nbytes > dm.numel() * 8, (m.count, m.nbytes)
    outs, seen = _four_calls(ev, rkd, da, m, IDX)
    for call, s in seen.items():
        assert "mul_prep" not in s and "behz_extend" not in s and "tensor" not in s, (name, call, s)
        assert s["mul_head"]["launches"] == 1 and s["mul_head"]["units"] == 2 * count, (name, call, s)  # two polynomials per item
        assert s["mul_mid"]["launches"] == 1 and s["mul_mid"]["units"] == count, (name, call, s)
    assert "mul_tail" in seen["mul"] and "mul_tail_sum" in seen["sum"] and "mul_tail_sum" in seen["sum_relin"], (name, seen)
    _check_all(c, ev, rkd, da, dm, outs, IDX, name)
    assert torch.equal(da, before[0]) and torch.equal(dm, before[1]), "an operand changed"
    ev.check()
    m.close()


# ---- 2: index forms under chunks -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("index", [[0], [0, 1, 2, 3, 4], [3, 3, 0, 4, 1, 2, 2, 4, 0, 0, 1, 3, 4, 4, 2]], ids=["broadcast", "period", "permuted"])
def test_index_forms_give_the_same_bits_under_every_chunk(index, monkeypatch):
    """default_4096, 3 groups x 5 terms over 5 prepared ciphertexts: {0}, {0..4} (the matrix-vector product) and a full-length index
    with repeats; one launch sequence at the default chunk, one group per chunk at 7 items, slices of 2, 2 and 1 terms at 2."""
    import torch

    c = _case("default_4096", 3, 5, nprep=5)
    ctx, ev, rkd, da, dm = _device(c, monkeypatch)
    m = ev.prepare(dm)
    first = None
    for chunk, launches in ((None, 1), (7, 3), (2, 9)):
        if chunk:
            ev.set_chunk_ops(chunk)
        outs, seen = _four_calls(ev, rkd, da, m, index)
        assert seen["sum"]["mul_tail_sum"]["launches"] == launches and seen["sum"]["mul_mid"]["launches"] == launches, (chunk, seen["sum"])
        assert seen["sum"]["mul_head"]["units"] == 2 * 15 and seen["mul"]["mul_head"]["units"] == 2 * 15, (chunk, seen)
        if first is None:
            first = outs
            _check_all(c, ev, rkd, da, dm, outs, index, chunk)
        for call in outs:
            assert torch.equal(outs[call], first[call]), (chunk, call)
    ev.check()
    m.close()


# ---- 3: the other paths ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,spec,env,small_batch", [
    ("n = 1024", UNIT1024, {}, False),
    ("a few items", "default_8192", {}, True),
    ("no split multiply", "default_4096", {"HIPBFV_NO_SPLIT_MUL": "1"}, False),
])
def test_off_the_split_path_the_multiplicands_are_gathered(name, spec, env, small_batch, monkeypatch):
    c = _case(spec, 2, 3)
    ctx, ev, rkd, da, dm = _device(c, monkeypatch, env, small_batch)
    m = ev.prepare(dm)
    outs, seen = _four_calls(ev, rkd, da, m, IDX)
    for call, s in seen.items():
        assert "mul_prep" not in s and "mul_mid" not in s and "mul_head" not in s and s.get("behz_floor_sk"), (name, call, s)
    _check_all(c, ev, rkd, da, dm, outs, IDX, name)
    ev.check()
    m.close()


def test_one_multiplicand_serves_the_whole_polynomial_and_the_split_path(monkeypatch):
    """default_8192 without HIPBFV_NO_SMALL_BATCH: 6 items take the whole-polynomial kernels (the copy is gathered), 40 items the
    split kernels (the prepared rows are read) -- the same object, the same evaluator, the oracle's words both times."""
    import torch
    from sunscreen_amd.batch import to_host

    c = _case("default_8192", 2, 3)
    ctx, ev, rkd, da, dm = _device(c, monkeypatch, small_batch=True)
    m, prep = _profiled(ev, lambda: ev.prepare(dm))
    assert prep["mul_prep"]["launches"] == 1, prep
    few, seen = _profiled(ev, lambda: ev.multiply_shared(_flat(da), m, IDX))
    assert "mul_mid" not in seen and "mul_prep" not in seen and seen.get("behz_floor_sk"), seen
    c.check_items(to_host(few), None, IDX, "6 items")
    many_in = _flat(da).repeat(7, 1, 1, 1)[:40].contiguous()  # item i is a[i % 6]; 6 is a multiple of the index period
    many, seen = _profiled(ev, lambda: ev.multiply_shared(many_in, m, IDX))
    assert seen["mul_mid"]["launches"] == 1 and seen["mul_head"]["units"] == 2 * 40 and "mul_prep" not in seen and "behz_floor_sk" not in seen, seen
    for i in range(40):
        assert torch.equal(many[i], few[i % 6]), i
    ev.check()
    m.close()


# ---- 4: the lane-split geometry build --------------------------------------------------------------------------------------------
def test_the_lane_split_geometry_build_gives_the_same_bits():
    """libhipbfv_geom8.so in a process of its own: prepared rows written and read in that build's register order, the words of the
    default build's case above, hence the oracle's."""
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
a, rk = to_device(z["a"]), RelinearizationKeys.from_array(ctx, z["rk"])
m = ev.prepare(to_device(z["m"]))
flat, idx = a.reshape(3, 2, a.shape[3], a.shape[4]), [0, 1, 0]
out = dict(mul=ev.multiply_shared(flat, m, idx), relin=ev.multiply_relin_shared(flat, m, idx, rk), sum3=ev.multiply_sum_shared(a, m, idx),
           sum2=ev.multiply_sum_relin_shared(a, m, idx, rk))
torch.cuda.synchronize()
seen = ev.profile_read()
assert seen["mul_prep"]["launches"] == 1 and seen["mul_mid"]["launches"] == 4 and seen["mul_head"]["units"] == 2 * 2 + 4 * 2 * 3, seen
ev.check()
np.savez(sys.argv[2], **{k: to_host(v) for k, v in out.items()})
""" % ROOT
    with tempfile.TemporaryDirectory() as td:
        src, dst = os.path.join(td, "in.npz"), os.path.join(td, "out.npz")
        np.savez(src, n=c.n, primes=np.array(c.primes, dtype=np.uint64), t=c.t, a=c.a, m=c.m, rk=c.rk)
        subprocess.check_call([sys.executable, "-c", script, src, dst], env=dict(os.environ, HIPBFV_LIB=lib, HIPBFV_NO_SMALL_BATCH="1"))
        got = np.load(dst)
        c.check_items(got["mul"], got["relin"], IDX, "geom8")
        c.check_sums(got["sum3"], got["sum2"], IDX, "geom8")


# ---- 5: refusals launch nothing --------------------------------------------------------------------------------------------------
def test_refusals_come_before_any_launch_or_write(monkeypatch):
    import torch
    from sunscreen_amd import Context, RelinearizationKeys, _lib
    from sunscreen_amd.batch import BatchEvaluator, _ptr, _stream, to_host

    c = _case("default_4096", 2, 3)
    ctx, ev, rkd, da, dm = _device(c, monkeypatch)
    L, h, K, n = _lib.load(), ev._h, ctx.K, c.n
    item = 2 * K * n
    m = ev.prepare(dm)
    other = BatchEvaluator(Context.from_raw(c.n, c.primes, c.t)).prepare(dm)  # the same parameters, another context object
    # `a` inside one allocation with room after it, so that outputs can be laid over it
    buf = torch.full((6 * item + 2 * 3 * K * n + item,), SENTINEL, dtype=torch.int64, device="cuda")
    buf[: 6 * item] = da.reshape(-1)
    a_in = buf[: 6 * item].view(2, 3, 2, K, n)
    out3 = torch.full((6, 3, K, n), SENTINEL, dtype=torch.int64, device="cuda")
    out2 = torch.full((6, 2, K, n), SENTINEL, dtype=torch.int64, device="cuda")
    idx, bad = (C.c_uint32 * 3)(0, 1, 0), (C.c_uint32 * 3)(0, 1, 2)  # bad: item 2 names prepared ciphertext 2 of 2
    empty = RelinearizationKeys()
    no_key = _hr(lambda: ev.relinearize(torch.zeros((1, 3, K, n), dtype=torch.int64, device="cuda"), empty))[0]
    assert no_key != 0
    ok = dict(a=_ptr(a_in), m=m.get_handle(), idx=idx, n=3, rk=rkd.get_handle(), o3=_ptr(out3), o2=_ptr(out2), terms=3)

    def run(which, **kw):  # the four calls on 6 items / 2 groups x 3 terms with the given arguments replaced
        p = dict(ok, **kw)
        if which == "mul":
            return L.hipbfv_batch_multiply_shared(h, p["a"], p["m"], p["idx"], p["n"], p["o3"], p.get("count", 6), _stream())
        if which == "relin":
            return L.hipbfv_batch_multiply_relin_shared(h, p["a"], p["m"], p["idx"], p["n"], p["rk"], p["o2"], p.get("count", 6), _stream())
        if which == "sum":
            return L.hipbfv_batch_multiply_sum_shared(h, p["a"], p["m"], p["idx"], p["n"], p["o3"], p.get("count", 2), p["terms"], _stream())
        return L.hipbfv_batch_multiply_sum_relin_shared(h, p["a"], p["m"], p["idx"], p["n"], p["rk"], p["o2"], p.get("count", 2), p["terms"], _stream())

    ALL = ("mul", "relin", "sum", "sum_relin")
    refused = [(w, kw, E_POINTER) for w in ALL for kw in (dict(a=None), dict(m=None), dict(idx=None), dict(o3=None, o2=None))]
    refused += [(w, dict(m=rkd.get_handle()), E_POINTER) for w in ALL]  # a key object is no multiplicand
    refused += [(w, kw, E_INVALIDARG) for w in ALL for kw in (dict(n=0), dict(idx=bad), dict(m=other.get_handle()))]
    refused += [(w, dict(terms=0), E_INVALIDARG) for w in ("sum", "sum_relin")]
    refused += [(w, dict(rk=k), no_key) for w in ("relin", "sum_relin") for k in (empty.get_handle(), None)]
    over = lambda off, shape: _ptr(buf[off: off + int(np.prod(shape))].view(*shape))  # noqa: E731
    refused += [("mul", dict(o3=over(0, (6, 3, K, n))), E_INVALIDARG), ("relin", dict(o2=over(item, (6, 2, K, n))), E_INVALIDARG),
                ("sum", dict(o3=over(item, (2, 3, K, n))), E_INVALIDARG), ("sum_relin", dict(o2=over(5 * item, (2, 2, K, n))), E_INVALIDARG),
                ("sum_relin", dict(o2=_ptr(a_in)), E_INVALIDARG)]  # (a sum's out2 exactly at a: the widths differ)
    before = buf.clone()
    ev.profile(True)
    ev.profile_reset()
    try:
        for which, kw, want in refused:
            got = run(which, **kw) & 0xFFFFFFFF
            assert got == want, (which, sorted(kw), hex(got), hex(want))
        assert L.hipbfv_Multiplicand_Create(h, _ptr(dm), 0, _stream(), C.byref(C.c_void_p())) & 0xFFFFFFFF == E_INVALIDARG
        assert L.hipbfv_Multiplicand_Create(h, None, 2, _stream(), C.byref(C.c_void_p())) & 0xFFFFFFFF == E_POINTER
        assert "item 2" in _hr(lambda: ev.multiply_shared(_flat(da), m, [0, 1, 2]))[1]
        for which in ALL:  # empty calls are accepted and launch nothing either
            assert run(which, count=0) == 0, which
        torch.cuda.synchronize()
        assert ev.profile_read() == {}, ev.profile_read()
    finally:
        ev.profile(False)
    assert torch.equal(buf, before) and (out3 == SENTINEL).all() and (out2 == SENTINEL).all()
    # out2 == a is the one overlap that is accepted: multiply_relin_shared in place
    want = ev.multiply_relin_shared(_flat(da), m, IDX, rkd)
    inplace = _flat(da).clone()
    got = ev.multiply_relin_shared(inplace, m, IDX, rkd, out=inplace)
    assert got.data_ptr() == inplace.data_ptr() and torch.equal(got, want)
    c.check_items(None, to_host(got), IDX, "in place")
    ev.check()
    other.close()
    m.close()


# ---- 6: transparent results ------------------------------------------------------------------------------------------------------
def test_transparent_results_are_reported_as_in_the_counterparts(monkeypatch):
    """Prepared ciphertext 1 is all zero.  multiply_shared of 3 items with index {0, 1, 0}: item 1's product is transparent and is named,
    as hipbfv_batch_multiply names it.  In a sum it is seen only when the whole group's sum is transparent: index {0, 1, 0} per group
    reports nothing, an index that gives group 1 the zero ciphertext in every term reports group 1."""
    from sunscreen_amd import _lib
    from sunscreen_amd.batch import _stream

    c = _case("default_4096", 2, 3)
    ctx, ev, rkd, da, dm = _device(c, monkeypatch)
    zm = dm.clone()
    zm[1] = 0
    m = ev.prepare(zm)
    first = C.c_uint64(123)
    status = lambda: (_lib.load().hipbfv_batch_status(ev._h, C.byref(first), _stream()) & 0xFFFFFFFF, first.value)  # noqa: E731
    flat = _flat(da)[:3].contiguous()
    ev.multiply(flat, _replicated(zm, IDX, 3))
    assert status() == (COR_E_INVALIDOPERATION, 1)
    for call in (lambda: ev.multiply_shared(flat, m, IDX), lambda: ev.multiply_relin_shared(flat, m, IDX, rkd)):
        call()
        hr, msg = _hr(ev.check)
        assert hr == COR_E_INVALIDOPERATION and "item 1)" in msg, (hex(hr), msg)
        call()
        assert status() == (COR_E_INVALIDOPERATION, 1)
    for call in (lambda idx: ev.multiply_sum_shared(da, m, idx), lambda idx: ev.multiply_sum_relin_shared(da, m, idx, rkd)):
        call(IDX)
        assert status() == (0, 2**64 - 1)
        call([0, 0, 0, 1, 1, 1])
        assert status() == (COR_E_INVALIDOPERATION, 1)
    m.close()


# ---- 7: streams ------------------------------------------------------------------------------------------------------------------
def test_a_product_on_another_stream_waits_for_the_preparation(monkeypatch):
    """prepare() is queued on one stream behind other work, the product at once on another, with no host synchronisation in between:
    the object's event orders them."""
    import torch
    from sunscreen_amd.batch import to_host

    c = _case("default_4096", 2, 3)
    ctx, ev, rkd, da, dm = _device(c, monkeypatch)
    torch.cuda.synchronize()
    s1, s2 = torch.cuda.Stream(), torch.cuda.Stream()
    with torch.cuda.stream(s1):
        x = torch.ones((2048, 2048), device="cuda")
        for _ in range(40):  # the preparation starts well after the product below has been queued
            x = (x @ x) * 1e-4
        m = ev.prepare(dm)
    with torch.cuda.stream(s2):
        out3 = ev.multiply_shared(_flat(da), m, IDX)
        out2 = ev.multiply_sum_relin_shared(da, m, IDX, rkd)
    torch.cuda.synchronize()
    c.check_items(to_host(out3), None, IDX, "two streams")
    c.check_sums(None, to_host(out2), IDX, "two streams")
    ev.check()
    m.close()
