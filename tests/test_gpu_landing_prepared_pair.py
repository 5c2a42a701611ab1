"""Products of two prepared operands on operands crafted so that the values INSIDE their kernels land on edges (tests/landing.py
sections F, G and I; tests/test_landing_cpu.py shows that every builder lands).

multiply_prepared, multiply_relin_prepared, multiply_sum_prepared and multiply_sum_relin_prepared run mul_mid_pair_kernel: both
operands are the unreduced rows that mul_prep_mid_kernel wrote, and the tensor product, the inverse passes, the store-reduce and the
packing are copies of mul_mid_shared_body's in three bodies (packed FP64, 8-byte FP64, integer), with a sequence at n = 16384 that
loads each operand row twice.  tests/test_gpu_landing_shared.py reaches the shared form only; here BOTH crafted operands sit in
prepared objects, each object holds a fresh decoy that no item names, and neither index is the identity: r_mtilde on its six edges and
the scaled rows on 0, q - 1, 1, (q -+ 1) / 2 enter through prepare's head alone, the floor reads y on its edges through products by
(1, 1) in both orders of the two objects, and the outputs land on 0, q_i - 1 and 1 in every row.

The reference is the oracle product that tests/test_gpu_landing_multiply.py caches; every result must also be torch.equal to the
library's counterpart call on the two gathered arrays.  Every assertion on values is word-for-word equality over all words of all
items and holds under every switch the suite runs with; the kernel names are asserted under the default arms only: on the split path
a product call launches no mul_head and no mul_prep, and its mul_mid units are the item count."""
import os
import subprocess
import sys
import tempfile

import numpy as np
import pytest

from tests import landing as LD
from tests.landing import landing
from tests.test_gpu_landing import DEFAULT_ARMS, _same
from tests.test_gpu_landing_multiply import _products, _relinearized
from tests.test_gpu_landing_shared import HEAD_RUNS, _dev, _nine_reference, _prepare, _replicated, _run_id, _sum_reference, _takes_split, _units

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module", autouse=True)
def _drop():
    yield
    LD.drop_landings()


def _ran_pair(seen, units, split: bool, items: int, what, launches: int = 1):
    """Under the default arms: on the split path no head and no preparation inside a product call and one middle launch over `items`
    operations; off it both gathered operands go through the whole-polynomial kernels."""
    if not DEFAULT_ARMS:
        return
    assert "mul_prep" not in seen, (what, seen)
    if split:
        assert "mul_head" not in seen and seen.get("mul_mid") == launches and units["mul_mid"] == items, (what, seen, units)
        assert "behz_extend" not in seen and "tensor" not in seen, (what, seen)
    else:
        assert seen.get("behz_floor_sk") and "mul_mid" not in seen, (what, seen)


def _pair_products(L, ev, rkd, x, y, ref3, ref2, split, what, launches=1, bi=None, salts=(11, 12)):
    """multiply_prepared (ref3) and multiply_relin_prepared (ref2) of x[i] y[i], both prepared beside a decoy, against the oracle and
    against the library's counterparts on the gathered arrays.  bi: the second index where y is shorter than x (a broadcast)."""
    import torch
    from sunscreen_amd.batch import to_host

    count = len(x)
    ma, da, ai = _prepare(L, ev, x, salts[0])
    mb, db, bi0 = _prepare(L, ev, y, salts[1])
    bi = bi0 if bi is None else bi
    assert len(ai) == len(bi) == count and ai != list(range(count)) and bi != list(range(count)), (ai, bi)
    ga, gb = _replicated(da, ai, count), _replicated(db, bi, count)
    if ref3 is not None:
        out, seen, units = _units(ev, lambda: ev.multiply_prepared(ma, ai, mb, bi))
        print(what, "multiply_prepared:", seen, units)
        _same(to_host(out), ref3, (what, "multiply_prepared"))
        assert torch.equal(out, ev.multiply(ga, gb)), (what, "multiply on the gathered operands")
        _ran_pair(seen, units, split, count, what, launches)
        if DEFAULT_ARMS and split:
            assert seen.get("mul_tail") == launches, (what, seen)
    if ref2 is not None:
        out, seen, units = _units(ev, lambda: ev.multiply_relin_prepared(ma, ai, mb, bi, rkd))
        print(what, "multiply_relin_prepared:", seen, units)
        _same(to_host(out), ref2, (what, "multiply_relin_prepared"))
        assert torch.equal(out, ev.multiply_relin(ga, gb, rkd)), (what, "multiply_relin on the gathered operands")
        _ran_pair(seen, units, split, count, what, launches)
        assert "ks_tail" in seen or "ks_moddown" in seen, (what, seen)
    ev.check()
    ma.close()
    mb.close()


# ---- the head's edges, through prepare alone ---------------------------------------------------------------------------------
@pytest.mark.parametrize("pid,arm,env", HEAD_RUNS, ids=[_run_id(r) for r in HEAD_RUNS])
def test_products_of_two_prepared_operands_with_r_mtilde_and_the_scaled_rows_on_their_edges(pid, arm, env, monkeypatch):
    """LD.mtilde_case with both factors prepared.  P1: FP64; P3: the packed body; P4: the sequence that loads each operand row twice,
    with per-row packing and with 8-byte rows (HIPBFV_PACK_ROWS=0); P5: integer data rows; W4096: the integer body, 60 bits; P1 on the
    integer base.  U1024, W2048 and four items at P3 by count gather both operands from the objects' copies."""
    L = landing(pid)
    a, b = LD.mtilde_case(L)
    ref3 = _products(L, "head", a, b)
    ref2 = _relinearized(L, "head", ref3) if env is None and arm == "split" else None
    ctx, ev, rkd = _dev(L, monkeypatch, arm, env)
    _pair_products(L, ev, rkd, a, b, ref3, ref2, _takes_split(L, len(a), arm), _run_id((pid, arm, env)))


# ---- the floor's inputs and the landed outputs -------------------------------------------------------------------------------
@pytest.mark.parametrize("pid", ["P1", "P3", "P4", "P5", "W4096", "W2048"])
def test_products_by_one_one_in_both_orders_of_the_two_objects(pid, monkeypatch):
    """The four operands of the floor tests times (1, 1), which sits beside a decoy in an object of its own and is named by every
    item: a0 and a1 ARE the tensor's d0 and d2, so the floor reads y on its edges and on q - 1 in all rows at once, and the outputs
    of the harvested operands are 0, q_i - 1 and 1 in every row.  Then the two objects change places."""
    L = landing(pid)
    fo, ones = LD.floor_operands(L), LD.ones_ct(L, 4)
    ref3 = _products(L, "floor", fo, ones)
    kinds = LD.output_case(L)[1]
    for i in range(2):  # the reference IS the target (tests/test_landing_cpu.py)
        assert (ref3[2 + i][0] == LD.kinds_to_words(L.primes, kinds[i, 0])).all() and (ref3[2 + i][2] == LD.kinds_to_words(L.primes, kinds[i, 1])).all()
    ref2 = _relinearized(L, "floor", ref3)
    ctx, ev, rkd = _dev(L, monkeypatch)
    split = _takes_split(L, 4, "split")
    import torch
    from sunscreen_amd.batch import to_host

    mf, df, fi = _prepare(L, ev, fo, 13)
    m1, d1, oi = _prepare(L, ev, ones[:1], 14)
    assert oi == [0] and m1.count == 2 and fi != [0, 1, 2, 3]
    oi = oi * 4
    gf, g1 = _replicated(df, fi, 4), _replicated(d1, oi, 4)
    for order, (mx, xi, gx), (my, yi, gy) in (("crafted x (1, 1)", (mf, fi, gf), (m1, oi, g1)), ("(1, 1) x crafted", (m1, oi, g1), (mf, fi, gf))):
        out, seen, units = _units(ev, lambda: ev.multiply_prepared(mx, xi, my, yi))
        _same(to_host(out), ref3, (pid, order, "multiply_prepared"))
        assert torch.equal(out, ev.multiply(gx, gy)), (pid, order)
        _ran_pair(seen, units, split, 4, (pid, order))
        out, seen, units = _units(ev, lambda: ev.multiply_relin_prepared(mx, xi, my, yi, rkd))
        _same(to_host(out), ref2, (pid, order, "multiply_relin_prepared"))
        assert torch.equal(out, ev.multiply_relin(gx, gy, rkd)), (pid, order, "relin")
        _ran_pair(seen, units, split, 4, (pid, order, "relin"))
    ev.check()
    mf.close()
    m1.close()


# ---- sums through q - 1 ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("pid", ["P3", "P4"])
def test_sums_of_prepared_products_pass_through_q_minus_1(pid, monkeypatch):
    """LD.output_sum_case: three terms whose outputs are 0, q_i - 1, q_i - 1 in some order in every coefficient of polynomials 0 and
    2; the sums are q_i - 2 in every word.  One mul_mid launch, one mul_tail_sum, no head."""
    import torch
    from sunscreen_amd.batch import to_host

    L = landing(pid)
    a, kinds = LD.output_sum_case(L)
    groups, terms = a.shape[:2]
    count = groups * terms
    ref3, ref2 = _sum_reference(L)
    qm2 = np.array(L.primes, dtype=np.uint64)[:, None] - 2
    assert (ref3[:, 0] == qm2).all() and (ref3[:, 2] == qm2).all()
    ctx, ev, rkd = _dev(L, monkeypatch)
    ma, da, ai = _prepare(L, ev, a.reshape((count,) + a.shape[2:]), 15)
    m1, d1, oi = _prepare(L, ev, LD.ones_ct(L, 1), 16)
    oi = oi * count
    assert ai != list(range(count)) and len(ai) == count
    ga, g1 = _replicated(da, ai, count).reshape(a.shape), _replicated(d1, oi, count).reshape(a.shape)
    for order, (mx, xi, gx), (my, yi, gy) in (("crafted x (1, 1)", (ma, ai, ga), (m1, oi, g1)), ("(1, 1) x crafted", (m1, oi, g1), (ma, ai, ga))):
        out, seen, units = _units(ev, lambda: ev.multiply_sum_prepared(mx, xi, my, yi, groups, terms))
        print(pid, order, "multiply_sum_prepared:", seen, units)
        _same(to_host(out), ref3, (pid, order, "multiply_sum_prepared"))
        assert torch.equal(out, ev.multiply_sum(gx, gy)), (pid, order)
        _ran_pair(seen, units, True, count, (pid, order))
        if DEFAULT_ARMS:
            assert seen.get("mul_tail_sum") == 1 and "mul_tail" not in seen and "eltwise" not in seen, seen
        out, seen, units = _units(ev, lambda: ev.multiply_sum_relin_prepared(mx, xi, my, yi, rkd, groups, terms))
        _same(to_host(out), ref2, (pid, order, "multiply_sum_relin_prepared"))
        assert torch.equal(out, ev.multiply_sum_relin(gx, gy, rkd)), (pid, order, "relin")
        _ran_pair(seen, units, True, count, (pid, order, "relin"))
        if DEFAULT_ARMS:
            assert seen.get("mul_tail_sum") == 1 and "ks_tail" in seen, seen
    ev.check()
    ma.close()
    m1.close()


# ---- more than eight operations at n = 16384 ---------------------------------------------------------------------------------
def _nine_pair(L):
    """(first uint64[10][2][K][n], a_index, second uint64[10][2][K][n], b_index): LD.nine_case with its items prepared too, beside
    a decoy of their own."""
    a, prepared, index, refs = LD.nine_case(L)
    first, ai = LD.with_decoy(L, list(a), 17)
    return first, ai, prepared, index


def test_nine_items_over_two_prepared_objects_at_16384(monkeypatch):
    """Nine operations pad to sixteen in the slice-major workgroup order: op = (slot % per) * 8 + xcd takes both of its values, in a
    kernel that reads BOTH operands through an index."""
    import torch
    from sunscreen_amd.batch import to_device, to_host

    L = landing("P4")
    first, ai, second, bi = _nine_pair(L)
    ref = _nine_reference(L)
    assert all(ai[i] != i and bi[i] != i for i in range(9))
    ctx, ev, rkd = _dev(L, monkeypatch)
    da, db = to_device(first), to_device(second)
    ma, mb = ev.prepare(da), ev.prepare(db)
    out, seen, units = _units(ev, lambda: ev.multiply_prepared(ma, ai, mb, bi))
    print("nine items:", seen, units)
    _same(to_host(out), ref, "nine items")
    assert torch.equal(out, ev.multiply(_replicated(da, ai, 9), _replicated(db, bi, 9)))
    _ran_pair(seen, units, True, 9, "nine items")
    ev.check()
    ma.close()
    mb.close()


def test_nine_items_in_the_lane_split_geometry_build():
    """The same case against libhipbfv_geom8.so in a process of its own (a time limit on the child)."""
    lib = os.path.join(ROOT, "sunscreen_amd", "lib", "variants", "libhipbfv_geom8.so")
    assert os.path.exists(lib), "build the variant library first: make -C sunscreen_amd/csrc variants (build() does)"
    L = landing("P4")
    first, ai, second, bi = _nine_pair(L)
    ref = _nine_reference(L)
    script = r"""
import sys, numpy as np, torch
sys.path.insert(0, %r)
from sunscreen_amd import Context
from sunscreen_amd.batch import BatchEvaluator, to_device, to_host
z = np.load(sys.argv[1])
ctx = Context.from_raw(int(z["n"]), [int(p) for p in z["primes"]], int(z["t"]))
ev = BatchEvaluator(ctx)
ma, mb = ev.prepare(to_device(z["first"])), ev.prepare(to_device(z["second"]))
torch.cuda.synchronize()
ev.profile(True)
out = ev.multiply_prepared(ma, [int(i) for i in z["ai"]], mb, [int(i) for i in z["bi"]])
torch.cuda.synchronize()
seen = ev.profile_read()
if %r:  # the default arms
    assert "mul_head" not in seen and "mul_prep" not in seen and seen["mul_mid"]["launches"] == 1 and seen["mul_mid"]["units"] == 9, seen
ev.check()
np.savez(sys.argv[2], out=to_host(out))
""" % (ROOT, DEFAULT_ARMS)
    with tempfile.TemporaryDirectory() as td:
        src, dst = os.path.join(td, "in.npz"), os.path.join(td, "out.npz")
        np.savez(src, n=L.n, primes=np.array(L.key_primes, dtype=np.uint64), t=L.t, first=first, second=second, ai=np.array(ai, dtype=np.int64),
                 bi=np.array(bi, dtype=np.int64))
        subprocess.run([sys.executable, "-c", script, src, dst], env=dict(os.environ, HIPBFV_LIB=lib, HIPBFV_NO_SMALL_BATCH="1"), check=True, timeout=120)
        got = np.load(dst)["out"]
    _same(got, ref, "nine items, geom8")


# ---- an item times itself, from one object -----------------------------------------------------------------------------------
@pytest.mark.parametrize("pid", ["P3", "P4"])
def test_an_item_times_itself_from_one_object(pid, monkeypatch):
    """rows_a == rows_b and the two indexes are equal: the oracle's square, and the words of multiply(a, a)."""
    import torch
    from sunscreen_amd.batch import to_device, to_host

    L = landing(pid)
    a, b = LD.mtilde_case(L)
    sq = np.ascontiguousarray(np.concatenate([a[:2], b[:2]]))  # the operands of test_square_with_r_mtilde_on_its_edges
    ref3 = _products(L, "square", sq, sq)
    ref2 = _relinearized(L, "square", ref3)
    ctx, ev, rkd = _dev(L, monkeypatch)
    m, dm, index = _prepare(L, ev, sq, 7)
    assert index != [0, 1, 2, 3]
    d = to_device(sq)
    out, seen, units = _units(ev, lambda: ev.multiply_prepared(m, index, m, index))
    _same(to_host(out), ref3, (pid, "own square"))
    assert torch.equal(out, ev.multiply(d, d)) and torch.equal(out, ev.multiply(_replicated(dm, index, 4), _replicated(dm, index, 4)))
    _ran_pair(seen, units, True, 4, (pid, "own square"))
    out, seen, units = _units(ev, lambda: ev.multiply_relin_prepared(m, index, m, index, rkd))
    _same(to_host(out), ref2, (pid, "own square, relin"))
    _ran_pair(seen, units, True, 4, (pid, "own square, relin"))
    ev.check()
    m.close()
