"""Prepared multiplicands and weighted sums of products on operands crafted so that the values INSIDE their kernels land on edges
(tests/landing.py sections F, G and I; tests/test_landing_cpu.py shows that every builder lands, that the oracle's multiply is
symmetric on these operands and which edges every weight vector meets).

The *_shared products and the weighted sums run sibling kernels with copies of arithmetic that tests/test_gpu_landing_multiply.py
never reaches: mul_prep_mid_kernel / mul_mid_shared_kernel (their own tensor product, the two-region sequence at n = 16384, the
unreduced 8-byte prepared rows written by one kernel and read by another, the slice-major workgroup order with more than eight
operations) and mul_tail_sum_weighted_kernel / scaled_accumulate_kernel (mul_shoup of a finished residue just before add_mod).

A  "Both roles": the crafted operand is PREPARED and the other one passed as `a` (the head launch inside prepare, mul_prep_mid and
   the b^ loads of mul_mid_shared read it), then the operands are swapped (the two-polynomial head of the product call reads it).
   BFV's tensor is symmetric, so one oracle product is the reference of both.  Every prepared object holds a fresh decoy that no
   item names, and the index is never the identity.
B  Weighted sums of products whose terms come out as 0 and q_i - 1 in every row of polynomials 0 and 2: weighted residues of 0 and
   q_i - 1, partial sums of exactly q_i (the `>= q` compare) and q_i - 1, final words 0, q_i - 1 and 1, and a weight that is 0
   modulo one prime alone.

Every assertion on values is word-for-word equality with the CPU oracle over all words of all items, and holds under every switch
the suite runs with; the kernel names are asserted under the default arms only.  Polynomial 1 of a product by (1, 1) is compared,
not landed."""
import os
import subprocess
import sys
import tempfile

import numpy as np
import pytest

from tests import landing as LD
from tests.landing import landing
from tests.test_gpu_landing import DEFAULT_ARMS, _device, _profiled, _same
from tests.test_gpu_landing_multiply import _products, _relinearized

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module", autouse=True)
def _drop():
    yield
    LD.drop_landings()


def _units(ev, call):
    """The result of call() and what it launched: ({name: launches}, {name: units})."""
    import torch

    ev.profile(True)
    ev.profile_reset()
    try:
        out = call()
        torch.cuda.synchronize()
        prof = ev.profile_read()
    finally:
        ev.profile(False)
    return out, {k: v["launches"] for k, v in prof.items()}, {k: v["units"] for k, v in prof.items()}


def _dev(L, monkeypatch, arm="split", env=None):
    """split: HIPBFV_NO_SMALL_BATCH=1, the pipelines chosen by the parameters alone; by_count: a few items take the whole-polynomial
    kernels.  The split multiply exists for n = 4096 ... 16384."""
    from sunscreen_amd import RelinearizationKeys

    ctx, ev = _device(L, monkeypatch, env, split=arm == "split")
    return ctx, ev, RelinearizationKeys.from_array(ctx, L.rk)


def _has_split(L) -> bool:
    return 12 <= L.n.bit_length() - 1 <= 14


def _takes_split(L, count: int, arm: str) -> bool:
    logn = L.n.bit_length() - 1
    return _has_split(L) and (arm == "split" or not (logn == 13 and count <= 16 or logn == 14 and count <= 4))


def _prepare(L, ev, ops, salt=0, extra_index=()):
    """(multiplicand, the device array that was prepared, index): `ops` beside a decoy, in LD.with_decoy's order."""
    from sunscreen_amd.batch import to_device

    prepared, index = LD.with_decoy(L, list(ops), salt)
    dm = to_device(prepared)
    m, seen, units = _units(ev, lambda: ev.prepare(dm))
    assert m.count == len(prepared), (m.count, len(prepared))
    if DEFAULT_ARMS:
        assert ("mul_prep" in seen) == _has_split(L), seen
        if _has_split(L):
            assert units["mul_prep"] == len(prepared) and units["mul_head"] == 2 * len(prepared), (seen, units)
    return m, dm, index + list(extra_index)


def _replicated(dm, index, count):
    import torch

    return dm.index_select(0, torch.tensor([int(index[i % len(index)]) for i in range(count)], dtype=torch.int64, device=dm.device)).contiguous()


def _ran_shared(seen, units, split: bool, items: int, what, launches: int = 1):
    """Under the default arms: on the split path no preparation inside a product call, one middle launch over `items` operations
    and a head over two polynomials per item; off it the gathered multiplicands go through the whole-polynomial kernels."""
    if not DEFAULT_ARMS:
        return
    assert "mul_prep" not in seen, (what, seen)
    if split:
        assert seen.get("mul_mid") == launches and units["mul_mid"] == items and units["mul_head"] == 2 * items, (what, seen, units)
        assert "behz_extend" not in seen and "tensor" not in seen, (what, seen)
    else:
        assert seen.get("behz_floor_sk") and "mul_mid" not in seen and "mul_head" not in seen, (what, seen)


def _roles(x, y):
    """(name, the operand passed as `a`, the operand prepared)."""
    return (("second operand prepared", x, y), ("first operand prepared", y, x))


def _shared_products(L, ev, rkd, x, y, ref3, ref2, split, what, salt=0, launches=1, extra_index=(), in_place=False):
    """multiply_shared (ref3) and multiply_relin_shared (ref2) of x[i] y[i] in both roles against the oracle and against the
    library's counterpart on the replicated operand."""
    import torch
    from sunscreen_amd.batch import to_device, to_host

    for role, a, b in _roles(x, y):
        m, dm, index = _prepare(L, ev, b, salt, extra_index)
        da, rep = to_device(a), _replicated(dm, index, len(a))
        assert len(set(index[: len(a)])) == 1 or index[: len(a)] != list(range(len(a))), index
        if ref3 is not None:
            out, seen, units = _units(ev, lambda: ev.multiply_shared(da, m, index))
            print(what, role, "multiply_shared:", seen)
            _same(to_host(out), ref3, (what, role, "multiply_shared"))
            assert torch.equal(out, ev.multiply(da, rep)), (what, role, "multiply on the replicated operand")
            _ran_shared(seen, units, split, len(a), (what, role), launches)
            if DEFAULT_ARMS and split:
                assert seen.get("mul_tail") == launches, (what, role, seen)
        if ref2 is not None:
            out, seen, units = _units(ev, lambda: ev.multiply_relin_shared(da, m, index, rkd))
            print(what, role, "multiply_relin_shared:", seen)
            _same(to_host(out), ref2, (what, role, "multiply_relin_shared"))
            assert torch.equal(out, ev.multiply_relin(da, rep, rkd)), (what, role, "multiply_relin on the replicated operand")
            _ran_shared(seen, units, split, len(a), (what, role), launches)
            assert "ks_tail" in seen or "ks_moddown" in seen, (what, role, seen)
            if in_place:
                buf = da.clone()
                got = ev.multiply_relin_shared(buf, m, index, rkd, out=buf)
                assert got.data_ptr() == buf.data_ptr()
                _same(to_host(got), ref2, (what, role, "multiply_relin_shared with out = a"))
        ev.check()
        m.close()


# ---- A1: the head's edges through prepare and through the product ------------------------------------------------------------
HEAD_RUNS = [("P1", "split", None), ("P3", "split", None), ("P4", "split", None), ("P4", "split", {"HIPBFV_PACK_ROWS": "0"}),
             ("P5", "split", None), ("W4096", "split", None), ("P1", "split", {"HIPBFV_NO_F64": "1"}),
             ("U1024", "split", None), ("W2048", "split", None), ("P3", "by_count", None)]


def _run_id(run):
    pid, arm, env = run
    return "-".join([pid, arm] + [f"{k}={v}" for k, v in (env or {}).items()])


@pytest.mark.parametrize("pid,arm,env", HEAD_RUNS, ids=[_run_id(r) for r in HEAD_RUNS])
def test_multiply_shared_with_r_mtilde_and_the_scaled_rows_on_their_edges(pid, arm, env, monkeypatch):
    """LD.mtilde_case: r_mtilde on its six edges in every polynomial, y on 0, q - 1, 1, (q -+ 1) / 2 and every row at q - 1 at once,
    in the prepared operand and in `a`.  P1: FP64; P3: packed, three regions; P4: two regions, per-row packing, and 8-byte rows; P5:
    integer data rows; W4096: all integer, 60 bits; P1 on the integer base.  U1024, W2048 and four items at P3 without
    HIPBFV_NO_SMALL_BATCH gather the multiplicands from the object's copy."""
    L = landing(pid)
    a, b = LD.mtilde_case(L)
    ref = _products(L, "head", a, b)
    ctx, ev, rkd = _dev(L, monkeypatch, arm, env)
    _shared_products(L, ev, rkd, a, b, ref, None, _takes_split(L, len(a), arm), _run_id((pid, arm, env)))


# ---- A2: through the fused pair ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("pid", ["P3", "P5", "P4"])
def test_multiply_relin_shared_with_r_mtilde_on_its_edges(pid, monkeypatch):
    """The fused multiply + relinearize over a prepared multiplicand (P5: the mixed pair); at P3 once more with out exactly a."""
    L = landing(pid)
    a, b = LD.mtilde_case(L)
    ref = _relinearized(L, "head", _products(L, "head", a, b))
    ctx, ev, rkd = _dev(L, monkeypatch)
    _shared_products(L, ev, rkd, a, b, None, ref, True, (pid, "relin"), in_place=pid == "P3")


# ---- A3: the floor's inputs and the landed outputs ---------------------------------------------------------------------------
@pytest.mark.parametrize("pid", ["P1", "P3", "P4", "P5", "W4096", "W2048"])
def test_shared_products_by_one_one_put_the_floor_inputs_and_the_outputs_on_their_edges(pid, monkeypatch):
    """The four operands of the floor tests times (1, 1).  With (1, 1) prepared once beside the decoy (broadcast index) the b^ rows
    are the transform of 1 and a0, a1 ARE d0, d2; with the four crafted operands prepared and a = (1, 1) the prepared rows carry
    them.  y on its edges and on q - 1 in all rows at once in front of the floor, outputs 0, q_i - 1 and 1 in every row.  W2048
    through the gathered multiplicands."""
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
    from sunscreen_amd.batch import to_device, to_host

    # (1, 1) prepared once: index [0], the decoy at place 1
    m, dm, index = _prepare(L, ev, ones[:1], 3)
    assert index == [0] and m.count == 2
    da, rep = to_device(fo), _replicated(dm, index, 4)
    out, seen, units = _units(ev, lambda: ev.multiply_shared(da, m, index))
    _same(to_host(out), ref3, (pid, "(1, 1) prepared", "multiply_shared"))
    assert torch.equal(out, ev.multiply(da, rep))
    _ran_shared(seen, units, split, 4, (pid, "(1, 1) prepared"))
    out, seen, units = _units(ev, lambda: ev.multiply_relin_shared(da, m, index, rkd))
    _same(to_host(out), ref2, (pid, "(1, 1) prepared", "multiply_relin_shared"))
    assert torch.equal(out, ev.multiply_relin(da, rep, rkd))
    _ran_shared(seen, units, split, 4, (pid, "(1, 1) prepared, relin"))
    ev.check()
    m.close()
    # the four crafted operands prepared, a = (1, 1)
    m, dm, index = _prepare(L, ev, fo, 3)
    da, rep = to_device(ones), _replicated(dm, index, 4)
    out, seen, units = _units(ev, lambda: ev.multiply_shared(da, m, index))
    _same(to_host(out), ref3, (pid, "crafted prepared", "multiply_shared"))
    assert torch.equal(out, ev.multiply(da, rep))
    _ran_shared(seen, units, split, 4, (pid, "crafted prepared"))
    out, seen, units = _units(ev, lambda: ev.multiply_relin_shared(da, m, index, rkd))
    _same(to_host(out), ref2, (pid, "crafted prepared", "multiply_relin_shared"))
    assert torch.equal(out, ev.multiply_relin(da, rep, rkd))
    _ran_shared(seen, units, split, 4, (pid, "crafted prepared, relin"))
    ev.check()
    m.close()


# ---- A4: sums through q - 1 --------------------------------------------------------------------------------------------------
def _sum_reference(L):
    """(ref3, ref2): the oracle's add of the oracle's products of LD.output_sum_case by (1, 1), and its relinearization."""

    def make():
        prods = LD.output_sum_products(L)
        sums = []
        for g in range(prods.shape[0]):
            acc = prods[g, 0]
            for j in range(1, prods.shape[1]):
                acc = L.o.add(acc, prods[g, j])
            sums.append(acc)
        return np.stack(sums), np.stack([L.o.relinearize(s, L.rk) for s in sums])

    return L.cached("shared output sums reference", make)


@pytest.mark.parametrize("pid", ["P3", "P4"])
def test_shared_sums_of_products_pass_through_q_minus_1(pid, monkeypatch):
    """Three terms whose outputs are 0, q_i - 1, q_i - 1 in some order in every coefficient of polynomials 0 and 2, summed by
    multiply_sum_shared and multiply_sum_relin_shared: (1, 1) prepared and broadcast, then all groups x terms crafted operands
    prepared (index_len == count) and a = (1, 1).  Polynomials 0 and 2 of the sums are q_i - 2 in every word."""
    import torch
    from sunscreen_amd.batch import to_device, to_host

    L = landing(pid)
    a, kinds = LD.output_sum_case(L)
    groups, terms = a.shape[:2]
    count = groups * terms
    ones = LD.ones_ct(L, count).reshape(a.shape)
    ref3, ref2 = _sum_reference(L)
    qm2 = np.array(L.primes, dtype=np.uint64)[:, None] - 2
    assert (ref3[:, 0] == qm2).all() and (ref3[:, 2] == qm2).all()
    ctx, ev, rkd = _dev(L, monkeypatch)
    flat = a.reshape((count,) + a.shape[2:])
    for what, x, prep in (("(1, 1) prepared", a, ones.reshape(flat.shape)[:1]), ("crafted prepared", ones, flat)):
        m, dm, index = _prepare(L, ev, prep, 4)
        assert len(index) in (1, count)
        da, rep = to_device(x), _replicated(dm, index, count).reshape(a.shape)
        out, seen, units = _units(ev, lambda: ev.multiply_sum_shared(da, m, index))
        print(pid, what, "multiply_sum_shared:", seen)
        _same(to_host(out), ref3, (pid, what, "multiply_sum_shared"))
        assert torch.equal(out, ev.multiply_sum(da, rep))
        _ran_shared(seen, units, True, count, (pid, what))
        if DEFAULT_ARMS:
            assert seen.get("mul_tail_sum") == 1 and "mul_tail" not in seen and "eltwise" not in seen, seen
        out, seen, units = _units(ev, lambda: ev.multiply_sum_relin_shared(da, m, index, rkd))
        _same(to_host(out), ref2, (pid, what, "multiply_sum_relin_shared"))
        assert torch.equal(out, ev.multiply_sum_relin(da, rep, rkd))
        _ran_shared(seen, units, True, count, (pid, what, "relin"))
        if DEFAULT_ARMS:
            assert seen.get("mul_tail_sum") == 1 and "ks_tail" in seen, seen
        ev.check()
        m.close()


# ---- A5: more than eight operations at n = 16384 -----------------------------------------------------------------------------
def _nine_reference(L):
    a, prepared, index, refs = LD.nine_case(L)
    fam = {"head": _products(L, "head", *LD.mtilde_case(L)), "floor": _products(L, "floor", LD.floor_operands(L), LD.ones_ct(L, 4))}
    return np.stack([fam[f][k] for f, k in refs])


def test_nine_items_over_nine_prepared_ciphertexts_at_16384(monkeypatch):
    """The slice-major workgroup order of n = 16384 pads the operations to a multiple of 8: with 10 prepared ciphertexts and 9 items
    per = (ops + 7) >> 3 is 2 in mul_prep_mid_kernel and in mul_mid_shared_kernel, and op = (slot % per) * 8 + xcd takes both of its
    values.  The four crafted head multiplicands, (1, 1) and the four floor operands prepared, each named once, none at its own
    place."""
    import torch
    from sunscreen_amd.batch import to_device, to_host

    L = landing("P4")
    a, prepared, index, refs = LD.nine_case(L)
    ref = _nine_reference(L)
    ctx, ev, rkd = _dev(L, monkeypatch)
    dm = to_device(prepared)
    m, seen, units = _units(ev, lambda: ev.prepare(dm))
    if DEFAULT_ARMS:
        assert seen.get("mul_prep") == 1 and units["mul_prep"] == 10 and units["mul_head"] == 20, (seen, units)
    da = to_device(a)
    out, seen, units = _units(ev, lambda: ev.multiply_shared(da, m, index))
    print("nine items:", seen, units)
    _same(to_host(out), ref, "nine items")
    assert torch.equal(out, ev.multiply(da, _replicated(dm, index, 9)))
    _ran_shared(seen, units, True, 9, "nine items")
    ev.check()
    m.close()


def test_nine_items_in_the_lane_split_geometry_build(monkeypatch):
    """The same case against libhipbfv_geom8.so in a process of its own (a time limit on the child): the words of the default
    build in this process, which are the oracle's."""
    from sunscreen_amd.batch import to_device, to_host

    lib = os.path.join(ROOT, "sunscreen_amd", "lib", "variants", "libhipbfv_geom8.so")
    assert os.path.exists(lib), "build the variant library first: make -C sunscreen_amd/csrc variants (build() does)"
    L = landing("P4")
    a, prepared, index, refs = LD.nine_case(L)
    ref = _nine_reference(L)
    script = r"""
import sys, numpy as np, torch
sys.path.insert(0, %r)
from sunscreen_amd import Context
from sunscreen_amd.batch import BatchEvaluator, to_device, to_host
z = np.load(sys.argv[1])
ctx = Context.from_raw(int(z["n"]), [int(p) for p in z["primes"]], int(z["t"]))
ev = BatchEvaluator(ctx)
ev.profile(True)
m = ev.prepare(to_device(z["prepared"]))
out = ev.multiply_shared(to_device(z["a"]), m, [int(i) for i in z["index"]])
torch.cuda.synchronize()
seen = ev.profile_read()
if %r:  # the default arms
    assert seen["mul_prep"]["units"] == 10 and seen["mul_mid"]["launches"] == 1 and seen["mul_mid"]["units"] == 9, seen
ev.check()
np.savez(sys.argv[2], out=to_host(out))
""" % (ROOT, DEFAULT_ARMS)
    with tempfile.TemporaryDirectory() as td:
        src, dst = os.path.join(td, "in.npz"), os.path.join(td, "out.npz")
        np.savez(src, n=L.n, primes=np.array(L.key_primes, dtype=np.uint64), t=L.t, a=a, prepared=prepared, index=np.array(index, dtype=np.int64))
        subprocess.run([sys.executable, "-c", script, src, dst], env=dict(os.environ, HIPBFV_LIB=lib, HIPBFV_NO_SMALL_BATCH="1"), check=True, timeout=120)
        got = np.load(dst)["out"]
    ctx, ev, rkd = _dev(L, monkeypatch)
    m = ev.prepare(to_device(prepared))
    here = to_host(ev.multiply_shared(to_device(a), m, index))
    m.close()
    _same(got, here, "nine items, geom8 against the default build")
    _same(got, ref, "nine items, geom8")


# ---- A6: a slice that starts inside the index --------------------------------------------------------------------------------
def test_a_chunk_that_starts_inside_the_index(monkeypatch):
    """P3, the four head items, three operations per launch: the second launch starts at item 3 of an index of length 5 (its last
    entry names the decoy and is never reached)."""
    L = landing("P3")
    a, b = LD.mtilde_case(L)
    ref = _products(L, "head", a, b)
    ctx, ev, rkd = _dev(L, monkeypatch, env={"HIPBFV_CHUNK_OPS": "3"})
    _shared_products(L, ev, rkd, a, b, ref, _relinearized(L, "head", ref), True, "chunks of 3", launches=2, extra_index=(1,))


# ---- A7: the same ciphertext on both sides -----------------------------------------------------------------------------------
@pytest.mark.parametrize("pid", ["P3", "P4"])
def test_an_item_times_its_own_prepared_copy(pid, monkeypatch):
    """a[i] is the ciphertext that was prepared: the oracle's square, and the words of multiply(a, a) (the squaring middle kernel)."""
    import torch
    from sunscreen_amd.batch import to_device, to_host

    L = landing(pid)
    a, b = LD.mtilde_case(L)
    sq = np.ascontiguousarray(np.concatenate([a[:2], b[:2]]))  # the operands of test_square_with_r_mtilde_on_its_edges
    ref = _products(L, "square", sq, sq)
    ctx, ev, rkd = _dev(L, monkeypatch)
    m, dm, index = _prepare(L, ev, sq, 7)
    d = to_device(sq)
    out, seen, units = _units(ev, lambda: ev.multiply_shared(d, m, index))
    _same(to_host(out), ref, (pid, "own prepared copy"))
    assert torch.equal(out, ev.multiply(d, d)) and torch.equal(out, ev.multiply(d, _replicated(dm, index, 4)))
    _ran_shared(seen, units, True, 4, (pid, "own prepared copy"))
    ev.check()
    m.close()


# ---- B: weighted sums on landed outputs --------------------------------------------------------------------------------------
def _weighted(L, ev, rkd, weights, what):
    """multiply_sum_weighted and multiply_sum_weighted_relin of LD.weighted_sum_case against the sums in Python integers and the
    oracle's relinearization of them; what both calls launched."""
    from sunscreen_amd.batch import to_device, to_host

    a, want3, events = LD.weighted_sum_case(L, weights)
    want2 = L.cached(("weighted relinearized", tuple(weights)), lambda: np.stack([L.o.relinearize(s, L.rk) for s in want3]))
    da = to_device(a)
    db = to_device(LD.ones_ct(L, a.shape[0] * a.shape[1]).reshape(a.shape))
    out3, seen3 = _profiled(ev, lambda: ev.multiply_sum_weighted(da, db, weights))
    print(what, weights, "raw q:", [int(v) for v in events["raw q"]], "zero weight:", [int(v) for v in events["zero weight"]], seen3)
    _same(to_host(out3), want3, (what, weights, "multiply_sum_weighted"))
    out2, seen2 = _profiled(ev, lambda: ev.multiply_sum_weighted_relin(da, db, weights, rkd))
    _same(to_host(out2), want2, (what, weights, "multiply_sum_weighted_relin"))
    ev.check()
    return seen3, seen2


def _weighted_all(L, ev, rkd, vectors, what, ran):
    """Every weight vector is run, and the ones whose words differ are named together with the edges they meet: a compare that is
    wrong at exactly q_i shows in the vectors that count a raw sum of q_i and in no other."""
    differ = []
    for w in vectors:
        try:
            seen3, seen2 = _weighted(L, ev, rkd, w, what)
        except AssertionError as e:
            print(what, w, "differs:", str(e)[:400])
            ev_ = LD.weighted_sum_case(L, w)[2]
            differ.append((w, "raw q in a row: %d, in polynomial 1: %d" % (int(ev_["raw q"].max()), int(ev_["raw q in polynomial 1"].max()))))
            continue
        if DEFAULT_ARMS:
            for seen in (seen3, seen2):
                assert ran(seen), (what, w, seen)
    assert not differ, f"weight vectors whose words differ: {differ}"


def _one_summing_tail(seen):
    return seen.get("mul_tail_sum") == 1 and "mul_tail" not in seen and "eltwise" not in seen and "behz_floor_sk" not in seen


WEIGHTED_SPLIT_RUNS = [("P3", None), ("P4", None), ("P4", {"HIPBFV_PACK_ROWS": "0"}), ("P5", None), ("W4096", None)]


@pytest.mark.parametrize("pid,env", WEIGHTED_SPLIT_RUNS, ids=[_run_id((p, "split", e)) for p, e in WEIGHTED_SPLIT_RUNS])
def test_weighted_sums_on_landed_outputs(pid, env, monkeypatch):
    """B1, mul_tail_sum_weighted_kernel: P3 (the 4-prime register-held sums, FP64), P4 (through the output rows), P5 (the mixed
    register-held sums), W4096 (mul_tail_sum_term_int).  (1, -1, 1) puts a partial sum of exactly q_i in two coefficients of three;
    (2^31 - 1, -(2^31 - 1), 1) does with weights that are not small; (-2^31, 2^31 - 1, 1) ends on 1 and (3, -2, -1) on q_i - 1."""
    L = landing(pid)
    ctx, ev, rkd = _dev(L, monkeypatch, env=env)
    _weighted_all(L, ev, rkd, LD.WEIGHT_VECTORS, pid, _one_summing_tail)


def test_weighted_sums_across_a_slice_boundary(monkeypatch):
    """B2, P3 with two operations per launch: every group arrives in slices of 2 and 1 terms, so the sum that is exactly q_i is
    formed onto the words an earlier launch left (`accumulate`), with the weight table read from row term0."""
    L = landing("P3")
    ctx, ev, rkd = _dev(L, monkeypatch, env={"HIPBFV_CHUNK_OPS": "2"})
    _weighted_all(L, ev, rkd, LD.WEIGHT_VECTORS, "P3, chunks of 2", lambda seen: seen.get("mul_tail_sum") == 4 and "eltwise" not in seen)


@pytest.mark.parametrize("pid", ["W2048", "U1024"])
def test_weighted_sums_on_the_folded_path(pid, monkeypatch):
    """B3, scaled_accumulate_kernel below the split kernels: one launch per term and group.  At U1024 also (q_1, -q_1, 1) -- a
    weight that is 0 modulo the 30-bit prime q_1 alone, from nonzero products -- and (2 q_1 - 2^31, 2^31 - 1, -2^31), weights
    above a modulus."""
    L = landing(pid)
    ctx, ev, rkd = _dev(L, monkeypatch)
    vectors = list(LD.WEIGHT_VECTORS) + (LD.modulus_weights(L) if pid == "U1024" else [])
    _weighted_all(L, ev, rkd, vectors, pid, lambda seen: seen.get("eltwise") == 2 * 3 and "mul_tail_sum" not in seen and seen.get("behz_floor_sk"))


def test_weighted_sums_with_30_bit_primes_at_4096(monkeypatch):
    """B4, S4096 = 30, 30 and 40-bit data primes at n = 4096: an int32 weight wraps both 30-bit moduli.  The four weight vectors and
    the two modulus-sized ones.  The library takes the SPLIT path here (read from the profiler on an MI355X: mul_head, mul_mid and one
    mul_tail_sum per call, no eltwise), and every key prime has an FP64 range plan: the register-held FP64 sums of
    mul_tail_sum_weighted_kernel with three data primes, the fourth row idle."""
    from tests.test_gpu_landing import _fp64_split

    L = landing("S4096")
    assert _fp64_split(L)
    ctx, ev, rkd = _dev(L, monkeypatch)
    _weighted_all(L, ev, rkd, list(LD.WEIGHT_VECTORS) + LD.modulus_weights(L), "S4096", _one_summing_tail)
