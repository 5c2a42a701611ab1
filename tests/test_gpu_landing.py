"""Kernels that end in a canonicalisation or a modular add, on operands crafted so that their OUTPUT lands on an exact edge.

Random residues and real encryptions put a result of exactly 0, exactly q - 1, or a pre-reduction integer that is a multiple of q in
front of a kernel about once in 2^40 words; tests/landing.py builds operands that put one in front of every thread (the method and
its reach are described there; tests/test_landing_cpu.py shows that every builder lands all of its words in the oracle).  Here every
assertion is word-for-word equality with the CPU oracle over all words of all items, and every test reads the profiler to see that
the kernel it is about ran: `ks_tail` (ks_tail, mulrelin_tail and mulrelin_tail_mixed report under that name), `ks_moddown`,
`eltwise`, `plain`, `ntt_inv`.  plain_addsub_kernel and the decryption's rounding are launched outside the profiler's table: their
tests assert the launches around them.

Sections: A stand-alone key-switch tails, B sums folded into the last kernel of a program step, C element-wise / plaintext / n-ary
kernels, D the product accumulators of the transform-domain matrix product, E decrypt."""
import os

import numpy as np
import pytest

from tests import landing as LD
from tests.landing import landing
from tests.oracle_program import run_program

pytestmark = pytest.mark.gpu

SWITCHES = ("HIPBFV_PROGRAM_SERIAL", "HIPBFV_NO_MEMBER_TAILS", "HIPBFV_NO_MERGED_PRODUCTS")
# the suite also runs under switches that take the multiply + relinearize off its fused FP64 tail: the launch counts differ there
DEFAULT_ARMS = not any(os.environ.get(k) == "1" for k in ("HIPBFV_NO_F64", "HIPBFV_SEAL_AUX", "HIPBFV_NO_FUSED_TAIL", "HIPBFV_NO_FUSED_HEAD"))


@pytest.fixture(scope="module", autouse=True)
def _drop():
    yield
    LD.drop_landings()


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


def _device(L, monkeypatch, env=None, split=True):
    """A fresh context and evaluator for L's parameters.  The switches are read when they are made: HIPBFV_NO_SMALL_BATCH=1 (split)
    sends a few items through the split kernels, without it the parameters and the count decide."""
    from sunscreen_amd import Context
    from sunscreen_amd.batch import BatchEvaluator

    for k, v in (env or {}).items():
        monkeypatch.setenv(k, v)
    if split:
        monkeypatch.setenv("HIPBFV_NO_SMALL_BATCH", "1")
    else:
        monkeypatch.delenv("HIPBFV_NO_SMALL_BATCH", raising=False)
    ctx = Context.from_raw(L.n, L.key_primes, L.t)
    assert ctx.K == L.K and ctx.key_primes == L.key_primes
    return ctx, BatchEvaluator(ctx)


def _same(got, want, what):
    assert got.shape == want.shape, (what, got.shape, want.shape)
    for i in range(len(want)):
        bad = np.argwhere(got[i] != want[i])
        assert bad.size == 0, (what, "item", i, "first difference at", bad[0].tolist(), int(got[i][tuple(bad[0])]), int(want[i][tuple(bad[0])]), len(bad))


def _fp64_split(L) -> bool:
    """Every key prime of L has an FP64 range plan for the split pipelines at L's degree (host only)."""
    import ctypes as C

    from sunscreen_amd import _lib

    out = (C.c_uint32 * 6)()
    for p in L.key_primes:
        assert _lib.load().hipbfv_debug_f64_plan(p, L.n.bit_length() - 1, out) == 0
        if not (out[0] and out[3]):
            return False
    return True


# ---- A: stand-alone key-switch tails ---------------------------------------------------------------------------------------
def _relin_reference(L):
    """The oracle's relinearizations of the crafted inputs (the transparent one with the exception switched off)."""

    def make():
        (ct3, want, names), (tr, tr_want) = L.relin_items()
        ref = np.stack([L.o.relinearize(c, L.rk) for c in ct3])
        L.o.throw_on_transparent = False
        try:
            tr_ref = L.o.relinearize(tr[0], L.rk)[None]
        finally:
            L.o.throw_on_transparent = True
        return ref, tr_ref

    return L.cached("relin reference", make)


RELIN_RUNS = [(p, True) for p in ("P1", "P2", "P3", "P4", "P5", "P6")] + [("P1", False), ("P3", False), ("P4", False)]


@pytest.mark.parametrize("pid,split", RELIN_RUNS, ids=[f"{p}-{'split' if s else 'by_count'}" for p, s in RELIN_RUNS])
def test_relinearize_lands_on_the_edges(pid, split, monkeypatch):
    """A1 / A2.  Both output polynomials on the pattern; polynomial 0 all 0; all q - 1; a random control; polynomial 1 all 0 but its
    very last word (returned bit-exact, not reported); then, in a call of its own, polynomial 1 all 0: reported transparent, as the
    oracle does.  P1 ... P6 through the split kernels; P1, P3 and P4 again with the pipeline chosen by the count (n = 16384 sends up
    to four items through the whole-polynomial kernels, so the first four items run there and end in ks_moddown)."""
    from sunscreen_amd import HipBfvError, RelinearizationKeys
    from sunscreen_amd.batch import to_device, to_host

    L = landing(pid)
    (ct3, want, names), (tr, tr_want) = L.relin_items()
    ref, tr_ref = _relin_reference(L)
    if pid == "P2":
        assert L.key_primes[-1] < max(L.key_primes[:-1]) and _fp64_split(L)  # the FP64 split kernels, p below a data prime
    if pid in ("P1", "P3", "P4"):
        assert _fp64_split(L)
    whole = not split and pid == "P4"
    if whole:
        ct3, ref, names = ct3[[0, 1, 2, 4]], ref[[0, 1, 2, 4]], [names[i] for i in (0, 1, 2, 4)]
    ctx, ev = _device(L, monkeypatch, split=split)
    rkd = RelinearizationKeys.from_array(ctx, L.rk)
    out, seen = _profiled(ev, lambda: ev.relinearize(to_device(ct3), rkd))
    print(pid, split, "relinearize:", seen)
    _same(to_host(out), ref, (pid, split, names))
    ev.check()  # the almost transparent item is not reported
    if whole:
        assert seen.get("ks_moddown") == 1 and "ks_tail" not in seen, seen
    else:
        assert seen.get("ks_tail") == 1 and seen.get("ks_head") == 1 and "ks_moddown" not in seen, seen
    out, seen = _profiled(ev, lambda: ev.relinearize(to_device(tr), rkd))
    assert ("ks_moddown" in seen) if whole else ("ks_tail" in seen), seen
    _same(to_host(out), tr_ref, (pid, split, "transparent"))
    with pytest.raises(HipBfvError, match="transparent"):
        ev.check()
    ev.check()


def _rotation_reference(L, elt):
    return L.cached(("rot reference", elt), lambda: np.stack([L.o.apply_galois(c, elt, L.galois_keys([elt])) for c in L.rotation_items(elt)[0]]))


@pytest.mark.parametrize("pid", ["P1", "P2", "P3", "P4", "P5"])
def test_rotations_land_polynomial_0_on_the_edges(pid, monkeypatch):
    """A3 / A4 / A5.  apply_galois, rotate_rows by 1 and by -3, rotate_columns with direct keys: polynomial 0 = sigma(c0) + ks0 landed
    through sigma^-1 on the pattern, on 0 and on q - 1; a random control; an item whose c1 cycles 0, q - 1, 1 (zeros and q - 1 under
    the sign flips of the gathers).  The same arrays under HIPBFV_NO_FUSED_GALOIS=1 in a fresh context give the same bits."""
    from sunscreen_amd import GaloisKeys
    from sunscreen_amd.batch import to_device, to_host

    L = landing(pid)
    ops = L.rotation_ops()
    gk = L.galois_keys([elt for _, elt, _ in ops])
    fused_by_default = os.environ.get("HIPBFV_NO_FUSED_GALOIS") != "1"
    outs = {}
    for env in ({}, {"HIPBFV_NO_FUSED_GALOIS": "1"}):
        ctx, ev = _device(L, monkeypatch, env)
        gkd = GaloisKeys.from_arrays(ctx, gk)
        for name, elt, step in ops:
            ct, want, names = L.rotation_items(elt)
            ref = _rotation_reference(L, elt)
            d = to_device(ct)
            if step is not None:
                call = lambda: ev.rotate_rows(d, step, gkd)  # noqa: E731
            elif elt == 2 * L.n - 1:
                call = lambda: ev.rotate_columns(d, gkd)  # noqa: E731
            else:
                call = lambda: ev.apply_galois(d, elt, gkd)  # noqa: E731
            out, seen = _profiled(ev, call)
            _same(to_host(out), ref, (pid, name, env, names))
            ev.check()
            assert seen.get("ks_tail") == 1 and seen.get("ks_head") == 1, (name, env, seen)
            assert ("galois" in seen) == (bool(env) or not fused_by_default), (name, env, seen)
            if env:
                assert (to_host(out) == outs[name]).all(), name
            else:
                outs[name] = to_host(out)


# ---- B: sums fused into the last kernel, through FheProgram ----------------------------------------------------------------
def _fold_program():
    """One product m = relinearize(multiply(x, y)) per graph, used only by its sum: m +- z, 2 m +- z, 3 m +- z, 4 m +- z (z: inputs
    2 ... 9, LD.FOLDS), and m + m alone."""
    from sunscreen_amd.program import FheProgram

    p = FheProgram()
    x, y = p.append_input_ciphertext(0), p.append_input_ciphertext(1)
    zs = [p.append_input_ciphertext(2 + g) for g in range(len(LD.FOLDS))]
    for g, (mult, sign) in enumerate(LD.FOLDS):
        m = p.append_relinearize(p.append_multiply(x, y))
        acc = m
        for _ in range(mult - 1):
            acc = p.append_add(acc, m)
        p.append_output_ciphertext((p.append_add if sign > 0 else p.append_sub)(acc, zs[g]))
    m = p.append_relinearize(p.append_multiply(x, y))
    p.append_output_ciphertext(p.append_add(m, m))
    return p


def _rotsum_program():
    from sunscreen_amd.program import FheProgram

    p = FheProgram()
    x, z1, z2 = (p.append_input_ciphertext(i) for i in range(3))
    p.append_output_ciphertext(p.append_add(p.append_rotate_left(x, p.append_input_literal(LD.ROT_STEP)), z1))
    p.append_output_ciphertext(p.append_add(p.append_swap_rows(x), z2))
    return p


def _take(a, batch):
    """The first `batch` input sets of a: the DISTINCT ones repeated."""
    return np.ascontiguousarray(a[np.arange(batch) % len(a)])


def _run_all_ways(p, ev, dev, rkd, gkd, monkeypatch):
    """The scheduled run (with the kernels it launched), the node-by-node run, the run without member tails and the run with a
    launch per product (member by member)."""
    from sunscreen_amd.batch import to_host

    for k in SWITCHES:
        monkeypatch.delenv(k, raising=False)
    got, seen = _profiled(ev, lambda: [to_host(t) for t in p.run(ev, dev, rkd, gkd)])
    others = {}
    for k in SWITCHES:
        monkeypatch.setenv(k, "1")
        others[k] = [to_host(t) for t in p.run(ev, dev, rkd, gkd)]
        monkeypatch.delenv(k, raising=False)
    return got, seen, others


def _program_reference(L, key, p, inputs, gk=None):
    """run_program of every DISTINCT input set (the oracle remembers the product of a pair of factors it has seen)."""

    def make():
        memo = LD.MemoOracle(L.o)
        return [run_program(memo, p.nodes, p.edges, [a[i] for a in inputs], L.rk, gk) for i in range(LD.DISTINCT)]

    return L.cached(key, make)


@pytest.mark.parametrize("pid", ["P1", "P4", "P5"])
def test_sums_folded_into_the_product_tails_land_on_the_edges(pid, monkeypatch):
    """B1, B3, B4, B5 for mult * m +- z (the MemberTail arm of the fused multiply + relinearize; the mixed tail on P5): every sum
    lands on the pattern through its addend; batches 1, 2 and 40."""
    from sunscreen_amd import HipBfvError, RelinearizationKeys
    from sunscreen_amd.batch import to_device

    L = landing(pid)
    x, y, m, z, T = LD.fold_case(L)
    p = _fold_program()
    desc = p.describe()
    if pid != "P5":
        assert _fp64_split(L) and desc[0].startswith("mul_relin members=9") and "lin_foldable=9" in desc[0], desc
    inputs = [x, y] + z
    ref = _program_reference(L, "fold reference", p, inputs)
    for i in range(LD.DISTINCT):
        for g in range(len(LD.FOLDS)):
            assert (ref[i][g] == T[g][i]).all()  # (what tests/test_landing_cpu.py shows: the reference IS the target)
    ctx, ev = _device(L, monkeypatch)
    rkd = RelinearizationKeys.from_array(ctx, L.rk)
    for batch in (1, 2, 40):
        dev = [to_device(_take(a, batch)) for a in inputs]
        got, seen, others = _run_all_ways(p, ev, dev, rkd, None, monkeypatch)
        print(pid, batch, "folded sums:", seen)
        assert "ks_tail" in seen, seen
        if pid != "P5" and DEFAULT_ARMS:  # all nine sums were written by the fused tail of ONE merged launch: no sum kernel, no multiply tail
            assert seen == {"mul_head": 1, "mul_mid": 1, "ks_head": 1, "ks_mid": 1, "ks_tail": 1}, seen
        for k in range(len(got)):
            _same(got[k], np.stack([ref[i % LD.DISTINCT][k] for i in range(batch)]), (pid, batch, "graph", k))
            for name, other in others.items():
                assert (other[k] == got[k]).all(), (pid, batch, k, name)
        ev.check()
    # B5: exactly one input set's addend lands polynomial 1 of m + z on all zeros
    bad = 2
    zt = _take(z[0], 4).copy()
    zt[bad] = LD.fold_transparent_addend(L, bad)
    dev = [to_device(_take(a, 4)) for a in inputs]
    dev[2] = to_device(zt)
    with pytest.raises(HipBfvError, match=f"transparent \\(input set {bad} "):
        p.run(ev, dev, rkd)
    with pytest.raises(RuntimeError, match="transparent"):
        run_program(LD.MemoOracle(L.o), p.nodes, p.edges, [x[bad], y[bad], zt[bad]] + [a[bad] for a in z[1:]], L.rk)
    ev.check()
    p.run(ev, [to_device(_take(a, 4)) for a in inputs], rkd)  # input set 3 of graph 0: all zero but the last word -- clean
    ev.check()


@pytest.mark.parametrize("pid", ["P1", "P4", "P5"])
def test_sums_folded_into_the_rotation_tails_land_on_the_edges(pid, monkeypatch):
    """B2 ... B5 for rotate_left(x, 1) + z and swap_rows(x) + z with direct keys (the addend of ks_tail): both polynomials of both
    sums land on the pattern."""
    from sunscreen_amd import GaloisKeys, HipBfvError
    from sunscreen_amd.batch import to_device

    L = landing(pid)
    x, gk, z_rot, z_swap, T_rot, T_swap, r = LD.rotsum_case(L)
    p = _rotsum_program()
    rot = [line for line in p.describe() if line.startswith("rotate")]
    assert len(rot) == 2 and all("add_foldable=1" in line for line in rot), p.describe()
    inputs = [x, z_rot, z_swap]
    ref = _program_reference(L, "rotsum reference", p, inputs, gk)
    for i in range(LD.DISTINCT):
        assert (ref[i][0] == T_rot[i]).all() and (ref[i][1] == T_swap[i]).all()
    ctx, ev = _device(L, monkeypatch)
    gkd = GaloisKeys.from_arrays(ctx, gk)
    for batch in (1, 2, 40):
        dev = [to_device(_take(a, batch)) for a in inputs]
        got, seen, others = _run_all_ways(p, ev, dev, None, gkd, monkeypatch)
        print(pid, batch, "rotation sums:", seen)
        assert seen == {"ks_head": 2, "ks_mid": 2, "ks_tail": 2} or os.environ.get("HIPBFV_NO_FUSED_GALOIS") == "1", seen  # no sum kernel
        assert seen.get("ks_tail") == 2, seen
        for k in range(2):
            _same(got[k], np.stack([ref[i % LD.DISTINCT][k] for i in range(batch)]), (pid, batch, "graph", k))
            for name, other in others.items():
                assert (other[k] == got[k]).all(), (pid, batch, k, name)
        ev.check()
    bad = 1
    zt = _take(z_rot, 4).copy()
    zt[bad] = LD.rotsum_transparent_addend(L, bad)
    with pytest.raises(HipBfvError, match=f"transparent \\(input set {bad} "):
        p.run(ev, [to_device(x), to_device(zt), to_device(z_swap)], None, gkd)
    with pytest.raises(RuntimeError, match="transparent"):
        run_program(LD.MemoOracle(L.o), p.nodes, p.edges, [x[bad], zt[bad], z_swap[bad]], L.rk, gk)
    ev.check()
    p.run(ev, [to_device(a) for a in inputs], None, gkd)  # input set 3: all zero but the last word -- clean
    ev.check()


# ---- C: element-wise, plaintext and n-ary kernels ---------------------------------------------------------------------------
C_SETS = ["U1024", "P1", "W2048"]


@pytest.mark.parametrize("pid", C_SETS)
def test_add_sub_and_negate_land_on_the_edges(pid, monkeypatch):
    """C1 / C2: eltwise_kernel.  add and sub landed on the pattern for sizes 2 and 3, out of place and in place; negate of
    ciphertexts holding 0, 1 and q - 1."""
    from sunscreen_amd.batch import to_device, to_host

    L = landing(pid)
    o = L.o
    ctx, ev = _device(L, monkeypatch)
    for size in (2, 3):
        x, ya, ys, T = LD.addsub_case(L, size)
        ref_add = np.stack([o.add(x[i], ya[i]) for i in range(len(x))])
        ref_sub = np.stack([o.sub(x[i], ys[i]) for i in range(len(x))])
        assert (ref_add == T).all() and (ref_sub == T).all()
        for fn, y, ref in ((ev.add, ya, ref_add), (ev.sub, ys, ref_sub)):
            dx, dy = to_device(x), to_device(y)
            out, seen = _profiled(ev, lambda: fn(dx, dy))
            assert seen == {"eltwise": 1}, seen
            _same(to_host(out), ref, (pid, size, fn.__name__))
            fn(dx, dy, out=dx)  # in place over the first operand
            _same(to_host(dx), ref, (pid, size, fn.__name__, "in place"))
            dx = to_device(x)
            fn(dx, dy, out=dy)  # ... and over the second
            _same(to_host(dy), ref, (pid, size, fn.__name__, "in place, second operand"))
            ev.check()
    neg = LD.negate_case(L)
    d = to_device(neg)
    out, seen = _profiled(ev, lambda: ev.negate(d))
    assert seen == {"eltwise": 1}, seen
    ref = np.stack([o.negate(c) for c in neg])
    _same(to_host(out), ref, (pid, "negate"))
    ev.negate(d, out=d)
    _same(to_host(d), ref, (pid, "negate in place"))
    ev.check()


@pytest.mark.parametrize("pid", C_SETS)
def test_add_plain_and_sub_plain_land_polynomial_0_on_the_edges(pid, monkeypatch):
    """C3: plain_addsub_kernel (launched outside the profiler's table: the call launches nothing the table knows).  c0 landed on the
    pattern; a plaintext per item and one shared by the batch; plaintext values 0, 1, t - 1, floor((t - 1) / 2), ceil(t / 2)."""
    from sunscreen_amd.batch import to_device, to_host

    L = landing(pid)
    o = L.o
    ctx, ev = _device(L, monkeypatch)
    for sub in (False, True):
        for shared in (False, True):
            ct, plain, T0 = LD.plain_case(L, sub, shared)
            ref = np.stack([(o.sub_plain if sub else o.add_plain)(ct[i], plain if shared else plain[i]) for i in range(len(ct))])
            assert (ref[:, 0] == T0).all()
            d, dp = to_device(ct), to_device(plain)
            fn = ev.sub_plain if sub else ev.add_plain
            out, seen = _profiled(ev, lambda: fn(d, dp))
            assert seen == {}, seen
            _same(to_host(out), ref, (pid, sub, shared))
            fn(d, dp, out=d)
            _same(to_host(d), ref, (pid, sub, shared, "in place"))
            ev.check()


@pytest.mark.parametrize("pid", C_SETS)
def test_multiply_plain_by_monomials_at_the_wrap(pid, monkeypatch):
    """C4: c x^e for e in {0, 1, n - 1} and c in {1, t - 1, floor((t - 1) / 2), ceil(t / 2)}, shared by the batch and one per item,
    on ciphertexts with 0 and q - 1 on both sides of the wrap.  The batched call multiplies inside its fused transform kernel
    (`plain`); the handle-level call takes mono_mul_kernel (launched outside the profiler's table), out of place and in place."""
    from sunscreen_amd import BFVEvaluator, Ciphertext, Plaintext
    from sunscreen_amd.batch import to_device, to_host

    L = landing(pid)
    o = L.o
    ctx, ev = _device(L, monkeypatch)
    ct = LD.mono_case(L)
    d = to_device(ct)
    monos = LD.monomials(L)
    for k, plain in enumerate(monos):
        out, seen = _profiled(ev, lambda: ev.multiply_plain(d, to_device(plain)))
        assert seen.get("plain") == 1, seen
        _same(to_host(out), np.stack([o.multiply_plain(c, plain) for c in ct]), (pid, "shared monomial", k))
    for first in (0, 4, 8):  # one monomial per item
        plains = np.stack(monos[first: first + 4])
        out, seen = _profiled(ev, lambda: ev.multiply_plain(d, to_device(plains)))
        assert seen.get("plain") == 1, seen
        _same(to_host(out), np.stack([o.multiply_plain(ct[i], plains[i]) for i in range(4)]), (pid, "monomial per item", first))
    ev.check()
    hev = BFVEvaluator(ctx)
    for k, plain in enumerate(monos):
        e = int(np.flatnonzero(plain)[0])
        pt = Plaintext.from_coefficients([0] * e + [int(plain[e])])
        for i in (k % 4, 3):
            c = Ciphertext.from_array(ctx, ct[i])
            ref = o.multiply_plain(ct[i], plain)
            _same(hev.multiply_plain(c, pt).to_array()[None], ref[None], (pid, "handle-level monomial", k, i))
            hev.multiply_plain_inplace(c, pt)
            _same(c.to_array()[None], ref[None], (pid, "handle-level monomial in place", k, i))


@pytest.mark.parametrize("pid", C_SETS)
def test_nary_sum_with_a_negated_first_term_lands_on_the_edges(pid, monkeypatch):
    """C5: nary_sum_kernel.  One Add / Sub / Negate tree over five inputs, ((((-a) + b) - c) + d) + e, the last input crafted."""
    from sunscreen_amd.batch import to_device, to_host
    from sunscreen_amd.program import FheProgram

    L = landing(pid)
    ins, T = LD.nary_case(L)
    p = FheProgram()
    a, b, c, d, e = (p.append_input_ciphertext(i) for i in range(5))
    p.append_output_ciphertext(p.append_add(p.append_add(p.append_sub(p.append_add(p.append_negate(a), b), c), d), e))
    assert p.describe()[0] == "sum members=1 terms=5 direct_outputs=1", p.describe()
    ctx, ev = _device(L, monkeypatch)
    for k in SWITCHES:
        monkeypatch.delenv(k, raising=False)
    dev = [to_device(x) for x in ins]
    (out,), seen = _profiled(ev, lambda: p.run(ev, dev))
    assert seen == {"eltwise": 1}, seen
    ref = np.stack([run_program(L.o, p.nodes, p.edges, [x[i] for x in ins])[0] for i in range(len(T))])
    assert (ref == T).all()
    _same(to_host(out), ref, (pid, "n-ary sum"))
    ev.check()


# ---- D: PIR product accumulators --------------------------------------------------------------------------------------------
def _dot_reference(L, rows, cols, kind):
    return L.cached(("dot reference", rows, cols, kind), lambda: LD.dot_reference(L.o, *LD.dot_case(L, rows, cols, kind)[:2]))


@pytest.mark.parametrize("kind", ["max", "landed", "landed_zero_column"])
@pytest.mark.parametrize("pid", ["W2048", "W4096", "P1"])
def test_product_accumulators_at_their_limits(pid, kind, monkeypatch):
    """D1 ... D4: dot_plain_ntt on operands written directly in the transform domain (no ct_to_ntt / plain_to_ntt) against sums in
    Python integers followed by the oracle's inverse transform.  60-bit primes (17 and 33 products of (q - 1)^2 pass the point where
    the lazy 128-bit accumulator must reduce), 1 ... 33 columns around that point, 1 ... 5 rows around the four rows of a thread;
    every word q - 1; sums that are exactly 0, exactly q - 1, the pattern; zero columns."""
    from sunscreen_amd.batch import to_device, to_host

    L = landing(pid)
    ctx, ev = _device(L, monkeypatch)
    for rows, cols, k in LD.DOT_CASES:
        if k != kind:
            continue
        ctn, pntt, T = LD.dot_case(L, rows, cols, kind)
        ref = _dot_reference(L, rows, cols, kind)
        out, seen = _profiled(ev, lambda: ev.dot_plain_ntt(to_device(ctn), to_device(pntt)))
        assert seen.get("plain") == 1 and seen.get("ntt_inv") == 1 and len(seen) == 2, seen
        _same(to_host(out), ref, (pid, kind, rows, cols))


def test_product_table_form_on_edge_operands(monkeypatch):
    """D5: dot_plain_tab_kernel -- the sum of plaintext products of a program (pir_lookup_graph's rows, each an output) with
    TransformedPlaintext arguments, batch 3, 5 rows, 17 columns; ciphertexts with 0 / q - 1 / 1 cycles, plaintexts cycling
    0, 1, t - 1, floor((t - 1) / 2), ceil(t / 2), three monomials."""
    from sunscreen_amd.batch import to_device, to_host
    from sunscreen_amd.program import FheProgram, TransformedPlaintext

    L = landing("P1")
    batch, rows, cols = 3, 5, 17
    cq, db = LD.table_case(L, batch, rows, cols)
    p = FheProgram()
    cqn = [p.append_input_ciphertext(j) for j in range(cols)]
    for i in range(rows):
        col = None
        for j in range(cols):
            term = p.append_multiply_plaintext(cqn[j], p.append_input_plaintext(cols + i * cols + j))
            col = term if col is None else p.append_add(col, term)
        p.append_output_ciphertext(col)
    assert p.describe()[0] == f"plain_matrix members={rows} columns={cols} direct_outputs={rows}", p.describe()
    ctx, ev = _device(L, monkeypatch)
    for k in SWITCHES:
        monkeypatch.delenv(k, raising=False)
    dbn = ev.plain_to_ntt(to_device(db))
    args = [to_device(cq[j]) for j in range(cols)] + [TransformedPlaintext(dbn[i, j]) for i in range(rows) for j in range(cols)]
    outs, seen = _profiled(ev, lambda: p.run(ev, args))
    assert seen.get("plain") == 1 and seen.get("ntt_inv", 0) >= 1, seen
    for b in range(batch):
        ref = run_program(L.o, p.nodes, p.edges, [cq[j][b] for j in range(cols)] + [db[i, j] for i in range(rows) for j in range(cols)])
        for i in range(rows):
            _same(to_host(outs[i])[b: b + 1], ref[i][None], ("table form", b, i))
    ev.check()


# ---- E: decrypt -------------------------------------------------------------------------------------------------------------
T_CASES = [("P1", 2), ("P1", 500), ("P1", None), ("P1", (1 << 60) - 1), ("P4", None)]


@pytest.mark.parametrize("pid,t", T_CASES, ids=[f"{p}-t{t or 'batching'}" for p, t in T_CASES])
def test_decrypt_rounds_the_landed_phases_as_the_oracle_does(pid, t, monkeypatch):
    """E: decrypt and decrypt_checked on ciphertexts whose phase c0 + c1 s is 0, 1, Q - 1, floor(Q / 2), floor(Q / 2) + 1 and the
    three integers around ceil((2 k + 1) Q / (2 t)) for k in {0, 1, floor(t / 2), t - 1}, cycled over the coefficients.  Expected: the
    oracle's decrypt, which tests/test_landing_cpu.py shows to be the integer algorithm on these phases."""
    from sunscreen_amd import SecretKey
    from sunscreen_amd.batch import to_device, to_host

    L = landing(pid, t)
    ct, phases = L.phase_items(2 if pid == "P4" else 4)
    ref = np.stack([L.o.decrypt(c, L.sk) for c in ct])
    ctx, ev = _device(L, monkeypatch)
    skd = SecretKey.from_array(ctx, L.sk)
    d = to_device(ct)
    out, seen = _profiled(ev, lambda: ev.decrypt(d, skd))
    assert seen.get("ntt_fwd") == 1 and seen.get("ntt_inv") == 1, seen
    _same(to_host(out), ref, (pid, t, "decrypt"))
    (plain, budget), seen = _profiled(ev, lambda: ev.decrypt_checked(d, skd))
    assert seen.get("ntt_fwd") == 1 and seen.get("ntt_inv") == 1, seen
    _same(to_host(plain), ref, (pid, t, "decrypt_checked"))
