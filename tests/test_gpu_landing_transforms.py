"""The whole-polynomial transforms and what is fused around them, on operands crafted so that the kernels' OWN outputs land on 0,
q - 1, 1 and (q +- 1) / 2 in every thread (tests/transform_landing.py builds them and states the models;
tests/test_transform_landing_cpu.py shows without a device that they land, and which lazy representatives the integer policy then
holds in front of its last conditional subtractions).

A  the stand-alone transform (ntt_pair_kernel, ntt_fwd_kernel / ntt_inv_kernel; ntt_head / ntt_midfwd / ntt_midinv / ntt_tail at
   n = 32768) forward and inverse with the special prime's row included, and ct_to_ntt.
B  the plaintext product: ct_plain_kernel's two policy instantiations, and the unfused ntt -> dyadic_plain_kernel -> ntt route at
   n = 32768, landed at the output, behind the forward half and in front of the inverse half; the handle-level calls and the
   one-column dot_plain_ntt on the same operands.
C  the BatchEncoder: the inverse transform modulo t with its output COEFFICIENTS on the targets of t.
D  mod_switch_kernel: both sides of the + h wrap of the last-prime residue, the last prime above and below a lower one.

Every assertion is word-for-word equality with the CPU oracle (and with the independent Python transform where one applies) over
all words.  Routes are read from the evaluator's profiler; mod_switch_kernel and the encoder are launched outside its table."""
import ctypes as C
import os

import numpy as np
import pytest

from tests import client_landing as CL
from tests import landing as LD
from tests import transform_landing as TL
from tests.client_landing import client

pytestmark = pytest.mark.gpu

NTT_SETS = ["U1024", "W2048", "P1", "P2", "S4096", "P3", "P5", "X8192", "P4", "P6"]
PLAIN_SETS = ["U1024", "W2048", "P1", "P3", "P5", "X8192", "P4", "P6"]
# the arithmetic policy of the whole-polynomial transforms by prime and degree (the context's range plan: FP64 up to 49 bits at these
# degrees): U1024 and X8192 hold 50-bit integer rows and 30-bit FP64 rows in ONE launch; under HIPBFV_NO_F64=1 every row is integer
MIXED, F64, INT = {"f64", "int"}, {"f64"}, {"int"}
POLICIES = {"U1024": MIXED, "X8192": MIXED, "P1": F64, "P2": F64, "S4096": F64, "P3": F64, "P4": F64, "W2048": INT, "P5": INT, "P6": INT}
MS_SETS = ["U1024", "S4096", "P2", "P3", "W2048", "P1"]


@pytest.fixture(scope="module", autouse=True)
def _drop():
    yield
    CL.drop_clients()


def _device(L):
    from sunscreen_amd import Context
    from sunscreen_amd.batch import BatchEvaluator

    ctx = Context.from_raw(L.n, L.key_primes, L.t)
    assert ctx.K == L.K and ctx.KK == L.KK and ctx.key_primes == L.key_primes
    return ctx, BatchEvaluator(ctx)


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


def _same(got, want, what):
    got, want = np.asarray(got), np.asarray(want)
    assert got.shape == want.shape, (what, got.shape, want.shape)
    bad = np.argwhere(got != want)
    assert bad.size == 0, (what, "first difference at", bad[0].tolist(), int(got[tuple(bad[0])]), int(want[tuple(bad[0])]), len(bad))


def _policies(L, primes) -> set:
    """{"f64", "int"}: the arithmetic policies the context gives these primes at L's degree (host only)."""
    from sunscreen_amd import _lib

    if os.environ.get("HIPBFV_NO_F64") == "1":
        return {"int"}
    out = (C.c_uint32 * 6)()
    seen = set()
    for p in primes:
        assert _lib.load().hipbfv_debug_f64_plan(p, L.n.bit_length() - 1, out) == 0
        seen.add("f64" if out[0] else "int")
    return seen


def _plaintext(p):
    from sunscreen_amd import Plaintext

    return Plaintext.from_coefficients([int(v) for v in p])


# ---- A: stand-alone transforms ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("pid", NTT_SETS)
def test_stand_alone_transforms_land_on_the_edges(pid):
    """2 KK polynomials (all paired at n <= 4096), 3 KK + 1 (the pairs, then KK + 1 through the single-polynomial kernel) and 1.
    The pattern rows go through the paired kernel in the first batch and through the single-polynomial kernel in the second.
    Forward of the landed rows is the target; the inverse of that is the landed row again, word for word; and the mirror image."""
    from sunscreen_amd.batch import to_device, to_host

    L = client(pid)
    KK = L.KK
    assert _policies(L, L.key_primes) in (POLICIES[pid], {"int"})
    if pid == "W2048":
        assert min(L.key_primes).bit_length() == 60
    ctx, ev = _device(L)
    batches = [TL.landed_transform_rows(L, ["pattern", "max"]), TL.landed_transform_rows(L, ["unit", "max", "pattern"], extra=1)]
    batches.append(tuple(a[:1] for a in batches[0]))
    for T, xf, xi in batches:
        assert len(T) in (2 * KK, 3 * KK + 1, 1)
        # the independent transform agrees with the targets on some rows of every batch (all of them up to n = 4096)
        for r in range(0, len(T), 1 if L.n <= 4096 else 5 if L.n <= 8192 else 17):
            assert (TL.ntt_plain(L, r % KK, xf[r]) == T[r]).all() and (TL.ntt_plain(L, r % KK, xi[r], inverse=True) == T[r]).all()
        d = to_device(xf)
        _, seen = _profiled(ev, lambda: ev.ntt(d, KK))
        assert seen == {"ntt_fwd": 1}, seen
        _same(to_host(d), T, (pid, len(T), "forward"))
        _, seen = _profiled(ev, lambda: ev.ntt(d, KK, inverse=True))
        assert seen == {"ntt_inv": 1}, seen
        _same(to_host(d), xf, (pid, len(T), "forward then inverse"))
        d = to_device(xi)
        ev.ntt(d, KK, inverse=True)
        _same(to_host(d), T, (pid, len(T), "inverse"))
        ev.ntt(d, KK)
        _same(to_host(d), xi, (pid, len(T), "inverse then forward"))


@pytest.mark.parametrize("pid", ["U1024", "W2048", "P1", "P5", "P6"])
def test_ct_to_ntt_lands_on_the_edges(pid):
    from sunscreen_amd.batch import to_device, to_host

    L = client(pid)
    ctx, ev = _device(L)
    for size in (2,) if pid == "P6" else (2, 3):
        ct, T = TL.landed_ciphertexts_for_ct_to_ntt(L, size)
        out, seen = _profiled(ev, lambda: ev.ct_to_ntt(to_device(ct)))
        assert seen == {"ntt_fwd": 1}, seen
        _same(to_host(out), T, (pid, size, "ct_to_ntt"))


# ---- B: the plaintext product ---------------------------------------------------------------------------------------------------------
def _assert_route(L, seen, chunks):
    """n = 32768: the unfused route (no fused kernel in the profile, one inverse transform per chunk); below it the fused kernel
    alone (the forward transforms in the profile are the plaintexts')."""
    if L.n == 32768:
        assert "plain" not in seen and seen.get("ntt_inv") == chunks, seen
    else:
        assert seen.get("plain") == chunks and "ntt_inv" not in seen, seen


@pytest.mark.parametrize("pid", PLAIN_SETS)
def test_multiply_plain_lands_at_the_output_and_either_side_of_the_product(pid):
    """Items landed at the output, behind the forward half, and in front of the inverse half, each with a plaintext of its own
    (0, 1, t - 1, floor(t / 2), ceil(t / 2) among random coefficients), chunks of two: out of place, then with out = ct; one shared
    plaintext; size 3; then one landed item through the handle-level calls and through the one-column dot_plain_ntt."""
    from sunscreen_amd import BFVEvaluator, Ciphertext
    from sunscreen_amd.batch import to_device, to_host

    L = client(pid)
    assert _policies(L, L.primes) in (POLICIES[pid], {"int"})  # (U1024, X8192: both instantiations have rows, each skips the other's)
    ctx, ev = _device(L)
    ev.set_chunk_ops(2)
    items = 5 if L.n <= 8192 else 3
    cts, plains, want, names = TL.multiply_plain_case(L, 2, items)  # (asserts: no zero word in NTT(lift p); the oracle lands)
    d, dp = to_device(cts), to_device(plains)
    out, seen = _profiled(ev, lambda: ev.multiply_plain(d, dp))
    _assert_route(L, seen, (items + 1) // 2)
    _same(to_host(out), want, (pid, names, "one plaintext per item"))
    _same(to_host(d), cts, (pid, "the operand of an out-of-place call"))
    assert ev.multiply_plain(d, dp, out=d) is d
    _same(to_host(d), want, (pid, names, "out = ct"))
    ev.check()
    # one shared plaintext
    cts1, p1, want1, names1 = TL.shared_plain_case(L, 2)
    out, seen = _profiled(ev, lambda: ev.multiply_plain(to_device(cts1), to_device(p1)))
    _assert_route(L, seen, 2)
    _same(to_host(out), want1, (pid, names1, "shared plaintext"))
    # size 3
    if L.n <= 16384:
        cts3, plains3, want3, names3 = TL.multiply_plain_case(L, 3, 3)
        d3 = to_device(cts3)
        _same(to_host(ev.multiply_plain(d3, to_device(plains3))), want3, (pid, names3, "size 3"))
        ev.multiply_plain(d3, to_device(plains3[0]), out=d3)
        _same(to_host(d3)[0], want3[0], (pid, "size 3, shared, out = ct"))
    # the handle-level calls on the item landed at the output
    hev = BFVEvaluator(ctx)
    a = Ciphertext.from_array(ctx, cts[0])
    _same(hev.multiply_plain(a, _plaintext(plains[0])).to_array(), want[0], (pid, "handle multiply_plain"))
    _same(a.to_array(), cts[0], (pid, "the handle's operand"))
    hev.multiply_plain_inplace(a, _plaintext(plains[0]))
    _same(a.to_array(), want[0], (pid, "handle multiply_plain_inplace"))
    # one column of the transform-domain matrix product over ct_to_ntt and plain_to_ntt of the same operands
    for k in range(3):
        ctn = ev.ct_to_ntt(to_device(cts[k : k + 1]))
        pn = ev.plain_to_ntt(to_device(plains[k : k + 1]))
        _same(to_host(pn)[0], TL.plain_transform(L, plains[k]), (pid, k, "plain_to_ntt"))
        _same(to_host(ev.dot_plain_ntt(ctn, pn.reshape(1, 1, L.K, L.n)))[0], want[k], (pid, names[k], "dot_plain_ntt with one column"))
    ev.check()


# ---- C: encode ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("pid", ["P1", "U1024"])
def test_encode_lands_its_coefficients_on_the_targets_of_t(pid):
    from sunscreen_amd.batch import to_device, to_host

    L = client(pid)
    ctx, ev = _device(L)
    Tp = TL.encode_targets(L)
    vals = [TL.land_encode(L, row) for row in Tp]
    unsigned, signed = np.stack([v for v, _ in vals]), np.stack([s for _, s in vals])
    for row in Tp:
        assert (L.o.batch_encode(L.o.batch_decode(row)) == row).all()
    for tv in LD.targets(L.t):
        assert (Tp[0] == np.uint64(tv)).any()
    _same(to_host(ev.encode(to_device(unsigned))), Tp, (pid, "encode"))
    _same(to_host(ev.encode(to_device(signed.view(np.uint64)), signed=True)), Tp, (pid, "signed encode"))
    _same(to_host(ev.decode(to_device(Tp))), unsigned, (pid, "decode"))
    _same(to_host(ev.decode(to_device(Tp), signed=True)).view(np.int64), signed, (pid, "signed decode"))


# ---- D: mod-switch --------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("pid", MS_SETS)
def test_mod_switch_lands_both_sides_of_the_half_wrap(pid):
    """The last-prime rows cycle 0, 1, h - 1, h, h + 1, h + 2, q_last - 1 against every target of the lower rows; one item switches
    to q_j - 1 everywhere.  U1024 and S4096: the last data prime above the lower ones by twenty and ten bits (reduce64, and a
    64-bit subtraction that would wrap without it); P2 and P1: below; P3: both in one kernel; W2048: 60-bit primes."""
    from sunscreen_amd import BFVEvaluator, Ciphertext
    from sunscreen_amd.batch import to_device, to_host

    L = client(pid)
    want_rel = {"U1024": {"above"}, "S4096": {"above"}, "P2": {"below"}, "P1": {"below"}, "P3": {"above", "below"}, "W2048": {"above"}}[pid]
    assert TL.relations(L) == want_rel
    assert pid not in ("U1024", "S4096") or TL.no_reduce64_applies(L)
    ctx, ev = _device(L)
    hev = BFVEvaluator(ctx)
    for size in (2, 3):
        ct, T = TL.mod_switch_case(L, size)  # (asserts: the RNS steps and the CRT statement agree, every class occurs, all landed)
        ref = np.stack([L.o.mod_switch_to_next(c) for c in ct])
        assert (ref == T).all()
        out = ev.mod_switch(to_device(ct))
        _same(to_host(out), T, (pid, size, "mod_switch"))
        ev.check()
        for it in range(2):
            a = Ciphertext.from_array(ctx, ct[it])
            _same(hev.mod_switch_to_next(a).to_array(), T[it], (pid, size, it, "handle mod_switch_to_next"))
