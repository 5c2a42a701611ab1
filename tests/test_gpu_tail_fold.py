"""The FP64 tails with their fixed scaling folded into the last two inverse stages (moddown_d.hpp tail_fold4_d) and the floor's single
product by q^-1 (B/B_j)^-1, bit for bit against the CPU oracle.

Every call whose last kernel is one of those tails, on 2-3 items (genuine encryptions plus one item of uniform random residues):
multiply_relin (mul_head / mul_mid / mulrelin_head / ks_mid / mulrelin_tail), multiply (mul_tail), relinearize and one rotation
(ks_head / ks_mid / ks_tail: the crafted operands of tests/landing.py, whose outputs land on 0, q - 1, 1 and the integers around
q / 2, i.e. on every side of the tail's canonicalisation), and multiply_sum_relin with 2 groups x 3 terms (mul_tail_sum).  Each
once more under HIPBFV_NO_FUSED_TAIL=1, which takes the product through the stand-alone mul_tail, ks_head and ks_tail.

Parameter sets (tests/landing.py SETS): P1 n = 4096 (K = 2 + 1), P3 n = 8192 (K = 4 + 1), P4 n = 16384 (K = 8 + 1: the GRID tail
and per-row packing), P5 54,54,54,56 bits (mixed: FP64 auxiliary rows beside integer data rows).  The lane-split geometry, which
keeps the unfolded stages but takes the new constants, runs the P4 cases against the geom-8 variant library in a process of its own
(the library is chosen when it is loaded)."""
import os
import subprocess
import sys

import numpy as np
import pytest

from tests import landing as LD
from tests.landing import landing

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PIDS = ["P1", "P3", "P4", "P5"]
ARMS = [{}, {"HIPBFV_NO_FUSED_TAIL": "1"}]
ARM_IDS = ["fused", "no_fused_tail"]
ROT_STEP = 1


@pytest.fixture(scope="module", autouse=True)
def _drop():
    yield
    LD.drop_landings()


def _device(L, monkeypatch, env):
    """A fresh context and evaluator (the switches are read when they are made); a few items go through the split kernels."""
    from sunscreen_amd import Context
    from sunscreen_amd.batch import BatchEvaluator

    for k, v in env.items():
        monkeypatch.setenv(k, v)
    monkeypatch.setenv("HIPBFV_NO_SMALL_BATCH", "1")
    ctx = Context.from_raw(L.n, L.key_primes, L.t)
    assert ctx.K == L.K and ctx.key_primes == L.key_primes
    return ctx, BatchEvaluator(ctx)


def _same(got, want, what):
    assert got.shape == want.shape, (what, got.shape, want.shape)
    for i in range(len(want)):
        bad = np.argwhere(got[i] != want[i])
        assert bad.size == 0, (what, "item", i, "first difference at", bad[0].tolist(), int(got[i][tuple(bad[0])]), int(want[i][tuple(bad[0])]), len(bad))


def _operands(L):
    """a, b: uint64[3][2][K][n] -- two genuine encryptions each and one item of uniform random residues; and the oracle's size-3
    products and their relinearizations.  Built once per parameter set."""

    def make():
        rng = L.rng(41)
        a = np.concatenate([L.fresh(rng, 2), LD.random_residues(rng, L.primes, (1, 2), L.n)])
        b = np.concatenate([L.fresh(rng, 2), LD.random_residues(rng, L.primes, (1, 2), L.n)])
        ref3 = np.stack([L.o.multiply(a[i], b[i]) for i in range(3)])
        ref2 = np.stack([L.o.relinearize(ref3[i], L.rk) for i in range(3)])
        return a, b, ref3, ref2

    return L.cached("tail fold operands", make)


@pytest.mark.parametrize("env", ARMS, ids=ARM_IDS)
@pytest.mark.parametrize("pid", PIDS)
def test_multiply_relin_and_multiply(pid, env, monkeypatch):
    """The fused multiply + relinearize and the plain multiply of the same three pairs; the genuine products decrypt."""
    from sunscreen_amd import RelinearizationKeys
    from sunscreen_amd.batch import to_device, to_host

    L = landing(pid)
    a, b, ref3, ref2 = _operands(L)
    ctx, ev = _device(L, monkeypatch, env)
    rkd = RelinearizationKeys.from_array(ctx, L.rk)
    da, db = to_device(a), to_device(b)
    _same(to_host(ev.multiply_relin(da, db, rkd)), ref2, (pid, env, "multiply_relin"))
    _same(to_host(ev.multiply(da, db)), ref3, (pid, env, "multiply"))
    ev.check()


@pytest.mark.parametrize("env", ARMS, ids=ARM_IDS)
@pytest.mark.parametrize("pid", PIDS)
def test_relinearize(pid, env, monkeypatch):
    """The size-3 products above, then the crafted inputs whose relinearization lands both output polynomials on the edge pattern,
    polynomial 0 on all 0 and on all q - 1 (three items: tests/landing.py relin_items)."""
    from sunscreen_amd import RelinearizationKeys
    from sunscreen_amd.batch import to_device, to_host

    L = landing(pid)
    a, b, ref3, ref2 = _operands(L)
    (ct3, want, names), _ = L.relin_items()
    ct3, want = ct3[:3], want[:3]
    ref = L.cached("tail fold relin reference", lambda: np.stack([L.o.relinearize(c, L.rk) for c in ct3]))
    assert (ref == want).all()  # the builder landed its targets in the oracle
    ctx, ev = _device(L, monkeypatch, env)
    rkd = RelinearizationKeys.from_array(ctx, L.rk)
    _same(to_host(ev.relinearize(to_device(ref3), rkd)), ref2, (pid, env, "relinearize of the products"))
    _same(to_host(ev.relinearize(to_device(ct3), rkd)), ref, (pid, env, "relinearize onto the edges", names[:3]))
    ev.check()


@pytest.mark.parametrize("env", ARMS, ids=ARM_IDS)
@pytest.mark.parametrize("pid", PIDS)
def test_rotation(pid, env, monkeypatch):
    """rotate_rows by one step: polynomial 0 landed on the pattern, on all 0 and on all q - 1 (tests/landing.py rotation_items)."""
    from sunscreen_amd import GaloisKeys
    from sunscreen_amd.batch import to_device, to_host

    L = landing(pid)
    elt = L.o.galois_elt_from_step(ROT_STEP)
    gk = L.galois_keys([elt])
    ct, want, names = L.rotation_items(elt)
    ct, want = ct[:3], want[:3]
    ref = L.cached("tail fold rotation reference", lambda: np.stack([L.o.apply_galois(c, elt, gk) for c in ct]))
    assert (ref == want).all()
    ctx, ev = _device(L, monkeypatch, env)
    gkd = GaloisKeys.from_arrays(ctx, gk)
    _same(to_host(ev.rotate_rows(to_device(ct), ROT_STEP, gkd)), ref, (pid, env, "rotate_rows", names[:3]))
    ev.check()


@pytest.mark.parametrize("env", ARMS, ids=ARM_IDS)
@pytest.mark.parametrize("pid", PIDS)
def test_multiply_sum_relin(pid, env, monkeypatch):
    """2 groups x 3 terms: group 0 of genuine encryptions, group 1 with one term of uniform random residues."""
    from sunscreen_amd import RelinearizationKeys
    from sunscreen_amd.batch import to_device, to_host

    L = landing(pid)

    def make():
        rng = L.rng(43)
        a = np.stack([L.fresh(rng, 3), np.concatenate([L.fresh(rng, 2), LD.random_residues(rng, L.primes, (1, 2), L.n)])])
        b = np.stack([L.fresh(rng, 3), np.concatenate([L.fresh(rng, 2), LD.random_residues(rng, L.primes, (1, 2), L.n)])])
        ref = []
        for g in range(2):
            acc = L.o.multiply(a[g, 0], b[g, 0])
            for j in range(1, 3):
                acc = L.o.add(acc, L.o.multiply(a[g, j], b[g, j]))
            ref.append(L.o.relinearize(acc, L.rk))
        return a, b, np.stack(ref)

    a, b, ref = L.cached("tail fold sums", make)
    ctx, ev = _device(L, monkeypatch, env)
    rkd = RelinearizationKeys.from_array(ctx, L.rk)
    _same(to_host(ev.multiply_sum_relin(to_device(a), to_device(b), rkd)), ref, (pid, env, "multiply_sum_relin"))
    ev.check()


def test_lane_split_library_at_n16384():
    """The n = 16384 cases above against the lane-split geometry (sunscreen_amd/lib/variants/libhipbfv_geom8.so), in a process of
    its own: the library is chosen through HIPBFV_LIB when it is loaded."""
    lib = os.path.join(ROOT, "sunscreen_amd", "lib", "variants", "libhipbfv_geom8.so")
    assert os.path.exists(lib), "build() makes the variant library"
    env = dict(os.environ, HIPBFV_LIB=lib)
    out = subprocess.run([sys.executable, "-m", "pytest", "-q", "-x", "-p", "no:cacheprovider", os.path.abspath(__file__), "-k", "P4 and not lane_split"],
                         cwd=ROOT, env=env, capture_output=True, text=True)
    tail = out.stdout.strip().splitlines()[-1] if out.stdout.strip() else ""
    assert out.returncode == 0 and "8 passed" in tail, out.stdout[-3000:] + out.stderr[-2000:]
