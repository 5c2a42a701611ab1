"""Sums of rotations on sources crafted so that the values inside ks_tail_sum_kernel and ks_tail_sum_weighted_kernel land on their
edges (tests/landing.py section J; tests/test_landing_cpu.py shows that every builder lands all of its words in the oracle, which
events every vector meets in every residue row, and that a fold with `>` for `>=` differs on these sums and on no random ones).

The summing tails finish every term with its own mod-down, gather sigma(c0) from the term's source, weight the canonical residue
(mul_shoup) and fold it with add_mod -- in registers, or through the output rows with the first term on a descriptor without records
-- and honour `accumulate` when a group is cut into slices.  Fresh encryptions put a finished residue of 0 or q - 1, a weighted
residue of 0 or q - 1, a raw sum of exactly q or q - 1, or a polynomial 1 that sums to zero in front of them about once in 2^40 to
2^50 words; here every thread sees them: finished terms on the pattern ("terms"), every partial sum on the pattern ("partial"), raw
sums of q - 1, q, q - 1, q in every word ("ladder"), a polynomial 1 that ends on all zeros or all zeros but one word, and sources
whose c0 and c1 are 0, q - 1 and 1 under the sign flips of the gather.

Every assertion on values is word-for-word equality with section J's `expected` over all words of all groups, and holds under every
switch the suite runs with; the kernel names are asserted under the default arms only.  Each case runs through rotate_rows_sum or
rotate_rows_sum_weighted and through the Galois-element form of the same terms."""
import ctypes as C
import os
import subprocess
import sys
import tempfile

import numpy as np
import pytest

from tests import landing as LD
from tests.landing import landing
from tests.test_gpu_landing import DEFAULT_ARMS, _device, _profiled, _same

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
COR_E_INVALIDOPERATION = 0x80131509
FUSED = DEFAULT_ARMS and os.environ.get("HIPBFV_NO_FUSED_GALOIS") != "1"  # the launches of the summing sequence are asserted
BODY_MODES = ("terms", "partial", "ladder")


@pytest.fixture(scope="module", autouse=True)
def _drop():
    yield
    LD.drop_landings()


def _keys(L, ctx, run):
    from sunscreen_amd import GaloisKeys

    name, steps, weights, galois, pow2 = run
    return GaloisKeys.from_arrays(ctx, LD.rotation_sum_keys(L, steps, galois, pow2))


def _forms(L, ev, dev, gkd, run, groups):
    """[(form, call)]: the row form (where the terms are steps) and the Galois-element form of the same terms (where every term has
    a key of its own), plain when the run has no weights."""
    name, steps, weights, galois, pow2 = run
    elts = [LD._element(L.o, s, galois) for s in steps]
    forms = []
    if not galois:
        forms.append(("rows", (lambda: ev.rotate_rows_sum(dev, list(steps), gkd, groups=groups)) if weights is None else
                      (lambda: ev.rotate_rows_sum_weighted(dev, list(steps), list(weights), gkd, groups=groups))))
    if not pow2:
        forms.append(("elements", (lambda: ev.apply_galois_sum(dev, elts, gkd, groups=groups)) if weights is None else
                      (lambda: ev.apply_galois_sum_weighted(dev, elts, list(weights), gkd, groups=groups))))
    return forms


def _one_summing_sequence(seen, sequences=1):
    return (seen.get("ks_head") == sequences and seen.get("ks_mid") == sequences and seen.get("ks_tail_sum") == sequences
            and not {"ks_tail", "galois", "ks_mac", "eltwise"} & set(seen))


def _folded(seen):
    return "ks_tail_sum" not in seen and seen.get("eltwise")


def _run_case(L, ev, gkd, run, mode, groups, what, ran=_one_summing_sequence, check=True):
    """Every form of one case against section J's expected; the tensor of the first form."""
    import torch
    from sunscreen_amd.batch import to_device, to_host

    name, steps, weights, galois, pow2 = run
    src, want, events = LD.rotation_sum_case(L, steps, weights, mode, groups, galois, pow2)
    dev = to_device(src)
    keep = dev.clone()
    first = None
    for form, call in _forms(L, ev, dev, gkd, run, groups):
        out, seen = _profiled(ev, call)
        print(what, name, mode, form, seen)
        _same(to_host(out), want, (what, name, mode, form))
        if FUSED and ran is not None:
            assert ran(seen), (what, name, mode, form, seen)
        if check:
            ev.check()
        assert first is None or torch.equal(out, first), (what, name, mode, form)
        first = out if first is None else first
    assert torch.equal(dev, keep), "the sources changed"
    return first


# ---- every body of the split summing tail ------------------------------------------------------------------------------------
BODY_SETS = ["P1", "P2", "P3", "X8192", "P4", "P5", "S4096"]


@pytest.mark.parametrize("mode", BODY_MODES)
@pytest.mark.parametrize("pid", BODY_SETS)
def test_every_body_of_the_summing_tails(pid, mode, monkeypatch):
    """P1: n = 4096, K = 2.  P2: the special prime below a data prime (the other arm of the mod-down).  P3: packed FP64 rows, K = 4 --
    sums in registers when unweighted, through the output rows when weighted.  X8192: 8-byte FP64 rows, K = 4, registers in both.  P4:
    K = 8, through the output rows.  P5: the MIXED integer bodies.  S4096: int32 weights wrap the 30-bit primes, and one weight is a
    prime of the set.  Every vector of LD.rotation_sum_runs: plain, small weights, +-1 with the identity first (the landed first term
    meets the descriptor without records), (0, -1, INT32_MIN, INT32_MAX), Galois elements 2 n - 5 and 2 n - 1."""
    from tests.bfv_helpers import params

    L = landing(pid)
    if pid == "X8192":  # the primes of the set tests/test_gpu_rotate_sum_weighted.py runs as the 8-byte FP64 body
        assert max(L.primes) >= 1 << 48 and L.K == 4 and [int(p) for p in params("seal_fhe_unit")[1]] == L.key_primes
    if pid == "P2":
        assert L.key_primes[-1] < max(L.key_primes[:-1])
    ctx, ev = _device(L, monkeypatch)
    groups = 2 if L.n >= 16384 else 3
    for run in LD.rotation_sum_runs(L):
        if run[4]:
            continue  # (the chains have their own test)
        _run_case(L, ev, _keys(L, ctx, run), run, mode, groups, pid)


# ---- slices ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("pid", ["P1", "P3", "P4"])
def test_slices_accumulate_onto_a_partial_sum_that_sits_on_the_pattern(pid, monkeypatch):
    """set_chunk_ops(3) over 4 terms: every group in slices of 3 + 1 terms, the second launch accumulating onto a stored partial sum
    that is on the pattern (ladder: on q - 1 in every word, the raw sum exactly q); then one group per sequence.  Both give the
    tensor of the unchunked call, which is the reference."""
    import torch
    from sunscreen_amd.batch import BatchEvaluator, multiply_sum_plan

    L = landing(pid)
    ctx, ev = _device(L, monkeypatch)
    ev3, ev7 = BatchEvaluator(ctx), BatchEvaluator(ctx)
    ev3.set_chunk_ops(3)
    ev7.set_chunk_ops(7)
    groups = 2 if L.n >= 16384 else 3
    plan3, plan7 = multiply_sum_plan(groups, 4, 3), multiply_sum_plan(groups, 4, 7)
    assert plan3[:2] == [(0, 1, 0, 3, False), (0, 1, 3, 1, True)] and len(plan3) == 2 * groups and len(plan7) == groups, (plan3, plan7)
    for run in LD.rotation_sum_runs(L)[:2]:
        assert run[1] == LD.STEPS_TWO_IDENTITIES
        gkd = _keys(L, ctx, run)
        for mode in ("partial", "ladder"):
            whole = _run_case(L, ev, gkd, run, mode, groups, pid)
            # (the second slice of every group is the last identity term alone: a summing tail without a key switch in front)
            sliced = _run_case(L, ev3, gkd, run, mode, groups, (pid, "chunk 3"),
                               lambda seen: seen.get("ks_tail_sum") == len(plan3) and seen.get("ks_head") == groups and seen.get("ks_mid") == groups
                               and not {"ks_tail", "galois", "ks_mac", "eltwise"} & set(seen))
            per_group = _run_case(L, ev7, gkd, run, mode, groups, (pid, "chunk 7"), lambda seen: _one_summing_sequence(seen, len(plan7)))
            assert torch.equal(sliced, whole) and torch.equal(per_group, whole), (pid, run[0], mode)


# ---- eight groups ------------------------------------------------------------------------------------------------------------
def test_eight_groups_take_the_xcd_row_order(monkeypatch):
    """8 groups x 4 terms at P1: 2 * 8 (polynomial, group) rows in the summing tail's grid, a multiple of 8.  Every group has its own
    phase of the pattern, so a row that lands in another group's place shows."""
    L = landing("P1")
    ctx, ev = _device(L, monkeypatch)
    for run in LD.rotation_sum_runs(L)[:2]:
        _run_case(L, ev, _keys(L, ctx, run), run, "partial", 8, "8 groups")


# ---- off the fused path ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", BODY_MODES)
def test_the_folded_route_at_p3(mode, monkeypatch):
    """HIPBFV_NO_FUSED_GALOIS=1: the terms are rotated into a stage and folded by the element-wise kernels (scaled_accumulate when
    weighted) -- the same words, and the tensor of the fused route."""
    import torch

    L = landing("P3")
    ctx, ev = _device(L, monkeypatch)
    fused = {run[0]: _run_case(L, ev, _keys(L, ctx, run), run, mode, 3, "P3 fused") for run in LD.rotation_sum_runs(L)[:4]}
    ctx, ev = _device(L, monkeypatch, {"HIPBFV_NO_FUSED_GALOIS": "1"})
    for run in LD.rotation_sum_runs(L)[:4]:
        out = _run_case(L, ev, _keys(L, ctx, run), run, mode, 3, "P3 folded", _folded if DEFAULT_ARMS else None)
        assert torch.equal(out, fused[run[0]]), run[0]


@pytest.mark.parametrize("pid", ["U1024", "W2048"])
def test_below_the_split_kernels_the_terms_are_staged_and_folded(pid, monkeypatch):
    """n = 1024 (30-bit rows beside 50-bit ones, and a weight that is one of the 30-bit primes) and n = 2048 (60-bit primes): the
    whole-polynomial key switch and the element-wise fold."""
    L = landing(pid)
    ctx, ev = _device(L, monkeypatch)
    for run in LD.rotation_sum_runs(L):
        for mode in BODY_MODES:
            _run_case(L, ev, _keys(L, ctx, run), run, mode, 3, pid, lambda seen: "ks_head" not in seen and _folded(seen) and seen.get("ks_mac"))


def test_the_integer_key_switch_at_32768(monkeypatch):
    """P6, 2 groups x 3 terms with the identity first."""
    L = landing("P6")
    ctx, ev = _device(L, monkeypatch)
    run = LD.rotation_sum_runs(L)[2]
    assert len(run[1]) == 3
    gkd = _keys(L, ctx, run)
    for mode in ("partial", "ladder"):
        _run_case(L, ev, gkd, run, mode, 2, "P6", None)


# ---- chain terms -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", BODY_MODES)
def test_chain_terms_enter_as_identity_terms_with_landed_polynomial_0(mode, monkeypatch):
    """Under the power-of-two keys 11 and -13 walk their NAF chains: they are rotated beforehand and enter the summing tail as
    (weighted) identity terms, whose polynomial 0 -- landed through the whole chain (LD.land_rotation) -- the tail reads from the
    rotated copy; 1 has its key and 0 is the identity."""
    L = landing("P1")
    ctx, ev = _device(L, monkeypatch)
    runs = [r for r in LD.rotation_sum_runs(L) if r[4]]
    assert len(runs) == 2
    for run in runs:
        _run_case(L, ev, _keys(L, ctx, run), run, mode, 3, "chains",
                  lambda seen: seen.get("ks_tail_sum") == 1 and "eltwise" not in seen)


# ---- the gathers -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("pid", ["P3", "P4"])
def test_sources_of_0_and_q_minus_1_under_the_sign_flips_of_the_gathers(pid, monkeypatch):
    """c0 and c1 of the first rotated term cycle 0, q - 1, 1: zeros and q - 1 where galois_gather negates, in the base (c0, gathered
    by the tail) and in the head's reads of c1.  Compared, not landed."""
    L = landing(pid)
    ctx, ev = _device(L, monkeypatch)
    for run in LD.rotation_sum_runs(L)[:2]:
        _run_case(L, ev, _keys(L, ctx, run), run, "gathers", 2, pid)


# ---- transparency ------------------------------------------------------------------------------------------------------------
TRANSPARENT_RUNS = [("P3", 0, "registers"), ("X8192", 1, "registers, weighted"), ("P3", 1, "through the output rows"), ("P4", 0, "through the output rows")]


@pytest.mark.parametrize("pid,k,form", TRANSPARENT_RUNS, ids=[f"{p}-{f}" for p, k, f in TRANSPARENT_RUNS])
def test_a_landed_transparent_sum_is_reported_under_its_group_and_an_almost_transparent_one_is_not(pid, k, form, monkeypatch):
    """An identity term lands the final polynomial 1 of group 1 on all zeros: COR_E_INVALIDOPERATION with first item 1, as the
    cancelling weights of tests/test_gpu_rotate_sum_weighted.py are reported.  On all zeros but the last word of the last row: a
    clean run.  Where the sums are held in registers and where they go through the output rows."""
    from sunscreen_amd import _lib
    from sunscreen_amd.batch import _stream
    from tests.test_gpu_rotation_steps import _hr

    L = landing(pid)
    ctx, ev = _device(L, monkeypatch)
    run = LD.rotation_sum_runs(L)[k]
    gkd = _keys(L, ctx, run)
    groups = 3
    lib, first = _lib.load(), C.c_uint64()
    ev.check()
    _run_case(L, ev, gkd, run, "almost", groups, (pid, form))  # (checks after every form: clean)
    assert lib.hipbfv_batch_status(ev._h, C.byref(first), _stream()) == 0 and first.value == 2**64 - 1
    src, want, _ = LD.rotation_sum_case(L, run[1], run[2], "transparent", groups, run[3], run[4])
    assert not want[LD.TRANSPARENT_GROUP, 1].any() and all(want[g, 1].any() for g in range(groups) if g != LD.TRANSPARENT_GROUP)
    _run_case(L, ev, gkd, run, "transparent", groups, (pid, form), check=False)
    hr, msg = _hr(ev.check)
    assert hr == COR_E_INVALIDOPERATION and f"item {LD.TRANSPARENT_GROUP})" in msg, (hex(hr), msg)
    ev.check()
    _run_case(L, ev, gkd, run, "transparent", groups, (pid, form), check=False)
    assert lib.hipbfv_batch_status(ev._h, C.byref(first), _stream()) & 0xFFFFFFFF == COR_E_INVALIDOPERATION and first.value == LD.TRANSPARENT_GROUP


# ---- the lane-split geometry build -------------------------------------------------------------------------------------------
def test_the_lane_split_geometry_build_gives_the_same_words(monkeypatch):
    """One P4 case, weighted and on the partial sums, against libhipbfv_geom8.so in a process of its own (a time limit on the child)."""
    lib = os.path.join(ROOT, "sunscreen_amd", "lib", "variants", "libhipbfv_geom8.so")
    assert os.path.exists(lib), "build the variant library first: make -C sunscreen_amd/csrc variants (build() does)"
    L = landing("P4")
    name, steps, weights, galois, pow2 = LD.rotation_sum_runs(L)[1]
    gk = LD.rotation_sum_keys(L, steps, galois, pow2)
    src, want, _ = LD.rotation_sum_case(L, steps, weights, "partial", 2, galois, pow2)
    script = r"""
import sys, numpy as np, torch
sys.path.insert(0, %r)
from sunscreen_amd import Context, GaloisKeys
from sunscreen_amd.batch import BatchEvaluator, to_device, to_host
z = np.load(sys.argv[1])
ctx = Context.from_raw(int(z["n"]), [int(p) for p in z["primes"]], int(z["t"]))
ev = BatchEvaluator(ctx)
ev.profile(True)
gk = GaloisKeys.from_arrays(ctx, {int(e): k for e, k in zip(z["elts"], z["keys"])})
out = ev.rotate_rows_sum_weighted(to_device(z["src"]), [int(s) for s in z["steps"]], [int(x) for x in z["w"]], gk, groups=2)
torch.cuda.synchronize()
seen = ev.profile_read()
if %r:
    assert seen["ks_tail_sum"]["launches"] == 1 and "ks_tail" not in seen and "eltwise" not in seen, seen
ev.check()
np.savez(sys.argv[2], out=to_host(out))
""" % (ROOT, FUSED)
    with tempfile.TemporaryDirectory() as td:
        a, b = os.path.join(td, "in.npz"), os.path.join(td, "out.npz")
        elts = sorted(gk)
        np.savez(a, n=L.n, primes=np.array(L.key_primes, dtype=np.uint64), t=L.t, src=src, elts=np.array(elts, dtype=np.uint64),
                 keys=np.stack([gk[e] for e in elts]), steps=np.array(steps, dtype=np.int64), w=np.array(weights, dtype=np.int64))
        subprocess.run([sys.executable, "-c", script, a, b], env=dict(os.environ, HIPBFV_LIB=lib, HIPBFV_NO_SMALL_BATCH="1"), check=True, timeout=120)
        got = np.load(b)["out"]
    _same(got, want, "geom8")
