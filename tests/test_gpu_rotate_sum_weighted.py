"""Weighted sums of rotations: hipbfv_batch_rotate_rows_sum_weighted / hipbfv_batch_apply_galois_sum_weighted give out[g] = sum_t
w_t (.) rotate(source of item g * terms + t, steps[t]) with the weight applied to every finished term inside the key switch's last
kernel (ks_tail_sum_weighted_kernel; profiler kind ks_tail_sum), just before the term is added.

The reference is the CPU oracle's o.rotate_rows / o.apply_galois per term, every residue row i scaled in Python integers by
(w mod q_i) and the scaled terms folded with o.add.  For 0 < |w| <= 3 the scaling is also asserted equal to the oracle's repeated
o.add (after o.negate when w < 0), which pins the definition to the oracle.  Decoded slots are compared with sum_t w_t * rolled rows
mod t only for small-weight sets (sum |w| <= 8), where the reference keeps noise budget; the extreme weights are judged by words alone.

Noise budget of the reference sums, measured on the CPU with the oracle (bits, the smallest over the groups of each case):
  n = 4096, K = 2 (the world of tests/test_gpu_rotation_steps.py):
    direct steps [1, -13, 0, 2045], weights [2, -1, 3, -2]: 46;  chain steps [11, 1707, 1, 2045], weights [3, -2, 2, -1]: 44
    Galois form, weights [2, -1, 3, -2]: 45;  8 groups x 2 terms, weights [3, -2]: 45;  taps (1, -2, 1): 46;  one term, weight -1: 47
  one small case per body, steps [1, -2, 0], weights [-2, 1, 3]:
    default_8192 (packed FP64, K = 4): 145;  seal_fhe_unit (8-byte FP64, K = 4): 115;  3 x 54 + 56 bits at n = 8192 (MIXED): 134;
    default_16384 (K = 8): 359;  n = 1024 with [50, 30, 30, 50, 50] bits: 129
"""
import ctypes as C
import os
import subprocess
import sys
import tempfile

import numpy as np
import pytest

from oracle import bfv_oracle as O
from tests.bfv_helpers import params
from tests.test_gpu_rotation_steps import COUNT, E_INVALIDARG, H, SENTINEL, _hr, _rolled, _slots, _World

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
E_POINTER = 0x80004003
COR_E_INVALIDOPERATION = 0x80131509
INT32_MIN, INT32_MAX = -(2**31), 2**31 - 1
GROUPS, TERMS = 5, 4
DIRECT_STEPS = [1, -13, 0, 2045]  # under D: three keys of their own and the identity
DIRECT_WEIGHTS = [2, -1, 3, -2]  # four distinct weights, the identity term carries 3; sum |w| = 8
CHAIN_STEPS = [11, 1707, 1, 2045]  # under P: three NAF chains and one direct key
CHAIN_WEIGHTS = [3, -2, 2, -1]
EXTREME_WEIGHTS = [0, -1, INT32_MIN, INT32_MAX]
BODY_STEPS, BODY_WEIGHTS = [1, -2, 0], [-2, 1, 3]  # the first term's weight is not 1, the identity term carries 3
assert GROUPS * TERMS == COUNT

_WORLD = []


@pytest.fixture(scope="module", autouse=True)
def _shared_world():
    yield
    while _WORLD:
        _WORLD.pop().close()


def _world() -> _World:
    if not _WORLD:
        _WORLD.append(_World())
    return _WORLD[0]


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


# ---- the reference -----------------------------------------------------------------------------------------------------------
def _source(groups, terms, src_index):
    return [i if src_index is None else src_index[i % len(src_index)] for i in range(groups * terms)]


def _scaled(o, ct, w):
    """Every word of residue row i times (w mod q_i) mod q_i, in Python integers; for 0 < |w| <= 3 also the oracle's |w| adds of the
    ciphertext, negated first when w < 0."""
    out = np.empty_like(ct)
    for i, q in enumerate(o.primes):
        out[:, i] = ((ct[:, i].astype(object) * (w % q)) % q).astype(np.uint64)
    if 0 < abs(w) <= 3:
        one = o.negate(ct) if w < 0 else ct
        acc = one
        for _ in range(abs(w) - 1):
            acc = o.add(acc, one)
        assert (np.asarray(acc) == out).all(), w
    return out


def _oracle_sums(o, cts, gk, steps, weights, groups, src_index, galois=False, cache=None):
    """out[g] = the oracle's rotations of the group's terms (every (source, step) rotated once), scaled, folded with o.add."""
    cache = {} if cache is None else cache
    src = _source(groups, len(steps), src_index)
    out = []
    for g in range(groups):
        acc = None
        for t, step in enumerate(steps):
            s = src[g * len(steps) + t]
            if (s, step) not in cache:
                if galois:
                    cache[(s, step)] = cts[s] if step == 1 else o.apply_galois(cts[s], step, gk)
                else:
                    cache[(s, step)] = o.rotate_rows(cts[s], step, gk) if step else cts[s]
            if (s, step, weights[t]) not in cache:
                cache[(s, step, weights[t])] = _scaled(o, cache[(s, step)], weights[t])
            term = cache[(s, step, weights[t])]
            acc = term if acc is None else o.add(acc, term)
        out.append(acc)
    return np.stack(out)


def _check_words(got, ref, what):
    for g in range(ref.shape[0]):
        assert (got[g] == ref[g]).all(), (what, g)


def _check_sums(o, sk, got, ref, vals, row_steps, weights, groups, src_index, what):
    """Word for word against the reference; the decoded slots against sum_t w_t * the rolled rows mod t (small weights only: the
    reference must keep noise budget).  row_steps: the row rotation of every term (None: that term swaps the rows)."""
    assert sum(abs(w) for w in weights) <= 8, weights
    src = _source(groups, len(row_steps), src_index)
    _check_words(got, ref, what)
    for g in range(groups):
        budget = o.noise_budget(ref[g], sk)
        print(f"noise budget [{what}] group {g}: {budget} bits")
        assert budget > 0, (what, g)
        want = np.zeros(vals[0].size, dtype=np.int64)
        for k, step in enumerate(row_steps):
            v = vals[src[g * len(row_steps) + k]]
            v = np.concatenate([v[v.size // 2:], v[: v.size // 2]]) if step is None else _rolled(v, step)
            want = (want + weights[k] * v.astype(np.int64)) % o.t
        assert (o.batch_decode(o.decrypt(got[g], sk)).astype(np.int64) == want).all(), (what, g)


_CASE1 = {}


def _case1(w):
    """The bits of case 1 at the default chunk (computed once): every other route to the same sums is compared with them."""
    import torch

    if "out" not in _CASE1:
        ev = w.ev("split")
        da = w.dev.clone()
        out, seen = _profiled(ev, lambda: ev.rotate_rows_sum_weighted(da, DIRECT_STEPS, DIRECT_WEIGHTS, w.gkd["D"]))
        assert torch.equal(da, w.dev), "the input changed"
        ev.check()
        _CASE1["out"], _CASE1["seen"] = out, seen
        _CASE1["cache"] = {}
        _CASE1["ref"] = _oracle_sums(w.o, w.cts, w.gk["D"], DIRECT_STEPS, DIRECT_WEIGHTS, GROUPS, None, cache=_CASE1["cache"])
    return _CASE1


# ---- 1: direct and identity terms --------------------------------------------------------------------------------------------
def test_direct_and_identity_terms_run_one_summing_sequence():
    """5 groups x 4 terms of distinct ciphertexts, three direct keys and the identity with weight 3: ONE ks_head, ks_mid and ks_tail_sum;
    no tail of single items, no rotated copy, no whole-polynomial key switch and no element-wise pass."""
    from sunscreen_amd.batch import to_host

    w = _world()
    c = _case1(w)
    seen = c["seen"]
    assert seen.get("ks_head") == 1 and seen.get("ks_mid") == 1 and seen.get("ks_tail_sum") == 1, seen
    assert not {"ks_tail", "galois", "ks_mac", "eltwise"} & set(seen), seen
    _check_sums(w.o, w.sk, to_host(c["out"]), c["ref"], w.vals, DIRECT_STEPS, DIRECT_WEIGHTS, GROUPS, None, "default chunk")


# ---- 2: chunks and slices ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("chunk,sequences", [(7, 5), (3, 10)])
def test_chunks_and_slices_give_the_same_bits(chunk, sequences):
    """chunk 7: one group per sequence.  chunk 3: every group in two slices, 3 + 1 terms, the second accumulating and reading the
    table from row 3 -- the four weights differ, so another row shows."""
    import torch
    from sunscreen_amd.batch import BatchEvaluator, multiply_sum_plan

    w = _world()
    plan = multiply_sum_plan(GROUPS, TERMS, chunk)
    assert len(plan) == sequences
    if chunk == 3:
        assert plan[:2] == [(0, 1, 0, 3, False), (0, 1, 3, 1, True)], plan[:2]
    assert len(set(DIRECT_WEIGHTS)) == TERMS
    ev = BatchEvaluator(w.ctx)
    ev.set_chunk_ops(chunk)
    out, seen = _profiled(ev, lambda: ev.rotate_rows_sum_weighted(w.dev, DIRECT_STEPS, DIRECT_WEIGHTS, w.gkd["D"]))
    assert seen.get("ks_tail_sum") == sequences and seen.get("ks_head") == sequences and seen.get("ks_mid") == sequences, seen
    assert not {"ks_tail", "galois", "ks_mac", "eltwise"} & set(seen), seen
    assert torch.equal(out, _case1(w)["out"]), chunk
    ev.check()


# ---- 3: all ones -------------------------------------------------------------------------------------------------------------
def test_all_ones_run_the_unweighted_launches():
    import torch

    w = _world()
    ev = w.ev("split")
    for steps, holding in ((DIRECT_STEPS, "D"), (CHAIN_STEPS, "P")):
        plain, seen_plain = _profiled(ev, lambda: ev.rotate_rows_sum(w.dev, steps, w.gkd[holding]))
        ones, seen_ones = _profiled(ev, lambda: ev.rotate_rows_sum_weighted(w.dev, steps, [1] * TERMS, w.gkd[holding]))
        assert torch.equal(ones, plain), holding
        assert seen_ones == seen_plain, (seen_ones, seen_plain)
    ev.check()


# ---- 4: extreme weights ------------------------------------------------------------------------------------------------------
def test_extreme_weights_give_the_words_of_the_python_integer_reference():
    """(0, -1, INT32_MIN, INT32_MAX): a zero weight is a term like any other (its key switch runs), both extremes exceed no prime but
    wrap the int32 negation.  Words only: the sum has no noise budget left."""
    from sunscreen_amd.batch import to_host

    w = _world()
    ev = w.ev("split")
    out, seen = _profiled(ev, lambda: ev.rotate_rows_sum_weighted(w.dev, DIRECT_STEPS, EXTREME_WEIGHTS, w.gkd["D"]))
    assert seen.get("ks_head") == 1 and seen.get("ks_mid") == 1 and seen.get("ks_tail_sum") == 1 and "eltwise" not in seen, seen
    ref = _oracle_sums(w.o, w.cts, w.gk["D"], DIRECT_STEPS, EXTREME_WEIGHTS, GROUPS, None, cache=_case1(w)["cache"])
    _check_words(to_host(out), ref, "extreme")
    ev.check()


# ---- 5: chain terms ----------------------------------------------------------------------------------------------------------
def test_chain_terms_are_rotated_beforehand_and_enter_as_weighted_identity_terms():
    """Holding P: 11, 1707 and 2045 walk their NAF chains, 1 has its key."""
    import torch
    from sunscreen_amd.batch import to_host

    w = _world()
    ref = _oracle_sums(w.o, w.cts, w.gk["P"], CHAIN_STEPS, CHAIN_WEIGHTS, GROUPS, None)
    outs = {}
    for kind in ("split", "chunk7"):
        ev = w.ev(kind)
        out, seen = _profiled(ev, lambda: ev.rotate_rows_sum_weighted(w.dev, CHAIN_STEPS, CHAIN_WEIGHTS, w.gkd["P"]))
        assert seen.get("ks_tail_sum") == (1 if kind == "split" else GROUPS) and "eltwise" not in seen, seen
        outs[kind] = out
        ev.check()
    assert torch.equal(outs["split"], outs["chunk7"])
    _check_sums(w.o, w.sk, to_host(outs["split"]), ref, w.vals, CHAIN_STEPS, CHAIN_WEIGHTS, GROUPS, None, "chains")


def test_a_chain_term_listed_twice_is_rotated_once():
    """(source g, step 11) twice with weights 2 and -3 under P: the launches of the one-term call with weight -1, and its bits."""
    import torch

    w = _world()
    ev = w.ev("split")
    twice, seen_twice = _profiled(ev, lambda: ev.rotate_rows_sum_weighted(w.dev[:GROUPS], [11, 11], [2, -3], w.gkd["P"], src_index=[i // 2 for i in range(2 * GROUPS)]))
    once, seen_once = _profiled(ev, lambda: ev.rotate_rows_sum_weighted(w.dev[:GROUPS], [11], [-1], w.gkd["P"]))
    assert torch.equal(twice, once)
    assert seen_twice == seen_once, (seen_twice, seen_once)
    ev.check()


# ---- 6: src_index ------------------------------------------------------------------------------------------------------------
def test_source_indexing():
    """One ciphertext per group by four steps; one set of four ciphertexts shared by all groups; the same (source, step) twice."""
    import torch
    from sunscreen_amd.batch import to_host

    w = _world()
    o, ev, gk = w.o, w.ev("split"), w.gk["D"]
    cache = _case1(w)["cache"]
    idx = [i // TERMS for i in range(COUNT)]
    got = to_host(ev.rotate_rows_sum_weighted(w.dev[:GROUPS], DIRECT_STEPS, DIRECT_WEIGHTS, w.gkd["D"], src_index=idx))
    ref = _oracle_sums(o, w.cts, gk, DIRECT_STEPS, DIRECT_WEIGHTS, GROUPS, idx, cache=cache)
    _check_sums(o, w.sk, got, ref, w.vals, DIRECT_STEPS, DIRECT_WEIGHTS, GROUPS, idx, "one per group")
    idx = [0, 1, 2, 3]
    out = ev.rotate_rows_sum_weighted(w.dev[:TERMS], DIRECT_STEPS, DIRECT_WEIGHTS, w.gkd["D"], groups=GROUPS, src_index=idx)
    ref = _oracle_sums(o, w.cts, gk, DIRECT_STEPS, DIRECT_WEIGHTS, 1, idx, cache=cache)
    _check_sums(o, w.sk, to_host(out[:1]), ref, w.vals, DIRECT_STEPS, DIRECT_WEIGHTS, 1, idx, "shared")
    for g in range(1, GROUPS):
        assert torch.equal(out[g], out[0]), g
    # the same (source, step) with weights 2 and -3 contributes -1
    twice = ev.rotate_rows_sum_weighted(w.dev[:4], [2045, 2045], [2, -3], w.gkd["D"], groups=1, src_index=[3, 3])
    once = ev.rotate_rows_sum_weighted(w.dev[:4], [2045], [-1], w.gkd["D"], groups=1, src_index=[3])
    assert torch.equal(twice, once)
    ref = np.stack([o.negate(o.rotate_rows(w.cts[3], 2045, gk))])
    _check_sums(o, w.sk, to_host(twice), ref, w.vals, [2045], [-1], 1, [3], "twice")
    ev.check()


# ---- 7: the Galois form ------------------------------------------------------------------------------------------------------
def test_apply_galois_sum_weighted():
    """The identity, the column element 2N - 1 and two row elements under D."""
    from sunscreen_amd.batch import to_host

    w = _world()
    o = w.o
    elts = [1, 2 * o.n - 1, o.galois_elt_from_step(1), o.galois_elt_from_step(2045)]
    ev = w.ev("split")
    out, seen = _profiled(ev, lambda: ev.apply_galois_sum_weighted(w.dev, elts, DIRECT_WEIGHTS, w.gkd["D"]))
    assert seen.get("ks_head") == 1 and seen.get("ks_tail_sum") == 1 and not {"ks_tail", "galois", "eltwise"} & set(seen), seen
    ref = _oracle_sums(o, w.cts, w.gk["D"], elts, DIRECT_WEIGHTS, GROUPS, None, galois=True)
    _check_sums(o, w.sk, to_host(out), ref, w.vals, [0, None, 1, 2045], DIRECT_WEIGHTS, GROUPS, None, "galois")
    ev.check()


# ---- 8: eight groups ---------------------------------------------------------------------------------------------------------
def test_eight_groups_take_the_xcd_row_order():
    """8 groups x 2 terms: the summing tail's grid has 2 * 8 (polynomial, group) rows, a multiple of 8 -- the XCD row order."""
    from sunscreen_amd.batch import to_host

    w = _world()
    steps, weights = [2045, -13], [3, -2]
    ev = w.ev("split")
    out, seen = _profiled(ev, lambda: ev.rotate_rows_sum_weighted(w.dev[:16], steps, weights, w.gkd["D"]))
    assert seen.get("ks_tail_sum") == 1 and "eltwise" not in seen, seen
    ref = _oracle_sums(w.o, w.cts, w.gk["D"], steps, weights, 8, None, cache=_case1(w)["cache"])
    _check_sums(w.o, w.sk, to_host(out), ref, w.vals, steps, weights, 8, None, "8 groups")
    ev.check()


# ---- 9: every body the dispatcher selects ------------------------------------------------------------------------------------
class _Small:
    """Fresh keys for exactly BODY_STEPS' elements, one encryption per item of 2 groups x 3 terms, the reference sums."""

    def __init__(self, n, primes, t, seed):
        self.n, self.primes, self.t = n, primes, t
        self.o = o = O.Oracle(n, primes, t)
        O.seed(seed)
        elts = sorted({o.galois_elt_from_step(s) for s in BODY_STEPS if s})
        self.sk, pk, _, self.gk = o.keygen(relin=False, galois_elts=elts)
        self.groups = 2
        self.vals = [_slots(n, t, j) for j in range(self.groups * len(BODY_STEPS))]
        self.cts = np.stack([o.encrypt(pk, o.batch_encode(v)) for v in self.vals])
        self.ref = _oracle_sums(o, self.cts, self.gk, BODY_STEPS, BODY_WEIGHTS, self.groups, None)

    def check(self, got, what):
        _check_sums(self.o, self.sk, got, self.ref, self.vals, BODY_STEPS, BODY_WEIGHTS, self.groups, None, what)


_SMALL = {}
_SEEDS = {"default_8192": 8193, "seal_fhe_unit": 8194, "mixed_8192": 5402, "default_16384": 16385, "unit_1024": 1025}


def _small(name):
    if name not in _SMALL:
        if name == "mixed_8192":
            n = 8192
            primes, t = O.coeff_modulus_create(n, [54, 54, 54, 56]), O.plain_batching(n, 17)
        elif name == "unit_1024":
            n = 1024
            primes, t = O.coeff_modulus_create(n, [50, 30, 30, 50, 50]), O.plain_batching(n, 20)
        else:
            n, primes, t = params(name)
        _SMALL[name] = _Small(n, primes, t, _SEEDS[name])
    return _SMALL[name]


def _run_small(c, monkeypatch):
    from sunscreen_amd import Context, GaloisKeys
    from sunscreen_amd.batch import BatchEvaluator, to_device, to_host

    ctx = Context.from_raw(c.n, c.primes, c.t)
    monkeypatch.setenv("HIPBFV_NO_SMALL_BATCH", "1")
    ev = BatchEvaluator(ctx)
    gkd = GaloisKeys.from_arrays(ctx, c.gk)
    dev = to_device(c.cts)
    out, seen = _profiled(ev, lambda: ev.rotate_rows_sum_weighted(dev, BODY_STEPS, BODY_WEIGHTS, gkd))
    ev.check()
    return ctx, to_host(out), seen


@pytest.mark.parametrize("name,K,KK", [("default_8192", 4, 5), ("seal_fhe_unit", 4, 5), ("mixed_8192", 3, 4), ("default_16384", 8, 9)])
def test_every_body_of_the_weighted_summing_tail(name, K, KK, monkeypatch):
    """default_8192: packed FP64 rows, K = 4 (the weighted body sums through the output rows: DESIGN.md 5.10.1).  seal_fhe_unit: two
    50-bit data primes, 8-byte FP64 rows, sums in registers.  mixed_8192: every key prime takes the integer policy (MIXED).
    default_16384: K = 8, the sums go through the output rows.  In the through-output forms the first term, weight -2, lands weighted
    on the descriptor without records."""
    c = _small(name)
    if name == "seal_fhe_unit":
        assert max(c.primes[:K]) >= 1 << 48
    assert BODY_WEIGHTS[0] != 1 and BODY_WEIGHTS[BODY_STEPS.index(0)] != 1
    ctx, got, seen = _run_small(c, monkeypatch)
    assert ctx.K == K and ctx.KK == KK
    assert seen.get("ks_head") == 1 and seen.get("ks_mid") == 1 and seen.get("ks_tail_sum") == 1, seen
    assert not {"ks_tail", "galois", "ks_mac", "eltwise"} & set(seen), seen
    c.check(got, name)


# ---- 10: the folded routes ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("chunk", [None, 3])
def test_the_folded_route_at_the_same_degree(chunk, monkeypatch):
    """HIPBFV_NO_FUSED_GALOIS=1 (read when an evaluator is made): the terms are rotated into a stage and folded by one scaled
    accumulate per term and group -- the bits of case 1.  chunk 3: every group is longer than the chunk and is folded in slices of
    3 + 1 terms, the second onto the first with the weight of row 3."""
    import torch
    from sunscreen_amd.batch import BatchEvaluator

    w = _world()
    monkeypatch.setenv("HIPBFV_NO_FUSED_GALOIS", "1")
    ev = BatchEvaluator(w.ctx)
    if chunk:
        ev.set_chunk_ops(chunk)
    out, seen = _profiled(ev, lambda: ev.rotate_rows_sum_weighted(w.dev, DIRECT_STEPS, DIRECT_WEIGHTS, w.gkd["D"]))
    assert "ks_tail_sum" not in seen and seen.get("eltwise") == GROUPS * TERMS, seen
    assert torch.equal(out, _case1(w)["out"])
    ev.check()


def test_below_the_split_kernels_the_terms_are_staged_and_folded(monkeypatch):
    """n = 1024 with the bit sizes of the reference's unit-test set: the whole-polynomial key switch and the scaled accumulate."""
    c = _small("unit_1024")
    ctx, got, seen = _run_small(c, monkeypatch)
    assert "ks_head" not in seen and "ks_tail_sum" not in seen and seen.get("ks_mac") and seen.get("eltwise") == 2 * 3, seen
    c.check(got, "n = 1024")


# ---- 11: the lane-split geometry build ---------------------------------------------------------------------------------------
def test_the_lane_split_geometry_build_gives_the_same_bits():
    """libhipbfv_geom8.so in a process of its own: the words of case 9's default_16384."""
    lib = os.path.join(ROOT, "sunscreen_amd", "lib", "variants", "libhipbfv_geom8.so")
    assert os.path.exists(lib), "build the variant library first: make -C sunscreen_amd/csrc variants (build() does)"
    c = _small("default_16384")
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
out = ev.rotate_rows_sum_weighted(to_device(z["cts"]), [int(s) for s in z["steps"]], [int(x) for x in z["w"]], gk)
torch.cuda.synchronize()
seen = ev.profile_read()
assert seen["ks_tail_sum"]["launches"] == 1 and "ks_tail" not in seen and "eltwise" not in seen, seen
ev.check()
np.savez(sys.argv[2], out=to_host(out))
""" % ROOT
    with tempfile.TemporaryDirectory() as td:
        src, dst = os.path.join(td, "in.npz"), os.path.join(td, "out.npz")
        elts = sorted(c.gk)
        np.savez(src, n=c.n, primes=np.array(c.primes, dtype=np.uint64), t=c.t, cts=c.cts, elts=np.array(elts, dtype=np.uint64),
                 keys=np.stack([c.gk[e] for e in elts]), steps=np.array(BODY_STEPS, dtype=np.int64), w=np.array(BODY_WEIGHTS, dtype=np.int64))
        subprocess.check_call([sys.executable, "-c", script, src, dst], env=dict(os.environ, HIPBFV_LIB=lib, HIPBFV_NO_SMALL_BATCH="1"))
        c.check(np.load(dst)["out"], "geom8")


# ---- 12: refusals ------------------------------------------------------------------------------------------------------------
def _raw(ev, ct, sources, src_index, index_len, steps, weights, gk, out, groups, terms):
    """The C entry point itself: the arguments a mirror would refuse on its own."""
    import torch
    from sunscreen_amd import _lib
    from sunscreen_amd.seal import _check

    idx = None if src_index is None else (C.c_uint32 * max(1, len(src_index)))(*src_index)
    st = None if steps is None else (C.c_int32 * max(1, len(steps)))(*steps)
    wt = None if weights is None else (C.c_int32 * max(1, len(weights)))(*weights)
    _check(_lib.load().hipbfv_batch_rotate_rows_sum_weighted(ev._h, C.c_void_p(ct.data_ptr()), sources, idx, index_len, st, wt,
                                                             gk.get_handle() if gk is not None else None, C.c_void_p(out.data_ptr()), groups, terms,
                                                             C.c_void_p(torch.cuda.current_stream().cuda_stream)))


def _refusals():
    one = [i // TERMS for i in range(COUNT)]
    wt = DIRECT_WEIGHTS
    # name, holding, (sources, src_index, index_len, steps, weights, groups, terms), HRESULT, words of the message
    return [
        ("no weights", "D", (COUNT, None, 0, DIRECT_STEPS, None, GROUPS, TERMS), E_POINTER, ()),
        ("a step of n/2", "D", (COUNT, None, 0, [1, -13, H, 2045], wt, GROUPS, TERMS), E_INVALIDARG, ("term 2:", "step count")),
        ("a step of n/2 with weight 0", "D", (COUNT, None, 0, [1, -13, H, 2045], [2, -1, 0, -2], GROUPS, TERMS), E_INVALIDARG, ("term 2:", "step count")),
        ("a missing chain key", "M", (COUNT, None, 0, [1, 0, 2, -11], wt, GROUPS, TERMS), E_INVALIDARG, ("term 3:", "key")),
        ("a missing chain key with weight 0", "M", (COUNT, None, 0, [1, 0, 2, -11], [2, -1, 3, 0], GROUPS, TERMS), E_INVALIDARG, ("term 3:", "key")),
        ("an index equal to sources", "D", (GROUPS, one[:7] + [GROUPS] + one[8:], COUNT, DIRECT_STEPS, wt, GROUPS, TERMS), E_INVALIDARG, ("item 7:",)),
        ("an empty index table", "D", (GROUPS, one, 0, DIRECT_STEPS, wt, GROUPS, TERMS), E_INVALIDARG, ("index",)),
        ("no table and too few sources", "D", (COUNT - 1, None, 0, DIRECT_STEPS, wt, GROUPS, TERMS), E_INVALIDARG, ("sources",)),
        ("no terms", "D", (COUNT, None, 0, DIRECT_STEPS, wt, GROUPS, 0), E_INVALIDARG, ("term",)),
        ("no steps", "D", (COUNT, None, 0, None, wt, GROUPS, TERMS), E_POINTER, ()),
    ]


@pytest.mark.parametrize("what,holding,args,hresult,words", _refusals(), ids=[r[0] for r in _refusals()])
def test_refusals_launch_nothing_and_write_nothing(what, holding, args, hresult, words):
    import torch

    w = _world()
    ev = w.ev("split")
    sources, src_index, index_len, steps, weights, groups, terms = args
    da = w.dev.clone()
    out = torch.full((GROUPS, 2, w.ctx.K, w.ctx.poly_modulus_degree), SENTINEL, dtype=torch.int64, device=da.device)
    (hr, msg), seen = _profiled(ev, lambda: _hr(lambda: _raw(ev, da, sources, src_index, index_len, steps, weights, w.gkd[holding], out, groups, terms)))
    assert hr == hresult and all(word in msg for word in words), (what, hex(hr), msg)
    assert seen == {}, (what, seen)
    assert bool((out == SENTINEL).all()) and torch.equal(da, w.dev), what


def test_overlapping_output_is_refused_and_no_groups_is_ok():
    import torch

    w = _world()
    ev = w.ev("split")
    buf = torch.cat([w.dev, torch.full_like(w.dev[:GROUPS], SENTINEL)])
    before = buf.clone()
    wt = DIRECT_WEIGHTS
    calls = {
        "out2 == ct2": lambda: _raw(ev, buf, COUNT, None, 0, DIRECT_STEPS, wt, w.gkd["D"], buf, GROUPS, TERMS),
        "one item of overlap": lambda: _raw(ev, buf, COUNT, None, 0, DIRECT_STEPS, wt, w.gkd["D"], buf[COUNT - 1:], GROUPS, TERMS),
    }
    for what in ("out2 == ct2", "one item of overlap"):
        (hr, msg), seen = _profiled(ev, lambda: _hr(calls[what]))
        assert hr == E_INVALIDARG and "overlap" in msg and seen == {}, (what, hex(hr), msg, seen)
    (hr, msg), seen = _profiled(ev, lambda: _hr(lambda: _raw(ev, buf, COUNT, None, 0, DIRECT_STEPS, wt, None, buf[COUNT:], GROUPS, TERMS)))
    assert hr == E_POINTER and seen == {}, (hex(hr), msg, seen)
    (hr, msg), seen = _profiled(ev, lambda: _hr(lambda: _raw(ev, buf, 0, None, 0, DIRECT_STEPS, wt, w.gkd["D"], buf[COUNT:], 0, TERMS)))
    assert hr == 0 and seen == {}, (hex(hr), msg, seen)
    torch.cuda.synchronize()
    assert torch.equal(buf, before)


def test_the_galois_form_refuses_as_the_row_form_does():
    import torch
    from sunscreen_amd import _lib
    from sunscreen_amd.seal import _check

    w = _world()
    ev = w.ev("split")
    out = torch.full((GROUPS, 2, w.ctx.K, w.ctx.poly_modulus_degree), SENTINEL, dtype=torch.int64, device=w.dev.device)
    o = w.o

    def raw(elts, weights):
        e = None if elts is None else (C.c_uint32 * len(elts))(*elts)
        wt = None if weights is None else (C.c_int32 * len(weights))(*weights)
        _check(_lib.load().hipbfv_batch_apply_galois_sum_weighted(ev._h, C.c_void_p(w.dev.data_ptr()), COUNT, None, 0, e, wt, w.gkd["D"].get_handle(),
                                                                  C.c_void_p(out.data_ptr()), GROUPS, TERMS, C.c_void_p(torch.cuda.current_stream().cuda_stream)))

    good = [1, 2 * o.n - 1, o.galois_elt_from_step(1), o.galois_elt_from_step(2045)]
    for what, elts, weights, hresult in (("no weights", good, None, E_POINTER), ("no elements", None, DIRECT_WEIGHTS, E_POINTER),
                                         ("an even element", good[:3] + [4], [2, -1, 3, 0], E_INVALIDARG),
                                         ("an element without a key", good[:3] + [o.galois_elt_from_step(7)], DIRECT_WEIGHTS, E_INVALIDARG)):
        (hr, msg), seen = _profiled(ev, lambda: _hr(lambda: raw(elts, weights)))
        assert hr == hresult and seen == {}, (what, hex(hr), msg, seen)
        assert hresult == E_POINTER or "term 3:" in msg, (what, msg)
    assert bool((out == SENTINEL).all())


# ---- 13: transparent sums ----------------------------------------------------------------------------------------------------
def test_cancelling_and_zero_weights_are_reported_under_the_group_number():
    """Group 1 lists (source 3, step 2045) twice, the other groups two different sources: weights (+1, -1) cancel group 1 alone.
    All-zero weights make every group transparent; the first is named."""
    from sunscreen_amd import _lib
    from sunscreen_amd.batch import _stream

    w = _world()
    ev = w.ev("split")
    L = _lib.load()
    first = C.c_uint64()
    ev.check()
    idx = [0, 1, 3, 3, 4, 5]
    out = ev.rotate_rows_sum_weighted(w.dev, [2045, 2045], [1, -1], w.gkd["D"], groups=3, src_index=idx)
    assert not out[1].any() and out[0].any() and out[2].any()
    hr, msg = _hr(ev.check)
    assert hr == COR_E_INVALIDOPERATION and "item 1)" in msg, (hex(hr), msg)
    ev.check()
    ev.rotate_rows_sum_weighted(w.dev, [2045, 2045], [1, -1], w.gkd["D"], groups=3, src_index=idx)
    assert L.hipbfv_batch_status(ev._h, C.byref(first), _stream()) & 0xFFFFFFFF == COR_E_INVALIDOPERATION and first.value == 1
    out = ev.rotate_rows_sum_weighted(w.dev, DIRECT_STEPS, [0, 0, 0, 0], w.gkd["D"])
    assert not out.any()
    assert L.hipbfv_batch_status(ev._h, C.byref(first), _stream()) & 0xFFFFFFFF == COR_E_INVALIDOPERATION and first.value == 0
    ev.rotate_rows_sum_weighted(w.dev, DIRECT_STEPS, DIRECT_WEIGHTS, w.gkd["D"])
    assert L.hipbfv_batch_status(ev._h, C.byref(first), _stream()) == 0 and first.value == 2**64 - 1


# ---- 14: the convolution workload --------------------------------------------------------------------------------------------
def test_convolve_slots_is_the_convolution_of_each_row():
    """Taps (1, -2, 1): slot j of each row = x[j] - 2 x[j + 1] + x[j + 2] mod t, indices within the row."""
    from sunscreen_amd import workloads
    from sunscreen_amd.batch import to_host

    w = _world()
    o, ev = w.o, w.ev("split")
    taps = (1, -2, 1)
    out, seen = _profiled(ev, lambda: workloads.convolve_slots(ev, w.dev[:GROUPS], taps, w.gkd["P"]))
    assert seen.get("ks_tail_sum") == 1 and "eltwise" not in seen, seen
    got = to_host(out)
    idx = [i // 3 for i in range(3 * GROUPS)]
    ref = _oracle_sums(o, w.cts, w.gk["P"], [0, 1, 2], list(taps), GROUPS, idx)
    _check_sums(o, w.sk, got, ref, w.vals, [0, 1, 2], list(taps), GROUPS, idx, "taps (1, -2, 1)")
    h = o.n // 2
    for g in range(GROUPS):
        x = w.vals[g].astype(np.int64).reshape(2, h)
        want = sum(tap * np.take(x, (np.arange(h) + k) % h, axis=1) for k, tap in enumerate(taps)) % o.t
        assert (o.batch_decode(o.decrypt(got[g], w.sk)).astype(np.int64) == want.reshape(-1)).all(), g
    ev.check()
