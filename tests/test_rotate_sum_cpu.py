"""Host-side checks of the sums of rotations (hipbfv_batch_rotate_rows_sum / hipbfv_batch_apply_galois_sum): the plan that decides
per term between the source itself, a direct key inside the summing sequence and a NAF chain beforehand, and cuts the call into
launch sequences (hipbfv_debug_rotate_sum_plan: no device is touched); the oracle side of tests/test_gpu_rotate_sum.py -- the fold
of the oracle's rotations decodes to the sum of the rolled rows with noise budget to spare, for the exact shapes of its first
group; the mirrors' shape checks; the symbols and their mirrors."""
import os
import re

import numpy as np
import pytest

from oracle import bfv_oracle as O
from tests import rotation_plan_expect as X
from tests.bfv_helpers import oracle_for, params
from tests.test_gpu_rotation_steps import COUNT, DIRECT, H, NAME, _rolled, _slots

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
E_INVALIDARG = 0x80070057
N = 2 * H
GROUPS, TERMS = 5, 4
DIRECT_STEPS = [1, -13, 0, 2045]
CHAIN_STEPS = [11, 1707, 1, 2045]
POW2 = X.pow2(N)
HELD = {"P": POW2, "D": POW2 + [X.elt(s, N) for s in DIRECT], "M": [e for e in POW2 if e != X.elt(4, N)]}


def _plan(steps, held, groups=GROUPS, chunk=4096, n=N):
    from sunscreen_amd.batch import rotate_sum_plan

    return rotate_sum_plan(n, steps, held, groups, chunk)


def _refused(steps, held, groups=GROUPS, chunk=4096):
    from sunscreen_amd.seal import HipBfvError

    with pytest.raises(HipBfvError) as e:
        _plan(steps, held, groups, chunk)
    return e.value.hresult & 0xFFFFFFFF, str(e.value)


@pytest.mark.parametrize("holding", ["P", "D", "M"])
@pytest.mark.parametrize("steps", [DIRECT_STEPS, CHAIN_STEPS, [1, -2, 0], [2045, 2045], [0], [1024, -1024, 2047, 1365, -683, 1025]],
                         ids=["direct", "chain", "small", "twice", "identity", "edges"])
def test_every_term_decides_as_the_one_rotation_planner_decides(steps, holding):
    held = HELD[holding]
    want = [X.expected(N, s, frozenset(held)) for s in steps]
    bad = [t for t, (k, _) in enumerate(want) if k in (X.TOO_LARGE, X.NO_KEY)]
    if bad:
        hr, msg = _refused(steps, held)
        assert hr == E_INVALIDARG and f"term {bad[0]}:" in msg and want[bad[0]][0] in msg, msg
        return
    kind, elt, rounds, _ = _plan(steps, held)
    assert kind == [k for k, _ in want]
    assert rounds == [r for _, r in want]
    for t, s in enumerate(steps):
        if kind[t] == X.DIRECT:
            assert elt[t] == X.elt(s, N), (t, s)


def test_the_kinds_of_the_gpu_cases():
    assert _plan(DIRECT_STEPS, HELD["D"])[0] == [X.DIRECT, X.DIRECT, X.COPY, X.DIRECT]
    kind, _, rounds, _ = _plan(CHAIN_STEPS, HELD["P"])
    assert kind == [X.CHAIN, X.CHAIN, X.DIRECT, X.CHAIN]
    assert rounds == [len(X.hops(11, N)), len(X.hops(1707, N)), 0, len(X.hops(2045, N))] == [3, 5, 0, 2]


def test_refused_steps_and_chunks():
    for steps, t, word in (([1, -13, H, 2045], 2, "step count"), ([-H], 0, "step count"), ([1, 0, 2, -11], 3, "key")):
        hr, msg = _refused(steps, HELD["M"] if word == "key" else HELD["D"])
        assert hr == E_INVALIDARG and f"term {t}:" in msg and word in msg, msg
    assert _plan([1, 0, 2, -11], HELD["P"])[0][3] == X.CHAIN  # (P holds the key of +4 that M lacks)
    hr, msg = _refused(DIRECT_STEPS, HELD["D"], chunk=0)  # as hipbfv_debug_multiply_sum_plan refuses it
    assert hr == E_INVALIDARG and "chunk" in msg, msg
    hr, msg = _refused([], HELD["D"])
    assert hr == E_INVALIDARG and "term" in msg, msg


@pytest.mark.parametrize("chunk", [20, 7, 3, 1])
def test_the_launch_sequences_are_the_sum_of_products_plan(chunk):
    """(5, 4): one sequence for all groups at 20; one group per sequence at 7; every group in slices of 3 + 1 at 3 and in four
    slices of one term at 1, every slice but a group's first accumulating."""
    from sunscreen_amd.batch import multiply_sum_plan

    seq = _plan(DIRECT_STEPS, HELD["D"], GROUPS, chunk)[3]
    want = {
        20: [(0, 5, 0, 4, False)],
        7: [(g, 1, 0, 4, False) for g in range(5)],
        3: [s for g in range(5) for s in ((g, 1, 0, 3, False), (g, 1, 3, 1, True))],
        1: [(g, 1, t, 1, t > 0) for g in range(5) for t in range(4)],
    }[chunk]
    assert seq == want
    assert seq == multiply_sum_plan(GROUPS, TERMS, chunk)
    assert _plan(DIRECT_STEPS, HELD["D"], 0, chunk)[3] == []


# ---- the oracle side of the GPU tests' first group: every expected sum decrypts to the sum of the rolled rows ------------------
@pytest.fixture(scope="module")
def world():
    n, primes, t = params(NAME)
    o = oracle_for(NAME)
    O.seed(7101)  # the world of tests/test_gpu_rotation_steps.py: the same keys and encryptions
    pow2 = [o.galois_elt_from_step(s * (1 << i)) for i in range(H.bit_length() - 1) for s in (1, -1)] + [2 * n - 1]
    direct = [o.galois_elt_from_step(s) for s in DIRECT]
    sk, pk, _, gk = o.keygen(relin=False, galois_elts=sorted(set(pow2)) + direct)
    vals = [_slots(n, t, j) for j in range(COUNT)]
    cts = np.stack([o.encrypt(pk, o.batch_encode(v)) for v in vals])
    return {"o": o, "sk": sk, "gk": {"P": {e: gk[e] for e in pow2}, "D": dict(gk)}, "vals": vals, "cts": cts, "t": t}


def _fold(w, holding, steps, groups, src, galois=False):
    """Per group: the oracle's rotations folded with o.add, the noise budget of the sum and the slots it must decode to."""
    o, gk = w["o"], w["gk"][holding]
    for g in range(groups):
        acc, want = None, np.zeros_like(w["vals"][0])
        for k, step in enumerate(steps):
            s = src[g * len(steps) + k]
            v = w["vals"][s]
            if galois:
                r = w["cts"][s] if step == 1 else o.apply_galois(w["cts"][s], step, gk)
                row = {1: 0, o.galois_elt_from_step(1): 1, o.galois_elt_from_step(2045): 2045}.get(step)
                v = np.concatenate([v[v.size // 2:], v[: v.size // 2]]) if row is None else _rolled(v, row)
            else:
                r = o.rotate_rows(w["cts"][s], step, gk) if step else w["cts"][s]
                v = _rolled(v, step)
            acc = r if acc is None else o.add(acc, r)
            want = (want + v) % np.uint64(w["t"])
        yield g, o.noise_budget(acc, w["sk"]), o.batch_decode(o.decrypt(acc, w["sk"])), want


def _shapes(o):
    ident = list(range(COUNT))
    return [
        ("case 1", "D", DIRECT_STEPS, GROUPS, ident, False),
        ("case 2, one per group", "D", DIRECT_STEPS, GROUPS, [i // TERMS for i in range(COUNT)], False),
        ("case 2, shared", "D", DIRECT_STEPS, 1, [0, 1, 2, 3], False),  # (every group is this one)
        ("case 2, twice", "D", [2045, 2045], 1, [3, 3], False),
        ("case 3", "P", CHAIN_STEPS, GROUPS, ident, False),
        ("case 4", "D", [2045], 2, ident, False),
        ("case 5", "D", [1, 2 * o.n - 1, o.galois_elt_from_step(1), o.galois_elt_from_step(2045)], GROUPS, ident, True),
    ]


def test_the_oracles_sums_decrypt_to_the_sum_of_the_rolled_rows(world):
    for what, holding, steps, groups, src, galois in _shapes(world["o"]):
        for g, budget, got, want in _fold(world, holding, steps, groups, src, galois):
            assert budget > 0, (what, g, budget)
            assert (got == want).all(), (what, g)


# ---- the mirrors ----------------------------------------------------------------------------------------------------------
def test_the_python_mirrors_check_their_shapes():
    import torch
    from sunscreen_amd.batch import BatchEvaluator

    class _Shapes(BatchEvaluator):
        def __init__(self):  # (no context, no device: the checks run before anything reaches the library)
            self.n, self.K = 8, 2

    ev = _Shapes()
    ct = torch.zeros((6, 2, 2, 8), dtype=torch.int64)
    assert ev._rotation_sum_args(ct, 3, None, None, torch.zeros((2, 2, 2, 8), dtype=torch.int64))[0] == 2
    assert ev._rotation_sum_args(ct, 2, None, [0, 1, 5, 5], torch.zeros((2, 2, 2, 8), dtype=torch.int64))[:3:2] == (2, 4)
    assert ev._rotation_sum_args(ct, 2, 4, [0, 1], torch.zeros((4, 2, 2, 8), dtype=torch.int64))[0] == 4
    for bad in (lambda: ev._rotation_sum_args(ct, 4, None, None, None),  # 6 sources are no whole number of groups of 4
                lambda: ev._rotation_sum_args(ct, 3, 3, None, None),  # 3 groups of 3 terms are not 6 sources
                lambda: ev._rotation_sum_args(ct, 0, None, None, None),
                lambda: ev._rotation_sum_args(ct, 2, None, [0, 6], None),  # an index equal to the sources
                lambda: ev._rotation_sum_args(ct, 2, None, [], None),
                lambda: ev._rotation_sum_args(ct, 2, None, [0, 1, 2], None),  # 3 items are no whole number of groups of 2
                lambda: ev._rotation_sum_args(ct, 3, None, None, torch.zeros((3, 2, 2, 8), dtype=torch.int64)),  # an output of another size
                lambda: ev._rotation_sum_args(ct[:, :, :1], 3, None, None, None)):
        with pytest.raises(AssertionError):
            bad()
    from sunscreen_amd import workloads

    with pytest.raises(ValueError):
        workloads.window_sum(ev, ct, 0, None)


def test_the_symbols_are_declared_exported_and_mirrored():
    from sunscreen_amd import _lib

    L = _lib.load()
    header = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "hipbfv.h")).read(), flags=re.S)
    head = ["void *", "const uint64_t *", "uint64_t", "const uint32_t *", "uint64_t"]
    tail = ["void *", "uint64_t *", "uint64_t", "uint64_t", "void *"]
    want = {
        "hipbfv_batch_rotate_rows_sum": head + ["const int32_t *"] + tail,
        "hipbfv_batch_apply_galois_sum": head + ["const uint32_t *"] + tail,
        "hipbfv_debug_rotate_sum_plan": ["uint64_t", "const int32_t *", "uint64_t", "const uint32_t *", "uint64_t", "uint64_t", "uint64_t", "int32_t *",
                                         "uint32_t *", "uint32_t *", "uint64_t *", "uint64_t", "uint64_t *"],
    }
    for name, types in want.items():
        m = re.search(r"long\s+" + name + r"\s*\(([^)]*)\)\s*;", header)
        assert m, name
        got = [re.sub(r"\s+", " ", p).strip() for p in m.group(1).split(",")]
        assert len(got) == len(types), (name, got)
        for p, t in zip(got, types):
            assert p.startswith(t) and re.fullmatch(r"\w+", p[len(t):].strip()), (name, p, t)
        assert hasattr(L, name), name
        assert len(_lib._SIGNATURES[name]) == len(types), name
    calls = list(want)[:2]
    for path, names in (("include/hipbfv.hpp", calls), ("rust/hip_bfv/src/batch.rs", calls), ("sunscreen_amd/batch.py", list(want)), ("INTEGRATION.md", calls)):
        text = open(os.path.join(ROOT, path)).read()
        for name in names:
            assert name in text, (path, name)
    from sunscreen_amd import workloads
    from sunscreen_amd.batch import BatchEvaluator

    hpp, rs = open(os.path.join(ROOT, "include", "hipbfv.hpp")).read(), open(os.path.join(ROOT, "rust", "hip_bfv", "src", "batch.rs")).read()
    for method in ("rotate_rows_sum", "apply_galois_sum"):
        assert callable(getattr(BatchEvaluator, method))
        assert "fn %s(" % method in rs and "void %s(" % method in hpp, method
    assert callable(workloads.window_sum)


def test_the_profiler_names_the_summing_tail_beside_its_twin():
    import ctypes as C

    from sunscreen_amd import _lib

    L = _lib.load()
    cnt = C.c_uint32()
    assert L.hipbfv_profile_kernel_count(C.byref(cnt)) == 0
    src = open(os.path.join(ROOT, "sunscreen_amd", "csrc", "evaluator.cpp")).read()
    names = re.findall(r'"(\w+)"', re.search(r"static const char\* names\[kKernCount\] = \{(.*?)\};", src, re.S).group(1))
    assert len(names) == cnt.value and names[names.index("ks_tail") + 1] == "ks_tail_sum", names
    enum = re.findall(r"kKern\w+", re.search(r"enum KernelId : int \{(.*?)\};", open(os.path.join(ROOT, "sunscreen_amd", "csrc", "evaluator.hpp")).read(), re.S).group(1))
    assert [e[5:].lower() for e in enum[:-1]] == [n.replace("_", "") for n in names], (enum, names)
