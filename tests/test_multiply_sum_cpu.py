"""Sums of products with one relinearization per group (hipbfv_batch_multiply_sum, _relin, _relin_keys), the part that needs no GPU:
the three entry points exist in every mirror of the C ABI, and the chunk and slice rule the evaluator launches by
(hipbfv_debug_multiply_sum_plan: no device is touched) matches a model written from the rule's description."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("hipbfv_batch_multiply_sum", "hipbfv_batch_multiply_sum_relin", "hipbfv_batch_multiply_sum_relin_keys")
E_INVALIDARG = 0x80070057
E_POINTER = 0x80004003


def _read(*parts):
    with open(os.path.join(ROOT, *parts)) as f:
        return f.read()


def _hr(v):
    return v & 0xFFFFFFFF


def test_the_entry_points_are_declared_exported_and_mirrored():
    from sunscreen_amd import _lib

    header = _read("include", "hipbfv.h")
    want = {
        NAMES[0]: ["void *", "const uint64_t *", "const uint64_t *", "uint64_t *", "uint64_t", "uint64_t", "void *"],
        NAMES[1]: ["void *", "const uint64_t *", "const uint64_t *", "void *", "uint64_t *", "uint64_t", "uint64_t", "void *"],
        NAMES[2]: ["void *", "const uint64_t *", "const uint64_t *", "void *const *", "uint64_t", "const uint32_t *", "uint64_t *", "uint64_t",
                   "uint64_t", "void *"],
    }
    for name, types in want.items():
        m = re.search(r"long %s\(([^;]*)\);" % name, header)
        assert m, name
        got = [re.sub(r"\s*\w+$", "", re.sub(r"\s+", " ", a.strip())) for a in m.group(1).split(",")]
        assert got == types, (name, got)
        assert len(_lib._SIGNATURES[name]) == len(types), name
    # exports.map hides the mangled names and nothing else: the library must export the three C names
    assert re.search(r"local:\s*_Z\*;\s*__hip_\*;", _read("sunscreen_amd", "csrc", "exports.map"))
    lib = os.path.join(ROOT, "sunscreen_amd", "lib", "libhipbfv.so")
    dyn = subprocess.run(["nm", "-D", "--defined-only", lib], capture_output=True, text=True, check=True).stdout
    exported = {line.split()[-1] for line in dyn.splitlines() if line.strip()}
    L = _lib.load()
    for name in NAMES + ("hipbfv_debug_multiply_sum_plan",):
        assert name in exported, name
        assert getattr(L, name).argtypes == _lib._SIGNATURES[name], name
    hpp, rs = _read("include", "hipbfv.hpp"), _read("rust", "hip_bfv", "src", "batch.rs")
    for name in NAMES:
        assert name + "(" in hpp, name
        assert "bindgen::" + name + "(" in rs, name
    from sunscreen_amd.batch import BatchEvaluator

    for method in ("multiply_sum", "multiply_sum_relin", "multiply_sum_relin_keys"):
        assert callable(getattr(BatchEvaluator, method))
        assert "fn %s(" % method in rs and "void %s(" % method in hpp, method


def test_the_profiler_names_the_summing_tail_last():
    """The kernel kinds are numbered by position (bench.py and the profiles read them by name): the new one is appended."""
    from sunscreen_amd import _lib

    L = _lib.load()
    cnt = C.c_uint32()
    assert L.hipbfv_profile_kernel_count(C.byref(cnt)) == 0
    src = _read("sunscreen_amd", "csrc", "evaluator.cpp")
    names = re.findall(r'"(\w+)"', re.search(r"static const char\* names\[kKernCount\] = \{(.*?)\};", src, re.S).group(1))
    assert len(names) == cnt.value and names[-2:] == ["mul_tail", "mul_tail_sum"], names
    enum = re.findall(r"kKern\w+", re.search(r"enum KernelId : int \{(.*?)\};", _read("sunscreen_amd", "csrc", "evaluator.hpp"), re.S).group(1))
    assert enum[-3:] == ["kKernMulTail", "kKernMulTailSum", "kKernCount"], enum[-3:]


def _model(groups, terms, chunk):
    """The rule as include/hipbfv.h and DESIGN.md state it, on arrays: which (group, term) pairs a launch sequence covers and whether
    it adds onto sums an earlier sequence wrote."""
    chunk = min(chunk, 65535)
    g, t = np.meshgrid(np.arange(groups), np.arange(terms), indexing="ij")
    if terms <= chunk:
        per = min(max(1, chunk // terms), 65535)
        seq = g // per
    else:
        seq = g * -(-terms // chunk) + t // chunk
    steps = []
    for s in np.unique(seq):
        gs, ts = g[seq == s], t[seq == s]
        steps.append((int(gs.min()), int(gs.max() - gs.min() + 1), int(ts.min()), int(ts.max() - ts.min() + 1), bool(ts.min() > 0)))
    return steps


@pytest.mark.parametrize("groups,terms,chunk", [
    (3, 5, 4096), (3, 5, 7), (3, 5, 2), (3, 5, 5), (3, 5, 10), (3, 5, 14), (3, 5, 15), (3, 5, 1), (1, 1, 1), (7, 1, 3), (1, 9, 4), (4, 3, 3),
    (2, 8, 7), (5, 2, 3), (0, 4, 8), (40, 3, 1 << 40), (2, 70000, 1 << 40)])
def test_the_chunk_and_slice_rule_matches_its_model(groups, terms, chunk):
    from sunscreen_amd.batch import multiply_sum_plan

    got = multiply_sum_plan(groups, terms, chunk)
    assert got == _model(groups, terms, chunk), (got, _model(groups, terms, chunk))
    # every (group, term) pair exactly once, at most a chunk of items and 65535 groups per sequence, a whole number of groups or a
    # slice of one, the first slice of a group writing and the later ones accumulating
    seen = np.zeros((groups, terms), dtype=np.int32)
    for g0, ng, t0, nt, acc in got:
        seen[g0:g0 + ng, t0:t0 + nt] += 1
        assert ng * nt <= min(chunk, 65535) and 1 <= ng <= 65535 and nt >= 1
        assert (t0 == 0 and nt == terms) or ng == 1
        assert acc == (t0 > 0)
    assert (seen == 1).all()


def test_the_three_chunk_settings_of_the_gpu_test_give_1_3_and_9_sequences():
    from sunscreen_amd.batch import multiply_sum_plan

    assert multiply_sum_plan(3, 5, 4096) == [(0, 3, 0, 5, False)]
    assert multiply_sum_plan(3, 5, 7) == [(g, 1, 0, 5, False) for g in range(3)]
    assert multiply_sum_plan(3, 5, 2) == [(g, 1, t0, nt, t0 > 0) for g in range(3) for t0, nt in ((0, 2), (2, 2), (4, 1))]


def test_the_plan_entry_point_refuses_what_the_calls_refuse():
    from sunscreen_amd import _lib

    L = _lib.load()
    n = C.c_uint64(77)
    buf = (C.c_uint64 * 10)()
    assert _hr(L.hipbfv_debug_multiply_sum_plan(3, 0, 8, buf, 2, C.byref(n))) == E_INVALIDARG  # no terms
    assert _hr(L.hipbfv_debug_multiply_sum_plan(3, 5, 0, buf, 2, C.byref(n))) == E_INVALIDARG
    assert _hr(L.hipbfv_debug_multiply_sum_plan(3, 5, 8, buf, 2, None)) == E_POINTER
    assert _hr(L.hipbfv_debug_multiply_sum_plan(3, 5, 8, None, 2, C.byref(n))) == E_POINTER
    assert _hr(L.hipbfv_debug_multiply_sum_plan(3, 5, 7, buf, 2, C.byref(n))) == E_INVALIDARG and n.value == 3  # capacity 2, three sequences
    assert L.hipbfv_debug_multiply_sum_plan(0, 5, 7, None, 0, C.byref(n)) == 0 and n.value == 0
