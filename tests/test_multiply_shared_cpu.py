"""Prepared multiplicands (hipbfv_Multiplicand_*, hipbfv_batch_multiply*_shared), the part that needs no GPU: the entry points exist
in every mirror of the C ABI, and the index rule -- item i multiplies by prepared ciphertext b_index[i % index_len], i = g * terms + t
in the sum forms -- holds for every launch sequence of the library's plan, which reads the call's index table from its first item."""
import ctypes as C
import os
import re
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEAD = ["void *", "const uint64_t *", "void *", "const uint32_t *", "uint64_t"]  # evaluator, a, multiplicand, b_index, index_len
WANT = {
    "hipbfv_Multiplicand_Create": ["void *", "const uint64_t *", "uint64_t", "void *", "void **"],
    "hipbfv_Multiplicand_Destroy": ["void *"],
    "hipbfv_Multiplicand_Count": ["void *", "uint64_t *"],
    "hipbfv_Multiplicand_Bytes": ["void *", "uint64_t *"],
    "hipbfv_batch_multiply_shared": HEAD + ["uint64_t *", "uint64_t", "void *"],
    "hipbfv_batch_multiply_relin_shared": HEAD + ["void *", "uint64_t *", "uint64_t", "void *"],
    "hipbfv_batch_multiply_sum_shared": HEAD + ["uint64_t *", "uint64_t", "uint64_t", "void *"],
    "hipbfv_batch_multiply_sum_relin_shared": HEAD + ["void *", "uint64_t *", "uint64_t", "uint64_t", "void *"],
}


def _read(*parts):
    with open(os.path.join(ROOT, *parts)) as f:
        return f.read()


def test_the_entry_points_are_declared_exported_and_mirrored():
    from sunscreen_amd import _lib
    from sunscreen_amd.batch import BatchEvaluator, Multiplicand

    header = re.sub(r"/\*.*?\*/", "", _read("include", "hipbfv.h"), flags=re.S)
    lib = os.path.join(ROOT, "sunscreen_amd", "lib", "libhipbfv.so")
    dyn = subprocess.run(["nm", "-D", "--defined-only", lib], capture_output=True, text=True, check=True).stdout
    exported = {line.split()[-1] for line in dyn.splitlines() if line.strip()}
    hpp, rs = _read("include", "hipbfv.hpp"), _read("rust", "hip_bfv", "src", "batch.rs")
    L = _lib.load()
    for name, types in WANT.items():
        m = re.search(r"long %s\(([^;]*)\);" % name, header)
        assert m, name
        got = [re.sub(r"\s*\w+$", "", re.sub(r"\s+", " ", a.strip())) for a in m.group(1).split(",")]
        assert got == types, (name, got)
        assert name in exported and len(getattr(L, name).argtypes) == len(types), name
        assert name + "(" in hpp or name + "," in hpp, name  # (the destructor is a template argument of the handle class)
        assert "bindgen::" + name + "(" in rs, name
    assert callable(BatchEvaluator.prepare) and hasattr(Multiplicand, "count") and hasattr(Multiplicand, "nbytes")
    assert "fn prepare(" in rs and "prepare_multiplicand(" in hpp
    for method in ("multiply_shared", "multiply_relin_shared", "multiply_sum_shared", "multiply_sum_relin_shared"):
        assert callable(getattr(BatchEvaluator, method))
        assert "fn %s(" % method in rs and "void %s(" % method in hpp, method
    n = C.c_uint64()
    for call in (lambda: L.hipbfv_Multiplicand_Count(None, C.byref(n)), lambda: L.hipbfv_Multiplicand_Bytes(None, C.byref(n)),
                 lambda: L.hipbfv_Multiplicand_Destroy(None)):
        assert call() & 0xFFFFFFFF == 0x80004003  # E_POINTER, no device touched


@pytest.mark.parametrize("chunk,sequences", [(4096, 1), (7, 3), (2, 9)])
@pytest.mark.parametrize("index_len", [1, 5, 15])
def test_the_index_rule_holds_under_chunks_and_slices(chunk, sequences, index_len):
    """3 groups x 5 terms: one sequence at the default chunk, one group per sequence at 7 items, slices of 2, 2 and 1 terms at 2.  A
    sequence covers the items first .. first + count of the call (group-major) and reads b_index[(first + i) % index_len]: every
    (group, term) pair once, each with the index the rule gives it."""
    from sunscreen_amd.batch import multiply_sum_plan

    b_index = {1: [0], 5: [0, 1, 2, 3, 4], 15: [3, 3, 0, 4, 1, 2, 2, 4, 0, 0, 1, 3, 4, 4, 2]}[index_len]
    plan = multiply_sum_plan(3, 5, chunk)
    assert len(plan) == sequences
    seen = {}
    for g0, ng, t0, nt, _acc in plan:
        assert (t0 == 0 and nt == 5) or ng == 1  # the sequence's items are consecutive items of the call
        first = g0 * 5 + t0
        for i in range(ng * nt):
            g, t = divmod(first + i, 5)
            assert (g, t) not in seen and g0 <= g < g0 + ng and t0 <= t < t0 + nt
            seen[(g, t)] = b_index[(first + i) % index_len]
    assert seen == {(g, t): b_index[(g * 5 + t) % index_len] for g in range(3) for t in range(5)}
