"""Products of two prepared operands (hipbfv_batch_multiply*_prepared), the part that needs no GPU: the entry points exist in every
mirror of the C ABI, the matrix-product index helper pairs A[i][t] with B[t][j], and the index rule -- item i multiplies prepared
ciphertext a_index[i % index_len] by b_index[i % index_len], i = g * terms + t in the sum forms -- holds for every launch sequence of
the library's plan, which reads the call's index table from its first item."""
import os
import re
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEAD = ["void *", "void *", "const uint32_t *", "void *", "const uint32_t *", "uint64_t"]  # evaluator, ma, a_index, mb, b_index, index_len
WANT = {
    "hipbfv_batch_multiply_prepared": HEAD + ["uint64_t *", "uint64_t", "void *"],
    "hipbfv_batch_multiply_relin_prepared": HEAD + ["void *", "uint64_t *", "uint64_t", "void *"],
    "hipbfv_batch_multiply_sum_prepared": HEAD + ["uint64_t *", "uint64_t", "uint64_t", "void *"],
    "hipbfv_batch_multiply_sum_relin_prepared": HEAD + ["void *", "uint64_t *", "uint64_t", "uint64_t", "void *"],
}


def _read(*parts):
    with open(os.path.join(ROOT, *parts)) as f:
        return f.read()


def test_the_entry_points_are_declared_exported_and_mirrored():
    from sunscreen_amd import _lib, workloads
    from sunscreen_amd.batch import BatchEvaluator

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
        assert name + "(" in hpp, name
        assert "bindgen::" + name + "(" in rs, name
    for method in ("multiply_prepared", "multiply_relin_prepared", "multiply_sum_prepared", "multiply_sum_relin_prepared"):
        assert callable(getattr(BatchEvaluator, method))
        assert "fn %s(" % method in rs and "void %s(" % method in hpp, method
    assert callable(workloads.matrix_product) and callable(workloads.matrix_product_index)
    for helper in ("matrix_product_index(", "matrix_product("):
        assert "fn " + helper in rs and "void " + helper in hpp, helper
    # (NULL evaluator: E_POINTER before any object or the device is touched)
    for name in WANT:
        args = [None] * len(WANT[name])
        for i, ty in enumerate(WANT[name]):
            if ty == "uint64_t":
                args[i] = 1
        assert getattr(L, name)(*args) & 0xFFFFFFFF == 0x80004003, name


@pytest.mark.parametrize("m,k,n", [(2, 3, 2), (3, 5, 2)])
def test_the_index_helper_pairs_a_row_of_a_with_a_column_of_b(m, k, n):
    """A is prepared row-major m x k, B row-major k x n: item (i * n + j) * k + t is A[i][t] * B[t][j], so group i * n + j sums row i of
    A against column j of B."""
    from sunscreen_amd.workloads import matrix_product_index

    a_index, b_index = matrix_product_index(m, k, n)
    assert len(a_index) == len(b_index) == m * n * k
    for i in range(m):
        for j in range(n):
            for t in range(k):
                item = (i * n + j) * k + t
                assert divmod(a_index[item], k) == (i, t), (i, j, t)  # A[i][t]
                assert divmod(b_index[item], n) == (t, j), (i, j, t)  # B[t][j]
    assert max(a_index) == m * k - 1 and max(b_index) == k * n - 1 and min(a_index) == min(b_index) == 0
    with pytest.raises(ValueError):
        matrix_product_index(m, 0, n)


@pytest.mark.parametrize("chunk", [4096, 7, 2])
@pytest.mark.parametrize("m,k,n", [(2, 3, 2), (3, 5, 2)])
def test_the_index_rule_holds_under_chunks_and_slices(chunk, m, k, n):
    """groups = m * n, terms = k.  A sequence covers the items first .. first + count of the call (group-major) and reads the pair
    (a_index, b_index)[(first + i) % index_len]: every (group, term) once, each with the pair the rule gives it -- with the full-length
    tables of the matrix product, and with a shorter period (their first k * n entries, reused cyclically)."""
    from sunscreen_amd.batch import multiply_sum_plan
    from sunscreen_amd.workloads import matrix_product_index

    a_index, b_index = matrix_product_index(m, k, n)
    groups, terms = m * n, k
    plan = multiply_sum_plan(groups, terms, chunk)
    for index_len in (len(a_index), k * n):
        seen = {}
        for g0, ng, t0, nt, _acc in plan:
            assert (t0 == 0 and nt == terms) or ng == 1  # the sequence's items are consecutive items of the call
            first = g0 * terms + t0
            for i in range(ng * nt):
                g, t = divmod(first + i, terms)
                assert (g, t) not in seen and g0 <= g < g0 + ng and t0 <= t < t0 + nt
                seen[(g, t)] = (a_index[(first + i) % index_len], b_index[(first + i) % index_len])
        assert seen == {(g, t): (a_index[(g * terms + t) % index_len], b_index[(g * terms + t) % index_len]) for g in range(groups) for t in range(terms)}
        if index_len == len(a_index):
            assert seen == {(i * n + j, t): (i * k + t, t * n + j) for i in range(m) for j in range(n) for t in range(k)}
