"""The weight table of the weighted sums of products (hipbfv_debug_weight_residues, host only) against Python integers: for every
weight w and modulus q the entry is (w mod q, canonical in [0, q), and floor(that * 2^64 / q)) -- the pair the kernels multiply by."""
import ctypes as C

import pytest

WEIGHTS = [0, 1, -1, 3, -2, 2**31 - 1, -(2**31)]
E_POINTER = 0x80004003
E_INVALIDARG = 0x80070057


def _is_prime(m):
    # Miller-Rabin with the first twelve primes as bases: deterministic below 3.3e24
    bases = (2, 3, 5, 7, 11, 13, 17, 19, 23, 29, 31, 37)
    if m < 2 or any(m % b == 0 for b in bases):
        return m in bases
    d, s = m - 1, 0
    while d % 2 == 0:
        d, s = d // 2, s + 1
    for b in bases:
        x = pow(b, d, m)
        if x in (1, m - 1):
            continue
        for _ in range(s - 1):
            x = x * x % m
            if x == m - 1:
                break
        else:
            return False
    return True


def _primes():
    """The largest primes of 61, 49, 36 and 20 bits (the table is host arithmetic on any modulus: no transform-friendliness needed); the
    20-bit one is below the two extreme weights, so |w| > q is exercised."""
    out = []
    for bits in (61, 49, 36, 20):
        m = (1 << bits) - 1
        while not _is_prime(m):
            m -= 2
        assert m.bit_length() == bits
        out.append(m)
    return out


def test_the_table_is_the_canonical_residue_and_its_exact_shoup_quotient():
    from sunscreen_amd.batch import weight_residues

    primes = _primes()
    tab = weight_residues(primes, WEIGHTS)
    assert len(tab) == len(WEIGHTS) and all(len(row) == len(primes) for row in tab)
    for t, w in enumerate(WEIGHTS):
        for i, q in enumerate(primes):
            r, quo = tab[t][i]
            assert r == w % q and 0 <= r < q, (w, q, r)  # (Python's % is the canonical residue for negative w too)
            assert quo == (r << 64) // q, (w, q, quo)
    assert abs(WEIGHTS[-1]) > primes[-1] and WEIGHTS[-2] > primes[-1]


def test_a_negated_weight_gives_the_negated_residue():
    from sunscreen_amd.batch import weight_residues

    primes = _primes()
    pos = [1, 3, 2, 2**31 - 1, 2**20, primes[-1], 2 * primes[-1]]  # (the last two are multiples of the 20-bit prime: residue 0 both ways)
    tab_p, tab_n = weight_residues(primes, pos), weight_residues(primes, [-w for w in pos])
    for t, w in enumerate(pos):
        for i, q in enumerate(primes):
            m = tab_p[t][i][0]
            assert m == w % q
            assert tab_n[t][i][0] == (q - m if m else 0), (w, q)
    assert tab_p[5][3][0] == 0 and tab_n[5][3] == (0, 0) and tab_n[6][3] == (0, 0)


def test_null_pointers_and_out_of_range_moduli_are_refused():
    from sunscreen_amd import _lib

    L = _lib.load()
    p = (C.c_uint64 * 1)(97)
    w = (C.c_int32 * 1)(5)
    out = (C.c_uint64 * 2)(7, 7)
    assert L.hipbfv_debug_weight_residues(None, 1, w, 1, out) & 0xFFFFFFFF == E_POINTER
    assert L.hipbfv_debug_weight_residues(p, 1, None, 1, out) & 0xFFFFFFFF == E_POINTER
    assert L.hipbfv_debug_weight_residues(p, 1, w, 1, None) & 0xFFFFFFFF == E_POINTER
    for bad in (0, 1, 1 << 62):
        assert L.hipbfv_debug_weight_residues((C.c_uint64 * 1)(bad), 1, w, 1, out) & 0xFFFFFFFF == E_INVALIDARG, bad
    assert list(out) == [7, 7]
    assert L.hipbfv_debug_weight_residues(p, 1, w, 1, out) == 0 and list(out) == [5, (5 << 64) // 97]


@pytest.mark.parametrize("name", ["hipbfv_batch_multiply_sum_weighted", "hipbfv_batch_multiply_sum_weighted_relin",
                                  "hipbfv_batch_multiply_sum_weighted_relin_keys", "hipbfv_debug_weight_residues"])
def test_the_entry_points_are_exported_and_declared(name):
    import os

    from sunscreen_amd import _lib

    assert hasattr(_lib.load(), name)
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    assert f"long {name}(" in open(os.path.join(root, "include", "hipbfv.h")).read()
