"""Weighted sums of rotations without a GPU: the two entry points are declared, exported and named by every mirror; the
tap-to-(steps, weights) helper of workloads.convolve_slots; and the weight table the new summing tail reads
(hipbfv_debug_weight_residues) on the primes of the GPU tests' world, against Python integers."""
import os
import re

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENTRY_POINTS = ["hipbfv_batch_rotate_rows_sum_weighted", "hipbfv_batch_apply_galois_sum_weighted"]
EXTREME = [0, -1, -(2**31), 2**31 - 1]


def _read(*parts):
    with open(os.path.join(ROOT, *parts)) as f:
        return f.read()


@pytest.mark.parametrize("name", ENTRY_POINTS)
def test_the_entry_points_are_declared_and_exported(name):
    from sunscreen_amd import _lib

    assert hasattr(_lib.load(), name)
    header = _read("include", "hipbfv.h")
    assert f"long {name}(" in header
    # the argument list of the unweighted call with `const int32_t *weights` behind the steps / elements
    decl = re.search(r"long %s\((.*?)\);" % name, header, re.S).group(1)
    plain = re.search(r"long %s\((.*?)\);" % name[: -len("_weighted")], header, re.S).group(1)
    args = [" ".join(a.split()) for a in decl.split(",")]
    want = [" ".join(a.split()) for a in plain.split(",")]
    assert args[:6] == want[:6] and args[6] == "const int32_t *weights" and args[7:] == want[6:], (args, want)


@pytest.mark.parametrize("name", ENTRY_POINTS)
def test_the_mirrors_name_the_entry_points(name):
    from sunscreen_amd import _lib
    from sunscreen_amd.batch import BatchEvaluator

    assert name in _read("include", "hipbfv.hpp")
    assert "bindgen::" + name in _read("rust", "hip_bfv", "src", "batch.rs")
    assert name in _read("sunscreen_amd", "batch.py") and name in _read("INTEGRATION.md")
    method = name[len("hipbfv_batch_"):]
    assert callable(getattr(BatchEvaluator, method))
    fn = getattr(_lib.load(), name)
    plain = getattr(_lib.load(), name[: -len("_weighted")])
    assert len(fn.argtypes) == len(plain.argtypes) + 1


def test_taps_become_steps_and_weights_in_tap_order_without_the_zero_taps():
    from sunscreen_amd.workloads import convolution_terms

    assert convolution_terms([1, -2, 1]) == ([0, 1, 2], [1, -2, 1])
    assert convolution_terms([-1, 0, 1]) == ([0, 2], [-1, 1])
    assert convolution_terms([0, 0, 5, 0]) == ([2], [5])
    assert convolution_terms([1, 4, 6, 4, 1]) == ([0, 1, 2, 3, 4], [1, 4, 6, 4, 1])
    assert convolution_terms([0, 0]) == ([], []) and convolution_terms([]) == ([], [])
    steps, weights = convolution_terms([2**31 - 1, 0, -(2**31)])
    assert steps == [0, 2] and weights == [2**31 - 1, -(2**31)] and all(type(w) is int for w in weights)


def test_convolve_slots_makes_one_weighted_call_with_one_source_per_group():
    """The arguments convolve_slots hands to the evaluator, seen by a stand-in: src_index[i] = i // terms over the non-zero taps."""
    from sunscreen_amd.workloads import convolve_slots

    class X:
        shape = (3, 2, 2, 64)

    class Ev:
        def rotate_rows_sum_weighted(self, x, steps, weights, gk, groups=None, src_index=None):
            self.seen = (x, steps, weights, gk, groups, src_index)
            return "out"

    ev, x = Ev(), X()
    assert convolve_slots(ev, x, [1, 0, -2, 1], "keys") == "out"
    assert ev.seen == (x, [0, 2, 3], [1, -2, 1], "keys", 3, [0, 0, 0, 1, 1, 1, 2, 2, 2])
    with pytest.raises(ValueError):
        convolve_slots(ev, x, [0, 0], "keys")


@pytest.mark.parametrize("name", ["default_4096_16", "seal_fhe_unit", "default_16384"])
def test_the_table_the_summing_tail_reads_on_the_tests_primes(name):
    """(w mod q_i, floor(r * 2^64 / q_i)) for the extreme weights on the data primes of the GPU tests' parameter sets."""
    from sunscreen_amd.batch import weight_residues
    from tests.bfv_helpers import oracle_for

    primes = oracle_for(name).primes
    tab = weight_residues(primes, EXTREME)
    assert len(tab) == len(EXTREME)
    for t, w in enumerate(EXTREME):
        assert len(tab[t]) == len(primes)
        for i, q in enumerate(primes):
            r = w % q
            assert tab[t][i] == (r, (r << 64) // q), (w, q, tab[t][i])
    assert all(pair == (0, 0) for pair in tab[0]) and all(tab[1][i][0] == q - 1 for i, q in enumerate(primes))
