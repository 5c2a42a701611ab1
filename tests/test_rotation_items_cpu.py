"""Host-side checks of the mixed-step rotation entry points: the symbols, their mirrors, and the plan that decides, per item,
between a copy, the mixed launch and a NAF chain group (hipbfv_debug_rotate_items_plan: no device is touched)."""
import os
import re

import pytest

from tests import rotation_plan_expect as X

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
E_INVALIDARG = 0x80070057
N = 4096
H = N // 2
INT_MIN = -(2**31)
COPY, DIRECT, CHAIN = 0, 1, 2


def _elt(step, n=N):
    """The Galois element of a row rotation: 3^step for a left rotation, 3^(n/2 - |step|) for a right one (mod 2n)."""
    assert 0 < abs(step) < n // 2
    return pow(3, step if step > 0 else n // 2 - abs(step), 2 * n)


POW2 = [_elt(s * (1 << i)) for i in range(H.bit_length() - 1) for s in (1, -1)]


def _plan(steps, present, n=N):
    from sunscreen_amd.batch import rotate_items_plan

    return rotate_items_plan(n, steps, present)


def _refused(steps, present, n=N):
    from sunscreen_amd.seal import HipBfvError

    with pytest.raises(HipBfvError) as e:
        _plan(steps, present, n)
    return e.value.hresult & 0xFFFFFFFF, str(e.value)


def test_both_symbols_are_exported_with_the_declared_arity():
    from sunscreen_amd import _lib

    L = _lib.load()
    header = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "hipbfv.h")).read(), flags=re.S)
    want = {
        "hipbfv_batch_apply_galois_items": ["void *", "const uint64_t *", "const uint32_t *", "void *", "uint64_t *", "uint64_t", "void *"],
        "hipbfv_batch_rotate_rows_items": ["void *", "const uint64_t *", "const int32_t *", "void *", "uint64_t *", "uint64_t", "void *"],
    }
    for name, types in want.items():
        m = re.search(r"long\s+" + name + r"\s*\(([^)]*)\)\s*;", header)
        assert m, name
        params = [re.sub(r"\s+", " ", p).strip() for p in m.group(1).split(",")]
        assert len(params) == len(types) == 7, (name, params)
        for p, t in zip(params, types):
            assert p.startswith(t) and re.fullmatch(r"\w+", p[len(t):].strip()), (name, p, t)
        assert hasattr(L, name), name
        assert len(_lib._SIGNATURES[name]) == 7, name
    assert len(_lib._SIGNATURES["hipbfv_debug_rotate_items_plan"]) == 8 and hasattr(L, "hipbfv_debug_rotate_items_plan")


def test_the_mirrors_name_both_entry_points():
    for path in ("include/hipbfv.hpp", "rust/hip_bfv/src/batch.rs", "sunscreen_amd/batch.py"):
        text = open(os.path.join(ROOT, path)).read()
        for name in ("hipbfv_batch_apply_galois_items", "hipbfv_batch_rotate_rows_items"):
            assert name in text, (path, name)
        for method in ("apply_galois_items", "rotate_rows_items"):
            assert re.search(r"\b" + method + r"\s*\(", text), (path, method)
    doc = open(os.path.join(ROOT, "INTEGRATION.md")).read()
    assert "hipbfv_batch_rotate_rows_items" in doc and "hipbfv_batch_apply_galois_items" in doc


def test_the_plan_copies_joins_the_mixed_launch_or_groups_by_chain():
    """D-like holding: the power-of-two keys and the direct key of 1365.  1365 and -683 share that element (they differ by
    n/2): both are direct, with the same element.  11 and -11 have no key of their own: one chain group per step, in the
    order the steps first appear, equal steps in one group."""
    e1365 = _elt(1365)
    assert e1365 == _elt(-683) and e1365 not in POW2
    steps = [0, 1, 1365, 11, -683, 11, -11, 0, -1024, 11]
    kind, group, chains = _plan(steps, POW2 + [e1365])
    assert kind == [COPY, DIRECT, DIRECT, CHAIN, DIRECT, CHAIN, CHAIN, COPY, DIRECT, CHAIN]
    assert [group[i] for i in (1, 2, 4, 8)] == [_elt(1), e1365, e1365, _elt(-1024)]
    assert [group[i] for i in (3, 5, 6, 9)] == [0, 0, 1, 0] and chains == 2
    assert group[0] == 0 and group[7] == 0


def test_two_steps_of_one_element_without_its_key_walk_their_own_chains():
    """Under the power-of-two keys alone 1365 = [1, 4, ..., 1024] and -683 = [1, 4, ..., 256, -1024] are different chains,
    although their element is one: they must not share a group."""
    kind, group, chains = _plan([1365, -683, 1365, 2047], POW2)
    assert kind == [CHAIN, CHAIN, CHAIN, DIRECT] and group[:3] == [0, 1, 0] and chains == 2
    assert group[3] == _elt(-1)  # n/2 - 1: the element, and the key, of step -1


def test_every_item_a_copy_and_no_item_direct():
    assert _plan([0, 0, 0], []) == ([COPY] * 3, [0] * 3, 0)
    assert _plan([], POW2) == ([], [], 0)
    kind, group, chains = _plan([11, 1707, 11, 2045], POW2)
    assert kind == [CHAIN] * 4 and group == [0, 1, 0, 2] and chains == 3
    # a single direct key and nothing else: steps it does not serve have no chain either
    assert _plan([5, 5], [_elt(5)]) == ([DIRECT, DIRECT], [_elt(5)] * 2, 0)


@pytest.mark.parametrize("bad", [H, -H, H + 1, 2**31 - 1, INT_MIN])
def test_a_refused_step_names_its_item(bad):
    hr, msg = _refused([1, 0, bad, bad], POW2)
    assert hr == E_INVALIDARG and re.search(r"\bitem 2\b", msg) and "step count" in msg, (hex(hr), msg)


def test_a_missing_key_names_the_first_item_that_needs_it():
    """-11 = [1, 4, -16] reads the key of +4; 11 = [-1, -4, 16] does not.  A step whose NAF is one part has no chain."""
    without4 = [e for e in POW2 if e != _elt(4)]
    kind, _, chains = _plan([11, 1, 11], without4)
    assert kind == [CHAIN, DIRECT, CHAIN] and chains == 1
    hr, msg = _refused([11, 1, -11, 4], without4)
    assert hr == E_INVALIDARG and re.search(r"\bitem 2\b", msg) and "key" in msg and "step count" not in msg, (hex(hr), msg)
    hr, msg = _refused([0, 4], without4)
    assert hr == E_INVALIDARG and re.search(r"\bitem 1\b", msg) and "key" in msg, (hex(hr), msg)


# ---- the planner against an independent derivation, every step of four degrees ----------------------------------------
def _sweep(n, name, held):
    """Accepted steps in batches (a refusal would name its item), the steps expected to be refused one per call."""
    want = {s: X.expected(n, s, held) for s in X.sweep_steps(n)}
    for chunk in X.batches([s for s in want if want[s][0] in (COPY, DIRECT, CHAIN)]):
        kind, group, chains = _plan(chunk, sorted(held), n)
        assert kind == [want[s][0] for s in chunk], (n, name, chunk)
        assert [g for s, g in zip(chunk, group) if want[s][0] == DIRECT] == [X.elt(s, n) for s in chunk if want[s][0] == DIRECT], (n, name, chunk)
        assert chains == kind.count(CHAIN), (n, name, chunk)  # (distinct steps: a group each)
    for step, (why, _) in want.items():
        if why in (X.TOO_LARGE, X.NO_KEY):
            hr, msg = _refused([0, step], sorted(held), n)
            assert hr == E_INVALIDARG and re.search(r"\bitem 1\b", msg) and why in msg, (n, name, step, msg)
            assert why == X.TOO_LARGE or X.TOO_LARGE not in msg, (n, name, step, msg)


@pytest.mark.parametrize("n", X.DEGREES)
def test_every_step_plans_as_the_independent_naf_says(n):
    """Kind and refusal of every step in (-n/2, n/2), of +-n/2, n/2 + 1, INT_MIN and INT_MAX, over every +-2^i key and over
    that set with each power removed in turn; then every step over a set that holds its own key alone: direct."""
    for name, held in X.holdings(n):
        _sweep(n, name, held)
    for step in range(-n // 2 + 1, n // 2):
        if step:
            assert _plan([step], [X.elt(step, n)], n) == ([DIRECT], [X.elt(step, n)], 0), (n, step)
    assert X.expected(n, n // 2 - 1, frozenset(X.pow2(n)))[0] == DIRECT  # the element of step -1


def test_the_edge_steps_of_degree_4096():
    """2047 and 2046 go through the keys of -1 and -2 and walk no chain; 2045, 1707 and 1365 are chains (their hop counts are in
    tests/test_rotation_items_keys_cpu.py); 11 does not read the key of +4, -11 does."""
    assert X.hops(2045, N) == [1, -4] and X.hops(1707, N) == [-1, -4, -16, -64, -256] and X.hops(1365, N) == [1, 4, 16, 64, 256, 1024]
    assert X.hops(11, N) == [-1, -4, 16] and X.hops(-11, N) == [1, 4, -16]
    kind, group, chains = _plan([2047, 2046, 2045, 1707, 1365], POW2)
    assert kind == [DIRECT, DIRECT, CHAIN, CHAIN, CHAIN] and group[:2] == [_elt(-1), _elt(-2)] and chains == 3
    without4 = [e for e in POW2 if e != _elt(4)]
    assert _plan([11], without4) == ([CHAIN], [0], 1)
    hr, msg = _refused([-11], without4)
    assert hr == E_INVALIDARG and "key" in msg and "step count" not in msg, msg
