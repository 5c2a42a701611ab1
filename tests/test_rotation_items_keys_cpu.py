"""Host-side checks of the mixed-step rotation batches with one key set per client: the symbols, their mirrors, and the plan
that decides per (key set, step) pair between a copy, the mixed launch and a NAF chain, numbers the mixed launch's key table
by (element, set) and counts the shared chain rounds (hipbfv_debug_rotate_items_keys_plan: no device is touched)."""
import os
import re

import pytest

from tests import rotation_plan_expect as X

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
E_INVALIDARG = 0x80070057
E_POINTER = 0x80004003
N = 4096
H = N // 2
COPY, DIRECT, CHAIN = 0, 1, 2


def _elt(step, n=N):
    """The Galois element of a row rotation: 3^step for a left rotation, 3^(n/2 - |step|) for a right one (mod 2n)."""
    assert 0 < abs(step) < n // 2
    return pow(3, step if step > 0 else n // 2 - abs(step), 2 * n)


def _naf(step):
    """SEAL's non-adjacent form of a step, least significant part first."""
    neg, v, parts, i = step < 0, abs(step), [], 0
    while v:
        z = 2 - (v & 3) if v & 1 else 0
        v = (v - z) >> 1
        if z:
            parts.append((-z if neg else z) * (1 << i))
        i += 1
    return parts


def _rounds(step, n=N):
    """The rounds of a step's chain: its NAF parts without the part of n/2 rows."""
    return len([p for p in _naf(step) if abs(p) != n // 2])


POW2 = [_elt(s * (1 << i)) for i in range(H.bit_length() - 1) for s in (1, -1)]


def _plan(steps, key_index, sets, n=N):
    from sunscreen_amd.batch import rotate_items_keys_plan

    return rotate_items_keys_plan(n, steps, key_index, sets)


def _refused(steps, key_index, sets, n=N):
    from sunscreen_amd.seal import HipBfvError

    with pytest.raises(HipBfvError) as e:
        _plan(steps, key_index, sets, n)
    return e.value.hresult & 0xFFFFFFFF, str(e.value)


def test_the_symbols_are_declared_exported_and_mirrored():
    from sunscreen_amd import _lib

    L = _lib.load()
    header = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "hipbfv.h")).read(), flags=re.S)
    keys_tail = ["void *const *", "uint64_t", "const uint32_t *", "uint64_t *", "uint64_t"]
    want = {
        "hipbfv_batch_apply_galois_items_keys": ["void *", "const uint64_t *", "const uint32_t *"] + keys_tail + ["void *"],
        "hipbfv_batch_rotate_rows_items_keys": ["void *", "const uint64_t *", "const int32_t *"] + keys_tail + ["void *"],
        "hipbfv_Pool_RotateRowsItemsKeys": ["void *", "const uint64_t *", "const int32_t *"] + keys_tail,
        "hipbfv_debug_rotate_items_keys_plan": ["uint64_t", "const int32_t *", "const uint32_t *", "uint64_t", "uint64_t", "const uint32_t *",
                                                "const uint64_t *", "int32_t *", "uint32_t *", "uint32_t *", "uint64_t *", "uint64_t *"],
    }
    for name, types in want.items():
        m = re.search(r"long\s+" + name + r"\s*\(([^)]*)\)\s*;", header)
        assert m, name
        params = [re.sub(r"\s+", " ", p).strip() for p in m.group(1).split(",")]
        assert len(params) == len(types), (name, params)
        for p, t in zip(params, types):
            assert p.startswith(t) and re.fullmatch(r"\w+", p[len(t):].strip()), (name, p, t)
        assert hasattr(L, name), name
        assert len(_lib._SIGNATURES[name]) == len(types), name
    for path, names in (("include/hipbfv.hpp", list(want)[:3]), ("rust/hip_bfv/src/batch.rs", list(want)[:2]), ("rust/hip_bfv/src/pool.rs", list(want)[2:3]),
                        ("sunscreen_amd/batch.py", [list(want)[0], list(want)[1], list(want)[3]]), ("sunscreen_amd/pool.py", list(want)[2:3]),
                        ("INTEGRATION.md", list(want)[:3])):
        text = open(os.path.join(ROOT, path)).read()
        for name in names:
            assert name in text, (path, name)
    from sunscreen_amd.batch import BatchEvaluator
    from sunscreen_amd.pool import DevicePool

    assert callable(BatchEvaluator.apply_galois_items_keys) and callable(BatchEvaluator.rotate_rows_items_keys)
    assert callable(DevicePool.rotate_rows_items_keys)


def test_two_clients_with_the_same_step_decide_differently_in_one_call():
    """Set 0: every power-of-two key and the direct key of 3; set 1: the powers of two alone.  3 = [-1, 4]: two rounds."""
    steps = [3, 3, 0, -1, 5, 3]
    sets = [0, 1, 1, 0, 1, 0]
    held = [POW2 + [_elt(3)], POW2]
    kind, entry, rounds_of, entries, rounds = _plan(steps, sets, held)
    assert kind == [DIRECT, CHAIN, COPY, DIRECT, CHAIN, DIRECT]
    assert entry[0] == entry[5] and entry[3] != entry[0] and entries == 2  # items 0 and 5: one (element, set) pair
    assert rounds_of == [0, 2, 0, 0, _rounds(5), 0] and _rounds(3) == 2 and _rounds(5) == 2
    assert rounds == max(_rounds(3), _rounds(5))
    # item 2 is a copy: its set is never looked at.  An all-zero-step client may hold nothing at all:
    steps2, sets2 = [3, 0, 0, -1, 0, 3], [0, 1, 1, 0, 1, 0]
    assert _plan(steps2, sets2, held) == _plan(steps2, sets2, [held[0], []])
    assert _plan(steps2, sets2, held)[0] == [DIRECT, COPY, COPY, DIRECT, COPY, DIRECT]
    # ... and with it, item 2 of the first batch still plans alike while the chain items are what is refused
    hr, msg = _refused(steps, sets, [held[0], []])
    assert hr == E_INVALIDARG and "item 1: key set 1" in msg, msg


def test_the_longest_chain_sets_the_rounds():
    steps = [11, 1365, 3, 1]  # 11 = [-1, -4, 16]; 1365 = [1, 4, 16, 64, 256, 1024]
    kind, entry, rounds_of, entries, rounds = _plan(steps, [0, 0, 1, 1], [POW2, POW2])
    assert kind == [CHAIN, CHAIN, CHAIN, DIRECT]
    assert rounds_of == [3, 6, 2, 0] and rounds == 6 and entries == 1 and entry[3] == 0
    assert _plan([], [], [POW2]) == ([], [], [], 0, 0)
    assert _plan([0, 0], [0, 0], [[]]) == ([COPY, COPY], [0, 0], [0, 0], 0, 0)


def test_table_entries_are_numbered_by_element_then_set():
    """Three sets hold the direct keys of 1, 3 and 5; the items arrive in no order at all.  1365 and -683 share one element."""
    e1365 = _elt(1365)
    assert e1365 == _elt(-683)
    held = [POW2 + [_elt(3), _elt(5), e1365]] * 3
    steps = [5, 3, 1, 3, 5, 1, 3, 1365, -683, 1]
    sets = [2, 1, 2, 0, 0, 0, 1, 1, 1, 2]
    kind, entry, rounds_of, entries, rounds = _plan(steps, sets, held)
    assert kind == [DIRECT] * 10 and rounds == 0 and rounds_of == [0] * 10
    pairs = sorted({(_elt(s), k) for s, k in zip(steps, sets)})
    assert entries == len(pairs) == 7
    assert entry == [pairs.index((_elt(s), k)) for s, k in zip(steps, sets)]
    assert entry[7] == entry[8]  # two steps, one element, one set: one key


@pytest.mark.parametrize("step", [H - 1, -(H - 1), N // 4, -N // 4])
def test_the_step_edges_direct_and_through_the_chain(step):
    """n/2 - 1 = [-1, n/2]: the n/2 part is skipped, so one round -- unless the power-of-two keys serve the step directly, as they
    do here (its element is that of step -1).  n/4 is a power of two: direct under POW2, refused without its key."""
    assert _plan([step], [0], [[_elt(step)]]) == ([DIRECT], [0], [0], 1, 0)
    kind, entry, rounds_of, entries, rounds = _plan([step, step], [1, 0], [POW2, [_elt(step)]])
    assert kind == [DIRECT, DIRECT] and entry == [1, 0] and entries == 2 and rounds == 0
    if abs(step) == N // 4:
        hr, msg = _refused([0, step], [0, 0], [[e for e in POW2 if e != _elt(step)]])
        assert hr == E_INVALIDARG and "item 1: key set 0" in msg and "key" in msg, msg


def test_the_chain_with_the_skipped_part():
    """-683 = [1, 4, 16, 64, 256, -1024] ... and 1707 = [-1, -4, -16, -64, -256, 2048]: the part of n/2 = 2048 rows is the identity on
    the rows and is skipped, 5 rounds; a set needs no key for it."""
    assert _naf(1707)[-1] == H and _rounds(1707) == 5
    kind, entry, rounds_of, entries, rounds = _plan([1707, 1], [0, 0], [POW2])
    assert kind == [CHAIN, DIRECT] and rounds_of == [5, 0] and rounds == 5
    # H - 1 without the key of -1 has a one-round chain of -1 alone: no key, refused
    hr, msg = _refused([H - 1], [0], [[e for e in POW2 if e != _elt(-1)]])
    assert hr == E_INVALIDARG and "item 0: key set 0" in msg


@pytest.mark.parametrize("bad", [H, -H, H + 1, 2**31 - 1, -(2**31)])
def test_a_refused_step_names_its_item_and_set(bad):
    hr, msg = _refused([1, 0, bad, bad], [0, 0, 1, 0], [POW2, POW2])
    assert hr == E_INVALIDARG and "item 2: key set 1" in msg and "step count" in msg, (hex(hr), msg)


def test_a_missing_chain_key_names_the_first_item_that_needs_it():
    """-11 = [1, 4, -16] reads the key of +4; 11 = [-1, -4, 16] does not.  Only set 1 lacks it."""
    without4 = [e for e in POW2 if e != _elt(4)]
    steps, sets = [11, -11, 11, -11, 4], [1, 0, 1, 1, 1]
    hr, msg = _refused(steps, sets, [POW2, without4])
    assert hr == E_INVALIDARG and "item 3: key set 1" in msg and "key" in msg and "step count" not in msg, (hex(hr), msg)
    kind, _, rounds_of, _, rounds = _plan(steps[:3], sets[:3], [POW2, without4])
    assert kind == [CHAIN] * 3 and rounds_of == [3, 3, 3] and rounds == 3


def test_a_key_index_out_of_range_is_refused_for_every_item():
    """... a copied item included, which references no set otherwise."""
    hr, msg = _refused([1, 0, 1], [0, 2, 0], [POW2, POW2])
    assert hr == E_INVALIDARG and "item 1: key set 2" in msg, (hex(hr), msg)
    hr, msg = _refused([1, 1], [0, 0xFFFFFFFF], [POW2])
    assert hr == E_INVALIDARG and "item 1: key set 4294967295" in msg, (hex(hr), msg)


def test_null_arguments_of_the_entry_points_need_no_device():
    import ctypes as C

    from sunscreen_amd import _lib

    L = _lib.load()
    hr = lambda x: x & 0xFFFFFFFF  # noqa: E731
    buf = (C.c_uint64 * 4)()
    steps, elts, idx = (C.c_int32 * 1)(1), (C.c_uint32 * 1)(3), (C.c_uint32 * 1)(0)
    sets = (C.c_void_p * 1)(None)
    assert hr(L.hipbfv_batch_rotate_rows_items_keys(None, buf, steps, sets, 1, idx, buf, 1, None)) == E_POINTER
    assert hr(L.hipbfv_batch_apply_galois_items_keys(None, buf, elts, sets, 1, idx, buf, 1, None)) == E_POINTER
    assert hr(L.hipbfv_Pool_RotateRowsItemsKeys(None, buf, steps, sets, 1, idx, buf, 1)) == E_POINTER
    kind, entry, rounds_of = (C.c_int32 * 1)(), (C.c_uint32 * 1)(), (C.c_uint32 * 1)()
    offsets, ne, nr = (C.c_uint64 * 2)(0, 0), C.c_uint64(), C.c_uint64()
    plan = L.hipbfv_debug_rotate_items_keys_plan
    assert hr(plan(N, None, idx, 1, 1, None, offsets, kind, entry, rounds_of, C.byref(ne), C.byref(nr))) == E_POINTER
    assert hr(plan(N, steps, idx, 1, 1, None, None, kind, entry, rounds_of, C.byref(ne), C.byref(nr))) == E_POINTER
    assert hr(plan(N, steps, idx, 1, 0, None, offsets, kind, entry, rounds_of, C.byref(ne), C.byref(nr))) == E_POINTER
    assert hr(plan(N + 1, steps, idx, 1, 1, None, offsets, kind, entry, rounds_of, C.byref(ne), C.byref(nr))) == E_INVALIDARG


# ---- the planner against an independent derivation, every step of four degrees ----------------------------------------
@pytest.mark.parametrize("n", X.DEGREES)
def test_every_step_plans_as_the_independent_naf_says(n):
    """Kind, refusal and rounds (the chain's hops, the n/2 part left out) of every step in (-n/2, n/2), of +-n/2, n/2 + 1,
    INT_MIN and INT_MAX: set 0 holds every +-2^i key, set 1 that set with one power removed (each power in turn).  Accepted
    steps go in batches (a refusal would name its item), the steps expected to be refused one per call.  Then every step with a
    set of its own that holds the step's key alone: direct, one table entry each."""
    for name, held in X.holdings(n):
        sets = [sorted(X.pow2(n)), sorted(held)]
        want = {(s, k): X.expected(n, s, frozenset(sets[k])) for s in X.sweep_steps(n) for k in (0, 1)}
        for chunk in X.batches([sk for sk in want if want[sk][0] in (COPY, DIRECT, CHAIN)]):
            kind, _, rounds_of, _, rounds = _plan([s for s, _ in chunk], [k for _, k in chunk], sets, n)
            assert kind == [want[sk][0] for sk in chunk], (n, name, chunk)
            assert rounds_of == [want[sk][1] for sk in chunk] and rounds == max(rounds_of), (n, name, chunk)
        for (step, k), (why, _) in want.items():
            if why in (X.TOO_LARGE, X.NO_KEY):
                hr, msg = _refused([0, step], [1 - k, k], sets, n)
                assert hr == E_INVALIDARG and "item 1: key set %d" % k in msg and why in msg, (n, name, step, k, msg)
                assert why == X.TOO_LARGE or X.TOO_LARGE not in msg, (n, name, step, k, msg)
    steps = [s for s in range(-n // 2 + 1, n // 2) if s]
    for chunk in X.batches(steps):
        kind, entry, rounds_of, entries, rounds = _plan(chunk, list(range(len(chunk))), [[X.elt(s, n)] for s in chunk], n)
        assert kind == [DIRECT] * len(chunk) and rounds_of == [0] * len(chunk) and (entries, rounds) == (len(chunk), 0), (n, chunk)
        assert sorted(entry) == list(range(len(chunk))), (n, chunk)


def test_the_edge_steps_of_degree_4096():
    """2047 and 2046 go through the keys of -1 and -2 and walk no chain; 2045 has two hops, 1707 five, 1365 six; 11 does not read
    the key of +4, -11 does."""
    kind, _, rounds_of, entries, rounds = _plan([2047, 2046, 2045, 1707, 1365, -1, -2], [0] * 7, [POW2])
    assert kind == [DIRECT, DIRECT, CHAIN, CHAIN, CHAIN, DIRECT, DIRECT] and rounds_of == [0, 0, 2, 5, 6, 0, 0]
    assert entries == 2 and rounds == 6  # 2047 and -1, 2046 and -2: one key each
    without4 = [e for e in POW2 if e != _elt(4)]
    assert _plan([11], [0], [without4])[2] == [3]
    hr, msg = _refused([-11], [0], [without4])
    assert hr == E_INVALIDARG and "item 0: key set 0" in msg and "step count" not in msg, msg
