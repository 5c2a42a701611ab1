"""Many queries against one database pass (hipbfv_batch_dot_plain_ntt_queries), the part that needs no GPU: the entry point and its
plan function exist in every mirror of the C ABI, and the product launches the evaluator issues (hipbfv_debug_dot_queries_plan: no
device is touched) match a model written from the rule's description."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAME, PLAN = "hipbfv_batch_dot_plain_ntt_queries", "hipbfv_debug_dot_queries_plan"
E_INVALIDARG = 0x80070057
E_POINTER = 0x80004003
SINGLE_RT = 4  # rows per thread of the single-query kernel (launch_dot_plain)
MAX_GRID_X = (1 << 31) - 1


def _read(*parts):
    with open(os.path.join(ROOT, *parts)) as f:
        return f.read()


def _hr(v):
    return v & 0xFFFFFFFF


def test_the_entry_points_are_declared_exported_and_mirrored():
    from sunscreen_amd import _lib

    header = _read("include", "hipbfv.h")
    want = {
        NAME: ["void *", "const uint64_t *", "uint64_t", "uint64_t", "const uint64_t *", "uint64_t", "uint64_t *", "void *"],
        PLAN: ["uint64_t", "uint64_t", "uint64_t", "uint64_t *", "uint64_t", "uint64_t *"],
    }
    for name, types in want.items():
        m = re.search(r"long %s\(([^;]*)\);" % name, header)
        assert m, name
        got = [re.sub(r"\s*\w+$", "", re.sub(r"\s+", " ", a.strip())) for a in m.group(1).split(",")]
        assert got == types, (name, got)
        assert len(_lib._SIGNATURES[name]) == len(types), name
    lib = os.path.join(ROOT, "sunscreen_amd", "lib", "libhipbfv.so")
    dyn = subprocess.run(["nm", "-D", "--defined-only", lib], capture_output=True, text=True, check=True).stdout
    exported = {line.split()[-1] for line in dyn.splitlines() if line.strip()}
    L = _lib.load()
    for name in (NAME, PLAN):
        assert name in exported, name
        assert getattr(L, name).argtypes == _lib._SIGNATURES[name], name
    hpp, rs = _read("include", "hipbfv.hpp"), _read("rust", "hip_bfv", "src", "batch.rs")
    assert NAME + "(" in hpp and "bindgen::" + NAME + "(" in rs
    assert "fn dot_plain_ntt_queries(" in rs and "void dot_plain_ntt_queries(" in hpp
    from sunscreen_amd import batch, workloads

    assert callable(batch.BatchEvaluator.dot_plain_ntt_queries) and callable(batch.dot_queries_plan) and callable(workloads.pir_lookup_queries)
    # the header's aliasing paragraph names the call among those that take no overlap at all
    para = header[header.index("Aliasing.  An output may be EXACTLY"):]
    para = para[: para.index("*/")]
    assert re.search(r"dot_plain_ntt,\s*\*?\s*dot_plain_ntt_queries\) accept no overlap at all", para), para


def _tile():
    """(QT, RT) of the query-tiled kernel, as the library reports it for two queries."""
    from sunscreen_amd.batch import dot_queries_plan

    (step,) = dot_queries_plan(2, 1, 1)
    return step[4], step[5]


def _model(queries, rows, K, QT, RT):
    """The rule as include/hipbfv.h states it: one query is one launch of the single-query kernel; otherwise the queries go in
    order, as many per launch as keep ceil(rows / RT) * ceil(queries / QT) within grid x (a whole number of tiles), a last launch
    left with one query being a single-query launch; every launch covers all rows."""
    if queries == 0:
        return []
    if queries == 1:
        return [(0, 1, 0, rows, 1, SINGLE_RT)]
    per = max(1, MAX_GRID_X // -(-rows // RT)) * QT
    steps = []
    for q0 in range(0, queries, per):
        c = min(per, queries - q0)
        steps.append((q0, 1, 0, rows, 1, SINGLE_RT) if c == 1 else (q0, c, 0, rows, QT, RT))
    return steps


@pytest.mark.parametrize("K", [1, 4, 8])
def test_the_plan_matches_its_model_and_tiles_the_rectangle_once(K):
    from sunscreen_amd.batch import dot_queries_plan

    QT, RT = _tile()
    assert QT >= 2 and RT >= 1
    for queries in range(0, 41):
        for rows in range(1, 10):
            got = dot_queries_plan(queries, rows, K)
            assert got == _model(queries, rows, K, QT, RT), (queries, rows, K, got)
            seen = np.zeros((queries, rows), dtype=np.int32)
            for q0, nq, r0, nr, qt, rt in got:
                assert nq >= 1 and nr >= 1 and qt >= 1 and rt >= 1
                assert (qt == 1) == (nq == 1), (queries, rows, got)  # one query: today's kernel; more: the tiled one
                assert -(-nr // rt) * -(-nq // qt) <= MAX_GRID_X
                seen[q0:q0 + nq, r0:r0 + nr] += 1
            assert (seen == 1).all(), (queries, rows, K, got)
            if queries == 1:
                assert len(got) == 1 and got[0][4] == 1
            if queries == 0:
                assert got == []
            if queries >= 2:
                assert len(got) == 1  # one product launch at every size a test can hold


def test_the_plan_splits_the_queries_where_grid_x_would_overflow():
    """2^32 - 1 rows are 2^31 row blocks at RT = 2 (more at RT = 1): one tile of queries per launch, and a last single query
    takes the single-query kernel."""
    from sunscreen_amd.batch import dot_queries_plan

    QT, RT = _tile()
    rows = (1 << 32) - 1
    got = dot_queries_plan(2 * QT + 1, rows, 4)
    assert got == _model(2 * QT + 1, rows, 4, QT, RT)
    if -(-rows // RT) > MAX_GRID_X // 2:
        assert got == [(0, QT, 0, rows, QT, RT), (QT, QT, 0, rows, QT, RT), (2 * QT, 1, 0, rows, 1, SINGLE_RT)]


def test_the_plan_entry_point_refuses_and_counts():
    from sunscreen_amd import _lib

    L = _lib.load()
    n = C.c_uint64(77)
    buf = (C.c_uint64 * 12)(*([0xABCD] * 12))
    assert _hr(L.hipbfv_debug_dot_queries_plan(3, 0, 4, buf, 2, C.byref(n))) == E_INVALIDARG  # no rows
    assert _hr(L.hipbfv_debug_dot_queries_plan(3, 5, 0, buf, 2, C.byref(n))) == E_INVALIDARG  # no residues
    assert _hr(L.hipbfv_debug_dot_queries_plan(1 << 32, 5, 4, buf, 2, C.byref(n))) == E_INVALIDARG
    assert _hr(L.hipbfv_debug_dot_queries_plan(3, 1 << 32, 4, buf, 2, C.byref(n))) == E_INVALIDARG
    assert n.value == 77 and list(buf) == [0xABCD] * 12
    assert _hr(L.hipbfv_debug_dot_queries_plan(3, 5, 4, buf, 2, None)) == E_POINTER
    assert _hr(L.hipbfv_debug_dot_queries_plan(3, 5, 4, None, 2, C.byref(n))) == E_POINTER
    assert L.hipbfv_debug_dot_queries_plan(0, 5, 4, None, 0, C.byref(n)) == 0 and n.value == 0
    # a capacity too small reports the count and writes nothing past it
    QT, RT = _tile()
    rows = (1 << 32) - 1
    want = _model(2 * QT + 1, rows, 4, QT, RT)
    if len(want) > 1:
        assert _hr(L.hipbfv_debug_dot_queries_plan(2 * QT + 1, rows, 4, buf, 1, C.byref(n))) == E_INVALIDARG and n.value == len(want)
        assert tuple(buf[:6]) == want[0] and list(buf[6:]) == [0xABCD] * 6
    assert _hr(L.hipbfv_debug_dot_queries_plan(3, 5, 4, None, 0, C.byref(n))) == E_INVALIDARG and n.value == 1
    assert list(buf[6:]) == [0xABCD] * 6


def test_the_tile_switch_names_an_instantiated_tile_or_changes_nothing(monkeypatch):
    """HIPBFV_DOT_QUERIES_TILE=<RT>x<QT> (the timing tool's switch) selects among the compiled tiles; anything else is the default."""
    from sunscreen_amd.batch import dot_queries_plan

    default = dot_queries_plan(5, 3, 4)
    for bad in ("", "7x9", "2", "x", "0x0"):
        monkeypatch.setenv("HIPBFV_DOT_QUERIES_TILE", bad)
        assert dot_queries_plan(5, 3, 4) == default, bad
    monkeypatch.setenv("HIPBFV_DOT_QUERIES_TILE", "1x4")
    assert dot_queries_plan(5, 3, 4) == [(0, 5, 0, 3, 4, 1)]
