"""Many queries against one pass over the database (hipbfv_batch_dot_plain_ntt_queries, dot_plain_q_kernel) on the GPU: operands
crafted at the accumulators' limits in the transform domain, the real transforms against the oracle, refusals that launch and write
nothing, and the three-call multi-client lookup (workloads.pir_lookup_queries)."""
import ctypes as C

import numpy as np
import pytest

from oracle import bfv_oracle as O
from tests import landing as LD
from tests.landing import landing

pytestmark = pytest.mark.gpu

E_INVALIDARG = 0x80070057
E_POINTER = 0x80004003
SENTINEL = 0x5A5A5A5A5A5A5A5A


@pytest.fixture(scope="module", autouse=True)
def _drop():
    yield
    LD.drop_landings()


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


def _device(L):
    from sunscreen_amd import Context
    from sunscreen_amd.batch import BatchEvaluator

    ctx = Context.from_raw(L.n, L.key_primes, L.t)
    assert ctx.K == L.K
    return ctx, BatchEvaluator(ctx)


def _same(got, want, what):
    assert got.shape == want.shape, (what, got.shape, want.shape)
    bad = np.argwhere(got != want)
    assert bad.size == 0, (what, "first difference at", bad[0].tolist(), int(got[tuple(bad[0])]), int(want[tuple(bad[0])]), len(bad))


def _tile(K):
    """(QT, RT) of the query-tiled kernel (host only)."""
    from sunscreen_amd.batch import dot_queries_plan

    (step,) = dot_queries_plan(2, 1, K)
    return step[4], step[5]


def _shapes(K):
    QT, RT = _tile(K)
    return [(1, 1, 1), (2, 2, 16), (3, 5, 17), (5, 3, 33), (QT + 1, RT + 1, 17), (2 * QT + 1, 1, 33), (QT, RT, 32)]


def _queries(ctn, count, crafted_last):
    """uint64[count][cols][2][K][n]: the case's ctn and count - 1 variants of it -- variant v is the columns rolled by v, its two
    polynomials exchanged when v is odd, so a wrong query, column or polynomial index cannot cancel.  The crafted one sits at index
    0, or (crafted_last) at index count - 1 with variant v at count - 1 - v."""
    qs = [ctn if v == 0 else (np.roll(ctn, v, axis=0)[:, ::-1] if v % 2 else np.roll(ctn, v, axis=0)) for v in range(count)]
    return np.ascontiguousarray(np.stack(qs[::-1] if crafted_last else qs))


def _reference(L, rows, cols, kind, count, crafted_last, q):
    """LD.dot_reference of query q of _queries(...): Python integers, then the oracle's inverse transform.  Built once per process."""

    def make():
        ctn, pntt, _ = LD.dot_case(L, rows, cols, kind)
        return LD.dot_reference(L.o, _queries(ctn, count, crafted_last)[q], pntt)

    v = count - 1 - q if crafted_last else q  # (the variant: the same words whichever way round the queries stand)
    return L.cached(("dot queries reference", rows, cols, kind, v), make)


@pytest.mark.parametrize("kind", ["max", "landed", "landed_zero_column"])
@pytest.mark.parametrize("pid", ["W2048", "W4096", "P1"])
def test_query_tiles_at_the_accumulators_limits(pid, kind):
    """Operands written directly in the transform domain.  60-bit primes with every word q - 1 (16, 17, 32 and 33 columns: one and
    two lazy reductions, the last pair and the odd last column), sums landed on 0, q - 1 and a pattern, zero columns; partial row
    blocks and partial query tiles, with the crafted query inside the full tile and inside the partial one.  Every query against the
    single-query call word for word; the first and the last against sums in Python integers and the oracle's inverse transform."""
    import torch
    from sunscreen_amd.batch import to_device, to_host

    L = landing(pid)
    ctx, ev = _device(L)
    for count, rows, cols in _shapes(L.K):
        if kind == "landed_zero_column" and cols < 3:
            continue
        ctn, pntt, T = LD.dot_case(L, rows, cols, kind)
        dp = to_device(pntt)
        for crafted_last in ((False,) if kind == "max" else (False, True)):
            qs = _queries(ctn, count, crafted_last)
            dq = to_device(qs)
            what = (pid, kind, count, rows, cols, crafted_last)
            out, seen = _profiled(ev, lambda: ev.dot_plain_ntt_queries(dq, dp))
            assert seen.get("plain") == 1 and set(seen) == {"plain", "ntt_inv"}, (what, seen)
            assert tuple(out.shape) == (count, rows, 2, L.K, L.n)
            for q in range(count):
                assert torch.equal(out[q], ev.dot_plain_ntt(dq[q], dp)), (what, "query", q)
            host = to_host(out)
            for q in sorted({0, count - 1}):
                _same(host[q], _reference(L, rows, cols, kind, count, crafted_last, q), what + ("query", q))
            if T is not None:
                # the crafted query's sums reach their targets: polynomial 0 of row r is T[r], polynomial 1 of row 0 is 0 where the
                # case could solve for it (LD.dot_case), in the transform domain
                crafted = host[count - 1 if crafted_last else 0]
                for r in range(rows):
                    for i in range(L.K):
                        assert (L.o.ntt(i, crafted[r, 0, i]) == T[r, i]).all(), (what, "row", r, "residue", i)
    ev.check()


def _oracle_rows(o, cts, plains):
    """[rows] of the reference's multiply_plain / add chain: sum_j multiply_plain(cts[j], plains[r][j])."""
    rows = []
    for r in range(plains.shape[0]):
        acc = o.multiply_plain(cts[0], plains[r, 0])
        for j in range(1, cts.shape[0]):
            acc = o.add(acc, o.multiply_plain(cts[j], plains[r, j]))
        rows.append(acc)
    return np.stack(rows)


def _real_case(L, count, rows, cols, salt):
    rng = L.rng(salt)
    cts = np.stack([L.fresh(rng, cols) for _ in range(count)])
    cts[count - 1, cols - 1] = (np.array(L.primes, dtype=np.uint64) - 1)[None, :, None]  # one extreme ciphertext: every word q - 1
    plains = np.stack([[L.o.batch_encode(rng.integers(0, L.t, L.n).astype(np.uint64)) for _ in range(cols)] for _ in range(rows)])
    return cts, plains


def _run_real(L, ev, cts, plains):
    from sunscreen_amd.batch import to_device

    count, cols = cts.shape[:2]
    dct = to_device(cts)
    ctn = ev.ct_to_ntt(dct.reshape((count * cols,) + tuple(dct.shape[2:]))).reshape(dct.shape)
    pntt = ev.plain_to_ntt(to_device(plains))
    out, seen = _profiled(ev, lambda: ev.dot_plain_ntt_queries(ctn, pntt))
    assert seen.get("plain") == 1 and set(seen) == {"plain", "ntt_inv"}, seen
    return ctn, pntt, out


def test_through_the_real_transforms_against_the_oracle_n4096():
    """n = 4096 default set, 3 queries x 2 rows x 3 columns, one ciphertext with every word q - 1: out[q][r] is the oracle's
    multiply_plain / add chain."""
    from sunscreen_amd.batch import to_host

    L = landing("P1")
    ctx, ev = _device(L)
    cts, plains = _real_case(L, 3, 2, 3, 71)
    _, _, out = _run_real(L, ev, cts, plains)
    host = to_host(out)
    for q in range(3):
        _same(host[q], _oracle_rows(L.o, cts[q], plains), ("n4096", "query", q))
    ev.check()


def test_through_the_real_transforms_n16384():
    """n = 16384 (K = 8), 5 queries x 5 rows x 3 columns: every query against the single-query call, one (query, row) against the
    oracle."""
    import torch
    from sunscreen_amd.batch import to_host

    L = landing("P4")
    ctx, ev = _device(L)
    cts, plains = _real_case(L, 5, 5, 3, 72)
    ctn, pntt, out = _run_real(L, ev, cts, plains)
    for q in range(5):
        assert torch.equal(out[q], ev.dot_plain_ntt(ctn[q], pntt)), q
    q, r = 4, 3  # (the query that holds the extreme ciphertext, inside the partial tile)
    _same(to_host(out[q, r]), _oracle_rows(L.o, cts[q], plains[r:r + 1])[0], ("n16384", q, r))
    ev.check()


def test_refusals_come_before_any_launch_or_write():
    import torch
    from sunscreen_amd import _lib
    from sunscreen_amd.batch import _ptr, _stream

    L = landing("P1")
    ctx, ev = _device(L)
    Lb = _lib.load()
    h = ev._h
    queries, rows, cols = 3, 2, 3
    ctw = 2 * L.K * L.n
    # one buffer: [ctn | pntt | out], so that overlapping ranges are plain pointer arithmetic
    n_ctn, n_pntt, n_out = queries * cols * ctw, rows * cols * L.K * L.n, queries * rows * ctw
    buf = torch.full((n_ctn + n_pntt + n_out,), SENTINEL, dtype=torch.int64, device="cuda")
    ctn, pntt, out = buf[:n_ctn], buf[n_ctn:n_ctn + n_pntt], buf[n_ctn + n_pntt:]
    word = 8
    calls = [
        ("NULL evaluator", lambda: Lb.hipbfv_batch_dot_plain_ntt_queries(None, _ptr(ctn), queries, cols, _ptr(pntt), rows, _ptr(out), _stream()), E_POINTER),
        ("NULL ctn", lambda: Lb.hipbfv_batch_dot_plain_ntt_queries(h, None, queries, cols, _ptr(pntt), rows, _ptr(out), _stream()), E_POINTER),
        ("NULL pntt", lambda: Lb.hipbfv_batch_dot_plain_ntt_queries(h, _ptr(ctn), queries, cols, None, rows, _ptr(out), _stream()), E_POINTER),
        ("NULL out", lambda: Lb.hipbfv_batch_dot_plain_ntt_queries(h, _ptr(ctn), queries, cols, _ptr(pntt), rows, None, _stream()), E_POINTER),
        ("cols = 0", lambda: Lb.hipbfv_batch_dot_plain_ntt_queries(h, _ptr(ctn), queries, 0, _ptr(pntt), rows, _ptr(out), _stream()), E_INVALIDARG),
        ("rows = 0", lambda: Lb.hipbfv_batch_dot_plain_ntt_queries(h, _ptr(ctn), queries, cols, _ptr(pntt), 0, _ptr(out), _stream()), E_INVALIDARG),
        ("queries beyond 2^32 - 1", lambda: Lb.hipbfv_batch_dot_plain_ntt_queries(h, _ptr(ctn), 1 << 32, cols, _ptr(pntt), rows, _ptr(out), _stream()), E_INVALIDARG),
        # the output range starts one word before the end of ctn / of pntt
        ("out overlaps ctn", lambda: Lb.hipbfv_batch_dot_plain_ntt_queries(h, _ptr(ctn), queries, cols, _ptr(pntt), rows, C.c_void_p(ctn.data_ptr() + (n_ctn - 1) * word), _stream()),
         E_INVALIDARG),
        ("out overlaps pntt", lambda: Lb.hipbfv_batch_dot_plain_ntt_queries(h, _ptr(ctn), queries, cols, _ptr(pntt), rows, C.c_void_p(pntt.data_ptr() + (n_pntt - 1) * word), _stream()),
         E_INVALIDARG),
        ("out is pntt", lambda: Lb.hipbfv_batch_dot_plain_ntt_queries(h, _ptr(ctn), queries, cols, _ptr(pntt), rows, _ptr(pntt), _stream()), E_INVALIDARG),
    ]
    ev.profile(True)
    ev.profile_reset()
    try:
        for what, call, want in calls:
            got = call() & 0xFFFFFFFF
            assert got == want, (what, hex(got), hex(want))
        # no queries: accepted, and nothing launched either
        assert Lb.hipbfv_batch_dot_plain_ntt_queries(h, _ptr(ctn), 0, cols, _ptr(pntt), rows, _ptr(out), _stream()) == 0
        torch.cuda.synchronize()
        assert ev.profile_read() == {}, ev.profile_read()
    finally:
        ev.profile(False)
    assert bool((buf == SENTINEL).all())
    ev.check()


@pytest.fixture(scope="module")
def lookup_case():
    """n = 4096, three clients with key pairs of their own, a 4 x 4 database of batch-encoded plaintexts, one-hot queries; the
    oracle's lazily relinearised lookups, computed once."""
    L = landing("P1")
    o, n, t = L.o, L.n, L.t
    rng = L.rng(4242)
    rows = cols = 4
    db_vals = rng.integers(0, t, (rows, cols, n)).astype(np.uint64)
    db = np.stack([[o.batch_encode(db_vals[r, c]) for c in range(cols)] for r in range(rows)])
    clients = []
    for c in range(3):
        O.seed(900 + c)
        sk, pk, rk, _ = o.keygen()
        clients.append((sk, pk, rk))
    one, zero = np.ones(n, dtype=np.uint64), np.zeros(n, dtype=np.uint64)

    def queries(pk, row, col):
        enc = lambda hot: o.encrypt(pk, o.batch_encode(one if hot else zero))  # noqa: E731
        return np.stack([enc(j == col) for j in range(cols)]), np.stack([enc(i == row) for i in range(rows)])

    def reference(c, colq, rowq):
        col = _oracle_rows(o, colq, db)
        acc = o.multiply(col[0], rowq[0])
        for i in range(1, rows):
            acc = o.add(acc, o.multiply(col[i], rowq[i]))
        return o.relinearize(acc, clients[c][2])

    picks = [(1, 2), (3, 0), (0, 3)]
    q = [queries(clients[c][1], *picks[c]) for c in range(3)]
    other = [(2, 1), (0, 0)]  # what clients 1 and 2 ask in the second run
    q2 = [q[0]] + [queries(clients[c][1], *other[c - 1]) for c in (1, 2)]
    return dict(L=L, db=db, db_vals=db_vals, clients=clients, picks=picks, q=q, q2=q2, refs=[reference(c, *q[c]) for c in range(3)])


def test_the_multi_client_lookup(lookup_case):
    """pir_lookup_queries: client c's answer has the bits of the oracle's relinearize(sum_i multiply(col_i, row_query_i)) under
    client c's key, decrypts under client c's secret key to the chosen entry, and does not change when the other clients' queries
    change."""
    import torch
    from sunscreen_amd import RelinearizationKeys
    from sunscreen_amd.batch import to_device, to_host
    from sunscreen_amd.workloads import pir_lookup_queries

    z = lookup_case
    L = z["L"]
    ctx, ev = _device(L)
    sets = [RelinearizationKeys.from_array(ctx, rk) for _, _, rk in z["clients"]]
    db_ntt = ev.plain_to_ntt(to_device(z["db"]))

    def run(q):
        colq = to_device(np.stack([c for c, _ in q]))
        rowq = to_device(np.stack([r for _, r in q]))
        return pir_lookup_queries(ev, colq, rowq, db_ntt, sets, [0, 1, 2])

    out = run(z["q"])
    assert tuple(out.shape) == (3, 2, L.K, L.n)
    host = to_host(out)
    for c in range(3):
        _same(host[c], z["refs"][c], ("client", c))
        row, col = z["picks"][c]
        assert (L.o.batch_decode(L.o.decrypt(host[c], z["clients"][c][0])) == z["db_vals"][row, col]).all(), c
    out2 = run(z["q2"])
    assert torch.equal(out2[0], out[0])
    assert not torch.equal(out2[1], out[1]) and not torch.equal(out2[2], out[2])
    ev.check()
