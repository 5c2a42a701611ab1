"""Program graphs of the reference's BFV examples used by BASELINE.json configs 4 and 5.

Each builder returns an `FheProgram` with the node structure the Sunscreen compiler emits for the
example (a Relinearize after every Multiply: sunscreen_backend/src/transforms/insert_relinearizations.rs:45-60).
"""
from __future__ import annotations

from .program import FheProgram


def _mul(p: FheProgram, a: int, b: int) -> int:
    return p.append_relinearize(p.append_multiply(a, b))


def chi_sq_optimized() -> FheProgram:
    """examples/chi_sq/src/main.rs:59-88 `chi_sq_optimized_impl`: 3 inputs -> (alpha, b1, b2, b3);
    6 mul+relin, 8 add, 1 sub."""
    p = FheProgram()
    n0, n1, n2 = (p.append_input_ciphertext(i) for i in range(3))
    x = p.append_add(p.append_add(n0, n0), n1)
    y = p.append_add(p.append_add(n2, n2), n1)
    n02 = _mul(p, n0, n2)
    n02 = p.append_add(n02, n02)
    n02 = p.append_add(n02, n02)
    n1sq = _mul(p, n1, n1)
    alpha = p.append_sub(n02, n1sq)
    alpha = _mul(p, alpha, alpha)
    b1 = _mul(p, x, x)
    b1 = p.append_add(b1, b1)
    b2 = _mul(p, x, y)
    b3 = _mul(p, y, y)
    b3 = p.append_add(b3, b3)
    for out in (alpha, b1, b2, b3):
        p.append_output_ciphertext(out)
    return p


def dot_product(lanes: int) -> FheProgram:
    """examples/dot_prod/src/main.rs:38-75: c = a*b; log2(lanes) rotate-and-add steps; + swap_rows."""
    p = FheProgram()
    a, b = p.append_input_ciphertext(0), p.append_input_ciphertext(1)
    c = _mul(p, a, b)
    shift = 1
    while shift < lanes:
        c = p.append_add(c, p.append_rotate_left(c, p.append_input_literal(shift)))
        shift *= 2
    c = p.append_add(c, p.append_swap_rows(c))
    p.append_output_ciphertext(c)
    return p


def pir_row(columns: int) -> FheProgram:
    """One row of examples/pir/src/main.rs:16-45: sum_j (col_query_j * db_j) where db_j are plaintext
    arguments, then multiplied by the row query.  Inputs: 0 = row query (ct), 1..columns = column
    queries (ct), columns+1..2*columns = database plaintexts."""
    p = FheProgram()
    row = p.append_input_ciphertext(0)
    acc = None
    for j in range(columns):
        cq = p.append_input_ciphertext(1 + j)
        db = p.append_input_plaintext(1 + columns + j)
        term = p.append_multiply_plaintext(cq, db)
        acc = term if acc is None else p.append_add(acc, term)
    p.append_output_ciphertext(_mul(p, acc, row))
    return p


def pir_lookup_graph(rows: int, columns: int) -> FheProgram:
    """The WHOLE `lookup` program of examples/pir/src/main.rs:16-45 for a rows x columns database, node for node as the
    compiler emits it: col[i] = db[i][0] * col_query[0]; col[i] = col[i] + db[i][j] * col_query[j]; sum = col[0] * row_query[0];
    sum = sum + col[i] * row_query[i] (a Relinearize after every Multiply).  Arguments, in the order of the fhe_program's
    signature: 0..columns-1 = col_query, columns..columns+rows-1 = row_query, then the database row-major
    (argument columns + rows + i * columns + j = database[i][j]).  One output."""
    p = FheProgram()
    cq = [p.append_input_ciphertext(j) for j in range(columns)]
    rq = [p.append_input_ciphertext(columns + i) for i in range(rows)]
    total = None
    for i in range(rows):
        col = None
        for j in range(columns):
            term = p.append_multiply_plaintext(cq[j], p.append_input_plaintext(columns + rows + i * columns + j))
            col = term if col is None else p.append_add(col, term)
        prod = _mul(p, col, rq[i])
        total = prod if total is None else p.append_add(total, prod)
    p.append_output_ciphertext(total)
    return p


def pir_lookup(ev, col_query, row_query, db_ntt, relin_keys):
    """examples/pir/src/main.rs:16-45 `lookup` for a sqrt(DB) x sqrt(DB) database, on the batch primitives instead of a
    node-by-node graph: col[i] = sum_j database[i][j] * col_query[j] as ONE transform-domain matrix-vector product
    (the column queries are transformed once, the pre-transformed database streams through once), then
    sum_i col[i] * row_query[i] as one batched multiply+relinearize and a pairwise reduction.

    col_query: int64[cols, 2, K, N], row_query: int64[rows, 2, K, N] (device), db_ntt: int64[rows, cols, K, N] from
    BatchEvaluator.plain_to_ntt.  Returns int64[1, 2, K, N].  Bit-identical to the reference's evaluation order
    except for the final summation order, which modular addition does not see."""
    col = ev.dot_plain_ntt(ev.ct_to_ntt(col_query), db_ntt)
    prod = ev.multiply_relin(col, row_query, relin_keys)
    while prod.shape[0] > 1:
        half = prod.shape[0] // 2
        head = ev.add(prod[:half].contiguous(), prod[half : 2 * half].contiguous())
        prod = head if prod.shape[0] == 2 * half else __import__("torch").cat([head, prod[2 * half :]])
    return prod


def pir_lookup_queries(ev, col_queries, row_queries, db_ntt, relin_key_sets, key_index):
    """`lookup` of examples/pir for Q clients against ONE database in three calls: ct_to_ntt of every column query,
    dot_plain_ntt_queries (the transformed database streams through once for all clients), multiply_sum_relin_keys with
    groups = Q and terms = rows (client c's sum is relinearised with relin_key_sets[key_index[c]]).

    col_queries: int64[Q, cols, 2, K, N], row_queries: int64[Q, rows, 2, K, N] (device), db_ntt: int64[rows, cols, K, N] from
    BatchEvaluator.plain_to_ntt, key_index: Q host integers.  Returns int64[Q, 2, K, N].

    The row side is the LAZILY relinearised sum: one key switch per client, with the bits of
    relinearize(sum_i multiply(col_i, row_query_i)).  It is not the reference's order, which relinearises after every row's multiply
    (pir_lookup, pir_lookup_graph); both decrypt to the same entry."""
    q, cols = col_queries.shape[0], col_queries.shape[1]
    ctn = ev.ct_to_ntt(col_queries.reshape((q * cols,) + tuple(col_queries.shape[2:]))).reshape(col_queries.shape)
    col = ev.dot_plain_ntt_queries(ctn, db_ntt)
    return ev.multiply_sum_relin_keys(col, row_queries, relin_key_sets, key_index)


def pir_lookup_sharded(ev, col_query, row_query_local, db_ntt_local, relin_keys, root: int = 0):
    """examples/pir with the database sharded by ROW over the ranks (SURVEY 8d config 5a, 8e "Exception"): this rank holds
    rows [lo, hi) of the transform-domain database and the matching slice of the row query; `pir_lookup` over them leaves one
    partial ciphertext per GPU, and `dist.reduce_ciphertexts` sums them on `root` (gather + add: the only data-path exchange
    in scope).  Returns int64[1, 2, K, N] on `root`, None elsewhere.  Modular addition is exact and order-free, so the answer
    has the bits of the unsharded lookup."""
    from . import dist as D

    return D.reduce_ciphertexts(pir_lookup(ev, col_query, row_query_local, db_ntt_local, relin_keys), ev.add, root)


def matrix_product_index(m: int, k: int, n: int):
    """The index tables of C = A B over prepared operands, A row-major m x k and B row-major k x n: item (i * n + j) * k + t multiplies
    A[i][t] = prepared ciphertext i * k + t of A by B[t][j] = prepared ciphertext t * n + j of B.  Returns (a_index, b_index), two lists
    of m * n * k integers: groups = m * n, terms = k in the sum forms."""
    if m <= 0 or k <= 0 or n <= 0:
        raise ValueError("matrix_product_index needs m, k, n >= 1")
    a_index = [i * k + t for i in range(m) for j in range(n) for t in range(k)]
    b_index = [t * n + j for i in range(m) for j in range(n) for t in range(k)]
    return a_index, b_index


def matrix_product(ev, ma, mb, m: int, k: int, n: int, relin_keys=None):
    """The ciphertext matrix product C[i][j] = sum_t A[i][t] * B[t][j] in one call: ma = ev.prepare of A's m * k ciphertexts (row-major),
    mb = ev.prepare of B's k * n.  Each distinct ciphertext was extended and transformed once when its object was made; the product
    runs no head and no forward transform (BatchEvaluator.multiply_sum_prepared).  Returns int64[m * n, 3, K, N], row-major, or
    int64[m * n, 2, K, N] with one key switch per entry when relin_keys is given.  The words of multiply, add and relinearize."""
    if ma.count != m * k or mb.count != k * n:
        raise ValueError(f"A holds {ma.count} ciphertexts for {m} x {k}, B {mb.count} for {k} x {n}")
    a_index, b_index = matrix_product_index(m, k, n)
    if relin_keys is None:
        return ev.multiply_sum_prepared(ma, a_index, mb, b_index, m * n, k)
    return ev.multiply_sum_relin_prepared(ma, a_index, mb, b_index, relin_keys, m * n, k)


def window_sum(ev, x, w: int, galois_keys):
    """The moving-window sum out[g] = sum over t < w of rotate_rows(x[g], t), one ciphertext per group, in one call: every term is
    finished and added inside the key switch's last kernel (BatchEvaluator.rotate_rows_sum with src_index[i] = i // w); x is not
    replicated.  galois_keys holds the keys of the steps 1 ... w - 1, or the power-of-two keys of their NAF chains.  Returns
    int64[groups, 2, K, N]: the words of rotate_rows and add."""
    if w <= 0:
        raise ValueError("window_sum needs a window of at least one slot")
    groups = x.shape[0]
    return ev.rotate_rows_sum(x, list(range(w)), galois_keys, groups=groups, src_index=[i // w for i in range(groups * w)])


def convolution_terms(taps):
    """(steps, weights) of a slot convolution with the integer taps taps[0 ... len - 1]: tap k is the step k with the weight taps[k], in
    tap order, and a zero tap is dropped (it would cost a key switch and contribute nothing).  Pure Python; all taps zero gives two
    empty lists."""
    steps, weights = [], []
    for k, tap in enumerate(taps):
        tap = int(tap)
        if tap:
            steps.append(k)
            weights.append(tap)
    return steps, weights


def convolve_slots(ev, x, taps, galois_keys):
    """The slot convolution out[g] slot j = sum over k of taps[k] * x[g] slot (j + k), within each of the two rows (rotate_rows wraps
    there), one ciphertext per group, in one call: BatchEvaluator.rotate_rows_sum_weighted over convolution_terms(taps) with
    src_index[i] = i // terms; x is not replicated, no plaintext is multiplied and a tap multiplies its term's noise by |tap|.
    galois_keys holds the keys of the non-zero taps' steps, or the power-of-two keys of their NAF chains.  Returns
    int64[groups, 2, K, N]: the words of rotate_rows, negate and add."""
    steps, weights = convolution_terms(taps)
    if not steps:
        raise ValueError("convolve_slots needs at least one non-zero tap")
    groups, terms = x.shape[0], len(steps)
    return ev.rotate_rows_sum_weighted(x, steps, weights, galois_keys, groups=groups, src_index=[i // terms for i in range(groups * terms)])
