"""The crafted operands of tests/landing.py land: for every builder and every parameter set tests/test_gpu_landing.py uses, the
ORACLE's result of the operation on the crafted operands equals the target on every crafted word -- all of them, none left out.  A
builder that did not land would leave the GPU comparison a test of random data; this is where that fails.  Also here: the oracle
raises "transparent" for the results landed on all zeros and does not for the almost transparent ones, and its decryption of the
landed phases is the integer algorithm of tests/test_oracle_decrypt_exact.py.  No GPU."""
import numpy as np
import pytest

from tests import landing as LD
from tests.landing import landing
from tests.test_oracle_decrypt_exact import _decrypt_over_the_integers


@pytest.fixture(scope="module", autouse=True)
def _drop():
    yield
    LD.drop_landings()


def test_pattern_gives_one_thread_different_targets():
    for n, primes in ((1024, [97, 193]), (32768, [(1 << 55) - 55, 12289, 40961])):
        pat = LD.pattern(primes, 2, n, 3)
        for p in range(2):
            for i, q in enumerate(primes):
                assert set(int(v) for v in pat[p, i]) == set(LD.targets(q))
                for t in (0, 1, n // 8 - 1):
                    assert len({int(pat[p, i, t + k * (n // 4)]) for k in range(4)}) == 4      # a tail thread's four coefficients
                    assert len({int(pat[p, i, t + k * (n // 8)]) for k in range(8)}) == 5      # a head thread's eight
            assert not (pat[p, 0] % primes[0] == pat[p, 1] % primes[0]).all() or primes[0] == primes[1]
        assert not (pat[0] == pat[1]).all()
    assert LD.targets(97) == [0, 96, 1, 48, 49]


@pytest.mark.parametrize("pid", ["P1", "P2", "P3", "P4", "P5", "P6"])
def test_relinearize_lands(pid):
    L = landing(pid)
    o, P, n = L.o, L.primes, L.n
    if pid == "P2":
        assert L.key_primes[-1] < max(L.key_primes[:-1])  # the special prime below a data prime
    (ct3, want, names), (tr, tr_want) = L.relin_items()
    assert len(ct3) == (4 if pid == "P6" else 5) and names[-1] == "almost transparent"
    for i, name in enumerate(names):
        assert (o.relinearize(ct3[i], L.rk) == want[i]).all(), name  # (does not raise: the almost transparent item included)
    by = dict(zip(names, want))
    assert (by["both polynomials on the pattern"] == LD.pattern(P, 2, n, 0)).all()
    assert (by["polynomial 0 all 0"][0] == 0).all()
    assert (by["polynomial 0 all q - 1"][0] == np.array(P, dtype=np.uint64)[:, None] - 1).all()
    almost = by["almost transparent"][1]
    assert almost[-1, -1] == 1 and almost.sum() == 1
    with pytest.raises(RuntimeError, match="transparent"):
        o.relinearize(tr[0], L.rk)
    o.throw_on_transparent = False
    try:
        got = o.relinearize(tr[0], L.rk)
    finally:
        o.throw_on_transparent = True
    assert (got == tr_want[0]).all() and (got[1] == 0).all()


@pytest.mark.parametrize("pid", ["P1", "P2", "P3", "P4", "P5"])
def test_rotations_land(pid):
    L = landing(pid)
    o, P, n = L.o, L.primes, L.n
    for name, elt, step in L.rotation_ops():
        ct, want, names = L.rotation_items(elt)
        gk = L.galois_keys([elt])
        for i, item in enumerate(names):
            if step is not None:
                got = o.rotate_rows(ct[i], step, gk)
            elif elt == 2 * n - 1:
                got = o.rotate_columns(ct[i], gk)
            else:
                got = o.apply_galois(ct[i], elt, gk)
            assert (got == want[i]).all(), (name, item)
        by = dict(zip(names, want))
        assert (by["polynomial 0 on the pattern"][0] == LD.pattern(P, 1, n, elt % 5)[0]).all(), name
        assert (by["polynomial 0 all 0"][0] == 0).all(), name
        assert (by["polynomial 0 all q - 1"][0] == np.array(P, dtype=np.uint64)[:, None] - 1).all(), name
        assert (by["c1 cycles 0, q - 1, 1"][0] == LD.pattern(P, 1, n, 4)[0]).all(), name
        edge = ct[names.index("c1 cycles 0, q - 1, 1")][1]
        assert all(set(int(v) for v in edge[i]) == {0, 1, q - 1} for i, q in enumerate(P))


@pytest.mark.parametrize("pid", ["P1", "P4", "P5"])
def test_addends_of_the_folded_sums_land(pid):
    L = landing(pid)
    o = L.o
    x, y, m, z, T = LD.fold_case(L)
    for g, (mult, sign) in enumerate(LD.FOLDS):
        for i in range(LD.DISTINCT):
            acc = m[i]
            for _ in range(mult - 1):
                acc = o.add(acc, m[i])
            got = o.add(acc, z[g][i]) if sign > 0 else o.sub(acc, z[g][i])
            assert (got == T[g][i]).all(), (mult, sign, i)
            if not (g == 0 and i == 3):
                assert (T[g][i] == LD.pattern(L.primes, 2, L.n, i + 2 * g)).all()
    assert (T[0][3][1] == LD.almost_zero(L.primes, L.n)).all()
    zt = LD.fold_transparent_addend(L, 2)
    with pytest.raises(RuntimeError, match="transparent"):
        o.add(m[2], zt)
    # the rotation sums
    x, gk, z_rot, z_swap, T_rot, T_swap, r = LD.rotsum_case(L)
    for i in range(LD.DISTINCT):
        assert (o.add(o.rotate_rows(x[i], LD.ROT_STEP, gk), z_rot[i]) == T_rot[i]).all(), i
        assert (o.add(o.rotate_columns(x[i], gk), z_swap[i]) == T_swap[i]).all(), i
        assert (T_swap[i] == LD.pattern(L.primes, 2, L.n, i + 3)).all()
    assert (T_rot[3][1] == LD.almost_zero(L.primes, L.n)).all() and (T_rot[0] == LD.pattern(L.primes, 2, L.n, 1)).all()
    with pytest.raises(RuntimeError, match="transparent"):
        o.add(r[1], LD.rotsum_transparent_addend(L, 1))


@pytest.mark.parametrize("pid", ["U1024", "P1", "W2048"])
def test_element_wise_plaintext_and_nary_operands_land(pid):
    L = landing(pid)
    o, P, n = L.o, L.primes, L.n
    if pid == "W2048":
        assert all(q.bit_length() == 60 for q in L.key_primes) and L.K == 3
    for size in (2, 3):
        x, ya, ys, T = LD.addsub_case(L, size)
        for i in range(len(x)):
            assert (o.add(x[i], ya[i]) == T[i]).all() and (o.sub(x[i], ys[i]) == T[i]).all(), (size, i)
            assert (T[i] == LD.pattern(P, size, n, i)).all()
    neg = LD.negate_case(L)
    for i in range(len(neg)):
        out = o.negate(neg[i])
        assert all(set(int(v) for v in out[p, k]) == {0, 1, q - 1} for p in range(2) for k, q in enumerate(P))
    for sub in (False, True):
        for shared in (False, True):
            ct, plain, T0 = LD.plain_case(L, sub, shared)
            assert set(LD.plain_edge_values(L.t)) <= set(int(v) for v in (plain if shared else plain[0]))
            for i in range(len(ct)):
                got = (o.sub_plain if sub else o.add_plain)(ct[i], plain if shared else plain[i])
                assert (got[0] == T0[i]).all() and (got[1] == ct[i][1]).all(), (sub, shared, i)
                assert (T0[i] == LD.pattern(P, 1, n, 2 * i + 1)[0]).all()
    mono = LD.mono_case(L)
    qm1 = np.array(P, dtype=np.uint64) - 1
    seen = set()
    for i in range(len(mono)):
        for pos in (0, 1, n - 2, n - 1):
            assert (mono[i, :, :, pos] == 0).all() or (mono[i, :, :, pos] == qm1[None, :]).all()
        seen.add(tuple(bool(mono[i, 0, 0, pos]) for pos in (0, n - 1)))
    assert len(seen) >= 3  # 0 and q - 1 on either side of the wrap, in several combinations
    assert len(LD.monomials(L)) == 12 and all(np.count_nonzero(p) == 1 for p in LD.monomials(L))
    ins, T = LD.nary_case(L)
    a, b, c, d, e = ins
    for i in range(len(a)):
        got = o.add(o.add(o.sub(o.add(o.negate(a[i]), b[i]), c[i]), d[i]), e[i])
        assert (got == T[i]).all() and (T[i] == LD.pattern(P, 2, n, i + 2)).all(), i


@pytest.mark.parametrize("pid", ["W2048", "W4096", "P1"])
def test_product_sums_land_in_the_transform_domain(pid):
    L = landing(pid)
    P, n = L.primes, L.n
    if pid != "P1":
        assert all(q.bit_length() == 60 and q < 1 << 60 for q in L.key_primes)
    for rows, cols, kind in LD.DOT_CASES:
        if kind != "max":
            ctn, pntt, T = LD.dot_case(L, rows, cols, kind)
            for i, q in enumerate(P):
                assert (ctn[:, :, i] < q).all() and (pntt[:, :, i] < q).all()  # canonical residues
            s = LD.dot_sums(P, ctn, pntt)
            assert (s[:, 0] == T).all(), (rows, cols, kind)  # polynomial 0 of every row, every word
            assert (T[0] == 0).all() and (s[0, 1] == 0).all(), (rows, cols, kind)  # row 0: both polynomials sum to 0
            if rows > 1:
                assert (T[1] == np.array(P, dtype=np.uint64)[:, None] - 1).all()
            if kind == "landed_zero_column" and cols >= 3:
                assert (ctn[cols // 2] == 0).all() and (pntt[:, cols // 2 - 1] == 0).all()
    # 16, 17, 32 and 33 products of (q - 1)^2 are what the lazy accumulators must hold: above 2^123 at 60-bit primes
    ctn, pntt, _ = LD.dot_case(L, 1, 33, "max")
    assert all((ctn[:, :, i] == q - 1).all() and (pntt[:, :, i] == q - 1).all() for i, q in enumerate(P))
    if pid != "P1":
        assert (33 * (P[0] - 1) ** 2).bit_length() in (125, 126)
    s = LD.dot_sums(P, ctn, pntt)
    assert all((s[0, :, i] == 33 % q).all() for i, q in enumerate(P))  # 33 (q - 1)^2 = 33 mod q


T_CASES = [("P1", 2), ("P1", 500), ("P1", None), ("P1", (1 << 60) - 1), ("P4", None)]


@pytest.mark.parametrize("pid,t", T_CASES, ids=[f"{p}-t{t or 'batching'}" for p, t in T_CASES])
def test_phases_land_and_decrypt_by_the_integer_algorithm(pid, t):
    L = landing(pid, t)
    o, Q = L.o, L.Q
    vals = L.phase_values()
    assert len(vals) == 17 and {0, 1, Q - 1, Q // 2, Q // 2 + 1} <= set(vals)
    for k in (0, 1, L.t // 2, L.t - 1):  # the three integers around the point where round(t x / Q) steps from k to k + 1
        b = [x for x in range(((2 * k + 1) * Q) // (2 * L.t) - 1, ((2 * k + 1) * Q) // (2 * L.t) + 3) if 2 * L.t * x >= (2 * k + 1) * Q][0]
        assert {(b - 1) % Q, b % Q, (b + 1) % Q} <= set(vals), k
    ct, phases = L.phase_items(2 if pid == "P4" else 4)
    for i in range(len(ct)):
        d = o.dot_with_secret(ct[i], L.sk)
        for j, q in enumerate(L.primes):
            assert (d[j] == np.array([x % q for x in phases[i]], dtype=np.uint64)).all(), (i, j)
        want, _ = _decrypt_over_the_integers(o, phases[i])
        assert (o.decrypt(ct[i], L.sk) == want).all(), i
        assert set(phases[i]) == set(vals)


# ---- F: the multiply head ----------------------------------------------------------------------------------------------------
def _head_model(P, x):
    """(y: K object rows, r: object[n], v: object[n]) of one polynomial from the primes alone: y_i = x_i 2^32 (q / q_i)^-1 mod q_i,
    v = sum y_i (q / q_i) over the integers, r = -v / q mod 2^32."""
    Q = LD._product(P)
    y = [LD._obj(x[i]) * ((1 << 32) * pow(Q // q, -1, q)) % q for i, q in enumerate(P)]
    v = sum(y[i] * (Q // q) for i, q in enumerate(P))
    return y, (-v * pow(Q, -1, 1 << 32)) % (1 << 32), v


def test_thread_cycle_gives_one_thread_consecutive_places():
    for n in (1024, 4096, 8192, 16384):
        for t in (0, 1, n // 8 - 1):
            assert len({int(LD.r_targets(n, 3)[t + k * (n // 8)]) for k in range(8)}) == 6   # a head thread's eight see all six (four asked for)
        assert set(int(v) for v in LD.r_targets(n)) == set(LD.R_TARGETS)
        idx = LD.thread_cycle(n, 4, 3, 1)
        for t in (0, 5, n // 4 - 1):
            assert {int(idx[t + k * (n // 4)]) for k in range(4)} == {0, 1, 2}               # a tail thread's four: all three
    assert LD.R_TARGETS == [0, 1, 2**31 - 1, 2**31, 2**31 + 1, 2**32 - 1]


HEAD_SETS = ["P1", "P3", "P4", "P5", "W2048", "U1024"]


@pytest.mark.parametrize("pid", HEAD_SETS)
def test_multiply_head_operands_land(pid):
    """Every coefficient of every crafted polynomial carries the intended r_mtilde and y_i (from the primes alone), and the oracle's
    behz_extend of it is the integer (sum y_i (q / q_i) + q centred(r)) / 2^32 mod every Bsk prime, r = 2^31 centred as -2^31."""
    L = landing(pid)
    o, P, n, Q = L.o, L.primes, L.n, L.Q
    free = next(i for i, q in enumerate(P) if q > 1 << 32)
    if pid == "U1024":
        assert [q.bit_length() for q in P] == [50, 30, 30, 50] and free == 0  # 30-bit rows below m~ beside 50-bit ones
    a, b = LD.mtilde_case(L)
    assert a.shape == b.shape == (4, 2, L.K, n)
    qm1 = np.array(P, dtype=object)[:, None] - 1
    seen_r = set()
    for i in range(4):
        for side, ops in enumerate((a, b)):
            kind = LD.MTILDE_KINDS[i][side]
            for p in range(2):
                x = ops[i, p]
                assert all((x[k] < q).all() for k, q in enumerate(P))  # canonical residues
                y, r, v = _head_model(P, x)
                shift = 5 * i + p + 3 * side
                if kind == "max":
                    assert all((y[k][1::2] == q - 1).all() and (y[k][0::2] == 0).all() for k, q in enumerate(P))
                    print(pid, "max operand: r_mtilde on the odd coefficients", hex(int(r[1])), "on the even ones", hex(int(r[0])))
                else:
                    assert (r == LD._obj(LD.r_targets(n, shift))).all(), (i, side, p)
                    seen_r |= set(int(v) for v in r)
                    assert (y[free] < 1 << 32).all()
                if kind == "edge":
                    pat = LD.pattern(P, 1, n, shift)[0]
                    assert all((y[k] == LD._obj(pat[k])).all() for k in range(L.K) if k != free), (i, side, p)
                    assert all(set(int(w) for w in y[k]) == set(LD.targets(q)) for k, q in enumerate(P) if k != free)
                if (i, p) in ((0, 0), (2, 0), (3, 1)):  # the integer model of the extension (all kinds, both sides)
                    rc = np.where(r >= 1 << 31, r - (1 << 32), r)
                    num = v + Q * rc
                    assert (num % (1 << 32) == 0).all()
                    ext = o.behz_extend(x)
                    for j, m in enumerate(o.bsk):
                        assert (LD._obj(ext[j]) == (num >> 32) % m).all(), (i, side, p, j)
    assert seen_r == set(LD.R_TARGETS)
    if pid == "P1":
        a3, b2 = LD.mtilde_case(L, 3, 2, 2)
        assert a3.shape[1] == 3 and (_head_model(P, a3[0, 2])[1] == LD._obj(LD.r_targets(n, 2))).all()


def test_the_turned_centring_differs_on_the_crafted_operands_only():
    """The integer multiply of tests/test_oracle_behz_exact.py with `>` for `>=` at r = 2^31: other words on the crafted operands
    (which the oracle does not follow), the same words on that file's random and extreme operands -- those never put 2^31 there."""
    from tests.test_oracle_behz_exact import behz_multiply_over_the_integers, random_and_extreme_operands

    L = landing("P1")
    a, b = LD.mtilde_case(L)
    right = behz_multiply_over_the_integers(a[0], b[0], L.primes, L.t)
    wrong = behz_multiply_over_the_integers(a[0], b[0], L.primes, L.t, turned=True)
    assert (L.o.multiply(a[0], b[0]) == right).all()
    differ = (right != wrong).any(axis=(0, 1))
    print("turned centring: coefficients that differ on the crafted operands:", int(differ.sum()), "of", L.n)
    assert differ.sum() > L.n // 6  # (r = 2^31 sits in every sixth coefficient of each factor; the product spreads it)
    for x, y in random_and_extreme_operands(np.random.default_rng(L.n + 17), L.primes, L.n, 2, 2)[:3]:
        assert (behz_multiply_over_the_integers(x, y, L.primes, L.t, turned=True) == behz_multiply_over_the_integers(x, y, L.primes, L.t)).all()


# ---- G: the floor's inputs and the multiply's outputs ------------------------------------------------------------------------
FLOOR_SETS = ["P1", "P3", "P4", "P5", "W2048"]


@pytest.mark.parametrize("pid", FLOOR_SETS)
def test_floor_inputs_and_harvested_outputs_land(pid):
    L = landing(pid)
    o, P, n, Q, t = L.o, L.primes, L.n, L.Q, L.t
    a, y = LD.floor_case(L)
    for i in range(2):
        for p in range(2):  # what the floor of polynomial 0 (2) of a (1, 1) reads, from the primes alone
            got = [LD._obj(a[i, p, k]) * (t * pow(Q // q, -1, q)) % q for k, q in enumerate(P)]
            assert all((got[k] == LD._obj(y[i, p, k])).all() for k in range(L.K)), (i, p)
    assert all(set(int(v) for v in y[0, p, k]) == set(LD.targets(q)) for p in range(2) for k, q in enumerate(P))
    assert not (y[0, 0] == y[0, 1]).all()  # different phases
    assert all((y[1, 0, k, 1::2] == q - 1).all() and (y[1, 0, k, 0::2] == 0).all() for k, q in enumerate(P))
    ones = LD.ones_ct(L, 1)[0]
    prod = o.multiply(a[0], ones)  # (1, 1) is what the builder says: d0 = a0 and d2 = a1 pass the same floor
    assert (prod[0] == o.multiply(np.stack([a[0, 0], a[0, 0]]), ones)[2]).all()
    # the harvested outputs
    ao, kinds, kept, stats = LD.output_case(L)
    print(pid, "harvest {family: [candidates, on 0, on -1, on +1]}:", stats, "kept", {v: len(c) for v, c in kept.items()})
    for v in (0, -1):
        assert len(set(kept[v])) >= 4, (v, kept[v])
    assert stats["small"][1] == 0 and stats["small"][3] == 0  # a small D has floor 0 or -1 and u' >= 1: never 0, never +1
    used = sorted(set(int(v) for v in kinds.ravel()))
    assert used[:2] == [-1, 0] and all(len(set(kept[v])) >= 4 for v in used)
    for i in range(2):
        out = o.multiply(ao[i], ones)
        for p, poly in ((0, 0), (1, 2)):
            assert (out[poly] == LD.kinds_to_words(P, kinds[i, p])).all(), (i, poly)  # every row of every coefficient
            for th in (0, 1, n // 4 - 1):  # a tail thread's four coefficients see every target in use
                assert {int(kinds[i, p, th + k * (n // 4)]) for k in range(4)} == set(used), (i, p, th)
    # the sums: per coefficient the three term outputs are 0, -1, -1 in some order
    if pid in ("P3", "P4"):
        asum, ksum = LD.output_sum_case(L)
        assert (ksum.sum(axis=1) == -2).all() and sorted(set(int(v) for v in ksum.ravel())) == [-1, 0]
        total = None
        for j in range(asum.shape[1]):
            term = o.multiply(asum[0, j], ones)
            assert (term[0] == LD.kinds_to_words(P, ksum[0, j, 0])).all() and (term[2] == LD.kinds_to_words(P, ksum[0, j, 1])).all()
            total = term if total is None else o.add(total, term)
        qm2 = np.array(P, dtype=np.uint64)[:, None] - 2
        assert (total[0] == qm2).all() and (total[2] == qm2).all()


# ---- H: decrypt's gamma correction -------------------------------------------------------------------------------------------
GAMMA_CASES = [(p, t) for p in ("P1", "P2", "P3", "W4096") for t in (None, 500, (1 << 60) - 1)]


@pytest.mark.parametrize("pid,t", GAMMA_CASES, ids=[f"{p}-t{t or 'batching'}" for p, t in GAMMA_CASES])
def test_gamma_residues_land_and_only_the_turned_branch_differs(pid, t):
    L = landing(pid, t)
    o, P, n, Q, gamma = L.o, L.primes, L.n, L.Q, int(L.o.gamma)
    if t == (1 << 60) - 1:
        assert t > max(P)  # t above every data prime
    G = LD.gamma_targets(gamma)
    assert gamma % 2 == 1 and G[3] == gamma >> 1 and len(set(G)) == 6
    sizes = (2, 3) if (pid, t) == ("P1", None) else (2,)
    for size in sizes:
        ct, phases, targets = LD.gamma_case(L, 2, size)
        assert ct.shape == (2, size, L.K, n)
        for i in range(2):
            assert set(targets[i]) == set(G)
            d = o.dot_with_secret(ct[i], L.sk)
            g = 0
            for k, q in enumerate(P):  # from the primes, t and gamma alone
                assert (d[k] == np.array([x % q for x in phases[i]], dtype=np.uint64)).all(), (i, k)
                g = g + (LD._obj(d[k]) * (L.t * gamma * pow(Q // q, -1, q)) % q) * ((Q // q) % gamma)
            g = g * (-pow(Q, -1, gamma)) % gamma
            assert (g == np.array(targets[i], dtype=object)).all(), i  # 100 % of the coefficients
            want, slack = _decrypt_over_the_integers(o, phases[i])
            assert [s % gamma for s in slack] == targets[i]
            assert (o.decrypt(ct[i], L.sk) == want).all(), i
            turned, _ = _decrypt_over_the_integers(o, phases[i], turned=True)
            assert ((turned != want) == (np.array(targets[i], dtype=object) == gamma >> 1)).all(), i


# ---- I: prepared multiplicands and weighted sums (tests/test_gpu_landing_shared.py) ------------------------------------------
SHARED_SETS = ["P1", "P3", "P4", "P5", "W4096", "W2048", "U1024"]


@pytest.mark.parametrize("pid", SHARED_SETS)
def test_the_oracle_multiply_is_symmetric_on_the_crafted_operands(pid):
    """BFV's tensor is symmetric: multiply(b, a) has the words of multiply(a, b).  One product of the oracle then serves the crafted
    operand in the prepared role and in the role of `a`; shown here per set, on a crafted head pair and on a floor operand by (1, 1),
    before tests/test_gpu_landing_shared.py relies on it."""
    L = landing(pid)
    o = L.o
    a, b = LD.mtilde_case(L)
    for i in (1, 3):  # edge times random, edge times all-rows-at-q-1
        assert (o.multiply(b[i], a[i]) == o.multiply(a[i], b[i])).all(), (pid, "head", i)
    if pid != "U1024":
        fo, ones = LD.floor_operands(L), LD.ones_ct(L, 1)[0]
        for i in (0, 3):
            assert (o.multiply(ones, fo[i]) == o.multiply(fo[i], ones)).all(), (pid, "floor", i)


def test_with_decoy_never_gives_the_identity():
    L = landing("P1")
    for m in (1, 4, 6):
        ops = [np.full((2, L.K, L.n), 10 + i, dtype=np.uint64) for i in range(m)]
        prepared, index = LD.with_decoy(L, ops)
        assert len(prepared) == m + 1 and 1 not in index and sorted(index + [1]) == list(range(m + 1))
        assert all((prepared[p] == ops[i]).all() for i, p in enumerate(index))
        assert m == 1 or (index != list(range(m)) and len({index[i + 1] - index[i] for i in range(m - 1)}) > 1)
        assert not any((prepared[1] == x).all() for x in ops)
    assert LD.with_decoy(L, [ops[0]])[1] == [0]  # the broadcast index beside the decoy


def test_the_nine_items_use_every_prepared_ciphertext_through_a_map_that_is_not_the_identity():
    L = landing("P4")
    a, prepared, index, refs = LD.nine_case(L)
    assert a.shape[0] == 9 and prepared.shape[0] == 10 and len(index) == 9
    assert sorted(index) == list(range(1, 10)) and 0 not in index                    # all nine, never the decoy
    assert all(index[i] != i for i in range(9)) and len({index[i + 1] - index[i] for i in range(8)}) > 2
    assert (9 + 7) >> 3 == 2 and (10 + 7) >> 3 == 2                                  # per = 2 in the product and in prepare
    assert sorted(refs) == sorted([("head", k) for k in range(4)] + [("floor", 1)] + [("floor", k) for k in range(4)])
    ma, mb = LD.mtilde_case(L)
    fo, ones = LD.floor_operands(L), LD.ones_ct(L, 1)[0]
    for i, (family, k) in enumerate(refs):  # item i and its prepared ciphertext ARE the pair of product k, in either order
        x, y = (ma[k], mb[k]) if family == "head" else (fo[k], ones)
        got = (a[i], prepared[index[i]])
        assert all((g == w).all() for g, w in zip(got, (x, y))) or all((g == w).all() for g, w in zip(got, (y, x))), i
    assert not any((prepared[0] == p).all() for p in prepared[1:])


WEIGHTED_SETS = ["P3", "P4", "P5", "W4096", "W2048", "U1024", "S4096"]


@pytest.mark.parametrize("pid", WEIGHTED_SETS)
def test_weighted_sums_land_and_meet_every_event_in_every_row(pid):
    """weighted_sum_case: the sums in Python integers are the oracle's negate / add chains where the weights are small, polynomials
    0 and 2 follow from the kinds and the weights alone (asserted inside the builder), and the weight vectors together put a raw
    sum of exactly q_i, one of q_i - 1, a final 0, q_i - 1 and 1 in front of every residue row; the modulus-sized weights add a
    weighted residue of 0 from a nonzero product in the row of q_1 alone."""
    L = landing(pid)
    o, P, n = L.o, L.primes, L.n
    if pid == "S4096":
        assert [q.bit_length() for q in P] == [30, 30, 40] and n == 4096
    prods = LD.output_sum_products(L)
    a, kinds = LD.output_sum_case(L)
    groups, terms = a.shape[:2]
    slots = groups * 2 * n
    vectors = list(LD.WEIGHT_VECTORS) + (LD.modulus_weights(L) if pid in ("U1024", "S4096") else [])
    total = {e: np.zeros(L.K, dtype=np.int64) for e in LD.SUM_EVENTS}
    for w in vectors:
        ops, want, events = LD.weighted_sum_case(L, w)
        assert ops is a and want.shape == (groups, 3, L.K, n)
        print(pid, w, {e: [int(v) for v in c] for e, c in events.items()})
        for e in LD.SUM_EVENTS:
            total[e] += events[e]
        if max(abs(x) for x in w) <= 3:  # the definition, pinned to the oracle: |w| additions of the (negated) product
            for g in range(groups):
                acc = None
                for j, x in enumerate(w):
                    base = o.negate(prods[g, j]) if x < 0 else prods[g, j]
                    for _ in range(abs(x)):
                        acc = base if acc is None else o.add(acc, base)
                assert (acc == want[g]).all(), (pid, w, g)
        if w == (1, -1, 1):  # two of the three orders of (0, -1, -1) pass through exactly q and end on 0
            assert all(2 * slots // 3 <= c <= 2 * slots // 3 + 2 for c in events["raw q"]) and (events["final 0"] == events["raw q"]).all()
            if pid == "P3":
                assert slots == 32768 and set(events["raw q"]) == {21845} and set(events["raw q - 1"]) == {32769}
        if w == (3, -2, -1) and pid == "P3":
            assert set(events["final q - 1"]) == {10923} and set(events["raw q - 1"]) == {21846}
    for e in LD.SUM_EVENTS[:5]:
        assert (total[e] > 0).all(), (pid, e, total[e])
    if pid in ("U1024", "S4096"):
        row = P.index(LD.modulus_weights(L)[0][0])
        assert total["zero weight"][row] > 0 and all(total["zero weight"][i] == 0 for i in range(L.K) if i != row), total["zero weight"]
        assert all(abs(x) > P[row] for x in LD.modulus_weights(L)[1][1:])  # above the modulus: (w mod q_1) is not w
    else:
        assert (total["zero weight"] == 0).all()
    # the unweighted sums of tests/test_gpu_landing_multiply.py are the all-ones case of the same builder: q - 2 everywhere
    if pid in ("P3", "P4"):
        qm2 = np.array(P, dtype=np.uint64)[:, None] - 2
        ones_sum = LD.weighted_sum_case(L, (1, 1, 1))[1]
        assert (ones_sum[:, 0] == qm2).all() and (ones_sum[:, 2] == qm2).all()


# ---- J: sums of rotations (tests/test_gpu_landing_rotate_sum.py) -------------------------------------------------------------
ROTATION_SUM_SETS = ["P1", "P2", "P3", "P4", "P5", "S4096", "U1024", "W2048", "X8192"]
CPU_GROUPS = 2


def _oracle_scaled(o, ct, w):
    """LD.scale_words of one rotated term; for 0 < |w| <= 3 also the oracle's own negate / add chain."""
    out = LD.scale_words(o.primes, ct, w)
    if 0 < abs(w) <= 3:
        one = o.negate(ct) if w < 0 else ct
        acc = one
        for _ in range(abs(w) - 1):
            acc = o.add(acc, one)
        assert (np.asarray(acc) == out).all(), w
    return out


def _oracle_sum(L, sources, steps, weights, gk, galois, g):
    """The oracle's rotate, scale and add chain of group g (the exception for a transparent sum switched off)."""
    o = L.o
    acc = None
    for t, s in enumerate(steps):
        term = _oracle_scaled(o, LD._rotate(o, sources[g * len(steps) + t], s, gk, galois), weights[t])
        acc = term if acc is None else o.add(acc, term)
    return acc


@pytest.mark.parametrize("pid", ROTATION_SUM_SETS)
def test_sums_of_rotations_land_and_meet_every_event_in_every_row(pid):
    """Every step and weight vector of the set in every mode: the oracle's rotations of the crafted sources, scaled and added, are
    `expected` on every word, the landed words are where the mode says, and the vectors together put every event of
    LD.ROTATION_SUM_EVENTS in front of every residue row."""
    L = landing(pid)
    o, P, n, K = L.o, L.primes, L.n, L.K
    if pid == "X8192":
        assert n == 8192 and [q.bit_length() for q in L.key_primes] == [50, 30, 30, 50, 50] and K == 4
    qm1 = np.array(P, dtype=np.uint64)[:, None] - 1
    total = {e: np.zeros(K, dtype=np.int64) for e in LD.ROTATION_SUM_EVENTS}
    o.throw_on_transparent = False
    try:
        for k, (name, steps, weights, galois, pow2) in enumerate(LD.rotation_sum_runs(L)):
            gk = LD.rotation_sum_keys(L, steps, galois, pow2)
            terms = len(steps)
            wts = weights or (1,) * terms
            ident = [LD._element(o, s, galois) == 1 for s in steps]
            for mode in LD.rotation_sum_modes(k):
                src, want, events = LD.rotation_sum_case(L, steps, weights, mode, CPU_GROUPS, galois, pow2)
                assert src.shape == (CPU_GROUPS * terms, 2, K, n) and want.shape == (CPU_GROUPS, 2, K, n)
                assert all((src[:, :, i] < q).all() for i, q in enumerate(P))  # canonical residues
                print(pid, name, mode, {e: [int(v) for v in c] for e, c in events.items()})
                for e in LD.ROTATION_SUM_EVENTS:
                    total[e] += events[e]
                for g in range(CPU_GROUPS):
                    assert (_oracle_sum(L, src, steps, wts, gk, galois, g) == want[g]).all(), (pid, name, mode, g)
                    last = terms - 1
                    free = np.array([wts[last] % q != 0 for q in P])  # rows whose last weight has an inverse
                    if mode == "terms":
                        for t, s in enumerate(steps):
                            r = LD._rotate(o, src[g * terms + t], s, gk, galois)
                            pat = LD.pattern(P, 2, n, t + g)
                            assert (r[0] == pat[0]).all() and (not ident[t] or (r[1] == pat[1]).all()), (pid, name, t, g)
                    elif mode == "partial" or (mode in ("transparent", "almost") and g != LD.TRANSPARENT_GROUP):
                        pat = LD.pattern(P, 2, n, last + g)
                        assert (want[g, 0][free] == pat[0][free]).all() and (not ident[last] or (want[g, 1][free] == pat[1][free]).all())
                    elif mode == "ladder":
                        end = qm1 if last % 2 == 0 else np.zeros_like(qm1)
                        assert (want[g, 0][free] == np.broadcast_to(end, (K, n))[free]).all(), (pid, name, g)
                    elif mode == "transparent":
                        assert not want[g, 1].any() and want[g, 0].any()
                    elif mode == "almost":
                        assert (want[g, 1] == LD.almost_zero(P, n)).all()
                    elif mode == "gathers":
                        t0 = ident.index(False)
                        assert all(set(int(v) for v in src[g * terms + t0, p, i]) == {0, 1, q - 1} for p in range(2) for i, q in enumerate(P))
                if mode == "ladder" and all(w % q for w in wts for q in P):  # every word: raw sums q - 1, q, q - 1, q
                    words = CPU_GROUPS * n
                    polys1 = [sum(1 for t in range(terms) if ident[t] and t <= u) > 0 for u in range(terms)]
                    assert all(c >= words * (terms // 2) for c in events["raw q"]) and all(c >= words * ((terms + 1) // 2) for c in events["raw q - 1"]), (events, polys1)
                if weights is not None and len(weights) == 4 and weights[1] in P and mode == "partial":  # the modulus-sized weight
                    row = P.index(weights[1])
                    assert events["zero weight"][row] > 0 and all(events["zero weight"][i] == 0 for i in range(K) if i != row), events["zero weight"]
    finally:
        o.throw_on_transparent = True
    print(pid, "events over all vectors and modes:", {e: [int(v) for v in c] for e, c in total.items()})
    zero_rows = np.array([any(w % q == 0 for r in LD.rotation_sum_runs(L) for w in (r[2] or ())) for q in P])
    for e in LD.ROTATION_SUM_EVENTS:
        assert ((total[e] > 0) == (zero_rows if e == "zero weight" else True)).all(), (pid, e, total[e])
    # the oracle reports the landed sum transparent, and the almost transparent one not
    name, steps, weights, galois, pow2 = LD.rotation_sum_runs(L)[0]
    gk = LD.rotation_sum_keys(L, steps, galois, pow2)
    src, want, _ = LD.rotation_sum_case(L, steps, weights, "transparent", CPU_GROUPS, galois, pow2)
    with pytest.raises(RuntimeError, match="transparent"):
        _oracle_sum(L, src, steps, (1,) * len(steps), gk, galois, LD.TRANSPARENT_GROUP)
    src, want, _ = LD.rotation_sum_case(L, steps, weights, "almost", CPU_GROUPS, galois, pow2)
    assert (_oracle_sum(L, src, steps, (1,) * len(steps), gk, galois, LD.TRANSPARENT_GROUP) == want[LD.TRANSPARENT_GROUP]).all()


@pytest.mark.parametrize("pid", ["P1", "S4096", "X8192"])
def test_the_turned_folds_differ_on_the_crafted_sums_only(pid):
    """LD.fold_terms with one comparison turned gives other words than the reference on the crafted sums and the same words on a
    random control of the same shape.  "add": `> q` for `>= q` -- every raw sum of exactly q_i that is the last one, or is followed by
    a weighted 0, stays q_i.  "product": the weighted residue without the Shoup product's last correction, left in [0, 2 q_i); the
    add's one subtraction repairs it unless the sum wraps as well, which the partial sums put in front of one thread in five at the
    last term (the sum on q_i - 1, the weighted residue 2) and the ladder in front of every one.  The quotient estimate is one short
    where the true residue is below about r q_i / 2^64, so a residue of 1 or 2 shows it at primes above 2^33 under a negative weight
    (w mod q_i and r both of the size of q_i; with weight 1 the estimate is exact); on random words it shows with probability q_i / 2^64.  It is judged at S4096 (a 40-bit row:
    shown on the crafted sums, 2^-24 per random word); at 50-bit primes the random control would meet it as well."""
    L = landing(pid)
    o, P = L.o, L.primes
    for k in (0, 1):
        name, steps, weights, galois, pow2 = LD.rotation_sum_runs(L)[k]
        gk = LD.rotation_sum_keys(L, steps, galois, pow2)
        wts = weights or (1,) * len(steps)
        turns = ("add", "product") if k == 1 and pid == "S4096" else ("add",)
        for mode in ("partial", "ladder", "random"):
            src, want, events = LD.rotation_sum_case(L, steps, weights, mode, CPU_GROUPS, galois, pow2)
            differ = dict.fromkeys(turns, 0)
            for g in range(CPU_GROUPS):
                vals = [LD._rotate(o, src[g * len(steps) + t], s, gk, galois) for t, s in enumerate(steps)]
                assert (LD.fold_terms(P, vals, wts) == want[g]).all()
                for turn in turns:
                    differ[turn] += int((LD.fold_terms(P, vals, wts, turned=turn) != want[g]).sum())
            print(pid, name, mode, "words where the turned fold differs:", differ, "raw sums of exactly q:", [int(v) for v in events["raw q"]])
            if mode == "random":
                assert not any(differ.values()) and not events["raw q"].any()
            else:
                assert all(d >= CPU_GROUPS * L.n // 5 for d in differ.values()) and (events["raw q"] > 0).all()


def test_chain_terms_land_under_the_power_of_two_keys():
    """land_rotation through the oracle's NAF chains over the holding "P" of tests/test_gpu_rotation_steps.py (same parameters): 11 and
    -13 (three hops, mixed signs), 2045 and 1707 (the skipped part of n / 2), and a step with a key of its own."""
    from tests.bfv_helpers import params

    L = landing("P1")
    o, P, n = L.o, L.primes, L.n
    pn, pprimes, pt = params("default_4096_16")
    assert (pn, [int(p) for p in pprimes], int(pt)) == (n, L.key_primes, L.t)
    gk = LD.rotation_sum_keys(L, LD.STEPS_CHAIN, pow2=True)
    assert len(gk) == 2 * 11 + 1 - 1  # (the steps 1024 and -1024 share their element)
    rng = L.rng(300)
    for k, step in enumerate((11, -13, 2045, 1707, 1, -1024)):
        assert (o.galois_elt_from_step(step) in gk) == (step in (1, -1024))
        T0 = LD.pattern(P, 1, n, k)[0]
        ct, want = LD.land_rotation(o, gk, step, LD.random_residues(rng, P, (), n), T0)
        got = o.rotate_rows(ct, step, gk)
        assert (got == want).all() and (got[0] == T0).all(), step
    # the Galois-element form of the same builder is land_galois
    elt = 2 * n - 5
    c1 = LD.random_residues(rng, P, (), n)
    a, b = LD.land_rotation(o, L.galois_keys([elt]), elt, c1, T0, galois=True), LD.land_galois(o, L.galois_keys([elt]), elt, c1, T0)
    assert (a[0] == b[0]).all() and (a[1] == b[1]).all()
