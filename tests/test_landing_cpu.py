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
