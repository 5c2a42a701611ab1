"""The crafted operands of tests/transform_landing.py land, shown without a device.

The independent transform (Python integers, psi from the oracle's root search) equals the oracle's on random rows of every
parameter set before anything else uses either.  Every builder lands under the oracle on every crafted word.  The model of the
integer policy's lazy arithmetic equals the oracle on every landed row and reports, per row, which representative stands in front
of the last conditional subtraction: at target 0 the representatives q, 2q and 3q all occur in a forward transform (and 0 where
it does), at target q - 1 a representative >= q occurs; in an inverse transform residue 0 arrives as q.  Every "occurs at least
once" condition is asserted here, on the reference alone.

Then what the crafted inputs are FOR: each deliberately wrong model (`canonical` with '>' at either compare, the subtraction after
the n^-1 product with '>', a lift with '>' for '>=' at ceil(t / 2), a mod-switch without + h, a truncating mod-switch, a
mod-switch without the reduction mod q_j where a 64-bit subtraction wraps) differs from the true one on the crafted inputs.  How
many random inputs each changes is printed beside it (run with -s), as information.  No GPU."""
import numpy as np
import pytest

from tests import client_landing as CL
from tests import landing as LD
from tests import transform_landing as TL
from tests.client_landing import client

TRANSFORM_SETS = ["P1", "U1024", "W2048", "P5"]     # FP64-range primes, 50/30-bit, 60-bit, 54/56-bit
LAZY_ROWS = {"P1": [0, 2], "U1024": [0, 1, 4], "W2048": [0, 1, 2, 3], "P5": [0, 1, 2, 3], "P6": [0]}
PLAIN_SETS = ["U1024", "W2048", "P1", "P5"]
MS_SETS = ["U1024", "P2", "P3", "S4096", "W2048", "P1"]


@pytest.fixture(scope="module", autouse=True)
def _drop():
    yield
    CL.drop_clients()


# ---- 1: the independent transform ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("pid", TRANSFORM_SETS + ["P3"])
def test_the_independent_transform_equals_the_oracle_on_random_rows(pid):
    L = client(pid)
    rng = L.rng(7001)
    for i, q in enumerate(L.key_primes):
        x = rng.integers(0, q, L.n, dtype=np.uint64)
        f = TL.ntt_plain(L, i, x)
        assert (f == L.o.ntt(i, x)).all(), (pid, i, "forward")
        assert (TL.ntt_plain(L, i, x, inverse=True) == L.o.ntt(i, x, inverse=True)).all(), (pid, i, "inverse")
        assert (TL.ntt_plain(L, i, f, inverse=True) == x).all(), (pid, i, "round trip")


def test_the_independent_transform_at_the_largest_degree():
    L = client("P6")
    rng = L.rng(7002)
    for i in (0, L.o.KK - 1):
        x = rng.integers(0, L.key_primes[i], L.n, dtype=np.uint64)
        assert (TL.ntt_plain(L, i, x) == L.o.ntt(i, x)).all()
        assert (TL.ntt_plain(L, i, x, inverse=True) == L.o.ntt(i, x, inverse=True)).all()


# ---- 2: landed transforms -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("pid", TRANSFORM_SETS)
def test_landed_rows_transform_to_their_targets_under_both_references(pid):
    L = client(pid)
    KK = L.o.KK
    T, xf, xi = TL.landed_transform_rows(L, ["unit", "max", "pattern"], extra=1)
    assert len(T) == 3 * KK + 1
    for r in range(len(T)):
        i = r % KK
        q = L.key_primes[i]
        assert int(xf[r].max()) < q and int(xi[r].max()) < q
        assert (L.o.ntt(i, xf[r]) == T[r]).all() and (L.o.ntt(i, xi[r], inverse=True) == T[r]).all(), (pid, r)
        assert (TL.ntt_plain(L, i, xf[r]) == T[r]).all() and (TL.ntt_plain(L, i, xi[r], inverse=True) == T[r]).all(), (pid, r)
    # every target in every pattern row; the constant and the unit rows are what they are named
    for i, q in enumerate(L.key_primes):
        for v in LD.targets(q):
            assert (T[2 * KK + i] == np.uint64(v)).any(), (pid, i, v)
        assert (T[KK + i] == np.uint64(q - 1)).all() and int(T[i].sum()) == 1


@pytest.mark.parametrize("pid", ["P1", "U1024", "P6"])
def test_landed_ciphertexts_for_ct_to_ntt(pid):
    L = client(pid)
    for size in (2, 3):
        if pid == "P6" and size == 3:
            continue  # (one size at n = 32768: the host side of fifteen rows per polynomial)
        ct, T = TL.landed_ciphertexts_for_ct_to_ntt(L, size)
        for it in range(len(ct)):
            for c in range(size):
                for i in range(L.K):
                    assert (L.o.ntt(i, ct[it, c, i]) == T[it, c, i]).all(), (pid, size, it, c, i)


# ---- 3: the lazy model and its events -------------------------------------------------------------------------------------------
def _print_events(pid, i, direction, table):
    print(f"{pid} prime {i} {direction}: " + ", ".join(f"target {t} as {m}q+: {c}" for (t, m), c in sorted(table.items())))


@pytest.mark.parametrize("pid", list(LAZY_ROWS))
def test_the_lazy_model_lands_and_every_representative_occurs(pid):
    L = client(pid)
    KK = L.o.KK
    for i in LAZY_ROWS[pid]:
        q = L.key_primes[i]
        T = TL.target_row(L, i, "pattern", i)
        # forward
        x = TL.land_forward(L, i, T)
        rep, out = TL.ntt_lazy(L, i, x)
        assert (out == T).all(), (pid, i, "the lazy forward model does not land")
        ev = TL.events(rep, out, q)
        _print_events(pid, i, "forward", ev)
        for mult in (1, 2, 3):
            assert ("0", mult) in ev, (pid, i, "residue 0 never stored as", mult, "q")
        assert any(("q-1", mult) in ev for mult in (1, 2, 3)), (pid, i, "residue q - 1 never stored above q")
        for variant in ("gt_2q", "gt_q"):
            wrong = TL._u64(TL.canonical(rep, q, variant))
            changed = int((wrong != T).sum())
            print(f"{pid} prime {i} canonical {variant}: changes {changed} of {L.n} crafted words")
            assert changed > 0, variant
        # inverse
        x = TL.land_inverse(L, i, T)
        rep, out = TL.ntt_lazy(L, i, x, inverse=True)
        assert (out == T).all(), (pid, i, "the lazy inverse model does not land")
        ev = TL.events(rep, out, q)
        _print_events(pid, i, "inverse", ev)
        assert ("0", 1) in ev, (pid, i, "residue 0 never arrives as q")
        assert ("q-1", 1) not in ev  # (the truncated quotient is exact there: see the module's description)
        changed = int((TL._u64(TL.scale_finish(rep, q, "gt")) != T).sum())
        print(f"{pid} prime {i} scale_canonical gt: changes {changed} of {L.n} crafted words")
        assert changed > 0
    # all q - 1, and zero but one word: the model lands there too (one row per set)
    i = LAZY_ROWS[pid][-1]
    for kind in ("max", "unit"):
        T = TL.target_row(L, i, kind, 3)
        assert (TL.ntt_lazy(L, i, TL.land_forward(L, i, T))[1] == T).all(), (pid, kind)
        assert (TL.ntt_lazy(L, i, TL.land_inverse(L, i, T), inverse=True)[1] == T).all(), (pid, kind)
    assert KK == L.KK


@pytest.mark.parametrize("pid", ["W2048", "P5"])
def test_mutated_canonical_on_random_words(pid):
    """Information (nothing asserted but the count of words): 2^20 uniformly random representatives in [0, 4q) through `canonical`
    with '>' for '>=', and the words of random rows through the lazy model both ways: 2^20 of them under the 60-bit prime, 2^15
    under the 54-bit one."""
    L = client(pid)
    i = 0
    q = L.key_primes[i]
    rng = L.rng(7003)
    reps = rng.integers(0, 4 * q, 1 << 20, dtype=np.uint64)
    q2 = np.uint64(2 * q)
    true = np.where(reps >= q2, reps - q2, reps)
    true = np.where(true >= np.uint64(q), true - np.uint64(q), true)
    for variant in ("gt_2q", "gt_q"):
        v = np.where(reps > q2 if variant == "gt_2q" else reps >= q2, reps - q2, reps)
        v = np.where(v > np.uint64(q) if variant == "gt_q" else v >= np.uint64(q), v - np.uint64(q), v)
        print(f"{pid} canonical {variant}: changes {int((v != true).sum())} of {reps.size} random representatives")
    changed = {"gt_2q": 0, "gt_q": 0, "scale gt": 0}
    rows = (1 << (20 if pid == "W2048" else 15)) // L.n
    for _ in range(rows):
        x = rng.integers(0, q, L.n, dtype=np.uint64)
        rep, out = TL.ntt_lazy(L, i, x)
        assert (out == L.o.ntt(i, x)).all()
        for variant in ("gt_2q", "gt_q"):
            changed[variant] += int((TL._u64(TL.canonical(rep, q, variant)) != out).sum())
        rep, out = TL.ntt_lazy(L, i, x, inverse=True)
        assert (out == L.o.ntt(i, x, inverse=True)).all()
        changed["scale gt"] += int((TL._u64(TL.scale_finish(rep, q, "gt")) != out).sum())
    print(f"{pid} random rows through the lazy model ({rows * L.n} words each way): changed {changed}")


# ---- 4: the plaintext product ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("pid", PLAIN_SETS)
def test_multiply_plain_lands_under_the_oracle(pid):
    L = client(pid)
    for size in (2, 3):
        cts, plains, want, names = TL.multiply_plain_case(L, size, items=4 if size == 2 else 3)
        for k, where in enumerate(names):
            ref = L.o.multiply_plain(cts[k], plains[k])
            assert (ref == want[k]).all()
            T = LD.pattern(L.primes, size, L.n, 2 * k)
            pn = TL.plain_transform(L, plains[k])
            for i, q in enumerate(L.primes):
                for c in range(size):
                    fwd = L.o.ntt(i, cts[k, c, i])
                    if k == 3:
                        continue
                    if where == "output":
                        assert (ref[c, i] == T[c, i]).all(), (pid, size, k, "output")
                    if where == "forward":
                        assert (fwd == T[c, i]).all(), (pid, size, k, "forward")
                    if where == "product":
                        assert (TL._u64(TL._obj(fwd) * TL._obj(pn[i]) % q) == T[c, i]).all(), (pid, size, k, "product")
        if size == 2:
            q0 = L.primes[0]
            assert (want[3, 0, 0] == np.uint64(q0 - 1)).all() and int(want[3, 1, 0].sum()) == 1
    cts, p, want, names = TL.shared_plain_case(L, 2)
    assert all((L.o.multiply_plain(cts[k], p) == want[k]).all() for k in range(len(cts)))


@pytest.mark.parametrize("pid", PLAIN_SETS)
def test_a_lift_with_the_wrong_compare_differs_on_the_crafted_plaintexts(pid):
    """ceil(t / 2) is among every crafted plaintext's coefficients: a lift with '>' there moves the plaintext by q_i - t in that
    coefficient, and every word of the product with it.  Random plaintexts hold ceil(t / 2) about n / t of the time."""
    L = client(pid)
    cts, plains, want, names = TL.multiply_plain_case(L, 2, items=4)
    p, ct = plains[0], cts[0]
    wrong = np.stack([np.stack([L.o.ntt(i, TL._u64(TL._obj(L.o.ntt(i, ct[c, i])) * TL._obj(TL.plain_transform(L, p, "gt")[i]) % q), inverse=True)
                                for i, q in enumerate(L.primes)]) for c in range(2)])
    crafted = int((wrong != want[0]).sum())
    rng = L.rng(7004)
    pr = rng.integers(0, L.t, L.n, dtype=np.uint64)
    random = int((TL.plain_transform(L, pr, "gt") != TL.plain_transform(L, pr)).sum())
    print(f"{pid} lift gt: changes {crafted} of {want[0].size} crafted output words; {random} of {L.K * L.n} transform words of a random plaintext")
    assert crafted > 0


# ---- 5: encode ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("pid", ["P1", "U1024"])
def test_encode_lands_on_the_coefficient_pattern(pid):
    L = client(pid)
    t = L.t
    for Tp in TL.encode_targets(L):
        v, s = TL.land_encode(L, Tp)
        assert (L.o.batch_encode(v) == Tp).all()
        assert int(np.abs(s).max()) <= t >> 1 and ((s % t).astype(np.uint64) == v).all()
        assert (L.o.batch_encode((s % t).astype(np.uint64)) == Tp).all()
    Tp = TL.encode_targets(L)[0]
    for tv in LD.targets(t):
        assert (Tp == np.uint64(tv)).any()


# ---- 6: mod-switch --------------------------------------------------------------------------------------------------------------
def test_the_mod_switch_sets_hold_every_relation():
    assert TL.relations(client("U1024")) == {"above"} and TL.relations(client("S4096")) == {"above"}  # by ten and twenty bits
    assert TL.relations(client("P2")) == {"below"}
    assert TL.relations(client("P3")) == {"above", "below"}
    assert TL.relations(client("W2048")) == {"above"} and min(client("W2048").primes).bit_length() == 60
    assert client("P1").K == 2 and TL.relations(client("P1")) == {"below"}
    assert TL.no_reduce64_applies(client("U1024")) and TL.no_reduce64_applies(client("S4096"))


@pytest.mark.parametrize("pid", MS_SETS)
def test_mod_switch_lands_and_mutated_models_differ(pid):
    L = client(pid)
    rng = L.rng(7005)
    for size in (2, 3):
        ct, T = TL.mod_switch_case(L, size)  # (asserts: the two statements agree, every class occurs, every word is landed)
        for it in range(2):
            assert (L.o.mod_switch_to_next(ct[it]) == T[it]).all(), (pid, size, it)
    ct, T = TL.mod_switch_case(L, 2)
    rnd = LD.random_residues(rng, L.primes, (2,), L.n)
    true_r = TL.mod_switch_rns(L, rnd)
    assert (true_r == L.o.mod_switch_to_next(rnd)).all() and (true_r == TL.mod_switch_integers(L, rnd)).all()
    for variant in ("no_half", "truncate", "no_reduce64"):
        applies = variant != "no_reduce64" or TL.no_reduce64_applies(L)
        crafted = sum(int((TL.mod_switch_rns(L, ct[it], variant) != T[it]).sum()) for it in range(2))
        random = int((TL.mod_switch_rns(L, rnd, variant) != true_r).sum())
        print(f"{pid} mod-switch {variant}: changes {crafted} of {T.size} crafted words, {random} of {true_r.size} random words"
              + ("" if applies else " (does not apply)"))
        if applies:
            assert crafted > 0, variant
