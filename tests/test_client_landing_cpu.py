"""The crafted operands of tests/client_landing.py land, shown without a device: u from tests/rng_ref.py, e drawn by numpy in
[-19, 19] (on the GPU the harvested e takes its place; the models do not care where the small integers come from).

For every parameter set of tests/test_gpu_client_landing.py: the two integer models of the encryption agree on every word, the
crafted key puts the key-level values on the targets, every pattern class occurs in every row and every target word is where its
class says (all of that is asserted inside landed_encryption), and under an ordinary oracle key the model's ciphertext decrypts in
the oracle to the plaintext.  For the CRT export: the Python CRT lands every named value, every subtraction count occurs, and
the crafted last row lands mod_switch_to_next in the oracle.

Then what the crafted inputs are FOR: each deliberately wrong model differs from the true one on the crafted inputs of every set
where the mutation applies.  How many uniformly random inputs it changes is printed beside it (run with -s), as information:
nothing is asserted about that number, and a mutation that random inputs also catch is no failure.  No GPU."""
import numpy as np
import pytest

from tests import client_landing as CL
from tests import landing as LD
from tests.client_landing import client

T_EXTRA = [2, (1 << 60) - 1]  # on P1: the r term needs the 128-bit product at the second
ENC_CASES = [(pid, None) for pid in CL.ENCRYPT_SETS] + [("P1", t) for t in T_EXTRA]
ENC_IDS = [f"{p}-t{t or 'batching'}" for p, t in ENC_CASES]


@pytest.fixture(scope="module", autouse=True)
def _drop():
    yield
    CL.drop_clients()


def _landed(L, op=1):
    """The landed encryption number `op` of the first seed with synthetic errors, built once per parameter set."""

    def make():
        u = CL.recompute_u(CL.SEEDS[0], L.n, op)
        e = CL.synthetic_e(L.rng(501), L.n)
        return (u, e) + CL.landed_encryption(L, u, e, shift=op)

    return L.cached(("cpu landed", op), make)


def test_the_recomputed_u_is_ternary_and_differs_per_counter_word():
    n = 4096
    us = [CL.recompute_u(CL.SEEDS[0], n, g) for g in (0, 1, 1 << 32, (1 << 32) + 1)]
    for u in us:
        assert set(np.unique(u).tolist()) == {-1, 0, 1}
        assert 0.6 < np.mean(u != 0) < 0.73
    for i in range(4):
        for k in range(i):
            assert (us[i] != us[k]).any()
    assert (CL.recompute_u(CL.SEEDS[1], n, 0) != us[0]).any()


@pytest.mark.parametrize("pid", CL.ENCRYPT_SETS)
def test_ntt_of_u_has_no_zero_for_the_fixed_seeds(pid):
    L = client(pid)
    for seed in CL.SEEDS:
        for op in (0, 1):
            assert (CL.ntt_of_u(L, CL.recompute_u(seed, L.n, op)) != 0).all(), (hex(seed), op)


@pytest.mark.parametrize("pid,t", ENC_CASES, ids=ENC_IDS)
def test_models_agree_and_every_target_word_is_landed(pid, t):
    L = client(pid, t)
    u, e, pk, m, T, x, divided, out = _landed(L)  # (the assertions are landed_encryption's)
    if pid == "P2":
        assert L.qsp < max(L.primes)  # the special prime below a data prime
    if pid == CL.SINGLE:
        assert L.KK == 1 and L.K == 1
    for row, q in zip(pk.reshape(-1, L.n), L.key_primes * 2):
        assert int(row.max()) < q  # a valid key: canonical residues
    # shifting the classes (another item of a batch) lands as well
    if L.n <= 4096:
        CL.landed_encryption(L, CL.recompute_u(CL.SEEDS[1], L.n, 0), e[::-1], shift=3)


@pytest.mark.parametrize("pid,t", ENC_CASES, ids=ENC_IDS)
def test_the_model_decrypts_in_the_oracle_under_an_ordinary_key(pid, t):
    L = client(pid, t)
    u = CL.recompute_u(CL.SEEDS[1], L.n, 5)
    e = CL.synthetic_e(L.rng(502), L.n)
    for m in (CL.plain_cycle(L, 2), L.rng(503).integers(0, L.t, L.n, dtype=np.uint64)):
        sk, pk = CL.ordinary_keys(L)
        x, divided, out = CL.encrypt_model(L, pk, u, e, m)
        assert (L.o.decrypt(out, sk) == m).all()


ENCRYPT_MUTATIONS = ["no_half", "truncate", "no_wrap", "no_reduce64", "add_gt"]


@pytest.mark.parametrize("pid,t", ENC_CASES, ids=ENC_IDS)
def test_mutated_encryption_models_differ_on_the_crafted_inputs(pid, t):
    L = client(pid, t)
    u, e, pk, m, T, x, divided, out = _landed(L)
    rng = L.rng(504)
    xr = LD.random_residues(rng, L.key_primes, (2,), L.n)
    mr = rng.integers(0, L.t, L.n, dtype=np.uint64)
    true_r = CL.finish_rns(L, xr, mr)[1]
    for variant in ENCRYPT_MUTATIONS:
        # no special prime: no division to get wrong, the plaintext addition alone
        applies = CL.no_reduce64_applies(L) if variant == "no_reduce64" else (L.KK > 1 or variant == "add_gt")
        crafted = int((CL.finish_rns(L, x, m, variant)[1] != out).sum())
        random = int((CL.finish_rns(L, xr, mr, variant)[1] != true_r).sum())
        print(f"{pid} t={L.t} {variant}: changes {crafted} of {out.size} crafted words, {random} of {true_r.size} random words"
              + ("" if applies else " (does not apply)"))
        if applies:
            assert crafted > 0, variant
    if pid in ("P1", "U1024"):
        assert CL.no_reduce64_applies(L)  # (q_sp a bit and twenty bits above a data prime)


# ---------------------------------------------------------------------------------------------------------------- CRT export
@pytest.mark.parametrize("pid", CL.CRT_SETS)
def test_crt_cases_land_and_mutated_composes_differ(pid):
    L = client(pid)
    P, K = L.primes, L.K
    rows, value, names, which = L.cached("crt", lambda: CL.crt_case(P, L.n))  # (the landing assertions are crt_case's)
    assert K == {CL.SINGLE: 1, "P1": 2, "W2048": 3, "U1024": 4, "P4": 8, "P6": 15}[pid]
    if pid == "W2048":
        assert L.Q.bit_length() > 64 * K - 16  # 60-bit primes: q fills all but a few bits of its limbs
    hist = CL.subtraction_histogram(P, rows)
    print(f"{pid} K={K}: coefficients needing 0 ... {K - 1} subtractions: {hist}")
    assert all(hist)
    lim = CL.limbs_of(value[0], K)
    assert K == 1 or (lim == np.uint64((1 << 64) - 1)).any()  # a limb of 2^64 - 1
    rng = L.rng(505)
    rr = LD.random_residues(rng, P, (2,), L.n)
    take = slice(0, 4096)  # (the limb-compare mutations run a Python loop per coefficient: a part of the cycle, all of it up to n = 4096)
    for variant, applies in (("one_fewer", K >= 2), ("top_limb", K >= 2), ("gt", False)):
        crafted = sum(int((CL.compose_model(P, rows[p][:, take], variant) != value[p][take]).sum()) for p in range(2))
        random = sum(int((CL.compose_model(P, rr[p][:, take], variant) != CL.compose_model(P, rr[p][:, take])).sum()) for p in range(2))
        print(f"{pid} K={K} {variant}: changes {crafted} crafted values, {random} random values of {2 * len(value[0][take])}")
        if applies:
            assert crafted > 0, variant
        if variant == "gt":
            # sum y_i (q / q_i) = 0 mod q forces every y_i = 0: the sum never EQUALS q, and '>' for '>=' changes nothing
            assert crafted == 0 and random == 0


@pytest.mark.parametrize("pid", CL.CRT_LOWER_SETS)
def test_the_crafted_last_row_lands_mod_switch_on_the_lower_level_cases(pid):
    L = client(pid)
    ct, rows, value = CL.lower_level_case(L)
    assert (L.o.mod_switch_to_next(ct) == rows).all()
    ql = L.primes[-1]
    for v in (0, 1, ql // 2 - 1, ql // 2, ql // 2 + 1, ql // 2 + 2, ql - 1):
        assert (ct[:, -1] == np.uint64(v)).any()
