"""tests/keygen_model.py does what it claims, shown without a device: its arithmetic against Python integers, its sampler against a
word-by-word restatement, the Gaussian's band and left-out share for the exact seeds and sizes tests/test_gpu_keygen_model.py uses,
the assembly and its inverse on synthetic a and e, deliberately wrong keys that check_key must refuse, and the builders of crafted
secrets landing their targets under assemble_model."""
import numpy as np
import pytest

from tests import client_landing as CL
from tests import keygen_model as KM
from tests import landing as LD
from tests import rng_ref
from tests.client_landing import client

SYNTH_SETS = ["P2", "U1024"]  # special prime below a data prime; KK = 5 with 30-bit rows beside 50-bit ones


@pytest.fixture(scope="module", autouse=True)
def _drop():
    yield
    CL.drop_clients()


def _obj(a):
    return np.asarray(a).astype(object)


def _synthetic(L, salt, digits):
    """(a uint64[digits][KK][n] without zeros, e int64[digits][n] uniform over the sampler's whole range)."""
    rng = L.rng(4000 + salt)
    a = np.stack([np.stack([rng.integers(1, q, L.n, dtype=np.uint64) for q in L.key_primes]) for _ in range(digits)])
    return a, rng.integers(-KM.E_MAX, KM.E_MAX + 1, (digits, L.n)).astype(np.int64)


def test_the_test_only_entry_point_is_declared_and_exported():
    import os
    import re

    from sunscreen_amd import _lib

    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    header = re.sub(r"/\*.*?\*/", "", open(os.path.join(root, "include", "hipbfv.h")).read(), flags=re.S)
    name = "hipbfv_debug_keygen_galois_secret"
    m = re.search(r"\blong\s+" + name + r"\s*\(([^)]*)\)\s*;", header)
    assert m, f"{name} is not declared in include/hipbfv.h"
    assert len(_lib._SIGNATURES[name]) == len(m.group(1).split(",")) == 3
    assert hasattr(_lib.load(), name), f"{name} is not exported"


# ---- arithmetic -----------------------------------------------------------------------------------------------------------------
def test_mulmod_is_exact_at_every_prime_size():
    rng = np.random.default_rng(11)
    primes = sorted(set(client("W2048").key_primes + client("U1024").key_primes + client("P2").key_primes + [(1 << 61) - 1]))
    for q in primes:
        a, b = rng.integers(0, q, 4096, dtype=np.uint64), rng.integers(0, q, 4096, dtype=np.uint64)
        a[:6] = [q - 1, 0, q - 1, 1, q // 2, q // 2 + 1]
        b[:6] = [q - 1, q - 1, 1, 1, 2, 2]
        assert (_obj(KM.mulmod(a, b, q)) == _obj(a) * _obj(b) % q).all(), q
        assert (_obj(KM.mulmod(a, np.uint64(q - 1), q)) == _obj(a) * (q - 1) % q).all(), q
        assert (KM.negmod(np.array([0, 1, q - 1], dtype=np.uint64), q) == np.array([0, q - 1, 1], dtype=np.uint64)).all()
        inv = KM.invmod(a[2:], q)
        assert (KM.mulmod(a[2:], inv, q) == 1).all()


def test_residues_and_centred_are_inverse():
    v = np.arange(-KM.E_MAX, KM.E_MAX + 1)
    for q in client("U1024").key_primes:
        assert (KM.centred(KM.residues(v, [q])[0], q) == v).all()


# ---- the sampler ----------------------------------------------------------------------------------------------------------------
def test_seeds_and_words_are_the_documented_ones():
    keys = KM.seed_keys(0x1234)
    assert keys == rng_ref.seed_from_u64_for_tests(0x1234)
    raw = np.array(KM.ENC_SEED512, dtype="<u8").tobytes()
    assert KM.seed_keys(KM.ENC_SEED512) == rng_ref.seed_from_512(raw) and len(raw) == 64
    assert KM.stream_word(3, 2) == 0x302 and KM.stream_word(1) == 0x100
    # word 0 of the encryption's block is the u that tests/client_landing.py recomputes
    for gop in (0, 1, (1 << 32) + 5):
        _, _, wu = KM.encrypt_error_words(keys, 64, gop)
        assert (((wu * np.uint64(3)) >> np.uint64(32)).astype(np.int64) - 1 == CL.recompute_u(0x1234, 64, gop)).all()
    s = KM.ternary(keys, 4096)
    assert set(np.unique(s)) == {-1, 0, 1}


def test_uniform_a_word_by_word_and_every_block_is_its_own():
    primes = client("P6").key_primes  # KK = 16: four blocks
    assert len(primes) == 16
    n = 32
    keys = KM.seed_keys(KM.GEN_SEED)
    word = KM.stream_word(2, 3) + (7 << 32)  # a high half too
    a = KM.uniform_a(keys, primes, n, word)
    for i, q in enumerate(primes):
        blk = rng_ref.chacha20_block(keys["pub"], np.arange(n), word & 0xFFFFFFFF, word >> 32, 0xA0 + (i >> 2))
        for x in (0, 1, n - 1):
            r = [int(blk[4 * (i & 3) + j][x]) for j in range(4)]
            wide = (((r[0] << 32) | r[1]) << 64) | ((r[2] << 32) | r[3])
            assert int(a[i][x]) == (wide >> 1) % q, (i, x)
    # the mutations the device test must see are visible in the model: another digit, another key, the secret key's block, one
    # block for all rows
    assert (KM.uniform_a(keys, primes, n, KM.stream_word(2, 0)) != KM.uniform_a(keys, primes, n, KM.stream_word(2, 1))).all(axis=1).any()
    assert (KM.uniform_a(keys, primes, n, KM.stream_word(2, 0)) != KM.uniform_a(keys, primes, n, KM.stream_word(3, 0))).any()
    same_block = KM.uniform_a(keys, [primes[0]] * 8, n, word)
    assert (same_block[0] != same_block[4]).any() and (same_block[0] != same_block[1]).any()


# ---- the Gaussian ---------------------------------------------------------------------------------------------------------------
def test_gaussian_constants_range_and_float32_error():
    assert KM.U1_SCALE == 2.0 ** -24  # 16777217.0f is 2^24
    assert KM.SIGMA32 == float(np.float32(3.2)) != 3.2
    assert 1.6e-5 < KM.GAUSS_ERROR < 1.7e-5 and KM.BAND == 10 * KM.GAUSS_ERROR
    # the extreme words: u1 = 2^-24 with cos = +-1 gives +-18.46, short of the clip; u1 = 1 gives 0
    top = 0xFFFFFFFF
    g = KM.gauss64(np.array([0, 0, top, 0xFF]), np.array([0, 1 << 31, 0, 0]))
    assert 18.45 < g[0] < 18.46 and -18.46 < g[1] < -18.45 and g[2] == 0.0 and g[3] == g[0]
    assert [int(v) for v in KM.rounded_gauss(np.array([0, 0]), np.array([0, 1 << 31]))[0]] == [KM.E_MAX, -KM.E_MAX]
    # numpy's float32 evaluation of the same expression stays inside the derived bound, and rounds differently only in the band
    rng = np.random.default_rng(5)
    a, b = rng.integers(0, 1 << 32, 400_000, dtype=np.uint64), rng.integers(0, 1 << 32, 400_000, dtype=np.uint64)
    g64, g32 = KM.gauss64(a, b), KM.gauss32(a, b).astype(np.float64)
    worst = float(np.abs(g64 - g32).max())
    print(f"float32 against float64 over {a.size} draws: largest difference {worst:.3g} (bound {KM.GAUSS_ERROR:.3g}, band {KM.BAND:.3g})")
    assert worst < KM.GAUSS_ERROR
    want, sure = KM.rounded_gauss(a, b)
    assert (np.rint(g32).astype(np.int64)[sure] == want[sure]).all()
    assert 1e-4 < float((~sure).mean()) < 6e-4  # about 2 BAND
    # compare_gauss: accepts either neighbour inside the band, nothing else, and nothing wrong outside it
    k = int(np.flatnonzero(~sure)[0])
    other = want.copy()
    other[k] += 1 if g64[k] > want[k] else -1
    KM.compare_gauss(other, a, b)
    for wrong in (want + (np.arange(a.size) == int(np.flatnonzero(sure)[0])), other + 2 * (np.arange(a.size) == k) * (other - want)):
        with pytest.raises(AssertionError):
            KM.compare_gauss(wrong, a, b)


def test_left_out_share_and_range_for_the_seeds_and_sizes_of_the_gpu_tests():
    """The float64 model alone leaves out fewer samples than the cap, key by key as the GPU tests count them, and never exceeds 18."""
    seeds = KM.seed_keys(KM.GEN_SEED)
    for pid in KM.GEN_SETS:
        L = client(pid)
        total = left = 0
        for stream, (name, kind, _) in enumerate(KM.key_plan(pid, L.n), 1):
            sure = []
            for z in KM.checked_digits(pid, L.K, kind):
                e, ok = KM.rounded_gauss(*KM.key_error_words(seeds, L.n, KM.stream_word(stream, z)))
                assert int(np.abs(e).max()) <= KM.E_MAX
                sure.append(ok)
            sure = np.stack(sure)
            assert float((~sure).mean()) < KM.LEFT_OUT_CAP, (pid, name, float((~sure).mean()))
            total, left = total + sure.size, left + int((~sure).sum())
        print(f"{pid}: {left} of {total} Gaussian samples inside the band: {100 * left / total:.4f} % (cap {100 * KM.LEFT_OUT_CAP} %)")
    seeds = KM.seed_keys(KM.ENC_SEED512)
    for pid in KM.ENC_SETS:
        L = client(pid)
        w0, w1, _ = KM.encrypt_error_words(seeds, L.n, 0)
        e, sure = KM.rounded_gauss(np.stack([w0[0], w1[0]]), np.stack([w0[1], w1[1]]))
        assert float((~sure).mean()) < KM.LEFT_OUT_CAP and int(np.abs(e).max()) <= KM.E_MAX and (e[0] != e[1]).any()
        e, sure = KM.rounded_gauss(*KM.key_error_words(seeds, L.n, KM.stream_word(1)))
        assert float((~sure).mean()) < KM.LEFT_OUT_CAP and int(np.abs(e).max()) <= KM.E_MAX


# ---- the assembly ---------------------------------------------------------------------------------------------------------------
def _galois_restated(rows, primes, n, elt):
    out = np.zeros_like(rows)
    k = np.arange(n, dtype=np.int64)
    idx, flip = (k * elt) % n, ((k * elt) // n) % 2 == 1
    for i, q in enumerate(primes):
        out[i][idx] = np.where(flip, KM.negmod(rows[i], q), rows[i])
    return out


@pytest.mark.parametrize("pid", SYNTH_SETS)
def test_galois_poly_on_every_key_level_row(pid):
    L = client(pid)
    s_coeff = KM.key_pattern(L.o)
    assert (KM.galois_poly(L.o, s_coeff, 1) == s_coeff).all()
    for elt in KM.galois_elements(L.n):
        got = KM.galois_poly(L.o, s_coeff, elt)
        assert got.shape == (L.KK, L.n) and (got == _galois_restated(s_coeff, L.key_primes, L.n, elt)).all(), elt
        assert all(int(r.max()) < q for r, q in zip(got, L.key_primes))  # canonical: a flipped 0 stays 0
    for elt in KM.SIGN_FLIP_ELEMENTS(L.n):
        assert min(KM.flipped_zeros(L.o, s_coeff, elt)) > 0, elt
    assert KM.flipped_zeros(L.o, s_coeff, 1) == [0] * L.KK


@pytest.mark.parametrize("pid", SYNTH_SETS)
def test_assemble_model_against_python_integers_and_its_inverse(pid):
    L = client(pid)
    P, KK = L.key_primes, L.KK
    (a,), (e,) = _synthetic(L, 1, 1)
    s = LD.random_residues(L.rng(4100), P, (), L.n)
    w = LD.random_residues(L.rng(4101), P, (), L.n)
    eh = KM.error_hat(L.o, e)
    for z in range(L.K):
        c0, c1 = KM.assemble_model(P, a, eh, s, w, z)
        for i, q in enumerate(P):
            want = (-(_obj(a[i]) * _obj(s[i]) + _obj(eh[i]))) % q
            if i == z:
                want = (want + _obj(w[i]) * (P[-1] % q)) % q
            assert (_obj(c0[i]) == want).all(), (z, i)
        assert (c1 == a).all()
        assert (KM.recover_errors(L.o, np.stack([c0, c1]), a, s, w, z) == e).all()
    c0, c1 = KM.assemble_model(P, a, eh, s, None, 0)
    assert (KM.recover_errors(L.o, np.stack([c0, c1]), a, s, None, 0) == e).all()
    assert KM.special_factor(P, 0) == P[-1] % P[0] and (pid != "P2" or P[-1] < P[0])


@pytest.mark.parametrize("pid", SYNTH_SETS)
def test_check_key_accepts_the_model_and_refuses_each_defect(pid):
    L = client(pid)
    o, P, K = L.o, L.key_primes, L.K
    seeds = KM.seed_keys(KM.GEN_SEED)
    stream = 4
    s = KM.ntt_rows(o, KM.residues(KM.ternary(seeds, L.n), P))
    w = KM.relin_w(o, s)
    digits = list(range(K))

    def make(a_word=lambda z: KM.stream_word(stream, z), e_word=lambda z: KM.stream_word(stream, z), subtract_once=False, post=None):
        key = np.zeros((K, 2, L.KK, L.n), dtype=np.uint64)
        for z in digits:
            a = KM.uniform_a(seeds, P, L.n, a_word(z))
            e = KM.rounded_gauss(*KM.key_error_words(seeds, L.n, e_word(z)))[0]
            key[z, 0], key[z, 1] = KM.assemble_model(P, a, KM.error_hat(o, e), s, w, z)
            if subtract_once:  # the w row's factor off by 2^64 mod q_z (a 64-bit difference that wrapped before its reduction)
                q = P[z]
                plain = KM.assemble_model(P, a, KM.error_hat(o, e), s, None, z)[0][z]
                key[z, 0, z] = KM.addmod(plain, KM.mulmod(w[z], np.uint64((P[-1] + (1 << 64)) % q), q), q)
        return key if post is None else post(key)

    parts = KM.check_key(o, seeds, make(), stream, s, w, digits)
    assert [p[0] for p in parts] == digits
    errors = np.stack([p[2] for p in parts])
    words = [KM.key_error_words(seeds, L.n, KM.stream_word(stream, z)) for z in digits]
    assert KM.compare_gauss(errors, np.stack([x[0] for x in words]), np.stack([x[1] for x in words])) < KM.LEFT_OUT_CAP
    # defects in the uniform polynomial are refused by check_key itself
    for bad in (make(a_word=lambda z: KM.stream_word(stream, 0)), make(a_word=lambda z: KM.stream_word(stream + 1, z))):
        with pytest.raises(AssertionError, match="c1 is not the uniform polynomial"):
            KM.check_key(o, seeds, bad, stream, s, w, digits)
    # one error for every digit: the key is consistent, the Gaussian comparison refuses it
    shared = KM.check_key(o, seeds, make(e_word=lambda z: KM.stream_word(stream, 0)), stream, s, w, digits)
    with pytest.raises(AssertionError, match="Gaussian differs"):
        KM.compare_gauss(np.stack([p[2] for p in shared]), np.stack([x[0] for x in words]), np.stack([x[1] for x in words]))
    # a wrong factor on the w row, and a word stored as q instead of 0
    with pytest.raises(AssertionError, match="c0 is not the model's"):
        KM.check_key(o, seeds, make(subtract_once=True), stream, s, w, digits)

    def store_q(key):
        key[K - 1, 0, K - 1, 5] = P[K - 1]  # (as if the word were 0 and its negation stored q)
        return key

    with pytest.raises(AssertionError, match="c0 is not the model's"):
        KM.check_key(o, seeds, make(post=store_q), stream, s, w, digits)


# ---- the crafted secrets ------------------------------------------------------------------------------------------------------------
def _shares_ok(rows_and_primes):
    for row, q in rows_and_primes:
        shares = KM.target_shares(row, q)
        assert min(shares) >= 0.10 and abs(sum(shares) - 1.0) < 1e-9, shares


@pytest.mark.parametrize("pid", KM.CRAFT_SETS)
def test_crafted_public_secret_lands_every_row(pid):
    L = client(pid)
    P = L.key_primes
    (a,), (e,) = _synthetic(L, 2, 1)
    T = KM.key_pattern(L.o)
    s, want = KM.craft_public_secret(L.o, a, e, T)
    c0, c1 = KM.assemble_model(P, a, KM.error_hat(L.o, e), s, None, 0)
    assert (c0 == want).all() and (c1 == a).all()
    assert (_obj(want) == (-_obj(T)) % LD._qcol(P, 0)).all()
    assert all(((T[i] == 0) == (c0[i] == 0)).all() and int(c0[i].max()) == q - 1 for i, q in enumerate(P))
    _shares_ok(zip(c0, P))


@pytest.mark.parametrize("pid", KM.CRAFT_SETS)
def test_crafted_identity_secret_lands_the_w_rows_and_the_plain_branch(pid):
    L = client(pid)
    P, K, KK = L.key_primes, L.K, L.KK
    a, e = _synthetic(L, 3, K)
    T = KM.key_pattern(L.o)
    s, landed = KM.craft_identity_secret(L.o, a, e, T)
    assert [(d, r) for d, r, _ in landed] == [(z, z) for z in range(K)] + [(0, KK - 1)]
    for d, r, want in landed:
        c0, _ = KM.assemble_model(P, a[d], KM.error_hat(L.o, e[d]), s, s, d)  # element 1: w = s
        assert (c0[r] == want).all(), (d, r)
        assert (want == (T[r] if r == d else KM.negmod(T[r], P[r]))).all()
    _shares_ok((want, P[r]) for _, r, want in landed)


@pytest.mark.parametrize("pid", KM.CRAFT_SETS)
def test_pattern_secret_has_flipped_zeros_in_every_row(pid):
    L = client(pid)
    s_coeff, s_ntt = KM.pattern_secret(L.o)
    assert (KM.ntt_rows(L.o, s_ntt, inverse=True) == s_coeff).all()
    _shares_ok(zip(s_coeff, L.key_primes))
    for elt in KM.SIGN_FLIP_ELEMENTS(L.n):
        assert min(KM.flipped_zeros(L.o, s_coeff, elt)) > 0, (pid, elt)
        sigma = KM.galois_poly(L.o, s_coeff, elt)
        assert all(int(r.max()) < q for r, q in zip(sigma, L.key_primes))
        assert (KM.galois_w(L.o, s_coeff, elt) == KM.ntt_rows(L.o, sigma)).all()
