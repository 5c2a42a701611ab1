"""Key generation on the device (keygen_ternary_kernel, keygen_sample_kernel, keygen_assemble_kernel, keygen_square_kernel,
keygen_galois_kernel and gauss_noise in sunscreen_amd/csrc/kernels_client.hip; the stream bookkeeping of Evaluator::keygen_* and
take_stream) against the integer model of tests/keygen_model.py, word for word.  tests/test_keygen_model_cpu.py shows without a
device that the model and its builders do what they claim.

2  every key of one seeded generator per parameter set: c1 is the uniform polynomial of the stream word (k << 8) + z in every row,
   the rows i != z hold one small error polynomial, that polynomial is rint(gauss64) of its two words outside the band around the
   half-integers (the share left out is counted against the 0.1 % cap), row z is the model's with w = s^2 or NTT(sigma_g(s));
   across all keys and digits the uniform and the error polynomials are pairwise distinct.
3  secrets crafted so that keygen_assemble_kernel's own output lands on 0, q - 1, 1 and the integers around q / 2: (A) a public key
   in every row, (B) the w row of every digit of the Galois key for element 1, and digit 0's special-prime row, (C) sign flips of a
   secret whose coefficients are the pattern; neg_mod(0) = 0 in keygen_galois_kernel is read off sigma_g(s) BEFORE its transform
   (KeyGenerator.debug_galois_secret): the transform accepts q for 0 and canonicalises, so no key shows the difference.
4  the same Gaussian model on the errors an encryption hands back, and the symmetric encryption's uniform polynomial."""
import numpy as np
import pytest

from tests import client_landing as CL
from tests import keygen_model as KM
from tests.client_landing import client

pytestmark = pytest.mark.gpu

assert KM.SINGLE == CL.SINGLE


@pytest.fixture(scope="module", autouse=True)
def _drop():
    yield
    _GENERATED.clear()
    _OPENED.clear()
    _CHECKED.clear()
    CL.drop_clients()


def _context(L):
    from sunscreen_amd import Context

    ctx = Context.from_raw(L.n, L.key_primes, L.t)
    assert ctx.K == L.K and ctx.KK == L.KK and ctx.key_primes == L.key_primes
    return ctx


def _same(got, want, what):
    got, want = np.asarray(got), np.asarray(want)
    assert got.shape == want.shape, (what, got.shape, want.shape)
    bad = np.argwhere(got != want)
    assert bad.size == 0, (what, "first difference at", bad[0].tolist(), int(got[tuple(bad[0])]), int(want[tuple(bad[0])]), len(bad))


def _galois_array(gk, ctx, elt):
    return gk.to_array(ctx, (elt - 1) // 2)


# ---- 2: every key of a generator --------------------------------------------------------------------------------------------------
_GENERATED: dict = {}
_OPENED: dict = {}
_CHECKED: dict = {}
GEN_CASES = [(pid, name) for pid in KM.GEN_SETS for name, _, _ in KM.key_plan(pid)]


def _generated(pid):
    """{name: (stream, kind, element, digits, uint64[digits][2][KK][n])}, the secret (NTT form) and its small polynomial: one seeded
    generator, the keys created in key_plan's order."""
    if pid not in _GENERATED:
        from sunscreen_amd import KeyGenerator

        L = client(pid)
        ctx = _context(L)
        kg = KeyGenerator(ctx, seed=KM.GEN_SEED)
        s_ntt = kg.secret_key().to_array(ctx)
        plan = KM.key_plan(pid, L.n)
        made, sigma = {}, {}
        stream = 0
        while stream < len(plan):
            name, kind, elt = plan[stream]
            if kind == "public":
                made[name] = kg.create_public_key().to_array(ctx)[None]
                stream += 1
            elif kind == "relin":
                made[name] = kg.create_relinearization_keys().to_array(ctx, 0)
                stream += 1
            else:  # the run of Galois keys in one call: one stream each, in the order given
                run = [p for p in plan[stream:] if p[1] == "galois"]
                gk = kg.create_galois_keys([p[2] for p in run])
                for p in run:
                    made[p[0]] = _galois_array(gk, ctx, p[2])
                    sigma[p[0]] = kg.debug_galois_secret(p[2])
                stream += len(run)
        keys = {}
        for k, (name, kind, elt) in enumerate(plan, 1):
            digits = KM.checked_digits(pid, L.K, kind)
            keys[name] = (k, kind, elt, digits, np.ascontiguousarray(made[name][digits]))
        _GENERATED[pid] = (keys, s_ntt, sigma)
    return _GENERATED[pid]


def _secret(pid):
    """(s int64[n], s_coeff uint64[KK][n]): the model's ternary secret; the device's must be its transform."""
    L = client(pid)

    def make():
        s = KM.ternary(KM.seed_keys(KM.GEN_SEED), L.n)
        return s, KM.residues(s, L.key_primes)

    return L.cached("keygen model secret", make)


def _w(pid, kind, elt, s_ntt):
    L = client(pid)
    if kind == "public":
        return None
    if kind == "relin":
        return KM.relin_w(L.o, s_ntt)
    return KM.galois_w(L.o, _secret(pid)[1], elt)


def _opened(pid, name):
    """[(z, a, e)] of one generated key, a and e the DEVICE's (KM.open_key: it needs the secret and w, no model of the sampler)."""
    if (pid, name) not in _OPENED:
        L = client(pid)
        generated, s_ntt, sigma = _generated(pid)
        stream, kind, elt, digits, key = generated[name]
        _same(s_ntt, KM.ntt_rows(L.o, _secret(pid)[1]), (pid, "the secret is not the transform of the model's ternary polynomial"))
        if kind == "galois":  # before its transform: every word canonical, a sign-flipped 0 of the ternary secret is 0
            _same(sigma[name], KM.galois_poly(L.o, _secret(pid)[1], elt), (pid, name, "sigma_g(s) in coefficient form"))
        _OPENED[(pid, name)] = KM.open_key(L.o, key, s_ntt, _w(pid, kind, elt, s_ntt), digits)
    return _OPENED[(pid, name)]


def _checked(pid, name):
    """[(z, a, e)] of one generated key compared with the model of the sampler (KM.check_key), and the Gaussian's left-out share."""
    if (pid, name) not in _CHECKED:
        L = client(pid)
        stream, kind, elt, digits, key = _generated(pid)[0][name]
        seeds = KM.seed_keys(KM.GEN_SEED)
        parts = KM.check_key(L.o, seeds, key, stream, None, None, digits, opened=_opened(pid, name))
        words = [KM.key_error_words(seeds, L.n, KM.stream_word(stream, z)) for z, _, _ in parts]
        share = KM.compare_gauss(np.stack([e for _, _, e in parts]), np.stack([w[0] for w in words]), np.stack([w[1] for w in words]))
        print(f"{pid} {name}: stream {stream}, digits {digits}: Gaussian samples left out {100 * share:.4f} % (cap {100 * KM.LEFT_OUT_CAP} %)")
        _CHECKED[(pid, name)] = (parts, share)
    return _CHECKED[(pid, name)]


@pytest.mark.parametrize("pid,name", GEN_CASES, ids=[f"{p}-{k}" for p, k in GEN_CASES])
def test_a_generated_key_equals_the_model_word_for_word(pid, name):
    parts, share = _checked(pid, name)
    assert share <= KM.LEFT_OUT_CAP
    assert [z for z, _, _ in parts] == _generated(pid)[0][name][3]


@pytest.mark.parametrize("pid", KM.GEN_SETS)
def test_no_two_keys_or_digits_share_randomness(pid):
    L = client(pid)
    every = [(name, z, a, e) for name, _, _ in KM.key_plan(pid, L.n) for z, a, e in _opened(pid, name)]
    assert len(every) == sum(len(KM.checked_digits(pid, L.K, kind)) for _, kind, _ in KM.key_plan(pid, L.n))
    for what, index in (("uniform polynomial", 2), ("error polynomial", 3)):
        seen = {}
        for item in every:
            h = np.ascontiguousarray(item[index]).tobytes()
            assert h not in seen, (pid, what, "shared by", seen[h], item[:2])
            seen[h] = item[:2]
    # (rows i and i + 4 of one digit are reduced by different primes: that they come from different blocks is what the comparison
    # with uniform_a pins, word for word)
    # the errors come from their own domain of the SECRET key: not the ternary secret's block, not the published key's
    seeds = KM.seed_keys(KM.GEN_SEED)
    s = _secret(pid)[0]
    tern = KM._block(seeds["secret"], L.n, 0, KM.DOMAIN_TERNARY)
    wrong_secret = KM.rounded_gauss(tern[0], tern[1])[0]
    for name, z, _, e in every:
        stream = _generated(pid)[0][name][0]
        pub = KM._block(seeds["pub"], L.n, KM.stream_word(stream, z), KM.DOMAIN_ERROR)
        assert (e != s).any() and (e != wrong_secret).any(), (pid, name, z, "the error repeats the ternary secret's stream")
        assert (e != KM.rounded_gauss(pub[0], pub[1])[0]).any(), (pid, name, z, "the error is drawn from the published key")


# ---- 3: crafted secrets -------------------------------------------------------------------------------------------------------------
def _generator(ctx, seed, s_ntt=None):
    from sunscreen_amd import KeyGenerator, SecretKey

    if s_ntt is None:
        return KeyGenerator(ctx, seed=seed)
    return KeyGenerator(ctx, SecretKey.from_array(ctx, s_ntt), seed=seed)


def _assert_targets_occur(L, landed):
    for digit, row, want in landed:
        shares = KM.target_shares(want, L.key_primes[row])
        assert min(shares) >= 0.10, (L.pid, digit, row, shares)


@pytest.mark.parametrize("pid", KM.CRAFT_SETS)
def test_a_public_key_landed_on_the_edges_in_every_row(pid):
    """(A) c0 = -T exactly: 0 where T = 0 (never q), q - 1, 1 and the integers around q / 2."""
    L = client(pid)
    ctx = _context(L)
    seed = KM.CRAFT_SEEDS["A"]
    seeds = KM.seed_keys(seed)
    kg = _generator(ctx, seed)
    s0 = kg.secret_key().to_array(ctx)
    ((_, a, e),) = KM.check_key(L.o, seeds, kg.create_public_key().to_array(ctx), 1, s0, None)
    s, want = KM.craft_public_secret(L.o, a, e, KM.key_pattern(L.o))
    _assert_targets_occur(L, [(0, i, want[i]) for i in range(L.KK)])
    pk = _generator(ctx, seed, s).create_public_key().to_array(ctx)
    _same(pk[1], a, (pid, "c1 of the landed public key"))
    _same(pk[0], want, (pid, "c0 of the landed public key"))
    ((_, _, e2),) = KM.check_key(L.o, seeds, pk, 1, s, None)
    assert (e2 == e).all(), "the error depends on the secret"


@pytest.mark.parametrize("pid", KM.CRAFT_SETS)
def test_the_w_row_landed_on_the_edges_in_every_digit(pid):
    """(B) the Galois key for element 1 has w = s: row z of digit z is (f_z - a_zz) s_z - e_hat_zz, landed on the pattern through
    the add_mod after mul_mod(w, factor); the special-prime row of digit 0 is landed through the plain branch."""
    L = client(pid)
    ctx = _context(L)
    seed = KM.CRAFT_SEEDS["B"]
    seeds = KM.seed_keys(seed)
    digits = list(range(L.K))
    kg = _generator(ctx, seed)
    s0 = kg.secret_key().to_array(ctx)
    parts = KM.check_key(L.o, seeds, _galois_array(kg.create_galois_keys([1]), ctx, 1), 1, s0, s0, digits)
    a, e = np.stack([p[1] for p in parts]), np.stack([p[2] for p in parts])
    s, landed = KM.craft_identity_secret(L.o, a, e, KM.key_pattern(L.o))
    _assert_targets_occur(L, landed)
    key = _galois_array(_generator(ctx, seed, s).create_galois_keys([1]), ctx, 1)
    for digit, row, want in landed:
        _same(key[digit][0][row], want, (pid, "landed row", digit, row))
    parts2 = KM.check_key(L.o, seeds, key, 1, s, s, digits)
    assert all((p2[2] == p[2]).all() for p, p2 in zip(parts, parts2)), "the error depends on the secret"


@pytest.mark.parametrize("pid", KM.CRAFT_SETS)
def test_sign_flips_of_a_pattern_secret(pid):
    """(C) s has the pattern as its COEFFICIENTS, zeros under a sign flip included: every row of every digit, the w row with
    w = NTT(sigma_g(s)) among them, is the model's."""
    L = client(pid)
    ctx = _context(L)
    seed = KM.CRAFT_SEEDS["C"]
    s_coeff, s_ntt = KM.pattern_secret(L.o)
    elts = KM.SIGN_FLIP_ELEMENTS(L.n)
    for elt in elts:
        assert min(KM.flipped_zeros(L.o, s_coeff, elt)) > 0, (pid, elt)
    kg = _generator(ctx, seed, s_ntt)
    gk = kg.create_galois_keys(list(elts))
    for stream, elt in enumerate(elts, 1):
        # what keygen_galois_kernel itself stores: the transform that follows would take a q for a 0 and hide it
        _same(kg.debug_galois_secret(elt), KM.galois_poly(L.o, s_coeff, elt), (pid, elt, "sigma_g(s) in coefficient form"))
        KM.check_key(L.o, KM.seed_keys(seed), _galois_array(gk, ctx, elt), stream, s_ntt, KM.galois_w(L.o, s_coeff, elt), list(range(L.K)))


# ---- 4: the encryption's errors -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("pid", KM.ENC_SETS)
def test_encryption_errors_are_the_model_gaussian_and_symmetric_c1_is_its_stream(pid):
    from sunscreen_amd import Encryptor, Plaintext, PublicKey, SecretKey

    L = client(pid)
    ctx = _context(L)
    sk, pk = CL.ordinary_keys(L)
    enc = Encryptor(ctx, PublicKey.from_array(ctx, pk), secret_key=SecretKey.from_array(ctx, sk))
    seeds = KM.seed_keys(KM.ENC_SEED512)
    plain = Plaintext.from_coefficients([1, 2, 3])
    # public key: operation 0 of the seed; u is word 0, e0 words 1 and 2, e1 words 3 and 4 of one block
    _, u, e, _ = enc.encrypt_return_components(plain, seed=KM.ENC_SEED512, disable_special_modulus=False)
    us = CL.small_from_rows(u.as_rns_u64s().reshape(L.K, L.n), L.primes)
    e_rows = e.as_rns_u64s().reshape(2, L.K, L.n)
    es = np.stack([CL.small_from_rows(e_rows[c], L.primes) for c in range(2)])
    w0, w1, wu = KM.encrypt_error_words(seeds, L.n, 0)
    assert (us == ((wu * np.uint64(3)) >> np.uint64(32)).astype(np.int64) - 1).all()
    share = KM.compare_gauss(es, np.stack([w0[0], w1[0]]), np.stack([w0[1], w1[1]]))
    print(f"{pid} encrypt_return_components: Gaussian samples left out {100 * share:.4f} % (cap {100 * KM.LEFT_OUT_CAP} %)")
    assert (es[0] != es[1]).any(), "e0 and e1 are one draw"
    assert int(np.abs(es).max()) <= KM.E_MAX
    # symmetric: the key generator's sampler at stream 1 of the seed
    ct, e, _ = enc.encrypt_symmetric_return_components(plain, seed=KM.ENC_SEED512)
    e1 = CL.small_from_rows(e.as_rns_u64s().reshape(L.K, L.n), L.primes)
    word = KM.stream_word(1)
    share = KM.compare_gauss(e1, *KM.key_error_words(seeds, L.n, word))
    print(f"{pid} encrypt_symmetric_return_components: Gaussian samples left out {100 * share:.4f} % (cap {100 * KM.LEFT_OUT_CAP} %)")
    a = KM.uniform_a(seeds, L.key_primes, L.n, word)
    c = ct.to_array()
    _same(KM.ntt_rows(L.o, c[1]), a[: L.K], (pid, "symmetric c1 is not the uniform polynomial of stream 1"))
    # c0 = Delta m + r - (a s + e) on the data rows, in the model's integers
    c0, _ = KM.assemble_model(L.primes, a[: L.K], KM.error_hat(L.o, e1)[: L.K], sk[: L.K], None, 0)
    m = np.zeros(L.n, dtype=np.uint64)
    m[:3] = [1, 2, 3]
    want = np.stack([KM.addmod(r, p, q) for r, p, q in zip(KM.ntt_rows(L.o, c0, inverse=True), CL.plain_term(L, m), L.primes)])
    _same(c[0], want, (pid, "symmetric c0"))
