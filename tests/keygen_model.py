"""An integer model of key generation's sampler and assembly (sunscreen_amd/csrc/kernels_client.hip: keygen_ternary_kernel,
keygen_sample_kernel, keygen_assemble_kernel, keygen_square_kernel, keygen_galois_kernel, gauss_noise) and of the stream bookkeeping
around them (Evaluator::keygen_* in evaluator_client.cpp, take_stream and encrypt_one in capi.cpp), with builders of SECRETS crafted so
that the assembled key lands on 0, q - 1, 1 and the two integers around q / 2 (the method of tests/landing.py).

Streams.  A generator numbers the keys it creates 1, 2, 3, ... (next_stream starts at 1; re-seeding restarts it); digit z of key number
k draws from the stream word (k << 8) + z, a public key from (k << 8).  The secret itself is stream word 0 in its own domain.  A block
is ChaCha20_block(key, (coefficient, word low half, word high half, domain)):

    ternary secret   secret key, domain 0x5E, word 0:             ((w0 * 3) >> 32) - 1
    error e          secret key, domain 0xE0, words 0 and 1:      one rounded Gaussian per coefficient, the same in every residue row
    uniform a        PUBLISHED key, domain 0xA0 + (i >> 2):       row i takes words 4 (i & 3) ... 4 (i & 3) + 3 as one 128-bit integer,
                                                                   most significant word first; a_i = (wide >> 1) mod q_i

The Encryptor: an encryption under a caller's 512-bit seed is operation 0 of that seed.  A public-key encryption draws u (word 0),
e0 (words 1, 2) and e1 (words 3, 4) from the secret key's block at (coefficient, gop low, gop high, domain 0); a symmetric encryption
is the key generator's sampler at stream number gop + 1, i.e. stream word (gop + 1) << 8: its c1 is uniform_a of that word (handed
back in coefficient form) and its e the Gaussian of words 0 and 1 at domain 0xE0.

Assembly.  c1 = a;  c0_i = -(a_i s_i + NTT(e)_i) mod q_i, and on row i = z of digit z of a key-switching key + w_z (q_sp mod q_z) with
w = s^2 (relinearization) or NTT(sigma_g(s)) (Galois element g).  Every word is canonical: -0 is 0, never q.

The Gaussian.  gauss_noise(a, b) = rint(clip(sqrtf(-2 logf(u1)) cospif(2 u2) 3.2f, +-19)), u1 = ((a >> 8) + 1) (1.0f / 16777217.0f),
u2 = (b >> 8) / 2^24.  16777217 = 2^24 + 1 is not a float: the literal 16777217.0f IS 2^24 (ties to even) and the constant exactly
2^-24, so u1 = m 2^-24 with m in [1, 2^24] is exact in float32 -- the model multiplies by U1_SCALE, the float32 quotient, not by the
real 1 / 16777217.  u1 >= 2^-24 bounds |z| by 3.2 sqrt(48 ln 2) = 18.46: the clip at +-19 cannot be reached (max |e| = 18).
logf and cospif cannot be restated bit for bit; gauss64 evaluates the same expression in float64 and the device must give
rint(gauss64) wherever gauss64 is further than BAND from a half-integer.  The float32 error behind BAND, with the error bounds the
OpenCL full profile allows the device functions (log <= 3 ulp, sqrt <= 3 ulp, cospi <= 4 ulp; HIP documents 1, 1 and 1), eps = 2^-24
the float32 rounding unit (an ulp is at most 2 eps relative), r = sqrt(-2 ln u1) <= 5.77, |c| <= 1:

    u1, 2 u2, -2 logf     exact scalings of exact inputs                                 0
    logf                  3 ulp relative, halved by the square root                      3 eps
    sqrtf                 3 ulp relative                                                 6 eps
    the two products      half an ulp each                                               2 eps
    cospif                4 ulp of a value <= 1: absolute 4 eps (an ulp below 1 is eps), times 3.2 r

    |float32 - exact| <= 3.2 r (11 eps |c| + 4 eps) <= 18.46 * 15 * 2^-24 = GAUSS_ERROR = 1.65e-5;  BAND = 10 * GAUSS_ERROR = 1.65e-4.

A Gaussian of sigma 3.2 puts about 2 BAND = 0.033 % of its draws that close to a half-integer; a test may leave out at most
LEFT_OUT_CAP = 0.1 % of its samples (tests/test_keygen_model_cpu.py counts the model's own share for the seeds and sizes the GPU tests
use, and measures numpy's float32 evaluation against the float64 one).

Test infrastructure, CPU only: imports the oracle, numpy and tests/rng_ref.py, never the library under test.  Residue arithmetic is
exact: products of 64-bit residues are formed in uint64 a few bits of the multiplier at a time (mulmod)."""
from __future__ import annotations

import math

import numpy as np

from oracle import bfv_oracle as O
from tests import landing as LD
from tests import rng_ref

DOMAIN_TERNARY, DOMAIN_ERROR, DOMAIN_UNIFORM = 0x5E, 0xE0, 0xA0
SIGMA32 = float(np.float32(3.2))
U1_SCALE = float(np.float32(1.0) / np.float32(16777217.0))  # 2^-24 exactly: see the module's docstring
GAUSS_ERROR = 3.2 * math.sqrt(48 * math.log(2)) * 15 * 2.0 ** -24
BAND = 10 * GAUSS_ERROR
LEFT_OUT_CAP = 1e-3
E_MAX = 18


# ------------------------------------------------------------------------------------------------------------- arithmetic
def mulmod(a, b, q: int) -> np.ndarray:
    """uint64: a * b mod q element by element for canonical residues a, b < q < 2^62, without leaving uint64: Horner over the
    multiplier in chunks of as many bits as q leaves free in a 64-bit word."""
    q = int(q)
    assert 1 < q < (1 << 62)
    a, b = np.asarray(a, dtype=np.uint64), np.asarray(b, dtype=np.uint64)
    bits = q.bit_length()
    cb = 64 - bits
    qq = np.uint64(q)
    if cb >= bits:
        return (a * b) % qq
    mask = np.uint64((1 << cb) - 1)
    acc = np.zeros(np.broadcast(a, b).shape, dtype=np.uint64)
    top = -(-bits // cb) * cb
    for sh in range(top - cb, -1, -cb):
        acc = ((acc << np.uint64(cb)) % qq + (a * ((b >> np.uint64(sh)) & mask)) % qq) % qq
    return acc


def addmod(a, b, q: int) -> np.ndarray:
    return (np.asarray(a, dtype=np.uint64) + np.asarray(b, dtype=np.uint64)) % np.uint64(q)


def negmod(a, q: int) -> np.ndarray:
    a = np.asarray(a, dtype=np.uint64)
    return np.where(a == 0, np.uint64(0), np.uint64(q) - a)


def invmod(a, q: int) -> np.ndarray:
    """uint64: a^-1 mod q word by word (Python integers; the crafted secrets are small)."""
    flat = [pow(int(v), -1, int(q)) for v in np.asarray(a).ravel().tolist()]
    return np.array(flat, dtype=np.uint64).reshape(np.shape(a))


def residues(v, primes) -> np.ndarray:
    """uint64[len(primes)][n]: the residues of the small signed integers v."""
    v = np.asarray(v, dtype=np.int64)
    return np.stack([np.where(v < 0, v + np.int64(q), v).astype(np.uint64) for q in primes])


def centred(row, q: int) -> np.ndarray:
    row = np.asarray(row, dtype=np.uint64)
    return np.where(row > np.uint64(q // 2), row.astype(np.int64) - np.int64(q), row.astype(np.int64))


def ntt_rows(o, rows, inverse: bool = False, first: int = 0) -> np.ndarray:
    """uint64[...][n]: the oracle's transform of key-level rows first, first + 1, ..."""
    return np.stack([o.ntt(first + i, np.ascontiguousarray(r), inverse=inverse) for i, r in enumerate(rows)])


# ------------------------------------------------------------------------------------------------------------ the sampler
def seed_keys(seed) -> dict:
    """{"secret", "pub"}: the two ChaCha keys of a 64-bit test seed (an int) or of a 512-bit seed (eight 64-bit words)."""
    if isinstance(seed, int):
        return rng_ref.seed_from_u64_for_tests(seed)
    assert len(seed) == 8
    return rng_ref.seed_from_512(np.array([int(w) for w in seed], dtype="<u8").tobytes())


def stream_word(stream: int, z: int = 0) -> int:
    return (int(stream) << 8) + int(z)


def _block(key8, n: int, word: int, domain: int):
    return rng_ref.chacha20_block(key8, np.arange(n), word & 0xFFFFFFFF, word >> 32, domain)


def ternary(keys: dict, n: int) -> np.ndarray:
    """int64[n]: the ternary secret of a seeded generator."""
    w0 = _block(keys["secret"], n, 0, DOMAIN_TERNARY)[0]
    return ((w0 * np.uint64(3)) >> np.uint64(32)).astype(np.int64) - 1


def uniform_a(keys: dict, primes, n: int, word: int) -> np.ndarray:
    """uint64[len(primes)][n]: the published uniform polynomial of stream word `word`, sampled in the transform domain."""
    out = np.zeros((len(primes), n), dtype=np.uint64)
    blk = None
    for i, q in enumerate(primes):
        q = int(q)
        if (i & 3) == 0:
            blk = _block(keys["pub"], n, word, DOMAIN_UNIFORM + (i >> 2))
        r = blk[4 * (i & 3): 4 * (i & 3) + 4]
        hi = (r[0] << np.uint64(32)) | r[1]
        lo = (r[2] << np.uint64(32)) | r[3]
        lo = (lo >> np.uint64(1)) | ((hi & np.uint64(1)) << np.uint64(63))  # wide >> 1 = hi * 2^64 + lo
        hi = hi >> np.uint64(1)
        out[i] = addmod(mulmod(hi % np.uint64(q), np.uint64((1 << 64) % q), q), lo % np.uint64(q), q)
    return out


def gauss64(a, b) -> np.ndarray:
    """float64: sqrt(-2 ln u1) cos(2 pi u2) 3.2 before rounding, for the 32-bit words a and b."""
    a, b = np.asarray(a, dtype=np.uint64), np.asarray(b, dtype=np.uint64)
    u1 = ((a >> np.uint64(8)) + np.uint64(1)).astype(np.float64) * U1_SCALE
    u2 = (b >> np.uint64(8)).astype(np.float64) / 16777216.0
    return np.sqrt(-2.0 * np.log(u1)) * np.cos(2.0 * np.pi * u2) * SIGMA32


def gauss32(a, b) -> np.ndarray:
    """float32: the same expression in numpy's float32 (NOT the device's logf and cospif: a measure of float32's error only)."""
    a, b = np.asarray(a, dtype=np.uint64), np.asarray(b, dtype=np.uint64)
    f = np.float32
    u1 = ((a >> np.uint64(8)).astype(f) + f(1.0)) * (f(1.0) / f(16777217.0))
    u2 = (b >> np.uint64(8)).astype(f) * (f(1.0) / f(16777216.0))
    c = np.cos((np.pi * (f(2.0) * u2).astype(np.float64))).astype(f)  # cospif: the argument's product with pi is not rounded
    return np.sqrt(f(-2.0) * np.log(u1)) * c * f(3.2)


def key_error_words(keys: dict, n: int, word: int):
    """(a, b): the two words behind the error of stream word `word` (key generation, symmetric encryption)."""
    blk = _block(keys["secret"], n, word, DOMAIN_ERROR)
    return blk[0], blk[1]


def encrypt_error_words(keys: dict, n: int, gop: int):
    """((a0, b0), (a1, b1)): the words behind e0 and e1 of public-key encryption number gop; and word 0, behind u."""
    blk = _block(keys["secret"], n, gop, 0)
    return (blk[1], blk[2]), (blk[3], blk[4]), blk[0]


def rounded_gauss(a, b):
    """(e int64, sure bool): rint(gauss64) and where the device's float32 evaluation must round the same way -- gauss64 further
    than BAND from every half-integer."""
    g = gauss64(a, b)
    frac = np.abs(g - np.floor(g) - 0.5)
    return np.rint(g).astype(np.int64), frac > BAND


def compare_gauss(got, a, b) -> float:
    """Asserts got == rint(gauss64(a, b)) wherever the model is sure and that at most LEFT_OUT_CAP of the samples are left out;
    returns the share left out."""
    want, sure = rounded_gauss(a, b)
    got = np.asarray(got, dtype=np.int64)
    assert got.shape == want.shape
    got, want, sure = got.ravel(), want.ravel(), sure.ravel()
    bad = np.flatnonzero(sure & (got != want))
    assert bad.size == 0, ("Gaussian differs from rint(gauss64) outside the band: first at", int(bad[0]), int(got[bad[0]]), int(want[bad[0]]), bad.size)
    # inside the band the device may round either way, to one of the two neighbours and nothing else
    assert (np.abs(got - want) <= 1).all(), "Gaussian inside the band is not one of the two neighbouring integers"
    share = float((~sure).mean())
    assert share <= LEFT_OUT_CAP, ("left out", share)
    return share


# ------------------------------------------------------------------------------------------------------------- the assembly
def special_factor(key_primes, z: int) -> int:
    return int(key_primes[-1]) % int(key_primes[z])


def assemble_model(primes, a, e_hat, s, w, z: int):
    """(c0, c1) uint64[KK][n] of one digit: c0_i = -(a_i s_i + e_hat_i) [+ w_z (q_sp mod q_z) on row z, when w is given] mod q_i,
    c1 = a; all in the transform domain, every word canonical."""
    c0 = np.zeros_like(np.asarray(a, dtype=np.uint64))
    for i, q in enumerate(primes):
        q = int(q)
        v = negmod(addmod(mulmod(a[i], s[i], q), e_hat[i], q), q)
        if w is not None and i == z:
            v = addmod(v, mulmod(w[i], np.uint64(special_factor(primes, z)), q), q)
        c0[i] = v
    return c0, np.array(a, dtype=np.uint64)


def recover_errors(o, key, a, s_ntt, w_ntt, z: int) -> np.ndarray:
    """int64[n]: the error polynomial of one digit, key = (c0, c1) uint64[2][KK][n]: the centred inverse transform of
    -(c0 + a s) mod q_i for every row i != z (every row when w_ntt is None: a public key has no w row); asserts that all of them
    are one polynomial."""
    out = None
    for i, q in enumerate(o.key_primes):
        if w_ntt is not None and i == z:
            continue
        r = negmod(addmod(key[0][i], mulmod(a[i], s_ntt[i], q), q), q)
        e = centred(o.ntt(i, r, inverse=True), q)
        assert out is None or (e == out).all(), ("the rows of one digit do not hold one error polynomial", z, i)
        out = e
    return out


def error_hat(o, e) -> np.ndarray:
    """uint64[KK][n]: NTT(e) in every key-level residue."""
    return ntt_rows(o, residues(e, o.key_primes))


def _special_oracle(o):
    """An oracle whose one data prime is o's special prime: apply_galois_poly works on data rows alone."""
    if not hasattr(o, "_keygen_model_special"):
        o._keygen_model_special = O.Oracle(o.n, [o.key_primes[-1], o.key_primes[0]], o.t)
    return o._keygen_model_special


def galois_poly(o, s_coeff, elt: int) -> np.ndarray:
    """uint64[KK][n]: sigma_elt of a key-level polynomial in coefficient form, through the oracle's apply_galois_poly (the data
    rows by o itself, the special-prime row by an oracle that has that prime as its data prime)."""
    s_coeff = np.ascontiguousarray(s_coeff, dtype=np.uint64)
    data = o.apply_galois_poly(s_coeff[: o.K], elt)
    sp = _special_oracle(o).apply_galois_poly(s_coeff[o.K:], elt)
    return np.concatenate([data, sp])


def galois_w(o, s_coeff, elt: int) -> np.ndarray:
    """uint64[KK][n]: w = NTT(sigma_elt(s)) of a Galois key."""
    return ntt_rows(o, galois_poly(o, s_coeff, elt))


def relin_w(o, s_ntt) -> np.ndarray:
    return np.stack([mulmod(s_ntt[i], s_ntt[i], q) for i, q in enumerate(o.key_primes)])


def open_key(o, key, s_ntt, w_ntt, digits=None):
    """One key taken apart with nothing but the secret and w: [(z, a, e)] with a = the key's own c1.  key: uint64[2][KK][n] (a
    public key: w_ntt None) or uint64[len(digits)][2][KK][n] holding the digits `digits` of a key-switching key.  Asserts that the
    rows i != z hold one small error polynomial e, and that c0 -- the w row included -- is assemble_model's for a, e, s and w."""
    key = np.asarray(key)
    if key.ndim == 3:
        key, digits = key[None], [0]
    out = []
    for d, z in enumerate(digits):
        a = np.array(key[d][1], dtype=np.uint64)
        e = recover_errors(o, key[d], a, s_ntt, w_ntt, z)
        assert int(np.abs(e).max()) <= E_MAX, ("error beyond what the sampler can give", z, int(np.abs(e).max()))
        c0, _ = assemble_model(o.key_primes, a, error_hat(o, e), s_ntt, w_ntt, z)
        bad = np.argwhere(key[d][0] != c0)
        assert bad.size == 0, ("c0 is not the model's", z, "first at [row, word]", bad[0].tolist(),
                               int(key[d][0][tuple(bad[0])]), int(c0[tuple(bad[0])]), len(bad))
        out.append((z, a, e))
    return out


def check_key(o, keys: dict, key, stream: int, s_ntt, w_ntt, digits=None, opened=None):
    """One generated key against the model, word for word: open_key (or its result, `opened`), and c1 == uniform_a of the stream
    word (k << 8) + z in every row of every digit.  Returns [(z, a, e)]."""
    opened = open_key(o, key, s_ntt, w_ntt, digits) if opened is None else opened
    for z, a, _ in opened:
        bad = np.argwhere(a != uniform_a(keys, o.key_primes, o.n, stream_word(stream, z)))
        assert bad.size == 0, ("c1 is not the uniform polynomial of its stream", stream, z, "first at", bad[0].tolist(), len(bad))
    return opened


# ------------------------------------------------------------------------------------------------------- crafted secrets
def key_pattern(o, shift: int = 0) -> np.ndarray:
    """uint64[KK][n]: landing.pattern over the key-level primes."""
    return LD.pattern(o.key_primes, 1, o.n, shift)[0]


def neg_rows(primes, T) -> np.ndarray:
    return np.stack([negmod(T[i], q) for i, q in enumerate(primes)])


def craft_public_secret(o, a, e, T):
    """(s_ntt, c0): (A) the secret whose public key has c0 = -T in every row: s_i = (T_i - e_hat_i) a_i^-1 mod q_i.  a: uint64[KK][n]
    (no zero entry), e: int[n], T: uint64[KK][n]."""
    assert (a != 0).all(), "a has a zero entry: choose another seed"
    eh = error_hat(o, e)
    s = np.zeros_like(a)
    for i, q in enumerate(o.key_primes):
        s[i] = mulmod(addmod(T[i], negmod(eh[i], q), q), invmod(a[i], q), q)
    return s, neg_rows(o.key_primes, T)


def craft_identity_secret(o, a, e, T):
    """(s_ntt, landed): (B) the secret whose Galois key for element 1 (w = s) lands every diagonal row and digit 0's special-prime
    row.  a: uint64[K][KK][n], e: int[K][n] (per digit), T: uint64[KK][n].  Row z < K of the secret serves digit z's own row,
    (f_z - a_zz) s_z - e_hat_zz = T_z with f_z = q_sp mod q_z; the special row serves digit 0's plain branch, -(a s + e_hat) = -T.
    landed: [(digit, row, expected c0 row)]."""
    P = o.key_primes
    K, KK = o.K, o.KK
    s = np.zeros((KK, o.n), dtype=np.uint64)
    landed = []
    for z in range(K):
        q = P[z]
        eh = o.ntt(z, residues(e[z], [q])[0])
        d = addmod(np.uint64(special_factor(P, z)), negmod(a[z][z], q), q)
        assert (a[z][z] != 0).all() and (d != 0).all(), "a or f - a has a zero entry: choose another seed"
        s[z] = mulmod(addmod(T[z], eh, q), invmod(d, q), q)
        landed.append((z, z, np.array(T[z], dtype=np.uint64)))
    q = P[KK - 1]
    eh = o.ntt(KK - 1, residues(e[0], [q])[0])
    assert (a[0][KK - 1] != 0).all(), "a has a zero entry: choose another seed"
    s[KK - 1] = mulmod(addmod(T[KK - 1], negmod(eh, q), q), invmod(a[0][KK - 1], q), q)
    landed.append((0, KK - 1, negmod(T[KK - 1], q)))
    return s, landed


SIGN_FLIP_ELEMENTS = lambda n: (3, 2 * n - 1, n + 1)  # noqa: E731


def pattern_secret(o):
    """(s_coeff, s_ntt) uint64[KK][n]: (C) the secret whose COEFFICIENT form is the five-target pattern in every row."""
    s_coeff = key_pattern(o)
    return s_coeff, ntt_rows(o, s_coeff)


def flipped_zeros(o, s_coeff, elt: int) -> list[int]:
    """Per row: how many coefficients of sigma_elt(s) are a sign-flipped 0 (index arithmetic alone, no oracle)."""
    n = o.n
    k = np.arange(n, dtype=np.int64)
    flipped = ((k * elt) // n) % 2 == 1
    return [int(((np.asarray(s_coeff[i]) == 0) & flipped).sum()) for i in range(len(s_coeff))]


def target_shares(row, q: int) -> list[float]:
    """The share of each of the five targets among the words of `row`."""
    row = np.asarray(row, dtype=np.uint64)
    return [float((row == np.uint64(v)).mean()) for v in LD.targets(q)]


# ------------------------------------------------------------------------------------------ what the GPU tests generate
GEN_SEED = 0x6B65796D6F64            # section 2: one generator per parameter set
CRAFT_SEEDS = {"A": 0xC0A5, "B": 0xC0B5, "C": 0xC0C5}  # section 3
ENC_SEED512 = [0x243F6A8885A308D3, 0x13198A2E03707344, 0xA4093822299F31D0, 0x082EFA98EC4E6C89,
               0x452821E638D01377, 0xBE5466CF34E90C6C, 0xC0AC29B7C97C50DD, 0x3F84D5B5B5470917]  # section 4
SINGLE = "default_2048_14"
GEN_SETS = [SINGLE, "P1", "P2", "U1024", "W2048", "P4", "P6"]
CRAFT_SETS = ["P1", "P2", "U1024", "W2048"]
ENC_SETS = ["P1", "U1024"]


GALOIS_NAMES = ["g3", "g3inv", "g2n-1", "gn+1", "g1"]


def galois_elements(n: int) -> list[int]:
    return [3, pow(3, -1, 2 * n), 2 * n - 1, n + 1, 1]


def key_plan(pid: str, n: int | None = None) -> list:
    """[(name, kind, Galois element)] in creation order: the k-th entry (from 1) is stream k.  The single-prime set has no
    key-switching keys; at n = 32768 the public key and the relinearization key are made alone.  (Without n: the names alone.)"""
    if pid == SINGLE:
        return [("pk", "public", None)]
    if pid == "P6":
        return [("pk", "public", None), ("rk", "relin", None)]
    elts = galois_elements(n) if n else [None] * len(GALOIS_NAMES)
    return ([("pk", "public", None), ("rk", "relin", None)] + [(g, "galois", e) for g, e in zip(GALOIS_NAMES, elts)]
            + [("pk2", "public", None)])


def checked_digits(pid: str, K: int, kind: str) -> list[int]:
    if kind == "public":
        return [0]
    return [0, K - 1] if pid == "P6" else list(range(K))
