"""Crafted operands and integer models for the kernels either side of the evaluator: the public-key encryption's divide-and-round
and plaintext addition (encrypt_finish_kernel on the fused route; add_key_level_kernel -> ks_moddown_kernel -> add_plain on the
component-returning route) and the CRT export (crt_compose_kernel, crt_decompose_kernel).  The method is tests/landing.py's: choose
what the kernel's OWN output must be in every thread and solve for the operand that gives it.

Encryption.  The sampled u and e depend on (seed, counter, coefficient) alone, never on the key, and the public key is the caller's.
Once u and e are known, pk_c = NTT(T_c - e_c) / NTT(u) pointwise in every key-level residue makes pk_c (*) u + e_c = T_c for any
target T_c (the host checks that NTT(u) has no zero entry).  u is recomputed from tests/rng_ref.py; e is HARVESTED from the
component-returning call on the device (the Gaussian is float arithmetic -- logf, cospif: tests/test_gpu_keygen_model.py holds it
against a float64 model; what is asserted of e HERE is |e| <= 19, the sampler's clip, and that every residue row holds the same
small integer).  Given u and e the encryption is stated twice in Python integers: finish_rns, SEAL's divide_and_round_q_last residue by
residue followed by + (Delta mod q_j) m + r, and finish_integers, floor((X + floor(q_sp / 2)) / q_sp) mod q_j of the CRT lift X.
The two share nothing but the key-level residues.

CRT export.  The compose kernel's y_i = x_i (q / q_i)^-1 mod q_i are a bijection of the residues row by row: y is chosen, x solved
for.  A consequence: the exact sum of y_i (q / q_i) is a multiple of q only when every y_i is 0, so the kernel's "equal counts as
>=" branch cannot be reached by any input (compose_model's variant "gt" shows it on every crafted and random value).  The decompose
kernel only ever sees limbs that the compose kernel produced (the API hands it nothing else): it is checked on canonical values
in [0, q) only.

Test infrastructure, CPU only: imports the oracle, numpy and tests/rng_ref.py, never the library under test."""
from __future__ import annotations

import numpy as np

from oracle import bfv_oracle as O
from tests import landing as LD
from tests import rng_ref
from tests.landing import _obj, _u64

E_BOUND = 19                      # the Gaussian sampler's clip
SEEDS = [0x0C1E57, 0x0C1E58]      # the 64-bit test seeds of the landed encryptions; NTT(u) has no zero for them (asserted)
SINGLE = "default_2048_14"        # one prime: no special prime, K = KK = 1
EXTRA_SETS = {SINGLE: lambda: (2048, O.bfv_default(2048), O.plain_batching(2048, 14))}
ENCRYPT_SETS = ["P1", "P2", "W4096", "U1024", "P4", "P6", SINGLE]
CRT_SETS = [SINGLE, "P1", "W2048", "U1024", "P4", "P6"]  # K = 1, 2, 3 (60-bit), 4, 8, 15
CRT_LOWER_SETS = ["P1", "U1024"]


class ClientLanding(LD.Landing):
    """landing.Landing plus the key level's constants; also made for the single-prime set, which landing.SETS does not hold."""

    def __init__(self, pid: str, t: int | None = None):
        if pid in LD.SETS:
            super().__init__(pid, t)
        else:
            n, primes, t0 = EXTRA_SETS[pid]()
            self.pid, self.n, self.key_primes, self.t = pid, n, [int(p) for p in primes], int(t if t is not None else t0)
            self.o = O.Oracle(n, self.key_primes, self.t)
            self.primes, self.K = self.o.primes, self.o.K
            self.Q = LD._product(self.primes)
            self._keys, self._gk, self._cache = None, {}, {}
        self.KK = self.o.KK
        self.qsp = self.key_primes[-1] if self.KK > 1 else None
        self.h = self.qsp // 2 if self.KK > 1 else None


_CLIENTS: dict = {}


def client(pid: str, t: int | None = None) -> ClientLanding:
    if (pid, t) not in _CLIENTS:
        _CLIENTS[(pid, t)] = ClientLanding(pid, t)
    return _CLIENTS[(pid, t)]


def drop_clients() -> None:
    _CLIENTS.clear()


# ------------------------------------------------------------------------------------------------------------ the sampler
def recompute_u(seed: int, n: int, gop: int) -> np.ndarray:
    """int64[n]: the ternary u of encryption number `gop` under the 64-bit test seed: ((w0 * 3) >> 32) - 1, w0 = word 0 of
    ChaCha20_block(secret key of the seed, (coefficient, gop low word, gop high word, domain 0))."""
    key = rng_ref.seed_from_u64_for_tests(seed)["secret"]
    w0 = rng_ref.chacha20_block(key, np.arange(n), gop & 0xFFFFFFFF, gop >> 32, 0)[0]
    return ((w0 * np.uint64(3)) >> np.uint64(32)).astype(np.int64) - 1


def small_from_rows(rows, primes) -> np.ndarray:
    """int64[n]: the one small integer polynomial behind residue rows uint64[K][n] (centred; every row must give the same)."""
    out = None
    for row, q in zip(rows, primes):
        v = _obj(row)
        v = np.where(v > q // 2, v - q, v).astype(np.int64)
        assert out is None or (v == out).all(), "the residue rows do not hold one small polynomial"
        out = v
    return out


def small_rows(v, primes) -> np.ndarray:
    """uint64[len(primes)][n]: the residues of the small integers v."""
    return _u64(np.stack([_obj(v) % int(q) for q in primes]))


def synthetic_e(rng, n: int) -> np.ndarray:
    """int64[2][n] uniform in [-19, 19]: stands in for the harvested errors where there is no device (every value of the clip's
    range, the two ends included, far more often than the Gaussian gives them)."""
    return rng.integers(-E_BOUND, E_BOUND + 1, (2, n)).astype(np.int64)


# ------------------------------------------------------------------------------------------------ A: the two integer models
def _mulmod(a, b, q: int) -> np.ndarray:
    return _u64((_obj(a) * _obj(b)) % q)


def ntt_of_u(L: ClientLanding, u) -> np.ndarray:
    """uint64[KK][n]: NTT(u) in every key-level residue."""
    return np.stack([L.o.ntt(i, small_rows(u, [q])[0]) for i, q in enumerate(L.key_primes)])


def key_level_values(L: ClientLanding, pk, u, e) -> np.ndarray:
    """uint64[2][KK][n]: x_c = pk_c (*) u + e_c per key-level residue (pk: uint64[2][KK][n] in NTT form; u int[n]; e int[2][n]); the
    negacyclic product through the oracle's transforms."""
    un = ntt_of_u(L, u)
    out = np.zeros((2, L.KK, L.n), dtype=np.uint64)
    for i, q in enumerate(L.key_primes):
        for c in range(2):
            x = L.o.ntt(i, _mulmod(pk[c][i], un[i], q), inverse=True)
            out[c, i] = _u64((_obj(x) + _obj(e[c])) % q)
    return out


def scaling_remainder(L: ClientLanding, m) -> np.ndarray:
    """object[n]: r = floor(((q mod t) m + floor((t + 1) / 2)) / t)."""
    return ((L.Q % L.t) * _obj(m) + (L.t + 1) // 2) // L.t


def plain_term(L: ClientLanding, m) -> np.ndarray:
    """uint64[K][n]: (Delta mod q_j) m + r mod q_j, Delta = floor(q / t)."""
    r = scaling_remainder(L, m)
    return _u64(np.stack([((L.Q // L.t) % q * _obj(m) + r) % q for q in L.primes]))


def _moddown_correction(L: ClientLanding, sp_row, j: int, variant: str | None):
    """What divide_and_round_q_last subtracts from data row j before the product by q_sp^-1: ((x_sp + h) mod q_sp) mod q_j - h mod q_j.
    `variant` names a deliberately wrong restatement (the mutations tests/test_client_landing_cpu.py holds the crafted inputs
    against): "no_half" leaves + h out of the special-prime row, "truncate" leaves h out altogether, "no_wrap" does not reduce
    x_sp + h mod q_sp."""
    qsp, h, qj = L.qsp, L.h, L.primes[j]
    sp = _obj(sp_row)
    if variant == "no_half":
        return (sp % qj - h % qj) % qj
    if variant == "truncate":
        return sp % qj
    if variant == "no_wrap":
        return ((sp + h) % qj - h % qj) % qj
    return (((sp + h) % qsp) % qj - h % qj) % qj


def _divide_row(L: ClientLanding, x_row, sp_row, j: int, variant: str | None):
    qsp, h, qj = L.qsp, L.h, L.primes[j]
    inv = pow(qsp, -1, qj)
    if variant == "no_reduce64":
        # the kernel's conditional modular subtractions on 64-bit words with tl NOT reduced mod q_j first (tl may exceed q_j where
        # q_sp > q_j): a - b, or a + q_j - b wrapped to 64 bits where a < b; the last product reduced as it is in the kernel
        mask = (1 << 64) - 1
        tl = (_obj(sp_row) + h) % qsp
        hq = h % qj
        tk = np.where(tl >= hq, tl - hq, (tl + qj - hq) & mask)
        d = _obj(x_row)
        d = np.where(d >= tk, d - tk, (d + qj - tk) & mask)
        return d * inv % qj
    return (_obj(x_row) - _moddown_correction(L, sp_row, j, variant)) * inv % qj


def no_reduce64_applies(L: ClientLanding) -> bool:
    """The mutation "no_reduce64" changes a word only where the unreduced tl makes a 64-bit subtraction wrap: with the data word at
    0 and tl at q_sp - 1 (both crafted) that is q_sp - 1 - (h mod q_j) > q_j for some data prime.  Where the special prime is
    above a data prime by less, every intermediate stays congruent and the final reduction hides the mutation: it does not apply."""
    return L.KK > 1 and any(L.qsp - 1 - L.h % q > q for q in L.primes)


def finish_rns(L: ClientLanding, x, m, variant: str | None = None):
    """Model (i), SEAL's RNS steps: (divided uint64[2][K][n], out uint64[2][K][n]) from the key-level values x uint64[2][KK][n] and
    the plaintext m uint64[n].  `divided` is the result of divide_and_round_q_last (x itself where there is no special prime);
    `out` adds (Delta mod q_j) m + r to polynomial 0.  (The mutations "truncate" and "no_wrap" are one function: (x_sp + h) mod q_j
    - h mod q_j is x_sp mod q_j whether or not x_sp + h was reduced mod q_sp first.  "add_gt" is the plaintext addition's
    conditional subtraction with '>' for '>=': a sum of exactly q_j stays q_j.)"""
    if L.KK == 1:
        divided = np.array(x[:, : L.K], dtype=np.uint64)
    else:
        moddown = None if variant == "add_gt" else variant
        divided = _u64(np.stack([np.stack([_divide_row(L, x[c][j], x[c][L.KK - 1], j, moddown) for j in range(L.K)]) for c in range(2)]))
    out = divided.copy()
    out[0] = LD.lin_mod(L.primes, [(1, divided[0]), (1, plain_term(L, m))])
    if variant == "add_gt":
        for j, q in enumerate(L.primes):
            out[0, j][(divided[0, j] != 0) & (out[0, j] == 0)] = q
    return divided, out


def ordinary_keys(L: ClientLanding):
    """(sk, pk): an ordinary oracle key pair, made once (no relinearization key: nothing here multiplies)."""

    def make():
        O.seed(0xC11E + L.n)
        return L.o.keygen(relin=False)[:2]

    return L.cached("ordinary keys", make)


def crt_lift(primes, rows) -> np.ndarray:
    """object[n]: the integer in [0, prod primes) with the given residues."""
    P = LD._product(primes)
    acc = 0
    for q, row in zip(primes, rows):
        q = int(q)
        acc = acc + (_obj(row) * pow(P // q, -1, q) % q) * (P // q)
    return acc % P


def finish_integers(L: ClientLanding, x, m) -> np.ndarray:
    """Model (ii), over Z: uint64[2][K][n], floor((X + floor(q_sp / 2)) / q_sp) mod q_j with X the CRT lift of the key-level residues
    into [0, Q q_sp); then + Delta m + r on polynomial 0, as integers."""
    add0 = (L.Q // L.t) * _obj(m) + scaling_remainder(L, m)
    out = []
    for c in range(2):
        X = crt_lift(L.key_primes, x[c])
        W = (X + L.h) // L.qsp if L.KK > 1 else X
        if c == 0:
            W = W + add0
        out.append(np.stack([W % q for q in L.primes]))
    return _u64(np.stack(out))


def encrypt_model(L: ClientLanding, pk, u, e, m):
    """(x, divided, out): both models of the encryption of m under pk with the sampled u and e; asserts that they agree on every
    word before anything is compared with it."""
    x = key_level_values(L, pk, u, e)
    divided, out = finish_rns(L, x, m)
    assert (out == finish_integers(L, x, m)).all(), "the two integer models of the encryption disagree"
    return x, divided, out


# ---------------------------------------------------------------------------------------------------- B: landed encryptions
def sp_values(L: ClientLanding) -> list[int]:
    """The special-prime residues both sides of the + h wrap (q_sp = 2 h + 1: x + h reaches q_sp at x = h + 1)."""
    h = L.h
    return [0, 1, h - 1, h, h + 1, h + 2, L.qsp - 1]


# data classes of a coefficient (with a special prime): 0-4 the five targets in the data rows BEFORE the division (the phase moved
# by 2 per row), 5 every data row at q_j - 1, 6-8 the word AFTER the division at 0 / q_j - 1 / 1, 9-10 polynomial 0's word after the
# plaintext addition at 0 / q_j - 1 (polynomial 1: after the division at (q_j -+ 1) / 2), 11 random residues.  Without a special
# prime the key-level value IS the word before the plaintext addition: classes 6-11 alone (numbered 0-5 there).
CLASSES_SPECIAL = 12
CLASSES_SINGLE = 6
PLAIN_CYCLE = 5


def plain_values(t: int) -> list[int]:
    return [0, 1, t - 1, t // 2, -(-t // 2)]


def class_counts(L: ClientLanding) -> tuple[int, int]:
    return (len(sp_values(L)), CLASSES_SPECIAL) if L.KK > 1 else (1, CLASSES_SINGLE)


def class_indices(L: ClientLanding, shift: int = 0):
    """(a, b, p): int[n] each -- the special-prime value, the data class and the plaintext value of every coefficient, as the digits
    of a mixed-radix count of the coefficients, so that every combination occurs (7 * 12 * 5 = 420 <= n)."""
    ns, nd = class_counts(L)
    assert ns * nd * PLAIN_CYCLE <= L.n
    k = np.arange(L.n)
    return (k + shift) % ns, (k // ns + shift) % nd, (k // (ns * nd) + shift) % PLAIN_CYCLE


def plain_cycle(L: ClientLanding, shift: int = 0) -> np.ndarray:
    """uint64[n]: plaintext COEFFICIENTS cycling 0, 1, t - 1, floor(t / 2), ceil(t / 2) in step with class_indices."""
    return np.array(plain_values(L.t), dtype=np.uint64)[class_indices(L, shift)[2]]


def encrypt_targets(L: ClientLanding, m, shift: int = 0) -> np.ndarray:
    """uint64[2][KK][n]: the key-level values T_c = pk_c (*) u + e_c that put every class of class_indices in front of the
    encryption's last steps.  Depends on the plaintext (the classes after the plaintext addition), not on u or e."""
    n, KK = L.n, L.KK
    a, b, _ = class_indices(L, shift)
    if KK == 1:
        b = b + 6  # (the classes after the division alone)
    rng = L.rng(900 + shift)
    T = LD.random_residues(rng, L.key_primes, (2,), n).astype(object)
    pt = _obj(plain_term(L, m))
    for c in range(2):
        sp = None
        if KK > 1:
            sp = np.array(sp_values(L), dtype=object)[(a + 3 * c) % len(sp_values(L))]
            T[c, KK - 1] = sp
        for j, q in enumerate(L.primes):
            tg = np.array(LD.targets(q), dtype=object)
            row = T[c, j]
            pre = b < 5
            row[pre] = tg[(b[pre] + 2 * j + c) % 5]
            row[b == 5] = q - 1
            # the word after the division (before the plaintext addition) that the classes 6-10 ask for
            want = np.zeros(n, dtype=object)
            want[b == 7] = q - 1
            want[b == 8] = 1
            if c == 0:
                want[b == 9] = (0 - pt[j][b == 9]) % q
                want[b == 10] = (q - 1 - pt[j][b == 10]) % q
            else:
                want[b == 9] = (q - 1) // 2
                want[b == 10] = (q + 1) // 2
            solved = (b >= 6) & (b <= 10)
            if KK > 1:
                x = (want * L.qsp + _moddown_correction(L, sp, j, None)) % q
            else:
                x = want
            row[solved] = x[solved]
    return _u64(T)


def craft_public_key(L: ClientLanding, T, u, e) -> np.ndarray:
    """uint64[2][KK][n], NTT form: pk_c = NTT(T_c - e_c) / NTT(u) pointwise in every key-level residue."""
    un = ntt_of_u(L, u)
    assert (un != 0).all(), "NTT(u) has a zero entry: choose another seed"
    pk = np.zeros((2, L.KK, L.n), dtype=np.uint64)
    for i, q in enumerate(L.key_primes):
        inv = np.array([pow(v, -1, q) for v in un[i].tolist()], dtype=object)
        for c in range(2):
            tn = L.o.ntt(i, _u64((_obj(T[c][i]) - _obj(e[c])) % q))
            pk[c, i] = _u64(_obj(tn) * inv % q)
    return pk


def assert_classes_occur(L: ClientLanding, x, divided, out, m) -> None:
    """Every pattern class occurs in every residue row of both polynomials -- read off the REFERENCE's values alone."""
    has = lambda row, v: bool((row == np.uint64(v)).any())  # noqa: E731
    for v in set(plain_values(L.t)):
        assert has(m, v), ("plaintext value", v)
    for c in range(2):
        if L.KK > 1:
            for v in sp_values(L):
                assert has(x[c][L.KK - 1], v), ("special-prime residue", c, v)
            allmax = np.ones(L.n, dtype=bool)
            for j, q in enumerate(L.primes):
                for v in LD.targets(q):
                    assert has(x[c][j], v), ("data residue before the division", c, j, v)
                allmax &= x[c][j] == np.uint64(q - 1)
            assert allmax.any(), ("every data row at q - 1 in one coefficient", c)
        for j, q in enumerate(L.primes):
            for v in (0, q - 1, 1):
                assert has(divided[c][j], v), ("word after the division", c, j, v)
        if c == 0:
            for j, q in enumerate(L.primes):
                for v in (0, q - 1):
                    assert has(out[0][j], v), ("word after the plaintext addition", j, v)


def landed_words(L: ClientLanding, divided, out, shift: int = 0) -> int:
    """Asserts that every target word is where its class says, coefficient by coefficient; returns how many words were checked."""
    a, b, _ = class_indices(L, shift)
    if L.KK == 1:
        b = b + 6
    count = 0
    for c in range(2):
        for j, q in enumerate(L.primes):
            after = {6: 0, 7: q - 1, 8: 1}
            if c == 1:
                after.update({9: (q - 1) // 2, 10: (q + 1) // 2})
            for cls, v in after.items():
                assert (divided[c][j][b == cls] == np.uint64(v)).all(), (c, j, cls)
                count += int((b == cls).sum())
            if c == 0:
                for cls, v in {9: 0, 10: q - 1}.items():
                    assert (out[0][j][b == cls] == np.uint64(v)).all(), (j, cls)
                    count += int((b == cls).sum())
    return count


def landed_encryption(L: ClientLanding, u, e, shift: int = 0):
    """(pk, m, T, x, divided, out): a plaintext on the cycle, the crafted key for the sampled u and e, and the model's ciphertext.
    The host side of the landing in one place: the key-level values ARE the targets, the two models agree, every class occurs
    and every target word is landed."""
    m = plain_cycle(L, shift)
    T = encrypt_targets(L, m, shift)
    pk = craft_public_key(L, T, u, e)
    x, divided, out = encrypt_model(L, pk, u, e, m)
    assert (x == T).all(), "the crafted key does not put the key-level values on the targets"
    assert_classes_occur(L, x, divided, out, m)
    assert landed_words(L, divided, out, shift) > 0
    return pk, m, T, x, divided, out


# ---------------------------------------------------------------------------------------------------------- D: the CRT export
def crt_constants(primes):
    Q = LD._product(primes)
    punct = [Q // int(q) for q in primes]
    return Q, punct, [pow(p % int(q), -1, int(q)) for p, q in zip(punct, primes)]


def compose_sum(primes, rows) -> np.ndarray:
    """object[n]: the exact sum of y_i (q / q_i), y_i = x_i (q / q_i)^-1 mod q_i -- what the compose kernel accumulates before its
    subtractions; floor(sum / q) in [0, K) is the number of subtractions it needs."""
    Q, punct, inv = crt_constants(primes)
    acc = 0
    for q, row, p, iv in zip(primes, rows, punct, inv):
        acc = acc + (_obj(row) * iv % int(q)) * p
    return acc


def compose_model(primes, rows, variant: str | None = None) -> np.ndarray:
    """object[n]: the CRT value in [0, q).  Variants (mutations): "one_fewer" makes at most K - 2 subtractions, "gt" subtracts
    while the sum is strictly above q, "top_limb" decides the compare by the most significant limb alone (a tie is "less")."""
    Q = LD._product(primes)
    K = len(primes)
    acc = compose_sum(primes, rows)
    if variant is None:
        return acc % Q
    if variant == "one_fewer":
        return acc - np.minimum(acc // Q, max(K - 2, 0)) * Q
    out = []
    for v in acc:
        for _ in range(K):
            if variant == "gt":
                ge = v > Q
            else:
                ge = (v >> (64 * K)) != 0 or (v >> (64 * (K - 1))) > (Q >> (64 * (K - 1)))
            if not ge:
                break
            v -= Q
        out.append(v)
    return np.array(out, dtype=object)


def limbs_of(values, K: int) -> np.ndarray:
    """uint64[n][K], least significant limb first."""
    mask = (1 << 64) - 1
    return _u64(np.stack([(_obj(values) >> (64 * l)) & mask for l in range(K)], axis=-1))


def crt_case_list(primes, rng):
    """[(name, residues: K integers, expected value or None, subtractions or None)]: the y vectors and the direct values."""
    P = [int(q) for q in primes]
    K = len(P)
    Q, punct, inv = crt_constants(P)
    cases = []

    def from_y(name, y, s=None):
        cases.append((name, [yi * p % q for yi, p, q in zip(y, punct, P)], sum(yi * p for yi, p in zip(y, punct)) % Q, s))

    from_y("every y at q_i - 1", [q - 1 for q in P], K - 1)
    from_y("every y at 0", [0] * K, 0)
    for i in range(K):
        from_y(f"y_{i} = 1 alone", [int(k == i) for k in range(K)], 0)
    for s in range(K):
        # sum y_i / q_i = s + 1 / 2: the same share in every row, and shares moved by a zero-sum jitter below 0.4 / K
        from_y(f"{s} subtractions, even shares", [q * (2 * s + 1) // (2 * K) for q in P], s)
        jit = rng.uniform(-0.4, 0.4, K)
        jit -= jit.mean()
        from_y(f"{s} subtractions, uneven shares", [int(q * ((s + 0.5) / K + j / K)) for q, j in zip(P, jit)], s)
    direct = [("1", 1), ("q - 1", Q - 1), ("floor(q / 2)", Q // 2), ("floor(q / 2) + 1", Q // 2 + 1)]
    k = 0
    while (1 << (64 * k)) < Q:
        direct += [(f"2^{64 * k} - 1", (1 << (64 * k)) - 1), (f"2^{64 * k}", 1 << (64 * k)), (f"2^{64 * k} + 1", (1 << (64 * k)) + 1)]
        k += 1
    for name, v in direct:
        v %= Q
        cases.append((name, [v % q for q in P], v, None))
    return cases


def crt_case(primes, n: int, salt: int = 0):
    """(rows uint64[2][K][n], value object[2][n], names, which int[2][n]): the cases of crt_case_list cycled over all coefficients of
    both polynomials (another phase in polynomial 1), half as many random residues after every round of them.  value is the Python
    CRT value in [0, q); which is the case index, -1 for a random coefficient.  Asserts on the host that every case's value is the
    one it names, that every number of subtractions 0 ... K - 1 occurs, and that the residues of value are the rows."""
    P = [int(q) for q in primes]
    K = len(P)
    Q = LD._product(P)
    rng = np.random.default_rng(7000 + 131 * K + n + salt)
    cases = crt_case_list(P, rng)
    period = len(cases) + len(cases) // 2 + 1
    assert period <= n
    rows = LD.random_residues(rng, P, (2,), n)
    which = np.full((2, n), -1, dtype=np.int64)
    table = np.array([c[1] for c in cases], dtype=object)  # [case][K]
    for p in range(2):
        idx = (np.arange(n) + 5 * p) % period
        which[p] = np.where(idx < len(cases), idx, -1)
        sel = which[p] >= 0
        for i in range(K):
            rows[p, i, sel] = _u64(table[which[p][sel], i])
    value = np.stack([compose_model(P, rows[p]) for p in range(2)])
    subs = np.stack([compose_sum(P, rows[p]) // Q for p in range(2)])
    for ci, (name, res, v, s) in enumerate(cases):
        at = which == ci
        assert at.any(), name
        assert (value[at] == v).all(), name
        assert s is None or (subs[at] == s).all(), (name, s)
    assert set(int(s) for s in np.unique(subs)) == set(range(K)) or K == 1, sorted(set(int(s) for s in np.unique(subs)))
    for p in range(2):
        assert (value[p] < Q).all() and (value[p] >= 0).all()
        for i, q in enumerate(P):
            assert (_u64(value[p] % q) == rows[p, i]).all()
    return rows, value, [c[0] for c in cases], which


def subtraction_histogram(primes, rows) -> list[int]:
    """How many coefficients of rows uint64[polys][K][n] need 0, 1, ..., K - 1 subtractions."""
    Q = LD._product(primes)
    subs = np.concatenate([compose_sum(primes, r) // Q for r in rows])
    return [int((subs == s).sum()) for s in range(len(primes))]


def land_mod_switch(L: ClientLanding, T_low, last_rows) -> np.ndarray:
    """uint64[2][K][n]: the ciphertext whose mod_switch_to_next is T_low (uint64[2][K - 1][n]) with last_rows (uint64[2][n]) in its
    last data row: divide_and_round_q_last by q_{K-1}, x_j = T_j q_last + ((x_last + h) mod q_last) mod q_j - h mod q_j solved row
    by row."""
    K = L.K
    ql = L.primes[K - 1]
    h = ql // 2
    ct = np.zeros((2, K, L.n), dtype=np.uint64)
    for c in range(2):
        last = (_obj(last_rows[c]) + h) % ql
        for j, q in enumerate(L.primes[: K - 1]):
            ct[c, j] = _u64((_obj(T_low[c][j]) * ql + last % q - h % q) % q)
        ct[c, K - 1] = last_rows[c]
    return ct


def lower_level_case(L: ClientLanding):
    """(ct uint64[2][K][n], rows uint64[2][K - 1][n], value): the lower level's CRT cases as the mod_switch_to_next of ct, whose
    last data row cycles both sides of the + h wrap."""

    def make():
        low = L.primes[:-1]
        rows, value, names, which = crt_case(low, L.n, salt=1)
        ql = L.primes[-1]
        edge = np.array([0, 1, ql // 2 - 1, ql // 2, ql // 2 + 1, ql // 2 + 2, ql - 1], dtype=np.uint64)
        last = np.stack([edge[(np.arange(L.n) // 3 + c) % 7] for c in range(2)])
        return land_mod_switch(L, rows, last), rows, value

    return L.cached("crt lower", make)
