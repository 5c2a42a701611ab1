"""Operands crafted so that a kernel's OUTPUT lands on an exact edge: 0, q - 1, 1 and the two integers around q / 2.

The kernels that end in a canonicalisation or a modular add (the key-switch tails, the sums folded into the fused multiply +
relinearize, the element-wise, plaintext and n-ary kernels, the product accumulators, the decryption's rounding) see such a result
about once in 2^40 words of random data.  The caller controls what the key-switch output is ADDED TO, so every such edge is
reachable without crafted keys: relinearize(c0, c1, c2) = (c0, c1) + ks(c2), hence (T0 - ks0, T1 - ks1, c2) relinearizes to exactly
T for any target T; a rotation's polynomial 0 is sigma(c0) + ks0(sigma(c1)); a folded sum is mult * m +- z with z a program input.

Test infrastructure, CPU only: imports the oracle and numpy, never the library under test.  All arithmetic on residues is in Python
integers (`object` arrays).  Every builder returns (operands, expected); tests/test_landing_cpu.py shows that the ORACLE maps the
operands to `expected` on every crafted word (a builder that does not land would make the GPU test vacuous), and
tests/test_gpu_landing.py compares the HIP kernels with the oracle on the same operands, word for word.

Values INSIDE the multiply and the decryption are reached through bijections instead (sections F, G, H below).  The extension's
rows y_i = x_i m~ (q / q_i)^-1 mod q_i are a bijection of the caller's x_i row by row, and r_mtilde is a function of the y_i mod 2^32:
the y are chosen and x solved for, one row above 2^32 taking up the target (land_mtilde).  A multiplication by (1, 1) has the tensor
d0 = a0, d1 = a0 + a1, d2 = a1, so the floor's inputs y_i = t d (q / q_i)^-1 mod q_i are again the caller's (land_floor_inputs), and
polynomial 0 (2) of the product is a function of a0[k] (a1[k]) alone: candidates whose product is 0, q_i - 1 or 1 in EVERY row are
harvested from the oracle (land_multiply_output; floor(t D / q) - u' with u' in [0, K) the fast conversion's overflow, so +1 is found
among D near j q / t, and a SMALL D never gives 0 or +1: its u' is at least 1).  The gamma residue of decrypt's rounding is a linear
form of (y_0, y_1) mod gamma: the nearest point of a two-dimensional lattice coset puts it on any target (land_gamma).
tests/test_gpu_landing_multiply.py runs these.  Section I hands the same operands to the prepared-multiplicand products (in both
roles: the oracle's multiply is symmetric) and to the weighted sums, with weight vectors chosen so that the sums of weighted residues
pass through exactly q_i and q_i - 1 and end on 0, q_i - 1 and 1 (weighted_sum_case); tests/test_gpu_landing_shared.py runs those, and tests/test_gpu_landing_prepared_pair.py hands the operands of
F, G and I to the products of TWO prepared operands.

Section J lands SUMS of rotations, sum_t w_t rotate(a_t, s_t) (tests/test_gpu_landing_rotate_sum.py runs them).  The caller owns c0
of every rotated term and both polynomials of every identity term (step 0), and the key-switch part of a rotated term does not
depend on its c0: every finished term's polynomial 0 is reachable (the edges in front of the mod-down's last reduction and of the
weighting product), and so is every PARTIAL sum of polynomial 0, term after term, by solving the term's residue from the target and
the sum so far, row by row (a row where w = 0 mod q_i has no inverse: the term adds 0 there and the target is the sum before it).
Through an identity term the sum's polynomial 1 is reachable too: on the pattern after each identity term, on all zeros (a
transparent sum) and on all zeros but one word.  land_rotation generalises land_galois to whatever rotation the oracle performs, a
NAF chain over power-of-two keys included: c0 enters a chain of key switches by permutation and addition alone.

What the method cannot reach: polynomial 1 of a stand-alone key switch or of a single rotated term (it is ks1 alone: in a sum of
rotations it is reached only through the sum, by an identity term), polynomial 1 of a product by
(1, 1) (a0 + a1 is not free once a0 and a1 are spent; it is compared all the same), and alpha_sk's own branch in the
Shenoy-Kumaresan step (alpha is a small integer far from m_sk / 2 in any valid run)."""
from __future__ import annotations

import numpy as np

from oracle import bfv_oracle as O


# ----------------------------------------------------------------------------------------------------------------- targets
def targets(q: int) -> list[int]:
    return [0, q - 1, 1, (q - 1) // 2, (q + 1) // 2]


def pattern(primes, polys: int, n: int, shift: int = 0) -> np.ndarray:
    """uint64[polys][K][n]: the five targets cycled over the coefficients, the phase moved by 2 per residue row and by 3 per
    polynomial.  n / 4 and n / 8 are powers of two, never a multiple of 5: the four coefficients {t + k n / 4} of one tail thread
    see four different targets and the eight {t + k n / 8} of one head thread all five."""
    j = np.arange(n)
    out = np.zeros((polys, len(primes), n), dtype=np.uint64)
    for p in range(polys):
        for i, q in enumerate(primes):
            out[p, i] = np.array(targets(q), dtype=np.uint64)[(j + shift + 2 * i + 3 * p) % 5]
    return out


def constant(primes, n: int, value) -> np.ndarray:
    """uint64[K][n]: `value` (an integer, or a function of q) in every word of one polynomial."""
    return np.stack([np.full(n, value(q) if callable(value) else value, dtype=np.uint64) for q in primes])


def almost_zero(primes, n: int) -> np.ndarray:
    """uint64[K][n]: 0 everywhere except the LAST word of the LAST residue row, which is 1 -- what a watch that leaves early, or
    that stops one word short, reports transparent."""
    out = np.zeros((len(primes), n), dtype=np.uint64)
    out[-1, -1] = 1
    return out


def cycle(primes, n: int, values) -> np.ndarray:
    """uint64[K][n]: values(q) cycled over the coefficients."""
    j = np.arange(n)
    return np.stack([np.array(values(q), dtype=np.uint64)[(j + i) % len(values(q))] for i, q in enumerate(primes)])


def random_residues(rng, primes, shape_before: tuple, n: int) -> np.ndarray:
    """uint64[*shape_before][K][n] uniform residues."""
    rows = [rng.integers(0, q, shape_before + (n,), dtype=np.uint64) for q in primes]
    return np.ascontiguousarray(np.stack(rows, axis=len(shape_before)))


# ------------------------------------------------------------------------------------------------------- integer arithmetic
def _qcol(primes, ndim: int) -> np.ndarray:
    """The primes as an object array that broadcasts against [..., K, n]."""
    return np.array([int(q) for q in primes], dtype=object).reshape((len(primes), 1))


def _obj(a) -> np.ndarray:
    return np.asarray(a).astype(object)


def _u64(a) -> np.ndarray:
    return np.ascontiguousarray(np.asarray(a).astype(np.uint64))


def lin_mod(primes, terms) -> np.ndarray:
    """sum of coef * array over `terms` = [(coef, uint64[..., K, n]), ...], mod q per residue row, in Python integers."""
    acc = None
    for coef, a in terms:
        a = _obj(a)
        if acc is None:
            acc = a if coef == 1 else int(coef) * a
        elif coef in (1, -1):
            acc = acc + a if coef == 1 else acc - a
        else:
            acc = acc + int(coef) * a
    return _u64(acc % _qcol(primes, 0))


# ---------------------------------------------------------------------------------------------------------------- builders
def land_relinearize(o, rk, c2, T):
    """(ct3, T): relinearize(ct3, rk) == T.  c2: uint64[K][n], T: uint64[2][K][n]."""
    zero = np.zeros_like(c2)
    ks = o.relinearize(np.stack([zero, zero, c2]), rk)
    base = lin_mod(o.primes, [(1, T), (-1, ks)])
    return np.stack([base[0], base[1], c2]), _u64(T)


def land_galois(o, gk, elt: int, c1, T0):
    """(ct2, expected): polynomial 0 of apply_galois(ct2, elt) == T0 (polynomial 1 is the key switch's own: expected[1] is the
    oracle's).  sigma_g(c0) + r0 = T0 with r = apply_galois((0, c1), g), so c0 = sigma_{g^-1}(T0 - r0)."""
    r = o.apply_galois(np.stack([np.zeros_like(c1), c1]), elt, gk)
    ginv = pow(int(elt), -1, 2 * o.n)
    c0 = o.apply_galois_poly(lin_mod(o.primes, [(1, T0), (-1, r[0])]), ginv)
    return np.stack([c0, c1]), np.stack([_u64(T0), r[1]])


def land_addend(o, m, mult: int, sign: int, T):
    """(z, T): mult * m + sign * z == T for the ciphertext m (uint64[2][K][n]); sign is +1 or -1."""
    assert sign in (1, -1)
    return lin_mod(o.primes, [(sign, T), (-sign * mult, m)]), _u64(T)


def land_add(o, x, T):
    """((x, y), T): x + y == T."""
    return (x, lin_mod(o.primes, [(1, T), (-1, x)])), _u64(T)


def land_sub(o, x, T):
    """((x, y), T): x - y == T."""
    return (x, lin_mod(o.primes, [(1, x), (-1, T)])), _u64(T)


def land_plain(o, plain, T0, sub: bool):
    """(c0, T0): polynomial 0 of add_plain / sub_plain((c0, c1), plain) == T0 for any c1.  add_plain of a ciphertext with c0 = 0
    gives the scaled plaintext round(q m / t) residue by residue (the oracle's, not a formula restated here)."""
    probe = np.zeros((2, o.K, o.n), dtype=np.uint64)
    probe[1, :, 0] = 1  # (not transparent)
    scaled = o.add_plain(probe, plain)[0]
    return lin_mod(o.primes, [(1, T0), (1 if sub else -1, scaled)]), _u64(T0)


def land_phase(o, sk, c1, phases):
    """(ct, residues): c0 + c1 s (+ c2 s^2 ...) == phases[k] mod Q in coefficient k.  phases: n integers in [0, Q); c1:
    uint64[K][n], or uint64[size - 1][K][n] for the polynomials 1 ... size - 1 of a larger ciphertext."""
    rest = c1[None] if c1.ndim == 2 else c1
    want = _u64(np.array([[int(x) % q for x in phases] for q in o.primes], dtype=object))
    d = o.dot_with_secret(np.concatenate([np.zeros_like(rest[:1]), rest]), sk)
    return np.concatenate([lin_mod(o.primes, [(1, want), (-1, d)])[None], rest]), want


# ---------------------------------------------------------------------------------------------------------- parameter sets
def _create(n, bits):
    return lambda: (n, O.coeff_modulus_create(n, bits), O.plain_batching(n, 20 if n <= 4096 else 17))


SETS = {
    "P1": lambda: (4096, O.bfv_default(4096), O.plain_batching(4096, 16)),    # K = 2, all FP64, special prime above the data primes
    "P2": lambda: (4096, O.coeff_modulus_create(4096, [40, 38, 36]), O.plain_batching(4096, 16)),  # special prime BELOW a data prime
    "P3": lambda: (8192, O.bfv_default(8192), O.plain_batching(8192, 17)),    # K = 4
    "P4": lambda: (16384, O.bfv_default(16384), O.plain_batching(16384, 17)),  # K = 8, 49-bit primes, per-row packing
    "P5": _create(8192, [54, 54, 54, 56]),                                     # mixed: integer data rows
    "P6": lambda: (32768, O.bfv_default(32768), O.plain_batching(32768, 17)),  # integer key switch
    "U1024": _create(1024, [50, 30, 30, 50, 50]),
    "W2048": _create(2048, [60, 60, 60, 60]),                                  # 60-bit primes, K = 3
    "W4096": _create(4096, [60, 60, 60]),                                      # 60-bit primes, K = 2
    "S4096": _create(4096, [30, 30, 40, 40]),                                  # 30-bit primes at n = 4096: an int32 weight wraps them
    "X8192": _create(8192, [50, 30, 30, 50, 50]),                              # K = 4 with 50-bit data primes: 8-byte FP64 rows
}


class Landing:
    """One parameter set: the oracle, one key pair (made on first use) and the crafted batches of every section, each built once
    per process and shared by the tests that name it.  Nothing here is changed after it is built."""

    def __init__(self, pid: str, t: int | None = None):
        n, primes, t0 = SETS[pid]()
        self.pid, self.n, self.key_primes, self.t = pid, n, [int(p) for p in primes], int(t if t is not None else t0)
        self.o = O.Oracle(n, self.key_primes, self.t)
        self.primes = self.o.primes
        self.K = self.o.K
        self.Q = 1
        for q in self.primes:
            self.Q *= q
        self._keys = None
        self._gk = {}
        self._cache = {}

    # -- keys
    @property
    def keys(self):
        if self._keys is None:
            O.seed(0x1A2D + self.n)
            self._keys = self.o.keygen()[:3]
        return self._keys

    @property
    def sk(self):
        return self.keys[0]

    @property
    def pk(self):
        return self.keys[1]

    @property
    def rk(self):
        return self.keys[2]

    def galois_keys(self, elts) -> dict:
        for e in elts:
            if e not in self._gk:
                key = np.zeros((self.K, 2, self.o.KK, self.n), dtype=np.uint64)
                O.lib().ora_keygen_galois(O.C.c_void_p(self.o._h), O._p(self.sk), O.C.c_uint32(e), O._p(key))
                self._gk[e] = key
        return {e: self._gk[e] for e in elts}

    def rng(self, salt: int):
        return np.random.default_rng(self.n * 131 + salt)

    def cached(self, key, make):
        if key not in self._cache:
            self._cache[key] = make()
        return self._cache[key]

    def fresh(self, rng, count: int) -> np.ndarray:
        """uint64[count][2][K][n]: encryptions of small slot vectors (products of two of them decrypt)."""
        return np.stack([self.o.encrypt(self.pk, self.o.batch_encode(rng.integers(0, 8, self.n).astype(np.uint64))) for _ in range(count)])

    # -- A1 / A2: relinearize
    def relin_items(self):
        """A1: (ct3 uint64[items][3][K][n], expected uint64[items][2][K][n], names); the LAST item is the almost transparent one.
        A2: (ct3 uint64[1][3][K][n], expected) whose output polynomial 1 is 0 everywhere."""

        def make():
            o, rk, P, n = self.o, self.rk, self.primes, self.n
            rng = self.rng(1)
            pat = pattern(P, 2, n, 0)
            plans = [
                ("both polynomials on the pattern", pat),
                ("polynomial 0 all 0", np.stack([constant(P, n, 0), pattern(P, 1, n, 1)[0]])),
                ("polynomial 0 all q - 1", np.stack([constant(P, n, lambda q: q - 1), pattern(P, 1, n, 2)[0]])),
                ("almost transparent", np.stack([pattern(P, 1, n, 3)[0], almost_zero(P, n)])),
            ]
            cts, want, names = [], [], []
            for name, T in plans:
                ct3, exp = land_relinearize(o, rk, random_residues(rng, P, (), n), T)
                cts.append(ct3), want.append(exp), names.append(name)
            if self.n < 32768:  # (n = 32768: four items; random size-3 inputs are the rest of the suite's there)
                ct3 = random_residues(rng, P, (3,), n)
                cts.insert(3, ct3), want.insert(3, o.relinearize(ct3, rk)), names.insert(3, "random control")
            tr, tr_want = land_relinearize(o, rk, random_residues(rng, P, (), n), np.stack([pat[0], constant(P, n, 0)]))
            return (np.stack(cts), np.stack(want), names), (tr[None], tr_want[None])

        return self.cached("relin", make)

    # -- A3 / A4: rotations with direct keys
    def rotation_ops(self):
        """[(name, galois element, step or None)]: apply_galois by an element that is no rotation step's neighbour, rotate_rows by 1
        and by -3, rotate_columns."""
        o = self.o
        return [("apply_galois", 2 * self.n - 5, None), ("rotate_rows +1", o.galois_elt_from_step(1), 1),
                ("rotate_rows -3", o.galois_elt_from_step(-3), -3), ("rotate_columns", 2 * self.n - 1, None)]

    def rotation_items(self, elt: int):
        """(ct2 uint64[5][2][K][n], expected, names) for apply_galois by `elt`: polynomial 0 landed through sigma^-1; the last item's
        c1 cycles 0, q - 1, 1 (zeros and q - 1 under the sign flips of the gathers)."""

        def make():
            o, P, n = self.o, self.primes, self.n
            gk = self.galois_keys([elt])
            rng = self.rng(elt)
            plans = [
                ("polynomial 0 on the pattern", pattern(P, 1, n, elt % 5)[0], None),
                ("polynomial 0 all 0", constant(P, n, 0), None),
                ("polynomial 0 all q - 1", constant(P, n, lambda q: q - 1), None),
                ("c1 cycles 0, q - 1, 1", pattern(P, 1, n, 4)[0], cycle(P, n, lambda q: [0, q - 1, 1])),
            ]
            cts, want, names = [], [], []
            for name, T0, c1 in plans:
                ct, exp = land_galois(o, gk, elt, random_residues(rng, P, (), n) if c1 is None else c1, T0)
                cts.append(ct), want.append(exp), names.append(name)
            ct = random_residues(rng, P, (2,), n)
            cts.insert(3, ct), want.insert(3, o.apply_galois(ct, elt, gk)), names.insert(3, "random control")
            return np.stack(cts), np.stack(want), names

        return self.cached(("rot", elt), make)

    # -- E: decrypt
    def phase_values(self) -> list[int]:
        Q, t = self.Q, self.t
        out = [0, 1, Q - 1, Q // 2, Q // 2 + 1]
        for k in (0, 1, t // 2, t - 1):
            b = -((-(2 * k + 1) * Q) // (2 * t))  # ceil((2 k + 1) Q / (2 t)): where round(t x / Q) steps from k to k + 1
            out += [b - 1, b, b + 1]
        return [v % Q for v in out]

    def phase_items(self, count: int = 4):
        """(ct2 uint64[count][2][K][n], phases: count lists of n integers): random c1, c0 landed so that coefficient k of item i has
        the phase phase_values()[(k + 5 i) % 17]."""

        def make():
            vals = self.phase_values()
            rng = self.rng(7)
            cts, phases = [], []
            for i in range(count):
                ph = [vals[(k + 5 * i) % len(vals)] for k in range(self.n)]
                ct, _ = land_phase(self.o, self.sk, random_residues(rng, self.primes, (), self.n), ph)
                cts.append(ct), phases.append(ph)
            return np.stack(cts), phases

        return self.cached(("phase", count), make)


_LANDINGS: dict = {}


def landing(pid: str, t: int | None = None) -> Landing:
    if (pid, t) not in _LANDINGS:
        _LANDINGS[(pid, t)] = Landing(pid, t)
    return _LANDINGS[(pid, t)]


def drop_landings() -> None:
    _LANDINGS.clear()


class MemoOracle:
    """The oracle with its two expensive calls remembered by their operands' bytes: run_program over a batch whose items share the
    factors of a product (and differ in the crafted addend) multiplies and relinearizes each distinct pair once.  Same calls, same
    results."""

    def __init__(self, o):
        self._o, self._memo = o, {}

    def __getattr__(self, name):
        return getattr(self._o, name)

    def _remember(self, key, make):
        if key not in self._memo:
            self._memo[key] = make()
        return self._memo[key]

    def multiply(self, a, b):
        return self._remember(("mul", a.tobytes(), b.tobytes()), lambda: self._o.multiply(a, b))

    def relinearize(self, ct3, rk):
        return self._remember(("relin", ct3.tobytes(), id(rk)), lambda: self._o.relinearize(ct3, rk))

    def rotate_rows(self, ct, steps, gk):
        return self._remember(("rot", ct.tobytes(), steps), lambda: self._o.rotate_rows(ct, steps, gk))

    def rotate_columns(self, ct, gk):
        return self._remember(("col", ct.tobytes()), lambda: self._o.rotate_columns(ct, gk))


# --------------------------------------------------------------------------------------------------- B: sums folded into tails
FOLDS = [(mult, sign) for mult in (1, 2, 3, 4) for sign in (1, -1)]  # mult * m + sign * z; then m + m alone
DISTINCT = 4  # input sets built per parameter set; a larger batch repeats them


def fold_case(L: Landing):
    """x, y: uint64[DISTINCT][2][K][n] fresh encryptions; m[i] = relinearize(multiply(x[i], y[i])) (the oracle's); z[g]:
    uint64[DISTINCT][2][K][n], the addend of graph g = FOLDS[g] crafted per input set so that the sum is the pattern; T[g] likewise.
    Input set 3 of graph 0 lands polynomial 1 on `almost_zero` (a clean run)."""

    def make():
        o, P, n = L.o, L.primes, L.n
        rng = L.rng(11)
        x, y = L.fresh(rng, DISTINCT), L.fresh(rng, DISTINCT)
        m = np.stack([o.relinearize(o.multiply(x[i], y[i]), L.rk) for i in range(DISTINCT)])
        z, T = [], []
        for g, (mult, sign) in enumerate(FOLDS):
            Tg = np.stack([pattern(P, 2, n, i + 2 * g) for i in range(DISTINCT)])
            if g == 0:
                Tg[3, 1] = almost_zero(P, n)
            zg = np.stack([land_addend(o, m[i], mult, sign, Tg[i])[0] for i in range(DISTINCT)])
            z.append(zg), T.append(Tg)
        return x, y, m, z, T

    return L.cached("fold", make)


def fold_transparent_addend(L: Landing, item: int):
    """The addend of graph 0 (m + z) for input set `item` that lands polynomial 1 of the sum on all zeros."""
    x, y, m, z, T = fold_case(L)
    target = np.stack([T[0][item][0], constant(L.primes, L.n, 0)])
    return land_addend(L.o, m[item], 1, 1, target)[0]


ROT_STEP = 1


def rotsum_case(L: Landing):
    """x: uint64[DISTINCT][2][K][n] random residues; z_rot / z_swap: the addends that land rotate_left(x, ROT_STEP) + z and
    swap_rows(x) + z on the pattern (both polynomials); gk: the two direct keys.  Input set 3 of the rotation lands polynomial 1 on
    `almost_zero`."""

    def make():
        o, P, n = L.o, L.primes, L.n
        elts = [o.galois_elt_from_step(ROT_STEP), 2 * n - 1]
        gk = L.galois_keys(elts)
        rng = L.rng(12)
        x = random_residues(rng, P, (DISTINCT, 2), n)
        T_rot = np.stack([pattern(P, 2, n, i + 1) for i in range(DISTINCT)])
        T_rot[3, 1] = almost_zero(P, n)
        T_swap = np.stack([pattern(P, 2, n, i + 3) for i in range(DISTINCT)])
        r = [o.rotate_rows(x[i], ROT_STEP, gk) for i in range(DISTINCT)]
        c = [o.rotate_columns(x[i], gk) for i in range(DISTINCT)]
        z_rot = np.stack([land_addend(o, r[i], 1, 1, T_rot[i])[0] for i in range(DISTINCT)])
        z_swap = np.stack([land_addend(o, c[i], 1, 1, T_swap[i])[0] for i in range(DISTINCT)])
        return x, gk, z_rot, z_swap, T_rot, T_swap, r

    return L.cached("rotsum", make)


def rotsum_transparent_addend(L: Landing, item: int):
    x, gk, z_rot, z_swap, T_rot, T_swap, r = rotsum_case(L)
    return land_addend(L.o, r[item], 1, 1, np.stack([T_rot[item][0], constant(L.primes, L.n, 0)]))[0]


# ------------------------------------------------------------------------------- C: element-wise, plaintext and n-ary kernels
def addsub_case(L: Landing, size: int, items: int = 5):
    """(x, y_add, y_sub, T): uint64[items][size][K][n]; x + y_add == T and x - y_sub == T, T the pattern (item i shifted by i);
    item 1 of x is q - 1 everywhere, item 2 is 0 everywhere."""

    def make():
        P, n = L.primes, L.n
        x = random_residues(L.rng(20 + size), P, (items, size), n)
        x[1] = np.stack([constant(P, n, lambda q: q - 1)] * size)
        x[2] = 0
        T = np.stack([pattern(P, size, n, i) for i in range(items)])
        return x, land_add(L.o, x, T)[0][1], land_sub(L.o, x, T)[0][1], T

    return L.cached(("addsub", size, items), make)


def negate_case(L: Landing):
    """uint64[3][2][K][n]: ciphertexts holding 0, 1 and q - 1 in three phases."""
    P, n = L.primes, L.n
    vals = [lambda q: [0, 1, q - 1], lambda q: [1, q - 1, 0], lambda q: [q - 1, 0, 1, 0, 0]]
    return np.stack([np.stack([cycle(P, n, v), cycle(P, n, v)[:, ::-1]]) for v in vals])


def plain_edge_values(t: int) -> list[int]:
    return [0, 1, t - 1, (t - 1) // 2, -(-t // 2)]


def plain_case(L: Landing, sub: bool, shared: bool, items: int = 4):
    """(ct uint64[items][2][K][n], plain uint64[items][n] or uint64[n], T0 uint64[items][K][n]): polynomial 0 of add_plain /
    sub_plain(ct, plain) == T0.  The plaintexts cycle plain_edge_values(t) in their first half and are random in the second."""

    def make():
        P, n, t = L.primes, L.n, L.t
        rng = L.rng(30 + 2 * sub + shared)
        edge = np.array(plain_edge_values(t), dtype=np.uint64)

        def one(i):
            p = rng.integers(0, t, n, dtype=np.uint64)
            p[: n // 2] = edge[(np.arange(n // 2) + i) % 5]
            return p

        plain = one(0) if shared else np.stack([one(i) for i in range(items)])
        c1 = random_residues(rng, P, (items,), n)
        T0 = np.stack([pattern(P, 1, n, 2 * i + 1)[0] for i in range(items)])
        c0 = np.stack([land_plain(L.o, plain if shared else plain[i], T0[i], sub)[0] for i in range(items)])
        return np.ascontiguousarray(np.stack([c0, c1], axis=1)), plain, T0

    return L.cached(("plain", sub, shared, items), make)


def monomials(L: Landing) -> list[np.ndarray]:
    """The twelve plaintexts c x^e, e in {0, 1, n - 1}, c in {1, t - 1, floor((t - 1) / 2), ceil(t / 2)}."""
    out = []
    for e in (0, 1, L.n - 1):
        for c in plain_edge_values(L.t)[1:]:
            p = np.zeros(L.n, dtype=np.uint64)
            p[e] = c
            out.append(p)
    return out


def mono_case(L: Landing):
    """uint64[4][2][K][n]: residues 0 and q - 1 on both sides of the wrap (coefficients 0, 1, n - 2, n - 1) in every combination
    over the items, 0 / q - 1 / 1 cycled in between for three items, random for the fourth."""

    def make():
        P, n = L.primes, L.n
        ct = np.stack([np.stack([cycle(P, n, lambda q: [0, q - 1, 1]), cycle(P, n, lambda q: [q - 1, 0, (q - 1) // 2, 0])])] * 3
                      + [random_residues(L.rng(40), P, (2,), n)])
        qm1 = np.array(P, dtype=np.uint64) - 1
        for i in range(4):
            for pos, bit in ((0, 1), (1, 2), (n - 2, 4), (n - 1, 8)):
                ct[i, :, :, pos] = qm1[None, :] if ((i + 1) * 5) & bit else 0
        return ct

    return L.cached("mono", make)


def nary_case(L: Landing, items: int = 4):
    """inputs: five uint64[items][2][K][n]; ((((-a) + b) - c) + d) + e == T with e crafted from the oracle's partial sum."""

    def make():
        o, P, n = L.o, L.primes, L.n
        a, b, c, d = (random_residues(L.rng(50 + k), P, (items, 2), n) for k in range(4))
        T = np.stack([pattern(P, 2, n, i + 2) for i in range(items)])
        part = np.stack([o.add(o.sub(o.add(o.negate(a[i]), b[i]), c[i]), d[i]) for i in range(items)])
        return [a, b, c, d, land_add(o, part, T)[0][1]], T

    return L.cached(("nary", items), make)


# --------------------------------------------------------------------------------------------- D: PIR product accumulators
def dot_sums(primes, ctn, pntt) -> np.ndarray:
    """uint64[rows][2][K][n]: sum_j ctn[j] * pntt[r][j] mod q, word by word in Python integers (the transform domain: no transform)."""
    ct = _obj(ctn)
    qc = _qcol(primes, 0)
    rows = []
    for r in range(pntt.shape[0]):
        acc = (ct * _obj(pntt[r])[:, None]).sum(axis=0)
        rows.append(acc % qc)
    return _u64(np.stack(rows))


def dot_reference(o, ctn, pntt) -> np.ndarray:
    """dot_sums followed by the oracle's inverse transform of every residue polynomial."""
    s = dot_sums(o.primes, ctn, pntt)
    out = np.zeros_like(s)
    for r in range(s.shape[0]):
        for p in range(2):
            for i in range(o.K):
                out[r, p, i] = o.ntt(i, s[r, p, i], inverse=True)
    return out


def dot_targets(primes, rows: int, n: int) -> np.ndarray:
    """uint64[rows][K][n]: row r lands on 0 (r % 3 == 0), on q - 1 (r % 3 == 1), on the pattern (r % 3 == 2)."""
    kinds = [lambda r: constant(primes, n, 0), lambda r: constant(primes, n, lambda q: q - 1), lambda r: pattern(primes, 1, n, r)[0]]
    return np.stack([kinds[r % 3](r) for r in range(rows)])


def dot_case(L: Landing, rows: int, cols: int, kind: str):
    """(ctn uint64[cols][2][K][n], pntt uint64[rows][cols][K][n], targets or None), written directly in the transform domain.
    kind "max": every word q - 1 in both operands.  kind "landed" / "landed_zero_column": random words; the LAST column of pntt is
    chosen word by word so that polynomial 0 of row r sums to dot_targets()[r], and polynomial 1 of the last ciphertext so that
    polynomial 1 of row 0 sums to 0; "landed_zero_column" has an all-zero ciphertext column and an all-zero plaintext column in the
    middle (cols >= 3)."""

    def make():
        P, n, K = L.primes, L.n, L.K
        if kind == "max":
            qm1 = (np.array(P, dtype=np.uint64) - 1)[:, None]
            return np.broadcast_to(qm1, (cols, 2, K, n)).copy(), np.broadcast_to(qm1, (rows, cols, K, n)).copy(), None
        rng = L.rng(1000 * rows + cols)
        ctn = random_residues(rng, P, (cols, 2), n)
        pntt = random_residues(rng, P, (rows, cols), n)
        ctn[-1, 0] = np.maximum(ctn[-1, 0], 1)  # (invertible)
        if kind == "landed_zero_column" and cols >= 3:
            ctn[cols // 2] = 0
            pntt[:, cols // 2 - 1] = 0
        T = dot_targets(P, rows, n)
        pntt[:, -1] = 0
        part = dot_sums(P, ctn, pntt)  # the sums without the last column
        for i, q in enumerate(P):
            inv = np.array([pow(int(v), -1, q) for v in ctn[-1, 0, i]], dtype=object)
            for r in range(rows):
                pntt[r, -1, i] = _u64((_obj(T[r, i]) - _obj(part[r, 0, i])) * inv % q)
            # polynomial 1 of row 0: ctn[-1][1] = -(the rest) / pntt[0][-1] where that word is invertible (else left as drawn)
            rest = _obj(part[0, 1, i])
            w = [int(v) for v in pntt[0, -1, i]]
            ctn[-1, 1, i] = _u64(np.array([(-int(s) * pow(x, -1, q)) % q if x else int(c) for s, x, c in zip(rest, w, ctn[-1, 1, i])], dtype=object))
        return ctn, pntt, T

    return L.cached(("dot", rows, cols, kind), make)


DOT_SHAPES = [(5, c) for c in (1, 15, 16, 17, 32, 33)] + [(r, 17) for r in (1, 3, 4)]
# every shape with every word q - 1 and with landed sums; the zero columns where the sixteen-product reduction point lies before
# and behind them (17 and 33 columns)
DOT_CASES = [(r, c, k) for r, c in DOT_SHAPES for k in ("max", "landed")] + [(5, 17, "landed_zero_column"), (5, 33, "landed_zero_column")]


def table_case(L: Landing, batch: int = 3, rows: int = 5, cols: int = 17):
    """The table form's operands (coefficient form: the reference interpreter multiplies plaintexts): cq uint64[cols][batch][2][K][n]
    ciphertexts with 0 / q - 1 / 1 cycles and random residues, db uint64[rows][cols][n] plaintexts cycling plain_edge_values(t)
    (three of them monomials, none zero)."""

    def make():
        P, n, t = L.primes, L.n, L.t
        rng = L.rng(60)
        cq = random_residues(rng, P, (cols, batch, 2), n)
        edge_ct = np.stack([cycle(P, n, lambda q: [0, q - 1, 1]), cycle(P, n, lambda q: [q - 1, 0])])
        cq[0, :] = edge_ct
        cq[cols // 2, 1] = np.stack([constant(P, n, lambda q: q - 1)] * 2)
        edge = np.array(plain_edge_values(t), dtype=np.uint64)
        db = rng.integers(1, t, (rows, cols, n), dtype=np.uint64)
        for r in range(rows):
            for j in range(0, cols, 2):
                db[r, j, : n // 2] = edge[(np.arange(n // 2) + r + j) % 5]
        for r, j, e, c in ((0, 1, 0, t - 1), (1, 3, n - 1, (t - 1) // 2), (2, 5, 1, 1)):
            db[r, j] = 0
            db[r, j, e] = c
        return cq, db

    return L.cached(("table", batch, rows, cols), make)


# ------------------------------------------------------------------------------------- shared by the sections F, G and H
def _product(primes) -> int:
    out = 1
    for q in primes:
        out *= int(q)
    return out


def thread_cycle(n: int, per_thread: int, length: int, shift: int = 0) -> np.ndarray:
    """int[n]: an index into a cycle of `length` such that the `per_thread` coefficients {t + j n / per_thread} of one thread take
    `per_thread` CONSECUTIVE indices.  (k % length alone gives one thread k-steps of n / per_thread, a power of two: with a cycle
    of six that is three different values at the most.)"""
    k = np.arange(n)
    stride = n // per_thread
    return (k % stride + k // stride + shift) % length


def scale_rows(primes, a, consts, invert: bool = False) -> np.ndarray:
    """uint64[K][n]: a[i] * consts[i] mod q_i (or a[i] / consts[i]) in Python integers."""
    rows = []
    for q, row, c in zip(primes, a, consts):
        c = pow(int(c), -1, int(q)) if invert else int(c)
        rows.append(_obj(row) * c % int(q))
    return _u64(np.stack(rows))


def odd_max(primes, n: int) -> np.ndarray:
    """uint64[K][n]: q_i - 1 in every row on the odd coefficients, 0 in every row on the even ones."""
    out = np.zeros((len(primes), n), dtype=np.uint64)
    for i, q in enumerate(primes):
        out[i, 1::2] = q - 1
    return out


# --------------------------------------------------------------- F: the multiply head -- r_mtilde and the y_i on their edges
M_TILDE = 1 << 32
R_TARGETS = [0, 1, (1 << 31) - 1, 1 << 31, (1 << 31) + 1, (1 << 32) - 1]


def ext_scale(primes) -> list[int]:
    """m~ (q / q_i)^-1 mod q_i: what the extension q -> Bsk u {m~} multiplies row i by first."""
    Q = _product(primes)
    return [(M_TILDE * pow(Q // q, -1, q)) % q for q in primes]


def r_targets(n: int, shift: int = 0) -> np.ndarray:
    """uint64[n]: R_TARGETS placed so that the eight coefficients of one head thread see all six."""
    return np.array(R_TARGETS, dtype=np.uint64)[thread_cycle(n, 8, len(R_TARGETS), shift)]


def land_mtilde(o, r_targets, y_of) -> np.ndarray:
    """uint64[K][n], one polynomial x whose scaled rows y_i = x_i m~ (q / q_i)^-1 mod q_i are y_of (uint64[K][n]) and whose
    r_mtilde = (sum y_i (q / q_i)) (-q^-1) mod 2^32 is r_targets (uint64[n]) in every coefficient.  x -> y is a bijection per
    row, so the y are chosen and x solved for; the first row whose prime is above 2^32 is `free`: its y is solved mod 2^32 from the
    target and the other rows (below 2^32, hence a residue).  r_targets None: all rows as given, r_mtilde whatever results."""
    P = [int(q) for q in o.primes]
    Q = _product(P)
    y = np.array(y_of, dtype=np.uint64)
    if r_targets is not None:
        free = next(i for i, q in enumerate(P) if q > M_TILDE)
        mask = np.uint64(M_TILDE - 1)
        c = [(Q // q) % M_TILDE for q in P]
        rest = np.zeros(y.shape[1], dtype=np.uint64)
        for i in range(len(P)):
            if i != free:
                rest = (rest + (y[i] & mask) * np.uint64(c[i])) & mask
        want = (np.asarray(r_targets, dtype=np.uint64) * np.uint64((-Q) % M_TILDE)) & mask  # the sum that gives the target
        y[free] = (((want - rest) & mask) * np.uint64(pow(c[free], -1, M_TILDE))) & mask
    return scale_rows(P, y, ext_scale(P), invert=True)


def mtilde_polynomial(L: "Landing", rng, kind: str, shift: int) -> np.ndarray:
    """One crafted polynomial: kind "random" (uniform y in the rows that are not free), "edge" (y cycling 0, q - 1, 1, (q -+ 1) / 2)
    or "max" (every y at q - 1 on the odd coefficients and 0 on the even ones, r_mtilde as it comes)."""
    P, n = L.primes, L.n
    if kind == "max":
        return land_mtilde(L.o, None, odd_max(P, n))
    y = random_residues(rng, P, (), n) if kind == "random" else pattern(P, 1, n, shift)[0]
    return land_mtilde(L.o, r_targets(n, shift), y)


MTILDE_KINDS = [("random", "edge"), ("edge", "random"), ("max", "random"), ("edge", "max")]


def mtilde_case(L: "Landing", size_a: int = 2, size_b: int = 2, items: int = 4):
    """(a uint64[items][size_a][K][n], b uint64[items][size_b][K][n]): item i multiplies a MTILDE_KINDS[i][0] operand by a
    MTILDE_KINDS[i][1] one; every polynomial has its own phase of the r_mtilde cycle."""

    def make():
        rng = L.rng(70 + 10 * size_a + size_b)
        a, b = [], []
        for i in range(items):
            ka, kb = MTILDE_KINDS[i % len(MTILDE_KINDS)]
            a.append(np.stack([mtilde_polynomial(L, rng, ka, 5 * i + p) for p in range(size_a)]))
            b.append(np.stack([mtilde_polynomial(L, rng, kb, 5 * i + p + 3) for p in range(size_b)]))
        return np.stack(a), np.stack(b)

    return L.cached(("mtilde", size_a, size_b, items), make)


# ------------------------------------------------------- G: the floor's inputs and the multiply's outputs, through b = (1, 1)
def floor_scale(o) -> list[int]:
    """t (q / q_i)^-1 mod q_i: the scaled inverse transform hands the floor y_i = d_i t (q / q_i)^-1 mod q_i."""
    P = [int(q) for q in o.primes]
    Q = _product(P)
    return [(int(o.t) * pow(Q // q, -1, q)) % q for q in P]


def ones_ct(L: "Landing", items: int) -> np.ndarray:
    """uint64[items][2][K][n]: (1, 1), the constant polynomial 1 twice.  Not transparent; its extension is the integer 1, so the
    tensor of a with it is d0 = a0, d1 = a0 + a1, d2 = a1 in every row."""
    b = np.zeros((items, 2, L.K, L.n), dtype=np.uint64)
    b[..., 0] = 1
    return b


def land_floor_inputs(o, y_of) -> np.ndarray:
    """uint64[K][n], the polynomial a with a_i t (q / q_i)^-1 = y_of[i] mod q_i: as a0 (a1) of a ciphertext multiplied by (1, 1),
    the floor of polynomial 0 (2) of the product reads exactly y_of."""
    return scale_rows(o.primes, y_of, floor_scale(o), invert=True)


def floor_case(L: "Landing"):
    """(a uint64[2][2][K][n], y uint64[2][2][K][n]): item 0 gives d0 and d2 the y cycle in different phases, item 1 has every row
    at q - 1 on the odd coefficients and 0 on the even ones (the conversion sums at their largest)."""

    def make():
        P, n = L.primes, L.n
        y = np.stack([pattern(P, 2, n, 1), np.stack([odd_max(P, n), odd_max(P, n)[:, ::-1].copy()])])
        a = np.stack([np.stack([land_floor_inputs(L.o, y[i, p]) for p in range(2)]) for i in range(2)])
        return a, y

    return L.cached("floor", make)


OUTPUT_TARGETS = (0, -1, 1)


def output_candidates(o, rng, count: int) -> list[int]:
    """Integers D whose product with (1, 1) may land on 0, -1 or +1: polynomial 0 of a (1, 1) is floor(t D / q) - u' coefficient by
    coefficient, u' in [0, K) the overflow of the fast conversion.  Half of them uniform in (-2^40, 2^40) (floor 0 or -1), half
    ceil(j q / t) + delta with j in [1, K] and delta uniform in (-2^40, 2^40) (floor j or j - 1, and u' is most often near K / 2:
    a small positive D has floor 0 and u' >= 1, so it never lands on 0 and none of the small ones lands on +1).  Even places hold
    the small candidates, odd places the others."""
    Q, t, K = _product(o.primes), int(o.t), o.K
    delta = [int(v) for v in rng.integers(-(1 << 40) + 1, 1 << 40, count)]
    j = [int(v) for v in rng.integers(1, K + 1, count)]
    return [d if k % 2 == 0 else -((-jj * Q) // t) + d for k, (d, jj) in enumerate(zip(delta, j))]


def _residues(primes, values) -> np.ndarray:
    return _u64(np.array([[int(v) % int(q) for v in values] for q in primes], dtype=object))


def land_multiply_output(o, rng=None, want: int = 4, rounds: int = 8, keep: int = 8):
    """({target: [D, ...]}, stats): candidates harvested from the oracle.  One candidate per coefficient of a0 and of a1, one oracle
    multiply by (1, 1) per round; kept are the D whose output (polynomial 0 for a0, polynomial 2 for a1) is 0 in every row, q_i - 1
    in every row, or 1 in every row.  Stops at `want` distinct candidates for 0 and for -1 (+1 is kept where found); fails loudly
    after `rounds` rounds.  stats: {family: [candidates, landed on 0, on -1, on +1]} for the two families of output_candidates."""
    rng = rng if rng is not None else np.random.default_rng(o.n + 77)
    P, n = [int(q) for q in o.primes], o.n
    b = np.zeros((2, o.K, n), dtype=np.uint64)
    b[..., 0] = 1
    wants = {0: np.zeros((o.K, 1), dtype=np.uint64), -1: np.array(P, dtype=np.uint64)[:, None] - 1, 1: np.ones((o.K, 1), dtype=np.uint64)}
    kept = {v: [] for v in OUTPUT_TARGETS}
    stats = {"small": [0, 0, 0, 0], "near j q / t": [0, 0, 0, 0]}
    small = np.arange(n) % 2 == 0  # (n is even: the places of a1's candidates have the parity of a0's)
    for _ in range(rounds):
        cand = output_candidates(o, rng, 2 * n)
        out = o.multiply(np.stack([_residues(P, cand[:n]), _residues(P, cand[n:])]), b)
        stats["small"][0] += n
        stats["near j q / t"][0] += n
        for poly, cs in ((0, cand[:n]), (2, cand[n:])):
            for slot, v in enumerate(OUTPUT_TARGETS):
                hit = np.flatnonzero((out[poly] == wants[v]).all(axis=0))
                stats["small"][1 + slot] += int(small[hit].sum())
                stats["near j q / t"][1 + slot] += int((~small[hit]).sum())
                for k in hit:
                    if cs[k] not in kept[v] and len(kept[v]) < keep:
                        kept[v].append(cs[k])
        if len(kept[0]) >= want and len(kept[-1]) >= want:
            return kept, stats
    raise RuntimeError(f"the harvest ran out: {stats} candidates / 0 / -1 / +1 after {rounds} rounds, kept {[len(kept[v]) for v in OUTPUT_TARGETS]}")


def output_polynomial(L: "Landing", kept, kinds) -> np.ndarray:
    """uint64[K][n]: coefficient k holds a harvested candidate for the target kinds[k] (the candidates of a target taken in turn)."""
    turn = thread_cycle(L.n, 4, 1 << 20) // 3
    return _residues(L.primes, [kept[int(v)][int(s) % len(kept[int(v)])] for v, s in zip(kinds, turn)])


def output_kinds(L: "Landing", targets, shift: int) -> np.ndarray:
    """int[n]: `targets` cycled so that the four coefficients {t + k n / 4} of one tail thread take four consecutive places."""
    return np.array(targets)[thread_cycle(L.n, 4, len(targets), shift)]


def output_case(L: "Landing"):
    """(a uint64[2][2][K][n], kinds int[2][2][n], kept, stats): polynomials 0 and 2 of a[i] (1, 1) are 0, q_i - 1 (and 1 where the
    harvest found some) in EVERY row, as kinds says, the targets in turn over a tail thread's coefficients."""

    def make():
        kept, stats = land_multiply_output(L.o, L.rng(80))
        targets = [v for v in OUTPUT_TARGETS if len(kept[v]) >= 4]
        kinds = np.stack([np.stack([output_kinds(L, targets, 2 * i + p) for p in range(2)]) for i in range(2)])
        a = np.stack([np.stack([output_polynomial(L, kept, kinds[i, p]) for p in range(2)]) for i in range(2)])
        return a, kinds, kept, stats

    return L.cached("output", make)


def output_sum_case(L: "Landing", groups: int = 2, terms: int = 3):
    """(a uint64[groups][terms][2][K][n], kinds int[groups][terms][2][n]): per coefficient the three terms' outputs are 0, q_i - 1,
    q_i - 1 in some order, so the sums of canonical residues pass through q_i - 1 and wrap to q_i - 2."""

    def make():
        kept = output_case(L)[2]
        kinds = np.stack([np.stack([np.stack([output_kinds(L, [0, -1, -1], g + j + p) for p in range(2)]) for j in range(terms)]) for g in range(groups)])
        a = np.stack([np.stack([np.stack([output_polynomial(L, kept, kinds[g, j, p]) for p in range(2)]) for j in range(terms)]) for g in range(groups)])
        return a, kinds

    return L.cached(("output sum", groups, terms), make)


def kinds_to_words(primes, kinds) -> np.ndarray:
    """uint64[..., K, n]: the residues of the small integers in kinds (int[..., n])."""
    k = np.asarray(kinds).astype(object)[..., None, :]
    return _u64(k % _qcol(primes, 0))


# ------------------------------------------------------------------------------------------ H: decrypt's gamma correction
def gamma_targets(gamma: int) -> list[int]:
    return [0, 1, gamma // 2 - 1, gamma // 2, gamma // 2 + 1, gamma - 1]


def _reduced_basis(u, v):
    """Lagrange-Gauss reduction of a two-dimensional integer basis."""
    norm = lambda w: w[0] * w[0] + w[1] * w[1]  # noqa: E731
    if norm(u) < norm(v):
        u, v = v, u
    while True:  # norm(u) >= norm(v)
        dot, nv = u[0] * v[0] + u[1] * v[1], norm(v)
        m = (2 * dot + nv) // (2 * nv)  # round(dot / nv)
        u = (u[0] - m * v[0], u[1] - m * v[1])
        if norm(u) >= nv:
            return v, u
        u, v = v, u


def _round_div(a: int, d: int) -> int:
    if d < 0:
        a, d = -a, -d
    return (2 * a + d) // (2 * d)


def land_gamma(o, targets, rng=None):
    """(phases: n integers in [0, Q), y uint64[K][n]): the gamma residue of decrypt's fast conversion,
    g = (sum y_i ((q / q_i) mod gamma)) (-q^-1) mod gamma with y_i = phase_i t gamma (q / q_i)^-1 mod q_i, is targets[k] in
    coefficient k.  The rows from the third on are random; (y_0, y_1) is the point of the coset
    {y_0 c_0 + y_1 c_1 = w mod gamma} nearest the middle of [0, q_0) x [0, q_1): a particular solution moved by the reduced basis
    of the lattice {y_0 c_0 + y_1 c_1 = 0} (determinant gamma, far below q_0 q_1), in exact integer arithmetic."""
    rng = rng if rng is not None else np.random.default_rng(o.n + 99)
    P, n, K, t, gamma = [int(q) for q in o.primes], o.n, o.K, int(o.t), int(o.gamma)
    assert K >= 2
    Q = _product(P)
    c = [(Q // q) % gamma for q in P]
    y = np.zeros((K, n), dtype=np.uint64)
    for i in range(2, K):
        y[i] = rng.integers(0, P[i], n, dtype=np.uint64)
    c0inv = pow(c[0], -1, gamma)
    b1, b2 = _reduced_basis((gamma, 0), ((-c[1] * c0inv) % gamma, 1))
    det = b1[0] * b2[1] - b1[1] * b2[0]
    assert abs(det) == gamma
    mid = (P[0] // 2, P[1] // 2)
    y0, y1 = [], []
    for k in range(n):
        rest = sum(int(y[i, k]) * c[i] for i in range(2, K))
        w = (-int(targets[k]) * Q - rest) % gamma  # sum y_i c_i must be w: g = w (-q^-1)
        px = (w * c0inv) % gamma
        dx, dy = mid[0] - px, mid[1]
        al, be = _round_div(dx * b2[1] - dy * b2[0], det), _round_div(b1[0] * dy - b1[1] * dx, det)
        for da, db in ((0, 0), (1, 0), (-1, 0), (0, 1), (0, -1), (1, 1), (-1, -1), (1, -1), (-1, 1)):
            x0 = px + (al + da) * b1[0] + (be + db) * b2[0]
            x1 = (al + da) * b1[1] + (be + db) * b2[1]
            if 0 <= x0 < P[0] and 0 <= x1 < P[1]:
                break
        else:
            raise RuntimeError(f"no point of the coset in the box at coefficient {k}")
        y0.append(x0), y1.append(x1)
    y[0], y[1] = _u64(np.array(y0, dtype=object)), _u64(np.array(y1, dtype=object))
    scale = [(t * gamma * pow(Q // q, -1, q)) % q for q in P]
    ph = scale_rows(P, y, scale, invert=True)
    acc = np.zeros(n, dtype=object)
    for i, q in enumerate(P):
        acc = acc + _obj(ph[i]) * (pow(Q // q, -1, q) * (Q // q))
    return [int(v) % Q for v in acc], y


def gamma_case(L: "Landing", items: int = 2, size: int = 2):
    """(ct uint64[items][size][K][n], phases, targets int[items][n]): random c1 (and c2), c0 landed on land_gamma's phases; the six
    targets cycled over the coefficients, item i shifted by 2 i."""

    def make():
        rng = L.rng(90 + size)
        G = gamma_targets(int(L.o.gamma))
        cts, phases, tg = [], [], []
        for i in range(items):
            want = [G[(k + 2 * i) % len(G)] for k in range(L.n)]
            ph, _ = land_gamma(L.o, want, rng)
            ct, _ = land_phase(L.o, L.sk, random_residues(rng, L.primes, (size - 1,), L.n), ph)
            cts.append(ct), phases.append(ph), tg.append(want)
        return np.stack(cts), phases, tg

    return L.cached(("gamma", items, size), make)


# ------------------------------------------------------------- I: prepared multiplicands and weighted sums on landed operands
def with_decoy(L: "Landing", ops, salt: int = 0):
    """(prepared uint64[len(ops) + 1][2][K][n], index): the ciphertexts to prepare with one fresh encryption that no item uses at
    place 1 and the operands in REVERSED order around it, and the index that names operand i.  Never the identity, never a constant
    step: a wrong index, a wrong row stride or a dropped index gives other words."""
    m = len(ops)
    places = [p for p in range(m + 1) if p != 1][::-1]
    prepared = np.empty((m + 1,) + ops[0].shape, dtype=np.uint64)
    prepared[1] = L.cached(("decoy", salt), lambda: L.fresh(L.rng(95 + salt), 1)[0])
    for i, p in enumerate(places):
        prepared[p] = ops[i]
    return prepared, places


def floor_operands(L: "Landing") -> np.ndarray:
    """uint64[4][2][K][n]: the two operands of floor_case and the two of output_case (what is multiplied by (1, 1))."""
    return np.ascontiguousarray(np.concatenate([floor_case(L)[0], output_case(L)[0]]))


NINE_INDEX = [6, 2, 9, 4, 1, 3, 8, 5, 7]


def nine_case(L: "Landing"):
    """(a uint64[9][2][K][n], prepared uint64[10][2][K][n], index, refs): nine items over nine prepared ciphertexts and a decoy at
    place 0.  Places 1 ... 4 hold the four multiplicands of mtilde_case (item: its first operand), place 5 holds (1, 1) (item: the
    floor operand with every row at q - 1), places 6 ... 9 the four floor operands (item: (1, 1)).  refs[i] = ("head" | "floor", k):
    item i's product is product k of that family (BFV's tensor is symmetric).  At n = 16384 nine operations make the slice-major
    workgroup order run with per = 2."""
    ma, mb = mtilde_case(L)
    fo = floor_operands(L)
    ones = ones_ct(L, 1)[0]
    prepared = np.stack([L.cached(("decoy", 9), lambda: L.fresh(L.rng(104), 1)[0])] + list(mb) + [ones] + list(fo))
    role = {p: (ma[p - 1], ("head", p - 1)) for p in range(1, 5)}
    role[5] = (fo[1], ("floor", 1))
    role.update({p: (ones, ("floor", p - 6)) for p in range(6, 10)})
    a = np.stack([role[p][0] for p in NINE_INDEX])
    return a, prepared, list(NINE_INDEX), [role[p][1] for p in NINE_INDEX]


def output_sum_products(L: "Landing", groups: int = 2, terms: int = 3) -> np.ndarray:
    """uint64[groups][terms][3][K][n]: the oracle's product of every term of output_sum_case with (1, 1), once per process."""

    def make():
        a = output_sum_case(L, groups, terms)[0]
        ones = ones_ct(L, 1)[0]
        return np.stack([np.stack([L.o.multiply(a[g, j], ones) for j in range(terms)]) for g in range(groups)])

    return L.cached(("output sum products", groups, terms), make)


WEIGHT_VECTORS = [(1, -1, 1), ((1 << 31) - 1, -((1 << 31) - 1), 1), (-(1 << 31), (1 << 31) - 1, 1), (3, -2, -1)]
SUM_EVENTS = ("raw q", "raw q - 1", "final 0", "final q - 1", "final 1", "zero weight", "raw q in polynomial 1")


def modulus_weights(L: "Landing") -> list:
    """Weights of the size of a 30-bit prime q_1 of the set: (q_1, -q_1, 1) is 0 modulo q_1 alone in its first two terms;
    (2 q_1 - 2^31, 2^31 - 1, -2^31) has two weights above q_1 in absolute value and a first one that is -2^31 modulo q_1."""
    q1 = next(q for q in L.primes if q.bit_length() == 30)
    return [(q1, -q1, 1), (2 * q1 - (1 << 31), (1 << 31) - 1, -(1 << 31))]


def weighted_sum_case(L: "Landing", weights, groups: int = 2, terms: int = 3):
    """(a uint64[groups][terms][2][K][n], expected uint64[groups][3][K][n], events {name: int[K]}): the operands of output_sum_case
    (to be multiplied by (1, 1)), the sums sum_t (w_t mod q_i) p_t mod q_i of the oracle's products p_t row by row in Python
    integers (DESIGN 5.6.1's definition), and how often each edge is met on polynomials 0 and 2, per residue row.  The kernels
    (mul_tail_sum_weighted_kernel's four bodies, scaled_accumulate_kernel) all add in term order, the first term onto 0:
    raw_t = acc_{t-1} + (p_t w_t mod q_i), acc_t = raw_t reduced; that order is counted.
    "raw q" / "raw q - 1": a raw_t that is exactly q_i (the `>= q` compare) / q_i - 1; "final 0" / "final q - 1" / "final 1": the
    stored word; "zero weight": a weighted residue of 0 from a nonzero product word.  Polynomial 1 (a0 + a1 through the floor: small
    integers too, not chosen) meets a raw sum of q_i under some weights as well; that is counted apart, "raw q in polynomial 1", so
    that a vector with no raw q_i ANYWHERE is known.
    Polynomials 0 and 2 are also derived from `kinds` and the weights alone; the two derivations must agree."""
    weights = tuple(int(w) for w in weights)
    assert len(weights) == terms

    def make():
        a, kinds = output_sum_case(L, groups, terms)
        prods = output_sum_products(L, groups, terms)
        P = [int(q) for q in L.primes]
        expected = np.zeros((groups, 3, L.K, L.n), dtype=np.uint64)
        events = {e: np.zeros(L.K, dtype=np.int64) for e in SUM_EVENTS}
        for i, q in enumerate(P):
            acc = np.zeros((groups, 3, L.n), dtype=object)
            for j, w in enumerate(weights):
                p = _obj(prods[:, j, :, i])
                wr = p * (w % q) % q
                raw = acc + wr
                events["raw q"][i] += int((raw[:, ::2] == q).sum())
                events["raw q - 1"][i] += int((raw[:, ::2] == q - 1).sum())
                events["zero weight"][i] += int(((wr[:, ::2] == 0) & (p[:, ::2] != 0)).sum())
                events["raw q in polynomial 1"][i] += int((raw[:, 1] == q).sum())
                acc = raw % q
            expected[:, :, i] = _u64(acc)
            for name, v in (("final 0", 0), ("final q - 1", q - 1), ("final 1", 1)):
                events[name][i] += int((acc[:, ::2] == v).sum())
            from_kinds = sum(_obj(kinds[:, j]) * w for j, w in enumerate(weights)) % q  # [groups][2][n]
            assert (from_kinds == acc[:, ::2]).all(), ("the sums from the kinds and from the oracle's products differ", L.pid, weights, i)
        return a, expected, events

    return L.cached(("weighted sum", weights, groups, terms), make)


# -------------------------------------------------------------------------------------------------------- J: sums of rotations
INT32_MIN, INT32_MAX = -(1 << 31), (1 << 31) - 1
ROTATION_SUM_MODES = ("terms", "partial", "ladder", "transparent", "almost", "gathers", "random")
ROTATION_SUM_EVENTS = ("term 0", "term q - 1", "term 1", "term (q - 1) / 2", "term (q + 1) / 2", "weighted 0", "weighted q - 1", "raw q",
                       "raw q - 1", "final 0", "final q - 1", "final 1", "zero weight")
TRANSPARENT_GROUP = 1  # the group whose polynomial 1 the modes "transparent" and "almost" land; the others are "partial"
STEPS_TWO_IDENTITIES = (1, 0, -3, 0)  # two identity terms, from different sources
STEPS_IDENTITY_FIRST = (0, 1, -3)     # the landed first term is an identity term
STEPS_CHAIN = (11, 0, 1, -13)         # under the power-of-two keys: 11 = [-1, -4, 16] and -13 = [-1, 4, -16] walk their NAF chains
ROTATION_WEIGHTS = (None, (2, -1, 3, -2), (-1, 1, -1, 1), (0, -1, INT32_MIN, INT32_MAX))


def galois_elements(L: "Landing") -> tuple:
    """The Galois-element form's terms: an element that is no step's neighbour, the identity, the column element, the identity."""
    return (2 * L.n - 5, 1, 2 * L.n - 1, 1)


def rotation_modulus_weights(L: "Landing", terms: int) -> tuple:
    """(2, q_1, -1, 1): the second weight is a 30-bit prime of the set, 0 modulo that prime alone (modulus_weights' idea)."""
    q1 = next(q for q in L.primes if q.bit_length() == 30)
    return (2, q1, -1, 1)[:terms]


def rotation_sum_runs(L: "Landing") -> list:
    """[(name, steps, weights, galois, pow2)]: the step and weight vectors of a parameter set, shared by tests/test_landing_cpu.py
    (every one lands) and tests/test_gpu_landing_rotate_sum.py.  The first two carry every mode, the others terms, partial and
    ladder (rotation_sum_modes).  The extreme vector's first weight is 0 in every row; the modulus-sized one (sets with a 30-bit prime) in one row alone."""
    runs = [("two identities", STEPS_TWO_IDENTITIES, None, False, False),
            ("two identities, small weights", STEPS_TWO_IDENTITIES, ROTATION_WEIGHTS[1], False, False),
            ("identity first, +-1", STEPS_IDENTITY_FIRST, ROTATION_WEIGHTS[2][:3], False, False),
            ("two identities, extreme weights", STEPS_TWO_IDENTITIES, ROTATION_WEIGHTS[3], False, False),
            ("elements, +-1", galois_elements(L), ROTATION_WEIGHTS[2], True, False),
            ("elements", galois_elements(L), None, True, False)]
    if L.n >= 16384:
        runs = runs[:3]  # (n = 16384 and above: the vectors that take another path there; the others stay with the smaller sets)
    if any(q.bit_length() == 30 for q in L.primes):
        runs.append(("two identities, a modulus-sized weight", STEPS_TWO_IDENTITIES, rotation_modulus_weights(L, 4), False, False))
    if L.pid == "P1":
        runs += [("chains", STEPS_CHAIN, None, False, True), ("chains, small weights", STEPS_CHAIN, ROTATION_WEIGHTS[1], False, True)]
    return runs


def rotation_sum_modes(run_index: int) -> tuple:
    return ROTATION_SUM_MODES[:6] if run_index < 2 else ROTATION_SUM_MODES[:3]


def _element(o, s: int, galois: bool) -> int:
    return int(s) if galois else (1 if s == 0 else int(o.galois_elt_from_step(int(s))))


def _rotate(o, ct, s: int, gk, galois: bool) -> np.ndarray:
    """The oracle's rotation of one ciphertext by term s (a step of rotate_rows, or a Galois element); the identity is a copy."""
    if _element(o, s, galois) == 1:
        return np.array(ct, dtype=np.uint64)
    return o.apply_galois(ct, int(s), gk) if galois else o.rotate_rows(ct, int(s), gk)


def land_rotation(o, gk, step_or_elt: int, c1, T0, galois: bool = False, r=None):
    """(ct2, expected): polynomial 0 of the oracle's rotation of ct2 == T0, for ANY rotation the oracle performs -- a direct key, a
    NAF chain over the keys gk holds, the identity.  c0 enters a chain of key switches by permutation and addition alone, so
    rotate((c0, c1))[0] = sigma_g(c0) + rotate((0, c1))[0] with g the total element, and c0 = sigma_{g^-1}(T0 - rotate((0, c1))[0]).
    r: rotate((0, c1)) where the caller has it already."""
    elt = _element(o, step_or_elt, galois)
    if r is None:
        r = _rotate(o, np.stack([np.zeros_like(c1), c1]), step_or_elt, gk, galois)
    c0 = lin_mod(o.primes, [(1, T0), (-1, r[0])])
    if elt != 1:
        c0 = o.apply_galois_poly(c0, pow(elt, -1, 2 * o.n))
    return np.stack([c0, c1]), np.stack([_u64(T0), r[1]])


def pow2_elements(L: "Landing") -> list:
    """The elements of every step +-2^i below n / 2 and of the column rotation: the holding "P" of tests/test_gpu_rotation_steps.py."""
    h = L.n // 2
    return sorted({L.o.galois_elt_from_step(s * (1 << i)) for i in range(h.bit_length() - 1) for s in (1, -1)} | {2 * L.n - 1})


def rotation_sum_keys(L: "Landing", steps, galois: bool = False, pow2: bool = False) -> dict:
    """The Galois keys of a case: the terms' own elements, or the power-of-two holding (a step without a key there is a chain)."""
    if pow2:
        return L.galois_keys(pow2_elements(L))
    return L.galois_keys(sorted({_element(L.o, s, galois) for s in steps} - {1}))


def scale_words(primes, a, w: int) -> np.ndarray:
    """uint64[..., K, n]: every word of residue row i times (w mod q_i) mod q_i.  Weights within 8 of 0 modulo q_i stay in uint64
    (8 q_i < 2^64), the others go through Python integers."""
    a = np.asarray(a, dtype=np.uint64)
    out = np.empty_like(a)
    for i, q in enumerate(primes):
        q, wm = int(q), int(w) % int(q)
        row = a[..., i, :]
        if wm <= 8:
            out[..., i, :] = (row * np.uint64(wm)) % np.uint64(q)
        elif q - wm <= 8:
            neg = (row * np.uint64(q - wm)) % np.uint64(q)
            out[..., i, :] = np.where(neg == 0, neg, np.uint64(q) - neg)
        else:
            out[..., i, :] = _u64(_obj(row) * wm % q)
    return out


def uncorrected_products(primes, a, w: int) -> np.ndarray:
    """uint64[..., K, n]: the weighted residues as a Shoup product WITHOUT its last correction leaves them, in [0, 2 q_i):
    r w - floor(r w' / 2^64) q_i with w = w mod q_i and w' = floor(w 2^64 / q_i).  The estimate of the quotient is one short where
    the true residue is below about r q_i / 2^64 -- on small weighted residues such as 1 and 2, hardly ever on random ones."""
    a = np.asarray(a, dtype=np.uint64)
    out = np.empty_like(a)
    for i, q in enumerate(primes):
        q, wm = int(q), int(w) % int(q)
        r = _obj(a[..., i, :])
        out[..., i, :] = _u64(r * wm - ((r * ((wm << 64) // q)) >> 64) * q)
    return out


def fold_terms(primes, terms, weights, turned=None, events=None) -> np.ndarray:
    """uint64[2][K][n]: sum_t (w_t mod q_i) terms[t] mod q_i in term order, the first term onto 0, as the kernels add:
    raw = acc + weighted term, acc = raw - q_i if raw >= q_i.  turned "add": `>` for `>=` (a model that is WRONG at a raw sum of
    exactly q_i and nowhere else); turned "product": the weighted residue left in [0, 2 q_i) (uncorrected_products).  events:
    {name: int[K]} counters of ROTATION_SUM_EVENTS to add to."""
    assert turned in (None, "add", "product"), turned
    acc = np.zeros_like(np.asarray(terms[0], dtype=np.uint64))
    qcol = np.array([int(q) for q in primes], dtype=np.uint64)[:, None]
    last = len(terms) - 1
    for t, (r, w) in enumerate(zip(terms, weights)):
        r = np.asarray(r, dtype=np.uint64)
        wr = uncorrected_products(primes, r, w) if turned == "product" else scale_words(primes, r, w)
        raw = acc + wr
        over = raw > qcol if turned == "add" else raw >= qcol
        nxt = np.where(over, raw - qcol, raw)
        if events is not None:
            half = qcol >> np.uint64(1)
            zero_w = np.array([int(w) % int(q) == 0 for q in primes])[:, None]
            for name, hit in (("term 0", r == 0), ("term q - 1", r == qcol - 1), ("term 1", r == 1), ("term (q - 1) / 2", r == half),
                              ("term (q + 1) / 2", r == half + 1), ("weighted 0", wr == 0), ("weighted q - 1", wr == qcol - 1),
                              ("raw q", raw == qcol), ("raw q - 1", raw == qcol - 1), ("zero weight", (r != 0) & zero_w)):
                events[name] += hit.sum(axis=(0, 2))
            if t == last:
                for name, hit in (("final 0", nxt == 0), ("final q - 1", nxt == qcol - 1), ("final 1", nxt == 1)):
                    events[name] += hit.sum(axis=(0, 2))
        acc = nxt
    return acc


def _solve_term(primes, T, acc, w: int, filler) -> np.ndarray:
    """uint64[K][n]: the residue r with acc + (w mod q_i) r == T mod q_i; in a row where w = 0 mod q_i, `filler`'s row."""
    out = np.array(filler, dtype=np.uint64)
    diff = lin_mod(primes, [(1, T), (-1, acc)])
    for i, q in enumerate(primes):
        wm = int(w) % int(q)
        if wm == 1:
            out[i] = diff[i]
        elif wm == int(q) - 1:
            out[i] = np.where(diff[i] == 0, diff[i], np.uint64(q) - diff[i])
        elif wm:
            out[i] = _u64(_obj(diff[i]) * pow(wm, -1, int(q)) % int(q))
    return out


def _sum_target(primes, n: int, mode: str, t: int, shift: int) -> np.ndarray:
    """uint64[2][K][n]: where the sum stands after term t.  ladder: q - 1, 0, q - 1, 0 in every word of polynomial 0 and the other
    phase in polynomial 1 (an identity term in an odd place ends it on q - 1, never on a transparent 0)."""
    if mode == "ladder":
        hi, lo = constant(primes, n, lambda q: q - 1), constant(primes, n, 0)
        return np.stack([hi, lo] if t % 2 == 0 else [lo, hi])
    return pattern(primes, 2, n, shift)


def rotation_sum_case(L: "Landing", steps, weights, mode: str, groups: int, galois: bool = False, pow2: bool = False):
    """(sources uint64[groups * terms][2][K][n], expected uint64[groups][2][K][n], events {name: int[K]}): item g * terms + t is the
    source of term t of group g; expected[g] = sum_t (w_t mod q_i) rotate(source, steps[t]) folded in term order (fold_terms), from
    the landed values and the oracle's rotate((0, c1)) -- tests/test_landing_cpu.py shows that the oracle's rotations of the sources,
    scaled and added, give exactly that.  weights None: all ones.  galois: the terms are Galois elements (1: the identity).  pow2: the
    keys are the power-of-two holding.  Group g moves every pattern by g.

    terms        polynomial 0 of every finished rotated term and both polynomials of every identity term on pattern(shift = t)
    partial      the running sum after term t on pattern(shift = t): polynomial 0 after every term, polynomial 1 after every
                 identity term.  In a row where w_t = 0 mod q_i the term adds 0 and the sum stays where it was.
    ladder       the same with constant targets: the sums go q - 1, 0, q - 1, 0, the weighted terms q - 1, 1, q - 1, 1 and the raw
                 sums q - 1, q, q - 1, q in every word
    transparent  partial, and the last identity term of group TRANSPARENT_GROUP lands the FINAL polynomial 1 on all zeros
    almost       the same on almost_zero
    gathers      compared, not landed: random sources, but c0 and c1 of the first rotated term of every group cycle 0, q - 1, 1
    random       random sources (the control of the turned model)"""
    import zlib

    assert mode in ROTATION_SUM_MODES, mode
    steps = tuple(int(s) for s in steps)
    terms = len(steps)
    wts = (1,) * terms if weights is None else tuple(int(w) for w in weights)
    assert len(wts) == terms
    key = ("rotation sum", steps, wts, mode, groups, galois, pow2)

    def make():
        o, P, n, K = L.o, L.primes, L.n, L.K
        gk = rotation_sum_keys(L, steps, galois, pow2)
        rng = L.rng(zlib.crc32(repr(key).encode()))
        ident = [_element(o, s, galois) == 1 for s in steps]
        zero = np.zeros((K, n), dtype=np.uint64)
        sources = np.zeros((groups * terms, 2, K, n), dtype=np.uint64)
        expected = np.zeros((groups, 2, K, n), dtype=np.uint64)
        events = {e: np.zeros(K, dtype=np.int64) for e in ROTATION_SUM_EVENTS}
        for g in range(groups):
            if mode in ("gathers", "random"):
                src = random_residues(rng, P, (terms, 2), n)
                if mode == "gathers":
                    t0 = ident.index(False)
                    src[t0] = np.stack([cycle(P, n, lambda q: [0, q - 1, 1]), cycle(P, n, lambda q: [1, 0, q - 1, 0, q - 1])])
                vals = [_rotate(o, src[t], steps[t], gk, galois) for t in range(terms)]
            else:
                # the key-switch part of every rotated term: it does not depend on c0
                c1 = {t: random_residues(rng, P, (), n) for t in range(terms) if not ident[t]}
                R = {t: _rotate(o, np.stack([zero, c1[t]]), steps[t], gk, galois) for t in c1}
                final1 = None  # (t, target): the identity term that lands the FINAL polynomial 1
                if mode in ("transparent", "almost") and g == TRANSPARENT_GROUP:
                    t1 = max(t for t in range(terms) if ident[t])
                    assert all(wts[t1] % q for q in P), "the landing identity term needs an invertible weight in every row"
                    rest = [(-1, scale_words(P, R[t][1], wts[t])) for t in range(t1 + 1, terms)]
                    final1 = (t1, lin_mod(P, [(1, zero if mode == "transparent" else almost_zero(P, n))] + rest))
                acc = np.zeros((2, K, n), dtype=np.uint64)
                src, vals = [], []
                for t in range(terms):
                    shift = t + g
                    filler = pattern(P, 2, n, shift)
                    if mode == "terms":
                        val = filler if ident[t] else np.stack([filler[0], R[t][1]])
                    else:
                        T = _sum_target(P, n, mode, t, shift)
                        if final1 is not None and final1[0] == t:
                            T[1] = final1[1]
                        v0 = _solve_term(P, T[0], acc[0], wts[t], filler[0])
                        val = np.stack([v0, _solve_term(P, T[1], acc[1], wts[t], filler[1]) if ident[t] else R[t][1]])
                    src.append(val if ident[t] else land_rotation(o, gk, steps[t], c1[t], val[0], galois, R[t])[0])
                    vals.append(val)
                    acc = fold_terms(P, [acc, val], [1, wts[t]])
            for t in range(terms):
                sources[g * terms + t] = src[t]
            expected[g] = fold_terms(P, vals, wts, events=events)
        return sources, expected, events

    return L.cached(key, make)
