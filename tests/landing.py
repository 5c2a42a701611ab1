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

What the method cannot reach: the multiply tails and the BEHZ floor (their outputs are not an affine function of anything the
caller holds), polynomial 1 of a stand-alone rotation (it is ks1 alone), and the gamma-correction boundary of decrypt."""
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
    """(ct2, residues): c0 + c1 s == phases[k] mod Q in coefficient k.  phases: n integers in [0, Q)."""
    want = _u64(np.array([[int(x) % q for x in phases] for q in o.primes], dtype=object))
    d = o.dot_with_secret(np.stack([np.zeros_like(c1), c1]), sk)
    return np.stack([lin_mod(o.primes, [(1, want), (-1, d)]), c1]), want


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
