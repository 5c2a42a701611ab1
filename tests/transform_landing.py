"""Crafted operands and integer models for the whole-polynomial transforms and what is fused around them: the stand-alone NTT, the
plaintext product (ct_plain_kernel, and the unfused ntt -> dyadic_plain_kernel -> ntt route at n = 32768), ct_to_ntt, the
BatchEncoder's encode and mod_switch_kernel.  The method is tests/landing.py's: choose what the kernel's OWN output must be in
every thread and solve for the operand that gives it.

A transform is a bijection: its output is any target T when its input is the inverse transform of T (land_forward, land_inverse).
The plaintext product's output is T when ct = INTT(NTT(T) / NTT(lift p)), pointwise, for a plaintext whose transform has no zero
word (land_multiply_plain).  The encoder's output coefficients are Tp when the slot values are the decode of Tp (land_encode).
mod_switch_to_next is solved row by row by client_landing.land_mod_switch (mod_switch_case).

Two statements of what the device is compared against, besides the oracle: a radix-2 negacyclic transform in Python integers
(ntt_plain: psi is the oracle's minimal primitive root, the butterfly network and the output order are SEAL's), and a model of the
integer policy's lazy arithmetic of sunscreen_amd/csrc/nttcore.hpp (ntt_lazy: the forward butterfly on [0, 4q) and the inverse on
[0, 2q) with the Shoup product's truncated quotient, `canonical`, and scale_canonical's product by n^-1).  The lazy model walks the
same butterfly network, so how the device groups stages into passes does not change a value; it reports the REPRESENTATIVE in
front of the last conditional subtractions, which is what the landed rows are for: a residue 0 stored as q, 2q or 3q, a residue
q - 1 stored as 2q - 1 or 3q - 1.  Of the inverse: the word in front of scale_canonical's one subtraction is
v w - floor(v w' / 2^64) q with w' = floor(w 2^64 / q); the truncated quotient is short by one only where frac(v w / q) is below
v / 2^64, so residue 0 arrives as q whenever v = q, and residue q - 1 always arrives as q - 1 itself.

The FP64 policy gets no float emulation: its rows are landed on the same targets ((q +- 1) / 2 is where rint(v / q) sits on a tie,
0 and q - 1 are where the sign fix matters) and compared with the oracle and ntt_plain.

Out of reach: plain_to_ntt's output (a plaintext's coefficients are below t: the transform's input is not free), and the
inverse-with-product kernel of encrypt and decrypt beyond what tests/client_landing.py already lands.

Test infrastructure, CPU only: imports the oracle and numpy, never the library under test."""
from __future__ import annotations

import types

import numpy as np

from oracle import bfv_oracle as O
from tests import client_landing as CL
from tests import landing as LD
from tests.landing import _obj, _u64

MASK64 = (1 << 64) - 1


# ---------------------------------------------------------------------------------------------- 1: an independent transform
def bit_reverse(i: int, bits: int) -> int:
    return int(format(i, f"0{bits}b")[::-1], 2)


def psi_tables(L, i: int):
    """(forward, inverse) object[n]: table[bit_reverse(k)] = psi^k (psi^-k), psi the minimal primitive 2n-th root of unity modulo
    key-level prime i.  Stage m of the forward transform reads forward[m + block]."""

    def make():
        q, n = L.key_primes[i], L.n
        bits = n.bit_length() - 1
        psi = O.minimal_primitive_root(2 * n, q)
        assert pow(psi, n, q) == q - 1
        ipsi = pow(psi, -1, q)
        fwd, inv = np.zeros(n, dtype=object), np.zeros(n, dtype=object)
        pw = ipw = 1
        for k in range(n):
            r = bit_reverse(k, bits)
            fwd[r], inv[r] = pw, ipw
            pw, ipw = pw * psi % q, ipw * ipsi % q
        return fwd, inv

    return L.cached(("psi", i), make)


def ntt_plain(L, i: int, x, inverse: bool = False) -> np.ndarray:
    """uint64[n]: the negacyclic transform of x modulo key-level prime i, every step reduced, in Python integers.  Forward:
    Cooley-Tukey, the gap halving from n / 2, X' = X + W Y, Y' = X - W Y with W = psi^bit_reverse(m + block), the output in the
    order that leaves (SEAL's).  Inverse: Gentleman-Sande, the gap doubling from 1, X' = X + Y, Y' = (X - Y) W^-1, then n^-1."""
    q, n = L.key_primes[i], L.n
    fwd, inv = psi_tables(L, i)
    a = _obj(x).copy()
    if not inverse:
        m, gap = 1, n // 2
        while m < n:
            a = a.reshape(m, 2, gap)
            X, Y = a[:, 0, :], a[:, 1, :] * fwd[m : 2 * m].reshape(m, 1) % q
            a = np.stack([(X + Y) % q, (X - Y) % q], axis=1)
            m, gap = 2 * m, gap // 2
        return _u64(a.reshape(n))
    m, gap = n // 2, 1
    while m >= 1:
        a = a.reshape(m, 2, gap)
        X, Y = a[:, 0, :], a[:, 1, :]
        a = np.stack([(X + Y) % q, (X - Y) * inv[m : 2 * m].reshape(m, 1) % q], axis=1)
        m, gap = m // 2, 2 * gap
    return _u64(a.reshape(n) * pow(n, -1, q) % q)


# ------------------------------------------------------------------------------------- 3: the integer policy's lazy arithmetic
def _shoup(w, q: int):
    """floor(w 2^64 / q): the Shoup quotient of a constant w < q."""
    return (w << 64) // q


def mul_shoup_lazy(x, w, wq, q: int):
    """x w - floor(x w' / 2^64) q on 64-bit words: congruent to x w, in [0, 2q) for any 64-bit x."""
    return (x * w - ((x * wq) >> 64) * q) & MASK64


def canonical(v, q: int, variant: str | None = None):
    """ArithI::canonical on [0, 4q).  Variants (mutations): "gt_2q" / "gt_q" write '>' for '>=' at the first / second compare."""
    q2 = 2 * q
    v = np.where(v > q2 if variant == "gt_2q" else v >= q2, v - q2, v)
    return np.where(v > q if variant == "gt_q" else v >= q, v - q, v)


def ntt_lazy(L, i: int, x, inverse: bool = False):
    """(representative object[n], out uint64[n]): the transform of the canonical row x under the integer policy.  Forward: the
    values in front of `canonical`, in [0, 4q).  Inverse: the words in front of scale_canonical's conditional subtraction, in
    [0, 2q).  The invariants of nttcore.hpp are asserted at every stage."""
    q, n = L.key_primes[i], L.n
    q2 = 2 * q
    assert q < (1 << 62)
    fwd, inv = psi_tables(L, i)
    a = _obj(x).copy()
    assert (a < q).all()
    if not inverse:
        fq = _shoup(fwd, q)
        m, gap = 1, n // 2
        while m < n:
            a = a.reshape(m, 2, gap)
            X, Y = a[:, 0, :], a[:, 1, :]
            xr = np.where(X >= q2, X - q2, X)
            t = mul_shoup_lazy(Y, fwd[m : 2 * m].reshape(m, 1), fq[m : 2 * m].reshape(m, 1), q)
            assert (t < q2).all()
            a = np.stack([xr + t, xr + q2 - t], axis=1)
            assert (a < 4 * q).all() and (a >= 0).all()
            m, gap = 2 * m, gap // 2
        rep = a.reshape(n)
        return rep, _u64(canonical(rep, q))
    iq = _shoup(inv, q)
    m, gap = n // 2, 1
    while m >= 1:
        a = a.reshape(m, 2, gap)
        X, Y = a[:, 0, :], a[:, 1, :]
        s = X + Y
        y = mul_shoup_lazy(X + q2 - Y, inv[m : 2 * m].reshape(m, 1), iq[m : 2 * m].reshape(m, 1), q)
        a = np.stack([np.where(s >= q2, s - q2, s), y], axis=1)
        assert (a < q2).all() and (a >= 0).all()
        m, gap = m // 2, 2 * gap
    ninv = pow(n, -1, q)
    rep = mul_shoup_lazy(a.reshape(n), ninv, _shoup(ninv, q), q)
    assert (rep < q2).all()
    return rep, _u64(np.where(rep >= q, rep - q, rep))


def scale_finish(rep, q: int, variant: str | None = None):
    """The conditional subtraction that ends mul_shoup ("gt": '>' for '>=')."""
    return np.where(rep > q if variant == "gt" else rep >= q, rep - q, rep)


def events(rep, out, q: int) -> dict:
    """{(target name, floor(representative / q)): words} over the words of one row whose canonical value is 0, q - 1 or 1."""
    table = {}
    for name, v in (("0", 0), ("q-1", q - 1), ("1", 1)):
        at = np.asarray(out) == np.uint64(v)
        for mult in set((rep[at] // q).tolist()):
            table[(name, int(mult))] = int((rep[at] // q == mult).sum())
    return table


# --------------------------------------------------------------------------------------------- 2: landed stand-alone transforms
def unit(q: int, n: int, at: int) -> np.ndarray:
    out = np.zeros(n, dtype=np.uint64)
    out[at % n] = 1
    return out


def target_row(L, i: int, kind: str, shift: int) -> np.ndarray:
    """uint64[n]: one target row for key-level prime i.  "pattern": the five targets at phase `shift`; "max": all q - 1; "unit": 0
    everywhere except one word equal to 1."""
    q, n = L.key_primes[i], L.n
    if kind == "pattern":
        return LD.pattern([q], 1, n, shift)[0, 0]
    if kind == "max":
        return np.full(n, q - 1, dtype=np.uint64)
    assert kind == "unit"
    return unit(q, n, 97 * shift + 5)


def transform_targets(L, kinds, extra: int = 0) -> np.ndarray:
    """uint64[len(kinds) * KK + extra][n]: one group of KK rows per entry of `kinds` (row r is transformed under key-level prime
    r % KK, as the stand-alone entry point counts them), then `extra` pattern rows.  A pattern row's phase differs from row to row."""
    KK = L.o.KK
    rows = [target_row(L, i, kind, g * KK + i) for g, kind in enumerate(kinds) for i in range(KK)]
    rows += [target_row(L, e % KK, "pattern", len(kinds) * KK + e + 1) for e in range(extra)]
    return np.stack(rows)


def land_forward(L, i: int, T) -> np.ndarray:
    """uint64[n]: the row whose FORWARD transform under key-level prime i is T."""
    return L.o.ntt(i, _u64(T), inverse=True)


def land_inverse(L, i: int, T) -> np.ndarray:
    """uint64[n]: the row whose INVERSE transform under key-level prime i is T."""
    return L.o.ntt(i, _u64(T))


def landed_transform_rows(L, kinds, extra: int = 0):
    """(T, x_forward, x_inverse) uint64[rows][n] each: forward(x_forward[r]) == T[r] == inverse(x_inverse[r]) under prime r % KK."""

    def make():
        T = transform_targets(L, kinds, extra)
        KK = L.o.KK
        xf = np.stack([land_forward(L, r % KK, T[r]) for r in range(len(T))])
        xi = np.stack([land_inverse(L, r % KK, T[r]) for r in range(len(T))])
        return T, xf, xi

    return L.cached(("transform rows", tuple(kinds), extra), make)


def landed_ciphertexts_for_ct_to_ntt(L, size: int, items: int = 2):
    """(ct uint64[items][size][K][n], T): ct_to_ntt(ct) == T.  Item 0 on the pattern; item 1: polynomial 0 all q - 1, polynomial 1
    zero but one word, any further polynomial on the pattern."""

    def make():
        P, n = L.primes, L.n
        T = np.stack([LD.pattern(P, size, n, 1 + 4 * it) for it in range(items)])
        if items > 1:
            T[1, 0] = LD.constant(P, n, lambda q: q - 1)
            T[1, 1] = np.stack([unit(q, n, 11 + i) for i, q in enumerate(P)])
        ct = np.stack([np.stack([np.stack([land_forward(L, i, T[it, c, i]) for i in range(L.K)]) for c in range(size)]) for it in range(items)])
        return ct, T

    return L.cached(("ct_to_ntt", size, items), make)


# ------------------------------------------------------------------------------------------------- 4: the plaintext product
def lift(L, p, i: int, variant: str | None = None) -> np.ndarray:
    """uint64[n]: SEAL's centred lift of plaintext coefficients to data prime i: v >= ceil(t / 2) -> v + q_i - t.  Variant "gt"
    (a mutation): '>' for '>=' at ceil(t / 2)."""
    t, q = L.t, L.primes[i]
    up = (t + 1) // 2
    v = _obj(p)
    return _u64(np.where(v > up if variant == "gt" else v >= up, v + q - t, v))


def edge_plaintext(L, salt: int) -> np.ndarray:
    """uint64[n]: random coefficients below t with 0, 1, t - 1, floor(t / 2) and ceil(t / 2) among them (several times each): no
    monomial, so no route takes the monomial shortcut."""
    rng = L.rng(7100 + salt)
    t = L.t
    p = rng.integers(0, t, L.n, dtype=np.uint64)
    edge = np.array([0, 1, t - 1, t // 2, (t + 1) // 2], dtype=np.uint64)
    at = rng.permutation(L.n)[:20]
    p[at] = edge[np.arange(20) % 5]
    assert int((p != 0).sum()) >= 2
    for v in edge:
        assert (p == v).any()
    return p


def plain_transform(L, p, variant: str | None = None) -> np.ndarray:
    """uint64[K][n]: NTT(lift p) per data prime (the oracle's transform of this file's lift)."""
    return np.stack([L.o.ntt(i, lift(L, p, i, variant)) for i in range(L.K)])


def _inverse_words(row, q: int) -> np.ndarray:
    """object[n]: the inverse mod q of every word (none is 0; n a power of two), with ONE modular inversion: a tree of pairwise
    products up to the product of all words, its inverse, and back down (the inverse of a left child is the parent's inverse times
    the right child)."""
    levels = [_obj(row)]
    while len(levels[-1]) > 1:
        a = levels[-1]
        levels.append(a[0::2] * a[1::2] % q)
    inv = np.array([pow(int(levels[-1][0]), -1, q)], dtype=object)
    for a in reversed(levels[:-1]):
        down = np.empty(len(a), dtype=object)
        down[0::2], down[1::2] = inv * a[1::2] % q, inv * a[0::2] % q
        inv = down
    return inv


def land_multiply_plain(L, p, T, where: str):
    """(ct uint64[size][K][n], want): the ciphertext that puts the target T (uint64[size][K][n]) at one place of multiply_plain(ct, p).
    "output": ct = INTT(NTT(T) / NTT(lift p)), the product's output is T (want = T).  "product": the same construction stated
    for the word in front of the inverse transform, c^ (.) p^ = T, so ct = INTT(T / p^) and the output is INTT(T) (want).
    "forward": ct = INTT(T), the forward half hands T to the product; want is None (the oracle's product is the reference)."""
    size = T.shape[0]
    pn = plain_transform(L, p)
    assert (pn != 0).all(), "NTT(lift p) has a zero word: choose another plaintext"
    ct = np.zeros((size, L.K, L.n), dtype=np.uint64)
    want = None if where == "forward" else np.zeros_like(ct)
    for i, q in enumerate(L.primes):
        inv = None if where == "forward" else _inverse_words(pn[i], q)
        for c in range(size):
            if where == "forward":
                ct[c, i] = L.o.ntt(i, T[c, i], inverse=True)
                continue
            That = L.o.ntt(i, T[c, i]) if where == "output" else T[c, i]
            ct[c, i] = L.o.ntt(i, _u64(_obj(That) * inv % q), inverse=True)
            want[c, i] = T[c, i] if where == "output" else L.o.ntt(i, T[c, i], inverse=True)
    return ct, want


WHERES = ("output", "forward", "product")


def multiply_plain_case(L, size: int, items: int = 3, salt: int = 0):
    """(cts uint64[items][size][K][n], plains uint64[items][n], want uint64[items][size][K][n], names): item k is landed at
    WHERES[k % 3] with its own edge plaintext and its own phase of the pattern; where items > 3, item 3 lands the output on
    polynomial 0 all q - 1 and polynomial 1 zero but one word.  want is the oracle's product, asserted equal to the target where
    the builder names one."""

    def make():
        P, n = L.primes, L.n
        cts, plains, wants, names = [], [], [], []
        for k in range(items):
            where = WHERES[k % 3]
            p = edge_plaintext(L, 10 * salt + k)
            T = LD.pattern(P, size, n, 2 * k + salt)
            if k == 3:
                T[0] = LD.constant(P, n, lambda q: q - 1)
                T[1] = np.stack([unit(q, n, 3 + i) for i, q in enumerate(P)])
            ct, want = land_multiply_plain(L, p, T, where)
            ref = L.o.multiply_plain(ct, p)
            assert want is None or (ref == want).all(), (L.pid, where, "does not land")
            cts.append(ct), plains.append(p), wants.append(ref), names.append(where)
        return np.stack(cts), np.stack(plains), np.stack(wants), names

    return L.cached(("multiply_plain", size, items, salt), make)


def shared_plain_case(L, size: int, items: int = 3):
    """(cts, plain uint64[n], want, names): as multiply_plain_case with ONE plaintext for every item."""

    def make():
        P, n = L.primes, L.n
        p = edge_plaintext(L, 99)
        cts, wants, names = [], [], []
        for k in range(items):
            where = WHERES[k % 3]
            ct, want = land_multiply_plain(L, p, LD.pattern(P, size, n, 3 * k + 1), where)
            ref = L.o.multiply_plain(ct, p)
            assert want is None or (ref == want).all(), (L.pid, where, "does not land")
            cts.append(ct), wants.append(ref), names.append(where)
        return np.stack(cts), p, np.stack(wants), names

    return L.cached(("multiply_plain shared", size, items), make)


# ------------------------------------------------------------------------------------------------------------- 5: encode
def land_encode(L, Tp):
    """(unsigned uint64[n], signed int64[n]): the slot values whose encoding has the COEFFICIENTS Tp (uint64[n], below t)."""
    v = L.o.batch_decode(_u64(Tp))
    s = v.astype(np.int64)
    s[v > np.uint64(L.t >> 1)] -= L.t
    return v, s


def encode_targets(L, items: int = 2) -> np.ndarray:
    """uint64[items][n]: coefficient patterns over targets(t), another phase per item; the last item is all t - 1 but one 0."""
    t, n = L.t, L.n
    out = np.stack([np.array(LD.targets(t), dtype=np.uint64)[(np.arange(n) + 2 * k) % 5] for k in range(items)])
    out[-1, :] = t - 1
    out[-1, n // 3] = 0
    return out


# ----------------------------------------------------------------------------------------------------------- 6: mod-switch
def last_values(ql: int) -> list[int]:
    """The last-prime residues both sides of the + h wrap (q_last = 2 h + 1: x + h reaches q_last at x = h + 1)."""
    h = ql // 2
    return [0, 1, h - 1, h, h + 1, h + 2, ql - 1]


def _level(L):
    """The data level seen as client_landing's models see the key level: the prime divided by is the LAST DATA prime."""
    ql = L.primes[-1]
    return types.SimpleNamespace(qsp=ql, h=ql // 2, primes=L.primes[:-1])


def mod_switch_rns(L, ct, variant: str | None = None) -> np.ndarray:
    """uint64[size][K - 1][n]: divide_and_round_q_last residue by residue (client_landing's statement of it, with the last data prime
    in the special prime's place).  Variants (mutations): "no_half", "truncate", "no_reduce64" as described there."""
    lv = _level(L)
    return _u64(np.stack([np.stack([CL._divide_row(lv, ct[c][j], ct[c][L.K - 1], j, variant) for j in range(L.K - 1)]) for c in range(len(ct))]))


def mod_switch_integers(L, ct) -> np.ndarray:
    """uint64[size][K - 1][n]: floor((X + h) / q_last) mod q_j of the CRT lift X of all K rows."""
    ql = L.primes[-1]
    out = []
    for c in range(len(ct)):
        W = (CL.crt_lift(L.primes, ct[c]) + ql // 2) // ql
        out.append(np.stack([W % q for q in L.primes[:-1]]))
    return _u64(np.stack(out))


def no_reduce64_applies(L) -> bool:
    """Whether leaving out the reduction of the last-prime residue mod q_j can make a 64-bit subtraction wrap (client_landing's
    condition with the last data prime as the divisor)."""
    ql = L.primes[-1]
    return any(ql - 1 - (ql // 2) % q > q for q in L.primes[:-1])


def relations(L) -> set:
    """{"above", "below"}: how the last data prime stands to the lower ones (mod_switch_kernel reduces the last-prime residue
    mod q_j only where q_last > q_j)."""
    ql = L.primes[-1]
    return {"above" if ql > q else "below" for q in L.primes[:-1]}


def mod_switch_case(L, size: int = 2):
    """(ct uint64[2][size][K][n], want uint64[2][size][K - 1][n]): item 0 switches to the five-target pattern in every lower row,
    item 1 to q_j - 1 everywhere; the last-prime rows cycle last_values (another phase per polynomial: 5 and 7 are coprime, every
    pair of a target and a last value occurs).  The two integer statements must agree, and every class must occur, before the
    device is looked at."""

    def make():
        P, K, n = L.primes, L.K, L.n
        low = P[: K - 1]
        ql = P[-1]
        edge = np.array(last_values(ql), dtype=np.uint64)
        last = np.stack([edge[(np.arange(n) + 3 * c) % 7] for c in range(size)])
        T = np.stack([LD.pattern(low, size, n, 1), np.stack([LD.constant(low, n, lambda q: q - 1)] * size)])
        cts = []
        for it in range(2):
            polys = [CL.land_mod_switch(L, T[it][[c, c]], last[[c, c]])[0] for c in range(size)]
            cts.append(np.stack(polys))
        ct = np.stack(cts)
        for it in range(2):
            got = mod_switch_rns(L, ct[it])
            assert (got == mod_switch_integers(L, ct[it])).all(), "the two statements of the mod-switch disagree"
            assert (got == T[it]).all(), "the mod-switch does not land"
        for c in range(size):
            for v in edge:
                assert (ct[:, c, K - 1] == v).any(), ("last-prime residue", c, int(v))
            for j, q in enumerate(low):
                for k, tv in enumerate(LD.targets(q)):
                    at = T[0, c, j] == np.uint64(tv)
                    assert len(set(ct[0, c, K - 1][at].tolist())) == 7, ("every last value at target", c, j, k)
            assert all((T[1, c, j] == np.uint64(q - 1)).all() for j, q in enumerate(low))
        return ct, T

    return L.cached(("mod_switch", size), make)
