"""What the row-rotation planner must decide, derived without the library and without SEAL's digit loop: the sweeps of
tests/test_rotation_items_cpu.py and tests/test_rotation_items_keys_cpu.py compare the library's plans against this.

The non-adjacent form comes from the identity 3v = 2v + v: where the bits of v >> 1 and of v + (v >> 1) differ there is a
digit, +1 if the bit is set in the sum and -1 if it is set in v >> 1 (Prodinger, "On binary representations of integers with
digits -1, 0, 1").  No recurrence over v mod 4 is involved."""
import functools

INT_MAX, INT_MIN = 2**31 - 1, -(2**31)
COPY, DIRECT, CHAIN = 0, 1, 2
TOO_LARGE, NO_KEY = "step count", "key"  # refusals: what the message speaks of
DEGREES = (8, 16, 64, 4096)


@functools.lru_cache(maxsize=None)
def elt(step, n):
    """The Galois element of a row rotation: 3^step for a left rotation, 3^(n/2 - |step|) for a right one (mod 2n)."""
    assert 0 < abs(step) < n // 2
    return pow(3, step if step > 0 else n // 2 - abs(step), 2 * n)


@functools.lru_cache(maxsize=None)
def naf(step):
    """The parts of the step's non-adjacent form, least significant first, the step's sign carried by every part."""
    v = abs(step)
    half, total = v >> 1, v + (v >> 1)
    digit = half ^ total
    sign = -1 if step < 0 else 1
    parts = [sign * (1 if (total >> i) & 1 else -1) * (1 << i) for i in range(digit.bit_length()) if (digit >> i) & 1]
    assert sum(parts) == step and all(abs(a) * 2 < abs(b) for a, b in zip(parts, parts[1:])), (step, parts)
    return parts


@functools.lru_cache(maxsize=None)
def hops(step, n):
    """The chain's hops: the parts without the part of n/2 rows (the identity on the rows)."""
    return [p for p in naf(step) if abs(p) != n // 2]


def expected(n, step, held):
    """(COPY | DIRECT | CHAIN, hops of the chain) or (TOO_LARGE | NO_KEY, 0) over a holding of Galois elements."""
    if step == 0:
        return COPY, 0
    if abs(step) >= n // 2:
        return TOO_LARGE, 0
    if elt(step, n) in held:
        return DIRECT, 0
    chain = hops(step, n)
    if len(naf(step)) < 2 or any(elt(p, n) not in held for p in chain):
        return NO_KEY, 0
    return CHAIN, len(chain)


def sweep_steps(n):
    """Every step in (-n/2, n/2), then the steps that must be refused."""
    return list(range(-n // 2 + 1, n // 2)) + [n // 2, -n // 2, n // 2 + 1, INT_MIN, INT_MAX]


def pow2(n):
    """The elements of the steps +-2^i below n/2, in the order (+1, -1, +2, -2, ...)."""
    return [elt(s * (1 << i), n) for i in range((n // 2).bit_length() - 1) for s in (1, -1)]


def holdings(n):
    """(name, held elements): every +-2^i key, then that set with one power removed -- each power in turn at the small degrees;
    at n = 4096 the key of +4 (a middle hop), of -1 (the first hop, and the element of n/2 - 1) and of n/4 (the last hop, which +n/4
    and -n/4 share)."""
    all_pow2 = frozenset(pow2(n))
    yield "pow2", all_pow2
    for step in [s * (1 << i) for i in range((n // 2).bit_length() - 1) for s in (1, -1)] if n <= 64 else (4, -1, n // 4):
        yield "pow2 without the key of %+d" % step, all_pow2 - {elt(step, n)}


def batches(steps, size=64):
    return [steps[i:i + size] for i in range(0, len(steps), size)]
