"""Row rotations of the CPU oracle at the edges of the step range, judged by what a rotation MEANS and by a hop order that
shares no code with the oracle's NAF loop.

`o.rotate_rows` restates SEAL's rotate_internal: the key of the step if it is there, else the non-adjacent form (NAF) of the
step, low digit first, as power-of-two rotations, a part of exactly n/2 rows skipped.  The library holds the same loop six
times and is judged against the oracle bit for bit (tests/test_gpu_rotation_steps.py), so an error made in both would be
invisible there.  Here the oracle answers to two things that know nothing of that loop: the decoded slots (both rows of the
slot matrix rolled by the step) and a chain of single hops whose order comes from the digits of (3|s|) xor |s|.

Two facts about the edge steps that the tests pin because they are easy to get wrong:
  * a step of n/2 - 2^k has the Galois element of step -2^k (3^(n/2 - 2^k)): with the power-of-two keys it is ONE hop through
    that key, and its NAF [-2^k, +n/2] is never walked;
  * the skipped n/2 part is reached by the other steps above n/3, e.g. n/2 - 3 = [+1, -4, +n/2] and 1707 at n = 4096
    = [-1, -4, -16, -64, -256, +n/2]: their elements are no power-of-two step's.
"""
import functools

import numpy as np
import pytest

from oracle import bfv_oracle as O
from tests.bfv_helpers import oracle_for

INT_MAX, INT_MIN = 2**31 - 1, -(2**31)


def naf_hops(step: int, n: int) -> list[int]:
    """The power-of-two rotations a chain by `step` makes, in order.  For x = |step| the NAF digit i is
    bit i + 1 of 3x minus bit i + 1 of x: non-zero where 3x and x differ there, negative where the bit is x's.  Low digit
    first; the sign of the step applied afterwards; a part of n/2 rows dropped."""
    x = abs(step)
    hops = []
    for i in range((3 * x).bit_length()):
        if ((3 * x ^ x) >> (i + 1)) & 1:
            hops.append(-(1 << i) if (x >> (i + 1)) & 1 else 1 << i)
    assert sum(hops) == x and all(abs(b) >= 4 * abs(a) for a, b in zip(hops, hops[1:])), (step, hops)  # non-adjacent
    if step < 0:
        hops = [-p for p in hops]
    return [p for p in hops if abs(p) != n // 2]


def test_the_independent_naf_on_known_decompositions():
    """The construction above against decompositions written out by hand (n = 4096, n/2 = 2048)."""
    n = 4096
    assert naf_hops(2047, n) == [-1]  # [-1, +2048]
    assert naf_hops(-2047, n) == [1]
    assert naf_hops(2046, n) == [-2]
    assert naf_hops(2045, n) == [1, -4]  # [+1, -4, +2048]
    assert naf_hops(1025, n) == [1, 1024]
    assert naf_hops(1365, n) == [1, 4, 16, 64, 256, 1024]
    assert naf_hops(-683, n) == [1, 4, 16, 64, 256, -1024]
    assert naf_hops(1707, n) == [-1, -4, -16, -64, -256]  # ... +2048 skipped
    assert naf_hops(11, n) == [-1, -4, 16]
    assert naf_hops(-11, n) == [1, 4, -16]
    assert naf_hops(-13, n) == [-1, 4, -16]
    assert naf_hops(7, n) == [-1, 8] and naf_hops(3, n) == [-1, 4] and naf_hops(-5, n) == [-1, -4]
    assert naf_hops(1024, n) == [1024] and naf_hops(1, n) == [1] and naf_hops(0, n) == []


def _slots(o):
    """Two rows that differ and are not periodic: a wrong step or a swapped row cannot decode to the expected roll."""
    return (3 * np.arange(o.n, dtype=np.uint64) + 1) % np.uint64(o.t)


def _rolled(v, step):
    h = v.size // 2
    return np.concatenate([np.roll(v[:h], -step), np.roll(v[h:], -step)])


def _decoded(o, ct, sk):
    return o.batch_decode(o.decrypt(ct, sk))


def test_every_step_at_toy_64_decodes_to_the_rolled_rows():
    """n = 64, every step in (-32, 32) over the power-of-two keys: both rows rolled by the step, the budget barely touched."""
    o = oracle_for("toy_64")
    assert (o.n, o.t) == (64, 257)
    h = o.n // 2
    O.seed(3)
    sk, pk, _, gk = o.keygen(relin=False, galois_elts="all")
    v = _slots(o)
    assert (v[:h] != v[h:]).any()
    ct = o.encrypt(pk, o.batch_encode(v))
    fresh = o.noise_budget(ct, sk)
    assert fresh >= 57
    bad, worst = [], fresh
    for step in range(-h + 1, h):
        r = o.rotate_rows(ct, step, gk)
        worst = min(worst, o.noise_budget(r, sk))
        if not (_decoded(o, r, sk) == _rolled(v, step)).all():
            bad.append(step)
    assert not bad, bad
    assert worst >= 57, (fresh, worst)  # a key switch adds noise far below the 60-bit fresh budget
    for step in (h, -h, h + 1, -h - 1, INT_MAX, INT_MIN):
        with pytest.raises(RuntimeError, match="invalid argument"):
            o.rotate_rows(ct, step, gk)


# n = 4096, n/2 = 2048: the edge steps the GPU suite runs through every caller (tests/test_gpu_rotation_steps.py)
EDGE_STEPS = (2047, -2047, 2046, 2045, -2045, 1707, 1025, 1365, -683, 11, -11, -13, 1024, -1024, 1, -1, 0)
REFUSED_STEPS = (2048, -2048, 2049, -2049, INT_MAX, INT_MIN)


@functools.lru_cache(maxsize=None)
def _world_4096():
    o = oracle_for("default_4096_16")
    O.seed(4096)
    sk, pk, _, gk = o.keygen(relin=False, galois_elts="all")
    v = _slots(o)
    ct = o.encrypt(pk, o.batch_encode(v))
    return o, sk, gk, v, ct


@pytest.mark.parametrize("step", EDGE_STEPS)
def test_edge_steps_at_4096_decode_and_equal_the_chain_of_single_hops(step):
    o, sk, gk, v, ct = _world_4096()
    h = o.n // 2
    got = o.rotate_rows(ct, step, gk)
    assert (_decoded(o, got, sk) == _rolled(v, step)).all(), step
    # a hop adds key-switch noise of at most the fresh noise's size: six of them cost log2(7) < 3 bits, one bit of slack
    assert o.noise_budget(got, sk) >= o.noise_budget(ct, sk) - 4, step
    # hop by hop, every hop with a dictionary that holds that hop's key alone: order, signs and the skip, bit for bit
    hops = naf_hops(step, o.n)
    elt = o.galois_elt_from_step(step) if step else 0
    if elt in gk:  # the step's own key is there (a power of two, or n/2 - 2^k through the key of -2^k): one hop, no chain
        assert abs(step) in (1, 1024) or h - abs(step) in (1, 2), step
        assert len(hops) == 1 and o.galois_elt_from_step(hops[0]) == elt, (step, hops)
    cur = ct
    for part in hops:
        e = o.galois_elt_from_step(part)
        cur = o.rotate_rows(cur, part, {e: gk[e]})
    assert (got == cur).all(), (step, hops)
    if len(hops) > 1:  # the order matters to the bits: the reversed chain decodes alike and differs word for word
        rev = ct
        for part in reversed(hops):
            e = o.galois_elt_from_step(part)
            rev = o.rotate_rows(rev, part, {e: gk[e]})
        assert (_decoded(o, rev, sk) == _rolled(v, step)).all() and not (rev == got).all(), step


def test_the_steps_that_reach_the_skipped_part():
    """n/2 - 1 and n/2 - 2 never walk their NAF under the power-of-two keys (their element is that of -1 and -2); n/2 - 3 and
    1707 do, and the part of n/2 rows in it has no Galois element at all (galois_elt_from_step refuses it)."""
    o, sk, gk, v, ct = _world_4096()
    h = o.n // 2
    assert o.galois_elt_from_step(h - 1) == o.galois_elt_from_step(-1) and o.galois_elt_from_step(h - 2) == o.galois_elt_from_step(-2)
    assert o.galois_elt_from_step(-(h - 1)) == o.galois_elt_from_step(1)
    assert o.galois_elt_from_step(h) == 0 and o.galois_elt_from_step(-h) == 0
    for step in (h - 3, -(h - 3), 1707):
        assert o.galois_elt_from_step(step) not in gk, step
    # without the key of -1 the step n/2 - 1 has neither a direct key nor a chain
    lacking = {e: k for e, k in gk.items() if e != o.galois_elt_from_step(-1)}
    with pytest.raises(RuntimeError, match="missing key"):
        o.rotate_rows(ct, h - 1, lacking)
    # a chain reads the keys of ITS signs: without the key of +4, 11 = [-1, -4, 16] works and -11 = [1, 4, -16] does not
    no4 = {e: k for e, k in gk.items() if e != o.galois_elt_from_step(4)}
    assert (o.rotate_rows(ct, 11, no4) == o.rotate_rows(ct, 11, gk)).all()
    for step in (-11, 1365):
        with pytest.raises(RuntimeError, match="missing key"):
            o.rotate_rows(ct, step, no4)


@pytest.mark.parametrize("step", REFUSED_STEPS)
def test_steps_of_half_the_degree_and_beyond_are_refused(step):
    o, sk, gk, v, ct = _world_4096()
    with pytest.raises(RuntimeError, match="invalid argument"):
        o.rotate_rows(ct, step, gk)
    assert o.galois_elt_from_step(step) == 0
