"""Mixed-step rotation batches with one key set per client: hipbfv_batch_rotate_rows_items_keys / hipbfv_batch_apply_galois_items_keys
rotate item i by its own step (element) through its own client's key set.  Every result is judged word for word against
hipbfv_batch_rotate_rows (hipbfv_batch_apply_galois) called on that item ALONE with its client's set -- the calls the existing suite
pins to the CPU oracle -- and every client decrypts and decodes its own items to the rows rolled by the item's step.

Main shape: n = 4096, the default primes (K = 2 + 1), three clients made by the library's seeded key generator:
  A holds the direct key of every step used here (and the powers of two, and the column key),
  B holds the power-of-two keys and the column key only,
  C holds B's keys plus the direct key of step 5.
So step 3 is direct for A and a chain for B and C in the same call, step 5 direct for A and C, step 7 a chain for B."""
import re

import numpy as np
import pytest

from tests.bfv_helpers import params
from tests.test_gpu_rotation_steps import E_INVALIDARG, SENTINEL, _rolled, _slots

pytestmark = pytest.mark.gpu

NAME = "default_4096_16"
N, H = 4096, 2048
A, B, C = 0, 1, 2
# 13 items, ungrouped: neither the steps nor the clients come in runs
STEPS = [3, 3, 0, 1, 5, -1, 7, H - 1, 3, -(H - 1), 5, 0, 7]
CLIENTS = [A, B, B, C, C, A, B, A, C, B, A, C, A]
assert len(STEPS) == len(CLIENTS) == 13 and set(STEPS) == {0, 1, -1, 3, 5, 7, H - 1, -(H - 1)}
DIRECT_OF = {A: (3, 5, 7), B: (), C: (5,)}


def _pow2_steps(n, most=None):
    steps = [s * (1 << i) for i in range((n // 2).bit_length() - 1) for s in (1, -1)]
    return [s for s in steps if most is None or abs(s) <= most]


class _Client:
    def __init__(self, ctx, seed, steps):
        from sunscreen_amd.seal import KeyGenerator

        gen = KeyGenerator(ctx, seed=seed)
        self.sk = gen.secret_key()
        self.pk = gen.create_public_key()
        self.gk = gen.create_galois_keys(steps=list(steps))  # step 0: the column key


class _World:
    """One context, its clients, one ciphertext per item under its own client's public key, and the single-item references,
    each computed once."""

    def __init__(self, name, holdings, steps, clients, seed):
        import torch
        from sunscreen_amd import Context
        from sunscreen_amd.batch import BatchEvaluator

        n, primes, t = params(name)
        self.n, self.t = n, t
        self.ctx = Context.from_raw(n, primes, t)
        self.ev = BatchEvaluator(self.ctx)
        self.clients = [_Client(self.ctx, seed + k, held) for k, held in enumerate(holdings)]
        self.sets = [c.gk for c in self.clients]
        self.steps, self.key_index = list(steps), np.asarray(clients, dtype=np.uint32)
        self.vals = [_slots(n, t, j) for j in range(len(steps))]
        cts = []
        for j, k in enumerate(clients):
            v = torch.from_numpy(self.vals[j].astype(np.int64)).cuda()[None]
            cts.append(self.ev.encrypt(self.ev.encode(v), self.clients[k].pk, seed=900 + j))
        self.dev = torch.cat(cts)
        self._refs = {}

    def ref(self, item, step, client):
        """hipbfv_batch_rotate_rows on that item alone with that client's set."""
        key = (item, step, client)
        if key not in self._refs:
            self._refs[key] = self.ev.rotate_rows(self.dev[item : item + 1], step, self.sets[client])[0].clone()
        return self._refs[key]

    def refs(self, steps=None, clients=None):
        import torch

        steps = self.steps if steps is None else steps
        clients = self.key_index if clients is None else clients
        return torch.stack([self.ref(i, s, int(k)) for i, (s, k) in enumerate(zip(steps, clients))])

    def decoded(self, ct, client):
        """The client's own view of one result: decrypt and decode with its secret key."""
        return self.ev.decode(self.ev.decrypt(ct[None], self.clients[client].sk))[0].cpu().numpy().astype(np.uint64)


_WORLDS = {}


@pytest.fixture(scope="module", autouse=True)
def _shared_worlds():
    yield
    _WORLDS.clear()


def main_world() -> _World:
    if "main" not in _WORLDS:
        pow2 = _pow2_steps(N) + [0]
        _WORLDS["main"] = _World(NAME, [pow2 + list(DIRECT_OF[A]), pow2, pow2 + list(DIRECT_OF[C])], STEPS, CLIENTS, seed=3100)
    return _WORLDS["main"]


def _refused(call):
    from sunscreen_amd import HipBfvError

    with pytest.raises(HipBfvError) as e:
        call()
    return e.value.hresult & 0xFFFFFFFF, str(e.value)


def _poisoned(w):
    import torch

    return torch.full_like(w.dev, SENTINEL)


class _Foreign:
    """A live handle that is no key object."""

    def __init__(self):
        from sunscreen_amd.program import FheProgram

        self._p = FheProgram()

    def get_handle(self):
        return self._p._h


# ---- main shape --------------------------------------------------------------------------------------------------------------
def test_the_plan_of_the_main_batch_mixes_decisions():
    """What the tests below run: direct and chain decisions for one step in one call (host plan over the clients' holdings)."""
    from sunscreen_amd.batch import rotate_items_keys_plan

    elt = lambda s: pow(3, s if s > 0 else H - abs(s), 2 * N)  # noqa: E731
    held = [[elt(s) for s in _pow2_steps(N) + list(DIRECT_OF[k])] for k in (A, B, C)]
    kind, entry, rounds_of, entries, rounds = rotate_items_keys_plan(N, STEPS, CLIENTS, held)
    assert kind == [1, 2, 0, 1, 1, 1, 2, 1, 2, 1, 1, 0, 1]
    assert rounds == 2 and [rounds_of[i] for i in (1, 6, 8)] == [2, 2, 2]
    assert entries == len({(elt(s), k) for s, k, d in zip(STEPS, CLIENTS, kind) if d == 1})


def test_every_item_has_the_words_of_its_own_single_call_and_decodes_for_its_client():
    import torch

    w = main_world()
    before = w.dev.clone()
    out = w.ev.rotate_rows_items_keys(w.dev, w.steps, w.sets, w.key_index)
    torch.cuda.synchronize()
    assert torch.equal(w.dev, before), "the input of an out-of-place call changed"
    ref = w.refs()
    for i, (s, k) in enumerate(zip(w.steps, w.key_index)):
        assert torch.equal(out[i], ref[i]), (i, s, int(k))
        assert (w.decoded(out[i], int(k)) == _rolled(w.vals[i], s)).all(), (i, s, int(k))
    w.ev.check()  # hipbfv_batch_status stays clean


def test_permuting_the_batch_permutes_the_output():
    import torch

    w = main_world()
    ref = w.refs()
    for seed in (1, 2):
        perm = np.random.default_rng(seed).permutation(len(w.steps))
        out = w.ev.rotate_rows_items_keys(w.dev[torch.from_numpy(perm).cuda()].contiguous(), [w.steps[p] for p in perm], w.sets, w.key_index[perm])
        assert torch.equal(out, ref[torch.from_numpy(perm).cuda()]), seed
    # grouped by client, and grouped by step: the same words
    for order in (np.argsort(w.key_index, kind="stable"), np.argsort(w.steps, kind="stable")):
        idx = torch.from_numpy(order).cuda()
        out = w.ev.rotate_rows_items_keys(w.dev[idx].contiguous(), [w.steps[p] for p in order], w.sets, w.key_index[order])
        assert torch.equal(out, ref[idx])
    w.ev.check()


def test_in_place_takes_the_grouped_path_and_gives_the_same_words():
    import torch

    w = main_world()
    buf = w.dev.clone()
    w.ev.profile(True)
    w.ev.profile_reset()
    try:
        got = w.ev.rotate_rows_items_keys(buf, w.steps, w.sets, w.key_index, out=buf)
        torch.cuda.synchronize()
        seen = {k: v["launches"] for k, v in w.ev.profile_read().items()}
    finally:
        w.ev.profile(False)
    assert got.data_ptr() == buf.data_ptr()
    assert torch.equal(buf, w.refs())
    # the direct items went group by group, one per (key, element) pair: more than one key-switch sequence
    assert seen.get("ks_mid", 0) > 1, seen
    # any other overlap is refused before anything is written
    wide = torch.cat([w.dev, w.dev[:1]])
    keep = wide.clone()
    hr, msg = _refused(lambda: w.ev.rotate_rows_items_keys(wide[:-1], w.steps, w.sets, w.key_index, out=wide[1:]))
    assert hr == E_INVALIDARG and torch.equal(wide, keep), msg
    w.ev.check()


def test_out_of_place_direct_items_share_one_launch_sequence_and_chains_share_their_rounds():
    """13 items, 3 clients, 8 steps: ONE head / middle / tail sequence for all direct items, then one per round (two rounds) for all
    chain items together -- 3 sequences, whatever the number of (set, step) pairs."""
    import torch

    w = main_world()
    w.ev.profile(True)
    w.ev.profile_reset()
    try:
        w.ev.rotate_rows_items_keys(w.dev, w.steps, w.sets, w.key_index)
        torch.cuda.synchronize()
        seen = {k: v["launches"] for k, v in w.ev.profile_read().items()}
    finally:
        w.ev.profile(False)
    assert seen.get("ks_head") == 3 and seen.get("ks_mid") == 3 and seen.get("ks_tail") == 3, seen
    assert "galois" not in seen, seen


def test_an_unreferenced_null_or_foreign_set_is_tolerated():
    """Sets no rotating item names: a NULL entry, a live handle that is no key object, and the set of a client whose items all copy."""
    import torch

    w = main_world()
    foreign = _Foreign()
    sets = [w.sets[A], None, foreign, w.sets[B], w.sets[C], None]
    remap = {A: 0, B: 3, C: 4}
    key_index = np.array([remap[int(k)] for k in w.key_index], dtype=np.uint32)
    # the copied items (step 0) name the NULL and the foreign entries: a copy references no set
    zeros = [i for i, s in enumerate(w.steps) if s == 0]
    key_index[zeros[0]], key_index[zeros[1]] = 1, 2
    out = w.ev.rotate_rows_items_keys(w.dev, w.steps, sets, key_index)
    assert torch.equal(out, w.refs())
    w.ev.check()


@pytest.mark.parametrize("case", ["step +n/2", "step -n/2", "key_index", "null set", "foreign set", "other context", "chain key missing", "key_index of a copy"])
def test_every_refusal_names_the_item_and_the_set_and_writes_nothing(case):
    import torch
    from sunscreen_amd import Context
    from sunscreen_amd.seal import KeyGenerator

    w = main_world()
    steps, sets, key_index = list(w.steps), list(w.sets), w.key_index.copy()
    if case.startswith("step"):
        item, k = 6, int(key_index[6])
        steps[item] = H if "+" in case else -H
    elif case == "key_index":
        item, k = 4, 3
        key_index[item] = 3
    elif case == "key_index of a copy":
        item, k = 2, 7
        assert steps[item] == 0
        key_index[item] = 7
    elif case == "null set":
        item, k = 1, B  # the first item that needs a key of B
        sets[B] = None
    elif case == "foreign set":
        item, k = 3, C
        sets[C] = _Foreign()
    elif case == "other context":
        n, primes, t = params(NAME)
        other = Context.from_raw(n, primes, t)
        item, k = 0, A
        sets[A] = KeyGenerator(other, seed=5).create_galois_keys(steps=[3])
    else:  # a set with the keys of 1, -1, 2, -2 alone: 3 = [-1, 4] lacks the key of 4; 1 and -1 are served
        item, k = 1, B
        sets[B] = KeyGenerator(w.ctx, seed=6).create_galois_keys(steps=[1, -1, 2, -2])
    out = _poisoned(w)
    hr, msg = _refused(lambda: w.ev.rotate_rows_items_keys(w.dev, steps, sets, key_index, out=out))
    torch.cuda.synchronize()
    assert hr == E_INVALIDARG and re.search(rf"item {item}: key set {k}: ", msg), (case, hex(hr), msg)
    assert bool((out == SENTINEL).all()), case
    w.ev.check()


def test_galois_elements_per_item_over_two_clients():
    """apply_galois_items_keys: the identity, element 3 (step 1), the column element 2N - 1 and the odd non-power elements 27 (step 3,
    A's direct key) and 243 (step 5: A's and C's) over A and C; an even or too large element and a key a set lacks are refused."""
    import torch

    w = main_world()
    col = 2 * N - 1
    elts = [1, 3, col, 27, 3, col, 243, 243]
    who = np.array([C, A, C, A, C, A, C, A], dtype=np.uint32)
    ct = w.dev[: len(elts)]
    out = w.ev.apply_galois_items_keys(ct, elts, w.sets, who)
    for i, (e, k) in enumerate(zip(elts, who)):
        want = ct[i] if e == 1 else w.ev.apply_galois(ct[i : i + 1], e, w.sets[int(k)])[0]
        assert torch.equal(out[i], want), (i, e, int(k))
    inplace = ct.clone()
    w.ev.apply_galois_items_keys(inplace, elts, w.sets, who, out=inplace)
    assert torch.equal(inplace, out)
    for bad, item, k, elts2, who2 in ((2, 1, A, [1, 2] + elts[2:], who), (2 * N + 1, 2, C, elts[:2] + [2 * N + 1] + elts[3:], who),
                                      (27, 3, C, elts, np.array([C, A, C, C, C, A, C, A], dtype=np.uint32))):
        poisoned = torch.full_like(ct, SENTINEL)
        hr, msg = _refused(lambda: w.ev.apply_galois_items_keys(ct, elts2, w.sets, who2, out=poisoned))
        assert hr == E_INVALIDARG and f"item {item}: key set {k}: " in msg, (bad, msg)
        assert bool((poisoned == SENTINEL).all()), bad
    w.ev.check()


def test_the_same_element_for_two_clients_takes_each_clients_own_key():
    """The same ciphertext words twice, the same step, two clients, both through a direct key: were the key table keyed by element
    alone, both items would come out alike.  Both orders, so that neither client is 'the first item of that element'."""
    import torch

    w = main_world()
    ct = torch.stack([w.dev[4], w.dev[4]])
    one = {k: w.ev.rotate_rows(ct[:1], 5, w.sets[k])[0] for k in (A, C)}
    assert not torch.equal(one[A], one[C])
    for order in ([A, C], [C, A]):
        out = w.ev.rotate_rows_items_keys(ct, [5, 5], w.sets, order)
        for i, k in enumerate(order):
            assert torch.equal(out[i], one[k]), (order, i)
        gal = w.ev.apply_galois_items_keys(ct, [243, 243], w.sets, order)
        assert torch.equal(gal, out), order
    # and as chains: step 3 through B's and C's own power-of-two keys
    chain = {k: w.ev.rotate_rows(ct[:1], 3, w.sets[k])[0] for k in (B, C)}
    assert not torch.equal(chain[B], chain[C])
    out = w.ev.rotate_rows_items_keys(ct, [3, 3], w.sets, [C, B])
    assert torch.equal(out[0], chain[C]) and torch.equal(out[1], chain[B])
    w.ev.check()


def test_count_zero_and_parameters_without_batching():
    import torch
    from sunscreen_amd import Context
    from sunscreen_amd.batch import BatchEvaluator

    import ctypes as C

    from sunscreen_amd import _lib

    w = main_world()
    out = _poisoned(w)
    hs = (C.c_void_p * 1)(None)
    for fn, per_item in ((_lib.load().hipbfv_batch_rotate_rows_items_keys, (C.c_int32 * 1)(1)), (_lib.load().hipbfv_batch_apply_galois_items_keys, (C.c_uint32 * 1)(3))):
        assert fn(w.ev._h, C.c_void_p(w.dev.data_ptr()), per_item, hs, 1, (C.c_uint32 * 1)(0), C.c_void_p(out.data_ptr()), 0, None) == 0
    torch.cuda.synchronize()
    assert bool((out == SENTINEL).all())
    n, primes, _ = params("simple_multiply")  # t = 262144: no batching
    ev = BatchEvaluator(Context.from_raw(n, primes, 262144))
    ct = torch.zeros((1, 2, ev.K, n), dtype=torch.int64, device="cuda")
    hr, msg = _refused(lambda: ev.rotate_rows_items_keys(ct, [1], [None], [0]))
    assert hr == 0x80131509 and "batching" in msg, (hex(hr), msg)


# ---- n = 8192: a chunk boundary, chains of unequal length, the skipped part -----------------------------------------------------
def test_n8192_chunks_of_four_and_chains_of_two_to_six_rounds():
    """9 items in chunks of 4 (4, 4, 1), 2 clients: A holds the direct keys of 11 and 3, B the powers of two alone.  B's chains:
    3 = [-1, 4] (2 rounds), 11 = [-1, -4, 16] (3), 85 = [1, 4, 16, 64] (4), 4093 = [1, -4, n/2 skipped] (2), 1365 (6 rounds): items
    finish in different rounds and in both stages, and the chain items themselves go in blocks of 4."""
    import torch

    name, n = "default_8192_17", 8192
    if name not in _WORLDS:
        pow2 = _pow2_steps(n) + [0]
        steps = [11, 3, 85, 0, 11, 1365, 4093, 3, -1]
        clients = [B, A, B, A, A, B, B, B, A]
        _WORLDS[name] = _World(name, [pow2 + [11, 3], pow2], steps, clients, seed=3200)
    from sunscreen_amd.batch import BatchEvaluator

    w = _WORLDS[name]
    ev4 = BatchEvaluator(w.ctx)  # (the world's own evaluator keeps the default chunk for the single-item references)
    ev4.set_chunk_ops(4)
    out = ev4.rotate_rows_items_keys(w.dev, w.steps, w.sets, w.key_index)
    inplace = w.dev.clone()
    ev4.rotate_rows_items_keys(inplace, w.steps, w.sets, w.key_index, out=inplace)
    ev4.check()
    ref = w.refs()
    for i, (s, k) in enumerate(zip(w.steps, w.key_index)):
        assert torch.equal(out[i], ref[i]), (i, s, int(k))
        assert torch.equal(inplace[i], ref[i]), ("in place", i, s, int(k))
        assert (w.decoded(out[i], int(k)) == _rolled(w.vals[i], s)).all(), (i, s, int(k))
    w.ev.check()


# ---- n = 16384: per-key-prime digit packing ----------------------------------------------------------------------------------------
def test_n16384_five_items_two_clients():
    import torch

    name = "default_16384_17"
    if name not in _WORLDS:
        few = [1, -1, 4, -4, 16, -16, 0]  # the keys the chains below read (a whole power-of-two set is 27 keys of 18 MiB)
        _WORLDS[name] = _World(name, [few + [3], few], [3, 3, 0, 11, -1], [A, B, B, B, A], seed=3300)
    w = _WORLDS[name]
    out = w.ev.rotate_rows_items_keys(w.dev, w.steps, w.sets, w.key_index)
    ref = w.refs()
    for i, (s, k) in enumerate(zip(w.steps, w.key_index)):
        assert torch.equal(out[i], ref[i]), (i, s, int(k))
        assert (w.decoded(out[i], int(k)) == _rolled(w.vals[i], s)).all(), (i, s, int(k))
    w.ev.check()
