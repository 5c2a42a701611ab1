"""The kernels either side of the evaluator (sunscreen_amd/csrc/kernels_client.hip) against integer models, bit for bit, on operands
crafted so that their own outputs land on the edges (tests/client_landing.py builds them and states the models;
tests/test_client_landing_cpu.py shows without a device that they land).

A / B  public-key encryption with a crafted public key: the divide-and-round by the special prime on both sides of its + h wrap,
       the data rows and the words after the division and after the plaintext addition on 0, q_j - 1 and 1, on the fused route
       (the batched encrypt and the handle's encrypt: encrypt_finish_kernel) and on the component-returning route
       (add_key_level_kernel -> ks_moddown_kernel -> add_plain).  u is recomputed from tests/rng_ref.py and must equal the device's
       in every coefficient; e is harvested from the device (the Gaussian is float arithmetic: its values are held against a
       float64 model in tests/test_gpu_keygen_model.py) and is asserted small, |e| <= 19, the one inequality of this file.
C      a batch against handle calls (first_op, a chunk boundary inside the batch, the shared plaintext, n = 32768) and the sampling
       counter across 2^32.
D      PolynomialArray's compose and decompose on crafted residues, every coefficient.  Decompose only ever sees limbs that compose
       produced (the API hands it nothing else): canonical values alone.
E      the encoder's signed edges.

Every "occurs at least once" condition is asserted on the host, on the reference alone, inside the builders, before a device
result is looked at."""
import numpy as np
import pytest

from tests import client_landing as CL
from tests import landing as LD
from tests.client_landing import client

pytestmark = pytest.mark.gpu

T_CASES_P1 = [2, (1 << 60) - 1]  # the r term needs the 128-bit product at the second (tests/test_gpu_landing.py: T_CASES)
ENC_CASES = [(pid, None) for pid in CL.ENCRYPT_SETS] + [("P1", t) for t in T_CASES_P1]
ENC_IDS = [f"{p}-t{t or 'batching'}" for p, t in ENC_CASES]


@pytest.fixture(scope="module", autouse=True)
def _drop():
    yield
    CL.drop_clients()


def _device(L):
    from sunscreen_amd import Context
    from sunscreen_amd.batch import BatchEvaluator

    ctx = Context.from_raw(L.n, L.key_primes, L.t)
    assert ctx.K == L.K and ctx.KK == L.KK and ctx.key_primes == L.key_primes
    return ctx, BatchEvaluator(ctx)


def _same(got, want, what):
    got, want = np.asarray(got), np.asarray(want)
    assert got.shape == want.shape, (what, got.shape, want.shape)
    bad = np.argwhere(got != want)
    assert bad.size == 0, (what, "first difference at", bad[0].tolist(), int(got[tuple(bad[0])]), int(want[tuple(bad[0])]), len(bad))


def _plaintext(m):
    from sunscreen_amd import Plaintext

    return Plaintext.from_coefficients([int(v) for v in m])


def _components(L, enc, m):
    """One component-returning handle call with the special prime in use: (ciphertext uint64[2][K][n], u int64[n], e int64[2][n]);
    u and e as the small integers behind their residue rows (every row the same one), |e| <= 19."""
    ct, u, e, r = enc.encrypt_return_components(_plaintext(m), disable_special_modulus=False)
    u_rows, e_rows = u.as_rns_u64s().reshape(L.K, L.n), e.as_rns_u64s().reshape(2, L.K, L.n)
    us = CL.small_from_rows(u_rows, L.primes)
    es = np.stack([CL.small_from_rows(e_rows[c], L.primes) for c in range(2)])
    assert int(np.abs(es).max()) <= CL.E_BOUND
    want_r = CL.scaling_remainder(L, m)
    assert [r.get_coefficient(i) for i in range(0, L.n, 97)] == [int(v) for v in want_r[::97]]
    return ct.to_array(), us, es


def _harvest(L, ctx, seed, ops):
    """{op: (u, e)} of the encryptions number `ops` under `seed`: what the component-returning call samples does not depend on the
    key or the plaintext, so any valid key serves (here: uniform residues)."""
    from sunscreen_amd import Encryptor, PublicKey

    any_key = PublicKey.from_array(ctx, LD.random_residues(L.rng(600), L.key_primes, (2,), L.n))
    enc = Encryptor(ctx, any_key, seed=seed)
    one = np.zeros(L.n, dtype=np.uint64)
    one[0] = 1
    out = {}
    for op in range(max(ops) + 1):
        _, u, e = _components(L, enc, one)
        assert (u == CL.recompute_u(seed, L.n, op)).all(), ("the device's u is not the documented ChaCha20 word", op)
        out[op] = (u, e)
    return out


# ---- A / B: landed encryptions ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("pid,t", ENC_CASES, ids=ENC_IDS)
def test_landed_encryptions_equal_the_integer_model_on_both_routes(pid, t):
    from sunscreen_amd import Encryptor, PublicKey
    from sunscreen_amd.batch import to_device, to_host

    L = client(pid, t)
    ctx, ev = _device(L)
    seed = CL.SEEDS[0]
    ops = [1] if L.n > 4096 else [0, 1]  # (the host side of one landing at n = 32768 takes seconds)
    sampled = _harvest(L, ctx, seed, ops)
    for op in ops:
        u, e = sampled[op]
        pk, m, T, x, divided, out = CL.landed_encryption(L, u, e, shift=op)  # (asserts: models agree, classes occur, words landed)
        pkd = PublicKey.from_array(ctx, pk)
        # the fused route, batched: the landed item alone at first_op = op
        got = to_host(ev.encrypt(to_device(m[None]), pkd, seed=seed, first_op=op))
        _same(got[0], out, (pid, "batched encrypt", op))
        # both handle routes: call number `op` of an encryptor with this seed
        for route in ("fused", "components"):
            enc = Encryptor(ctx, pkd, seed=seed)
            for _ in range(op):
                enc.encrypt(_plaintext([1]))
            if route == "fused":
                _same(enc.encrypt(_plaintext(m)).to_array(), out, (pid, "handle encrypt", op))
            else:
                ct, u2, e2 = _components(L, enc, m)
                assert (u2 == u).all() and (e2 == e).all()
                _same(ct, out, (pid, "handle encrypt_return_components", op))
        if op == 1 and L.n <= 4096:
            # a batch of two under the key crafted for item 1: item 1 is landed, item 0 is the model's under the same key
            u0, e0 = sampled[0]
            both = to_host(ev.encrypt(to_device(np.stack([m[::-1], m])), pkd, seed=seed, first_op=0))
            _same(both[1], out, (pid, "item 1 of a batch"))
            _same(both[0], CL.encrypt_model(L, pk, u0, e0, m[::-1].copy())[2], (pid, "item 0 of a batch"))


# ---- C: batch against handle, and the counter --------------------------------------------------------------------------------------
@pytest.mark.parametrize("pid", ["P1", "P6"])
def test_a_batch_equals_the_handle_calls_and_the_model(pid):
    """Five distinct plaintexts at first_op = 2 with a chunk boundary after every second item against handle calls 2 ... 6 of one
    encryptor; one shared plaintext (stride 0) against handle call 1; each against the model.  n = 32768 is the one degree that
    forms pk (.) NTT(u) in encrypt_dyadic_kernel and inverts with the plain transform."""
    from sunscreen_amd import Encryptor, PublicKey
    from sunscreen_amd.batch import to_device, to_host

    L = client(pid)
    ctx, ev = _device(L)
    seed = CL.SEEDS[1]
    sk, pk = CL.ordinary_keys(L)
    pkd = PublicKey.from_array(ctx, pk)
    rng = L.rng(601)
    ms = rng.integers(0, L.t, (5, L.n), dtype=np.uint64)
    ms[1] = CL.plain_cycle(L, 1)
    shared = CL.plain_cycle(L, 4)
    enc = Encryptor(ctx, pkd, seed=seed)
    calls = [np.zeros(L.n, dtype=np.uint64), shared] + list(ms)
    handle = [_components(L, enc, m) for m in calls]
    ev.set_chunk_ops(2)
    batch = to_host(ev.encrypt(to_device(ms), pkd, seed=seed, first_op=2))
    one = to_host(ev.encrypt(to_device(shared), pkd, seed=seed, first_op=1))
    assert one.shape == (1, 2, L.K, L.n)
    for k in range(5):
        _same(batch[k], handle[2 + k][0], (pid, "batch item", k, "against handle call", 2 + k))
    _same(one[0], handle[1][0], (pid, "the shared plaintext against handle call 1"))
    for op in range(1, 7):
        ct, u, e = handle[op]
        assert (u == CL.recompute_u(seed, L.n, op)).all(), op
        # (n = 32768: model (i) alone, six items of 16 key-level rows; the landed test above holds (ii) against it at this degree)
        x = CL.key_level_values(L, pk, u, e)
        want = CL.finish_rns(L, x, calls[op])[1]
        assert L.n > 16384 or (want == CL.finish_integers(L, x, calls[op])).all()
        _same(ct, want, (pid, "handle call against the model", op))
    assert (L.o.decrypt(batch[4], sk) == ms[4]).all()


def test_the_sampling_counter_carries_into_its_high_word():
    """A batch of three at first_op = 2^32 - 1 on the single-prime set (nothing is divided there: the equations hold exactly).  With
    u recomputed at (gop low word, gop high word), c1 - pk1 (*) u and c0 - pk0 (*) u - Delta m - r are the error polynomials: every
    coefficient within the sampler's clip.  A wrong counter word makes both uniform residues."""
    from sunscreen_amd import PublicKey
    from sunscreen_amd.batch import to_device, to_host

    L = client(CL.SINGLE)
    assert L.KK == 1
    ctx, ev = _device(L)
    seed = CL.SEEDS[1]
    sk, pk = CL.ordinary_keys(L)
    ms = L.rng(602).integers(0, L.t, (3, L.n), dtype=np.uint64)
    first = (1 << 32) - 1
    cts = to_host(ev.encrypt(to_device(ms), PublicKey.from_array(ctx, pk), seed=seed, first_op=first))
    zero = np.zeros((2, L.n), dtype=np.int64)
    errs = []
    for k in range(3):
        u = CL.recompute_u(seed, L.n, first + k)
        pku = CL.key_level_values(L, pk, u, zero)
        rest = LD.lin_mod(L.primes, [(1, cts[k]), (-1, pku)])
        rest[0] = LD.lin_mod(L.primes, [(1, rest[0]), (-1, CL.plain_term(L, ms[k]))])
        e = np.stack([CL.small_from_rows(rest[c], L.primes) for c in range(2)])
        assert int(np.abs(e).max()) <= CL.E_BOUND, (k, int(np.abs(e).max()))
        errs.append(e)
        assert (L.o.decrypt(cts[k], sk) == ms[k]).all()
    assert (errs[0] != errs[1]).any() and (errs[1] != errs[2]).any()
    # the same three counters reached one at a time
    for k in (1, 2):
        _same(to_host(ev.encrypt(to_device(ms[k : k + 1]), PublicKey.from_array(ctx, pk), seed=seed, first_op=first + k))[0], cts[k], k)


# ---- D: the CRT export ---------------------------------------------------------------------------------------------------------
def _check_array(pa, rows, value, what):
    """Every coefficient: the limbs are the Python CRT value in [0, q), to_rns gives the residues back, and the state flags are
    those of tests/test_gpu_client.py's round trip."""
    polys, K, n = rows.shape
    assert pa.is_reserved() and pa.is_rns()
    assert (pa.num_polynomials(), pa.poly_modulus_degree(), pa.coeff_modulus_size()) == (polys, n, K)
    _same(pa.as_u64s(), rows.ravel(), (what, "the array of a ciphertext is its data"))
    want = np.stack([CL.limbs_of(value[p], K) for p in range(polys)])
    mp = pa.as_multiprecision_u64s().reshape(polys, n, K)
    assert pa.is_rns()
    _same(pa.as_u64s(), rows.ravel(), (what, "unchanged by the multiprecision view"))
    _same(mp, want, (what, "compose"))
    pa.to_multiprecision()
    assert pa.is_multiprecision() and not pa.is_rns()
    _same(pa.as_u64s(), want.ravel(), (what, "to_multiprecision"))
    _same(pa.as_rns_u64s(), rows.ravel(), (what, "decompose through the RNS view"))
    assert pa.is_multiprecision()
    pa.to_rns()
    assert pa.is_rns()
    _same(pa.as_u64s(), rows.ravel(), (what, "to_rns"))


@pytest.mark.parametrize("pid", CL.CRT_SETS)
def test_crt_export_on_crafted_residues(pid):
    from sunscreen_amd import Ciphertext, PolynomialArray

    L = client(pid)
    ctx, _ = _device(L)
    rows, value, names, which = L.cached("crt", lambda: CL.crt_case(L.primes, L.n))  # (asserts: every case and subtraction count occurs)
    pa = PolynomialArray.new_from_ciphertext(ctx, Ciphertext.from_array(ctx, rows))
    _check_array(pa, rows, value, pid)


@pytest.mark.parametrize("pid", CL.CRT_LOWER_SETS)
def test_crt_export_at_the_level_below(pid):
    """The lower level's constants: cases crafted against q / q_{K-1}, reached by drop_modulus() of a crafted array and as the array
    of a mod_switch_to_next result (whose operand is crafted so that the switch itself lands on the cases)."""
    from sunscreen_amd import BFVEvaluator, Ciphertext, PolynomialArray

    L = client(pid)
    ctx, _ = _device(L)
    ct, rows, value = CL.lower_level_case(L)
    full = np.concatenate([rows, LD.random_residues(L.rng(603), L.primes[-1:], (2,), L.n)], axis=1)
    top = PolynomialArray.new_from_ciphertext(ctx, Ciphertext.from_array(ctx, full))
    low = top.drop_modulus()
    _check_array(low, rows, value, (pid, "drop_modulus"))
    assert top.is_rns() and top.coeff_modulus_size() == L.K
    _same(top.as_u64s(), full.ravel(), (pid, "the array dropped from"))
    assert (L.o.mod_switch_to_next(ct) == rows).all()
    lower = BFVEvaluator(ctx).mod_switch_to_next(Ciphertext.from_array(ctx, ct))
    _same(lower.to_array(), rows, (pid, "mod_switch_to_next lands on the cases"))
    _check_array(PolynomialArray.new_from_ciphertext(ctx, lower), rows, value, (pid, "mod_switch_to_next"))


# ---- E: the encoder's signed edges -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("pid", ["P1", "U1024"])
def test_signed_encoding_at_its_edges(pid):
    from sunscreen_amd import HipBfvError
    from sunscreen_amd.batch import to_device, to_host

    L = client(pid)
    ctx, ev = _device(L)
    n, t = L.n, L.t
    assert t % 2 == 1 and (pid != "U1024" or t.bit_length() == 20)
    half = t >> 1
    edge = np.array([half, -half, 0, 1, -1], dtype=np.int64)
    sv = np.stack([edge[np.arange(n) % 5], edge[(np.arange(n) + 2) % 5][::-1]])
    for v in edge:
        assert (sv[0] == v).any() and (sv[1] == v).any()
    enc = ev.encode(to_device(sv.view(np.uint64)), signed=True)
    _same(to_host(enc), np.stack([L.o.batch_encode((v % t).astype(np.uint64)) for v in sv]), (pid, "signed encode"))
    _same(to_host(ev.decode(enc, signed=True)).view(np.int64), sv, (pid, "signed decode"))
    # one step outside the range, and the one int64 without a negative: refused, alone in one item of the batch
    for bad in (-half - 1, half + 1, np.iinfo(np.int64).min):
        for item in range(2):
            w = sv.copy()
            w[item, 3] = bad
            with pytest.raises(HipBfvError) as ei:
                ev.encode(to_device(w.view(np.uint64)), signed=True)
            assert ei.value.kind == "InvalidArgument", (bad, item)
    # slot values floor(t / 2) and floor(t / 2) + 1: the last positive and the first negative representative
    slots = np.zeros((2, n), dtype=np.uint64)
    slots[0, 0::2], slots[0, 1::2] = half, half + 1
    slots[1, 0::2], slots[1, 1::2] = half + 1, half
    plain = np.stack([L.o.batch_encode(s) for s in slots])
    dec = to_host(ev.decode(to_device(plain), signed=True)).view(np.int64)
    assert (dec[0, 0::2] == half).all() and (dec[0, 1::2] == half + 1 - t).all()
    assert (dec[1, 0::2] == half + 1 - t).all() and (dec[1, 1::2] == half).all()
