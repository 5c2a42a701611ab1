"""Every plain-modulus-dependent path on the device at the plain moduli the reference's programs use.

Sunscreen compiles with PlainModulusConstraint::Raw (PlainModulus::raw): t = 262144 by default, 64, 500 and 1024 in its tests.
The library accepts any t in [2, 2^60) coprime to q, and the t-dependent code has branches of its own: the Barrett constant of
a power of two (decrypt), the (t+1)/2 rounding of add/sub_plain, the centred lift and the monomial rule of multiply_plain (off
once t reaches a data prime), the auxiliary base sized by bits(t) (SEAL's 61-bit base as the fallback), the encoder's NTT over Z_t
on the FP64 or the integer policy.  Everything here is compared word for word with the oracle; add_plain / sub_plain also with
the integer formula, and a short chain at the reference's moduli with the same arithmetic over Python integers in Z_t[X]/(X^n+1).
"""
import functools
from fractions import Fraction

import numpy as np
import pytest

from oracle import bfv_oracle as O
from tests.test_gpu_noise_budget import _budget, _close, _modulus, _worst
from tests.test_oracle_behz_exact import _negacyclic, _prod

pytestmark = pytest.mark.gpu

T59, T60M1 = 1 << 59, (1 << 60) - 1
# (id, n, data prime bits or None for SEAL's default set, t)
CASES = [(f"n2048_default_t{t}", 2048, None, t) for t in (64, 500)]
CASES += [("n2048_default_tbatch40", 2048, None, O.plain_batching(2048, 40))]  # 32 + bits(t) + bits(q) >= 122: SEAL's extra aux prime
CASES += [(f"n4096_default_t{t}", 4096, None, t) for t in (2, 3, 64, 500, 1024, 262144, T59, T60M1)]
CASES += [(f"n8192_default_t{t}", 8192, None, t) for t in (500, T59)]
CASES += [(f"n8192_default_tbatch{b}", 8192, None, O.plain_batching(8192, b)) for b in (55, 60)]  # integer-policy encoder, fallback base
CASES += [(f"n8192_3x54_t{t}", 8192, [54, 54, 54, 56], t) for t in (500, T59)]
CASES += [("n16384_default_t64", 16384, None, 64), ("n16384_default_tbatch60", 16384, None, O.plain_batching(16384, 60))]
CASES += [("n1024_2x30_t2^40+15", 1024, [30, 30, 31], (1 << 40) + 15)]  # t above every data prime: fast_plain_lift off
CASES += [("n32768_default_t500", 32768, None, 500)]
IDS = [c[0] for c in CASES]


def _case(name):
    _, n, bits, t = next(c for c in CASES if c[0] == name)
    return _setup(n, None if bits is None else tuple(bits), t)


@functools.lru_cache(maxsize=None)
def _setup(n, bits, t):
    """oracle, context, evaluator and keys (oracle-made, loaded into the library) of one parameter set, built once per module"""
    from sunscreen_amd import Context, GaloisKeys, PublicKey, RelinearizationKeys, SecretKey
    from sunscreen_amd.batch import BatchEvaluator

    primes = O.bfv_default(n) if bits is None else O.coeff_modulus_create(n, list(bits))
    o = O.Oracle(n, primes, t)
    o.throw_on_transparent = False
    batching = O.is_prime(t) and (t - 1) % (2 * n) == 0
    elts = [o.galois_elt_from_step(1), 2 * n - 1] if batching and len(primes) > 1 else []
    O.seed(n ^ (t & 0xFFFF))
    sk, pk, rk, gk = o.keygen(relin=len(primes) > 1, galois_elts=elts)
    ctx = Context.from_raw(n, primes, t)
    ev = BatchEvaluator(ctx)
    ev.set_transparent_check(False)
    keys = dict(sk=sk, pk=pk, rk=rk, gk=gk, skd=SecretKey.from_array(ctx, sk), pkd=PublicKey.from_array(ctx, pk),
                rkd=RelinearizationKeys.from_array(ctx, rk) if rk is not None else None,
                gkd=GaloisKeys.from_arrays(ctx, gk) if gk else None)
    return o, ctx, ev, keys, batching


def _q(o):
    return [int(p) for p in o.primes[: o.K]]


def _random_cts(o, rng, count, size=2):
    return np.stack([np.stack([rng.integers(0, p, (size, o.n), dtype=np.uint64) for p in _q(o)], axis=1) for _ in range(count)])


def _extreme_cts(o, size=2):
    """every residue q_i - 1 (the integer -1), and floor(Q/2) spread over the residues"""
    q = _q(o)
    Q = _prod(q)
    top = np.stack([np.full((size, o.n), p - 1, dtype=np.uint64) for p in q], axis=1)
    mid = np.stack([np.full((size, o.n), (Q // 2) % p, dtype=np.uint64) for p in q], axis=1)
    return np.stack([top, mid])


def _plaintexts(o, rng):
    """the special values, an all-upper-half plaintext, monomials with a lower-half and with upper-half coefficients"""
    n, t = o.n, o.t
    half_up = (t + 1) >> 1
    out = []
    special = rng.integers(0, t, n, dtype=np.uint64)
    special[:5] = [0, 1, t - 1, (t - 1) // 2, half_up]
    out.append(special)
    out.append(rng.integers(half_up, t, n, dtype=np.uint64) if half_up < t else np.full(n, t - 1, dtype=np.uint64))
    for e, coeff in ((5, (t - 1) // 2), (n - 1, half_up), (0, t - 1), (17, 1)):
        if 0 < coeff < t:
            mono = np.zeros(n, dtype=np.uint64)
            mono[e] = coeff
            out.append(mono)
    return np.stack(out)


def _scaled(o, m):
    """round(Q * m / t) as SEAL adds it: floor(Q/t) * m + floor((m * (Q mod t) + floor((t+1)/2)) / t)"""
    Q, t = _prod(_q(o)), o.t
    return (Q // t) * m + (m * (Q % t) + ((t + 1) >> 1)) // t


@pytest.mark.parametrize("name", IDS)
def test_plain_ops_match_the_oracle_and_the_integer_rounding(name):
    from sunscreen_amd.batch import to_device, to_host

    o, ctx, ev, keys, _ = _case(name)
    rng = np.random.default_rng(101)
    plains = _plaintexts(o, rng)
    P = plains.shape[0]
    cts = np.concatenate([_extreme_cts(o), _random_cts(o, rng, P - 2)]) if P >= 2 else _random_cts(o, rng, P)
    dct, dpl = to_device(cts), to_device(plains)
    got = {op: to_host(getattr(ev, op)(dct, dpl)) for op in ("add_plain", "sub_plain", "multiply_plain")}
    for i in range(P):
        for op in got:
            assert (got[op][i] == getattr(o, op)(cts[i], plains[i])).all(), (name, op, i)
    # the integer meaning of add / sub_plain, for the plaintext that holds the special values
    q = _q(o)
    y = [_scaled(o, int(m)) for m in plains[0]]
    for j, p in enumerate(q):
        col = cts[0, 0, j].tolist()
        assert got["add_plain"][0, 0, j].tolist() == [(c + v) % p for c, v in zip(col, y)], (name, j)
        assert got["sub_plain"][0, 0, j].tolist() == [(c - v) % p for c, v in zip(col, y)], (name, j)
        assert (got["add_plain"][0, 1, j] == cts[0, 1, j]).all()
    # one plaintext shared by every ciphertext (stride 0): the dense special one, then a monomial
    for k in (0, P - 1):
        for op in ("add_plain", "sub_plain", "multiply_plain"):
            shared = to_host(getattr(ev, op)(dct, to_device(plains[k])))
            for i in range(P):
                assert (shared[i] == getattr(o, op)(cts[i], plains[k])).all(), (name, op, "shared", k, i)
    ev.check()


@pytest.mark.parametrize("name", IDS)
def test_evaluator_ops_match_the_oracle(name):
    from sunscreen_amd import SecretKey
    from sunscreen_amd.batch import BatchEvaluator, to_device, to_host

    o, ctx, ev, keys, batching = _case(name)
    rng = np.random.default_rng(202)
    a = np.concatenate([_random_cts(o, rng, 1), _extreme_cts(o)])
    b = np.concatenate([_random_cts(o, rng, 1), _extreme_cts(o)[::-1]])
    da, db = to_device(a), to_device(b)
    m = to_host(ev.multiply(da, db))
    for i in range(a.shape[0]):
        assert (m[i] == o.multiply(a[i], b[i])).all(), (name, "multiply", i)
    if keys["rk"] is not None:
        mr = to_host(ev.multiply_relin(da, db, keys["rkd"]))
        c3 = np.concatenate([_random_cts(o, rng, 1, 3), _extreme_cts(o, 3)])
        r = to_host(ev.relinearize(to_device(c3), keys["rkd"]))
        for i in range(a.shape[0]):
            assert (mr[i] == o.relinearize(o.multiply(a[i], b[i]), keys["rk"])).all(), (name, "multiply_relin", i)
            assert (r[i] == o.relinearize(c3[i], keys["rk"])).all(), (name, "relinearize", i)
    if keys["gkd"] is not None:
        rr = to_host(ev.rotate_rows(da, 1, keys["gkd"]))
        rc = to_host(ev.rotate_columns(da, keys["gkd"]))
        for i in range(a.shape[0]):
            assert (rr[i] == o.rotate_rows(a[i], 1, keys["gk"])).all(), (name, "rotate_rows", i)
            assert (rc[i] == o.rotate_columns(a[i], keys["gk"])).all(), (name, "rotate_columns", i)
    if o.K >= 2:
        sw = ev.mod_switch(da)
        o1 = o.next_level()
        sk = keys["sk"]
        sk1 = np.ascontiguousarray(np.concatenate([sk[: o1.K], sk[o.K :]]))
        ev1 = BatchEvaluator(ctx.next_level())
        swh = to_host(sw)
        dec = to_host(ev1.decrypt(sw, SecretKey.from_array(ctx.next_level(), sk1)))
        for i in range(a.shape[0]):
            assert (swh[i] == o.mod_switch_to_next(a[i])).all(), (name, "mod_switch", i)
            assert (dec[i] == o1.decrypt(swh[i], sk1)).all(), (name, "mod_switch + decrypt", i)
    ev.check()


@pytest.mark.parametrize("name", IDS)
def test_decrypt_and_noise_budget_match_the_oracle_and_the_exact_norm(name):
    import torch
    from sunscreen_amd.batch import to_device, to_host

    o, ctx, ev, keys, _ = _case(name)
    sk, pk = keys["sk"], keys["pk"]
    rng = np.random.default_rng(303)
    msgs = np.concatenate([_plaintexts(o, rng)[:2], rng.integers(0, o.t, (1, o.n), dtype=np.uint64)])
    fresh = np.stack([o.encrypt(pk, m) for m in msgs])
    q = _modulus(o)
    batches = [np.concatenate([fresh, _random_cts(o, rng, 1), _extreme_cts(o)])]
    batches.append(np.concatenate([np.stack([o.multiply(fresh[0], fresh[2]), o.multiply(fresh[1], fresh[1])]), _extreme_cts(o, 3)]))
    for cts in batches:
        d = to_device(cts)
        plain = to_host(ev.decrypt(d, keys["skd"]))
        budget, noise = ev.noise_budget(d, keys["skd"], with_noise=True)
        plain2, chk = ev.decrypt_checked(d, keys["skd"])
        torch.cuda.synchronize()
        budget, noise, chk, plain2 = budget.cpu().numpy(), noise.cpu().numpy(), chk.cpu().numpy(), to_host(plain2)
        for i in range(cts.shape[0]):
            want = o.decrypt(cts[i], sk)
            assert (plain[i] == want).all() and (plain2[i] == want).all(), (name, cts.shape[1], i)
            worst = _worst(o, cts[i], sk)
            assert int(budget[i]) == int(chk[i]) == _budget(q, worst) == o.noise_budget(cts[i], sk), (name, cts.shape[1], i)
            assert _close(float(noise[i]), Fraction(worst, q)), (name, cts.shape[1], i)
    for i in range(msgs.shape[0]):  # fresh encryptions with budget decrypt to the message
        if o.noise_budget(fresh[i], sk) > 0:
            assert (to_host(ev.decrypt(to_device(fresh[i : i + 1]), keys["skd"]))[0] == msgs[i]).all(), (name, i)


@pytest.mark.parametrize("name", IDS)
def test_encrypt_decrypts_under_the_oracle_with_a_fresh_budget(name):
    from sunscreen_amd.batch import to_device, to_host

    o, ctx, ev, keys, _ = _case(name)
    sk, pk = keys["sk"], keys["pk"]
    rng = np.random.default_rng(404)
    msgs = _plaintexts(o, rng)
    cts = to_host(ev.encrypt(to_device(msgs), keys["pkd"], seed=77))
    ref = o.noise_budget(o.encrypt(pk, msgs[0]), sk)
    for i in range(msgs.shape[0]):
        b = o.noise_budget(cts[i], sk)
        assert abs(b - ref) <= 2, (name, i, b, ref)
        if ref > 2:
            assert (o.decrypt(cts[i], sk) == msgs[i]).all(), (name, i)
        for k, p in enumerate(_q(o)):
            assert int(cts[i][:, k].max()) < p


BATCHING_IDS = [c[0] for c in CASES if O.is_prime(c[3]) and (c[3] - 1) % (2 * c[1]) == 0]


@pytest.mark.parametrize("name", BATCHING_IDS)
def test_batch_encoder_is_bit_exact_and_flags_values_out_of_range(name):
    from sunscreen_amd import HipBfvError
    from sunscreen_amd.batch import to_device, to_host

    o, ctx, ev, keys, batching = _case(name)
    assert batching
    n, t = o.n, o.t
    half = t >> 1
    rng = np.random.default_rng(505)
    vals = rng.integers(0, t, (3, n), dtype=np.uint64)
    vals[0, :6] = [0, 1, t - 1, half, half + 1, half - 1]
    vals[1] = np.arange(n, dtype=np.uint64) * (t // n)
    enc = to_host(ev.encode(to_device(vals)))
    for i in range(3):
        assert (enc[i] == o.batch_encode(vals[i])).all(), (name, i)
    assert (to_host(ev.decode(to_device(enc))) == vals).all()
    junk = rng.integers(0, t, (2, n), dtype=np.uint64)
    dj = to_host(ev.decode(to_device(junk)))
    for i in range(2):
        assert (dj[i] == o.batch_decode(junk[i])).all(), (name, i)
    sv = rng.integers(-half, half + 1, (2, n)).astype(np.int64)
    sv[0, :4] = [half, -half, 0, -1]
    senc = ev.encode(to_device(sv.view(np.uint64)), signed=True)
    for i in range(2):
        want = o.batch_encode(np.array([int(v) % t for v in sv[i]], dtype=np.uint64))
        assert (to_host(senc)[i] == want).all(), (name, i)
    assert (to_host(ev.decode(senc, signed=True)).view(np.int64) == sv).all()
    # one beyond the range: t unsigned, +-(t >> 1) + 1 signed
    for bad, signed in ((t, False), (half + 1, True), (-(half + 1), True)):
        v = np.zeros((1, n), dtype=np.int64)
        v[0, 3] = bad
        with pytest.raises(HipBfvError):
            ev.encode(to_device(v.view(np.uint64)), signed=signed)
            ev.check()


@pytest.mark.parametrize("name", ["n4096_default_t64", "n4096_default_t500"])
def test_plain_to_ntt_and_dot_plain_ntt_equal_multiply_plain_and_add(name):
    from sunscreen_amd.batch import to_device, to_host

    o, ctx, ev, keys, _ = _case(name)
    rng = np.random.default_rng(606)
    rows, cols = 2, 3
    plains = np.stack([_plaintexts(o, rng)[[0, 1, 3]], rng.integers(0, o.t, (cols, o.n), dtype=np.uint64)])
    cts = _random_cts(o, rng, cols)
    cts[0] = _extreme_cts(o)[0]
    pntt = ev.plain_to_ntt(to_device(plains))
    out = to_host(ev.dot_plain_ntt(ev.ct_to_ntt(to_device(cts)), pntt))
    for r in range(rows):
        want = o.multiply_plain(cts[0], plains[r, 0])
        for c in range(1, cols):
            want = o.add(want, o.multiply_plain(cts[c], plains[r, c]))
        assert (out[r] == want).all(), (name, r)
    ev.check()


def _ring_mul(a, b, t):
    """a * b in Z_t[X]/(X^n + 1), Python integers"""
    bits = 2 * t.bit_length() + len(a).bit_length() + 4
    return [v % t for v in _negacyclic([int(x) for x in a], [int(x) for x in b], bits)]


@pytest.mark.parametrize("n", [4096, 8192])
@pytest.mark.parametrize("t", [64, 500, 1024, 262144])
def test_chain_at_the_reference_moduli_means_the_same_in_z_t(n, t):
    """encrypt -> multiply_relin -> add_plain -> multiply_plain -> decrypt, batched and through the SEAL-named handles, equals
    the same arithmetic over Python integers wherever the oracle leaves the result a positive noise budget."""
    import torch
    from sunscreen_amd import BFVEvaluator, Ciphertext, Decryptor, Encryptor, Plaintext
    from sunscreen_amd.batch import to_device, to_host

    o, ctx, ev, keys, _ = _setup(n, None, t)
    rng = np.random.default_rng(n + t)
    a, b, c = (rng.integers(0, t, n, dtype=np.uint64) for _ in range(3))
    d = np.zeros(n, dtype=np.uint64)
    d[0], d[9], d[n - 1] = 2, t - 1, (t + 1) >> 1  # few, small and upper-half coefficients: cheap in noise
    want = _ring_mul([(x + int(y)) % t for x, y in zip(_ring_mul(a, b, t), c)], d, t)
    # batched
    enc = ev.encrypt(to_device(np.stack([a, b])), keys["pkd"], seed=n + t)
    r = ev.multiply_relin(enc[:1].contiguous(), enc[1:].contiguous(), keys["rkd"])
    r = ev.multiply_plain(ev.add_plain(r, to_device(c)), to_device(d))
    got = to_host(ev.decrypt(r, keys["skd"]))[0]
    torch.cuda.synchronize()
    rh = to_host(r)[0]
    encs = to_host(enc)
    ref = o.multiply_plain(o.add_plain(o.relinearize(o.multiply(encs[0], encs[1]), keys["rk"]), c), d)
    assert (rh == ref).all()
    budget = o.noise_budget(rh, keys["sk"])
    if n >= 8192:
        assert budget > 0, (n, t)
    if budget > 0:
        assert got.tolist() == want, (n, t)
    # handle level: Encryptor / BFVEvaluator / Decryptor as run.rs issues them
    he, hd, be = Encryptor(ctx, keys["pkd"], seed=n ^ t), Decryptor(ctx, keys["skd"]), BFVEvaluator(ctx)
    pa, pb = Plaintext.from_coefficients([int(x) for x in a]), Plaintext.from_coefficients([int(x) for x in b])
    ca, cb = he.encrypt(pa), he.encrypt(pb)
    hr = be.relinearize(be.multiply(ca, cb), keys["rkd"])
    hr = be.multiply_plain(be.add_plain(hr, Plaintext.from_coefficients([int(x) for x in c])), Plaintext.from_coefficients([int(x) for x in d]))
    hb = hd.invariant_noise_budget(hr)
    assert hb == o.noise_budget(hr.to_array(), keys["sk"])
    if hb > 0:
        out = hd.decrypt(hr)
        coeffs = [out.get_coefficient(k) for k in range(out.len())]
        assert coeffs + [0] * (n - len(coeffs)) == want, (n, t)
    if n >= 8192:
        assert hb > 0, (n, t)


def test_fhe_program_with_plaintext_literal_and_multiply_plaintext_at_t500():
    """A program as Sunscreen compiles it with Raw(500): Literal::Plaintext nodes consumed by MultiplyPlaintext and AddPlaintext,
    against the reference's node walk on the oracle, and what it decrypts to against Z_t[X]/(X^n+1) over Python integers."""
    from sunscreen_amd import Plaintext
    from sunscreen_amd.batch import to_device, to_host
    from sunscreen_amd.program import FheProgram, encode_plaintext_literal
    from tests.oracle_program import run_program

    n, t = 4096, 500
    o, ctx, ev, keys, _ = _setup(n, None, t)
    rng = np.random.default_rng(707)
    lit_coeffs = np.zeros(n, dtype=np.uint64)
    lit_coeffs[:4] = [3, t - 1, (t + 1) >> 1, (t - 1) >> 1]  # 3 - X + ... : upper-half coefficients take the centred lift
    blob = encode_plaintext_literal(n, O.bfv_default(n), t, Plaintext.from_coefficients([int(c) for c in lit_coeffs]).as_bytes())
    p = FheProgram()
    a = p.append_input_ciphertext(0)
    b = p.append_input_ciphertext(1)
    lit = p.append_plaintext_literal(blob)
    p.append_output_ciphertext(p.append_add(a, p.append_add_plaintext(p.append_multiply_plaintext(b, lit), lit)))
    batch = 2
    va, vb = rng.integers(0, t, (batch, n), dtype=np.uint64), rng.integers(0, t, (batch, n), dtype=np.uint64)
    ca = np.stack([o.encrypt(keys["pk"], v) for v in va])
    cb = np.stack([o.encrypt(keys["pk"], v) for v in vb])
    (out,) = p.run(ev, [to_device(ca), to_device(cb)], keys["rkd"])
    out = to_host(out)
    for i in range(batch):
        (ref,) = run_program(o, p.nodes, p.edges, [ca[i], cb[i]], keys["rk"], literals={lit: lit_coeffs})
        assert (out[i] == ref).all(), i
        assert o.noise_budget(out[i], keys["sk"]) > 0
        want = [(int(x) + y + int(z)) % t for x, y, z in zip(va[i], _ring_mul(vb[i], lit_coeffs, t), lit_coeffs)]
        assert o.decrypt(out[i], keys["sk"]).tolist() == want, i


@pytest.mark.parametrize("t", [0, 1, 1 << 60, (1 << 64) - 1])
def test_plain_moduli_outside_the_range_are_refused(t):
    """include/hipbfv.h, hipbfv_Context_Create: t in [2, 2^60).  The oracle model does not check t; SEAL refuses these too."""
    from sunscreen_amd import Context, HipBfvError

    with pytest.raises(HipBfvError) as ei:
        Context.from_raw(4096, O.bfv_default(4096), t)
    assert ei.value.kind == "InvalidArgument"


def test_a_plain_modulus_sharing_a_factor_with_q_is_refused():
    from sunscreen_amd import Context, HipBfvError

    primes = O.bfv_default(4096)
    for t in (primes[0], 2 * primes[1]):
        with pytest.raises(HipBfvError) as ei:
            Context.from_raw(4096, primes, t)
        assert ei.value.kind == "InvalidArgument"
