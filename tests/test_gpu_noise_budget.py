"""The invariant-noise measure on device batches: hipbfv_batch_noise_budget and hipbfv_batch_decrypt_checked.

The reference's Runtime::decrypt asks for the invariant noise budget of every result before it decrypts it (Error::TooMuchNoise
at 0; sunscreen_runtime/src/runtime.rs:175-190) and measure_noise_budget takes the minimum over a value's ciphertexts
(runtime.rs:221-233).  Budgets are exact integers: every one is checked against the oracle's noise_budget (Python integers) and
the handle-level Decryptor_InvariantNoiseBudget; the f64 noise against Fraction(worst, Q).
"""
from fractions import Fraction

import numpy as np
import pytest

from oracle import bfv_oracle as O
from tests.bfv_helpers import params

pytestmark = pytest.mark.gpu

E_INVALIDARG = 0x80070057
NAMES = ["default_4096_16", "default_8192_17", "seal_fhe_unit", "default_16384_17", "default_32768_17", "bits_54_54_54_56"]


def _params(name):
    if name == "bits_54_54_54_56":  # the north-star literal: n = 8192, 3 x 54-bit data primes
        return 8192, O.coeff_modulus_create(8192, [54, 54, 54, 56]), O.plain_batching(8192, 17)
    return params(name)


def _setup(name, seed=31):
    from sunscreen_amd import Context, PublicKey, RelinearizationKeys, SecretKey
    from sunscreen_amd.batch import BatchEvaluator

    n, primes, t = _params(name)
    o = O.Oracle(n, primes, t)
    O.seed(seed)
    sk, pk, rk, _ = o.keygen()
    ctx = Context.from_raw(n, primes, t)
    return o, sk, ctx, BatchEvaluator(ctx), SecretKey.from_array(ctx, sk), PublicKey.from_array(ctx, pk), RelinearizationKeys.from_array(ctx, rk)


def _modulus(o):
    q = 1
    for p in o.primes[: o.K]:
        q *= p
    return q


def _worst(o, ct, sk):
    """max_x |[t * ct(s)(x)]_Q| centred, with Python integers (what the oracle's noise_budget measures)."""
    d = o.dot_with_secret(ct, sk)
    q = _modulus(o)
    v = [0] * o.n
    for i, p in enumerate(o.primes[: o.K]):
        qi = q // p
        f = pow(qi % p, -1, p) * o.t % p
        for k, r in enumerate(d[i].tolist()):
            v[k] += r * f % p * qi
    worst = 0
    for x in v:
        x %= q
        worst = max(worst, q - x if x > q // 2 else x)
    return worst


def _budget(q, worst):
    return max(0, q.bit_length() - worst.bit_length() - 1)


def _close(got, exact):
    """|got - exact| <= 2^-50 * exact"""
    return abs(Fraction(got) - exact) <= exact * Fraction(1, 1 << 50)


def _handle(ctx, skd, arr, level_ctx=None):
    """Decryptor_InvariantNoiseBudget / Decryptor_InvariantNoise of one ciphertext (of level_ctx: a lower level of ctx)"""
    from sunscreen_amd import Ciphertext, Decryptor

    d = Decryptor(ctx, skd)
    c = Ciphertext.from_array(level_ctx or ctx, arr)
    return d.invariant_noise_budget(c), d.invariant_noise(c)


def _items(o, ev, skd, pkd, rkd, rng):
    """size-2 items: fresh encryptions, relinearized products, repeated squares down to budget 0, random junk, all zero;
    size-3 items: unrelinearized products"""
    import torch
    from sunscreen_amd.batch import to_device

    n, t = o.n, o.t
    fresh = ev.encrypt(to_device(rng.integers(0, t, (3, n), dtype=np.uint64)), pkd, seed=int(rng.integers(1 << 62)))
    prod3 = ev.multiply(fresh[:2].contiguous(), fresh[1:].contiguous())
    relin = ev.multiply_relin(fresh[:2].contiguous(), fresh[1:].contiguous(), rkd)
    squares, x = [], fresh[:1].contiguous()
    for _ in range(64):  # every square costs bits: the chain reaches 0 well before 64 steps for every parameter set
        x = ev.multiply_relin(x, x, rkd)
        squares.append(x)
        if int(ev.noise_budget(x, skd)[0]) == 0:
            break
    junk = to_device(np.stack([np.stack([rng.integers(0, q, (2, n), dtype=np.uint64) for q in o.primes[: o.K]], axis=1) for _ in range(2)]))
    zero = torch.zeros((1, 2, o.K, n), dtype=torch.int64, device=fresh.device)
    ct2 = torch.cat([fresh, relin] + squares + [junk, zero]).contiguous()
    return ct2, prod3.contiguous(), len(squares)


@pytest.mark.parametrize("name", NAMES)
def test_batch_budgets_match_the_oracle_and_the_handle_level_call(name):
    import torch
    from sunscreen_amd.batch import to_host

    o, sk, ctx, ev, skd, pkd, rkd = _setup(name)
    q = _modulus(o)
    rng = np.random.default_rng(5)
    ct2, ct3, nsq = _items(o, ev, skd, pkd, rkd, rng)
    for ct in (ct2, ct3):
        budget, noise = ev.noise_budget(ct, skd, with_noise=True)
        torch.cuda.synchronize()
        budget, noise = budget.cpu().numpy(), noise.cpu().numpy()
        host = to_host(ct)
        for i in range(ct.shape[0]):
            worst = _worst(o, host[i], sk)
            assert int(budget[i]) == _budget(q, worst) == o.noise_budget(host[i], sk), (name, i)
            hb, hn = _handle(ctx, skd, host[i])
            assert hb == int(budget[i]), (name, i)
            exact = Fraction(worst, q)
            assert _close(float(noise[i]), exact) and _close(hn, exact), (name, i, float(noise[i]), hn, float(exact))
    b2 = ev.noise_budget(ct2, skd).cpu().numpy()
    assert b2[0] > 0 and b2[-1] == q.bit_length() - 1, (name, b2)  # fresh; all zero
    assert b2[-3] == 0 and b2[-2] == 0, name  # junk
    assert b2[3 + 2 + nsq - 1] == 0, (name, b2)  # the square chain ends exhausted
    # the checked decrypt reports the same budgets
    plain, chk = ev.decrypt_checked(ct2, skd)
    assert (chk.cpu().numpy() == b2).all()


@pytest.mark.parametrize("name", NAMES)
def test_boundary_norms_built_in_python(name):
    """c1 = 0 and c0 = T * t^-1 mod Q at one coefficient: t * phase mod Q = T there and 0 elsewhere.  Both sides of the centring
    threshold and norms 2^64k - 1, 2^64k (either sign) for every 2^64k < Q/2: the bit count crosses limb boundaries."""
    import torch
    from sunscreen_amd.batch import to_device

    o, sk, ctx, ev, skd, pkd, rkd = _setup(name)
    q = _modulus(o)
    tinv = pow(o.t, -1, q)
    targets = [(q - 1) // 2, (q + 1) // 2, (q + 3) // 2, 1, q - 1]
    k = 1
    while (1 << (64 * k)) < q // 2:
        targets += [(1 << (64 * k)) - 1, 1 << (64 * k), q - (1 << (64 * k)), q - (1 << (64 * k)) + 1]
        k += 1
    arr = np.zeros((len(targets), 2, o.K, o.n), dtype=np.uint64)
    for j, tv in enumerate(targets):
        c0 = tv * tinv % q
        for i, p in enumerate(o.primes[: o.K]):
            arr[j, 0, i, (j * 37) % o.n] = c0 % p
    budget, noise = ev.noise_budget(to_device(arr), skd, with_noise=True)
    torch.cuda.synchronize()
    budget, noise = budget.cpu().numpy(), noise.cpu().numpy()
    for j, tv in enumerate(targets):
        norm = q - tv if tv >= (q + 1) // 2 else tv
        assert int(budget[j]) == _budget(q, norm), (name, j, hex(tv))
        assert _close(float(noise[j]), Fraction(norm, q)), (name, j)
        hb, hn = _handle(ctx, skd, arr[j])
        assert hb == int(budget[j]) and _close(hn, Fraction(norm, q)), (name, j)
    assert int(budget[0]) == int(budget[1]) == _budget(q, (q - 1) // 2)


@pytest.mark.parametrize("name", ["default_8192_17", "default_16384_17", "bits_54_54_54_56"])
def test_decrypt_checked_gives_decrypts_bits_and_noise_budgets(name):
    import torch
    from sunscreen_amd.batch import to_host

    o, sk, ctx, ev, skd, pkd, rkd = _setup(name)
    rng = np.random.default_rng(9)
    ct2, ct3, _ = _items(o, ev, skd, pkd, rkd, rng)
    for ct in (ct2, ct3):
        plain, budget = ev.decrypt_checked(ct, skd)
        ref_plain, ref_budget = ev.decrypt(ct, skd), ev.noise_budget(ct, skd)
        torch.cuda.synchronize()
        assert (to_host(plain) == to_host(ref_plain)).all(), name
        assert (budget.cpu().numpy() == ref_budget.cpu().numpy()).all(), name
        host, got = to_host(ct), to_host(plain)
        for i in (0, ct.shape[0] - 1):
            assert (got[i] == o.decrypt(host[i], sk)).all(), (name, i)


@pytest.mark.parametrize("name", ["default_4096_16", "default_16384_17"])
def test_chunking_does_not_change_the_results(name):
    """one item, and a batch over more than three chunks (hipbfv_set_chunk_ops): the same budgets, noise and plaintexts"""
    import torch
    from sunscreen_amd.batch import BatchEvaluator, to_host

    o, sk, ctx, ev, skd, pkd, rkd = _setup(name)
    ct2, _, _ = _items(o, ev, skd, pkd, rkd, np.random.default_rng(11))
    b_ref, n_ref = ev.noise_budget(ct2, skd, with_noise=True)
    p_ref, c_ref = ev.decrypt_checked(ct2, skd)
    small = BatchEvaluator(ctx)
    small.set_chunk_ops(2)
    assert ct2.shape[0] > 6
    b, nz = small.noise_budget(ct2, skd, with_noise=True)
    p, c = small.decrypt_checked(ct2, skd)
    singles = [small.noise_budget(ct2[i : i + 1].contiguous(), skd, with_noise=True) for i in range(ct2.shape[0])]
    torch.cuda.synchronize()
    assert (b.cpu() == b_ref.cpu()).all() and (nz.cpu() == n_ref.cpu()).all()
    assert (to_host(p) == to_host(p_ref)).all() and (c.cpu() == c_ref.cpu()).all() and (c.cpu() == b_ref.cpu()).all()
    for i, (bi, ni) in enumerate(singles):
        assert int(bi[0]) == int(b_ref[i]) and float(ni[0]) == float(n_ref[i]), (name, i)


@pytest.mark.parametrize("name", ["default_8192_17", "default_32768_17"])
def test_a_lower_level_after_a_batched_mod_switch(name):
    import torch
    from sunscreen_amd import SecretKey
    from sunscreen_amd.batch import BatchEvaluator, to_host

    o, sk, ctx, ev, skd, pkd, rkd = _setup(name)
    ct2, _, _ = _items(o, ev, skd, pkd, rkd, np.random.default_rng(13))
    sub = ct2[[0, 1, 3, ct2.shape[0] - 1]].contiguous()
    sw = ev.mod_switch(sub)
    ctx1 = ctx.next_level()
    o1 = o.next_level()
    sk1 = np.ascontiguousarray(np.concatenate([sk[: o1.K], sk[o.K :]]))
    sk1d = SecretKey.from_array(ctx1, sk1)
    ev1 = BatchEvaluator(ctx1)
    budget, noise = ev1.noise_budget(sw, sk1d, with_noise=True)
    plain, chk = ev1.decrypt_checked(sw, sk1d)
    torch.cuda.synchronize()
    q1 = _modulus(o1)
    host, got = to_host(sw), to_host(plain)
    for i in range(sw.shape[0]):
        worst = _worst(o1, host[i], sk1)
        assert int(budget[i]) == _budget(q1, worst) == o1.noise_budget(host[i], sk1) == int(chk[i]), (name, i)
        assert _close(float(noise[i]), Fraction(worst, q1)), (name, i)
        hb, hn = _handle(ctx, skd, host[i], ctx1)  # the handle-level decryptor of the top context, at the lower level
        assert hb == int(budget[i]) and _close(hn, Fraction(worst, q1)), (name, i)
        assert (got[i] == o1.decrypt(host[i], sk1)).all(), (name, i)


def test_every_overlap_is_refused_and_the_storage_is_left_untouched():
    """No output may overlap ct or another output (include/hipbfv.h, "Aliasing"): E_INVALIDARG before any launch."""
    import ctypes as C

    import torch
    from sunscreen_amd import _lib
    from sunscreen_amd.batch import _stream

    o, sk, ctx, ev, skd, pkd, rkd = _setup("default_4096_16")
    L = _lib.load()
    count, n, K = 4, o.n, o.K
    ctw = count * 2 * K * n
    rng = np.random.default_rng(17)
    words = rng.integers(-(1 << 62), 1 << 62, ctw + 2 * count * n + 64, dtype=np.int64)
    junk = np.stack([rng.integers(0, q, (count, 2, n), dtype=np.uint64) for q in o.primes[:K]], axis=2)  # valid residues for ct
    words[:ctw] = junk.reshape(-1).view(np.int64)
    store = torch.from_numpy(words).cuda()
    before = store.clone()
    base = store.data_ptr()
    ct, after = base, base + ctw * 8  # after: the first byte behind the ciphertexts

    def nb(budget, noise):
        return L.hipbfv_batch_noise_budget(ev._h, C.c_void_p(ct), 2, skd.get_handle(), C.c_void_p(budget), C.c_void_p(noise) if noise else None,
                                           count, _stream())

    def dc(plain, budget):
        return L.hipbfv_batch_decrypt_checked(ev._h, C.c_void_p(ct), 2, skd.get_handle(), C.c_void_p(plain), C.c_void_p(budget), count, _stream())

    refused = [
        nb(ct, None), nb(ct + ctw * 8 - 4, None), nb(after, ct + 8), nb(after, ct + ctw * 8 - 8),  # an output inside / straddling ct
        nb(after, after), nb(after, after + 8), nb(after + 8, after),  # budget and noise overlap each other
        dc(ct + 64, after), dc(after, ct + 16), dc(after - 8, after + count * n * 8),  # plain / budget overlap ct
        dc(after, after), dc(after, after + count * n * 8 - 4), dc(after + 4, after),  # budget and plain overlap each other
    ]
    torch.cuda.synchronize()
    assert all(hr & 0xFFFFFFFF == E_INVALIDARG for hr in refused), [hex(h & 0xFFFFFFFF) for h in refused]
    assert torch.equal(store, before)
    # adjacent ranges are not overlaps: budget right behind ct, noise right behind budget, plain right behind budget
    assert nb(after, after + count * 4) == 0
    assert dc(after + count * 4, after) == 0
    torch.cuda.synchronize()
    assert torch.equal(store[: ctw], before[: ctw])
    # count == 0 launches nothing and succeeds; a null required pointer is E_POINTER
    assert L.hipbfv_batch_noise_budget(ev._h, C.c_void_p(ct), 2, skd.get_handle(), C.c_void_p(after), None, 0, _stream()) == 0
    assert L.hipbfv_batch_noise_budget(ev._h, C.c_void_p(ct), 1, skd.get_handle(), C.c_void_p(after), None, count, _stream()) & 0xFFFFFFFF == E_INVALIDARG
