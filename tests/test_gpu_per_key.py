"""Per-key batches on the GPU (SURVEY 8d config 3 "per-ciphertext-key worst case").

The reference passes the keys with every call (sunscreen_runtime/src/run.rs:100-105: `relin_keys`, `galois_keys`;
runtime.rs:310-327), so a server that batches the calls of many clients holds one key set per client.  Every test
calls libhipbfv.so through the C ABI (hipbfv_batch_*_keys, hipbfv_Program_RunKeys) with SEVERAL key sets in one call
and checks every item bit for bit against the CPU oracle run with that item's own keys.
"""
import os

import numpy as np
import pytest

from oracle import bfv_oracle as O
from tests.bfv_helpers import oracle_for, params
from tests.oracle_program import run_program

pytestmark = pytest.mark.gpu


def _tenants(name, ntenants, galois=None, seed=100, relin=True):
    """`ntenants` independent key sets (secret, public, relinearisation, Galois) of one parameter set."""
    from sunscreen_amd import Context, GaloisKeys, RelinearizationKeys
    from sunscreen_amd.batch import BatchEvaluator

    n, primes, t = params(name) if isinstance(name, str) else name
    o = oracle_for(name) if isinstance(name, str) else O.Oracle(n, primes, t)
    ctx = Context.from_raw(n, primes, t)
    ev = BatchEvaluator(ctx)
    ten = []
    for k in range(ntenants):
        O.seed(seed + k)
        sk, pk, rk, gk = o.keygen(galois_elts=galois)
        ten.append(
            {
                "sk": sk,
                "pk": pk,
                "rk": rk,
                "gk": gk,
                "rkd": RelinearizationKeys.from_array(ctx, rk) if relin and rk is not None else None,
                "gkd": GaloisKeys.from_arrays(ctx, gk) if gk else None,
            }
        )
    return o, ctx, ev, ten


def _enc(o, ten, key_index, rng, hi=50):
    vals = rng.integers(0, hi, (len(key_index), o.n)).astype(np.uint64)
    try:
        cts = np.stack([o.encrypt(ten[k]["pk"], o.batch_encode(v % o.t)) for v, k in zip(vals, key_index)])
    except ValueError:  # parameters without batching
        cts = np.stack([o.encrypt(ten[k]["pk"], v % o.t) for v, k in zip(vals, key_index)])
    return vals, cts


@pytest.mark.parametrize(
    "name,ntenants,count,chunk",
    [
        ("default_4096_16", 9, 26, 0),  # 9 key sets (one of them unused), scrambled items, one launch
        ("default_4096_16", 8, 21, 5),  # chunks of 5: every chunk sorts its own items
        ("default_8192_17", 8, 10, 0),  # the headline degree (fused five-kernel pipeline at count > 8)
        ("default_16384_17", 3, 5, 0),  # K = 8
    ],
)
def test_multiply_relinearize_with_one_key_set_per_client(name, ntenants, count, chunk):
    """>= 8 distinct relinearisation keys in ONE call; unsorted key indices; every item equals the oracle run with its key."""
    from sunscreen_amd.batch import to_device, to_host

    o, ctx, ev, ten = _tenants(name, ntenants)
    rng = np.random.default_rng(ntenants * 1000 + count)
    used = ntenants - 1 if ntenants == 9 else ntenants
    key_index = rng.integers(0, used, count).astype(np.uint32)
    key_index[:used] = rng.permutation(used)  # every used key set appears
    if chunk:
        ev.set_chunk_ops(chunk)
    va, a = _enc(o, ten, key_index, rng)
    vb, b = _enc(o, ten, key_index, rng)
    sets = [x["rkd"] for x in ten]
    da, db = to_device(a), to_device(b)
    fused = to_host(ev.multiply_relin_keys(da, db, sets, key_index))
    prod = ev.multiply(da, db)
    relin = to_host(ev.relinearize_keys(prod, sets, key_index))
    square = to_host(ev.multiply_relin_keys(da, da, sets, key_index))
    for i in range(count):
        k = int(key_index[i])
        ref = o.relinearize(o.multiply(a[i], b[i]), ten[k]["rk"])
        assert (fused[i] == ref).all(), (name, i, k)
        assert (relin[i] == ref).all(), (name, i, k)
        assert (square[i] == o.relinearize(o.multiply(a[i], a[i]), ten[k]["rk"])).all(), (name, i, k)
        if o.t % (2 * o.n) == 1:
            assert (o.batch_decode(o.decrypt(fused[i], ten[k]["sk"])) == (va[i] * vb[i]) % o.t).all()
    # another client's key gives other bits: the selection is not ignored
    other = (int(key_index[0]) + 1) % used
    assert not (fused[0] == o.relinearize(o.multiply(a[0], b[0]), ten[other]["rk"])).all()


def test_per_key_call_with_one_key_equals_the_single_key_call():
    """All items on key set 0 of several = hipbfv_batch_multiply_relin with that key, word for word (a large batch: the walk
    order of the key-switch kernel differs between the two calls, the bits must not)."""
    import torch
    from sunscreen_amd.batch import to_device

    o, ctx, ev, ten = _tenants("default_8192_17", 2)
    rng = np.random.default_rng(77)
    count = 67  # not a multiple of 8: the last XCD's run of the walk is short
    _, a = _enc(o, ten, [0] * 4, rng)
    _, b = _enc(o, ten, [0] * 4, rng)
    da = to_device(a).repeat(17, 1, 1, 1)[:count].contiguous()
    db = to_device(b).repeat(17, 1, 1, 1)[:count].contiguous()
    db[5:] = db[5:].roll(1, 0)  # (not 17 copies of the same four products)
    single = ev.multiply_relin(da, db, ten[0]["rkd"])
    sets = [ten[1]["rkd"], ten[0]["rkd"]]
    perkey = ev.multiply_relin_keys(da, db, sets, np.ones(count, dtype=np.uint32))
    mixed = ev.multiply_relin_keys(da, db, sets, (np.arange(count) % 2).astype(np.uint32))
    single1 = ev.multiply_relin(da, db, ten[1]["rkd"])
    torch.cuda.synchronize()
    assert torch.equal(single, perkey)
    odd = torch.arange(count, device=mixed.device) % 2 == 1
    assert torch.equal(mixed[odd], single[odd]) and torch.equal(mixed[~odd], single1[~odd])


def _shape_trials():
    # HIPBFV_FUZZ_PERKEY_TRIALS="lo:hi": extended campaigns (profiles/r06_s38_*); the suite's own are 0:6
    lo, hi = (int(x) for x in os.environ.get("HIPBFV_FUZZ_PERKEY_TRIALS", "0:6").split(":"))
    return range(lo, hi)


@pytest.mark.parametrize("trial", _shape_trials())
def test_per_key_random_shapes(trial):
    """Random tenant counts, batch sizes, chunk sizes and key assignments (runs of one key, every eighth item, unused key sets,
    counts that are no multiple of 8: the per-XCD walk of the key-switch kernels): every item of the per-key calls equals the
    single-key call with that item's key word for word, and two items per trial equal the oracle."""
    import torch
    from sunscreen_amd.batch import to_device, to_host

    rng = np.random.default_rng(9000 + trial)
    name = ("default_4096_16", "default_8192_17", "default_4096_16", "default_16384_17")[trial % 4]
    ntenants = int(rng.integers(1, 4 if "16384" in name else 10))
    count = int(rng.integers(1, 24 if "16384" in name else 90))
    o, ctx, ev, ten = _tenants(name, ntenants, seed=300 + trial)
    chunk = int(rng.choice([0, 0, 3, 8, 17]))
    if chunk:
        ev.set_chunk_ops(chunk)
    kind = trial % 3
    if kind == 0:
        key_index = rng.integers(0, ntenants, count)
    elif kind == 1:
        key_index = np.sort(rng.integers(0, ntenants, count))  # runs of one key
    else:
        key_index = np.arange(count) % ntenants  # neighbours never share a key
    key_index = key_index.astype(np.uint32)
    n, primes = o.n, params(name)[1]
    K = o.K
    a = np.stack([rng.integers(0, pr, (count, 2, n), dtype=np.uint64) for pr in primes[:K]], axis=2)
    b = np.stack([rng.integers(0, pr, (count, 2, n), dtype=np.uint64) for pr in primes[:K]], axis=2)
    da, db = to_device(a), to_device(b)
    sets = [x["rkd"] for x in ten]
    fused = ev.multiply_relin_keys(da, db, sets, key_index)
    relin = ev.relinearize_keys(ev.multiply(da, db), sets, key_index)
    torch.cuda.synchronize()
    assert torch.equal(fused, relin), (trial, name, ntenants, count, chunk)
    ki = torch.from_numpy(key_index.astype(np.int64)).to(fused.device)
    for k in range(ntenants):
        sel = ki == k
        if not bool(sel.any()):
            continue
        single = ev.multiply_relin(da[sel].contiguous(), db[sel].contiguous(), sets[k])
        assert torch.equal(fused[sel], single), (trial, name, ntenants, count, chunk, k)
    got = to_host(fused)
    for i in {0, count - 1}:
        assert (got[i] == o.relinearize(o.multiply(a[i], b[i]), ten[int(key_index[i])]["rk"])).all(), (trial, name, i)


def test_per_key_small_batches_take_the_whole_polynomial_pipeline():
    """A few items (<= 8 at n = 8192 under the product default) run through ks_mac instead of the split kernels: same contract."""
    from sunscreen_amd.batch import to_device, to_host

    o, ctx, ev, ten = _tenants("default_8192_17", 3)
    rng = np.random.default_rng(8)
    key_index = np.array([2, 0, 1, 2], dtype=np.uint32)
    _, a = _enc(o, ten, key_index, rng)
    _, b = _enc(o, ten, key_index, rng)
    got = to_host(ev.multiply_relin_keys(to_device(a), to_device(b), [x["rkd"] for x in ten], key_index))
    for i, k in enumerate(key_index):
        assert (got[i] == o.relinearize(o.multiply(a[i], b[i]), ten[int(k)]["rk"])).all(), i


def test_per_key_integer_policy_primes_3x54():
    """The north star's literal 3 x 54-bit set: integer-policy key primes (ks_mid_int_kernel) with per-item keys."""
    from sunscreen_amd.batch import to_device, to_host

    n = 8192
    primes = O.coeff_modulus_create(n, [54, 54, 54, 56])
    o, ctx, ev, ten = _tenants((n, primes, O.plain_batching(n, 17)), 4)
    rng = np.random.default_rng(54)
    key_index = np.array([3, 1, 0, 2, 1, 3, 0, 2, 2, 1], dtype=np.uint32)
    _, a = _enc(o, ten, key_index, rng)
    _, b = _enc(o, ten, key_index, rng)
    got = to_host(ev.multiply_relin_keys(to_device(a), to_device(b), [x["rkd"] for x in ten], key_index))
    for i, k in enumerate(key_index):
        assert (got[i] == o.relinearize(o.multiply(a[i], b[i]), ten[int(k)]["rk"])).all(), i


@pytest.mark.parametrize("name,count", [("default_4096_16", 11), ("default_8192_17", 6)])
def test_rotations_with_one_galois_key_set_per_client(name, count):
    """>= 4 Galois key sets in one call: direct keys, SEAL's NAF chain over power-of-two keys, the column swap."""
    from sunscreen_amd.batch import to_device, to_host

    o, ctx, ev, ten = _tenants(name, 5, galois="all", relin=False)
    rng = np.random.default_rng(count)
    key_index = rng.integers(0, 5, count).astype(np.uint32)
    key_index[:5] = rng.permutation(5)
    _, a = _enc(o, ten, key_index, rng)
    da = to_device(a)
    sets = [x["gkd"] for x in ten]
    for steps in (1, -3, 7):  # 1: a key every set holds; -3, 7: NAF chains (4 - 1, 8 - 1) over the power-of-two keys
        got = to_host(ev.rotate_rows_keys(da, steps, sets, key_index))
        for i, k in enumerate(key_index):
            assert (got[i] == o.rotate_rows(a[i], steps, ten[int(k)]["gk"])).all(), (steps, i)
    got = to_host(ev.rotate_columns_keys(da, sets, key_index))
    for i, k in enumerate(key_index):
        assert (got[i] == o.rotate_columns(a[i], ten[int(k)]["gk"])).all(), i
    elt = 9  # 3^2 mod 2n: the Galois element of a rotation by 2
    got = to_host(ev.apply_galois_keys(da, elt, sets, key_index))
    for i, k in enumerate(key_index):
        assert (got[i] == o.apply_galois(a[i], elt, ten[int(k)]["gk"])).all(), i


def test_program_run_with_one_key_set_per_input_set():
    """hipbfv_Program_RunKeys: the dot-product graph (multiply + relinearize, rotations, adds: examples/dot_prod/src/main.rs:38-75)
    over a batch whose input sets belong to 8 clients; merged launches number their items member-major and must still pick
    each input set's keys.  Both executors."""
    import os

    from sunscreen_amd.batch import to_device, to_host
    from sunscreen_amd.workloads import chi_sq_optimized, dot_product

    o, ctx, ev, ten = _tenants("default_4096_16", 8, galois="all")
    rng = np.random.default_rng(21)
    batch = 11
    key_index = rng.integers(0, 8, batch).astype(np.uint32)
    key_index[:8] = rng.permutation(8)
    prog = dot_product(o.n // 2)
    va, ca = _enc(o, ten, key_index, rng, hi=4)
    vb, cb = _enc(o, ten, key_index, rng, hi=4)
    rks, gks = [x["rkd"] for x in ten], [x["gkd"] for x in ten]
    for serial in ("0", "1"):
        os.environ["HIPBFV_PROGRAM_SERIAL"] = serial
        try:
            (out,) = prog.run(ev, [to_device(ca), to_device(cb)], rks, gks, key_index=key_index)
        finally:
            os.environ.pop("HIPBFV_PROGRAM_SERIAL", None)
        out = to_host(out)
        for i, k in enumerate(key_index):
            (ref,) = run_program(o, prog.nodes, prog.edges, [ca[i], cb[i]], ten[int(k)]["rk"], ten[int(k)]["gk"])
            assert (out[i] == ref).all(), (serial, i)
            dot = int((va[i].astype(np.int64) * vb[i].astype(np.int64)).sum()) % o.t
            assert (o.batch_decode(o.decrypt(out[i], ten[int(k)]["sk"])) == dot).all()
    # chi_sq (examples/chi_sq/src/main.rs:59-88): several multiply+relinearize members per round -> merged launches
    # (r06 s27: merged at every batch size -- 40 input sets: 3 x 40 and 2 x 40 items per launch, the key of item m * 40 + j is input set j's)
    prog = chi_sq_optimized()
    for key_index in (np.array([4, 7, 0, 4, 2], dtype=np.uint32), rng.integers(0, 8, 40).astype(np.uint32)):
        cts = [_enc(o, ten, key_index, rng, hi=7)[1] for _ in range(3)]
        outs = [to_host(t) for t in prog.run(ev, [to_device(c) for c in cts], rks, None, key_index=key_index)]
        for i, k in enumerate(key_index):  # every input set against the oracle under ITS client's keys
            ref = run_program(o, prog.nodes, prog.edges, [c[i] for c in cts], ten[int(k)]["rk"])
            for j in range(4):
                assert (outs[j][i] == ref[j]).all(), (len(key_index), i, j)


def test_per_key_argument_errors():
    """key_index out of range: E_INVALIDARG before anything is launched; a key set without the key: the missing-key error of the
    single-key call; a key object of another context counts as missing."""
    from sunscreen_amd import Context, RelinearizationKeys
    from sunscreen_amd.batch import to_device
    from sunscreen_amd.seal import HipBfvError

    o, ctx, ev, ten = _tenants("default_4096_16", 2)
    rng = np.random.default_rng(1)
    _, a = _enc(o, ten, [0, 1, 0], rng)
    da = to_device(a)
    sets = [x["rkd"] for x in ten]
    with pytest.raises(HipBfvError):
        ev.multiply_relin_keys(da, da, sets, np.array([0, 2, 1], dtype=np.uint32))
    n, primes, t = params("default_4096_16")
    other_ctx = Context.from_raw(n, primes, t)
    foreign = RelinearizationKeys.from_array(other_ctx, ten[0]["rk"])
    with pytest.raises(HipBfvError):
        ev.multiply_relin_keys(da, da, [sets[0], foreign], np.array([0, 1, 0], dtype=np.uint32))
    # and the call still works afterwards
    ev.multiply_relin_keys(da, da, sets, np.array([0, 1, 0], dtype=np.uint32))


def test_concurrent_clients_with_their_own_keys_on_one_evaluator():
    """The drop-in shape of a multi-tenant server: host threads (sunscreen_runtime's rayon pool, run.rs:415-469) call ONE
    evaluator's handle-level relinearize / rotate, each thread with its own client's keys.  Calls that meet in flight are
    combined into one per-key batch (capi.cpp: requests of one kind combine across keys); every result must be the oracle's for
    that client's key, whoever it was combined with."""
    import threading

    from sunscreen_amd import BFVEvaluator, Ciphertext

    o, ctx, bev, ten = _tenants("default_4096_16", 6, galois=[3])
    ev = BFVEvaluator(ctx)
    rng = np.random.default_rng(66)
    nthreads, iters = 6, 8
    vals = rng.integers(0, 30, (nthreads, 2, o.n)).astype(np.uint64)
    cts = [[o.encrypt(ten[i]["pk"], o.batch_encode(vals[i, j])) for j in range(2)] for i in range(nthreads)]
    exp_relin = [o.relinearize(o.multiply(c[0], c[1]), ten[i]["rk"]) for i, c in enumerate(cts)]
    exp_rot = [o.rotate_rows(c[0], 1, ten[i]["gk"]) for i, c in enumerate(cts)]
    errors = []
    start = threading.Barrier(nthreads)

    def worker(i):
        try:
            a, b = Ciphertext.from_array(ctx, cts[i][0]), Ciphertext.from_array(ctx, cts[i][1])
            start.wait()
            for _ in range(iters):
                m = ev.multiply(a, b)
                ev.relinearize_inplace(m, ten[i]["rkd"])
                if not (m.to_array() == exp_relin[i]).all():
                    errors.append((i, "relinearize mismatch"))
                r = ev.rotate_rows(a, 1, ten[i]["gkd"])
                if not (r.to_array() == exp_rot[i]).all():
                    errors.append((i, "rotation mismatch"))
        except Exception as e:  # noqa: BLE001
            errors.append((i, repr(e)))

    ts = [threading.Thread(target=worker, args=(i,)) for i in range(nthreads)]
    for th in ts:
        th.start()
    for th in ts:
        th.join()
    assert not errors, errors


# ---- per-client key isolation: tenants that hold DIFFERENT kinds of keys (include/hipbfv.h: the per-item key rule) ----
E_INVALIDARG = 0x80070057


def _mixed_tenants(name):
    """Tenant D: the power-of-two Galois keys plus the direct keys of steps 3 and -5; tenant P: the power-of-two keys only
    (steps 3, -5, 7 take SEAL's NAF chain); tenant R: a relinearisation key and no Galois key; `foreign`: P's keys loaded
    into another context of the same parameters (a key object the evaluator must not accept)."""
    from sunscreen_amd import Context, GaloisKeys, RelinearizationKeys
    from sunscreen_amd.batch import BatchEvaluator

    n, primes, t = params(name)
    o = oracle_for(name)
    ctx = Context.from_raw(n, primes, t)
    ev = BatchEvaluator(ctx)
    O.seed(501)
    skP, pkP, rkP, gkP = o.keygen(galois_elts="all")
    elts = sorted(gkP) + [o.galois_elt_from_step(3), o.galois_elt_from_step(-5)]
    O.seed(502)
    skD, pkD, rkD, gkD = o.keygen(galois_elts=elts)
    O.seed(503)
    skR, pkR, rkR, _ = o.keygen()
    ten = {
        "D": {"sk": skD, "pk": pkD, "rk": rkD, "gk": gkD},
        "P": {"sk": skP, "pk": pkP, "rk": rkP, "gk": gkP},
        "R": {"sk": skR, "pk": pkR, "rk": rkR, "gk": {}},
    }
    for x in ten.values():
        x["rkd"] = RelinearizationKeys.from_array(ctx, x["rk"])
        x["gkd"] = GaloisKeys.from_arrays(ctx, x["gk"]) if x["gk"] else None
    other = Context.from_raw(n, primes, t)
    foreign = {"rkd": RelinearizationKeys.from_array(other, rkP), "gkd": GaloisKeys.from_arrays(other, gkP), "ctx": other}
    return o, ctx, ev, ten, foreign


def _enc_for(o, pks, rng):
    return np.stack([o.encrypt(pk, o.batch_encode(rng.integers(0, o.t, o.n).astype(np.uint64))) for pk in pks])


@pytest.mark.parametrize(
    "name,count,chunk",
    [
        ("default_4096_16", 23, 5),  # chunks of 5, a short last chunk
        ("default_8192_17", 21, 7),  # above the small-batch limit (16 at n = 8192), three chunks
        ("default_8192_17", 9, 0),
    ],
)
def test_rotate_rows_keys_with_mixed_holdings(name, count, chunk):
    """D's items rotate with D's direct keys, P's items over P's NAF chain, whoever else is in the batch: every item equals the
    oracle with its own keys and, word for word, the single-key call with that item's set; out of place and in place."""
    import torch
    from sunscreen_amd.batch import to_device, to_host

    o, ctx, ev, ten, _ = _mixed_tenants(name)
    if chunk:
        ev.set_chunk_ops(chunk)
    rng = np.random.default_rng(count * 31 + chunk)
    key_index = rng.integers(0, 2, count).astype(np.uint32)
    key_index[:2] = (1, 0)
    who = ["D", "P"]
    a = _enc_for(o, [ten[who[k]]["pk"] for k in key_index], rng)
    da = to_device(a)
    sets = [ten["D"]["gkd"], ten["P"]["gkd"]]
    ki = torch.from_numpy(key_index.astype(np.int64)).to(da.device)
    for steps in (3, -5, 7):
        got = ev.rotate_rows_keys(da, steps, sets, key_index)
        inplace = da.clone()
        ev.rotate_rows_keys(inplace, steps, sets, key_index, out=inplace)
        torch.cuda.synchronize()
        assert torch.equal(got, inplace), (name, steps)
        for k in (0, 1):
            sel = ki == k
            single = ev.rotate_rows(da[sel].contiguous(), steps, sets[k])
            assert torch.equal(got[sel], single), (name, steps, who[k])
        host = to_host(got)
        for i, k in enumerate(key_index):
            ref = o.rotate_rows(a[i], steps, ten[who[k]]["gk"])
            assert (host[i] == ref).all(), (name, steps, i, who[k])
    ev.check()


def test_unreferenced_key_sets_are_not_validated():
    """NULL, a set without the key and a key object of another context in the key arrays, never named by key_index: every
    per-key call succeeds with the bits of the referenced sets alone."""
    from sunscreen_amd.batch import to_device, to_host

    o, ctx, ev, ten, foreign = _mixed_tenants("default_4096_16")
    rng = np.random.default_rng(5)
    key_index = np.array([0, 4, 4, 0, 4, 0, 0, 4, 4, 0, 4], dtype=np.uint32)  # sets 1, 2, 3 unused
    who = {0: "D", 4: "P"}
    a = _enc_for(o, [ten[who[k]]["pk"] for k in key_index], rng)
    b = _enc_for(o, [ten[who[k]]["pk"] for k in key_index], rng)
    da, db = to_device(a), to_device(b)
    rsets = [ten["D"]["rkd"], None, ten["P"]["gkd"], foreign["rkd"], ten["P"]["rkd"]]  # 2: a Galois object, no relin key
    gsets = [ten["D"]["gkd"], None, ten["R"]["rkd"], foreign["gkd"], ten["P"]["gkd"]]  # 2: R's relin object, no Galois key
    mr = to_host(ev.multiply_relin_keys(da, db, rsets, key_index))
    rl = to_host(ev.relinearize_keys(ev.multiply(da, db), rsets, key_index))
    elt = o.galois_elt_from_step(2)
    ag = to_host(ev.apply_galois_keys(da, elt, gsets, key_index))
    rc = to_host(ev.rotate_columns_keys(da, gsets, key_index))
    rr = {s: to_host(ev.rotate_rows_keys(da, s, gsets, key_index)) for s in (3, -5)}
    for i, k in enumerate(key_index):
        x = ten[who[k]]
        ref = o.relinearize(o.multiply(a[i], b[i]), x["rk"])
        assert (mr[i] == ref).all() and (rl[i] == ref).all(), i
        assert (ag[i] == o.apply_galois(a[i], elt, x["gk"])).all(), i
        assert (rc[i] == o.rotate_columns(a[i], x["gk"])).all(), i
        for s in (3, -5):
            assert (rr[s][i] == o.rotate_rows(a[i], s, x["gk"])).all(), (s, i)
    ev.check()


def test_referenced_key_set_without_the_key_fails_like_the_single_key_call():
    """A set key_index names that lacks the key (NULL, a set without it, another context's object): E_INVALIDARG before
    anything is launched, the error names the set, the output keeps its sentinel, the evaluator serves the next call.  For
    rotate_rows_keys "without the key" means neither the direct key nor the NAF chain's power-of-two keys."""
    import torch
    from sunscreen_amd.batch import to_device, to_host
    from sunscreen_amd.seal import HipBfvError

    o, ctx, ev, ten, foreign = _mixed_tenants("default_4096_16")
    rng = np.random.default_rng(6)
    count = 6
    a = _enc_for(o, [ten["P"]["pk"]] * count, rng)
    da = to_device(a)
    ct3 = ev.multiply(da, da)
    # the single-key calls fail the same way
    with pytest.raises(HipBfvError) as exc:
        ev.rotate_rows(da, 3, ten["R"]["rkd"])
    assert exc.value.hresult == E_INVALIDARG
    with pytest.raises(HipBfvError) as exc:
        ev.relinearize(ct3, ten["P"]["gkd"])
    assert exc.value.hresult == E_INVALIDARG
    key_index = np.array([0, 1, 0, 2, 0, 0], dtype=np.uint32)
    cases = {
        "relinearize_keys": lambda bad, out: ev.relinearize_keys(ct3, [ten["P"]["rkd"], ten["P"]["rkd"], bad], key_index, out=out),
        "multiply_relin_keys": lambda bad, out: ev.multiply_relin_keys(da, da, [ten["P"]["rkd"], ten["P"]["rkd"], bad], key_index, out=out),
        "apply_galois_keys": lambda bad, out: ev.apply_galois_keys(da, o.galois_elt_from_step(1), [ten["P"]["gkd"], ten["D"]["gkd"], bad], key_index, out=out),
        "rotate_columns_keys": lambda bad, out: ev.rotate_columns_keys(da, [ten["P"]["gkd"], ten["D"]["gkd"], bad], key_index, out=out),
        "rotate_rows_keys": lambda bad, out: ev.rotate_rows_keys(da, 3, [ten["P"]["gkd"], ten["D"]["gkd"], bad], key_index, out=out),
    }
    relin_bad = [None, ten["P"]["gkd"], foreign["rkd"]]
    galois_bad = [None, ten["R"]["rkd"], foreign["gkd"]]
    sentinel = -0x5A5A5A5A5A5A5A5B
    for what, call in cases.items():
        for bad in relin_bad if "relin" in what else galois_bad:
            out = torch.full_like(da, sentinel)
            with pytest.raises(HipBfvError) as exc:
                call(bad, out)
            assert exc.value.hresult == E_INVALIDARG, (what, exc.value)
            assert "key set 2" in str(exc.value), (what, str(exc.value))
            torch.cuda.synchronize()
            assert bool((out == sentinel).all()), what
    ev.check()
    # the evaluator works for the next call
    good = to_host(ev.rotate_rows_keys(da, 3, [ten["P"]["gkd"], ten["D"]["gkd"]], key_index % 2))
    for i, k in enumerate(key_index % 2):
        assert (good[i] == o.rotate_rows(a[i], 3, ten[("P", "D")[k]]["gk"])).all(), i


def _rotate_3_5_program():
    from sunscreen_amd.program import FheProgram

    p = FheProgram()
    a = p.append_input_ciphertext(0)
    r3 = p.append_rotate_left(a, p.append_input_literal(3))
    r5 = p.append_rotate_left(a, p.append_input_literal(5))
    p.append_output_ciphertext(p.append_add(r3, r5))
    return p


def test_program_run_keys_with_mixed_holdings():
    """hipbfv_Program_RunKeys, both executors: input sets of D (direct key of step 3) and P (NAF chain) interleaved -- every set
    equals hipbfv_Program_Run with that set's keys alone and the oracle with its keys; chi_sq with an unreferenced NULL
    relinearisation slot; a referenced key object of another context fails as in the batch calls."""
    import torch
    from sunscreen_amd.batch import to_device, to_host
    from sunscreen_amd.seal import HipBfvError
    from sunscreen_amd.workloads import chi_sq_optimized

    o, ctx, ev, ten, foreign = _mixed_tenants("default_4096_16")
    rng = np.random.default_rng(44)
    prog = _rotate_3_5_program()
    key_index = np.array([0, 1, 1, 0, 1, 0, 0, 1, 0], dtype=np.uint32)
    who = ["D", "P"]
    cts = _enc_for(o, [ten[who[k]]["pk"] for k in key_index], rng)
    dct = to_device(cts)
    gks = [ten["D"]["gkd"], ten["P"]["gkd"]]
    for serial in ("0", "1"):
        os.environ["HIPBFV_PROGRAM_SERIAL"] = serial
        try:
            (out,) = prog.run(ev, [dct], None, gks, key_index=key_index)
            singles = [prog.run(ev, [dct[i : i + 1].contiguous()], None, gks[int(k)])[0] for i, k in enumerate(key_index)]
        finally:
            os.environ.pop("HIPBFV_PROGRAM_SERIAL", None)
        torch.cuda.synchronize()
        host = to_host(out)
        for i, k in enumerate(key_index):
            assert torch.equal(out[i : i + 1], singles[i]), (serial, i, who[k])
            (ref,) = run_program(o, prog.nodes, prog.edges, [cts[i]], None, ten[who[k]]["gk"])
            assert (host[i] == ref).all(), (serial, i, who[k])
    # chi_sq: relin slot 1 is NULL and never named
    prog = chi_sq_optimized()
    key_index = np.array([0, 2, 2, 0, 2], dtype=np.uint32)
    rks = [ten["D"]["rkd"], None, ten["P"]["rkd"]]
    own = {0: "D", 2: "P"}
    args = [_enc_for(o, [ten[own[k]]["pk"] for k in key_index], np.random.default_rng(j)) for j in range(3)]
    for serial in ("0", "1"):
        os.environ["HIPBFV_PROGRAM_SERIAL"] = serial
        try:
            outs = [to_host(t) for t in prog.run(ev, [to_device(c) for c in args], rks, None, key_index=key_index)]
        finally:
            os.environ.pop("HIPBFV_PROGRAM_SERIAL", None)
        for i, k in enumerate(key_index):
            ref = run_program(o, prog.nodes, prog.edges, [c[i] for c in args], ten[own[int(k)]]["rk"])
            for j in range(4):
                assert (outs[j][i] == ref[j]).all(), (serial, i, j)
    with pytest.raises(HipBfvError) as exc:
        prog.run(ev, [to_device(c) for c in args], [ten["D"]["rkd"], None, foreign["rkd"]], None, key_index=key_index)
    assert exc.value.hresult == E_INVALIDARG
    assert "key set 2" in str(exc.value), str(exc.value)
    ev.check()


def test_concurrent_clients_with_mixed_galois_holdings_on_one_evaluator():
    """The handle-level drop-in shape with clients D and P rotating by 3 at once: requests that meet in flight combine only
    when they share a Galois element, so D's thread gets the direct-key bits and P's the NAF-chain bits."""
    import threading

    from sunscreen_amd import BFVEvaluator, Ciphertext

    o, ctx, _, ten, _ = _mixed_tenants("default_4096_16")
    ev = BFVEvaluator(ctx)
    rng = np.random.default_rng(67)
    clients = ["D", "P", "D", "P", "D", "P"]
    cts = [_enc_for(o, [ten[c]["pk"]], rng)[0] for c in clients]
    exp = [o.rotate_rows(ct, 3, ten[c]["gk"]) for ct, c in zip(cts, clients)]
    naf_only = {e: k for e, k in ten["D"]["gk"].items() if e != o.galois_elt_from_step(3)}
    assert not (exp[0] == o.rotate_rows(cts[0], 3, naf_only)).all()  # the direct key and the NAF chain give other bits
    errors = []
    start = threading.Barrier(len(clients))

    def worker(i):
        try:
            a = Ciphertext.from_array(ctx, cts[i])
            start.wait()
            for _ in range(8):
                r = ev.rotate_rows(a, 3, ten[clients[i]]["gkd"])
                if not (r.to_array() == exp[i]).all():
                    errors.append((i, clients[i], "rotation mismatch"))
        except Exception as e:  # noqa: BLE001
            errors.append((i, repr(e)))

    ts = [threading.Thread(target=worker, args=(i,)) for i in range(len(clients))]
    for th in ts:
        th.start()
    for th in ts:
        th.join()
    assert not errors, errors
