#!/usr/bin/env python3
"""tools/pool_timing.py -- the device pool (hipbfv_Pool_*) from HOST memory: what a server gets when its ciphertexts arrive from
the network and it hands them to DevicePool as they are.

Legs (every rate counts the whole synchronous call: host-to-device copies, compute, device-to-host copies):
  mulrelin    -- hipbfv_Pool_MultiplyRelin, one member on device 0, at n = 8192 (batch 2048, chunks of 256) and n = 16384 (batch
                 1024, chunks of 128), inputs and outputs pinned (torch pin_memory) and pageable (numpy)
  chi_sq      -- hipbfv_Pool_ProgramRun of sunscreen_amd/workloads.py:chi_sq_optimized at n = 16384 from pageable host memory,
                 members [0] and [0, 0] (what a second member on the same link does), beside the resident rate of
                 FheProgram.run on the same batch (inputs and outputs in HBM, for scale)
  bits_equal  -- whether every pool result above equals the single-device call word for word
Only the library is used (its own key generator; operands are uniform canonical residues: valid ciphertext bit patterns).
Prints one JSON object."""
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

REPS = 5


def _residues(n, primes, K, count, seed):
    rng = np.random.default_rng(seed)
    out = np.empty((count, 2, K, n), dtype=np.uint64)
    for k in range(K):
        out[:, :, k, :] = rng.integers(0, primes[k], (count, 2, n), dtype=np.uint64)
    return out


def _best(fn):
    fn()  # warm-up: buffers, key copies, plans
    best = float("inf")
    for _ in range(REPS):
        t0 = time.perf_counter()
        fn()
        best = min(best, time.perf_counter() - t0)
    return best


def _context(n):
    from sunscreen_amd.seal import CoefficientModulus, Context, KeyGenerator

    primes = [int(m.value()) for m in CoefficientModulus.bfv_default(n)]
    ctx = Context.from_raw(n, primes, 114689 if n == 8192 else 786433)
    return ctx, primes, KeyGenerator(ctx, seed=7).create_relinearization_keys()


def mulrelin(n, batch, chunk):
    import torch

    from sunscreen_amd import DevicePool
    from sunscreen_amd.batch import BatchEvaluator, to_device, to_host

    ctx, primes, rk = _context(n)
    K = ctx.K
    a = _residues(n, primes, K, batch, 1)
    b = _residues(n, primes, K, batch, 2)
    ref = to_host(BatchEvaluator(ctx).multiply_relin(to_device(a), to_device(b), rk))
    torch.cuda.empty_cache()
    shape = (batch, 2, K, n)
    pa, pb, po = (torch.empty(shape, dtype=torch.int64, pin_memory=True) for _ in range(3))
    pa.numpy()[:] = a.view(np.int64)
    pb.numpy()[:] = b.view(np.int64)
    out = np.empty(shape, dtype=np.uint64)
    pool = DevicePool(ctx, [0])
    pool.set_chunk(chunk)
    t_pin = _best(lambda: pool.multiply_relin(pa, pb, rk, out=po))
    eq = bool((po.numpy().view(np.uint64) == ref).all())
    t_page = _best(lambda: pool.multiply_relin(a, b, rk, out=out))
    eq = eq and bool((out == ref).all())
    pool.close()
    return {
        "n": n, "batch": batch, "chunk": chunk, "K": K,
        "pinned_ops_per_s": round(batch / t_pin, 1), "pageable_ops_per_s": round(batch / t_page, 1),
        "pinned_ms": round(t_pin * 1e3, 2), "pageable_ms": round(t_page * 1e3, 2), "bits_equal": eq,
    }


def chi_sq(n, batch, chunk):
    import torch

    from sunscreen_amd import DevicePool
    from sunscreen_amd.batch import BatchEvaluator, to_device, to_host
    from sunscreen_amd.workloads import chi_sq_optimized

    ctx, primes, rk = _context(n)
    prog = chi_sq_optimized()
    cts = [_residues(n, primes, ctx.K, batch, 10 + i) for i in range(3)]
    ev = BatchEvaluator(ctx)
    dev_in = [to_device(c) for c in cts]

    def resident():
        prog.run(ev, dev_in, rk)
        torch.cuda.synchronize()

    t_res = _best(resident)
    ref = [to_host(t) for t in prog.run(ev, dev_in, rk)]
    del dev_in
    torch.cuda.empty_cache()
    res = {"n": n, "batch": batch, "chunk": chunk, "resident_programs_per_s": round(batch / t_res, 1)}
    eq = True
    for label, members in (("members_0", [0]), ("members_0_0", [0, 0])):
        pool = DevicePool(ctx, members)
        pool.set_chunk(chunk)
        outs = [np.empty((batch, 2, ctx.K, n), dtype=np.uint64) for _ in range(4)]
        t = _best(lambda: pool.run(prog, cts, rk, outputs=outs))
        eq = eq and all((o == r).all() for o, r in zip(outs, ref))
        res[f"pageable_programs_per_s_{label}"] = round(batch / t, 1)
        pool.close()
    res["bits_equal"] = bool(eq)
    return res


def main():
    import torch

    from sunscreen_amd import _lib

    _lib.load().hipbfv_set_device(0)
    torch.cuda.set_device(0)
    out = {
        "tool": "pool_timing",
        "device": torch.cuda.get_device_name(0),
        "reps": REPS,
        "mulrelin": [mulrelin(8192, 2048, 256), mulrelin(16384, 1024, 128)],
        "chi_sq": chi_sq(16384, 1024, 128),
    }
    out["bits_equal"] = all(r["bits_equal"] for r in out["mulrelin"]) and out["chi_sq"]["bits_equal"]
    print(json.dumps(out))


if __name__ == "__main__":
    main()
