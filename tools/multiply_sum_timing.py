#!/usr/bin/env python3
"""tools/multiply_sum_timing.py -- sums of products with one relinearization per group (hipbfv_batch_multiply_sum_relin) against the two
ways a caller had before it, on one GPU, device-resident operands of uniform canonical residues (valid ciphertext bit patterns).

Shapes: n = 8192 with 512 groups x 8 terms, n = 16384 with 128 x 8 (SEAL's default primes).

Arms, alternating in one process, ROUNDS samples of CALLS whole calls each:
  new           one multiply_sum_relin call
  lazy_by_hand  hipbfv_batch_multiply on all terms, a tree of hipbfv_batch_add (3 calls for 8 terms), hipbfv_batch_relinearize:
                the same bits, checked word for word
  eager         hipbfv_batch_multiply_relin on all terms, then the add tree on the size-2 results: what callers do today
                (a key switch per term; other bits, so only timed)
The comparison arms get their best layout: their operands are a TERM-major copy ([terms][groups]) made outside the timed region, so
that every level of the tree adds two contiguous halves in one call.
Prints one JSON object: per shape and arm the best and the median time of a call and the run-to-run spread ((max - min) / median)."""
import json
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

SHAPES = [(8192, 512, 8), (16384, 128, 8)]
ROUNDS, CALLS = 10, 3


def measure(n, groups, terms):
    import torch

    from sunscreen_amd.batch import BatchEvaluator, to_device
    from sunscreen_amd.seal import CoefficientModulus, Context, KeyGenerator

    primes = [int(m.value()) for m in CoefficientModulus.bfv_default(n)]
    ctx = Context.from_raw(n, primes, 114689)
    rk = KeyGenerator(ctx, seed=n).create_relinearization_keys()
    ev = BatchEvaluator(ctx)
    K = ctx.K
    rng = np.random.default_rng(n)

    def operand():
        host = np.empty((groups, terms, 2, K, n), dtype=np.uint64)
        for k in range(K):
            host[:, :, :, k, :] = rng.integers(0, primes[k], (groups, terms, 2, n), dtype=np.uint64)
        return to_device(host)

    a, b = operand(), operand()
    count = groups * terms
    a_tm = a.transpose(0, 1).contiguous().view(count, 2, K, n)
    b_tm = b.transpose(0, 1).contiguous().view(count, 2, K, n)
    out_new = torch.empty((groups, 2, K, n), dtype=a.dtype, device=a.device)
    out_lazy, out_eager = torch.empty_like(out_new), torch.empty_like(out_new)
    prod3 = torch.empty((count, 3, K, n), dtype=a.dtype, device=a.device)
    prod2 = torch.empty((count, 2, K, n), dtype=a.dtype, device=a.device)
    assert terms & (terms - 1) == 0, "the tree halves the terms"

    def tree(buf):
        live = count
        while live > groups:
            live //= 2
            ev.add(buf[:live], buf[live:2 * live], out=buf[:live])
        return buf[:groups]

    def arm_new():
        ev.multiply_sum_relin(a, b, rk, out=out_new)

    def arm_lazy():
        ev.multiply(a_tm, b_tm, out=prod3)
        ev.relinearize(tree(prod3), rk, out=out_lazy)

    def arm_eager():
        ev.multiply_relin(a_tm, b_tm, rk, out=prod2)
        out_eager.copy_(tree(prod2))

    arms = {"new": arm_new, "lazy_by_hand": arm_lazy, "eager": arm_eager}
    for fn in arms.values():  # warm-up: scratch, code objects
        fn()
        fn()
    torch.cuda.synchronize()
    equal = bool(torch.equal(out_new, out_lazy))
    samples = {k: [] for k in arms}
    for _ in range(ROUNDS):
        for name, fn in arms.items():
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for _ in range(CALLS):
                fn()
            torch.cuda.synchronize()
            samples[name].append((time.perf_counter() - t0) / CALLS)
    ev.profile(True)
    ev.profile_reset()
    arm_new()
    torch.cuda.synchronize()
    kernels = {k: round(v["ms"], 3) for k, v in ev.profile_read().items()}
    ev.profile_reset()
    arm_lazy()
    torch.cuda.synchronize()
    kernels_lazy = {k: round(v["ms"], 3) for k, v in ev.profile_read().items()}
    ev.profile(False)
    res = {"n": n, "K": K, "groups": groups, "terms": terms, "new_equals_lazy_by_hand": equal, "kernel_ms_new": kernels,
           "kernel_ms_lazy_by_hand": kernels_lazy}
    for name, ts in samples.items():
        med = statistics.median(ts)
        res[name] = {"best_ms": round(min(ts) * 1e3, 3), "median_ms": round(med * 1e3, 3), "spread": round((max(ts) - min(ts)) / med, 4),
                     "median_terms_per_s": round(count / med, 1)}
    med = {k: statistics.median(v) for k, v in samples.items()}
    res["new_over_lazy_by_hand_median"] = round(med["lazy_by_hand"] / med["new"], 4)
    res["new_over_eager_median"] = round(med["eager"] / med["new"], 4)
    del a, b, a_tm, b_tm, prod3, prod2
    torch.cuda.empty_cache()
    return res


def main():
    import torch

    res = {"device": torch.cuda.get_device_name(0), "rounds": ROUNDS, "calls_per_sample": CALLS, "shapes": [measure(*s) for s in SHAPES]}
    print(json.dumps(res))
    return 0 if all(s["new_equals_lazy_by_hand"] for s in res["shapes"]) else 1


if __name__ == "__main__":
    sys.exit(main())
