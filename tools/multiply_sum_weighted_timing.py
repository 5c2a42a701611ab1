#!/usr/bin/env python3
"""tools/multiply_sum_weighted_timing.py -- weighted sums of products with one relinearization per group
(hipbfv_batch_multiply_sum_weighted_relin) against what a caller had before it, on one GPU, device-resident operands of uniform
canonical residues (valid ciphertext bit patterns).

Shapes: n = 8192 with 512 groups x 8 terms, n = 16384 with 128 x 8, weights alternating +1 / -1; and one determinant shape per degree
(terms = 2, weights (1, -1)) with the same number of products: 2048 x 2 and 512 x 2.  SEAL's default primes.

Arms, alternating in one process, ROUNDS samples of CALLS whole calls each:
  new         one multiply_sum_weighted_relin call
  by_hand     the parent's entry points only: hipbfv_batch_multiply on all terms, hipbfv_batch_negate on the negative ones, a tree of
              hipbfv_batch_add, hipbfv_batch_relinearize: the same bits, checked word for word
  eager       hipbfv_batch_multiply_relin on all terms, then negate and the add tree on the size-2 results (a key switch per term;
              other bits, so only timed)
  unweighted  hipbfv_batch_multiply_sum_relin on the same operands: other bits; what the weight costs
The comparison arms get their best layout: their operands are a TERM-major copy ([terms][groups]) made outside the timed region, the
positive terms first, so that the negative ones are one contiguous half (one negate call) and every level of the tree adds two
contiguous halves in one call.
Prints one JSON object: per shape and arm the best and the median time of a call and the run-to-run spread ((max - min) / median), and the
HIP-event time per kernel of one `new` and one `unweighted` call."""
import json
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

SHAPES = [(8192, 512, 8), (16384, 128, 8), (8192, 2048, 2), (16384, 512, 2)]
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
    weights = [1 if t % 2 == 0 else -1 for t in range(terms)]

    def operand():
        host = np.empty((groups, terms, 2, K, n), dtype=np.uint64)
        for k in range(K):
            host[:, :, :, k, :] = rng.integers(0, primes[k], (groups, terms, 2, n), dtype=np.uint64)
        return to_device(host)

    a, b = operand(), operand()
    count = groups * terms
    order = [t for t in range(terms) if weights[t] > 0] + [t for t in range(terms) if weights[t] < 0]
    a_tm = a.transpose(0, 1)[order].contiguous().view(count, 2, K, n)
    b_tm = b.transpose(0, 1)[order].contiguous().view(count, 2, K, n)
    out_new = torch.empty((groups, 2, K, n), dtype=a.dtype, device=a.device)
    out_hand, out_eager, out_unw = torch.empty_like(out_new), torch.empty_like(out_new), torch.empty_like(out_new)
    prod3 = torch.empty((count, 3, K, n), dtype=a.dtype, device=a.device)
    prod2 = torch.empty((count, 2, K, n), dtype=a.dtype, device=a.device)
    assert terms & (terms - 1) == 0 and terms >= 2, "the tree halves the terms"

    def signed_tree(buf):
        ev.negate(buf[count // 2:], out=buf[count // 2:])
        live = count
        while live > groups:
            live //= 2
            ev.add(buf[:live], buf[live:2 * live], out=buf[:live])
        return buf[:groups]

    def arm_new():
        ev.multiply_sum_weighted_relin(a, b, weights, rk, out=out_new)

    def arm_by_hand():
        ev.multiply(a_tm, b_tm, out=prod3)
        ev.relinearize(signed_tree(prod3), rk, out=out_hand)

    def arm_eager():
        ev.multiply_relin(a_tm, b_tm, rk, out=prod2)
        out_eager.copy_(signed_tree(prod2))

    def arm_unweighted():
        ev.multiply_sum_relin(a, b, rk, out=out_unw)

    arms = {"new": arm_new, "by_hand": arm_by_hand, "eager": arm_eager, "unweighted": arm_unweighted}
    for fn in arms.values():  # warm-up: scratch, code objects
        fn()
        fn()
    torch.cuda.synchronize()
    equal = bool(torch.equal(out_new, out_hand))
    samples = {k: [] for k in arms}
    for _ in range(ROUNDS):
        for name, fn in arms.items():
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for _ in range(CALLS):
                fn()
            torch.cuda.synchronize()
            samples[name].append((time.perf_counter() - t0) / CALLS)
    kernels = {}
    ev.profile(True)
    for name in ("new", "unweighted", "by_hand"):
        ev.profile_reset()
        arms[name]()
        torch.cuda.synchronize()
        kernels[name] = {k: round(v["ms"], 3) for k, v in ev.profile_read().items()}
    ev.profile(False)
    res = {"n": n, "K": K, "groups": groups, "terms": terms, "weights": weights, "new_equals_by_hand": equal, "kernel_ms": kernels}
    for name, ts in samples.items():
        med = statistics.median(ts)
        res[name] = {"best_ms": round(min(ts) * 1e3, 3), "median_ms": round(med * 1e3, 3), "spread": round((max(ts) - min(ts)) / med, 4),
                     "median_terms_per_s": round(count / med, 1)}
    med = {k: statistics.median(v) for k, v in samples.items()}
    res["by_hand_over_new_median"] = round(med["by_hand"] / med["new"], 4)
    res["eager_over_new_median"] = round(med["eager"] / med["new"], 4)
    res["new_over_unweighted_median"] = round(med["new"] / med["unweighted"], 4)
    # the condition of the change: new's median below by_hand's by more than the larger of the two arms' spreads
    # (max - min, in seconds)
    res["new_beats_by_hand"] = bool(med["by_hand"] - med["new"] > max(max(samples[k]) - min(samples[k]) for k in ("new", "by_hand")))
    del a, b, a_tm, b_tm, prod3, prod2
    torch.cuda.empty_cache()
    return res


def main():
    import torch

    res = {"device": torch.cuda.get_device_name(0), "rounds": ROUNDS, "calls_per_sample": CALLS, "shapes": [measure(*s) for s in SHAPES]}
    print(json.dumps(res))
    return 0 if all(s["new_equals_by_hand"] for s in res["shapes"]) else 1


if __name__ == "__main__":
    sys.exit(main())
