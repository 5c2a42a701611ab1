#!/usr/bin/env python3
"""tools/multiply_shared_timing.py [out.json] -- products over a prepared multiplicand against the parent's entry points on a replicated
second operand, on one GPU, device-resident operands of uniform canonical residues (valid ciphertext bit patterns), SEAL's default primes.

Shapes: the matrix-vector product out[g] = sum_t A[g][t] * x[t] (b_index = {0..7}; n = 8192: 512 groups x 8 terms, n = 16384: 128 x 8) and
the broadcast a[i] * x (b_index = {0}; n = 8192: 4096 items, n = 16384: 1024).  Arms, alternating in one process, ROUNDS samples of CALLS
whole calls each: `new` = one *_shared call, prepare() outside the timed region and timed on its own; `by_hand` = multiply_sum_relin /
multiply_relin on a replicated b made outside the timed region (the same words, compared in the run).  Prints and writes (default
profiles/multiply_shared_timing.json) one JSON object: per shape and arm best and median ms and spread ((max - min) / median), HIP-event
ms per kernel of one call of each arm and of prepare(), the bytes the multiplicand holds, the uses that repay prepare(), and the
condition: new's median below by_hand's by more than the larger of the two arms' spreads."""
import json
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

# (n, groups, terms): terms == 0 is the broadcast multiply_relin_shared of `groups` items
SHAPES = [(8192, 512, 8), (16384, 128, 8), (8192, 4096, 0), (16384, 1024, 0)]
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
    sums = terms > 0
    count = groups * terms if sums else groups
    nprep = terms if sums else 1
    index = list(range(nprep))

    def operand(items):
        host = np.empty((items, 2, K, n), dtype=np.uint64)
        for k in range(K):
            host[:, :, k, :] = rng.integers(0, primes[k], (items, 2, n), dtype=np.uint64)
        return to_device(host)

    a, x = operand(count), operand(nprep)
    b = x.repeat(count // nprep, 1, 1, 1).contiguous()  # item i uses x[i % nprep]
    if sums:
        a, b = a.view(groups, terms, 2, K, n), b.view(groups, terms, 2, K, n)
    out_new = torch.empty((groups, 2, K, n), dtype=a.dtype, device=a.device)
    out_hand = torch.empty_like(out_new)
    torch.cuda.synchronize()
    prep = []
    m = None
    for _ in range(ROUNDS + 1):  # (the first one warms up)
        if m is not None:
            m.close()
        t0 = time.perf_counter()
        m = ev.prepare(x)
        torch.cuda.synchronize()
        prep.append(time.perf_counter() - t0)
    prep = prep[1:]

    if sums:
        arms = {"new": lambda: ev.multiply_sum_relin_shared(a, m, index, rk, out=out_new),
                "by_hand": lambda: ev.multiply_sum_relin(a, b, rk, out=out_hand)}
    else:
        arms = {"new": lambda: ev.multiply_relin_shared(a, m, index, rk, out=out_new),
                "by_hand": lambda: ev.multiply_relin(a, b, rk, out=out_hand)}
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
    for name, fn in list(arms.items()) + [("prepare", lambda: ev.prepare(x).close())]:
        ev.profile_reset()
        fn()
        torch.cuda.synchronize()
        kernels[name] = {k: round(v["ms"], 3) for k, v in ev.profile_read().items()}
    ev.profile(False)
    res = {"n": n, "K": K, "call": "multiply_sum_relin_shared" if sums else "multiply_relin_shared", "groups": groups, "terms": terms, "items": count,
           "prepared": nprep, "multiplicand_bytes": m.nbytes, "new_equals_by_hand": equal, "kernel_ms": kernels}
    for name, ts in samples.items():
        med = statistics.median(ts)
        res[name] = {"best_ms": round(min(ts) * 1e3, 3), "median_ms": round(med * 1e3, 3), "spread": round((max(ts) - min(ts)) / med, 4),
                     "median_items_per_s": round(count / med, 1)}
    med = {k: statistics.median(v) for k, v in samples.items()}
    pm = statistics.median(prep)
    res["prepare"] = {"best_ms": round(min(prep) * 1e3, 3), "median_ms": round(pm * 1e3, 3), "spread": round((max(prep) - min(prep)) / pm, 4)}
    gain = med["by_hand"] - med["new"]
    res["uses_to_repay_prepare"] = round(pm / gain, 3) if gain > 0 else None
    res["by_hand_over_new_median"] = round(med["by_hand"] / med["new"], 4)
    # the condition of the change: new's median below by_hand's by more than the larger of the two arms' spreads (max - min, in seconds)
    res["new_beats_by_hand"] = bool(gain > max(max(samples[k]) - min(samples[k]) for k in ("new", "by_hand")))
    m.close()
    del a, b, x
    torch.cuda.empty_cache()
    return res


def main():
    import torch

    out = sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "profiles", "multiply_shared_timing.json")
    res = {"device": torch.cuda.get_device_name(0), "rounds": ROUNDS, "calls_per_sample": CALLS, "shapes": [measure(*s) for s in SHAPES]}
    text = json.dumps(res)
    print(text)
    os.makedirs(os.path.dirname(os.path.abspath(out)), exist_ok=True)
    with open(out, "w") as f:
        f.write(text + "\n")
    return 0 if all(s["new_equals_by_hand"] for s in res["shapes"]) else 1


if __name__ == "__main__":
    sys.exit(main())
