#!/usr/bin/env python3
"""tools/multiply_prepared_timing.py [out.json] -- the ciphertext matrix product C = A B over two prepared operands against the best the
*_shared calls offer, on one GPU, device-resident operands of uniform canonical residues (valid ciphertext bit patterns), SEAL's default
primes.

Shapes (n, A m x k, B k x cols; groups = m * cols, terms = k): n = 8192: 32 x 8 times 8 x 16 (512 groups x 8 terms), n = 16384: 16 x 8
times 8 x 8 (128 x 8) -- the item counts of tools/multiply_shared_timing.py -- and per degree one shape with 4 times as many distinct
ciphertexts in A and in B at the same item count (8 x 128 times 128 x 4, 4 x 128 times 128 x 2): what happens when the prepared rows
stop fitting in L2.  Arms, alternating in one process, ROUNDS samples of CALLS whole calls each, every prepare() outside the timed region:
`new` = multiply_sum_relin_prepared; `by_hand` = multiply_sum_relin_shared with B prepared and A replicated into a[g][t] outside the
timed region (the same words, compared in the run).  Prints and writes (default profiles/multiply_prepared_timing.json) one JSON object:
per shape and arm best and median ms and spread ((max - min) / median), HIP-event ms per kernel of one call of each arm, the bytes the
objects and the replicated operand hold, and the condition: new's median below by_hand's by more than the larger of the two arms' spreads."""
import json
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

# (n, m, k, cols, the condition applies): the last two have 4 x the distinct ciphertexts of the first two at the same item count
SHAPES = [(8192, 32, 8, 16, True), (16384, 16, 8, 8, True), (8192, 8, 128, 4, False), (16384, 4, 128, 2, False)]
ROUNDS, CALLS = 10, 3


def measure(n, m, k, cols, conditioned):
    import torch

    from sunscreen_amd.batch import BatchEvaluator, to_device
    from sunscreen_amd.seal import CoefficientModulus, Context, KeyGenerator
    from sunscreen_amd.workloads import matrix_product_index

    primes = [int(p.value()) for p in CoefficientModulus.bfv_default(n)]
    ctx = Context.from_raw(n, primes, 114689)
    rk = KeyGenerator(ctx, seed=n).create_relinearization_keys()
    ev = BatchEvaluator(ctx)
    K = ctx.K
    rng = np.random.default_rng(n + m)
    groups, terms = m * cols, k
    a_index, b_index = matrix_product_index(m, k, cols)

    def operand(items):
        host = np.empty((items, 2, K, n), dtype=np.uint64)
        for r in range(K):
            host[:, :, r, :] = rng.integers(0, primes[r], (items, 2, n), dtype=np.uint64)
        return to_device(host)

    A, B = operand(m * k), operand(k * cols)
    ma, mb = ev.prepare(A), ev.prepare(B)
    a_rep = A.index_select(0, torch.tensor(a_index, dtype=torch.int64, device=A.device)).view(groups, terms, 2, K, n).contiguous()
    out_new = torch.empty((groups, 2, K, n), dtype=A.dtype, device=A.device)
    out_hand = torch.empty_like(out_new)
    arms = {"new": lambda: ev.multiply_sum_relin_prepared(ma, a_index, mb, b_index, rk, groups, terms, out=out_new),
            "by_hand": lambda: ev.multiply_sum_relin_shared(a_rep, mb, b_index, rk, out=out_hand)}
    for fn in arms.values():  # warm-up: scratch, code objects
        fn()
        fn()
    torch.cuda.synchronize()
    equal = bool(torch.equal(out_new, out_hand))
    samples = {name: [] for name in arms}
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
    for name, fn in arms.items():
        ev.profile_reset()
        fn()
        torch.cuda.synchronize()
        kernels[name] = {kind: round(v["ms"], 3) for kind, v in ev.profile_read().items()}
    ev.profile(False)
    res = {"n": n, "K": K, "A": [m, k], "B": [k, cols], "groups": groups, "terms": terms, "items": groups * terms, "distinct": m * k + k * cols,
           "condition_applies": conditioned, "prepared_bytes": ma.nbytes + mb.nbytes, "replicated_a_bytes": a_rep.numel() * 8,
           "new_equals_by_hand": equal, "kernel_ms": kernels}
    for name, ts in samples.items():
        med = statistics.median(ts)
        res[name] = {"best_ms": round(min(ts) * 1e3, 3), "median_ms": round(med * 1e3, 3), "spread": round((max(ts) - min(ts)) / med, 4),
                     "median_items_per_s": round(groups * terms / med, 1)}
    med = {name: statistics.median(ts) for name, ts in samples.items()}
    res["by_hand_over_new_median"] = round(med["by_hand"] / med["new"], 4)
    # the condition of the change: new's median below by_hand's by more than the larger of the two arms' spreads (max - min, in seconds)
    res["new_beats_by_hand"] = bool(med["by_hand"] - med["new"] > max(max(ts) - min(ts) for ts in samples.values()))
    ma.close()
    mb.close()
    del A, B, a_rep
    torch.cuda.empty_cache()
    return res


def main():
    import torch

    if not torch.cuda.is_available():
        sys.exit("multiply_prepared_timing.py needs a GPU")
    out = sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "profiles", "multiply_prepared_timing.json")
    res = {"device": torch.cuda.get_device_name(0), "rounds": ROUNDS, "calls_per_sample": CALLS, "shapes": [measure(*s) for s in SHAPES]}
    text = json.dumps(res)
    print(text)
    os.makedirs(os.path.dirname(os.path.abspath(out)), exist_ok=True)
    with open(out, "w") as f:
        f.write(text + "\n")
    return 0 if all(s["new_equals_by_hand"] for s in res["shapes"]) else 1


if __name__ == "__main__":
    sys.exit(main())
