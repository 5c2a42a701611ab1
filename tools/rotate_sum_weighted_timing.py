#!/usr/bin/env python3
"""tools/rotate_sum_weighted_timing.py [out.json] -- a weighted sum of 8 rotations per group in one call against the same sum by hand,
on one GPU, device-resident operands of uniform canonical residues (valid ciphertext bit patterns), SEAL's default primes, a direct
key per step.

Shapes (n, groups; terms = 8, steps 1 ... 8, distinct ciphertexts): n = 8192: 128 groups (1024 items), n = 16384: 64 groups (512 items)
-- those of tools/rotate_sum_timing.py.  The weights alternate +1 / -1, so that a sequence by hand with the same words exists.  Arms,
alternating in one process, ROUNDS samples of CALLS whole calls each:
`new` = rotate_rows_sum_weighted; `by_hand` = rotate_rows_items over the groups * terms items into a term-major staging buffer with the
positive terms first, ONE negate over the negative half of the stage, then terms - 1 add passes over contiguous slices -- entry points of
the parent alone, whose kernels are unchanged instruction for instruction (tools/isa_fingerprint.sh), so the arm runs from this build;
`unweighted` = rotate_rows_sum on the same operands: other bits, it shows what the weight costs.  new and by_hand are compared word for
word in the run.  Prints and writes (default profiles/rotate_sum_weighted_timing.json) one JSON object: per shape and arm best and median
ms and spread ((max - min) / median), HIP-event ms per kernel of one call of each arm, the ratios of the medians and whether new's median
is below by_hand's by more than the larger of the two arms' spreads.  Recorded, not gated."""
import json
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

SHAPES = [(8192, 128), (16384, 64)]
STEPS = [1, 2, 3, 4, 5, 6, 7, 8]
WEIGHTS = [1, -1, 1, -1, 1, -1, 1, -1]
ROUNDS, CALLS = 10, 3


def measure(n, groups):
    import torch

    from sunscreen_amd.batch import BatchEvaluator, to_device
    from sunscreen_amd.seal import CoefficientModulus, Context, KeyGenerator

    primes = [int(p.value()) for p in CoefficientModulus.bfv_default(n)]
    ctx = Context.from_raw(n, primes, 114689 if n == 8192 else 786433)
    gk = KeyGenerator(ctx, seed=7).create_galois_keys(steps=STEPS)
    ev = BatchEvaluator(ctx)
    K, terms = ctx.K, len(STEPS)
    rng = np.random.default_rng(n)
    host = np.empty((groups * terms, 2, K, n), dtype=np.uint64)
    for r in range(K):
        host[:, :, r, :] = rng.integers(0, primes[r], (groups * terms, 2, n), dtype=np.uint64)
    ct = to_device(host)
    del host
    out_new = torch.empty((groups, 2, K, n), dtype=ct.dtype, device=ct.device)
    out_hand = torch.empty_like(out_new)
    out_plain = torch.empty_like(out_new)
    stage = torch.empty_like(ct)

    # the by-hand arm: the items ordered term-major (item t' * groups + g), the positive terms first, so that every term is one
    # contiguous slice of the stage and the negative terms are its second half -- what a caller who controls the layout would do
    order = [t for t in range(terms) if WEIGHTS[t] > 0] + [t for t in range(terms) if WEIGHTS[t] < 0]
    npos = sum(1 for wt in WEIGHTS if wt > 0)
    tm = ct.view(groups, terms, 2, K, n)[:, order].transpose(0, 1).contiguous().view(groups * terms, 2, K, n)
    tm_steps = [STEPS[t] for t in order for _ in range(groups)]

    def by_hand():
        ev.rotate_rows_items(tm, tm_steps, gk, out=stage)
        neg = stage[npos * groups:]
        ev.negate(neg, out=neg)
        s = stage.view(terms, groups, 2, K, n)
        ev.add(s[0], s[1], out=out_hand)
        for t in range(2, terms):
            ev.add(out_hand, s[t], out=out_hand)
        return out_hand

    arms = {"new": lambda: ev.rotate_rows_sum_weighted(ct, STEPS, WEIGHTS, gk, out=out_new), "by_hand": by_hand,
            "unweighted": lambda: ev.rotate_rows_sum(ct, STEPS, gk, out=out_plain)}
    for name, fn in arms.items():  # warm-up: scratch, code objects
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
    res = {"n": n, "K": K, "groups": groups, "terms": terms, "items": groups * terms, "steps": STEPS, "weights": WEIGHTS, "new_equals_by_hand": equal,
           "kernel_ms": kernels}
    for name, ts in samples.items():
        med = statistics.median(ts)
        res[name] = {"best_ms": round(min(ts) * 1e3, 3), "median_ms": round(med * 1e3, 3), "spread": round((max(ts) - min(ts)) / med, 4),
                     "median_items_per_s": round(groups * terms / med, 1)}
    med = {name: statistics.median(ts) for name, ts in samples.items()}
    res["by_hand_over_new_median"] = round(med["by_hand"] / med["new"], 4)
    res["new_over_unweighted_median"] = round(med["new"] / med["unweighted"], 4)
    pair = [samples["new"], samples["by_hand"]]
    res["larger_spread_ms"] = round(max(max(ts) - min(ts) for ts in pair) * 1e3, 3)
    res["new_beats_by_hand"] = bool(med["by_hand"] - med["new"] > max(max(ts) - min(ts) for ts in pair))
    del ct, tm, stage
    torch.cuda.empty_cache()
    return res


def main():
    import torch

    if not torch.cuda.is_available():
        sys.exit("rotate_sum_weighted_timing.py needs a GPU")
    out = sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "profiles", "rotate_sum_weighted_timing.json")
    res = {"device": torch.cuda.get_device_name(0), "rounds": ROUNDS, "calls_per_sample": CALLS, "shapes": [measure(*s) for s in SHAPES]}
    text = json.dumps(res)
    print(text)
    os.makedirs(os.path.dirname(os.path.abspath(out)), exist_ok=True)
    with open(out, "w") as f:
        f.write(text + "\n")
    return 0 if all(s["new_equals_by_hand"] for s in res["shapes"]) else 1


if __name__ == "__main__":
    sys.exit(main())
