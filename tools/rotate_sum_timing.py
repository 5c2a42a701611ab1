#!/usr/bin/env python3
"""tools/rotate_sum_timing.py [out.json] -- a sum of 8 rotations per group in one call against the same sum by hand, on one GPU,
device-resident operands of uniform canonical residues (valid ciphertext bit patterns), SEAL's default primes, a direct key per step.

Shapes (n, groups; terms = 8, steps 1 ... 8, distinct ciphertexts): n = 8192: 128 groups (1024 items), n = 16384: 64 groups (512 items)
-- the item counts of tools/rotate_items_timing.py.  Arms, alternating in one process, ROUNDS samples of CALLS whole calls each:
`new` = rotate_rows_sum; `by_hand` = rotate_rows_items over the groups * terms items into a staging buffer, then terms - 1 add passes
over the groups, with the items ordered term-major so that every add reads contiguous slices of the stage (the best a caller who
controls the layout can do; the ratio is taken against this arm); `by_hand_item_major` = the same with the call's own item order,
where every term is compacted before its add.  The by-hand arm's kernels are the parent's, instruction for
instruction (tools/isa_fingerprint.sh), so it runs from this build.  The two results are compared word for word in the run.  Prints
and writes (default profiles/rotate_sum_timing.json) one JSON object: per shape and arm best and median ms and spread ((max - min) /
median), HIP-event ms per kernel of one call of each arm, the ratio of the medians and whether new's median is below by_hand's by more
than the larger of the two arms' spreads.  Recorded, not gated."""
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
    stage = torch.empty_like(ct)
    item_steps = STEPS * groups

    def by_hand():
        ev.rotate_rows_items(ct, item_steps, gk, out=stage)
        s = stage.view(groups, terms, 2, K, n)
        # (a term's items are `terms` ciphertexts apart: the add reads contiguous buffers, so term t is compacted first -- the
        # copy a caller of the batch interface pays too, unless the staging layout is term-major; both are timed below)
        ev.add(s[:, 0].contiguous(), s[:, 1].contiguous(), out=out_hand)
        for t in range(2, terms):
            ev.add(out_hand, s[:, t].contiguous(), out=out_hand)
        return out_hand

    # the by-hand arm without the compaction copies: the items ordered term-major (item t * groups + g), so that term t is one
    # contiguous slice of the stage -- what a caller who controls the layout would do
    tm = ct.view(groups, terms, 2, K, n).transpose(0, 1).contiguous().view(groups * terms, 2, K, n)
    tm_steps = [s for s in STEPS for _ in range(groups)]

    def by_hand_term_major():
        ev.rotate_rows_items(tm, tm_steps, gk, out=stage)
        s = stage.view(terms, groups, 2, K, n)
        ev.add(s[0], s[1], out=out_hand)
        for t in range(2, terms):
            ev.add(out_hand, s[t], out=out_hand)
        return out_hand

    arms = {"new": lambda: ev.rotate_rows_sum(ct, STEPS, gk, out=out_new), "by_hand": by_hand_term_major, "by_hand_item_major": by_hand}
    equal = {}
    for name, fn in arms.items():  # warm-up: scratch, code objects
        fn()
        fn()
        torch.cuda.synchronize()
        if name != "new":
            equal[name] = bool(torch.equal(out_new, out_hand))
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
    res = {"n": n, "K": K, "groups": groups, "terms": terms, "items": groups * terms, "steps": STEPS, "new_equals": equal, "kernel_ms": kernels}
    for name, ts in samples.items():
        med = statistics.median(ts)
        res[name] = {"best_ms": round(min(ts) * 1e3, 3), "median_ms": round(med * 1e3, 3), "spread": round((max(ts) - min(ts)) / med, 4),
                     "median_items_per_s": round(groups * terms / med, 1)}
    med = {name: statistics.median(ts) for name, ts in samples.items()}
    res["by_hand_over_new_median"] = round(med["by_hand"] / med["new"], 4)
    pair = [samples["new"], samples["by_hand"]]
    res["larger_spread_ms"] = round(max(max(ts) - min(ts) for ts in pair) * 1e3, 3)
    res["new_beats_by_hand"] = bool(med["by_hand"] - med["new"] > max(max(ts) - min(ts) for ts in pair))
    del ct, tm, stage
    torch.cuda.empty_cache()
    return res


def main():
    import torch

    if not torch.cuda.is_available():
        sys.exit("rotate_sum_timing.py needs a GPU")
    out = sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "profiles", "rotate_sum_timing.json")
    res = {"device": torch.cuda.get_device_name(0), "rounds": ROUNDS, "calls_per_sample": CALLS, "shapes": [measure(*s) for s in SHAPES]}
    text = json.dumps(res)
    print(text)
    os.makedirs(os.path.dirname(os.path.abspath(out)), exist_ok=True)
    with open(out, "w") as f:
        f.write(text + "\n")
    return 0 if all(all(s["new_equals"].values()) for s in res["shapes"]) else 1


if __name__ == "__main__":
    sys.exit(main())
