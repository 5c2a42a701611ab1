#!/usr/bin/env python3
"""tools/rotate_items_keys_timing.py -- a multi-tenant rotation queue in one call (hipbfv_batch_rotate_rows_items_keys) against the
best the per-key API offers without it: one hipbfv_batch_rotate_rows_keys call per distinct step over gathered items.

1024 items at n = 8192, device-resident, on one GPU: 64 clients x 8 distinct steps, every (client, step) pair twice, shuffled.
Every client holds the keys of 1, -1, 2, -2, 4, -4, 8 and 16, so the steps 1, -1, 2, 4 rotate through their own key and the steps
3 = [-1, 4], 5 = [1, 4], 6 = [-2, 8], 12 = [-4, 16] walk two-hop NAF chains: half of the items take chains.

Arms, alternating in one process, ROUNDS samples of CALLS whole calls each:
  new   one rotate_rows_items_keys call: one launch sequence for the 512 direct items, two shared rounds for the 512 chain items
  old   per distinct step: gather the step's items and their key_index (index_select), one rotate_rows_keys call (which decides
        per set and runs the chain in place), scatter the results (index_copy_) -- eight calls, gathers and scatters counted
Operands are uniform canonical residues: valid ciphertext bit patterns.  Checks the two arms against each other word for word.
Prints one JSON object: per arm the best and the median rate, and the run-to-run spread ((max - min) / median of its samples)."""
import json
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

N, CLIENTS, BATCH = 8192, 64, 1024
ROUNDS, CALLS = 10, 4
DIRECT, CHAIN = [1, -1, 2, 4], [3, 5, 6, 12]
HELD = [1, -1, 2, -2, 4, -4, 8, 16]


def main():
    import torch

    from sunscreen_amd.batch import BatchEvaluator, to_device
    from sunscreen_amd.seal import CoefficientModulus, Context, KeyGenerator

    primes = [int(m.value()) for m in CoefficientModulus.bfv_default(N)]
    ctx = Context.from_raw(N, primes, 114689)
    sets = [KeyGenerator(ctx, seed=100 + k).create_galois_keys(steps=HELD) for k in range(CLIENTS)]
    ev = BatchEvaluator(ctx)
    K = ctx.K
    rng = np.random.default_rng(N)
    host = np.empty((BATCH, 2, K, N), dtype=np.uint64)
    for k in range(K):
        host[:, :, k, :] = rng.integers(0, primes[k], (BATCH, 2, N), dtype=np.uint64)
    ct = to_device(host)
    del host
    steps_all = DIRECT + CHAIN
    pairs = [(c, s) for c in range(CLIENTS) for s in steps_all] * (BATCH // (CLIENTS * len(steps_all)))
    assert len(pairs) == BATCH
    order = rng.permutation(BATCH)
    key_index = np.array([pairs[p][0] for p in order], dtype=np.uint32)
    steps = np.array([pairs[p][1] for p in order], dtype=np.int32)
    out_new, out_old = torch.empty_like(ct), torch.empty_like(ct)
    index = {s: torch.from_numpy(np.nonzero(steps == s)[0]).to(ct.device) for s in steps_all}
    kidx = {s: np.ascontiguousarray(key_index[steps == s]) for s in steps_all}
    per = max(v.numel() for v in index.values())
    stage_in = torch.empty((per,) + tuple(ct.shape[1:]), dtype=ct.dtype, device=ct.device)
    stage_out = torch.empty_like(stage_in)

    def arm_new():
        ev.rotate_rows_items_keys(ct, steps, sets, key_index, out=out_new)

    def arm_old():
        for s in steps_all:
            c = index[s].numel()
            torch.index_select(ct, 0, index[s], out=stage_in[:c])
            ev.rotate_rows_keys(stage_in[:c], s, sets, kidx[s], out=stage_out[:c])
            out_old.index_copy_(0, index[s], stage_out[:c])

    arms = {"new_one_call": arm_new, "old_call_per_step": arm_old}
    for fn in arms.values():  # warm-up: scratch, staging blocks, code objects
        fn()
        fn()
    torch.cuda.synchronize()
    equal = bool(torch.equal(out_new, out_old))
    ev.check()
    samples = {k: [] for k in arms}
    for _ in range(ROUNDS):
        for name, fn in arms.items():
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for _ in range(CALLS):
                fn()
            torch.cuda.synchronize()
            samples[name].append((time.perf_counter() - t0) / CALLS)
    res = {"device": torch.cuda.get_device_name(0), "n": N, "K": K, "batch": BATCH, "clients": CLIENTS, "direct_steps": DIRECT, "chain_steps": CHAIN,
           "rounds": ROUNDS, "calls_per_sample": CALLS, "new_equals_old": equal}
    for name, ts in samples.items():
        med = statistics.median(ts)
        res[name] = {"best_ms": round(min(ts) * 1e3, 3), "median_ms": round(med * 1e3, 3), "best_rot_per_s": round(BATCH / min(ts), 1),
                     "median_rot_per_s": round(BATCH / med, 1), "spread": round((max(ts) - min(ts)) / med, 4)}
    res["new_over_old_median"] = round(statistics.median(samples["old_call_per_step"]) / statistics.median(samples["new_one_call"]), 4)
    print(json.dumps(res))
    return 0 if equal else 1


if __name__ == "__main__":
    sys.exit(main())
