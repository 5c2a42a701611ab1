#!/usr/bin/env python3
"""tools/rotate_items_timing.py -- what a mixed-step rotation batch costs beside the uniform call (hipbfv_batch_rotate_rows_items
against hipbfv_batch_rotate_rows), device-resident batches on one GPU.

Arms, at n = 8192 (batch 4096) and n = 16384 (batch 1024), alternating in one process, best of 5 whole calls each:
  a  rotate_rows with one step                        -- the yardstick: the uniform launch sequence, a scalar automorphism
  b  rotate_rows_items with that step for every item  -- the same work through the per-item table and the per-item key path
  c  rotate_rows_items with 8 distinct direct steps, interleaved item by item -- one launch sequence
  d  what a caller does for (c) without the entry point: per step, gather the step's items (index_select), one uniform call,
     scatter the results (index_copy_) -- eight launch sequences, gathers and scatters counted
Every step has its own key (no NAF chains).  Operands are uniform canonical residues: valid ciphertext bit patterns.  Also
checks (c) against (d) word for word.  Prints one JSON object (the shader clock is sampled while arm (c) keeps running)."""
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

REPS = 5
STEPS = [1, -1, 2, -2, 4, -4, 8, -8]


def arms(n, batch):
    import torch

    from sunscreen_amd.batch import BatchEvaluator, to_device
    from sunscreen_amd.seal import CoefficientModulus, Context, KeyGenerator

    primes = [int(m.value()) for m in CoefficientModulus.bfv_default(n)]
    ctx = Context.from_raw(n, primes, 114689 if n == 8192 else 786433)
    gk = KeyGenerator(ctx, seed=7).create_galois_keys(steps=STEPS)
    ev = BatchEvaluator(ctx)
    K = ctx.K
    rng = np.random.default_rng(n)
    host = np.empty((batch, 2, K, n), dtype=np.uint64)
    for k in range(K):
        host[:, :, k, :] = rng.integers(0, primes[k], (batch, 2, n), dtype=np.uint64)
    ct = to_device(host)
    del host
    out = torch.empty_like(ct)
    same = np.full(batch, STEPS[0], dtype=np.int32)
    mixed = np.array([STEPS[i % len(STEPS)] for i in range(batch)], dtype=np.int32)
    index = [torch.arange(j, batch, len(STEPS), device=ct.device) for j in range(len(STEPS))]
    stage_in = torch.empty((index[0].numel(),) + tuple(ct.shape[1:]), dtype=ct.dtype, device=ct.device)
    stage_out = torch.empty_like(stage_in)
    out_d = torch.empty_like(ct)

    def arm_d():
        for j, step in enumerate(STEPS):
            c = index[j].numel()
            torch.index_select(ct, 0, index[j], out=stage_in[:c])
            ev.rotate_rows(stage_in[:c], step, gk, out=stage_out[:c])
            out_d.index_copy_(0, index[j], stage_out[:c])

    calls = {
        "a_uniform": lambda: ev.rotate_rows(ct, STEPS[0], gk, out=out),
        "b_items_one_step": lambda: ev.rotate_rows_items(ct, same, gk, out=out),
        "c_items_8_steps": lambda: ev.rotate_rows_items(ct, mixed, gk, out=out),
        "d_8_uniform_calls": arm_d,
    }
    best = {k: float("inf") for k in calls}
    for fn in calls.values():  # warm-up: scratch, staging blocks
        fn()
    torch.cuda.synchronize()
    for _ in range(REPS):
        for name, fn in calls.items():
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            fn()
            torch.cuda.synchronize()
            best[name] = min(best[name], time.perf_counter() - t0)
    calls["c_items_8_steps"]()
    arm_d()
    torch.cuda.synchronize()
    equal = bool(torch.equal(out, out_d))
    ev.check()
    from bench import power_leg

    power = power_leg(calls["c_items_8_steps"], torch.cuda.synchronize)
    res = {"n": n, "batch": batch, "K": K, "steps": STEPS, "c_equals_d": equal, "power": power}
    for name, t in best.items():
        res[name + "_rot_per_s"] = round(batch / t, 1)
        res[name + "_ms"] = round(t * 1e3, 3)
    res["b_over_a"] = round(best["a_uniform"] / best["b_items_one_step"], 4)
    res["c_over_d"] = round(best["d_8_uniform_calls"] / best["c_items_8_steps"], 4)
    del ct, out, out_d, stage_in, stage_out
    torch.cuda.empty_cache()
    return res


def main():
    import torch

    result = {"device": torch.cuda.get_device_name(0), "reps": REPS, "runs": [arms(8192, 4096), arms(16384, 1024)]}
    print(json.dumps(result))
    return 0 if all(r["c_equals_d"] for r in result["runs"]) else 1


if __name__ == "__main__":
    sys.exit(main())
