#!/usr/bin/env python3
"""tools/noise_budget_timing.py -- what the invariant-noise measure costs on the GPU box (reported, not asserted).

  batched:      BatchEvaluator.noise_budget over 1024 fresh ciphertexts at n = 16384 and 4096 at n = 8192, and the extra time of
                decrypt_checked over decrypt on the same batch (median of --reps timed runs after a warm-up, stream synchronised);
  handle level: the same number of Decryptor_InvariantNoiseBudget calls, one ciphertext per call (8 distinct ciphertexts in turn).

--handle-only measures the handle-level calls alone: with HIPBFV_LIB=<a library of an older tree> and HIPBFV_LIB_ALLOW_MISSING=1
that is the "before" column (the batched entry points do not exist there).  Prints one JSON object per parameter set."""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--handle-only", action="store_true")
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--sets", default="16384:1024,8192:4096", help="n:count,...")
    args = ap.parse_args()

    import torch
    from oracle import bfv_oracle as O
    from sunscreen_amd import Ciphertext, Context, Decryptor, PublicKey, SecretKey
    from sunscreen_amd.batch import BatchEvaluator, to_device, to_host

    for spec in args.sets.split(","):
        n, count = (int(x) for x in spec.split(":"))
        primes, t = O.bfv_default(n), O.plain_batching(n, 17)
        o = O.Oracle(n, primes, t)
        O.seed(7)
        sk, pk, _, _ = o.keygen(relin=False)
        ctx = Context.from_raw(n, primes, t)
        ev = BatchEvaluator(ctx)
        skd, pkd = SecretKey.from_array(ctx, sk), PublicKey.from_array(ctx, pk)
        rng = np.random.default_rng(1)
        ct = ev.encrypt(to_device(rng.integers(0, t, (count, n), dtype=np.uint64)), pkd, seed=99)
        torch.cuda.synchronize()
        res = {"n": n, "K": ctx.K, "count": count, "device": torch.cuda.get_device_name(0), "lib": "HIPBFV_LIB" if os.environ.get("HIPBFV_LIB") else "tree"}

        def timed(f):
            f()
            torch.cuda.synchronize()
            ms = []
            for _ in range(args.reps):
                t0 = time.perf_counter()
                f()
                torch.cuda.synchronize()
                ms.append((time.perf_counter() - t0) * 1e3)
            return round(statistics.median(ms), 3)

        if not args.handle_only:
            res["noise_budget_ms"] = timed(lambda: ev.noise_budget(ct, skd))
            res["noise_budget_with_noise_ms"] = timed(lambda: ev.noise_budget(ct, skd, with_noise=True))
            res["decrypt_ms"] = timed(lambda: ev.decrypt(ct, skd))
            res["decrypt_checked_ms"] = timed(lambda: ev.decrypt_checked(ct, skd))
            res["decrypt_checked_extra_ms"] = round(res["decrypt_checked_ms"] - res["decrypt_ms"], 3)
            res["noise_budget_us_per_ct"] = round(res["noise_budget_ms"] * 1e3 / count, 3)
        host = to_host(ct[:8])
        d = Decryptor(ctx, skd)
        cts = [Ciphertext.from_array(ctx, host[i]) for i in range(8)]
        budgets = [d.invariant_noise_budget(c) for c in cts]  # warm-up
        t0 = time.perf_counter()
        for i in range(count):
            d.invariant_noise_budget(cts[i % 8])
        res["handle_calls"] = count
        res["handle_total_ms"] = round((time.perf_counter() - t0) * 1e3, 3)
        res["handle_ms_per_call"] = round(res["handle_total_ms"] / count, 4)
        res["handle_budgets"] = budgets
        if not args.handle_only:
            batch = ev.noise_budget(ct[:8].contiguous(), skd).cpu().tolist()
            res["batch_matches_handle"] = batch == budgets
        print(json.dumps(res), flush=True)
        del ct
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
