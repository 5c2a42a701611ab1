#!/usr/bin/env python3
"""tools/dot_plain_queries_timing.py [out.json] [--only-q Q] [--no-tiles] -- Q queries against one transformed database: one call of
hipbfv_batch_dot_plain_ntt_queries against Q calls of hipbfv_batch_dot_plain_ntt, on one GPU, device-resident operands of uniform
canonical residues, SEAL's default primes.

Shapes: n = 8192 (K = 4) with 256 x 256 entries and n = 16384 (K = 8) with 128 x 128: both databases are 16 GiB in the transform
domain, far beyond the Infinity Cache.  Q = 1, 2, 4, 8, 16.  Arms, alternating in one process, ROUNDS samples each, timed with device
events over a window of `reps` repetitions (reps * Q single-query calls, or reps calls of the new entry point):
  per_query   Q calls of dot_plain_ntt, one per query (the parent's way, its kernels unchanged);
  one_call    one call of dot_plain_ntt_queries on the same operands, the library's default tile;
  tile_RxQ    the same under HIPBFV_DOT_QUERIES_TILE=RxQ, for every other compiled tile (the candidates the default was chosen from).
The outputs of all arms are compared before anything is timed.  Prints and writes (default profiles/dot_plain_queries_timing.json) one
JSON object: per shape, Q and arm the median and best ms per repetition, the spread (max - min, ms), entries * queries per second;
the shader clock and package power rocm-smi reports while the new call runs; the tile in use; and the condition of the change:
`one_call` faster than `per_query` by more than the larger of the two spreads."""
import json
import os
import statistics
import sys


ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

SHAPES = [(8192, 256, 256), (16384, 128, 128)]  # (n, rows, cols)
QUERIES = [1, 2, 4, 8, 16]
ROUNDS = 5
TILES = ["2x2", "1x4", "1x2"]  # <RT>x<QT>: evaluator.hpp kDotQueriesTiles


def uniform(torch, shape, primes, n):
    """int64[*shape, K, n] on the device: residue row k uniform below primes[k]."""
    out = torch.empty(tuple(shape) + (len(primes), n), dtype=torch.int64, device="cuda")
    for k, p in enumerate(primes):
        out[..., k, :].copy_(torch.randint(0, int(p), tuple(shape) + (n,), dtype=torch.int64, device="cuda"))
    return out


def measure(n, rows, cols, queries, tiles):
    import torch

    import bench
    from sunscreen_amd.batch import BatchEvaluator, dot_queries_plan
    from sunscreen_amd.seal import CoefficientModulus, Context

    primes = [int(m.value()) for m in CoefficientModulus.bfv_default(n)]
    ctx = Context.from_raw(n, primes, 114689)
    ev = BatchEvaluator(ctx)
    K = ctx.K
    torch.manual_seed(n)
    db = torch.empty((rows, cols, K, n), dtype=torch.int64, device="cuda")
    for r0 in range(0, rows, 16):
        db[r0:r0 + 16] = uniform(torch, (min(16, rows - r0), cols), primes[:K], n)
    ctn_all = uniform(torch, (max(queries), cols, 2), primes[:K], n)
    os.environ.pop("HIPBFV_DOT_QUERIES_TILE", None)
    default = "%dx%d" % tuple(reversed(dot_queries_plan(2, rows, K)[0][4:6]))
    res = {"n": n, "K": K, "rows": rows, "cols": cols, "database_bytes": db.numel() * 8, "default_tile_RTxQT": default, "by_queries": []}
    for Q in queries:
        ctn = ctn_all[:Q].contiguous()
        reps = max(2, 16 // Q)

        def per_query():
            return [ev.dot_plain_ntt(ctn[q], db) for q in range(Q)]

        def tiled(tile):
            def run():
                if tile is None:
                    os.environ.pop("HIPBFV_DOT_QUERIES_TILE", None)
                else:
                    os.environ["HIPBFV_DOT_QUERIES_TILE"] = tile
                try:
                    return ev.dot_plain_ntt_queries(ctn, db)
                finally:
                    os.environ.pop("HIPBFV_DOT_QUERIES_TILE", None)
            return run

        arms = {"per_query": per_query, "one_call": tiled(None)}
        for t in tiles:
            if t != default:
                arms["tile_" + t] = tiled(t)
        want = torch.stack(per_query())  # (also the warm-up)
        equal = {}
        for name, fn in arms.items():
            if name != "per_query":
                fn()
                equal[name] = bool(torch.equal(fn(), want))
        del want
        torch.cuda.synchronize()
        samples = {k: [] for k in arms}
        for _ in range(ROUNDS):
            for name, fn in arms.items():
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                torch.cuda.synchronize()
                e0.record()
                for _ in range(reps):
                    fn()
                e1.record()
                e1.synchronize()
                samples[name].append(e0.elapsed_time(e1) / reps)
        ev.profile(True)
        kernels = {}
        for name in ("per_query", "one_call"):
            ev.profile_reset()
            arms[name]()
            torch.cuda.synchronize()
            kernels[name] = {k: {"ms": round(v["ms"], 3), "launches": v["launches"]} for k, v in ev.profile_read().items()}
        ev.profile(False)
        entry = {"queries": Q, "reps_per_sample": reps, "plan": dot_queries_plan(Q, rows, K), "equal_to_per_query": equal, "kernel_ms": kernels}
        for name, ts in samples.items():
            med = statistics.median(ts)
            entry[name] = {"median_ms": round(med, 4), "best_ms": round(min(ts), 4), "spread_ms": round(max(ts) - min(ts), 4),
                           "entries_queries_per_s": round(rows * cols * Q / (med * 1e-3), 1)}
        a, b = samples["per_query"], samples["one_call"]
        gain = statistics.median(a) - statistics.median(b)
        spread = max(max(a) - min(a), max(b) - min(b))
        entry["per_query_over_one_call_median"] = round(statistics.median(a) / statistics.median(b), 4)
        entry["one_call_faster_beyond_spread"] = bool(gain > spread)
        entry["one_call_not_slower_beyond_spread"] = bool(-gain <= spread)
        if Q == 8 and len(queries) > 1:  # (not in a profiler's single-Q run: the sampler starts rocm-smi as a child)
            entry["power_and_clock_one_call"] = bench.power_leg(arms["one_call"], torch.cuda.synchronize)
        res["by_queries"].append(entry)
        print(json.dumps(entry), file=sys.stderr, flush=True)
    del db, ctn_all
    torch.cuda.empty_cache()
    return res


def main():
    import torch

    import argparse

    ap = argparse.ArgumentParser()
    ap.add_argument("out", nargs="?", default=os.path.join(ROOT, "profiles", "dot_plain_queries_timing.json"))
    ap.add_argument("--only-q", type=int, default=0, help="one Q (for a profiler run of the new call: --only-q 8 --no-tiles /dev/null)")
    ap.add_argument("--no-tiles", action="store_true", help="leave the other compiled tiles out")
    a = ap.parse_args()
    out, queries, tiles = a.out, ([a.only_q] if a.only_q else QUERIES), ([] if a.no_tiles else TILES)
    shapes = [measure(n, rows, cols, queries, tiles) for n, rows, cols in SHAPES]
    ok = all(all(e["equal_to_per_query"].values()) for s in shapes for e in s["by_queries"])
    res = {"device": torch.cuda.get_device_name(0), "rounds": ROUNDS, "timer": "device events around a window of reps_per_sample repetitions",
           "all_outputs_equal": ok, "shapes": shapes}
    text = json.dumps(res)
    print(text)
    if out != os.devnull:
        os.makedirs(os.path.dirname(os.path.abspath(out)), exist_ok=True)
    with open(out, "w") as f:
        f.write(text + "\n")
    return 0 if ok else 1


if __name__ == "__main__":
    sys.exit(main())
