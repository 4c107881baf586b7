#!/usr/bin/env python3
"""Timings of batched pinned sweeps (DESIGN.md §4 "Batched pinned sweeps";
results under profiles/batch/).

Workload: synthetic R = 64, n = 7, m = 5, objectives [MEAN af1, MEAN ff1],
K = 100; the bases are the first `--sets` records of the n = 5 sweep.  One
process, warm, median of `--reps` with min .. max, one JSON line:

  batch_wall_ms   launch -> result of the batch
  loop_wall_ms    the same sets as single pinned sweeps (handles created
                  beforehand), launch -> result each, one after the other
  batch_kernel_ms the batch kernel's event time; per config = / (sets * 1,711)
  unpinned_kernel_ms  sweep_fast_kernel<7> (forced fast, unpinned) over a rank
                  range of the same total size
  lane_utilisation    configs of a set / lane slots of its unit's pass
  scored_kernel_ms    the batch kernel over the same sets with [SCORE, MEAN af1,
                  MEAN ff1] and the default ranking (validity is computed)
  bounded_kernel_ms   the same as a bounded batch (prev_sums: the bases' Atlas
                  sums, DESIGN.md §4 "Streaming evolving search"); null on a
                  library without bote_batch_create_bounded (BOTE_LIB_PATH)
  scored_valid, bounded_valid  valid configs over all sets

The two paths' results are compared before anything is timed.

  python scripts/batch_timing.py [--sets 100] [--reps 7] [--warmup 2] [--max-blocks 0]
"""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from fantoch_amd import _lib  # noqa: E402
from fantoch_amd.bote import DEFAULT_RANKING, DevicePlanet, PinnedBatch, Sweep, eval_configs  # noqa: E402
from fantoch_amd.planet import Planet  # noqa: E402


def med(xs):
    return {"median": round(statistics.median(xs), 4), "min": round(min(xs), 4), "max": round(max(xs), 4)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sets", type=int, default=100)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--max-blocks", type=int, default=0)
    args = ap.parse_args()

    p = Planet.synthetic(64)
    dp = DevicePlanet(p)
    srv = np.arange(64, dtype=np.uint32)
    objs = [(_lib.OBJ_MEAN, 0), (_lib.OBJ_MEAN, 1)]
    kw = dict(K=100, ranking=None, digest=False)
    base = Sweep(dp, srv, srv, 5, objs, **kw)
    base.launch()
    recs = base.result().tops[0][:args.sets]
    batch = PinnedBatch.from_records(base, recs, 7, max_blocks=args.max_blocks)
    sets = batch.pinned_sets.tolist()
    singles = [Sweep(dp, srv, srv, 7, objs, pinned=s, **kw) for s in sets]

    def run_batch():
        batch.launch()
        return batch.result()

    def run_loop():
        out = []
        for sw in singles:
            sw.launch()
            out.append(sw.result())
        return out

    a, b = run_batch(), run_loop()
    assert [r.tops for r in a] == [r.tops for r in b], "batch and single sweeps differ"
    walls = {"batch": [], "loop": []}
    kms = []
    for i in range(args.warmup + args.reps):
        for name, fn in (("batch", run_batch), ("loop", run_loop)):
            t0 = time.perf_counter()
            fn()
            dt = (time.perf_counter() - t0) * 1e3
            if i >= args.warmup:
                walls[name].append(dt)
        if i >= args.warmup:
            kms.append(batch.kernel_ms())
    loop_kernel = [sum(sw.kernel_ms() for sw in singles)]
    per_set = batch.total
    configs = per_set * len(sets)
    un = Sweep(dp, srv, srv, 7, objs, kernel="fast", **kw)
    ums = []
    for i in range(args.warmup + args.reps):
        un.launch(0, configs)
        un.result()
        if i >= args.warmup:
            ums.append(un.kernel_ms())
    # the scored batch, and the bounded one beside it (alternating)
    sobjs = [(_lib.OBJ_SCORE, 0)] + objs
    skw = dict(K=100, ranking=DEFAULT_RANKING, digest=False, max_blocks=args.max_blocks)
    scored = PinnedBatch(dp, srv, srv, 7, sets, sobjs, **skw)
    bounded = None
    if hasattr(_lib.lib(), "bote_batch_create_bounded"):
        prev = eval_configs(dp, srv, srv, 5, configs=np.asarray(sets, dtype=np.uint32), values=False).s1[:, [0, 2]]
        bounded = PinnedBatch(dp, srv, srv, 7, sets, sobjs, prev_sums=prev, **skw)
    sms, bms, svalid, bvalid = [], [], None, None
    for i in range(args.warmup + args.reps):
        scored.launch()
        svalid = sum(r.valid for r in scored.result())
        if i >= args.warmup:
            sms.append(scored.kernel_ms())
        if bounded is not None:
            bounded.launch()
            bvalid = sum(r.valid for r in bounded.result())
            if i >= args.warmup:
                bms.append(bounded.kernel_ms())
    slices, units, grid = batch.plan()
    runlen = max(1, min(32, -(-(-(-per_set // slices)) // 256)))
    slots = -(-(-(-per_set // slices)) // (runlen * 256)) * runlen * 256 * slices
    doc = {"sets": len(sets), "configs_per_set": per_set, "configs": configs, "path": batch.kernel_path(),
           "slices": slices, "units": units, "grid": grid, "deferred": batch.deferred(),
           "batch_wall_ms": med(walls["batch"]), "loop_wall_ms": med(walls["loop"]),
           "ratio_loop_min_over_batch_median": round(min(walls["loop"]) / statistics.median(walls["batch"]), 2),
           "batch_below_loop_min": statistics.median(walls["batch"]) < min(walls["loop"]),
           "batch_kernel_ms": med(kms), "loop_kernel_ms_sum": round(loop_kernel[0], 4),
           "batch_ns_per_config": round(statistics.median(kms) * 1e6 / configs, 3),
           "unpinned_kernel_ms": med(ums), "unpinned_ns_per_config": round(statistics.median(ums) * 1e6 / configs, 3),
           "lane_utilisation": round(per_set / slots, 4), "runlen": runlen,
           "scored_kernel_ms": med(sms), "bounded_kernel_ms": med(bms) if bms else None,
           "scored_valid": svalid, "bounded_valid": bvalid,
           "lib": os.environ.get("BOTE_LIB_PATH", "tree")}
    print(json.dumps(doc))


if __name__ == "__main__":
    main()
