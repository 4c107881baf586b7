#!/usr/bin/env python3
"""Wall time of the streaming evolving search (fantoch_amd.evolve.Evolve,
DESIGN.md §4 "Streaming evolving search"; results under profiles/evolve/).

Workload: synthetic R = 64, levels 3 -> 13, beam = 256, K = 32.  One process:
one warm-up run, then `--reps` runs; one JSON line with the wall time of run()
(median, min .. max) and, from the median run, per level the frontier, the
batches, the chains kept and the sum of the kernel times.

  python scripts/evolve_timing.py [--ranking 110,35,0,15] [--beam 256] [-K 32] [--reps 3]
"""
import argparse
import json
import os
import statistics
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from fantoch_amd.bote import DevicePlanet, FTMetric, RankingParams  # noqa: E402
from fantoch_amd.evolve import Evolve  # noqa: E402
from fantoch_amd.planet import Planet  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--regions", type=int, default=64)
    ap.add_argument("--ranking", default="110,35,0,15")
    ap.add_argument("--beam", type=int, default=256)
    ap.add_argument("-K", type=int, default=32)
    ap.add_argument("--reps", type=int, default=3)
    args = ap.parse_args()
    a, b, c, d = (float(x) for x in args.ranking.split(","))
    params = RankingParams(a, b, c, d, 3, 13, FTMetric.F1F2)
    dp = DevicePlanet(Planet.synthetic(args.regions))
    srv = np.arange(args.regions, dtype=np.uint32)
    ev = Evolve(dp, srv, srv, params, beam=args.beam, K=args.K)
    ev.run()
    runs = sorted((ev.run() for _ in range(args.reps)), key=lambda r: r.wall_s)
    mid = runs[len(runs) // 2]
    walls = [r.wall_s * 1e3 for r in runs]
    print(json.dumps({
        "regions": args.regions, "levels": mid.ns, "ranking": args.ranking, "beam": args.beam, "K": args.K,
        "chains": len(mid.chains), "exhaustive": mid.exhaustive, "best_score": mid.chains[0][0] if mid.chains else None,
        "wall_ms": {"median": round(statistics.median(walls), 3), "min": round(min(walls), 3), "max": round(max(walls), 3)},
        "kernel_ms_sum": round(sum(lv.kernel_ms for lv in mid.levels), 4),
        "per_level": [{"n": lv.n, "frontier": lv.frontier, "batches": lv.batches, "chains": lv.chains,
                       "kernel_ms": round(lv.kernel_ms, 4)} for lv in mid.levels],
        "lib": os.environ.get("BOTE_LIB_PATH", "tree")}))


if __name__ == "__main__":
    main()
