#!/usr/bin/env python3
"""Kernel time of the generic kernel's top-K families (bote_eval.hpp) on the
synthetic R = 64 planet at n = 7, one forced-generic launch over a rank range:

  python scripts/generic_timing.py [--ranks 100000000] [--rounds 7] [--warmup 2]

prints one JSON line: per family the median of `rounds` launches with
min .. max (event-timed, ms) after `warmup` launches, and the library
(BOTE_LIB_PATH, for an A/B against another build: one process per line).
Families: topk / topk_x (default objectives, base / extended keys), pctl
(p95 af1, p75 af1C, MAX e), mdtm (MDTM af1, MDTM ff1C, p95 af1), pinned /
pinned_mdtm (position 0 pinned: default objectives / MAX e, p95 af1)."""
import argparse
import json
import os
import statistics
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from fantoch_amd import _lib  # noqa: E402
from fantoch_amd.bote import DEFAULT_OBJECTIVES, DEFAULT_RANKING, DevicePlanet, Sweep  # noqa: E402
from fantoch_amd.planet import Planet  # noqa: E402

P, MAX, MDTM, MEAN = _lib.OBJ_PCTL, _lib.OBJ_MAX, _lib.OBJ_MDTM, _lib.OBJ_MEAN
FAMILIES = {
    "topk": dict(objs=DEFAULT_OBJECTIVES, ranking=DEFAULT_RANKING, digest=True),
    "topk_x": dict(objs=DEFAULT_OBJECTIVES, ranking=DEFAULT_RANKING, digest=True, keys=_lib.KEYS_TEMPO_ALL_LEADERS),
    "pctl": dict(objs=[(P(9500), 0), (P(7500), 5), (MAX, 4)]),
    "mdtm": dict(objs=[(MDTM, 0), (MDTM, 6), (P(9500), 0)]),
    "pinned": dict(objs=DEFAULT_OBJECTIVES, ranking=DEFAULT_RANKING, digest=True, pinned=[0]),
    "pinned_mdtm": dict(objs=[(MAX, 4), (P(9500), 0), (MEAN, 0)], pinned=[0]),
}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--ranks", type=int, default=100_000_000, help="per launch (at most the rank space)")
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=2)
    args = ap.parse_args()
    dp = DevicePlanet(Planet.synthetic(64))
    srv = np.arange(64, dtype=np.uint32)
    out = {"lib": os.environ.get("BOTE_LIB_PATH", "this build"), "ranks": args.ranks}
    for name, f in FAMILIES.items():
        sw = Sweep(dp, srv, srv, 7, f["objs"], K=100, ranking=f.get("ranking"), digest=f.get("digest", False),
                   kernel="generic", keys=f.get("keys", _lib.KEYS_BASE), pinned=f.get("pinned"))
        assert sw.kernel_path() == "generic"
        ranks = min(args.ranks, sw.total)
        rb = (sw.total - ranks) // 2
        ms = []
        for i in range(args.warmup + args.rounds):
            sw.launch(rb, rb + ranks)
            r = sw.result()
            if i >= args.warmup:
                ms.append(sw.kernel_ms())
        out[name] = {"median_ms": round(statistics.median(ms), 3), "min_ms": round(min(ms), 3),
                     "max_ms": round(max(ms), 3), "digest": r.digest, "first": r.tops[0][:1]}
    print(json.dumps(out))


if __name__ == "__main__":
    main()
