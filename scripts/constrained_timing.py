"""Constrained-sweep timings (profiles/constrained/README.md): synthetic R=64 n=7 in
full, K = 100, 2 warm-up launches, then 7 timed ones (5 on the generic kernel),
event-timed kernel ms; one process per line appended to
OUT/constrained_timing.jsonl (OUT: $CONSTRAINED_OUT, default the working
directory).  BOTE_LIB_PATH picks another build of the library for the sweeps both
builds can run (the parent commit's, for an A/B).
  prep            the bounds: per constraint the median key of its own list, from
                  Census.quantiles([0.5]) -> OUT/constrained_bounds.json
  run ENTRY LABEL one entry:
    a          the default five objectives, forced fast, no constraint
    b          a plus the constraint MEAN af1 <= its median key, forced fast
    b_control  a plus MEAN af1 once more as a sixth objective: the same key with a list
    b_generic  b on the forced generic kernel
    c          [MEAN af1, MEAN ff1] with the constraints p95 af1 and MAX ff1 at their
               median keys, forced fast (the list variant)
    c_control  [MEAN af1, MEAN ff1, p95 af1, MAX ff1] as four objectives, forced fast"""
import hashlib
import json
import os
import statistics
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from fantoch_amd import _lib  # noqa: E402
from fantoch_amd.bote import DEFAULT_OBJECTIVES, DEFAULT_RANKING, Census, DevicePlanet, Sweep  # noqa: E402
from fantoch_amd.planet import Planet  # noqa: E402

MEAN, MAX, P95 = _lib.OBJ_MEAN, _lib.OBJ_MAX, _lib.OBJ_PCTL(9500)
AF1, FF1 = _lib.SLOT_AF1, _lib.SLOT_FF1
CONS = [(MEAN, AF1), (P95, AF1), (MAX, FF1)]  # the kinds bounded at their median keys
OUT = os.environ.get("CONSTRAINED_OUT", ".")
BOUNDS = os.path.join(OUT, "constrained_bounds.json")


def entry(name, bound):
    """(objectives, constraints or None, kernel, ranking) of an entry."""
    two = [(MEAN, AF1), (MEAN, FF1)]
    return {
        "a": (list(DEFAULT_OBJECTIVES), None, "fast", DEFAULT_RANKING),
        "b": (list(DEFAULT_OBJECTIVES), [(MEAN, AF1, bound(MEAN, AF1))], "fast", DEFAULT_RANKING),
        "b_control": (list(DEFAULT_OBJECTIVES) + [(MEAN, AF1)], None, "fast", DEFAULT_RANKING),
        "b_generic": (list(DEFAULT_OBJECTIVES), [(MEAN, AF1, bound(MEAN, AF1))], "generic", DEFAULT_RANKING),
        "c": (two, [(P95, AF1, bound(P95, AF1)), (MAX, FF1, bound(MAX, FF1))], "fast", None),
        "c_control": (two + [(P95, AF1), (MAX, FF1)], None, "fast", None),
    }[name]


def main():
    os.makedirs(OUT, exist_ok=True)
    dp, srv = DevicePlanet(Planet.synthetic(64), 0), np.arange(64, dtype=np.uint32)
    if sys.argv[1] == "prep":
        c = Census(dp, srv, srv, 7, CONS, None)
        keys = [row[0] for row in c.quantiles([0.5])]
        with open(BOUNDS, "w") as fh:
            json.dump({f"{k}:{s}": key for (k, s), key in zip(CONS, keys)}, fh)
        print("median keys", keys, flush=True)
        return
    name, label = sys.argv[2], sys.argv[3]
    bounds = json.load(open(BOUNDS)) if os.path.exists(BOUNDS) else {}
    objs, cons, kernel, ranking = entry(name, lambda k, s: int(bounds[f"{k}:{s}"]))
    kw = {} if cons is None else {"constraints": cons}  # (the parent's Sweep takes no constraints)
    sw = Sweep(dp, srv, srv, 7, objs, K=100, ranking=ranking, kernel=kernel, **kw)
    n = 5 if kernel == "generic" else 7
    for _ in range(2):
        sw.launch()
        sw.kernel_ms()
    ms = []
    for _ in range(n):
        sw.launch()
        ms.append(sw.kernel_ms())
    r = sw.result()
    doc = {"entry": name, "label": label, "lib": "parent" if os.environ.get("BOTE_LIB_PATH") else "tree",
           "kernel": sw.kernel_path(), "launches": n, "median_ms": round(statistics.median(ms), 3),
           "min_ms": round(min(ms), 3), "max_ms": round(max(ms), 3), "configs": sw.total, "deferred": sw.deferred(),
           "valid": r.valid, "lists": [len(t) for t in r.tops],
           "tops_sha": hashlib.sha256(json.dumps(r.tops).encode()).hexdigest()[:16]}
    if cons is not None:
        doc["admitted"] = sw.admitted()
        doc["constraints"] = [[k, s, str(b)] for k, s, b in cons]
    with open(os.path.join(OUT, "constrained_timing.jsonl"), "a") as fh:
        fh.write(json.dumps(doc) + "\n")
    print(json.dumps(doc), flush=True)


main()
