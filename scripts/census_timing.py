"""Census timings against top-K sweeps (profiles/census/README.md): synthetic R=64
n=7 in full, 2 warm-up launches, then 7 timed ones (5 on the generic kernel),
event-timed kernel ms; one process per line appended to OUT/census_timing.jsonl
(OUT: $CENSUS_OUT, default the working directory).  BOTE_LIB_PATH picks another
build of the library for the sweeps (the parent commit's, for an A/B).
  prep                      thresholds (top: the first 16 records of each list; spread: the keys
                            at the quantiles 1/17 .. 16/17) -> OUT/census_thr.json
  sweep  SET LABEL          forced-kernel top-K sweep (K = 100)
  census SET LABEL WHICH    census with the `top` or the `spread` thresholds
SET: fast5 (the default five, forced fast) or gen4 (MEAN, MAX, p95, MDTM af1, forced generic)."""
import hashlib
import json
import os
import statistics
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from fantoch_amd import _lib  # noqa: E402
from fantoch_amd.bote import DEFAULT_OBJECTIVES, DEFAULT_RANKING, DevicePlanet, Sweep  # noqa: E402
from fantoch_amd.planet import Planet  # noqa: E402

SETS = {"fast5": (list(DEFAULT_OBJECTIVES), "fast"),
        "gen4": ([(_lib.OBJ_MEAN, 0), (_lib.OBJ_MAX, 0), (_lib.OBJ_PCTL(9500), 0), (_lib.OBJ_MDTM, 0)], "generic")}
OUT = os.environ.get("CENSUS_OUT", ".")
THR = os.path.join(OUT, "census_thr.json")


def setup(name):
    objs, kernel = SETS[name]
    p = Planet.synthetic(64)
    return objs, kernel, DevicePlanet(p, 0), np.arange(64, dtype=np.uint32)


def emit(doc):
    doc["lib"] = "parent" if os.environ.get("BOTE_LIB_PATH") else "tree"
    with open(os.path.join(OUT, "census_timing.jsonl"), "a") as fh:
        fh.write(json.dumps(doc) + "\n")
    print(json.dumps(doc), flush=True)


def timed(launch, kernel_ms, n):
    for _ in range(2):
        launch()
        kernel_ms()
    ms = []
    for _ in range(n):
        launch()
        ms.append(kernel_ms())
    return {"launches": n, "median_ms": round(statistics.median(ms), 3), "min_ms": round(min(ms), 3),
            "max_ms": round(max(ms), 3)}


def main():
    os.makedirs(OUT, exist_ok=True)
    mode = sys.argv[1]
    if mode == "prep":
        from fantoch_amd.bote import Census
        doc = {}
        for name in SETS:
            objs, kernel, dp, srv = setup(name)
            sw = Sweep(dp, srv, srv, 7, objs, K=100, ranking=DEFAULT_RANKING, kernel=kernel)
            sw.launch()
            tops = sw.result().tops
            c = Census(dp, srv, srv, 7, objs, DEFAULT_RANKING, kernel=kernel)
            qs = [i / 17 for i in range(1, 17)]
            keys = c.quantiles(qs)
            doc[name] = {"top": [[list(x) for x in t[:16]] for t in tops],
                         "spread": [[[k, 0] for k in row] for row in keys]}
            print(name, "quantile keys", keys, flush=True)
        with open(THR, "w") as fh:
            json.dump(doc, fh)
        return
    name, label = sys.argv[2], sys.argv[3]
    objs, kernel, dp, srv = setup(name)
    n = 7 if name == "fast5" else 5
    if mode == "sweep":
        sw = Sweep(dp, srv, srv, 7, objs, K=100, ranking=DEFAULT_RANKING, kernel=kernel)
        doc = timed(lambda: sw.launch(), sw.kernel_ms, n)
        r = sw.result()
        doc.update(entry=f"{name}_sweep", label=label, kernel=sw.kernel_path(), configs=sw.total, deferred=sw.deferred(),
                   valid=r.valid, sha=hashlib.sha256(json.dumps(r.tops).encode()).hexdigest()[:16])
    else:
        from fantoch_amd.bote import Census
        which = sys.argv[4]
        thr = json.load(open(THR))[name][which]
        c = Census(dp, srv, srv, 7, objs, DEFAULT_RANKING, kernel=kernel)
        doc = timed(lambda: c.launch(thr), c.kernel_ms, n)
        r = c.result()
        doc.update(entry=f"{name}_census_{which}", label=label, kernel=c.kernel_path(), configs=c.total,
                   deferred=c.deferred(), valid=r.valid, below=r.below.tolist())
    emit(doc)


main()
