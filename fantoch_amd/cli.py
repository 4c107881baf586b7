"""`python -m fantoch_amd` — the reference's bote binary, and flags for the
search the reference hard-codes.

With no arguments it does what `fantoch_bote/src/main.rs:4-85` does: the
distance table of the 13 regions (`distance_table`, main.rs:9-30, through
`Planet::distance_matrix`, planet/mod.rs:144-177), then `Search::new(3, 13,
R13C13, save_search = true)`, `sorted_evolving_configs` under
`RankingParams::new(110, 35, 0, 15, 3, 13, F1F2)` and, for the best chain,
`score: {:?}` and one `Search::stats_fmt` line per configuration
(main.rs:32-85).  Everything is computed by the gfx950 kernels
(libbote_hip.so); there is no CPU path.

The reference has no CLI (parameters are hard-coded in
main.rs:31-60).  Subcommands expose them, and the sweep the hot path serves:

  python -m fantoch_amd [main] [--lat-dir D] [--input R13C13] [--min-n 3] [--max-n 13]
                        [--ranking 110,35,0,15] [--ft-metric F1F2] [--chains 1] [--no-save-search]
  python -m fantoch_amd distance-table [--lat-dir D] [--regions a,b,...]
  python -m fantoch_amd stats --config a,b,c [--clients ...] [--tempo] [--lat-dir D]
  python -m fantoch_amd sweep (--synthetic R [--seed S] | --lat-dir D) --n N [--K 100]
                        [--objectives default|config5|mean:af1,cov:af1,max:af1,p95:af1,p99.9:e,mdtm:af1,score,...]
                        [--keys base|tempo-all-leaders] [--gpus G] [--rank-begin B --rank-end E]
                        [--pinned a,b | --pinned 3,9 | --pinned-sets "a,b;c,d"]
                        [--where "mean:ff1<=140,p99:af1<=300,cov:ff1C<=key:0x3f..."]
  python -m fantoch_amd evolve (--synthetic R [--seed S] | --lat-dir D [--input R13C13|R17C17|R20C20])
                        [--min-n 3] [--max-n 13] [--beam B] [-K 100] [--ranking 110,35,0,15] [--ft F1F2]
                        [--chains 1]
  python -m fantoch_amd census (--synthetic R [--seed S] | --lat-dir D) --n N [--objectives ...]
                        [--ranking 110,35,0,15] [--ft F1F2] [--kernel auto|generic|fast]
                        [--config a,b,c] [--quantiles 0.01,0.5,0.99]
"""
from __future__ import annotations

import argparse
import json
import sys
from decimal import Decimal
from typing import List, Optional, Sequence

# main.rs:12-25
REGIONS13 = ("asia-southeast1", "europe-west4", "southamerica-east1", "australia-southeast1", "europe-west2",
             "asia-south1", "us-east1", "asia-northeast1", "europe-west1", "asia-east1", "us-west1", "europe-west3",
             "us-central1")


def rust_f64(x: float) -> str:
    """Rust's `{}` / `{:?}` of an f64 (float.rs:97-101 Debug = Display): the
    shortest round-trip digits, never in exponent form, integral values with
    no fractional part ("10360" for 10360.0, "-0" for -0.0)."""
    if x != x:
        return "NaN"
    if x in (float("inf"), float("-inf")):
        return "inf" if x > 0 else "-inf"
    s = format(Decimal(repr(float(x))), "f")
    if "." in s:
        s = s.rstrip("0").rstrip(".")
    return s


def _planet(args):
    from .planet import Planet

    if getattr(args, "synthetic", None):
        return Planet.synthetic(args.synthetic, args.seed)
    return Planet.from_dir(args.lat_dir) if args.lat_dir else Planet.new()


def distance_table(planet, regions: Sequence[str]) -> str:
    """main.rs:9-30: `if let Ok(matrix) = planet.distance_matrix(regions) { println!("{}", matrix) }`."""
    from .planet import Region

    return planet.distance_matrix([Region(r) for r in regions])


def best_chains(args, out=sys.stdout) -> int:
    """main.rs:32-85 (the search, then the best chain's score and stats).
    main.rs takes the best chain with `.next().unwrap()`, which panics (exit
    101) when no evolving chain exists: with no chain this prints an error to
    stderr and returns 101."""
    from .bote import FTMetric, RankingParams, Search, SearchInput

    planet = _planet(args)
    search = Search(args.min_n, args.max_n, SearchInput(args.input), save_search=args.save_search,
                    planet=planet, device=args.device)
    a, b, c, d = (int(x) for x in args.ranking.split(","))
    params = RankingParams.new(a, b, c, d, args.min_n, args.max_n, FTMetric[args.ft_metric])
    chains = search.sorted_evolving_configs(params, limit=args.chains)
    if not chains:
        print("error: no evolving config chain (main.rs:66-69 `.next().unwrap()` on None)", file=sys.stderr)
        return 101
    for score, css, _clients in chains[:args.chains]:
        print(f"score: {rust_f64(score.value())}", file=out)
        sorted_config: List = []
        for cs in css:
            for region in cs.config:
                if region not in sorted_config:
                    sorted_config.append(region)
            print(Search.stats_fmt(cs.stats, len(cs.config)), file=out)
        if args.show_order:  # (main.rs builds `sorted_config` but does not print it)
            print(f"sorted_config: {sorted_config!r}", file=out)
    return 0


def config_stats(args, out=sys.stdout) -> None:
    """`Search::compute_stats` (search.rs:262-319) of one config, printed as
    `Search::stats_fmt`, and Tempo's keys (config.rs:317-329) with --tempo."""
    from .bote import Bote, Search

    planet = _planet(args)
    bote = Bote.from_(planet, args.device)
    config = args.config.split(",")
    clients = args.clients.split(",") if args.clients else [r.name for r in planet.regions()]
    stats = Search.compute_stats(config, clients, bote, tempo=args.tempo)
    print(Search.stats_fmt(stats, len(config)), file=out)
    if args.tempo:
        for key in sorted(k for k in stats.map if k.startswith("t")):
            print(f"{key}={stats.map[key]!r}", file=out)


def _pctl_kind(name: str):
    """p95, p99.9, p99.99 -> the percentile objective kind (None: not of that form);
    up to two decimals, 0.01 .. 99.99."""
    import re

    from . import _lib

    m = re.fullmatch(r"p(\d{1,2})(?:\.(\d{1,2}))?", name)
    if not m:
        return None
    bp = int(m.group(1)) * 100 + int((m.group(2) or "").ljust(2, "0"))
    return _lib.OBJ_PCTL(bp)  # (p0 is refused there)


def _objective_name(kind: int) -> str:
    from . import _lib

    if _lib.is_pctl(kind):
        whole, frac = divmod(kind & 0xFFFF, 100)
        return f"p{whole}" + (f".{frac:02d}".rstrip("0") if frac else "")
    return {_lib.OBJ_SCORE: "score", _lib.OBJ_MEAN: "mean", _lib.OBJ_COV: "cov", _lib.OBJ_MAX: "max",
            _lib.OBJ_MDTM: "mdtm"}[kind]


def _objectives(spec: str):
    from . import _lib
    from .bote import CONFIG5_OBJECTIVES, DEFAULT_OBJECTIVES

    if spec == "default":
        return list(DEFAULT_OBJECTIVES)
    if spec == "config5":
        return list(CONFIG5_OBJECTIVES)
    kinds = {"score": _lib.OBJ_SCORE, "mean": _lib.OBJ_MEAN, "cov": _lib.OBJ_COV, "max": _lib.OBJ_MAX,
             "mdtm": _lib.OBJ_MDTM}
    out = []
    for item in spec.split(","):
        if item == "score":
            out.append((_lib.OBJ_SCORE, 0))
            continue
        kind, slot = item.split(":")
        pctl = _pctl_kind(kind)
        out.append((kinds[kind] if pctl is None else pctl, _lib.SLOT_NAMES_X.index(slot)))
    return out


def _pinned(spec: Optional[str], names: Sequence[str]) -> Optional[List[int]]:
    """--pinned: comma-separated region names or positions into the server list
    (the planet's regions in name order), as --config takes names for `stats`."""
    if not spec:
        return None
    names = list(names)
    out = []
    for item in spec.split(","):
        item = item.strip()
        if item.isdigit():
            pos = int(item)
            if pos >= len(names):
                raise ValueError(f"--pinned: position {pos} is outside the {len(names)} servers")
        elif item in names:
            pos = names.index(item)
        else:
            raise ValueError(f"--pinned: unknown region {item!r}")
        if pos in out:
            raise ValueError(f"--pinned: {item!r} is given twice")
        out.append(pos)
    return out


def _pinned_sets(spec: Optional[str], names: Sequence[str]) -> Optional[List[List[int]]]:
    """--pinned-sets: ';'-separated --pinned lists, all of one size."""
    if not spec:
        return None
    sets = [_pinned(part, names) for part in spec.split(";")]
    if any(s is None for s in sets) or len({len(s) for s in sets}) != 1:
        raise ValueError("--pinned-sets: every set needs the same number of members, at least one")
    return sets


def sweep(args, out=sys.stdout):
    """The exhaustive sweep of every n-subset (search.rs:199-319 + the ranking's
    compute_score, search.rs:421-472) streamed through the device top-K, sharded
    over --gpus devices (bote_search_*), as one JSON object: per objective the
    K best (key, colex rank, regions), the valid count and the digest."""
    import numpy as np

    from . import _lib
    from .bote import (DEFAULT_RANKING, DevicePlanet, MultiDeviceSearch, PinnedBatch, Sweep, max_key, mdtm_key,
                       parse_where, pctl_key)

    planet = _planet(args)
    srv = np.arange(planet.R, dtype=np.uint32)
    objs = _objectives(args.objectives)
    keys = _lib.KEYS_TEMPO_ALL_LEADERS if args.keys == "tempo-all-leaders" else _lib.KEYS_BASE
    pinned = _pinned(getattr(args, "pinned", None), planet.names)
    if pinned is not None and (args.gpus > 1 or keys != _lib.KEYS_BASE):
        raise ValueError("--pinned sweeps run on one device with the base key set")
    sets = _pinned_sets(getattr(args, "pinned_sets", None), planet.names)
    if sets is not None:
        if pinned is not None:
            raise ValueError("--pinned-sets and --pinned exclude each other")
        if args.gpus > 1 or keys != _lib.KEYS_BASE or args.rank_begin is not None or args.rank_end is not None:
            raise ValueError("--pinned-sets sweeps every set's whole rank space on one device with the base key set")
    where = getattr(args, "where", None)
    cons = parse_where(where, planet.R, args.n) if where else None
    if cons is not None and (args.gpus > 1 or keys != _lib.KEYS_BASE or pinned is not None or sets is not None):
        raise ValueError("--where sweeps run unpinned on one device with the base key set")
    admitted = None
    # (--rank-begin / --rank-end of a pinned sweep are pinned ranks)
    total = _lib.binomial(planet.R, args.n) if pinned is None else _lib.pinned_total(planet.R, args.n, len(pinned))
    rb = args.rank_begin or 0
    re = total if args.rank_end is None else args.rank_end
    if sets is not None:
        total = re = _lib.pinned_total(planet.R, args.n, len(sets[0]))
        batch = PinnedBatch(DevicePlanet(planet, args.device), srv, srv, args.n, sets, objs, K=args.K,
                            ranking=DEFAULT_RANKING, digest=True)
        batch.launch()
        results = batch.result()
    elif args.gpus > 1:
        dps = [DevicePlanet(planet, d) for d in range(args.gpus)]
        h = MultiDeviceSearch(dps, srv, srv, args.n, objectives=objs, K=args.K, ranking=DEFAULT_RANKING,
                              rank_begin=rb, rank_end=re, keys=keys)
        h.launch()
        res = h.result()
    else:
        sw = Sweep(DevicePlanet(planet, args.device), srv, srv, args.n, objs, K=args.K, ranking=DEFAULT_RANKING,
                   digest=True, keys=keys, pinned=pinned, constraints=cons)
        sw.launch(rb, re)
        res = sw.result()
        admitted = sw.admitted() if cons is not None else None

    def regions(rank):
        return [planet.names[i] for i in _lib.colex_unrank(int(rank), args.n, planet.R)]

    def record(kind, slot, key, rank):
        rec = {"key": str(key), "rank": rank, "regions": regions(rank)}
        if kind == _lib.OBJ_MAX:  # the composite key's halves
            rec["max"], rec["sum"] = max_key(key)
        elif _lib.is_pctl(kind):  # Histogram::percentile's f64 (a midpoint may end in .5)
            twice, rec["sum"] = pctl_key(key)
            rec["percentile"] = twice / 2
            rec = {k: rec[k] for k in ("key", "rank", "regions", "percentile", "sum")}
        elif kind == _lib.OBJ_MDTM:  # Histogram::mdtm = 2 H / count^2 (count: the clients, or n for a colocated slot)
            h, total = mdtm_key(key)
            count = args.n if 5 <= slot < 10 or 14 <= slot < 18 else planet.R
            rec["mdtm"], rec["sum"] = 2 * h / count ** 2, total
        return rec

    def block(res, pinned):
        doc = {"regions": planet.R, "n": args.n, "rank_begin": rb, "rank_end": re, "configs": re - rb,
               "keys": args.keys, "gpus": args.gpus, "valid": res.valid, "digest": str(res.digest),
               "objectives": [{"objective": _objective_name(k) + ("" if k == _lib.OBJ_SCORE else ":" + _lib.SLOT_NAMES_X[s]),
                               "top": [record(k, s, key, rank) for key, rank in res.tops[o][:args.show]]}
                              for o, (k, s) in enumerate(objs)]}
        if pinned is not None:
            doc["pinned"] = pinned
        if admitted is not None:  # beside the valid count: "admitted N of TOTAL"
            doc["where"], doc["admitted"] = where, admitted
            doc["admitted_of"] = f"admitted {admitted} of {re - rb}"
        print(json.dumps(doc, indent=None if args.compact else 1), file=out)
        return doc

    if sets is not None:  # one block per set, each as --pinned prints that set
        return [block(r, s) for r, s in zip(results, sets)]
    return block(res, pinned)


def _decode_key(kind: int, slot: int, key: int, n: int, clients: int) -> dict:
    """A quantile's key in the objective's own terms (the keys of include/bote_hip.h)."""
    import numpy as np

    from . import _lib
    from .bote import max_key, mdtm_key, pctl_key
    from .evolve import key_score

    rec = {"key": str(key)}
    count = n if 5 <= slot < 10 else clients
    if kind == _lib.OBJ_SCORE:
        rec["score"] = float(key_score(np.array([key], np.uint64))[0])
    elif kind == _lib.OBJ_MEAN:
        rec["sum"], rec["mean"] = key, key / count
    elif kind == _lib.OBJ_COV:  # the key is fl64(V / S1^2) = cov^2 (count - 1) / count
        ratio = float(np.array([key], np.uint64).view(np.float64)[0])
        rec["cov"] = None if ratio != ratio or count < 2 else (ratio * count / (count - 1)) ** 0.5
    elif kind == _lib.OBJ_MAX:
        rec["max"], rec["sum"] = max_key(key)
    elif _lib.is_pctl(kind):
        twice, rec["sum"] = pctl_key(key)
        rec["percentile"] = twice / 2
    elif kind == _lib.OBJ_MDTM:
        h, rec["sum"] = mdtm_key(key)
        rec["mdtm"] = 2 * h / count ** 2
    return rec


def census(args, out=sys.stdout):
    """Where a config stands among all C(R, n) (--config: per objective its position,
    the population and their ratio) and the shape of each objective over the space
    (--quantiles: per objective the key at each quantile of the full ordering), by
    census sweeps (bote_census_*), as one JSON line."""
    import numpy as np

    from . import _lib
    from .bote import Census, DevicePlanet, FTMetric, RankingParams

    if not args.config and not args.quantiles:
        raise ValueError("census: give --config and/or --quantiles")
    planet = _planet(args)
    srv = np.arange(planet.R, dtype=np.uint32)
    objs = _objectives(args.objectives)
    a, b, c, d = (float(x) for x in args.ranking.split(","))
    params = RankingParams(a, b, c, d, args.n, args.n, FTMetric[args.ft])
    cs = Census(DevicePlanet(planet, args.device), srv, srv, args.n, objs, ranking=params,
                kernel=None if args.kernel == "auto" else args.kernel)
    names = [_objective_name(k) + ("" if k == _lib.OBJ_SCORE else ":" + _lib.SLOT_NAMES_X[s]) for k, s in objs]
    doc = {"regions": planet.R, "n": args.n, "configs": cs.total, "kernel": cs.kernel_path(),
           "objectives": [{"objective": name} for name in names]}
    if args.config:
        try:
            pos = _pinned(args.config, planet.names)
        except ValueError as e:  # (the same syntax as --pinned: names or positions)
            raise ValueError(str(e).replace("--pinned", "--config")) from None
        doc["config"] = [planet.names[p] for p in sorted(pos)]
        for o, (position, population) in enumerate(cs.position_of(pos)):
            doc["objectives"][o].update(position=position, population=population,
                                        share=None if position is None or not population else position / population)
    if args.quantiles:
        qs = [float(x) for x in args.quantiles.split(",")]
        doc["quantiles"] = qs
        for o, keys in enumerate(cs.quantiles(qs)):
            doc["objectives"][o]["quantile_keys"] = [None if k is None else _decode_key(*objs[o], k, args.n, planet.R)
                                                     for k in keys]
    print(json.dumps(doc), file=out)
    return doc


def evolve(args, out=sys.stdout) -> int:
    """The streaming evolving search (evolve.py): the best chains' scores and, per
    level, the region names, then whether the search was exhaustive (then the
    chains are Search::sorted_evolving_configs').  No chain: exit 101, as `main`."""
    import numpy as np

    from .bote import DevicePlanet, FTMetric, RankingParams, SearchInput
    from .evolve import Evolve

    planet = _planet(args)
    if args.input and not args.synthetic:
        regions, _ = SearchInput(args.input).get_inputs(args.max_n, planet)
        srv = np.array(sorted(planet.idx(r) for r in regions), dtype=np.uint32)
    else:
        srv = np.arange(planet.R, dtype=np.uint32)
    a, b, c, d = (float(x) for x in args.ranking.split(","))
    params = RankingParams(a, b, c, d, args.min_n, args.max_n, FTMetric[args.ft])
    res = Evolve(DevicePlanet(planet, args.device), srv, srv, params, beam=args.beam, K=args.K).run()
    for lv in res.levels:
        print(f"level n={lv.n}: frontier {lv.frontier}, batches {lv.batches}, chains {lv.chains}, "
              f"kernel {lv.kernel_ms:.3f} ms", file=out)
    print(f"chains: {len(res.chains)}", file=out)
    print("exhaustive: " + ("yes (the chains are sorted_evolving_configs')" if res.exhaustive
                            else "no (a list came back full or the beam cut)"), file=out)
    if not res.chains:
        print("error: no evolving config chain", file=sys.stderr)
        return 101
    for chain in res.chains[:args.chains]:
        print(f"score: {rust_f64(chain[0])}", file=out)
        for n, ids in zip(res.ns, res.configs_of(chain)):
            print(f"n={n}: " + ",".join(planet.names[i] for i in ids), file=out)
    return 0


def build_parser() -> argparse.ArgumentParser:
    ap = argparse.ArgumentParser(prog="python -m fantoch_amd", description=__doc__.split("\n\n")[0], allow_abbrev=False)
    sub = ap.add_subparsers(dest="cmd")

    def planet_flags(p, synthetic=False):
        p.add_argument("--lat-dir", default=None, help="a directory of ping .dat files (default: latency_gcp)")
        if synthetic:
            p.add_argument("--synthetic", type=int, default=None, metavar="R", help="synthetic R-region planet")
            p.add_argument("--seed", type=int, default=None)
        p.add_argument("--device", type=int, default=0)

    def main_flags(p):
        planet_flags(p)
        p.add_argument("--input", default="R13C13", choices=["R13C13", "R17C17", "R20C20", "R17CMaxN"])
        p.add_argument("--min-n", type=int, default=3)
        p.add_argument("--max-n", type=int, default=13)
        p.add_argument("--ranking", default="110,35,0,15",
                       help="min_mean_fpaxos_improv,min_mean_epaxos_improv,min_fairness_fpaxos_improv,"
                            "min_mean_decrease")
        p.add_argument("--ft-metric", default="F1F2", choices=["F1", "F1F2"])
        p.add_argument("--chains", type=int, default=1, help="best chains to print (main.rs: 1)")
        p.add_argument("--no-save-search", dest="save_search", action="store_false",
                       help="do not write {min}_{max}_{input}.data (main.rs saves it)")
        p.add_argument("--no-distance-table", dest="distance_table", action="store_false")
        p.add_argument("--show-order", action="store_true", help="also print the chain's sorted_config")

    main_flags(ap)
    main_flags(sub.add_parser("main", allow_abbrev=False, help="main.rs: distance table + best evolving chain"))
    p = sub.add_parser("distance-table", allow_abbrev=False, help="Planet::distance_matrix of the given regions")
    planet_flags(p)
    p.add_argument("--regions", default=",".join(REGIONS13))
    p = sub.add_parser("stats", allow_abbrev=False, help="Search::compute_stats of one config (stats_fmt)")
    planet_flags(p, synthetic=True)
    p.add_argument("--config", required=True, help="comma-separated region names")
    p.add_argument("--clients", default=None, help="comma-separated region names (default: every region)")
    p.add_argument("--tempo", action="store_true", help="also Tempo's fast/tiny/write keys")
    p = sub.add_parser("sweep", allow_abbrev=False, help="exhaustive n-subset sweep with the device top-K")
    planet_flags(p, synthetic=True)
    p.add_argument("--n", type=int, required=True)
    p.add_argument("--K", type=int, default=100)
    p.add_argument("--show", type=int, default=10, help="records printed per objective")
    p.add_argument("--objectives", default="default")
    p.add_argument("--keys", default="base", choices=["base", "tempo-all-leaders"])
    p.add_argument("--gpus", type=int, default=1)
    p.add_argument("--rank-begin", type=int, default=None)
    p.add_argument("--rank-end", type=int, default=None)
    p.add_argument("--pinned", default=None,
                   help="region names or positions every swept config contains (rank flags are then pinned ranks)")
    p.add_argument("--pinned-sets", default=None,
                   help="';'-separated --pinned lists of one size: one launch sweeps every set, one block per set")
    p.add_argument("--where", default=None,
                   help="rank only the configs within key bounds: KIND:SLOT<=VALUE[,...], e.g. "
                        "'mean:ff1<=140,p99:af1<=300,cov:ff1C<=key:0x3f9...' (mean, cov, max, mdtm, pNN; a cov "
                        "bound is a raw key); prints the admitted count beside the valid count")
    p.add_argument("--compact", action="store_true")
    p = sub.add_parser("evolve", allow_abbrev=False, help="streaming evolving search: bounded pinned batches and a beam")
    planet_flags(p, synthetic=True)
    p.add_argument("--input", default=None, choices=["R13C13", "R17C17", "R20C20"],
                   help="the reference's server/client set of a GCP planet (default: every region)")
    p.add_argument("--min-n", type=int, default=3)
    p.add_argument("--max-n", type=int, default=13)
    p.add_argument("--beam", type=int, default=None, help="partial chains kept after each level (default: all)")
    p.add_argument("-K", "--K", dest="K", type=int, default=100, help="records kept per list")
    p.add_argument("--ranking", default="110,35,0,15",
                   help="min_mean_fpaxos_improv,min_mean_epaxos_improv,min_fairness_fpaxos_improv,"
                        "min_mean_decrease")
    p.add_argument("--ft", default="F1F2", choices=["F1", "F1F2"])
    p.add_argument("--chains", type=int, default=1, help="best chains to print")
    p = sub.add_parser("census", allow_abbrev=False,
                       help="census sweeps: a config's position among all C(R, n), quantiles of the objectives")
    planet_flags(p, synthetic=True)
    p.add_argument("--n", type=int, required=True)
    p.add_argument("--objectives", default="default")
    p.add_argument("--ranking", default="110,35,0,15",
                   help="min_mean_fpaxos_improv,min_mean_epaxos_improv,min_fairness_fpaxos_improv,"
                        "min_mean_decrease")
    p.add_argument("--ft", default="F1F2", choices=["F1", "F1F2"])
    p.add_argument("--kernel", default="auto", choices=["auto", "generic", "fast"])
    p.add_argument("--config", default=None, help="region names or positions: the config whose position is asked")
    p.add_argument("--quantiles", default=None, help="comma-separated q in (0, 1]: the key at each quantile")
    return ap


def main(argv: Optional[Sequence[str]] = None, out=sys.stdout) -> int:
    args = build_parser().parse_args(argv)
    cmd = args.cmd or "main"
    if cmd == "main":
        if args.distance_table:
            print(distance_table(_planet(args), REGIONS13), file=out)
        return best_chains(args, out)
    elif cmd == "distance-table":
        print(distance_table(_planet(args), args.regions.split(",")), file=out)
    elif cmd == "stats":
        config_stats(args, out)
    elif cmd == "sweep":
        sweep(args, out)
    elif cmd == "census":
        census(args, out)
    elif cmd == "evolve":
        return evolve(args, out)
    return 0
