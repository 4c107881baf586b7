"""Census sweeps (bote_census_*, fantoch_amd.bote.Census): per objective and
threshold record, the number of offered configs before it in the lists' unsigned
(key, rank) order, on the fast kernel's census variant (with the generic
kernel's fix-up of deferred configs and its overflow fallback) and on the
generic kernel's.

The expected counts come from the CPU oracle's complete order
(OraclePlanet.sweep with K = every config: a SCORE list holds the valid configs,
every other list every config) by bisection, from a device sweep's own lists
(record i has i configs before it), or from per-config keys built of the
oracle's per-client values (tests/host_keys.py).  Every comparison is exact
equality."""
import bisect
import math
from fractions import Fraction

import numpy as np
import pytest

import oracle as O
from fantoch_amd import _lib
from fantoch_amd.bote import DEFAULT_OBJECTIVES, DEFAULT_RANKING, Census, DevicePlanet, Sweep
from fantoch_amd.planet import Planet
from tests.host_keys import colex_positions, key_of, slot_values

pytestmark = pytest.mark.gpu

U64 = (1 << 64) - 1
SCORE, MEAN, COV, MAX, MDTM = _lib.OBJ_SCORE, _lib.OBJ_MEAN, _lib.OBJ_COV, _lib.OBJ_MAX, _lib.OBJ_MDTM
AF1, FF1, E = 0, 1, 4
OBJS = [(SCORE, 0), (MEAN, AF1), (MEAN, FF1), (COV, AF1), (COV, 5 + FF1), (MEAN, E)]
RP = (110.0, 35.0, 0.0, 15.0)
KERNELS = [None, "fast", "generic"]
NAN_KEY = 0x7FF8000000000000
T = _lib.CENSUS_MAX_THRESHOLDS


@pytest.fixture(scope="module")
def gcp():
    p = Planet.new()
    return p, DevicePlanet(p), O.OraclePlanet.of(p)


_FULL = {}


def full_order(gcp, n):
    """The oracle's complete ordered lists of GCP (every region a server and a client) for OBJS,
    as Python-int (key, rank) tuples, and the valid count; computed once per n."""
    p, _, o = gcp
    if n not in _FULL:
        srv = np.arange(p.R, dtype=np.uint32)
        total = math.comb(p.R, n)
        tops, valid, _ = o.sweep(srv, srv, n, 0, total, OBJS, total, RP, 2, 8)
        lists = [[(int(k), int(r)) for k, r in t] for t in tops]
        assert len(lists[0]) == valid and all(len(t) == total for t in lists[1:])
        assert all(t == sorted(t) for t in lists)
        _FULL[n] = (lists, valid)
    return _FULL[n]


def below(lst, thr):
    """The records of the ascending list before `thr`, by bisection."""
    return bisect.bisect_left(lst, thr)


def equal_key_pairs(lst, want=2):
    """Both members of the first `want` disjoint adjacent pairs of records sharing a key."""
    out, i = [], 0
    while i + 1 < len(lst) and len(out) < 2 * want:
        if lst[i][0] == lst[i + 1][0]:
            out += [lst[i], lst[i + 1]]
            i += 2
        else:
            i += 1
    return out


def thresholds_of(lst, kind):
    """Members at the ends and the middle, tied neighbours, and records of no config; ascending, T of them."""
    members = [lst[i] for i in (0, 1, len(lst) // 2, len(lst) - 2, len(lst) - 1)]
    k = lst[len(lst) // 3][0]
    thr = members + equal_key_pairs(lst) + [(k, 0), (k, U64), (0, 0), (U64, U64)]
    if kind == COV:
        thr.append((NAN_KEY, 0))
    assert len(thr) <= T
    thr += [(U64, U64)] * (T - len(thr))
    return sorted(thr)


# ------------------------------------------------------------------------
@pytest.mark.parametrize("n", [3, 5])
def test_counts_against_the_oracles_full_order(gcp, n):
    """GCP n = 3 (1,140 configs, 47 valid) and n = 5 (15,504, 839 valid) on auto, forced fast and
    forced generic: list members at both ends and the middle, both members of tied pairs (rank
    decides), (k, 0) and (k, 2^64 - 1) around a key of the list, (0, 0), all ones, and for COV a
    NaN pattern, which is above every finite key in the integer order."""
    p, dp, _ = gcp
    lists, valid = full_order(gcp, n)
    assert (len(lists[0]), len(lists[1])) == {3: (47, 1140), 5: (839, 15504)}[n]
    assert len({k for k, _ in lists[1]}) == {3: 908, 5: 2807}[n]
    assert len(equal_key_pairs(lists[1])) == 4 and len(equal_key_pairs(lists[2])) == 4
    srv = np.arange(p.R, dtype=np.uint32)
    thr = [thresholds_of(lst, kind) for lst, (kind, _) in zip(lists, OBJS)]
    want = np.array([[below(lst, t) for t in row] for lst, row in zip(lists, thr)], dtype=np.uint64)
    for kernel in KERNELS:
        c = Census(dp, srv, srv, n, OBJS, DEFAULT_RANKING, kernel=kernel)
        assert c.kernel_path() == ("generic" if kernel == "generic" else "fast"), kernel
        assert c.total == len(lists[1])
        c.launch(thr)
        res = c.result()
        print(n, kernel, res.valid, res.below.tolist())
        assert res.valid == valid, kernel
        assert np.array_equal(res.below, want), (n, kernel)


@pytest.mark.parametrize("objs,path", [
    ([(MEAN, AF1), (MAX, AF1), (_lib.OBJ_PCTL(9500), AF1), (MDTM, AF1)], "generic"),
    (list(DEFAULT_OBJECTIVES), "fast"),
])
def test_a_sweeps_own_records_have_their_indices(gcp, objs, path):
    """GCP n = 7 (77,520 configs), K = 100: record i of a full sweep's list has i configs before it.
    MAX, p95 and MDTM objectives run the generic kernel's census variant, the default five the fast
    kernel's; thresholds are the first 16 and the last 16 records of every list."""
    p, dp, _ = gcp
    srv = np.arange(p.R, dtype=np.uint32)
    sw = Sweep(dp, srv, srv, 7, objs, K=100, ranking=DEFAULT_RANKING)
    sw.launch()
    tops = sw.result().tops
    assert all(len(t) == 100 for t in tops)
    c = Census(dp, srv, srv, 7, objs, DEFAULT_RANKING)
    assert c.kernel_path() == path
    for lo in (0, 100 - T):
        c.launch([t[lo:lo + T] for t in tops])
        got = c.result().below
        print(path, lo, got.tolist())
        assert np.array_equal(got, np.tile(np.arange(lo, lo + T, dtype=np.uint64), (len(objs), 1))), (path, lo)


@pytest.mark.parametrize("kernel", [None, "generic"])
def test_counts_of_rank_ranges_add(gcp, kernel):
    """GCP n = 5 split at a rank that is no multiple of 64 and at one inside the last wavefront of
    the range: the parts' counts and valid counts sum to the whole's; an empty range counts nothing."""
    p, dp, _ = gcp
    lists, valid = full_order(gcp, 5)
    total = len(lists[1])
    srv = np.arange(p.R, dtype=np.uint32)
    thr = [thresholds_of(lst, kind) for lst, (kind, _) in zip(lists, OBJS)]
    c = Census(dp, srv, srv, 5, OBJS, DEFAULT_RANKING, kernel=kernel)
    c.launch(thr)
    whole = c.result()
    cuts = [0, 1000, total - 10, total]
    assert cuts[1] % 64 and total - cuts[2] < 64
    parts = []
    for rb, re in zip(cuts, cuts[1:]):
        c.launch(thr, rb, re)
        parts.append(c.result())
    assert np.array_equal(sum(r.below for r in parts), whole.below)
    assert sum(r.valid for r in parts) == whole.valid == valid
    # the first part against the oracle: the list's records below the cut, in order
    first = np.array([[below([x for x in lst if x[1] < cuts[1]], t) for t in row] for lst, row in zip(lists, thr)],
                     dtype=np.uint64)
    assert np.array_equal(parts[0].below, first)
    c.launch(thr, 777, 777)
    empty = c.result()
    assert empty.valid == 0 and not empty.below.any()


def count_below(keys, thr):
    """Configs r with (keys[r], r) < thr, from per-rank keys."""
    k, r = np.uint64(thr[0]), thr[1]
    ranks = np.arange(len(keys), dtype=np.uint64)
    return int(np.count_nonzero((keys < k) | ((keys == k) & (ranks < np.uint64(min(r, U64))))))


def test_deferred_configs_are_counted_by_the_fix_up():
    """The twin planet of tests/test_gpu_tail.py (synthetic R = 32, regions 4 and 5 at 200 from all
    others and 50 from each other), n = 4 in full (35,960 configs), forced fast: the 435 configs
    holding both twins tie on the leader's COV exactly, so the fast kernel defers them and the
    generic kernel's census variant counts them from the queue.  Thresholds include the records of
    twin-holding configs.  Counts equal the forced-generic census's and, for the MEAN objectives,
    those built from the oracle's per-client values."""
    base = Planet.synthetic(32)
    lat = base.lat.astype(np.int64).copy()
    for t in (4, 5):
        lat[t, :] = 200
        lat[:, t] = 200
    lat[4, 4] = lat[5, 5] = 0
    lat[4, 5] = lat[5, 4] = 50
    p = Planet(base.names, lat)
    dp, o = DevicePlanet(p), O.OraclePlanet.of(p)
    srv = np.arange(32, dtype=np.uint32)
    objs = [(SCORE, 0), (MEAN, AF1), (MEAN, FF1), (COV, AF1), (MEAN, E)]
    pos = colex_positions(32, 4)
    total = len(pos)
    twins = [r for r, c in enumerate(pos.tolist()) if 4 in c and 5 in c]
    assert total == 35960 and len(twins) == 435
    vals, _ = o.compute_stats(srv[pos], srv, threads=8)
    keys = {o_: key_of(MEAN, slot_values(vals, slot, 32, 4)) for o_, (kind, slot) in enumerate(objs) if kind == MEAN}
    # SCORE and COV thresholds: records of the generic sweep's lists
    sw = Sweep(dp, srv, srv, 4, objs, K=100, ranking=DEFAULT_RANKING, kernel="generic")
    sw.launch()
    tops = sw.result().tops
    picks = [twins[0], twins[217], twins[434], 0, total // 2, total - 1]
    thr = []
    for o_, (kind, _) in enumerate(objs):
        if kind == MEAN:
            thr.append(sorted((int(keys[o_][r]), r) for r in picks))
        else:
            t = tops[o_]
            k = t[len(t) // 2][0]
            thr.append(sorted([t[0], t[len(t) // 2], t[-1], (k, 0), (k, U64), (U64, U64)]))
    got = {}
    for kernel in ("fast", "generic"):
        c = Census(dp, srv, srv, 4, objs, DEFAULT_RANKING, kernel=kernel)
        assert c.kernel_path() == kernel
        c.launch(thr)
        got[kernel] = c.result()
        if kernel == "fast":
            assert 435 <= c.deferred() < total
        else:
            assert c.deferred() == 0
    print(got["fast"].below.tolist(), got["fast"].valid)
    assert got["fast"].valid == got["generic"].valid
    assert np.array_equal(got["fast"].below, got["generic"].below)
    for o_, k in keys.items():
        assert got["fast"].below[o_].tolist() == [count_below(k, t) for t in thr[o_]], objs[o_]
    # the SCORE and COV lists' own records: their indices
    for o_, (kind, _) in enumerate(objs):
        if kind != MEAN:
            t = tops[o_]
            idx = {t[0]: 0, t[len(t) // 2]: len(t) // 2, t[-1]: len(t) - 1}
            for j, x in enumerate(thr[o_]):
                if x in idx:
                    assert int(got["fast"].below[o_, j]) == idx[x], (objs[o_], x)


def test_overflowed_queue_counts_the_range_once():
    """Planet.equidistant(7, 48), n = 5: every one of the 1,712,304 configs defers, the queue
    overflows, the fast pass's counts are discarded on the device and the generic kernel counts the
    range.  Every config has the key the oracle gives for rank 0, so (k, r) has exactly r configs
    before it, (k + 1, 0) all of them and (k, 0) none: a config counted twice shows."""
    _, p = Planet.equidistant(7, 48)
    dp, o = DevicePlanet(p), O.OraclePlanet.of(p)
    srv = np.arange(48, dtype=np.uint32)
    objs = [(MEAN, AF1), (MEAN, FF1)]
    total = math.comb(48, 5)
    vals, _ = o.compute_stats(srv[:5].reshape(1, 5), srv)
    ks = [int(key_of(MEAN, slot_values(vals, slot, 48, 5))[0]) for _, slot in objs]
    ranks = [0, 1, 12345, 1 << 20, total - 1]
    c = Census(dp, srv, srv, 5, objs, DEFAULT_RANKING, kernel="fast")
    assert c.kernel_path() == "fast" and c.total == total
    c.launch([[(k, r) for r in ranks] + [(k + 1, 0), (U64, U64)] for k in ks])
    res = c.result()
    print(res.below.tolist(), c.deferred())
    assert c.deferred() == total
    assert res.below.tolist() == [ranks + [total, total]] * 2


def test_position_of_and_quantiles(gcp):
    """GCP n = 5 against the oracle's order: a config's position is its record's index in each
    list (None for SCORE when it is not valid), and the quantile at q is the key of the record at
    index ceil(q population) - 1: q = 1.0 (the last record), a q inside a group of tied keys, and
    small and middle ones."""
    p, dp, _ = gcp
    lists, valid = full_order(gcp, 5)
    total = len(lists[1])
    srv = np.arange(p.R, dtype=np.uint32)
    c = Census(dp, srv, srv, 5, OBJS, DEFAULT_RANKING)
    scored = {r for _, r in lists[0]}
    invalid = next(r for r in range(total) if r not in scored)
    for rank in (lists[0][0][1], lists[0][len(lists[0]) // 2][1], invalid, 0, total - 1):
        got = c.position_of(_lib.colex_unrank(rank, 5, p.R))
        want = []
        for o_, lst in enumerate(lists):
            at = [i for i, x in enumerate(lst) if x[1] == rank]
            want.append((at[0] if at else None, valid if o_ == 0 else total))
        assert got == want, rank
    assert c.position_of(_lib.colex_unrank(invalid, 5, p.R))[0] == (None, valid)
    # a q that lands inside a tie group of MEAN af1: the middle of its longest run of equal keys
    keys1 = [k for k, _ in lists[1]]
    run_key = max(set(keys1), key=keys1.count)
    lo, hi = keys1.index(run_key), keys1.index(run_key) + keys1.count(run_key)
    assert hi - lo >= 3
    q_tie = ((lo + hi) // 2 + 0.5) / total
    qs = [0.01, 0.5, q_tie, 0.99, 1.0]
    got = c.quantiles(qs)
    for o_, lst in enumerate(lists):
        want = [lst[math.ceil(Fraction(q) * len(lst)) - 1][0] for q in qs]
        assert got[o_] == want, OBJS[o_]
    assert got[1][2] == run_key and [g[-1] for g in got] == [lst[-1][0] for lst in lists]


def test_cli_prints_positions_and_quantiles(gcp):
    """`census --n 5 --config ... --quantiles ...` on GCP: one JSON line whose positions,
    populations and quantile keys are the oracle's (default objectives)."""
    import io
    import json

    from fantoch_amd import cli

    p, _, _ = gcp
    lists, valid = full_order(gcp, 5)
    total = len(lists[1])
    # the default five are OBJS without COV ff1C
    mine = [lists[OBJS.index(o_)] for o_ in DEFAULT_OBJECTIVES]
    rank = lists[0][3][1]
    names = [p.names[i] for i in _lib.colex_unrank(rank, 5, p.R)]
    out = io.StringIO()
    assert cli.main(["census", "--n", "5", "--config", ",".join(reversed(names)), "--quantiles", "0.25,1.0"], out=out) == 0
    lines = out.getvalue().strip().splitlines()
    assert len(lines) == 1
    doc = json.loads(lines[0])
    assert (doc["regions"], doc["n"], doc["configs"], doc["kernel"], doc["config"]) == (p.R, 5, total, "fast", names)
    assert [o_["objective"] for o_ in doc["objectives"]] == ["score", "mean:af1", "mean:ff1", "cov:af1", "mean:e"]
    for o_, lst in zip(doc["objectives"], mine):
        at = [i for i, x in enumerate(lst) if x[1] == rank][0]
        assert (o_["position"], o_["population"], o_["share"]) == (at, len(lst), at / len(lst))
        want = [lst[math.ceil(Fraction(q) * len(lst)) - 1][0] for q in (0.25, 1.0)]
        assert [int(k["key"]) for k in o_["quantile_keys"]] == want
    assert doc["objectives"][0]["position"] == 3 and doc["objectives"][0]["population"] == valid
    assert doc["objectives"][1]["quantile_keys"][1]["sum"] == mine[1][-1][0]


def test_handle_outlives_the_planet_and_relaunches_with_another_t(gcp):
    """One handle launched with T = 3, 16 and 1 in turn gives each launch's own counts; a census
    may be destroyed after its planet, launched or not."""
    p, _, _ = gcp
    lists, valid = full_order(gcp, 3)
    srv = np.arange(p.R, dtype=np.uint32)
    dp = DevicePlanet(p)
    c = Census(dp, srv, srv, 3, OBJS, DEFAULT_RANKING)
    idle = Census(dp, srv, srv, 3, OBJS, DEFAULT_RANKING, kernel="generic")
    full = [thresholds_of(lst, kind) for lst, (kind, _) in zip(lists, OBJS)]
    for t in (3, T, 1):
        thr = [row[-t:] for row in full]
        c.launch(thr)
        res = c.result()
        assert res.below.shape == (len(OBJS), t) and res.valid == valid
        assert res.below.tolist() == [[below(lst, x) for x in row] for lst, row in zip(lists, thr)], t
    c.launch(full)  # (no result call: destroy waits for the launch)
    lib = _lib.lib()
    assert lib.bote_planet_destroy(dp.h) == 0
    dp.h = None
    for h in (c, idle):
        assert lib.bote_census_destroy(h.h) == 0
        h.h = None
