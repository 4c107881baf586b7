"""Streaming evolving search on the device: bounded pinned batches
(PinnedBatch with prev_sums, bote_batch_create_bounded) and the beam driver on
top (fantoch_amd.evolve.Evolve, `python -m fantoch_amd evolve`).

Every expected value comes from the CPU oracle: a bounded set's SCORE list and
valid count are `sweep_ranks` over the supersets that pass Search::
min_mean_decrease, the predicate computed here in f64 from the oracle's
compute_stats sums; its MEAN and COV lists and its digest are `sweep_ranks` over
all supersets.  The driver is compared with the reference's chains
(tests/golden/chains.json) and with a restatement over the oracle's scores.
Every comparison is exact equality."""
import io
import itertools
import json
import math
import os

import numpy as np
import pytest

import oracle as O
from fantoch_amd import _lib, cli
from fantoch_amd.bote import (DEFAULT_OBJECTIVES, DEFAULT_RANKING, DevicePlanet, FTMetric, PinnedBatch, RankingParams,
                              Sweep, eval_configs)
from fantoch_amd.evolve import Evolve
from fantoch_amd.planet import Planet

pytestmark = pytest.mark.gpu

K = 100
NO_BOUND = 0xFFFFFFFF
END = 1 << 27
AF1, AF2 = 0, 2
CHAINS = json.load(open(os.path.join(os.path.dirname(__file__), "golden", "chains.json")))


def colex(c):
    return sum(math.comb(x, j + 1) for j, x in enumerate(c))


def supersets(ns, n, pinned):
    """The n-supersets of `pinned` among ns positions sorted by full colex rank, and those ranks."""
    free = [x for x in range(ns) if x not in pinned]
    cfgs = [tuple(sorted(set(pinned) | set(c))) for c in itertools.combinations(free, n - len(pinned))]
    cfgs.sort(key=colex)
    return np.array(cfgs, dtype=np.uint32), np.array([colex(c) for c in cfgs], dtype=np.uint64)


def ranking(rp, ft=FTMetric.F1F2):
    return RankingParams(float(rp[0]), float(rp[1]), float(rp[2]), float(rp[3]), 3, 13, ft)


def atlas_sums(o, srv, cli_, cfgs, threads=8):
    """(ncfg, 2) exact sums of the Atlas Input slots (f = 1, 2) from the oracle's per-client values."""
    nc = len(cli_)
    vals, _ = o.compute_stats(srv[np.asarray(cfgs, dtype=np.uint32)], cli_, threads=threads)
    return np.stack([vals[:, AF1 * nc:(AF1 + 1) * nc].sum(axis=1), vals[:, AF2 * nc:(AF2 + 1) * nc].sum(axis=1)], axis=1)


def passes(prev, sums, nc, dec, fs):
    """Search::min_mean_decrease per config: for f in fs, fl(prev_f / nc) - fl(S1_f / nc) >= dec."""
    ok = np.ones(len(sums), dtype=bool)
    for f in fs:
        ok &= np.float64(prev[f - 1]) / np.float64(nc) - sums[:, f - 1].astype(np.float64) / np.float64(nc) >= \
            np.float64(dec)
    return ok


def want_bounded(o, srv, cli_, n, ns, pinned, prev, rp, ft, objs=DEFAULT_OBJECTIVES, k=K, threads=8, sums=None):
    """The oracle's result of one bounded set: (tops, valid, digest), and the pass mask
    (sums: the supersets' atlas_sums, when the caller has them)."""
    cfgs, ranks = supersets(ns, n, [int(x) for x in pinned])
    sums = atlas_sums(o, srv, cli_, cfgs, threads) if sums is None else sums
    ok = passes(prev, sums, len(cli_), rp[3], FTMetric(ft).fs(n - 2))
    tops_all, _, digest = o.sweep_ranks(srv, cli_, n, ranks, objs, k, tuple(rp), ft, threads)
    tops = [list(t) for t in tops_all]
    valid = 0
    for i, (kind, _) in enumerate(objs):
        if kind == _lib.OBJ_SCORE:
            tops[i] = []
    if ok.any():
        tp, valid, _ = o.sweep_ranks(srv, cli_, n, ranks[ok], objs, k, tuple(rp), ft, threads)
        for i, (kind, _) in enumerate(objs):
            if kind == _lib.OBJ_SCORE:
                tops[i] = list(tp[i])
    return (tops, valid, digest), ok


def launched(b):
    b.launch()
    return [(r.tops, r.valid, r.digest) for r in b.result()]


def device_sums(dp, srv, cli_, n, sets):
    return eval_configs(dp, srv, cli_, n, configs=np.asarray(sets, dtype=np.uint32), values=False).s1[:, [AF1, AF2]]


@pytest.fixture(scope="module")
def gcp():
    p = Planet.new()
    return p, DevicePlanet(p), O.OraclePlanet.of(p), np.arange(p.R, dtype=np.uint32)


def best_sets(dp, srv, n, count):
    sw = Sweep(dp, srv, srv, n, DEFAULT_OBJECTIVES, K=K, ranking=DEFAULT_RANKING, digest=True)
    sw.launch()
    recs = sw.result().tops[0][:count]
    assert len(recs) == count
    return [[int(x) for x in _lib.colex_unrank(int(r), n, len(srv))] for _, r in recs]


# --------------------------------------------------------------------- 1 ---
def test_bounded_batch_against_the_oracle(gcp):
    """GCP n = 5 over the first 40 SCORE records of the n = 3 sweep (136 supersets per
    set), default ranking: f = 1 only (fs(3)), the AF2 word reads no bound."""
    p, dp, o, srv = gcp
    rp = (110.0, 35.0, 0.0, 15.0)
    sets = best_sets(dp, srv, 3, 40)
    prev = device_sums(dp, srv, srv, 3, sets)
    assert np.array_equal(prev[:, 0], atlas_sums(o, srv, srv, sets)[:, 0])
    prev[:, 1] = 0  # (n = 3 has no f = 2 slot)
    want = [want_bounded(o, srv, srv, 5, p.R, s, prev[i], rp, 2) for i, s in enumerate(sets)]
    assert any(0 < ok.sum() < len(ok) for _, ok in want)  # the limit rejects part of some set
    assert any(w[1] < o.sweep_ranks(srv, srv, 5, supersets(p.R, 5, s)[1], DEFAULT_OBJECTIVES, K, rp, 2, 8)[1]
               for (w, _), s in zip(want[:8], sets[:8]))  # ... and valid configs among them
    got = {}
    for kernel in (None, "fast", "generic"):
        b = PinnedBatch(dp, srv, srv, 5, sets, DEFAULT_OBJECTIVES, K=K, ranking=DEFAULT_RANKING, digest=True,
                        kernel=kernel, prev_sums=prev)
        assert b.kernel_path() == ("generic" if kernel == "generic" else "fast") and b.total == 136
        lim = b.limits()
        assert lim.shape == (40, 2) and np.all(lim[:, 1] == NO_BOUND)
        assert lim[:, 0].tolist() == [_lib.mean_decrease_limit(int(x), p.R, 15.0) for x in prev[:, 0]]
        got[kernel] = launched(b)
        for i, s in enumerate(sets):
            assert got[kernel][i] == want[i][0], (kernel, s)
    assert got[None] == got["fast"] == got["generic"]


# --------------------------------------------------------------------- 2 ---
@pytest.mark.parametrize("ft", [FTMetric.F1F2, FTMetric.F1])
def test_both_f_terms(gcp, ft):
    """GCP n = 7 over the first 32 SCORE records of the n = 5 sweep (105 supersets per
    set): f = 2 is in fs(5) under F1F2.  Some set has valid supersets that pass the AF1
    limit and that the AF2 limit alone rejects.  Under F1 the AF2 word reads no bound."""
    p, dp, o, srv = gcp
    rp = (110.0, 35.0, 0.0, 15.0)
    sets = best_sets(dp, srv, 5, 32)
    prev = device_sums(dp, srv, srv, 5, sets)
    assert np.array_equal(prev, atlas_sums(o, srv, srv, sets))
    want = [want_bounded(o, srv, srv, 7, p.R, s, prev[i], rp, ft.value) for i, s in enumerate(sets)]
    if ft is FTMetric.F1F2:
        only_af2 = []
        for i, s in enumerate(sets):
            cfgs, _ = supersets(p.R, 7, s)
            sums = atlas_sums(o, srv, srv, cfgs)
            _, valid = o.scores(srv[cfgs], srv, rp, 2)
            ok1 = passes(prev[i], sums, p.R, 15.0, [1])
            ok2 = np.float64(prev[i][1]) / np.float64(p.R) - sums[:, 1].astype(np.float64) / np.float64(p.R) >= 15.0
            if (valid.astype(bool) & ok1 & ~ok2).any():
                only_af2.append(i)
        assert only_af2, "no set whose valid supersets only the AF2 limit rejects"
        for i in only_af2:  # the AF2 limit shows in the result
            assert want[i][0][1] < int((o.scores(srv[supersets(p.R, 7, sets[i])[0]], srv, rp, 2)[1]).sum())
    for kernel in (None, "generic"):
        b = PinnedBatch(dp, srv, srv, 7, sets, DEFAULT_OBJECTIVES, K=K, ranking=ranking(rp, ft), digest=True,
                        kernel=kernel, prev_sums=prev)
        lim = b.limits()
        if ft is FTMetric.F1:
            assert np.all(lim[:, 1] == NO_BOUND) and np.all(lim[:, 0] < END)
        else:
            assert lim.tolist() == [[_lib.mean_decrease_limit(int(x), p.R, 15.0) for x in row] for row in prev]
        got = launched(b)
        for i, s in enumerate(sets):
            assert got[i] == want[i][0], (kernel, ft, s)


# --------------------------------------------------------------------- 3 ---
def test_edges_of_the_limit(gcp):
    p, dp, o, srv = gcp
    base = best_sets(dp, srv, 3, 1)[0]
    cfgs, ranks = supersets(p.R, 5, base)
    sums = atlas_sums(o, srv, srv, cfgs)
    objs = DEFAULT_OBJECTIVES

    def run(prev_af1, dec, kernel=None):
        rp = (110.0, 35.0, 0.0, dec)
        b = PinnedBatch(dp, srv, srv, 5, [base], objs, K=K, ranking=ranking(rp), digest=True, kernel=kernel,
                        prev_sums=[[prev_af1, 0]])
        return b, launched(b)[0], want_bounded(o, srv, srv, 5, p.R, base, [prev_af1, 0], rp, 2)[0]

    plain = PinnedBatch(dp, srv, srv, 5, [base], objs, K=K, ranking=DEFAULT_RANKING, digest=True)
    assert np.all(plain.limits() == NO_BOUND)
    unbounded = launched(plain)[0]
    tops_all, valid_all, digest_all = o.sweep_ranks(srv, srv, 5, ranks, objs, K, (110.0, 35.0, 0.0, 15.0), 2, 8)
    assert unbounded == ([list(t) for t in tops_all], valid_all, digest_all)  # unchanged from today
    # a decrease of 0 from X's own sum: X passes (equal means), a larger sum does not
    score_ranks = [r for _, r in unbounded[0][0]]
    assert unbounded[1] == len(score_ranks) < K  # (the list holds every valid superset)
    by_rank = {int(r): int(s) for r, s in zip(ranks, sums[:, 0])}
    xr = sorted(score_ranks, key=lambda r: by_rank[r])[len(score_ranks) // 2]
    larger = [r for r in score_ranks if by_rank[r] > by_rank[xr]]
    assert larger and any(by_rank[r] < by_rank[xr] for r in score_ranks)
    for kernel in (None, "generic"):
        b, got, want = run(by_rank[xr], 0.0, kernel)
        assert b.limits().tolist() == [[by_rank[xr] + 1, NO_BOUND]]
        assert got == want
        listed = {r for _, r in got[0][0]}
        assert xr in listed and not (listed & set(larger))
        assert got[1] == sum(1 for r in score_ranks if by_rank[r] <= by_rank[xr]) == len(listed)
    # nothing passes: no valid config, an empty SCORE list, everything else as without the bound
    for kernel in (None, "generic"):
        b, got, want = run(0, 15.0, kernel)
        assert b.limits().tolist() == [[0, NO_BOUND]]
        assert got == want and got[1] == 0 and got[0][0] == []
        assert got[0][1:] == unbounded[0][1:] and got[2] == unbounded[2]
    # a huge previous sum within range: every config passes
    b, got, want = run(END - 1, 15.0)
    assert b.limits()[0, 0] > int(sums[:, 0].max())
    assert got == want == unbounded
    with pytest.raises(_lib.BoteError, match=r"pinned set 0: previous sum must be below 2\^27"):
        run(END, 15.0)
    with pytest.raises(_lib.BoteError, match="a bounded batch needs ranking params"):
        PinnedBatch(dp, srv, srv, 5, [base], [(_lib.OBJ_MEAN, AF1)], K=K, ranking=None, prev_sums=[[5, 5]])


# --------------------------------------------------------------------- 4 ---
def test_sliced_sets():
    """Synthetic R = 64, n = 5, four sets of 2: C(62, 3) = 37,820 supersets each, cut
    into slices; each set's limit is its own (the median AF1 sum of its supersets)."""
    p = Planet.synthetic(64)
    dp, o = DevicePlanet(p), O.OraclePlanet.of(p)
    srv = np.arange(64, dtype=np.uint32)
    rp = (110.0, 35.0, 0.0, 15.0)
    sets = [[0, 63], [17, 30], [5, 6], [44, 2]]
    prev, sums = [], []
    for s in sets:
        sums.append(atlas_sums(o, srv, srv, supersets(64, 5, s)[0], threads=16))
        prev.append([int(np.median(sums[-1][:, 0])) + 15 * 64, 0])
    b = PinnedBatch(dp, srv, srv, 5, sets, DEFAULT_OBJECTIVES, K=K, ranking=DEFAULT_RANKING, digest=True,
                    prev_sums=prev)
    slices, units, _ = b.plan()
    assert b.kernel_path() == "fast" and b.total == 37820 and 1 < slices <= 7 and units == 4 * slices
    got = launched(b)
    for i, s in enumerate(sets):
        want, ok = want_bounded(o, srv, srv, 5, 64, s, prev[i], rp, 2, threads=16, sums=sums[i])
        assert 0 < ok.sum() < len(ok)
        assert got[i] == want, s


# --------------------------------------------------------------------- 5 ---
def test_deferral_recompute_carries_the_limits():
    """The twin planet of test_deferred_configs_that_belong_to_two_sets (synthetic R =
    32, regions 4 and 5 at 200 from all others and 50 from each other), n = 4, sets [4],
    [5], [6], limits that reject part of each set: the batch defers configs, so every
    set is recomputed on the generic kernel, with its limits.  Ranking (10, 5, 0, 5):
    set [6] then has 601 valid supersets, 194 of them under its limit (no superset of a
    twin is valid under any ranking)."""
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
    rp = (10.0, 5.0, 0.0, 5.0)
    sets = [[4], [5], [6]]
    prev = []
    for s in sets:
        sums = atlas_sums(o, srv, srv, supersets(32, 4, s)[0])
        prev.append([int(np.median(sums[:, 0])) + 5 * 32, 0])
    b = PinnedBatch(dp, srv, srv, 4, sets, DEFAULT_OBJECTIVES, K=K, ranking=ranking(rp), digest=True,
                    kernel="fast", prev_sums=prev)
    assert b.kernel_path() == "fast" and b.total == 4495
    got = launched(b)
    assert b.deferred() > 0
    for i, s in enumerate(sets):
        want, ok = want_bounded(o, srv, srv, 4, 32, s, prev[i], rp, 2)
        assert 0 < ok.sum() < len(ok)
        assert got[i] == want, s
    assert got[2][1] == 194 and len(got[2][0][0]) == K


# --------------------------------------------------------------------- 6 ---
def case_lists(p, case):
    regions = cli.REGIONS13 if case["input"] == "R13C13" else p.names
    return np.array(sorted(p.index[r] for r in regions), dtype=np.uint32)


def names_of(p, res, chain):
    return [sorted(p.names[i] for i in ids) for ids in res.configs_of(chain)]


@pytest.mark.parametrize("case,nchains", [("R13C13_0", 27), ("R13C13_1", 36), ("R13C13_2", 6270), ("R20C20_0", 6110)])
def test_exhaustive_search_equals_the_reference_chains(gcp, case, nchains):
    p, dp, _, _ = gcp
    c = CHAINS["cases"][case]
    assert c["nchains"] == nchains
    srv = case_lists(p, c)
    res = Evolve(dp, srv, srv, ranking(c["params"]), beam=None, K=100).run()
    assert res.exhaustive
    assert len(res.chains) == nchains
    gold = c["chains"][:50]
    m = len(gold)
    assert [s for s, _ in res.chains[:m]] == [g[0] for g in gold]  # (== on floats: bit-equal but for the zeros' sign)
    assert np.array_equal(res.scores[:m].view(np.uint64), np.array([g[0] for g in gold], np.float64).view(np.uint64))
    # runs of equal scores wholly inside the fixture's chains: the same sets of chains
    i = 0
    while i < m:
        j = i
        while j < m and gold[j][0] == gold[i][0]:
            j += 1
        if j < m or m == nchains:
            mine = sorted(names_of(p, res, ch) for ch in res.chains[i:j])
            assert mine == sorted([sorted(lv) for lv in g[1]] for g in gold[i:j]), (case, i, j)
        i = j
    assert [lv.n for lv in res.levels] == [3, 5, 7, 9, 11, 13] and res.levels[-1].chains == nchains
    assert all(lv.batches == -(-lv.frontier // 1024) for lv in res.levels)


# --------------------------------------------------------------------- 7 ---
def restated(o, srv, cl, rp, ft, levels, k, beam):
    """The driver's rules over the oracle's tables of every C(ns, n) configs: the K best
    valid configs at the first level, then per distinct chain end its K best valid
    supersets that pass min_mean_decrease, lists ordered by (score descending, colex rank);
    chains scored by the left-to-right f64 sum, ordered by (score descending, ranks), the
    `beam` best kept after each level."""
    ns, nc, dec = len(srv), len(cl), np.float64(rp[3])
    tabs = {}
    for n in levels:
        cfgs = np.array(sorted(itertools.combinations(range(ns), n), key=colex), dtype=np.uint32)
        score, valid = o.scores(srv[cfgs], cl, tuple(rp), ft)
        tabs[n] = {"sets": [frozenset(c) for c in cfgs.tolist()], "ranks": [colex(c) for c in cfgs.tolist()],
                   "score": score, "valid": valid, "s": atlas_sums(o, srv, cl, cfgs)}

    def select(ch):
        ch = sorted(ch, key=lambda c: (-c[0], c[1]))
        return ch[:beam], len(ch) > beam

    t = tabs[levels[0]]
    first = sorted((i for i in range(len(t["ranks"])) if t["valid"][i]), key=lambda i: (-t["score"][i], t["ranks"][i]))
    exhaustive = len(first) <= k
    chains, cut = select([(np.float64(t["score"][i]), (t["ranks"][i],), i) for i in first[:k]])
    exhaustive = exhaustive and not cut
    for pn, n in zip(levels, levels[1:]):
        q, t = tabs[pn], tabs[n]
        ext = {}
        for e in sorted({c[2] for c in chains}):
            ok = [i for i in range(len(t["ranks"])) if t["valid"][i] and q["sets"][e] <= t["sets"][i] and all(
                np.float64(q["s"][e][f - 1]) / np.float64(nc) - np.float64(t["s"][i][f - 1]) / np.float64(nc) >= dec
                for f in FTMetric(ft).fs(pn))]
            ok.sort(key=lambda i: (-t["score"][i], t["ranks"][i]))
            exhaustive = exhaustive and len(ok) < k
            ext[e] = ok[:k]
        chains, cut = select([(c[0] + np.float64(t["score"][i]), c[1] + (t["ranks"][i],), i)
                              for c in chains for i in ext[c[2]]])
        exhaustive = exhaustive and not cut
    return [(float(c[0]), list(c[1])) for c in chains], exhaustive


def test_a_cutting_beam(gcp):
    """R13C13 at (10, 5, 0, 5), beam = 64, K = 8: lists come back full and the beam cuts."""
    p, dp, o, _ = gcp
    c = CHAINS["cases"]["R13C13_2"]
    assert c["params"] == [10.0, 5.0, 0.0, 5.0]
    srv = case_lists(p, c)
    want, want_exhaustive = restated(o, srv, srv, c["params"], 2, [3, 5, 7, 9, 11, 13], 8, 64)
    res = Evolve(dp, srv, srv, ranking(c["params"]), beam=64, K=8).run()
    assert not res.exhaustive and not want_exhaustive
    assert 0 < len(want) <= 64
    assert res.chains == want
    assert np.array_equal(res.scores.view(np.uint64), np.array([s for s, _ in want], np.float64).view(np.uint64))
    assert max(lv.chains for lv in res.levels) <= 64 and max(lv.frontier for lv in res.levels) <= 64


# --------------------------------------------------------------------- 8 ---
def test_cli_prints_the_best_chain():
    out = io.StringIO()
    assert cli.main(["evolve", "--input", "R13C13"], out) == 0
    lines = out.getvalue().splitlines()
    best = CHAINS["cases"]["R13C13_0"]["chains"][0]
    assert cli.rust_f64(best[0]).startswith("10360.3")
    assert f"score: {cli.rust_f64(best[0])}" in lines
    at = lines.index(f"score: {cli.rust_f64(best[0])}")
    assert lines[at + 1:at + 7] == [f"n={len(lv)}: " + ",".join(sorted(lv)) for lv in best[1]]
    assert "chains: 27" in lines
    assert any(ln.startswith("exhaustive: yes") for ln in lines)
    out = io.StringIO()
    assert cli.main(["evolve", "--input", "R13C13", "--ranking", "10,5,0,5", "--beam", "64", "-K", "8"], out) == 0
    assert any(ln.startswith("exhaustive: no") for ln in out.getvalue().splitlines())
