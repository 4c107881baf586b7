"""Batched pinned sweeps (bote_batch_*, PinnedBatch): many pinned sets swept by
one launch of the fast kernel's batch variant, or set by set on the generic
kernel.

Every expected value comes from the CPU oracle over `supersets(ns, n, pinned)`:
the supersets sorted by full colex rank, built with itertools and math.comb
(never with the library's unranking).  Every comparison is exact equality, and
every set of a batch is compared."""
import io
import itertools
import json
import math
import random

import numpy as np
import pytest

import oracle as O
from fantoch_amd import _lib, cli
from fantoch_amd.bote import DEFAULT_OBJECTIVES, DEFAULT_RANKING, DevicePlanet, PinnedBatch, Sweep
from fantoch_amd.planet import Planet

pytestmark = pytest.mark.gpu

K = 100
RP = (110.0, 35.0, 0.0, 15.0)
MEAN, MAX, MDTM, P95 = _lib.OBJ_MEAN, _lib.OBJ_MAX, _lib.OBJ_MDTM, _lib.OBJ_PCTL(9500)
AF1, FF1 = 0, 1


def colex(c):
    return sum(math.comb(x, j + 1) for j, x in enumerate(c))


def supersets(ns, n, pinned):
    """The n-supersets of `pinned` among ns positions sorted by full colex rank, and those ranks."""
    free = [x for x in range(ns) if x not in pinned]
    cfgs = [tuple(sorted(set(pinned) | set(c))) for c in itertools.combinations(free, n - len(pinned))]
    cfgs.sort(key=colex)
    return np.array(cfgs, dtype=np.uint32), np.array([colex(c) for c in cfgs], dtype=np.uint64)


def oracle_lists(o, srv, cli_, n, ranks, objs=DEFAULT_OBJECTIVES, k=K, threads=8):
    tops, valid, digest = o.sweep_ranks(srv, cli_, n, ranks, objs, k, RP, 2, threads)
    return [list(t) for t in tops], valid, digest


def batch(dp, srv, cli_, n, sets, kernel=None, objs=DEFAULT_OBJECTIVES, ranking=DEFAULT_RANKING, digest=True, k=K,
          max_blocks=0):
    return PinnedBatch(dp, srv, cli_, n, sets, objs, K=k, ranking=ranking, digest=digest, kernel=kernel,
                       max_blocks=max_blocks)


def launched(b):
    b.launch()
    return [(r.tops, r.valid, r.digest) for r in b.result()]


def single(dp, srv, cli_, n, pinned, kernel=None, objs=DEFAULT_OBJECTIVES, ranking=DEFAULT_RANKING, digest=True, k=K,
           rb=0, re=None):
    sw = Sweep(dp, srv, cli_, n, objs, K=k, ranking=ranking, digest=digest, kernel=kernel, pinned=pinned)
    sw.launch(rb, re)
    r = sw.result()
    return r.tops, r.valid, r.digest


@pytest.fixture(scope="module")
def gcp():
    p = Planet.new()
    return p, DevicePlanet(p), O.OraclePlanet.of(p), np.arange(p.R, dtype=np.uint32)


def want_of(o, srv, cli_, n, ns, sets, cache=None, **kw):
    """The oracle's result per set (one oracle run per distinct set)."""
    cache = {} if cache is None else cache
    out = []
    for s in sets:
        key = tuple(sorted(int(x) for x in s))
        if key not in cache:
            cache[key] = oracle_lists(o, srv, cli_, n, supersets(ns, n, list(key))[1], **kw)
        out.append(cache[key])
    return out


# --------------------------------------------------------------------- 1 ---
def test_all_pairs_on_four_workgroups(gcp):
    """GCP R = 20, n = 3, every pair as a set (190 sets of 18 configs: fewer than a
    wave and than K), max_blocks = 4: a workgroup walks about 48 units, with a fresh
    top-K and the set's own counters for each."""
    p, dp, o, srv = gcp
    sets = [list(c) for c in itertools.combinations(range(p.R), 2)]
    assert len(sets) == 190
    want = want_of(o, srv, srv, 3, p.R, sets)
    assert all(len(w[0][1]) == 18 for w in want)  # (MEAN af1: every config)
    for kernel in (None, "fast"):
        b = batch(dp, srv, srv, 3, sets, kernel, max_blocks=4)
        assert b.kernel_path() == "fast" and b.total == 18
        assert b.plan() == (1, 190, 4)
        got = launched(b)
        assert len(got) == 190
        for i in range(190):
            assert got[i] == want[i], (kernel, sets[i])
        for _, r in got[7][0][1][:3]:  # records carry full colex ranks
            assert set(sets[7]) <= set(b.config_of(r))


# --------------------------------------------------------------------- 2 ---
def test_extend_the_best_of_the_last_level(gcp):
    """GCP n = 5 over the first 40 SCORE records of the n = 3 sweep (from_records):
    136 configs per set; equal to the oracle and to a single pinned sweep per set,
    whatever the order of the sets and of the positions within a set."""
    p, dp, o, srv = gcp
    sw3 = Sweep(dp, srv, srv, 3, DEFAULT_OBJECTIVES, K=K, ranking=DEFAULT_RANKING, digest=True)
    sw3.launch()
    recs = sw3.result().tops[0][:40]
    assert len(recs) == 40
    b = PinnedBatch.from_records(sw3, recs, 5)
    assert b.kernel_path() == "fast" and b.total == 136 and b.K == K and b.digest
    sets = b.pinned_sets.tolist()
    for s, (_, r) in zip(sets, recs):  # the sets are the records' configs (positions == ids here)
        assert colex(sorted(s)) == r and len(set(s)) == 3
    got = launched(b)
    want = want_of(o, srv, srv, 5, p.R, sets)
    for i, s in enumerate(sets):
        assert got[i] == want[i], s
        assert got[i] == single(dp, srv, srv, 5, s), s
    order = list(range(40))
    random.Random(5).shuffle(order)
    assert order != list(range(40))
    got2 = launched(batch(dp, srv, srv, 5, [sets[i][::-1] for i in order]))
    for j, i in enumerate(order):
        assert got2[j] == want[i], sets[i]


# --------------------------------------------------------------------- 3 ---
def test_equal_sets_give_equal_results(gcp):
    p, dp, o, srv = gcp
    sets = [[3, 9, 15], [15, 3, 9], [3, 9, 16]]
    got = launched(batch(dp, srv, srv, 7, sets))
    want = want_of(o, srv, srv, 7, p.R, sets)
    assert got[0] == got[1] and got[0] != got[2]
    for i in range(3):
        assert got[i] == want[i], sets[i]


# --------------------------------------------------------------------- 4 ---
@pytest.mark.parametrize("n,sets", [
    (9, [[0, 1, 2, 3, 4, 5, 6], [13, 14, 15, 16, 17, 18, 19], [0, 3, 6, 9, 12, 15, 18], [19, 1, 17, 3, 15, 5, 13],
         [2, 4, 6, 8, 10, 12, 14], [0, 1, 2, 17, 18, 19, 9], [5, 6, 7, 8, 9, 10, 11], [1, 2, 4, 8, 16, 3, 9]]),
    (13, [list(range(11)), list(range(9, 20)), [0, 2, 4, 6, 8, 10, 12, 14, 16, 18, 19],
          [19, 17, 15, 13, 11, 9, 7, 5, 3, 1, 0]]),
])
def test_the_non_pipelined_client_loop(gcp, n, sets):
    """N > 8: the client loop without the software pipeline."""
    p, dp, o, srv = gcp
    b = batch(dp, srv, srv, n, sets)
    assert b.kernel_path() == "fast"
    got = launched(b)
    want = want_of(o, srv, srv, n, p.R, sets)
    for i, s in enumerate(sets):
        assert got[i] == want[i], s


# --------------------------------------------------------------------- 5 ---
@pytest.mark.parametrize("kernel", ["fast", "generic"])
def test_lists_that_are_not_the_identity(gcp, kernel):
    """The 13 regions of the reference's main.rs as servers, clients 0..6 (one quad
    and a remainder of 3, a separate row table), n = 5."""
    p, dp, o, _ = gcp
    srv = np.array(sorted(p.index[r] for r in cli.REGIONS13), dtype=np.uint32)
    cl = np.arange(7, dtype=np.uint32)
    assert len(srv) == 13 and srv.tolist() != list(range(13))
    sets = [[2, 11], [0, 12], [5, 6]]
    b = batch(dp, srv, cl, 5, sets, kernel)
    assert b.kernel_path() == kernel
    got = launched(b)
    want = want_of(o, srv, cl, 5, 13, sets)
    for i, s in enumerate(sets):
        assert got[i] == want[i], s


# --------------------------------------------------------------------- 6 ---
@pytest.fixture(scope="module")
def r64():
    p = Planet.synthetic(64)
    return p, DevicePlanet(p), O.OraclePlanet.of(p), np.arange(64, dtype=np.uint32)


def test_synthetic_r64_n7(r64):
    """16 sets of 5 spread over [0, 63], one holding 0 and 63: 1,711 configs each."""
    p, dp, o, srv = r64
    rng = random.Random(64)
    sets = [[0, 17, 30, 44, 63]] + [rng.sample(range(64), 5) for _ in range(15)]
    assert {x for s in sets for x in s} >= {0, 63} and len({x for s in sets for x in s}) > 40
    b = batch(dp, srv, srv, 7, sets)
    assert b.kernel_path() == "fast" and b.total == 1711 and b.plan()[:2] == (1, 16)
    got = launched(b)
    want = want_of(o, srv, srv, 7, 64, sets, threads=16)
    for i, s in enumerate(sets):
        assert got[i] == want[i], s


def test_synthetic_r64_sliced_sets(r64):
    """n = 6, sets [5] and [63]: C(63, 5) = 7,028,847 configs per set, cut into
    slices.  The lists equal the single pinned sweeps' (that path equals the oracle
    at 35,990 configs, tests/test_gpu_pinned.py); around the first slice boundary
    the single sweep over 2 x 2,048 pinned ranks equals the oracle there, and the
    batch's records among those configs are the oracle's that reach its lists."""
    p, dp, o, srv = r64
    total = math.comb(63, 5)
    sets = [[5], [63]]
    b = batch(dp, srv, srv, 6, sets)
    slices, units, _ = b.plan()
    assert b.kernel_path() == "fast" and b.total == total and 1 < slices <= 7 and units == 2 * slices
    got = launched(b)
    for i, s in enumerate(sets):
        assert got[i] == single(dp, srv, srv, 6, s), s
    bound = -(-total // slices)  # the first slice's end
    lo, hi = bound - 2048, bound + 2048
    for i, s in enumerate(sets):
        free = [x for x in range(64) if x != s[0]]
        # pinned rank r is the colex rank of the free indices: colex order over [0, 63) is reverse
        # lexicographic order of the mirrored indices, so ranks [lo, hi) are one slice of itertools' order
        lex = itertools.islice(itertools.combinations(range(63), 5), total - hi, total - lo)
        cfgs = [tuple(sorted([s[0]] + [free[62 - y] for y in c])) for c in lex]
        ranks = np.array(sorted(colex(c) for c in cfgs), dtype=np.uint64)
        assert len(ranks) == 4096
        near = oracle_lists(o, srv, srv, 6, ranks, threads=16)
        assert single(dp, srv, srv, 6, s, rb=lo, re=hi) == near, s
        inside = set(ranks.tolist())
        for lst, nl in zip(got[i][0], near[0]):
            mine = [rec for rec in lst if rec[1] in inside]
            assert mine == [rec for rec in nl if len(lst) < K or rec <= lst[-1]], s


# --------------------------------------------------------------------- 7 ---
def test_deferred_configs_that_belong_to_two_sets():
    """The twin planet of test_deferred_configs_carry_full_ranks (synthetic R = 32,
    regions 4 and 5 at 200 from all others and 50 from each other), n = 4: the 435
    configs that hold both twins defer for set [4] and again for set [5] (and the 29
    with 6 for set [6]); the queue entries carry their set."""
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
    sets = [[4], [5], [6]]
    b = batch(dp, srv, srv, 4, sets, "fast")
    assert b.kernel_path() == "fast" and b.total == 4495
    got = launched(b)
    assert b.deferred() >= 2 * 435
    want = want_of(o, srv, srv, 4, 32, sets)
    for i, s in enumerate(sets):
        assert got[i] == want[i], s


# --------------------------------------------------------------------- 8 ---
def test_overflow_recomputes_every_set():
    """Planet.equidistant(7, 48), n = 6, sets [0] and [1]: every leader choice is an
    exact tie, so all 2 x 1,533,939 > 2^20 configs defer and the batch is recomputed
    set by set.  Each list is the first K supersets by full rank under the one key."""
    _, p = Planet.equidistant(7, 48)
    dp, o = DevicePlanet(p), O.OraclePlanet.of(p)
    srv = np.arange(48, dtype=np.uint32)
    objs = [(MEAN, AF1), (MEAN, FF1)]
    sets = [[0], [1]]
    b = batch(dp, srv, srv, 6, sets, "fast", objs, ranking=None, digest=False)
    assert b.kernel_path() == "fast" and b.total == 1533939
    got = launched(b)
    assert b.deferred() > 1 << 20
    for i, s in enumerate(sets):
        # colex order takes the largest member first: the first K supersets hold only low free positions
        free = [x for x in range(48) if x != s[0]][:12]
        first = sorted((tuple(sorted(s + list(c))) for c in itertools.combinations(free, 5)), key=colex)[:K]
        ranks = [colex(c) for c in first]
        assert ranks == sorted(ranks) and len(ranks) == K
        vals, _ = o.compute_stats(srv[np.array(first[:1], dtype=np.uint32)], srv)
        for (kind, slot), t in zip(objs, got[i][0]):
            key = int(vals[0, slot * 48:(slot + 1) * 48].sum())
            assert t == [(key, r) for r in ranks], (s, slot)


# --------------------------------------------------------------------- 9 ---
def key_of(kind, v):
    """Per-config key of one slot's values (ncfg, count); H by its definition."""
    v = np.asarray(v).astype(np.int64)
    c, s = v.shape[1], v.sum(axis=1)
    u = v.astype(np.uint64)
    if kind == MEAN:
        return s.astype(np.uint64)
    if kind == MDTM:
        h = np.maximum(c * v - s[:, None], 0).sum(axis=1)
        return (h.astype(np.uint64) << np.uint64(27)) | s.astype(np.uint64)
    if kind == MAX:
        return (u.max(axis=1) << np.uint64(32)) | s.astype(np.uint64)
    idx, whole = _lib.percentile_index(kind & 0xFFFF, c)
    a = np.sort(u, axis=1)
    twice = 2 * a[:, 0] if idx == 0 else a[:, idx - 1] + a[:, idx] if whole else 2 * a[:, idx - 1]
    return (twice << np.uint64(32)) | s.astype(np.uint64)


def test_tail_objectives_run_the_generic_kernel(gcp):
    p, dp, o, srv = gcp
    n, nc, sets = 5, p.R, [[0, 19], [3, 4]]
    objs = [(MEAN, AF1), (MAX, AF1), (P95, FF1), (MDTM, AF1)]
    b = batch(dp, srv, srv, n, sets, None, objs, ranking=None, digest=False)
    assert b.kernel_path() == "generic" and b.deferred() == 0
    got = launched(b)
    for i, s in enumerate(sets):
        cfgs, ranks = supersets(p.R, n, s)
        vals, _ = o.compute_stats(srv[cfgs], srv, threads=8)
        want = []
        for kind, slot in objs:
            keys = key_of(kind, vals[:, slot * nc:(slot + 1) * nc])
            order = np.lexsort((ranks, keys))[:K]
            want.append([(int(keys[j]), int(ranks[j])) for j in order])
        assert got[i][0] == want, s

    def plain_sweep_still_works():
        un = Sweep(dp, srv, srv, 3, [(MEAN, AF1)], K=K, ranking=None)
        un.launch()
        all3 = np.arange(math.comb(p.R, 3), dtype=np.uint64)
        assert un.result().tops == oracle_lists(o, srv, srv, 3, all3, [(MEAN, AF1)])[0]

    with pytest.raises(_lib.BoteError, match=r"the fast kernel's pinned variant computes SCORE, MEAN and COV "
                                             r"objectives \(generic kernel\)") as e:
        batch(dp, srv, srv, n, sets, "fast", objs, ranking=None, digest=False)
    assert e.value.code == -1
    plain_sweep_still_works()
    with pytest.raises(_lib.BoteError, match=r"the group kernel does not sweep pinned members "
                                             r"\(fast or generic kernel\)") as e:
        batch(dp, srv, srv, n, sets, "group", [(MEAN, AF1)], ranking=None, digest=False)
    assert e.value.code == -1
    plain_sweep_still_works()
    with pytest.raises(_lib.BoteError, match=r"pinned set 1: duplicate position"):
        batch(dp, srv, srv, n, [[0, 19], [3, 3]], None, objs, ranking=None, digest=False)


# -------------------------------------------------------------------- 10 ---
def test_cli_prints_one_block_per_set():
    def run(*flags):
        out = io.StringIO()
        assert cli.main(["sweep", "--n", "5", "--K", "20", "--show", "5", "--compact"] + list(flags), out) in (0, None)
        return out.getvalue().splitlines()

    blocks = run("--pinned-sets", "0,19;asia-east1,4")
    assert len(blocks) == 2
    assert blocks[0] == run("--pinned", "0,19")[0] and blocks[1] == run("--pinned", "asia-east1,4")[0]
    doc = json.loads(blocks[1])
    assert doc["configs"] == 816 and len(doc["pinned"]) == 2 and len(doc["objectives"][1]["top"]) == 5
    with pytest.raises(ValueError, match="exclude each other"):
        run("--pinned-sets", "0,19", "--pinned", "3")
