"""Every instantiation family of the generic kernel (bote_eval.hpp: full outputs,
plain top-K, the percentile and the MDTM passes, the pinned variant; base and
extended keys) at every config size n = 2..16, so that a wrong row in the
dispatcher over the families' units (bote_kernels.hip eval_fn) fails a test.

Every case runs on GCP R = 20 with all regions as servers and clients.  Rank
ranges are 2,048 ranks around the middle of the rank space (all of it where it
is smaller); sweeps are forced onto the generic kernel.  Every expected value
comes from the CPU oracle (compute_stats, scores, moments_x, sweep,
sweep_ranks), keys of MAX / percentile / MDTM objectives from its per-client
values as tests/host_keys.py builds them; every comparison is exact equality.
Each test first asserts that its expectation tells configs apart: more than
one distinct key in an expected list, and with a ranking 0 < valid < ranks."""
import math

import numpy as np
import pytest

import oracle as O
from fantoch_amd import _lib
from fantoch_amd.bote import DEFAULT_OBJECTIVES, DevicePlanet, FTMetric, RankingParams, Sweep, eval_configs, eval_keys
from fantoch_amd.planet import Planet
from tests.host_keys import MAX, MDTM, MEAN, key_of, slot_values, supersets, top_of

pytestmark = pytest.mark.gpu

K = 16
SIZES = list(range(2, 17))
RANKING = RankingParams.new(30, 10, 0, 15, 3, 13, FTMetric.F1F2)
RP, FT = (30.0, 10.0, 0.0, 15.0), 2
P = _lib.OBJ_PCTL
AF1, FF1, E = 0, 1, 4
U64MAX = np.iinfo(np.uint64).max


@pytest.fixture(scope="module")
def gcp():
    p = Planet.new()
    assert p.R == 20
    return p, DevicePlanet(p), O.OraclePlanet.of(p), np.arange(p.R, dtype=np.uint32)


def rank_range(n):
    total = math.comb(20, n)
    rb = max(0, total // 2 - 1024)
    return rb, min(total, rb + 2048)


_CASE = {}


def case(gcp, n):
    """The configs of n's rank range (positions = region ids) and the oracle's compute_stats of them, once per n."""
    if n not in _CASE:
        o, srv = gcp[2], gcp[3]
        rb, re = rank_range(n)
        cfg = np.array([_lib.colex_unrank(r, n, 20) for r in range(rb, re)], dtype=np.uint32)
        vals, lead = o.compute_stats(srv[cfg], srv, threads=8)
        _CASE[n] = dict(rb=rb, re=re, cfg=cfg, vals=vals, lead=lead)
    return _CASE[n]


def need(bp, count):
    """How many of a slot's largest values percentile bp takes (at most 8 on the generic kernel)."""
    return count - max(_lib.percentile_index(bp, count)[0], 1) + 1


def member_percentile(n):
    """The lowest of a few percentiles over the n members whose need the library admits: the deepest list."""
    return P(next(bp for bp in (5000, 6000, 7000, 7500, 8000, 9000) if need(bp, n) <= 8))


def tells_apart(lists):
    assert all(len({k for k, _ in lst}) > 1 for lst in lists), "an expected list holds one key only"


def value_lists(c, n, objs, ranks):
    """Top-K lists of `objs` from compute_stats' values of configs with those ranks."""
    return [top_of(key_of(kind, slot_values(c, slot, 20, n)), K, ranks) for kind, slot in objs]


def generic(dp, srv, n, objs, ranking=None, digest=False, keys=_lib.KEYS_BASE, pinned=None):
    sw = Sweep(dp, srv, srv, n, objs, K=K, ranking=ranking, digest=digest, kernel="generic", keys=keys, pinned=pinned)
    assert sw.kernel_path() == "generic"
    return sw


def launched(sw, rb=0, re=None):
    sw.launch(rb, re)
    r = sw.result()
    return r.tops, r.valid, r.digest


# --------------------------------------------------------------------- 1 ---
@pytest.mark.parametrize("n", SIZES)
def test_full_outputs_base_keys(gcp, n):
    """bote_eval over the range as explicit configs and as a rank range: per-client
    values, leaders, s1 / s2, score and validity."""
    p, dp, o, srv = gcp
    c = case(gcp, n)
    cnt = c["re"] - c["rb"]
    ov = c["vals"]
    score, valid = o.scores(srv[c["cfg"]], srv, RP, FT)
    assert 0 < int(valid.sum()) < cnt
    s1 = np.zeros((cnt, 10), np.uint64)
    s2 = np.zeros((cnt, 10), np.uint64)
    for slot in range(10):
        v = slot_values(ov, slot, 20, n)
        absent = v[:, 0] == U64MAX  # (af2 / ff2 where max_f < 2)
        s1[:, slot] = np.where(absent, U64MAX, v.sum(axis=1))
        s2[:, slot] = np.where(absent, U64MAX, (v * v).sum(axis=1))
    assert len(np.unique(s1[:, AF1])) > 1
    for how in (dict(configs=c["cfg"]), dict(rank_begin=c["rb"], ncfg=cnt)):
        r = eval_configs(dp, srv, srv, n, ranking=RANKING, **how)
        assert np.array_equal(r.vals.astype(np.uint64), np.where(ov == U64MAX, np.uint64(0xFFFFFFFF), ov)), list(how)
        assert np.array_equal(r.leader, c["lead"]), list(how)
        assert np.array_equal(r.s1, s1) and np.array_equal(r.s2, s2), list(how)
        assert np.array_equal(r.score.view(np.uint64), score.view(np.uint64)), list(how)
        assert np.array_equal(r.valid.astype(bool), valid.astype(bool)), list(how)


# --------------------------------------------------------------------- 2 ---
@pytest.mark.parametrize("n", SIZES)
def test_full_outputs_extended_keys(gcp, n):
    """bote_eval_keys: all 20 slots' and every leader's moments (compute_stats_x)."""
    p, dp, o, srv = gcp
    c = case(gcp, n)
    s1, s2, a1, a2, lead = o.moments_x(srv[c["cfg"]], srv, threads=8)
    if n // 2 < 2:  # f = 2 leaders do not exist
        a1[:, 1, :] = U64MAX
        a2[:, 1, :] = U64MAX
    assert len(np.unique(s1[:, _lib.SLOT_TT1])) > 1 and len(np.unique(a1[:, 0, :], axis=0)) > 1
    for how in (dict(configs=c["cfg"]), dict(rank_begin=c["rb"], ncfg=c["re"] - c["rb"])):
        got = eval_keys(dp, srv, srv, n, keys=_lib.KEYS_TEMPO_ALL_LEADERS, **how)
        assert np.array_equal(got.leader, lead), list(how)
        assert np.array_equal(got.s1, s1) and np.array_equal(got.s2, s2), list(how)
        assert np.array_equal(got.al_s1, a1) and np.array_equal(got.al_s2, a2), list(how)


# --------------------------------------------------------------------- 3 ---
@pytest.mark.parametrize("keys", [_lib.KEYS_BASE, _lib.KEYS_TEMPO_ALL_LEADERS])
@pytest.mark.parametrize("n", SIZES)
def test_plain_topk(gcp, n, keys):
    """The default objectives with the digest (with the extended key set it folds
    slots 10..19 and every leader's moments): lists, valid count, digest."""
    p, dp, o, srv = gcp
    rb, re = rank_range(n)
    tops, valid, digest = o.sweep(srv, srv, n, rb, re, DEFAULT_OBJECTIVES, K, RP, FT, 8,
                                  keys=1 if keys == _lib.KEYS_TEMPO_ALL_LEADERS else 0)
    tops = [list(t) for t in tops]
    assert 0 < valid < re - rb
    tells_apart(tops[1:2])  # (MEAN af1)
    sw = generic(dp, srv, n, DEFAULT_OBJECTIVES, RANKING, True, keys)
    got = launched(sw, rb, re)
    assert got[1:] == (valid, digest)
    assert got[0] == tops


# --------------------------------------------------------------------- 4 ---
@pytest.mark.parametrize("n", SIZES)
def test_percentile_passes(gcp, n):
    """EVAL_PCTL: p95 af1 over the 20 clients (needs 2), the deepest admitted of a
    few percentiles over the n members, and MAX e."""
    p, dp, o, srv = gcp
    c = case(gcp, n)
    objs = [(P(9500), AF1), (member_percentile(n), 5 + AF1), (MAX, E)]
    want = value_lists(c["vals"], n, objs, np.arange(c["rb"], c["re"]))
    tells_apart(want)
    assert launched(generic(dp, srv, n, objs), c["rb"], c["re"])[0] == want


# --------------------------------------------------------------------- 5 ---
@pytest.mark.parametrize("n", SIZES)
def test_mdtm_passes(gcp, n):
    """EVAL_MDTM: MDTM af1 (Input) and MDTM ff1C (Colocated) beside p95 af1 (p95 ff1
    has one key over most of these ranges: one leader, one quorum latency)."""
    p, dp, o, srv = gcp
    c = case(gcp, n)
    objs = [(MDTM, AF1), (MDTM, 5 + FF1), (P(9500), AF1)]
    want = value_lists(c["vals"], n, objs, np.arange(c["rb"], c["re"]))
    tells_apart(want)
    assert launched(generic(dp, srv, n, objs), c["rb"], c["re"])[0] == want


# --------------------------------------------------------------------- 6 ---
@pytest.mark.parametrize("n", SIZES)
def test_pinned(gcp, n):
    """The pinned variant over its whole pinned rank space, the m = max(1, n - 3)
    highest positions pinned (at most C(19, 3) = 969 supersets): SCORE / MEAN / COV
    with the digest (EVAL_PLAIN), then MAX e and p95 af1 (EVAL_MDTM).  With these
    members pinned the oracle finds valid configs under the ranking at n = 3..7
    only (none of the 19 at n = 2, none from n = 8 on, whatever thresholds >= 0
    the ranking has): there the valid count and the SCORE list are equal as zero
    and empty, and the digest and the other lists still cover every config."""
    p, dp, o, srv = gcp
    m = max(1, n - 3)
    pinned = list(range(20 - m, 20))
    cfgs, ranks = supersets(20, n, pinned)
    assert len(ranks) == math.comb(20 - m, n - m) <= 969
    tops, valid, digest = o.sweep_ranks(srv, srv, n, ranks, DEFAULT_OBJECTIVES, K, RP, FT, 8)
    tops = [list(t) for t in tops]
    assert valid < len(ranks) and (valid > 0) == (3 <= n <= 7)
    tells_apart(tops[1:2])
    sw = generic(dp, srv, n, DEFAULT_OBJECTIVES, RANKING, True, pinned=pinned)
    assert sw.total == len(ranks)
    got = launched(sw)
    assert got[1:] == (valid, digest)
    assert got[0] == tops
    objs = [(MAX, E), (P(9500), AF1), (MEAN, AF1)]
    vals, _ = o.compute_stats(srv[cfgs], srv, threads=8)
    want = value_lists(vals, n, objs, ranks)
    tells_apart(want)
    assert launched(generic(dp, srv, n, objs, pinned=pinned))[0] == want
