"""Pinned sweeps (bote_sweep_create_pinned): the search over the supersets of
pinned positions, on the fast kernel's pinned variant (bote_sweep.hip) and on
the generic kernel.

Every expected value comes from the CPU oracle over `supersets(ns, n, pinned)`:
the supersets sorted by full colex rank, built with itertools and math.comb
(never with bote_pinned_config).  OraclePlanet.sweep_ranks over those full ranks
gives lists, valid count and digest for SCORE / MEAN / COV; compute_stats'
per-client values, turned into keys in numpy (H by its definition), cover MAX /
p95 / MDTM.  Every comparison is exact equality."""
import itertools
import math

import numpy as np
import pytest
import torch

import oracle as O
from fantoch_amd import _lib, cli
from fantoch_amd.bote import DEFAULT_OBJECTIVES, DEFAULT_RANKING, DevicePlanet, Sweep
from fantoch_amd.planet import Planet

pytestmark = pytest.mark.gpu

K = 100
RP = (110.0, 35.0, 0.0, 15.0)
MEAN, MAX, MDTM, P95 = _lib.OBJ_MEAN, _lib.OBJ_MAX, _lib.OBJ_MDTM, _lib.OBJ_PCTL(9500)
AF1, FF1 = 0, 1


def supersets(ns, n, pinned):
    """The n-supersets of `pinned` among ns positions sorted by full colex rank, and those ranks."""
    free = [x for x in range(ns) if x not in pinned]
    cfgs = [tuple(sorted(set(pinned) | set(c))) for c in itertools.combinations(free, n - len(pinned))]
    rank = lambda c: sum(math.comb(x, j + 1) for j, x in enumerate(c))
    cfgs.sort(key=rank)
    return np.array(cfgs, dtype=np.uint32), np.array([rank(c) for c in cfgs], dtype=np.uint64)


def oracle_lists(o, srv, cli_, n, ranks, objs=DEFAULT_OBJECTIVES, k=K, threads=8):
    tops, valid, digest = o.sweep_ranks(srv, cli_, n, ranks, objs, k, RP, 2, threads)
    return [list(t) for t in tops], valid, digest


def sweep(dp, srv, cli_, n, pinned, kernel=None, objs=DEFAULT_OBJECTIVES, ranking=DEFAULT_RANKING, digest=True, k=K):
    return Sweep(dp, srv, cli_, n, objs, K=k, ranking=ranking, digest=digest, kernel=kernel, pinned=pinned)


def launched(sw, rb=0, re=None):
    sw.launch(rb, re)
    r = sw.result()
    return r.tops, r.valid, r.digest


@pytest.fixture(scope="module")
def gcp():
    p = Planet.new()
    return p, DevicePlanet(p), O.OraclePlanet.of(p)


_N7 = {}


def n7_case(gcp):
    """GCP n = 7 pinned [3, 9, 15]: the supersets, their ranks and the oracle's result (once)."""
    p, dp, o = gcp
    if not _N7:
        srv = np.arange(p.R, dtype=np.uint32)
        cfgs, ranks = supersets(p.R, 7, [3, 9, 15])
        _N7.update(srv=srv, cfgs=cfgs, ranks=ranks, want=oracle_lists(o, srv, srv, 7, ranks))
    return _N7


# --------------------------------------------------------------------- 1 ---
@pytest.mark.parametrize("n,pinned,count", [(3, [7, 2], 18), (5, [0, 1], 816), (5, [18, 19], 816),
                                            (7, [3, 9, 15], 2380), (9, [0, 5, 10, 19], 4368), (13, [6], 50388)])
def test_gcp_pinned_sweep_vs_oracle(gcp, n, pinned, count):
    """GCP R = 20, every region server and client, default objectives and ranking
    with the digest, on auto, forced fast and forced generic: m = n - 1 with fewer
    configs than a wave and than K from unsorted input; the lowest and the highest
    positions; interleaved pins that a lane's run walks across; the non-pipelined
    client loop (n = 9); m = 1."""
    p, dp, o = gcp
    srv = np.arange(p.R, dtype=np.uint32)
    cfgs, ranks = supersets(p.R, n, pinned)
    assert len(ranks) == count
    want = oracle_lists(o, srv, srv, n, ranks)
    for kernel, path in ((None, "fast"), ("fast", "fast"), ("generic", "generic")):
        sw = sweep(dp, srv, srv, n, pinned, kernel)
        assert sw.kernel_path() == path and sw.total == count
        got = launched(sw)
        assert got[1:] == want[1:], (kernel, "valid count or digest")
        assert got[0] == want[0], kernel
        for _, r in got[0][1][:3]:  # records carry full colex ranks: config_of works unchanged
            assert set(pinned) <= set(sw.config_of(r))


# --------------------------------------------------------------------- 2 ---
def merged(sw, bounds):
    """Launch each [bounds[i], bounds[i+1]) and merge the result blocks on the device."""
    nb, parts = sw.result_bytes(), len(bounds) - 1
    dev = torch.device("cuda", sw.dp.device)
    src = torch.empty(parts * nb, dtype=torch.uint8, device=dev)
    dst = torch.empty(nb, dtype=torch.uint8, device=dev)
    st = torch.cuda.current_stream(dev).cuda_stream
    for i in range(parts):
        sw.launch(bounds[i], bounds[i + 1], st)
        sw.result_device(src.data_ptr() + i * nb, st)
    sw.merge_device(src.data_ptr(), parts, dst.data_ptr(), st)
    r = sw.parse_block(dst.cpu().numpy())
    return r.tops, r.valid, r.digest


@pytest.mark.parametrize("kernel", [None, "generic"])
def test_sub_ranges_and_shards(gcp, kernel):
    p, dp, o = gcp
    c = n7_case(gcp)
    sw = sweep(dp, c["srv"], c["srv"], 7, [3, 9, 15], kernel)
    total = sw.total
    assert total == 2380
    single = launched(sw)
    assert single == c["want"]
    # 1,013 is no multiple of the lane count
    assert merged(sw, [0, 1013, total]) == single
    assert launched(sw, 500, 1500) == oracle_lists(o, c["srv"], c["srv"], 7, c["ranks"][500:1500])
    b = sw.split(0, total, 3)
    assert b[0] == 0 and b[-1] == total and b == sorted(b) and len(b) == 4
    assert merged(sw, b) == single
    with pytest.raises(_lib.BoteError, match="rank range out of bounds"):
        sw.launch(0, total + 1)
    with pytest.raises(_lib.BoteError, match="rank range out of bounds"):
        sw.split(0, total + 1, 2)


# --------------------------------------------------------------------- 3 ---
@pytest.mark.parametrize("kernel", ["fast", "generic"])
def test_lists_that_are_not_the_identity(gcp, kernel):
    """Servers = the 13 regions of the reference's main.rs in name order, as ids;
    clients = the first 7 regions (one quad and a remainder of 3, a separate row
    table); n = 5, pinned [2, 11]."""
    p, dp, o = gcp
    srv = np.array(sorted(p.index[r] for r in cli.REGIONS13), dtype=np.uint32)
    cl = np.arange(7, dtype=np.uint32)
    assert len(srv) == 13 and srv.tolist() != list(range(13))
    _, ranks = supersets(13, 5, [2, 11])
    sw = sweep(dp, srv, cl, 5, [2, 11], kernel)
    assert sw.kernel_path() == kernel
    assert launched(sw) == oracle_lists(o, srv, cl, 5, ranks)


# --------------------------------------------------------------------- 4 ---
def test_synthetic_r64_n6():
    p = Planet.synthetic(64)
    dp, o = DevicePlanet(p), O.OraclePlanet.of(p)
    srv = np.arange(64, dtype=np.uint32)
    _, ranks = supersets(64, 6, [5, 31, 63])
    assert len(ranks) == 35990
    sw = sweep(dp, srv, srv, 6, [5, 31, 63])
    assert sw.kernel_path() == "fast"
    assert launched(sw) == oracle_lists(o, srv, srv, 6, ranks, threads=16)


# --------------------------------------------------------------------- 5 ---
def test_deferred_configs_carry_full_ranks():
    """The twin planet of tests/test_gpu_tail.py (synthetic R = 32, regions 4 and 5
    at 200 from all others and 50 from each other), n = 4, pinned [4]: the 435
    supersets that also hold twin 5 tie exactly on the leader's COV, so the fast
    kernel defers them, and their records reach the lists through the unchanged
    rank-list fix-up: the queue holds full ranks."""
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
    cfgs, ranks = supersets(32, 4, [4])
    assert len(ranks) == 4495 and sum(1 for c in cfgs.tolist() if 5 in c) == 435
    sw = sweep(dp, srv, srv, 4, [4], "fast")
    assert sw.kernel_path() == "fast"
    got = launched(sw)
    assert sw.deferred() >= 435
    assert got == oracle_lists(o, srv, srv, 4, ranks)


# --------------------------------------------------------------------- 6 ---
def test_overflow_fallback():
    """Planet.equidistant(7, 48), n = 6, pinned [0]: every leader choice is an exact
    tie, so each of the C(47, 5) = 1,533,939 > 2^20 configs defers, the queue
    overflows and the generic kernel recomputes the range.  Each list is the
    first K supersets' full ranks under the one key the oracle gives a config."""
    _, p = Planet.equidistant(7, 48)
    dp, o = DevicePlanet(p), O.OraclePlanet.of(p)
    srv = np.arange(48, dtype=np.uint32)
    objs = [(MEAN, AF1), (MEAN, FF1)]
    sw = sweep(dp, srv, srv, 6, [0], "fast", objs, ranking=None, digest=False)
    assert sw.kernel_path() == "fast" and sw.total == 1533939
    tops, _, _ = launched(sw)
    assert sw.deferred() == sw.total
    # the first K supersets by full rank: {0} and 5 of 1..47 in colex order
    first = [(0,) + c for c in itertools.islice(
        sorted(itertools.combinations(range(1, 48), 5), key=lambda c: c[::-1]), K)]
    ranks = [sum(math.comb(x, j + 1) for j, x in enumerate(c)) for c in first]
    assert ranks == sorted(ranks)
    vals, _ = o.compute_stats(srv[np.array(first[:1], dtype=np.uint32)], srv)
    for (kind, slot), t in zip(objs, tops):
        key = int(vals[0, slot * 48:(slot + 1) * 48].sum())
        assert t == [(key, r) for r in ranks], slot


# --------------------------------------------------------------------- 7 ---
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
    p, dp, o = gcp
    srv = np.arange(p.R, dtype=np.uint32)
    n, nc, pinned = 5, p.R, [0, 19]
    objs = [(MEAN, AF1), (MAX, AF1), (P95, FF1), (MDTM, AF1), (MDTM, 5 + FF1)]
    cfgs, ranks = supersets(p.R, n, pinned)
    vals, _ = o.compute_stats(srv[cfgs], srv, threads=8)
    want = []
    for kind, slot in objs:
        v = vals[:, slot * nc:(slot + 1) * nc] if slot < 5 else vals[:, 5 * nc + (slot - 5) * n:5 * nc + (slot - 4) * n]
        keys = key_of(kind, v)
        order = np.lexsort((ranks, keys))[:K]
        want.append([(int(keys[i]), int(ranks[i])) for i in order])
    sw = sweep(dp, srv, srv, n, pinned, None, objs, ranking=None, digest=False)
    assert sw.kernel_path() == "generic"
    assert launched(sw)[0] == want
    # MAX alone takes the generic kernel's plain pinned variant, a percentile alone the other one
    for i in (1, 2):
        one = sweep(dp, srv, srv, n, pinned, None, objs[i:i + 1], ranking=None, digest=False)
        assert one.kernel_path() == "generic"
        assert launched(one)[0] == want[i:i + 1], objs[i]

    def plain_sweep_still_works():
        un = Sweep(dp, srv, srv, 3, [(MEAN, AF1)], K=K, ranking=None)
        un.launch()
        all3 = np.arange(math.comb(p.R, 3), dtype=np.uint64)
        assert un.result().tops == oracle_lists(o, srv, srv, 3, all3, [(MEAN, AF1)])[0]

    with pytest.raises(_lib.BoteError, match=r"the fast kernel's pinned variant computes SCORE, MEAN and COV "
                                             r"objectives \(generic kernel\)") as e:
        sweep(dp, srv, srv, n, pinned, "fast", objs, ranking=None, digest=False)
    assert e.value.code == -1
    plain_sweep_still_works()
    with pytest.raises(_lib.BoteError, match=r"the group kernel does not sweep pinned members "
                                             r"\(fast or generic kernel\)") as e:
        sweep(dp, srv, srv, n, pinned, "group", [(MEAN, AF1)], ranking=None, digest=False)
    assert e.value.code == -1
    plain_sweep_still_works()


# --------------------------------------------------------------------- 8 ---
def test_consistent_with_the_unpinned_sweep(gcp):
    p, dp, o = gcp
    srv = np.arange(p.R, dtype=np.uint32)
    objs = [(MEAN, AF1)]
    un = Sweep(dp, srv, srv, 5, objs, K=128, ranking=None)
    un.launch()
    top = un.result().tops[0]
    best = _lib.colex_unrank(top[0][1], 5, p.R).tolist()
    # [0, 1], and two members of the unpinned sweep's best config (so that some record holds the pair)
    for pinned, some in (([0, 1], False), (best[:2], True)):
        pin = sweep(dp, srv, srv, 5, pinned, None, objs, ranking=None, digest=False, k=128)
        got = launched(pin)[0][0]
        held = [rec for rec in top if set(pinned) <= set(_lib.colex_unrank(rec[1], 5, p.R).tolist())]
        assert held or not some
        it = iter(got)
        assert all(rec in it for rec in held), pinned  # (a subsequence: same (key, rank), same relative order)
        if held:
            assert got[0] == held[0]  # the pinned sweep's best is the unpinned list's first superset


# --------------------------------------------------------------------- 9 ---
def test_checkpointed(gcp, tmp_path):
    p, dp, o = gcp
    c = n7_case(gcp)
    path = str(tmp_path / "pinned.npz")
    sw = sweep(dp, c["srv"], c["srv"], 7, [3, 9, 15])
    assert sw.run_checkpointed(path, chunk=700, stop_after=1) is None
    other = sweep(dp, c["srv"], c["srv"], 7, [3, 9, 16])
    with pytest.raises(ValueError, match="different sweep"):
        other.run_checkpointed(path, chunk=700)
    r = sw.run_checkpointed(path, chunk=700)
    assert (r.tops, r.valid, r.digest) == c["want"]
