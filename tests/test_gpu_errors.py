"""GPU tests of the C ABI's refusals: every public entry that validates is
called with one bad argument (the BoteError's code and text are asserted; the
checks are bote_host.cpp's, tested alone by tests/native/host_check.cpp), then
a valid call on the same planet must give what it gave before the bad one.
None of the bad calls reaches a kernel.  Also the sweep handle's per-range
table cache across its 16-entry clear."""
import contextlib
import ctypes as C

import numpy as np
import pytest

from fantoch_amd import _lib
from fantoch_amd.bote import (CONFIG5_OBJECTIVES, DEFAULT_OBJECTIVES, DEFAULT_RANKING, DevicePlanet,
                              MultiDeviceSearch, Sweep, eval_configs, eval_keys, eval_leaderless)
from fantoch_amd.planet import Planet

pytestmark = pytest.mark.gpu

ARG, QUORUM, RANGE = -1, -2, -4
N, K = 4, 4  # C(8, 4) = 70 ranks


def synthetic(R, seed):
    """Latencies in [1, 200] off the diagonal, 0 on it: fast-path eligible."""
    lat = np.random.default_rng(seed).integers(1, 201, (R, R))
    np.fill_diagonal(lat, 0)
    return Planet([f"r{i:03d}" for i in range(R)], lat)


@contextlib.contextmanager
def refused(code, msg):
    with pytest.raises(_lib.BoteError) as e:
        yield
    assert e.value.code == code
    assert str(e.value) == f"{_lib.ERRORS[code]}: {msg}"


@pytest.fixture(scope="module")
def planet():
    return synthetic(8, 8)


@pytest.fixture(scope="module")
def dp(planet):
    return DevicePlanet(planet)


SRV = np.arange(8, dtype=np.uint32)


def sweep_result(dp, **kw):
    sw = Sweep(dp, SRV, SRV, N, DEFAULT_OBJECTIVES, K=K, ranking=DEFAULT_RANKING, digest=True, **kw)
    sw.launch()
    r = sw.result()
    return r.tops, r.valid, r.digest


def test_single_configuration_entries(dp):
    """bote_quorum_latencies, bote_leaderless, bote_leader, bote_all_leaders, bote_best_leader."""
    L = _lib.lib()
    bad_srv = np.array([0, 3, 8], np.uint32)  # region id R
    froms = np.array([0, 3], np.uint32)

    def single(fn, *args, nout=8):
        out = np.zeros(nout, np.uint64)
        _lib.check(fn(dp.h, *args, out))
        return out.tolist()

    def best(srv, q, stat):
        pos, lat = C.c_uint32(), np.zeros(8, np.uint64)
        _lib.check(L.bote_best_leader(dp.h, srv, len(srv), SRV, 8, q, stat, C.byref(pos), _lib.ptr(lat)))
        return pos.value, lat.tolist()

    calls = [
        (lambda srv=SRV, q=3: single(L.bote_quorum_latencies, froms, 2, srv, len(srv), q, nout=2),
         dict(srv=bad_srv), ARG, "servers: region id out of range"),
        (lambda q=3: single(L.bote_leaderless, SRV, 8, SRV, 8, q), dict(q=0), ARG, "quorum size 0"),
        (lambda leader=2: single(L.bote_leader, leader, SRV, 8, SRV, 8, 3), dict(leader=8), ARG, "leader out of range"),
        (lambda q=3: single(L.bote_all_leaders, SRV, 8, SRV, 8, q, nout=64), dict(q=9), QUORUM,
         "quorum larger than the server set"),
        (lambda stat=_lib.STAT_MEAN: best(SRV, 3, stat), dict(stat=3), ARG, "unknown stat"),
    ]
    for call, bad, code, msg in calls:
        before = call()
        assert any(before[1] if isinstance(before, tuple) else before)
        with refused(code, msg):
            call(**bad)
        assert call() == before


def test_eval_entries(dp):
    """bote_eval, bote_eval_keys, bote_eval_leaderless."""
    def same(a, b, fields):
        return all(np.array_equal(getattr(a, f), getattr(b, f)) for f in fields)

    cfg = np.array([[0, 1, 2, 7], [1, 3, 5, 6]], np.uint32)
    bad_cfg = np.array([[0, 1, 2, 7], [1, 3, 5, 8]], np.uint32)  # position ns
    before = eval_configs(dp, SRV, SRV, N, configs=cfg, ranking=DEFAULT_RANKING)
    with refused(ARG, "config position out of range"):
        eval_configs(dp, SRV, SRV, N, configs=bad_cfg, ranking=DEFAULT_RANKING)
    with refused(ARG, "rank range out of bounds"):
        eval_configs(dp, SRV, SRV, N, rank_begin=69, ncfg=2)
    assert same(eval_configs(dp, SRV, SRV, N, configs=cfg, ranking=DEFAULT_RANKING), before,
                ("vals", "leader", "s1", "s2", "mean", "cov", "score", "valid"))

    before = eval_keys(dp, SRV, SRV, N, configs=cfg)
    with refused(ARG, "unknown key set"):
        eval_keys(dp, SRV, SRV, N, configs=cfg, keys=2)
    with refused(ARG, "duplicate position in config"):
        eval_keys(dp, SRV, SRV, N, configs=np.array([[0, 1, 1, 7]], np.uint32))
    assert same(eval_keys(dp, SRV, SRV, N, configs=cfg), before, ("s1", "s2", "al_s1", "al_s2", "leader"))

    before = eval_leaderless(dp, SRV, SRV, N, [2, 3, 4], configs=cfg)
    with refused(QUORUM, "quorum larger than the config"):
        eval_leaderless(dp, SRV, SRV, N, [2, 5], configs=cfg)
    with refused(ARG, "1 to 8 quorum sizes"):
        eval_leaderless(dp, SRV, SRV, N, [1] * 9, configs=cfg)
    assert same(eval_leaderless(dp, SRV, SRV, N, [2, 3, 4], configs=cfg), before, ("vals", "s1", "s2"))


def test_sweep_and_search_entries(planet, dp):
    """bote_sweep_create_keys (before and after its device buffers exist),
    bote_sweep_launch, bote_sweep_split, bote_search_create."""
    before = sweep_result(dp)
    assert all(len(t) == K for t in before[0][1:])  # (the MEAN and COV lists: every config has a key)
    with refused(RANGE, "K must be in [1, 128]"):
        Sweep(dp, SRV, SRV, N, DEFAULT_OBJECTIVES, K=0)
    with refused(ARG, "servers: duplicate region"):
        Sweep(dp, [0, 1, 2, 3, 4, 5, 6, 6], SRV, N, DEFAULT_OBJECTIVES, K=K)
    assert sweep_result(dp) == before

    # refused after the lists (and for the first, the fast-path layouts) are on
    # the device: the half-built handle is destroyed
    slow = planet.lat.copy()
    slow[2, 5] = 5000  # above the packed kernels' 4095
    dslow = DevicePlanet(Planet(planet.names, slow))
    for kw, pl, n, msg in (
            (dict(kernel="group"), dp, 3, "group kernel needs n >= 4"),
            (dict(kernel="fast"), dslow, N, "the fast/group kernel is not eligible for this planet and lists"),
            (dict(kernel="fast", keys=_lib.KEYS_TEMPO_ALL_LEADERS, objectives=CONFIG5_OBJECTIVES), dp, N,
             "the extended key set runs on the group kernel (n = 4..7, config 5's objectives) or the generic kernel")):
        kw.setdefault("objectives", DEFAULT_OBJECTIVES)
        with refused(ARG, msg):
            Sweep(pl, SRV, SRV, n, K=K, ranking=DEFAULT_RANKING, digest=True, **kw)
        assert sweep_result(dp) == before

    sw = Sweep(dp, SRV, SRV, N, DEFAULT_OBJECTIVES, K=K, ranking=DEFAULT_RANKING, digest=True)
    sw.launch()
    with refused(ARG, "rank range out of bounds"):
        sw.launch(0, 71)
    with refused(ARG, "rank range out of bounds"):
        sw.launch(5, 4)
    with refused(ARG, "parts must be >= 1"):
        sw.split(0, 70, 0)
    r = sw.result()  # (the valid launch's: the refused ones enqueued nothing)
    assert (r.tops, r.valid, r.digest) == before
    sw.launch()
    r = sw.result()
    assert (r.tops, r.valid, r.digest) == before
    assert sw.split(0, 70, 2)[0::2] == [0, 70]

    with refused(ARG, "rank range out of bounds"):
        MultiDeviceSearch([dp], SRV, SRV, N, K=K, rank_begin=10, rank_end=5)
    with refused(ARG, "config size larger than the server list"):
        MultiDeviceSearch([dp, dp], SRV, SRV, 9, K=K)
    h = MultiDeviceSearch([dp, dp], SRV, SRV, N, K=K)
    h.launch()
    r = h.result()
    assert (r.tops, r.valid, r.digest) == before


def test_range_tables_across_the_cache_clear():
    """One group-kernel sweep handle over 34 distinct ranges of a 16-region
    planet's C(16, 4) = 1,820 ranks, then the first range again.  The handle
    keeps at most 16 ranges' chunk tables and empties the cache on a miss that
    finds it full: the 17th range does, and the 33rd clears a cache refilled
    since.  The 34th and the repeated first range (dropped by the first clear)
    are built anew after a clear.  Every result equals the generic kernel's
    over the same range.

    None of these ranges takes the top-K seed sample, so its cache (the same
    RangeCache) is not crossed here: bote_host's sample_count gives at least
    min(4096, waves) one-step chunks and needs 512 ranks of range for each,
    and a group launch has at least 4 waves, so no range of 1,820 ranks
    samples (tests/native/host_check.cpp checks that for every wave count).
    test_gpu_seed.py and the large-workload tests remain that cache's cover."""
    dp = DevicePlanet(synthetic(16, 16))
    srv = np.arange(16, dtype=np.uint32)
    group, generic = (Sweep(dp, srv, srv, N, DEFAULT_OBJECTIVES, K=K, ranking=DEFAULT_RANKING, digest=True, kernel=k)
                      for k in ("group", "generic"))
    assert group.kernel_path() == "group" and generic.kernel_path() == "generic" and group.total == 1820
    ranges = ([(0, 1820)] + [(97 * i, 97 * i + 64 + 3 * i) for i in range(1, 18)] +
              [(53 * i, 53 * i + 87 + i) for i in range(1, 17)])
    assert len(set(ranges)) == 34 and all(e - b >= 64 and e <= 1820 for b, e in ranges)
    for b, e in ranges + ranges[:1]:
        got = []
        for sw in (group, generic):
            sw.launch(b, e)
            r = sw.result()
            got.append((r.tops, r.valid, r.digest))
        assert got[0] == got[1], (b, e)
        assert all(len(t) == K for t in got[0][0][1:])
