"""GPU tests of the C-ABI boundary added for SURVEY.md §8b: the one-call
multi-device search (bote_search_topk), the device-side overflow fallback of
the fast sweep (no host round trip per launch) and the stream-ordered per-call
entry points (reentrant across planet handles)."""
import json
import os
import threading

import numpy as np
import pytest

import oracle as O
from fantoch_amd import _lib
from fantoch_amd.bote import (DEFAULT_OBJECTIVES, DEFAULT_RANKING, Bote, DevicePlanet, MultiDeviceSearch, Sweep,
                              search_topk)
from fantoch_amd.planet import Planet

pytestmark = pytest.mark.gpu
GOLDEN = os.path.join(os.path.dirname(__file__), "golden")


def _same(a, b):
    return (a.valid, a.digest, a.tops) == (b.valid, b.digest, b.tops)


def test_search_topk_shards_equal_unsharded():
    """devices = [0, 0, 0] (and 9 shards, a two-level merge tree): identical to
    one unsharded sweep of the same rank range."""
    p = Planet.synthetic(64)
    dp = DevicePlanet(p)
    srv = np.arange(64, dtype=np.uint32)
    rb, re = 300_000_000, 330_000_000
    sw = Sweep(dp, srv, srv, 7, DEFAULT_OBJECTIVES, K=100, ranking=DEFAULT_RANKING, digest=True)
    sw.launch(rb, re)
    full = sw.result()
    assert _same(search_topk([dp], srv, srv, 7, rank_begin=rb, rank_end=re), full)
    three = [DevicePlanet(p) for _ in range(3)]  # distinct handles on one device
    assert _same(search_topk(three, srv, srv, 7, rank_begin=rb, rank_end=re), full)
    assert _same(search_topk([dp] * 9, srv, srv, 7, rank_begin=rb, rank_end=re), full)


def test_search_topk_full_r64n7_vs_oracle_fixture():
    """The bench workload in full through bote_search_topk with 3 shards on
    device 0, against the oracle's full sweep (tests/golden/syn_r64n7_full.json)."""
    path = os.path.join(GOLDEN, "syn_r64n7_full.json")
    if not os.path.exists(path):
        pytest.skip("fixture not generated yet (scripts/oracle_fixtures.sh)")
    fx = json.load(open(path))
    p = Planet.synthetic(64)
    dps = [DevicePlanet(p) for _ in range(3)]
    srv = np.arange(64, dtype=np.uint32)
    got = search_topk(dps, srv, srv, 7)
    assert (got.valid, got.digest) == (fx["valid"], fx["digest"])
    assert got.tops == [[tuple(r) for r in t] for t in fx["tops"]]


def test_search_handle_repeated_launch_is_device_work_only():
    """bote_search_create/launch/result over devices [0, 0, 0] and the full
    R=64 n=7 rank space: the handle's shard bounds are bote_sweep_split's,
    every launch equals the oracle's full sweep, and a repeated launch (no
    host walk, no allocation) costs about one single-device sweep."""
    import time

    path = os.path.join(GOLDEN, "syn_r64n7_full.json")
    if not os.path.exists(path):
        pytest.skip("fixture not generated yet (scripts/oracle_fixtures.sh)")
    fx = json.load(open(path))
    want = (fx["valid"], fx["digest"], [[tuple(r) for r in t] for t in fx["tops"]])
    p = Planet.synthetic(64)
    dps = [DevicePlanet(p) for _ in range(3)]
    srv = np.arange(64, dtype=np.uint32)
    h = MultiDeviceSearch(dps, srv, srv, 7)
    sw = Sweep(dps[0], srv, srv, 7, DEFAULT_OBJECTIVES, K=100, ranking=DEFAULT_RANKING, digest=True)
    assert h.bounds() == sw.split(0, sw.total, 3)
    h.launch()
    r = h.result()
    assert (r.valid, r.digest, r.tops) == want
    sw.launch()
    sw.result()

    def timed(fn, reps=5):
        best = []
        for _ in range(reps):
            t0 = time.perf_counter()
            fn()
            best.append(time.perf_counter() - t0)
        return sorted(best)[reps // 2]

    t_handle = timed(lambda: (h.launch(), h.result()))
    t_single = timed(lambda: (sw.launch(), sw.result()))
    print(f"search handle, 3 shards on one GPU: {t_handle * 1e3:.2f} ms per launch+result; "
          f"single sweep {t_single * 1e3:.2f} ms; ratio {t_handle / t_single:.3f}")
    r = h.result()
    assert (r.valid, r.digest, r.tops) == want
    assert t_handle < 1.15 * t_single
    # back-to-back launches with no result() between them: the second launch's
    # shard copies wait for the first launch's merge tree (bote_search::merged_ev)
    for _ in range(3):
        h.launch()
    r = h.result()
    assert (r.valid, r.digest, r.tops) == want


def test_search_handle_errors_leave_no_state():
    """Refused creations (planets that differ, a bad K, a bad range) return
    their codes; handles created afterwards work."""
    p = Planet.synthetic(64)
    q = Planet.synthetic(64, seed=1)
    srv = np.arange(64, dtype=np.uint32)
    a, b = DevicePlanet(p), DevicePlanet(q)
    with pytest.raises(_lib.BoteError, match="differ"):
        MultiDeviceSearch([a, b], srv, srv, 7)
    with pytest.raises(_lib.BoteError, match="K must be"):
        MultiDeviceSearch([a, a], srv, srv, 7, K=0)
    with pytest.raises(_lib.BoteError, match="out of bounds"):
        MultiDeviceSearch([a], srv, srv, 7, rank_begin=10, rank_end=5)
    h = MultiDeviceSearch([a, a], srv, srv, 7, rank_begin=1000, rank_end=200_000)
    h.launch()
    sw = Sweep(a, srv, srv, 7, DEFAULT_OBJECTIVES, K=100, ranking=DEFAULT_RANKING, digest=True)
    sw.launch(1000, 200_000)
    assert _same(h.result(), sw.result())


def test_overflow_fallback_is_device_side():
    """A planet whose configs all defer (more than the 2^20-entry queue): the
    generic fallback is chosen on the device; result_device (no host sync in
    the library) then a device merge equals the oracle."""
    import torch

    from fantoch_amd.dist import merge_gathered

    regions, p = Planet.equidistant(7, 48)
    dp = DevicePlanet(p)
    o = O.OraclePlanet.of(p)
    srv = np.arange(p.R, dtype=np.uint32)
    total = _lib.binomial(p.R, 5)
    tops, valid, digest = o.sweep(srv, srv, 5, 0, total, DEFAULT_OBJECTIVES, 100,
                                  (110.0, 35.0, 0.0, 15.0), 2, 8)
    sw = Sweep(dp, srv, srv, 5, DEFAULT_OBJECTIVES, K=100, ranking=DEFAULT_RANKING, digest=True, kernel="fast")
    nb = sw.result_bytes()
    g = torch.empty(2 * nb, dtype=torch.uint8, device="cuda")
    stream = torch.cuda.current_stream().cuda_stream
    half = total // 2
    sw.launch(0, half, stream)
    sw.result_device(g.data_ptr(), stream)
    sw.launch(half, total, stream)
    sw.result_device(g.data_ptr() + nb, stream)
    got = merge_gathered(sw, g, 2)
    assert (got.valid, got.digest) == (valid, digest)
    assert got.tops == [list(t) for t in tops]
    # and through the multi-device entry point
    got2 = search_topk([dp, dp], srv, srv, 5)
    assert (got2.valid, got2.digest, got2.tops) == (valid, digest, [list(t) for t in tops])


def test_per_call_entries_concurrent_handles():
    """Bote::leaderless / leader / best_leader from 4 threads, each on its own
    planet handle (own stream and workspace), equal the oracle."""
    p = Planet.new()
    o = O.OraclePlanet.of(p)
    errors = []

    def worker(seed):
        try:
            b = Bote(p)
            rng = np.random.default_rng(seed)
            for _ in range(25):
                ns = int(rng.integers(2, 12))
                servers = rng.choice(p.R, ns, replace=False)
                clients = rng.choice(p.R, int(rng.integers(1, 20)), replace=True)
                q = int(rng.integers(1, ns + 1))
                sv = [p.names[i] for i in servers]
                cv = [p.names[i] for i in clients]
                assert [v for _, v in b.leaderless(sv, cv, q)] == o.leaderless(servers, clients, q).tolist()
                lead = int(rng.integers(0, p.R))
                assert [v for _, v in b.leader(p.names[lead], sv, cv, q)] == o.leader(lead, servers, clients,
                                                                                      q).tolist()
        except Exception as e:  # surfaced below
            errors.append(e)

    th = [threading.Thread(target=worker, args=(s,)) for s in range(4)]
    for t in th:
        t.start()
    for t in th:
        t.join()
    assert not errors, errors


def test_tempo_quorums_every_gcp_config():
    """BASELINE config 2's Tempo keys on the whole GCP planet: for EVERY config
    of every n = 3..13 and f = 1, 2, Tempo's fast (n/2+f), tiny fast (2f) and
    write (f+1) quorums (fantoch/src/config.rs:317-329) through
    bote_eval_leaderless equal the oracle's Bote::leaderless: exact sums and
    sums of squares for every config (Input and Colocated), full per-client
    vectors for a sample."""
    from math import comb

    from fantoch_amd.bote import eval_leaderless, tempo_quorums

    p = Planet.new()
    dp = DevicePlanet(p)
    o = O.OraclePlanet.of(p)
    srv = np.arange(p.R, dtype=np.uint32)
    for n in range(3, 14):
        qs = sorted({q for _, _, q in tempo_quorums(n)})
        total = comb(p.R, n)
        for rb in range(0, total, 40_000):
            cnt = min(40_000, total - rb)
            r = eval_leaderless(dp, srv, srv, n, qs, rank_begin=rb, ncfg=cnt, values=True)
            cfg = np.array([_lib.colex_unrank(x, n, p.R) for x in range(rb, rb + cnt)], dtype=np.uint32)
            ov = o.leaderless_batch(srv[cfg], srv, qs, threads=8)
            nc = p.R
            assert np.array_equal(r.s1[:, :, 0], ov[:, :, :nc].sum(axis=2)), n
            assert np.array_equal(r.s1[:, :, 1], ov[:, :, nc:].sum(axis=2)), n
            assert np.array_equal(r.s2[:, :, 0], (ov[:, :, :nc] ** 2).sum(axis=2)), n
            assert np.array_equal(r.s2[:, :, 1], (ov[:, :, nc:] ** 2).sum(axis=2)), n
            assert np.array_equal(r.vals[::97].astype(np.uint64), ov[::97]), n


def test_tempo_stats_keys_and_unsorted_configs():
    """Search.compute_stats(..., tempo=True) adds tf/ttf/twf keys whose
    histograms equal the oracle's leaderless for an unsorted server list and
    a client subset with repeats."""
    from fantoch_amd.bote import Search, tempo_quorums
    from fantoch_amd.protocol import ClientPlacement

    p = Planet.new()
    b = Bote(p)
    o = O.OraclePlanet.of(p)
    rng = np.random.default_rng(11)
    for n in (3, 5, 7, 9, 13):
        cfg = rng.choice(p.R, n, replace=False)
        cli = rng.choice(p.R, 15, replace=True)
        st = Search.compute_stats([p.names[i] for i in cfg], [p.names[i] for i in cli], b, tempo=True)
        for proto, f, q in tempo_quorums(n):
            want_i = sorted(o.leaderless(cfg, cli, q).tolist())
            want_c = sorted(o.leaderless(cfg, cfg, q).tolist())
            assert list(st.get(proto, f, ClientPlacement.Input).iter_values()) == want_i
            assert list(st.get(proto, f, ClientPlacement.Colocated).iter_values()) == want_c
        assert "af1" in st.map and "e" in st.map  # the reference's keys are still there


def test_sweep_split_bounds():
    """bote_sweep_split: ascending bounds covering the range; on the group
    kernel the first shard of R=64 n=7 (the small-group region, more work per
    config) gets fewer ranks than an equal share; shards swept separately and
    merged equal the oracle's full-sweep fixture."""
    import torch

    from fantoch_amd.dist import merge_gathered

    p = Planet.synthetic(64)
    dp = DevicePlanet(p)
    srv = np.arange(64, dtype=np.uint32)
    sw = Sweep(dp, srv, srv, 7, DEFAULT_OBJECTIVES, K=100, ranking=DEFAULT_RANKING, digest=True)
    assert sw.kernel_path() == "group"
    b = sw.split(0, sw.total, 8)
    assert b[0] == 0 and b[-1] == sw.total and all(x < y for x, y in zip(b, b[1:]))
    assert b[1] < sw.total // 8
    assert sw.split(100, 100, 3) == [100] * 4
    g = sw.split(5, 1000, 4)
    assert g[0] == 5 and g[-1] == 1000 and g == sorted(g)
    path = os.path.join(GOLDEN, "syn_r64n7_full.json")
    if not os.path.exists(path):
        pytest.skip("full fixture not generated")
    fx = json.load(open(path))
    nb = sw.result_bytes()
    gathered = torch.empty(8 * nb, dtype=torch.uint8, device="cuda")
    stream = torch.cuda.current_stream().cuda_stream
    for i in range(8):
        sw.launch(b[i], b[i + 1], stream)
        sw.result_device(gathered.data_ptr() + i * nb, stream)
    got = merge_gathered(sw, gathered, 8)
    assert (got.valid, got.digest) == (fx["valid"], fx["digest"])
    assert got.tops == [[tuple(r) for r in t] for t in fx["tops"]]


def test_group_kernel_exact_with_32_bit_moments_and_64_bit_v():
    """The s32 && !v32 boundary of the group kernel's selection (ADVICE r06
    item 4; bote_host.cpp fast_limits): a planet whose sums of squares fit 32
    bits while V = cnt s2 - s1^2 does not, so the SI kernels (V in 32 bits)
    must not run.  Twice the synthetic R=128 planet, all 128 clients, the
    first 24 regions as servers (10,626 and 346,104 configs; groups longer
    than 64 ranks, so multi-step groups occur): the group kernel's valid
    count, digest and every top-K list equal the generic kernel's.
    tests/native/host_check.cpp pins that these numbers give v32 = 0."""
    base = Planet.synthetic(128)
    p = Planet(base.names, 2 * base.lat)
    nc, mx = 128, int(p.lat.max())
    assert nc * mx >= 2**16, "precondition: V does not fit 32 bits (v32 = 0)"
    assert nc * (2 * mx) ** 2 < 2**32 and 3 * nc * mx < 2**24, "precondition: the moments do (s32 = 1)"
    dp = DevicePlanet(p)
    srv = np.arange(24, dtype=np.uint32)
    cli = np.arange(128, dtype=np.uint32)
    for n in (4, 7):
        got = {}
        for kernel in ("group", "generic"):
            sw = Sweep(dp, srv, cli, n, DEFAULT_OBJECTIVES, K=100, ranking=DEFAULT_RANKING, digest=True,
                       kernel=kernel)
            assert sw.kernel_path() == kernel
            sw.launch()
            got[kernel] = sw.result()
        g, e = got["group"], got["generic"]
        assert g.valid == e.valid and g.digest == e.digest, n
        assert len(g.tops) == len(DEFAULT_OBJECTIVES)
        for o in range(len(DEFAULT_OBJECTIVES)):
            assert g.tops[o] == e.tops[o], f"n={n} objective {o}"


def test_step_overhead_outside_the_sweep_kernel():
    """Guard rail (the per-step cost outside the sweep kernel grew
    4.5x unnoticed): back-to-back full R=64 n=7 sweeps on one stream, each
    with its result copied to pinned host memory, as bench.py's steps are.
    Wall time per step minus the event-timed kernel (the HIP events ride on
    the kernel's dispatch) -- the zeroing, sample launch, seed, fix-up, merge
    and copy -- stays below 0.3 ms (round 5: ~0.2 ms of a 14.6 ms step)."""
    import time

    import torch

    p = Planet.synthetic(64)
    dp = DevicePlanet(p)
    srv = np.arange(64, dtype=np.uint32)
    sw = Sweep(dp, srv, srv, 7, DEFAULT_OBJECTIVES, K=100, ranking=DEFAULT_RANKING, digest=True)
    stream = torch.cuda.current_stream().cuda_stream
    host = torch.empty(sw.result_bytes(), dtype=torch.uint8, pin_memory=True)
    for _ in range(2):
        sw.launch(0, sw.total, stream)
        sw.result_device(host.data_ptr(), stream)
    torch.cuda.synchronize()
    sw.timing_reset()
    steps = 8
    overs = []
    for rep in range(2):  # (the better of two passes: a host or queue blip is not the library's cost)
        sw.timing_reset()
        t0 = time.perf_counter()
        for _ in range(steps):
            sw.launch(0, sw.total, stream)
            sw.result_device(host.data_ptr(), stream)
        torch.cuda.synchronize()
        dt = (time.perf_counter() - t0) / steps * 1e3
        kms, n = sw.timing()
        assert n == steps
        overs.append(dt - kms / n)
        print(f"pass {rep}: step {dt:.3f} ms, sweep kernel {kms / n:.3f} ms, outside the kernel {overs[-1]:.3f} ms")
        if rep == 0:
            # the result first (a timing miss must not hide it)
            fx = os.path.join(GOLDEN, "syn_r64n7_full.json")
            if os.path.exists(fx):
                f = json.load(open(fx))
                r = sw.parse_block(host.numpy())
                assert (r.valid, str(r.digest)) == (f["valid"], str(f["digest"]))
    # a loose guard (round 5-6: 0.13-0.14 ms measured; 4.5x that went
    # unnoticed in round 4): the bench line's step_overhead_ms is the figure
    assert min(overs) < 0.6, f"outside the kernel {min(overs):.3f} ms per step"
