"""MDTM (mean distance to mean) objectives of the streaming sweep
(include/bote_hip.h BOTE_OBJ_MDTM): key = (H << 27) | sum of a slot, H = the sum
over the slot's values above its mean of (count * x - sum), on the fast kernel's
MDTM variant (bote_sweep.hip, FAST_MDTM: a second pass over the clients) and on
the generic kernel (bote_eval.hpp).

Every expected list comes from the CPU oracle: OraclePlanet.compute_stats over
the sweep's configs in colex order gives each slot's per-client values; numpy
builds H by the direct definition (never by the kernels' threshold identity);
the lists are the K least by (key, rank).  Every comparison is exact equality
of the full (key, rank) lists."""
import io
import json

import numpy as np
import pytest

import oracle as O
from fantoch_amd import _lib, cli
from fantoch_amd.bote import DevicePlanet, MultiDeviceSearch, Sweep, mdtm_key, search_topk
from fantoch_amd.planet import Planet
from tests.host_keys import colex_positions, slot_values

pytestmark = pytest.mark.gpu

K = 100
MEAN, MAX, MDTM, P = _lib.OBJ_MEAN, _lib.OBJ_MAX, _lib.OBJ_MDTM, _lib.OBJ_PCTL
AF1, FF1, AF2, FF2, E = 0, 1, 2, 3, 4
KERNELS = [None, "fast", "generic"]


def objectives(n):
    objs = [(MEAN, AF1), (MDTM, AF1), (MDTM, FF1), (MDTM, E), (MDTM, 5 + AF1), (MDTM, 5 + FF1)]
    if n // 2 >= 2:
        objs += [(MDTM, AF2), (MDTM, 5 + FF2)]
    return objs


def top_of(keys, k=K, base=0):
    """The k least (key, rank) of per-rank keys (rank = base + index), ascending."""
    keys = np.asarray(keys, dtype=np.uint64)
    order = np.lexsort((np.arange(len(keys)), keys))[:k]
    return [(int(keys[r]), base + int(r)) for r in order]


def half_deviation(v):
    """H of every row by its definition: the sum of the positive (count * x - sum)."""
    v = np.asarray(v).astype(np.int64)
    c, s = v.shape[1], v.sum(axis=1)
    return np.maximum(c * v - s[:, None], 0).sum(axis=1), s


def key_of(kind, v):
    """Per-config key of one slot's values (ncfg, count)."""
    h, s = half_deviation(v)
    if kind == MEAN:
        return s.astype(np.uint64)
    if kind == MDTM:
        assert int(s.max()) < (1 << 27) - 1 and int(h.max()) < 1 << 37
        return (h.astype(np.uint64) << np.uint64(27)) | s.astype(np.uint64)
    u = np.asarray(v, dtype=np.uint64)
    if kind == MAX:
        return (u.max(axis=1) << np.uint64(32)) | s.astype(np.uint64)
    assert _lib.is_pctl(kind)
    idx, whole = _lib.percentile_index(kind & 0xFFFF, u.shape[1])
    a = np.sort(u, axis=1)
    twice = 2 * a[:, 0] if idx == 0 else a[:, idx - 1] + a[:, idx] if whole else 2 * a[:, idx - 1]
    return (twice << np.uint64(32)) | s.astype(np.uint64)


def expected(o, srv, cli_, n, objs):
    """The oracle's top-K lists of a full sweep over the n-subsets of `srv`."""
    srv = np.asarray(srv, dtype=np.uint32)
    vals, _ = o.compute_stats(srv[colex_positions(len(srv), n)], cli_, threads=8)
    return [top_of(key_of(kind, slot_values(vals, slot, len(cli_), n))) for kind, slot in objs]


def run(dp, srv, cli_, n, objs, kernel, keys=_lib.KEYS_BASE, k=K, rb=0, re=None):
    sw = Sweep(dp, srv, cli_, n, objs, K=k, ranking=None, kernel=kernel, keys=keys)
    sw.launch(rb, sw.total if re is None else re)
    return sw, sw.result().tops


def path_of(kernel):
    return "generic" if kernel == "generic" else "fast"


@pytest.fixture(scope="module")
def gcp():
    p = Planet.new()
    return p, DevicePlanet(p), O.OraclePlanet.of(p)


_VALS = {}


def gcp_values(gcp, n):
    """compute_stats of every GCP n-subset, every region as server and client (computed once per n)."""
    p, _, o = gcp
    if n not in _VALS:
        srv = np.arange(p.R, dtype=np.uint32)
        _VALS[n] = o.compute_stats(srv[colex_positions(p.R, n)], srv, threads=8)[0]
    return _VALS[n]


def gcp_expected(gcp, n, objs):
    vals = gcp_values(gcp, n)
    return [top_of(key_of(kind, slot_values(vals, slot, gcp[0].R, n))) for kind, slot in objs]


# ------------------------------------------------------------------ 1, 9 ---
@pytest.mark.parametrize("n", [3, 5, 7, 9, 11])
def test_gcp_full_sweep_vs_oracle(gcp, n):
    """GCP R=20 (nq = 5: an odd quad count), n = 3 (one leaderless table), 5, 7
    (two), 9 (two; the non-pipelined client loop) and 11 (three: the second
    pass's second qtab plane; the read-back of the third table is the next
    test's), on auto (the MDTM variant of the fast kernel), forced fast and
    forced generic.  n = 3 has configs with H = 0 on af1C (the zero key).  Then
    the f64 value: 2 H / c^2 from mdtm_key against the oracle's Histogram::mdtm
    of the record's values, within 1e-12 relative (the project's COV bar, DESIGN
    §2), and exactly 0.0 when H = 0."""
    p, dp, o = gcp
    srv = np.arange(p.R, dtype=np.uint32)
    objs = objectives(n)
    want = gcp_expected(gcp, n, objs)
    if n == 3:
        af1c = key_of(MDTM, slot_values(gcp_values(gcp, 3), 5 + AF1, p.R, 3))
        assert int(((af1c >> np.uint64(27)) == 0).sum()) >= 1
        assert mdtm_key(want[objs.index((MDTM, 5 + AF1))][0][0])[0] == 0
    for kernel in KERNELS:
        sw, tops = run(dp, srv, srv, n, objs, kernel)
        assert sw.kernel_path() == path_of(kernel), kernel
        assert tops == want, (n, kernel)
    vals = gcp_values(gcp, n)
    worst = 0.0
    for (kind, slot), t in zip(objs, tops):
        if kind != MDTM:
            continue
        v = slot_values(vals, slot, p.R, n)
        c = v.shape[1]
        for key, r in t:
            h, s1 = mdtm_key(key)
            assert s1 == int(v[r].sum())
            got, ref = 2 * h / c ** 2, float(O.hist_stats(v[r])[3])
            if h == 0:
                assert got == 0.0 and ref == 0.0, (slot, r)
            else:
                worst = max(worst, abs(got - ref) / ref)
                assert abs(got - ref) <= 1e-12 * ref, (slot, r, got, ref)
    print(f"n={n}: worst relative difference of 2H/c^2 to the oracle's mdtm {worst:.3g}")


def test_gcp_n11_colocated_third_table_vs_oracle(gcp):
    """At n = 11 the third leaderless table is E's, and the only slot that reads
    its colocated values is eC (5 + E), which objectives(11) has no room for
    (MAXOBJ): MDTM eC (the read-back of the lane's second qtab plane) beside
    MDTM e (the second pass's second plane), on auto, forced fast and forced
    generic."""
    p, dp, _ = gcp
    srv = np.arange(p.R, dtype=np.uint32)
    objs = [(MEAN, AF1), (MDTM, 5 + E), (MDTM, E)]
    want = gcp_expected(gcp, 11, objs)
    assert len({k for k, _ in want[1]}) > 1  # (the eC keys tell configs apart)
    for kernel in KERNELS:
        sw, tops = run(dp, srv, srv, 11, objs, kernel)
        assert sw.kernel_path() == path_of(kernel), kernel
        assert tops == want, kernel


# --------------------------------------------------------------------- 2 ---
@pytest.mark.parametrize("kernel", ["fast", "generic"])
def test_every_config_key(gcp, kernel):
    """GCP n = 5 in consecutive windows of 128 ranks with K = 128: every one of
    the 15,504 configs is reported for every objective.  Among them, on af1,
    are configs with a client exactly at an integral mean (r = 0: that client
    is not above the mean) and configs with r = c - 1 (the floor is exact)."""
    p, dp, _ = gcp
    srv = np.arange(p.R, dtype=np.uint32)
    objs = objectives(5)
    vals = gcp_values(gcp, 5)
    v = slot_values(vals, AF1, p.R, 5).astype(np.int64)
    c, s = v.shape[1], v.sum(axis=1)
    at_mean = int(((s % c == 0) & (v * c == s[:, None]).any(axis=1)).sum())
    r_max = int((s % c == c - 1).sum())
    print(f"af1: {at_mean} configs with a client at an integral mean, {r_max} with r = c - 1")
    assert at_mean > 0 and r_max > 0
    keys = [key_of(kind, slot_values(vals, slot, p.R, 5)) for kind, slot in objs]
    sw = Sweep(dp, srv, srv, 5, objs, K=128, ranking=None, kernel=kernel)
    assert sw.kernel_path() == kernel and sw.total == len(vals) == 15504
    for rb in range(0, sw.total, 128):
        re = min(rb + 128, sw.total)
        sw.launch(rb, re)
        tops = sw.result().tops
        for k, t in zip(keys, tops):
            assert t == top_of(k[rb:re], k=128, base=rb), (kernel, rb)


# --------------------------------------------------------------------- 3 ---
@pytest.mark.parametrize("ncli", [2, 3, 5, 6, 7, 13])
def test_client_remainders(gcp, ncli):
    """GCP n = 5 with the first 2, 3, 5, 6, 7, 13 regions as clients: no full
    quad with 2 and 3 clients, a remainder of 1, 2 and 3 after one quad, and
    three quads plus one client; the second pass's mask keeps the remainder's
    dead clients out of both the sum above the mean and the count."""
    p, dp, o = gcp
    srv = np.arange(p.R, dtype=np.uint32)
    cli_ = np.arange(ncli, dtype=np.uint32)
    objs = objectives(5)
    want = expected(o, srv, cli_, 5, objs)
    for kernel in KERNELS:
        sw, tops = run(dp, srv, cli_, 5, objs, kernel)
        assert sw.kernel_path() == path_of(kernel), kernel
        assert tops == want, (ncli, kernel)


# --------------------------------------------------------------------- 4 ---
def test_server_subset_in_name_order(gcp):
    """17 of the 20 regions as servers (positions differ from region ids), all 20 as clients."""
    p, dp, o = gcp
    srv = np.array([r for r in range(p.R) if r not in (0, 7, 19)], dtype=np.uint32)
    cli_ = np.arange(p.R, dtype=np.uint32)
    objs = objectives(5)
    want = expected(o, srv, cli_, 5, objs)
    for kernel in KERNELS:
        sw, tops = run(dp, srv, cli_, 5, objs, kernel)
        assert sw.kernel_path() == path_of(kernel), kernel
        assert tops == want, kernel


# --------------------------------------------------------------------- 5 ---
def test_unsorted_servers_run_generic(gcp):
    p, dp, o = gcp
    srv = np.arange(p.R, dtype=np.uint32)[::-1].copy()
    srv[[3, 11]] = srv[[11, 3]]
    cli_ = np.arange(p.R, dtype=np.uint32)
    objs = objectives(5)
    sw, tops = run(dp, srv, cli_, 5, objs, None)
    assert sw.kernel_path() == "generic"
    assert tops == expected(o, srv, cli_, 5, objs)


def test_latency_above_4095_runs_generic(gcp):
    """One latency raised to 5000: off the packed fast path, values above 4095 in the keys."""
    p, _, _ = gcp
    lat = p.lat.astype(np.int64).copy()
    lat[2, 9] = lat[9, 2] = 5000
    q = Planet(p.names, lat)
    dq, o = DevicePlanet(q), O.OraclePlanet.of(q)
    srv = np.arange(q.R, dtype=np.uint32)
    objs = objectives(5)
    sw, tops = run(dq, srv, srv, 5, objs, None)
    assert sw.kernel_path() == "generic"
    assert tops == expected(o, srv, srv, 5, objs)


def test_extended_key_set_runs_generic(gcp):
    """[MDTM tt1, MDTM tw2C, MDTM fl1] on GCP n = 5: Tempo tiny f = 1 (q = 2,
    Input), Tempo write f = 2 (q = 3, Colocated) through leaderless_batch, and
    FPaxos under the best leader by mean (best_leader stat 0, then leader)."""
    p, dp, o = gcp
    n, nc = 5, p.R
    srv = np.arange(p.R, dtype=np.uint32)
    objs = [(MDTM, _lib.SLOT_TT1), (MDTM, _lib.SLOT_TW2 + _lib.SLOT_X_COLOCATED), (MDTM, _lib.SLOT_FL1)]
    cfgs = srv[colex_positions(p.R, n)]
    lv = o.leaderless_batch(cfgs, srv, [2, 3], threads=8)
    fl = np.array([o.leader(int(c[o.best_leader(c, srv, 2, 0)]), c, srv, 2) for c in cfgs], dtype=np.uint64)
    want = [top_of(key_of(MDTM, lv[:, 0, :nc])), top_of(key_of(MDTM, lv[:, 1, nc:])), top_of(key_of(MDTM, fl))]
    sw, tops = run(dp, srv, srv, n, objs, None, keys=_lib.KEYS_TEMPO_ALL_LEADERS)
    assert sw.kernel_path() == "generic"
    assert tops == want


# --------------------------------------------------------------------- 6 ---
def test_ties_arrive_through_the_deferred_path():
    """The twin planet of tests/test_gpu_tail.py (synthetic R=32, regions 4 and 5
    at 200 from all others and 50 from each other), n = 4 in full on the forced
    fast kernel: the 435 configs holding both twins tie exactly on the leader's
    COV, so the fast kernel defers each of them and their MDTM keys arrive
    through the generic fix-up and the merge."""
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
    objs = objectives(4)
    want = expected(o, srv, srv, 4, objs)
    sw, tops = run(dp, srv, srv, 4, objs, "fast")
    assert sw.kernel_path() == "fast"
    assert sw.deferred() >= 435
    assert tops == want


def test_all_configs_tie_overflow_fallback():
    """Planet.equidistant(7, 48), n = 5: every leader choice is an exact tie, so
    every one of the 1,712,304 configs defers, the queue overflows and the
    generic fallback recomputes the range.  Each list is ranks 0..99 under one
    key, which the oracle gives for rank 0."""
    _, p = Planet.equidistant(7, 48)
    dp, o = DevicePlanet(p), O.OraclePlanet.of(p)
    srv = np.arange(48, dtype=np.uint32)
    objs = objectives(5)
    vals, _ = o.compute_stats(srv[:5].reshape(1, 5), srv)
    sw, tops = run(dp, srv, srv, 5, objs, "fast")
    assert sw.kernel_path() == "fast"
    assert sw.deferred() == sw.total == 1712304
    for (kind, slot), t in zip(objs, tops):
        key = int(key_of(kind, slot_values(vals, slot, 48, 5))[0])
        assert t == [(key, r) for r in range(K)], (kind, slot)


# --------------------------------------------------------------------- 7 ---
def test_sharded_equals_single(gcp):
    """GCP n = 7: two shards through MultiDeviceSearch and search_topk, and one
    sweep launched over two rank ranges merged with merge_device, equal the
    single sweep (which equals the oracle)."""
    import torch

    p, dp, _ = gcp
    srv = np.arange(p.R, dtype=np.uint32)
    objs = objectives(7)
    want = gcp_expected(gcp, 7, objs)
    h = MultiDeviceSearch([dp, dp], srv, srv, 7, objectives=objs, K=K, ranking=None, digest=False)
    h.launch()
    assert h.result().tops == want
    assert search_topk([dp, dp], srv, srv, 7, objectives=objs, K=K, ranking=None, digest=False).tops == want
    sw = Sweep(dp, srv, srv, 7, objs, K=K, ranking=None)
    assert sw.kernel_path() == "fast"
    dev = torch.device("cuda", dp.device)
    st = torch.cuda.current_stream(dev).cuda_stream
    nb = sw.result_bytes()
    pair = torch.empty(2 * nb, dtype=torch.uint8, device=dev)
    out = torch.empty(nb, dtype=torch.uint8, device=dev)
    cut = 31_013  # (not a multiple of the block's lane count)
    sw.launch(0, cut, st)
    sw.result_device(pair.data_ptr(), st)
    sw.launch(cut, sw.total, st)
    sw.result_device(pair.data_ptr() + nb, st)
    sw.merge_device(pair.data_ptr(), 2, out.data_ptr(), st)
    assert sw.parse_block(out.cpu().numpy()).tops == want


# --------------------------------------------------------------------- 8 ---
def test_routing_and_refusals(gcp):
    """A forced group kernel refuses MDTM; the fast kernel's MDTM variant carries
    no maxima or lists, so forced fast refuses MDTM beside MAX, and AUTO runs
    MDTM beside MAX or a percentile on the generic kernel."""
    p, dp, _ = gcp
    srv = np.arange(p.R, dtype=np.uint32)
    with pytest.raises(_lib.BoteError, match="the group kernel does not compute MDTM objectives "
                                             r"\(fast or generic kernel\)") as e:
        Sweep(dp, srv, srv, 5, [(MEAN, AF1), (MDTM, AF1)], K=K, ranking=None, kernel="group")
    assert e.value.code == -1
    # a later sweep on the same planet is unaffected
    sw, tops = run(dp, srv, srv, 5, objectives(5), None)
    assert sw.kernel_path() == "fast"
    assert tops == gcp_expected(gcp, 5, objectives(5))
    with pytest.raises(_lib.BoteError, match="MDTM variant carries no maxima or lists") as e:
        Sweep(dp, srv, srv, 5, [(MDTM, AF1), (MAX, AF1)], K=K, ranking=None, kernel="fast")
    assert e.value.code == -1
    for objs in ([(MDTM, AF1), (MAX, AF1)], [(MDTM, AF1), (P(9500), AF1)]):
        sw, tops = run(dp, srv, srv, 5, objs, None)
        assert sw.kernel_path() == "generic", objs
        assert tops == gcp_expected(gcp, 5, objs), objs


# -------------------------------------------------------------------- 10 ---
def test_cli_prints_mdtm_and_sum(gcp):
    buf = io.StringIO()
    assert cli.main(["sweep", "--objectives", "mean:af1,mdtm:af1", "--n", "5"], out=buf) == 0
    doc = json.loads(buf.getvalue())
    want = gcp_expected(gcp, 5, objectives(5))
    assert [x["objective"] for x in doc["objectives"]] == ["mean:af1", "mdtm:af1"]
    mean, md = doc["objectives"]
    assert set(mean["top"][0]) == {"key", "rank", "regions"}
    assert [(int(x["key"]), x["rank"]) for x in mean["top"]] == want[0][:10]
    assert [(int(x["key"]), x["rank"]) for x in md["top"]] == want[1][:10]
    for x, (key, _) in zip(md["top"], want[1]):
        h, total = mdtm_key(key)
        assert (x["mdtm"], x["sum"]) == (2 * h / gcp[0].R ** 2, total)
        assert list(x) == ["key", "rank", "regions", "mdtm", "sum"]
