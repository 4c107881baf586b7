"""MAX (worst-client) objectives of the streaming sweep: key = (max << 32) | sum
of a slot (include/bote_hip.h BOTE_OBJ_MAX), on the fast kernel's TAIL variant
(bote_sweep.hip) and on the generic kernel (bote_eval.hpp).

Every expected list comes from the CPU oracle: OraclePlanet.compute_stats over
the sweep's configs in colex order gives each slot's per-client values, whose
max and sum build the key; the lists are the K least by (key, rank).  Every
comparison is exact equality of the full (key, rank) lists."""
import io
import json

import numpy as np
import pytest

import oracle as O
from fantoch_amd import _lib, cli
from fantoch_amd.bote import (DEFAULT_RANKING, DevicePlanet, MultiDeviceSearch, Sweep, eval_configs, max_key,
                              search_topk)
from fantoch_amd.planet import Planet
from tests.host_keys import colex_positions, slot_values

pytestmark = pytest.mark.gpu

K = 100
MEAN, MAX = _lib.OBJ_MEAN, _lib.OBJ_MAX
AF1, FF1, AF2, FF2, E = 0, 1, 2, 3, 4
KERNELS = [None, "fast", "generic"]


def objectives(n):
    objs = [(MEAN, AF1), (MAX, AF1), (MAX, FF1), (MAX, E), (MAX, 5 + AF1), (MAX, 5 + FF1)]
    if n // 2 >= 2:
        objs += [(MAX, AF2), (MAX, 5 + FF2)]
    return objs


def top_of(keys, k=K):
    """The k least (key, rank) of per-rank keys, ascending."""
    keys = np.asarray(keys, dtype=np.uint64)
    order = np.lexsort((np.arange(len(keys)), keys))[:k]
    return [(int(keys[r]), int(r)) for r in order]


def key_of(kind, v):
    """Per-config key of one slot's values (ncfg, count)."""
    s = v.sum(axis=1)
    return s if kind == MEAN else (v.max(axis=1) << np.uint64(32)) | s


def expected(o, srv, cli, n, objs):
    """The oracle's top-K lists of a full sweep over the n-subsets of `srv`."""
    srv = np.asarray(srv, dtype=np.uint32)
    vals, _ = o.compute_stats(srv[colex_positions(len(srv), n)], cli, threads=8)
    return [top_of(key_of(kind, slot_values(vals, slot, len(cli), n))) for kind, slot in objs]


def run(dp, srv, cli, n, objs, kernel, keys=_lib.KEYS_BASE):
    sw = Sweep(dp, srv, cli, n, objs, K=K, ranking=None, kernel=kernel, keys=keys)
    sw.launch(0, sw.total)
    return sw, sw.result().tops


@pytest.fixture(scope="module")
def gcp():
    p = Planet.new()
    return p, DevicePlanet(p), O.OraclePlanet.of(p)


_WANT = {}


def gcp_expected(gcp, n):
    """The full-sweep lists of GCP with every region as server and client (computed once per n)."""
    p, _, o = gcp
    if n not in _WANT:
        srv = np.arange(p.R, dtype=np.uint32)
        _WANT[n] = expected(o, srv, srv, n, objectives(n))
    return _WANT[n]


# ------------------------------------------------------------------ 1, 8 ---
@pytest.mark.parametrize("n", [3, 5, 7, 9, 11])
def test_gcp_full_sweep_vs_oracle(gcp, n):
    """GCP R=20 (nq = 5: the pipelined pair loop with an odd quad count), n = 3
    (one leaderless table), 5, 7 (two), 9 (two; the non-pipelined loop) and 11
    (three: the second qtab plane on the Input side, the smallest odd n that has
    one; its colocated side is the next test's), on auto (the
    TAIL fast kernel), forced fast and forced generic.  Then, without the
    oracle: every reported record's key is rebuilt from eval_configs'
    per-client values of that rank."""
    p, dp, _ = gcp
    srv = np.arange(p.R, dtype=np.uint32)
    objs, want = objectives(n), gcp_expected(gcp, n)
    for kernel in KERNELS:
        sw, tops = run(dp, srv, srv, n, objs, kernel)
        assert sw.kernel_path() == ("generic" if kernel == "generic" else "fast"), kernel
        assert tops == want, (n, kernel)
    ranks = sorted({r for t in want for _, r in t})
    cfg = np.array([_lib.colex_unrank(r, n, p.R) for r in ranks], dtype=np.uint32)
    ev = eval_configs(dp, srv, srv, n, configs=cfg).vals.astype(np.uint64)
    row = {r: i for i, r in enumerate(ranks)}
    for (kind, slot), t in zip(objs, want):
        v = slot_values(ev, slot, p.R, n)
        for key, r in t:
            x = v[row[r]]
            assert key == (int(x.sum()) if kind == MEAN else (int(x.max()) << 32) | int(x.sum())), (kind, slot, r)
            if kind == MAX:
                assert max_key(key) == (int(x.max()), int(x.sum()))


def test_gcp_n11_colocated_third_table_vs_oracle(gcp):
    """At n = 11 the third leaderless table is E's, and the only slot that reads
    its colocated values is eC (5 + E), which objectives(11) has no room for
    (MAXOBJ): MAX eC (the Q phase's maximum of the third table), beside MAX e
    and MAX af2C, on auto, forced fast and forced generic."""
    p, dp, o = gcp
    srv = np.arange(p.R, dtype=np.uint32)
    objs = [(MEAN, AF1), (MAX, 5 + E), (MAX, E), (MAX, 5 + AF2)]
    want = expected(o, srv, srv, 11, objs)
    assert len({k for k, _ in want[1]}) > 1  # (the eC keys tell configs apart)
    for kernel in KERNELS:
        sw, tops = run(dp, srv, srv, 11, objs, kernel)
        assert sw.kernel_path() == ("generic" if kernel == "generic" else "fast"), kernel
        assert tops == want, kernel


# --------------------------------------------------------------------- 2 ---
@pytest.mark.parametrize("ncli", [2, 3, 5, 6, 7, 13])
def test_client_remainders(gcp, ncli):
    """GCP n = 5 with the first 2, 3, 5, 6, 7, 13 regions as clients: no full
    quad with 2 and 3 clients left, a remainder of 1, 2 and 3 after one quad, and
    three quads plus one client (pair loop, single quad, remainder), all with a
    separate region-row table; the remainder's dead clients count 0 in the max."""
    p, dp, o = gcp
    srv = np.arange(p.R, dtype=np.uint32)
    cli_ = np.arange(ncli, dtype=np.uint32)
    objs = objectives(5)
    want = expected(o, srv, cli_, 5, objs)
    for kernel in KERNELS:
        sw, tops = run(dp, srv, cli_, 5, objs, kernel)
        assert sw.kernel_path() == ("generic" if kernel == "generic" else "fast"), kernel
        assert tops == want, (ncli, kernel)


# --------------------------------------------------------------------- 3 ---
def test_server_subset_in_name_order(gcp):
    """17 of the 20 regions as servers (positions differ from region ids), all 20 as clients."""
    p, dp, o = gcp
    srv = np.array([r for r in range(p.R) if r not in (0, 7, 19)], dtype=np.uint32)
    cli_ = np.arange(p.R, dtype=np.uint32)
    objs = objectives(5)
    want = expected(o, srv, cli_, 5, objs)
    for kernel in KERNELS:
        sw, tops = run(dp, srv, cli_, 5, objs, kernel)
        assert sw.kernel_path() == ("generic" if kernel == "generic" else "fast"), kernel
        assert tops == want, kernel


# --------------------------------------------------------------------- 4 ---
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
    """One latency raised to 5000: off the packed fast path, and a max above 4095 in the keys."""
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
    """[MAX tt1, MAX tw2C, MAX fl1] on GCP n = 5: Tempo tiny f = 1 (q = 2, Input),
    Tempo write f = 2 (q = 3, Colocated) through leaderless_batch, and FPaxos
    under the best leader by mean (best_leader stat 0, then leader)."""
    p, dp, o = gcp
    n, nc = 5, p.R
    srv = np.arange(p.R, dtype=np.uint32)
    objs = [(MAX, _lib.SLOT_TT1), (MAX, _lib.SLOT_TW2 + _lib.SLOT_X_COLOCATED), (MAX, _lib.SLOT_FL1)]
    cfgs = srv[colex_positions(p.R, n)]
    lv = o.leaderless_batch(cfgs, srv, [2, 3], threads=8)
    fl = np.array([o.leader(int(c[o.best_leader(c, srv, 2, 0)]), c, srv, 2) for c in cfgs], dtype=np.uint64)
    want = [top_of(key_of(MAX, lv[:, 0, :nc])), top_of(key_of(MAX, lv[:, 1, nc:])), top_of(key_of(MAX, fl))]
    sw, tops = run(dp, srv, srv, n, objs, None, keys=_lib.KEYS_TEMPO_ALL_LEADERS)
    assert sw.kernel_path() == "generic"
    assert tops == want


# --------------------------------------------------------------------- 5 ---
def test_ties_arrive_through_the_deferred_path():
    """The twin planet of test_group_deferred_leader_lanes_equal_generic
    (synthetic R=32, regions 4 and 5 at 200 from all others and 50 from each
    other), n = 4 in full (35,960 configs) on the forced fast kernel.  Measured
    on the oracle: all 435 configs holding both twins have twin 4 as leader by
    an exact COV tie (so the fast kernel defers each of them: 435 is that
    oracle-measured count), and all 435 share one MAX ff1 key (max 250 and one
    sum), the least of the sweep.  So the MAX ff1 list is the 100 lowest of
    those 435 ranks: every record arrives through the generic fix-up and the
    merge, ordered by rank alone."""
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
    pos = colex_positions(32, 4)
    want = expected(o, srv, srv, 4, objs)
    twins = [r for r, c in enumerate(pos.tolist()) if 4 in c and 5 in c]
    assert len(twins) == 435
    ff1 = want[objs.index((MAX, FF1))]
    assert [r for _, r in ff1] == twins[:K] and len({k for k, _ in ff1}) == 1 and max_key(ff1[0][0])[0] == 250
    sw, tops = run(dp, srv, srv, 4, objs, "fast")
    assert sw.kernel_path() == "fast"
    assert sw.deferred() >= 435
    assert tops == want


# --------------------------------------------------------------------- 6 ---
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
    objs, want = objectives(7), gcp_expected(gcp, 7)
    h = MultiDeviceSearch([dp, dp], srv, srv, 7, objectives=objs, K=K, ranking=None, digest=False)
    h.launch()
    assert h.result().tops == want
    assert search_topk([dp, dp], srv, srv, 7, objectives=objs, K=K, ranking=None, digest=False).tops == want
    sw = Sweep(dp, srv, srv, 7, objs, K=K, ranking=None)
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


# --------------------------------------------------------------------- 9 ---
def test_forced_group_refuses_max(gcp):
    p, dp, _ = gcp
    srv = np.arange(p.R, dtype=np.uint32)
    with pytest.raises(_lib.BoteError, match="the group kernel does not compute MAX objectives") as e:
        Sweep(dp, srv, srv, 5, [(MEAN, AF1), (MAX, AF1)], K=K, ranking=None, kernel="group")
    assert e.value.code == -1
    # a later sweep on the same planet is unaffected
    sw, tops = run(dp, srv, srv, 5, objectives(5), None)
    assert tops == gcp_expected(gcp, 5)


# -------------------------------------------------------------------- 10 ---
def test_cli_prints_max_and_sum(gcp):
    buf = io.StringIO()
    assert cli.main(["sweep", "--objectives", "mean:af1,max:af1", "--n", "5"], out=buf) == 0
    doc = json.loads(buf.getvalue())
    want = gcp_expected(gcp, 5)
    assert [x["objective"] for x in doc["objectives"]] == ["mean:af1", "max:af1"]
    mean, mx = doc["objectives"]
    assert set(mean["top"][0]) == {"key", "rank", "regions"}
    assert [(int(x["key"]), x["rank"]) for x in mean["top"]] == want[0][:10]
    assert [(int(x["key"]), x["rank"]) for x in mx["top"]] == want[1][:10]
    first = mx["top"][0]
    assert (first["max"], first["sum"]) == max_key(want[1][0][0])
    assert list(first) == ["key", "rank", "regions", "max", "sum"]
