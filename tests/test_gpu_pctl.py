"""Percentile objectives of the streaming sweep (include/bote_hip.h
BOTE_OBJ_PCTL): key = (2 * Histogram::percentile(p) << 32) | sum of a slot, on
the fast kernel's sorted-list variant (bote_sweep.hip, FAST_LIST) and on the
generic kernel (bote_eval.hpp).

Every expected list comes from the CPU oracle: OraclePlanet.compute_stats (or
leaderless_batch / best_leader + leader for the extended key set) over the
sweep's configs in colex order gives each slot's per-client values; the order
statistic that _lib.percentile_index selects from them (checked against the
oracle's Histogram::percentile in tests/test_pctl_host.py) and their sum build
the key; the lists are the K least by (key, rank).  Every comparison is exact
equality of the full (key, rank) lists."""
import io
import json

import numpy as np
import pytest

import oracle as O
from fantoch_amd import _lib, cli
from fantoch_amd.bote import DevicePlanet, MultiDeviceSearch, Sweep, max_key, pctl_key, search_topk
from fantoch_amd.planet import Planet
from tests.host_keys import colex_positions, slot_values

pytestmark = pytest.mark.gpu

K = 100
MEAN, MAX, P = _lib.OBJ_MEAN, _lib.OBJ_MAX, _lib.OBJ_PCTL
AF1, FF1, AF2, FF2, E = 0, 1, 2, 3, 4
KERNELS = [None, "fast", "generic"]


def objectives(n):
    """needs over 20 clients: p95 2 (whole), p93 2, p85 4 (whole: the full list
    depth), p99 1, p90 3 (whole); over the n = 3, 5, 7, 9, 11 members: p75 2, 2, 3, 3, 4."""
    objs = [(MEAN, AF1), (P(9500), AF1), (P(9300), FF1), (P(8500), E), (P(9900), AF1), (P(7500), 5 + AF1),
            (P(7500), 5 + FF1)]
    if n // 2 >= 2:
        objs += [(P(9000), AF2)]
    return objs


def top_of(keys, k=K, base=0):
    """The k least (key, rank) of per-rank keys (rank = base + index), ascending."""
    keys = np.asarray(keys, dtype=np.uint64)
    order = np.lexsort((np.arange(len(keys)), keys))[:k]
    return [(int(keys[r]), base + int(r)) for r in order]


def key_of(kind, v):
    """Per-config key of one slot's values (ncfg, count)."""
    v = np.asarray(v, dtype=np.uint64)
    s = v.sum(axis=1)
    if kind == MEAN:
        return s
    if kind == MAX:
        return (v.max(axis=1) << np.uint64(32)) | s
    assert _lib.is_pctl(kind)
    idx, whole = _lib.percentile_index(kind & 0xFFFF, v.shape[1])
    a = np.sort(v, axis=1)
    twice = 2 * a[:, 0] if idx == 0 else a[:, idx - 1] + a[:, idx] if whole else 2 * a[:, idx - 1]
    return (twice << np.uint64(32)) | s


def expected(o, srv, cli_, n, objs, configs=None, base=0):
    """The oracle's top-K lists of a sweep over the n-subsets of `srv` (all of them, or `configs` positions)."""
    srv = np.asarray(srv, dtype=np.uint32)
    pos = colex_positions(len(srv), n) if configs is None else configs
    vals, _ = o.compute_stats(srv[pos], cli_, threads=8)
    return [top_of(key_of(kind, slot_values(vals, slot, len(cli_), n)), base=base) for kind, slot in objs]


def run(dp, srv, cli_, n, objs, kernel, keys=_lib.KEYS_BASE, rb=0, re=None):
    sw = Sweep(dp, srv, cli_, n, objs, K=K, ranking=None, kernel=kernel, keys=keys)
    sw.launch(rb, sw.total if re is None else re)
    return sw, sw.result().tops


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
    p = gcp[0]
    vals = gcp_values(gcp, n)
    return [top_of(key_of(kind, slot_values(vals, slot, p.R, n))) for kind, slot in objs]


# --------------------------------------------------------------------- 1 ---
@pytest.mark.parametrize("n", [3, 5, 7, 9, 11])
def test_gcp_full_sweep_vs_oracle(gcp, n):
    """GCP R=20 (nq = 5: the pipelined pair loop with an odd quad count), n = 3
    (one leaderless table), 5, 7 (two), 9 (two; the non-pipelined loop) and 11
    (three: the second qtab plane on the Input side; the colocated lists of the
    third table are the next test's), on auto (the list variant of the fast
    kernel), forced fast and forced generic
    (p75 over 11 members needs 4, the full list depth: still fast); then one
    sweep mixing MAX af1 with p95 and p99 af1: p99 over 20 clients is the
    maximum, so its records are the MAX records with T = 2 * max."""
    p, dp, _ = gcp
    srv = np.arange(p.R, dtype=np.uint32)
    objs = objectives(n)
    want = gcp_expected(gcp, n, objs)
    for kernel in KERNELS:
        sw, tops = run(dp, srv, srv, n, objs, kernel)
        assert sw.kernel_path() == ("generic" if kernel == "generic" else "fast"), kernel
        for (kind, slot), t, w in zip(objs, tops, want):
            assert t == w, (n, kernel, hex(kind), slot)
    mixed = [(MAX, AF1), (P(9500), AF1), (P(9900), AF1)]
    wantm = gcp_expected(gcp, n, mixed)
    assert wantm[1] == want[1] and wantm[2] == want[4]
    for kernel in KERNELS:
        sw, tops = run(dp, srv, srv, n, mixed, kernel)
        assert sw.kernel_path() == ("generic" if kernel == "generic" else "fast"), kernel
        assert tops == wantm, (n, kernel)
        assert [(2 * max_key(k)[0], max_key(k)[1], r) for k, r in tops[0]] == [pctl_key(k) + (r,) for k, r in tops[2]]


def test_gcp_n11_colocated_third_table_vs_oracle(gcp):
    """At n = 11 the third leaderless table is E's, and the only slot that reads
    its colocated values is eC (5 + E), which objectives(11) has no room for
    (MAXOBJ): p75 eC (needs 4 of the 11 members' values: the list variant's
    second list of the qtab read-back) and MAX eC (its first entry), beside p95
    e, on auto, forced fast and forced generic."""
    p, dp, _ = gcp
    srv = np.arange(p.R, dtype=np.uint32)
    assert _lib.percentile_index(7500, 11) == (8, False)  # (the 8th smallest = the 4th largest)
    objs = [(MEAN, AF1), (P(7500), 5 + E), (MAX, 5 + E), (P(9500), E)]
    want = gcp_expected(gcp, 11, objs)
    assert len({k for k, _ in want[1]}) > 1  # (the eC keys tell configs apart)
    for kernel in KERNELS:
        sw, tops = run(dp, srv, srv, 11, objs, kernel)
        assert sw.kernel_path() == ("generic" if kernel == "generic" else "fast"), kernel
        assert tops == want, kernel


# --------------------------------------------------------------------- 2 ---
def test_need_5_to_8_runs_generic(gcp):
    """p80 af1 needs 5 and p65 af1 needs 8 of the 20 clients' values: deeper than
    the fast kernel's lists, so AUTO takes the generic kernel and a forced fast
    kernel is refused; a later sweep on the same planet is unaffected."""
    p, dp, _ = gcp
    srv = np.arange(p.R, dtype=np.uint32)
    assert [_lib.percentile_index(bp, 20) for bp in (8000, 6500)] == [(16, True), (13, True)]
    objs = [(MEAN, AF1), (P(8000), AF1), (P(6500), AF1), (P(9500), AF1)]
    want = gcp_expected(gcp, 5, objs)
    for kernel in (None, "generic"):
        sw, tops = run(dp, srv, srv, 5, objs, kernel)
        assert sw.kernel_path() == "generic"
        assert tops == want, kernel
    for deep in (P(8000), P(6500)):
        with pytest.raises(_lib.BoteError, match="percentile lists are 4 deep") as e:
            Sweep(dp, srv, srv, 5, [(MEAN, AF1), (deep, AF1)], K=K, ranking=None, kernel="fast")
        assert e.value.code == -1
    with pytest.raises(_lib.BoteError, match="percentile needs more than 8") as e:
        Sweep(dp, srv, srv, 5, [(P(5000), AF1)], K=K, ranking=None)
    assert e.value.code == -4
    with pytest.raises(_lib.BoteError, match="the group kernel does not compute percentile objectives") as e:
        Sweep(dp, srv, srv, 5, [(MEAN, AF1), (P(9500), AF1)], K=K, ranking=None, kernel="group")
    assert e.value.code == -1
    objs5 = objectives(5)
    sw, tops = run(dp, srv, srv, 5, objs5, None)
    assert sw.kernel_path() == "fast"
    assert tops == gcp_expected(gcp, 5, objs5)


# --------------------------------------------------------------------- 3 ---
@pytest.mark.parametrize("ncli", [2, 3, 5, 6, 7, 13])
def test_client_remainders(gcp, ncli):
    """GCP n = 5 with the first 2, 3, 5, 6, 7, 13 regions as clients: p75 af1 and
    ff1 need 1, 2, 2, 2, 3, 4 values, so with 2 and 3 clients the list is deeper
    than the live clients and the remainder quad's dead clients (entered as 0)
    must not be selected; p50 af1 (needs 2, 2, 3, 4, 4) for the counts up to 7."""
    p, dp, o = gcp
    srv = np.arange(p.R, dtype=np.uint32)
    cli_ = np.arange(ncli, dtype=np.uint32)
    need = lambda bp: ncli - max(_lib.percentile_index(bp, ncli)[0], 1) + 1  # noqa: E731
    assert need(7500) == {2: 1, 3: 2, 5: 2, 6: 2, 7: 3, 13: 4}[ncli]
    objs = [(MEAN, AF1), (P(7500), AF1), (P(7500), FF1)]
    if ncli <= 7:
        assert need(5000) == {2: 2, 3: 2, 5: 3, 6: 4, 7: 4}[ncli]
        objs.append((P(5000), AF1))
    want = expected(o, srv, cli_, 5, objs)
    for kernel in KERNELS:
        sw, tops = run(dp, srv, cli_, 5, objs, kernel)
        assert sw.kernel_path() == ("generic" if kernel == "generic" else "fast"), kernel
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
        assert sw.kernel_path() == ("generic" if kernel == "generic" else "fast"), kernel
        assert tops == want, kernel


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
    """One latency raised to 5000: off the packed fast path, and values above 4095 in the lists."""
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


# --------------------------------------------------------------------- 5 ---
def test_extended_key_set_runs_generic(gcp):
    """[p95 tt1, p50 tw2C, p95 fl1, p85 fl2] on GCP n = 5: Tempo tiny f = 1 (q = 2,
    Input), Tempo write f = 2 (q = 3, Colocated: the median of 5 members) through
    leaderless_batch, and FPaxos under the best leader by mean (best_leader stat
    0, then leader)."""
    p, dp, o = gcp
    n, nc = 5, p.R
    srv = np.arange(p.R, dtype=np.uint32)
    objs = [(P(9500), _lib.SLOT_TT1), (P(5000), _lib.SLOT_TW2 + _lib.SLOT_X_COLOCATED), (P(9500), _lib.SLOT_FL1),
            (P(8500), _lib.SLOT_FL2)]
    cfgs = srv[colex_positions(p.R, n)]
    lv = o.leaderless_batch(cfgs, srv, [2, 3], threads=8)
    fl1 = np.array([o.leader(int(c[o.best_leader(c, srv, 2, 0)]), c, srv, 2) for c in cfgs], dtype=np.uint64)
    fl2 = np.array([o.leader(int(c[o.best_leader(c, srv, 3, 0)]), c, srv, 3) for c in cfgs], dtype=np.uint64)
    want = [top_of(key_of(objs[0][0], lv[:, 0, :nc])), top_of(key_of(objs[1][0], lv[:, 1, nc:])),
            top_of(key_of(objs[2][0], fl1)), top_of(key_of(objs[3][0], fl2))]
    sw, tops = run(dp, srv, srv, n, objs, None, keys=_lib.KEYS_TEMPO_ALL_LEADERS)
    assert sw.kernel_path() == "generic"
    assert tops == want


# --------------------------------------------------------------------- 6 ---
def test_percentile_keys_arrive_through_the_deferred_path():
    """The twin planet of tests/test_gpu_tail.py's deferred-path test (synthetic
    R=32, regions 4 and 5 at 200 from all others and 50 from each other), n = 4
    in full on the forced fast kernel: the 435 configs holding both twins have
    their leader by an exact COV tie, so the fast kernel defers each of them and
    their percentile keys come from the generic fix-up and the merge."""
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
    # over 32 clients: p95 needs 3, p90 4; over 4 members: p75 2 (whole)
    objs = [(MEAN, AF1), (P(9500), AF1), (P(9500), FF1), (P(9000), E), (P(7500), 5 + AF1), (P(7500), 5 + FF1),
            (P(9500), AF2), (MAX, FF1)]
    pos = colex_positions(32, 4)
    want = expected(o, srv, srv, 4, objs)
    twins = [r for r, c in enumerate(pos.tolist()) if 4 in c and 5 in c]
    assert len(twins) == 435
    # the deferred configs do reach the lists: the MAX ff1 list is the first K of them (tests/test_gpu_tail.py)
    assert [r for _, r in want[7]] == twins[:K]
    sw, tops = run(dp, srv, srv, 4, objs, "fast")
    assert sw.kernel_path() == "fast"
    assert sw.deferred() >= 435
    assert tops == want


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
def test_synthetic_r64_n7_window():
    """Synthetic R=64 n=7, one window of 65,536 colex ranks: 16 full client
    quads (eight pipelined pairs and the flush), two leaderless tables.  Over
    64 clients p95 needs 4 (the full list depth) and p99 needs 2."""
    p = Planet.synthetic(64)
    dp, o = DevicePlanet(p), O.OraclePlanet.of(p)
    srv = np.arange(64, dtype=np.uint32)
    rb, re = 5_000_000, 5_000_000 + 65_536
    assert [_lib.percentile_index(bp, 64) for bp in (9500, 9900)] == [(61, False), (63, False)]
    objs = [(MEAN, AF1), (P(9500), AF1), (P(9900), E), (P(9500), FF1), (P(9500), AF2)]
    cfg = np.array([_lib.colex_unrank(r, 7, 64) for r in range(rb, re)], dtype=np.uint32)
    want = expected(o, srv, srv, 7, objs, configs=cfg, base=rb)
    for kernel in ("fast", "generic"):
        sw, tops = run(dp, srv, srv, 7, objs, kernel, rb=rb, re=re)
        assert sw.kernel_path() == kernel
        assert tops == want, kernel


# --------------------------------------------------------------------- 9 ---
def test_cli_prints_percentile_and_sum(gcp):
    buf = io.StringIO()
    assert cli.main(["sweep", "--objectives", "mean:af1,p95:af1", "--n", "5"], out=buf) == 0
    doc = json.loads(buf.getvalue())
    want = gcp_expected(gcp, 5, [(MEAN, AF1), (P(9500), AF1)])
    assert [x["objective"] for x in doc["objectives"]] == ["mean:af1", "p95:af1"]
    mean, pc = doc["objectives"]
    assert set(mean["top"][0]) == {"key", "rank", "regions"}
    assert [(int(x["key"]), x["rank"]) for x in mean["top"]] == want[0][:10]
    assert [(int(x["key"]), x["rank"]) for x in pc["top"]] == want[1][:10]
    for x, (key, _) in zip(pc["top"], want[1]):
        twice, total = pctl_key(key)
        assert (x["percentile"], x["sum"]) == (twice / 2, total)
        assert list(x) == ["key", "rank", "regions", "percentile", "sum"]
