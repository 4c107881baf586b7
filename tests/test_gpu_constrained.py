"""Constrained sweeps (bote_sweep_create_constrained, Sweep(constraints=...)):
only the configs whose constraint keys are within their bounds are offered to
the lists; the valid count and the digest stay the unconstrained sweep's; the
admitted configs are counted.  On the fast kernel's constrained variant (with
the generic kernel's fix-up of deferred configs and its overflow fallback) and
on the generic kernel's.

Every expected list is built on the CPU: from the oracle's complete order
(OraclePlanet.sweep with K = every config) filtered to the admitted ranks and
cut to K (tests/constrained_expect.py), or from per-config keys built of the
oracle's per-client values (tests/host_keys.py).  Every comparison is exact
equality, and every test that applies a real bound first asserts on the CPU side
that the bound bites: 0 < admitted < total and an expectation that differs from
the unconstrained one."""
import math

import numpy as np
import pytest

import oracle as O
from fantoch_amd import _lib
from fantoch_amd._lib import BoteError
from fantoch_amd.bote import DEFAULT_RANKING, DevicePlanet, Sweep
from fantoch_amd.planet import Planet
from tests import constrained_expect as X
from tests.constrained_expect import AF1, AF2, COV, E, FF1, MAX, MDTM, MEAN, NAN_KEY, OBJS, SCORE, U64
from tests.host_keys import colex_positions, key_of, slot_values, top_of

pytestmark = pytest.mark.gpu

K = 100
KERNELS = [None, "fast", "generic"]
P = _lib.OBJ_PCTL


@pytest.fixture(scope="module")
def gcp():
    p = Planet.new()
    return p, DevicePlanet(p), O.OraclePlanet.of(p)


_FULL = {}


def full_order(gcp, n):
    """(lists, valid, digest) of GCP's complete order for OBJS, computed once per n."""
    p, _, o = gcp
    if n not in _FULL:
        _FULL[n] = X.full_order(o, p.R, n)
    return _FULL[n]


def run(dp, R, n, objs, cons, kernel, ranking=DEFAULT_RANKING, rb=0, re=None):
    srv = np.arange(R, dtype=np.uint32)
    sw = Sweep(dp, srv, srv, n, objs, K=K, ranking=ranking, digest=True, kernel=kernel, constraints=cons)
    sw.launch(rb, sw.total if re is None else re)
    return sw, sw.result()


def path_of(kernel):
    return "generic" if kernel == "generic" else "fast"


# --------------------------------------------------------------------- 1 ---
@pytest.mark.parametrize("case", list(X.CASES))
@pytest.mark.parametrize("n", [3, 5])
def test_against_the_oracles_full_order(gcp, n, case):
    """GCP, every region a server and a client, n = 3 (1,140 configs, 47 valid) and n = 5 (15,504,
    839 valid), K = 100, on auto, forced fast and forced generic; bounds at the key of record
    total // d of the constraint's own complete list.  The admitted counts and the admitted valid
    configs are the ones measured on the CPU oracle (X.CASES)."""
    p, dp, _ = gcp
    lists, valid, digest = full_order(gcp, n)
    total = math.comb(p.R, n)
    assert (total, valid) == {3: (1140, 47), 5: (15504, 839)}[n]
    cons = X.case_constraints(lists, OBJS, total, case)
    adm = X.admitted_ranks(lists, OBJS, cons)
    want = X.filtered(lists, adm, K)
    n_adm, n_score = X.CASES[case][1][n]
    # the constraint bites, by the figures measured on the oracle
    assert len(adm) == n_adm and 0 < n_adm < total and want != [lst[:K] for lst in lists]
    score_all = [rec for rec in lists[0] if rec[1] in adm]
    assert n_score is None or len(score_all) == n_score
    assert len(want[0]) == min(len(score_all), K) and all(len(w) == K for w in want[1:])
    assert len(cons) + len(OBJS) <= 8
    for kernel in KERNELS:
        sw, res = run(dp, p.R, n, OBJS, cons, kernel)
        print(n, case, kernel, sw.kernel_path(), sw.admitted(), res.valid, [len(t) for t in res.tops])
        assert sw.kernel_path() == path_of(kernel), kernel
        assert res.tops == want, (n, case, kernel)
        assert sw.admitted() == n_adm, kernel
        assert (res.valid, res.digest) == (valid, digest), kernel  # not filtered


@pytest.mark.parametrize("n", [3, 5])
def test_no_bound_every_bound_zero_and_nan(gcp, n):
    """On each path: every bound 2^64 - 1 is the plain sweep in lists, valid count and digest, with
    admitted == total; every bound 0 admits nothing (no key is 0) and leaves every list empty; a COV
    bound of the NaN pattern admits every finite key."""
    p, dp, _ = gcp
    lists, valid, digest = full_order(gcp, n)
    total = math.comb(p.R, n)
    srv = np.arange(p.R, dtype=np.uint32)
    assert min(k for lst in lists[1:] for k, _ in lst) > 0
    assert max(k for k, _ in lists[3]) < NAN_KEY and max(k for k, _ in lists[4]) < NAN_KEY
    kinds = [(MEAN, FF1), (COV, 5 + FF1)]
    for kernel in KERNELS:
        plain = Sweep(dp, srv, srv, n, OBJS, K=K, ranking=DEFAULT_RANKING, digest=True, kernel=kernel)
        plain.launch()
        pr = plain.result()
        assert pr.tops == [lst[:K] for lst in lists] and (pr.valid, pr.digest) == (valid, digest)
        sw, res = run(dp, p.R, n, OBJS, [(k, s, U64) for k, s in kinds], kernel)
        assert (res.tops, res.valid, res.digest) == (pr.tops, pr.valid, pr.digest), kernel
        assert sw.admitted() == total, kernel
        sw, res = run(dp, p.R, n, OBJS, [(k, s, 0) for k, s in kinds], kernel)
        assert res.tops == [[] for _ in OBJS] and sw.admitted() == 0, kernel
        assert (res.valid, res.digest) == (valid, digest), kernel
        sw, res = run(dp, p.R, n, OBJS, [(COV, AF1, NAN_KEY), (COV, 5 + FF1, NAN_KEY)], kernel)
        assert (res.tops, res.valid, res.digest) == (pr.tops, pr.valid, pr.digest), kernel
        assert sw.admitted() == total, kernel


# --------------------------------------------------------------------- 2 ---
_VALS = {}


def gcp_values(gcp, n):
    p, _, o = gcp
    if n not in _VALS:
        srv = np.arange(p.R, dtype=np.uint32)
        _VALS[n] = o.compute_stats(srv[colex_positions(p.R, n)], srv, threads=8)[0]
    return _VALS[n]


TAIL_CASES = {
    # objectives, constraint kinds, the path on auto / forced fast (None: forced fast is refused), and d:
    # the bound is the key at index total // d of the constraint's ascending keys (3, or 10 where at
    # total // 3 the bound leaves the 100 best of a list as they are)
    "list": ([(MEAN, AF1), (MAX, AF1)], [(P(9500), AF1), (MAX, FF1)], "fast", 3),
    "mdtm": ([(MEAN, AF1)], [(MDTM, AF1)], "fast", 3),
    "mdtm_beside_max": ([(MEAN, AF1), (MAX, AF1)], [(MDTM, AF1)], None, 10),
    "deep_percentile": ([(MEAN, AF1)], [(P(7000), AF1)], None, 10),
    "max": ([(MEAN, FF1), (MEAN, E)], [(MAX, 5 + FF1), (MAX, E)], "fast", 3),
    "colocated": ([(MEAN, AF1), (MDTM, 5 + AF1)], [(MDTM, 5 + FF1), (MDTM, E)], "fast", 3),
}


@pytest.mark.parametrize("case", list(TAIL_CASES))
def test_tail_kinds(gcp, case):
    """GCP n = 5: MAX, percentile and MDTM constraints, keys by their definitions over the oracle's
    per-client values (host_keys.key_of); each bound is the key of the config at index total // d of
    the constraint's ascending keys (TAIL_CASES).  The list variant serves a percentile and a MAX constraint, the
    MDTM variant an MDTM one; MDTM beside MAX and a percentile that needs 7 values run the generic
    kernel (forced fast refuses)."""
    p, dp, _ = gcp
    n, nc = 5, p.R
    objs, ckinds, fast_path, d = TAIL_CASES[case]
    vals = gcp_values(gcp, n)
    total = len(vals)
    assert total == 15504
    if case == "deep_percentile":
        assert _lib.percentile_index(7000, nc)[0] == 14  # the 7 largest of 20 decide it
    keys = {e: key_of(e[0], slot_values(vals, e[1], nc, n)) for e in objs + ckinds}
    cons = [(k, s, int(np.sort(keys[(k, s)])[total // d])) for k, s in ckinds]
    mask = np.ones(total, bool)
    for k, s, b in cons:
        mask &= keys[(k, s)] <= np.uint64(b)
    ranks = np.nonzero(mask)[0]
    n_adm = len(ranks)
    want = [top_of(keys[e][mask], K, ranks) for e in objs]
    # the constraints bite, in every list
    assert 0 < n_adm < total and all(w != top_of(keys[e], K) for w, e in zip(want, objs))
    srv = np.arange(p.R, dtype=np.uint32)
    plain = Sweep(dp, srv, srv, n, objs, K=K, ranking=None, digest=True, kernel="generic")
    plain.launch()
    pr = plain.result()
    for kernel in KERNELS:
        if kernel == "fast" and fast_path is None:
            with pytest.raises(BoteError) as ei:
                run(dp, p.R, n, objs, cons, kernel, ranking=None)
            assert ei.value.code == -1
            continue
        sw, res = run(dp, p.R, n, objs, cons, kernel, ranking=None)
        print(case, kernel, sw.kernel_path(), sw.admitted(), n_adm)
        assert sw.kernel_path() == ("generic" if kernel == "generic" or fast_path is None else fast_path), kernel
        assert res.tops == want, (case, kernel)
        assert sw.admitted() == n_adm, kernel
        assert (res.valid, res.digest) == (pr.valid, pr.digest), kernel


# --------------------------------------------------------------------- 3 ---
@pytest.fixture(scope="module")
def twin():
    """The twin planet of tests/test_gpu_tail.py (synthetic R = 32, regions 4 and 5 at 200 from all
    others and 50 from each other), n = 4: its complete order, and the 435 ranks holding both twins."""
    base = Planet.synthetic(32)
    lat = base.lat.astype(np.int64).copy()
    for t in (4, 5):
        lat[t, :] = 200
        lat[:, t] = 200
    lat[4, 4] = lat[5, 5] = 0
    lat[4, 5] = lat[5, 4] = 50
    p = Planet(base.names, lat)
    lists, valid, digest = X.full_order(O.OraclePlanet.of(p), 32, 4)
    twins = {r for r, c in enumerate(colex_positions(32, 4).tolist()) if 4 in c and 5 in c}
    assert len(twins) == 435 and valid == 354 and len(lists[1]) == 35960
    return p, DevicePlanet(p), lists, valid, digest, twins


@pytest.mark.parametrize("d,n_adm,n_twin", [(10, 3598, 27), (4, 8991, 419)])
def test_deferred_configs_are_admitted_or_rejected_by_the_fix_up(twin, d, n_adm, n_twin):
    """Forced fast: the 435 configs holding both twins defer (an exact COV tie between the leaders),
    so the generic kernel's constrained fix-up decides them: with (COV, af1) bounded at its list's
    record total // d some of them are admitted and some rejected (the counts measured on the
    oracle).  The lists equal the oracle's filtered order and the forced generic kernel's; the
    valid count and the digest are unchanged."""
    p, dp, lists, valid, digest, twins = twin
    total = 35960
    cons = [(COV, AF1, X.bound_at(lists[OBJS.index((COV, AF1))], total // d))]
    adm = X.admitted_ranks(lists, OBJS, cons)
    want = X.filtered(lists, adm, K)
    assert len(adm) == n_adm and len(adm & twins) == n_twin and 0 < n_twin < 435
    assert 0 < n_adm < total and want != [lst[:K] for lst in lists]
    sw, res = run(dp, 32, 4, OBJS, cons, "fast")
    assert sw.kernel_path() == "fast" and sw.deferred() >= 435
    gw, gres = run(dp, 32, 4, OBJS, cons, "generic")
    print(d, sw.deferred(), sw.admitted(), gw.admitted(), res.valid)
    assert res.tops == want and gres.tops == want
    assert sw.admitted() == n_adm and gw.admitted() == n_adm
    assert (res.valid, res.digest) == (valid, digest) == (gres.valid, gres.digest) and valid == 354


# --------------------------------------------------------------------- 4 ---
@pytest.mark.parametrize("below", [0, 1])
def test_overflow_fallback_counts_the_range_once(below):
    """Planet.equidistant(7, 48), n = 5, forced fast: every one of the 1,712,304 configs defers, the
    queue overflows and the generic fallback recomputes the range; every config has one key per
    slot.  A MEAN constraint at that key admits all (each list is ranks 0..99, and the count is the
    fallback's alone: the range once); at that key - 1 it admits none."""
    _, p = Planet.equidistant(7, 48)
    dp, o = DevicePlanet(p), O.OraclePlanet.of(p)
    srv = np.arange(48, dtype=np.uint32)
    objs = [(MEAN, AF1), (MEAN, FF1), (MEAN, E)]
    vals, _ = o.compute_stats(srv[:5].reshape(1, 5), srv)
    key = {e: int(key_of(MEAN, slot_values(vals, e[1], 48, 5))[0]) for e in objs}
    assert key[(MEAN, FF1)] > 1
    sw, res = run(dp, 48, 5, objs, [(MEAN, FF1, key[(MEAN, FF1)] - below)], "fast", ranking=None)
    total = 1712304
    assert sw.kernel_path() == "fast" and sw.total == total
    assert sw.deferred() == total
    if below:
        assert sw.admitted() == 0 and res.tops == [[], [], []]
    else:
        assert sw.admitted() == total
        assert res.tops == [[(key[e], r) for r in range(K)] for e in objs]


# --------------------------------------------------------------------- 5 ---
def test_range_split_merge_and_checkpoints(gcp, tmp_path):
    """GCP n = 5: two launches over the halves of the rank space, merged with merge_device, equal
    one launch; their admitted counts add to the full one; run_checkpointed in small chunks gives
    the same lists."""
    import torch

    p, dp, _ = gcp
    n = 5
    lists, valid, digest = full_order(gcp, n)
    total = math.comb(p.R, n)
    cons = X.case_constraints(lists, OBJS, total, "mean_e")
    adm = X.admitted_ranks(lists, OBJS, cons)
    want = X.filtered(lists, adm, K)
    assert 0 < len(adm) < total and want != [lst[:K] for lst in lists]
    half = total // 2
    lo = sum(1 for r in adm if r < half)
    assert 0 < lo < len(adm)
    for kernel in (None, "generic"):
        sw, res = run(dp, p.R, n, OBJS, cons, kernel)
        assert res.tops == want and sw.admitted() == len(adm)
        nb = sw.result_bytes()
        dev = torch.device("cuda", dp.device)
        pair = torch.empty(2 * nb, dtype=torch.uint8, device=dev)
        out = torch.empty(nb, dtype=torch.uint8, device=dev)
        st = torch.cuda.current_stream(dev).cuda_stream
        sw.launch(0, half, st)
        sw.result_device(pair.data_ptr(), st)
        a0 = sw.admitted(st)
        sw.launch(half, total, st)
        sw.result_device(pair.data_ptr() + nb, st)
        a1 = sw.admitted(st)
        sw.merge_device(pair.data_ptr(), 2, out.data_ptr(), st)
        torch.cuda.synchronize(dev)
        merged = sw.parse_block(out.cpu().numpy())
        assert (a0, a1) == (lo, len(adm) - lo), kernel
        assert (merged.tops, merged.valid, merged.digest) == (want, valid, digest), kernel
        ck = sw.run_checkpointed(str(tmp_path / f"ck_{kernel}.npz"), chunk=4000)
        assert (ck.tops, ck.valid, ck.digest) == (want, valid, digest), kernel
    # a checkpoint under other bounds is refused
    other = Sweep(dp, np.arange(p.R, dtype=np.uint32), np.arange(p.R, dtype=np.uint32), n, OBJS, K=K,
                  ranking=DEFAULT_RANKING, digest=True, constraints=[(MEAN, E, 1)])
    with pytest.raises(ValueError):
        other.run_checkpointed(str(tmp_path / "ck_None.npz"), chunk=4000)


# --------------------------------------------------------------------- 6 ---
def test_no_constraints_through_the_new_entry_plans_as_before(gcp):
    """constraints=[] takes bote_sweep_create_constrained with n_con = 0: the same path as
    bote_sweep_create_keys (GCP n = 5 on auto, and a synthetic R = 32, n = 4 sweep whose path on
    auto is the group kernel), the same lists, valid count and digest, and admitted == the range."""
    p, dp, _ = gcp
    lists, valid, digest = full_order(gcp, 5)
    syn = Planet.synthetic(32)
    sdp = DevicePlanet(syn)
    for planet, d, n, kernels in ((p, dp, 5, [None, "fast", "generic"]), (syn, sdp, 4, [None, "group", "fast"])):
        srv = np.arange(planet.R, dtype=np.uint32)
        for kernel in kernels:
            plain = Sweep(d, srv, srv, n, OBJS, K=K, ranking=DEFAULT_RANKING, digest=True, kernel=kernel)
            sw = Sweep(d, srv, srv, n, OBJS, K=K, ranking=DEFAULT_RANKING, digest=True, kernel=kernel, constraints=[])
            assert sw.kernel_path() == plain.kernel_path(), (planet.R, kernel)
            assert sw.geometry() == plain.geometry(), (planet.R, kernel)
            plain.launch()
            sw.launch()
            a, b = plain.result(), sw.result()
            assert (a.tops, a.valid, a.digest) == (b.tops, b.valid, b.digest), (planet.R, kernel)
            assert sw.admitted() == sw.total == plain.admitted()
            sw.launch(10, 1000)
            assert sw.admitted() == 990
            if planet is p and kernel is None:
                assert sw.kernel_path() == "fast" and b.tops == [lst[:K] for lst in lists]
                assert (b.valid, b.digest) == (valid, digest)
            if planet is syn and kernel is None:
                assert sw.kernel_path() == "group"
    # with a constraint, auto leaves the group kernel for the fast one
    srv = np.arange(32, dtype=np.uint32)
    sw = Sweep(sdp, srv, srv, 4, OBJS, K=K, ranking=DEFAULT_RANKING, digest=True, constraints=[(MEAN, AF1, U64)])
    assert sw.kernel_path() == "fast"


# --------------------------------------------------------------------- 8 ---
def test_cli_where_prints_the_admitted_count(gcp):
    """sweep --where on GCP n = 5 with "mean e <= v", v the decimal of the mean_e case's bound: the
    admitted count beside the valid count, and the lists of the admitted configs."""
    import io
    import json

    from fantoch_amd import cli

    p, _, _ = gcp
    lists, valid, digest = full_order(gcp, 5)
    total = math.comb(p.R, 5)
    (kind, slot, bound), = X.case_constraints(lists, OBJS, total, "mean_e")
    v = f"{bound * 5 // 100}.{bound * 5 % 100:02d}"  # bound / 20 clients, exactly
    adm = X.admitted_ranks(lists, OBJS, [(kind, slot, bound)])
    want = X.filtered(lists, adm, K)
    assert len(adm) == 5174 and want[0][:10] != lists[0][:10]  # the bound bites in what is printed
    buf = io.StringIO()
    assert cli.main(["sweep", "--objectives", "score,mean:af1", "--n", "5", "--where", f"mean:e<={v}"], out=buf) == 0
    doc = json.loads(buf.getvalue())
    assert (doc["valid"], doc["admitted"], doc["configs"]) == (valid, 5174, total)
    assert doc["admitted_of"] == f"admitted 5174 of {total}" and doc["where"] == f"mean:e<={v}"
    score, mean = doc["objectives"]
    assert [(int(x["key"]), x["rank"]) for x in score["top"]] == want[0][:10]
    assert [(int(x["key"]), x["rank"]) for x in mean["top"]] == want[1][:10]


# --------------------------------------------------------------------- 7 ---
def test_refusals_leave_the_planet_usable(gcp):
    """Each refusal's code and text; afterwards the planet's next plain sweep is unchanged."""
    p, dp, _ = gcp
    lists, valid, digest = full_order(gcp, 3)
    srv = np.arange(p.R, dtype=np.uint32)
    seven = [(MEAN, s) for s in (0, 1, 4, 5, 6, 9)] + [(COV, 0)]

    def make(n, objs, cons, kernel=None, keys=_lib.KEYS_BASE, ranking=None):
        return Sweep(dp, srv, srv, n, objs, K=K, ranking=ranking, kernel=kernel, keys=keys, constraints=cons)

    cases = [
        (dict(n=5, objs=[(MEAN, AF1)], cons=[(MEAN, FF1, 5)], kernel="group"), -1,
         "the group kernel does not apply constraints (fast or generic kernel)"),
        (dict(n=5, objs=[(MEAN, AF1)], cons=[(MEAN, FF1, 5)], keys=_lib.KEYS_TEMPO_ALL_LEADERS), -1,
         "constrained sweeps compute the base key set"),
        (dict(n=5, objs=[(MEAN, AF1)], cons=[(SCORE, 0, 5)]), -1, "SCORE is not a constraint kind"),
        (dict(n=3, objs=[(MEAN, AF1)], cons=[(MEAN, AF2, 5)]), -1,
         "constraint slot does not exist for this n (max_f < 2)"),
        (dict(n=5, objs=seven, cons=[(MEAN, FF1, 5), (COV, FF1, 5)]), -4, "more than 8 objectives and constraints"),
        (dict(n=5, objs=[(MAX, AF1)], cons=[(MDTM, AF1, 5)], kernel="fast"), -1,
         "the fast kernel's MDTM variant carries no maxima or lists: a sweep with MDTM and MAX or percentile "
         "objectives runs the generic kernel, which computes both"),
        (dict(n=5, objs=[(MEAN, AF1)], cons=[(P(7000), AF1, 5)], kernel="fast"), -1,
         "the fast kernel's percentile lists are 4 deep: an objective needs 7 of its slot's largest values "
         "(generic kernel)"),
        (dict(n=5, objs=[(MEAN, AF1)], cons=[(17, AF1, 5)]), -1, "unknown constraint kind"),
        (dict(n=5, objs=[(MEAN, AF1)], cons=[(MEAN, 10, 5)]), -1, "constraint slot out of range"),
        (dict(n=5, objs=[(MEAN, AF1)], cons=[(P(5000), AF1, 5)]), -4,
         "percentile constraint needs more than 8 of the slot's largest values"),
    ]
    for kw, code, text in cases:
        with pytest.raises(BoteError) as ei:
            make(**kw)
        assert ei.value.code == code and str(ei.value).endswith(": " + text), (kw, str(ei.value))
        sw = Sweep(dp, srv, srv, 3, OBJS, K=K, ranking=DEFAULT_RANKING, digest=True)
        sw.launch()
        r = sw.result()
        assert (r.tops, r.valid, r.digest) == ([lst[:K] for lst in lists], valid, digest), kw
