"""Constrained sweeps, CPU only: the exact bound helpers (fantoch_amd.bote
mean_bound, max_bound, pctl_bound, mdtm_bound) against brute force, the CLI's
--where parser, and the oracle-side filter that builds the GPU tests'
expectations (tests/constrained_expect.py), which must reproduce the admitted
and admitted-valid counts measured on the CPU oracle for GCP n = 3."""
import itertools
import math
from fractions import Fraction

import numpy as np
import pytest

from fantoch_amd import _lib
from fantoch_amd.bote import max_bound, mdtm_bound, mean_bound, parse_where, pctl_bound

MEAN, COV, MAX, MDTM = _lib.OBJ_MEAN, _lib.OBJ_COV, _lib.OBJ_MAX, _lib.OBJ_MDTM

# bounds v to try: integers, halves, thirds, a value below every statistic and decimal strings
VS = [Fraction(a, b) for a in range(0, 25) for b in (1, 2, 3, 7)] + [Fraction(10 ** 6)]


def test_mean_bound_against_every_sum_and_count():
    """A config passes iff its exact mean S1 / count <= v, for every sum up to 60 and count up to 8."""
    for count in range(1, 9):
        for v in VS:
            b = mean_bound(v, count)
            for s1 in range(0, 61):
                assert (s1 <= b) == (Fraction(s1, count) <= v), (count, v, s1)
    assert mean_bound("140.5", 20) == 2810 and mean_bound("140.54", 20) == 2810 and mean_bound("140.55", 20) == 2811
    assert mean_bound("0.1", 10) == 1 and mean_bound(0.1, 10) == 1  # (the float 0.1 is a little above 1/10)
    assert mean_bound("0.3", 10) == 3 and mean_bound(0.3, 10) == 2  # (the float 0.3 is a little below 3/10)


def test_max_and_percentile_bounds_against_every_key():
    """MAX: key = max << 32 | S1 passes iff max <= m; a percentile's key holds twice the percentile
    (an integer; the percentile may end in .5) and passes iff percentile <= v.  Every sum field."""
    sums = [0, 1, 12345, (1 << 27) - 2, 0xFFFFFFFF]
    for v in VS[:100]:
        bm, bp = max_bound(v), pctl_bound(v)
        for x in range(0, 60):
            for s1 in sums:
                assert ((x << 32 | s1) <= bm) == (x <= v), (v, x, s1)
                assert ((x << 32 | s1) <= bp) == (Fraction(x, 2) <= v), (v, x, s1)  # x = twice the percentile
    assert pctl_bound("300") == 600 << 32 | 0xFFFFFFFF and pctl_bound("12.5") == 25 << 32 | 0xFFFFFFFF


def test_mdtm_bound_against_every_small_histogram():
    """Every multiset of up to 4 values in 0..6: H by its definition, key = H << 27 | S1, and the
    config passes iff its exact mdtm = sum |x - mean| / count = 2 H / count^2 <= v."""
    for count in range(1, 5):
        for xs in itertools.combinations_with_replacement(range(7), count):
            s1 = sum(xs)
            h = sum(max(count * x - s1, 0) for x in xs)
            mdtm = sum(abs(Fraction(x) - Fraction(s1, count)) for x in xs) / count
            assert mdtm == Fraction(2 * h, count * count)
            key = h << 27 | s1
            for v in VS[:60]:
                assert (key <= mdtm_bound(v, count)) == (mdtm <= v), (xs, v)
    assert mdtm_bound("0", 20) == (1 << 27) - 1


def test_negative_bounds_are_refused():
    for f in (mean_bound, mdtm_bound):
        with pytest.raises(ValueError):
            f("-1", 20)
    for f in (max_bound, pctl_bound):
        with pytest.raises(ValueError):
            f(Fraction(-1, 2))


def test_where_parsing_is_exact():
    got = parse_where("mean:ff1<=140.55, p99:af1<=300,cov:ff1C<=key:0x3f90000000000000,mdtm:e<=12.25,max:af1C<=99,"
                      "p99.9:af2<=7.5,mean:eC<=key:17", 20, 5)
    assert got == [(MEAN, 1, 2811), (_lib.OBJ_PCTL(9900), 0, 600 << 32 | 0xFFFFFFFF), (COV, 6, 0x3F90000000000000),
                   (MDTM, 4, (12 * 400 + 100) // 2 << 27 | ((1 << 27) - 1)), (MAX, 5, 99 << 32 | 0xFFFFFFFF),
                   (_lib.OBJ_PCTL(9990), 2, 15 << 32 | 0xFFFFFFFF), (MEAN, 9, 17)]
    # a colocated slot's count is n, an Input slot's the clients
    assert parse_where("mean:af1C<=10.5", 20, 5) == [(MEAN, 5, 52)] and parse_where("mean:af1<=10.5", 20, 5) == [(MEAN, 0, 210)]
    # a long decimal is taken digit by digit: 0.1 + 2^-60 as a float would be 0.1
    assert parse_where("mean:af1<=0.10000000000000000001", 10 ** 20, 3) == [(MEAN, 0, 10 ** 19 + 1)]
    assert parse_where("mean:af1<=0.1", 10 ** 20, 3) == [(MEAN, 0, 10 ** 19)]


@pytest.mark.parametrize("text", [
    "", "mean:ff1", "mean:ff1<140", "mean:ff1>=140", "mean:zz<=1", "mean:FF1<=1", "score:af1<=1", "avg:af1<=1",
    "mean:ff1<=abc", "mean:ff1<=-5", "mean:ff1<=1e3", "mean:ff1<=1,", "cov:af1<=0.5", "cov:af1<=key:zz",
    "mean:af1<=key:-1", "mean:af1<=key:0x10000000000000000", "p0:af1<=5", "p100:af1<=5", "p99.999:af1<=5", "p:af1<=5",
])
def test_where_refuses_bad_input(text):
    with pytest.raises(ValueError):
        parse_where(text, 20, 5)


def test_oracle_filter_reproduces_the_measured_counts_of_gcp_n3():
    """The expectation code of tests/test_gpu_constrained.py on GCP n = 3 (1,140 configs, 47 valid):
    the admitted count and the admitted valid configs of every table row, ties at the bound admitted."""
    import oracle as O
    from fantoch_amd.planet import Planet
    from tests import constrained_expect as X

    p = Planet.new()
    total = math.comb(p.R, 3)
    lists, valid, _ = X.full_order(O.OraclePlanet.of(p), p.R, 3)
    assert (total, valid) == (1140, 47)
    valid_ranks = {r for _, r in lists[0]}
    for case, (_, want) in X.CASES.items():
        cons = X.case_constraints(lists, X.OBJS, total, case)
        adm = X.admitted_ranks(lists, X.OBJS, cons)
        n_adm, n_score = want[3]
        assert len(adm) == n_adm and 0 < len(adm) < total, case
        got = X.filtered(lists, adm, 100)
        assert got != [lst[:100] for lst in lists], case  # the constraint bites
        assert len(got[0]) == len(adm & valid_ranks) and (n_score is None or len(got[0]) == n_score), case
        for lst, g in zip(lists[1:], got[1:]):
            assert len(g) == 100 and g == sorted(g) and {r for _, r in g} <= adm
        # inclusive: the record at the bound's index is admitted, with every record tied with it
        if len(cons) == 1:
            (kind, slot, bound), = cons
            own = lists[X.OBJS.index((kind, slot))]
            assert own[total // 3][0] == bound and all(r in adm for k, r in own if k == bound)
    # no bound at all, and a bound below every key
    every = X.admitted_ranks(lists, X.OBJS, [(MEAN, 1, X.U64)])
    assert len(every) == total and X.filtered(lists, every, 100) == [lst[:100] for lst in lists]
    assert min(k for lst in lists[1:] for k, _ in lst) > 0
    assert X.admitted_ranks(lists, X.OBJS, [(MEAN, 1, 0)]) == set()
    assert np.uint64(X.NAN_KEY) > max(np.uint64(k) for k, _ in lists[3])  # a NaN pattern is above every finite COV key
