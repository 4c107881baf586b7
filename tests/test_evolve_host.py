"""Streaming evolving search on the host, CPU only: the limit of
Search::min_mean_decrease (bote_mean_decrease_limit) against the plain f64
predicate, the same natively under ASan + UBSan with the new refusals
(tests/native/host_check_evolve.cpp, a stand-alone program linked against
bote_host.cpp), the key <-> score round trip, the selection step (beam_select),
the CLI's flags and the declarations."""
import os
import shutil
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NATIVE = os.path.join(ROOT, "tests", "native")
CSRC = os.path.join(ROOT, "fantoch_amd", "csrc")

NEW_ENTRIES = ("bote_batch_create_bounded", "bote_batch_limits", "bote_mean_decrease_limit")
COUNTS = (2, 13, 20, 64, 127, 4096)
DECREASES = (0.0, 15.0, 5.0, 0.1, -3.0, 1e9)
END = 1 << 27
WINDOW = 200


def passes(prev_s1, s1, count, dec):
    """Histogram::mean_improv(prev, this) >= min_mean_decrease in plain f64."""
    return np.float64(prev_s1) / np.float64(count) - np.float64(s1) / np.float64(count) >= np.float64(dec)


def prevs_of(count):
    top = count * 2 * 16383
    return [0, 1, count, 15 * count - 1, 15 * count, 15 * count + 1, 257 * count + 3, top // 3, top, END - 1]


@pytest.mark.parametrize("count", COUNTS)
def test_limit_equals_the_plain_predicate(count):
    from fantoch_amd import _lib

    for dec in DECREASES:
        for prev in prevs_of(count):
            lim = _lib.mean_decrease_limit(prev, count, dec)
            assert 0 <= lim <= END
            s = np.arange(max(lim - WINDOW, 0), min(lim + WINDOW, END), dtype=np.uint64)
            s = np.concatenate([s, np.array([0, END - 1], dtype=np.uint64)])
            want = passes(prev, s.astype(np.float64), count, dec)
            assert np.array_equal(want, s < np.uint64(lim)), (count, dec, prev, lim)


@pytest.mark.parametrize("count", COUNTS)
def test_limit_is_monotone(count):
    from fantoch_amd import _lib

    walk = list(range(0, END, END // 61 + 1)) + [END - 1]
    for dec in DECREASES:
        lims = [_lib.mean_decrease_limit(prev, count, dec) for prev in walk]
        assert lims == sorted(lims), (count, dec)  # non-decreasing in prev_s1
    for prev in (300 * count, count * 2 * 16383, END - 1):
        lims = [_lib.mean_decrease_limit(prev, count, dec) for dec in sorted(DECREASES)]
        assert lims == sorted(lims, reverse=True), (count, prev)  # non-increasing in min_mean_decrease


def test_limit_ends_and_refusals():
    from fantoch_amd import _lib

    assert _lib.mean_decrease_limit(0, 20, 15.0) == 0  # nothing passes
    assert _lib.mean_decrease_limit(5000, 20, 1e9) == 0
    assert _lib.mean_decrease_limit(0, 20, -1e9) == END  # everything does
    assert _lib.mean_decrease_limit(6000, 20, 0.0) == 6001 and _lib.mean_decrease_limit(6000, 20, 15.0) == 5701
    assert _lib.mean_decrease_limit(5000, 20, float("nan")) == 0
    with pytest.raises(_lib.BoteError, match="a mean needs count >= 1") as e:
        _lib.mean_decrease_limit(5, 0, 0.0)
    assert e.value.code == -1
    with pytest.raises(_lib.BoteError, match=r"previous sum must be below 2\^27") as e:
        _lib.mean_decrease_limit(END, 20, 0.0)
    assert e.value.code != -1
    assert _lib.lib().bote_mean_decrease_limit(5, 20, 0.0, None) == -1
    assert _lib.lib().bote_last_error() == b"out_limit is null"


@pytest.mark.skipif(shutil.which("g++") is None, reason="no host compiler")
def test_limit_and_refusals_natively_under_asan_ubsan():
    out = os.path.join(NATIVE, "build", "host_check_evolve")
    os.makedirs(os.path.dirname(out), exist_ok=True)
    # (the flags of tests/native/Makefile's host_check, and no contraction, as the library's host code is built)
    subprocess.run([os.environ.get("CXX", "g++"), "-O1", "-g", "-std=c++17", "-Wall", "-Wextra", "-ffp-contract=off",
                    "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-o", out,
                    os.path.join(NATIVE, "host_check_evolve.cpp"), os.path.join(CSRC, "bote_host.cpp")], check=True)
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=1", UBSAN_OPTIONS="halt_on_error=1")
    r = subprocess.run([out], capture_output=True, text=True, env=env, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "evolve host ok" in r.stdout, r.stdout
    assert "runtime error" not in r.stderr and "AddressSanitizer" not in r.stderr, r.stderr


# ------------------------------------------------------- keys and selection --
def bits(x):
    return np.asarray(x, dtype=np.float64).view(np.uint64)


def test_key_score_round_trip_is_bit_exact():
    from fantoch_amd.evolve import key_score, score_key

    near = np.float64(10360.307692307693)
    vals = np.array([0.0, -0.0, 1.0, -1.0, -110.5, 5e-324, -5e-324, 1e300, -1e300, np.inf, -np.inf,
                     near, np.nextafter(near, np.inf), np.nextafter(near, -np.inf), 10360.3, 10360.0], dtype=np.float64)
    keys = score_key(vals)
    assert keys.dtype == np.uint64 and np.array_equal(bits(key_score(keys)), bits(vals))
    # the key's order: ascending keys are descending scores, -0.0 just below 0.0
    order = np.argsort(keys, kind="stable")
    assert np.all(np.diff(vals[order]) <= 0)
    assert score_key(-0.0)[0] == score_key(0.0)[0] + 1
    assert score_key(near)[0] + 1 == score_key(np.nextafter(near, -np.inf))[0]
    # the device's formula, ~orderable: sign set -> the bits, else -> their complement without the sign
    assert score_key(1.0)[0] == np.uint64(~(0x3FF0000000000000 | 1 << 63) & (2 ** 64 - 1))
    assert score_key(-1.0)[0] == np.uint64(0xBFF0000000000000)
    # a NaN score has one key (no valid config scores NaN; the all-ones padding key is not a score's)
    assert score_key(np.nan)[0] == score_key(-np.nan)[0]
    # and back from raw keys
    raw = np.array([0, 1, 2 ** 63, 2 ** 63 - 1, 0x4000000000000000, 0xBFF0000000000000], dtype=np.uint64)
    back = key_score(raw)
    ok = ~np.isnan(back)
    assert np.array_equal(score_key(back[ok]), raw[ok])


def test_beam_select_orders_by_score_then_ranks():
    from fantoch_amd.evolve import beam_select

    scores = np.array([5.0, 7.5, 5.0, -1.0, 7.5, 5.0, 0.0, -0.0])
    ranks = np.array([[9, 1], [3, 8], [2, 7], [0, 0], [3, 2], [9, 0], [4, 4], [1, 1]], dtype=np.uint64)
    keep, cut = beam_select(scores, ranks, None)
    assert not cut
    # 7.5: (3,2) < (3,8); 5.0: (2,7) < (9,0) < (9,1); the zeros by ranks, whatever their sign; -1.0 last
    assert keep.tolist() == [4, 1, 2, 5, 0, 7, 6, 3]
    for beam in (8, 9, 1000):  # a beam at least as wide as the input keeps everything
        k2, c2 = beam_select(scores, ranks, beam)
        assert k2.tolist() == keep.tolist() and not c2
    k3, c3 = beam_select(scores, ranks, 3)
    assert k3.tolist() == [4, 1, 2] and c3
    k7, c7 = beam_select(scores, ranks, 7)
    assert k7.tolist() == keep.tolist()[:7] and c7
    # one level, large ranks (above 2^53: compared as integers), an empty input
    big = np.array([[2 ** 63 + 1], [2 ** 63], [5]], dtype=np.uint64)
    assert beam_select(np.array([1.0, 1.0, 1.0]), big, None)[0].tolist() == [2, 1, 0]
    k0, c0 = beam_select(np.zeros(0), np.zeros((0, 2), np.uint64), 4)
    assert len(k0) == 0 and not c0
    # scores one ulp apart are distinct
    a = np.float64(10360.307692307693)
    assert beam_select(np.array([np.nextafter(a, -np.inf), a]), np.array([[0], [1]], np.uint64), 1)[0].tolist() == [1]
    with pytest.raises(ValueError):
        beam_select(scores, ranks, -1)


def test_evolve_refuses_bad_levels():
    from fantoch_amd.bote import FTMetric, RankingParams
    from fantoch_amd.evolve import Evolve

    srv = list(range(20))
    for lo, hi in ((3, 12), (1, 13), (3, 17), (5, 3)):
        with pytest.raises(ValueError, match="evolving levels"):
            Evolve(None, srv, srv, RankingParams.new(110, 35, 0, 15, lo, hi, FTMetric.F1F2))
    with pytest.raises(ValueError, match="beam"):
        Evolve(None, srv, srv, RankingParams.new(110, 35, 0, 15, 3, 13, FTMetric.F1F2), beam=0)
    with pytest.raises(ValueError, match="larger than the server list"):
        Evolve(None, srv[:9], srv, RankingParams.new(110, 35, 0, 15, 3, 13, FTMetric.F1F2))
    e = Evolve(None, srv, srv, RankingParams.new(110, 35, 0, 15, 4, 16, FTMetric.F1))
    assert e.ns == [4, 6, 8, 10, 12, 14, 16]


def test_cli_parses_evolve_flags():
    from fantoch_amd import cli

    a = cli.build_parser().parse_args(["evolve", "--input", "R13C13"])
    assert (a.cmd, a.min_n, a.max_n, a.beam, a.K, a.ranking, a.ft, a.chains) == \
        ("evolve", 3, 13, None, 100, "110,35,0,15", "F1F2", 1)
    a = cli.build_parser().parse_args(["evolve", "--synthetic", "64", "--min-n", "3", "--max-n", "13", "--beam", "256",
                                       "-K", "32", "--ranking", "10,5,0,5", "--ft", "F1", "--chains", "3"])
    assert (a.synthetic, a.beam, a.K, a.ranking, a.ft, a.chains) == (64, 256, 32, "10,5,0,5", "F1", 3)


# ------------------------------------------------------------- declarations --
def test_header_and_library_declare_the_new_entries():
    from fantoch_amd import _lib

    with open(_lib.INCLUDE_H) as fh:
        text = fh.read()
    L = _lib.lib()
    for name in NEW_ENTRIES:
        assert f" {name}(" in text and name in _lib.EXPORTS and hasattr(L, name)


def test_the_rust_and_integration_mirrors_declare_them():
    for rel in (os.path.join("integration", "rust"), "INTEGRATION.md"):
        path = os.path.join(ROOT, rel)
        if os.path.isdir(path):
            text = "".join(open(os.path.join(d, f)).read() for d, _, fs in os.walk(path) for f in fs
                           if f.endswith((".rs", ".md")))
        else:
            text = open(path).read()
        for name in NEW_ENTRIES:
            assert name in text, (rel, name)
