"""The percentile objective (BOTE_OBJ_PCTL) in the host code, CPU only: the
index arithmetic of Histogram::percentile (bote_percentile_index) and the
order-statistic form of the key against the oracle's Histogram, the argument
checks of bote_sweep_create_keys under ASan + UBSan (tests/native/
host_check_pctl.cpp, a stand-alone program linked against bote_host.cpp), the
Python key helpers and the CLI's objective parser."""
import os
import shutil
import subprocess

import numpy as np
import pytest

import oracle as O
from fantoch_amd import _lib, cli
from fantoch_amd.bote import pctl_key, pctl_kind

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NATIVE = os.path.join(ROOT, "tests", "native")
CSRC = os.path.join(ROOT, "fantoch_amd", "csrc")

FIXED_BP = [1, 5000, 7500, 8000, 8500, 9000, 9300, 9500, 9900, 9990, 9999]


def twice_percentile(s, bp):
    """2 * percentile of the ascending values s by the order-statistic form."""
    idx, whole = _lib.percentile_index(bp, len(s))
    if idx == 0:
        return 2 * int(s[0])
    if whole:
        return int(s[idx - 1]) + int(s[idx])
    return 2 * int(s[idx - 1])


def test_percentile_index_and_order_statistic_match_the_oracle():
    """Every count 1..4096, the fixed percentiles and 20 seeded random ones,
    random values with heavy ties: twice the oracle's Histogram::percentile is
    the order statistic that percentile_index selects (half-way cases such as
    p50 of an odd count and idx = 0 included)."""
    rng = np.random.default_rng(20261019)
    bps = FIXED_BP + [int(b) for b in rng.integers(1, 10000, size=20)]
    for count in range(1, 4097):
        # heavy ties: few distinct values, fewer still for some counts
        s = np.sort(rng.integers(1, 3 + count % 7, size=count).astype(np.uint64) * np.uint64(10 + count % 13))
        shuffled = rng.permutation(s)
        for bp in bps:
            idx, whole = _lib.percentile_index(bp, count)
            x = (bp / 10000.0) * count
            assert 0 <= idx <= count and (not whole or 1 <= idx < count), (bp, count, idx, whole)
            assert abs(x - idx) <= 0.5 and whole == (x == idx), (bp, count, idx, whole)
            want = O.hist_percentile(shuffled, bp / 10000.0)
            assert twice_percentile(s, bp) == 2 * want, (bp, count, idx, whole, want)


def test_percentile_index_known_rows_and_errors():
    rows = [(9500, 20, 19, True), (8500, 20, 17, True), (8000, 20, 16, True), (6500, 20, 13, True),
            (9900, 20, 20, False), (9500, 64, 61, False), (9900, 64, 63, False), (9500, 128, 122, False),
            (5000, 5, 3, False), (7500, 9, 7, False), (5000, 1, 1, False), (1, 4096, 0, False)]
    for bp, c, idx, whole in rows:
        assert _lib.percentile_index(bp, c) == (idx, whole), (bp, c)
    for bp, c in [(0, 20), (10000, 20), (9500, 0)]:
        with pytest.raises(_lib.BoteError) as e:
            _lib.percentile_index(bp, c)
        assert e.value.code == -1


@pytest.mark.skipif(shutil.which("g++") is None, reason="no host compiler")
def test_percentile_objective_checks_under_asan_ubsan():
    out = os.path.join(NATIVE, "build", "host_check_pctl")
    os.makedirs(os.path.dirname(out), exist_ok=True)
    # (the flags of tests/native/Makefile's host_check)
    subprocess.run([os.environ.get("CXX", "g++"), "-O1", "-g", "-std=c++17", "-Wall", "-Wextra",
                    "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-o", out,
                    os.path.join(NATIVE, "host_check_pctl.cpp"), os.path.join(CSRC, "bote_host.cpp")], check=True)
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=1", UBSAN_OPTIONS="halt_on_error=1")
    r = subprocess.run([out], capture_output=True, text=True, env=env, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "pctl host ok" in r.stdout, r.stdout
    assert "runtime error" not in r.stderr and "AddressSanitizer" not in r.stderr, r.stderr


def test_pctl_key_helpers_and_cli_objectives():
    assert _lib.OBJ_PCTL(9500) == 0x10000 | 9500 and _lib.OBJ_PCTL(1) == 0x10001 and _lib.OBJ_PCTL(9999) == 0x10000 | 9999
    with open(_lib.INCLUDE_H) as fh:
        assert "#define BOTE_OBJ_PCTL(bp) (0x10000u | (bp))" in fh.read()
    for bad in (0, 10000, -1, 0x10000):
        with pytest.raises(ValueError):
            _lib.OBJ_PCTL(bad)
    assert _lib.is_pctl(_lib.OBJ_PCTL(9500)) and not _lib.is_pctl(_lib.OBJ_MAX) and not _lib.is_pctl(0x10000)
    assert not _lib.is_pctl(0x10000 | 10000) and not _lib.is_pctl(0x20000 | 9500)
    assert pctl_key((475 << 32) | 3456) == (475, 3456)
    assert pctl_key(0) == (0, 0)
    # the largest key: twice = 4 * 16383, sum = 4096 * 2 * 16383 < 2^27
    assert pctl_key((65532 << 32) | (4096 * 32766)) == (65532, 4096 * 32766)
    assert pctl_kind(0.95) == _lib.OBJ_PCTL(9500) and pctl_kind(0.999) == _lib.OBJ_PCTL(9990)
    assert pctl_kind(0.0001) == _lib.OBJ_PCTL(1) and pctl_kind(0.9999) == _lib.OBJ_PCTL(9999) and pctl_kind(0.5) == _lib.OBJ_PCTL(5000)
    for bad in (0.0, 1.0, 0.95001, 1.5):
        with pytest.raises(ValueError):
            pctl_kind(bad)
    assert cli._objectives("mean:af1,p95:af1,p99:ff1,p99.9:e,p50:af1C,score") == [
        (_lib.OBJ_MEAN, 0), (_lib.OBJ_PCTL(9500), 0), (_lib.OBJ_PCTL(9900), 1), (_lib.OBJ_PCTL(9990), 4),
        (_lib.OBJ_PCTL(5000), 5), (_lib.OBJ_SCORE, 0)]
    assert cli._objectives("p50:ff1C,p99.99:fl1,p0.01:e,p5:af1,p7.5:af1") == [
        (_lib.OBJ_PCTL(5000), 6), (_lib.OBJ_PCTL(9999), _lib.SLOT_FL1), (_lib.OBJ_PCTL(1), 4), (_lib.OBJ_PCTL(500), 0),
        (_lib.OBJ_PCTL(750), 0)]
    for bad in ("p0:af1", "p100:af1", "p95.123:af1", "p0.00:af1", "p:af1", "p95.:af1", "P95:af1"):
        with pytest.raises((ValueError, KeyError)):
            cli._objectives(bad)
    for bp, name in [(9500, "p95"), (9990, "p99.9"), (9999, "p99.99"), (5000, "p50"), (1, "p0.01"), (750, "p7.5"), (9905, "p99.05")]:
        assert cli._objective_name(_lib.OBJ_PCTL(bp)) == name
        assert cli._pctl_kind(name) == _lib.OBJ_PCTL(bp)
