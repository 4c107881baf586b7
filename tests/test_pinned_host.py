"""Pinned sweeps (bote_sweep_create_pinned) in the host code, CPU only: the
argument checks and pinned_config under ASan + UBSan (tests/native/
host_check_pinned.cpp, a stand-alone program linked against bote_host.cpp),
the Python helpers against itertools, the CLI's --pinned and the header."""
import itertools
import math
import os
import shutil
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NATIVE = os.path.join(ROOT, "tests", "native")
CSRC = os.path.join(ROOT, "fantoch_amd", "csrc")

SHAPES = [(9, 4, 1), (9, 4, 3), (10, 5, 2), (8, 3, 2), (11, 7, 4), (20, 13, 1)]


def pinned_sets(ns, m):
    """lowest, highest (unsorted, with ns - 1) and interleaved positions"""
    return [list(range(m)), [ns - 1 - i for i in range(m)], [(1 + i * (ns - 2) // m) % ns for i in range(m)][::-1]]


def supersets(ns, n, pinned):
    """The n-supersets of `pinned` among ns positions, sorted by full colex rank, and those ranks."""
    free = [x for x in range(ns) if x not in pinned]
    cfgs = [tuple(sorted(set(pinned) | set(c))) for c in itertools.combinations(free, n - len(pinned))]
    rank = lambda c: sum(math.comb(x, j + 1) for j, x in enumerate(c))
    cfgs.sort(key=rank)
    return cfgs, [rank(c) for c in cfgs]


@pytest.mark.skipif(shutil.which("g++") is None, reason="no host compiler")
def test_pinned_checks_and_configs_under_asan_ubsan():
    out = os.path.join(NATIVE, "build", "host_check_pinned")
    os.makedirs(os.path.dirname(out), exist_ok=True)
    # (the flags of tests/native/Makefile's host_check)
    subprocess.run([os.environ.get("CXX", "g++"), "-O1", "-g", "-std=c++17", "-Wall", "-Wextra",
                    "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-o", out,
                    os.path.join(NATIVE, "host_check_pinned.cpp"), os.path.join(CSRC, "bote_host.cpp")], check=True)
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=1", UBSAN_OPTIONS="halt_on_error=1")
    r = subprocess.run([out], capture_output=True, text=True, env=env, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "pinned host ok" in r.stdout, r.stdout
    assert "runtime error" not in r.stderr and "AddressSanitizer" not in r.stderr, r.stderr


@pytest.mark.parametrize("ns,n,m", SHAPES)
def test_pinned_total_and_config_against_itertools(ns, n, m):
    from fantoch_amd import _lib

    assert _lib.pinned_total(ns, n, m) == math.comb(ns - m, n - m)
    for pinned in pinned_sets(ns, m):
        cfgs, ranks = supersets(ns, n, pinned)
        assert len(cfgs) == _lib.pinned_total(ns, n, m)
        # pinned-rank order is full-rank order (the order lemma): pinned rank i is the i-th superset by full rank
        step = max(1, len(cfgs) // 400)
        for pr in list(range(0, len(cfgs), step)) + [len(cfgs) - 1]:
            pos, full = _lib.pinned_config(pr, n, ns, pinned)
            assert tuple(int(x) for x in pos) == cfgs[pr] and full == ranks[pr]
            assert _lib.colex_unrank(full, n, ns).tolist() == list(cfgs[pr])
        with pytest.raises(_lib.BoteError):
            _lib.pinned_config(len(cfgs), n, ns, pinned)


def test_pinned_helpers_refuse_bad_input():
    from fantoch_amd import _lib

    assert _lib.pinned_total(20, 5, 0) == 0 and _lib.pinned_total(20, 5, 5) == 0 and _lib.pinned_total(4, 5, 1) == 0
    assert _lib.pinned_total(64, 7, 2) == 6471002 and _lib.pinned_total(128, 7, 2) == 244222650
    for bad in ([3, 3], [3, 20]):
        with pytest.raises(_lib.BoteError):
            _lib.pinned_config(0, 5, 20, bad)
    with pytest.raises(_lib.BoteError):
        _lib.pinned_config(0, 2, 20, [3, 4])


def test_cli_parses_pinned():
    from fantoch_amd import cli

    names = ["asia-east1", "europe-west1", "us-east1", "us-west1"]
    assert cli._pinned(None, names) is None and cli._pinned("", names) is None
    assert cli._pinned("us-east1,asia-east1", names) == [2, 0]
    assert cli._pinned("3,0", names) == [3, 0]
    assert cli._pinned("us-west1, 1", names) == [3, 1]
    for bad in ("mars-1", "4", "us-east1,2", "1,1"):
        with pytest.raises(ValueError):
            cli._pinned(bad, names)
    args = cli.build_parser().parse_args(["sweep", "--n", "5", "--pinned", "eu-west-1,us-east-1", "--rank-begin", "3"])
    assert args.pinned == "eu-west-1,us-east-1" and args.rank_begin == 3
    assert cli.build_parser().parse_args(["sweep", "--n", "5"]).pinned is None


def test_header_declares_the_pinned_entries():
    from fantoch_amd import _lib

    with open(_lib.INCLUDE_H) as fh:
        text = fh.read()
    for name in ("bote_pinned_total", "bote_pinned_config", "bote_sweep_create_pinned"):
        assert f" {name}(" in text and name in _lib.EXPORTS
    L = _lib.lib()
    assert all(hasattr(L, name) for name in ("bote_pinned_total", "bote_pinned_config", "bote_sweep_create_pinned"))
    assert np.dtype(np.uint64).itemsize == 8
