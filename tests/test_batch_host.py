"""Batched pinned sweeps (bote_batch_*) in the host code, CPU only: the argument
checks and the unit plan under ASan + UBSan (tests/native/host_check_batch.cpp,
a stand-alone program linked against bote_host.cpp), the CLI's --pinned-sets and
the header."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NATIVE = os.path.join(ROOT, "tests", "native")
CSRC = os.path.join(ROOT, "fantoch_amd", "csrc")

BATCH_ENTRIES = ("bote_batch_create", "bote_batch_launch", "bote_batch_result", "bote_batch_deferred",
                 "bote_batch_path", "bote_batch_last_kernel_ms", "bote_batch_plan", "bote_batch_destroy")


@pytest.mark.skipif(shutil.which("g++") is None, reason="no host compiler")
def test_batch_checks_and_unit_plan_under_asan_ubsan():
    out = os.path.join(NATIVE, "build", "host_check_batch")
    os.makedirs(os.path.dirname(out), exist_ok=True)
    # (the flags of tests/native/Makefile's host_check)
    subprocess.run([os.environ.get("CXX", "g++"), "-O1", "-g", "-std=c++17", "-Wall", "-Wextra",
                    "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-o", out,
                    os.path.join(NATIVE, "host_check_batch.cpp"), os.path.join(CSRC, "bote_host.cpp")], check=True)
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=1", UBSAN_OPTIONS="halt_on_error=1")
    r = subprocess.run([out], capture_output=True, text=True, env=env, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "batch host ok" in r.stdout, r.stdout
    assert "runtime error" not in r.stderr and "AddressSanitizer" not in r.stderr, r.stderr


def test_cli_parses_pinned_sets():
    from fantoch_amd import cli

    names = ["asia-east1", "europe-west1", "us-east1", "us-west1"]
    assert cli._pinned_sets(None, names) is None and cli._pinned_sets("", names) is None
    assert cli._pinned_sets("us-east1,asia-east1;3,0", names) == [[2, 0], [3, 0]]
    assert cli._pinned_sets("1", names) == [[1]]
    assert cli._pinned_sets("1,2;1,2; 2,1", names) == [[1, 2], [1, 2], [2, 1]]  # equal sets are allowed
    for bad in ("1,2;3", "1;;2", "mars-1;1", "1,1;2,3", "4;1"):
        with pytest.raises(ValueError):
            cli._pinned_sets(bad, names)
    args = cli.build_parser().parse_args(["sweep", "--n", "5", "--pinned-sets", "0,19;3,4"])
    assert args.pinned_sets == "0,19;3,4" and args.pinned is None
    assert cli.build_parser().parse_args(["sweep", "--n", "5"]).pinned_sets is None


def test_header_declares_the_batch_entries():
    from fantoch_amd import _lib

    with open(_lib.INCLUDE_H) as fh:
        text = fh.read()
    for name in BATCH_ENTRIES:
        assert f" {name}(" in text and name in _lib.EXPORTS
    assert "#define BOTE_BATCH_MAX_SETS 1024" in text
    L = _lib.lib()
    assert all(hasattr(L, name) for name in BATCH_ENTRIES)


def test_the_rust_and_integration_mirrors_declare_them():
    for rel in (os.path.join("integration", "rust"), "INTEGRATION.md"):
        path = os.path.join(ROOT, rel)
        if os.path.isdir(path):
            text = "".join(open(os.path.join(d, f)).read() for d, _, fs in os.walk(path) for f in fs
                           if f.endswith((".rs", ".md")))
        else:
            text = open(path).read()
        for name in BATCH_ENTRIES:
            assert name in text, (rel, name)
