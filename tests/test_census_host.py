"""Census sweeps on the host, CPU only: the launch and creation checks and the
routing natively under ASan + UBSan (tests/native/host_check_census.cpp, a
stand-alone program linked against bote_host.cpp), the refusals the library
gives before it touches a device, the declarations and their mirrors, and the
CLI's flags."""
import ctypes as C
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NATIVE = os.path.join(ROOT, "tests", "native")
CSRC = os.path.join(ROOT, "fantoch_amd", "csrc")

ENTRIES = ("bote_census_create", "bote_census_launch", "bote_census_result", "bote_census_deferred",
           "bote_census_path", "bote_census_last_kernel_ms", "bote_census_destroy")


@pytest.mark.skipif(shutil.which("g++") is None, reason="no host compiler")
def test_checks_and_routing_natively_under_asan_ubsan():
    out = os.path.join(NATIVE, "build", "host_check_census")
    os.makedirs(os.path.dirname(out), exist_ok=True)
    # (the flags of tests/native/Makefile's host_check, and no contraction, as the library's host code is built)
    subprocess.run([os.environ.get("CXX", "g++"), "-O1", "-g", "-std=c++17", "-Wall", "-Wextra", "-ffp-contract=off",
                    "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-o", out,
                    os.path.join(NATIVE, "host_check_census.cpp"), os.path.join(CSRC, "bote_host.cpp")], check=True)
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=1", UBSAN_OPTIONS="halt_on_error=1")
    r = subprocess.run([out], capture_output=True, text=True, env=env, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "census host ok" in r.stdout, r.stdout
    assert "runtime error" not in r.stderr and "AddressSanitizer" not in r.stderr, r.stderr


def test_library_refuses_before_it_touches_a_device():
    from fantoch_amd import _lib

    L = _lib.lib()
    srv = np.arange(20, dtype=np.uint32)
    objs = (_lib.Objective * 2)(_lib.Objective(_lib.OBJ_MEAN, 0), _lib.Objective(_lib.OBJ_MAX, 0))
    h = C.c_void_p()
    assert L.bote_census_create(None, srv, 20, srv, 20, 5, objs, 2, None, _lib.KERNELS["group"], C.byref(h)) == -1
    assert L.bote_last_error() == b"the group kernel does not run census sweeps (fast or generic kernel)"
    assert L.bote_census_create(None, srv, 20, srv, 20, 5, objs, 2, None, _lib.KERNELS["fast"], C.byref(h)) == -1
    assert L.bote_last_error() == b"planet is null"
    assert L.bote_census_create(None, srv, 20, srv, 20, 5, objs, 2, None, 0, None) == -1
    assert L.bote_last_error() == b"out is null"
    assert not h
    thr = np.zeros((2, 1, 2), np.uint64)
    assert L.bote_census_launch(None, _lib.ptr(thr), 1, 0, 1, None) == -1
    assert L.bote_last_error() == b"census is null"
    below = np.zeros(2, np.uint64)
    assert L.bote_census_result(None, None, _lib.ptr(below), None) == -1
    v = C.c_uint64()
    assert L.bote_census_deferred(None, None, C.byref(v)) == -1
    assert L.bote_census_path(None, None) == -1
    assert L.bote_census_last_kernel_ms(None, None) == -1
    assert L.bote_census_destroy(None) == 0  # like the other handles: destroying nothing is fine


def test_header_library_and_binding_declare_the_entries():
    from fantoch_amd import _lib

    with open(_lib.INCLUDE_H) as fh:
        text = fh.read()
    L = _lib.lib()
    for name in ENTRIES:
        assert f" {name}(" in text and name in _lib.EXPORTS and hasattr(L, name)
        assert getattr(L, name).argtypes is not None, name
    m = re.search(r"#define BOTE_CENSUS_MAX_THRESHOLDS (\d+)", text)
    assert m and int(m.group(1)) == _lib.CENSUS_MAX_THRESHOLDS == 16
    assert "typedef struct bote_census bote_census;" in text
    # the contract's one-line consequence is stated where a caller reads it
    assert "has below == i" in text


def test_the_rust_and_integration_mirrors_declare_them():
    from fantoch_amd import _lib

    with open(_lib.INCLUDE_H) as fh:
        header = fh.read()
    for rel in (os.path.join("integration", "rust", "src", "hip.rs"), "INTEGRATION.md"):
        with open(os.path.join(ROOT, rel)) as fh:
            text = fh.read()
        assert "pub struct bote_census" in text, rel
        for name in ENTRIES:
            decl = re.search(r"pub fn %s\((.*?)\)\s*->\s*c_int;" % name, text, re.S)
            assert decl, (rel, name)
            # as many parameters as the header's declaration
            hdr = re.search(r"int %s\((.*?)\);" % name, header, re.S)
            assert len(decl.group(1).split(",")) == len(hdr.group(1).split(",")), (rel, name)
    with open(os.path.join(ROOT, "integration", "rust", "src", "hip.rs")) as fh:
        assert "pub const BOTE_CENSUS_MAX_THRESHOLDS: u32 = 16;" in fh.read()
    with open(os.path.join(ROOT, "INTEGRATION.md")) as fh:
        assert "BOTE_CENSUS_MAX_THRESHOLDS" in fh.read()


def test_census_refuses_bad_thresholds_on_the_host():
    """Census.launch shapes its thresholds before the library sees them."""
    from fantoch_amd.bote import Census

    c = Census.__new__(Census)  # (no device: the shape checks come first)
    c.objectives, c.h, c.total = [(1, 0), (1, 1)], None, 10
    with pytest.raises(ValueError, match="one row of thresholds per objective"):
        c.launch([[(0, 0)]])
    with pytest.raises(ValueError, match="one row of thresholds per objective"):
        c.launch([[(0, 0)], [(0, 0), (1, 1)]])
    with pytest.raises(ValueError, match=r"outside \(0, 1\]"):
        c.quantiles([0.5, 0.0])
    with pytest.raises(ValueError, match=r"outside \(0, 1\]"):
        c.quantiles([1.5])
    c.n, c.servers = 3, np.arange(10, dtype=np.uint32)
    for bad in ([1, 2], [1, 1, 2], [1, 2, 10]):
        with pytest.raises(ValueError, match="3 distinct positions"):
            c.position_of(bad)


def test_cli_parses_census_flags():
    from fantoch_amd import cli

    a = cli.build_parser().parse_args(["census", "--n", "5", "--config", "a,b,c,d,e"])
    assert (a.cmd, a.n, a.objectives, a.ranking, a.ft, a.kernel, a.config, a.quantiles, a.synthetic) == \
        ("census", 5, "default", "110,35,0,15", "F1F2", "auto", "a,b,c,d,e", None, None)
    a = cli.build_parser().parse_args(["census", "--synthetic", "64", "--seed", "3", "--n", "7", "--objectives",
                                       "mean:af1,max:af1,p95:af1,mdtm:af1", "--ranking", "10,5,0,5", "--ft", "F1",
                                       "--kernel", "generic", "--quantiles", "0.01,0.5,0.99"])
    assert (a.synthetic, a.seed, a.n, a.ranking, a.ft, a.kernel, a.quantiles) == \
        (64, 3, 7, "10,5,0,5", "F1", "generic", "0.01,0.5,0.99")
    assert cli._objectives(a.objectives) == [(1, 0), (16, 0), (0x10000 | 9500, 0), (18, 0)]
    with pytest.raises(SystemExit):
        cli.build_parser().parse_args(["census", "--config", "a,b,c"])  # --n is required
    with pytest.raises(SystemExit):
        cli.build_parser().parse_args(["census", "--n", "5", "--kernel", "group"])
    with pytest.raises(ValueError, match="--config and/or --quantiles"):
        cli.census(cli.build_parser().parse_args(["census", "--n", "5"]))


def test_cli_decodes_quantile_keys():
    from fantoch_amd import _lib, cli
    from fantoch_amd.evolve import score_key

    assert cli._decode_key(_lib.OBJ_MEAN, 0, 1300, 5, 20) == {"key": "1300", "sum": 1300, "mean": 65.0}
    assert cli._decode_key(_lib.OBJ_MEAN, 5, 1300, 5, 20)["mean"] == 260.0  # a colocated slot holds n values
    assert cli._decode_key(_lib.OBJ_MAX, 0, (250 << 32) | 1300, 5, 20) == {"key": str((250 << 32) | 1300), "max": 250,
                                                                           "sum": 1300}
    d = cli._decode_key(_lib.OBJ_PCTL(9500), 0, (401 << 32) | 1300, 5, 20)
    assert (d["percentile"], d["sum"]) == (200.5, 1300)
    d = cli._decode_key(_lib.OBJ_MDTM, 0, (800 << 27) | 1300, 5, 20)
    assert (d["mdtm"], d["sum"]) == (4.0, 1300)
    assert cli._decode_key(_lib.OBJ_SCORE, 0, int(score_key(10360.5)[0]), 5, 20)["score"] == 10360.5
    ratio = np.array([0.19], np.float64).view(np.uint64)[0]
    assert cli._decode_key(_lib.OBJ_COV, 0, int(ratio), 5, 20)["cov"] == (0.19 * 20 / 19) ** 0.5
    assert cli._decode_key(_lib.OBJ_COV, 0, (1 << 64) - 1, 5, 20)["cov"] is None
