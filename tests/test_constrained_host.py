"""Constrained sweeps on the host, CPU only: the argument checks and the routing
over the union of kinds natively under ASan + UBSan
(tests/native/host_check_constrained.cpp, a stand-alone program linked against
bote_host.cpp), the refusals the library gives before it touches a device, and
the declarations with their mirrors."""
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

ENTRIES = ("bote_sweep_create_constrained", "bote_sweep_admitted")


@pytest.mark.skipif(shutil.which("g++") is None, reason="no host compiler")
def test_checks_and_routing_natively_under_asan_ubsan():
    out = os.path.join(NATIVE, "build", "host_check_constrained")
    os.makedirs(os.path.dirname(out), exist_ok=True)
    # (the flags of the sibling host_check programs, and no contraction, as the library's host code is built)
    subprocess.run([os.environ.get("CXX", "g++"), "-O1", "-g", "-std=c++17", "-Wall", "-Wextra", "-ffp-contract=off",
                    "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-o", out,
                    os.path.join(NATIVE, "host_check_constrained.cpp"), os.path.join(CSRC, "bote_host.cpp")],
                   check=True)
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=1", UBSAN_OPTIONS="halt_on_error=1")
    r = subprocess.run([out], capture_output=True, text=True, env=env, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "constrained host ok" in r.stdout, r.stdout
    assert "runtime error" not in r.stderr and "AddressSanitizer" not in r.stderr, r.stderr


def test_library_refuses_before_it_touches_a_device():
    from fantoch_amd import _lib

    L = _lib.lib()
    srv = np.arange(20, dtype=np.uint32)
    objs = (_lib.Objective * 1)(_lib.Objective(_lib.OBJ_MEAN, 0))
    cons = (_lib.Constraint * 1)(_lib.Constraint(_lib.OBJ_MEAN, 1, 1000))
    h = C.c_void_p()

    def create(objs, n_obj, cons, n_con, kernel="auto", out=C.byref(h)):
        return L.bote_sweep_create_constrained(None, srv, 20, srv, 20, 5, objs, n_obj, cons, n_con, 100, None,
                                               0, _lib.KERNELS[kernel], out)

    assert create(objs, 1, cons, 1, out=None) == -1
    assert L.bote_last_error() == b"out is null"
    assert create(objs, 1, cons, 1) == -1  # the sweep's own checks come first
    assert L.bote_last_error() == b"planet is null"
    assert not h
    v = C.c_uint64(7)
    assert L.bote_sweep_admitted(None, None, C.byref(v)) == -1
    assert L.bote_last_error() == b"null argument"


def test_header_library_and_bindings_declare_the_entries():
    from fantoch_amd import _lib

    with open(_lib.INCLUDE_H) as fh:
        text = fh.read()
    L = _lib.lib()
    for name in ENTRIES:
        assert re.search(r"\b%s\(" % name, text), name
        assert name in _lib.EXPORTS and hasattr(L, name), name
    assert re.search(r"typedef struct \{\s*uint32_t kind;[^}]*uint32_t slot;[^}]*uint64_t max_key;\s*\} bote_constraint;",
                     text)
    assert C.sizeof(_lib.Constraint) == 16 and _lib.Constraint.max_key.offset == 8
    with open(os.path.join(ROOT, "integration", "rust", "src", "hip.rs")) as fh:
        rust = fh.read()
    for name in ENTRIES:
        assert re.search(r"\bfn %s\(" % name, rust), name
    assert "pub struct bote_constraint" in rust
    with open(os.path.join(ROOT, "INTEGRATION.md")) as fh:
        doc = fh.read()
    for name in ENTRIES:
        assert name in doc, name
