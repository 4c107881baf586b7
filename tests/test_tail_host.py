"""The MAX (worst-client) objective in the host code, CPU only: the argument
checks of bote_sweep_create_keys under ASan + UBSan (tests/native/
host_check_tail.cpp, a stand-alone program linked against bote_host.cpp), the
Python key helper and the CLI's objective parser."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NATIVE = os.path.join(ROOT, "tests", "native")
CSRC = os.path.join(ROOT, "fantoch_amd", "csrc")


@pytest.mark.skipif(shutil.which("g++") is None, reason="no host compiler")
def test_max_objective_checks_under_asan_ubsan():
    out = os.path.join(NATIVE, "build", "host_check_tail")
    os.makedirs(os.path.dirname(out), exist_ok=True)
    # (the flags of tests/native/Makefile's host_check)
    subprocess.run([os.environ.get("CXX", "g++"), "-O1", "-g", "-std=c++17", "-Wall", "-Wextra",
                    "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-o", out,
                    os.path.join(NATIVE, "host_check_tail.cpp"), os.path.join(CSRC, "bote_host.cpp")], check=True)
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=1", UBSAN_OPTIONS="halt_on_error=1")
    r = subprocess.run([out], capture_output=True, text=True, env=env, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "tail host ok" in r.stdout, r.stdout
    assert "runtime error" not in r.stderr and "AddressSanitizer" not in r.stderr, r.stderr


def test_max_key_helper_and_cli_objectives():
    from fantoch_amd import _lib, cli
    from fantoch_amd.bote import max_key

    assert _lib.OBJ_MAX == 16
    with open(_lib.INCLUDE_H) as fh:
        assert "#define BOTE_OBJ_MAX 16" in fh.read()
    assert max_key((237 << 32) | 3456) == (237, 3456)
    assert max_key(0) == (0, 0)
    # the largest key: max = 2 * 16383, sum = 4096 * 2 * 16383 < 2^27
    assert max_key((32766 << 32) | (4096 * 32766)) == (32766, 4096 * 32766)
    assert cli._objectives("mean:af1,max:af1,max:ff1C,score") == [
        (_lib.OBJ_MEAN, 0), (_lib.OBJ_MAX, 0), (_lib.OBJ_MAX, 6), (_lib.OBJ_SCORE, 0)]
    assert cli._objectives("max:fl1") == [(_lib.OBJ_MAX, _lib.SLOT_FL1)]
