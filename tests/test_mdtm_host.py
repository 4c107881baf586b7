"""The MDTM objective (BOTE_OBJ_MDTM) in the host code, CPU only: the argument
checks of bote_sweep_create_keys and the key's bounds under ASan + UBSan
(tests/native/host_check_mdtm.cpp, a stand-alone program linked against
bote_host.cpp), the Python key helper and the CLI's objective parser."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NATIVE = os.path.join(ROOT, "tests", "native")
CSRC = os.path.join(ROOT, "fantoch_amd", "csrc")


@pytest.mark.skipif(shutil.which("g++") is None, reason="no host compiler")
def test_mdtm_objective_checks_under_asan_ubsan():
    out = os.path.join(NATIVE, "build", "host_check_mdtm")
    os.makedirs(os.path.dirname(out), exist_ok=True)
    # (the flags of tests/native/Makefile's host_check)
    subprocess.run([os.environ.get("CXX", "g++"), "-O1", "-g", "-std=c++17", "-Wall", "-Wextra",
                    "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-o", out,
                    os.path.join(NATIVE, "host_check_mdtm.cpp"), os.path.join(CSRC, "bote_host.cpp")], check=True)
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=1", UBSAN_OPTIONS="halt_on_error=1")
    r = subprocess.run([out], capture_output=True, text=True, env=env, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "mdtm host ok" in r.stdout, r.stdout
    assert "runtime error" not in r.stderr and "AddressSanitizer" not in r.stderr, r.stderr


def test_mdtm_key_helper_and_cli_objectives():
    from fantoch_amd import _lib, cli
    from fantoch_amd.bote import mdtm_key

    assert _lib.OBJ_MDTM == 18 and _lib.MDTM_SUM_BITS == 27
    with open(_lib.INCLUDE_H) as fh:
        text = fh.read()
    assert "#define BOTE_OBJ_MDTM 18" in text and "#define BOTE_MDTM_SUM_BITS 27" in text
    assert not _lib.is_pctl(_lib.OBJ_MDTM)
    assert mdtm_key((1234 << 27) | 3456) == (1234, 3456)
    assert mdtm_key(0) == (0, 0)
    assert mdtm_key(3456) == (0, 3456)
    # the largest halves: H = 4096^2 * 32766 / 4 < 2^37, sum = 4096 * 32766 < 2^27 - 1
    h, s = 4096 * 4096 * 32766 // 4, 4096 * 32766
    assert h < 1 << 37 and s < (1 << 27) - 1 and ((h << 27) | s) < (1 << 64) - 1
    assert mdtm_key((h << 27) | s) == (h, s)
    assert cli._objectives("mean:af1,mdtm:af1,mdtm:ff1C,score") == [
        (_lib.OBJ_MEAN, 0), (_lib.OBJ_MDTM, 0), (_lib.OBJ_MDTM, 6), (_lib.OBJ_SCORE, 0)]
    assert cli._objectives("mdtm:fl1") == [(_lib.OBJ_MDTM, _lib.SLOT_FL1)]
    assert cli._objective_name(_lib.OBJ_MDTM) == "mdtm"
