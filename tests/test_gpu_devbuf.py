"""The overlap context's device buffer (DevBuf, csrc/msgpu_devbuf.h) tested by a stand-alone program, tests/cpp/test_devbuf.hip,
built here with the library's compiler and flags and run twice: with MSGPU_POISON in its environment (a block is exactly as
large as the request and reads back as 0xA5, a byte written at `size` or at -1 is found by check() and named by buffer, size
and side, a view that outgrows its allocation keeps its first `off` bytes and gets fresh guards, every larger request
reallocates, a block that is given back is checked first) and without it (need + need/8 + 256, `hint`, `grow_by`, no guards,
no allocation inside the slack).  The bytes the program writes outside a block lie in the buffer's own guards: nothing out
of bounds is touched.  This program is the proof that fill and guards work; no test shows it by damaging a context."""
import os
import subprocess

import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "muchsalsa_amd", "csrc")


@pytest.fixture(scope="module")
def devbuf_bin(tmp_path_factory):
    out = str(tmp_path_factory.mktemp("cpp") / "test_devbuf")
    # HIPCC, ARCH and CXXFLAGS of csrc/Makefile (a program, so no -fPIC; -O1: it is compiled at test time)
    subprocess.run(["/opt/rocm/bin/hipcc", "--offload-arch=gfx950", "-O1", "-std=c++17", "-pthread", "-ffp-contract=off", "-Wall", "-Wextra",
                    "-Wno-unused-parameter", "-I", os.path.join(ROOT, "include"), "-I", CSRC,
                    os.path.join(ROOT, "tests", "cpp", "test_devbuf.hip"), "-o", out], check=True, timeout=600)
    return out


@pytest.mark.parametrize("poison", [True, False], ids=["poisoned", "plain"])
def test_the_devbuf_program(devbuf_bin, poison):
    env = {k: v for k, v in os.environ.items() if k != "MSGPU_POISON"}
    if poison:
        env["MSGPU_POISON"] = "1"
    r = subprocess.run([devbuf_bin], env=env, capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
    assert r.stdout.strip() == ("ok poisoned" if poison else "ok plain")
