"""The stages' device arena (DevArena, csrc/msgpu_stage.h) tested by a stand-alone program, tests/cpp/test_arena.hip, built here
with the library's compiler and flags and run twice: with MSGPU_POISON in its environment (every block reads back as 0xA5,
a byte written behind or in front of a block is found by verify() and by drop() and named by block, size and side, a
rewound reservation is poisoned again) and without it (no guards, nothing verified); in both the addresses are 256-byte
aligned, get_zeroed gives zeros, and the offsets inside a reservation, live and peak are those of the other mode.  The bytes
the program writes outside a block lie in the arena's own guards: nothing out of bounds is touched."""
import os
import subprocess

import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "muchsalsa_amd", "csrc")


@pytest.fixture(scope="module")
def arena_bin(tmp_path_factory):
    out = str(tmp_path_factory.mktemp("cpp") / "test_arena")
    # HIPCC, ARCH and CXXFLAGS of csrc/Makefile (a program, so no -fPIC; -O1: it is compiled at test time)
    subprocess.run(["/opt/rocm/bin/hipcc", "--offload-arch=gfx950", "-O1", "-std=c++17", "-pthread", "-ffp-contract=off", "-Wall", "-Wextra",
                    "-Wno-unused-parameter", "-I", os.path.join(ROOT, "include"), "-I", CSRC,
                    os.path.join(ROOT, "tests", "cpp", "test_arena.hip"), "-o", out], check=True, timeout=600)
    return out


@pytest.mark.parametrize("poison", [True, False], ids=["poisoned", "plain"])
def test_the_arena_program(arena_bin, poison):
    env = {k: v for k, v in os.environ.items() if k != "MSGPU_POISON"}
    if poison:
        env["MSGPU_POISON"] = "1"
    r = subprocess.run([arena_bin], env=env, capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
    assert r.stdout.strip() == ("ok poisoned" if poison else "ok plain")
