"""The unitig assembly on keys of four 64-bit words (k = 97) once more on device memory that is poisoned and fenced, the way
tests/test_gpu_poisoned_arena.py runs the stages: MSGPU_POISON is set for every test of this file, so every block of the arena is
exactly as large as the request, reads 0xA5 until a kernel writes it and stands between guards that the run verifies before it
returns MSGPU_OK.  The loads and stores of keys of several words are the new memory traffic; a store one word too far lands in
a guard and fails the run by name.  The cases and the comparison are tests/test_gpu_unitigs_wide.py's."""
import faulthandler
import os

import pytest

import test_gpu_unitigs_wide as wide_tests

pytestmark = pytest.mark.gpu

LIMIT = 600  # seconds per test


@pytest.fixture(autouse=True)
def poison(monkeypatch):
    monkeypatch.setenv("MSGPU_POISON", "1")  # (the arena asks per call)


@pytest.fixture(scope="module")
def ug():
    import __graft_entry__ as g
    g.build()
    from muchsalsa_amd import unitigs
    return unitigs


@pytest.fixture(autouse=True)
def time_limit(ug):  # (after ug: the build is not the test's time)
    faulthandler.dump_traceback_later(LIMIT, exit=True)  # works while the main thread sits in a native call
    yield
    faulthandler.cancel_dump_traceback_later()


@pytest.mark.parametrize("name", ("ladder-97-97", "edge-97", "hairpin_gfa-97"))
def test_wide_keys_on_the_poisoned_arena(ug, tmp_path, name):
    """a ladder (count, tips, joins, doubling, order, write), a bubble case (forks, walks) and rule 10's links"""
    assert os.environ.get("MSGPU_POISON") == "1"
    wide_tests.check_case(ug, tmp_path, name)
