"""The SAM stage's cases once more, on device memory that is poisoned and fenced, as tests/test_gpu_poisoned_arena.py does it
for the other stages: MSGPU_POISON is set for every test of this file, so every block of the stage's two arenas (the resident
tables; the batch's reservation) comes filled with 0xA5 and lies between guards that the stage checks before it returns
MSGPU_OK.  The inputs and the comparisons are those of tests/test_gpu_sam.py, whose checks this file calls: every byte of the
text and every entry of the line table against the plain-Python restatement.  A difference under poison is a byte of the text,
or a table entry, that a kernel read before anything wrote it -- a line whose size the count pass got wrong shows here as 0xA5
between two lines; a stage error that begins with "arena guard:" is a write outside a block.  No test provokes a device
fault."""
import faulthandler

import pytest

import samcases
import test_gpu_sam as base

pytestmark = pytest.mark.gpu

LIMIT = 300  # seconds per test


@pytest.fixture(autouse=True)
def poison(monkeypatch):
    monkeypatch.setenv("MSGPU_POISON", "1")  # (the arena asks per call)


@pytest.fixture(scope="module")
def mods():
    import __graft_entry__ as g
    g.build()
    from muchsalsa_amd import _lib, mapper, sam
    return {"lib": _lib, "mp": mapper, "sam": sam}


@pytest.fixture(scope="module")
def stage(mods):
    with mods["sam"].Context() as ctx:
        yield ctx


@pytest.fixture(autouse=True)
def time_limit(mods):  # (after mods: the build is not the test's time)
    faulthandler.dump_traceback_later(LIMIT, exit=True)  # works while the main thread sits in a native call
    yield
    faulthandler.cancel_dump_traceback_later()


@pytest.mark.parametrize("name", samcases.names())
def test_against_the_restatement(mods, stage, tmp_path, name):
    base.check_case(mods, stage, tmp_path, name)


@pytest.mark.parametrize("name", [b[0] for b in samcases.BAD])
def test_every_violation_of_s1_is_its_error_text(mods, stage, tmp_path, name):
    base.check_bad(mods, stage, tmp_path, name)


def test_batches(mods, stage, tmp_path):
    """the batch arena is rewound, and poisoned again, between the batches"""
    base.test_batches(mods, stage, tmp_path)


def test_the_paired_workload_through_the_mapper(mods, tmp_path):
    base.test_the_paired_workload_through_the_mapper(mods, tmp_path)
