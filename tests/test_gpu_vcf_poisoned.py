"""The VCF output's cases once more, on device memory that is poisoned and fenced, as tests/test_gpu_sam_poisoned.py does it for
the SAM stage: MSGPU_POISON is set for every test of this file, so every block of the polisher's arena, the VCF's among them,
comes filled with 0xA5 and lies between guards that the stage checks before it returns MSGPU_OK.  The inputs and the
comparisons are those of tests/test_gpu_vcf.py, whose checks this file calls: every byte of the text and every row of the
variant table against the plain-Python restatement.  A difference under poison is a byte of the text, or a word of a row, that
a kernel read before anything wrote it -- a line whose size the count pass got wrong shows here as 0xA5 between two lines; a
stage error that begins with "arena guard:" is a write outside a block.  No test provokes a device fault."""
import faulthandler

import pytest

import test_gpu_vcf as base

pytestmark = pytest.mark.gpu

LIMIT = 600  # seconds per test


@pytest.fixture(autouse=True)
def poison(monkeypatch):
    monkeypatch.setenv("MSGPU_POISON", "1")  # (the arena asks per call)


@pytest.fixture(scope="module")
def pl():
    import __graft_entry__ as g
    g.build()
    from muchsalsa_amd import polish
    return polish


@pytest.fixture(scope="module")
def stage(pl):
    with pl.Context() as ctx:
        yield ctx


@pytest.fixture(autouse=True)
def time_limit(pl):  # (after pl: the build is not the test's time)
    faulthandler.dump_traceback_later(LIMIT, exit=True)  # works while the main thread sits in a native call
    yield
    faulthandler.cancel_dump_traceback_later()


@pytest.mark.parametrize("kind,name", base.CASES)
def test_case(pl, stage, tmp_path, kind, name):
    base.test_case(pl, stage, tmp_path, kind, name)


def test_the_ranked_form_feeds_the_same_code(pl, stage, tmp_path):
    base.test_the_ranked_form_feeds_the_same_code(pl, stage, tmp_path)


def test_the_mates_form_feeds_the_same_code(pl, stage, tmp_path):
    base.test_the_mates_form_feeds_the_same_code(pl, stage, tmp_path)


def test_v7_refuses_a_name_and_the_context_goes_on(pl, stage, tmp_path):
    base.test_v7_refuses_a_name_and_the_context_goes_on(pl, stage, tmp_path)


def test_nothing_of_a_large_run_survives_into_the_next(pl, stage, tmp_path):
    base.test_nothing_of_a_large_run_survives_into_the_next(pl, stage, tmp_path)
