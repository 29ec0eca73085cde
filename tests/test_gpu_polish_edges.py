"""The kernels of the polishing stage at their edges, on the GPU: the inputs of tests/pledgecases.py (more than 256 chains,
reads and draft records, voters between non-voters in every block, chains of one column, spans that end on the first and last
lane of a block, insertion events in a second record, 256 events, groups of events across a block, 32-letter insertions that
differ in the highest and in the lowest bits, I runs of 64 and 65 letters, insertions beside deletions and beside each other,
depths of min_depth - 1 on either side of a slot, negative scores, identities at 2^32 - 1, lower case on strand 1, a draft N,
"other" votes alone, records that come out with 60, 61 and 120 bases, D at a chain's ends, the ranked form over two blocks)
through run_tables, compared as tests/test_gpu_polish.py compares: the FASTA byte for byte, every count and the record table
against the plain-Python restatements, without any tolerance, and then against the hand-derived literals of the case.  That the
inputs meet the conditions they were built for is asserted in tests/test_polish_edges_host.py.  No test provokes a device
fault: the tables that break rule 1 must end in an error before a kernel walks a run.  Every test runs under its own time
limit: a watchdog ends the process when a stage call does not come back."""
import faulthandler
import os

import pytest

import pl_oracle
import plcases
import pledgecases as P
import test_gpu_polish as base

pytestmark = pytest.mark.gpu

LIMIT = 600  # seconds per test
CASES = P.names()
VIOLATIONS = sorted(P.violations())


@pytest.fixture(scope="module")
def pl():
    import __graft_entry__ as g
    g.build()
    from muchsalsa_amd import polish
    return polish


@pytest.fixture(autouse=True)
def time_limit(pl):  # (after pl: the build is not the test's time)
    faulthandler.dump_traceback_later(LIMIT, exit=True)  # works while the main thread sits in a native call
    yield
    faulthandler.cancel_dump_traceback_later()


def _run(pl, d, name, **more):
    c = P.cases()[name]
    return base._tables(pl, d, dict(c, params=P.how(c)), **more)


def _check(pl, got, name):
    """test_gpu_polish._same against the restatement, then the case's literals"""
    res, tb, text = got
    base._same(pl, res, tb, text, P.expected(name))
    assert P.meets_literals(name, text, tb["records"], {k: res[pl._strip(k)] for k in pl_oracle.COUNTS}) == []


@pytest.mark.parametrize("name", CASES)
def test_edge_case(pl, tmp_path, name):
    got = _run(pl, tmp_path, name)
    print(name, P.cases()[name]["note"], got[0])
    _check(pl, got, name)


def test_rule_1_on_a_table_of_600_chains_and_the_context_goes_on(pl, tmp_path):
    """each broken table -> MSGPU_E_ARG naming the chain and what is wrong, nothing written; the same context then polishes
    the unbroken table correctly"""
    from muchsalsa_amd import _lib
    out = os.path.join(str(tmp_path), "out.fa")
    with pl.Context() as ctx:
        for name in VIOLATIONS:
            c, ranks, chain, what = P.violations()[name]
            dp, rp = plcases.write_case(c, tmp_path)
            how = {} if ranks is None else dict(ranks=ranks)
            with pytest.raises(pl.PolishError) as e:
                pl.run_tables(dp, rp, out, c["chains"], c["runs"], context=ctx, **how)
            print(name, e.value)
            assert e.value.code == _lib.E_ARG and "chain %d: %s (" % (chain, what) in str(e.value), name
            assert not os.path.exists(out)
            _check(pl, _run(pl, tmp_path, "chains_600_interleaved", context=ctx), "chains_600_interleaved")
            os.remove(out)


def test_nothing_of_a_large_run_survives_into_the_next(pl, tmp_path):
    with pl.Context() as ctx:
        a = _run(pl, tmp_path, "events_256", context=ctx)
        b = _run(pl, tmp_path, "records_300", context=ctx)
        c = _run(pl, tmp_path, "events_256", context=ctx)
    assert a[2] == c[2] and a[1] == c[1] and a[0] == c[0]
    _check(pl, a, "events_256")
    _check(pl, b, "records_300")


def test_planted_in_three_records_through_the_mapper(pl, tmp_path):
    wl = P.planted_three_records()
    dp, rp, out = (os.path.join(str(tmp_path), n) for n in ("draft.fa", "reads.fa", "out.fa"))
    with open(dp, "wb") as f:
        f.write(wl["draft"])
    with open(rp, "wb") as f:
        f.write(wl["reads"])
    tb = {}
    res = pl.run(dp, rp, out, tables=tb)
    want, mapped = P.expected_planted_three_records()
    print(res)
    assert res["rounds"][0]["map"]["chains"] == len(mapped["chains"])
    with open(out, "rb") as h:
        text = h.read()
    base._same(pl, res, tb, text, want)
    assert all(tb["records"][r][4] >= 10 for r in (1, 2)) and tb["records"][3] == (500, 500, 0, 0, 0, 0)
    assert text.endswith(P.wrap(b"unmapped", wl["unmapped"]))
