"""The kernels of the unitig coverage filter and of the read scrubber at their edges, on the GPU: the inputs of
tests/ufedgecases.py (touching, empty, inverted and repeated lines in every width class of pass 1, staircases whose maximum
falls on the last lane, the last LDS line and the ends of the sweep's rounds, runs of 499 and 500 positions, a value equal to
the upper bound, a fractional Q3) and of tests/scrubedgecases.py (no pairs, no read-to-read lines, chunks of 2 ... 257 lines,
an edge whose first pair comes late, lines at 499 and 500 from the state, strands, a chain of 130 lines, group heads on every
lane, a pair folded in three batches, a pair that is never together, ranges that touch, hundreds of ranges on one node, the
trim, short records and the wrap) through the stages on files, compared as tests/test_gpu_unitig_filter.py and
tests/test_gpu_scrubber.py compare: the graph rows, the report and every output byte against the plain-Python restatements,
without any tolerance, and then against the hand-derived literals of the case.  That the inputs meet the conditions they were
built for is asserted in tests/test_scrub_uf_edges_host.py.  Every test runs under its own time limit: a watchdog ends the
process when a stage call does not come back."""
import faulthandler

import pytest

import scrubedgecases as S
import test_gpu_scrubber as scrubber_tests
import test_gpu_unitig_filter as filter_tests
import ufedgecases as U

pytestmark = pytest.mark.gpu

LIMIT = 600  # seconds per test
UF_PASS1 = U.names(pass2=False)
UF_PASS2 = U.names(pass2=True)
SCRUB = S.names()


@pytest.fixture(scope="module")
def stages():
    import __graft_entry__ as g
    g.build()
    from muchsalsa_amd import scrubber, unitig_filter
    return {"uf": unitig_filter, "sc": scrubber}


@pytest.fixture(autouse=True)
def time_limit(stages):  # (after stages: the build is not the test's time)
    faulthandler.dump_traceback_later(LIMIT, exit=True)  # works while the main thread sits in a native call
    yield
    faulthandler.cancel_dump_traceback_later()


def _filter(stages, tmp_path, name, packed):
    """test_gpu_unitig_filter._check on a case: the report and every output byte against the restatement"""
    c = U.cases()[name]
    res, wrep = filter_tests._check(stages["uf"], tmp_path, c.paf, c.fasta, packed)
    with open(str(tmp_path / "x.out.fa"), "rb") as h:
        got = h.read()
    want, rep = U.expected(name)
    assert wrep == rep and got == want
    assert {k: res[k] for k in ("wave_blocks", "group_blocks", "giant_blocks")} == U.classes(c.paf)
    return got, res


@pytest.mark.parametrize("packed", [False, True])
@pytest.mark.parametrize("name", UF_PASS1)
def test_filter_pass1(stages, tmp_path, name, packed):
    got, res = _filter(stages, tmp_path, name, packed)
    lit = U.cases()[name].lit
    print(name, "q3", res["q3"])
    assert res["q3"] == lit["q3"] and res["outliers"] == 0
    assert {k: res[k] for k in lit["klass"]} == lit["klass"]


@pytest.mark.parametrize("packed", [False, True])
@pytest.mark.parametrize("name", UF_PASS2)
def test_filter_pass2(stages, tmp_path, name, packed):
    got, res = _filter(stages, tmp_path, name, packed)
    lit = U.cases()[name].lit
    print(name, res["q1"], res["q3"], res["upper"], res["outliers"], res["rescued"], res["fragments"])
    assert (res["q1"], res["q3"], res["upper"], res["outliers"], res["rescued"]) == (
        lit["q1"], lit["q3"], lit["upper"], lit["outliers"], lit["rescued"])
    assert res["fragments"] == sum(len(f) for f in lit["frags"].values())
    lengths = U.record_lengths(got)
    for uid, frags in lit["frags"].items():
        assert U.fragments(got, uid) == frags and uid not in lengths
        for k, n, _, _ in frags:
            assert lengths[b"%s_%d" % (uid, k)] == lit["lengths"].get(b"%s_%d" % (uid, k), n)


@pytest.mark.parametrize("name", SCRUB)
def test_scrubber(stages, tmp_path, name):
    c = S.cases()[name]
    got, res, st = scrubber_tests._check(stages["sc"], tmp_path, c.anchors, c.ava, c.reads, c.subset_size)
    assert got == S.expected(name)[2]
    print(name, {k: res[k] for k in ("nodes", "edges", "pairs", "ava_lines", "batches", "records")})
    assert S.meets_literals(name, got, dict(res, chunks=st["chunks"])) == []
    if "row_x" in c.extra:  # late_first_pair: the rows of X and Y as the device built them
        _, _, graph = scrubber_tests._stage(stages["sc"], str(tmp_path), c.anchors, c.ava, c.reads, c.subset_size, tag="again")
        node = st["graph"]["node"]
        for r, key in (("X", "row_x"), ("Y", "row_y")):
            lo, hi = int(graph["row_off"][node[r]]), int(graph["row_off"][node[r] + 1])
            assert graph["adj"][lo:hi].tolist() == c.extra[key]
