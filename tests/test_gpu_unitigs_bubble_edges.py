"""Bubble popping (rule 9) on the GPU, on the edge inputs of tests/ugbubbleedgecases.py: structures aimed at single lines of
k_ug_forks, k_ug_bubbles and the phase loop -- four lanes of a quad at work, two bubbles in one quad, a lane that walks to a merge
of its own, branches of one and two k-mers, the limit between two branch lengths and at the parameter's cap, products that
differ by less than a branch length, ties on either strand, self-complementary forks and merges, a second phase that pops, forks
over several workgroups in tangled graphs -- at key widths on both sides of one and of two 64-bit words.  Every case is compared
with the plain-Python restatement (tests/ug_bubble_oracle.py) without any tolerance: both FASTA texts, the unitig table, the tip
rounds, the bubble rounds and what msgpu_ug_result_bubbles says; once more with every read reverse-complemented; and with the
unitig graph on (rule 10) against tests/ug_graph_oracle.py on the popped result.  The fixtures, the watchdog and the comparison
are those of tests/test_gpu_unitigs_bubbles.py.  No test provokes a device fault."""
import time

import pytest

import test_gpu_unitigs_bubbles as base
import test_gpu_unitigs_graph as graph_tests
import ugbubbleedgecases as cases
from test_gpu_unitigs_bubbles import time_limit, ug  # noqa: F401  (fixtures)

pytestmark = pytest.mark.gpu


def _totals(want):
    """msgpu_ug_bubble_stats without its times, from a result of the restatement"""
    br = want["bubble_rounds"]
    return dict(bubble=want["bubble"], n_phases=want["bubble_phases"], n_rounds=len(br), reserved=0, n_bubbles=want["bubbles"],
                n_branches_removed=want["bubble_branches"], n_kmers_removed=want["bubble_kmers"],
                max_forks=max(b[1] for b in br), reserved2=0)


@pytest.mark.parametrize("name,k", cases.CASES)
def test_against_the_restatement(ug, tmp_path, name, k):  # noqa: F811
    data, prm = cases.workload(name, k)[0], cases.params(name, k)
    flipped = cases.flipped(data)
    wants = [cases.expected(name, k, bubble=None if pops is None else bubble)[0] for bubble, pops in cases.runs(name, k)]
    t0 = time.perf_counter()  # (the seconds printed are the stage's, not the restatement's)
    paths = base._paths(tmp_path, "ctx")
    base._write(paths, [data])
    by_ctx = dict(trim=prm["trim"], min_length=prm["min_length"], min_count=prm["min_count"])
    bctx, gctx = base._Ctx(), graph_tests._Ctx()
    try:
        # (a case with several values of ``bubble`` runs them on these two contexts one behind the other: pops, does not, pops)
        for i, ((bubble, pops), want) in enumerate(zip(cases.runs(name, k), wants)):
            assert want["bubble"] == bubble
            if pops is not None:
                assert (want["bubble_kmers"] > 0) == pops and cases.unpopped(name, k, want) == (not pops)
            # the stage by its Python entry, and the same input with every read reverse-complemented
            for tag, d in (("f%d" % i, data), ("r%d" % i, flipped)):
                res, tb, texts = base._stage(ug, tmp_path, k, [d], tag, **dict(prm, bubble=bubble))
                base._equal(res, tb, texts, want)
                assert res["bubble_max_forks"] == max(b[1] for b in want["bubble_rounds"])
            # one context: what msgpu_ug_result_bubbles says
            assert bctx.set(bubble) == bctx.lib.OK
            got = bctx.run(k, paths, **by_ctx)
            assert got[:3] == (want["all"], want["cut"], want["rounds"]) and got[4] == want["bubble_rounds"]
            stats = {key: v for key, v in got[3].items() if not key.endswith("_ms")}
            assert stats == _totals(want)
            # rule 10 on the popped result, and the graph off again
            gctx.bubbles(bubble)
            graph_tests._on_and_off(gctx, k, paths[:1], want, **by_ctx)
            print("%s k %d bubble %d: tip rounds %r, bubble rounds %r, %d phases, %d unitigs" % (
                name, k, bubble, want["rounds"], want["bubble_rounds"], want["bubble_phases"], len(want["unitigs"])))
    finally:
        bctx.close()
        gctx.close()
    print("%s k %d: %.3f s" % (name, k, time.perf_counter() - t0))
