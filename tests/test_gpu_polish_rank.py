"""The polisher's rule 2 in ranked form on the GPU (msgpu_pl_run_ranked): a read votes with every primary of sufficient mapping
quality and never with a secondary -- the FASTA byte for byte, the counts and the record table against the plain-Python
restatement (tests/pl_rank_oracle.py around tests/pl_oracle.py, the rank rows by tests/map_rank_oracle.py), without any tolerance;
rule 1's check (j); polish.run and hybrid.run with min_mapq against run_tables on the files they name.  No test provokes a device
fault.  Every test runs under its own time limit."""
import faulthandler
import hashlib
import os

import pytest

import hybridcases
import map_oracle
import map_rank_oracle as ro
import pl_oracle
import pl_rank_oracle
import plcases

pytestmark = pytest.mark.gpu

LIMIT = 600  # seconds per test
EQ, X = plcases.EQ, plcases.X


@pytest.fixture(scope="module")
def pl():
    import __graft_entry__ as g
    g.build()
    from muchsalsa_amd import polish
    return polish


@pytest.fixture(autouse=True)
def time_limit(pl):
    faulthandler.dump_traceback_later(LIMIT, exit=True)
    yield
    faulthandler.cancel_dump_traceback_later()


def _case(draft, reads, chains, runs):
    return dict(draft=draft, reads=reads, chains=chains, runs=runs, params={}, note="")


def split_case():
    """a draft with 100 bases that no read has: four reads align with one part in front of them and one behind.  The draft's
    base 300, in the second part, is wrong"""
    G = plcases._g(2000, 31)
    truth = G[0:400]
    draft = truth[:300] + bytes([plcases.other(truth[300])]) + truth[301:]
    read = truth[0:150] + truth[250:400]
    reads = [(b"r%d" % q, read) for q in range(4)]
    chains, runs = [], []
    for q in range(4):
        first = [150 << 4 | EQ]
        second = [50 << 4 | EQ, 1 << 4 | X, 99 << 4 | EQ]
        chains += [plcases.chain(q, 0, 300, 0, 150, first, qs=0, qe=150, score=150), plcases.chain(q, 0, 300, 250, 400, second, qs=150, qe=300, score=140)]
        runs += [first, second]
    return _case([(b"d0", draft)], reads, chains, runs), truth


def repeat_case():
    """a draft with two copies of a repeat; three reads span copy 1 with its left flank, one read is the repeat alone and fits
    both copies equally.  Copy 2 of the draft has a wrong base that only the repeat-only read could vote on"""
    G = plcases._g(2000, 33)
    R = G[1000:1100]
    draft = G[0:200] + R + G[300:500] + R[:40] + bytes([plcases.other(R[40])]) + R[41:] + G[600:700]
    reads, chains, runs = [], [], []
    for q in range(3):  # [100, 300) of the draft: flank and copy 1
        reads.append((b"s%d" % q, draft[100:300]))
        runs.append([200 << 4 | EQ])
        chains.append(plcases.chain(q, 0, 200, 100, 300, runs[-1], score=200))
    reads.append((b"rep", R))
    one, two = [100 << 4 | EQ], [40 << 4 | EQ, 1 << 4 | X, 59 << 4 | EQ]
    chains += [plcases.chain(3, 0, 100, 200, 300, one, score=100), plcases.chain(3, 0, 100, 500, 600, two, score=100)]
    runs += [one, two]
    return _case([(b"d0", draft)], reads, chains, runs)


def _tables(pl, d, c, **how):
    dp, rp = plcases.write_case(c, d)
    out = os.path.join(str(d), "out.fa")
    if os.path.exists(out):
        os.remove(out)
    tb = {}
    res = pl.run_tables(dp, rp, out, c["chains"], c["runs"], tables=tb, **how)
    with open(out, "rb") as h:
        return res, tb, h.read()


def _same(pl, got, want):
    res, tb, text = got
    assert res["lost_publications"] == 0
    assert len(text) == len(want["text"]) and text == want["text"] == tb["text"]
    assert tb["records"] == want["records"]
    assert {k: res[pl._strip(k)] for k in pl_oracle.COUNTS} == {k: want[k] for k in pl_oracle.COUNTS}


def _ranks(chains):
    """the rows of the device (mapper.rank_tables), which are the restatement's"""
    from muchsalsa_amd import mapper
    rows = mapper.rank_tables(chains)
    assert rows == ro.rank(chains)
    return rows


def test_a_read_with_two_primaries_votes_with_both(pl, tmp_path):
    c, truth = split_case()
    ranks = _ranks(c["chains"])
    assert [r[0] for r in ranks] == list(range(8)) and all(r[3] == 18 for r in ranks)  # 60 * score * 3 anchors / (10 * score)
    plain = _tables(pl, tmp_path, c)
    _same(pl, plain, pl_oracle.run(c["draft"], c["reads"], c["chains"], c["runs"]))
    assert plain[0]["voters"] == 4 and plain[0]["cols_eq"] == 4 * 150 and plain[0]["cols_x"] == 0  # one part of every read
    assert plain[1]["records"][0][5] == 100 * 4 * 150 // 400 and plain[0]["pos_substituted"] == 0
    ranked = _tables(pl, tmp_path, c, ranks=ranks, min_mapq=1)
    _same(pl, ranked, pl_rank_oracle.run(c["draft"], c["reads"], c["chains"], c["runs"], ranks, min_mapq=1))
    assert ranked[0]["voters"] == 8 and ranked[0]["ignored"] == 0 and ranked[0]["cols_eq"] == 4 * 299 and ranked[0]["cols_x"] == 4
    assert ranked[1]["records"][0][5] == 100 * 4 * 300 // 400 and ranked[0]["pos_substituted"] == 1
    assert ranked[2] == pl_oracle.fasta(b"d0", truth)  # the wrong base behind the gap is corrected by the second parts
    assert _tables(pl, tmp_path, c, ranks=ranks, min_mapq=19)[0]["voters"] == 0


def test_a_read_on_two_repeat_copies_votes_at_min_mapq_0_only_and_a_secondary_never(pl, tmp_path):
    c = repeat_case()
    ranks = _ranks(c["chains"])
    assert ranks[3] == (3, 100, 1, 0) and ranks[4] == (3, 0, 0, 0) and all(r[3] > 0 for r in ranks[:3])
    for min_mapq, voters in ((0, [0, 1, 2, 3]), (1, [0, 1, 2])):
        want = pl_rank_oracle.run(c["draft"], c["reads"], c["chains"], c["runs"], ranks, min_mapq=min_mapq)
        assert want["voters"] == voters
        got = _tables(pl, tmp_path, c, ranks=ranks, min_mapq=min_mapq)
        _same(pl, got, want)
        assert got[0]["voters"] == len(voters) and got[0]["ignored"] == 5 - len(voters)
        assert got[0]["cols_x"] == 0  # chain 4, the secondary with the X column, never votes
        assert got[0]["max_depth"] == len(voters)  # (copy 1 is covered by the spanning reads and, at 0, by the repeat read)
    # with a better identity threshold nothing changes for the secondary either: eligibility comes first, primacy still holds
    got = _tables(pl, tmp_path, c, ranks=ranks, min_mapq=0, min_identity=100)
    _same(pl, got, pl_rank_oracle.run(c["draft"], c["reads"], c["chains"], c["runs"], ranks, min_mapq=0, min_identity=100))


def test_a_bad_rank_row_is_an_error_reported_last_and_the_context_goes_on(pl, tmp_path):
    from muchsalsa_amd import _lib
    c = repeat_case()
    good = ro.rank(c["chains"])
    want = pl_rank_oracle.run(c["draft"], c["reads"], c["chains"], c["runs"], good)
    out = os.path.join(str(tmp_path), "out.fa")

    def with_row(i, row):
        rows = list(good)
        rows[i] = row
        return rows

    bad = {"parent out of range": (with_row(4, (5, 0, 0, 0)), 4), "parent of another query record": (with_row(4, (2, 0, 0, 0)), 4),
           "parent that is no primary": (with_row(3, (4, 0, 0, 0)), 3), "mapq beyond 60": (with_row(1, (1, 0, 0, 61)), 1),
           "the largest parent": (with_row(0, (4294967295, 0, 0, 0)), 0)}
    with pl.Context() as ctx:
        for name, (rows, chain) in sorted(bad.items()):
            with pytest.raises(pl_oracle.PolishError) as w:
                pl_rank_oracle.run(c["draft"], c["reads"], c["chains"], c["runs"], rows)
            assert (w.value.chain, w.value.what) == (chain, "rank"), name
            with pytest.raises(pl.PolishError) as e:
                _tables(pl, tmp_path, c, ranks=rows, context=ctx)
            print(name, e.value)
            assert e.value.code == _lib.E_ARG and "chain %d: rank (" % chain in str(e.value), name
            assert not os.path.exists(out)
            _same(pl, _tables(pl, tmp_path, c, ranks=good, context=ctx), want)
        # (j) is reported last: the same chain's query range is wrong too; and a smaller chain's other violation comes first
        chains = list(c["chains"])
        chains[4] = chains[4][:7] + (101,) + chains[4][8:]
        both = dict(c, chains=chains)
        for rows in (with_row(4, (5, 0, 0, 0)), with_row(4, (3, 0, 0, 99))):
            with pytest.raises(pl.PolishError) as e:
                _tables(pl, tmp_path, both, ranks=rows, context=ctx)
            assert "chain 4: query range (" in str(e.value)
        with pytest.raises(pl.PolishError) as e:
            _tables(pl, tmp_path, both, ranks=with_row(1, (1, 0, 0, 61)), context=ctx)
        assert "chain 1: rank (" in str(e.value)
        # msgpu_pl_run does not look at ranks: the plain form on the same context, unchanged
        _same(pl, _tables(pl, tmp_path, c, context=ctx), pl_oracle.run(c["draft"], c["reads"], c["chains"], c["runs"]))


def test_polish_run_with_min_mapq_is_the_ranked_mapping_and_run_tables(pl, tmp_path):
    """polish.run(min_mapq=1) on the planted workload: the PAF is the restatement's ranked one, the FASTA is run_tables' on the
    mapper's tables and the restatement's; without min_mapq the bytes are those of the plain form"""
    from muchsalsa_amd import mapper
    wl = plcases.workload("planted")
    draft, reads = map_oracle.parse(wl["draft"], False), map_oracle.parse(wl["reads"], False)
    mapped = plcases.expected_workload("planted")[1]
    rows = ro.rank(mapped["chains"])
    want = pl_rank_oracle.run(draft, reads, mapped["chains"], mapped["packed"], rows, min_mapq=1)
    dp, rp = plcases.write_workload("planted", tmp_path)
    out, paf = os.path.join(str(tmp_path), "out.fa"), os.path.join(str(tmp_path), "kept.paf")
    tb = {}
    res = pl.run(dp, rp, out, tables=tb, paf=paf, min_mapq=1)
    with open(paf, "rb") as h:
        assert h.read() == ro.ranked_paf(mapped["paf"], rows)
    with open(out, "rb") as h:
        text = h.read()
    _same(pl, (res, tb, text), want)
    mt = {}
    mapper.run(dp, rp, os.path.join(str(tmp_path), "again.paf"), tables=mt, cigar=1, exact=1, rank=True)
    assert mt["ranks"] == rows and mt["chains"] == mapped["chains"]
    again = os.path.join(str(tmp_path), "again.fa")
    pl.run_tables(dp, rp, again, mt["chains"], mt["runs"], ranks=mt["ranks"], min_mapq=1)
    with open(again, "rb") as h:
        assert h.read() == text
    print("planted: %d chains, %d voters at min_mapq = 1 (%d in the plain form)" % (res["chains"], res["voters"],
                                                                                 plcases.expected_workload("planted")[0]["n_voters"]))
    plain = os.path.join(str(tmp_path), "plain.fa")
    pl.run(dp, rp, plain)
    with open(plain, "rb") as h:
        assert h.read() == plcases.expected_workload("planted")[0]["text"]


def test_the_driver_passes_min_mapq_to_the_polish_stage_alone(pl, tmp_path):
    """hybrid.run(polish=1, min_mapq=1): every file of the pipeline has the recorded length and digest (the four mappings keep
    ranking off), and the polished file is polish.run's and run_tables' on the files the driver names"""
    from muchsalsa_amd import hybrid, mapper
    (tmp_path / "in").mkdir()
    inputs = hybridcases.write_inputs(tmp_path / "in")
    out = str(tmp_path / "out")
    res = hybrid.run(hybridcases.K_FILTER, hybridcases.K_ASSEMBLY, hybridcases.NAME, inputs[0], inputs[1], inputs[2], out, polish=1,
                     min_mapq=1)
    for rel, rec in sorted(hybridcases.expected()["files"].items()):
        with open(os.path.join(out, rel), "rb") as h:
            data = h.read()
        assert (len(data), hashlib.sha256(data).hexdigest()) == (rec["bytes"], rec["sha256"]), rel
    for key in ("map_unitigs", "map_corrected", "ava", "map_exact"):
        assert "rank" not in res[key] and "ranks" not in res[key]
    files = res["files"]
    with open(files["polished"], "rb") as h:
        polished = h.read()
    alone = os.path.join(str(tmp_path), "alone.fa")
    pl.run(files["assembly"], files["scrubbed"], alone, min_mapq=1)
    mt = {}
    mapper.run(files["assembly"], files["scrubbed"], os.path.join(str(tmp_path), "m.paf"), tables=mt, cigar=1, exact=1, rank=True)
    tables = os.path.join(str(tmp_path), "tables.fa")
    got = pl.run_tables(files["assembly"], files["scrubbed"], tables, mt["chains"], mt["runs"], ranks=mt["ranks"], min_mapq=1)
    with open(alone, "rb") as a, open(tables, "rb") as b:
        assert a.read() == b.read() == polished and len(polished) > 0
    assert got["voters"] == res["polish"]["voters"] >= 1 and mt["ranks"] == ro.rank(mt["chains"])
