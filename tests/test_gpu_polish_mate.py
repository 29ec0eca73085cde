"""The polisher's rule 2 in mates form on the GPU (msgpu_pl_run_mates): a chain votes iff it is eligible, selected and its pair is
placed best once -- the FASTA byte for byte, the counts and the record table against the plain-Python restatement
(tests/pl_mate_oracle.py around tests/pl_oracle.py, the mate rows by tests/map_mate_oracle.py), without any tolerance; rule 1's
check (k); polish.run with mates against the restatements of the mapper and of the polisher.  No test provokes a device fault.
Every test runs under its own time limit."""
import faulthandler
import functools
import os

import pytest

import map_cigar_oracle
import map_mate_oracle as mo
import map_oracle
import pl_mate_oracle
import pl_oracle
import plcases

pytestmark = pytest.mark.gpu

LIMIT = 600  # seconds per test
EQ, X = plcases.EQ, plcases.X
MIN_SCORE = 40


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


def repeat_pairs_case():
    """a draft with two copies of a 120-base repeat that differ in one base (base 40 of copy B).  Three pairs: mate 1 lies
    inside copy A, reverse, and has a chain of the same score on either copy, the one on copy B (with its X column) first in
    table order; mate 2 lies forward in A's unique flank.  Chains 3p, 3p + 1, 3p + 2 are pair p's: on B, on A, in the flank"""
    G = plcases._g(3000, 41)
    R = G[2000:2120]
    RB = R[:40] + bytes([plcases.other(R[40])]) + R[41:]
    draft = G[0:200] + R + G[400:600] + RB + G[700:800]  # copy A at 200, copy B at 520
    reads, chains, runs = [], [], []
    for p in range(3):
        inside = R[10:110]
        reads.append((b"p%d/1" % p, map_oracle.revcomp(inside)))
        reads.append((b"p%d/2" % p, draft[20 + 10 * p:120 + 10 * p]))
        on_b, on_a, flank = [30 << 4 | EQ, 1 << 4 | X, 69 << 4 | EQ], [100 << 4 | EQ], [100 << 4 | EQ]
        chains += [plcases.chain(2 * p, 0, 100, 530, 630, on_b, strand=1, score=100), plcases.chain(2 * p, 0, 100, 210, 310, on_a, strand=1, score=100),
                   plcases.chain(2 * p + 1, 0, 100, 20 + 10 * p, 120 + 10 * p, flank, score=100)]
        runs += [on_b, on_a, flank]
    return dict(draft=[(b"d0", draft)], reads=reads, chains=chains, runs=runs, params={}, note="")


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


def _rows(chains, max_insert):
    """the rows of the device (mapper.mate_tables), which are the restatement's"""
    from muchsalsa_amd import mapper
    rows = mapper.mate_tables(chains, max_insert=max_insert)
    assert rows == mo.mates(chains, max_insert)[0]
    return rows


def test_a_read_inside_a_repeat_votes_on_the_copy_its_mate_names(pl, tmp_path):
    c = repeat_pairs_case()
    rows = _rows(c["chains"], 400)  # (at 400 the chain on copy B is too far from the flank: one concordant combination)
    assert [r[2] for r in rows] == [0, 1, 1] * 3 and all(r[3] == 1 for r in rows if r[2]) and rows[1] == (2, 290, 1, 1)
    draft = c["draft"][0][1]
    want = pl_mate_oracle.run(c["draft"], c["reads"], c["chains"], c["runs"], rows)
    assert want["voters"] == [1, 2, 4, 5, 7, 8]
    got = _tables(pl, tmp_path, c, mates=rows)
    _same(pl, got, want)
    assert got[0]["voters"] == 6 and got[0]["ignored"] == 3 and got[0]["cols_x"] == 0 and got[0]["cols_eq"] == 600
    assert got[1]["records"][0][5] == want["records"][0][5] and got[0]["pos_substituted"] == 0
    assert got[2] == pl_oracle.fasta(b"d0", draft)  # copy B keeps its own base: nobody voted there
    # msgpu_pl_run on the same table takes the first chain in table order at equal score and block: the one on copy B
    plain = _tables(pl, tmp_path, c)
    want_plain = pl_oracle.run(c["draft"], c["reads"], c["chains"], c["runs"])
    assert want_plain["voters"] == [0, 2, 3, 5, 6, 8]
    _same(pl, plain, want_plain)
    assert plain[0]["voters"] == 6 and plain[0]["cols_x"] == 3 and plain[0]["pos_substituted"] == 1
    assert plain[2] != got[2] and plain[2] == pl_oracle.fasta(b"d0", draft[:520] + draft[200:320] + draft[640:])  # copy B overwritten by A


def test_an_ambiguous_pair_votes_nowhere_and_an_unselected_chain_never(pl, tmp_path):
    c = repeat_pairs_case()
    rows = _rows(c["chains"], 1000)  # both copies within reach of the flank: equal sums, n_best = 2
    assert [r[2:] for r in rows] == [(0, 0), (1, 2), (1, 2)] * 3
    want = pl_mate_oracle.run(c["draft"], c["reads"], c["chains"], c["runs"], rows)
    got = _tables(pl, tmp_path, c, mates=rows)
    _same(pl, got, want)
    assert want["voters"] == [] and got[0]["voters"] == 0 and got[0]["ignored"] == 9 and got[0]["max_depth"] == 0
    # the chains on copy B carry the X column; selected by nobody, they vote at no max_insert, whatever their identity
    for max_insert in (400, 1000):
        got = _tables(pl, tmp_path, c, mates=_rows(c["chains"], max_insert), min_identity=100)
        assert got[0]["cols_x"] == 0
    # an ineligible selected chain does not vote either: eligibility comes first
    low = dict(c, chains=[ch[:10] + (90, 100) if i % 3 == 1 else ch for i, ch in enumerate(c["chains"])])
    rows = _rows(low["chains"], 400)
    got = _tables(pl, tmp_path, low, mates=rows, min_identity=95)
    _same(pl, got, pl_mate_oracle.run(low["draft"], low["reads"], low["chains"], low["runs"], rows, min_identity=95))
    assert got[0]["voters"] == 3


def test_a_bad_mate_row_is_an_error_reported_last_and_the_context_goes_on(pl, tmp_path):
    from muchsalsa_amd import _lib
    c = repeat_pairs_case()
    good = mo.mates(c["chains"], 400)[0]
    tl = good[1][1]
    want = pl_mate_oracle.run(c["draft"], c["reads"], c["chains"], c["runs"], good)
    out = os.path.join(str(tmp_path), "out.fa")

    def with_rows(**rows):
        table = list(good)
        for i, row in rows.items():
            table[int(i[1:])] = row
        return table

    bad = {"mate out of range": (with_rows(r1=(9, tl, 1, 1)), 1), "the largest mate": (with_rows(r4=(4294967295, tl, 1, 1)), 4),
           "mate's row naming another chain": (with_rows(r2=(0, tl, 1, 1)), 1),
           "mate of the same query record": (with_rows(r0=(1, tl, 1, 1), r1=(0, tl, 1, 1)), 0),
           "mate of another pair": (with_rows(r1=(5, tl, 1, 1), r5=(1, tl, 1, 1), r2=mo.EMPTY, r4=mo.EMPTY), 1),
           "cls = 2": (with_rows(r0=(mo.NONE, 0, 2, 0)), 0), "selected with n_best = 0": (with_rows(r1=(2, tl, 1, 0), r2=(1, tl, 1, 0)), 1)}
    with pl.Context() as ctx:
        for name, (rows, chain) in sorted(bad.items()):
            with pytest.raises(pl_oracle.PolishError) as w:
                pl_mate_oracle.run(c["draft"], c["reads"], c["chains"], c["runs"], rows)
            assert (w.value.chain, w.value.what) == (chain, "mates"), name
            with pytest.raises(pl.PolishError) as e:
                _tables(pl, tmp_path, c, mates=rows, context=ctx)
            print(name, e.value)
            assert e.value.code == _lib.E_ARG and "chain %d: mates (" % chain in str(e.value), name
            assert not os.path.exists(out)
            _same(pl, _tables(pl, tmp_path, c, mates=good, context=ctx), want)
        # (k) is reported last: the same chain's query range (f) is wrong too; and a smaller chain's (k) comes first
        chains = list(c["chains"])
        chains[4] = chains[4][:7] + (101,) + chains[4][8:]
        both = dict(c, chains=chains)
        with pytest.raises(pl.PolishError) as e:
            _tables(pl, tmp_path, both, mates=with_rows(r4=(9, tl, 1, 1)), context=ctx)
        assert "chain 4: query range (" in str(e.value)
        with pytest.raises(pl.PolishError) as e:
            _tables(pl, tmp_path, both, mates=with_rows(r1=(9, tl, 1, 1)), context=ctx)
        assert "chain 1: mates (" in str(e.value)
        # msgpu_pl_run does not look at mate rows: the plain form on the same context, unchanged
        _same(pl, _tables(pl, tmp_path, c, context=ctx), pl_oracle.run(c["draft"], c["reads"], c["chains"], c["runs"]))
    with pytest.raises(TypeError):
        pl.run_tables("d", "r", out, c["chains"], c["runs"], mates=good, ranks=[(i, 0, 0, 0) for i in range(9)])


# ---- polish.run(mates=True)

PLANTED = (100, 125, 150)  # offsets inside the repeat's second copy at which the draft is wrong


@functools.lru_cache(maxsize=None)
def planted():
    """synth.mates_workload's genome (one 250-base repeat, two copies), error-free pairs drawn from it, and a draft that is the
    genome with three substitutions in the middle of the second copy: every read that covers them lies inside the repeat"""
    from muchsalsa_amd import synth
    w = synth.mates_workload(genome=4000, seed=1, coverage=12, read_len=100, insert=300, repeat_len=250)
    g = w["genome"]
    at = [w["repeats"][1] + o for o in PLANTED]
    draft = bytearray(g)
    for p in at:
        draft[p] = plcases.other(g[p])
    one, two = map_oracle.parse(w["illumina_1"], True), map_oracle.parse(w["illumina_2"], True)
    reads = [r for pair in zip(one, two) for r in pair]
    return dict(w, draft=bytes(draft), at=at, reads=reads)


def test_polish_run_with_mates_is_the_mated_mapping_and_run_tables(pl, tmp_path):
    """polish.run(mates=True) on the planted case: the PAF is the restatement's with rule 13's tags, the FASTA is the
    restatement's; the errors planted inside the repeat copy are corrected with mates on, and not with mates off, where every
    read that covers them fits the other, intact copy better"""
    from muchsalsa_amd import mapper
    w = planted()
    paths = {}
    for key, text in (("draft", b">g\n" + w["draft"] + b"\n"), ("illumina_1", w["illumina_1"]), ("illumina_2", w["illumina_2"])):
        paths[key] = os.path.join(str(tmp_path), key + (".fa" if key == "draft" else ".fq"))
        with open(paths[key], "wb") as h:
            h.write(text)
    pairs = os.path.join(str(tmp_path), "pairs.fq")
    assert mapper.interleave(paths["illumina_1"], paths["illumina_2"], pairs) == len(w["reads"]) // 2
    draft = [(b"g", w["draft"])]
    mapped = map_cigar_oracle.cigar_run(draft, w["reads"], min_score=MIN_SCORE, exact=1)
    rows, counts = mo.mates(mapped["chains"], 1000, n_records=len(w["reads"]))
    want = pl_mate_oracle.run(draft, w["reads"], mapped["chains"], mapped["packed"], rows)
    out, paf = os.path.join(str(tmp_path), "out.fa"), os.path.join(str(tmp_path), "kept.paf")
    tb = {}
    res = pl.run(paths["draft"], pairs, out, tables=tb, paf=paf, mates=True, min_score=MIN_SCORE)
    with open(paf, "rb") as h:
        assert h.read() == mo.mated_paf(mapped["paf"], rows)
    with open(out, "rb") as h:
        text = h.read()
    _same(pl, (res, tb, text), want)
    assert {k: res["rounds"][0]["map"]["mate"][k] for k in mo.STATS} == counts
    polished = b"".join(text.split(b"\n")[1:])
    print("planted: %d chains, %d voters, %r" % (res["chains"], res["voters"], counts))
    assert len(polished) == len(w["genome"]) and all(polished[p] == w["genome"][p] for p in w["at"])
    plain = os.path.join(str(tmp_path), "plain.fa")
    pl.run(paths["draft"], pairs, plain, min_score=MIN_SCORE)
    with open(plain, "rb") as h:
        off = b"".join(h.read().split(b"\n")[1:])
    assert len(off) == len(w["genome"]) and any(off[p] != w["genome"][p] for p in w["at"])
    with pytest.raises(TypeError):
        pl.run(paths["draft"], pairs, plain, mates=True, min_mapq=1)


def test_the_driver_adds_the_mates_stage_behind_everything_else(pl, tmp_path):
    """hybrid.run(polish_mates=1): every file of the pipeline has the recorded length and digest, and the new file is
    polish.run's with mates on the files the stage names; with polish=1 as well its draft is the long-read-polished file"""
    import hashlib

    import hybridcases
    from muchsalsa_amd import hybrid, mapper
    (tmp_path / "in").mkdir()
    inputs = hybridcases.write_inputs(tmp_path / "in")
    out = str(tmp_path / "out")
    res = hybrid.run(hybridcases.K_FILTER, hybridcases.K_ASSEMBLY, hybridcases.NAME, inputs[0], inputs[1], inputs[2], out, polish_mates=1)
    for rel, rec in sorted(hybridcases.expected()["files"].items()):
        with open(os.path.join(out, rel), "rb") as h:
            data = h.read()
        assert (len(data), hashlib.sha256(data).hexdigest()) == (rec["bytes"], rec["sha256"]), rel
    files = res["files"]
    assert files["polished_mates"] == os.path.join(os.path.realpath(out), hybrid.POLISHED_MATES_NAME) and "polished" not in files
    assert files["interleaved"] == os.path.join(os.path.realpath(out), hybrid.INTERLEAVED_NAME)
    again = os.path.join(str(tmp_path), "again.fq")
    assert mapper.interleave(inputs[0], inputs[1], again) == res["interleave"]["pairs"] > 0
    with open(again, "rb") as a, open(files["interleaved"], "rb") as b:
        assert a.read() == b.read()
    with open(files["polished_mates"], "rb") as h:
        polished = h.read()
    alone = os.path.join(str(tmp_path), "alone.fa")
    got = pl.run(files["assembly"], files["interleaved"], alone, mates=True, **hybrid.MATES_MAPPING)
    with open(alone, "rb") as h:
        assert h.read() == polished and len(polished) > 0
    assert got["voters"] == res["polish_mates"]["voters"] >= 1
    print("polish_mates: %r" % {k: res["polish_mates"]["rounds"][0]["map"]["mate"][k] for k in mo.STATS})
    # with the long-read polish in front, the mates stage's draft is its output
    out2 = str(tmp_path / "out2")
    res2 = hybrid.run(hybridcases.K_FILTER, hybridcases.K_ASSEMBLY, hybridcases.NAME, inputs[0], inputs[1], inputs[2], out2, polish=1,
                      polish_mates=1)
    f2 = res2["files"]
    both = os.path.join(str(tmp_path), "both.fa")
    pl.run(f2["polished"], f2["interleaved"], both, mates=True, **hybrid.MATES_MAPPING)
    with open(both, "rb") as a, open(f2["polished_mates"], "rb") as b:
        assert a.read() == b.read()
    with open(f2["assembly"], "rb") as a, open(files["assembly"], "rb") as b:
        assert a.read() == b.read()
