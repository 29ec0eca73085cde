"""The SAM stage on the device against its restatement in plain Python (tests/sam_oracle.py): every named case of
tests/samcases.py byte for byte and line for line in all four (eqx, md) combinations, every violation of S1 as its error text,
the stage behind mapper.run on a paired and on a long-read workload, and S11's batches."""
import functools
import os

import pytest

import map_oracle
import sam_oracle
import samcases

pytestmark = pytest.mark.gpu

MIN_SCORE = 40


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


def check_case(mods, stage, directory, name):
    """the case through sam.run_tables in every form, each equal to the restatement in text and line table"""
    sam = mods["sam"]
    c = samcases.case(name)
    tp, qp = samcases.write_case(c, directory)
    targets, queries, chains, ops, off, ranks, mates = samcases.tables(c)
    forms = [(eqx, md, True) for eqx in (True, False) for md in (False, True)] + [(True, True, False)]
    first = None
    for eqx, md, unmapped in forms:
        want, want_lines = sam_oracle.run(targets, queries, chains, ops, off, ranks, mates, eqx=eqx, md=md, unmapped=unmapped)
        text, lines, stats = sam.run_tables(tp, qp, chains, ops, off, ranks, mates, eqx=eqx, md=md, unmapped=unmapped, context=stage)
        form = "%s eqx=%d md=%d unmapped=%d" % (name, eqx, md, unmapped)
        if text != want:
            at = next((i for i, (a, b) in enumerate(zip(text, want)) if a != b), min(len(text), len(want)))
            raise AssertionError("%s: %d bytes against %d, the first difference at byte %d: %r against %r" %
                                 (form, len(text), len(want), at, text[max(0, at - 60):at + 40], want[max(0, at - 60):at + 40]))
        assert lines == want_lines, form
        assert stats["lines"] == len(want_lines) and stats["bytes_out"] == len(want) and stats["lost_publications"] == 0, form
        assert stats["unmapped"] == sum(1 for ln in want_lines if ln[0] is None), form
        assert stats["short"] + stats["long"] == len(want_lines), form
        assert stats["params"] == {"eqx": int(eqx), "md": int(md), "unmapped": int(unmapped)}, form
        first = first if (eqx, md, unmapped) != forms[0] else stats
    return first  # (the counts of eqx = 1, md = 0: the form whose line sizes the class boundary's case is fitted to)


@pytest.mark.parametrize("name", samcases.names())
def test_against_the_restatement(mods, stage, tmp_path, name):
    stats = check_case(mods, stage, tmp_path, name)
    if name == "long":
        assert stats["long"] == 2 and stats["short"] == 2
    if name == "boundary":
        assert stats["short"] == 2 and stats["long"] == 1  # 2047 and 2048 bytes; 2049


def check_bad(mods, stage, directory, name):
    _, c, want = next(b for b in samcases.BAD if b[0] == name)
    sam, lib = mods["sam"], mods["lib"]
    tp, qp = samcases.write_case(c, directory)
    targets, queries, chains, ops, off, ranks, mates = samcases.tables(c)
    with pytest.raises(sam_oracle.SamTableError) as told:
        sam_oracle.run(targets, queries, chains, ops, off, ranks, mates)
    assert str(told.value).startswith(want)
    out = os.path.join(str(directory), "out.sam")
    with pytest.raises(sam.SamError) as e:
        sam.run_tables(tp, qp, chains, ops, off, ranks, mates, out=out, context=stage)
    assert e.value.code == lib.E_ARG and (": " + want) in str(e.value), str(e.value)
    assert not os.path.exists(out)
    # the context goes on: a good table behind the bad one
    good = samcases.case("instance")
    gt, gq = samcases.write_case(good, directory)
    text, _, _ = sam.run_tables(gt, gq, *samcases.tables(good)[2:], context=stage)
    assert text == sam_oracle.run(*samcases.tables(good))[0]


@pytest.mark.parametrize("name", [b[0] for b in samcases.BAD])
def test_every_violation_of_s1_is_its_error_text(mods, stage, tmp_path, name):
    check_bad(mods, stage, tmp_path, name)


def test_arguments_that_the_stage_refuses(mods, stage, tmp_path):
    sam, lib = mods["sam"], mods["lib"]
    c = samcases.case("instance")
    tp, qp = samcases.write_case(c, tmp_path)
    _, _, chains, ops, off, ranks, _ = samcases.tables(c)
    for kw in (dict(ranks=[]), dict(off=off[:-1]), dict(ops=ops[:-1])):
        with pytest.raises(sam.SamError) as e:
            sam.run_tables(tp, qp, **dict(dict(chains=chains, ops=ops, off=off, ranks=ranks), **kw), context=stage)
        assert e.value.code == lib.E_ARG
    with pytest.raises(sam.SamError) as e:
        sam.run_tables(os.path.join(str(tmp_path), "missing.fa"), qp, chains, ops, off, ranks, context=stage)
    assert "targets" in str(e.value)


# ---- end to end: mapper.run(..., sam=...)

@functools.lru_cache(maxsize=None)
def paired_workload():
    from muchsalsa_amd import synth
    return synth.mates_workload(genome=4000, seed=1, coverage=8, read_len=100, insert=300, repeat_len=250, error=0.06)


@functools.lru_cache(maxsize=None)
def long_workload():
    from muchsalsa_amd import synth
    return synth.mapper_workload(24, 3000, 0, 5, coverage=8, tiled=True, unitig_len=(2500, 6000), fastq=False)


def _end_to_end(mp, d, targets_path, queries_path, targets, queries, **kw):
    paf, plain, out = (os.path.join(str(d), n) for n in ("with.paf", "without.paf", "out.sam"))
    tb = {}
    res = mp.run(targets_path, queries_path, paf, tables=tb, sam=out, min_score=MIN_SCORE, **kw)
    mp.run(targets_path, queries_path, plain, cigar=1, exact=1, rank=True, min_score=MIN_SCORE,
           **{k: v for k, v in kw.items() if not k.startswith("sam_")})
    with open(paf, "rb") as a, open(plain, "rb") as b:
        assert a.read() == b.read()
    with open(out, "rb") as h:
        text = h.read()
    ops = [x for r in tb["runs"] for x in r]
    off = [0]
    for r in tb["runs"]:
        off.append(off[-1] + len(r))
    want, lines = sam_oracle.run(targets, queries, tb["chains"], ops, off, tb["ranks"], tb.get("mates"), eqx=not kw.get("sam_m", False),
                                 md=kw.get("sam_md", False))
    assert len(text) == len(want) and text == want
    assert res["sam"]["lines"] == len(lines) and res["sam"]["chains"] == len(tb["chains"]) and res["sam"]["seconds"]["format"] >= 0
    return res, tb, text


def test_the_paired_workload_through_the_mapper(mods, tmp_path):
    """--mates --extend: proper pairs, pairs with one mate mapped and pairs without a chain all occur"""
    mp = mods["mp"]
    w = paired_workload()
    names = {}
    for key, data in (("genome.fa", b">g\n" + w["genome"] + b"\n"), ("1.fq", w["illumina_1"]), ("2.fq", w["illumina_2"])):
        names[key] = os.path.join(str(tmp_path), key)
        with open(names[key], "wb") as h:
            h.write(data)
    pairs = os.path.join(str(tmp_path), "pairs.fq")
    mp.interleave(names["1.fq"], names["2.fq"], pairs)
    with open(pairs, "rb") as h:
        queries = map_oracle.parse(h.read(), True)
    res, tb, text = _end_to_end(mp, tmp_path, names["genome.fa"], pairs, [(b"g", w["genome"])], queries, mates=True, extend=20, sam_md=True)
    flags = [int(ln.split(b"\t")[1]) for ln in text.split(b"\n") if ln and not ln.startswith(b"@")]
    assert len(flags) >= len(queries) and all(f & 1 for f in flags)
    assert sum(1 for f in flags if f & 2) > 100 and any(f & 4 for f in flags) and any(f & 8 and not f & 4 for f in flags)
    assert res["sam"]["unmapped"] > 0 and res["sam"]["representative"] + res["sam"]["unmapped"] == len(queries)


def test_a_long_read_workload_through_the_mapper(mods, tmp_path):
    """long reads on tiled unitigs: lines of the long class, supplementary lines where a read spans two unitigs"""
    mp = mods["mp"]
    w = long_workload()
    tpath, qpath = os.path.join(str(tmp_path), "unitigs.fa"), os.path.join(str(tmp_path), "reads.fa")
    with open(tpath, "wb") as h:
        h.write(w["unitigs"])
    with open(qpath, "wb") as h:
        h.write(w["reads"])
    targets, queries = map_oracle.parse(w["unitigs"], False), map_oracle.parse(w["reads"], False)
    res, tb, text = _end_to_end(mp, tmp_path, tpath, qpath, targets, queries, extend=20, sam_md=True)
    assert res["sam"]["long"] > 0 and res["sam"]["supplementary"] > 0
    _end_to_end(mp, tmp_path, tpath, qpath, targets, queries, sam_m=True)


def test_an_error_of_the_sam_stage_leaves_neither_file(mods, tmp_path):
    """a target name of 255 bytes is the mapper's business nowhere and S1's host check here"""
    mp = mods["mp"]
    tpath, qpath = os.path.join(str(tmp_path), "t.fa"), os.path.join(str(tmp_path), "q.fa")
    with open(tpath, "wb") as h:
        h.write(b">" + b"n" * 255 + b"\nACGTACGTAC\n")
    with open(qpath, "wb") as h:
        h.write(b">q\nACGTACGTAC\n")
    paf, out = os.path.join(str(tmp_path), "o.paf"), os.path.join(str(tmp_path), "o.sam")
    with pytest.raises(mods["sam"].SamError) as e:
        mp.run(tpath, qpath, paf, sam=out)
    assert "target record 0: a name longer than 254 bytes" in str(e.value)
    assert not os.path.exists(paf) and not os.path.exists(out)
    mp.run(tpath, qpath, paf)  # (the mapper alone takes the file)
    assert os.path.exists(paf)


def test_a_duplicate_target_name_is_the_loaders_business(mods, stage, tmp_path):
    """the loader keeps the first record of a name: the stage sees one record, the header names it once, and a chain that
    points at the dropped record is S1's error"""
    sam, lib = mods["sam"], mods["lib"]
    c = samcases.case("instance")
    doubled = dict(c, targets=c["targets"] + [(b"t", b"GGGGCCCCAAAATTTT")])
    tp, qp = samcases.write_case(doubled, tmp_path)
    text, lines, _ = sam.run_tables(tp, qp, *samcases.tables(c)[2:], context=stage)
    assert (text, lines) == sam_oracle.run(*samcases.tables(c)) and text.count(b"@SQ") == 1
    chains = [c["chains"][0][:1] + (1,) + c["chains"][0][2:]]
    with pytest.raises(sam.SamError) as e:
        sam.run_tables(tp, qp, chains, *samcases.tables(c)[3:], context=stage)
    assert e.value.code == lib.E_ARG and "chain 0: target record" in str(e.value)


# ---- S11: batches

def _units_case():
    """six equal pairs: every unit has the same lines and the same text bound"""
    import random
    rng = random.Random(21)
    c = samcases.Case("units", paired=True)
    t = c.target(b"t", samcases.rand_seq(rng, 400))
    for p in range(6):
        _, a = c.read(b"u%d/1" % p, t, 10 + p, "30=1X19=", rng)
        _, b = c.read(b"u%d/2" % p, t, 150 + p, "50=", rng, strand=1)
        c.pair(a, b)
    return c.done()


def test_batches(mods, stage, tmp_path):
    """the same text under budgets that give 1, 3 and 6 batches; a pair is never split; an over-budget unit is named"""
    sam, lib = mods["sam"], mods["lib"]
    c = _units_case()
    tp, qp = samcases.write_case(c, tmp_path)
    tabs = samcases.tables(c)[2:]
    want, want_lines = sam_oracle.run(*samcases.tables(c), md=True)
    text, lines, stats = sam.run_tables(tp, qp, *tabs, md=True, context=stage)
    assert text == want and lines == want_lines and len(stats["batches"]) == 1
    b = stats["batches"][0]
    assert b["n_lines"] == 12 and b["bytes_bound"] == sam.batch_bytes(12, b["text_bound"]) and b["text_bytes"] <= b["text_bound"]
    runs = [samcases.tables(c)[4][i + 1] - samcases.tables(c)[4][i] for i in range(12)]
    assert b["text_bound"] == sum(sam_oracle.line_bound(ch, runs[i], 50, True) for i, ch in enumerate(c["chains"]))
    unit = b["text_bound"] // 6
    for n_units, n_batches in ((6, 1), (2, 3), (1, 6)):
        budget = sam.batch_bytes(2 * n_units, unit * n_units)
        text, lines, stats = sam.run_tables(tp, qp, *tabs, md=True, budget_bytes=budget, context=stage)
        assert text == want and lines == want_lines, n_batches
        got = stats["batches"]
        assert len(got) == n_batches and stats["budget_bytes"] == budget
        assert all(x["first_query"] % 2 == 0 and x["n_queries"] == 2 * n_units and x["bytes_bound"] <= budget and x["bytes_peak"] <= x["bytes_bound"]
                   for x in got)
        assert sum(x["text_bytes"] for x in got) + stats["header_bytes"] == len(want)
    with pytest.raises(sam.SamError) as e:
        sam.run_tables(tp, qp, *tabs, md=True, budget_bytes=sam.batch_bytes(2, unit) - 1, context=stage)
    assert e.value.code == lib.E_NOMEM and "pair 0 (query records 0 and 1)" in str(e.value)
    # single-end: the unit is the record
    single = tabs[:4] + (None,)
    want1, lines1 = sam_oracle.run(*samcases.tables(c)[:6], None)
    text, lines, stats = sam.run_tables(tp, qp, *single, budget_bytes=sam.batch_bytes(1, sam_oracle.line_bound(c["chains"][0], 3, 50, False)), context=stage)
    assert text == want1 and lines == lines1 and len(stats["batches"]) == 12
    with pytest.raises(sam.SamError) as e:
        sam.run_tables(tp, qp, *single, budget_bytes=1000, context=stage)
    assert e.value.code == lib.E_NOMEM and "query record 0" in str(e.value)
