"""A1: msgpu_parse_paf (host code of libmsgpu, runs without a GPU) against the oracle's parser and hand-made cases."""
import numpy as np
import pytest

from muchsalsa_amd import overlap, synth


def _line(q="u1", qlen=1000, qs=0, qe=600, strand="+", t="r1", tlen=5000, ts=100, te=700, nm=550, extra="600\t60"):
    return "\t".join(str(x) for x in (q, qlen, qs, qe, strand, t, tlen, ts, te, nm)) + ("\t" + extra if extra else "")


SENTINEL = "u0\t1\t0\t1\t+\tr0\t1\t0\t1\t0\t1\t0"


def _write(tmp_path, lines, trailing_newline=True, name="x.paf"):
    p = tmp_path / name
    p.write_text("\n".join(lines) + ("\n" if trailing_newline else ""))
    return str(p)


def test_matches_oracle_on_synthetic_text(oracle, tmp_path):
    tab = synth.paf_table(150, 4000, 400, 21)
    path = _write(tmp_path, synth.paf_lines(tab))
    got = overlap.parse_paf(path)
    want = oracle.parse_paf(path)
    assert got.rows.tobytes() == want["rows"].tobytes()
    assert got.n_lines == want["n_lines"]
    assert got.read_names == want["read_names"] and got.anchor_names == want["anchor_names"]


def test_last_line_is_never_parsed(tmp_path):
    # BlastFileReader.cpp:76: lineIdx < getLineCount() - 1
    good = _line()
    for nl in (True, False):
        p = overlap.parse_paf(_write(tmp_path, [good, good.replace("r1", "r2")], trailing_newline=nl))
        assert p.n_lines == 2 and len(p.rows) == 1 and p.read_names == ["r1"]
    assert len(overlap.parse_paf(_write(tmp_path, [good])).rows) == 0
    assert len(overlap.parse_paf(_write(tmp_path, [], trailing_newline=False)).rows) == 0


def test_filter_and_primary_thresholds(tmp_path):
    # keep iff nmatch >= 400 and span >= 400 (:106-107); primary iff span >= 500 and nmatch >= 500 (:121-122)
    cases = [  # (qs, qe, nmatch) -> (kept, primary)
        ((0, 400, 400), (True, False)), ((0, 399, 400), (False, False)), ((0, 400, 399), (False, False)),
        ((0, 500, 500), (True, True)), ((0, 499, 500), (True, False)), ((0, 500, 499), (True, False)),
        ((10, 510, 1000), (True, True)),
    ]
    lines = [_line(q="u%d" % i, qs=c[0][0], qe=c[0][1], nm=c[0][2], t="r%d" % i) for i, c in enumerate(cases)]
    p = overlap.parse_paf(_write(tmp_path, lines + [SENTINEL]))
    kept = {int(r["line"]): bool(r["flags"] & 2) for r in p.rows}
    for i, c in enumerate(cases):
        assert (i in kept) == c[1][0], (i, c)
        if c[1][0]:
            assert kept[i] == c[1][1], (i, c)


def test_fields_ranges_direction_and_registry_order(tmp_path):
    lines = [
        _line(q="uB", qs=5, qe=905, strand="-", t="rZ", tlen=7777, ts=40, te=950, nm=800),
        _line(q="uA", qs=0, qe=300, t="rSKIP", nm=900),              # rejected: span < 400 -> registers nothing
        _line(q="uA", qs=0, qe=450, strand="+", t="rY", tlen=6000, ts=0, te=460, nm=420),
        _line(q="uB", qs=0, qe=450, strand="x", t="rZ", tlen=1, ts=3, te=9, nm=444),
        SENTINEL,
    ]
    p = overlap.parse_paf(_write(tmp_path, lines))
    assert p.read_names == ["rZ", "rY"] and p.anchor_names == ["uB", "uA"]  # first-seen, rejected rows skipped
    r0, r1, r2 = p.rows
    assert (r0["anchor_id"], r0["read_id"], r0["read_len"], r0["i_lo"], r0["i_hi"], r0["n_lo"], r0["n_hi"], r0["score"],
            r0["line"], r0["flags"]) == (0, 0, 7777, 5, 904, 40, 949, 800, 0, 2)  # '-' -> dir 0, primary
    assert (r1["anchor_id"], r1["read_id"], r1["line"], r1["flags"]) == (1, 1, 2, 1)
    assert (r2["anchor_id"], r2["read_id"], r2["line"], r2["flags"], r2["read_len"]) == (0, 0, 3, 0, 1)  # "x" != "+"


def test_errors(tmp_path):
    from muchsalsa_amd import _lib
    with pytest.raises(overlap.MsgpuError) as e:
        overlap.parse_paf(str(tmp_path / "missing.paf"))
    assert e.value.code == _lib.E_IO
    with pytest.raises(overlap.MsgpuError) as e:  # "Invalid BLAST file."
        overlap.parse_paf(_write(tmp_path, ["a\tb\tc", SENTINEL]))
    assert e.value.code == _lib.E_FORMAT
    with pytest.raises(overlap.MsgpuError) as e:  # empty line -> no tokens
        overlap.parse_paf(_write(tmp_path, ["", SENTINEL]))
    assert e.value.code == _lib.E_FORMAT
    with pytest.raises(overlap.MsgpuError) as e:  # std::stoi would throw
        overlap.parse_paf(_write(tmp_path, [_line(qs="abc"), SENTINEL]))
    assert e.value.code == _lib.E_NUMBER
    # a malformed LAST line is harmless: it is never parsed
    assert len(overlap.parse_paf(_write(tmp_path, [_line(), "garbage"])).rows) == 1


def test_crlf_and_leading_space_numbers(tmp_path):
    # std::stoi skips leading whitespace and stops at the first non-digit ('\r' stays in the last column)
    p = overlap.parse_paf(_write(tmp_path, [_line(qs=" 7", nm="550\r", extra=""), SENTINEL]))
    assert len(p.rows) == 1 and int(p.rows[0]["i_lo"]) == 7 and int(p.rows[0]["score"]) == 550


def test_register_sequences_follows_the_registry(tmp_path):
    """msgpu_paf_register_sequences = Registry::operator[] per record of a sequence file on the PAF's own registries
    (SequenceAccessor.cpp:171,215): names the PAF registered keep their id, unknown names take the next free ids in file
    order, a name that occurs twice in the file has one id; reads and unitigs are separate registries."""
    from muchsalsa_amd import overlap, sequences
    paf = tmp_path / "x.paf"
    lines = ["u1\t900\t0\t900\t+\tr7\t5000\t10\t910\t800\t900\t60", "u0\t900\t0\t900\t-\tr3\t5000\t10\t910\t800\t900\t60",
             "u1\t900\t0\t900\t+\tr3\t5000\t2000\t2900\t800\t900\t60", "last\t1\t0\t1\t+\tnever\t1\t0\t1\t0\t1\t0"]
    paf.write_text("\n".join(lines) + "\n")
    p = overlap.parse_paf(str(paf))
    assert p.read_names == ["r7", "r3"] and p.anchor_names == ["u1", "u0"] and (p.n_reads, p.n_anchors) == (2, 2)
    fa = tmp_path / "n.fa"
    fa.write_bytes(b">r3 d\nACGT\n>new1\nAC\n>r7\nGG\n>new2\nTT\n")
    f = sequences.SeqFile(str(fa))
    ids, space = p.register_sequences(0, f)
    assert list(ids) == [1, 2, 0, 3] and space == 4
    ids2, space2 = p.register_sequences(0, f)  # registering again changes nothing
    assert list(ids2) == [1, 2, 0, 3] and space2 == 4
    fu = tmp_path / "u.fa"
    fu.write_bytes(b">u0\nAC\n>u9\nGT\n>u1\nTT\n")
    idu, spu = p.register_sequences(1, sequences.SeqFile(str(fu)))
    assert list(idu) == [1, 2, 0] and spu == 3
    assert p.read_names == ["r7", "r3"]  # the view's name lists are the PAF's own registrations


@pytest.mark.parametrize("threads", [2, 3, 7, 16, 64])
def test_chunked_parse_keeps_the_registry_order(oracle, tmp_path, monkeypatch, threads):
    """The file is parsed in chunks on several threads, each with its own name lists; the Registry ids of the whole file
    (first-seen order, line by line, BlastFileReader.cpp:110-111) are worked out from those lists.  Same rows, ids and name
    tables as the one-thread parse and the oracle for any number of chunks -- with names that return in later chunks,
    rejected lines (their names register nothing), and look-ups of further names afterwards (the registry's hash index is
    built at the first look-up)."""
    from muchsalsa_amd import sequences
    rng = np.random.default_rng(threads)
    lines = []
    for i in range(3000):
        q, t = "u%d" % rng.integers(0, 400), "read_%d" % rng.integers(0, 150)
        nm = int(rng.choice([550, 20]))  # (20 < MINIMUM_MATCHES: the line is dropped before the Registry sees it)
        lines.append(_line(q=q, t=t, ts=int(rng.integers(0, 3000)), te=int(rng.integers(3000, 5000)), nm=nm))
    path = _write(tmp_path, lines + [SENTINEL])
    want = oracle.parse_paf(path)
    monkeypatch.setenv("MSGPU_PARSE_THREADS", str(threads))
    got = overlap.parse_paf(path)
    assert got.rows.tobytes() == want["rows"].tobytes() and got.n_lines == want["n_lines"]
    assert got.read_names == want["read_names"] and got.anchor_names == want["anchor_names"]
    fa = tmp_path / "n.fa"
    fa.write_bytes(b">read_3\nAC\n>brand_new\nGG\n>" + want["read_names"][-1].encode() + b"\nTT\n")
    ids, space = got.register_sequences(0, sequences.SeqFile(str(fa)))
    n = len(want["read_names"])
    assert list(ids) == [want["read_names"].index("read_3"), n, n - 1] and space == n + 1


def test_column_counts_and_trailing_tabs(oracle, tmp_path):
    """std::getline drops an empty token behind the final delimiter and keeps empty tokens in the middle; the tokeniser
    looks at the first ten columns only.  Lines of every length around the 16-byte steps of the line scanner, with and
    without columns behind the tenth, against the oracle's parser; a line with nine columns and a trailing tab is short."""
    from muchsalsa_amd import _lib
    ten = _line(extra="")                     # exactly ten columns
    assert len(overlap.parse_paf(_write(tmp_path, [ten, SENTINEL])).rows) == 1
    assert len(overlap.parse_paf(_write(tmp_path, [ten + "\t", SENTINEL])).rows) == 1          # an empty eleventh token
    assert len(overlap.parse_paf(_write(tmp_path, [ten + "\t\t\tx\t", SENTINEL])).rows) == 1   # empty tokens in the middle
    nine = "\t".join(ten.split("\t")[:9])
    for bad in (nine, nine + "\t"):
        with pytest.raises(overlap.MsgpuError) as e:
            overlap.parse_paf(_write(tmp_path, [bad, SENTINEL]))
        assert e.value.code == _lib.E_FORMAT
    lines = []
    for pad in range(0, 40):                   # names of every length: tabs and line ends at every offset of a 16-byte step
        lines.append(_line(q="u" + "x" * pad, t="r" + "y" * (pad % 7), extra="600\t60" if pad % 3 else ""))
        lines.append(_line(q="u%d" % pad, t="r" * (pad + 1), extra="z" * pad))
    path = _write(tmp_path, lines + [SENTINEL])
    got, want = overlap.parse_paf(path), oracle.parse_paf(path)
    assert got.rows.tobytes() == want["rows"].tobytes() and len(got.rows) == len(lines)
    assert got.read_names == want["read_names"] and got.anchor_names == want["anchor_names"]
    # the same without a trailing newline behind the (never parsed) last line, and with the file ending inside a 16-byte step
    path = _write(tmp_path, lines + ["x"], trailing_newline=False)
    assert overlap.parse_paf(path).rows.tobytes() == want["rows"].tobytes()


@pytest.mark.parametrize("min_matches,th_length,th_matches", [(0, 0, 0), (420, 600, 450), (500, 500, 700), (600, 2000, 500)])
def test_non_default_filter_thresholds_match_oracle(oracle, tmp_path, min_matches, th_length, th_matches):
    """min_matches (:106-107), th_length and th_matches (:121-122) are read from msgpu_params: at values other than the
    defaults the accepted rows and their primary flags equal the oracle's parse with the same params, and the
    thresholds bite (the accepted set or the primary flags differ from the default parse)."""
    tab = synth.paf_table(150, 4000, 400, 22, min_intersection=300)
    path = _write(tmp_path, synth.paf_lines(tab))
    p = overlap.default_params()
    p.min_matches, p.th_length, p.th_matches = min_matches, th_length, th_matches
    q = oracle.default_params()
    q.min_matches, q.th_length, q.th_matches = min_matches, th_length, th_matches
    got = overlap.parse_paf(path, p)
    want = oracle.parse_paf(path, q)
    assert got.rows.tobytes() == want["rows"].tobytes()
    assert got.read_names == want["read_names"] and got.anchor_names == want["anchor_names"]
    base = oracle.parse_paf(path)["rows"]
    if (min_matches, th_length, th_matches) == (0, 0, 0):
        assert len(want["rows"]) > len(base)
    assert want["rows"].tobytes() != base.tobytes()
    span = want["rows"]["i_hi"] - want["rows"]["i_lo"] + 1
    assert (span >= min_matches).all() and ((want["rows"]["flags"] & 2 != 0) <= (span >= th_length)).all()
