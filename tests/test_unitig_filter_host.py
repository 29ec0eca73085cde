"""Unitig coverage filter, host side (no GPU): the numpy restatement against hand-derived fixtures, msgpu_uf_parse against
a Python split, its rejections with their line numbers, and msgpu_uf_quartiles against numpy.percentile.

Fixture a (tests/golden/unitig_filter/a.*): blocks N1, N2, R, N3, N4, N5, N1 (7 blocks, 6 ids).
  N1, first block: 9 reads on [0, 10) -> 9; N1 again as the LAST block: 1 read -> 1, and the last block wins: N1 = 1.
  N2 = 1 (one read), N3 = 1 (one read; its FASTA record is empty), N4 = 2 (two reads on [0, 10)).
  N5: reads rA, rA, rB, rC on [0, 50): pass 1 counts rA once -> 3 (4 without the de-duplication).
  R (qlen 4000, 2800 bases): r1..r6 on [0, 100) -> 6; r1, r2, r3 again on [100, 601) add nothing in pass 1.
  values {1, 1, 1, 2, 3, 6}: q1 = index 1.25 -> 1.0; q3 = index 3.75 -> 3 - (3 - 2) * 0.25 = 2.75 (numpy's t >= 0.5
  branch); upper = 2.75 + 1.5 * 1.75 = 5.375.  R = 6 > 5.375 is the only outlier; N1 (9 in its first block) is not.
  Pass 2 on R with ALL lines, cov <= 2.75:
    [0, 100) 6, [100, 601) 3 (the repeated reads count now): out
    [601, 1100) 0: 499 positions, dropped; [1100, 1110) 3: out
    [1110, 1610) 0 and 2 on [1200, 1300) (2 <= 2.75): 500 positions -> R_0 500 1110 1609
    [1610, 1620) 3; [1620, 2121): 501 -> R_1 501 1620 2120; [2121, 2130) 3
    [2130, 2700): 570 -> R_2; [2700, 2710) 3; [2710, 3300): 590 -> R_3, only 90 bases left in the sequence
    [3300, 3310) 3; [3310, 4000): 690 -> R_4 at the profile's end, past the sequence's end: header line only.
  Normal blocks write the whole record with the description line (trailing whitespace stripped): N1 twice, N3 as a
  header line only; Z is named by no line and is not written.
  report: upper 5.375, Q3 2.75, 7 blocks, 1 outlier, 1 rescued.
Fixture b: M1 = 1, M2 = M3 = M4 = 2, R2 = 9 (nine reads on [0, 100)) -> q1 = q3 = 2.0, upper = 2.0.  R2's reads t1, t2
  on [300, 900) give cov 2 == q3, which is kept: one run [100, 1200) -> R2_0 1100 100 1199 (without the equality the
  runs [100, 300) and [900, 1200) would both be too short).
"""
import os

import numpy as np
import pytest

import uf_oracle

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = os.path.join(ROOT, "tests", "golden", "unitig_filter")


@pytest.fixture(scope="module")
def uf():
    import __graft_entry__ as g
    g.build()
    from muchsalsa_amd import unitig_filter
    return unitig_filter


def _read(name, mode="rb"):
    with open(os.path.join(GOLD, name), mode) as f:
        return f.read()


@pytest.mark.parametrize("fx", ["a", "b"])
def test_oracle_matches_hand_derived_fixture(fx):
    out, rep = uf_oracle.run(_read(fx + ".paf"), _read(fx + ".fa"))
    assert out == _read(fx + ".out.fa")
    assert uf_oracle.report_lines(rep) == _read(fx + ".report.txt", "r")


def test_fixture_rules_are_the_ones_claimed():
    """the fixture exercises what its derivation says: the rules changed one at a time change the result"""
    paf, fa = _read("a.paf"), _read("a.fa")
    out, rep = uf_oracle.run(paf, fa)
    assert rep["q3"] == 2.75 and rep["upper"] == 5.375
    assert b">R_0 500 1110 1609\n" in out and b">R_1 501 1620 2120\n" in out and b"601" not in out
    assert out.count(b">N1 first unitig\n") == 2 and b">N3 empty\n>N4" in out and b">R_4 690 3310 3999\n>N3" in out
    assert b">Z" not in out
    # without the last block of N1 its first block (value 9) decides: q3 moves and nothing is an outlier
    head = paf.rsplit(b"\n", 2)[0] + b"\n"
    _, rep2 = uf_oracle.run(head, fa)
    assert rep2["blocks"] == 6 and rep2["outliers"] == 0


def test_parse_matches_python_split(uf, tmp_path):
    from muchsalsa_amd import synth
    paf, _ = synth.unitig_filter_workload(300, 4000, 800, 5, n_repeats=3, repeat_hits=(100, 400), n_long=1,
                                          long_len=30000, long_hits=2000, n_dup=50, n_again=20)
    p = tmp_path / "u.paf"
    p.write_bytes(paf)
    for threads in ("1", "3", "7"):
        os.environ["MSGPU_PARSE_THREADS"] = threads
        try:
            with uf.UfPaf(str(p)) as h:
                t = h.tables()
        finally:
            del os.environ["MSGPU_PARSE_THREADS"]
        rows = [ln.split("\t") for ln in paf.decode().splitlines()]
        assert len(t["line_qs"]) == len(rows)
        assert t["line_qs"].tolist() == [int(r[2]) for r in rows]
        assert t["line_qe"].tolist() == [int(r[3]) for r in rows]
        assert [t["reads"][i] for i in t["line_read"]] == [r[5] for r in rows]
        seen = {}
        for r in rows:
            seen.setdefault(r[5], len(seen))
        assert t["reads"] == list(seen)  # first-seen ids
        starts = [0] + [i for i in range(1, len(rows)) if rows[i][0] != rows[i - 1][0]]
        assert t["block_first"].tolist() == starts
        assert t["block_n"].tolist() == np.diff(starts + [len(rows)]).tolist()
        assert [t["unitigs"][u] for u in t["block_unitig"]] == [rows[s][0] for s in starts]
        assert t["block_qlen"].tolist() == [int(rows[s][1]) for s in starts]
        assert t["line_block"].tolist() == np.repeat(np.arange(len(starts)), t["block_n"]).tolist()
        last = {}
        for b, s in enumerate(starts):
            last[rows[s][0]] = b
        assert t["unitig_last_block"].tolist() == [last[n] for n in t["unitigs"]]
        assert len(t["unitigs"]) < len(starts)  # ids came back as later blocks


GOOD = "u1\t100\t0\t50\t+\tr1\t7\n"


@pytest.mark.parametrize("text,line", [
    ("", 1),
    (GOOD + "\n" + GOOD, 2),                                   # a blank line
    (GOOD + "   \t \n", 2),                                    # only whitespace: blank once stripped
    (GOOD + "u1\t100\t0\t50\t+\tr1\n", 2),                    # 6 fields
    (GOOD + "u1\t100\t0\t50\t+\tr1\t\t\n", 2),                # trailing tabs are stripped: 6 fields
    (GOOD + GOOD + "u1\tx\t0\t50\t+\tr1\t7\n", 3),            # non-numeric qlen
    (GOOD + "u1\t100\t-1\t50\t+\tr1\t7\n", 2),                # negative qstart
    (GOOD + "u1\t100\t0\t-5\t+\tr1\t7\n", 2),                 # negative qend
    (GOOD + "u1\t100\t0\t5x\t+\tr1\t7\n", 2),
    (GOOD + "u1\t100\t0\t50\t+\tr1\tseven\n", 2),             # column 6 must be an integer
    (GOOD + "u1\t100\t0\t101\t+\tr1\t7\n", 2),                # qend > qlen
    (GOOD + "u1\t200\t0\t150\t+\tr1\t7\n", 2),                # qend > the qlen of the block's FIRST line
    (GOOD + "\t100\t0\t50\t+\tr1\t7\n", 2),                   # empty unitig id
])
def test_parse_rejects_with_line_number(uf, tmp_path, text, line):
    p = tmp_path / "bad.paf"
    p.write_text(text)
    with pytest.raises(uf.UnitigFilterError) as ei:
        uf.UfPaf(str(p))
    assert ei.value.line == line
    with pytest.raises(uf_oracle.OracleError) as eo:
        uf_oracle.run(text.encode(), b">u1\nACGT\n")
    assert eo.value.line == line


def test_parse_accepts_what_the_rules_allow(uf, tmp_path):
    p = tmp_path / "ok.paf"
    # no trailing newline, CRLF, negative column 6, qstart >= qend (an empty interval), a later block with another qlen
    p.write_bytes(b"u1\t100\t0\t100\t+\tr1\t-7\r\nu1\t90\t60\t40\t+\tr2\t0\nu2\t5\t0\t5\t-\tr1\t1\tx\ty\nu1\t300\t0\t250\t+\tr3\t2")
    with uf.UfPaf(str(p)) as h:
        t = h.tables()
    assert t["block_qlen"].tolist() == [100, 5, 300] and t["block_n"].tolist() == [2, 1, 1]
    assert t["unitig_last_block"].tolist() == [2, 1]


def test_quartiles_bit_identical_to_numpy(uf):
    rng = np.random.default_rng(7)
    cases = [np.array([v]) for v in (0, 1, 5, 4294967295)]
    cases += [np.array([3, 9]), np.array([9, 3]), np.array([1, 2, 3]), np.array([7] * 50), np.array([0] * 1000)]
    for k in range(1000):
        n = int(rng.integers(1, 400)) if k % 3 else int(rng.integers(1, 8))
        hi = [2, 5, 100, 10**6, 2**32 - 1][k % 5]
        v = rng.integers(0, hi, size=n, endpoint=(hi < 2**32 - 1))
        if k % 7 == 0:
            v[: n // 2] = v[0]  # large ties
        cases.append(v)
    for v in cases:
        q1, q3, up = uf.quartiles(v)
        w1 = np.percentile(v.astype(np.int64), 25)
        w3 = np.percentile(v.astype(np.int64), 75)
        wu = w3 + 1.5 * (w3 - w1)
        assert (q1, q3, up) == (float(w1), float(w3), float(wu)), v
        assert np.float64(q1).tobytes() == np.float64(w1).tobytes() and np.float64(up).tobytes() == np.float64(wu).tobytes()


def test_report_text_format(uf):
    assert uf.report_text(5.375, 2.75, 7, 1, 1) == _read("a.report.txt", "r")
    assert uf.report_text(2.0, 2.0, 5, 1, 1) == _read("b.report.txt", "r")
    assert uf.report_text(1e16, 0.1 + 0.2, 3, 0, 0).splitlines()[1:3] == ["upper_outlier: 1e+16", "Q3: 0.30000000000000004"]
