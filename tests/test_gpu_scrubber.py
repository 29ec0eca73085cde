"""Read scrubber on the GPU: every test runs the stage on files, compares the output byte for byte with the plain-Python
restatement's text (tests/scrub_oracle.py) and, where a fixture of the reference script exists (tests/golden/scrubber), as a
record set with it.  Every test runs under its own time limit: a watchdog ends the process when a stage call does not come
back."""
import faulthandler
import hashlib
import json
import os
import subprocess
import sys

import numpy as np
import pytest

import scrub_oracle

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = os.path.join(ROOT, "tests", "golden", "scrubber")
LIMIT = 600  # seconds per test


@pytest.fixture(scope="module")
def sc():
    import __graft_entry__ as g
    g.build()
    from muchsalsa_amd import scrubber
    return scrubber


@pytest.fixture(autouse=True)
def time_limit(sc):  # (after sc: the build is not the test's time)
    faulthandler.dump_traceback_later(LIMIT, exit=True)  # works while the main thread sits in a native call
    yield
    faulthandler.cancel_dump_traceback_later()


def _read(name):
    with open(os.path.join(GOLD, name), "rb") as f:
        return f.read()


def _sorted(text):
    recs = scrub_oracle.records(text)
    return b"".join(b">" + h + b"\n" + recs[h] for h in sorted(recs)), len(recs)


def _stage(sc, d, anchors, ava, reads_file, subset_size, tag="x", ext=".fa"):
    pa, pv, pr = os.path.join(d, tag + ".anchors.paf"), os.path.join(d, tag + ".ava.paf"), os.path.join(d, tag + ".reads" + ext)
    out = os.path.join(d, tag + ".out.fa")
    for p, data in ((pa, anchors), (pv, ava), (pr, reads_file)):
        with open(p, "wb") as h:
            h.write(data)
    graph = {}
    res = sc.run(pa, pr, out, pv, subset_size=subset_size, device=0, graph=graph)
    with open(out, "rb") as h:
        return h.read(), res, graph


def _check(sc, tmp_path, anchors, ava, reads_file, subset_size=scrub_oracle.SUBSET_SIZE, reads=None, tag="x", ext=".fa"):
    """the stage against the restatement: the read graph row by row, the counts, the text byte for byte"""
    reads = scrub_oracle.parse_fasta(reads_file) if reads is None else reads
    batches, st = scrub_oracle.scrub(anchors, ava, reads, subset_size)
    want = scrub_oracle.text(batches)
    got, res, graph = _stage(sc, str(tmp_path), anchors, ava, reads_file, subset_size, tag, ext)
    adj = st["graph"]["adj"]
    assert graph["row_off"].tolist() == np.concatenate(([0], np.cumsum([len(a) for a in adj]))).tolist()
    assert graph["adj"].tolist() == [w for a in adj for w in a]
    assert (res["nodes"], res["edges"], res["hits"], res["ava_lines"], res["batches"], res["records"]) == (
        st["nodes"], st["edges"], st["hits"], st["ava_lines"], st["batches"], st["records"])
    assert len(got) == len(want)
    assert got == want
    return got, res, st


@pytest.mark.parametrize("fx", ["a", "b"])
def test_fixture(sc, tmp_path, fx):
    meta = json.loads(_read(fx + ".json"))
    got, res, _ = _check(sc, tmp_path, _read(fx + ".anchors.paf"), _read(fx + ".ava.paf"), _read(fx + ".reads.fa"),
                         meta["subset_size"])
    text, n = _sorted(got)
    assert n == meta["records"] and res["batches"] == meta["batches"]
    assert text == _read(fx + ".out.sorted.fa")  # the reference script's record set


@pytest.mark.parametrize("subset_size,n_batches", [(60000, 1), (1200, 2), (300, 7)])
def test_subset_sizes(sc, tmp_path, subset_size, n_batches):
    from muchsalsa_amd import synth
    anchors, ava, fa = synth.scrubber_workload(2000, 5000, 8000, 4)
    _, res, st = _check(sc, tmp_path, anchors, ava, fa, subset_size)
    assert res["batches"] == n_batches
    if n_batches > 1:  # nodes that were in a subset, stayed, and were folded again
        assert res["subset_total"] > res["nodes"]


def _line(a, b, s, e, strand="+", alen=4000, blen=4000, sb=None, eb=None):
    sb, eb = (s if sb is None else sb), (e if eb is None else eb)
    return b"%s\t%d\t%d\t%d\t%s\t%s\t%d\t%d\t%d\t%d\t%d\t60\n" % (a, alen, s, e, strand.encode(), b, blen, sb, eb, e - s, e - s)


def _bases(n, seed):
    rng = np.random.default_rng(seed)
    return np.frombuffer(b"ACGT", np.uint8)[rng.integers(0, 4, n)].tobytes()


def test_fold_changes_in_a_later_batch(sc, tmp_path):
    """Chunks u1 = (A, B, C), u2 = (B, D), u3 = (C, E); subset size 3.  Batch 1 is {A, B, C} with the centre {A}: B and C keep
    the neighbours D and E.  Batch 2 starts at B: {B, C, D}, centre {B, D}.  The pair (B, C) has the lines (0, 1000), (2000,
    3000), (1200, 1900): the first walk gives (0, 1900) -- the second line is 1000 away when it is met -- and the second walk,
    on top of it, joins (2000, 3000).  B's first record is [200, 3000] only because its entry was folded in both batches."""
    anchors = (_line(b"u1", b"A", 0, 600, sb=300, eb=900) + _line(b"u1", b"B", 0, 600, sb=300, eb=900) +
               _line(b"u1", b"C", 0, 600, sb=3500, eb=3900) + _line(b"u2", b"B", 0, 600, sb=400, eb=800) +
               _line(b"u2", b"D", 0, 600, sb=300, eb=900) + _line(b"u3", b"C", 0, 600, sb=3400, eb=3950) +
               _line(b"u3", b"E", 0, 600, sb=300, eb=900))
    ava = _line(b"B", b"C", 0, 1000) + _line(b"C", b"B", 2000, 3000) + _line(b"B", b"C", 1200, 1900)
    fa = b"".join(b">%s\n%s\n" % (n, _bases(4000, i)) for i, n in enumerate([b"A", b"B", b"C", b"D", b"E"]))
    got, res, st = _check(sc, tmp_path, anchors, ava, fa, 3)
    assert [(s, sub, cen) for s, sub, cen in st["plan"]] == [(0, [0, 1, 2], [0]), (1, [1, 2, 3], [1, 3]), (2, [2, 4], [2, 4])]
    recs = scrub_oracle.records(got)
    assert len(recs[b"B_0"].replace(b"\n", b"")) == 2801 and b"B_1" not in recs
    assert len(recs[b"C_0"].replace(b"\n", b"")) == 2801 and len(recs[b"C_1"].replace(b"\n", b"")) == 401
    # with both reads in the centre of one batch the entry is walked once: (0, 1900)
    got1, _, _ = _check(sc, tmp_path, anchors, ava, fa, 60000, tag="one")
    assert len(scrub_oracle.records(got1)[b"B_0"].replace(b"\n", b"")) == 1701


def test_hub_with_hundreds_of_partners_and_a_node_with_none(sc, tmp_path):
    rng = np.random.default_rng(5)
    n = 300
    names = [b"hub"] + [b"p%d" % i for i in range(n)]
    anchors = b"".join(_line(b"u0", r, 0, 700, alen=900, blen=9000, sb=4000, eb=4700) for r in names)
    anchors += _line(b"u9", b"lone", 0, 700, alen=900, blen=9000, sb=100, eb=8950)  # no read-to-read line names it
    anchors += _line(b"u8", b"short", 0, 700, alen=900, blen=300, sb=0, eb=120)      # [200, 100]: a header line alone
    lines = []
    for i in range(n):
        s = int(rng.integers(0, 1500)) if i % 2 else 5800 + int(rng.integers(0, 1500))  # two bands on the hub
        e = s + int(rng.integers(500, 1200))
        strand = "+-"[i % 2]
        a, b = (b"hub", names[1 + i]) if i % 3 else (names[1 + i], b"hub")
        lines.append(_line(a, b, s, e, strand, 9000, 9000, 10, 10 + e - s))
        if i % 4 == 0:  # a second line of the pair: near, far, or on the other strand
            gap = [100, 499, 500, 900][(i // 4) % 4]
            lines.append(_line(a, b, e + gap, e + gap + 600, strand if i % 8 else "+-"[(i + 1) % 2], 9000, 9000, 20, 620))
    order = rng.permutation(len(lines))
    ava = b"".join(lines[k] for k in order)
    fa = b"".join(b">%s\n%s\n" % (r, _bases(9000, i)) for i, r in enumerate(names + [b"lone"])) + b">short\n" + _bases(300, 1) + b"\n"
    got, res, st = _check(sc, tmp_path, anchors, ava, fa)
    assert res["pairs"] == (n + 1) * n // 2 and res["batches"] == 1
    recs = scrub_oracle.records(got)
    assert sum(1 for h in recs if h.startswith(b"hub_")) >= 2
    assert len(recs[b"lone_0"].replace(b"\n", b"")) == 8601 and recs[b"short_0"] == b""
    assert b">short_0\n>" in got or got.endswith(b">short_0\n")


def test_fastq_input(sc, tmp_path):
    from muchsalsa_amd import synth
    anchors, ava, fq = synth.scrubber_workload(300, 4000, 900, 5, fastq=True)
    _, _, fa = synth.scrubber_workload(300, 4000, 900, 5)
    assert fq.startswith(b"@r0\n")
    reads = scrub_oracle.parse_fasta(fa)
    got, _, _ = _check(sc, tmp_path, anchors, ava, fq, 100, reads=reads, tag="q", ext=".fq")
    got_fa, _, _ = _check(sc, tmp_path, anchors, ava, fa, 100, tag="a", ext=".fasta")
    assert got == got_fa


def test_workload_config1(sc, tmp_path):
    from muchsalsa_amd import synth
    anchors, ava, fa = synth.scrubber_workload(10000, 5000, 50000, 1)
    _, res, _ = _check(sc, tmp_path, anchors, ava, fa)
    assert res["nodes"] == 10000 and res["pairs"] > 2_000_000 and res["batches"] == 1
    _, res, _ = _check(sc, tmp_path, anchors, ava, fa, 2500, tag="many")
    assert res["batches"] >= 4


def test_reference_digest_at_the_default_subset_size(sc, tmp_path):
    """More than 60000 nodes, so that the script's own subset size cuts the reads into batches: the record count and the
    SHA-256 of the sorted records are the reference script's (tools/make_scrubber_fixtures.py)."""
    from muchsalsa_amd import synth
    meta = json.loads(_read("big.json"))
    assert meta["subset_size"] == scrub_oracle.SUBSET_SIZE and meta["nodes"] > scrub_oracle.SUBSET_SIZE
    anchors, ava, fa = synth.scrubber_workload(**meta["shape"])
    got, res, _ = _check(sc, tmp_path, anchors, ava, fa)
    assert (res["nodes"], res["edges"], res["batches"]) == (meta["nodes"], meta["edges"], meta["batches"])
    text, n = _sorted(got)
    assert n == meta["records"]
    assert hashlib.sha256(text).hexdigest() == meta["sha256_sorted"]


def test_command_line_matches_run(sc, tmp_path):
    from muchsalsa_amd import synth
    anchors, ava, fa = synth.scrubber_workload(300, 4000, 900, 5)
    got, res, _ = _stage(sc, str(tmp_path), anchors, ava, fa, 100, tag="api")
    d = str(tmp_path)
    out = os.path.join(d, "cli.out.fa")
    env = dict(os.environ, PYTHONPATH=ROOT)
    r = subprocess.run(["timeout", "-k", "10", "300", sys.executable, "-m", "muchsalsa_amd.scrubber",
                        os.path.join(d, "api.anchors.paf"), os.path.join(d, "api.reads.fa"), out,
                        os.path.join(d, "api.ava.paf"), "--subset-size", "100"], cwd=ROOT, env=env, capture_output=True,
                       text=True)
    assert r.returncode == 0, r.stderr
    line = json.loads(r.stdout.strip().splitlines()[-1])
    assert {k: line[k] for k in res} == res and res["batches"] == 4
    assert set(line["seconds"]) >= {"parse", "graph", "batching", "fold", "union", "gather", "format", "copy", "write"}
    with open(out, "rb") as h:
        assert h.read() == got
    r = subprocess.run(["timeout", "-k", "10", "60", sys.executable, "-m", "muchsalsa_amd.scrubber", out], cwd=ROOT, env=env,
                       capture_output=True, text=True)
    assert r.returncode == 2 and "subset-size" in r.stderr


def test_missing_read_writes_nothing(sc, tmp_path):
    anchors = (_line(b"u1", b"A", 0, 600) + _line(b"u1", b"B", 0, 400) + _line(b"u1", b"B", 0, 600) +
               _line(b"u2", b"C", 0, 600))
    fa = b">A\n" + _bases(4000, 1) + b"\n>C\n" + _bases(4000, 2) + b"\n"
    pa, pv, pr, out = (tmp_path / n for n in ("m.paf", "m.ava.paf", "m.fa", "m.out.fa"))
    pa.write_bytes(anchors)
    pv.write_bytes(_line(b"A", b"C", 0, 1000))
    pr.write_bytes(fa)
    with pytest.raises(sc.ScrubberError) as ei:
        sc.run(str(pa), str(pr), str(out), str(pv))
    from muchsalsa_amd import _lib
    assert ei.value.code == _lib.E_IDS and ei.value.line == 3  # B's first surviving line
    assert not out.exists()
    with pytest.raises(scrub_oracle.OracleError) as eo:
        scrub_oracle.scrub(anchors, _line(b"A", b"C", 0, 1000), scrub_oracle.parse_fasta(fa))
    assert eo.value.line == 3


def test_empty_centre_is_an_error_in_time(sc, tmp_path):
    """An input check: the graph is built and batched, no batch can close with a centre, nothing is written."""
    import time
    from muchsalsa_amd import _lib, synth
    anchors, ava, fa = synth.scrubber_workload(300, 4000, 900, 5)
    with pytest.raises(scrub_oracle.EmptyCentre) as eo:
        scrub_oracle.scrub(anchors, ava, scrub_oracle.parse_fasta(fa), 12)
    d = str(tmp_path)
    t0 = time.perf_counter()
    with pytest.raises(sc.ScrubberError) as ei:
        _stage(sc, d, anchors, ava, fa, 12, tag="e")
    assert time.perf_counter() - t0 < 60
    assert ei.value.code == _lib.E_LAYOUT
    start = scrub_oracle.read_graph(anchors)["names"][eo.value.start]
    assert "read %s " % start in str(ei.value)
    assert not os.path.exists(os.path.join(d, "e.out.fa"))
