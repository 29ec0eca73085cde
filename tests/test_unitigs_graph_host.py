"""The unitig graph of the short-read unitig assembly (rule 10), host side (no GPU): the plain-Python restatement
(tests/ug_graph_oracle.py) on every unitig case of tests/kmeredgecases.py -- the GFA text judged from the text alone
(a second statement, independent of how the links were found), completeness against the cleaned graph's edges, the
conditions the GPU tests rely on, three texts written out by hand -- and the C-ABI, the signatures, the command line's
argument check, hybrid.output_names and the rule's sentences in the header, the docstring and DESIGN.md.

Rule 10 (c) at a unitig that is one self-complementary k-mer: such a unitig has no "-", so an adjacency at one has no mirror
and is written as it is, the adjacency the other way as well.  That is what the figures below ask for (hairpin-64: 2 such
links of 2 adjacencies; dense-6-100-0: 508 of them, 8,446 links of 16,384 adjacencies), and what a reader of GFA needs: from
"L x + i +" it derives i- -> x-, never i+ -> x-."""
import hashlib
import inspect
import os
import re
import subprocess
import sys

import pytest

import kmeredgecases as ec
import ug_graph_oracle as go
import ug_oracle

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
UG_CASES = ec.names("ug")
_COMP = bytes.maketrans(b"ACGT", b"TGCA")


@pytest.fixture(scope="module")
def ug():
    import __graft_entry__ as g
    g.build()
    from muchsalsa_amd import unitigs
    return unitigs


_GRAPHS = {}


def graph(name):
    if name not in _GRAPHS:
        _GRAPHS[name] = go.graph(ec.expected(name))
    return _GRAPHS[name]


def parse_gfa(text):
    """-> (segments [(id, sequence, LN, KC)], links [(from, from_rev, to, to_rev, overlap)]), every byte accounted for"""
    lines = text.split(b"\n")
    assert lines[0] == b"H\tVN:Z:1.0" and lines[-1] == b""
    segs, links = [], []
    for line in lines[1:-1]:
        f = line.split(b"\t")
        if f[0] == b"S":
            assert not links, "an S line behind an L line"
            m = re.fullmatch(rb"S\t(0|[1-9][0-9]*)\t([ACGT]+)\tLN:i:([1-9][0-9]*)\tKC:i:([1-9][0-9]*)", line)
            assert m, line
            segs.append((int(m.group(1)), m.group(2), int(m.group(3)), int(m.group(4))))
        else:
            m = re.fullmatch(rb"L\t(0|[1-9][0-9]*)\t([+-])\t(0|[1-9][0-9]*)\t([+-])\t(0|[1-9][0-9]*)M", line)
            assert m, line
            links.append((int(m.group(1)), int(m.group(2) == b"-"), int(m.group(3)), int(m.group(4) == b"-"), int(m.group(5))))
    return segs, links


def _plus_only(seq, k):
    return len(seq) == k and seq == seq[::-1].translate(_COMP)


def _mirror(link, seqs, k):
    """the mirror of a link as rule 10 (c) states it, from the sequences alone"""
    f, fr, t, tr = link
    if _plus_only(seqs[f], k) or _plus_only(seqs[t], k):
        return link
    return (t, 1 - tr, f, 1 - fr)


@pytest.mark.parametrize("name", UG_CASES)
def test_the_text_is_well_formed(name):
    r, k = ec.expected(name), ec.expected(name)["k"]
    segs, links = parse_gfa(graph(name)["gfa"])
    recs = r["all"].split(b"\n")
    assert len(segs) == len(r["unitigs"]) == (len(recs) - 1) // 2
    for i, (sid, seq, ln, kc) in enumerate(segs):  # every S line is the FASTA record of its id
        assert sid == i and recs[2 * i] == b">%d %d %d" % (i, ln, kc) and recs[2 * i + 1] == seq and len(seq) == ln
    seqs = [s[1] for s in segs]

    def strand(i, rev):
        assert not (rev and _plus_only(seqs[i], k)), "a - of a unitig that exists as + only"
        return seqs[i][::-1].translate(_COMP) if rev else seqs[i]

    tuples = [l[:4] for l in links]
    assert tuples == sorted(tuples) and len(set(tuples)) == len(tuples)  # strictly ascending
    have = set(tuples)
    for f, fr, t, tr, overlap in links:
        assert overlap == k - 1
        assert strand(f, fr)[len(seqs[f]) - (k - 1):] == strand(t, tr)[:k - 1]
        m = _mirror((f, fr, t, tr), seqs, k)
        assert m == (f, fr, t, tr) or m not in have, "a link and its mirror are both written"
        assert (f, fr, t, tr) <= m
    assert tuples == graph(name)["links"]


@pytest.mark.parametrize("name", UG_CASES)
def test_the_links_cover_the_edges_that_were_not_joined(name):
    r, k = ec.expected(name), ec.expected(name)["k"]
    g = ug_oracle.Graph(r["counts"], k)
    units = go.oriented(r)
    open_edges = set()
    for s in g.nodes():
        joined = ug_oracle.joined_next(g, s)[0]
        open_edges.update((s, t) for t in g.succ(s) if t != joined)
    closing = {(c[-1], c[0]) for c, t in zip(r["chains"], r["unitigs"]) if t[4]}
    closing |= {(ug_oracle.rc(b, k), ug_oracle.rc(a, k)) for a, b in closing}
    covered = {}
    for link in graph(name)["links"]:
        x, y = (link[0], link[1]), (link[2], link[3])
        for a, b in {(x, y), go.mirror(units, (x, y))}:
            e = (units[a][-1], units[b][0])
            covered[e] = covered.get(e, 0) + 1
    assert all(n == 1 for n in covered.values())
    assert open_edges <= set(covered) and set(covered) - open_edges <= closing
    gr = graph(name)
    assert gr["adjacencies"] == 2 * len(gr["links"]) - gr["self_mirror"] == len(covered)
    assert gr["dead_ends"] == sum(1 for c in units.values() if not g.succ(c[-1]))


def _figures(name):
    """-> (unitigs, adjacencies, links, self-mirrored, links at a + only unitig, self-loops i+ -> i+ of linear unitigs, the
    orientation pairs, the largest out-degree of an end)"""
    r, gr = ec.expected(name), graph(name)
    units = go.oriented(r)
    alone = sum(1 for l in gr["links"] if (l[0], 1) not in units or (l[2], 1) not in units)
    loops = sum(1 for l in gr["links"] if l[0] == l[2] and l[1] == l[3] == 0 and not r["unitigs"][l[0]][4])
    out = {}
    for x, _ in go.adjacencies(r)[0]:
        out[x] = out.get(x, 0) + 1
    return (len(r["unitigs"]), gr["adjacencies"], len(gr["links"]), gr["self_mirror"], alone, loops,
            {(l[1], l[3]) for l in gr["links"]}, max(out.values(), default=0))


def test_the_cases_meet_their_conditions():
    every = {(0, 0), (0, 1), (1, 0), (1, 1)}
    dense = [n for n in UG_CASES if n.startswith("dense-")]
    assert any(_figures(n)[6] == every for n in dense) and _figures("selfcomp-4")[6] == every
    for n in dense:  # an end of out-degree 4: dense-2-60-* upwards
        k, d = int(n.split("-")[1]), int(n.split("-")[2])
        if d >= 60:
            assert _figures(n)[7] == 4, n
    assert _figures("hairpin-33")[3:5] == (1, 0) and _figures("hairpin-63")[3:5] == (1, 0)
    assert _figures("dense-5-100-0")[3:5] == (64, 0)
    assert _figures("high-32-ug")[5] == 2
    for k in ec.RINGS_K:
        r, gr = ec.expected("rings-%d" % k), graph("rings-%d" % k)
        cyclic = [i for i, t in enumerate(r["unitigs"]) if t[4]]
        assert len(cyclic) == 12 and gr["links"] == [(i, 0, i, 0) for i in cyclic]
    assert [_figures(n)[4] for n in ("hairpin-64", "selfcomp-32", "selfcomp-64")] == [2, 2, 2]
    assert _figures("dense-6-100-0")[:5] == (2080, 16384, 8446, 508, 508)
    none = [n for n in UG_CASES if n.startswith("wave-") or (n.startswith("tile-") and n.endswith("n-ug"))]
    assert len(none) >= 10 and all(_figures(n)[1:3] == (0, 0) for n in none)
    ids = {len(str(l[0])) for l in graph("dense-6-100-0")["links"]}
    assert ids == {1, 2, 3, 4} and len(graph("dense-6-100-0")["links"]) > 256 * 8
    for n in ("ladder-33-33", "ladder-64-64", "selfcomp-64"):  # 128-bit keys with forks
        assert ec.expected(n)["k"] > 32 and _figures(n)[2] >= 2, n


HAIRPIN_33 = (b"H\tVN:Z:1.0\n"
              b"S\t0\tCGACAACGGCACCTCGTTGGCTATAGTACCGCCTTACGTATCTCTTCGTTTGGCTCCCTGCTCCCTCGGCTGACTAACAGAATTGATATTGTACCTAGGTACCTAGG"
              b"TACAATATC\tLN:i:116\tKC:i:168\n"
              b"L\t0\t+\t0\t-\t32M\n")
LADDER_21_1 = (b"H\tVN:Z:1.0\n"
               b"S\t0\tAACAGACACCAGTTGAGCCCGAA\tLN:i:23\tKC:i:3\n"
               b"S\t1\tACTGTCTTGACGTTGGCGAGCTGCTGAGCCGTGAACCTTGAAACGGTGCTTGTTATTCTAAATACAGACACTCAGGGTGTCGTGGACACCGTGCCAAATCTTAACCC"
               b"AAGCACCAACCGGGGTCCGTTGTAAGTCAGATACCAG\tLN:i:144\tKC:i:128\n"
               b"S\t2\tACTGTCTTGACGTTGGCGAGTG\tLN:i:22\tKC:i:2\n"
               b"S\t3\tAGACACCAGTTGAGCCCGAACGCGCCGAGAGTAACGAGTTTACTTACGCTGGACAAAGGCCCATGTTCTTATTAAAGAGTGAT\tLN:i:83\tKC:i:67\n"
               b"S\t4\tCTCGCCAACGTCAAGACAGTGGCATTCCGTAGCTCCTAATACTGTAAACGTAAACGTCCCAAAGACACCAGTTGAGCCCGAA\tLN:i:82\tKC:i:66\n"
               b"L\t0\t+\t3\t+\t20M\n"
               b"L\t1\t-\t4\t+\t20M\n"
               b"L\t2\t-\t4\t+\t20M\n"
               b"L\t3\t-\t4\t-\t20M\n")
# rings-15: the circles of 1000 and of 5000 + 14 bases are pinned by their first bases, their length and their digest
RINGS_15 = [
    (b"AAAAAAAATAGCCTTCTGAG", 1014, 2000, "seq0"),
    (b"AAAAACCTCCCGAGCTTCACTCGCACAGCAATCTGGAAGTGGAGACACAGTAAATGGGTCCTACCGCTCGGCGTTGACAACGGTAAAGCACGCACGATCGTGTGAATGCGCGGTAGCGGGT"
     b"GGTCACTCAAAAACCTCCCGAG", 143, 258, None),
    (b"AAAATATGTATGACAGTGCGATGCCTATGATCCCCCGCAATGGGGCACTTACTGTCTCTACCATTAAAATATGTATGAC", 79, 130, None),
    (b"AAACAATTCTAACTTGATAAATATAATCATGACTTGCTCCCATTTAGAGGGCATCTCCGATATTACTATAAATTGTCGGTTGTTGCTTTGCAGCACCGCCCAGCGCCTAGCTGGCCCTCCGA"
     b"GGGACGAAACAATTCTAACT", 142, 256, None),
    (b"AAACACGTCACCTGGCGGTCGGTCTCCGCGAGTAAGAAACCCAGGGACGGGTAGTTAGGCGTAGGCTCGTTCAGTATGATCAGGTACTCCACTATGCATCAGATAGAAGGCAAGATAACTAC"
     b"GACGGCCAGACGAGGTGTAAGTACTTTACCAATTCCCGGAACCCTCGTGTCCATCGGTGAATCATTGTCCCCGACAGGGGAGGCGGCATTACAACGGCCGAAGGTGGCATGGAGGGCTATGC"
     b"CGGGCTGTGCCCTAAACACGTCACCTG", 271, 514, None),
    (b"AAACCAATGCTAACGTTGGATGTCCGCTAACAAGTAAACTGCTTTGCACCTAGCGCGCCTTCACAAACCAATGCTAAC", 78, 128, None),
    (b"AAACGGGCGCAGCACCGTTGAGAGAACAGGCATGCCCTTTCGTAAGACACGCCTACGTTAGTGAAACGGGCGCAGCA", 77, 126, None),
    (b"AAACGTACTGACTCTAGTCGCGCAATAGCCGGCATCACTGGTTCGTAGGTGCCTCTCCGACTAACCCTTTGAGCCCGTTGTAGATCCCTTATTAAGCGGAGTACTTCCACTCGTGAACTAAG"
     b"ACCTGATGTCAGGTGACCGTTAATCTGAAGCTCTAGCTTATTTGGTGCCCGCCTACTGACGAATATGTCCTAGACGTACGCTATGACGCCAACGATAGTGATATAACAAGGGCGATGTCTCA"
     b"GGATATCTTCCAAACGTACTGACTC", 269, 510, None),
    (b"AAATAGTATCATGAGTCAGGCTACCGATGTCAGTCCGGACGGGCAACTGCTGGCACGCTTCAGGCTACGTGATGCAGTACAATTCCGACCTAACCCGTTACCAGGAGATATAGGACTGCAGA"
     b"ATTGCAAATAGTATCATGA", 141, 254, None),
    (b"AGAGAGAGAGAGAGAG", 16, 4, None),
    (b"ATGCCATGCCATGCCATGC", 19, 10, None),
    (b"CCGCCGCCGCCGCCGCC", 17, 6, None),
    (b"GGTAGTAACGTGACCCGAGG", 5014, 5000, "seq12"),
]
RINGS_15_SHA256 = {"seq0": "92bc13106b0a882f0fd70b5eb3049bee7db20e8e77f0b970bd804c9680426f27",
                   "seq12": "bfefa4e00e19ea479c581d0b403ff320e174106473f11b2a0ab6f9b138f5a4ec"}


def test_three_texts_written_out_by_hand():
    assert graph("hairpin-33")["gfa"] == HAIRPIN_33
    assert graph("ladder-21-1")["gfa"] == LADDER_21_1
    got = graph("rings-15")["gfa"].split(b"\n")
    assert got[0] == b"H\tVN:Z:1.0" and got[-1] == b"" and len(got) == 1 + 13 + 12 + 1
    for i, (seq, length, cover, digest) in enumerate(RINGS_15):
        f = got[1 + i].split(b"\t")
        assert f[:2] == [b"S", b"%d" % i] and f[3:] == [b"LN:i:%d" % length, b"KC:i:%d" % cover] and len(f[2]) == length
        if digest is None:
            assert f[2] == seq
        else:
            assert f[2].startswith(seq) and set(f[2]) <= set(b"ACGT")
            assert hashlib.sha256(f[2]).hexdigest() == RINGS_15_SHA256[digest]
        if i < 12:  # a circle of n k-mers: n + k - 1 bases, the first k - 1 again at the end
            assert f[2][:14] == f[2][-14:]
    assert got[14:26] == [b"L\t%d\t+\t%d\t+\t14M" % (i, i) for i in range(12)]


def test_abi_exports_the_graph_symbols(ug):
    import ctypes as C
    from muchsalsa_amd import _lib, hybrid
    header = open(os.path.join(ROOT, "include", "msgpu.h")).read()
    bound = {n for n, _, _ in _lib.SYMBOLS}
    for n in ("msgpu_ug_set_graph", "msgpu_ug_result_links"):
        assert hasattr(_lib.lib(), n) and n in bound and n + "(" in header, n
    assert "#define MSGPU_UG_TEXT_GFA 2" in header and _lib.UG_TEXT_GFA == 2
    assert C.sizeof(_lib.UgLink) == 12 and C.sizeof(_lib.UgGraphStats) == 5 * 8 + 4 * 4
    for struct, fields in (("msgpu_ug_link", _lib.UgLink), ("msgpu_ug_graph_stats", _lib.UgGraphStats)):
        body = header[header.index("typedef struct " + struct):header.index("} " + struct + ";")]
        at = 0
        for name, _ in fields._fields_:  # every field, in the header's order
            m = re.compile(r"\b%s\b" % name).search(body, at)
            assert m, (struct, name)
            at = m.end()
    assert inspect.signature(ug.run).parameters["gfa"].default is None
    assert inspect.signature(hybrid.run).parameters["gfa"].default is False


def test_output_names_are_unchanged():
    from muchsalsa_amd import hybrid
    names = hybrid.output_names("asm", "/data/reads.fastq")
    assert sorted(names) == sorted(["report", "unitigs", "unitigs_cut", "link", "unitigs_paf", "corrected_paf", "scrubbed", "exact_paf",
                                    "assembly", "corrected", "ava_paf", "target", "query", "align"])
    assert hybrid.gfa_name("asm") == os.path.join("ABYSS", "asm-unitigs.gfa") and hybrid.gfa_name("asm") not in names.values()
    assert names["unitigs"] == os.path.join("ABYSS", "asm-unitigs.fa")


def test_the_statements_of_rule_10_agree(ug):
    header = " ".join(open(os.path.join(ROOT, "include", "msgpu.h")).read().replace(" *", " ").split())
    doc = " ".join(ug.__doc__.split())
    design = " ".join(open(os.path.join(ROOT, "DESIGN.md")).read().split())
    for phrase in ("A unitig that is one self-complementary k-mer exists as i+ only",
                   "For every oriented unitig x and every t in succ(last(x)) (rule 3, on the cleaned set) there is an adjacency "
                   "x -> y with first(y) = t",
                   "Such a y always exists: an edge that rule 5 did not join ends at a node without a joined predecessor",
                   "The closing join of a cycle is the adjacency i+ -> i+",
                   "x -> y and y' -> x' are one link; ' flips the orientation",
                   "with + < -, the smaller of the two is written",
                   "Equal tuples (a hairpin i+ -> i-) are written once",
                   "it is written as it is and is counted with the self-mirrored links",
                   "The links are written ascending by that tuple",
                   "All unitigs are written, with no length cut: links to short unitigs would otherwise dangle",
                   "makes the tuple fit 64 bits (31 + 1 + 31 + 1)",
                   "adjacencies = 2 links - self-mirrored links"):
        assert phrase in header and phrase in doc and phrase in design, phrase
    for text in (header, doc, design):
        assert "LN:i:<length>" in text and "KC:i:<coverage>" in text and "<k-1>M" in text and "VN:Z:1.0" in text


def test_command_line_rejects_a_bad_gfa(ug, tmp_path):
    env = dict(os.environ, PYTHONPATH=ROOT)
    p = [str(tmp_path / n) for n in ("1.fq", "2.fq", "all.fa", "cut.fa")]
    assert "[--gfa F]" in ug.__doc__.split("\n\n")[1]
    for args in (["--gfa"], ["--gfa", ""], ["--gfa", "--bubble"], ["--gfa", str(tmp_path / "g.gfa"), "--gfa", str(tmp_path / "h.gfa")]):
        out = subprocess.run([sys.executable, "-m", "muchsalsa_amd.unitigs", "31"] + p + args, cwd=ROOT, env=env,
                             capture_output=True, timeout=300)
        assert out.returncode == 2 and b"[--gfa F]" in out.stderr, args
    assert not any(os.path.exists(x) for x in p[2:] + [str(tmp_path / "g.gfa"), str(tmp_path / "h.gfa")])
