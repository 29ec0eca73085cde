"""The SAM stage's named cases, as tables plus sequences: the smallest shapes at which its kernels can go wrong.  A case is a
dict: ``name``, ``targets`` and ``queries`` (lists of (name, bases), bytes), ``chains``, ``ops``, ``off``, ``ranks``,
``mates`` (None: single-end) as tests/sam_oracle.py takes them, and ``acgt`` (the sequences are upper-case A, C, G, T and every
= / X letter is true on them, so the independent validator of tests/test_sam_host.py applies).  ``CASES`` are accepted by the
stage, ``BAD`` (name, case, the words its error begins with) are S1's violations.  Everything is built from fixed seeds."""
import os
import random
import re

import sam_oracle

CODE = {"I": 1, "D": 2, "=": 7, "X": 8}
COMP = bytes.maketrans(b"ACGTacgt", b"TGCAtgca")


def rand_seq(rng, n):
    return bytes(rng.choice(b"ACGT") for _ in range(n))


def revcomp(s):
    return s.translate(COMP)[::-1]


def parse_runs(spec):
    """ "3=1X1D" -> [(3, "="), (1, "X"), (1, "D")] """
    return [(int(n), op) for n, op in re.findall(r"(\d+)([=XID])", spec)]


def other(b, step=1):
    return b"ACGT"[(b"ACGT".index(bytes([b]).upper()) + step) % 4]


def aligned(tseq, t_start, spec, rng):
    """the oriented query segment that aligns to tseq from t_start by the runs of ``spec`` -> (segment, t_end)"""
    out, x = bytearray(), t_start
    for n, op in parse_runs(spec):
        if op == "=":
            out += tseq[x:x + n]
            x += n
        elif op == "X":
            out += bytes(other(b) for b in tseq[x:x + n])
            x += n
        elif op == "D":
            x += n
        else:
            out += rand_seq(rng, n)
    assert x <= len(tseq), "the runs leave the target"
    return bytes(out), x


class Case:
    def __init__(self, name, paired=False, acgt=True):
        self.name, self.paired, self.acgt = name, paired, acgt
        self.targets, self.queries, self.chains, self.runs, self.ranks, self.mates = [], [], [], [], [], []

    def target(self, name, seq):
        self.targets.append((name, seq))
        return len(self.targets) - 1

    def query(self, name, seq):
        self.queries.append((name, seq))
        return len(self.queries) - 1

    def chain(self, q, t, strand, q_start, q_end, t_start, spec, score=100, anchors=3, parent=None, sub=0, mapq=60, n_sec=0):
        """a chain of query record q (records in rising order); parent None: a primary"""
        runs = parse_runs(spec) if isinstance(spec, str) else spec
        t_end = t_start + sum(n for n, op in runs if op != "I")
        eq = sum(n for n, op in runs if op == "=")
        block = sum(n for n, _ in runs)
        i = len(self.chains)
        self.chains.append((q, t, strand, anchors, score, block - eq, q_start, q_end, t_start, t_end, eq, block))
        self.runs.append([n << 4 | CODE[op] for n, op in runs])
        self.ranks.append((i if parent is None else parent, sub, n_sec, mapq))
        self.mates.append((0xffffffff, 0, 0, 0))
        return i

    def read(self, name, t, t_start, spec, rng, lclip=0, rclip=0, strand=0, **kw):
        """a read made to align to target t by ``spec`` with clips, stored on ``strand``; its record and its one chain"""
        seg, _ = aligned(self.targets[t][1], t_start, spec, rng)
        oq = rand_seq(rng, lclip) + seg + rand_seq(rng, rclip)
        q = self.query(name, revcomp(oq) if strand else oq)
        qs, qe = (rclip, len(oq) - lclip) if strand else (lclip, len(oq) - rclip)
        return q, self.chain(q, t, strand, qs, qe, t_start, spec, **kw)

    def pair(self, a, b, n_best=1):
        """chains a and b are each other's selected mates (rule 13's row)"""
        ca, cb = self.chains[a], self.chains[b]
        f, r = (ca, cb) if ca[2] == 0 else (cb, ca)
        tl = r[9] - f[8]
        self.mates[a], self.mates[b] = (b, tl, 1, n_best), (a, tl, 1, n_best)

    def done(self):
        off = [0]
        for r in self.runs:
            off.append(off[-1] + len(r))
        return dict(name=self.name, targets=self.targets, queries=self.queries, chains=self.chains, ops=[x for r in self.runs for x in r], off=off,
                    ranks=self.ranks, mates=self.mates if self.paired else None, acgt=self.acgt)


def tables(c):
    return c["targets"], c["queries"], c["chains"], c["ops"], c["off"], c["ranks"], c["mates"]


def fasta(recs):
    return b"".join(b">%s\n%s\n" % (n, s) for n, s in recs)


def write_case(c, directory):
    tp, qp = os.path.join(str(directory), "targets.fa"), os.path.join(str(directory), "queries.fa")
    with open(tp, "wb") as f:
        f.write(fasta(c["targets"]))
    with open(qp, "wb") as f:
        f.write(fasta(c["queries"]))
    return tp, qp


# ---- the instance of the rules' text, and its twins

T20 = b"ACGTACGTACGTACGTACGT"


def instance(strand=0):
    c = Case("instance" if not strand else "instance-reverse")
    c.target(b"t", T20)
    q = b"TTCGTGGTAACG"
    c.query(b"q", revcomp(q) if strand else q)
    qs, qe = (1, 10) if strand else (2, 11)
    c.chain(0, 0, strand, qs, qe, 5, "3=1X1D2=1I2=", score=40)
    return c.done()


def _simple():
    rng = random.Random(11)
    out = []
    c = Case("no-queries")
    c.target(b"t", T20)
    out.append(c.done())
    c = Case("no-chains")
    c.target(b"t", T20)
    c.query(b"a", b"ACGT")
    c.query(b"b", b"")
    c.query(b"c", b"acgtnRyACGT")
    c.acgt = False
    out.append(c.done())
    c = Case("no-chains-paired", paired=True)
    c.target(b"t", T20)
    c.query(b"p/1", b"ACGTA")
    c.query(b"p/2", b"GGCA")
    out.append(c.done())
    # clips: none, left only, right only, on both strands (the sides swap)
    c = Case("clips")
    t = c.target(b"ref", rand_seq(rng, 300))
    for strand in (0, 1):
        for lc, rc in ((0, 0), (7, 0), (0, 12), (3, 10)):
            c.read(b"r%d_%d_%d" % (strand, lc, rc), t, 20 + 3 * lc, "30=1X9=2I10=3D8=", rng, lclip=lc, rclip=rc, strand=strand)
    out.append(c.done())
    # decimal widths: positions and run lengths either side of 10, 100, 1000
    c = Case("widths")
    t = c.target(b"wide", rand_seq(rng, 4100))
    for k, n in enumerate((9, 10, 99, 100, 999, 1000)):
        c.read(b"w%d" % n, t, n - 1, "%d=" % n, rng, strand=k & 1)
        c.read(b"v%d" % n, t, n, "%d=1X%dD%d=%dI5=" % (n, n, n, n), rng, lclip=n, rclip=n, strand=1 - (k & 1))
    out.append(c.done())
    # SEQ of 0, 1 .. 33 bytes: unmapped, forward and reverse (the 32-bit stores of SEQ begin at any alignment)
    c = Case("seq-lengths")
    t = c.target(b"s", rand_seq(rng, 80))
    for n in range(0, 34):
        c.query(b"u%d" % n, rand_seq(rng, n))
        if n:
            c.read(b"f%d" % n, t, n, "%d=" % n, rng)
            c.read(b"r%d" % n, t, 40 - n, "%d=" % n, rng, strand=1)
            c.read(b"c%d" % n, t, 5, "%d=" % n, rng, lclip=n % 4, rclip=(n + 1) % 3, strand=n & 1)
    out.append(c.done())
    # M: = X = X collapses to one run, with I and D at the stretch's head and tail, and a chain of one run
    c = Case("m-merge")
    t = c.target(b"m", rand_seq(rng, 200))
    for k, spec in enumerate(("5=", "1X", "2=1X2=1X", "1I2=1X2=1X1D3=", "3=1D2=1X1=1X1I4=2X", "2D1X1=1X1=2I1=", "4=1I1X1D1X1I1=1X")):
        c.read(b"m%d" % k, t, 10 + k, spec, rng, lclip=k % 2, strand=k & 1)
    out.append(c.done())
    # MD: a mismatch in the first and in the last column, neighbours, a deletion next to a mismatch, an insertion in a count
    c = Case("md")
    t = c.target(b"d", rand_seq(rng, 200))
    for k, spec in enumerate(("1X5=", "5=1X", "3=2X3=", "3=1X1X3=", "3=2D1X3=", "3=1X2D3=", "3=2I4=", "1X", "2D", "1D1X1D", "12=3X10=11D1X1=1I1=",
                              "2I3=", "3=2I", "1X1I1X", "1D2I1D2=")):
        c.read(b"d%d" % k, t, 7 * k, spec, rng, strand=k & 1)
    out.append(c.done())
    # lower-case and non-ACGT bytes in target and read, both strands
    c = Case("bytes", acgt=False)
    t = c.target(b"low", b"ACGTacgtNNRYacgtACGTnnacgtACGTKMacgtTTGA")
    c.query(b"fw", b"acgTNnRyGATtaca")
    c.chain(0, t, 0, 2, 13, 4, "3=2X1D3=1I2X", score=30)
    c.query(b"rv", b"acgTNnRyGATtacaXx")
    c.chain(1, t, 1, 1, 15, 20, "4X2D5=1I4X", score=30)
    c.query(b"un", b"xXacgtNRYKMacgu")
    out.append(c.done())
    # names of 1 and of 254 bytes; "/1" is a name, not a suffix
    c = Case("names", paired=True)
    t0 = c.target(b"x", rand_seq(rng, 60))
    t1 = c.target(b"L" * 254, rand_seq(rng, 70))
    _, a = c.read(b"/1", t0, 3, "20=", rng)
    _, b = c.read(b"/2", t1, 30, "20=", rng, strand=1)
    _, a2 = c.read(b"Q" * 252 + b"/1", t1, 2, "30=", rng)
    _, b2 = c.read(b"Q" * 252 + b"/2", t1, 35, "30=", rng, strand=1)
    c.pair(a2, b2)
    c.read(b"z/3", t0, 1, "9=", rng)
    c.read(b"y", t0, 9, "9=", rng)
    out.append(c.done())
    # a record with more than 64 chains; two non-overlapping primaries; a score tie for the representative
    c = Case("roles")
    t = c.target(b"rep", rand_seq(rng, 60) * 80)
    seg, _ = aligned(c.targets[t][1], 0, "50=", rng)
    q = c.query(b"many", seg)
    first = len(c.chains)
    for k in range(70):
        c.chain(q, t, 0, 0, 50, 60 * k, "50=", score=200 - k if k != 5 else 300, parent=None if k == 5 else first + 5, sub=199 if k == 5 else 0,
                mapq=0)
    a, _ = aligned(c.targets[t][1], 7, "20=1X20=", rng)
    b, _ = aligned(c.targets[t][1], 307, "30=", rng)
    q = c.query(b"split", a + b"GG" + revcomp(b))  # the second part maps on the other strand
    c.chain(q, t, 0, 0, 41, 7, "20=1X20=", score=80)
    c.chain(q, t, 1, 43, 73, 307, "30=", score=90, sub=4)
    q = c.query(b"tie", a + b)
    c.chain(q, t, 0, 0, 41, 7, "20=1X20=", score=77)
    c.chain(q, t, 0, 41, 71, 307, "30=", score=77)
    c.chain(q, t, 0, 41, 71, 367, "30=", score=60, parent=len(c.chains) - 1)
    c.query(b"last", b"ACGTT")
    out.append(c.done())
    return out


def _pairs():
    rng = random.Random(12)
    c = Case("pairs", paired=True)
    t0 = c.target(b"chr1", rand_seq(rng, 600))
    t1 = c.target(b"chr2", rand_seq(rng, 400))
    # a proper pair, FR, mate 1 forward; and one with mate 1 reverse (mate 1's TLEN is negative)
    _, a = c.read(b"pp/1", t0, 10, "40=1X9=", rng, lclip=2)
    _, b = c.read(b"pp/2", t0, 200, "50=", rng, strand=1)
    c.pair(a, b)
    _, a = c.read(b"rf/1", t0, 300, "50=", rng, strand=1)
    _, b = c.read(b"rf/2", t0, 120, "25=1D25=", rng)
    c.pair(a, b, n_best=2)
    # equal t_start of the two mates: record 2p's line is the positive one
    _, a = c.read(b"eq/1", t0, 90, "45=", rng, strand=1)
    _, b = c.read(b"eq/2", t0, 90, "30=", rng)
    c.pair(a, b)
    # one mate unmapped, either side; both unmapped
    c.read(b"m1/1", t0, 50, "30=", rng, strand=1)
    c.query(b"m1/2", rand_seq(rng, 33))
    c.query(b"m2/1", rand_seq(rng, 31))
    c.read(b"m2/2", t1, 60, "30=", rng)
    c.query(b"uu/1", rand_seq(rng, 20))
    c.query(b"uu/2", rand_seq(rng, 21))
    # mates on different targets, not selected: the mate line is the partner's representative
    c.read(b"dt/1", t0, 400, "35=", rng)
    c.read(b"dt/2", t1, 100, "35=", rng, strand=1)
    # a selected chain that is not its record's representative: mate 2's best chain lies elsewhere, its secondary is concordant
    _, a = c.read(b"ns/1", t0, 20, "40=", rng)
    seg, _ = aligned(c.targets[t1][1], 300, "40=", rng)
    q = c.query(b"ns/2", revcomp(seg))
    best = c.chain(q, t1, 1, 0, 40, 300, "40=", score=120, sub=90, mapq=15, n_sec=1)
    b = c.chain(q, t0, 1, 0, 40, 180, "20=1X19=", score=90, parent=best, mapq=0)
    c.pair(a, b)
    # discordant on one target, same strand: not selected, TLEN by the representatives
    c.read(b"dc/1", t0, 500, "30=", rng)
    c.read(b"dc/2", t0, 450, "30=", rng)
    return [c.done()]


def _long():
    """one line of a few thousand runs and ~50 kB, beside short ones; lines either side of the class boundary"""
    rng = random.Random(13)
    c = Case("long")
    t = c.target(b"contig", rand_seq(rng, 52000))
    unit = [(27, "="), (1, "X"), (25, "="), (1, "I"), (26, "="), (2, "D"), (31, "="), (2, "X"), (23, "="), (3, "I"), (29, "="), (1, "D")]
    runs = unit * 260 + [(64, "=")]
    for strand in (0, 1):
        seg, _ = aligned(c.targets[t][1], 100, "".join("%d%s" % r for r in runs), rng)
        oq = rand_seq(rng, 40) + seg + rand_seq(rng, 1000)
        q = c.query(b"long%d" % strand, revcomp(oq) if strand else oq)
        qs, qe = (1000, len(oq) - 40) if strand else (40, len(oq) - 1000)
        c.chain(q, t, strand, qs, qe, 100, runs, score=40000, anchors=900)
        c.read(b"short%d" % strand, t, 5000, "60=1X60=", rng, strand=strand)
    cases = [c.done()]
    # the class boundary: lines of MSGPU_SAM_SHORT_BYTES - 1, exactly, + 1 bytes (the read's length is fitted to the line's)
    c = Case("boundary")
    t = c.target(b"b", rand_seq(rng, 2200))
    for want in (2047, 2048, 2049):
        n = want - 60
        for _ in range(4):
            probe = Case("probe")
            probe.target(b"b", c.targets[t][1])
            probe.read(b"e%d" % want, 0, 3, "%d=" % n, random.Random(want))
            d = probe.done()
            text, lines = sam_oracle.run(*tables(d))
            n += want - (len(text) - lines[0][3])
        c.read(b"e%d" % want, t, 3, "%d=" % n, random.Random(want))
    cases.append(c.done())
    return cases


CASES = [instance(0), instance(1)] + _simple() + _pairs() + _long()


def names():
    return [c["name"] for c in CASES]


def case(name):
    return next(c for c in CASES if c["name"] == name)


# ---- S1's violations: a good table with one thing wrong (or two: the smallest chain and the first check win)

def _bad():
    base = case("pairs")

    def mutated(fn, src=base):
        c = dict(src, chains=[tuple(x) for x in src["chains"]], ops=list(src["ops"]), off=list(src["off"]), ranks=list(src["ranks"]),
                 mates=None if src["mates"] is None else list(src["mates"]), targets=list(src["targets"]), queries=list(src["queries"]))
        fn(c)
        return c

    def field(i, k, v):
        def fn(c):
            ch = list(c["chains"][i])
            ch[k] = v
            c["chains"][i] = tuple(ch)
        return fn

    def both(*fns):
        def fn(c):
            for f in fns:
                f(c)
        return fn

    def setter(key, i, v):
        def fn(c):
            c[key][i] = v
        return fn
    out = [
        ("off0", mutated(setter("off", 0, 1)), "chain 0: offsets"),
        ("off-decreasing", mutated(setter("off", 4, 0)), "chain 3: offsets"),
        ("off-beyond", mutated(setter("off", 3, 10 ** 6)), "chain 2: offsets"),
        ("order", mutated(field(8, 0, 1)), "chain 8: query order"),
        ("strand", mutated(field(2, 2, 2)), "chain 2: strand"),
        ("query-record", mutated(field(len(base["chains"]) - 1, 0, 1000)), "chain %d: query record" % (len(base["chains"]) - 1)),
        ("target-record", mutated(field(1, 1, 2)), "chain 1: target record"),
        ("target-range", mutated(field(1, 9, 601)), "chain 1: target range"),
        ("target-range-reversed", mutated(both(field(1, 8, 300), field(1, 9, 299))), "chain 1: target range"),
        ("query-range", mutated(field(0, 7, 1000)), "chain 0: query range"),
        ("run-op", mutated(setter("ops", 1, 1 << 4 | 3)), "chain 0: run"),
        ("run-length", mutated(setter("ops", 3, 7)), "chain 1: run"),
        ("target-consumption", mutated(field(3, 9, base["chains"][3][9] + 1)), "chain 3: target consumption"),
        ("query-consumption", mutated(field(3, 7, base["chains"][3][7] - 1)), "chain 3: query consumption"),
        ("parent-range", mutated(setter("ranks", 2, (10 ** 6, 0, 0, 0))), "chain 2: rank"),
        ("parent-other-record", mutated(setter("ranks", 2, (0, 0, 0, 0))), "chain 2: rank"),
        ("parent-secondary", mutated(setter("ranks", 11, (12, 0, 0, 0))), "chain 11: rank"),
        ("mate-range", mutated(setter("mates", 0, (10 ** 6, 5, 1, 1))), "chain 0: mates"),
        ("mate-not-back", mutated(setter("mates", 1, (2, 5, 1, 1))), "chain 0: mates"),
        ("mate-same-record", mutated(both(setter("mates", 0, (0, 5, 1, 1)))), "chain 0: mates"),
        # two things wrong: the smaller chain wins over a later bad offset, and of one chain the first check
        ("strand-before-offsets", mutated(both(field(1, 2, 3), setter("off", 6, 0))), "chain 1: strand"),
        ("range-before-consumption", mutated(both(field(4, 9, 700), field(4, 7, 0))), "chain 4: target range"),
        ("odd-pairs", mutated(lambda c: c["queries"].pop()), "mates: %d query records" % (len(base["queries"]) - 1)),
        ("name-255", mutated(lambda c: c["targets"].__setitem__(0, (b"n" * 255, c["targets"][0][1]))), "target record 0: a name longer than 254 bytes"),
        ("query-name-255", mutated(lambda c: c["queries"].__setitem__(3, (b"n" * 255, c["queries"][3][1]))), "query record 3: a name longer than 254"),
    ]
    return out


BAD = _bad()
