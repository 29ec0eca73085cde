"""Assembly evaluation restated in plain Python, from the rules in include/msgpu.h ("assembly evaluation") -- not from the
kernels.  FASTQ parsing and the windows are kf_oracle's (rule 1 is the filter's); keys are Python integers."""
import math
from collections import Counter

import kf_oracle

ROWS, CLASSES = kf_oracle.HIGH + 1, 5
_SPACE = b" \t\n\v\f\r"


def parse_fasta(data):
    """-> [(name, bases)]: a line starting with '>' opens a record, its name is cut at the first blank; the other lines
    are the record's bases with every blank removed"""
    out = []
    for line in kf_oracle.lines_of(data):
        if line.startswith(b">"):
            words = line[1:].split()
            out.append([words[0].decode() if words else "", bytearray()])
        elif out:
            out[-1][1] += bytes(b for b in line if b not in _SPACE)
    return [(n, bytes(s)) for n, s in out]


def windows(seq, k):
    """rule 2 for one record: per window position its canonical k-mer, or None where a byte outside ACGTacgt breaks it"""
    out = []
    mask = (1 << (2 * k)) - 1
    fw = rc = run = 0
    for i, b in enumerate(seq):
        c = kf_oracle._CODE.get(b)
        if c is None:
            run = 0
        else:
            fw = ((fw << 2) | c) & mask
            rc = (rc >> 2) | ((3 - c) << (2 * (k - 1)))
            run += 1
        if i >= k - 1:
            out.append(min(fw, rc) if run >= k else None)
    return out


def read_counts(k, reads):
    """rule 1: ``reads`` is a list of one or two FASTQ texts -> Counter R"""
    R = Counter()
    for f, data in enumerate(reads):
        for rec in kf_oracle.parse_fastq(data, f):
            R.update(kf_oracle.canonical_kmers(rec[1], k))
    return R


def qv(missing, windows_, k):
    """rule 4 -> a float, math.inf, or None"""
    if not windows_:
        return None
    if not missing:
        return math.inf
    p = missing / windows_
    e = 1.0 if p == 1.0 else -math.expm1(math.log1p(-p) / k)
    return -10 * math.log10(e) + 0.0


def qv_text(missing, windows_, k):
    v = qv(missing, windows_, k)
    return "-" if v is None else "inf" if v == math.inf else "%.2f" % v


def run(k, reads, assembly, name="assembly.fa", min_count=2, R=None):
    """The whole stage for one assembly (a FASTA text) -> dict: records [(name, length, windows, missing)], total, spectrum
    {(c, a): n} without zeros, intervals [(record, start, end)], solid, found, the texts head / report / spectrum_text / bed"""
    if not 1 <= k <= 64 or not 1 <= min_count <= 10000:
        raise ValueError("parameters")
    R = read_counts(k, reads) if R is None else R
    recs = parse_fasta(assembly)
    A = Counter()
    records, intervals = [], []
    for r, (rname, seq) in enumerate(recs):
        ws = windows(seq, k)
        A.update(x for x in ws if x is not None)
        miss = [x is not None and R.get(x, 0) == 0 for x in ws]
        records.append((rname, len(seq), sum(x is not None for x in ws), sum(miss)))
        s = None
        for i, m in enumerate(miss + [False]):  # rule 7
            if m and s is None:
                s = i
            elif not m and s is not None:
                intervals.append((r, s, i - 1 + k))
                s = None
    total = tuple(sum(x[j] for x in records) for j in (1, 2, 3))
    spectrum = Counter()
    for x, a in R.items():
        spectrum[(min(A.get(x, 0), CLASSES - 1), min(a, kf_oracle.HIGH))] += 1
    for x, c in A.items():
        if x not in R:
            spectrum[(min(c, CLASSES - 1), 0)] += 1
    solid = sum(n for (c, a), n in spectrum.items() if a >= min_count)
    found = sum(n for (c, a), n in spectrum.items() if a >= min_count and c >= 1)
    head = "#k\t%d\tmin_count\t%d\n" % (k, min_count)
    name_line = "#assembly\t%s\n" % name
    report = name_line + "record\tlength\twindows\tmissing\tqv\n"
    for rname, length, w, m in records + [("total",) + total]:
        report += "%s\t%d\t%d\t%d\t%s\n" % (rname, length, w, m, qv_text(m, w, k))
    report += "completeness\t%d\t%d\t%s\n" % (found, solid, "%.4f" % (100 * found / solid) if solid else "-")
    spectrum_text = name_line
    for a in sorted(set(a for _, a in spectrum)):
        spectrum_text += "%d\t%s\n" % (a, "\t".join(str(spectrum.get((c, a), 0)) for c in range(CLASSES)))
    bed = name_line + "".join("%s\t%d\t%d\n" % (recs[r][0], s, e) for r, s, e in intervals)
    return {"records": records, "total": total, "spectrum": dict(spectrum), "intervals": intervals, "solid": solid, "found": found,
            "head": head.encode(), "report": report.encode(), "spectrum_text": spectrum_text.encode(), "bed": bed.encode()}
