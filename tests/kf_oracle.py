"""The k-mer abundance filter restated in plain Python / numpy, from the rules in include/msgpu.h ("k-mer abundance filter")
and the observed behaviour of the reference pipeline's threshold script -- not from the kernels.  Any k up to 64: keys are
Python integers; where numpy forms the windows of a whole file at once a key is two uint64 halves."""
import numpy as np

HIGH = 10001
MASK64 = (1 << 64) - 1
_CODE = {ord(c): i for i, c in enumerate("ACGT")}
_CODE.update({ord(c): i for i, c in enumerate("acgt")})


class FastqError(ValueError):
    def __init__(self, file, line, what):
        super().__init__("file %d line %d: %s" % (file, line, what))
        self.file, self.line = file, line


class DegenerateHistogram(ValueError):
    pass


def lines_of(data):
    """only '\\n' ends a line; a last line without it counts"""
    if not data:
        return []
    out = data.split(b"\n")
    if data.endswith(b"\n"):
        out.pop()
    return out


def parse_fastq(data, file=0):
    """-> [(line1, line2, line3, line4)]; FastqError at the smallest offending 1-based line"""
    ls = lines_of(data)
    for i, l in enumerate(ls):
        m = i & 3
        if m == 0 and not l.startswith(b"@"):
            raise FastqError(file, i + 1, "no '@'")
        if m == 2 and not l.startswith(b"+"):
            raise FastqError(file, i + 1, "no '+'")
        if m == 3 and len(l) != len(ls[i - 2]):
            raise FastqError(file, i + 1, "lengths differ")
    if len(ls) & 3:
        raise FastqError(file, len(ls) + 1, "ends inside a record")
    return [tuple(ls[i:i + 4]) for i in range(0, len(ls), 4)]


def parse_pair(data1, data2):
    r1 = parse_fastq(data1, 0)
    r2 = parse_fastq(data2, 1)
    if len(r1) != len(r2):
        f = 0 if len(r1) < len(r2) else 1
        raise FastqError(f, 4 * min(len(r1), len(r2)) + 1, "record counts differ")
    return r1, r2


def canonical_kmers(seq, k):
    """the canonical k-mer (a Python int) of every window of ``seq`` (bytes), in order"""
    out = []
    mask = (1 << (2 * k)) - 1
    fw = rc = run = 0
    for b in seq:
        c = _CODE.get(b)
        if c is None:
            run = 0
            continue
        fw = ((fw << 2) | c) & mask
        rc = (rc >> 2) | ((3 - c) << (2 * (k - 1)))
        run += 1
        if run >= k:
            out.append(min(fw, rc))
    return out


def _shl(hi, lo, s):
    """(hi, lo) << s on two uint64 halves; hi = None stands for a number that fits the lower half before and after"""
    U = np.uint64
    if s == 0:
        return hi, lo
    if hi is None:
        return None, lo << U(s)
    if s < 64:
        return (hi << U(s)) | (lo >> U(64 - s)), lo << U(s)
    return lo << U(s - 64), np.zeros_like(lo)


def _or(a, b):
    return (None if a[0] is None else a[0] | b[0]), a[1] | b[1]


def windows_numpy(big, k):
    """canonical_kmers over one byte string for every start position at once: -> (hi, lo, ok), the key's upper / lower 64
    bits and whether the window is one (the same rule, vectorised: the large workloads would take hours otherwise).  A
    window of a + b bases is put together from the window of a bases at its start and the one of b bases behind it."""
    lut = np.full(256, 4, np.uint8)
    for b, c in _CODE.items():
        lut[b] = c
    code = lut[np.frombuffer(big, np.uint8)]
    n = len(code) - k + 1
    if n <= 0:
        z = np.zeros(0, np.uint64)
        return z, z, np.zeros(0, bool)
    bad = np.concatenate(([0], np.cumsum(code > 3)))
    ok = (bad[k:] - bad[:-k]) == 0
    c = (code & 3).astype(np.uint64)
    wide = k > 32
    zero = (lambda x: np.zeros_like(x)) if wide else (lambda x: None)

    def cut(t, lo_, hi_):
        return (None if t[0] is None else t[0][lo_:hi_]), t[1][lo_:hi_]

    def join(x, a, y, b):  # the windows of a bases (forward, reverse) and those of b bases -> the windows of a + b bases
        (fx, rx), (fy, ry) = x, y
        m = min(len(fx[1]), len(fy[1]) - a)
        f = _or(_shl(*cut(fx, 0, m), 2 * b), cut(fy, a, a + m))
        r = _or(cut(rx, 0, m), _shl(*cut(ry, a, a + m), 2 * a))
        return f, r

    power, size = ((zero(c), c), (zero(c), np.uint64(3) - c)), 1  # the windows of one base
    acc, have = None, 0
    while size <= k:
        if k & size:
            acc = power if not have else join(acc, have, power, size)
            have += size
        if 2 * size <= k:
            power = join(power, size, power, size)
        size *= 2
    (fh, fl), (rh, rl) = acc
    if not wide:
        z = np.zeros(n, np.uint64)
        return z, np.minimum(fl[:n], rl[:n]), ok
    f_small = (fh < rh) | ((fh == rh) & (fl <= rl))
    return np.where(f_small, fh, rh)[:n], np.where(f_small, fl, rl)[:n], ok


def _joined(records1, records2):
    """every sequence line behind one another, '\n' between them (it breaks the windows), and each line's start"""
    seqs = [r[1] for rs in (records1, records2) for r in rs]
    lens = np.array([len(x) for x in seqs], np.int64)
    starts = np.concatenate(([0], np.cumsum(lens + 1)))[:len(seqs)] if seqs else np.zeros(0, np.int64)
    return b"\n".join(seqs), starts, lens


def count_arrays(hi, lo, k):
    """the windows' keys -> (hi, lo, count) per distinct key, ascending"""
    if not len(lo):
        z = np.zeros(0, np.uint64)
        return z, z, np.zeros(0, np.int64)
    if k <= 32:
        lo = np.sort(lo)
        hi = np.zeros_like(lo)
    else:
        order = np.lexsort((lo, hi))
        hi, lo = hi[order], lo[order]
    head = np.concatenate(([True], (hi[1:] != hi[:-1]) | (lo[1:] != lo[:-1])))
    at = np.flatnonzero(head)
    return hi[at], lo[at], np.diff(np.concatenate((at, [len(lo)])))


def count(records1, records2, k):
    """-> (dict canonical k-mer -> count, windows)"""
    big, _, _ = _joined(records1, records2)
    hi, lo, ok = windows_numpy(big, k)
    uh, ul, cnt = count_arrays(hi[ok], lo[ok], k)
    return {(h << 64) | l: c for h, l, c in zip(uh.tolist(), ul.tolist(), cnt.tolist())}, int(ok.sum())


def histogram(counts):
    """counts: a dict key -> count, or an array of counts"""
    c = np.asarray(list(counts.values()) if isinstance(counts, dict) else counts, np.int64)
    h = np.bincount(np.minimum(c, HIGH), minlength=HIGH + 1)
    return [(int(a), int(h[a])) for a in np.flatnonzero(h)]


def histogram_text(rows):
    return b"".join(b"%d %d\n" % (a, f) for a, f in rows)


def threshold(rows):
    """-> (q1, q3, upper) as the reference script computes them, total as the pipeline's awk line sums it;
    DegenerateHistogram where the script dies or prints a number <= 0"""
    rest = [f for a, f in rows if a != 1]
    if not rest:
        raise DegenerateHistogram("no row besides a = 1")
    total = sum(rest)
    q1_th = round((total + 1) * 0.25)
    q3_th = round((total + 1) * 0.75)
    q1 = q3 = cur = 0
    for a, f in rows:
        if a > 1:
            cur += f
            if q1 == 0 and cur >= q1_th:
                q1 = a
            elif q3 == 0 and cur >= q3_th:
                q3 = a
                break
    upper = q3 + 2 * (q3 - q1)
    if q3 == 0 or upper <= 0:
        raise DegenerateHistogram("upper = %d" % upper)
    return q1, q3, upper


def kmer_text(key, k):
    return "".join("ACGT"[(key >> (2 * (k - 1 - j))) & 3] for j in range(k))


def dump_text(abundant, k):
    return b"".join(b">%d\n%s\n" % (c, kmer_text(x, k).encode()) for x, c in abundant)


def run(k, data1, data2):
    """The whole stage -> dict: histogram rows, q1 / q3 / upper, abundant [(key, count)] ascending, verdict (a list of 0 / 1
    per pair), verdict1 / verdict2 (per mate), out1 / out2 / report (bytes), windows, distinct, other_bytes (sequence bytes outside ACGTacgt)."""
    if not 1 <= k <= 64:
        raise ValueError("k")
    r1, r2 = parse_pair(data1, data2)
    big, starts, lens = _joined(r1, r2)
    hi, lo, ok = windows_numpy(big, k)
    uh, ul, cnt = count_arrays(hi[ok], lo[ok], k)
    windows = int(ok.sum())
    rows = histogram(cnt)
    q1, q3, upper = threshold(rows)
    sel = cnt >= upper
    abundant = [((h << 64) | l, c) for h, l, c in zip(uh[sel].tolist(), ul[sel].tolist(), cnt[sel].tolist())]  # ascending
    aset = set(x for x, _ in abundant)
    hit = np.zeros(len(big) + 1, np.int64)
    if aset and len(lo):
        ab = sorted(aset, key=lambda x: (x & MASK64, x >> 64))
        ab_lo, ab_hi = np.array([x & MASK64 for x in ab], np.uint64), np.array([x >> 64 for x in ab], np.uint64)
        cand = np.flatnonzero(ok & np.isin(lo, ab_lo))
        if len(set(ab_lo.tolist())) == len(ab):  # one key per lower half: compare the upper halves side by side
            cand = cand[ab_hi[np.searchsorted(ab_lo, lo[cand])] == hi[cand]]
        else:
            cand = np.array([p for p in cand.tolist() if ((int(hi[p]) << 64) | int(lo[p])) in aset], np.int64)
        hit[cand + 1] = 1
    hit = np.cumsum(hit)
    mate = ((hit[np.minimum(starts + lens, len(big))] - hit[starts]) > 0).astype(int).tolist() if len(starts) else []
    v1, v2 = mate[:len(r1)], mate[len(r1):]
    verdict = [a | b for a, b in zip(v1, v2)]
    out = [b"".join(b"".join(l + b"\n" for l in r) for r, v in zip(rs, verdict) if not v) for rs in (r1, r2)]
    return {"histogram": rows, "q1": q1, "q3": q3, "upper": upper, "abundant": abundant, "verdict": verdict,
            "verdict1": v1, "verdict2": v2, "out1": out[0], "out2": out[1], "windows": windows, "distinct": int(len(cnt)),
            "report": b"abundance threshold for k-mer filtering:  %d\n" % upper, "pairs": len(r1),
            "other_bytes": int((~np.isin(np.frombuffer(big, np.uint8), list(_CODE) + [10])).sum())}
