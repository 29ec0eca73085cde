"""Restatement of the unitig coverage filter for the tests, written from the stage's rules (muchsalsa_amd/unitig_filter.py's
docstring) and structurally independent of the device: it works on PER-BASE coverage arrays (a difference array per
block, np.cumsum, np.maximum.reduceat), where the device sweeps sorted interval endpoints.

run(paf_bytes, fasta_bytes) -> (out.fa bytes, report dict); OracleError(line) where the stage must fail."""
import numpy as np

WRAP = 60
MIN_RUN = 500
CHUNK = 1 << 24  # positions per difference array


class OracleError(Exception):
    def __init__(self, what, line=0):
        super().__init__("%s (line %d)" % (what, line))
        self.line = line


def _int(tok, line, signed=False):
    neg = signed and tok[:1] == b"-"
    t = tok[1:] if neg else tok
    if not t or not t.isdigit():
        raise OracleError("not an integer: %r" % tok, line)
    v = int(t)
    if v > 2**31 - 1:
        raise OracleError("out of range: %r" % tok, line)
    return -v if neg else v


def parse_paf(data):
    """-> (names per line, qlen, qs, qe, reads per line) with the stage's checks."""
    if not data:
        raise OracleError("empty PAF", 1)
    lines = data.split(b"\n")
    if lines[-1] == b"":
        lines.pop()
    names, reads = [], []
    qlen = np.empty(len(lines), np.int64)
    qs = np.empty(len(lines), np.int64)
    qe = np.empty(len(lines), np.int64)
    for i, raw in enumerate(lines):
        ln = i + 1
        f = raw.rstrip(b" \t\n\v\f\r").split(b"\t")
        if f == [b""] or len(f) < 7:
            raise OracleError("blank line or fewer than 7 fields", ln)
        qlen[i] = _int(f[1], ln)
        qs[i] = _int(f[2], ln)
        qe[i] = _int(f[3], ln)
        _int(f[6], ln, signed=True)
        if not f[0]:
            raise OracleError("empty unitig id", ln)
        names.append(f[0])
        reads.append(f[5])
    return names, qlen, qs, qe, reads


def parse_fasta(data):
    """id -> (description, bases); first record of an id wins; every isspace byte is removed from the bases."""
    recs = {}
    cur = None
    body = []

    def close():
        if cur is not None and cur[0] not in recs:
            recs[cur[0]] = (cur[1], b"".join(b"".join(x.split()) for x in body))

    for raw in data.split(b"\n"):
        if raw[:1] == b">":
            close()
            desc = raw[1:].rstrip(b" \t\n\v\f\r")
            cur = (desc.split(None, 1)[0] if desc.split() and not desc[:1].isspace() else b"", desc)
            body = []
        elif cur is not None:
            body.append(raw)
    close()
    return recs


def _blocks(names):
    starts = [0] + [i for i in range(1, len(names)) if names[i] != names[i - 1]]
    return np.asarray(starts, np.int64), np.asarray(starts[1:] + [len(names)], np.int64)


def _block_max(qlen, line_block, qs, qe, use):
    """per block: max over [0, qlen) of the coverage by the lines in `use` (per-base difference arrays)."""
    nb = len(qlen)
    out = np.zeros(nb, np.int64)
    base = np.concatenate(([0], np.cumsum(qlen + 1)))
    b = 0
    while b < nb:
        e = b + 1
        while e < nb and base[e + 1] - base[b] <= CHUNK:
            e += 1
        lo, hi = base[b], base[e]
        m = use & (line_block >= b) & (line_block < e) & (qs < qe)
        diff = (np.bincount(base[line_block[m]] - lo + qs[m], minlength=hi - lo) -
                np.bincount(base[line_block[m]] - lo + qe[m], minlength=hi - lo))
        cov = np.cumsum(diff)
        out[b:e] = np.maximum.reduceat(cov, base[b:e] - lo)
        b = e
    return out


def _runs(cov, t):
    """maximal runs of cov <= t (as [start, end] inclusive) of >= MIN_RUN positions"""
    good = np.concatenate(([False], cov <= t, [False])).astype(np.int8)
    d = np.diff(good)
    s, e = np.flatnonzero(d == 1), np.flatnonzero(d == -1)
    keep = (e - s) >= MIN_RUN
    return list(zip(s[keep].tolist(), (e[keep] - 1).tolist()))


def _wrap(seq):
    return b"".join(seq[i:i + WRAP] + b"\n" for i in range(0, len(seq), WRAP))


def run(paf, fasta):
    names, qlen_l, qs, qe, reads = parse_paf(paf)
    b0, b1 = _blocks(names)
    nb = len(b0)
    qlen = qlen_l[b0]
    line_block = np.repeat(np.arange(nb), b1 - b0)
    bad = np.flatnonzero(qe > qlen[line_block])
    if len(bad):
        raise OracleError("qend beyond the block's qlen", int(bad[0]) + 1)
    # pass 1: the first line of each read id in a block
    rid = {}
    rcode = np.fromiter((rid.setdefault(r, len(rid)) for r in reads), np.int64, len(reads))
    key = line_block * (len(rid) + 1) + rcode
    _, first = np.unique(key, return_index=True)
    use = np.zeros(len(names), bool)
    use[first] = True
    value = _block_max(qlen, line_block, qs, qe, use)
    by_id = {}
    for b in range(nb):
        by_id[names[b0[b]]] = int(value[b])  # the last block wins
    vals = np.asarray(list(by_id.values()), np.int64)
    q1 = np.percentile(vals, 25)
    q3 = np.percentile(vals, 75)
    upper = q3 + 1.5 * (q3 - q1)
    recs = parse_fasta(fasta)
    for b in range(nb):
        if names[b0[b]] not in recs:
            raise OracleError("unitig missing from the FASTA", int(b0[b]) + 1)
    out = []
    n_out = n_resc = 0
    for b in range(nb):
        name = names[b0[b]]
        desc, seq = recs[name]
        if by_id[name] > upper:
            n_out += 1
            L = int(qlen[b])
            s, e = qs[b0[b]:b1[b]], qe[b0[b]:b1[b]]
            m = s < e
            cov = np.cumsum(np.bincount(s[m], minlength=L + 1) - np.bincount(e[m], minlength=L + 1))[:L]
            runs = _runs(cov, q3)
            n_resc += 1 if runs else 0
            for k, (st, en) in enumerate(runs):
                out.append(b">%s_%d %d %d %d\n" % (name, k, en - st + 1, st, en) + _wrap(seq[st:en + 1]))
        else:
            out.append(b">" + desc + b"\n" + _wrap(seq))
    report = {"upper": float(upper), "q1": float(q1), "q3": float(q3), "blocks": nb, "outliers": n_out,
              "rescued": n_resc}
    return b"".join(out), report


def report_lines(r):
    return ">>> unitig filter \nupper_outlier: {}\nQ3: {}\n#all unitigs: {}\n#outliers: {}\n#rescued outliers: {}\n".format(
        r["upper"], r["q3"], r["blocks"], r["outliers"], r["rescued"])
