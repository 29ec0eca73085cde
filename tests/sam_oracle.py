"""The SAM stage's rules S1 - S11 (include/msgpu.h, "SAM output"; muchsalsa_amd/sam.py) in plain Python: tables in, bytes and
line table out.  Sequential and slow on purpose: every line is walked run by run and column by column, where the device
works from scans.  ``targets`` and ``queries`` are lists of (name, bases) with bytes; ``chains`` holds per chain the tuple
(query, target, strand, anchors, score, nm, q_start, q_end, t_start, t_end, matches, block); ``ops`` the runs of all chains
(len << 4 | op), ``off`` their n + 1 offsets; ``ranks`` per chain (parent, sub, n_secondary, mapq); ``mates`` None or per
chain (mate, tlen, cls, n_best)."""

OPS = {1: "I", 2: "D", 7: "=", 8: "X"}
LINE_FIXED = 1024
HEADER_HD = b"@HD\tVN:1.6\tSO:unsorted\tGO:query\n"
HEADER_PG = b"@PG\tID:muchsalsa_amd\tPN:muchsalsa_amd\n"


class SamTableError(ValueError):
    """what the stage answers with MSGPU_E_ARG; str() is the text its message begins with"""


def check(targets, queries, chains, ops, off, ranks, mates=None):
    """S1's device checks: None, or "chain <i>: <the first words of the violated check>" """
    n = len(chains)
    for i, ch in enumerate(chains):
        query, target, strand, _, _, _, q_start, q_end, t_start, t_end = ch[:10]

        def bad(what):
            return "chain %d: %s" % (i, what)
        if (i == 0 and off[0] != 0) or off[i + 1] < off[i] or off[i + 1] > off[n]:
            return bad("offsets")
        if i and query < chains[i - 1][0]:
            return bad("query order")
        if strand > 1:
            return bad("strand")
        if query >= len(queries):
            return bad("query record")
        if target >= len(targets):
            return bad("target record")
        if not t_start <= t_end <= len(targets[target][1]):
            return bad("target range")
        if not q_start <= q_end <= len(queries[query][1]):
            return bad("query range")
        tc = qc = 0
        bad_run = False
        for r in ops[off[i]:off[i + 1]]:
            length, op = r >> 4, r & 15
            if length < 1 or op not in OPS:
                bad_run = True
                continue
            tc += length if op != 1 else 0
            qc += length if op != 2 else 0
        if bad_run:
            return bad("run")
        if tc != t_end - t_start:
            return bad("target consumption")
        if qc != q_end - q_start:
            return bad("query consumption")
        parent = ranks[i][0]
        if not (parent < n and chains[parent][0] == query and ranks[parent][0] == parent):
            return bad("rank")
        if mates is not None and mates[i][2] == 1:
            m = mates[i][0]
            if not (m < n and chains[m][0] == query ^ 1 and mates[m][2] == 1 and mates[m][0] == i):
                return bad("mates")
    return None


def fold(b, comp=False):
    c = chr(b).upper()
    if c not in "ACGT":
        return "N"
    return {"A": "T", "C": "G", "G": "C", "T": "A"}[c] if comp else c


def oriented(seq, strand):
    """S6's bytes of the read: as the file holds it, or reversed and complemented"""
    return "".join(fold(b, True) for b in reversed(seq)) if strand else "".join(fold(b) for b in seq)


def qname(name, paired):
    name = name if isinstance(name, bytes) else name.encode()
    if paired and len(name) > 2 and name[-2:] in (b"/1", b"/2"):
        name = name[:-2]
    return name.decode("latin-1")


def cigar(runs, lclip, rclip, clip, eqx):
    parts = [[lclip, clip]] if lclip else []
    for r in runs:
        length, op = r >> 4, OPS[r & 15]
        if not eqx and op in "=X":
            op = "M"
        if op == "M" and parts and parts[-1][1] == "M":
            parts[-1][0] += length
        else:
            parts.append([length, op])
    if rclip:
        parts.append([rclip, clip])
    return "".join("%d%s" % (p[0], p[1]) for p in parts) or "*"


def md_string(runs, tseq):
    """S10 over the target bytes tseq = target[t_start:t_end]"""
    out, count, x = [], 0, 0
    for r in runs:
        length, op = r >> 4, OPS[r & 15]
        if op == "=":
            count += length
            x += length
        elif op == "X":
            for _ in range(length):
                out.append("%d%s" % (count, fold(tseq[x])))
                count = 0
                x += 1
        elif op == "D":
            out.append("%d^%s" % (count, "".join(fold(b) for b in tseq[x:x + length])))
            count = 0
            x += length
    out.append("%d" % count)
    return "".join(out)


def header(targets):
    names = [t[0] if isinstance(t[0], bytes) else t[0].encode() for t in targets]
    return HEADER_HD + b"".join(b"@SQ\tSN:%s\tLN:%d\n" % (nm, len(t[1])) for nm, t in zip(names, targets)) + HEADER_PG


def host_check(targets, queries, mates):
    seen = set()
    for what, recs in (("target", targets), ("query", queries)):
        for r, (name, _) in enumerate(recs):
            name = name if isinstance(name, bytes) else name.encode()
            if not name:
                raise SamTableError("%s record %d: an empty name" % (what, r))
            if len(name) > 254:
                raise SamTableError("%s record %d: a name longer than 254 bytes" % (what, r))
            if what == "target":
                if name in seen:
                    raise SamTableError("target record %d: its name is that of an earlier record" % r)
                seen.add(name)


def representatives(queries, chains, ranks):
    rep = [None] * len(queries)
    for i, ch in enumerate(chains):
        if ranks[i][0] == i and (rep[ch[0]] is None or ch[4] > chains[rep[ch[0]]][4]):
            rep[ch[0]] = i
    return rep


def run(targets, queries, chains, ops, off, ranks, mates=None, eqx=True, md=False, unmapped=True):
    """(text, lines): the file's bytes, and per alignment line (chain or None, query, flag, offset)"""
    paired = mates is not None
    if paired and len(queries) % 2:
        raise SamTableError("mates: %d query records" % len(queries))
    host_check(targets, queries, mates)
    err = check(targets, queries, chains, ops, off, ranks, mates)
    if err:
        raise SamTableError(err)
    tname = [(t[0] if isinstance(t[0], str) else t[0].decode("latin-1")) for t in targets]
    rep = representatives(queries, chains, ranks)
    by_query = [[] for _ in queries]
    for i, ch in enumerate(chains):
        by_query[ch[0]].append(i)
    text, lines = [header(targets)], []
    at = len(text[0])

    def side(q):
        return (1 | (0x80 if q & 1 else 0x40)) if paired else 0

    def emit(chain, q, flag, cols):
        nonlocal at
        line = ("\t".join(str(c) for c in cols) + "\n").encode("latin-1")
        lines.append((chain, q, flag, at))
        text.append(line)
        at += len(line)

    for q, (name, seq) in enumerate(queries):
        qn = qname(name, paired)
        if not by_query[q]:
            if not unmapped:
                continue
            ml = rep[q ^ 1] if paired else None
            flag = 4 | side(q)
            if ml is not None:
                mc = chains[ml]
                flag |= 0x20 if mc[2] else 0
                cols = [qn, flag, tname[mc[1]], mc[8] + 1, 0, "*", "=", mc[8] + 1, 0]
            else:
                flag |= 8 if paired else 0
                cols = [qn, flag, "*", 0, 0, "*", "*", 0, 0]
            emit(None, q, flag, cols + [oriented(seq, 0) or "*", "*"])
            continue
        for i in by_query[q]:
            _, target, strand, anchors, score, nm, q_start, q_end, t_start, t_end = chains[i][:10]
            parent, sub, _, mapq = ranks[i]
            secondary = parent != i
            supplementary = not secondary and rep[q] != i
            flag = (0x10 if strand else 0) | (0x100 if secondary else 0) | (0x800 if supplementary else 0) | side(q)
            rnext, pnext, tlen = "*", 0, 0
            if paired:
                if mates[i][2] == 1:
                    flag |= 2
                    ml = mates[i][0]
                else:
                    ml = rep[q ^ 1]
                if ml is not None:
                    mc = chains[ml]
                    flag |= 0x20 if mc[2] else 0
                    pnext = mc[8] + 1
                    if mc[1] == target:
                        rnext = "="
                        mag = max(t_end, mc[9]) - min(t_start, mc[8])
                        tlen = mag if t_start < mc[8] or (t_start == mc[8] and q % 2 == 0) else -mag
                    else:
                        rnext = tname[mc[1]]
                else:
                    flag |= 8
                    rnext, pnext = "=", t_start + 1
            qlen = len(seq)
            lclip, rclip = (qlen - q_end, q_start) if strand else (q_start, qlen - q_end)
            runs = ops[off[i]:off[i + 1]]
            oq = oriented(seq, strand)
            if secondary:
                s = "*"
            elif supplementary:
                s = oq[lclip:qlen - rclip] or "*"
            else:
                s = oq or "*"
            cols = [qn, flag, tname[target], t_start + 1, mapq, cigar(runs, lclip, rclip, "H" if secondary or supplementary else "S", eqx),
                    rnext, pnext, tlen, s, "*", "NM:i:%d" % nm, "AS:i:%d" % score, "cm:i:%d" % anchors]
            if not secondary:
                cols.append("s2:i:%d" % sub)
            cols.append("tp:A:%s" % ("S" if secondary else "P"))
            if paired and mates[i][2] == 1:
                cols.append("nb:i:%d" % mates[i][3])
            if md:
                cols.append("MD:Z:" + md_string(runs, targets[target][1][t_start:t_end]))
            emit(i, q, flag, cols)
    return b"".join(text), lines


def line_bound(chain, n_runs, qlen, md):
    """S11's text bound of a chain's line (chain None: an unmapped line)"""
    if chain is None:
        return LINE_FIXED + qlen
    return LINE_FIXED + qlen + 11 * (n_runs + 2) + ((2 * (chain[9] - chain[8]) + 11 * (n_runs + 1)) if md else 0)
