"""Rule 10 of the mapper (include/msgpu.h, "unitig-to-read mapping": the alignment of one segment pair) and the mapper's
cigar mode restated in plain Python, on top of tests/map_oracle.py: dictionaries per row, no cleverness.  It is the yardstick
of msgpu_edit_script and of ``mapper.run(..., cigar=1)``: words, run tables, chain tables and PAF bytes are compared with
this module's without tolerance."""
import map_oracle

X, D, I = 1, 2, 3           # the kinds of a script word (kind << 30 | run)
LETTER = {0: b"=", X: b"X", D: b"D", I: b"I"}
BAM = {b"I": 1, b"D": 2, b"=": 7, b"X": 8}
ORDER = (X, D, I)           # the tie rule: the first of these whose candidate is valid and the largest


def table(a, b, band, order=ORDER):
    """rule 10's table -> (d, rows) with rows[e][k] = (G, x0, op); d = band + 1 and rows = None for a capped pair"""
    n, m = len(a), len(b)
    ks = m - n
    if abs(ks) > band:
        return band + 1, None

    def slide(i, k):
        while i < n and i + k < m and a[i] == b[i + k]:
            i += 1
        return i

    g0 = slide(0, 0)
    rows = [{0: (g0, 0, 0)}]
    if ks == 0 and g0 == n:
        return 0, rows
    for e in range(1, band + 1):
        prev, cur = rows[-1], {}
        for k in range(-e, e + 1):
            cand = {}
            if k in prev and prev[k][0] < min(n, m - k):
                cand[X] = prev[k][0] + 1
            if k + 1 in prev and prev[k + 1][0] < n:
                cand[D] = prev[k + 1][0] + 1
            if k - 1 in prev and prev[k - 1][0] + k <= m:
                cand[I] = prev[k - 1][0]
            if not cand:
                continue
            x0 = max(cand.values())
            op = [o for o in order if cand.get(o) == x0][0]
            cur[k] = (slide(x0, k), x0, op)
        rows.append(cur)
        if ks in cur and cur[ks][0] == n:
            return e, rows
    return band + 1, None


def script(a, b, band, order=ORDER):
    """-> (d, words): d = min(distance, band + 1); words = None for a capped pair, else d + 1 words: word t < d is
    kind << 30 | the '=' columns in front of edit t, word d the trailing '=' run (kind 0)"""
    d, rows = table(a, b, band, order)
    if rows is None:
        return d, None
    words = [0] * (d + 1)
    k, carry = len(b) - len(a), 0
    for e in range(d, 0, -1):
        g, x0, op = rows[e][k]
        words[e] = carry << 30 | (g - x0)
        carry = op
        k += {X: 0, D: 1, I: -1}[op]
    assert k == 0
    words[0] = carry << 30 | rows[0][0][0]
    return d, words


def columns(words):
    """script words -> [(letter, length)], zero lengths left out, not merged"""
    out = []
    for w in words:
        if w & 0x3fffffff:
            out.append((b"=", w & 0x3fffffff))
        if w >> 30:
            out.append((LETTER[w >> 30], 1))
    return out


def check_script(a, b, band, words):
    """the validity properties of rule 10 for one pair's words: both lengths consumed, '=' equal, 'X' unequal"""
    i = j = edits = 0
    for letter, ln in columns(words):
        for _ in range(ln):
            if letter == b"=":
                assert a[i] == b[j]
            elif letter == b"X":
                assert a[i] != b[j]
            i += letter in (b"=", b"X", b"D")
            j += letter in (b"=", b"X", b"I")
            edits += letter != b"="
    assert (i, j) == (len(a), len(b))
    return edits


def merge(runs):
    out = []
    for letter, ln in runs:
        if not ln:
            continue
        if out and out[-1][0] == letter:
            out[-1] = (letter, out[-1][1] + ln)
        else:
            out.append((letter, ln))
    return out


def chain_runs(anchors, k, tseq, qseq_oriented, band, stats):
    """the alignment of one chain -> (merged [(letter, length)], its capped segments)"""
    runs, capped = [(b"=", k)], 0
    for (x0, y0), (x1, y1) in zip(anchors, anchors[1:]):
        dx, dy = x1 - x0, y1 - y0
        c = min(dx, dy, k)
        lt, lq = dx - c, dy - c
        if lt or lq:
            xe, ye = x1 + k - c, y1 + k - c
            d, words = script(tseq[xe - lt:xe], qseq_oriented[ye - lq:ye], band)
            if words is None:
                stats["pairs_capped"] += 1
                capped += 1
                runs += [(b"D", lt), (b"I", lq)]
            else:
                stats["pairs_d0" if d == 0 else "pairs_lds" if d <= LDS_MAX_D else "pairs_slab"] += 1
                stats["max_d"] = max(stats["max_d"], d)
                stats["script_words"] += d + 1
                for w in words:
                    if w >> 30:
                        stats["xdi"[(w >> 30) - 1] + "_columns"] += 1
                runs += columns(words)
        runs.append((b"=", c))
    return merge(runs), capped


LDS_MAX_D = 31  # msgpu_align.hip, ES_LDS_MAXD: the class boundary the stats report


def cigar_run(targets, queries, exact_result=None, **params):
    """map_oracle.run(..., exact=1) with rule 10's figures -> a dict: ``paf`` (bytes), ``chains`` (the fields of
    msgpu_map_chain), ``runs`` (per chain [(letter, length)]), ``cigars`` (per chain the string), ``packed`` (per chain
    [len << 4 | BAM code]), ``capped`` (per chain its capped segments), ``align`` (the counts of msgpu_map_astats) and ``exact``
    (map_oracle's result; ``exact_result`` hands in one that a caller has computed for the same arguments already)"""
    r = exact_result if exact_result is not None else map_oracle.run(targets, queries, **dict(params, exact=1))
    p = r["params"]
    if p["ava"]:
        queries = targets
    stats = dict(pairs_d0=0, pairs_lds=0, pairs_slab=0, pairs_capped=0, max_d=0, x_columns=0, i_columns=0, d_columns=0,
                 script_words=0, runs=0)
    chains, lines, all_runs, all_capped, rc = [], [], [], [], {}
    for ch, anchors in zip(r["chains"], r["notes"].get("chain_anchors", [])):
        q, t, s, n, score, _, qs, qe, ts, te, _, _ = ch
        qseq = queries[q][1]
        if s and q not in rc:
            rc[q] = map_oracle.revcomp(qseq)
        runs, capped = chain_runs(anchors, p["k"], targets[t][1], rc[q] if s else qseq, p["band"], stats)
        all_capped.append(capped)
        matches = sum(ln for letter, ln in runs if letter == b"=")
        block = sum(ln for _, ln in runs)
        stats["runs"] += len(runs)
        chains.append((q, t, s, n, score, block - matches, qs, qe, ts, te, matches, block))
        all_runs.append(runs)
        lines.append(b"%s\t%d\t%d\t%d\t%s\t%s\t%d\t%d\t%d\t%d\t%d\t255\tcm:i:%d\ts1:i:%d\tNM:i:%d\tcg:Z:%s\n" % (
            queries[q][0], len(qseq), qs, qe, b"-" if s else b"+", targets[t][0], len(targets[t][1]), ts, te, matches, block, n,
            score, block - matches, b"".join(b"%d%s" % (ln, letter) for letter, ln in runs)))
    return {"paf": b"".join(lines), "chains": chains, "runs": all_runs,
            "cigars": ["".join("%d%s" % (ln, letter.decode()) for letter, ln in runs) for runs in all_runs],
            "packed": [[ln << 4 | BAM[letter] for letter, ln in runs] for runs in all_runs], "capped": all_capped, "align": stats,
            "exact": r}
