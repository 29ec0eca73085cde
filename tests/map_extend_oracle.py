"""Rule 11 of the mapper (include/msgpu.h, "unitig-to-read mapping": end extension) restated in plain Python on top of
tests/map_cigar_oracle.py and tests/map_oracle.py: dictionaries per row, every row computed, no cleverness.  It is the
yardstick of msgpu_extend_ends and of ``mapper.run(..., cigar=1, extend=E)``: end cells, words, run tables, chain tables, PAF
bytes and counts are compared with this module's without tolerance."""
import map_cigar_oracle as cg
import map_oracle

P = 8  # the rule's penalty (MSGPU_MAP_EXTEND_PENALTY)
X, D, I = cg.X, cg.D, cg.I


def better(s, e, k, bs, be, bk):
    """rule 11.3's order: the greater score, then the smaller e, then the smaller |k|, then the negative k"""
    if s != bs:
        return s > bs
    if e != be:
        return e < be
    if abs(k) != abs(bk):
        return abs(k) < abs(bk)
    return k < bk


def reach(a, b, band, early_stop=False):
    """rule 11.2 to 11.4 on the flanks (a, b) -> ((e, k, x, y, score, rows), words).  Every row 0..band is computed; ``rows``
    is the first e with n + m - P * e <= the best score of the rows before it, or band + 1.  ``early_stop`` ends the table at
    that row instead (the kernel's way; the tests show that it changes nothing)."""
    n, m = len(a), len(b)

    def slide(i, k):
        while i < n and i + k < m and a[i] == b[i + k]:
            i += 1
        return i

    g0 = slide(0, 0)
    table = [{0: (g0, 0, 0)}]
    best, charged = (2 * g0, 0, 0), None
    for e in range(1, band + 1):
        if charged is None and n + m - P * e <= best[0]:
            charged = e
            if early_stop:
                break
        prev, cur = table[-1], {}
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
            op = [o for o in cg.ORDER if cand.get(o) == x0][0]
            cur[k] = (slide(x0, k), x0, op)
            s = 2 * cur[k][0] + k - P * e
            if better(s, e, k, *best):
                best = (s, e, k)
        table.append(cur)
    score, es, ks = best
    words = [0] * (es + 1)
    k, carry = ks, 0
    for e in range(es, 0, -1):
        g, x0, op = table[e][k]
        words[e] = carry << 30 | (g - x0)
        carry = op
        k += {X: 0, D: 1, I: -1}[op]
    assert k == 0
    words[0] = carry << 30 | table[0][0][0]
    x = table[es][ks][0]
    return (es, ks, x, x + ks, score, band + 1 if charged is None else charged), words


def check_extension(a, b, end, words):
    """rule 11.4's validity properties: e + 1 words, exactly x bytes of a and y bytes of b consumed, '=' equal, X unequal,
    e columns that are not '=', and the score is x + y - P * e"""
    e, k, x, y, score, _ = end
    assert len(words) == e + 1 and words[-1] >> 30 == 0 and all(w >> 30 for w in words[:-1])
    i = j = edits = 0
    for letter, ln in cg.columns(words):
        for _ in range(ln):
            if letter == b"=":
                assert a[i] == b[j]
            elif letter == b"X":
                assert a[i] != b[j]
            i += letter in (b"=", b"X", b"D")
            j += letter in (b"=", b"X", b"I")
            edits += letter != b"="
    assert (i, j, edits) == (x, y, e) and y == x + k and score == x + y - P * e and x <= len(a) and y <= len(b)


STATS = ("n_ends", "n_ends_extended", "n_ends_at_sequence_end", "t_bases", "q_bases", "x_columns", "i_columns", "d_columns", "max_e",
         "rows", "n_inconsistent")


def flanks(anchors, k, tseq, oq, extend):
    """rule 11.1 -> ((A, B) of the left end, (A, B) of the right end) and the room (target, query) either end has"""
    (x0, y0), (x1, y1) = anchors[0], anchors[-1]
    te, ye = x1 + k, y1 + k
    left = (tseq[x0 - min(extend, x0):x0][::-1], oq[y0 - min(extend, y0):y0][::-1])
    right = (tseq[te:te + min(extend, len(tseq) - te)], oq[ye:ye + min(extend, len(oq) - ye)])
    return (left, right), ((x0, y0), (len(tseq) - te, len(oq) - ye))


def extend_run(targets, queries, extend, cigar_result=None, **params):
    """cigar_run with rule 11 -> a dict: ``paf``, ``chains``, ``runs``, ``cigars``, ``packed`` as cigar_run's, ``ext`` (per
    chain the end cells (left, right)), ``stats`` (the counts of msgpu_map_xstats) and ``cigar`` (cigar_run's result;
    ``cigar_result`` hands in one computed for the same arguments).  extend = 0 gives cigar_run's bytes."""
    r = cigar_result if cigar_result is not None else cg.cigar_run(targets, queries, **params)
    p = r["exact"]["params"]
    if p["ava"]:
        queries = targets
    k, band = p["k"], p["band"]
    stats = dict.fromkeys(STATS, 0)
    stats["extend"] = extend
    chains, lines, all_runs, ext, rc = [], [], [], [], {}
    if not extend:
        return dict(r, ext=[], stats=dict(stats, extend=0), cigar=r)
    for ch, anchors, runs in zip(r["chains"], r["exact"]["notes"].get("chain_anchors", []), r["runs"]):
        q, t, s, n, score, nm, qs, qe, ts, te, matches, block = ch
        qseq, tseq = queries[q][1], targets[t][1]
        if s and q not in rc:
            rc[q] = map_oracle.revcomp(qseq)
        oq = rc[q] if s else qseq
        pairs, room = flanks(anchors, k, tseq, oq, extend)
        ends, cols = [], []
        for (a, b), (t_room, q_room) in zip(pairs, room):
            end, words = reach(a, b, band)
            check_extension(a, b, end, words)
            ends.append(end)
            cols.append(cg.columns(words))
            e, _, x, y, _, rows = end
            stats["n_ends"] += 1
            stats["n_ends_extended"] += x + y > 0
            stats["n_ends_at_sequence_end"] += x == t_room or y == q_room
            stats["t_bases"] += x
            stats["q_bases"] += y
            for w in words:
                if w >> 30:
                    stats["xdi"[(w >> 30) - 1] + "_columns"] += 1
            stats["max_e"] = max(stats["max_e"], e)
            stats["rows"] += rows
        (eL, _, xL, yL, _, _), (eR, _, xR, yR, _, _) = ends
        runs = cg.merge(cols[0][::-1] + list(runs) + cols[1])
        y0, ye = anchors[0][1] - yL, anchors[-1][1] + k + yR
        qs, qe = (len(qseq) - ye, len(qseq) - y0) if s else (y0, ye)
        ts, te = ts - xL, te + xR
        matches = sum(ln for letter, ln in runs if letter == b"=")
        block = sum(ln for _, ln in runs)
        assert block - matches == nm + eL + eR
        assert te - ts == sum(ln for c, ln in runs if c in (b"=", b"X", b"D"))
        assert qe - qs == sum(ln for c, ln in runs if c in (b"=", b"X", b"I"))
        chains.append((q, t, s, n, score, block - matches, qs, qe, ts, te, matches, block))
        all_runs.append(runs)
        ext.append(tuple(ends))
        lines.append(b"%s\t%d\t%d\t%d\t%s\t%s\t%d\t%d\t%d\t%d\t%d\t255\tcm:i:%d\ts1:i:%d\tNM:i:%d\tcg:Z:%s\n" % (
            queries[q][0], len(qseq), qs, qe, b"-" if s else b"+", targets[t][0], len(tseq), ts, te, matches, block, n, score,
            block - matches, b"".join(b"%d%s" % (ln, letter) for letter, ln in runs)))
    return {"paf": b"".join(lines), "chains": chains, "runs": all_runs, "ext": ext, "stats": stats, "cigar": r,
            "cigars": ["".join("%d%s" % (ln, letter.decode()) for letter, ln in runs) for runs in all_runs],
            "packed": [[ln << 4 | cg.BAM[letter] for letter, ln in runs] for runs in all_runs],
            "n_runs": sum(len(runs) for runs in all_runs)}
