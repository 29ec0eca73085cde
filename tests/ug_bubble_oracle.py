"""Rule 9 of the short-read unitig assembly (include/msgpu.h, "short-read unitig assembly": bubble popping on request)
restated in plain Python, on top of ug_oracle, which holds rules 1-8 -- from the rule's text, not from the kernels.

    (a) simple branch   branch
    (b), (c) bubble     bubble_round: the judging side, the winner
    (d) rounds          bubble_round: the snapshot, and the assertions that no k-mer is claimed twice and no winner leaves
    (e) phases          clean
"""
import ug_oracle
from ug_oracle import Graph, canon, rc, texts, tip_round, tip_rounds, unitigs  # noqa: F401  (re-exported for the tests)

BUBBLE_MAX = 4096


def branch(g, b, bubble):
    """(a) the simple branch that starts at b, a successor of a fork -> (path, merge) or None"""
    if len(g.pred(b)) != 1:
        return None
    path = [b]
    while True:
        nxt = g.succ(path[-1])
        if len(nxt) != 1:
            return None
        t = nxt[0]
        if len(g.pred(t)) >= 2:
            return path, t
        if len(path) == bubble:
            return None
        path.append(t)


def fork_branches(g, u, bubble):
    """-> {merge: [(base c, path)]} over the simple branches of the fork u, c ascending"""
    out = {}
    for b in g.succ(u):  # ascending by the base
        br = branch(g, b, bubble)
        if br is not None:
            out.setdefault(br[1], []).append((b & 3, br[0]))
    return out


def bubble_round(S, k, bubble, found=None):
    """(b)-(d), one round on the snapshot ``S`` -> (canonical k-mers that leave, forks, bubbles, branches removed).
    ``found`` (a list) receives every bubble that was judged: (u, t, [(c, path)], index of the winner), and every bubble
    that was left because fork and merge are one k-mer, with the winner None."""
    g = Graph(S, k)
    gone, claimed, kept = set(), {}, set()
    forks = bubbles = branches = 0
    for u in g.nodes():
        if len(g.succ(u)) < 2:
            continue
        forks += 1
        for t, brs in fork_branches(g, u, bubble).items():
            if len(brs) < 2:
                continue
            if canon(u, k) == canon(t, k):
                if found is not None:
                    found.append((u, t, brs, None))
                continue
            if not u < rc(t, k):
                continue  # the mirror bubble (rc(t), rc(u)) is the one that is judged
            win = 0
            for i in range(1, len(brs)):
                a, b = brs[i][1], brs[win][1]
                if sum(S[canon(x, k)] for x in a) * len(b) > sum(S[canon(x, k)] for x in b) * len(a):
                    win = i  # (among equals the smaller base stays)
            bubbles += 1
            for i, (c, path) in enumerate(brs):
                mers = {canon(x, k) for x in path}
                for x in mers:
                    assert x not in claimed, "a k-mer lies in two branches"
                    claimed[x] = (u, t, c)
                if i == win:
                    kept |= mers
                else:
                    gone |= mers
                    branches += 1
            if found is not None:
                found.append((u, t, brs, win))
    assert not (gone & kept), "a round removes a winner"
    return gone, forks, bubbles, branches


def clean(solid, k, trim, bubble, found=None):
    """rule 4, then (e) -> (what cleaning leaves, tip rounds [(limit, removed)], bubble rounds [(tip rounds before it,
    forks, bubbles, branches removed, k-mers removed)], bubble phases).  ``found`` receives a list per bubble round."""
    S, rounds = tip_rounds(solid, k, trim)
    brounds, phases = [], 0
    while bubble:
        phases += 1
        phase_removed = 0
        while True:
            seen = [] if found is not None else None
            gone, forks, bubbles, branches = bubble_round(S, k, bubble, seen)
            if found is not None:
                found.append(seen)
            for x in gone:
                del S[x]
            brounds.append((len(rounds), forks, bubbles, branches, len(gone)))
            phase_removed += len(gone)
            if not gone:
                break
        if not phase_removed or not trim:
            break
        tips_removed = 0
        while True:
            gone = tip_round(S, k, trim)
            for x in gone:
                del S[x]
            rounds.append((trim, len(gone)))
            tips_removed += len(gone)
            if not gone:
                break
        if not tips_removed:
            break
    return S, rounds, brounds, phases


def run(k, datas, bubble=0, min_count=2, trim=None, min_length=500, found=None):
    """ug_oracle.run with rule 9 -> its dict, and ``bubble``, ``bubble_rounds`` [(tip rounds before it, forks, bubbles,
    branches removed, k-mers removed)], ``bubble_phases``, ``bubbles``, ``bubble_branches`` and ``bubble_kmers`` (totals)"""
    if not 2 <= k <= 64 or min_count < 1 or not 0 <= bubble <= BUBBLE_MAX:
        raise ValueError("k / min_count / bubble")
    trim = k if trim is None else trim
    records = ug_oracle.parse_files(datas)
    counts, windows = ug_oracle.count_files(records, k)
    solid = {x: c for x, c in counts.items() if c >= min_count}
    S, rounds, brounds, phases = clean(solid, k, trim, bubble, found)
    units, blocked = unitigs(S, k)
    table, all_text, cut_text = texts(units, S, k, min_length)
    chains = [u[1] for u in sorted(units, key=lambda u: u[0])]
    other = sum(1 for rs in records for r in rs for b in r[1] if b not in b"ACGTacgt")
    return {"k": k, "records": [len(r) for r in records], "windows": windows, "distinct": len(counts), "solid": len(solid),
            "solid_after": len(S), "rounds": rounds, "unitigs": table, "kept": sum(1 for t in table if t[0] >= min_length),
            "cycles": sum(t[4] for t in table), "longest": max([len(c) for c in chains], default=0), "all": all_text,
            "cut": cut_text, "chains": chains, "blocked": blocked, "counts": S,
            "alone": sum(1 for c in chains if len(c) == 1 and c[0] == rc(c[0], k)), "other_bytes": other,
            "bubble": bubble, "bubble_rounds": brounds, "bubble_phases": phases, "bubbles": sum(r[2] for r in brounds),
            "bubble_branches": sum(r[3] for r in brounds), "bubble_kmers": sum(r[4] for r in brounds)}
