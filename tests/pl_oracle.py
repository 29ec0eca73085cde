"""The polishing stage (muchsalsa_amd.polish, include/msgpu.h "pileup consensus") restated in plain Python: rules 1-7, one
function per rule, integers only, no numpy.  It is the yardstick of the stage's tests: the GPU's FASTA, counts and record table
are compared with this module's without tolerance.  Chains are the tuples of msgpu_map_chain (query, target, strand, anchors,
score, nm, q_start, q_end, t_start, t_end, matches, block); the runs of chain i are runs[i], each len << 4 | op."""

PARAMS = dict(min_depth=3, min_identity=0)
OP_I, OP_D, OP_EQ, OP_X = 1, 2, 7, 8
A, C, G, T, DEL, OTHER = range(6)
CLASS = {65: A, 67: C, 71: G, 84: T}
LETTER = b"ACGT"
COMP = {65: 84, 84: 65, 67: 71, 71: 67}
LINE = 60
MAX_INS = 32
# rule 1: what can be wrong with a chain, in the order in which one chain's violations are looked at
WHAT = ("query order", "strand", "query record", "target record", "target range", "query range", "run", "target consumption",
        "query consumption")
COUNTS = ("n_chains", "n_runs", "n_voters", "n_ignored", "cols_eq", "cols_x", "cols_d", "cols_i", "pos_verbatim", "pos_unchanged",
          "pos_substituted", "pos_deleted", "ins_usable", "ins_unusable", "ins_at_ends", "ins_applied", "bases_inserted",
          "max_depth", "bytes_out")


class PolishError(ValueError):
    def __init__(self, chain, what):
        super().__init__("chain %d: %s" % (chain, what))
        self.chain, self.what = chain, what


def fold(b):
    return b - 32 if 97 <= b <= 122 else b


def consumed(runs):
    """(target bases, query bases) that a list of runs consumes; a run of an unknown op consumes nothing"""
    t = sum(r >> 4 for r in runs if r & 15 in (OP_EQ, OP_X, OP_D))
    q = sum(r >> 4 for r in runs if r & 15 in (OP_EQ, OP_X, OP_I))
    return t, q


def check(draft, reads, chains, runs):
    """rule 1: raises PolishError for the smallest chain that breaks it, naming the first of WHAT that it breaks"""
    for i, ch in enumerate(chains):
        q, t, s, _, _, _, qs, qe, ts, te, _, _ = ch
        bad = []
        if i and q < chains[i - 1][0]:
            bad.append("query order")
        if s not in (0, 1):
            bad.append("strand")
        if q >= len(reads):
            bad.append("query record")
        if t >= len(draft):
            bad.append("target record")
        if t < len(draft) and not ts < te <= len(draft[t][1]):
            bad.append("target range")
        if q < len(reads) and not qs <= qe <= len(reads[q][1]):
            bad.append("query range")
        if any(r >> 4 < 1 or r & 15 not in (OP_I, OP_D, OP_EQ, OP_X) for r in runs[i]):
            bad.append("run")
        tc, qc = consumed(runs[i])
        if tc != te - ts:
            bad.append("target consumption")
        if qc != qe - qs:
            bad.append("query consumption")
        if bad:
            raise PolishError(i, min(bad, key=WHAT.index))


def voters(chains, min_identity):
    """rule 2: the indices of the voters, one per query record at most"""
    best = {}
    for i, ch in enumerate(chains):
        q, score, matches, block = ch[0], ch[4], ch[10], ch[11]
        if matches * 100 < min_identity * block:
            continue
        if q not in best or (score, block) > (chains[best[q]][4], chains[best[q]][11]):
            best[q] = i  # (a later chain has to be strictly better: the first in table order wins a tie)
    return sorted(best.values())


def oriented(seq, strand):
    """rule 3: the oriented query, folded"""
    if strand:
        seq = bytes(COMP.get(b, b) for b in reversed(seq))
    return bytes(fold(b) for b in seq)


def pileup(draft, reads, chains, runs, voting, stats):
    """rule 4 -> (counters[record][position] = [A, C, G, T, del, other], events {(record, slot): {(L, packed): count}})"""
    counters = [[[0] * 6 for _ in seq] for _, seq in draft]
    events = {}
    cache = {}
    for i in voting:
        q, t, s, _, _, _, qs, qe, ts, te, _, _ = chains[i]
        if (q, s) not in cache:
            cache[(q, s)] = oriented(reads[q][1], s)
        oq = cache[(q, s)]
        j = qs if s == 0 else len(oq) - qe  # where the chain starts in the oriented query
        p = ts
        for n, r in enumerate(runs[i]):
            ln, op = r >> 4, r & 15
            if op in (OP_EQ, OP_X):
                for x in range(ln):
                    counters[t][p + x][CLASS.get(oq[j + x], OTHER)] += 1
                stats["cols_eq" if op == OP_EQ else "cols_x"] += ln
                p += ln
                j += ln
            elif op == OP_D:
                for x in range(ln):
                    counters[t][p + x][DEL] += 1
                stats["cols_d"] += ln
                p += ln
            else:
                stats["cols_i"] += ln
                letters = oq[j:j + ln]
                if n == 0 or n == len(runs[i]) - 1:
                    stats["ins_at_ends"] += 1
                elif ln <= MAX_INS and all(b in CLASS for b in letters):
                    stats["ins_usable"] += 1
                    packed = 0
                    for b in letters:
                        packed = packed << 2 | CLASS[b]
                    at = events.setdefault((t, p), {})
                    at[(ln, packed)] = at.get((ln, packed), 0) + 1
                else:
                    stats["ins_unusable"] += 1
                j += ln
    return counters, events


def call(cnt, draft_byte, min_depth):
    """rule 5 for one position -> ("verbatim" | "unchanged" | "substituted" | "deleted", the bytes emitted)"""
    if sum(cnt) < min_depth or not any(cnt[:5]):
        return "verbatim", bytes([draft_byte])
    top = max(cnt[:5])
    tied = [c for c in (A, C, G, T, DEL) if cnt[c] == top]
    own = CLASS.get(fold(draft_byte))
    winner = own if own in tied else tied[0]
    if winner == own:
        return "unchanged", bytes([draft_byte])
    if winner == DEL:
        return "deleted", b""
    return "substituted", LETTER[winner:winner + 1]


def insertion(cands, depth_left, depth_here, min_depth):
    """rule 6 for one slot -> the letters put in front of the position's call (b"": none)"""
    (ln, packed), count = min(cands.items(), key=lambda kv: (-kv[1], kv[0][0], kv[0][1]))
    m = min(depth_left, depth_here)
    if m < min_depth or 2 * count <= m:
        return b""
    return bytes(LETTER[packed >> 2 * (ln - 1 - x) & 3] for x in range(ln))


def fasta(name, bases):
    """rule 7: a record of msgpu_fasta_format (one with no bases: the header and an empty line)"""
    lines = [bases[x:x + LINE] for x in range(0, len(bases), LINE)] or [b""]
    return b">" + name + b"\n" + b"\n".join(lines) + b"\n"


def run(draft, reads, chains, runs, **params):
    """draft, reads: [(name, bases)].  -> a dict: ``text`` (the polished FASTA), ``records`` (per draft record: length in, length
    out, substitutions, deletions, insertions, mean depth x 100) and the counts of msgpu_pl_stats (COUNTS)."""
    p = dict(PARAMS, **params)
    if p["min_depth"] < 1 or not 0 <= p["min_identity"] <= 100:
        raise ValueError("parameters")
    check(draft, reads, chains, runs)
    stats = dict.fromkeys(COUNTS, 0)
    voting = voters(chains, p["min_identity"])
    stats.update(n_chains=len(chains), n_runs=sum(len(r) for r in runs), n_voters=len(voting), n_ignored=len(chains) - len(voting))
    counters, events = pileup(draft, reads, chains, runs, voting, stats)
    text, records = [], []
    for t, (name, seq) in enumerate(draft):
        out, subs, dels, ins, depth_sum = [], 0, 0, 0, 0
        for pos, b in enumerate(seq):
            depth = sum(counters[t][pos])
            depth_sum += depth
            stats["max_depth"] = max(stats["max_depth"], depth)
            if pos > 0 and (t, pos) in events:
                letters = insertion(events[(t, pos)], sum(counters[t][pos - 1]), depth, p["min_depth"])
                if letters:
                    out.append(letters)
                    ins += 1
                    stats["ins_applied"] += 1
                    stats["bases_inserted"] += len(letters)
            kind, emitted = call(counters[t][pos], b, p["min_depth"])
            stats["pos_" + kind] += 1
            subs += kind == "substituted"
            dels += kind == "deleted"
            out.append(emitted)
        bases = b"".join(out)
        records.append((len(seq), len(bases), subs, dels, ins, depth_sum * 100 // len(seq) if seq else 0))
        text.append(fasta(name, bases))
    text = b"".join(text)
    stats["bytes_out"] = len(text)
    return dict(stats, text=text, records=records, voters=voting)
