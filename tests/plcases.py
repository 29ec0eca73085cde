"""Inputs of the polishing stage's tests, shared by the host and the GPU file: hand-made tables (the smallest shapes at which
the kernels can go wrong), the tables that break rule 1, and the two workloads that go through the mapper; the restatement's
result for each is computed once per process.

A hand case is a dict: ``draft`` and ``reads`` ([(name, bases)]), ``chains`` (the tuples of msgpu_map_chain), ``runs`` (per
chain the list of len << 4 | op), ``params`` and ``note``."""
import functools
import os

import map_cigar_oracle
import map_oracle
import pl_oracle

I, D, EQ, X = pl_oracle.OP_I, pl_oracle.OP_D, pl_oracle.OP_EQ, pl_oracle.OP_X


def _g(n, seed):
    from muchsalsa_amd import synth
    return synth.genome_bases(n, seed).tobytes()


def fasta(recs):
    return b"".join(b">%s\n%s\n" % (n, s) for n, s in recs)


def other(b, step=1):
    return b"ACGT"[(b"ACGT".index(bytes([b]).upper()) + step) % 4]


def aligned(draft, ts, script):
    """a read that aligns to draft[ts:] by ``script`` -- ("=", n), ("X", n) (every base replaced by the next letter), ("x", letters)
    (replaced by these), ("e", letters) (an '=' run over these letters, whatever they are), ("I", letters), ("D", n) -> (the read, its runs, t_end)"""
    read, runs, p = [], [], ts
    for op, arg in script:
        if op == "=":
            read.append(draft[p:p + arg])
            runs.append(arg << 4 | EQ)
            p += arg
        elif op == "X":
            read.append(bytes(other(b) for b in draft[p:p + arg]))
            runs.append(arg << 4 | X)
            p += arg
        elif op in ("x", "e"):
            read.append(arg)
            runs.append(len(arg) << 4 | (X if op == "x" else EQ))
            p += len(arg)
        elif op == "I":
            read.append(arg)
            runs.append(len(arg) << 4 | I)
        else:
            runs.append(arg << 4 | D)
            p += arg
    return b"".join(read), runs, p


def chain(q, t, qlen, ts, te, runs, strand=0, qs=0, qe=None, score=100, matches=None, block=None):
    qe = qlen if qe is None else qe
    m = sum(r >> 4 for r in runs if r & 15 == EQ)
    b = sum(r >> 4 for r in runs)
    return (q, t, strand, 3, score, b - m, qs, qe, ts, te, m if matches is None else matches, b if block is None else block)


def case(draft, scripts, params=None, note="", names=None):
    """``scripts``: per read (target record, t_start, script) or a dict with more: strand, flanks (bases put around the read),
    score, matches, block, read (the index of an earlier read that this chain belongs to; qs: where in that read the chain
    starts, 0 if it is not given); a dict with ``bases`` alone is a read record without a chain"""
    if isinstance(draft, bytes):
        draft = [(b"d0", draft)]
    reads, chains, runs = [], [], []
    for n, s in enumerate(scripts):
        s = s if isinstance(s, dict) else dict(t=s[0], ts=s[1], script=s[2])
        if "bases" in s:
            reads.append((b"r%d" % len(reads), s["bases"]))
            continue
        seq, r, te = aligned(draft[s["t"]][1], s["ts"], s["script"])
        left, right = s.get("flanks", (b"", b""))
        if "read" in s:
            q = s["read"]  # a further chain of an earlier read: its columns read that read's first bytes, whatever the script says
            assert not left and not right and s.get("qs", 0) + len(seq) <= len(reads[q][1]) and not s.get("strand")
            left = reads[q][1][:s.get("qs", 0)]
        else:
            q = len(reads)
            whole = left + seq + right
            reads.append((b"r%d" % q, map_oracle.revcomp(whole) if s.get("strand") else whole))
        qlen = len(reads[q][1])
        qs, qe = (len(left), len(left) + len(seq)) if not s.get("strand") else (len(right), len(right) + len(seq))
        chains.append(chain(q, s["t"], qlen, s["ts"], te, r, strand=s.get("strand", 0), qs=qs, qe=qe, score=s.get("score", 100),
                            matches=s.get("matches"), block=s.get("block")))
        runs.append(r)
    order = sorted(range(len(chains)), key=lambda i: chains[i][0])  # rule 1: by query record (stable)
    return dict(draft=draft, reads=reads, chains=[chains[i] for i in order], runs=[runs[i] for i in order], params=params or {},
                note=note)


@functools.lru_cache(maxsize=None)
def hand_cases():
    G = _g(8000, 77)
    d = bytearray(G[:130])
    d[7] |= 0x20
    d[64] |= 0x20
    d[65] = ord("N")
    d[129] |= 0x20
    d = bytes(d)  # 130 bases: two wavefront widths and three FASTA lines are crossed; lower case and an N
    u = bytes(G[200:330])
    at = 50
    g_at = bytearray(u)
    g_at[at] = ord("G")
    g_at = bytes(g_at)
    whole = lambda *mid: [("=", at)] + list(mid)
    rest = lambda used: [("=", 130 - at - used)]
    same = (0, 0, [("=", 130)])
    sub = (0, 0, whole(("X", 1)) + rest(1))
    dele = (0, 0, whole(("D", 1)) + rest(1))
    ins = lambda letters: (0, 0, whole(("I", letters)) + rest(0))
    ins32, ins33 = bytes(G[400:432]), bytes(G[500:533])
    big = bytearray(G[1000:7000])
    big[10] |= 0x20
    big = bytes(big)
    long_read = bytearray(big[500:5500])
    for p in (0, 63, 64, 255, 256, 2500, 4999):
        long_read[p] = other(long_read[p])
    many = []
    for n in range(66):
        many += [("=", 3 + n % 4), ("X", 1), ("=", 2), ("D", 1 + n % 2), ("=", 4), ("I", bytes(G[7000 + n:7001 + n + n % 3]))]
    many = many[:199] + [("=", 5)]
    two = [(b"first", bytes(G[200:330])), (b"second desc", bytes(G[330:420]))]
    gone = [(b"kept", bytes(G[200:290])), (b"gone", bytes(G[300:370]))]
    return {
        "identity": case(d, [same] * 3, note="three identical reads: the output is the draft's bytes"),
        "identity_reads_differ_in_case": case(d, [(0, 0, [("x", d.swapcase())])] * 3, note="case folding on both sides"),
        "sub_2of3": case(u, [sub, sub, same], note="a substitution by 2 of 3"),
        "tie_draft": case(u, [sub, same], dict(min_depth=2), "a 1:1 tie with the draft's base among the tied"),
        "tie_others": case(g_at, [(0, 0, whole(("x", b"T")) + rest(1)), (0, 0, whole(("x", b"C")) + rest(1))], dict(min_depth=2),
                           "a tie between two bases that are not the draft's: C before T"),
        "del_wins": case(u, [dele, dele, same], note="a deletion by 2 of 3"),
        "del_ties_draft": case(u, [dele, same], dict(min_depth=2), "a deletion tying with the draft's base"),
        "del_ties_other": case(u, [dele, sub], dict(min_depth=2), "a deletion tying with another base: the base comes first"),
        "ins_2of3": case(u, [ins(b"AC"), ins(b"AC"), same], note="AC inserted by 2 of 3"),
        "ins_1of2": case(u, [ins(b"AC"), same], dict(min_depth=2), "an insertion by 1 of 2 is no majority"),
        "ins_3_against_1": case(u, [ins(b"AC")] * 3 + [ins(b"A")], note="two competing insertions, one with the majority"),
        "ins_equal_counts": case(u, [ins(b"AC")] * 2 + [ins(b"A")] * 2, note="equal counts are no majority of the depth"),
        # the events' voters start at the slot (an I at the chain's start, which is ignored, then the event), so the depth left
        # of the slot is that of the three other reads alone: 2 * 2 > 3, and of the two candidates the shorter wins
        "ins_tie_shorter": case(u, [(0, at, [("I", b"G"), ("I", b"AC")] + rest(0))] * 2 + [(0, at, [("I", b"G"), ("I", b"T")] + rest(0))] * 2 +
                                [same] * 3, note="two lengths with equal counts: the shorter wins"),
        "ins_tie_letters": case(u, [(0, at, [("I", b"G"), ("I", b"CA")] + rest(0))] * 2 + [(0, at, [("I", b"G"), ("I", b"AT")] + rest(0))] * 2 +
                                [same] * 3, note="equal counts and lengths: the smaller packed letters win"),
        "ins_32_and_33": case(u, [(0, 0, [("=", 40), ("I", ins32), ("=", 40), ("I", ins33), ("=", 50)])] * 2 + [same],
                              note="32 letters are usable, 33 are not"),
        "ins_with_n": case(u, [ins(b"ANC"), ins(b"ANC"), same], note="an N inside an insertion"),
        "ins_lower_case": case(u, [ins(b"ac"), ins(b"Ac"), same], note="lower case inside an insertion is folded"),
        "ins_at_ends": case(u, [(0, 10, [("I", b"AC"), ("=", 100), ("I", b"GT")])] * 3, note="an I as first and as last run"),
        "ins_at_record_edges": case(u, [(0, 0, [("I", b"A"), ("I", b"CC"), ("=", 130), ("I", b"GG"), ("I", b"T")])] * 3,
                                    note="usable events at slot 0 and at slot tlen are never applied"),
        "depth_edge": case(u, [(0, 0, [("=", 20), ("X", 1), ("=", 40), ("X", 1), ("=", 68)])] * 2 + [(0, 40, [("=", 21), ("X", 1), ("=", 68)])],
                           note="depth min_depth - 1 next to depth min_depth: only the second substitution is made"),
        "strand_1": case(u, [dict(t=0, ts=5, script=[("=", 30), ("X", 2), ("=", 10), ("I", b"ACG"), ("=", 20), ("D", 2), ("=", 40)], strand=1,
                                  flanks=(b"TTTTT", b"GGGGGGG"))] * 2 + [same], note="strand-1 voters with flanks"),
        "flanks": case(u, [dict(t=0, ts=5, script=[("=", 30), ("X", 2), ("=", 70)], flanks=(b"ACGTA", b"CC"))] * 2 + [same],
                       note="q_start > 0 and q_end < qlen"),
        "two_chains_equal": case(u, [dict(t=0, ts=0, script=whole(("X", 1)) + rest(1)), dict(t=0, ts=0, script=whole(("X", 1)) + rest(1), read=0),
                                     sub, same, same], note="a read with two chains of equal score and block votes once"),
        "two_chains_unequal": case(u, [dict(t=0, ts=0, script=[("=", 130)], score=90), dict(t=0, ts=at, script=[("X", 1), ("=", 20)], read=0, score=95),
                                       sub, same], dict(min_depth=2), "the chain with the greater score votes, wherever it stands"),
        "two_chains_block": case(u, [dict(t=0, ts=at, script=[("X", 1), ("=", 20)], flanks=(b"", u[:120])), dict(t=0, ts=0, script=[("=", 130)], read=0), sub, same],
                                 dict(min_depth=2), "equal scores: the greater block votes"),
        "min_identity": case(u, [dict(t=0, ts=0, script=whole(("X", 1)) + rest(1), matches=89, block=100),
                                 dict(t=0, ts=0, script=whole(("X", 1)) + rest(1), matches=90, block=100), same],
                             dict(min_identity=90, min_depth=2), "min_identity cuts one voter: the substitution has 1 of 2, not 2 of 3"),
        "long_run": case(big, [(0, 500, [("e", bytes(long_read))])], dict(min_depth=1), "one run of 5,000 columns on 6,000 bases"),
        "many_runs": case(bytes(G[1000:2200]), [(0, 17, many)], dict(min_depth=1), "one chain of 200 runs"),
        "two_records": case(two, [(1, 0, [("=", 30), ("X", 1), ("=", 59)])] * 3, note="two records, the first without voters"),
        "all_deleted": case(gone, [dict(t=1, ts=0, script=[("D", 70)], flanks=(b"ACGT", b"TT"))] * 3 + [(0, 0, [("=", 90)])] * 3, note="a record whose every base is deleted"),
        "zero_chains": case(two, [], note="no chains"),
    }


HAND = tuple(hand_cases())


@functools.lru_cache(maxsize=None)
def violations():
    """name -> (a case that breaks rule 1, the chain and the entry of pl_oracle.WHAT that the error must name)"""
    base = hand_cases()["strand_1"]
    assert len(base["chains"]) == 3
    out = {}

    def broken(name, chain_index, what, field=None, value=None, runs=None):
        c = dict(base, chains=list(base["chains"]), runs=[list(r) for r in base["runs"]])
        if field is not None:
            ch = list(c["chains"][chain_index])
            ch[field] = value
            c["chains"][chain_index] = tuple(ch)
        if runs is not None:
            c["runs"][chain_index] = runs
        out[name] = (c, chain_index, what)

    r1 = base["runs"][1]
    tlen = len(base["draft"][0][1])
    broken("query_order", 2, "query order", 0, 0)
    broken("strand", 1, "strand", 2, 2)
    broken("query_record", 2, "query record", 0, 3)
    broken("target_record", 0, "target record", 1, 1)
    broken("t_end_beyond", 1, "target range", 9, tlen + 1)
    broken("t_start_at_end", 1, "target range", 8, base["chains"][1][9])
    broken("q_end_beyond", 1, "query range", 7, len(base["reads"][1][1]) + 1)
    broken("q_start_behind_end", 1, "query range", 6, base["chains"][1][7] + 1)
    broken("run_length_0", 1, "run", runs=r1[:2] + [0 << 4 | EQ] + r1[2:])
    broken("run_op", 1, "run", runs=[r1[0] & ~15 | 3] + r1[1:])
    broken("target_short", 1, "target consumption", runs=r1[:-1] + [r1[-1] - 16])  # (both sides fall short: the target is named)
    broken("query_long", 1, "query consumption", runs=r1 + [1 << 4 | I])
    broken("no_runs", 0, "target consumption", runs=[])
    # two bad chains: the smaller index is named, whatever the other breaks
    c = dict(base, chains=list(base["chains"]), runs=[list(r) for r in base["runs"]])
    c["chains"][2] = c["chains"][2][:2] + (7,) + c["chains"][2][3:]
    c["runs"][1] = r1 + [1 << 4 | I]
    out["two_bad_chains"] = (c, 1, "query consumption")
    return out


def write_case(c, directory):
    """the case's files in ``directory`` -> (draft path, reads path)"""
    dp, rp = os.path.join(str(directory), "draft.fa"), os.path.join(str(directory), "reads.fa")
    with open(dp, "wb") as f:
        f.write(fasta(c["draft"]))
    with open(rp, "wb") as f:
        f.write(fasta(c["reads"]))
    return dp, rp


def expected_tables(c):
    """pl_oracle.run on a hand case; the names of a draft are cut at the first whitespace, as the stage cuts them"""
    draft = [(n.split()[0] if n.split() else b"", s) for n, s in c["draft"]]
    return pl_oracle.run(draft, c["reads"], c["chains"], c["runs"], **c["params"])


@functools.lru_cache(maxsize=None)
def expected_hand(name):
    return expected_tables(hand_cases()[name])


# ---- through the mapper

GENOME, N_READS, READ_LEN, EVERY = 20000, 40, 3000, 150
PLANTED = dict(seed=5, error=0.0)
NOISY = dict(seed=5, error=0.06)


@functools.lru_cache(maxsize=None)
def workload(name):
    """-> dict: ``genome`` (the truth), ``draft`` (FASTA bytes: the genome with one substitution, insertion or deletion of 1-3 bases
    about every EVERY bases), ``reads`` (FASTA bytes: N_READS reads of READ_LEN genome bases on both strands; ``planted``:
    error-free, ``noisy``: the long-read error model at 6 %)"""
    from muchsalsa_amd import synth
    shape = dict(planted=PLANTED, noisy=NOISY)[name]
    g = synth.genome_bases(GENOME, shape["seed"])
    n = GENOME // EVERY
    at = synth._randint(shape["seed"], 201, n, 20, EVERY - 20)
    kind = synth._randint(shape["seed"], 202, n, 0, 2)
    size = synth._randint(shape["seed"], 203, n, 1, 3)
    letters = synth._randint(shape["seed"], 204, 3 * n, 0, 3)
    draft, p = [], 0
    for i in range(n):
        q = i * EVERY + int(at[i])
        draft.append(g[p:q].tobytes())
        if kind[i] == 0:  # substitution
            draft.append(bytes(other(b, 1 + int(letters[3 * i + j]) % 3) for j, b in enumerate(g[q:q + size[i]].tobytes())))
            p = q + int(size[i])
        elif kind[i] == 1:  # insertion into the draft
            draft.append(bytes(b"ACGT"[int(x)] for x in letters[3 * i:3 * i + int(size[i])]))
            p = q
        else:  # deletion from the draft
            p = q + int(size[i])
    draft.append(g[p:].tobytes())
    recs, _, _ = synth._long_reads(g, N_READS, READ_LEN, shape["seed"] + 1, shape["error"], 0.0005 if shape["error"] else 0.0,
                                   0.001 if shape["error"] else 0.0, False)
    return dict(genome=g.tobytes(), draft=fasta([(b"draft", b"".join(draft))]), reads=b"".join(recs))


def write_workload(name, directory):
    wl = workload(name)
    dp, rp = os.path.join(str(directory), "draft.fa"), os.path.join(str(directory), "reads.fa")
    with open(dp, "wb") as f:
        f.write(wl["draft"])
    with open(rp, "wb") as f:
        f.write(wl["reads"])
    return dp, rp


def polish_round(draft_text, reads_text, **params):
    """one round in the restatement: map_oracle / map_cigar_oracle, then pl_oracle -> (pl_oracle's result, the cigar result)"""
    draft, reads = map_oracle.parse(draft_text, False), map_oracle.parse(reads_text, False)
    mapped = map_cigar_oracle.cigar_run(draft, reads)
    return pl_oracle.run(draft, reads, mapped["chains"], mapped["packed"], **params), mapped


@functools.lru_cache(maxsize=None)
def expected_workload(name):
    wl = workload(name)
    return polish_round(wl["draft"], wl["reads"])
