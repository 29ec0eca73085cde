"""Edge inputs of the polishing stage (msgpu_polish.hip), built against the way its kernels are written and shared by
tests/test_polish_edges_host.py and tests/test_gpu_polish_edges.py.  ``cases()`` maps a name to a case of tests/plcases.py (draft,
reads, chains, runs, params, note; a ranked case also ``ranks`` and ``min_mapq``) with one more key, ``lit``: the polished bases of
every draft record (``bases``), written by construction from the draft's bytes, the counts of pl_oracle.COUNTS that the case
exists for, where it matters the whole output (``text``) and the records' mean depths x 100 (``depth_x100``).  No literal is
computed by the restatement.  ``expected(name)`` is the restatement's result (pl_oracle.run, pl_rank_oracle.run for a ranked
case), once per process.  ``note`` names what in the kernels the case aims at.  Every kernel of the stage launches blocks of
256 threads, so "a block" below is 256 chains, reads, records, runs, events or columns.

Blocks:     chains_300, chains_600_interleaved, span_1_chains, spans_on_block_edges, records_300, reads_300_sparse
Insertions: ins_in_second_record, events_256, events_300_one_group, events_two_groups_across_a_block, ins_32_top_bits,
            ins_32_low_bits, ins_32_sign_bit, ins_64_and_65_letters, ins_before_deleted, ins_behind_deleted, ins_adjacent_runs,
            ins_left_depth_decides, ins_right_depth_decides, ins_left_depth_enough, ins_right_depth_enough
Rules 2, 3, 5, 7: scores_negative, identity_bounds_100, identity_bounds_0, identity_bounds_50, strand_1_lower_case,
            strand_1_lower_case_ins, draft_n_corrected, draft_n_tie, other_votes_only, min_depth_huge, out_60, out_60_inserted,
            out_120, out_61, d_at_chain_ends
Ranked:     ranked_300, ranked_two_primaries_overlap
``violations()``: the 600-chain table broken in one place (rule 1); ``planted_three_records()``: a four-record draft for
polish.run.

reads_300_sparse has 301 read records: reads 0 .. 299, of which 0, 255, 256 and 299 alone have chains, and one more behind them,
so that the last read of the file has no chain although read 299 has one."""
import collections
import functools

import map_oracle
import map_rank_oracle
import pl_oracle
import pl_rank_oracle
import plcases

AT = 50          # where most cases edit their 130-base draft
MIN_MAPQ = 30    # the ranked cases' threshold: a chain of 7 anchors has mapq 42, one of 3 anchors has 18
TOP = 2**32 - 1  # the greatest matches / block of a chain


def o(seq, p):
    """the letter that plcases.aligned's ("X", 1) puts at position p"""
    return bytes([plcases.other(seq[p])])


def wrap(name, bases):
    """rule 7, by hand: lines of 60, no empty line behind a full one, an empty line for a record without bases"""
    if not bases:
        return b">" + name + b"\n\n"
    return b">" + name + b"\n" + b"".join(bases[x:x + 60] + b"\n" for x in range(0, len(bases), 60))


@functools.lru_cache(maxsize=None)
def _genome():
    return plcases._g(20000, 78)


def _u():
    return bytes(plcases._g(8000, 77)[200:330])  # the draft of plcases.hand_cases


def _add(c, name, draft, scripts, lit, note, params=None):
    c[name] = dict(plcases.case(draft, scripts, params, note), lit=lit)


def whole(*mid):
    """a script over all 130 bases: '=' up to AT, ``mid``, '=' to the end"""
    used = sum(arg if op in ("X", "D") else len(arg) if op in ("x", "e") else 0 for op, arg in mid)
    return [("=", AT)] + list(mid) + [("=", 130 - AT - used)]


SAME = (0, 0, [("=", 130)])
SUB = (0, 0, whole(("X", 1)))


def ins(letters):
    return (0, 0, whole(("I", letters)))


# ---- blocks -------------------------------------------------------------------------------------------------------------

def _block_cases(c):
    u = _u()
    sub_u = u[:AT] + o(u, AT) + u[AT + 1:]
    voters = [SAME if n % 3 == 2 else SUB for n in range(300)]
    _add(c, "chains_300", u, voters, dict(bases=[sub_u], max_depth=300, n_voters=300, n_ignored=0, cols_x=200, pos_substituted=1),
         "k_pl_check_chain, k_pl_voter_key / _idx and k_pl_spans over two blocks; wave_count on the 44 live lanes of the second")
    both = []
    for n, v in enumerate(voters):
        both += [dict(t=0, ts=0, script=v[2], score=100), dict(t=0, ts=0, script=[("X", 130)], read=n, score=90)]
    _add(c, "chains_600_interleaved", u, both,
         dict(bases=[sub_u], n_chains=600, n_voters=300, n_ignored=300, cols_x=200, max_depth=300, pos_substituted=1),
         "span[i] = 0 between voters in every block: the scan of the spans and k_pl_pileup's search pass over every second chain; "
         "a non-voter's 130 X columns reach no counter")
    _add(c, "span_1_chains", u, [(0, n % 130, [("X", 1)]) for n in range(390)],
         dict(bases=[bytes(plcases.other(b) for b in u)], max_depth=3, n_voters=390, cols_x=390, cols_eq=0, pos_substituted=130,
              depth_x100=[300]),
         "every column is a chain of its own: last_le over S ends on every lane, a == u in the search over T")
    w = bytes(_genome()[1000:1600])
    spans = [
        (0, 0, [("=", 100), ("X", 1), ("=", 50), ("D", 1), ("=", 40), ("I", b"GT"), ("=", 64)]),  # 256 columns: block 0
        (0, 256, [("X", 1), ("=", 62), ("X", 1)]),                                                  # 64: lanes 0 .. 63 of block 1
        (0, 320, [("X", 1)]),                                                                       # 1
        (0, 321, [("X", 1), ("=", 253), ("X", 1)]),                                                 # 255: up to lane 63 of block 2
        (0, 343, [("=", 232), ("X", 1), ("=", 23), ("X", 1)]),                                      # 257: block 3 and one lane
    ]
    text = (w[:100] + o(w, 100) + w[101:151] + w[152:192] + b"GT" + w[192:256] + o(w, 256) + w[257:319] + o(w, 319) + o(w, 320) +
            o(w, 321) + w[322:575] + o(w, 575) + w[576:599] + o(w, 599))
    _add(c, "spans_on_block_edges", w, spans,
         dict(bases=[text], n_voters=5, cols_x=8, cols_d=1, cols_i=2, cols_eq=256 + 64 + 1 + 255 + 257 - 9, ins_applied=1,
              pos_substituted=7, pos_deleted=1, max_depth=2),
         "spans of 256, 64, 1, 255 and 257 columns: chains begin on lane 0 and end on lane 255 of k_pl_pileup's blocks",
         dict(min_depth=1))

    g = _genome()
    draft, p = [], 2000
    for r in range(300):
        n = r % 131
        draft.append((b"d%d" % r, bytes(g[p:p + n])))
        p += n
    seq = lambda r: draft[r][1]
    scripts = ([(1, 0, [("X", 1)])] * 3 +
               [(255, 0, [("=", 10), ("X", 1), ("=", 113)])] * 2 + [(255, 0, [("=", 124)])] +
               [(256, 0, [("D", 1), ("=", 124)])] * 2 + [(256, 0, [("=", 125)])] +
               [(299, 0, [("=", 36), ("I", b"AC"), ("=", 1)])] * 2 + [(299, 0, [("=", 37)])])
    out = [s for _, s in draft]
    out[1] = o(seq(1), 0)
    out[255] = seq(255)[:10] + o(seq(255), 10) + seq(255)[11:]
    out[256] = seq(256)[1:]
    out[299] = seq(299)[:36] + b"AC" + seq(299)[36:]
    _add(c, "records_300", draft, scripts,
         dict(bases=out, pos_substituted=2, pos_deleted=1, ins_applied=1, bases_inserted=2, max_depth=3,
              pos_verbatim=sum(len(s) for _, s in draft) - 1 - 124 - 125 - 37),
         "pl_record's search and k_pl_reclen over 300 records in two blocks, records of length 0, 1 and 60; rec_sub / rec_del / "
         "rec_ins beyond row 255")

    with_chain = {0: SUB, 255: SUB, 256: SUB, 299: SAME}
    scripts = [with_chain[q] if q in with_chain else dict(bases=bytes(g[q:q + q % 7])) for q in range(301)]
    _add(c, "reads_300_sparse", u, scripts,
         dict(bases=[sub_u], n_chains=4, n_voters=4, max_depth=4, cols_x=3, pos_substituted=1, pos_verbatim=0),
         "vkey[query] and vidx[query] at 255, 256 and 299, Q.off / Q.len of empty read records, a last read without a chain; "
         "at min_depth = 4 every one of the four voters is needed", dict(min_depth=4))


# ---- insertion events ---------------------------------------------------------------------------------------------------

def _tie_32(first, second):
    """plcases' ins_tie_shorter with two 32-letter candidates: ``first`` stands first in table order"""
    voter = lambda letters: (0, AT, [("I", b"G"), ("I", letters), ("=", 130 - AT)])
    return [voter(first)] * 2 + [voter(second)] * 2 + [SAME] * 3


def _insertion_cases(c):
    u = _u()
    G = _genome()
    ac = u[:AT] + b"AC" + u[AT:]
    r0, r1 = bytes(G[200:330]), bytes(G[330:420])
    events = (1, 0, [("=", 1), ("I", b"AC"), ("=", 44), ("I", b"G"), ("=", 44), ("I", b"TT"), ("=", 1), ("I", b"CA"), ("I", b"G")])
    _add(c, "ins_in_second_record", [(b"first", r0), (b"second", r1)], [SAME] * 3 + [events, events, (1, 0, [("=", 90)])],
         dict(bases=[r0, r1[:1] + b"AC" + r1[1:45] + b"G" + r1[45:89] + b"TT" + r1[89:]], ins_applied=3, ins_usable=8, ins_at_ends=2,
              bases_inserted=5, max_depth=3),
         "(R.off[target] + p) << 6 | L, best[] and pos > R.off[r] with R.off != 0: events at slots 1, 45 and tlen - 1 of record 1, "
         "and one at slot tlen; record 0 has depth 3 at the same slots and takes nothing")
    _add(c, "events_256", u, [ins(b"AC")] * 256 + [SAME] * 44,
         dict(bases=[ac], ins_usable=256, ins_applied=1, bases_inserted=2, max_depth=300, cols_i=512),
         "n_ev == 256: k_stage_seg_starts' thread n is alone in a second block; one group that fills a block")
    _add(c, "events_300_one_group", u, [ins(b"AC")] * 300, dict(bases=[ac], ins_usable=300, ins_applied=1, bases_inserted=2),
         "one group of 300 equal events across the block boundary of k_pl_heads and k_stage_seg_starts")
    _add(c, "events_two_groups_across_a_block", u, [ins(b"AC")] * 200 + [ins(b"A")] * 100,
         dict(bases=[ac], ins_usable=300, ins_applied=1, bases_inserted=2),
         "sorted, 100 events A stand before 200 events AC: the head of the second group is event 100, its end is in block 1")
    s = bytes(G[400:432])
    for name, win, lose, note in (
            ("ins_32_top_bits", b"G" + s[1:], b"T" + s[1:], "bits 63:62 of ev_seq alone differ: a sort over fewer than 64 bits"),
            ("ins_32_low_bits", s[:31] + b"A", s[:31] + b"C", "bits 1:0 of ev_seq alone differ"),
            ("ins_32_sign_bit", b"C" + s[1:], b"G" + s[1:], "bit 63 differs: a signed compare of ev_seq")):
        _add(c, name, u, _tie_32(lose, win), dict(bases=[u[:AT] + win + u[AT:]], ins_usable=4, ins_applied=1, bases_inserted=32),
             note + "; the loser stands first in table order, so a stable sort that misses the bits keeps it first")
    l64, l65 = bytes(G[500:564]), bytes(G[600:665])
    _add(c, "ins_64_and_65_letters", u, [(0, 0, [("=", 40), ("I", l64), ("=", 40), ("I", l65), ("=", 50)])] * 3,
         dict(bases=[u], ins_unusable=6, ins_usable=0, cols_i=3 * 129, ins_applied=0),
         "L = 64 and 65 do not fit the key's 6 bits: L <= 32 is asked before a key is made")
    _add(c, "ins_before_deleted", u, [(0, 0, [("=", 50), ("I", b"AC"), ("D", 1), ("=", 79)])] * 2 + [SAME],
         dict(bases=[u[:50] + b"AC" + u[51:]], ins_applied=1, pos_deleted=1),
         "outlen = ins_len + 0: k_pl_scatter writes the letters and no call behind them")
    _add(c, "ins_behind_deleted", u, [(0, 0, [("=", 49), ("D", 1), ("I", b"AC"), ("=", 80)])] * 2 + [SAME],
         dict(bases=[u[:49] + b"AC" + u[50:]], ins_applied=1, pos_deleted=1),
         "the slot's left neighbour is deleted: its depth (del votes with the rest) still counts")
    _add(c, "ins_adjacent_runs", u, [(0, 0, [("=", 50), ("I", b"C"), ("I", b"A"), ("=", 80)])] * 2 + [SAME],
         dict(bases=[u[:50] + b"A" + u[50:]], ins_usable=4, ins_applied=1, bases_inserted=1),
         "two I runs side by side: four events at one slot in two groups of two, the smaller letter wins")
    event = (0, 40, [("=", 10), ("I", b"AC"), ("=", 10)])
    left, right = (0, 0, [("=", 50)]), (0, 50, [("=", 80)])
    for name, extra, text, applied in (("ins_left_depth_decides", [right], u, 0), ("ins_right_depth_decides", [left], u, 0),
                                       ("ins_left_depth_enough", [right, left], ac, 1), ("ins_right_depth_enough", [left, right], ac, 1)):
        _add(c, name, u, [event, event] + extra, dict(bases=[text], ins_usable=2, ins_applied=applied, max_depth=3),
             "m = min(depth(p - 1), depth(p)) against min_depth with 2 and 3 on either side of slot 50")


# ---- rules 2, 3, 5 and 7 ------------------------------------------------------------------------------------------------

def _scores_negative(u):
    """four pairs of equal reads, pair k on [30 k, 30 k + 30): the winning chain has its X at + 10, the other at + 20"""
    p10, p20 = [("=", 10), ("X", 1), ("=", 19)], [("=", 20), ("X", 1), ("=", 9)]
    scripts = []
    for k, scores in enumerate(((-5, -3), (0, -1), (-2**31, -2**31 + 1), (-2**31,))):
        ts, win = 30 * k, scores.index(max(scores))
        parts = [p10 if j == win else p20 for j in range(len(scores))]
        seqs = [plcases.aligned(u, ts, p)[0] for p in parts]
        for copy in range(2):
            q = 2 * k + copy
            first = dict(t=0, ts=ts, script=parts[0], score=scores[0], flanks=(b"", b"".join(seqs[1:])))
            if len(scores) == 1:
                first.update(matches=0, block=0)  # the whole voter key, score biased and block, is 0
            scripts.append(first)
            if len(scores) == 2:
                scripts.append(dict(t=0, ts=ts, script=parts[1], score=scores[1], read=q, qs=30))
    return scripts


def _identity(u, ratios):
    """three reads; the first two hold an X at 60 and have (matches, block) = ratios[0], ratios[1]"""
    x60 = [("=", 60), ("X", 1), ("=", 69)]
    return [dict(t=0, ts=0, script=x60, matches=m, block=b) for m, b in ratios] + [SAME]


def _rule_cases(c):
    u = _u()
    text = u[:10] + o(u, 10) + u[11:40] + o(u, 40) + u[41:70] + o(u, 70) + u[71:100] + o(u, 100) + u[101:]
    _add(c, "scores_negative", u, _scores_negative(u), dict(bases=[text], n_voters=8, n_ignored=6, cols_x=8, pos_substituted=4, max_depth=2),
         "score ^ 0x80000000 in the voter key: -5 < -3, -1 < 0, -2^31 < -2^31 + 1, and a key of 0 still votes", dict(min_depth=2))
    x60 = u[:60] + o(u, 60) + u[61:]
    _add(c, "identity_bounds_100", u, _identity(u, [(TOP, TOP), (TOP - 1, TOP)]), dict(bases=[u], n_voters=2, n_ignored=1, cols_x=1),
         "matches * 100 >= min_identity * block at 2^32 - 1: equal votes, one less does not (1 X against 1 '=': the draft's base)",
         dict(min_identity=100, min_depth=2))
    _add(c, "identity_bounds_0", u, _identity(u, [(0, TOP), (0, TOP)]), dict(bases=[x60], n_voters=3, n_ignored=0, cols_x=2),
         "min_identity = 0: matches = 0 votes", dict(min_identity=0, min_depth=2))
    _add(c, "identity_bounds_50", u, _identity(u, [(2**31, TOP), (2**31, TOP)]), dict(bases=[x60], n_voters=3, n_ignored=0, cols_x=2),
         "2^31 * 100 >= 50 * (2^32 - 1) holds in 64 bits; cut to 32 bits the left side is 0", dict(min_identity=50, min_depth=2))

    a = u[:AT] + b"A" + u[AT + 1:]
    rc = lambda script: dict(t=0, ts=0, script=script, strand=1)
    _add(c, "strand_1_lower_case", a, [rc(whole(("x", b"t")))] * 2 + [SAME], dict(bases=[a[:AT] + b"T" + a[AT + 1:]], pos_substituted=1),
         "pl_class complements upper case only and then folds: the stored t stays t and votes T; folding first would vote A")
    _add(c, "strand_1_lower_case_ins", u, [rc(whole(("I", b"ac")))] * 2 + [SAME], dict(bases=[u[:AT] + b"AC" + u[AT:]], ins_applied=1, bases_inserted=2),
         "the same inside an insertion: the stored ca is read as ac and inserts AC; folding first would insert TG")

    n = u[:AT] + b"N" + u[AT + 1:]
    x = lambda letter: (0, 0, whole(("x", letter)))
    _add(c, "draft_n_corrected", n, [x(b"G")] * 3, dict(bases=[u[:AT] + b"G" + u[AT + 1:]], pos_substituted=1, pos_verbatim=0),
         "own = PL_OTHER in k_pl_call: a draft N is corrected")
    _add(c, "draft_n_tie", n, [x(b"T"), x(b"C")], dict(bases=[u[:AT] + b"C" + u[AT + 1:]], pos_substituted=1), "own = PL_OTHER is never among the tied: C before T",
         dict(min_depth=2))
    _add(c, "other_votes_only", u, [x(b"N")] * 3, dict(bases=[u], pos_verbatim=1, pos_unchanged=129, max_depth=3),
         "depth 3 of 'other' votes alone: v[A] | ... | v[DEL] == 0 keeps the byte")
    _add(c, "min_depth_huge", u, [SUB, SUB, ins(b"AC"), ins(b"AC"), SAME], dict(bases=[u], pos_verbatim=130, ins_applied=0, ins_usable=2, max_depth=5),
         "min_depth = 2^31 - 1 against 32-bit depths", dict(min_depth=2**31 - 1))

    G = _genome()
    d61, d59, d121, d60 = bytes(G[3000:3061]), bytes(G[3100:3159]), bytes(G[3200:3321]), bytes(G[3400:3460])
    dele = lambda n: [(0, 0, [("=", 30), ("D", 1), ("=", n - 31)])] * 2 + [(0, 0, [("=", n)])]
    insert = lambda n: [(0, 0, [("=", 30), ("I", b"G"), ("=", n - 30)])] * 2 + [(0, 0, [("=", n)])]
    b = d61[:30] + d61[31:]
    _add(c, "out_60", d61, dele(61), dict(bases=[b], text=b">d0\n" + b + b"\n", bytes_out=65, pos_deleted=1), "61 - 1 bases: one full line")
    b = d59[:30] + b"G" + d59[30:]
    _add(c, "out_60_inserted", d59, insert(59), dict(bases=[b], text=b">d0\n" + b + b"\n", bytes_out=65, ins_applied=1), "59 + 1 bases: one full line")
    b = d121[:30] + d121[31:]
    _add(c, "out_120", d121, dele(121), dict(bases=[b], text=b">d0\n" + b[:60] + b"\n" + b[60:] + b"\n", bytes_out=126), "121 - 1 bases: two full lines")
    b = d60[:30] + b"G" + d60[30:]
    _add(c, "out_61", d60, insert(60), dict(bases=[b], text=b">d0\n" + b[:60] + b"\n" + b[60:] + b"\n", bytes_out=67), "60 + 1 bases: a second line of one base")
    _add(c, "d_at_chain_ends", u, [(0, 0, [("D", 1), ("=", 128), ("D", 1)])] * 2 + [SAME], dict(bases=[u[1:129]], pos_deleted=2, cols_d=4, ins_at_ends=0),
         "D as a chain's first and last run, at position 0 and tlen - 1: an ordinary column, unlike I")


# ---- ranked form --------------------------------------------------------------------------------------------------------

def _ranked(draft, reads, chains, runs, lit, note, params=None):
    ranks = map_rank_oracle.rank(chains)
    return dict(draft=draft, reads=reads, chains=chains, runs=runs, params=params or {}, note=note, ranks=ranks, min_mapq=MIN_MAPQ, lit=lit)


def _anchors(ch, n):
    return ch[:3] + (n,) + ch[4:]


def _ranked_cases(c):
    u = _u()
    # 150 reads, each in two chains: bases [0, 65) of the read on [0, 65) of the draft, [65, 130) on [65, 130).  Read q's id
    # modulo 4 says which of its chains have 7 anchors (mapq 42, voting) and which 3 (mapq 18): first, second, both, none.
    # A voting chain has its X at 20 (100), another at 30 (110).
    reads, chains, runs = [], [], []
    votes = ((1, 0), (0, 1), (1, 1), (0, 0))
    for q in range(150):
        parts = []
        for half, v in enumerate(votes[q % 4]):
            at = (20 if v else 30) + 80 * half
            lo = 65 * half
            seq, r, te = plcases.aligned(u, lo, [("=", at - lo), ("X", 1), ("=", lo + 65 - at - 1)])
            parts.append(seq)
            chains.append(_anchors(plcases.chain(q, 0, 130, lo, te, r, qs=lo, qe=lo + 65, score=65), 7 if v else 3))
            runs.append(r)
        reads.append((b"r%d" % q, b"".join(parts)))
    text = u[:20] + o(u, 20) + u[21:100] + o(u, 100) + u[101:]
    c["ranked_300"] = _ranked([(b"d0", u)], reads, chains, runs,
                              dict(bases=[text], n_chains=300, n_voters=150, n_ignored=150, cols_x=150, max_depth=75, pos_substituted=2, depth_x100=[7500]),
                              "k_pl_voter_ranked and pl_votes' flag over two blocks; 75 voters of 150 chains on either half")
    # read 0 in two parts whose target spans share [50, 80); both parts hold an X at 60.  Read 1 is the draft.
    a, ra, _ = plcases.aligned(u, 0, [("=", 60), ("X", 1), ("=", 19)])
    b, rb, _ = plcases.aligned(u, 50, [("=", 10), ("X", 1), ("=", 69)])
    chains = [plcases.chain(0, 0, 160, 0, 80, ra, qs=0, qe=80, score=80), plcases.chain(0, 0, 160, 50, 130, rb, qs=80, qe=160, score=79),
              plcases.chain(1, 0, 130, 0, 130, [130 << 4 | plcases.EQ], score=130)]
    chains = [_anchors(ch, 7) for ch in chains]
    c["ranked_two_primaries_overlap"] = _ranked(
        [(b"d0", u)], [(b"r0", a + b), (b"r1", u)], chains, [ra, rb, [130 << 4 | plcases.EQ]],
        dict(bases=[u[:60] + o(u, 60) + u[61:]], n_voters=3, max_depth=3, cols_x=2, pos_substituted=1, depth_x100=[100 * (80 + 80 + 130) // 130]),
        "a read votes twice where its primaries overlap on the target: 2 X against 1 '=' at 60, depth 3 on [50, 80)", dict(min_depth=2))


# ---- the cases ----------------------------------------------------------------------------------------------------------

@functools.lru_cache(maxsize=None)
def cases():
    c = collections.OrderedDict()
    _block_cases(c)
    _insertion_cases(c)
    _rule_cases(c)
    _ranked_cases(c)
    return c


def names():
    return list(cases())


def how(c):
    """the keywords of run_tables beside the tables: the parameters, and the rank rows of a ranked case"""
    return dict(c["params"], ranks=c["ranks"], min_mapq=c["min_mapq"]) if "ranks" in c else dict(c["params"])


@functools.lru_cache(maxsize=None)
def expected(name):
    c = cases()[name]
    if "ranks" in c:
        return pl_rank_oracle.run(c["draft"], c["reads"], c["chains"], c["runs"], c["ranks"], min_mapq=c["min_mapq"], **c["params"])
    return plcases.expected_tables(c)


def meets_literals(name, text, records, counts):
    """the literals of a case that an output text, a record table and the counts (by the names of pl_oracle.COUNTS) miss"""
    c = cases()[name]
    lit, bad = c["lit"], []
    want = b"".join(wrap(n, b) for (n, _), b in zip(c["draft"], lit["bases"]))
    if len(lit["bases"]) != len(c["draft"]) or text != want:
        bad.append("text: %r, not %r" % (text[:200], want[:200]))
    if "text" in lit and text != lit["text"]:
        bad.append("text: %r, not %r" % (text, lit["text"]))
    if [r[:2] for r in records] != [(len(s), len(b)) for (_, s), b in zip(c["draft"], lit["bases"])]:
        bad.append("record lengths")
    if "depth_x100" in lit and [r[5] for r in records] != lit["depth_x100"]:
        bad.append("depth x 100: %r, not %r" % ([r[5] for r in records], lit["depth_x100"]))
    for k in pl_oracle.COUNTS:
        if k in lit and counts[k] != lit[k]:
            bad.append("%s: %d, not %d" % (k, counts[k], lit[k]))
    assert set(lit) <= set(pl_oracle.COUNTS) | {"bases", "text", "depth_x100"}
    return bad


# ---- rule 1 on the 600-chain table --------------------------------------------------------------------------------------

@functools.lru_cache(maxsize=None)
def violations():
    """name -> (chains_600_interleaved broken in one or two places, rank rows or None, the chain and the entry of pl_oracle.WHAT
    -- or "rank" -- that the error must name)"""
    base = cases()["chains_600_interleaved"]
    out = {}

    def broken(name, chain, what, strand=None, more_query=None, bad_op=None, parent=None):
        c = dict(base, chains=list(base["chains"]), runs=[list(r) for r in base["runs"]])
        ranks = None
        if strand is not None:
            c["chains"][strand] = c["chains"][strand][:2] + (2,) + c["chains"][strand][3:]
        if more_query is not None:
            c["runs"][more_query].append(1 << 4 | plcases.I)
        if bad_op is not None:
            c["runs"][bad_op][-1] = c["runs"][bad_op][-1] & ~15 | 3
        if parent is not None:
            ranks = map_rank_oracle.rank(c["chains"])
            ranks[parent[0]] = (parent[1], 0, 0, 0)
        out[name] = (c, ranks, chain, what)

    broken("strand_at_599", 599, "strand", strand=599)
    broken("query_consumption_at_300", 300, "query consumption", more_query=300)
    broken("two_bad_chains_in_two_blocks", 300, "query consumption", strand=599, more_query=300)
    broken("run_op_in_the_last_run", 599, "run", bad_op=599)
    broken("rank_parent_at_299", 299, "rank", parent=(299, 300))  # chain 300 belongs to the next read
    return out


# ---- a draft of several records through the mapper ----------------------------------------------------------------------

CUTS = (7000, 14000)


@functools.lru_cache(maxsize=None)
def planted_three_records():
    """plcases.workload("planted") with its draft in three records, the middle one reverse-complemented, and a fourth record
    of 500 bases that no read maps to -> dict: ``draft`` and ``reads`` (FASTA bytes), ``unmapped`` (the fourth record's bases)"""
    from muchsalsa_amd import synth
    wl = plcases.workload("planted")
    (_, d), = map_oracle.parse(wl["draft"], False)
    unmapped = synth.genome_bases(500, 99).tobytes()
    recs = [(b"left", d[:CUTS[0]]), (b"middle", map_oracle.revcomp(d[CUTS[0]:CUTS[1]])), (b"right", d[CUTS[1]:]), (b"unmapped", unmapped)]
    return dict(draft=plcases.fasta(recs), reads=wl["reads"], unmapped=unmapped)


@functools.lru_cache(maxsize=None)
def expected_planted_three_records():
    """(pl_oracle's result, the cigar result) of one round in the restatement"""
    wl = planted_three_records()
    return plcases.polish_round(wl["draft"], wl["reads"])
