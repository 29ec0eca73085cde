"""The edge cases of the polishing stage (tests/pledgecases.py), host side (no GPU): the restatements (tests/pl_oracle.py,
tests/pl_rank_oracle.py) give every hand-derived literal, both the bases of every record and the counts, and every condition
that keeps tests/test_gpu_polish_edges.py from passing on nothing holds -- the sizes cross the block of 256 they were built to
cross, the events number what they should, the candidates differ in the bits named, the voters alternate where they should."""
import os
import time

import pytest

import map_oracle
import pl_oracle
import pl_rank_oracle
import plcases
import pledgecases as P

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
I, D, EQ, X = plcases.I, plcases.D, plcases.EQ, plcases.X
BLOCK = 256  # threads of every kernel's workgroup


# ---- the lists ----------------------------------------------------------------------------------------------------------

def test_the_gpu_file_runs_these_cases_and_leaves_none_out():
    import test_gpu_polish_edges as G
    assert G.CASES == P.names() and G.VIOLATIONS == sorted(P.violations()) and P.cases() is P.cases()
    assert len(P.names()) == len(set(P.names())) == 38
    for name in ("test_gpu_polish_edges.py", "test_polish_edges_host.py", "pledgecases.py"):
        with open(os.path.join(ROOT, "tests", name)) as f:
            text = f.read()
        assert "sk" "ip" not in text and "xf" "ail" not in text, name


@pytest.mark.parametrize("name", P.names())
def test_the_restatement_gives_the_literals(name):
    c = P.cases()[name]
    t0 = time.perf_counter()
    want = P.expected(name)
    assert time.perf_counter() - t0 < 2
    assert P.meets_literals(name, want["text"], want["records"], want) == []
    assert c["note"] and len(c["lit"]) >= 2
    assert len(plcases.fasta(c["draft"])) + len(plcases.fasta(c["reads"])) + 48 * len(c["chains"]) + 4 * sum(len(r) for r in c["runs"]) < 1000000
    assert want["cols_eq"] + want["cols_x"] + want["cols_d"] <= 39000  # the largest pile-up
    if "ranks" in c:  # the rank rows are the mapper's rule 12 on this table
        import map_rank_oracle
        map_rank_oracle.invariants(c["chains"], c["ranks"])
    assert P.wrap(b"x", b"") == b">x\n\n" == pl_oracle.fasta(b"x", b"")


def _events(name):
    """the usable events of a case at slots 0 < p < tlen, as (record, slot, L, packed) in table order"""
    c = P.cases()[name]
    out = []
    for i in P.expected(name)["voters"]:
        ch, runs = c["chains"][i], c["runs"][i]
        oq = pl_oracle.oriented(c["reads"][ch[0]][1], ch[2])
        j, p = ch[6] if ch[2] == 0 else len(oq) - ch[7], ch[8]
        for n, r in enumerate(runs):
            ln, op = r >> 4, r & 15
            if op == I:
                letters = oq[j:j + ln]
                if 0 < n < len(runs) - 1 and ln <= 32 and all(b in pl_oracle.CLASS for b in letters) and 0 < p < len(c["draft"][ch[1]][1]):
                    packed = 0
                    for b in letters:
                        packed = packed << 2 | pl_oracle.CLASS[b]
                    out.append((ch[1], p, ln, packed))
            if op != I:
                p += ln
            if op != D:
                j += ln
    return out


# ---- blocks -------------------------------------------------------------------------------------------------------------

def test_block_conditions():
    c = P.cases()
    for name in ("chains_300", "chains_600_interleaved", "span_1_chains", "ranked_300"):
        assert len(c[name]["chains"]) > BLOCK and len(c[name]["chains"]) % 64, name  # the last wavefront is partly live
    v = set(P.expected("chains_600_interleaved")["voters"])
    assert all((i in v) != (i + 1 in v) for i in range(599)) and 256 in v and 599 not in v
    assert all(c["chains_600_interleaved"]["runs"][i] == [130 << 4 | X] for i in range(600) if i not in v)
    spans = [ch[9] - ch[8] for ch in c["span_1_chains"]["chains"]]
    assert spans == [1] * 390 and [ch[8] for ch in c["span_1_chains"]["chains"]] == [n % 130 for n in range(390)]
    e = c["spans_on_block_edges"]
    spans = [ch[9] - ch[8] for ch in e["chains"]]
    assert spans == [256, 64, 1, 255, 257] and len(e["draft"][0][1]) == 600 and e["params"] == dict(min_depth=1)
    first = [sum(spans[:k]) for k in range(5)]  # the chains' first columns
    assert first[1] % BLOCK == 0 and (first[1] - 1) % BLOCK == 255 and (first[4] - 1) % 64 == 63
    ops = {r & 15 for r in e["runs"][0]}
    assert ops == {I, D, EQ, X} and e["runs"][0][0] & 15 != I and e["runs"][0][-1] & 15 != I
    r = c["records_300"]
    lens = [len(s) for _, s in r["draft"]]
    assert len(lens) == 300 and lens == [n % 131 for n in range(300)] and lens.count(0) >= 2 and 60 in lens and max(lens) == 130
    assert sorted({ch[1] for ch in r["chains"]}) == [1, 255, 256, 299] and all([ch[1] for ch in r["chains"]].count(t) == 3 for t in (1, 255, 256, 299))
    want = P.expected("records_300")
    assert len(want["records"]) == 300 and want["text"].count(b">d0\n\n>d1\n") == 1 and b">d131\n\n" in want["text"]
    assert [i for i, rec in enumerate(want["records"]) if rec[2:5] != (0, 0, 0)] == [1, 255, 256, 299]
    s = c["reads_300_sparse"]
    assert len(s["reads"]) == 301 and sorted({ch[0] for ch in s["chains"]}) == [0, 255, 256, 299]
    assert sum(1 for _, b in s["reads"] if not b) >= 10 and s["reads"][254][1] and not s["reads"][259][1] and s["reads"][300][1]
    assert s["params"] == dict(min_depth=4) and len(P.expected("reads_300_sparse")["voters"]) == 4


# ---- insertion events ---------------------------------------------------------------------------------------------------

def test_event_conditions():
    c = P.cases()
    two = c["ins_in_second_record"]
    assert len(two["draft"]) == 2 and len(two["draft"][0][1]) > 0  # record 1 lies behind record 0's bases: its store offset is not 0
    tlen = len(two["draft"][1][1])
    ev = _events("ins_in_second_record")
    assert sorted(set(ev)) == [(1, 1, 2, 0b0001), (1, 45, 1, 0b10), (1, tlen - 1, 2, 0b1111)] and len(ev) == 6
    assert P.expected("ins_in_second_record")["ins_usable"] == 8  # with the two at slot tlen, which no test of 0 < p < tlen passes
    assert P.expected("ins_in_second_record")["records"][0] == (130, 130, 0, 0, 0, 300)
    assert len(_events("events_256")) == BLOCK and len(set(_events("events_256"))) == 1
    assert len(_events("events_300_one_group")) == 300 and len(set(_events("events_300_one_group"))) == 1
    ev = sorted(_events("events_two_groups_across_a_block"), key=lambda e: e[1:])
    heads = [i for i in range(300) if i == 0 or ev[i] != ev[i - 1]]
    assert heads == [0, 100] and heads[1] % 64 and ev[0][2:] == (1, 0) and ev[-1][2:] == (2, 0b0001)
    for name, bits in (("ins_32_top_bits", 1 << 62), ("ins_32_low_bits", 1), ("ins_32_sign_bit", 3 << 62)):
        ev = _events(name)
        lose, win = ev[0], ev[2]  # the loser stands first in table order
        assert len(ev) == 4 and ev[0] == ev[1] and ev[2] == ev[3] and lose[:3] == win[:3] == (0, P.AT, 32)
        assert lose[3] ^ win[3] == bits and win[3] < lose[3] < 1 << 64, name
        assert (lose[3] ^ win[3]) >> 62 == {"ins_32_top_bits": 1, "ins_32_low_bits": 0, "ins_32_sign_bit": 3}[name]
    sign = _events("ins_32_sign_bit")
    assert sign[2][3] < 1 << 63 <= sign[0][3]  # read as signed, the loser would be the smaller
    runs = c["ins_64_and_65_letters"]["runs"][0]
    assert [r >> 4 for r in runs if r & 15 == I] == [64, 65] and runs[0] & 15 == EQ and runs[-1] & 15 == EQ and _events("ins_64_and_65_letters") == []
    assert [(r >> 4, r & 15) for r in c["ins_before_deleted"]["runs"][0]] == [(50, EQ), (2, I), (1, D), (79, EQ)]
    assert [(r >> 4, r & 15) for r in c["ins_behind_deleted"]["runs"][0]] == [(49, EQ), (1, D), (2, I), (80, EQ)]
    assert [(r >> 4, r & 15) for r in c["ins_adjacent_runs"]["runs"][0]] == [(50, EQ), (1, I), (1, I), (80, EQ)]
    assert _events("ins_adjacent_runs") == [(0, 50, 1, 1), (0, 50, 1, 0)] * 2
    for name, (left, right) in (("ins_left_depth_decides", (2, 3)), ("ins_right_depth_decides", (3, 2)), ("ins_left_depth_enough", (3, 3)),
                                ("ins_right_depth_enough", (3, 3))):
        depth = [0] * 130
        for i in P.expected(name)["voters"]:
            for p in range(c[name]["chains"][i][8], c[name]["chains"][i][9]):
                depth[p] += 1
        assert (depth[P.AT - 1], depth[P.AT]) == (left, right) and c[name]["params"] == {} and len(_events(name)) == 2, name


# ---- rules 2, 3, 5 and 7 ------------------------------------------------------------------------------------------------

def test_rule_conditions():
    c = P.cases()
    s = c["scores_negative"]
    by_read = {}
    for i, ch in enumerate(s["chains"]):
        by_read.setdefault(ch[0], []).append((ch[4], i))
    assert [tuple(x for x, _ in by_read[q]) for q in range(0, 8, 2)] == [(-5, -3), (0, -1), (-2**31, -2**31 + 1), (-2**31,)]
    assert P.expected("scores_negative")["voters"] == [max(v)[1] for _, v in sorted(by_read.items())]
    assert all(ch[4] <= 0 for ch in s["chains"]) and s["chains"][-1][10:] == (0, 0) and s["params"] == dict(min_depth=2)
    # only the voter of a read has its X at + 10
    for i, (ch, runs) in enumerate(zip(s["chains"], s["runs"])):
        assert (runs[0] >> 4 == 10) == (i in P.expected("scores_negative")["voters"])
    assert [ch[10:] for ch in c["identity_bounds_100"]["chains"]][:2] == [(P.TOP, P.TOP), (P.TOP - 1, P.TOP)]
    assert P.expected("identity_bounds_100")["voters"] == [0, 2]
    assert [ch[10:] for ch in c["identity_bounds_0"]["chains"]][:2] == [(0, P.TOP)] * 2 and c["identity_bounds_0"]["params"]["min_identity"] == 0
    m, b = c["identity_bounds_50"]["chains"][0][10:]
    assert m * 100 >= 50 * b and m * 100 % 2**32 < 50 * b % 2**32  # cut to 32 bits the chain would not vote
    for name, stored in (("strand_1_lower_case", b"t"), ("strand_1_lower_case_ins", b"ca")):
        k = c[name]
        assert [ch[2] for ch in k["chains"]] == [1, 1, 0]
        lower = bytes(x for x in k["reads"][0][1] if 97 <= x <= 122)
        assert lower == stored and map_oracle.revcomp(stored) == stored[::-1]  # rule 3 complements no lower-case byte
    assert c["strand_1_lower_case"]["draft"][0][1][P.AT:P.AT + 1] == b"A"
    for name in ("draft_n_corrected", "draft_n_tie"):
        assert c[name]["draft"][0][1][P.AT:P.AT + 1] == b"N" and c[name]["draft"][0][1].count(b"N") == 1
    assert all(r[1][P.AT:P.AT + 1] == b"N" for r in c["other_votes_only"]["reads"]) and b"N" not in c["other_votes_only"]["draft"][0][1]
    assert c["min_depth_huge"]["params"] == dict(min_depth=2**31 - 1)
    for name, n_in, n_out in (("out_60", 61, 60), ("out_60_inserted", 59, 60), ("out_120", 121, 120), ("out_61", 60, 61)):
        want = P.expected(name)
        assert want["records"][0][:2] == (n_in, n_out) and want["text"] == c[name]["lit"]["text"] and b"\n\n" not in want["text"]
        assert [len(x) for x in want["text"].split(b"\n")[1:-1]] == [60] * (n_out // 60) + [n_out % 60] * (n_out % 60 > 0)
    runs = c["d_at_chain_ends"]["runs"][0]
    ch = c["d_at_chain_ends"]["chains"][0]
    assert runs[0] == 1 << 4 | D and runs[-1] == 1 << 4 | D and (ch[8], ch[9]) == (0, 130)


# ---- ranked form --------------------------------------------------------------------------------------------------------

def test_ranked_conditions():
    c = P.cases()["ranked_300"]
    assert len(c["chains"]) == 300 and len(c["reads"]) == 150 and all(r[0] == i for i, r in enumerate(c["ranks"]))
    assert {r[3] for r in c["ranks"]} == {18, 42} and c["min_mapq"] == 30
    v = set(P.expected("ranked_300")["voters"])
    assert v == {i for i, r in enumerate(c["ranks"]) if r[3] == 42}
    assert [i in v for i in range(256, 264)] == [True, False, False, True, True, True, False, False]  # reads 128 .. 131
    assert sum(1 for i in range(256, 299) if (i in v) != (i + 1 in v)) >= 20
    plain = pl_oracle.run(c["draft"], c["reads"], c["chains"], c["runs"])
    assert plain["n_voters"] == 150 and plain["voters"] != sorted(v)  # the plain form lets the first chain of every read vote
    c = P.cases()["ranked_two_primaries_overlap"]
    a, b = c["chains"][:2]
    assert a[0] == b[0] and a[7] <= b[6] and max(a[8], b[8]) < min(a[9], b[9]) and [r[0] for r in c["ranks"]] == [0, 1, 2]
    assert P.expected("ranked_two_primaries_overlap")["voters"] == [0, 1, 2]
    plain = pl_oracle.run(c["draft"], c["reads"], c["chains"], c["runs"], **c["params"])
    assert plain["voters"] == [0, 2] and plain["pos_substituted"] == 0  # voting once, the X at 60 ties with the draft's base


# ---- rule 1 on the large table ------------------------------------------------------------------------------------------

def test_violations_on_the_large_table():
    v = P.violations()
    assert sorted(v) == ["query_consumption_at_300", "rank_parent_at_299", "run_op_in_the_last_run", "strand_at_599",
                         "two_bad_chains_in_two_blocks"]
    for name, (c, ranks, chain, what) in v.items():
        assert len(c["chains"]) == 600
        with pytest.raises(pl_oracle.PolishError) as e:
            if ranks is None:
                pl_oracle.run(c["draft"], c["reads"], c["chains"], c["runs"])
            else:
                pl_rank_oracle.run(c["draft"], c["reads"], c["chains"], c["runs"], ranks)
        assert (e.value.chain, e.value.what) == (chain, what), name
        assert what == "rank" or what in pl_oracle.WHAT
    both = v["two_bad_chains_in_two_blocks"][0]
    assert both["chains"][599][2] == 2 and 300 // BLOCK != 599 // BLOCK
    last = v["run_op_in_the_last_run"][0]
    assert last["runs"][-1][-1] & 15 == 3 and all(r & 15 in (I, D, EQ, X) for runs in last["runs"][:-1] for r in runs)
    assert P.cases()["chains_600_interleaved"]["chains"][599][2] == 0  # (the shared table itself is untouched)


# ---- through the mapper -------------------------------------------------------------------------------------------------

def test_planted_three_records():
    wl = P.planted_three_records()
    draft = map_oracle.parse(wl["draft"], False)
    (_, whole), = map_oracle.parse(plcases.workload("planted")["draft"], False)
    assert [n for n, _ in draft] == [b"left", b"middle", b"right", b"unmapped"] and [len(s) for _, s in draft][::3] == [7000, 500]
    assert draft[0][1] + map_oracle.revcomp(draft[1][1]) + draft[2][1] == whole
    want, mapped = P.expected_planted_three_records()
    assert {ch[1] for ch in mapped["chains"]} == {0, 1, 2}
    assert all(want["records"][r][4] >= 10 for r in (1, 2)) and want["records"][3] == (500, 500, 0, 0, 0, 0)
    assert want["text"].endswith(P.wrap(b"unmapped", wl["unmapped"]))
