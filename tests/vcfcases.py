"""Inputs of the tests of the polisher's VCF output (msgpu_vcf.hip; rules V1 - V9), shared by tests/test_vcf_host.py and
tests/test_gpu_vcf.py: named tables built with plcases.case, each with its expected lines (``lines``) written by hand from the
draft's bytes -- no literal is computed by the restatement -- and ``note``, what in the kernels the case aims at.  The kernels
launch blocks of 256 threads over the draft's bases and over the blocks of V1; a line of more than the bound
(_lib.VCF_SHORT_BYTES) is written by several workgroups.

Basic:      no_edit, snp_first, snp_last, snp_second_record, sub_2of3
Merged:     mnp_2, mnp_3, mnp_257_at_255, mnp_257_at_256, two_blocks_one_apart
Deletions:  del_at_0, del_at_0_second_record, del_at_end, del_whole_record
Insertions: ins_pure, ins_leading_slot, ins_trailing_slot, ins_between_deletions, ins_32, ins_next_to_deletion
REF bytes:  ref_bytes
Widths:     pos_widths, dp_ao_widths
Long lines: line_bound_minus_1, line_bound, line_bound_plus_1, del_40000
Tables:     blocks_300, records_300, names_1_and_254
``bad_names()``: the drafts that V7 refuses."""
import collections
import functools

import pledgecases
import plcases
import vcf_oracle

AT = 50  # where most cases edit their 130-base draft
DEL_LINE = 38  # the bytes of a deletion's line at POS 50 of record d0 with DP = AO = 3, beside its n deleted bases


def ln(name, pos, ref, alt, dp, ao, kind, end=None):
    """V5, by hand"""
    return b"%s\t%d\t.\t%s\t%s\t.\tPASS\t%sDP=%d;AO=%d;TYPE=%s\n" % (name, pos, ref, alt, b"" if end is None else b"END=%d;" % end, dp, ao, kind)


def sw(seq, a, n=1):
    """the letters that plcases.aligned's ("X", n) puts at [a, a + n)"""
    return bytes(plcases.other(b) for b in seq[a:a + n])


def script(tlen, *edits, ts=0, te=None):
    """a script over [ts, te) of a draft: '=' between the edits (position, op, arg), which ascend"""
    out, p = [], ts
    for at, op, arg in edits:
        if at > p:
            out.append(("=", at - p))
            p = at
        out.append((op, arg))
        p += arg if op in ("X", "D") else len(arg) if op in ("x", "e") else 0
    te = tlen if te is None else te
    if te > p:
        out.append(("=", te - p))
    return out


def _add(c, name, draft, scripts, lines, note, params=None):
    c[name] = dict(plcases.case(draft, scripts, params, note), lines=lines)


def _three(tlen, *edits, t=0):
    return [(t, 0, script(tlen, *edits))] * 3


@functools.lru_cache(maxsize=None)
def cases():
    from muchsalsa_amd import _lib
    c = collections.OrderedDict()
    u, G = pledgecases._u(), pledgecases._genome()
    two = [(b"first", u), (b"second desc", bytes(G[5000:5090]))]
    s2 = two[1][1]
    # ---- basic
    _add(c, "no_edit", u, _three(130), [], "no head: the header alone, no kernel behind the first read-back")
    _add(c, "snp_first", u, _three(130, (0, "X", 1)), [ln(b"d0", 1, u[0:1], sw(u, 0), 3, 3, b"snp")], "a head at a record's first byte: no byte in front")
    _add(c, "snp_last", u, _three(130, (129, "X", 1)), [ln(b"d0", 130, u[129:130], sw(u, 129), 3, 3, b"snp")], "an end at a record's last byte: no byte behind")
    _add(c, "snp_second_record", two, _three(90, (0, "X", 1), (89, "X", 1), t=1),
         [ln(b"second", 1, s2[0:1], sw(s2, 0), 3, 3, b"snp"), ln(b"second", 90, s2[89:90], sw(s2, 89), 3, 3, b"snp")],
         "a record whose store offset is not 0: positions are the record's; the name is cut at the blank")
    _add(c, "sub_2of3", u, [(0, 0, script(130, (AT, "X", 1)))] * 2 + [(0, 0, script(130))], [ln(b"d0", 51, u[50:51], sw(u, 50), 3, 2, b"snp")],
         "AO below DP: the winning counter, not the depth")
    # ---- merged substitutions
    _add(c, "mnp_2", u, _three(130, (AT, "X", 2)), [ln(b"d0", 51, u[50:52], sw(u, 50, 2), 3, 3, b"mnp")], "two edited neighbours are one block")
    _add(c, "mnp_3", u, _three(130, (AT, "X", 3)), [ln(b"d0", 51, u[50:53], sw(u, 50, 3), 3, 3, b"mnp")], "three")
    d600 = bytes(G[2000:2600])
    for at in (255, 256):
        _add(c, "mnp_257_at_%d" % at, d600, _three(600, (at, "X", 257)), [ln(b"d0", at + 1, d600[at:at + 257], sw(d600, at, 257), 3, 3, b"mnp")],
             "a block across the edges of the 256-thread blocks of k_vcf_flags and k_vcf_compact: head and end in different workgroups")
    _add(c, "two_blocks_one_apart", u, _three(130, (AT, "X", 1), (AT + 2, "X", 1)),
         [ln(b"d0", 51, u[50:51], sw(u, 50), 3, 3, b"snp"), ln(b"d0", 53, u[52:53], sw(u, 52), 3, 3, b"snp")], "one unchanged base between two blocks")
    # ---- deletions
    _add(c, "del_at_0", u, _three(130, (0, "D", 2)), [ln(b"d0", 1, u[0:3], u[2:3], 3, 3, b"del")], "anchored behind: a = 0")
    _add(c, "del_at_0_second_record", two, _three(90, (0, "D", 2), t=1), [ln(b"second", 1, s2[0:3], s2[2:3], 3, 3, b"del")],
         "anchored behind in a record behind another: the byte in front belongs to the first record")
    _add(c, "del_at_end", u, _three(130, (128, "D", 2)), [ln(b"d0", 128, u[127:130], u[127:128], 3, 3, b"del")], "b = tlen, anchored in front")
    gone = [(b"kept", bytes(G[200:290])), (b"gone", bytes(G[300:370]))]
    _add(c, "del_whole_record", gone, [dict(t=1, ts=0, script=[("D", 70)], flanks=(b"ACGT", b"TT"))] * 3 + [(0, 0, [("=", 90)])] * 3,
         [ln(b"gone", 1, gone[1][1][0:1], b"<DEL>", 3, 3, b"del", end=70)], "a = 0 and b = tlen: <DEL> and END")
    # ---- insertions
    _add(c, "ins_pure", u, _three(130, (AT, "I", b"AC")), [ln(b"d0", 50, u[49:50], u[49:50] + b"AC", 3, 3, b"ins")], "a = b: a block of its own")
    _add(c, "ins_leading_slot", u, _three(130, (AT, "I", b"G"), (AT, "X", 1)), [ln(b"d0", 51, u[50:51], b"G" + sw(u, 50), 3, 3, b"complex")],
         "an insertion at slot a of a block: in front of call(a) in ALT0, and no block of its own")
    _add(c, "ins_trailing_slot", u, _three(130, (AT, "X", 1), (AT + 1, "I", b"G")), [ln(b"d0", 51, u[50:51], sw(u, 50) + b"G", 3, 3, b"complex")],
         "an insertion at slot b: behind call(b - 1), owned by the block, no head at b")
    _add(c, "ins_between_deletions", u, _three(130, (AT, "D", 1), (AT + 1, "I", b"GT"), (AT + 1, "D", 1)), [ln(b"d0", 51, u[50:52], b"GT", 3, 3, b"complex")],
         "|REF0| = |ALT0| = 2 and yet no mnp: the block holds deletions and an insertion")
    i32 = bytes(G[400:432])
    _add(c, "ins_32", u, _three(130, (AT, "I", i32)), [ln(b"d0", 50, u[49:50], u[49:50] + i32, 3, 3, b"ins")], "the longest insertion")
    _add(c, "ins_next_to_deletion", u, _three(130, (AT, "I", b"AC"), (AT, "D", 1)), [ln(b"d0", 51, u[50:51], b"AC", 3, 3, b"complex")],
         "ALT0 is the insertion alone: call(a) emits nothing")
    # ---- REF bytes
    d = bytearray(u)
    d[50], d[52], d[60] = ord("N"), ord("R"), ord("N")
    d[51] |= 0x20
    d = bytes(d)
    _add(c, "ref_bytes", d, _three(130, (AT, "D", 3), (60, "x", b"A")),
         [ln(b"d0", 50, u[49:50] + b"N" + u[51:52] + b"N", u[49:50], 3, 3, b"del"), ln(b"d0", 61, b"N", b"A", 3, 3, b"snp")],
         "a draft N, a lower-case byte and an R inside REF; a substituted N")
    # ---- decimal widths
    big = plcases._g(10050, 79)
    edits, lines = [], []
    for k in (10, 100, 1000, 10000):
        edits += [(k - 2, "X", 1), (k, "I", b"A")]
        lines += [ln(b"d0", k - 1, big[k - 2:k - 1], sw(big, k - 2), 3, 3, b"snp"), ln(b"d0", k, big[k - 1:k], big[k - 1:k] + b"A", 3, 3, b"ins")]
    _add(c, "pos_widths", big, _three(10050, *edits), lines, "POS either side of 10, 100, 1000 and 10000")
    # 100 short reads from 10 on: all cover 20, 99 cover 40, 10 cover 60, 9 cover 80, each with an X there
    ends = [90] * 9 + [70] + [50] * 89 + [30]
    reads = [(0, 10, script(130, *[(s, "X", 1) for s in (20, 40, 60, 80) if s < te], ts=10, te=te)) for te in ends]
    _add(c, "dp_ao_widths", u, reads, [ln(b"d0", s + 1, u[s:s + 1], sw(u, s), n, n, b"snp") for s, n in ((20, 100), (40, 99), (60, 10), (80, 9))],
         "DP and AO either side of 10 and 100")
    # ---- long lines
    d700 = bytes(G[3000:3700])
    for name, extra in (("line_bound_minus_1", -1), ("line_bound", 0), ("line_bound_plus_1", 1)):
        n = _lib.VCF_SHORT_BYTES - DEL_LINE + extra
        _add(c, name, d700, _three(700, (AT, "D", n)), [ln(b"d0", 50, d700[49:50 + n], d700[49:50], 3, 3, b"del")],
             "a line of the bound %+d bytes: the last of the wavefront's class, the first of the workgroups'" % extra)
    d41k = plcases._g(41000, 80)
    _add(c, "del_40000", d41k, _three(41000, (500, "D", 40000)), [ln(b"d0", 500, d41k[499:40500], d41k[499:500], 3, 3, b"del")],
         "a block beyond VCF_ROW_WAVE: reduced by eight workgroups; REF is the line")
    # ---- table sizes
    d1300 = bytes(G[6000:7300])
    _add(c, "blocks_300", d1300, _three(1300, *[(10 + 4 * i, "X", 1) for i in range(300)]),
         [ln(b"d0", 11 + 4 * i, d1300[10 + 4 * i:11 + 4 * i], sw(d1300, 10 + 4 * i), 3, 3, b"snp") for i in range(300)], "more than a block of blocks")
    recs = [(b"c%d" % i, bytes(G[8000 + 40 * i:8040 + 40 * i])) for i in range(300)]
    r255, r256, r299 = recs[255][1], recs[256][1], recs[299][1]
    _add(c, "records_300", recs, _three(40, (0, "X", 1), t=255) + _three(40, (39, "D", 1), t=256) + _three(40, (20, "I", b"T"), t=299),
         [ln(b"c255", 1, r255[0:1], sw(r255, 0), 3, 3, b"snp"), ln(b"c256", 39, r256[38:40], r256[38:39], 3, 3, b"del"),
          ln(b"c299", 20, r299[19:20], r299[19:20] + b"T", 3, 3, b"ins")], "more than a block of records; variants in records 255, 256 and 299")
    long_name = b"y" * 254
    _add(c, "names_1_and_254", [(b"x", u), (long_name, s2)], _three(130, (5, "X", 1)) + _three(90, (5, "X", 1), t=1),
         [ln(b"x", 6, u[5:6], sw(u, 5), 3, 3, b"snp"), ln(long_name, 6, s2[5:6], sw(s2, 5), 3, 3, b"snp")], "names of 1 and of 254 bytes")
    return c


def names():
    return list(cases())


@functools.lru_cache(maxsize=None)
def bad_names():
    """name -> (a case whose draft V7 refuses, the record and the entry of vcf_oracle.BAD_NAME that the error must name)"""
    u = pledgecases._u()
    out = collections.OrderedDict()
    for tag, drafts, record, why in (("empty", [b""], 0, 0), ("long_255", [b"ok", b"z" * 255], 1, 1), ("star", [b"*x"], 0, 2), ("equals", [b"ok", b"=x"], 1, 2),
                                     ("comma", [b"a,b"], 0, 3), ("less", [b"a<b"], 0, 3), ("greater", [b"ok", b"a>b"], 1, 3), ("del_byte", [b"a\x7fb"], 0, 3),
                                     ("high_byte", [b"a\x80b"], 0, 3)):
        out[tag] = (plcases.case([(n, u) for n in drafts], _three(130, (AT, "X", 1))), record, vcf_oracle.BAD_NAME[why])
    return out


def mates_case():
    """test_gpu_polish_mate.repeat_pairs_case with mate rows (mate, tlen, cls, n_best) written by hand: of pair p's chains 3p (on
    copy B, with an X column), 3p + 1 (on copy A) and 3p + 2 (in the flank) -> (the case, the rows that select the chain on A
    with the flank's, the rows that select the one on B: its X column then makes a variant)"""
    import test_gpu_polish_mate
    on_a = [row for p in range(3) for row in ((0, 0, 0, 0), (3 * p + 2, 290, 1, 1), (3 * p + 1, 290, 1, 1))]
    on_b = [row for p in range(3) for row in ((3 * p + 2, 610, 1, 1), (0, 0, 0, 0), (3 * p, 610, 1, 1))]
    return test_gpu_polish_mate.repeat_pairs_case(), on_a, on_b


def clean(draft):
    """the draft's names as the stage cleans them: cut at the first whitespace"""
    return [(n.split()[0] if n.split() else b"", s) for n, s in draft]


def expected_of(c, voting=None):
    """vcf_oracle.run on a case of plcases' shape"""
    return vcf_oracle.run(clean(c["draft"]), c["reads"], c["chains"], c["runs"], voting=voting, **c["params"])


@functools.lru_cache(maxsize=None)
def expected(name):
    return expected_of(cases()[name])
