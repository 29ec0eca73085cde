"""The polisher's VCF output (include/msgpu.h, rules V1 - V7 behind "pileup consensus"; msgpu_vcf.hip) restated in plain Python,
sequentially, on tests/pl_oracle.py's check, voters, pileup, call and insertion.  It is the yardstick of the VCF's tests: the
GPU's text and variant rows are compared with this module's without tolerance.  ``run`` takes the voters as an argument, so
the ranked and the mates restatements (pl_rank_oracle.voters, pl_mate_oracle.voters) feed it as well.  ``apply`` is independent
of all of it: it parses the text alone and edits a draft by it."""
import pl_oracle

SNP, MNP, INS, DEL, COMPLEX = range(5)
TYPES = ("snp", "mnp", "ins", "del", "complex")
NONE, LEFT, RIGHT, WHOLE = range(4)
ROW = ("record", "a", "ref_len", "alt_len", "dp", "ao", "type", "anchor", "offset", "length")
COUNTS = ("n_variants", "n_snp", "n_mnp", "n_ins", "n_del", "n_complex", "n_whole_deleted", "ref_bases", "alt_bases", "header_bytes",
          "text_bytes")
BAD_NAME = ("an empty name", "a name longer than 254 bytes", "a name that begins with * or =",
            "a name with a byte outside 0x21..0x7e or one of , < >", "its name is that of an earlier record")


class NameError_(ValueError):
    def __init__(self, record, why):
        super().__init__("VCF: draft record %d: %s" % (record, why))
        self.record, self.why = record, why


def base(b):
    """a draft byte as REF shows it"""
    b = pl_oracle.fold(b)
    return b if b in pl_oracle.CLASS else ord("N")


def folded(seq):
    return bytes(base(b) for b in seq)


def check_names(names):
    """V7: raises NameError_ for the first record whose name is refused, with the first of BAD_NAME that it meets"""
    seen = set()
    for r, n in enumerate(names):
        if not n:
            raise NameError_(r, BAD_NAME[0])
        if len(n) > 254:
            raise NameError_(r, BAD_NAME[1])
        if n[:1] in (b"*", b"="):
            raise NameError_(r, BAD_NAME[2])
        if any(b < 0x21 or b > 0x7e or b in b",<>" for b in n):
            raise NameError_(r, BAD_NAME[3])
        if n in seen:
            raise NameError_(r, BAD_NAME[4])
        seen.add(n)


def header(draft):
    """V6"""
    return (b"##fileformat=VCFv4.2\n##source=muchsalsa_amd.polish\n" +
            b"".join(b"##contig=<ID=%s,length=%d>\n" % (n, len(s)) for n, s in draft) +
            b"##INFO=<ID=DP,Number=1,Type=Integer,Description=\"Least depth over the block's positions\">\n"
            b"##INFO=<ID=AO,Number=1,Type=Integer,Description=\"Least support among the block's edits\">\n"
            b"##INFO=<ID=TYPE,Number=1,Type=String,Description=\"snp, mnp, ins, del or complex\">\n"
            b"##INFO=<ID=END,Number=1,Type=Integer,Description=\"Last position of a deleted record\">\n"
            b"##ALT=<ID=DEL,Description=\"Deletion of the whole record\">\n"
            b"#CHROM\tPOS\tID\tREF\tALT\tQUAL\tFILTER\tINFO\n")


def record_blocks(seq, cnt, events_at, min_depth):
    """V1, V2, V4 for one draft record -> [(a, b, ALT0, dp, ao, holds a deletion, holds an insertion)], by a"""
    tlen = len(seq)
    depth = [sum(c) for c in cnt]
    calls = [pl_oracle.call(cnt[p], seq[p], min_depth) for p in range(tlen)]
    e = [kind in ("substituted", "deleted") for kind, _ in calls]
    ins = {}  # slot -> (letters, the applied group's count)
    for p in range(1, tlen):
        if p in events_at:
            letters = pl_oracle.insertion(events_at[p], depth[p - 1], depth[p], min_depth)
            if letters:
                packed = 0
                for b in letters:
                    packed = packed << 2 | pl_oracle.CLASS[b]
                ins[p] = (letters, events_at[p][(len(letters), packed)])

    def support(p):
        kind, emitted = calls[p]
        return cnt[p][pl_oracle.DEL if kind == "deleted" else pl_oracle.CLASS[emitted[0]]]

    out, p = [], 0
    while p < tlen:
        if e[p]:
            a = p
            while p < tlen and e[p]:
                p += 1
            b = p
            alt = b"".join(ins.get(x, (b"",))[0] + calls[x][1] for x in range(a, b)) + ins.get(b, (b"",))[0]
            sup = [support(x) for x in range(a, b)] + [ins[x][1] for x in range(a, b + 1) if x in ins]
            out.append((a, b, alt, min(depth[a:b]), min(sup), any(calls[x][0] == "deleted" for x in range(a, b)),
                        any(x in ins for x in range(a, b + 1))))
        else:
            if p in ins and not (p > 0 and e[p - 1]):
                out.append((p, p, ins[p][0], min(depth[p - 1], depth[p]), ins[p][1], False, True))
            p += 1
    return out


def line(name, seq, block):
    """V3 - V5 -> (the line, the row's (ref_len, alt_len, dp, ao, type, anchor))"""
    a, b, alt0, dp, ao, has_del, has_ins = block
    ref0, tlen = folded(seq[a:b]), len(seq)
    if not ref0:
        kind = INS
    elif not alt0:
        kind = DEL
    elif len(ref0) == len(alt0) and not has_del and not has_ins:
        kind = SNP if len(ref0) == 1 else MNP
    else:
        kind = COMPLEX
    end = b""
    if ref0 and alt0:
        anchor, pos, ref, alt = NONE, a + 1, ref0, alt0
    elif a > 0:
        x = folded(seq[a - 1:a])
        anchor, pos, ref, alt = LEFT, a, x + ref0, x + alt0
    elif b < tlen:
        x = folded(seq[b:b + 1])
        anchor, pos, ref, alt = RIGHT, 1, ref0 + x, alt0 + x
    else:
        anchor, pos, ref, alt, end = WHOLE, 1, folded(seq[:1]), b"<DEL>", b"END=%d;" % tlen
    text = b"%s\t%d\t.\t%s\t%s\t.\tPASS\t%sDP=%d;AO=%d;TYPE=%s\n" % (name, pos, ref, alt, end, dp, ao, TYPES[kind].encode())
    return text, (len(ref0), len(alt0), dp, ao, kind, anchor)


def run(draft, reads, chains, runs, voting=None, **params):
    """draft, reads: [(name, bases)], the draft's names as the stage cleans them.  ``voting``: the voters' chain indices (None:
    pl_oracle.voters).  -> a dict: ``text``, ``rows`` (the tuples of ROW), ``lines`` and the counts of COUNTS."""
    p = dict(pl_oracle.PARAMS, **params)
    pl_oracle.check(draft, reads, chains, runs)
    check_names([n for n, _ in draft])
    if voting is None:
        voting = pl_oracle.voters(chains, p["min_identity"])
    counters, events = pl_oracle.pileup(draft, reads, chains, runs, voting, dict.fromkeys(pl_oracle.COUNTS, 0))
    head = header(draft)
    lines, rows, at = [], [], len(head)
    for t, (name, seq) in enumerate(draft):
        events_at = {slot: groups for (rec, slot), groups in events.items() if rec == t}
        for block in record_blocks(seq, counters[t], events_at, p["min_depth"]):
            text, row = line(name, seq, block)
            rows.append((t, block[0]) + row + (at, len(text)))
            lines.append(text)
            at += len(text)
    counts = dict(n_variants=len(rows), n_whole_deleted=sum(r[7] == WHOLE for r in rows), ref_bases=sum(r[2] for r in rows),
                  alt_bases=sum(r[3] for r in rows), header_bytes=len(head), text_bytes=at)
    for k, n in enumerate(TYPES):
        counts["n_" + n] = sum(r[6] == k for r in rows)
    return dict(counts, text=head + b"".join(lines), rows=rows, lines=lines)


def apply(draft, vcf_text):
    """The text alone, applied to a draft: [(name, bases)] -> [(name, the edited bases)], every unedited base folded as REF
    shows it.  Asserts what a reader of the file relies on: the header's contigs are the draft's, the lines are in record
    order and ascending without overlap, and REF is the draft."""
    order = {n: i for i, (n, _) in enumerate(draft)}
    per, contigs, last = {n: [] for n, _ in draft}, [], (-1, 0)
    for ln in vcf_text.split(b"\n"):
        if ln.startswith(b"##contig=<ID="):
            name, length = ln[len(b"##contig=<ID="):-1].rsplit(b",length=", 1)
            contigs.append((name, int(length)))
        if not ln or ln.startswith(b"#"):
            continue
        name, pos, _id, ref, alt, qual, filt, info = ln.split(b"\t")
        assert _id == b"." and qual == b"." and filt == b"PASS"
        info = dict(kv.split(b"=") for kv in info.split(b";"))
        start = int(pos) - 1
        stop = int(info[b"END"]) if alt == b"<DEL>" else start + len(ref)
        assert (order[name], start) >= last, "the lines' order"
        last = (order[name], start + 1)
        per[name].append((start, stop, ref, b"" if alt == b"<DEL>" else alt))
    assert contigs == [(n, len(s)) for n, s in draft]
    out = []
    for name, seq in draft:
        f, parts, at = folded(seq), [], 0
        for start, stop, ref, alt in per[name]:
            assert f[start:start + len(ref)] == ref and stop <= len(f), "REF is the draft"
            if start == at - 1:  # the base that anchored the line in front (V3, behind a block at 0) anchors this one too
                assert ref[:1] == alt[:1]
                start, alt = at, alt[1:]
            assert start >= at, "the lines overlap"
            parts += [f[at:start], alt]
            at = stop
        out.append((name, b"".join(parts) + f[at:]))
    return out
