r"""SAM output on the GPU: the mapper's tables (chains, runs, rank rows, mate rows) as SAM 1.6 text.

    python -m muchsalsa_amd.mapper <targets.fa|fq> <queries.fa|fq> <out.paf> --sam <out.sam> [--md] [--cigar-m] [...]

is the command that uses it (``mapper.run(..., sam=PATH)``); ``run_tables`` is the stage on given tables.  The stage loads
both files itself, checks the tables on the device, and formats every line there: count, scan, write.  It is additive: with it
unused, every byte of every other output is as before.  The stage is defined by the rules below, in integers only, and
checked, without tolerance, against the tests' restatement in plain Python (tests/sam_oracle.py), not against another tool.
The rules (include/msgpu.h, "SAM output"); parameters eqx (0 / 1, default 1), md (0 / 1, default 0), unmapped (0 / 1,
default 1):

 S1. inputs and checks.  Both files through msgpu_seq_parse_upload; the chain table in output order; the run tables (runs
     of chain i: ops[off[i] .. off[i + 1]), each len << 4 | op); the rank rows (required); optionally the mate rows.  The
     checks are complete on the device before any formatting kernel runs; a failure is MSGPU_E_ARG "chain <i>: <what>" for
     the smallest bad chain and, of that chain, the first violated check in this order: (a) off[0] = 0, the offsets do not
     decrease (and none exceeds off[n_chains], the size of the run table); (b) query does not decrease; (c) strand <= 1;
     (d) the query record and the target record are in range; (e) t_start <= t_end <= tlen; (f) q_start <= q_end <= qlen;
     (g) every op is one of 1 (I), 2 (D), 7 (=), 8 (X) with length > 0 (a run that breaks this consumes nothing); (h) the
     runs consume exactly t_end - t_start target bases and (i) q_end - q_start query bases; (j) parent is in range, lies in
     the same query record and names a chain that is its own parent; (k) with mates, for a chain with cls = 1: mate is in
     range, lies in the partner record (query ^ 1) and its row has cls = 1 and points back.  With mates an odd number of query
     records is MSGPU_E_ARG naming the count.  Host checks, each MSGPU_E_ARG naming the record: two target records with the
     same name (the loader keeps the first record of a name and drops the later ones, so a file cannot bring this about:
     the records, and the chain table's indices, are those the loader keeps, and the check guards the header); a name
     longer than 254 bytes; an empty name (both files).
 S2. header.  "@HD\tVN:1.6\tSO:unsorted\tGO:query", one "@SQ\tSN:<name>\tLN:<length>" per target record in file order,
     "@PG\tID:muchsalsa_amd\tPN:muchsalsa_amd"; nothing else (no version, no command line): the text is a function of the
     inputs alone.
 S3. lines and their order.  One line per chain, in the chain table's order.  With unmapped = 1 a query record without a
     chain gets one unmapped line in its place in query record order: every read appears, and a pair's lines are adjacent.
 S4. roles within a query record.  The representative is the rank-primary chain (parent == own index) with the greatest
     score, the smallest index on a tie.  The other primaries are supplementary (0x800), the rank-secondaries secondary
     (0x100).
 S5. clips and CIGAR.  With oq the oriented query: left clip = q_start on strand 0, qlen - q_end on strand 1; right clip =
     the other remainder.  The CIGAR is the left clip, the runs, the right clip; zero-length clips are left out; a CIGAR
     without any run or clip is '*'.  The representative clips with S, supplementary and secondary lines with H.  With
     eqx = 1 the runs are written as they are (=, X, I, D); with eqx = 0 every maximal stretch of neighbouring = and X runs
     becomes one M run.
 S6. SEQ.  A byte is folded to upper case; A, C, G, T stay (on strand 1 they are complemented and the read reversed); every
     other byte becomes N.  Representative: the whole oriented read.  Supplementary: oq's aligned part only.  Secondary: '*'.
     Unmapped: the read as the file holds it, folded the same way.  A SEQ without bases is '*'.  QUAL is always '*'.  (The
     = / X letters are rule 10's, on the bytes as the stores hold them: on lower-case or non-ACGT input they can disagree
     with a comparison of SEQ against the reference; on upper-case ACGT input they cannot.)
 S7. columns of a chain line.  QNAME: the query name; with mates a trailing "/1" or "/2" is removed when the name is longer
     than two bytes.  FLAG: S8.  RNAME: the target name.  POS: t_start + 1.  MAPQ: the rank row's mapq.  CIGAR: S5.  RNEXT,
     PNEXT, TLEN: S8.  SEQ, QUAL: S6.  Then the tags, in this order: NM:i:<nm>, AS:i:<score>, cm:i:<n_anchors>, s2:i:<sub>
     (representative and supplementary lines only), tp:A:P (primaries) or tp:A:S (secondaries), nb:i:<n_best> (lines with
     cls = 1 only), MD:Z:<md> (with md = 1).
 S8. FLAG and the mate columns.  0x10 iff strand = 1; 0x100 and 0x800 by S4.  Without mates: RNEXT '*', PNEXT 0, TLEN 0.
     With mates: 0x1 on every line; 0x40 on the lines of record 2p, 0x80 on those of record 2p + 1; 0x2 iff cls = 1.  The
     mate line of a chain is `mate` if cls = 1, else the representative of the partner record, else none.  If it exists:
     0x20 iff it is on strand 1; RNEXT is '=' on the same target, else its target's name; PNEXT is its POS; on the same
     target TLEN's magnitude is max(t_end) - min(t_start) over the two, positive on the line with the smaller t_start and
     negative on the other, on equal t_start the line of record 2p is the positive one (for a proper pair this is +- rule
     13's tl); on different targets TLEN is 0.  If no mate line exists: 0x8, RNEXT '=', PNEXT = own POS, TLEN 0.
 S9. unmapped lines.  FLAG 0x4, plus 0x1 and 0x40 / 0x80 with mates.  With a mate line (paired only: the representative of
     the partner record): 0x20 iff it is reverse; RNAME and POS are the mate line's; RNEXT '='; PNEXT is the mate line's
     POS; TLEN 0.  Without: 0x8 too when paired; RNAME '*', POS 0, RNEXT '*', PNEXT 0, TLEN 0.  In both cases MAPQ 0,
     CIGAR '*', no tags.
S10. MD (with md = 1).  Walk the runs with the target bytes folded as in S6 (no complement).  = columns add to a running
     count; an X column writes the count, the target base, and resets the count; a D run writes the count, '^', the target
     bases, and resets the count; I runs do nothing (they do not split a count); the final count is written.  So the string
     begins and ends with a number; neighbouring mismatches, and a mismatch next to a deletion, are separated by 0.
S11. batches and limits.  Resident for a run: the two stores, the names, the chain, rank and mate rows with every chain's
     FLAG and mate line, the run tables with their scans.  Per batch of consecutive query records (whole pairs with mates):
     the line table, the per-line sizes and their 64-bit scan, the class lists, the text.  A line's text bound is
     1024 + qlen + 11 * (runs + 2), with md = 1 plus 2 * (t_end - t_start) + 11 * (runs + 1); an unmapped line's is
     1024 + qlen.  msgpu_sam_batch_bytes(params, lines, text bound) bounds the device bytes of a batch; the cut is the
     mapper's greedy cut (rule 9) on msgpu_sam_batch_bytes <= budget with fewer than 2^31 lines per batch; budget_bytes = 0
     stands for the free device memory once the resident part is allocated (an eighth less, again and again, while the
     device cannot give the largest batch's bytes as one block).  The batches' texts one behind the other, behind the header,
     are the file.  A record (with mates: a pair) that exceeds the budget alone is MSGPU_E_NOMEM naming it.  Fewer than 2^31
     chains and runs, fewer than 2^32 lines; the file limits are the mapper's.  Every limit is an error, never a fault.  On
     any error there is no result.
For instance target t = ACGTACGTACGTACGTACGT, query q = TTCGTGGTAACG, one chain: strand 0, q 2..11, t 5..14, runs
3= 1X 1D 2= 1I 2=, score 40, 3 anchors, primary, mapq 60, with md = 1:
  q\t0\tt\t6\t60\t2S3=1X1D2=1I2=1S\t*\t0\t0\tTTCGTGGTAACG\t*\tNM:i:3\tAS:i:40\tcm:i:3\ts2:i:0\ttp:A:P\tMD:Z:3A0^C4
and with eqx = 0 the CIGAR is 2S4M1D2M1I2M1S.
Out of scope: base qualities (the stores keep none), the SA:Z and MC:Z tags, BAM, coordinate sorting.
"""
import contextlib
import ctypes as C
import os

import numpy as np

from . import _lib
from ._stage import StageError, stage_context, text_view

__all__ = ["SamError", "Context", "run_tables", "run_pointers", "batch_bytes", "DEFAULTS"]

DEFAULTS = dict(eqx=True, md=False, unmapped=True)
COUNTS = tuple(n for n, t in _lib.SamStats._fields_ if t is C.c_uint64)


class SamError(StageError):
    """A rejected table, input or parameter, or a device failure."""

    def __init__(self, code, detail=""):
        super().__init__(code, detail=detail)


def Context(device=0):
    """a device context of the stage for any number of ``run_tables(..., context=...)``; a context manager"""
    return stage_context("sam", device, SamError)


def batch_bytes(n_lines, text_bound):
    """msgpu_sam_batch_bytes (S11): the bound on the device bytes of a batch; no device call"""
    prm = _lib.SamParams(1, 0, 1, 0)
    return int(_lib.lib().msgpu_sam_batch_bytes(C.byref(prm), int(n_lines), int(text_bound)))


def _rows(rows, dtype, what, n):
    if len(rows) != n:
        raise SamError(_lib.E_ARG, "%d chains, %d %s" % (n, len(rows), what))
    table = np.zeros(n, dtype=dtype)
    for i, r in enumerate(rows):
        table[i] = tuple(int(x) for x in r)
    return table


def run_tables(targets, queries, chains, ops, off, ranks, mates=None, out=None, eqx=True, md=False, unmapped=True, budget_mb=None,
               budget_bytes=None, device=0, context=None, timings=None):
    """The stage on given tables: ``chains`` holds per chain the tuple (query, target, strand, anchors, score, nm, q_start, q_end,
    t_start, t_end, matches, block) in output order, ``ops`` the runs of all chains (len << 4 | op) and ``off`` the n + 1 offsets
    of the chains' runs in it, ``ranks`` per chain (parent, sub, n_secondary, mapq) and ``mates`` (None: single-end) per chain
    (mate, tlen, cls, n_best), as ``mapper.run``'s tables have them.  Returns (text, lines, stats): the text as bytes, per
    alignment line the tuple (chain, query, flag, offset) with chain = None for an unmapped line, and the counts of
    msgpu_sam_stats with ``batches`` (a dict per batch with the fields of msgpu_sam_batch).  ``out`` (a path) receives the text
    (nothing on an error).  ``budget_mb`` / ``budget_bytes`` bound the device memory of a batch (neither: the free device
    memory).  ``timings`` (a dict) receives seconds per step; ``context`` is an entered Context to run on."""
    if budget_mb is not None and budget_bytes is not None:
        raise TypeError("budget_mb and budget_bytes: one budget")
    budget = 0 if budget_mb is None else max(1, int(float(budget_mb) * (1 << 20)))
    if budget_bytes is not None:
        budget = max(1, int(budget_bytes))
    n = len(chains)
    table = _rows(chains, _lib.MAP_CHAIN_DTYPE, "chains", n)
    rank_rows = _rows(ranks, _lib.MAP_RANK_DTYPE, "rank rows", n)
    mate_rows = None if mates is None else _rows(mates, _lib.MAP_MATE_DTYPE, "mate rows", n)
    off_a = np.array([int(x) for x in off], dtype=np.uint64)
    ops_a = np.array([int(x) for x in ops], dtype=np.uint32)
    if len(off_a) != n + 1:
        raise SamError(_lib.E_ARG, "%d chains, %d offsets" % (n, len(off_a)))
    if n and int(off_a[n]) > len(ops_a):
        raise SamError(_lib.E_ARG, "off[%d] = %d, %d runs" % (n, int(off_a[n]), len(ops_a)))
    text, lines, stats = run_pointers(targets, queries, table.ctypes.data, n, ops_a.ctypes.data, off_a.ctypes.data, rank_rows.ctypes.data,
                                      None if mate_rows is None else mate_rows.ctypes.data, eqx=eqx, md=md, unmapped=unmapped, budget=budget,
                                      device=device, context=context, timings=timings)
    if out is not None:
        with open(out, "wb") as h:
            h.write(text)
    return text, lines, stats


def run_pointers(targets, queries, chains, n, ops, off, ranks, mates, eqx=True, md=False, unmapped=True, budget=0, device=0, context=None,
                 timings=None, lines=True):
    """msgpu_sam_run on tables that lie in memory already (addresses; ``mates`` None: single-end), as the mapper's result holds
    them: nothing is converted.  Returns (text, lines, stats) as run_tables does; ``lines`` = False leaves the line table out."""
    prm = _lib.SamParams(1 if eqx else 0, 1 if md else 0, 1 if unmapped else 0, 0)
    L = _lib.lib()
    with (stage_context("sam", device, SamError) if context is None else contextlib.nullcontext(context)) as stage:
        with stage.run(C.byref(prm), os.fsencode(targets), os.fsencode(queries), chains, n, ops, off, ranks, mates, 0, int(budget)) as res:
            st = _lib.SamStats()
            L.msgpu_sam_result_stats(res, C.byref(st))
            text = bytes(text_view(L.msgpu_sam_result_text, res))
            table = []
            if lines:
                lp, m = C.POINTER(_lib.SamLine)(), C.c_uint64()
                L.msgpu_sam_result_lines(res, C.byref(lp), C.byref(m))
                rows = (np.frombuffer((C.c_char * (24 * m.value)).from_address(C.addressof(lp.contents)), dtype=_lib.SAM_LINE_DTYPE)
                        if m.value else [])
                table = [(None if int(r["chain"]) == _lib.SAM_UNMAPPED else int(r["chain"]), int(r["query"]), int(r["flag"]), int(r["offset"]))
                         for r in rows]
            bp, m = C.POINTER(_lib.SamBatch)(), C.c_uint64()
            L.msgpu_sam_result_batches(res, C.byref(bp), C.byref(m))
            batches = [{f: int(getattr(bp[i], f)) for f, _ in _lib.SamBatch._fields_} for i in range(m.value)]
    if timings is not None:
        timings.update({name[:-3]: getattr(st, name) / 1e3 for name, t in _lib.SamStats._fields_ if t is C.c_float})
    stats = dict({(name[2:] if name.startswith("n_") else name): int(getattr(st, name)) for name in COUNTS},
                 params={name: int(getattr(st.params, name)) for name in DEFAULTS}, batches=batches)
    return text, table, stats
