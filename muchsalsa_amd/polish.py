"""The pipeline's polishing step on the GPU: a pile-up consensus of a draft assembly from the reads mapped onto it.

    python -m muchsalsa_amd.polish <draft.fa> <reads.fa|fq> <out.fa> [--rounds N] [--min-depth N] [--min-identity N] [--paf F]
            [-k N] [-w N] [--max-occ N] [--min-score N] [--min-count N] [--max-gap N] [--bandwidth N] [--band N] [--budget-mb N]
            [--extend N] [--min-mapq N] [--mates] [--max-insert N] [--vcf F]

prints one JSON line of counts and seconds.  Each round maps the reads onto the draft with muchsalsa_amd.mapper in cigar mode
(its rule 10; the options of the second line are the mapper's) and lets the chains vote; the output of a round is the draft of
the next.  With ``--min-mapq N`` (0..60) the mapping also ranks the chains (the mapper's rule 12) and rule 2 takes its ranked
form.  With ``--mates`` the reads file is an interleaved file of pairs (``mapper.interleave``), the mapping marks the proper pairs
(the mapper's rule 13, ``--max-insert N`` its longest template) and rule 2 takes its mates form; it does not combine with
``--min-mapq``.  ``--paf F`` keeps the last round's PAF in F.  ``--vcf F`` writes what the polish changed as VCF 4.2 into F
(rules V1 - V9 below; one round only).  The reference tree has no polisher: the stage is defined by the rules
below, in integers only, and checked, without tolerance, against the tests' restatement in plain Python (tests/pl_oracle.py).
The rules (include/msgpu.h, "pileup consensus"); parameters min_depth (>= 1, default 3) and min_identity (a percentage, 0..100,
default 0):

 1. tables.  The input is a chain table (the fields of msgpu_map_chain, the reads as queries and the draft as targets) and per
    chain its runs, each len << 4 | op.  Per chain: (a) its query record is not smaller than the previous chain's; (b) strand
    is 0 or 1; (c) the query record and (d) the target record are in range; (e) t_start < t_end <= tlen; (f) q_start <= q_end
    <= qlen; (g) every run has len >= 1 and an op in {1 = I, 2 = D, 7 = '=', 8 = X}; (h) the runs consume exactly
    t_end - t_start target bases ('=', X, D) and (i) q_end - q_start query bases ('=', X, I); a run that breaks (g) consumes
    nothing.  The violation reported is that of the smallest chain index, and of that chain the first in the order (a) .. (i):
    MSGPU_E_ARG, "chain <i>: <what>".  The check is a device pass that publishes the smallest bad chain through the scalar
    block, and it is complete before any kernel walks a run: a bad table ends in an error, never in a fault.  In ranked form
    (``ranks`` given; msgpu_pl_run_ranked) a check (j) is added and reported last: the rank row's parent is in range and names a
    chain of the same query record that is its own parent, and mapq <= 60; otherwise "chain <i>: rank".  In mates form
    (``mates`` given; msgpu_pl_run_mates) a check (k) is added and reported last: cls <= 1 on every row, and for a row with
    cls == 1 the mate is in range, the mate's row has cls == 1 and names this chain, the mate's query record is this one's ^ 1,
    and n_best >= 1; otherwise "chain <i>: mates".
 2. voters.  A chain is eligible iff matches * 100 >= min_identity * block.  Per query record the voter is the eligible chain
    with the greatest score, then the greatest block, then the first in table order.  Every other chain is ignored and counted.
    Ranked form (with the mapper's rule 12 rows): a chain votes iff it is eligible, primary (parent == its own index) and
    mapq >= min_mapq.  So a read may have several voters (a split alignment votes with every part), a secondary never votes, and
    a read placed equally on two repeat copies (mapq 0) votes only at min_mapq = 0.  Everything behind the voters' spans is the
    same in both forms.  Mates form (with the mapper's rule 13 rows): a chain votes iff it is eligible, selected (cls == 1)
    and n_best == 1.  So a pair placed equally well twice does not vote, an unselected chain never votes, and a read inside a
    repeat copy votes on the copy that its mate names.  Everything behind the voters' spans is the same code in all three forms.
 3. oriented query.  Column j of a chain reads byte q_start + j_q of the query for strand 0 (j_q: the query bases that the
    columns in front of j consume); for strand 1 the oriented query is MSGPU_COPY_REVCOMP's of the whole record (reversed,
    A <-> T and C <-> G in upper case, every other byte as it is), and the chain starts at qlen - q_end in it.  The byte is then
    folded to upper case; A, C, G and T vote for themselves, any other byte votes "other".
 4. pile-up.  Per draft base six 32-bit counters: A, C, G, T, del, other.  An '=' or X column of a voter adds the class of its
    query byte at its target position, a D column adds del; depth(p) is the sum of the six.  An I run of length L of a voter
    that lies between target positions p - 1 and p is one insertion event at slot p; it is usable iff L <= 32 and all its bytes
    are A, C, G or T, and is then keyed (slot, L, the letters packed at 2 bits, the first in the highest bits); an unusable
    event is counted and ignored, and so is an I run that is the first or the last run of its chain.
 5. call, per position p.  depth(p) < min_depth, or A = C = G = T = del = 0: the draft's byte, verbatim.  Else the winner is the
    greatest of A, C, G, T, del; on a tie the draft's own folded base if it is among the tied, else the first of A, C, G, T,
    del.  The winner is the draft's folded base: the draft's byte, verbatim (case is kept: a polish that changes nothing is
    the identity on bytes); del: nothing; else the winner's upper-case letter.
 6. insertions, per slot p with 0 < p < tlen of a record: the usable events are grouped by (L, letters); the candidate is the
    group with the greatest count, then the smaller L, then the smaller packed letters; with m = min(depth(p - 1), depth(p)) it
    is applied iff m >= min_depth and 2 * count > m, and its letters are emitted in front of position p's call.  (Usable events
    at other slots are counted and never applied.)
 7. output.  The records in the draft's order: '>' + the cleaned name + a line feed, then the bases in lines of 60; a record
    that comes out without bases is the header and an empty line.  On any error nothing is written.
 8. limits, each an error and never a fault: the file limits are the mapper's; fewer than 2^31 chains and runs, fewer than 2^40
    columns of voters, a polished record below 2^32 bases.  Device memory: 45 bytes per draft base (the six counters, the
    slot's winner, the call, the output length and its scan), 40 bytes per run, 60 bytes per insertion event (with the sort
    buffers) and the output must fit beside the two stores, else MSGPU_E_NOMEM naming the sizes.  Batching over reads is out
    of scope.

On request (``vcf=PATH``, ``--vcf F``; MSGPU_PL_VCF) the edits are also written as VCF 4.2, formatted on the device
(msgpu_vcf.hip) and checked without tolerance against tests/vcf_oracle.py.  Without it nothing of this runs, and with it the
FASTA, the record table and the counts are what they are without it.  Per draft record of tlen bases; e(p): rule 5 substituted or
deleted position p; ins(p): the letters rule 6 applies at slot p (empty for p = 0 and p = tlen):

 V1. blocks.  A block is a maximal run [a, b) of positions with e(p); it owns the applied insertions at slots a .. b, both ends
     included.  An applied insertion at a slot p with neither e(p - 1) nor e(p) is a block of its own with a = b = p.  Every
     position heads at most one block, and blocks never touch: an unchanged position lies between two of them.
 V2. alleles.  REF0 = the draft's bytes of [a, b), folded to upper case, any byte outside ACGT written N.  ALT0 = ins(a) call(a)
     ins(a + 1) call(a + 1) ... call(b - 1) ins(b), for a = b ins(a) alone: the bytes the polisher emits for the block, always
     upper-case ACGT.
 V3. anchoring.  Both non-empty: POS = a + 1, REF = REF0, ALT = ALT0.  One of them empty and a > 0: the draft's byte at a - 1
     (unchanged by maximality; folded, non-ACGT as N) is put in front of both, POS = a.  One empty, a = 0 and b < tlen: the
     draft's byte at b is put behind both, POS = 1.  a = 0 and b = tlen (the whole record deleted): POS = 1, REF = the folded
     first base, ALT = <DEL>, and INFO gains END=<tlen> in front of DP.  Indels inside repeats are not left-aligned: positions
     are where the alignment put them (out of scope).
 V4. INFO, integers only.  DP = the minimum of depth(p) over [a, b), for a = b min(depth(a - 1), depth(a)).  AO = the minimum
     over the block's edits of their support: the winning counter at an edited position, the applied group's count at an
     applied slot.  TYPE = ins if REF0 is empty; del if ALT0 is empty; snp or mnp if |REF0| = |ALT0| (1, or more) and the block
     holds neither a deletion nor an insertion; complex otherwise.
 V5. line.  <name> TAB <POS> TAB . TAB <REF> TAB <ALT> TAB . TAB PASS TAB [END=n;]DP=d;AO=a;TYPE=t LF, in draft-record order,
     then by a.
 V6. header, written on the host: ##fileformat=VCFv4.2, ##source=muchsalsa_amd.polish, one ##contig=<ID=name,length=tlen> per
     draft record in order, ##INFO lines for DP, AO, TYPE and END, ##ALT=<ID=DEL,...>, and the #CHROM ... INFO line without
     sample columns.  A draft without variants is the header alone.
 V7. names, checked only when VCF is asked for: a draft record is refused with MSGPU_E_ARG naming the record if its cleaned name
     is empty, longer than 254 bytes, holds a byte outside 0x21..0x7e or one of , < >, begins with * or =, or repeats an earlier
     record's name (the loader keeps the first of two records of one id, so a file read through it never does).  Nothing is
     written in that case, and the context goes on.
 V8. rounds.  A VCF's coordinates are those of the draft of its own round: VCF with more than one round is a TypeError, from
     the command usage and exit status 2.
 V9. limits, each an error and never a fault: fewer than 2^31 blocks; the extra device memory (12 bytes per draft base, 72
     bytes per block, the text) is compared with what is free where the sizes are known, else MSGPU_E_NOMEM naming them.
"""
import contextlib
import ctypes as C
import json
import os
import sys
import time

import numpy as np

from . import _lib, mapper
from ._stage import StageError, stage_context, text_view

__all__ = ["PolishError", "Context", "run_tables", "run", "main", "DEFAULTS"]

DEFAULTS = dict(min_depth=3, min_identity=0)
CHAIN_DTYPE = np.dtype([(n, "<i4" if n == "score" else "<u4") for n, _ in _lib.MapChain._fields_])
COUNTS = tuple(n for n, t in _lib.PlStats._fields_ if t is C.c_uint64)
RECORD = tuple(n for n, _ in _lib.PlRecord._fields_)
VARIANT = tuple(n for n, _ in _lib.PlVariant._fields_)
VCF_COUNTS = tuple(n for n, t in _lib.PlVcfStats._fields_ if t is C.c_uint64)


class PolishError(StageError):
    """A rejected table, input or parameter, or a device failure."""

    def __init__(self, code, detail=""):
        super().__init__(code, detail=detail)


def Context(device=0):
    """a device context of the stage for any number of ``run_tables(..., context=...)``; a context manager"""
    return stage_context("pl", device, PolishError)


def _strip(name):
    return name[2:] if name.startswith("n_") else name


def run_tables(draft, reads, out, chains, runs, device=0, tables=None, timings=None, context=None, ranks=None, min_mapq=0, mates=None,
               vcf=None, **params):
    """The stage on given tables: ``chains`` holds per chain the tuple (query, target, strand, anchors, score, nm, q_start, q_end,
    t_start, t_end, matches, block) and ``runs`` per chain the list of len << 4 | op, as muchsalsa_amd.mapper's ``tables`` have
    them (reads = queries, draft = targets).  Writes ``out`` (nothing on an error); returns the counts of msgpu_pl_stats.
    ``params``: the names of DEFAULTS.  ``tables`` (a dict) receives ``records`` (per draft record the tuple of RECORD) and
    ``text`` (bytes); ``timings`` (a dict) seconds per step; ``context`` an entered Context to run on (``device`` is not read).
    ``ranks`` (per chain the tuple (parent, sub, n_secondary, mapq) of the mapper's rule 12, as ``mapper.run(..., rank=True)`` and
    ``mapper.rank_tables`` give it) switches rule 2 to its ranked form with ``min_mapq``.  ``mates`` (per chain the tuple (mate,
    tlen, cls, n_best) of the mapper's rule 13, as ``mapper.run(..., mates=True)`` and ``mapper.mate_tables`` give it) switches
    rule 2 to its mates form; giving both is a TypeError.  ``vcf`` (a path; None: off) also writes what the polish changed as
    VCF 4.2 (rules V1 - V9) into it, when the run succeeds: ``tables`` then receives ``vcf`` (bytes) and ``variants`` (per
    line the tuple of VARIANT), the returned dict a key ``vcf`` with the counts of msgpu_pl_vcf_stats (VCF_COUNTS), and
    ``timings`` the seconds ``vcf``; on an error neither file is written."""
    unknown = set(params) - set(DEFAULTS)
    if unknown:
        raise TypeError("unknown parameters: %s" % ", ".join(sorted(unknown)))
    p = dict(DEFAULTS, **params)
    t0 = time.perf_counter()
    L = _lib.lib()
    if len(chains) != len(runs):
        raise PolishError(_lib.E_ARG, "%d chains, %d run lists" % (len(chains), len(runs)))
    if ranks is not None and mates is not None:
        raise TypeError("ranks and mates: rule 2 takes one form")
    if mates is not None and len(mates) != len(chains):
        raise PolishError(_lib.E_ARG, "%d chains, %d mate rows" % (len(chains), len(mates)))
    if ranks is not None and len(ranks) != len(chains):
        raise PolishError(_lib.E_ARG, "%d chains, %d rank rows" % (len(chains), len(ranks)))
    if ranks is not None and not 0 <= int(min_mapq) < (1 << 32):
        raise PolishError(_lib.E_ARG, "min_mapq = %d" % int(min_mapq))
    for name, v in p.items():
        if not -(1 << 31) <= int(v) < (1 << 31):
            raise PolishError(_lib.E_ARG, "%s = %d" % (name, int(v)))
    table = np.zeros(len(chains), dtype=CHAIN_DTYPE)
    for i, ch in enumerate(chains):
        table[i] = tuple(int(x) for x in ch)
    off = np.zeros(len(runs) + 1, dtype=np.uint64)
    off[1:] = np.cumsum([len(r) for r in runs], dtype=np.uint64)
    ops = np.fromiter((x for r in runs for x in r), dtype=np.uint32, count=int(off[-1]))
    prm = _lib.PlParams(int(p["min_depth"]), int(p["min_identity"]))
    if ranks is not None:
        rows = np.zeros(len(ranks), dtype=_lib.MAP_RANK_DTYPE)
        for i, r in enumerate(ranks):
            rows[i] = tuple(int(x) for x in r)
    if mates is not None:
        rows = np.zeros(len(mates), dtype=_lib.MAP_MATE_DTYPE)
        for i, r in enumerate(mates):
            if not all(0 <= int(x) < (1 << 32) for x in r):
                raise PolishError(_lib.E_ARG, "mate row %d: %r" % (i, tuple(r)))
            rows[i] = tuple(int(x) for x in r)
    flags = _lib.PL_VCF if vcf is not None else 0
    vst = None
    with (stage_context("pl", device, PolishError) if context is None else contextlib.nullcontext(context)) as stage:
        with (stage.run(C.byref(prm), os.fsencode(draft), os.fsencode(reads), table.ctypes.data, len(chains), ops.ctypes.data,
                        off.ctypes.data, rows.ctypes.data, flags, fn="run_mates") if mates is not None else
              stage.run(C.byref(prm), os.fsencode(draft), os.fsencode(reads), table.ctypes.data, len(chains), ops.ctypes.data,
                        off.ctypes.data, flags) if ranks is None else
              stage.run(C.byref(prm), os.fsencode(draft), os.fsencode(reads), table.ctypes.data, len(chains), ops.ctypes.data,
                        off.ctypes.data, rows.ctypes.data, int(min_mapq), flags, fn="run_ranked")) as res:
            st = _lib.PlStats()
            L.msgpu_pl_result_stats(res, C.byref(st))
            text = text_view(L.msgpu_pl_result_text, res)
            if tables is not None:
                rp, m = C.POINTER(_lib.PlRecord)(), C.c_uint64()
                L.msgpu_pl_result_records(res, C.byref(rp), C.byref(m))
                tables["records"] = [tuple(int(getattr(rp[i], f)) for f in RECORD) for i in range(m.value)]
                tables["text"] = bytes(text)
            if vcf is not None:
                vst = _lib.PlVcfStats()
                L.msgpu_pl_result_vcf_stats(res, C.byref(vst))
                vtext = text_view(L.msgpu_pl_result_vcf, res)
                if tables is not None:
                    vp, m = C.POINTER(_lib.PlVariant)(), C.c_uint64()
                    L.msgpu_pl_result_variants(res, C.byref(vp), C.byref(m))
                    raw = C.string_at(vp, m.value * C.sizeof(_lib.PlVariant)) if m.value else b""
                    tables["variants"] = [tuple(int(x) for x in row) for row in np.frombuffer(raw, dtype=_lib.PL_VARIANT_DTYPE).tolist()]
                    tables["vcf"] = bytes(vtext)
            t1 = time.perf_counter()
            with open(out, "wb") as h:
                h.write(text)
            if vcf is not None:
                with open(vcf, "wb") as h:
                    h.write(vtext)
            t_write = time.perf_counter() - t1
    if timings is not None:
        timings.update({name[:-3]: getattr(st, name) / 1e3 for name, t in _lib.PlStats._fields_ if t is C.c_float})
        timings["stage_wall"] = timings.pop("wall")
        timings.update({"file": t_write, "total": time.perf_counter() - t0})
        if vst is not None:
            timings["vcf"] = vst.vcf_ms / 1e3
    more = {} if vst is None else {"vcf": {_strip(name): int(getattr(vst, name)) for name in VCF_COUNTS}}
    return dict({_strip(name): int(getattr(st, name)) for name in COUNTS},
                params={name: int(getattr(st.params, name)) for name in DEFAULTS}, **more)


def run(draft, reads, out, rounds=1, budget_mb=None, device=0, paf=None, tables=None, timings=None, extend=0, min_mapq=None, mates=False,
        max_insert=_lib.MAP_MAX_INSERT_DEFAULT, vcf=None, **params):
    """``rounds`` times: mapper.run(draft_i, reads, ..., exact=1, cigar=1) and run_tables on its tables; the output of round i is
    the draft of round i + 1, the last one is ``out``.  Intermediate drafts and PAFs are written beside ``out`` and removed
    afterwards; ``paf`` keeps the last round's PAF.  ``params``: the names of DEFAULTS and of mapper.DEFAULTS (exact and ava are
    the stage's own).  Returns the last round's counts with ``rounds`` (per round ``map`` and ``polish``); ``tables`` and
    ``timings`` receive the last round's.  ``extend`` (0: off) is the mapper's rule 11 parameter for every round's mapping: the
    reads then vote beyond their outermost seeds too.  ``min_mapq`` not None switches the mapper's rule 12 on for every round's
    mapping and rule 2 to its ranked form: the PAF then carries the mapping quality and the tp / s2 tags.  ``mates`` = True:
    ``reads`` is an interleaved file of pairs (mapper.interleave), every round's mapping runs the mapper's rule 13 with
    ``max_insert`` and rule 2 takes its mates form; with ``min_mapq`` it is a TypeError (one form at a time).  ``vcf`` (a path):
    run_tables' ``vcf``; with more than one round it is a TypeError (rule V8: a VCF's coordinates are its own round's draft's)."""
    if mates and min_mapq is not None:
        raise TypeError("mates and min_mapq: rule 2 takes one form")
    rounds = int(rounds)
    if vcf is not None and rounds > 1:
        raise TypeError("vcf and rounds = %d: a VCF's coordinates are those of the draft of its own round (rule V8)" % rounds)
    unknown = set(params) - set(DEFAULTS) - (set(mapper.DEFAULTS) - {"exact", "ava"})
    if unknown or rounds < 1:
        raise TypeError("unknown parameters: %s" % ", ".join(sorted(unknown)) if unknown else "rounds = %d" % rounds)
    own = {k: v for k, v in params.items() if k in DEFAULTS}
    theirs = {k: v for k, v in params.items() if k not in DEFAULTS}
    made, per_round, current = [], [], draft
    try:
        for r in range(rounds):
            last = r == rounds - 1
            target = out if last else "%s.round%d.fa" % (out, r + 1)
            paf_r = paf if last and paf is not None else "%s.round%d.paf" % (out, r + 1)
            if paf_r != paf:
                made.append(paf_r)
            if not last:
                made.append(target)
            tb, tm = {}, {}
            ranked = min_mapq is not None
            paired = dict(mates=True, max_insert=max_insert) if mates else {}  # (without the option the calls are what they were)
            mapped = mapper.run(current, reads, paf_r, device=device, tables=tb, budget_mb=budget_mb, cigar=1, exact=1, extend=extend,
                                rank=ranked, **paired, **theirs)
            voters = dict(mates=tb["mates"]) if mates else {}
            if vcf is not None:  # (without the option the calls are what they were)
                voters["vcf"] = vcf
            got = run_tables(current, reads, target, tb["chains"], tb["runs"], device=device, tables=tables if last else None,
                             timings=tm, ranks=tb["ranks"] if ranked else None, min_mapq=min_mapq if ranked else 0, **voters, **own)
            per_round.append({"map": dict({k: mapped[k] for k in ("chains", "anchors", "pairs", "capped")},
                                          **({"mate": mapped["mate"]} if mates else {})), "polish": got})
            current = target
    finally:
        for path in made:
            if os.path.exists(path):
                os.remove(path)
    if timings is not None:
        timings.update(tm)
    return dict(per_round[-1]["polish"], rounds=per_round)


def main(argv):
    args, p, ok, budget, rounds, paf = list(argv), {}, True, None, 1, None
    opts = dict(mapper._OPTS, **{"--min-depth": "min_depth", "--min-identity": "min_identity", "--rounds": "rounds"})
    for name, key in opts.items():
        if name in args:
            i = args.index(name)
            try:
                p[key] = int(args[i + 1])
            except (IndexError, ValueError):
                ok = False
            del args[i:i + 2]
    if "--budget-mb" in args:
        i = args.index("--budget-mb")
        try:
            budget = float(args[i + 1])
            ok = ok and 0 < budget < float("inf")
        except (IndexError, ValueError):
            ok = False
        del args[i:i + 2]
    if "--paf" in args:
        i = args.index("--paf")
        ok = ok and i + 1 < len(args)
        paf = args[i + 1] if i + 1 < len(args) else None
        del args[i:i + 2]
    extend = 0
    if "--extend" in args:
        i = args.index("--extend")
        try:
            extend = int(args[i + 1])
            ok = ok and 1 <= extend <= _lib.MAP_EXTEND_MAX
        except (IndexError, ValueError):
            ok = False
        del args[i:i + 2]
    min_mapq = None
    if "--min-mapq" in args:
        i = args.index("--min-mapq")
        try:
            min_mapq = int(args[i + 1])
            ok = ok and 0 <= min_mapq <= 60
        except (IndexError, ValueError):
            ok = False
        del args[i:i + 2]
    vcf = None
    if "--vcf" in args:
        i = args.index("--vcf")
        ok = ok and i + 1 < len(args)
        vcf = args[i + 1] if i + 1 < len(args) else None
        del args[i:i + 2]
    mates, max_insert = "--mates" in args, _lib.MAP_MAX_INSERT_DEFAULT
    if mates:
        args.remove("--mates")
    if "--max-insert" in args:  # (implies --mates)
        i = args.index("--max-insert")
        try:
            max_insert = int(args[i + 1])
            ok = ok and 1 <= max_insert < (1 << 31)
        except (IndexError, ValueError):
            ok = False
        del args[i:i + 2]
        mates = True
    ok = ok and not (mates and min_mapq is not None)
    rounds = p.pop("rounds", 1)
    q = dict(mapper.DEFAULTS, **dict(DEFAULTS, **p))
    ok = ok and 4 <= q["k"] <= 32 and 1 <= q["w"] <= 64 and q["max_occ"] >= 1 and 1 <= q["band"] <= 127
    ok = ok and q["max_gap"] >= 0 and q["bandwidth"] >= 0 and q["min_depth"] >= 1 and 0 <= q["min_identity"] <= 100 and rounds >= 1
    ok = ok and len(args) == 3 and not any(a.startswith("-") for a in args) and not (vcf is not None and rounds > 1)
    if not ok:
        sys.stderr.write(__doc__.split("\n\n")[1] + "\n")
        return 2
    timings = {}
    paired = dict(mates=True, max_insert=max_insert) if mates else {}
    if vcf is not None:
        paired["vcf"] = vcf
    out = run(args[0], args[1], args[2], rounds=rounds, budget_mb=budget, paf=paf, timings=timings, extend=extend, min_mapq=min_mapq, **paired,
              **p)
    out["seconds"] = {key: round(v, 4) for key, v in timings.items()}
    print(json.dumps(out))
    return 0


if __name__ == "__main__":
    _lib.PRELOAD_TORCH = False  # this process never imports torch
    sys.exit(main(sys.argv[1:]))
