"""The pipeline's short-read unitig assembly on the GPU: what ``abyss-pe k=K name=NAME in='R1 R2' unitigs`` and the awk cut
at MINLENGTH behind it write in the reference pipeline -- ``NAME-unitigs.fa`` and ``NAME-unitigs.l500.fa`` -- from one or two
FASTQ files (the k-mer filter's outputs) alone.

    python -m muchsalsa_amd.unitigs <k> <in_1.fq> <in_2.fq> <out_all.fa> <out_cut.fa>
            [--min-count N] [--trim N] [--min-length N] [--budget-mb N] [--bubble N] [--gfa F] [--wide]

prints one JSON line of counts and seconds; with ``--gfa F`` the unitig graph is written to F as GFA 1 (rule 10), where
``abyss-pe graph=gfa`` leaves its adjacency graph beside the FASTA; ``--wide`` moves the upper bound of k from 64 to 128
(``run(..., wide=True)``; msgpu_ug_set_wide: k = 65..96 runs on keys of three 64-bit words, k = 97..128 on keys of four, k <= 64
as without it).  ABySS is not needed, and it is not part of the reference tree: the stage is
defined by the rules below and checked, without tolerance, against the tests' restatement in plain Python
(tests/ug_oracle.py), not against ABySS.  The rules (include/msgpu.h, "short-read unitig assembly"); parameters k (2..64, or 2..128 after msgpu_ug_set_wide),
min_count (>= 1, default 2), trim (>= 0, default k: the longest tip, in k-mers), min_length (default 500, the pipeline's
MINLENGTH), bubble (0..4096, default 0 = off: rule 9):

1. Input: one or two FASTQ files.  The FASTQ rules and the window rules are rules 1 and 2 of the k-mer abundance filter
   (muchsalsa_amd.kmer_filter), word for word, error code, file and line included.  The files are not pairs: their record
   counts may differ and the second may be missing.  count(x) = windows of all files whose canonical k-mer is x, exact.
2. Solid set S = the canonical k-mers with count >= min_count.
3. Oriented graph: every k-base string s whose canonical form is in S is an oriented node; s and rc(s) are two nodes of one
   k-mer, or one node if s is its own reverse complement.  succ(s) = { s[1:]+c : c in ACGT, canon(s[1:]+c) in S },
   pred(s) = { c+s[:-1] : c in ACGT, canon(c+s[:-1]) in S }.
4. Tip removal, in rounds on a snapshot of S.  The limits are 1, 2, 4, ... (doubling, every value below trim), then trim; each
   limit runs once, after that the round at trim repeats until a round removes nothing; trim = 0: no round.  In a round, for
   every oriented node s with pred(s) empty: path = [s], then repeat: if |succ(last)| != 1 stop, no tip; let t be the one
   successor; if |pred(t)| >= 2 the path is a tip, stop; if |path| = limit stop, no tip; else append t.  All k-mers of all
   tips of a round leave S together when the round ends.  Islands (dead at both ends) stay; the length cut deals with them.
   Each round's (limit, k-mers removed) is reported.
5. Unitigs: s -> t is joined iff succ(s) = {t}, pred(t) = {s}, neither s nor t is its own reverse complement and
   canon(s) != canon(t): no self-loop and no hairpin is ever joined.  Unitigs are the maximal chains of joined nodes; every
   k-mer of S lies in exactly one.  Every unitig exists as two mirror chains, which these rules make distinct (a one-node
   chain of a self-complementary k-mer exists once).  Linear chain: the one whose first k-mer, as a 2k-bit number, is smaller
   than its mirror's first k-mer is emitted (no tie is possible).  Cycle: it starts at the smallest oriented node among the
   cycle and its mirror and goes round once: n k-mers give n + k - 1 bases, the closing join is not written.  Sequence = the
   first k-mer and the last base of every further node, upper case.  coverage = sum of count over its k-mers (64 bits).
6. Output: the unitigs ascending by the first k-mer of the emitted orientation; id = rank in that order, over all unitigs,
   before any cut.  A record is ``>id length coverage\\n``, the sequence on one line, ``\\n`` (ABySS's header shape; the
   pipeline's awk reads field 2).  Two texts: all records, and the records with length >= min_length, ids unchanged.
7. Limits, each an error and never a fault: fewer than 2^31 solid k-mers; the file limits of the k-mer filter; everything
   resident in device memory together, else the stage fails naming the sizes.  On any error nothing is written.

9. Bubble popping, on request (``bubble``; msgpu_ug_set_bubbles).  The parameter is bubble >= 0, the longest branch in k-mers;
   0 means off, and rules 1-8 alone apply; a SNP makes branches of k k-mers, so values from k upwards are useful; values above
   4096 are MSGPU_E_ARG.
   (a) Simple branch.  All degrees are taken in the snapshot S of the round.  Let u be an oriented node with
       |succ(u)| >= 2, and b in succ(u).  If |pred(b)| != 1 there is no branch.  path = [b], then repeat: if
       |succ(last)| != 1 there is no branch; let t be the one successor; if |pred(t)| >= 2 the branch is path and its
       merge is t; otherwise, if |path| = bubble there is no branch; otherwise append t.  This is the tip walk of rule 4
       with a fork in front of it.  A successor of u that is itself a merge (|pred| >= 2) is no branch.
   (b) Bubble.  A bubble is a fork u, a merge t, and the >= 2 simple branches of u whose merge is t.  It must have
       canon(u) != canon(t): a bubble whose fork and merge are one k-mer is never popped (a palindromic passage).  The
       mirror of the bubble (u, t) is the bubble (rc(t), rc(u)).  A bubble is judged once, from the side whose fork is the
       smaller 2k-bit string: from u iff u < rc(t).
   (c) Winner.  The winner is the branch with the greatest mean count: branch A beats branch B iff
       sum(A) len(B) > sum(B) len(A), sum = the sum of count over the branch's k-mers, the products in 64 bits (the cap of
       4096 keeps them below 2^56).  Among equals, the branch entered from the judging fork by the smaller base c wins.
       Every k-mer of every other branch of the bubble leaves S.  One fork may hold several bubbles (different merges);
       each is judged alone.
   (d) Rounds.  A bubble round judges all bubbles on a snapshot; all losers leave together when the round ends.  A
       branch's inner nodes have in- and out-degree 1, so each k-mer lies in at most one branch of one bubble or its
       mirror, and no round removes a winner.  The neighbour bytes are refreshed behind a round as behind a tip round.
   (e) Order of the phases.  Rule 4 runs as it is.  Then a bubble phase: rounds repeat until a round removes nothing (that
       last round is recorded too).  If the bubble phase removed nothing in total, or trim = 0, cleaning is done.
       Otherwise a tip phase runs: the round at trim alone, repeated until it removes nothing; if it removed nothing,
       cleaning is done, otherwise the next bubble phase runs.  Rules 5-8 then run on what is left; n_solid_trimmed is
       what cleaning leaves.
   (f) Not done: complex bubbles (overlapping variants whose branches fork again or merge at different nodes) and
       zero-length branches are left alone, and there is no erosion.
10. The unitig graph as GFA 1, on request (``gfa``; msgpu_ug_set_graph).  It is off by default, and with it off every output,
    table, count and kernel launch of the stage is what rules 1-9 make it.  The rule is defined on what rules 1-9 leave.
    (a) Oriented unitigs.  Unitig i (its id is its rank, rule 6) exists as i+ and i-: i+ is the emitted chain and i- is its
        mirror.  A unitig that is one self-complementary k-mer exists as i+ only.  first(x) and last(x) are the first and
        the last oriented node of the oriented unitig x.
    (b) Adjacencies.  For every oriented unitig x and every t in succ(last(x)) (rule 3, on the cleaned set) there is an
        adjacency x -> y with first(y) = t.  Such a y always exists: an edge that rule 5 did not join ends at a node
        without a joined predecessor.  The closing join of a cycle is the adjacency i+ -> i+.
    (c) Mirror.  x -> y and y' -> x' are one link; ' flips the orientation.  As tuples (from id, from orientation, to id,
        to orientation) with + < -, the smaller of the two is written.  Equal tuples (a hairpin i+ -> i-) are written
        once.  A unitig that exists as i+ only has no i-, so an adjacency with such a unitig at either end has no mirror:
        it is written as it is and is counted with the self-mirrored links.  (A reader of GFA takes the mirror of
        x+ -> i+ to be i- -> x-, so the adjacency i+ -> x- needs a line of its own.)
    (d) Order.  The links are written ascending by that tuple.
    (e) Text, GFA 1.  The header "H\\tVN:Z:1.0\\n"; one line per unitig in id order,
        "S\\t<id>\\t<sequence>\\tLN:i:<length>\\tKC:i:<coverage>\\n", where sequence, length and coverage are exactly those of
        the FASTA record (rule 6); one line per link, "L\\t<from>\\t<+|->\\t<to>\\t<+|->\\t<k-1>M\\n".  All unitigs are
        written, with no length cut: links to short unitigs would otherwise dangle.
    (f) Limits, each an error and never a fault.  Rule 7's bound of fewer than 2^31 solid k-mers makes the tuple fit 64 bits
        (31 + 1 + 31 + 1); fewer than 2^32 links; device memory as in rule 7, MSGPU_E_NOMEM naming the sizes.  The counts
        obey adjacencies = 2 links - self-mirrored links.

Known differences from ``abyss-pe unitigs``, none of which could be checked against the program (it is not installed where
this project is built):

* exact counts, where ABySS 2 keeps its k-mers in a Bloom filter;
* bubble popping only on request, and only rule 9's simple bubbles: complex bubbles and zero-length branches are left
  alone; no erosion of the ends;
* islands are kept until the length cut;
* ids and the order of the records are this stage's;
* a sequence is one line.

The mask (rule 8 of include/msgpu.h).  ``run(..., pair=p, dropped=m)`` runs on a resident ``kmer_filter.Pair`` instead of
files; ``m`` is a byte per pair, 1 = dropped, what the k-mer filter returns as its verdicts.  The stage on a pair with the
mask m gives the result of the stage on the two files that hold the records with m = 0, in order: both texts, the unitig
table, the rounds, the windows, the distinct and solid k-mers before and after the tips, the unitig counts and the longest
chain.  ``records`` and ``bytes_in`` are the pair's own.  With a mask both files hold as many records as m has bytes.
"""
import ctypes as C
import json
import os
import sys
import time

from . import _lib
from ._stage import StageError, stage_context, text_view

__all__ = ["UnitigError", "BUBBLE_MAX", "run", "main"]


BUBBLE_MAX = 4096  # MSGPU_UG_BUBBLE_MAX


class UnitigError(StageError):
    """A rejected input or a device failure; ``line`` = 1-based line (0: none) of ``file`` (0 / 1: the first / second
    FASTQ)."""


def run(k, in_1, in_2, out_all, out_cut, device=0, min_count=2, trim=None, min_length=500, budget_mb=None, tables=None,
        timings=None, pair=None, dropped=None, bubble=None, gfa=None, wide=False):
    """The whole stage: writes ``out_all`` and ``out_cut``; returns the counts.  ``in_2`` may be None.  ``trim`` None: k.
    With ``pair`` (an entered kmer_filter.Pair) the stage runs on the resident files on the pair's device and ``in_1`` /
    ``in_2`` / ``device`` are not read; ``dropped`` (bytes or a uint8 array, one per pair, 1 = dropped) is the mask.
    ``budget_mb`` bounds the count's partition buffers (None: half of the free device memory).  ``tables`` (a dict)
    receives ``rounds`` [(limit, k-mers removed)] and ``unitigs`` [(length, coverage, first k-mer, offset of the sequence in
    the all text, cyclic)] in output order; ``timings`` (a dict) seconds per step (``files``: writing the two outputs), and ``round_seconds`` [(tips,
    neighbour bytes)] per round.  ``bubble`` (None or 0: off) is rule 9's parameter; the dict then holds ``bubble``,
    ``bubbles``, ``bubble_rounds`` [[tip rounds before it, bubbles, k-mers removed]], ``bubble_kmers`` and ``bubble_max_forks`` (the
    largest fork list of a round), ``tables`` receives
    ``bubble_rounds`` [(tip rounds before it, forks, bubbles, branches removed, k-mers removed)] and ``timings``
    ``bubble_forks`` / ``bubble_walk`` / ``bubble_adjacency`` (seconds).  ``gfa`` (None: off) is a path: rule 10's text is
    written there, the dict then holds ``links``, ``link_self_mirror``, ``dead_ends`` and ``gfa_bytes``, ``tables`` receives
    ``links`` [(from, from_rev, to, to_rev)] and ``timings`` ``graph_links`` / ``graph_sort`` / ``graph_text`` (seconds).
    ``wide`` = True moves the upper bound of k from 64 to 128 (msgpu_ug_set_wide); the first k-mer in ``unitigs`` is the whole
    k-mer at any k (msgpu_ug_result_first_kmers).  ``timings`` also receives ``peak_bytes``, not a time: the most device memory the run's
    own arena held at once (msgpu_ug_result_peak_bytes; a pair's files are not counted)."""
    L = _lib.lib()
    t0 = time.perf_counter()
    if dropped is not None and pair is None:
        raise TypeError("dropped needs pair")
    mask = None if dropped is None else bytes(bytearray(dropped))
    bubble = 0 if bubble is None else int(bubble)
    if not 0 <= bubble < (1 << 32):
        raise UnitigError(_lib.E_ARG, detail="bubble = %d" % bubble)
    with stage_context("ug", device if pair is None else pair.device, UnitigError) as stage:
        budget = 0 if budget_mb is None else max(1, int(float(budget_mb) * (1 << 20)))
        prm = _lib.UgParams(int(k), int(min_count) if 0 <= int(min_count) < (1 << 32) else 0, -1 if trim is None else int(trim),
                            min(max(int(min_length), 0), (1 << 32) - 1))
        if trim is not None and int(trim) < 0:
            raise UnitigError(_lib.E_ARG, detail="trim = %d" % int(trim))
        if bubble:
            stage.check(L.msgpu_ug_set_bubbles(stage.ctx, bubble))
        if gfa is not None:
            stage.check(L.msgpu_ug_set_graph(stage.ctx, 1))
        if wide:
            stage.check(L.msgpu_ug_set_wide(stage.ctx, 1))
        with (stage.run(C.byref(prm), os.fsencode(in_1), None if in_2 is None else os.fsencode(in_2), 0, budget) if pair is None
              else stage.run(C.byref(prm), pair.handle, mask, 0 if mask is None else len(mask), 0, budget, fn="run_pair")) as res:
            st = _lib.UgStats()
            L.msgpu_ug_result_stats(res, C.byref(st))
            rp, n = C.POINTER(_lib.UgRound)(), C.c_uint64()
            L.msgpu_ug_result_rounds(res, C.byref(rp), C.byref(n))
            rounds = [(int(rp[i].limit), int(rp[i].removed)) for i in range(n.value)]
            round_s = [(rp[i].tips_ms / 1e3, rp[i].adjacency_ms / 1e3) for i in range(n.value)]
            bs, bp = _lib.UgBubbleStats(), C.POINTER(_lib.UgBubbleRound)()
            L.msgpu_ug_result_bubbles(res, C.byref(bs), C.byref(bp), C.byref(n))
            bubble_rounds = [(int(b.after_tip_rounds), int(b.forks), int(b.bubbles), int(b.branches_removed), int(b.removed))
                             for b in (bp[i] for i in range(n.value))]
            if tables is not None:
                up = C.POINTER(_lib.UgUnitig)()
                L.msgpu_ug_result_unitigs(res, C.byref(up), C.byref(n))
                tables["rounds"] = rounds
                tables["bubble_rounds"] = bubble_rounds
                fp, fw = C.POINTER(C.c_uint64)(), C.c_uint32()
                L.msgpu_ug_result_first_kmers(res, C.byref(fp), C.byref(fw), C.byref(n))
                w = fw.value
                first = [sum(int(fp[i * w + j]) << (64 * j) for j in range(w)) for i in range(n.value)]
                tables["unitigs"] = [(int(u.length), int(u.coverage), first[i], int(u.offset), int(u.cyclic))
                                     for i, u in ((i, up[i]) for i in range(n.value))]
            peak = int(L.msgpu_ug_result_peak_bytes(res))
            gs, lp = _lib.UgGraphStats(), C.POINTER(_lib.UgLink)()
            L.msgpu_ug_result_links(res, C.byref(gs), C.byref(lp), C.byref(n))
            if tables is not None and gfa is not None:
                tables["links"] = [(int(getattr(l, "from")), int(l.from_rev), int(l.to), int(l.to_rev))
                                   for l in (lp[i] for i in range(n.value))]
            t1 = time.perf_counter()
            texts = ((out_all, _lib.UG_TEXT_ALL), (out_cut, _lib.UG_TEXT_CUT))
            for path, which in texts if gfa is None else texts + ((gfa, _lib.UG_TEXT_GFA),):
                with open(path, "wb") as h:
                    h.write(text_view(L.msgpu_ug_result_text, res, which))
            t_write = time.perf_counter() - t1
    if timings is not None:
        timings.update({name[:-3]: getattr(st, name) / 1e3 for name, _ in _lib.UgStats._fields_ if name.endswith("_ms")})
        timings["stage_wall"] = timings.pop("wall")
        timings.update({"bubble_" + name[:-3]: getattr(bs, name) / 1e3 for name in ("forks_ms", "walk_ms", "adjacency_ms")})
        if gfa is not None:
            timings.update({"graph_" + name[:-3]: getattr(gs, name) / 1e3 for name in ("links_ms", "sort_ms", "text_ms")})
        timings.update({"files": t_write, "total": time.perf_counter() - t0, "round_seconds": round_s, "peak_bytes": peak})
    graph = {} if gfa is None else {"links": int(gs.n_links), "link_self_mirror": int(gs.n_self_mirror),
                                    "dead_ends": int(gs.n_dead_ends), "gfa_bytes": int(gs.gfa_bytes)}
    return dict({"k": int(st.k), "min_count": int(st.min_count), "trim": int(st.trim), "min_length": int(st.min_length),
            "records": [int(x) for x in st.n_records], "windows": int(st.n_windows), "distinct": int(st.n_distinct),
            "solid": int(st.n_solid), "solid_after": int(st.n_solid_trimmed), "tip_rounds": int(st.n_tip_rounds),
            "rounds": [list(r) for r in rounds], "unitigs": int(st.n_unitigs), "kept": int(st.n_unitigs_kept),
            "cycles": int(st.n_cycles), "longest": int(st.longest_chain), "doubling_rounds": int(st.doubling_rounds),
            "partitions": int(st.n_partitions), "largest_partition": int(st.largest_partition),
            "lost_publications": int(st.n_lost_publications), "bytes_in": [int(x) for x in st.bytes_in],
            "bytes_out": [int(x) for x in st.bytes_out], "bubble": int(bs.bubble), "bubbles": int(bs.n_bubbles),
            "bubble_rounds": [[r[0], r[2], r[4]] for r in bubble_rounds], "bubble_kmers": int(bs.n_kmers_removed),
            "bubble_max_forks": int(bs.max_forks)}, **graph)


def main(argv):
    args = list(argv)
    opts = {"--min-count": 2, "--trim": None, "--min-length": 500, "--budget-mb": None, "--bubble": 0, "--gfa": None}
    wide = "--wide" in args
    if wide:
        args.remove("--wide")
    ok = True
    for name in opts:
        if name in args:
            i = args.index(name)
            try:
                opts[name] = (float if name == "--budget-mb" else str if name == "--gfa" else int)(args[i + 1])
                ok = ok and not (name == "--gfa" and (not opts[name] or opts[name].startswith("--")))
            except (IndexError, ValueError):
                ok = False
            del args[i:i + 2]
    try:
        k = int(args[0]) if args else 0
    except ValueError:
        ok = False
    ok = ok and opts["--min-count"] >= 1 and (opts["--trim"] is None or opts["--trim"] >= 0) and opts["--min-length"] >= 0
    ok = ok and (opts["--budget-mb"] is None or opts["--budget-mb"] > 0) and not any(a.startswith("--") for a in args)
    ok = ok and 0 <= opts["--bubble"] <= BUBBLE_MAX
    if not ok or len(args) != 5:
        sys.stderr.write(__doc__.split("\n\n")[1] + "\n")
        return 2
    timings = {}
    out = run(k, args[1], args[2], args[3], args[4], min_count=opts["--min-count"], trim=opts["--trim"],
              min_length=opts["--min-length"], budget_mb=opts["--budget-mb"], timings=timings, bubble=opts["--bubble"],
              gfa=opts["--gfa"], wide=wide)
    rs = timings.pop("round_seconds")
    out["seconds"] = {key: round(v, 4) for key, v in timings.items()}
    out["round_seconds"] = [[round(a, 5), round(b, 5)] for a, b in rs]
    print(json.dumps(out))
    return 0


if __name__ == "__main__":
    _lib.PRELOAD_TORCH = False  # this process never imports torch
    sys.exit(main(sys.argv[1:]))
