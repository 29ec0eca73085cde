"""The pipeline's mapping step on the GPU: what its four ``minimap2 -k15 -w5 -m100 -g10000 -r2000 --max-chain-skip 25`` calls
write -- a PAF of every record of a query file against every record of a target file, by minimizer seeds and a chaining DP.

    python -m muchsalsa_amd.mapper <targets.fa|fq> <queries.fa|fq> <out.paf> [-k N] [-w N] [--exact] [--cigar] [--ava]
            [--max-occ N] [--min-score N] [--min-count N] [--max-gap N] [--bandwidth N] [--band N] [--budget-mb N]
            [--extend N] [--rank] [--mates] [--max-insert N] [--sam F] [--md] [--cigar-m]

prints one JSON line of counts and seconds.  ``--budget-mb`` (N > 0) bounds the device memory of a batch of query records
(rule 9; without it: the free device memory).  With ``--ava`` the two paths name the same file (the reads against
themselves: the read-to-read PAF muchsalsa_amd.scrubber takes as its fourth input); ``--exact`` adds the base-level match
count of the PAF muchsalsa itself parses (the pipeline's ``-c --eqx`` call); ``--cigar`` (which implies ``--exact``) aligns
every segment base by base (rule 10): column 10 is then the number of ``=`` columns, column 11 the number of alignment columns,
and the line ends in a ``cg:Z:`` string of ``=``, ``X``, ``I`` and ``D`` runs; ``--extend N`` (1..65535, which implies
``--cigar``) extends every chain beyond its outermost seeds by up to N bases at either end (rule 11); ``--rank`` marks every chain
as primary or secondary and writes a mapping quality into column 12 (rule 12); ``--mates`` reads the query file as interleaved
pairs and marks the proper pair of every pair (rule 13), ``--max-insert N`` (1..2^31 - 1, default 1000, which implies
``--mates``) is its longest template; ``--sam F`` (which implies ``--cigar`` and ``--rank``) also writes the chains as SAM 1.6 text
into F, formatted on the device by muchsalsa_amd.sam (its rules S1 - S11): with ``--mates`` the mate rows become the pair's flags
and mate columns, ``--md`` adds the MD tag and ``--cigar-m`` writes M in place of = and X; the PAF is written as before.
minimap2 is not needed, and it is not part of
the reference tree: the stage is defined by the rules below, in integers only, and checked, without tolerance, against the
tests' restatement in plain Python (tests/map_oracle.py), not against minimap2.  The rules (include/msgpu.h,
"unitig-to-read mapping"); parameters k (4..32, default 15), w (1..64, 5), max_occ (>= 1, 200), max_gap (10000), bandwidth
(2000), max_pred (fixed at 64), min_score (100), min_count (3), exact (0 / 1), band (1..127, 64), ava (0 / 1); cigar (0 / 1),
extend (0..65535), rank (False / True), mates (False / True) and max_insert are keywords of ``run`` beside them:

 1. windows: the alphabet, case folding, 2-bit code, canonical key (min(fw, rc) as 2k-bit numbers) and the break at any
    other byte are those of the k-mer filter's rolling window (KfRoll).  A stretch is a maximal run of k-mer start
    positions without a break.  The strand bit of a position is 1 iff rc < fw.
 2. minimizers: h(i) = kf_hash(key(i)).  A window is w consecutive k-mer start positions inside one stretch; a stretch with
    fewer than w positions has none.  A window's minimizer is its position with the smallest (h, position).  A sequence's
    minimizers are the union over its windows, each position once.
 3. index: every target minimizer as (key, target record, position, strand).  A key with more than max_occ entries is left
    out whole; the number of keys and entries left out is reported.
 4. anchors: every query minimizer meets every index entry of its key.  Relative strand s = query strand ^ target strand,
    x = the target position, y = the query position if s = 0, else qlen - k - position (the position in the
    reverse-complemented query, so a collinear chain rises in both coordinates on both strands).  With ava the query file
    is the target file, and an anchor is kept only if the query record index is smaller than the target record index.  A
    group is (query record, target record, s); its anchors are ordered by (x, y); equal (x, y) cannot occur.
 5. chaining, per group over the anchors 0..n-1 in that order: f(i) = max(k, max over j in [max(0, i - 64), i) of
    f(j) + gain - pen), taken over the j with dx = x_i - x_j > 0, dy = y_i - y_j > 0, dx <= max_gap, dy <= max_gap and
    dd = |dx - dy| <= bandwidth; gain = min(dx, dy, k); pen = 0 if dd = 0, else (dd * k) / 100 + (floor(log2(dd)) >> 1)
    with integer division.  pred(i) is the j that gives the maximum, the largest such j on a tie; it is "none" when k
    alone is at least as good.
 6. chains: the anchors of a group are visited by (f descending, index ascending).  An unused anchor starts a chain; the
    chain follows pred over unused anchors and ends before the first used anchor u or at "none";
    score = f(start) - (f(u) if it ended at a used anchor, else 0); all its anchors become used.  The chain is emitted iff
    score >= min_score and it has at least min_count anchors.  A group with fewer than min_count anchors, or with
    n * k < min_score, can emit nothing and is dropped before the DP.
 7. figures of a chain with anchors a_0 < ... < a_{m-1} (rising x).  For each link i >= 1: c_i = min(dx, dy, k),
    lt_i = dx - c_i, lq_i = dy - c_i; the link's segment is target [x_i + k - c_i - lt_i, x_i + k - c_i) against the
    oriented query [y_i + k - c_i - lq_i, y_i + k - c_i); d_i = that pair's Levenshtein distance inside band with
    msgpu_edit_distance's semantics, min(distance, band + 1), over the bytes as the stores hold them (the oriented query
    of s = 1 is MSGPU_COPY_REVCOMP's: reversed, A <-> T and C <-> G in upper case, every other byte as it is); if
    lt_i = lq_i = 0 then d_i = 0; d_i is computed only in exact mode.  block = k + sum (c_i + max(lt_i, lq_i)).  Seed
    mode: matches = k + sum c_i.  Exact mode: matches = k + sum (c_i + max(lt_i, lq_i) - d_i), never negative because
    d_i <= max(lt_i, lq_i).  Target range [x_0, x_{m-1} + k).  Query range in forward coordinates: [y_0, y_{m-1} + k) for
    s = 0, [qlen - y_{m-1} - k, qlen - y_0) for s = 1.
 8. output: one line per chain: the twelve PAF columns ('+' / '-' in column 5, mapping quality 255), then cm:i:<anchors>,
    s1:i:<score> and, in exact mode, NM:i:<sum d_i>.  Lines are ordered by (query record, target record, strand, order of
    emission in the group).  On any error nothing is written.
 9. limits and batches.  Limits, each an error and never a fault: fewer than 2^31 index entries, anchors and segment pairs
    per batch, at most 2^30 distinct target keys; a record shorter than 2^31 bases, a file below 2^38; a group's n * k
    below 2^31.  Resident while the index lives (``Index``): the target store, its sketch and the index (sorted entries,
    distinct keys, counts, starts, hash table); resident for the whole run besides: the query store and sketch, the
    anchor count of every query minimizer and its 64-bit exclusive scan.  Everything whose size
    depends on the anchors exists per batch of consecutive query records (a group never spans two query records, and rule 8
    orders by query record first, so the batches' lines one behind the other are the PAF of the whole input): the anchors
    and their sort buffers, the groups, classes and lists, f, pred, the sort keys, the chains with their table and, in
    exact mode, the segment pairs, their distances and the oriented copies of the batch's query records (2 * their bases).
    msgpu_map_batch_bytes(params, anchors, query bases) bounds the device bytes of a batch.  The cut is greedy: with a(r),
    b(r) the anchors and bases of query record r, a batch starts at the first record not yet taken and takes consecutive
    records while msgpu_map_batch_bytes(params, sum a, sum b) <= budget and sum a < 2^31; it holds at least one record;
    records without anchors join the running batch; no query records, no batches.  budget_bytes > 0 is the budget of a
    batch (the resident part is not counted); 0 stands for the free device memory once the resident part is allocated (an
    eighth less, again and again, while the device cannot give the largest batch's bytes as one block).  A
    record that exceeds the budget on its own is MSGPU_E_NOMEM, one with 2^31 anchors or more MSGPU_E_ARG, naming the
    record, its anchors and the bytes against the budget.  Splitting one query record over ranges of targets, and
    splitting the index, are out of scope.
10. the alignment of one segment pair, and cigar mode (cigar = 1, which needs exact = 1).  a is the target bytes, n of them,
    b the oriented query bytes, m of them, compared as the stores hold them (rule 7); ks = m - n; slide(i, k) is the largest
    i' >= i with a[i..i') == b[i+k..i'+k), i' <= n, i'+k <= m.  The table: G_0[0] = slide(0, 0) and nothing else is defined
    in row 0.  For e >= 1 and |k| <= e the candidates of cell (e, k) are X: G_{e-1}[k] + 1, valid iff G_{e-1}[k] is defined
    and < min(n, m - k); D (a target base without a query base): G_{e-1}[k+1] + 1, valid iff G_{e-1}[k+1] is defined and
    < n; I (a query base without a target base): G_{e-1}[k-1], valid iff it is defined and G_{e-1}[k-1] + k <= m.
    x0(e, k) is the largest valid candidate (none: the cell is undefined), G_e[k] = slide(x0, k), and the cell's op is the
    first of X, D, I whose candidate is valid and equals x0.  d is the first e with G_e[ks] = n; the pair is capped when
    |ks| > band or no such e <= band exists, and then d_i = band + 1 as in rule 7.  The script is read backwards from
    (d, ks): G_e[k] - x0 ``=`` columns lie behind the cell's op, which leads to (e-1, k) for X, (e-1, k+1) for D,
    (e-1, k-1) for I; row 0 ends the walk with G_0[0] leading ``=`` columns.  Only valid candidates enter: one that would
    step outside the matrix is no edit (rule 7's clamped recurrence may hold such values; they are harmless for the number,
    not for a script).  The script has exactly d columns that are not ``=``, every ``=`` column holds equal bytes and every
    X column unequal ones, and it consumes exactly n and m bytes.  With cigar = 1 a chain's alignment is k ``=`` columns
    for anchor 0, then for every link in rising order the segment's script followed by c_i ``=`` columns (seed bases:
    ``=`` by rule 1's case folding even where the bytes differ in case); a link with lt_i = lq_i = 0 has no segment; a
    capped segment is written lt_i D then lq_i I, zero lengths left out; neighbouring runs of one letter are merged.
    matches = the ``=`` columns, block = all columns, nm = block - matches.  The line is the twelve columns, cm, s1,
    NM:i:<nm>, then cg:Z:<runs> in target-forward order, which is the oriented query's order on both strands.  The runs
    consume exactly t_end - t_start target bases and q_end - q_start query bases; for a chain without a capped segment
    matches is at least rule 7's exact-mode value (a segment has at least max(lt, lq) columns, d of them no ``=``).  Rule 9
    with cigar = 1: msgpu_map_batch_bytes adds the slab of the scripts' tables (slots * (band + 1)^2 words, a constant
    number of slots that MSGPU_ALIGN_SLOTS=<n> lowers; no slab for a band of at most 31, whose tables all lie in LDS) to
    the fixed part and, per anchor, band + 1 words of script, the
    64-bit offset, the script length, the class list entry, the ``=`` columns behind the segment and the two column
    counts.  Without cigar every byte of every output is as before.
11. end extension, on request (``extend``; msgpu_map_set_extension).  The parameter is extend = E: 0 is off, 1..65535 the
    longest flank on either sequence; E > 0 needs cigar = 1 (and so exact = 1), else the run fails with MSGPU_E_ARG naming
    both.  The penalty is a constant of the rule, P = 8.  (1) Flanks of a chain with anchors a_0..a_{m-1}, oq the oriented
    query of rule 7, tlen and qlen the lengths, rev byte reversal (no complement: oq is oriented already).  Right:
    A = target[t_end .. t_end + n), n = min(E, tlen - t_end); B = oq[yE .. yE + m), yE = y_{m-1} + k, m = min(E, qlen - yE).
    Left: A = rev(target[x_0 - n .. x_0)), n = min(E, x_0); B = rev(oq[y_0 - m .. y_0)), m = min(E, y_0).  (2) The table is
    rule 10's on (A, n, B, m), rows e = 0..band: the same slide, the same three candidates with the same validity tests
    (only candidates that stay inside the matrix enter), the same tie order X, D, I.  Nothing of rule 10's end test is used:
    |m - n| may exceed the band and no row ends the table early.  (3) Every defined cell has x = G_e[k], y = x + k and
    score = x + y - P * e.  The end cell (e*, k*) is the one with the greatest score; on equal scores the smaller e wins,
    then the smaller |k|, then the negative k.  Cell (0, 0) always exists with score 2 * G_0[0] >= 0, so the end cell
    exists, and x* = y* = 0 means "no extension".  A row e with n + m - P * e <= the best score of the rows before it cannot
    win, nor can a later one: ``rows``, the number of rows an end is charged with, is the first such e, or band + 1.
    (4) The script is the walk back from (e*, k*) exactly as rule 10 walks back from (d, ks): e* + 1 words, consuming
    exactly x* bytes of A and y* bytes of B, every ``=`` column equal and every X column unequal; a left flank's columns are
    written in reverse order.  (5) The chain: its runs are the left columns, rule 10's chain alignment, the right columns,
    neighbouring runs merged; t_start -= x*_L, t_end += x*_R; the oriented query range grows by y*_L and y*_R and rule 7
    turns it into forward coordinates; matches, block and nm are counted on the columns; cm, s1, n_anchors, score, the
    chain's place in the output order and which chains exist are untouched.  The runs consume exactly the new target and
    query ranges.  (6) With E = 0 every byte is as before.  It follows that a flank whose shorter side matches the longer
    side's start without an edit is extended to that sequence's end: cell (0, 0) wins.  Rule 9 with E > 0:
    msgpu_map_batch_bytes_ext adds, per anchor, two ends' descriptors (24 bytes each), end cells (24 bytes each) and
    band + 1 script words each; the slab is cigar mode's.
12. primaries, secondaries and mapping quality, on request (``rank``; msgpu_map_set_ranking; off by default; it needs no other
    mode: seed, exact, cigar, ava and extend all combine with it).  The chains of one query record, over all targets and both
    strands, with their indices in output order (rule 8), are ranked among themselves.  For a chain c: len(c) = q_end - q_start
    of rule 7's forward query range, and ov(c, p) = max(0, min(q_end_c, q_end_p) - max(q_start_c, q_start_p)).  Rule 11 changes
    no rank: rule 12 reads the ranges as rule 7 leaves them, before any extension.  (1) Visiting order: by (score descending,
    output index ascending).  (2) A visited chain c is compared with the primaries visited before it, in visiting order: the
    first primary p with 2 * ov(c, p) > min(len(c), len(p)) makes c secondary with parent(c) = p; if there is none, c is
    primary and parent(c) = c.  The mask level is one half and the comparison is strict.  (3) Of a primary p: sub(p) is the
    greatest score among its secondaries, 0 if it has none; n_secondary(p) is the number of its secondaries s with
    10 * score(s) >= 9 * score(p); both are 0 for a secondary.  (4) mapq of a primary with s1 = score(p) > 0:
    (60 * (s1 - sub) * min(n_anchors, 10)) / (10 * s1), the products in 64 bits, integer division, clamped to 0..60; 0 if
    s1 <= 0; 0 for a secondary.  (5) With ranking on column 12 is mapq and the tags are tp:A:P or tp:A:S, cm:i, s1:i,
    s2:i:<sub>, then NM and cg as before; line order, every other column, the chain table and the run tables are untouched.
    (6) With ranking off every byte is as before: 255, no tp, no s2.  (7) A query record's chains never span two batches (rule
    9), so the rule runs per batch; parent is an index into the whole run's chain table; with ranking on a run has fewer than
    2^32 chains, else MSGPU_E_ARG.  msgpu_map_batch_bytes_rank bounds a batch (104 bytes per anchor and a fixed 24 * 256 bytes
    more than msgpu_map_batch_bytes_ext).  The mask level 1/2, the ratio 0.9 and the mapq formula are choices modelled on
    minimap2's, unchecked on real reads.
13. mates, on request (``mates``; msgpu_map_set_mates(ctx, on, max_insert); off by default; it needs no other mode: seed, exact,
    cigar, extend and rank all combine with it; with ava it is MSGPU_E_ARG).  The query file is interleaved: records 2p and
    2p + 1 are mate 1 and mate 2 of pair p; the names are not compared; an odd number of query records is MSGPU_E_ARG naming
    the count.  max_insert is 1..2^31 - 1, default 1000.  The rule reads the chain table as the run leaves it, behind rule
    11's extension.  (1) Concordant: chain a of record 2p and chain b of record 2p + 1 are concordant iff they have the same
    target record, their strands differ, and with f the chain of strand 0 and r the chain of strand 1:
    f.t_start <= r.t_start, f.t_end <= r.t_end (the forward mate lies to the left and neither passes the other) and
    tl = r.t_end - f.t_start <= max_insert.  Either mate may be the forward one.  (2) Selection: among the concordant
    combinations of a pair one is selected: the greatest score(a) + score(b) (a 64-bit sum), then the smaller tl, then the
    smaller index of a, then the smaller index of b.  n_best is the number of concordant combinations whose sum equals the
    greatest sum, whatever their tl, clamped to 2^32 - 1.  (3) Rows, one per chain in output order, {mate, tlen, cls,
    n_best}: the two selected chains have cls = 1, mate = the other's index in the whole run's chain table, tlen = tl and
    the pair's n_best; every other chain has {0xffffffff, 0, 0, 0}.  (4) Counts (msgpu_map_mstats): the pairs of the input,
    proper pairs, ambiguous pairs (proper with n_best > 1), discordant pairs (chains on both mates, none concordant),
    single pairs (chains on one mate only), unmapped pairs, the pairs per kernel class, the largest pair in chains, the
    sum, minimum and maximum of tlen over the proper pairs (integers: no order reaches them) and the step's device time.
    (5) With mates on every line carries pr:A:P or pr:A:U behind s1:i (behind s2:i with ranking on); a P line also carries
    mi:i:<the mate's line, 0-based>, tl:i:<tlen>, nb:i:<n_best>; NM and cg follow as before; line order and every other
    column are untouched.  (6) With mates off every byte of every output is as before.  (7) Rule 9 with mates on: the unit
    of the greedy cut is the pair: a batch starts at an even record and holds whole pairs, a(p) = a(2p) + a(2p + 1) and
    likewise the bases; a pair that exceeds the budget on its own is MSGPU_E_NOMEM naming the pair; with mates on a run has
    fewer than 2^32 chains, else MSGPU_E_ARG.  msgpu_map_batch_bytes_mates bounds a batch (it equals
    msgpu_map_batch_bytes_rank for mates = 0): per anchor it adds 60 bytes (three words of segment heads, numbers and
    starts, the count of mate 1's chains, three words of class lists, 16 bytes of the pair's selection, the row) and a fixed
    12 * 256 bytes.  (8) Orientation FR only, the selection order and n_best are choices modelled on short-read mappers,
    unchecked on real reads.

Known differences from minimap2, none of which could be checked against the program (it is not installed where this project
is built):

* the hash is the project's (kf_hash), not minimap2's;
* leftmost-minimum windows;
* an absolute occurrence cap (max_occ) instead of a fraction of the distinct minimizers;
* a fixed window of 64 predecessors instead of the skip heuristic of ``--max-chain-skip``;
* an integer gap cost;
* no ``--dual`` / ``-D`` diagonal filtering beyond the ava rule;
* primary / secondary marking and a mapping quality only with ``--rank`` (rule 12): without it all chains are kept unmarked,
  as with ``-P``, and column 12 is 255; rule 12 decides by query overlap alone, and its integer formula has none of
  minimap2's chain-length terms;
* no CIGAR without ``--cigar``: exact mode alone gives a match count that is a lower bound from unit-cost distances per
  link, not minimap2's count of ``=`` columns.  With ``--cigar`` the columns are counted on a unit-cost alignment of every
  segment between two seeds (rule 10), not on minimap2's affine-gap alignment, and a segment beyond the band is written
  as a deletion and an insertion;
* end extension: none without ``--extend``; with it, rule 11 (unit costs, P = 8, no end bonus);
* pairs: none without ``--mates``; with it, rule 13: orientation FR only, one insert bound and no insert-size model, no mate
  rescue, the selection order (score sum, then the shorter template, then the chains' indices) and n_best are choices
  modelled on short-read mappers, unchecked on real reads.

``Index(targets, k=, w=)`` is a context manager that keeps the targets' store, sketch and index on the device;
``run(None, queries, out, index=ix, ...)`` then maps onto it, any number of times, with any parameters but k and w (the
occurrence cap is applied at look-up).  With ava the index's own records are the queries.  Every result equals that of
the run by files.
"""
import contextlib
import ctypes as C
import json
import os
import sys
import time

import numpy as np

from . import _lib
from ._stage import StageError, stage_context, text_view

__all__ = ["MapError", "Index", "run", "rank_tables", "mate_tables", "interleave", "main", "DEFAULTS"]

DEFAULTS = dict(k=15, w=5, max_occ=200, max_gap=10000, bandwidth=2000, min_score=100, min_count=3, exact=0, band=64, ava=0)


class MapError(StageError):
    """A rejected input or parameter, or a device failure."""

    def __init__(self, code, detail=""):
        super().__init__(code, detail=detail)


def _params(p):
    return _lib.MapParams(int(p["k"]), int(p["w"]), int(p["max_occ"]), int(p["max_gap"]), int(p["bandwidth"]), 64,
                          int(p["min_score"]), int(p["min_count"]), int(p["exact"]), int(p["band"]), int(p["ava"]),
                          int(p.get("cigar", 0)))


class Index:
    """The targets resident in device memory with their sketch and index (msgpu_map_index), in a mapper context of its own.
    ``stats`` holds the counts and the seconds of the build.  One index serves any number of ``run(..., index=ix)``."""

    def __init__(self, targets, device=0, k=DEFAULTS["k"], w=DEFAULTS["w"]):
        self.targets, self.device, self.k, self.w = targets, device, int(k), int(w)
        self.handle, self._stack, self.stats = C.c_void_p(), None, None

    def __enter__(self):
        with contextlib.ExitStack() as stack:
            self.stage = stack.enter_context(stage_context("map", self.device, MapError))
            self.create()
            stack.callback(self.free)
            self._stack = stack.pop_all()
        return self

    def create(self):
        """(again, after free(): the context holds one index at a time)"""
        L = _lib.lib()
        prm = _params(dict(DEFAULTS, k=self.k, w=self.w))
        self.stage.check(L.msgpu_map_index_create(self.stage.ctx, C.byref(prm), os.fsencode(self.targets), C.byref(self.handle)))
        st = _lib.MapIndexStats()
        L.msgpu_map_index_stats(self.handle, C.byref(st))
        self.stats = {"records": int(st.n_records), "bases": int(st.n_bases), "minimizers": int(st.n_minimizers),
                      "keys": int(st.n_keys), "index_entries": int(st.n_index_entries), "k": int(st.k), "w": int(st.w),
                      "seconds": {n[:-3]: getattr(st, n) / 1e3 for n, _ in _lib.MapIndexStats._fields_ if n.endswith("_ms")}}

    def free(self):
        if self.handle:
            _lib.lib().msgpu_map_index_free(self.handle)
            self.handle = C.c_void_p()

    def __exit__(self, *exc):
        self._stack.close()
        return False


def _rank_stats(rst):
    return dict({name: int(getattr(rst, name)) for name, t in _lib.MapRankStats._fields_ if t is not C.c_float},
                seconds={"rank": rst.rank_ms / 1e3})


def rank_tables(chains, device=0, context=None, stats=None):
    """Rule 12 on a chain table (msgpu_map_rank_tables): ``chains`` holds per chain the tuple ``tables["chains"]`` of ``run`` has
    (only query, anchors, score, q_start and q_end are read), in output order.  Returns per chain the tuple (parent, sub,
    n_secondary, mapq), parent an index into ``chains``.  ``context``: an entered ``stage_context("map", ...)`` or an Index's
    ``stage``; ``stats`` (a dict) receives the counts of msgpu_map_rstats."""
    table = np.zeros(len(chains), dtype=_lib.MAP_CHAIN_DTYPE)
    for i, ch in enumerate(chains):
        table[i] = tuple(int(x) for x in ch)
    rows = np.zeros(len(chains), dtype=_lib.MAP_RANK_DTYPE)
    L = _lib.lib()
    with (stage_context("map", device, MapError) if context is None else contextlib.nullcontext(context)) as stage:
        stage.check(L.msgpu_map_rank_tables(stage.ctx, table.ctypes.data, len(chains), rows.ctypes.data))
        if stats is not None:
            rst = _lib.MapRankStats()
            L.msgpu_map_rank_tables_stats(stage.ctx, C.byref(rst))
            stats.update(_rank_stats(rst))
    return [tuple(int(x) for x in r) for r in rows]


def _mate_stats(mst):
    return dict({name: int(getattr(mst, name)) for name, t in _lib.MapMateStats._fields_ if t is not C.c_float},
                seconds={"mates": mst.mate_ms / 1e3})


def mate_tables(chains, max_insert=_lib.MAP_MAX_INSERT_DEFAULT, device=0, context=None, stats=None):
    """Rule 13 on a chain table (msgpu_map_mate_tables): ``chains`` holds per chain the tuple ``tables["chains"]`` of ``run`` has
    (only query, target, strand, score, t_start and t_end are read), in output order.  Returns per chain the tuple (mate, tlen,
    cls, n_best), mate an index into ``chains``.  ``context``: an entered ``stage_context("map", ...)`` or an Index's ``stage``;
    ``stats`` (a dict) receives the counts of msgpu_map_mstats (n_pairs: the pairs with a chain)."""
    if not 0 <= int(max_insert) < (1 << 32):
        raise MapError(_lib.E_ARG, "max_insert = %d" % int(max_insert))
    table = np.zeros(len(chains), dtype=_lib.MAP_CHAIN_DTYPE)
    for i, ch in enumerate(chains):
        table[i] = tuple(int(x) for x in ch)
    rows = np.zeros(len(chains), dtype=_lib.MAP_MATE_DTYPE)
    L = _lib.lib()
    with (stage_context("map", device, MapError) if context is None else contextlib.nullcontext(context)) as stage:
        stage.check(L.msgpu_map_mate_tables(stage.ctx, table.ctypes.data, len(chains), int(max_insert), rows.ctypes.data))
        if stats is not None:
            mst = _lib.MapMateStats()
            L.msgpu_map_mate_tables_stats(stage.ctx, C.byref(mst))
            stats.update(_mate_stats(mst))
    return [tuple(int(x) for x in r) for r in rows]


def interleave(in_1, in_2, out):
    """Two FASTQ files of four-line records, mate 1's and mate 2's in the same order, streamed into one interleaved file (record
    2p from ``in_1``, 2p + 1 from ``in_2``): rule 13's query file.  Host only.  Returns the pairs; ValueError on unequal record
    counts or on a record that is not ``@name``, bases, ``+``, as many qualities (``out`` is then removed).  The sequence loader
    keeps the reference's reading of FASTQ, in which a quality line that starts with ``@`` is taken for a description line; that
    would drop records and shift every pair behind it, so such a quality line is written with ``A`` (the next quality) as its
    first byte.  The mapper reads no qualities; every other byte is copied."""
    def record(h, path, number):
        lines = [h.readline() for _ in range(4)]
        if not lines[0]:
            return None
        if (not lines[3] or not lines[0].startswith(b"@") or not lines[2].startswith(b"+") or
                len(lines[1].rstrip(b"\r\n")) != len(lines[3].rstrip(b"\r\n")) or not lines[1].rstrip(b"\r\n")):
            raise ValueError("%s: record %d is not a four-line FASTQ record" % (path, number))
        if lines[3].startswith(b"@"):
            lines[3] = b"A" + lines[3][1:]
        return b"".join(line if line.endswith(b"\n") else line + b"\n" for line in lines)

    pairs = 0
    try:
        with open(in_1, "rb") as h1, open(in_2, "rb") as h2, open(out, "wb") as o:
            while True:
                r1, r2 = record(h1, in_1, pairs), record(h2, in_2, pairs)
                if r1 is None and r2 is None:
                    return pairs
                if r1 is None or r2 is None:
                    raise ValueError("%s has %s records than %s (%d pairs read)" % (in_1, "fewer" if r1 is None else "more", in_2, pairs))
                o.write(r1)
                o.write(r2)
                pairs += 1
    except ValueError:
        with contextlib.suppress(OSError):
            os.remove(out)
        raise


def run(targets, queries, out, device=0, tables=None, timings=None, budget_mb=None, index=None, cigar=0, extend=0, rank=False, mates=False,
        max_insert=_lib.MAP_MAX_INSERT_DEFAULT, sam=None, sam_md=False, sam_m=False, **params):
    """The whole stage: writes ``out`` (nothing on an error); returns the counts, among them ``batches`` (rule 9's cut: a dict
    per batch with the fields of msgpu_map_batch) and ``budget_bytes`` (what a batch had).  ``params``: the names of DEFAULTS.
    ``budget_mb`` bounds the device memory of a batch (None: the free device memory).  With
    ava = 1, ``queries`` is None or ``targets``.  ``tables`` (a dict) receives ``chains``: per line of the PAF the tuple
    (query, target, strand, anchors, score, nm, q_start, q_end, t_start, t_end, matches, block) and ``text`` (bytes);
    ``timings`` (a dict) seconds per step.  With ``index`` (an entered Index) the run maps onto it: ``targets`` and ``device``
    are not read, k and w default to the index's, and with ava = 1 ``queries`` is None.  ``cigar`` = 1 (rule 10; it needs
    exact = 1) writes the base-level figures and a ``cg:Z:`` string per line; ``tables`` then also receives ``cigars`` (a list
    of strings, one per line) and ``runs`` (per line the list of len << 4 | BAM code), and the returned dict's ``align``
    holds the counts and seconds of msgpu_map_astats.  ``extend`` = E > 0 (rule 11; it needs cigar = 1) extends every chain at
    both ends; the returned dict then has ``extend`` (the fields of msgpu_map_xstats, the time under ``seconds``) and ``tables``
    receives ``ext``: per line the pair (left end, right end), each (e, k, x, y, score, rows).  The value is set on the context
    for this run: an ``index`` serves runs with any extend, one after the other.  ``rank`` = True (rule 12) marks primaries and
    secondaries and writes the mapping quality; the result then carries ``ranks`` (per line the tuple (parent, sub, n_secondary,
    mapq)) and ``rank`` (the counts of msgpu_map_rstats, the time under ``seconds``); ``tables`` receives ``ranks`` too.  Like
    extend it is set on the context for this run.  ``mates`` = True (rule 13) reads ``queries`` as interleaved pairs with
    ``max_insert`` as the longest template; the result then carries ``mates`` (per line the tuple (mate, tlen, cls, n_best)) and
    ``mate`` (the counts of msgpu_map_mstats, the time under ``seconds``); ``tables`` receives ``mates`` too.  Set on the context
    for this run, like rank.  ``sam`` = PATH also writes the chains as SAM into PATH (muchsalsa_amd.sam, from the result's own
    tables; with ``mates`` the mate rows are passed on): it implies cigar = 1, exact = 1 and rank = True, ``sam_md`` adds the MD
    tag, ``sam_m`` writes M runs; the returned dict then has ``sam`` (the counts of msgpu_sam_stats).  The PAF in ``out`` is that
    of the same run without ``sam``; on any error neither file is written."""
    if sam is not None:
        cigar, rank, params = 1, True, dict(params, exact=1)
    if index is not None:
        params = dict({"k": index.k, "w": index.w}, **params)
    unknown = set(params) - set(DEFAULTS)
    if unknown:
        raise TypeError("unknown parameters: %s" % ", ".join(sorted(unknown)))
    p = dict(DEFAULTS, **params)
    L = _lib.lib()
    t0 = time.perf_counter()
    budget = 0 if budget_mb is None else max(1, int(float(budget_mb) * (1 << 20)))
    for name, v in p.items():
        if not -(1 << 31) <= int(v) < (1 << 31) or (name == "max_occ" and int(v) < 0):
            raise MapError(_lib.E_ARG, "%s = %d" % (name, int(v)))
    qpath = None if queries is None else os.fsencode(queries)
    with (stage_context("map", device, MapError) if index is None else contextlib.nullcontext(index.stage)) as stage:
        prm = _params(dict(p, cigar=cigar))
        if not 0 <= int(extend) < (1 << 32):
            raise MapError(_lib.E_ARG, "extend = %d" % int(extend))
        stage.check(L.msgpu_map_set_extension(stage.ctx, int(extend)))
        stage.check(L.msgpu_map_set_ranking(stage.ctx, 1 if rank else 0))
        if not 0 <= int(max_insert) < (1 << 32):
            raise MapError(_lib.E_ARG, "max_insert = %d" % int(max_insert))
        stage.check(L.msgpu_map_set_mates(stage.ctx, 1 if mates else 0, int(max_insert)))
        with (stage.run(C.byref(prm), os.fsencode(targets), qpath, 0, budget) if index is None else
              stage.run(C.byref(prm), index.handle, qpath, 0, budget, fn="run_index")) as res:
            st = _lib.MapStats()
            L.msgpu_map_result_stats(res, C.byref(st))
            text = text_view(L.msgpu_map_result_text, res)
            bp = C.POINTER(_lib.MapBatch)()
            m = C.c_uint64()
            L.msgpu_map_result_batches(res, C.byref(bp), C.byref(m))
            batches = [{f: int(getattr(bp[i], f)) for f, _ in _lib.MapBatch._fields_} for i in range(m.value)]
            budget_used = int(L.msgpu_map_result_budget(res))
            ast = _lib.MapAlignStats()
            L.msgpu_map_result_align_stats(res, C.byref(ast))
            xst = _lib.MapExtStats()
            L.msgpu_map_result_ext_stats(res, C.byref(xst))
            rst, ranks = _lib.MapRankStats(), None
            L.msgpu_map_result_rank_stats(res, C.byref(rst))
            if rst.ranking:
                rp, m = C.POINTER(_lib.MapRank)(), C.c_uint64()
                L.msgpu_map_result_ranks(res, C.byref(rp), C.byref(m))
                rows = (np.frombuffer((C.c_char * (16 * m.value)).from_address(C.addressof(rp.contents)), dtype=_lib.MAP_RANK_DTYPE)
                        if m.value else [])
                ranks = [tuple(int(x) for x in r) for r in rows]
            mst, mate_rows = _lib.MapMateStats(), None
            L.msgpu_map_result_mate_stats(res, C.byref(mst))
            if mst.mates:
                mp_, m = C.POINTER(_lib.MapMate)(), C.c_uint64()
                L.msgpu_map_result_mates(res, C.byref(mp_), C.byref(m))
                mates_at = C.addressof(mp_.contents) if m.value else None
                rows = (np.frombuffer((C.c_char * (16 * m.value)).from_address(C.addressof(mp_.contents)), dtype=_lib.MAP_MATE_DTYPE)
                        if m.value else [])
                mate_rows = [tuple(int(x) for x in r) for r in rows]
            if tables is not None:
                if ranks is not None:
                    tables["ranks"] = ranks
                if mate_rows is not None:
                    tables["mates"] = mate_rows
                cp = C.POINTER(_lib.MapChain)()
                m = C.c_uint64()
                L.msgpu_map_result_chains(res, C.byref(cp), C.byref(m))
                names = [f for f, _ in _lib.MapChain._fields_]
                tables["chains"] = [tuple(int(getattr(cp[i], f)) for f in names) for i in range(m.value)]
                tables["text"] = bytes(text)
                ops, off, m = C.POINTER(C.c_uint32)(), C.POINTER(C.c_uint64)(), C.c_uint64()
                L.msgpu_map_result_cigars(res, C.byref(ops), C.byref(off), C.byref(m))
                tables["runs"] = [[int(ops[j]) for j in range(off[i], off[i + 1])] for i in range(m.value)]
                tables["cigars"] = ["".join("%d%s" % (r >> 4, "MIDNSHP=X"[r & 15]) for r in runs) for runs in tables["runs"]]
                if xst.extend:
                    ep, m = C.POINTER(_lib.ExtEnd)(), C.c_uint64()
                    L.msgpu_map_result_ext_ends(res, C.byref(ep), C.byref(m))
                    end = [tuple(int(getattr(ep[i], f)) for f, _ in _lib.ExtEnd._fields_) for i in range(m.value)]
                    tables["ext"] = list(zip(end[0::2], end[1::2]))
            sam_text = None
            if sam is not None:  # (before the PAF is written: an error leaves neither file)
                from . import sam as sam_stage
                cp, rp = C.POINTER(_lib.MapChain)(), C.POINTER(_lib.MapRank)()
                ops, off, m = C.POINTER(C.c_uint32)(), C.POINTER(C.c_uint64)(), C.c_uint64()
                L.msgpu_map_result_ranks(res, C.byref(rp), C.byref(m))
                L.msgpu_map_result_cigars(res, C.byref(ops), C.byref(off), C.byref(m))
                L.msgpu_map_result_chains(res, C.byref(cp), C.byref(m))
                none = np.zeros(1, dtype=_lib.MAP_MATE_DTYPE)  # (mates without a chain: rows there are none of)
                sam_timings = {}
                tpath = index.targets if index is not None else targets
                sam_text, _, sam_stats = sam_stage.run_pointers(
                    tpath, queries if queries is not None else tpath,
                    C.cast(cp, C.c_void_p), m.value, C.cast(ops, C.c_void_p), C.cast(off, C.c_void_p), C.cast(rp, C.c_void_p),
                    (mates_at or none.ctypes.data) if mst.mates else None, eqx=not sam_m, md=sam_md, budget=budget,
                    device=index.device if index is not None else device, timings=sam_timings, lines=False)
                sam_stats["seconds"] = sam_timings
            t1 = time.perf_counter()
            with open(out, "wb") as h:
                h.write(text)
            if sam_text is not None:
                with open(sam, "wb") as h:
                    h.write(sam_text)
            t_write = time.perf_counter() - t1
    if timings is not None:
        timings.update({name[:-3]: getattr(st, name) / 1e3 for name, _ in _lib.MapStats._fields_ if name.endswith("_ms")})
        timings["stage_wall"] = timings.pop("wall")
        timings.update({"file": t_write, "total": time.perf_counter() - t0})
    ext = {}
    if xst.extend:
        ext["extend"] = dict({name: int(getattr(xst, name)) for name, t in _lib.MapExtStats._fields_
                              if t is not C.c_float and name != "reserved"}, seconds={"extend": xst.extend_ms / 1e3})
    if ranks is not None:
        ext["ranks"] = ranks
        ext["rank"] = _rank_stats(rst)
    if mate_rows is not None:
        ext["mates"] = mate_rows
        ext["mate"] = _mate_stats(mst)
    if sam is not None:
        ext["sam"] = sam_stats
    return {**ext, "params": {name: int(getattr(st.params, name)) for name in DEFAULTS}, "records": [int(x) for x in st.n_records],
            "bases": [int(x) for x in st.n_bases], "minimizers": [int(x) for x in st.n_minimizers], "keys": int(st.n_keys),
            "keys_dropped": int(st.n_keys_dropped), "entries_dropped": int(st.n_entries_dropped), "anchors": int(st.n_anchors),
            "n_groups": int(st.n_groups), "groups_kept": int(st.n_groups_kept), "groups_small": int(st.n_groups_small),
            "groups_large": int(st.n_groups_large), "largest_group": int(st.largest_group),
            "group_hist": [int(x) for x in st.group_hist], "chains": int(st.n_chains), "below_score": int(st.n_chains_below_score),
            "below_count": int(st.n_chains_below_count), "chains_cut": int(st.n_chains_cut), "pairs": int(st.n_pairs),
            "capped": int(st.n_pairs_capped), "lost_publications": int(st.n_lost_publications), "bytes_out": int(st.bytes_out),
            "batches": batches, "budget_bytes": budget_used, "cigar": int(st.params.cigar),
            "align": dict({name: int(getattr(ast, name)) for name, t in _lib.MapAlignStats._fields_ if t is not C.c_float},
                          seconds={name[:-3]: getattr(ast, name) / 1e3 for name, t in _lib.MapAlignStats._fields_ if t is C.c_float})}


_OPTS = {"-k": "k", "-w": "w", "--max-occ": "max_occ", "--min-score": "min_score", "--min-count": "min_count",
         "--max-gap": "max_gap", "--bandwidth": "bandwidth", "--band": "band"}


def main(argv):
    args, p, ok, budget = list(argv), {}, True, None
    for flag in ("--exact", "--ava"):
        if flag in args:
            args.remove(flag)
            p[flag[2:]] = 1
    cigar = 0
    if "--cigar" in args:  # (implies --exact)
        args.remove("--cigar")
        cigar = p["exact"] = 1
    extend = 0
    if "--extend" in args:  # (implies --cigar)
        i = args.index("--extend")
        try:
            extend = int(args[i + 1])
            ok = 1 <= extend <= _lib.MAP_EXTEND_MAX
        except (IndexError, ValueError):
            ok = False
        del args[i:i + 2]
        cigar = p["exact"] = 1
    rank = "--rank" in args
    if rank:
        args.remove("--rank")
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
    sam = {}
    if "--sam" in args:  # (implies --cigar and --rank)
        i = args.index("--sam")
        ok = ok and i + 1 < len(args) and not args[i + 1].startswith("-")
        sam["sam"] = args[i + 1] if i + 1 < len(args) else None
        del args[i:i + 2]
    for flag, key in (("--md", "sam_md"), ("--cigar-m", "sam_m")):
        if flag in args:
            args.remove(flag)
            sam[key] = True
            ok = ok and "sam" in sam
    for name, key in _OPTS.items():
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
    q = dict(DEFAULTS, **p)
    ok = ok and 4 <= q["k"] <= 32 and 1 <= q["w"] <= 64 and q["max_occ"] >= 1 and 1 <= q["band"] <= 127
    ok = ok and q["max_gap"] >= 0 and q["bandwidth"] >= 0 and not any(a.startswith("-") for a in args)
    ok = ok and len(args) == 3 and (not q["ava"] or args[0] == args[1]) and not (mates and q["ava"])
    if not ok:
        sys.stderr.write(__doc__.split("\n\n")[1] + "\n")
        return 2
    timings = {}
    more = dict(mates=True, max_insert=max_insert) if mates else {}  # (without the option the call is the one it always was)
    more.update(sam)
    out = run(args[0], args[1], args[2], timings=timings, budget_mb=budget, cigar=cigar, extend=extend, rank=rank, **p, **more)
    out.pop("ranks", None)  # (the table is the PAF's; the line keeps the counts)
    out.pop("mates", None)
    out["seconds"] = {key: round(v, 4) for key, v in timings.items()}
    print(json.dumps(out))
    return 0


if __name__ == "__main__":
    _lib.PRELOAD_TORCH = False  # this process never imports torch
    sys.exit(main(sys.argv[1:]))
