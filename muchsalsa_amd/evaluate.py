"""Assembly evaluation on the GPU: consensus QV and completeness of one or more assemblies from the k-mers of the accurate
short reads, without a reference genome -- the k-mer spectrum of the reads against the k-mers of the assembly, which is
Merqury's method.

    python -m muchsalsa_amd.evaluate <k> <in_1.fq> <in_2.fq> <report.tsv> <assembly.fa> [<assembly.fa> ...]
            [--min-count N] [--spectrum F] [--bed F] [--budget-mb N]

prints one JSON line of counts and seconds.  Merqury is not needed, and it is not part of the reference tree: the stage is
defined by the rules below and checked, without tolerance, on integers, against the tests' restatement in plain Python
(tests/ev_oracle.py), not against Merqury.  The rules (include/msgpu.h, "assembly evaluation"); parameters k (1..64),
min_count (1..10000, default 2, the unitig stage's default; anything else is MSGPU_E_ARG):

1. Read k-mers.  These follow the k-mer abundance filter's rules for FASTQ, for windows (k in 1..64, case folded, any
   byte outside ACGTacgt breaks the windows that hold it) and for canonical keys, error code, file and line included.
   The two cases are one file, and two files, which may have different record counts (the unitig stage's msgpu_pair
   semantics).  R(x) is the exact number of windows of the read files whose canonical k-mer is x.
2. Assembly k-mers.  A window is k consecutive bases of one FASTA record, with the same alphabet rule.  It never crosses
   two records.  A(x) is the number of assembly windows whose canonical k-mer is x (its copy number).  A window with
   R(x) = 0 is missing.
3. Per record and in total.  The figures are length, windows, missing.  A record shorter than k has 0 windows.
4. QV.  This is host arithmetic in double precision from the two integers (msgpu_ev_qv).  With p = missing / windows,
   the error rate is e = -expm1(log1p(-p) / k).  This form avoids cancellation for small p.
   qv = -10 * log10(e) + 0.0, so that e = 1 prints 0.00, never -0.00.  missing = 0 gives +inf (text inf).
   windows = 0 gives no value (NaN, text -).
5. Spectrum.  S[c][a] is the number of distinct canonical k-mers x with copy class c = min(A(x), 4) and read
   abundance a.  a is 0 for assembly-only k-mers; there c >= 1.  Otherwise a = min(R(x), 10001); row 10001 is the
   filter's cap row.  That makes 5 x 10002 counters.  For every a >= 1 the sum over c is the filter's histogram row.
6. Completeness.  This is host arithmetic on the spectrum for the parameter min_count.  solid is the sum of S[c][a] over
   a >= min_count and all c.  found is the same sum over c >= 1.
7. Error intervals, on request.  One interval is made per maximal run of consecutive missing windows of a record.  A
   run of windows s..e gives (record, s, e + k).  Intervals are not merged, so two runs separated by one present window
   give two intervals that overlap.  They are ordered by record, then start.  A run never continues into the next record.
8. Report text.  It is tab-separated.  The first line is ``#k <k> min_count <m>``.  Per assembly: a line
   ``#assembly <file name>`` (the path's last component), then the header ``record length windows missing qv``, then one
   line per record in file order; the name is the record name up to the first blank; qv is printed with %.2f.  Then a
   line ``total ...``, and a line ``completeness <found> <solid> <100 * found / solid with %.4f, or - when solid = 0>``.
   ``--spectrum F`` writes the lines ``a c0 c1 c2 c3 c4`` for the rows that are not all zero, ``--bed F`` writes
   ``name start end``; each of the two opens an assembly's lines with its ``#assembly`` line as well.
9. Limits.  Each is an error that names the figure, never a fault.  At most 2^30 distinct read k-mers (the hash table
   over them has 2^31 slots at most).  Fewer than 2^31 assembly windows: the bases of an assembly stay below 2^31 (a
   3 Gb genome is out of scope).  The file limits of the filter and of the sequence store.  Everything resident together
   within the budget, else MSGPU_E_NOMEM naming the sizes.

The table of the reads (``Table``) is made once, from files or from an entered ``kmer_filter.Pair``, and serves any number
of assemblies; ``run(..., table=t)`` reads it.
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

__all__ = ["EvaluateError", "Table", "qv", "run", "main"]


class EvaluateError(StageError):
    """A rejected input or a device failure; ``line`` = 1-based line (0: none) of ``file`` (0 / 1: the first / second
    FASTQ)."""


def qv(missing, windows, k):
    """msgpu_ev_qv (host, no device): rule 4; +inf for missing = 0, NaN for windows = 0"""
    out = C.c_double()
    rc = _lib.lib().msgpu_ev_qv(int(missing), int(windows), int(k), C.byref(out))
    if rc != _lib.OK:
        raise EvaluateError(rc, detail="missing = %d, windows = %d, k = %d" % (missing, windows, k))
    return out.value


def _budget(budget_mb):
    return 0 if budget_mb is None else max(1, int(float(budget_mb) * (1 << 20)))


class Table:
    """The reads' k-mers at one k resident in device memory (msgpu_ev_table): the distinct canonical keys, their counts and
    the hash table over them.  Made from one or two FASTQ files (``in2`` may be None), or from an entered
    ``kmer_filter.Pair`` (``pair``; ``in1`` / ``in2`` / ``device`` are then not read).  A context manager; ``stats`` holds
    the counts and seconds of the build."""

    def __init__(self, k, in1=None, in2=None, pair=None, device=0, budget_mb=None):
        self.k, self.paths, self.pair, self.budget = int(k), (in1, in2), pair, _budget(budget_mb)
        self.device = device if pair is None else pair.device
        self.handle, self.stage, self.stats, self._stack = C.c_void_p(), None, None, None

    def __enter__(self):
        L = _lib.lib()
        with contextlib.ExitStack() as stack:
            stage = stack.enter_context(stage_context("ev", self.device, EvaluateError))
            if self.pair is None:
                in1, in2 = self.paths
                stage.check(L.msgpu_ev_table_open(stage.ctx, self.k, os.fsencode(in1), None if in2 is None else os.fsencode(in2),
                                                  self.budget, C.byref(self.handle)))
            else:
                stage.check(L.msgpu_ev_table_open_pair(stage.ctx, self.k, self.pair.handle, self.budget, C.byref(self.handle)))
            stack.callback(self.close)
            st = _lib.EvTableStats()
            L.msgpu_ev_table_stats(self.handle, C.byref(st))
            self.stats = {"k": int(st.k), "records": [int(x) for x in st.n_records], "bytes_in": [int(x) for x in st.bytes_in],
                          "windows": int(st.n_windows), "distinct": int(st.n_distinct), "partitions": int(st.n_partitions),
                          "largest_partition": int(st.largest_partition), "bytes_resident": int(st.bytes_resident),
                          "seconds": {name[:-3]: getattr(st, name) / 1e3 for name, _ in _lib.EvTableStats._fields_
                                      if name.endswith("_ms")}}
            self.stage = stage
            self._stack = stack.pop_all()
        return self

    def close(self):
        if self.handle:
            _lib.lib().msgpu_ev_table_free(self.handle)
            self.handle = C.c_void_p()

    def __exit__(self, *exc):
        self._stack.close()
        return False


def _one(L, res, path, tables, timings, texts):
    """what a result holds of one assembly -> its dict; the texts are appended to ``texts``"""
    st = _lib.EvStats()
    L.msgpu_ev_result_stats(res, C.byref(st))
    report = bytes(text_view(L.msgpu_ev_result_text, res, _lib.EV_TEXT_REPORT))
    texts["head"] = bytes(text_view(L.msgpu_ev_result_text, res, _lib.EV_TEXT_HEAD))
    texts["report"].append(report)
    texts["spectrum"].append(bytes(text_view(L.msgpu_ev_result_text, res, _lib.EV_TEXT_SPECTRUM)))
    texts["bed"].append(bytes(text_view(L.msgpu_ev_result_text, res, _lib.EV_TEXT_BED)))
    rp, tp, n = C.POINTER(_lib.EvRecord)(), C.POINTER(_lib.EvRecord)(), C.c_uint64()
    L.msgpu_ev_result_records(res, C.byref(rp), C.byref(tp), C.byref(n))
    total = (int(tp[0].length), int(tp[0].windows), int(tp[0].missing))
    lines = report.split(b"\n")
    if tables is not None:
        names = [l.split(b"\t")[0].decode(errors="replace") for l in lines[2:2 + n.value]]
        sp, ip, ni = C.POINTER(C.c_uint64)(), C.POINTER(_lib.EvInterval)(), C.c_uint64()
        L.msgpu_ev_result_spectrum(res, C.byref(sp))
        L.msgpu_ev_result_intervals(res, C.byref(ip), C.byref(ni))
        tables.setdefault("assemblies", []).append({
            "records": [(names[i], int(rp[i].length), int(rp[i].windows), int(rp[i].missing)) for i in range(n.value)],
            "total": total,
            "spectrum": np.ctypeslib.as_array(sp, shape=(_lib.EV_CLASSES, _lib.EV_ROWS)).copy(),
            "intervals": [(int(ip[i].record), int(ip[i].start), int(ip[i].end)) for i in range(ni.value)],
            "report": report})
    if timings is not None:
        timings.setdefault("assemblies", []).append({name[:-3]: getattr(st, name) / 1e3 for name, _ in _lib.EvStats._fields_
                                                     if name.endswith("_ms")})
    return {"assembly": os.path.basename(os.fspath(path)), "records": int(st.n_records), "length": total[0], "windows": total[1],
            "missing": total[2], "qv": lines[2 + n.value].split(b"\t")[4].decode(), "missing_distinct": int(st.n_missing_distinct),
            "solid": int(st.solid), "found": int(st.found), "completeness": lines[3 + n.value].split(b"\t")[3].decode(),
            "intervals": int(st.n_intervals), "lost_publications": int(st.n_lost_publications), "bytes_peak": int(st.bytes_peak)}


def run(k, in1, in2, assemblies, report, min_count=2, spectrum=None, bed=None, budget_mb=None, device=0, table=None, tables=None,
        timings=None):
    """The whole stage: writes ``report`` (and ``spectrum`` / ``bed`` when given) for the ``assemblies`` (one path or a list
    of paths), in their order; returns the counts.  ``in2`` may be None.  With ``table`` (an entered Table) the stage reads
    the resident table and ``in1`` / ``in2`` / ``device`` / ``budget_mb`` are not read; ``k`` must be the table's.
    ``budget_mb`` bounds the count's partition buffers (None: half of the free device memory).  ``tables`` (a dict) receives
    ``assemblies``: per assembly ``records`` [(name, length, windows, missing)], ``total``, ``spectrum`` (5 x 10002), ``intervals``
    [(record, start, end)] (rule 7 runs when ``bed`` or ``tables`` is given) and ``report`` (its block of the text);
    ``timings`` (a dict) seconds per step."""
    L = _lib.lib()
    t0 = time.perf_counter()
    if isinstance(assemblies, (str, bytes, os.PathLike)):
        assemblies = [assemblies]
    assemblies = list(assemblies)
    if not assemblies:
        raise EvaluateError(_lib.E_ARG, detail="no assembly")
    if not 1 <= int(min_count) <= 10000:
        raise EvaluateError(_lib.E_ARG, detail="min_count = %d is outside 1..10000" % int(min_count))
    prm = _lib.EvParams(int(k), int(min_count), 1 if (bed is not None or tables is not None) else 0, 0)
    texts = {"head": b"", "report": [], "spectrum": [], "bed": []}
    out = []
    if table is None and len(assemblies) == 1:  # msgpu_ev_run: open, run, free
        with stage_context("ev", device, EvaluateError) as stage:
            with stage.run(C.byref(prm), os.fsencode(in1), None if in2 is None else os.fsencode(in2), os.fsencode(assemblies[0]), 0,
                           _budget(budget_mb)) as res:
                out.append(_one(L, res, assemblies[0], tables, timings, texts))
        reads = None
    else:
        with (Table(k, in1, in2, device=device, budget_mb=budget_mb) if table is None else contextlib.nullcontext(table)) as t:
            for path in assemblies:
                with t.stage.run(C.byref(prm), t.handle, os.fsencode(path), 0, fn="run_table") as res:
                    out.append(_one(L, res, path, tables, timings, texts))
            reads = t.stats
    t1 = time.perf_counter()
    for path, text in ((report, texts["head"] + b"".join(texts["report"])), (spectrum, b"".join(texts["spectrum"])),
                       (bed, b"".join(texts["bed"]))):
        if path is not None:
            with open(path, "wb") as h:
                h.write(text)
    if timings is not None:
        if reads is not None:
            timings["table"] = dict(reads["seconds"])
        timings.update({"files": time.perf_counter() - t1, "total": time.perf_counter() - t0})
    result = {"k": int(k), "min_count": int(min_count), "assemblies": out}
    if reads is not None:
        result["reads"] = {key: v for key, v in reads.items() if key != "seconds"}
    return result


def main(argv):
    args = list(argv)
    opts = {"--min-count": 2, "--spectrum": None, "--bed": None, "--budget-mb": None}
    ok = True
    for name in opts:
        if name in args:
            i = args.index(name)
            try:
                opts[name] = (float if name == "--budget-mb" else int if name == "--min-count" else str)(args[i + 1])
                ok = ok and not (isinstance(opts[name], str) and (not opts[name] or opts[name].startswith("--")))
            except (IndexError, ValueError):
                ok = False
            del args[i:i + 2]
    k = 0
    try:
        k = int(args[0]) if args else 0
    except ValueError:
        ok = False
    ok = ok and 1 <= opts["--min-count"] <= 10000 and (opts["--budget-mb"] is None or opts["--budget-mb"] > 0)
    ok = ok and not any(a.startswith("--") for a in args)
    if not ok or len(args) < 5:
        sys.stderr.write(__doc__.split("\n\n")[1] + "\n")
        return 2
    timings = {}
    out = run(k, args[1], args[2], args[4:], args[3], min_count=opts["--min-count"], spectrum=opts["--spectrum"], bed=opts["--bed"],
              budget_mb=opts["--budget-mb"], timings=timings)

    def rounded(v):
        return {key: rounded(x) for key, x in v.items()} if isinstance(v, dict) else [rounded(x) for x in v] if isinstance(v, list) \
            else round(v, 5)
    out["seconds"] = rounded(timings)
    print(json.dumps(out))
    return 0


if __name__ == "__main__":
    _lib.PRELOAD_TORCH = False  # this process never imports torch
    sys.exit(main(sys.argv[1:]))
