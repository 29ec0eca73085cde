"""The pipeline's Illumina k-mer abundance filter on the GPU: what the reference pipeline's first step ("K-mer Filtering of
Illumina Reads": jellyfish count -C / histo, ``setAbundanceThresholdFromHisto.py``, jellyfish dump -L, bbduk hdist=0) writes
-- the two filtered FASTQ files and the threshold line of ``report.txt`` -- from the two Illumina files alone.

    python -m muchsalsa_amd.kmer_filter <k> <in_1.fq> <in_2.fq> <report.txt> <out_1.fq> <out_2.fq>
            [--histo PATH] [--kmers PATH] [--budget-mb N]

prints one JSON line of counts and seconds.  Neither jellyfish nor bbduk is needed.  The threshold rule is pinned to the
reference script itself (run unchanged, its outputs recorded as data under tests/golden/kmer_filter); counting and
filtering are defined by the rules below and checked against the tests' restatement in plain Python.  The rules
(include/msgpu.h, "k-mer abundance filter"):

* FASTQ: four lines per record, only '\\n' ends a line, a last line without '\\n' counts.  Line 1 starts with '@', line 3
  with '+', lines 2 and 4 have the same number of bytes (0 is allowed).  Anything else is an error that names the file
  (0 / 1) and the 1-based line (the smallest offending one; file 0 is judged first); so is a file that ends inside a record
  (at its first missing line), and so are two files with different record counts (the shorter file, at its first missing
  line).  On any error nothing is written.
* k-mers: a window is k (1..64) consecutive bytes of a line 2, all of them in ``ACGTacgt`` (case folded); any other byte
  breaks the windows that hold it.  A=0, C=1, G=2, T=3, first base most significant, as a 2k-bit unsigned number; the
  canonical k-mer of a window is the smaller of that number and the number of its reverse complement (jellyfish's ``-C``:
  with this code numeric order is the lexicographic order of the text).  A read shorter than k has no window.
* counts: count(x) = number of windows of both files whose canonical k-mer is x.  Exact.
* histogram: row (a, f): f distinct canonical k-mers have count a, for 1 <= a <= 10000; one row a = 10001 holds every
  k-mer with a count above 10000 (jellyfish histo's default ``--high``); rows with f = 0 are left out; text ``"a f\\n"``.
* threshold = what the script prints for that histogram and total = sum of f over the rows with a != 1:
  q1_th = round((total + 1) * 0.25), q3_th = round((total + 1) * 0.75) with Python's round (half to even); rows with a > 1
  in order, a running sum of f; q1 = a of the first row where the sum reaches q1_th; q3 = a of the first *later* row where
  it reaches q3_th (the script's ``elif``: the row that sets q1 never sets q3); upper = q3 + 2 * (q3 - q1).  If q3 is never
  set the script prints a number <= 0, and with no row besides a = 1 it dies: both are a stage error ("degenerate
  histogram"), nothing written.  Whenever q3 is set, q3 > q1 >= 2, hence upper >= 5: the count pass puts every k-mer into
  the histogram and keeps only those with a count of 5 or more for the threshold to choose from.
* abundant set = the canonical k-mers with count >= upper (``jellyfish dump -L``).
* verdict: pair i is dropped when read 1 or read 2 has at least one window whose canonical k-mer is in the abundant set
  (exact match, one hit suffices, either mate condemns the pair).  Surviving pairs are written in input order; a record is
  its four input lines byte for byte, each ended by '\\n'.
* report: ``report.txt`` is created or truncated and holds ``abundance threshold for k-mer filtering:  <upper>\\n`` (two
  blanks, as the pipeline's ``echo`` joins its two arguments).

Limits: a file below 2^32 records and 2^40 bytes; both files, the partition buffers and the outputs are resident in device
memory together, otherwise the stage fails naming the sizes; files larger than that are out of scope.

Known differences.  From bbduk's documented defaults, none of which could be checked against the program:

* ``maskmiddle=t`` lets the middle base of a k-mer mismatch; this stage matches all k bases;
* k > 31 is emulated there by runs of 31-mers; here a window of up to 64 bases is one key;
* the '+' line may be rewritten there; here it is copied;
* its output order is not the input order unless ``ordered=t``; here it is.

From jellyfish:

* the pipeline's ``--bf-size`` run drops most singletons through a Bloom filter, i.e. approximates the same table above
  abundance 1 (all the threshold rule reads); this stage counts exactly (the "classic approach" the pipeline keeps as a
  comment), so row 1 of its histogram is the true one;
* ``dump`` writes in hash order, ``--kmers`` in ascending key order;
* the pipeline's progress lines are replaced by the JSON line.
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

__all__ = ["KmerFilterError", "Pair", "threshold", "run", "main"]


class KmerFilterError(StageError):
    """A rejected input or a device failure; ``line`` = 1-based line (0: none) of ``file`` (0 / 1: the first / second
    FASTQ)."""


def threshold(rows):
    """msgpu_kf_threshold (host, no device): histogram rows [(abundance, frequency), ...] -> (q1, q3, upper).
    KmerFilterError (MSGPU_E_LAYOUT) for a degenerate histogram, where the script dies or prints a number <= 0."""
    rows = list(rows)
    a = np.ascontiguousarray([r[0] for r in rows], dtype=np.uint64)
    f = np.ascontiguousarray([r[1] for r in rows], dtype=np.uint64)
    q1, q3, up = C.c_int64(), C.c_int64(), C.c_int64()
    rc = _lib.lib().msgpu_kf_threshold(a.ctypes.data if len(rows) else None, f.ctypes.data if len(rows) else None,
                                       len(rows), C.byref(q1), C.byref(q3), C.byref(up))
    if rc != _lib.OK:
        raise KmerFilterError(rc, detail="degenerate histogram" if rc == _lib.E_LAYOUT else "")
    return int(q1.value), int(q3.value), int(up.value)


class Pair:
    """The two Illumina files resident in device memory (msgpu_pair): their bytes, their line starts, the FASTQ rules
    checked.  ``run(..., pair=p)`` here and ``unitigs.run(..., pair=p)`` then read them where they lie, any number of
    times, at any k; neither changes them.  A context manager; the files are judged when it is entered (two files of
    different record counts are accepted here: the filter rejects them, the unitig stage takes them without a mask)."""

    def __init__(self, in1, in2, device=0):
        self.paths, self.device, self.handle = (in1, in2), device, C.c_void_p()
        self._stack = None

    def __enter__(self):
        with contextlib.ExitStack() as stack:
            stage = stack.enter_context(stage_context("kf", self.device, KmerFilterError))
            stage.check(_lib.lib().msgpu_kf_open_pair(stage.ctx, os.fsencode(self.paths[0]), os.fsencode(self.paths[1]),
                                                      C.byref(self.handle)))
            stack.callback(self.close)
            self.stage = stage
            self._stack = stack.pop_all()
        return self

    def close(self):
        if self.handle:
            _lib.lib().msgpu_pair_close(self.handle)
            self.handle = C.c_void_p()

    def __exit__(self, *exc):
        self._stack.close()
        return False


def _arr(p, n, dtype):
    return np.ctypeslib.as_array(p, shape=(n,)).copy() if n else np.zeros(0, dtype)


def run(k, in1, in2, report, out1, out2, device=0, budget_mb=None, histo=None, kmers=None, timings=None, tables=None,
        pair=None):
    """The whole stage: writes ``out1``, ``out2`` and ``report`` (and ``histo`` / ``kmers`` when given); returns the
    counts.  With ``pair`` (an entered Pair) the stage runs on the resident files, ``in1`` / ``in2`` / ``device`` are not
    read, and ``out1`` / ``out2`` may be None: that text is then not written.  ``budget_mb`` bounds the partition buffers (None: half of the free device memory).  ``timings`` (a dict)
    receives seconds per step; ``tables`` (a dict) receives ``histogram`` (rows), ``key_hi`` / ``key_lo`` / ``count`` (the
    abundant set, ascending) and ``verdict`` (a byte per pair, 1 = dropped)."""
    L = _lib.lib()
    t0 = time.perf_counter()
    budget = 0 if budget_mb is None else max(1, int(float(budget_mb) * (1 << 20)))
    with (stage_context("kf", device, KmerFilterError) if pair is None else contextlib.nullcontext(pair.stage)) as stage:
        with (stage.run(int(k), os.fsencode(in1), os.fsencode(in2), 0, budget) if pair is None else
              stage.run(int(k), pair.handle, 0, budget, fn="run_pair")) as res:
            st = _lib.KfStats()
            L.msgpu_kf_result_stats(res, C.byref(st))
            if tables is not None:
                a, f, n = C.POINTER(C.c_uint64)(), C.POINTER(C.c_uint64)(), C.c_uint64()
                L.msgpu_kf_result_histogram(res, C.byref(a), C.byref(f), C.byref(n))
                tables["histogram"] = list(zip(_arr(a, n.value, np.uint64).tolist(), _arr(f, n.value, np.uint64).tolist()))
                hi, lo, cnt = C.POINTER(C.c_uint64)(), C.POINTER(C.c_uint64)(), C.POINTER(C.c_uint32)()
                L.msgpu_kf_result_abundant(res, C.byref(hi), C.byref(lo), C.byref(cnt), C.byref(n))
                tables["key_hi"], tables["key_lo"] = _arr(hi, n.value, np.uint64), _arr(lo, n.value, np.uint64)
                tables["count"] = _arr(cnt, n.value, np.uint32)
                v = C.POINTER(C.c_uint8)()
                L.msgpu_kf_result_verdicts(res, C.byref(v), C.byref(n))
                tables["verdict"] = _arr(v, n.value, np.uint8)
            t1 = time.perf_counter()
            files = [(out1, _lib.KF_TEXT_OUT_A), (out2, _lib.KF_TEXT_OUT_B), (report, _lib.KF_TEXT_REPORT)]
            if histo is not None:
                files.append((histo, _lib.KF_TEXT_HISTO))
            if kmers is not None:
                files.append((kmers, _lib.KF_TEXT_KMERS))
            for path, which in files:
                if path is None:
                    continue
                with open(path, "wb") as h:
                    h.write(text_view(L.msgpu_kf_result_text, res, which))
            t_write = time.perf_counter() - t1
    if timings is not None:
        timings.update({"load": st.load_ms / 1e3, "records": st.records_ms / 1e3, "bins": st.bins_ms / 1e3,
                        "extract": st.extract_ms / 1e3, "sort": st.sort_ms / 1e3, "runs": st.runs_ms / 1e3,
                        "hist": st.hist_ms / 1e3, "select": st.select_ms / 1e3, "verdict": st.verdict_ms / 1e3,
                        "output": st.output_ms / 1e3, "copy": st.copy_ms / 1e3, "stage_wall": st.wall_ms / 1e3,
                        "write": t_write, "total": time.perf_counter() - t0})
    return {"k": int(st.k), "pairs_in": int(st.n_pairs), "pairs_out": int(st.n_pairs_out), "windows": int(st.n_windows),
            "distinct": int(st.n_distinct), "candidates": int(st.n_candidates), "q1": int(st.q1), "q3": int(st.q3),
            "upper": int(st.upper), "abundant": int(st.n_abundant), "partitions": int(st.n_partitions),
            "largest_partition": int(st.largest_partition), "bytes_in": [int(x) for x in st.bytes_in],
            "bytes_out": [int(x) for x in st.bytes_out]}


def main(argv):
    args = list(argv)
    opts = {"--histo": None, "--kmers": None, "--budget-mb": None}
    ok = True
    for name in opts:
        if name in args:
            i = args.index(name)
            if i + 1 < len(args):
                opts[name] = args[i + 1]
            else:
                ok = False
            del args[i:i + 2]
    try:
        k = int(args[0]) if args else 0
        budget = None if opts["--budget-mb"] is None else float(opts["--budget-mb"])
        ok = ok and (budget is None or budget > 0)
    except ValueError:
        ok = False
    if not ok or len(args) != 6:
        sys.stderr.write(__doc__.split("\n\n")[1] + "\n")
        return 2
    timings = {}
    out = run(k, args[1], args[2], args[3], args[4], args[5], budget_mb=budget, histo=opts["--histo"],
              kmers=opts["--kmers"], timings=timings)
    out["seconds"] = {key: round(v, 4) for key, v in timings.items()}
    print(json.dumps(out))
    return 0


if __name__ == "__main__":
    _lib.PRELOAD_TORCH = False  # this process never imports torch
    sys.exit(main(sys.argv[1:]))
