"""The pipeline's unitig coverage filter on the GPU: what the reference pipeline's ``unitig_filter.py`` step writes
(``unitigs_corrected.fa`` and the report lines), from the same four arguments.

    python -m muchsalsa_amd.unitig_filter <unitigs.paf> <unitigs.fa> <report.txt> <out.fa>

prints one JSON line of counts and seconds.  The rules (include/msgpu.h, "unitig coverage filter"):

* every PAF line counts; a block is a maximal run of consecutive lines with the same column 0, its profile is as long as
  the qlen (column 1) of its first line; covered positions are [qstart, qend);
* pass 1: a block's value is its maximum coverage by the first line of each read id (column 5) in the block; an id that
  forms several blocks takes the value of its last block; q1, q3 = numpy.percentile(values, 25 / 75) over one value per
  id, upper = q3 + 1.5 * (q3 - q1);
* pass 2, per block in PAF order: a block whose id's value is greater than upper is an outlier, and its coverage by ALL
  its lines is cut into maximal runs of cov <= q3; runs of >= 500 positions are written as ``>{id}_{k} {len} {start}
  {end}`` (end inclusive, bases clipped to the sequence); every other block writes the unitig's whole record, its header
  being the description line;
* FASTA in lines of 60; the report's six lines are appended, never truncated.

Where the reference script would stop with an exception this stage raises UnitigFilterError (with the 1-based PAF line
where there is one) and writes nothing.  Known differences from the reference script, all on input it does not expect:

* no ``.idx`` side file is written next to the unitigs;
* of two FASTA records with the same id the first one is used (the sequence store's rule);
* whitespace inside sequence lines: every ``isspace`` byte is removed (the sequence loader's rule), where Biopython
  removes spaces and carriage returns only;
* integers are plain decimal digits (a leading '-' in column 6 too); Python's int() also takes ``+5``, `` 5`` and
  ``5_000``;
* only '\\n' ends a line (Python's text mode also splits at a lone '\\r').
"""
import ctypes as C
import json
import os
import sys
import time

import numpy as np

from . import _lib
from ._stage import StageError, stage_context, text_view

__all__ = ["UnitigFilterError", "UfPaf", "quartiles", "run", "report_text", "main"]


class UnitigFilterError(StageError):
    """A rejected input or a device failure; ``line`` = 1-based PAF line (0: none)."""

    def __init__(self, code, detail="", line=0):
        super().__init__(code, 0, line, detail)

    @staticmethod
    def where(file, line):
        return " (PAF line %d)" % line


class UfPaf:
    """msgpu_uf_parse: the filter's PAF tokenised on the host."""

    def __init__(self, path):
        L = _lib.lib()
        h, line = C.c_void_p(), C.c_uint64(0)
        rc = L.msgpu_uf_parse(os.fsencode(path), C.byref(h), C.byref(line))
        if rc != _lib.OK:
            raise UnitigFilterError(rc, os.fspath(path), int(line.value))
        self.handle = h

    def tables(self):
        """Copies of the tables as numpy arrays (uint32)."""
        t = _lib.UfTables()
        _lib.lib().msgpu_uf_get_tables(self.handle, C.byref(t))

        def arr(p, n):
            return np.ctypeslib.as_array(p, shape=(n,)).copy() if n else np.zeros(0, np.uint32)

        nl, nb, nu = int(t.n_lines), int(t.n_blocks), int(t.n_unitigs)
        out = {k: arr(getattr(t, k), nl) for k in ("line_block", "line_qs", "line_qe", "line_read")}
        out.update({k: arr(getattr(t, k), nb) for k in ("block_first", "block_n", "block_qlen", "block_unitig")})
        out["unitig_last_block"] = arr(t.unitig_last_block, nu)
        out["unitigs"] = [_lib.lib().msgpu_uf_unitig_name(self.handle, i).decode() for i in range(nu)]
        out["reads"] = [_lib.lib().msgpu_uf_read_name(self.handle, i).decode() for i in range(int(t.n_reads))]
        return out

    def close(self):
        if self.handle:
            _lib.lib().msgpu_uf_free(self.handle)
            self.handle = None

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


def quartiles(values):
    """(q1, q3, upper) of msgpu_uf_quartiles: numpy.percentile's linear method, bit for bit."""
    v = np.ascontiguousarray(values, dtype=np.uint32)
    q1, q3, up = C.c_double(), C.c_double(), C.c_double()
    rc = _lib.lib().msgpu_uf_quartiles(v.ctypes.data, v.size, C.byref(q1), C.byref(q3), C.byref(up))
    if rc != _lib.OK:
        raise UnitigFilterError(rc, "quartiles of %d values" % v.size)
    return q1.value, q3.value, up.value


def report_text(upper, q3, n_blocks, n_outliers, n_rescued):
    """The six report lines (floats as Python's str of a float64)."""
    return (">>> unitig filter \n"
            "upper_outlier: %s\n"
            "Q3: %s\n"
            "#all unitigs: %d\n"
            "#outliers: %d\n"
            "#rescued outliers: %d\n" % (str(float(upper)), str(float(q3)), n_blocks, n_outliers, n_rescued))


def run(paf, unitigs, report, out, device=0, timings=None, packed=False):
    """The whole stage: writes ``out`` and appends to ``report``; returns the counts and q1 / q3 / upper.
    ``packed``: gather from the 2-bit sequence store.  ``timings`` (a dict) receives seconds per step."""
    L = _lib.lib()
    t0 = time.perf_counter()
    with UfPaf(paf) as u:
        t_parse = time.perf_counter() - t0
        with stage_context("uf", device, UnitigFilterError) as stage:
            with stage.run(u.handle, os.fsencode(unitigs), _lib.UF_PACKED if packed else 0) as res:
                st = _lib.UfStats()
                L.msgpu_uf_result_stats(res, C.byref(st))
                text = bytes(text_view(L.msgpu_uf_result_text, res))
    t1 = time.perf_counter()
    with open(out, "wb") as f:
        f.write(text)
    with open(report, "a") as f:
        f.write(report_text(st.upper, st.q3, st.n_blocks, st.n_outliers, st.n_rescued))
    t_write = time.perf_counter() - t1
    if timings is not None:
        timings.update({"parse": t_parse, "load": st.load_ms / 1e3, "upload": st.upload_ms / 1e3,
                        "pass1": st.pass1_ms / 1e3, "pass2": st.pass2_ms / 1e3, "plan": st.plan_ms / 1e3,
                        "gather": st.gather_ms / 1e3, "format": st.format_ms / 1e3, "copy": st.copy_ms / 1e3,
                        "stage_wall": st.wall_ms / 1e3, "write": t_write, "total": time.perf_counter() - t0})
    return {"lines": int(st.n_lines), "blocks": int(st.n_blocks), "ids": int(st.n_ids),
            "outliers": int(st.n_outliers), "rescued": int(st.n_rescued), "fragments": int(st.n_fragments),
            "records": int(st.n_records), "bases": int(st.bases), "text_bytes": int(st.text_bytes),
            "wave_blocks": int(st.n_wave), "group_blocks": int(st.n_group), "giant_blocks": int(st.n_giant),
            "q1": st.q1, "q3": st.q3, "upper": st.upper}


def main(argv):
    if len(argv) != 4:
        sys.stderr.write(__doc__.split("\n\n")[1] + "\n")
        return 2
    timings = {}
    out = run(argv[0], argv[1], argv[2], argv[3], timings=timings)
    out["seconds"] = {k: round(v, 4) for k, v in timings.items()}
    print(json.dumps(out))
    return 0


if __name__ == "__main__":
    _lib.PRELOAD_TORCH = False  # this process never imports torch
    sys.exit(main(sys.argv[1:]))
