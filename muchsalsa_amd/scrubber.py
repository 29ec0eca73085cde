"""The pipeline's read scrubber on the GPU: what the reference pipeline's ``scrubber_bfs.py`` step writes (the scrubbed
long reads, ``02_<reads>.scrubbed.fa``), from the anchor PAF, the reads and a read-to-read PAF.

    python -m muchsalsa_amd.scrubber <anchors.paf> <reads.fa|fq> <out.fa> <ava.paf> [--subset-size N]

prints one JSON line of counts and seconds.  The script maps every batch of reads against itself with ``minimap2 -x
ava-ont``; this stage maps nothing: ``ava.paf`` is all reads against all reads, mapped once, and a batch uses its lines
whose two reads are both in the batch, in file order.  ``python -m muchsalsa_amd.mapper <reads> <reads> <ava.paf> --ava``
writes such a file (and, without ``--ava``, the anchor PAF from the unitigs and the reads).  The rules (include/msgpu.h,
"read scrubber"):

* anchor PAF in line order: a line of one token is skipped, so is one with col3 - col2 < 500; a read (column 5) is a node
  from its first surviving line on, its length column 6 of that line; the first surviving line of a (read, anchor) counts
  and gives the anchor range (col7, col8); a chunk is a maximal run of counting lines with one column 0; a counting line
  joins its read to every read already in the chunk; a node's neighbours are ordered by when their edge was added;
* batches: breadth-first from the smallest remaining name outside the subset, nodes in discovery order until the subset
  holds ``subset_size`` (60000) nodes; a component that leaves it smaller merges into the next start; the centre is every
  subset node without a remaining neighbour outside the subset;
* read-to-read lines of a batch: skipped are col0 == col5, a name outside the subset, col3 - col2 < 500; the line folds
  (col2, col3, strand) into the entry of (col0, col5) and (col7, col8, strand) into that of (col5, col0): the first
  line creates (S, E, D), a later (s, e, d) with d == D and (|S - e| < 500 or |s - E| < 500) widens it to (min, max);
  entries persist from batch to batch;
* per centre node the entries' (S, E) and the anchor ranges are sorted and merged left to right (a range joins the last
  covered one when cs <= e and s <= ce); covered range i is ``>{read}_{i}`` with the bases [max(cs, 200), min(ce, length -
  200)], end inclusive, in lines of 60; an empty slice gives the header line alone.  The centre leaves the graph.

Where the script would stop with an exception this stage raises ScrubberError (with the 1-based line and the file where
there is one) and writes nothing.  Known differences from the script:

* record order: the script walks a Python ``set`` of strings, so its order changes with the hash seed; this stage writes
  the batches in order and inside a batch the centre nodes by node number (first-seen order of the anchor PAF);
* a batch with an empty centre: the script removes nothing and builds the same batch again, for ever (a small subset size
  on a dense graph does this); this stage raises ScrubberError naming the batch's start read and writes nothing;
* a read that the reads file lacks is an error with the anchor PAF line of the read's first surviving hit, and nothing is
  written (the script stops at that read, after the batches before it);
* column 6 below 200 makes the slice's end index negative, which Python counts from the end of the sequence: here it is
  an error at that line;
* a read-to-read line is judged names first (a line whose two reads are not both nodes is in no batch, whatever else it
  holds), then by its field count and integers, then by its span;
* no ``.idx`` side file is written next to the reads; of two records with the same name the first one is used; every
  ``isspace`` byte inside sequence lines is removed; integers are plain decimal digits (a leading '-' in column 6 only);
  only '\\n' ends a line -- the unitig filter's rules;
* the script's progress lines on standard output are replaced by the JSON line.
"""
import ctypes as C
import json
import os
import sys
import time

import numpy as np

from . import _lib
from ._stage import StageError, stage_context, text_view

__all__ = ["ScrubberError", "ScrubPaf", "batches", "run", "main", "SUBSET_SIZE"]

SUBSET_SIZE = _lib.SCRUB_SUBSET


class ScrubberError(StageError):
    """A rejected input or a device failure; ``line`` = 1-based line (0: none) of ``file`` (0 anchor PAF, 1 read-to-read
    PAF)."""

    def __init__(self, code, detail="", line=0, file=0):
        super().__init__(code, file, line, detail)

    @staticmethod
    def where(file, line):
        return " (%s line %d)" % (("anchor PAF", "read-to-read PAF")[file], line)


def _arr(p, n, dtype):
    return np.ctypeslib.as_array(p, shape=(n,)).copy() if n else np.zeros(0, dtype)


class ScrubPaf:
    """msgpu_scrub_parse: the anchor PAF and the read-to-read PAF tokenised on the host."""

    def __init__(self, anchors, ava):
        L = _lib.lib()
        h, line, which = C.c_void_p(), C.c_uint64(0), C.c_int(0)
        rc = L.msgpu_scrub_parse(os.fsencode(anchors), os.fsencode(ava), C.byref(h), C.byref(line), C.byref(which))
        if rc != _lib.OK:
            raise ScrubberError(rc, os.fspath(ava if which.value else anchors), int(line.value), int(which.value))
        self.handle = h

    def tables(self):
        """Copies of the tables as numpy arrays, plus the node names."""
        t = _lib.ScrubTables()
        _lib.lib().msgpu_scrub_get_tables(self.handle, C.byref(t))
        nn, nh, nc, na = int(t.n_nodes), int(t.n_hits), int(t.n_chunks), int(t.n_ava)
        out = {"node_length": _arr(t.node_length, nn, np.int32), "node_line": _arr(t.node_line, nn, np.uint32)}
        out.update({k: _arr(getattr(t, k), nh, np.uint32) for k in ("hit_node", "hit_anchor", "hit_line")})
        out.update({k: _arr(getattr(t, k), nh, np.int32) for k in ("hit_s", "hit_e")})
        out.update({k: _arr(getattr(t, k), nc, np.uint32) for k in ("chunk_first", "chunk_n")})
        out.update({k: _arr(getattr(t, k), na, np.uint32) for k in ("ava_a", "ava_b", "ava_strand", "ava_line")})
        out.update({k: _arr(getattr(t, k), na, np.int32) for k in ("ava_sa", "ava_ea", "ava_sb", "ava_eb")})
        out["nodes"] = [_lib.lib().msgpu_scrub_node_name(self.handle, i).decode() for i in range(nn)]
        out["n_anchor_lines"], out["n_ava_lines"] = int(t.n_anchor_lines), int(t.n_ava_lines)
        return out

    def name_order(self):
        """The node ids sorted by name (the order the script's min() takes its starts in)."""
        t = _lib.ScrubTables()
        _lib.lib().msgpu_scrub_get_tables(self.handle, C.byref(t))
        out = np.zeros(int(t.n_nodes), np.uint32)
        _lib.lib().msgpu_scrub_name_order(self.handle, out.ctypes.data)
        return out

    def close(self):
        if self.handle:
            _lib.lib().msgpu_scrub_free(self.handle)
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


def batches(by_name, row_off, adj, subset_size=SUBSET_SIZE):
    """msgpu_scrub_plan_create (host): the batches of a graph in CSR form (rows in insertion order) -> a list of
    (first start, subset in the order its nodes were added, centre by ascending id).  ScrubberError (``node`` = the
    batch's first start) when a batch has an empty centre."""
    L = _lib.lib()
    by_name = np.ascontiguousarray(by_name, dtype=np.uint32)
    row_off = np.ascontiguousarray(row_off, dtype=np.uint64)
    adj = np.ascontiguousarray(adj, dtype=np.uint32)
    p, bad = C.c_void_p(), C.c_uint32()
    rc = L.msgpu_scrub_plan_create(len(by_name), by_name.ctypes.data, row_off.ctypes.data,
                                   adj.ctypes.data if adj.size else None, int(subset_size), C.byref(p), C.byref(bad))
    if rc != _lib.OK:
        err = ScrubberError(rc, "start node %d" % bad.value if rc == _lib.E_LAYOUT else "")
        err.node = int(bad.value)
        raise err
    try:
        t = _lib.ScrubPlanTables()
        L.msgpu_scrub_plan_get(p, C.byref(t))
        nb = int(t.n_batches)
        so, co = _arr(t.subset_off, nb + 1, np.uint64), _arr(t.centre_off, nb + 1, np.uint64)
        sub, cen, start = _arr(t.subset, int(so[nb]), np.uint32), _arr(t.centre, int(co[nb]), np.uint32), _arr(t.start, nb,
                                                                                                             np.uint32)
        return [(int(start[b]), sub[int(so[b]):int(so[b + 1])].tolist(), cen[int(co[b]):int(co[b + 1])].tolist())
                for b in range(nb)]
    finally:
        L.msgpu_scrub_plan_free(p)


def run(anchors, reads, out, ava, subset_size=SUBSET_SIZE, device=0, timings=None, graph=None):
    """The whole stage: writes ``out``; returns the counts.  ``timings`` (a dict) receives seconds per step; ``graph`` (a
    dict) receives the read graph the device built (``row_off``, ``adj``)."""
    L = _lib.lib()
    t0 = time.perf_counter()
    with ScrubPaf(anchors, ava) as s:
        t_parse = time.perf_counter() - t0
        with stage_context("scrub", device, ScrubberError) as stage:
            with stage.run(s.handle, os.fsencode(reads), int(subset_size)) as res:
                st = _lib.ScrubStats()
                L.msgpu_scrub_result_stats(res, C.byref(st))
                text = bytes(text_view(L.msgpu_scrub_result_text, res))
                if graph is not None:
                    ro, ad = C.POINTER(C.c_uint64)(), C.POINTER(C.c_uint32)()
                    L.msgpu_scrub_result_graph(res, C.byref(ro), C.byref(ad))
                    graph["row_off"] = _arr(ro, int(st.n_nodes) + 1, np.uint64)
                    graph["adj"] = _arr(ad, 2 * int(st.n_edges), np.uint32)
    t1 = time.perf_counter()
    with open(out, "wb") as f:
        f.write(text)
    t_write = time.perf_counter() - t1
    if timings is not None:
        timings.update({"parse": t_parse, "load": st.load_ms / 1e3, "graph": st.graph_ms / 1e3,
                        "batching": st.batch_ms / 1e3, "fold": st.fold_ms / 1e3, "union": st.union_ms / 1e3,
                        "plan": st.plan_ms / 1e3, "gather": st.gather_ms / 1e3, "format": st.format_ms / 1e3,
                        "copy": st.copy_ms / 1e3, "stage_wall": st.wall_ms / 1e3, "write": t_write,
                        "total": time.perf_counter() - t0})
    return {"nodes": int(st.n_nodes), "hits": int(st.n_hits), "pairs": int(st.n_pairs), "edges": int(st.n_edges),
            "ava_lines": int(st.n_ava), "batches": int(st.n_batches), "subset_total": int(st.n_subset_total),
            "interval_slots": int(st.n_intervals), "records": int(st.n_records), "bases": int(st.bases),
            "text_bytes": int(st.text_bytes)}


def main(argv):
    subset = SUBSET_SIZE
    args = list(argv)
    if "--subset-size" in args:
        k = args.index("--subset-size")
        try:
            subset = int(args[k + 1])
        except (IndexError, ValueError):
            subset = 0
        del args[k:k + 2]
    if len(args) != 4 or subset <= 0:
        sys.stderr.write(__doc__.split("\n\n")[1] + "\n")
        return 2
    timings = {}
    out = run(args[0], args[1], args[2], args[3], subset_size=subset, timings=timings)
    out["seconds"] = {k: round(v, 4) for k, v in timings.items()}
    print(json.dumps(out))
    return 0


if __name__ == "__main__":
    _lib.PRELOAD_TORCH = False  # this process never imports torch
    sys.exit(main(sys.argv[1:]))
