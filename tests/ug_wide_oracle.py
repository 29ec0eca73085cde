"""The restatement of the short-read unitig assembly at any k.  tests/ug_oracle.py, ug_bubble_oracle.py and ug_graph_oracle.py
state the rules on Python integers and are free of a key width but for two places: ``ug_oracle.rc`` reads 16 bytes, and
``kf_oracle.count`` (behind ``ug_oracle.count_files``) forms its windows in two 64-bit halves.  This module gives both for any
k -- ``rc`` by the rule itself (the bases reversed and complemented), ``count_files`` by ``kf_oracle.canonical_kmers``, the
window rule in plain integers -- and binds them in ONE place, ``bound()``, which sets the two names in the restatement's
modules and puts them back.  ``run`` is ug_bubble_oracle.run without its bound on k, under that binding; rule 10 is
ug_graph_oracle.graph on its result."""
import contextlib

import kf_oracle
import ug_bubble_oracle
import ug_graph_oracle
import ug_oracle


def rc_by_rule(x, k):
    """reverse complement of a k-mer (an integer, first base most significant) by the rule itself, base by base"""
    out = 0
    for _ in range(k):
        out = (out << 2) | (3 - (x & 3))
        x >>= 2
    return out


_RC_BYTE = bytes(rc_by_rule(b, 4) for b in range(256))


def rc(x, k):
    """the same for any k, four bases per byte by a table, the byte order by reading the bytes the other way round (the
    workloads call it millions of times)"""
    n = (2 * k + 7) // 8
    return int.from_bytes(x.to_bytes(n, "little").translate(_RC_BYTE), "big") >> (8 * n - 2 * k)


def count_files(records, k):
    """-> (dict canonical k-mer -> count over all files, windows), for any k"""
    counts, windows = {}, 0
    for rs in records:
        for r in rs:
            for x in kf_oracle.canonical_kmers(r[1], k):
                counts[x] = counts.get(x, 0) + 1
                windows += 1
    return counts, windows


@contextlib.contextmanager
def bound():
    """the one place where the restatement's modules get the wide ``rc`` and ``count_files``"""
    saved = (ug_oracle.rc, ug_oracle.count_files, ug_bubble_oracle.rc)
    ug_oracle.rc, ug_oracle.count_files, ug_bubble_oracle.rc = rc, count_files, rc
    try:
        yield
    finally:
        ug_oracle.rc, ug_oracle.count_files, ug_bubble_oracle.rc = saved


def run(k, datas, bubble=0, min_count=2, trim=None, min_length=500, found=None, graph=False):
    """ug_bubble_oracle.run (rules 1-9) for 2 <= k <= 128 -> its dict; ``graph`` adds ``graph``, ug_graph_oracle.graph's dict
    (rule 10)"""
    if not 2 <= k <= 128 or min_count < 1 or not 0 <= bubble <= ug_bubble_oracle.BUBBLE_MAX:
        raise ValueError("k / min_count / bubble")
    trim = k if trim is None else trim
    # (the composition below is ug_bubble_oracle.run's, copied because that function refuses k > 64 before it does anything;
    # tests/test_unitigs_wide_host.py compares this function with the narrow restatement below k = 65, so a change to the original that is not made here fails there)
    with bound():
        records = ug_oracle.parse_files(datas)
        counts, windows = ug_oracle.count_files(records, k)
        solid = {x: c for x, c in counts.items() if c >= min_count}
        S, rounds, brounds, phases = ug_bubble_oracle.clean(solid, k, trim, bubble, found)
        units, blocked = ug_oracle.unitigs(S, k)
        table, all_text, cut_text = ug_oracle.texts(units, S, k, min_length)
        chains = [u[1] for u in sorted(units, key=lambda u: u[0])]
        other = sum(1 for rs in records for r in rs for b in r[1] if b not in b"ACGTacgt")
        r = {"k": k, "records": [len(x) for x in records], "windows": windows, "distinct": len(counts), "solid": len(solid),
             "solid_after": len(S), "rounds": rounds, "unitigs": table, "kept": sum(1 for t in table if t[0] >= min_length),
             "cycles": sum(t[4] for t in table), "longest": max([len(c) for c in chains], default=0), "all": all_text,
             "cut": cut_text, "chains": chains, "blocked": blocked, "counts": S,
             "alone": sum(1 for c in chains if len(c) == 1 and c[0] == rc(c[0], k)), "other_bytes": other,
             "bubble": bubble, "bubble_rounds": brounds, "bubble_phases": phases, "bubbles": sum(b[2] for b in brounds),
             "bubble_branches": sum(b[3] for b in brounds), "bubble_kmers": sum(b[4] for b in brounds)}
        if graph:
            r["graph"] = ug_graph_oracle.graph(r)
    return r
