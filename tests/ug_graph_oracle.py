"""Rule 10 of the short-read unitig assembly (the unitig graph as GFA 1) restated in plain Python, from the rule in
include/msgpu.h ("short-read unitig assembly") -- not from the kernels.  It stands on what ug_oracle.run (or
ug_bubble_oracle.run) leaves: ``chains`` (per unitig in output order, its oriented nodes), ``counts`` (the cleaned solid
set), ``unitigs`` (the table) and ``all`` (the FASTA text).

    (a) oriented unitigs   oriented
    (b) adjacencies        adjacencies (asserts that every target is the first node of an oriented unitig)
    (c) mirror             mirror, links
    (d) order              links
    (e) text               gfa
    statistics             graph
"""
import ug_oracle


def oriented(r):
    """(a) -> {(id, rev): [oriented nodes]}; a unitig that is one self-complementary k-mer exists as (id, 0) only"""
    k, out = r["k"], {}
    for i, chain in enumerate(r["chains"]):
        out[(i, 0)] = list(chain)
        if not (len(chain) == 1 and chain[0] == ug_oracle.rc(chain[0], k)):
            out[(i, 1)] = [ug_oracle.rc(x, k) for x in reversed(chain)]
    return out


def adjacencies(r):
    """(b) -> ([((from id, from rev), (to id, to rev))] over every oriented unitig and every successor of its last node,
    the oriented unitig ends without a successor)"""
    g = ug_oracle.Graph(r["counts"], r["k"])
    units = oriented(r)
    first = {}
    for x, chain in units.items():
        assert chain[0] not in first, "two oriented unitigs start at one node"
        first[chain[0]] = x
    out, dead = [], 0
    for x in sorted(units):
        succ = g.succ(units[x][-1])
        dead += not succ
        for t in succ:
            assert t in first, "an adjacency ends inside a unitig: unitig %r, target %x" % (x, t)
            out.append((x, first[t]))
    return out, dead


def mirror(units, link):
    """(c): x -> y and y' -> x' are one link, ' flips the orientation; a link at a unitig that exists as + only (one
    self-complementary k-mer) has no mirror and stands for itself"""
    (x, y) = link
    if (x[0], 1) not in units or (y[0], 1) not in units:
        return link
    return ((y[0], 1 - y[1]), (x[0], 1 - x[1]))


def links(r):
    """(c), (d) -> (the links [(from, from_rev, to, to_rev)] ascending, the adjacencies, the self-mirrored links, the dead
    ends)"""
    units = oriented(r)
    adj, dead = adjacencies(r)
    assert len(set(adj)) == len(adj)
    have = set(adj)
    kept, self_mirror = [], 0
    for a in adj:
        m = mirror(units, a)
        assert m in have, "an adjacency without its mirror"
        if a <= m:
            kept.append((a[0][0], a[0][1], a[1][0], a[1][1]))
            self_mirror += a == m
    kept.sort()
    return kept, len(adj), self_mirror, dead


def gfa(r, table):
    """(e) -> the text"""
    seqs = r["all"].split(b"\n")[1::2]
    out = [b"H\tVN:Z:1.0\n"]
    for i, (t, seq) in enumerate(zip(r["unitigs"], seqs)):
        assert len(seq) == t[0]
        out.append(b"S\t%d\t%s\tLN:i:%d\tKC:i:%d\n" % (i, seq, t[0], t[1]))
    for f, fr, t, tr in table:
        out.append(b"L\t%d\t%s\t%d\t%s\t%dM\n" % (f, b"+-"[fr:fr + 1], t, b"+-"[tr:tr + 1], r["k"] - 1))
    return b"".join(out)


def graph(r):
    """rule 10 on a result of ug_oracle.run -> {"links": the table, "adjacencies", "self_mirror", "dead_ends", "gfa": the
    text}"""
    table, n_adj, self_mirror, dead = links(r)
    assert n_adj == 2 * len(table) - self_mirror
    return {"links": table, "adjacencies": n_adj, "self_mirror": self_mirror, "dead_ends": dead, "gfa": gfa(r, table)}
