"""Plain-Python restatement of the read scrubber's rules (include/msgpu.h, "read scrubber"): dicts and lists only.  It is the
checker of muchsalsa_amd.scrubber, not the product, and it produces the stage's canonical record order (batches in order,
inside a batch the centre nodes by node number).

scrub(anchor_paf, ava_paf, reads, subset_size) -> (batches, stats); text(batches) -> the output file's bytes;
OracleError(line, file) where the stage must fail (file 0: anchor PAF, 1: read-to-read PAF), EmptyCentre where a batch has
an empty centre."""

SUBSET_SIZE = 60000
NEAR = 500   # shortest hit; also how near two lines of a pair must be to join
TRIM = 200   # bases dropped at both ends of a read


class OracleError(Exception):
    def __init__(self, what, line=0, file=0):
        super().__init__("%s (file %d line %d)" % (what, file, line))
        self.line = line
        self.file = file


class EmptyCentre(Exception):
    def __init__(self, start):
        super().__init__("the batch that starts at node %d has an empty centre" % start)
        self.start = start


def _int(tok, line, file, signed=False):
    body = tok[1:] if signed and tok[:1] == "-" else tok
    if not body or any(c not in "0123456789" for c in body):
        raise OracleError("not an integer: %r" % tok, line, file)
    v = int(tok)
    if abs(v) > 2**31 - 1:
        raise OracleError("out of range: %r" % tok, line, file)
    return v


def _lines(data):
    """(1-based number, tokens) of every line; only '\\n' ends a line; str.rstrip() then split('\\t')"""
    rows = data.split(b"\n")
    if rows and rows[-1] == b"":
        rows.pop()
    for i, raw in enumerate(rows):
        yield i + 1, raw.decode("utf-8", "surrogateescape").rstrip(" \t\n\r\x0b\x0c").split("\t")


def read_graph(anchor_paf):
    """Rule 1 -> dict(names, node (name -> id), length, line (1-based, of the node's first surviving line), anchors (per
    node: anchor -> (s, e), first hit only), adj (per node: neighbours in the order their edges were added), hits, chunks)"""
    node, names, length, first_line, anchors, adj, have = {}, [], [], [], [], [], []
    prev, chunk, n_hits, n_chunks = None, [], 0, 0
    for ln, t in _lines(anchor_paf):
        if len(t) == 1:
            continue
        if len(t) < 9:
            raise OracleError("fewer than 9 fields", ln, 0)
        if t[0] == "":
            raise OracleError("empty column 0", ln, 0)
        s1, e1, s2, e2 = (_int(t[k], ln, 0) for k in (2, 3, 7, 8))
        len2 = _int(t[6], ln, 0, signed=True)
        if e1 - s1 < NEAR:
            continue
        a, r = t[0], t[5]
        if r not in node:
            if len2 < TRIM:
                raise OracleError("read length %d: the slice would end at a negative index" % len2, ln, 0)
            node[r] = len(names)
            names.append(r)
            length.append(len2)
            first_line.append(ln)
            anchors.append({})
            adj.append([])
            have.append(set())
        v = node[r]
        if a in anchors[v]:
            continue
        anchors[v][a] = (s2, e2)
        n_hits += 1
        if a != prev:
            chunk, prev = [], a
            n_chunks += 1
        for u in chunk:
            if v not in have[u]:
                have[u].add(v)
                have[v].add(u)
                adj[u].append(v)
                adj[v].append(u)
        chunk.append(v)
    if not names:
        raise OracleError("no node", 1, 0)
    return dict(names=names, node=node, length=length, line=first_line, anchors=anchors, adj=adj, hits=n_hits,
                chunks=n_chunks)


def ava_lines(ava_paf, node):
    """Rule 3's tests that do not depend on the batch -> [(id of column 0, id of column 5, s1, e1, strand, s2, e2)]"""
    out = []
    for ln, t in _lines(ava_paf):
        if len(t) < 6:          # one token, or no second name: in no batch
            continue
        if t[0] == t[5]:
            continue
        i1, i2 = node.get(t[0]), node.get(t[5])
        if i1 is None or i2 is None:
            continue
        if len(t) < 9:
            raise OracleError("fewer than 9 fields", ln, 1)
        s1, e1, s2, e2 = (_int(t[k], ln, 1) for k in (2, 3, 7, 8))
        if e1 - s1 < NEAR:
            continue
        out.append((i1, i2, s1, e1, t[4], s2, e2))
    return out


def batches(names, adj, subset_size=SUBSET_SIZE):
    """Rule 2 -> [(first start, subset in the order its nodes were added, centre by ascending id)].  The search is
    networkx's bfs_edges(G, start, depth_limit=subset_size) over the remaining graph."""
    n = len(names)
    alive = [True] * n
    n_alive = n
    by_name = sorted(range(n), key=lambda i: names[i].encode("utf-8", "surrogateescape"))
    out = []
    subset, members, first = [], set(), None
    while n_alive:
        start = next(i for i in by_name if alive[i] and i not in members)
        if first is None:
            first = start
        order, seen = [start], {start}
        level, depth = [start], 0
        while level and depth < subset_size:
            nxt = []
            for u in level:
                for w in adj[u]:
                    if alive[w] and w not in seen:
                        seen.add(w)
                        order.append(w)
                        nxt.append(w)
            level, depth = nxt, depth + 1
        for v in order:
            if len(subset) >= subset_size:
                break
            if v not in members:
                members.add(v)
                subset.append(v)
        if len(subset) < subset_size and n_alive > len(subset):
            continue
        centre = sorted(v for v in subset if all((not alive[w]) or w in members for w in adj[v]))
        if not centre:
            raise EmptyCentre(first)
        out.append((first, subset, centre))
        for v in centre:
            alive[v] = False
        n_alive -= len(centre)
        subset, members, first = [], set(), None
    return out


def _fold(d, key, s, e, direction):
    if key not in d:
        d[key] = (s, e, direction)
    else:
        S, E, D = d[key]
        if direction == D and (abs(S - e) < NEAR or abs(s - E) < NEAR):
            d[key] = (min(s, S), max(e, E), direction)


def covered(ranges):
    """Rule 4's merge of (s, e) pairs"""
    cov = []
    for s, e in sorted(ranges):
        if cov and cov[-1][0] <= e and s <= cov[-1][1]:
            cov[-1] = (min(s, cov[-1][0]), max(e, cov[-1][1]))
        else:
            cov.append((s, e))
    return cov


def scrub(anchor_paf, ava_paf, reads, subset_size=SUBSET_SIZE):
    """anchor_paf / ava_paf: bytes; reads: dict name (str) -> bases (bytes).  -> (batches, stats): a batch is a list of
    (header bytes without '\\n', bases) in node order."""
    g = read_graph(anchor_paf)
    names, length, adj = g["names"], g["length"], g["adj"]
    ava = ava_lines(ava_paf, g["node"])
    for v, name in enumerate(names):
        if name not in reads:
            raise OracleError("read %s is not in the reads file" % name, g["line"][v], 0)
    plan = batches(names, adj, subset_size)
    entries = [{} for _ in names]
    out = []
    for _, subset, centre in plan:
        members = set(subset)
        for (i1, i2, s1, e1, strand, s2, e2) in ava:
            if i1 in members and i2 in members:
                _fold(entries[i1], i2, s1, e1, strand)
                _fold(entries[i2], i1, s2, e2, strand)
        recs = []
        for v in centre:
            iv = [(s, e) for (s, e, _) in entries[v].values()] + list(g["anchors"][v].values())
            seq = reads[names[v]]
            for i, (cs, ce) in enumerate(covered(iv)):
                lo, hi = max(cs, TRIM), min(ce, length[v] - TRIM)
                recs.append((b">%s_%d" % (names[v].encode("utf-8", "surrogateescape"), i), seq[lo:hi + 1]))
        out.append(recs)
    return out, dict(nodes=len(names), edges=sum(len(x) for x in adj) // 2, hits=g["hits"], chunks=g["chunks"],
                     ava_lines=len(ava), batches=len(plan), records=sum(len(b) for b in out),
                     plan=plan, graph=g)


def _wrap(b):
    return b"".join(b[i:i + 60] + b"\n" for i in range(0, len(b), 60))


def text(batches_):
    return b"".join(h + b"\n" + _wrap(s) for b in batches_ for h, s in b)


def records(data):
    """output text -> {header: body}; headers are unique"""
    out = {}
    for rec in data.split(b">")[1:]:
        h, _, body = rec.partition(b"\n")
        assert h not in out, h
        out[h] = body
    return out


def parse_fasta(data):
    """reads of a FASTA (first record of a name wins, whitespace inside sequence lines removed)"""
    out = {}
    for rec in data.split(b">")[1:]:
        h, _, body = rec.partition(b"\n")
        name = h.split()[0].decode() if h.split() else ""
        out.setdefault(name, b"".join(body.split()))
    return out
