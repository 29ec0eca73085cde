#!/usr/bin/env python3
"""Pin the read scrubber to the reference pipeline's own script, as data.

    python tools/make_scrubber_fixtures.py <reference checkout> [--only small|big|edges]

Reads <reference checkout>/pipeline/scrubber_bfs.py at run time and executes it unchanged but for its subset size
(needs networkx), with two stand-ins: ``Bio.SeqIO.index_db`` returns the reads of the synthetic workload, and ``os.system``
(the script's minimap2 call) writes the lines of the workload's read-to-read PAF whose two reads are both in the batch's
temp_sequences.fa, in file order.  Inputs come from muchsalsa_amd.synth.scrubber_workload by (shape, seed); nothing of the
script's text is kept.  Written under tests/golden/scrubber/:

  <name>.anchors.paf, <name>.ava.paf, <name>.reads.fa   the inputs of a small case
  <name>.out.sorted.fa                                  the script's records, sorted by header line
  <name>.json                                           shape, seed, subset size, record count, SHA-256 of the sorted records
  big.json                                              the same figures for an input of more than 60000 nodes (the only
                                                        way to meet the script's own batching); its inputs are regenerated
                                                        from (shape, seed) by the test
  edges.json                                            per scrubber case of tests/scrubedgecases.py the subset size, the
                                                        script's record count and the SHA-256 of its sorted records; a case
                                                        the script cannot process is listed under "unprocessed" with the reason

The script never ends on a batch with an empty centre, so every case is first run through the plain-Python restatement
(tests/scrub_oracle.py), which raises on one: a shape that does is skipped and the next candidate is tried."""
import hashlib
import io
import json
import os
import re
import sys
import tempfile
import types

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import scrub_oracle  # noqa: E402
from muchsalsa_amd import synth  # noqa: E402

GOLD = os.path.join(ROOT, "tests", "golden", "scrubber")

# (name, scrubber_workload arguments, subset size)
SMALL = [
    ("a", dict(n_reads=12, read_len=1800, n_anchors=16, seed=11, hole_every=3, n_again=3, n_strangers=4), 60000),
    ("b", dict(n_reads=28, read_len=1800, n_anchors=40, seed=12, coverage=5, hole_every=4, n_again=5, n_strangers=4), 10),
]
# candidates for the big case, tried in order
BIG = [
    dict(n_reads=66000, read_len=1600, n_anchors=40000, seed=21, n_again=500, n_strangers=200),
    dict(n_reads=70000, read_len=1800, n_anchors=50000, seed=22, n_again=500, n_strangers=200),
]


class _Seq:
    def __init__(self, b):
        self.b = b

    def __getitem__(self, k):
        return _Seq(self.b[k])

    def __len__(self):
        return len(self.b)

    def __str__(self):
        return self.b.decode()


class _Rec:
    def __init__(self, b):
        self.seq = _Seq(b)


def run_script(script, anchors, ava, reads, subset_size):
    """The reference script on (anchor PAF bytes, read-to-read PAF bytes, {name: bases}) -> its output file's bytes."""
    src = open(script).read()
    src, n = re.subn(r"(?m)^(\w*subset_size\w*\s*=\s*)\d+", lambda m: m.group(1) + str(subset_size), src, count=1)
    assert n == 1, "no subset size assignment found in the script"
    ava_lines = ava.decode().split("\n")
    with tempfile.TemporaryDirectory() as tmp:
        with open(os.path.join(tmp, "a.paf"), "wb") as f:
            f.write(anchors)
        open(os.path.join(tmp, "reads.fa"), "wb").close()

        def fake_system(cmd):
            with open(os.path.join(tmp, "temp_sequences.fa")) as f:
                ids = set(ln[1:].strip() for ln in f if ln.startswith(">"))
            with open(os.path.join(tmp, "temp_pwa.paf"), "w") as f:
                for ln in ava_lines:
                    t = ln.split("\t")
                    if len(t) > 5 and t[0] in ids and t[5] in ids:
                        f.write(ln + "\n")
            return 0

        bio, seqio = types.ModuleType("Bio"), types.ModuleType("Bio.SeqIO")
        seqio.index_db = lambda idx, f, fmt: {k: _Rec(v) for k, v in reads.items()}
        bio.SeqIO = seqio
        saved = (os.system, sys.argv, sys.stdout, sys.modules.get("Bio"), sys.modules.get("Bio.SeqIO"))
        sys.modules["Bio"], sys.modules["Bio.SeqIO"] = bio, seqio
        os.system = fake_system
        sys.argv = [script, os.path.join(tmp, "a.paf"), os.path.join(tmp, "reads.fa"), os.path.join(tmp, "out.fa"), tmp]
        sys.stdout = io.StringIO()
        try:
            g = {"__name__": "__main__"}
            exec(compile(src, script, "exec"), g)
            g["output"].close()
        finally:
            os.system, sys.argv, sys.stdout = saved[:3]
            for k, v in (("Bio", saved[3]), ("Bio.SeqIO", saved[4])):
                if v is None:
                    sys.modules.pop(k, None)
                else:
                    sys.modules[k] = v
        with open(os.path.join(tmp, "out.fa"), "rb") as f:
            return f.read()


def sorted_records(text):
    """the records of an output file sorted by header line, as one text"""
    recs = scrub_oracle.records(text)
    return b"".join(b">" + h + b"\n" + recs[h] for h in sorted(recs)), len(recs)


def case(script, shape, subset_size):
    """-> (inputs, sorted script output, meta) or None when the restatement finds a batch with an empty centre"""
    anchors, ava, fa = synth.scrubber_workload(**shape)
    reads = scrub_oracle.parse_fasta(fa)
    try:
        mine, st = scrub_oracle.scrub(anchors, ava, reads, subset_size)
    except scrub_oracle.EmptyCentre as e:
        print("  skipped:", e)
        return None
    ref = run_script(script, anchors, ava, reads, subset_size)
    ref_sorted, n = sorted_records(ref)
    mine_sorted, n_mine = sorted_records(scrub_oracle.text(mine))
    assert n == n_mine and ref_sorted == mine_sorted, "the restatement and the script disagree on %r" % (shape,)
    meta = dict(shape=shape, subset_size=subset_size, nodes=st["nodes"], edges=st["edges"], batches=st["batches"],
                records=n, sha256_sorted=hashlib.sha256(ref_sorted).hexdigest())
    return (anchors, ava, fa), ref_sorted, meta


def edges(script):
    """The script on every case of tests/scrubedgecases.py -> the content of edges.json."""
    import scrubedgecases
    out = {"cases": {}, "unprocessed": {}}
    for name, c in scrubedgecases.cases().items():
        reads = scrub_oracle.parse_fasta(c.reads)
        try:
            scrub_oracle.scrub(c.anchors, c.ava, reads, c.subset_size)
        except scrub_oracle.EmptyCentre as e:
            out["unprocessed"][name] = "empty centre: %s" % e
            continue
        except scrub_oracle.OracleError as e:
            out["unprocessed"][name] = "an accepted difference (the stage raises): %s" % e
            continue
        ref_sorted, n = sorted_records(run_script(script, c.anchors, c.ava, reads, c.subset_size))
        out["cases"][name] = dict(subset_size=c.subset_size, records=n, sha256_sorted=hashlib.sha256(ref_sorted).hexdigest())
        print("  ", name, out["cases"][name])
    return out


def main(argv):
    only = None
    if "--only" in argv:
        only = argv[argv.index("--only") + 1]
        argv = [a for a in argv if a not in ("--only", only)]
    if len(argv) != 1:
        sys.stderr.write(__doc__.split("\n\n")[1] + "\n")
        return 2
    script = os.path.join(argv[0], "pipeline", "scrubber_bfs.py")
    os.makedirs(GOLD, exist_ok=True)
    if only in (None, "small"):
        for name, shape, subset in SMALL:
            print("case", name, shape, subset)
            got = case(script, shape, subset)
            assert got is not None, "small case %s has a batch with an empty centre" % name
            (anchors, ava, fa), ref_sorted, meta = got
            for suffix, data in ((".anchors.paf", anchors), (".ava.paf", ava), (".reads.fa", fa), (".out.sorted.fa", ref_sorted)):
                with open(os.path.join(GOLD, name + suffix), "wb") as f:
                    f.write(data)
            with open(os.path.join(GOLD, name + ".json"), "w") as f:
                json.dump(meta, f, indent=1, sort_keys=True)
                f.write("\n")
            print("  ", meta)
    if only in (None, "edges"):
        print("edge cases")
        with open(os.path.join(GOLD, "edges.json"), "w") as f:
            json.dump(edges(script), f, indent=1, sort_keys=True)
            f.write("\n")
    if only in (None, "big"):
        for shape in BIG:
            print("big case", shape)
            got = case(script, shape, scrub_oracle.SUBSET_SIZE)
            if got is None:
                continue
            meta = got[2]
            assert meta["nodes"] > scrub_oracle.SUBSET_SIZE and meta["batches"] >= 2, meta
            with open(os.path.join(GOLD, "big.json"), "w") as f:
                json.dump(meta, f, indent=1, sort_keys=True)
                f.write("\n")
            print("  ", meta)
            break
        else:
            raise SystemExit("no big candidate ends: every one has a batch with an empty centre")
    return 0


if __name__ == "__main__":
    sys.exit(main(sys.argv[1:]))
