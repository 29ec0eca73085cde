#!/usr/bin/env python3
"""Pin the k-mer abundance filter's threshold rule to the reference pipeline's own script, as data.

    python tools/make_kmer_filter_fixtures.py <reference checkout>

Reads <reference checkout>/pipeline/setAbundanceThresholdFromHisto.py at run time and runs it unchanged, as a child
process, on generated histogram files; ``total`` comes from the pipeline's own awk line, which is cut out of
<reference checkout>/pipeline/pipeline.sh at run time and run by awk on the same file.  Nothing of either text is kept.
Written under tests/golden/kmer_filter/:

  threshold.json      per case: name, rows [[abundance, frequency], ...], total (what awk printed), printed (the integer the
                      script printed, or null), failed (the script ended with an error)
  tiny_<x>.1.fq, tiny_<x>.2.fq, tiny_<x>.json
                      a FASTQ pair small enough to be read by eye and what the plain-Python restatement
                      (tests/kf_oracle.py) makes of it: k, histogram, q1 / q3 / upper, the abundant k-mers as text with their
                      counts, the verdict per pair and per mate

A generator: it needs the reference checkout and awk, and no test runs it."""
import json
import os
import random
import re
import subprocess
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import kf_oracle  # noqa: E402

GOLD = os.path.join(ROOT, "tests", "golden", "kmer_filter")

NAMED = [
    ("issue_1", [(1, 1000), (2, 50), (3, 30), (4, 10), (5, 6), (9, 4)]),
    ("issue_2_elif", [(1, 1000), (2, 500), (3, 1)]),
    ("issue_3", [(2, 1), (3, 1)]),
    ("issue_4_q3_never", [(1, 10), (7, 3)]),
    ("issue_5_only_row_1", [(1, 10)]),
    # total + 1 = 502: 125.5 rounds to 126 and 376.5 to 376; the sums 125 | 126 and 376 | 377 fall on different rows
    ("round_ties", [(1, 7), (2, 125), (3, 1), (4, 250), (5, 1), (6, 124)]),
    ("round_ties_no_row_1", [(2, 125), (3, 1), (4, 250), (5, 1), (6, 124)]),
    ("elif_first_row_past_q3", [(1, 3), (2, 900), (5, 50), (8, 50)]),
    ("elif_single_row", [(1, 3), (4, 100)]),
    ("row_10001_is_q3", [(1, 50), (2, 10), (3, 10), (10001, 40)]),
    ("row_10001_is_q1_and_last", [(1, 50), (10001, 40)]),
    ("row_10001_behind_q3", [(1, 5), (2, 40), (3, 40), (4, 40), (10001, 1)]),
    ("q3_never_two_rows", [(2, 1), (9, 0)]),
    ("total_one", [(1, 4), (6, 1)]),
    ("no_row_1_three_rows", [(2, 10), (3, 10), (4, 10)]),
    ("wide_gap", [(1, 100000), (2, 3000), (40, 3000), (41, 1), (5000, 2)]),
]


def random_cases(n, seed):
    rnd = random.Random(seed)
    out = []
    for i in range(n):
        n_rows = rnd.randint(1, 40)
        pool = list(range(1 if rnd.random() < 0.8 else 2, 200)) + [rnd.randint(200, 10000) for _ in range(5)] + [10001]
        abund = sorted(set(rnd.sample(pool, min(n_rows, len(pool)))))
        shape = rnd.choice(("flat", "falling", "peak"))
        rows = []
        for a in abund:
            if shape == "flat":
                f = rnd.randint(1, 50)
            elif shape == "falling":
                f = max(1, int(100000 / (a ** rnd.uniform(1.0, 2.5))) + rnd.randint(0, 3))
            else:
                f = max(1, int(5000 / (1 + (a - 30) ** 2)) + rnd.randint(0, 5))
            rows.append((a, f))
        out.append(("random_%02d_%s" % (i, shape), rows))
    return out


def run_reference(reference, rows):
    script = os.path.join(reference, "pipeline", "setAbundanceThresholdFromHisto.py")
    shell = open(os.path.join(reference, "pipeline", "pipeline.sh")).read()
    line = [l for l in shell.splitlines() if "TOTAL_NON_UNIQUE_KMERS=" in l and "awk" in l]
    awk_program = re.search(r"awk\s+'([^']+)'", line[0]).group(1)
    with tempfile.TemporaryDirectory() as d:
        histo = os.path.join(d, "k.histo")
        with open(histo, "wb") as f:
            f.write(kf_oracle.histogram_text(rows))
        total = subprocess.run(["awk", awk_program, histo], check=True, capture_output=True, text=True).stdout.strip()
        # the pipeline passes $TOTAL unquoted: an empty sum leaves the script without its second argument
        p = subprocess.run([sys.executable, script, histo] + ([total] if total else []), capture_output=True, text=True)
    printed = None
    if p.returncode == 0:
        printed = int(p.stdout.strip())
    return total, printed, p.returncode != 0


TINY = {
    # k = 3.  ACG / CGT are one canonical k-mer, so are AAA / TTT; the poly-A pair makes AAA abundant and condemns pair 2 by
    # its second mate alone
    "a": (3, [("AAAAAAAAAAAA", "TTTTTTTTTT"), ("ACGTACGTAC", "GGCCGGCC"), ("CCGGATCC", "ggatAAAc"), ("ACGTN", ""),
              ("TGCATGCA", "GCATGCAT"), ("CATG", "AC")]),
    # k = 4, a palindrome (ACGT) counts once per window; N breaks windows; lower case folds, so pair 2 falls with pair 0
    "b": (4, [("ACGTACGTACGTACGTACGTACGTACGTACGT", "ACGTNACGTNACGTACGTACGTACGT"), ("GGGGCCCC", "GATTACA"),
              ("ggatccaa", "TTGacgtG"), ("GATCGATC", "CAGTCAGT"), ("GGATCCAATT", "AATTGGATCC")]),
}


def tiny_case(k, pairs):
    fq = [b"".join(b"@t%d/%d\n%s\n+\n%s\n" % (i, m + 1, p[m].encode(), b"I" * len(p[m])) for i, p in enumerate(pairs))
          for m in (0, 1)]
    r = kf_oracle.run(k, fq[0], fq[1])
    meta = {"k": k, "windows": r["windows"], "distinct": r["distinct"], "histogram": r["histogram"], "q1": r["q1"],
            "q3": r["q3"], "upper": r["upper"], "abundant": [[kf_oracle.kmer_text(x, k), c] for x, c in r["abundant"]],
            "verdict": r["verdict"], "verdict1": r["verdict1"], "verdict2": r["verdict2"]}
    return fq, meta


def main(argv):
    if len(argv) != 1:
        sys.stderr.write(__doc__.split("\n\n")[1] + "\n")
        return 2
    os.makedirs(GOLD, exist_ok=True)
    cases = []
    for name, rows in NAMED + random_cases(50, 20260101):
        total, printed, failed = run_reference(argv[0], rows)
        cases.append({"name": name, "rows": [list(r) for r in rows], "total": total, "printed": printed, "failed": failed})
    with open(os.path.join(GOLD, "threshold.json"), "w") as f:
        f.write("{\"cases\": [\n" + ",\n".join(json.dumps(c) for c in cases) + "\n]}\n")
    for name, (k, pairs) in TINY.items():
        fq, meta = tiny_case(k, pairs)
        for m in (0, 1):
            with open(os.path.join(GOLD, "tiny_%s.%d.fq" % (name, m + 1)), "wb") as f:
                f.write(fq[m])
        with open(os.path.join(GOLD, "tiny_%s.json" % name), "w") as f:
            json.dump(meta, f, indent=1)
            f.write("\n")
    print("%d threshold cases (%d where the script failed, %d where it printed a number <= 0), %d tiny pairs" % (
        len(cases), sum(c["failed"] for c in cases), sum(c["printed"] is not None and c["printed"] <= 0 for c in cases),
        len(TINY)))
    return 0


if __name__ == "__main__":
    sys.exit(main(sys.argv[1:]))
