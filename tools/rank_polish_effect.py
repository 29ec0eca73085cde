"""What the mapper's rule 12 does to polishing, on the CPU, by the tests' restatements alone (no GPU, no library):

    python tools/rank_polish_effect.py [repeat_len=4000] [differences=4]

``planted`` of tests/plcases.py (a 20,000-base genome, a draft with an error about every 150 bases, 40 error-free reads of 3,000
bases) with one planted two-copy repeat: genome[12000 : 12000 + repeat_len] becomes a copy of genome[2000 : 2000 + repeat_len]
with ``differences`` substitutions spread over it, so a read that lies inside one copy fits the other almost or exactly as well.
Prints one JSON line: the Levenshtein distance to the genome of the draft, of one polishing round in the plain form of the
polisher's rule 2, and of one round in ranked form at min_mapq = 1, with the voters of both rounds and the reads that rule 12
gives mapping quality 0.  A figure to report, not a test."""
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]


def distance(a, b):
    """Levenshtein distance by furthest-reaching diagonals, O((len + d) * d)"""
    n, m = len(a), len(b)

    def slide(x, k):
        while x < n and x + k < m:
            L = min(512, n - x, m - x - k)
            if a[x:x + L] == b[x + k:x + k + L]:
                x += L
                continue
            return next(x + j for j in range(L) if a[x + j] != b[x + k + j])
        return x

    front = {0: slide(0, 0)}
    d = 0
    while front.get(m - n, -1) < n:
        d += 1
        new = {}
        for k in range(-d, d + 1):
            best = -1
            if k in front and front[k] < n and front[k] + k < m:
                best = max(best, front[k] + 1)
            if k + 1 in front and front[k + 1] < n:
                best = max(best, front[k + 1] + 1)
            if k - 1 in front and front[k - 1] + k <= m:
                best = max(best, front[k - 1])
            if best >= 0 and 0 <= best + k <= m:
                new[k] = slide(best, k)
        front = new
    return d


def main(argv):
    import map_cigar_oracle
    import map_oracle
    import map_rank_oracle
    import pl_oracle
    import pl_rank_oracle
    import plcases
    from muchsalsa_amd import synth
    repeat_len = int(argv[0]) if argv else 4000
    differences = int(argv[1]) if len(argv) > 1 else 4
    plain_genome = synth.genome_bases

    def with_repeat(n, seed):
        g = plain_genome(n, seed).copy()
        g[12000:12000 + repeat_len] = g[2000:2000 + repeat_len]
        for j in range(differences):
            at = 12000 + (2 * j + 1) * repeat_len // (2 * differences)
            g[at] = b"ACGT"[(b"ACGT".index(bytes([int(g[at])])) + 1) % 4]
        return g

    synth.genome_bases = with_repeat
    try:
        plcases.workload.cache_clear()
        wl = plcases.workload("planted")
    finally:
        synth.genome_bases = plain_genome
        plcases.workload.cache_clear()
    draft, reads = map_oracle.parse(wl["draft"], False), map_oracle.parse(wl["reads"], False)
    mapped = map_cigar_oracle.cigar_run(draft, reads)
    rows = map_rank_oracle.rank(mapped["chains"])
    plain = pl_oracle.run(draft, reads, mapped["chains"], mapped["packed"])
    ranked = pl_rank_oracle.run(draft, reads, mapped["chains"], mapped["packed"], rows, min_mapq=1)
    bases = lambda text: b"".join(text.split(b"\n")[1:])
    print(json.dumps({"repeat_len": repeat_len, "differences": differences, "chains": len(mapped["chains"]), "reads": len(reads),
                      "primaries": sum(1 for i, r in enumerate(rows) if r[0] == i),
                      "primaries_mapq0": sum(1 for i, r in enumerate(rows) if r[0] == i and r[3] == 0),
                      "voters_plain": plain["n_voters"], "voters_min_mapq_1": ranked["n_voters"],
                      "distance_draft": distance(draft[0][1], wl["genome"]), "distance_plain": distance(bases(plain["text"]), wl["genome"]),
                      "distance_min_mapq_1": distance(bases(ranked["text"]), wl["genome"])}))
    return 0


if __name__ == "__main__":
    sys.exit(main(sys.argv[1:]))
