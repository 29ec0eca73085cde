"""The workload of the whole-pipeline tests (muchsalsa_amd.hybrid), shared by tools/make_hybrid_fixtures.py, the host file and
the GPU file: the shape, the command's arguments and the recorded expectation (tests/golden/hybrid/expected.json: per output
file its byte count and SHA-256, and the counts the conditions below are stated on)."""
import functools
import json
import os

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EXPECTED = os.path.join(ROOT, "tests", "golden", "hybrid", "expected.json")

SHAPE = dict(genome=30000, seed=3, coverage=40, read_len=100, n_long=64, long_len=3000)
K_FILTER, K_ASSEMBLY, NAME = 21, 31, "hy"
READS_NAME = "nanopore.fastq"  # BASE = "nanopore"


@functools.lru_cache(maxsize=None)
def workload():
    from muchsalsa_amd import synth
    return synth.hybrid_workload(**SHAPE)


def write_inputs(directory):
    """-> the paths of the two Illumina files and of the long reads"""
    wl = workload()
    paths = [os.path.join(str(directory), n) for n in ("illumina_1.fq", "illumina_2.fq", READS_NAME)]
    for path, key in zip(paths, ("illumina_1", "illumina_2", "reads")):
        with open(path, "wb") as h:
            h.write(wl[key])
    return paths


def expected():
    with open(EXPECTED) as h:
        return json.load(h)


def conditions_missed(e):
    """the conditions the workload was chosen for, on the recorded counts alone -> list of those missed"""
    c, missed = e["counts"], []
    if not 0 < c["pairs_dropped"] < c["pairs"]:
        missed.append("the filter drops %d of %d pairs" % (c["pairs_dropped"], c["pairs"]))
    if c["unitigs_500"] < 5:
        missed.append("%d unitigs of 500 bases or more" % c["unitigs_500"])
    if c["coverage_outliers"] < 1 and not c["coverage_filter_changes"]:
        missed.append("the coverage filter changes nothing")
    if c["reads_scrubbed"] < 1:
        missed.append("the scrubber changes no read")
    if c["exact_rows_accepted"] < 100:
        missed.append("%d accepted rows in the exact PAF" % c["exact_rows_accepted"])
    if c["contigs"] < 1:
        missed.append("no contig")
    return missed
