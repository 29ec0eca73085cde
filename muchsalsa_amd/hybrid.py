"""The whole pipeline as one command: from the two Illumina files and the long-read file to ``03.assembly.unpolished.fa``,
every step of the reference's ``pipeline/pipeline.sh`` as the GPU stage of this package, in the script's order.

    python -m muchsalsa_amd.hybrid <k_filter> <k_assembly> <name> <illumina_1.fq> <illumina_2.fq> <nanopore.fq|fa> <outdir> [cores=4] [bloom_mem]

takes the script's seven to nine positional arguments in its order (pipeline.sh:38-57) and prints one JSON line of per-stage
counts and seconds.  ``bloom_mem`` is accepted and ignored: the counts are exact.  jellyfish, bbduk, ABySS and minimap2 are
not needed.  k_assembly may be 2..128: above 64 the unitig assembly's wide keys are switched on (``run(..., wide=None)``); k_filter
stays 2..64.  The steps, after the inputs are checked to be non-empty files (pipeline.sh:125):

 1. the Illumina pair is opened: both files go to device memory once (kmer_filter.Pair);
 2. the k-mer abundance filter runs on it at k_filter; ``report.txt`` is created with the threshold line (pipeline.sh:136-151);
 3. the unitig assembly runs on the same resident pair at k_assembly with the filter's verdicts as its mask and
    min_length 500 (pipeline.sh:153-159): the filtered FASTQ files, the histogram and the k-mer dump are never written;
 4. the pair is closed;
 5. the index of the long reads is built once (mapper.Index);
 6. the cut unitigs are mapped onto it and the unitig coverage filter runs, appending to ``report.txt`` (pipeline.sh:161-165);
 7. the corrected unitigs are mapped onto the same index, the reads against themselves (ava) on the same index, and the
    scrubber runs (pipeline.sh:167-171);
 8. the index is freed;
 9. the corrected unitigs are mapped exactly onto the scrubbed reads, a new target file (pipeline.sh:173-175);
10. ``pipeline.run`` assembles, and its ``temp_1.target.fa`` is copied (pipeline.sh:177-181).

Files under ``outdir``, with the script's names (BASE = the long-read file's base name without a ``.fastq`` suffix, as
``basename "$NANO" .fastq`` gives it): ``report.txt``, ``ABYSS/<name>-unitigs.fa``, ``ABYSS/<name>-unitigs.l500.fa``,
``00_<long-read file name>`` (a relative symbolic link to the input, which every later step reads through),
``01_unitigs.to_<BASE>.paf``, ``01_contigs_corrected.to_<BASE>.paf``, ``02_<BASE>.scrubbed.fa``,
``02_contigs_corrected.to_<BASE>.scrubbed.paf``, ``03.assembly.unpolished.fa``.  What the script leaves in its temporary
folder goes under ``outdir/tmp/``: ``unitigs_corrected.fa``, ``<BASE>.ava.paf`` and the three ``temp_1.*`` files.
``run(..., gfa=True)`` adds ``ABYSS/<name>-unitigs.gfa``, the unitig graph (what ``abyss-pe graph=gfa`` leaves there).
``run(..., evaluate=K)`` adds ``06.assembly.evaluation.tsv``: QV and completeness of the assembly, and of its polished forms,
from the Illumina reads' k-mers at k = K (muchsalsa_amd.evaluate).

Between stages whose hand-off is one of those files -- the pipeline's deliverables and its checkpoints -- the file stays the
hand-off.  An error in any stage stops the run: HybridError, the stage's name in front of the stage's own message; the
files of the finished stages stay.
"""
import json
import os
import shutil
import sys
import time

from . import _lib

__all__ = ["HybridError", "MIN_LENGTH", "POLISHED_NAME", "POLISHED_MATES_NAME", "POLISHED_VCF_NAME", "POLISHED_MATES_VCF_NAME", "EVALUATION_NAME", "INTERLEAVED_NAME", "MATES_MAPPING", "gfa_name", "output_names", "link_input", "run", "main"]

MIN_LENGTH = 500  # pipeline.sh:29
POLISHED_NAME = "04.assembly.polished.fa"  # written only by run(..., polish=N): not one of output_names
POLISHED_MATES_NAME = "05.assembly.polished.mates.fa"  # written only by run(..., polish_mates=N): not one of output_names
POLISHED_VCF_NAME = "04.assembly.polished.vcf"  # written only by run(..., polish=1, vcf=True): not one of output_names
POLISHED_MATES_VCF_NAME = "05.assembly.polished.mates.vcf"  # written only by run(..., polish_mates=1, vcf=True), likewise
EVALUATION_NAME = "06.assembly.evaluation.tsv"  # written only by run(..., evaluate=K): not one of output_names
INTERLEAVED_NAME = os.path.join("tmp", "illumina.interleaved.fq")  # the two Illumina inputs as one file of pairs, likewise
# The mapper's parameters for the short reads of the polish_mates stage.  The mapper's default min_score of 100 is the score of
# a perfect 100-base read and would drop nearly every mate; 40 is a choice, unchecked on real reads.
MATES_MAPPING = dict(min_score=40)


class HybridError(RuntimeError):
    """A stage failed, or an input is missing: ``stage`` names it, ``cause`` is the stage's own exception (None: an input)."""

    def __init__(self, stage, message, cause=None):
        super().__init__("%s: %s" % (stage, message))
        self.stage, self.cause = stage, cause


def output_names(name, nanopore):
    """the files of a run, relative to the output folder, by what they are (pipeline.sh:130-181)"""
    file_name = os.path.basename(nanopore)
    base = file_name[:-len(".fastq")] if file_name.endswith(".fastq") and file_name != ".fastq" else file_name
    return {"report": "report.txt",
            "unitigs": os.path.join("ABYSS", "%s-unitigs.fa" % name),
            "unitigs_cut": os.path.join("ABYSS", "%s-unitigs.l%d.fa" % (name, MIN_LENGTH)),
            "link": "00_" + file_name,
            "unitigs_paf": "01_unitigs.to_%s.paf" % base,
            "corrected_paf": "01_contigs_corrected.to_%s.paf" % base,
            "scrubbed": "02_%s.scrubbed.fa" % base,
            "exact_paf": "02_contigs_corrected.to_%s.scrubbed.paf" % base,
            "assembly": "03.assembly.unpolished.fa",
            "corrected": os.path.join("tmp", "unitigs_corrected.fa"),
            "ava_paf": os.path.join("tmp", "%s.ava.paf" % base),
            "target": os.path.join("tmp", "temp_1.target.fa"),
            "query": os.path.join("tmp", "temp_1.query.fa"),
            "align": os.path.join("tmp", "temp_1.align.paf")}


def gfa_name(name):
    """the unitig graph beside the unitigs, written only by run(..., gfa=True): not one of output_names"""
    return os.path.join("ABYSS", "%s-unitigs.gfa" % name)


def link_input(path, directory, prefix="00_"):
    """pipeline.sh's make_link (91-99): a relative symbolic link to ``path`` in ``directory``, replacing one that exists"""
    link = os.path.join(directory, prefix + os.path.basename(path))
    target = os.path.relpath(os.path.realpath(path), os.path.realpath(directory))
    if os.path.lexists(link):
        os.remove(link)
    os.symlink(target, link)
    return link


def run(k_filter, k_assembly, name, illumina_1, illumina_2, nanopore, outdir, cores=4, bloom_mem=None, device=0, cigar=False,
        bubble=None, polish=None, extend=None, min_mapq=None, gfa=False, polish_mates=None, max_insert=None, evaluate=None, wide=None, vcf=False):
    """The whole pipeline (the module's docstring); returns one dict: per stage its counts and ``seconds`` (wall, the stage
    call alone; every stage call ends in a device synchronise), ``files`` (the names of output_names, absolute) and the
    total ``seconds``.  ``bloom_mem`` is ignored.  ``cigar`` = True: the exact mapping (step 9) aligns base by base and writes
    ``cg:Z:`` strings (muchsalsa_amd.mapper's rule 10), as pipeline.sh:175's ``-c --eqx`` asks for; every file written before
    that PAF is the same.  ``bubble`` (None or 0: off) is the unitig assembly's rule 9 parameter (muchsalsa_amd.unitigs): bubbles
    with branches of up to that many k-mers are popped before the unitigs are written.  ``polish`` (None or 0: off) = N >= 1 adds a
    last stage ``"polish"``: N rounds of muchsalsa_amd.polish of the assembly by the scrubbed reads into POLISHED_NAME, named by
    ``files["polished"]``; every other file is the same.  ``extend`` (None or 0: off) = N is the mapper's rule 11 parameter: step 9
    then runs with cigar = 1 and extend = N, and so does every mapping of the polish stage; every file written before step 9's
    PAF is the same.  ``min_mapq`` (None: off) = N goes to the polish stage only (muchsalsa_amd.polish's rule 2 in ranked form: its
    mappings run with the mapper's rule 12 on, and a read votes with its primaries of mapping quality N or more); the four
    mappings of the pipeline keep ranking off: their consumers read columns 1 to 11 and want every chain, as with ``-P``.
    ``gfa`` = True: the unitig assembly also writes its graph (muchsalsa_amd.unitigs' rule 10) to ``ABYSS/<name>-unitigs.gfa``
    (gfa_name), named by ``files["gfa"]``; every other file is the same.  ``polish_mates`` (None or 0: off) = N >= 1 adds a last
    stage ``"polish_mates"``, the accurate short reads' pass over the assembly: mapper.interleave writes the two Illumina inputs
    as one file of pairs (INTERLEAVED_NAME), then N rounds of muchsalsa_amd.polish with mates on (the mapper's rule 13, the
    polisher's rule 2 in mates form) polish the long-read-polished file if ``polish`` was given, else the assembly, into
    POLISHED_MATES_NAME, named by ``files["polished_mates"]``; every other file is the same.  Its mappings run with MATES_MAPPING
    (a min_score fit for 100-base reads: a choice, unchecked on real reads) and ``max_insert`` (None: the mapper's default);
    neither the extension nor the mapping quality threshold reaches this stage.  ``evaluate`` (None or 0: off) = K adds a last
    stage ``"evaluate"`` (muchsalsa_amd.evaluate): the Illumina pair is opened again (it is not kept resident through the mapping
    stages), one table of its k-mers is built at k = K, and the assembly, and the polished files where they were written, are
    evaluated on it into EVALUATION_NAME (QV per record and in total, completeness), named by ``files["evaluation"]``; every
    other file is the same.  ``wide`` (None: on exactly when k_assembly > 64) is the unitig assembly's switch for k up to 128
    (muchsalsa_amd.unitigs; pipeline.sh's README recommends k_assembly = 90); False keeps the refusal of k_assembly > 64.  The
    k-mer filter and the evaluation stay at k <= 64: their k are parameters of their own.  ``vcf`` = True: every polishing stage
    that was asked for also writes what it changed as VCF 4.2 (muchsalsa_amd.polish, rules V1 - V9) beside its FASTA, into
    POLISHED_VCF_NAME (``files["polished_vcf"]``) and POLISHED_MATES_VCF_NAME (``files["polished_mates_vcf"]``); such a stage
    with more than one round is a HybridError before any stage runs (a VCF's coordinates are its own round's draft's); every
    other file is the same."""
    from . import kmer_filter, mapper, pipeline, scrubber, unitig_filter, unitigs
    t_all = time.perf_counter()
    for path in (illumina_1, illumina_2, nanopore):  # pipeline.sh:68-75, 125
        if not os.path.isfile(path) or os.path.getsize(path) == 0:
            raise HybridError("inputs", "file '%s' is empty or does not exist" % path)
    if vcf:
        for key, rounds in (("polish", polish), ("polish_mates", polish_mates)):
            if rounds and int(rounds) > 1:
                raise HybridError(key, "vcf with %d rounds: a VCF's coordinates are those of the draft of its own round" % int(rounds))
    out = os.path.realpath(outdir)  # pipeline.sh:60
    names = output_names(name, nanopore)
    files = {key: os.path.join(out, rel) for key, rel in names.items()}
    for d in (out, os.path.join(out, "ABYSS"), os.path.join(out, "tmp")):
        os.makedirs(d, exist_ok=True)
    reads = link_input(nanopore, out)  # pipeline.sh:134: every step reads the link
    gfa_path = os.path.join(out, gfa_name(name)) if gfa else None
    result = {}

    def stage(key, fn, *args, **kw):
        t0 = time.perf_counter()
        try:
            res = fn(*args, **kw)
        except (RuntimeError, OSError, ValueError) as e:
            raise HybridError(key, str(e), e) from e
        result[key] = dict(res if isinstance(res, dict) else {}, seconds=round(time.perf_counter() - t0, 4))
        return res

    tables = {}
    pair = kmer_filter.Pair(illumina_1, illumina_2, device=device)
    stage("open_pair", pair.__enter__)
    try:
        stage("filter", kmer_filter.run, int(k_filter), None, None, files["report"], None, None, pair=pair, tables=tables)
        stage("unitigs", unitigs.run, int(k_assembly), None, None, files["unitigs"], files["unitigs_cut"], pair=pair,
              dropped=tables["verdict"], min_length=MIN_LENGTH, bubble=bubble, gfa=gfa_path,
              wide=int(k_assembly) > 64 if wide is None else bool(wide))
    finally:
        pair.__exit__(None, None, None)
    index = mapper.Index(reads, device=device)
    stage("index", lambda: {k: v for k, v in dict(index.__enter__().stats, seconds_of_build=index.stats["seconds"]).items() if k != "seconds"})
    try:
        stage("map_unitigs", mapper.run, None, files["unitigs_cut"], files["unitigs_paf"], index=index)
        stage("unitig_filter", unitig_filter.run, files["unitigs_paf"], files["unitigs_cut"], files["report"], files["corrected"],
              device=device)
        stage("map_corrected", mapper.run, None, files["corrected"], files["corrected_paf"], index=index)
        stage("ava", mapper.run, None, None, files["ava_paf"], index=index, ava=1)
    finally:
        index.__exit__(None, None, None)
    stage("scrubber", scrubber.run, files["corrected_paf"], reads, files["scrubbed"], files["ava_paf"], device=device)
    stage("map_exact", mapper.run, files["scrubbed"], files["corrected"], files["exact_paf"], device=device, exact=1,
          cigar=1 if cigar or extend else 0, extend=int(extend or 0))
    stage("assembly", pipeline.run, files["exact_paf"], files["corrected"], files["scrubbed"], os.path.join(out, "tmp"),
          threads=int(cores), device=device)
    shutil.copyfile(files["target"], files["assembly"])  # pipeline.sh:181
    result["files"] = dict(files, link=reads)
    if gfa:
        result["files"]["gfa"] = gfa_path
    if polish:
        from . import polish as polisher
        result["files"]["polished"] = os.path.join(out, POLISHED_NAME)
        more = {}
        if vcf:
            result["files"]["polished_vcf"] = more["vcf"] = os.path.join(out, POLISHED_VCF_NAME)
        stage("polish", polisher.run, files["assembly"], files["scrubbed"], result["files"]["polished"], rounds=int(polish),
              device=device, extend=int(extend or 0), min_mapq=min_mapq, **more)
    if polish_mates:
        from . import polish as polisher
        pairs = os.path.join(out, INTERLEAVED_NAME)
        result["files"]["interleaved"] = pairs
        result["files"]["polished_mates"] = os.path.join(out, POLISHED_MATES_NAME)
        stage("interleave", lambda: {"pairs": mapper.interleave(illumina_1, illumina_2, pairs)})
        more = {} if max_insert is None else {"max_insert": int(max_insert)}
        if vcf:
            result["files"]["polished_mates_vcf"] = more["vcf"] = os.path.join(out, POLISHED_MATES_VCF_NAME)
        stage("polish_mates", polisher.run, result["files"]["polished"] if polish else files["assembly"], pairs,
              result["files"]["polished_mates"], rounds=int(polish_mates), device=device, mates=True, **more, **MATES_MAPPING)
    if evaluate:
        from . import evaluate as evaluator
        result["files"]["evaluation"] = os.path.join(out, EVALUATION_NAME)
        drafts = [files["assembly"]] + [result["files"][key] for key in ("polished", "polished_mates") if key in result["files"]]
        stage("evaluate", evaluator.run, int(evaluate), illumina_1, illumina_2, drafts, result["files"]["evaluation"], device=device)
    result["seconds"] = round(time.perf_counter() - t_all, 4)
    return result


def main(argv):
    args = list(argv)
    try:
        if not 7 <= len(args) <= 9:
            raise ValueError
        k_filter, k_assembly = int(args[0]), int(args[1])
        cores = int(args[7]) if len(args) > 7 else 4
    except ValueError:
        sys.stderr.write(__doc__.split("\n\n")[1] + "\n")
        return 2
    try:
        out = run(k_filter, k_assembly, args[2], args[3], args[4], args[5], args[6], cores=cores,
                  bloom_mem=args[8] if len(args) > 8 else None)
    except HybridError as e:  # (pipeline.sh:12-18: the message, exit code 1)
        sys.stderr.write("ERROR: %s\n" % e)
        return 1
    print(json.dumps(out))
    return 0


if __name__ == "__main__":
    _lib.PRELOAD_TORCH = False  # this process never imports torch
    sys.exit(main(sys.argv[1:]))
