"""The whole pipeline as one command on the GPU (muchsalsa_amd.hybrid), on the workload of
tests/hybridcases.py: every file the driver writes has the length and SHA-256 recorded in tests/golden/hybrid/expected.json (the
whole chain on the CPU with the tests' restatements, tools/make_hybrid_fixtures.py), and equals, byte for byte, what the existing
stage functions give when they are called one after the other through files -- the filtered FASTQ files included.  Nothing here
has a tolerance.  Every test runs under its own time limit."""
import faulthandler
import hashlib
import json
import os
import subprocess
import sys

import pytest

import hybridcases

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIMIT = 600  # seconds per test


@pytest.fixture(scope="module")
def hy():
    import __graft_entry__ as g
    g.build()
    from muchsalsa_amd import hybrid
    return hybrid


@pytest.fixture(autouse=True)
def time_limit(hy):
    faulthandler.dump_traceback_later(LIMIT, exit=True)
    yield
    faulthandler.cancel_dump_traceback_later()


@pytest.fixture(scope="module")
def inputs(tmp_path_factory):
    return hybridcases.write_inputs(tmp_path_factory.mktemp("hybrid_in"))


@pytest.fixture(scope="module")
def driven(hy, inputs, tmp_path_factory):
    """the driver's run, once -> (result, output folder)"""
    out = str(tmp_path_factory.mktemp("hybrid_out") / "out")
    res = hy.run(hybridcases.K_FILTER, hybridcases.K_ASSEMBLY, hybridcases.NAME, inputs[0], inputs[1], inputs[2], out)
    print(json.dumps({k: v for k, v in res.items() if k != "files"}))
    return res, out


def read(path):
    with open(path, "rb") as h:
        return h.read()


def test_every_file_has_the_recorded_length_and_digest(hy, driven):
    res, out = driven
    e = hybridcases.expected()
    wrong = []
    for rel, rec in sorted(e["files"].items()):
        data = read(os.path.join(out, rel))
        print("%-50s %8d bytes (recorded %8d)" % (rel, len(data), rec["bytes"]))
        if (len(data), hashlib.sha256(data).hexdigest()) != (rec["bytes"], rec["sha256"]):
            wrong.append(rel)
    assert wrong == []
    c = e["counts"]
    assert (res["filter"]["pairs_in"], res["filter"]["pairs_in"] - res["filter"]["pairs_out"], res["filter"]["upper"]) == (
        c["pairs"], c["pairs_dropped"], c["threshold"])
    assert (res["unitigs"]["unitigs"], res["unitigs"]["kept"]) == (c["unitigs"], c["unitigs_500"])
    assert (res["map_unitigs"]["chains"], res["map_corrected"]["chains"], res["ava"]["chains"], res["map_exact"]["chains"]) == (
        c["unitigs_paf_rows"], c["corrected_paf_rows"], c["ava_rows"], c["exact_rows"])
    assert (res["assembly"]["rows"], res["assembly"]["contigs"]) == (c["exact_rows_accepted"], c["contigs"])
    assert res["index"]["records"] == c["long_reads"] and res["unitigs"]["lost_publications"] == 0
    link = os.path.join(out, hy.output_names(hybridcases.NAME, inputs_name())["link"])
    assert os.path.islink(link) and not os.path.isabs(os.readlink(link))
    assert not any("filtered" in n or n.endswith((".histo", ".jf")) for _, _, names in os.walk(out) for n in names)


def inputs_name():
    return hybridcases.READS_NAME


def test_the_files_equal_the_chain_of_the_stages_by_files(hy, driven, inputs, tmp_path):
    """what the parent of this change offers: eight calls, every hand-off a file"""
    from muchsalsa_amd import kmer_filter, mapper, pipeline, scrubber, unitig_filter, unitigs
    res, out = driven
    names = hy.output_names(hybridcases.NAME, inputs[2])
    d = str(tmp_path)
    p = {k: os.path.join(d, k) for k in ("report", "f1.fq", "f2.fq", "all.fa", "cut.fa", "u.paf", "corrected.fa", "c.paf", "ava.paf",
                                         "scrubbed.fa", "exact.paf")}
    kmer_filter.run(hybridcases.K_FILTER, inputs[0], inputs[1], p["report"], p["f1.fq"], p["f2.fq"])
    assert 0 < os.path.getsize(p["f1.fq"]) < os.path.getsize(inputs[0])
    unitigs.run(hybridcases.K_ASSEMBLY, p["f1.fq"], p["f2.fq"], p["all.fa"], p["cut.fa"], min_length=500)
    mapper.run(inputs[2], p["cut.fa"], p["u.paf"])
    unitig_filter.run(p["u.paf"], p["cut.fa"], p["report"], p["corrected.fa"])
    mapper.run(inputs[2], p["corrected.fa"], p["c.paf"])
    mapper.run(inputs[2], inputs[2], p["ava.paf"], ava=1)
    scrubber.run(p["c.paf"], inputs[2], p["scrubbed.fa"], p["ava.paf"])
    mapper.run(p["scrubbed.fa"], p["corrected.fa"], p["exact.paf"], exact=1)
    os.mkdir(os.path.join(d, "asm"))
    pipeline.run(p["exact.paf"], p["corrected.fa"], p["scrubbed.fa"], os.path.join(d, "asm"), threads=4)
    same = {"report": "report", "unitigs": "all.fa", "unitigs_cut": "cut.fa", "unitigs_paf": "u.paf", "corrected": "corrected.fa",
            "corrected_paf": "c.paf", "ava_paf": "ava.paf", "scrubbed": "scrubbed.fa", "exact_paf": "exact.paf"}
    for key, mine in same.items():
        assert read(os.path.join(out, names[key])) == read(p[mine]), key
    for key, mine in (("target", "temp_1.target.fa"), ("query", "temp_1.query.fa"), ("align", "temp_1.align.paf"),
                      ("assembly", "temp_1.target.fa")):
        assert read(os.path.join(out, names[key])) == read(os.path.join(d, "asm", mine)), key


def test_the_command_line_in_a_fresh_process(hy, driven, inputs, tmp_path):
    out = str(tmp_path / "cli")
    p = subprocess.run([sys.executable, "-m", "muchsalsa_amd.hybrid", str(hybridcases.K_FILTER), str(hybridcases.K_ASSEMBLY),
                        hybridcases.NAME, inputs[0], inputs[1], inputs[2], out, "4", "8G"], cwd=ROOT, capture_output=True, text=True,
                       timeout=LIMIT)
    assert p.returncode == 0, p.stderr[-2000:]
    res = json.loads(p.stdout.strip().splitlines()[-1])
    assert res["assembly"]["contigs"] == driven[0]["assembly"]["contigs"] >= 1
    assert read(os.path.join(out, "03.assembly.unpolished.fa")) == read(os.path.join(driven[1], "03.assembly.unpolished.fa"))


def test_a_missing_input_is_an_error_naming_the_file(hy, inputs, tmp_path):
    missing = str(tmp_path / "no_such_reads.fq")
    out = str(tmp_path / "out")
    with pytest.raises(hy.HybridError) as e:
        hy.run(hybridcases.K_FILTER, hybridcases.K_ASSEMBLY, hybridcases.NAME, inputs[0], inputs[1], missing, out)
    assert e.value.stage == "inputs" and missing in str(e.value)
    assert not os.path.exists(out) or os.listdir(out) == []
    p = subprocess.run([sys.executable, "-m", "muchsalsa_amd.hybrid", "21", "31", "x", inputs[0], missing, inputs[2], out], cwd=ROOT,
                       capture_output=True, text=True, timeout=LIMIT)
    assert p.returncode != 0 and missing in p.stderr
