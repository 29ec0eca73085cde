"""The whole-pipeline command (muchsalsa_amd.hybrid) without a GPU: the new symbols and structs of the two device-resident
hand-offs, the command's usage, the names of its output files, the link, the error without a device, the recorded expectation
of tests/golden/hybrid and the workload it was recorded on."""
import ctypes as C
import os

import pytest

import hybridcases


@pytest.fixture(scope="module")
def lib():
    import __graft_entry__ as g
    g.build()
    from muchsalsa_amd import _lib
    return _lib


def test_the_new_symbols_exist_and_the_structs_have_their_sizes(lib):
    L = lib.lib()
    for name in ("msgpu_kf_open_pair", "msgpu_pair_close", "msgpu_kf_run_pair", "msgpu_ug_run_pair", "msgpu_map_index_create",
                 "msgpu_map_index_free", "msgpu_map_index_stats", "msgpu_map_run_index"):
        assert hasattr(L, name) and name in {n for n, _, _ in lib.SYMBOLS}, name
    # msgpu_map_istats: five 64-bit counts, k and w, five times in ms and a reserved word
    assert C.sizeof(lib.MapIndexStats) == 5 * 8 + 2 * 4 + 5 * 4 + 4 == 72
    assert [f for f, _ in lib.MapIndexStats._fields_][:7] == ["n_records", "n_bases", "n_minimizers", "n_keys", "n_index_entries", "k", "w"]
    # the existing structs are as they were: the hand-offs add no field
    assert C.sizeof(lib.KfStats) == 176 and C.sizeof(lib.UgStats) == 224 and C.sizeof(lib.MapStats) == 424
    from muchsalsa_amd import kmer_filter, mapper, unitigs
    import inspect
    assert "pair" in inspect.signature(kmer_filter.run).parameters and "index" in inspect.signature(mapper.run).parameters
    assert {"pair", "dropped"} <= set(inspect.signature(unitigs.run).parameters)
    assert hasattr(kmer_filter, "Pair") and hasattr(mapper, "Index")


def test_null_arguments_are_codes(lib):
    L, out = lib.lib(), C.c_void_p()
    prm = lib.MapParams()
    L.msgpu_map_default_params(C.byref(prm))
    assert L.msgpu_kf_open_pair(None, b"a", b"b", C.byref(out)) == lib.E_ARG
    assert L.msgpu_kf_run_pair(None, 21, None, 0, 0, C.byref(out)) == lib.E_ARG
    assert L.msgpu_ug_run_pair(None, None, None, None, 0, 0, 0, C.byref(out)) == lib.E_ARG
    assert L.msgpu_map_index_create(None, C.byref(prm), b"t", C.byref(out)) == lib.E_ARG
    assert L.msgpu_map_run_index(None, C.byref(prm), None, None, 0, 0, C.byref(out)) == lib.E_ARG
    assert L.msgpu_map_index_stats(None, None) == lib.E_ARG
    L.msgpu_pair_close(None)
    L.msgpu_map_index_free(None)


@pytest.mark.parametrize("n", (0, 6, 10))
def test_usage(lib, n, capsys):
    from muchsalsa_amd import hybrid
    assert hybrid.main(["21", "31", "x", "a", "b", "c", "out", "4", "8G", "more"][:n]) == 2
    err = capsys.readouterr().err
    assert "python -m muchsalsa_amd.hybrid <k_filter> <k_assembly> <name>" in err and "[cores=4] [bloom_mem]" in err


def test_a_k_that_is_no_number_is_the_usage(lib, capsys):
    from muchsalsa_amd import hybrid
    assert hybrid.main(["k", "31", "x", "a", "b", "c", "out"]) == 2


@pytest.mark.parametrize("path,base", [("reads.fastq", "reads"), ("reads.fq", "reads.fq"), ("dir/x.fastq", "x"),
                                       ("/data/run.1.fastq", "run.1"), ("a.b.fa", "a.b.fa")])
def test_output_names(lib, path, base):
    from muchsalsa_amd import hybrid
    n = hybrid.output_names("asm", path)
    assert n["report"] == "report.txt" and n["assembly"] == "03.assembly.unpolished.fa"
    assert n["unitigs"] == os.path.join("ABYSS", "asm-unitigs.fa") and n["unitigs_cut"] == os.path.join("ABYSS", "asm-unitigs.l500.fa")
    assert n["link"] == "00_" + os.path.basename(path)
    assert n["unitigs_paf"] == "01_unitigs.to_%s.paf" % base and n["corrected_paf"] == "01_contigs_corrected.to_%s.paf" % base
    assert n["scrubbed"] == "02_%s.scrubbed.fa" % base and n["exact_paf"] == "02_contigs_corrected.to_%s.scrubbed.paf" % base
    assert n["corrected"] == os.path.join("tmp", "unitigs_corrected.fa") and n["ava_paf"] == os.path.join("tmp", base + ".ava.paf")
    assert [n[k] for k in ("target", "query", "align")] == [os.path.join("tmp", "temp_1." + x) for x in ("target.fa", "query.fa", "align.paf")]
    assert len(set(n.values())) == len(n)


def test_the_link_is_relative(lib, tmp_path):
    from muchsalsa_amd import hybrid
    (tmp_path / "in").mkdir()
    (tmp_path / "runs" / "out").mkdir(parents=True)
    src = tmp_path / "in" / "reads.fastq"
    src.write_bytes(b"@r\nACGT\n+\nIIII\n")
    for _ in (0, 1):  # a second run replaces the link
        link = hybrid.link_input(str(src), str(tmp_path / "runs" / "out"))
        assert link == str(tmp_path / "runs" / "out" / "00_reads.fastq") and os.path.islink(link)
        assert os.readlink(link) == os.path.join("..", "..", "in", "reads.fastq")
        with open(link, "rb") as h:
            assert h.read() == src.read_bytes()


def test_a_missing_or_empty_input_names_the_file_and_creates_nothing(lib, tmp_path):
    from muchsalsa_amd import hybrid
    a, b, c = (tmp_path / n for n in ("1.fq", "2.fq", "reads.fq"))
    a.write_bytes(b"@r\nACGT\n+\nIIII\n")
    b.write_bytes(b"")
    for second, third in ((b, c), (a, c)):  # an empty file; a missing one
        with pytest.raises(hybrid.HybridError) as e:
            hybrid.run(21, 31, "x", str(a), str(second), str(third), str(tmp_path / "out"))
        assert e.value.stage == "inputs" and str(third if second is a else second) in str(e.value)
    assert not (tmp_path / "out").exists()


def test_without_a_device_the_first_stage_says_so(lib, tmp_path):
    import torch
    if torch.cuda.is_available():
        return  # (tests/test_gpu_hybrid.py runs the command where a device exists)
    from muchsalsa_amd import hybrid
    paths = hybridcases.write_inputs(tmp_path)
    with pytest.raises(hybrid.HybridError) as e:
        hybrid.run(21, 31, "x", paths[0], paths[1], paths[2], str(tmp_path / "out"))
    assert e.value.stage == "open_pair" and str(e.value).startswith("open_pair: ") and e.value.cause.code == lib.E_NODEVICE
    assert sorted(os.listdir(tmp_path / "out")) == ["00_" + hybridcases.READS_NAME, "ABYSS", "tmp"]


def test_the_recorded_expectation_meets_the_conditions(lib):
    from muchsalsa_amd import hybrid
    e = hybridcases.expected()
    assert hybridcases.conditions_missed(e) == []
    assert (e["shape"], e["k_filter"], e["k_assembly"], e["name"], e["reads_name"]) == (
        hybridcases.SHAPE, hybridcases.K_FILTER, hybridcases.K_ASSEMBLY, hybridcases.NAME, hybridcases.READS_NAME)
    names = hybrid.output_names(hybridcases.NAME, hybridcases.READS_NAME)
    assert set(e["files"]) == set(names.values()) - {names["link"]}
    for rec in e["files"].values():
        assert rec["bytes"] > 0 and len(rec["sha256"]) == 64
    assert e["files"][names["assembly"]] == e["files"][names["target"]]
    wl = hybridcases.workload()
    assert e["counts"]["pairs"] == wl["illumina_1"].count(b"\n") // 4 and e["counts"]["long_reads"] == hybridcases.SHAPE["n_long"]


def test_the_workload_is_deterministic_in_its_seed(lib):
    from muchsalsa_amd import synth
    shape = dict(hybridcases.SHAPE, genome=6000, n_long=8, long_len=1000, copies=2, repeat_len=300)
    a, b, c = synth.hybrid_workload(**shape), synth.hybrid_workload(**shape), synth.hybrid_workload(**dict(shape, seed=shape["seed"] + 1))
    for key in ("illumina_1", "illumina_2", "reads", "genome"):
        assert a[key] == b[key] and a[key] != c[key], key
    assert a["illumina_1"].count(b"\n") == a["illumina_2"].count(b"\n") == 4 * (6000 * 40 // 200)
    assert a["reads"].count(b"\n") == 4 * 8 and a["reads"].startswith(b"@r0\n")
    assert synth.hybrid_workload(**dict(shape, fastq=False))["reads"].startswith(b">r0\n")
    # the Illumina pairs are kmer_filter_workload's on the same genome
    kf = synth.kmer_filter_workload(genome=6000, coverage=40, read_len=100, seed=shape["seed"], families=2, copies=2, repeat_len=300)
    assert (a["illumina_1"], a["illumina_2"]) == kf
