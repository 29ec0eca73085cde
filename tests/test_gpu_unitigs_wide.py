"""Short-read unitig assembly above k = 64 on the GPU (``unitigs.run(..., wide=True)``, msgpu_ug_set_wide): keys of three 64-bit
words at k = 65..96 and of four at k = 97..128.  Every case (tests/ugwidecases.py) is compared without any tolerance with the
restatement at any k (tests/ug_wide_oracle.py): both FASTA texts, the unitig table with the whole first k-mer
(msgpu_ug_result_first_kmers), the counts, the tip rounds, the bubble rounds and the GFA text where the case asks for them.
Beside the cases: the switch itself (off: today's refusal of k = 65 in today's words; on: k <= 64 gives the bytes it gives with
the switch off, on one context, in both orders), the pair path behind the k-mer filter's mask, and the hybrid command at
k_assembly = 65.  Every test runs under its own time limit: a watchdog ends the process when a stage call does not come back."""
import ctypes as C
import faulthandler
import os

import pytest

import kmeredgecases as E
import ug_wide_oracle
import ugwidecases as cases

pytestmark = pytest.mark.gpu

LIMIT = 600  # seconds per test


@pytest.fixture(scope="module")
def ug():
    import __graft_entry__ as g
    g.build()
    from muchsalsa_amd import unitigs
    return unitigs


@pytest.fixture(autouse=True)
def time_limit(ug):  # (after ug: the build is not the test's time)
    faulthandler.dump_traceback_later(LIMIT, exit=True)  # works while the main thread sits in a native call
    yield
    faulthandler.cancel_dump_traceback_later()


def _paths(d, tag="x"):
    return [os.path.join(str(d), tag + "." + n) for n in ("1.fq", "2.fq", "all.fa", "cut.fa", "gfa")]


def _write(paths, datas):
    for path, data in zip(paths, datas):
        with open(path, "wb") as h:
            h.write(data)


def _read(path):
    with open(path, "rb") as h:
        return h.read()


def _stage(ug, d, k, datas, tag="x", graph=False, wide=True, **kw):
    p = _paths(d, tag)
    _write(p, datas)
    tables, timings = {}, {}
    res = ug.run(k, p[0], p[1] if len(datas) > 1 else None, p[2], p[3], device=0, tables=tables, timings=timings, wide=wide,
                 gfa=p[4] if graph else None, **kw)
    tables["peak_bytes"] = timings["peak_bytes"]
    return res, tables, [_read(x) for x in (p[2:] if graph else p[2:4])]


def _equal(res, tb, texts, want):
    """a result of the stage is the restatement's: the texts, the tables, every count"""
    n_files = len(want["records"])
    assert tb["rounds"] == want["rounds"] and res["tip_rounds"] == len(want["rounds"])
    assert tb["bubble_rounds"] == want["bubble_rounds"]
    assert (res["bubble"], res["bubbles"], res["bubble_kmers"]) == (want["bubble"], want["bubbles"], want["bubble_kmers"])
    assert (res["records"][:n_files], res["windows"], res["distinct"], res["solid"], res["solid_after"]) == (
        want["records"], want["windows"], want["distinct"], want["solid"], want["solid_after"])
    assert (res["unitigs"], res["kept"], res["cycles"], res["longest"]) == (
        len(want["unitigs"]), want["kept"], want["cycles"], want["longest"])
    assert tb["unitigs"] == want["unitigs"]  # (length, coverage, the whole first k-mer, offset, cyclic)
    assert len(texts[0]) == len(want["all"]) and len(texts[1]) == len(want["cut"])
    assert texts[0] == want["all"] and texts[1] == want["cut"]
    assert res["bytes_out"] == [len(texts[0]), len(texts[1])] and res["lost_publications"] == 0
    if "graph" in want:
        g = want["graph"]
        assert texts[2] == g["gfa"] and tb["links"] == g["links"]
        assert (res["links"], res["link_self_mirror"], res["dead_ends"], res["gfa_bytes"]) == (
            len(g["links"]), g["self_mirror"], g["dead_ends"], len(g["gfa"]))


def check_case(ug, d, name, tag="x"):
    """the case on the stage against the restatement -> (the stage's counts, its tables, its texts, the restatement's result)"""
    k, files, params = cases.cases()[name]
    want = cases.expected(name)
    res, tb, texts = _stage(ug, d, k, files, tag, **params)
    print("%s: rounds %r, bubble rounds %r, %d unitigs (%d kept, %d cycles), longest %d, %d partitions" % (
        name, tb["rounds"], tb["bubble_rounds"], res["unitigs"], res["kept"], res["cycles"], res["longest"], res["partitions"]))
    assert res["k"] == k and tb["peak_bytes"] >= 2 * (24 if k <= 96 else 32) * res["largest_partition"]  # the two key buffers
    _equal(res, tb, texts, want)
    return res, tb, texts, want


@pytest.mark.parametrize("name", cases.names(cases.HAND))
def test_hand_made_cases(ug, tmp_path, name):
    res, _, _, want = check_case(ug, tmp_path, name)
    if name.startswith("rings"):
        assert want["cycles"] == 2 and want["longest"] == 300
    if name.startswith("selfcomp"):
        assert want["alone"] >= 1 and want["blocked"] >= 1
    if name.startswith("hairpin"):
        assert want["blocked"] >= 1


@pytest.mark.parametrize("k", cases.KS)
def test_ladders(ug, tmp_path, k):
    """tips of every limit and every limit + 1: the rounds are the plan (kmeredgecases.ladder_plan), the walks and the joins
    read keys whose top word is in use"""
    _, tb, _, want = check_case(ug, tmp_path, "ladder-%d-%d" % (k, k))
    assert want["rounds"] == E.ladder_plan(k) == tb["rounds"] and sum(r for _, r in want["rounds"]) > 3 * k


@pytest.mark.parametrize("k", cases.KS_EDGE)
def test_the_order_rests_on_the_top_word_and_on_the_lowest(ug, tmp_path, k):
    """two first k-mers that differ in their first base alone, two in their last alone: a sort that drops a word, or takes the
    words the wrong way round, fails here"""
    _, tb, _, want = check_case(ug, tmp_path, "words-%d" % k)
    x1, x2, y1, y2 = (cases.kmer_of(t) for t in cases.words_reads(k)[1])
    firsts = [t[2] for t in want["unitigs"]]
    assert all(x in firsts for x in (x1, x2, y1, y2))  # each starts a unitig of its own, in the emitted orientation
    assert x1 ^ x2 == 1 << (2 * k - 2) and y1 ^ y2 == 1 and (x1 >> 64 * ((2 * k - 1) // 64)) != (x2 >> 64 * ((2 * k - 1) // 64))
    got = [t[2] for t in tb["unitigs"]]
    assert got == sorted(got) == firsts and got.index(x1) < got.index(x2) and got.index(y1) + 1 == got.index(y2)


@pytest.mark.parametrize("k", cases.KS_SMALL)
def test_small_workload(ug, tmp_path, k):
    want = cases.expected("small-%d" % k)
    assert any(removed for _, removed in want["rounds"]) and want["kept"] >= 2  # the reference reaches the kernels aimed at
    assert want["solid_after"] < want["solid"] < want["distinct"] and want["other_bytes"] > 0
    res, _, _, _ = check_case(ug, tmp_path, "small-%d" % k)
    assert res["trim"] == k and res["min_count"] == 2 and res["min_length"] == 500


@pytest.mark.parametrize("flip", (False, True), ids=("as_written", "flipped"))
@pytest.mark.parametrize("k", cases.KS_EDGE)
@pytest.mark.parametrize("name", cases.BUBBLES)
def test_bubbles(ug, tmp_path, name, k, flip):
    full = "%s-%d%s" % (name, k, "-flip" if flip else "")
    assert cases.bubble_conditions(full)[1] == []
    res, _, _, _ = check_case(ug, tmp_path, full)
    assert res["bubble"] == 3 * k and res["bubbles"] == 1


class Ctx:
    """one msgpu_ugctx by ctypes: the switches, runs by files, and what the accessors say about each"""

    def __init__(self):
        from muchsalsa_amd import _lib
        self.lib, self.L, self.ctx = _lib, _lib.lib(), C.c_void_p()
        assert self.L.msgpu_ug_create(0, C.byref(self.ctx)) == _lib.OK

    def close(self):
        self.L.msgpu_ug_destroy(self.ctx)

    def error(self):
        return self.L.msgpu_ug_last_error(self.ctx)

    def run(self, k, paths, min_count=2, trim=-1, min_length=500):
        """-> (code, None) or (OK, dict: all, cut, gfa (bytes), unitigs (the table), graph (rule 10's counts))"""
        lib, L, res = self.lib, self.L, C.c_void_p()
        prm = lib.UgParams(k, min_count, trim, min_length)
        rc = L.msgpu_ug_run(self.ctx, C.byref(prm), os.fsencode(paths[0]), os.fsencode(paths[1]) if len(paths) > 1 else None, 0, 0,
                            C.byref(res))
        if rc != lib.OK:
            assert not res.value
            return rc, None
        try:
            out, n = {}, C.c_uint64()
            for key, which in (("all", lib.UG_TEXT_ALL), ("cut", lib.UG_TEXT_CUT), ("gfa", lib.UG_TEXT_GFA)):
                out[key] = C.string_at(L.msgpu_ug_result_text(res, which, C.byref(n)), n.value)
            up, fp, fw = C.POINTER(lib.UgUnitig)(), C.POINTER(C.c_uint64)(), C.c_uint32()
            assert L.msgpu_ug_result_unitigs(res, C.byref(up), C.byref(n)) == lib.OK
            units = [(int(u.length), int(u.coverage), int(u.first_hi), int(u.first_lo), int(u.offset), int(u.cyclic))
                     for u in (up[i] for i in range(n.value))]
            assert L.msgpu_ug_result_first_kmers(res, C.byref(fp), C.byref(fw), C.byref(n)) == lib.OK and n.value == len(units)
            out["words"] = fw.value
            out["unitigs"] = [(u[0], u[1], sum(int(fp[i * fw.value + j]) << (64 * j) for j in range(fw.value)), u[4], u[5])
                              for i, u in enumerate(units)]
            out["low128"] = [(u[2] << 64) | u[3] for u in units]
            gs, lp = lib.UgGraphStats(), C.POINTER(lib.UgLink)()
            assert L.msgpu_ug_result_links(res, C.byref(gs), C.byref(lp), C.byref(n)) == lib.OK
            out["graph"] = {f: int(getattr(gs, f)) for f in ("n_links", "n_adjacencies", "n_self_mirror", "n_dead_ends", "gfa_bytes")}
            return rc, out
        finally:
            L.msgpu_ug_result_free(res)


@pytest.fixture
def ctx(ug):
    c = Ctx()
    yield c
    c.close()


@pytest.mark.parametrize("k", cases.KS_EDGE)
@pytest.mark.parametrize("name", ("three_in", "hairpin"))
def test_graph(ug, ctx, tmp_path, name, k):
    """rule 10 on wide keys: the links of a fork case and of the hairpin, "<k-1>M", and the counts' identity"""
    full = "%s-%d" % ("hairpin_gfa" if name == "hairpin" else name, k)
    _, tb, texts, want = check_case(ug, tmp_path, full)
    g = want["graph"]
    assert g["links"] and texts[2].endswith(b"\t%dM\n" % (k - 1)) and texts[2].count(b"\t%dM\n" % (k - 1)) == len(g["links"])
    if name == "three_in":
        assert g["adjacencies"] >= 8 and not g["self_mirror"]  # in-degree 4: the forks stay at trim = 0
    else:
        assert g["self_mirror"] >= 1  # i+ -> i-: its own mirror
    # the counts through the C interface: adjacencies = 2 links - self-mirrored links
    _, files, params = cases.cases()[full]
    p = _paths(tmp_path, "c")
    _write(p, files)
    assert ctx.L.msgpu_ug_set_wide(ctx.ctx, 1) == ctx.lib.OK and ctx.L.msgpu_ug_set_graph(ctx.ctx, 1) == ctx.lib.OK
    rc, got = ctx.run(k, p[:len(files)], min_count=params.get("min_count", 2), trim=params.get("trim", -1),
                      min_length=params["min_length"])
    assert rc == ctx.lib.OK and got["gfa"] == g["gfa"] and got["unitigs"] == want["unitigs"] and got["words"] == (3 if k <= 96 else 4)
    assert got["graph"] == {"n_links": len(g["links"]), "n_adjacencies": g["adjacencies"], "n_self_mirror": g["self_mirror"],
                            "n_dead_ends": g["dead_ends"], "gfa_bytes": len(g["gfa"])}
    assert got["graph"]["n_adjacencies"] == 2 * got["graph"]["n_links"] - got["graph"]["n_self_mirror"]
    assert got["low128"] == [t[2] & ((1 << 128) - 1) for t in want["unitigs"]]  # first_hi, first_lo: the low 128 bits


def test_the_switch(ug, ctx, tmp_path):
    lib, L = ctx.lib, ctx.L
    k, files, params = cases.cases()["ladder-65-65"]
    p = _paths(tmp_path, "s")
    _write(p, files)
    run65 = lambda k_=65: ctx.run(k_, p[:1], min_count=1, trim=k, min_length=0)  # noqa: E731
    # off, what a new context has: today's refusal in today's words
    assert run65() == (lib.E_ARG, None) and ctx.error() == b"k = 65 is outside 2..64"
    assert L.msgpu_ug_set_wide(None, 1) == lib.E_ARG
    # on: 2..128
    assert L.msgpu_ug_set_wide(ctx.ctx, 1) == lib.OK
    assert run65(129) == (lib.E_ARG, None) and ctx.error() == b"k = 129 is outside 2..128"
    assert run65(1) == (lib.E_ARG, None) and ctx.error() == b"k = 1 is outside 2..128"
    rc, got = run65()
    want = cases.expected("ladder-65-65")
    assert rc == lib.OK and ctx.error() == b"" and got["all"] == want["all"] and got["unitigs"] == want["unitigs"] and got["words"] == 3
    # off again: the refusal is back
    assert L.msgpu_ug_set_wide(ctx.ctx, 0) == lib.OK
    assert run65() == (lib.E_ARG, None) and ctx.error() == b"k = 65 is outside 2..64"
    with pytest.raises(ug.UnitigError) as e:
        ug.run(65, p[0], None, p[2], p[3], device=0, min_count=1, min_length=0)
    assert e.value.code == lib.E_ARG and "k = 65 is outside 2..64" in str(e.value) and not os.path.exists(p[2])


@pytest.mark.parametrize("k", (33, 64))
@pytest.mark.parametrize("wide_first", (False, True), ids=("off_then_on", "on_then_off"))
def test_narrow_k_is_untouched_by_the_switch(ug, ctx, tmp_path, k, wide_first):
    """k <= 64 with the switch on: the bytes and the table of the run with it off, on one context, in both orders"""
    name = "ladder-%d-%d" % (k, k)
    _, _, files, params = E.cases()[name]
    want = E.expected(name)
    p = _paths(tmp_path, "n")
    _write(p, files)
    got = {}
    for on in ((1, 0) if wide_first else (0, 1)):
        assert ctx.L.msgpu_ug_set_wide(ctx.ctx, on) == ctx.lib.OK
        rc, got[on] = ctx.run(k, p[:1], min_count=params["min_count"], trim=params["trim"], min_length=params["min_length"])
        assert rc == ctx.lib.OK
    assert got[0] == got[1] and got[1]["words"] == 2
    assert got[1]["all"] == want["all"] and got[1]["cut"] == want["cut"] and got[1]["unitigs"] == want["unitigs"]


# (on this shape the filter at k = 21 drops 287 of 1066 pairs, and 20 of the 43 unitigs at k = 65 have 200 bases or more)
PAIR_SHAPE = dict(genome=20000, coverage=16, read_len=150, seed=4, families=2, copies=4, repeat_len=300)


def test_the_pair_path_behind_the_filters_mask(ug, tmp_path):
    """msgpu_ug_run_pair at k = 65 on a resident pair with the k-mer filter's verdicts at k = 21 as the mask gives what the run
    by files gives on the filter's two output files"""
    from muchsalsa_amd import kmer_filter, synth
    p = [os.path.join(str(tmp_path), n) for n in ("1.fq", "2.fq", "report.txt", "f.1.fq", "f.2.fq")]
    _write(p, synth.kmer_filter_workload(**PAIR_SHAPE))
    out = {tag: [os.path.join(str(tmp_path), "%s.%s.fa" % (tag, n)) for n in ("all", "cut")] for tag in ("pair", "files")}
    tb = {"pair": {}, "files": {}}
    with kmer_filter.Pair(p[0], p[1]) as pair:
        ft = {}
        kf = kmer_filter.run(21, None, None, p[2], p[3], p[4], pair=pair, tables=ft)
        assert 0 < kf["pairs_out"] < kf["pairs_in"]
        a = ug.run(65, None, None, out["pair"][0], out["pair"][1], pair=pair, dropped=ft["verdict"], tables=tb["pair"], min_length=200,
                   wide=True)
    b = ug.run(65, p[3], p[4], out["files"][0], out["files"][1], tables=tb["files"], min_length=200, wide=True)
    for key in ("windows", "distinct", "solid", "solid_after", "rounds", "unitigs", "kept", "cycles", "longest"):
        assert a[key] == b[key], key
    assert tb["pair"] == tb["files"] and [_read(x) for x in out["pair"]] == [_read(x) for x in out["files"]]
    want = ug_wide_oracle.run(65, [_read(p[3]), _read(p[4])], min_length=200)
    assert _read(out["pair"][0]) == want["all"] and tb["pair"]["unitigs"] == want["unitigs"] and 0 < a["kept"] < a["unitigs"]
    assert a["records"] == [kf["pairs_in"]] * 2 and b["records"] == [kf["pairs_out"]] * 2


HYBRID_SHAPE = dict(genome=30000, seed=3, coverage=40, read_len=150, n_long=64, long_len=3000)  # tests/hybridcases.py's, reads of 150


def test_hybrid_at_k_assembly_65(ug, tmp_path):
    """the hybrid command's shape at k_assembly = 65 (the existing fixture's reads are 100 bases, too short for 2 x 65): it
    switches the wide keys on by itself, reaches the assembly, and its unitig files are the stand-alone stage's on the
    filter's outputs; wide = False keeps the refusal.  No claim about the assembly beyond its existence."""
    from muchsalsa_amd import hybrid, kmer_filter, synth
    wl = synth.hybrid_workload(**HYBRID_SHAPE)
    inputs = [os.path.join(str(tmp_path), n) for n in ("illumina_1.fq", "illumina_2.fq", "nanopore.fastq")]
    _write(inputs, [wl[key] for key in ("illumina_1", "illumina_2", "reads")])
    with pytest.raises(hybrid.HybridError) as e:
        hybrid.run(21, 65, "hy", inputs[0], inputs[1], inputs[2], os.path.join(str(tmp_path), "refused"), wide=False)
    assert e.value.stage == "unitigs" and "k = 65 is outside 2..64" in str(e.value)
    out = os.path.join(str(tmp_path), "out")
    res = hybrid.run(21, 65, "hy", inputs[0], inputs[1], inputs[2], out)
    assert os.path.isfile(res["files"]["assembly"]) and res["unitigs"]["k"] == 65 and res["unitigs"]["unitigs"] > 0
    p = [os.path.join(str(tmp_path), n) for n in ("report.txt", "f.1.fq", "f.2.fq", "all.fa", "cut.fa")]
    kmer_filter.run(21, inputs[0], inputs[1], p[0], p[1], p[2])
    alone = ug.run(65, p[1], p[2], p[3], p[4], min_length=hybrid.MIN_LENGTH, wide=True)
    assert _read(res["files"]["unitigs"]) == _read(p[3]) and _read(res["files"]["unitigs_cut"]) == _read(p[4])
    assert alone["unitigs"] == res["unitigs"]["unitigs"] and alone["kept"] == res["unitigs"]["kept"]
