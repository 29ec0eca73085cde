"""The unitig graph of the short-read unitig assembly (rule 10) on the GPU: the stage with the graph switched on against the
plain-Python restatement (tests/ug_graph_oracle.py) without any tolerance -- the GFA bytes, the link table and the statistics
-- on every unitig case of tests/kmeredgecases.py, the unitig tests' own workloads and the diploid one with and without
rule 9; and what must not depend on the feature: both FASTA texts and the unitig table, a context switched on, off and on,
partitions, one file or two, the mask, a second run, the device memory, the pipeline's files.  No test provokes a device
fault.  Every test runs under its own time limit: a watchdog ends the process when a stage call does not come back."""
import ctypes as C
import faulthandler
import hashlib
import json
import os
import subprocess
import sys

import pytest

import kmeredgecases as ec
import ug_graph_oracle as go
import ug_oracle
import ugbubblecases
import ugcases

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIMIT = 300  # seconds per test
UG_CASES = ec.names("ug")


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


def _write(d, datas, tag="x"):
    paths = [os.path.join(str(d), "%s.%d.fq" % (tag, i + 1)) for i in range(len(datas))]
    for path, data in zip(paths, datas):
        with open(path, "wb") as h:
            h.write(data)
    return paths


def _read(path):
    with open(path, "rb") as h:
        return h.read()


class _Ctx:
    """one msgpu_ugctx by ctypes: runs by files, and everything a result holds"""

    def __init__(self):
        from muchsalsa_amd import _lib
        self.lib, self.L, self.ctx = _lib, _lib.lib(), C.c_void_p()
        assert self.L.msgpu_ug_create(0, C.byref(self.ctx)) == _lib.OK

    def close(self):
        self.L.msgpu_ug_destroy(self.ctx)

    def graph(self, on):
        assert self.L.msgpu_ug_set_graph(self.ctx, on) == self.lib.OK

    def bubbles(self, bubble):
        assert self.L.msgpu_ug_set_bubbles(self.ctx, bubble) == self.lib.OK

    def run(self, k, paths, min_count=2, trim=None, min_length=500, budget=0):
        """-> dict: all, cut, gfa (bytes), unitigs (the table), links (the table), graph (the statistics without the times),
        ms (the three times)"""
        lib, L, res = self.lib, self.L, C.c_void_p()
        prm = lib.UgParams(k, min_count, -1 if trim is None else trim, min_length)
        rc = L.msgpu_ug_run(self.ctx, C.byref(prm), os.fsencode(paths[0]), os.fsencode(paths[1]) if len(paths) > 1 else None, 0,
                            budget, C.byref(res))
        assert rc == lib.OK, L.msgpu_ug_last_error(self.ctx)
        try:
            n = C.c_uint64()
            out = {}
            for key, which in (("all", lib.UG_TEXT_ALL), ("cut", lib.UG_TEXT_CUT), ("gfa", lib.UG_TEXT_GFA)):
                p = L.msgpu_ug_result_text(res, which, C.byref(n))
                out[key] = C.string_at(p, n.value)
            up = C.POINTER(lib.UgUnitig)()
            assert L.msgpu_ug_result_unitigs(res, C.byref(up), C.byref(n)) == lib.OK
            out["unitigs"] = [(int(u.length), int(u.coverage), (int(u.first_hi) << 64) | int(u.first_lo), int(u.offset), int(u.cyclic))
                              for u in (up[i] for i in range(n.value))]
            gs, lp = lib.UgGraphStats(), C.POINTER(lib.UgLink)()
            assert L.msgpu_ug_result_links(res, C.byref(gs), C.byref(lp), C.byref(n)) == lib.OK
            out["links"] = [(int(getattr(l, "from")), int(l.from_rev), int(l.to), int(l.to_rev)) for l in (lp[i] for i in range(n.value))]
            assert all(lp[i].reserved == 0 for i in range(n.value))
            out["graph"] = {f: int(getattr(gs, f)) for f in ("n_links", "n_adjacencies", "n_self_mirror", "n_dead_ends", "gfa_bytes")}
            out["ms"] = (gs.links_ms, gs.sort_ms, gs.text_ms)
            assert gs.reserved == 0
            st = lib.UgStats()
            L.msgpu_ug_result_stats(res, C.byref(st))
            assert st.n_lost_publications == 0 and list(st.bytes_out) == [len(out["all"]), len(out["cut"])]
        finally:
            L.msgpu_ug_result_free(res)
        return out


@pytest.fixture(scope="module")
def ctx(ug):
    c = _Ctx()
    yield c
    c.close()


OFF = {"n_links": 0, "n_adjacencies": 0, "n_self_mirror": 0, "n_dead_ends": 0, "gfa_bytes": 0}


def _is_off(got):
    assert got["gfa"] == b"" and got["links"] == [] and got["graph"] == OFF and got["ms"] == (0.0, 0.0, 0.0)


def _equals(got, want_graph):
    """a result of the stage with the graph on is the restatement's"""
    assert len(got["gfa"]) == len(want_graph["gfa"])
    assert got["gfa"] == want_graph["gfa"]
    assert got["links"] == want_graph["links"]
    assert got["graph"] == {"n_links": len(want_graph["links"]), "n_adjacencies": want_graph["adjacencies"],
                            "n_self_mirror": want_graph["self_mirror"], "n_dead_ends": want_graph["dead_ends"],
                            "gfa_bytes": len(want_graph["gfa"])}


def _on_and_off(ctx, k, paths, want, **prm):
    """the stage with the graph on against the restatement `want` (a result of ug_oracle.run), and its FASTA texts and unitig
    table against those of the stage with the graph off"""
    ctx.graph(1)
    on = ctx.run(k, paths, **prm)
    ctx.graph(0)
    off = ctx.run(k, paths, **prm)
    _is_off(off)
    for key in ("all", "cut", "unitigs"):
        assert on[key] == off[key], key
    assert on["all"] == want["all"] and on["cut"] == want["cut"] and on["unitigs"] == want["unitigs"]
    _equals(on, go.graph(want))
    return on


@pytest.mark.parametrize("name", UG_CASES)
def test_edge_cases(ctx, tmp_path, name):
    _, k, files, params = ec.cases()[name]
    on = _on_and_off(ctx, k, _write(tmp_path, files), ec.expected(name), **ec.oracle_params(params))
    print("%s: %d unitigs, %r, links %.3f ms, sort %.3f ms, text %.3f ms" % ((name, len(on["unitigs"]), on["graph"]) + on["ms"]))


@pytest.mark.parametrize("k", [15, 31, 32, 33, 64])
def test_small_workload(ctx, tmp_path, k):
    on = _on_and_off(ctx, k, _write(tmp_path, ugcases.files("small")), ugcases.expected("small", k))
    print("small, k %d: %d unitigs, %r, links %.3f ms, sort %.3f ms, text %.3f ms" % ((k, len(on["unitigs"]), on["graph"]) + on["ms"]))
    assert on["graph"]["n_links"] > 0


def test_k_2_overlaps_by_one_base(ctx, tmp_path):
    on = _on_and_off(ctx, 2, _write(tmp_path, ugcases.files("tiny")), ugcases.expected("tiny", 2))
    assert on["links"] and on["gfa"].endswith(b"\t1M\n")


def test_diploid_with_and_without_bubbles(ctx, tmp_path):
    paths = _write(tmp_path, [ugbubblecases.workload("diploid")[0]])
    popped, plain = ugbubblecases.expected("diploid", 31)[0], ugbubblecases.plain("diploid", 31)
    try:
        ctx.bubbles(93)
        a = _on_and_off(ctx, 31, paths, popped)
        ctx.bubbles(0)
        b = _on_and_off(ctx, 31, paths, plain)
    finally:
        ctx.bubbles(0)
    assert a["graph"]["n_links"] != b["graph"]["n_links"]
    print("diploid, k 31: %d links with bubble = 93, %d without" % (a["graph"]["n_links"], b["graph"]["n_links"]))


def test_partitions_files_and_the_mask_do_not_change_the_graph(ug, ctx, tmp_path):
    import test_gpu_unitigs_bubbles as bubble_tests
    from muchsalsa_amd import kmer_filter
    k, datas = 31, ugcases.files("small")
    want = ugcases.expected("small", k)
    want_graph = go.graph(want)
    mb = bubble_tests._budget_for(ug, tmp_path, k, datas, 3, 20, want["windows"])
    p = bubble_tests._paths(tmp_path, "three")
    bubble_tests._write(p, datas)
    gfa, tables = os.path.join(str(tmp_path), "three.gfa"), {}
    res = ug.run(k, p[0], p[1], p[2], p[3], budget_mb=mb, tables=tables, gfa=gfa)
    assert res["partitions"] == 3 and _read(gfa) == want_graph["gfa"] and tables["links"] == want_graph["links"]
    assert (res["links"], res["link_self_mirror"], res["dead_ends"], res["gfa_bytes"]) == (
        len(want_graph["links"]), want_graph["self_mirror"], want_graph["dead_ends"], len(want_graph["gfa"]))
    assert _read(p[2]) == want["all"] and _read(p[3]) == want["cut"]
    # one file against two
    ctx.graph(1)
    try:
        one = ctx.run(k, _write(tmp_path, [b"".join(datas)], "one"))
    finally:
        ctx.graph(0)
    _equals(one, want_graph)
    # a pair under a mask against the files of the kept records
    recs = [[d.split(b"\n")[i:i + 4] for i in range(0, d.count(b"\n"), 4)] for d in datas]
    half = min(len(recs[0]), len(recs[1]))
    mask = bytes(1 if i % 3 == 1 else 0 for i in range(half))
    text = lambda rs: b"".join(b"\n".join(r) + b"\n" for r in rs)
    whole = _write(tmp_path, [text(recs[0][:half]), text(recs[1][:half])], "whole")
    kept = _write(tmp_path, [text([r for r, m in zip(rs[:half], mask) if not m]) for rs in recs], "kept")
    by_files = dict(tables={}, gfa=os.path.join(str(tmp_path), "kept.gfa"))
    by_pair = dict(tables={}, gfa=os.path.join(str(tmp_path), "pair.gfa"))
    a = ug.run(k, kept[0], kept[1], p[2], p[3], **by_files)
    with kmer_filter.Pair(whole[0], whole[1]) as pair:
        b = ug.run(k, None, None, p[2], p[3], pair=pair, dropped=mask, **by_pair)
    assert _read(by_pair["gfa"]) == _read(by_files["gfa"]) and by_pair["tables"] == by_files["tables"]
    assert {key: a[key] for key in ("links", "link_self_mirror", "dead_ends", "gfa_bytes")} == {
        key: b[key] for key in ("links", "link_self_mirror", "dead_ends", "gfa_bytes")}
    assert _read(by_files["gfa"]) == go.graph(ug_oracle.run(k, [_read(x) for x in kept]))["gfa"] and a["links"] > 0


def test_one_context_on_off_on_and_two_runs(ug, tmp_path):
    want = ec.expected("dense-5-60-0")
    _, k, files, params = ec.cases()["dense-5-60-0"]
    paths, prm = _write(tmp_path, files), ec.oracle_params(params)
    c = _Ctx()
    try:
        fresh = c.run(k, paths, **prm)  # a new context has the graph off
        _is_off(fresh)
        c.graph(1)
        first, again = c.run(k, paths, **prm), c.run(k, paths, **prm)
        c.graph(0)
        off = c.run(k, paths, **prm)
        c.graph(7)  # any value but 0 is on
        third = c.run(k, paths, **prm)
    finally:
        c.close()
    _is_off(off)
    _equals(first, go.graph(want))
    for r in (first, again, third):
        assert all(t > 0 for t in r.pop("ms"))
    fresh.pop("ms"), off.pop("ms")
    assert first == again == third and fresh == off
    assert {key: first[key] for key in ("all", "cut", "unitigs")} == {key: off[key] for key in ("all", "cut", "unitigs")}


def test_the_python_dict_changes_only_with_gfa(ug, tmp_path):
    _, k, files, params = ec.cases()["selfcomp-4"]
    p = _write(tmp_path, files) + [os.path.join(str(tmp_path), n) for n in ("all.fa", "cut.fa", "g.gfa")]
    prm = ec.oracle_params(params)
    t_off, t_on, s_off, s_on = {}, {}, {}, {}
    off = ug.run(k, p[0], None, p[1], p[2], tables=t_off, timings=s_off, **prm)
    assert not os.path.exists(p[3])
    on = ug.run(k, p[0], None, p[1], p[2], tables=t_on, timings=s_on, gfa=p[3], **prm)
    new = {"links", "link_self_mirror", "dead_ends", "gfa_bytes"}
    assert set(on) - set(off) == new and {key: on[key] for key in off} == off and "links" not in t_off
    assert set(s_on) - set(s_off) == {"graph_links", "graph_sort", "graph_text"}
    want = go.graph(ec.expected("selfcomp-4"))
    assert _read(p[3]) == want["gfa"] and t_on["links"] == want["links"] and on["gfa_bytes"] == len(want["gfa"])
    with pytest.raises(ug.UnitigError):  # on any error nothing is written
        ug.run(1, p[0], None, p[1] + ".e", p[2] + ".e", gfa=p[3] + ".e")
    assert not any(os.path.exists(x + ".e") for x in p[1:])


def test_no_device_memory_is_lost(ug, tmp_path):
    import torch
    _, k, files, params = ec.cases()["dense-6-100-0"]
    paths, prm = _write(tmp_path, files), ec.oracle_params(params)

    def cycle():
        c = _Ctx()
        try:
            c.graph(1)
            assert c.run(k, paths, **prm)["graph"]["n_links"] == 8446
        finally:
            c.close()

    cycle()  # warm-up: the runtime's pools, the kernels' code objects
    torch.cuda.synchronize()
    before = torch.cuda.mem_get_info(0)[0]
    for _ in range(2):
        cycle()
    torch.cuda.synchronize()
    after = torch.cuda.mem_get_info(0)[0]
    print("free device memory: %d bytes before the first create, %d after the last destroy" % (before, after))
    assert after >= before


def test_the_command_line_writes_the_graph(ug, tmp_path):
    _, k, files, params = ec.cases()["hairpin-64"]
    p = _write(tmp_path, files) + [str(tmp_path / n) for n in ("all.fa", "cut.fa", "g.gfa")]
    env = dict(os.environ, PYTHONPATH=ROOT)
    out = subprocess.run([sys.executable, "-m", "muchsalsa_amd.unitigs", str(k), p[0], p[0], p[1], p[2], "--min-count", "2",
                          "--min-length", "0", "--gfa", p[3]], cwd=ROOT, env=env, capture_output=True, timeout=LIMIT)
    assert out.returncode == 0, out.stderr
    res = json.loads(out.stdout)
    want = ug_oracle.run(k, [files[0], files[0]], min_count=2, min_length=0)  # (the command line takes two files)
    g = go.graph(want)
    assert _read(p[3]) == g["gfa"] and _read(p[1]) == want["all"]
    assert (res["links"], res["link_self_mirror"], res["dead_ends"], res["gfa_bytes"]) == (2, 2, g["dead_ends"], len(g["gfa"]))
    assert set(res["seconds"]) >= {"graph_links", "graph_sort", "graph_text"}


@pytest.mark.parametrize("name", ["dense-6-100-0", "rings-64", "hairpin-64", "selfcomp-4"])
def test_on_a_poisoned_arena(ctx, tmp_path, monkeypatch, name):
    monkeypatch.setenv("MSGPU_POISON", "1")  # (the arena asks per call)
    _, k, files, params = ec.cases()[name]
    _on_and_off(ctx, k, _write(tmp_path, files), ec.expected(name), **ec.oracle_params(params))


def test_the_pipeline_writes_the_graph_on_request(ug, tmp_path):
    import hybridcases
    from muchsalsa_amd import hybrid, kmer_filter
    inputs = hybridcases.write_inputs(tmp_path)
    out, plain = str(tmp_path / "out"), str(tmp_path / "plain")
    res = hybrid.run(hybridcases.K_FILTER, hybridcases.K_ASSEMBLY, hybridcases.NAME, inputs[0], inputs[1], inputs[2], out, gfa=True)
    wrong = []
    for rel, rec in sorted(hybridcases.expected()["files"].items()):
        data = _read(os.path.join(out, rel))
        if (len(data), hashlib.sha256(data).hexdigest()) != (rec["bytes"], rec["sha256"]):
            wrong.append(rel)
    assert wrong == []
    assert res["files"]["gfa"] == os.path.join(os.path.realpath(out), hybrid.gfa_name(hybridcases.NAME))
    # the stage alone on the same pair and mask, and the restatement on the files of the kept records
    d = str(tmp_path)
    f1, f2, direct = os.path.join(d, "f1.fq"), os.path.join(d, "f2.fq"), os.path.join(d, "direct.gfa")
    tables = {}
    with kmer_filter.Pair(inputs[0], inputs[1]) as pair:
        kmer_filter.run(hybridcases.K_FILTER, None, None, os.path.join(d, "report.txt"), f1, f2, pair=pair, tables=tables)
        alone = ug.run(hybridcases.K_ASSEMBLY, None, None, os.path.join(d, "a.fa"), os.path.join(d, "c.fa"), pair=pair,
                       dropped=tables["verdict"], min_length=hybrid.MIN_LENGTH, gfa=direct)
    assert _read(res["files"]["gfa"]) == _read(direct)
    assert {key: v for key, v in res["unitigs"].items() if key != "seconds"} == alone and alone["links"] > 0
    want = ug_oracle.run(hybridcases.K_ASSEMBLY, [_read(f1), _read(f2)], min_length=hybrid.MIN_LENGTH)
    assert _read(direct) == go.graph(want)["gfa"] and _read(res["files"]["unitigs"]) == want["all"]
    # without gfa: no entry, no file
    res = hybrid.run(hybridcases.K_FILTER, hybridcases.K_ASSEMBLY, hybridcases.NAME, inputs[0], inputs[1], inputs[2], plain)
    assert "gfa" not in res["files"] and "links" not in res["unitigs"]
    assert not any(n.endswith(".gfa") for _, _, names in os.walk(plain) for n in names)
