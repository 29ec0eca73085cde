"""The mapper, host side (no GPU): the plain-Python restatement (tests/map_oracle.py) against its own recorded results for the
hand-made cases (tests/golden/mapper, made by tools/make_mapper_fixtures.py), its invariants on every workload, the conditions
the GPU tests rely on (checked on the restatement alone), the C-ABI's symbols, the command line's argument check, and the
error without a device.

A hand case worked out on paper (k = 4, w = 1, so every k-mer position is a minimizer): target ``ACGGTTCA`` against the query
``CGGTTC``.  The query's 4-mers CGGT, GGTT, GTTC sit at target positions 1, 2, 3 with the same strand bits, so the group
(0, 0, +) has the anchors (1, 0), (2, 1), (3, 2) (none of the three is its own reverse complement: rc(GGTT) = AACC).
f = 4, 5, 6 (gain 1 per link, dd = 0), one chain of 3 anchors with score 6, target range [1, 7), query range [0, 6),
block = matches = 4 + 1 + 1 = 6."""
import json
import os
import subprocess
import sys

import pytest

import map_oracle
import mapcases

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = os.path.join(ROOT, "tests", "golden", "mapper")
sys.path.insert(0, os.path.join(ROOT, "tools"))


@pytest.fixture(scope="module")
def mp():
    import __graft_entry__ as g
    g.build()
    from muchsalsa_amd import mapper
    return mapper


def test_paper_cases():
    r = map_oracle.run([(b"t", b"ACGGTTCA")], [(b"q", b"CGGTTC")], k=4, w=1, min_score=6, min_count=3)
    assert r["chains"] == [(0, 0, 0, 3, 6, 0, 0, 6, 1, 7, 6, 6)]
    assert r["paf"] == b"q\t6\t0\t6\t+\tt\t8\t1\t7\t6\t6\t255\tcm:i:3\ts1:i:6\n"
    assert map_oracle.run([(b"t", b"ACGGTTCA")], [(b"q", b"CGGTTC")], k=4, w=1, min_score=7, min_count=3)["chains"] == []
    r = map_oracle.run([(b"t", b"ACGGTTCA")], [(b"q", b"GAACCG")], k=4, w=1, min_score=6, min_count=3, exact=1)
    assert r["chains"] == [(0, 0, 1, 3, 6, 0, 0, 6, 1, 7, 6, 6)] and r["paf"].endswith(b"s1:i:6\tNM:i:0\n")
    # the gap cost: dd = 5 at k = 15 costs 5 * 15 // 100 + (2 >> 1) = 1
    f, pred = map_oracle.chain_dp([(0, 0), (20, 25)], 15, 10000, 2000)
    assert (f, pred) == ([15, 29], [-1, 0])
    assert map_oracle.chain_dp([(0, 0), (20, 2025)], 15, 10000, 2000)[1] == [-1, -1]  # dd = 2005 > bandwidth
    assert map_oracle.chain_dp([(0, 0), (10001, 10001)], 15, 10000, 2000)[1] == [-1, -1]  # beyond max_gap
    # the 64 predecessors: anchor 65 cannot see anchor 0
    far = [(0, 0)] + [(1000 + i, 5000 - i) for i in range(64)] + [(2000, 6000)]
    assert map_oracle.chain_dp(far, 15, 10000, 10000)[1][-1] != 0
    assert map_oracle.banded_distance(b"ACGT", b"AGT", 2) == 1 and map_oracle.banded_distance(b"", b"AAA", 2) == 3
    assert map_oracle.banded_distance(b"AAAA", b"TTTT", 2) == 3 and map_oracle.banded_distance(b"", b"", 1) == 0
    assert map_oracle.revcomp(b"ACGTNacg") == b"gcaNACGT"
    assert map_oracle.minimizers(b"ACGTACGTAC", 4, 8) == [] and len(map_oracle.minimizers(b"ACGTACGTAC", 4, 7)) >= 1


@pytest.mark.parametrize("name", mapcases.HAND)
def test_restatement_against_its_recorded_results(name):
    import make_mapper_fixtures
    with open(os.path.join(GOLD, name + ".json")) as f:
        want = json.load(f)
    assert make_mapper_fixtures.record(name) == want


def test_hand_cases_are_what_they_are_made_for():
    e = mapcases.expected
    assert len(e("perfect")["chains"]) == 1 and e("perfect")["chains"][0][2] == 0 and e("perfect")["notes"]["short_links"] > 0
    assert e("perfect")["chains"][0][10] == e("perfect")["chains"][0][11]  # matches = block
    assert [c[2] for c in e("reverse")["chains"]] == [1]
    assert e("reverse")["chains"][0][6:10] == e("perfect")["chains"][0][6:10]
    assert [g[4] for g in e("two_chains")["groups"]] == [2]
    assert e("cut")["chains_cut"] == 1 and len(e("cut")["chains"]) == 2
    assert e("one_sided")["notes"]["one_sided"] >= 1 and e("one_sided")["chains"][0][5] == 6
    assert e("beyond_band")["capped"] == 1 and e("beyond_band")["chains"][0][5] == 65
    assert e("n_split")["minimizers"][1] < e("perfect")["minimizers"][1]
    assert e("short_stretch")["chains"][0][0] == 1 and map_oracle.minimizers(mapcases._records("short_stretch")[1][0][1], 15, 5) == []
    assert e("empty_queries")["paf"] == b"" and e("empty_queries")["minimizers"][1] == 0
    assert e("over_max_occ")["keys_dropped"] > 0 and e("over_max_occ", max_occ=200)["keys_dropped"] == 0
    assert e("over_max_occ")["paf"] != e("over_max_occ", max_occ=200)["paf"]


@pytest.mark.parametrize("case", mapcases.CASES, ids=mapcases.case_id)
def test_restatement_invariants(case):
    r = mapcases.expected(case[0], **case[1])
    t, q = mapcases._records(case[0])
    mapcases.invariants(r, t, t if q is None else q)
    if r["params"]["ava"]:
        assert all(c[0] < c[1] for c in r["chains"])
    if not r["params"]["exact"]:
        assert all(c[5] == 0 for c in r["chains"]) and b"NM:i:" not in r["paf"]


def test_the_workloads_meet_the_conditions():
    """what keeps the GPU tests from passing on nothing"""
    e = mapcases.expected
    main = e("main")
    strands = [c[2] for c in main["chains"]]
    assert strands.count(0) >= 10 and strands.count(1) >= 10
    assert main["largest_group"] > 64 and any(g[4] >= 2 for g in main["groups"]) and main["chains_cut"] >= 1
    assert main["below_score"] >= 1 and e("small", min_score=40, min_count=10)["below_count"] >= 1
    low = e("main", max_occ=12)
    assert low["keys_dropped"] >= 1 and main["keys_dropped"] == 0 and low["paf"] != main["paf"]
    assert main["notes"]["start_ties"] >= 1 and main["notes"]["pred_ties"] >= 1  # ties in f resolved by index
    assert e("clean", exact=1, band=8)["capped"] >= 1 and e("clean", exact=1)["capped"] == 0
    ava = e("main_ava")
    assert ava["chains"] and all(c[0] < c[1] for c in ava["chains"]) and ava["largest_group"] > 64
    assert main["groups_small"] >= 1 and main["groups_large"] >= 1


def test_the_tiled_paf_passes_the_overlap_loader(mp, tmp_path):
    """at least 100 lines of the exact-mode PAF pass msgpu_parse_paf's default thresholds (a host call)"""
    from muchsalsa_amd import overlap
    path = os.path.join(str(tmp_path), "tiled.paf")
    with open(path, "wb") as f:
        f.write(mapcases.expected("tiled", exact=1)["paf"])
    paf = overlap.parse_paf(path)
    assert len(paf.rows) >= 100


def test_abi_exports_every_mapper_symbol(mp):
    import ctypes as C
    from muchsalsa_amd import _lib
    names = ["msgpu_map_" + n for n in ("default_params", "create", "destroy", "last_error", "run", "result_stats", "result_chains",
                                        "result_text", "result_free")]
    header = open(os.path.join(ROOT, "include", "msgpu.h")).read()
    bound = {n for n, _, _ in _lib.SYMBOLS}
    for n in names:
        assert hasattr(_lib.lib(), n) and n in bound and n + "(" in header, n
    assert C.sizeof(_lib.MapParams) == 48 and C.sizeof(_lib.MapChain) == 48 and C.sizeof(_lib.MapStats) == 424
    prm = _lib.MapParams()
    _lib.lib().msgpu_map_default_params(C.byref(prm))
    assert {k: getattr(prm, k) for k in mp.DEFAULTS} == mp.DEFAULTS == map_oracle.PARAMS and prm.max_pred == map_oracle.MAX_PRED


def test_the_three_statements_of_the_rules_agree(mp):
    header = " ".join(open(os.path.join(ROOT, "include", "msgpu.h")).read().replace(" *", " ").split())
    doc = " ".join(mp.__doc__.split())
    for phrase in ("A window's minimizer is its position with the smallest (h, position)",
                   "A key with more than max_occ entries is left out whole",
                   "else qlen - k - position", "/ 100 + (floor(log2(dd)) >> 1)", "the largest such j on a tie",
                   "score = f(start) - (f(u) if it ended at a used anchor, else 0)", "min(distance, band + 1)",
                   "matches = k + sum (c_i + max(lt_i, lq_i) - d_i)", "fewer than 2^31 index entries, anchors and segment pairs"):
        assert phrase in header and phrase in doc, phrase
    for word in ("not minimap2's", "leftmost-minimum", "occurrence cap", "64 predecessors", "integer gap cost", "--dual",
                 "primary / secondary", "mapping quality", "no CIGAR", "end extension"):
        assert word in doc, word
    from muchsalsa_amd import scrubber
    assert "muchsalsa_amd.mapper" in scrubber.__doc__ and "--ava" in scrubber.__doc__


def test_command_line_rejects_bad_arguments(mp, tmp_path):
    env = dict(os.environ, PYTHONPATH=ROOT)
    p = [str(tmp_path / n) for n in ("t.fa", "q.fa", "out.paf")]

    def code(*args):
        out = subprocess.run([sys.executable, "-m", "muchsalsa_amd.mapper"] + list(args), cwd=ROOT, env=env, capture_output=True,
                             timeout=300)
        if out.returncode == 2:
            assert b"python -m muchsalsa_amd.mapper" in out.stderr
        return out.returncode

    assert code() == 2 and code(*p[:2]) == 2 and code(*p, "extra") == 2 and code(*p, "-k") == 2 and code(*p, "-k", "x") == 2
    assert code(*p, "-k", "3") == 2 and code(*p, "-k", "33") == 2 and code(*p, "-w", "0") == 2 and code(*p, "-w", "65") == 2
    assert code(*p, "--max-occ", "0") == 2 and code(*p, "--band", "128") == 2 and code(*p, "--what", "1") == 2
    assert code(*p, "--ava") == 2 and code(*p, "--max-gap", "-1") == 2
    assert not os.path.exists(p[2])


def test_no_device_means_an_error_not_a_fallback(mp, tmp_path):
    import torch
    if torch.cuda.is_available():
        pytest.skip("a GPU is present: the stage would run")
    import ctypes as C
    from muchsalsa_amd import _lib
    ctx = C.c_void_p()
    assert _lib.lib().msgpu_map_create(0, C.byref(ctx)) == _lib.E_NODEVICE and not ctx.value
    tp, qp = mapcases.write_inputs("perfect", tmp_path)
    out = os.path.join(str(tmp_path), "out.paf")
    with pytest.raises(mp.MapError) as e:
        mp.run(tp, qp, out)
    assert e.value.code == _lib.E_NODEVICE and not os.path.exists(out)


def test_the_workload_generator_is_deterministic():
    from muchsalsa_amd import synth
    a, b = synth.mapper_workload(**mapcases.TINY), synth.mapper_workload(**mapcases.TINY)
    assert a["reads"] == b["reads"] and a["unitigs"] == b["unitigs"] and a["genome"] == b["genome"]
    reads = map_oracle.parse(a["reads"], True)
    assert len(reads) == 6 and all(n == b"r%d" % i for i, (n, _) in enumerate(reads))
    assert all(500 <= len(s) <= 3000 for _, s in map_oracle.parse(a["unitigs"], False))
    big = synth.mapper_workload(**mapcases.MAIN)["reads"]
    assert b"N" in big.replace(b"@", b"") and any(c in big for c in (b"a", b"c", b"g", b"t"))
    tiled = synth.mapper_workload(**mapcases.TILED)
    assert sum(int(x) for x in tiled["unitig_len"]) == len(tiled["genome"])
