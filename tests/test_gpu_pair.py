"""The short-read pair that stays in device memory (msgpu_pair) and the unitig stage's mask (rule 8 of
include/msgpu.h): a run on a resident pair under a mask equals, without any tolerance, the run by files on the two files the
test writes itself from the kept records -- both texts, the unitig table, the rounds and the counts.  The reference is the
stage by files, whose own tests compare it with the restatement.  Bad arguments are rejected with an error code; no test
provokes a device fault.  Every test runs under its own time limit."""
import ctypes as C
import faulthandler
import functools
import os

import pytest

pytestmark = pytest.mark.gpu

LIMIT = 600  # seconds per test
SHAPE = dict(genome=6000, coverage=30, read_len=100, seed=13, families=2, copies=4, repeat_len=300)  # 900 pairs
SAME = ("windows", "distinct", "solid", "solid_after", "unitigs", "kept", "cycles", "longest", "rounds", "tip_rounds", "bytes_out")


@pytest.fixture(scope="module")
def mods():
    import __graft_entry__ as g
    g.build()
    from muchsalsa_amd import _lib, kmer_filter, unitigs
    return _lib, kmer_filter, unitigs


@pytest.fixture(autouse=True)
def time_limit(mods):
    faulthandler.dump_traceback_later(LIMIT, exit=True)
    yield
    faulthandler.cancel_dump_traceback_later()


@functools.lru_cache(maxsize=None)
def records(n=None):
    """-> (records of file 1, records of file 2), the first n pairs of the workload (None: all)"""
    from muchsalsa_amd import synth
    out = []
    for data in synth.kmer_filter_workload(**SHAPE):
        lines = data.split(b"\n")[:-1]
        recs = [b"\n".join(lines[i:i + 4]) + b"\n" for i in range(0, len(lines), 4)]
        out.append(tuple(recs[:n]))
    assert len(out[0]) == len(out[1]) == (900 if n is None else n)
    return out[0], out[1]


def write(d, tag, recs, keep=None):
    """the two files of the records i with keep[i] (None: all) -> their paths"""
    paths = []
    for m, side in enumerate(recs):
        p = os.path.join(str(d), "%s.%d.fq" % (tag, m + 1))
        with open(p, "wb") as h:
            h.write(b"".join(r for i, r in enumerate(side) if keep is None or keep[i]))
        paths.append(p)
    return paths


def unitigs_of(ug, d, tag, k, **kw):
    """the stage by files or on a pair -> (counts or the error's code, tables, both texts)"""
    out = [os.path.join(str(d), "%s.%s.fa" % (tag, n)) for n in ("all", "cut")]
    tables = {}
    try:
        res = ug.run(k, kw.pop("in_1", None), kw.pop("in_2", None), out[0], out[1], tables=tables, min_length=100, **kw)
    except ug.UnitigError as e:
        return e.code, None, None
    texts = []
    for p in out:
        with open(p, "rb") as h:
            texts.append(h.read())
    return res, tables, texts


def filter_of(kf, d, tag, k, **kw):
    out = [os.path.join(str(d), "%s.%s" % (tag, n)) for n in ("report.txt", "1.fq", "2.fq")]
    tables = {}
    res = kf.run(k, kw.pop("in1", None), kw.pop("in2", None), out[0], out[1], out[2], tables=tables, **kw)
    texts = []
    for p in out:
        with open(p, "rb") as h:
            texts.append(h.read())
    return res, tables, texts


def same_filter(a, b):
    for key in ("pairs_in", "pairs_out", "windows", "distinct", "candidates", "q1", "q3", "upper", "abundant", "bytes_in", "bytes_out"):
        assert a[0][key] == b[0][key], key
    assert a[1]["histogram"] == b[1]["histogram"] and a[2] == b[2]
    for key in ("key_hi", "key_lo", "count", "verdict"):
        assert a[1][key].tobytes() == b[1][key].tobytes(), key


@functools.lru_cache(maxsize=None)
def verdicts(k):
    """the filter's own verdicts on the whole workload, from the run by files (computed once)"""
    import tempfile
    from muchsalsa_amd import kmer_filter
    with tempfile.TemporaryDirectory() as d:
        res, tb, _ = filter_of(kmer_filter, d, "v", k, **dict(zip(("in1", "in2"), write(d, "v", records()))))
    v = tuple(int(x) for x in tb["verdict"])
    assert 0 < sum(v) < len(v) == 900
    return v


def mask(name, n):
    if name == "none":
        return None
    if name == "filter":
        return list(verdicts(21))[:n]
    return {"all": [1] * n, "second": [i & 1 for i in range(n)], "first256": [int(i < 256) for i in range(n)],
            "but_last": [1] * (n - 1) + [0]}[name]


# the whole workload: every mask at both key widths; 1, 64 and 65 pairs (below, at and just above a wavefront): the masks that
# differ there; one case in three partitions
CASES = ([(None, m, k, None) for k in (21, 33) for m in ("none", "all", "filter", "second", "first256", "but_last")] +
         [(n, m, 21, None) for n in (1, 64, 65) for m in ("none", "all", "second", "but_last")] +
         [(65, "second", 33, None), (None, "filter", 21, "three"), (None, "second", 33, "three")])


@pytest.mark.parametrize("case", CASES, ids=lambda c: "-".join(str(x) for x in c))
def test_a_masked_pair_equals_the_files_of_the_kept_records(mods, tmp_path, case):
    _lib, kf, ug = mods
    n, mname, k, parts = case
    recs = records(n)
    n = len(recs[0])
    m = mask(mname, n)
    whole = write(tmp_path, "in", recs)
    kept = write(tmp_path, "kept", recs, None if m is None else [not x for x in m])
    want = unitigs_of(ug, tmp_path, "files", k, in_1=kept[0], in_2=kept[1])
    budget = None
    if parts == "three":  # a budget of a third of the windows' bytes (20 / 36 bytes per key), and a little: three partitions
        budget = want[0]["windows"] * (20 if k <= 32 else 36) / 2.6 / 2 ** 20
    with kf.Pair(whole[0], whole[1]) as pair:
        got = unitigs_of(ug, tmp_path, "pair", k, pair=pair, dropped=None if m is None else bytes(m), budget_mb=budget)
    if not isinstance(want[0], dict):  # an error by files: the same code on the pair
        assert got[0] == want[0]
        return
    assert isinstance(got[0], dict), got[0]
    print("%r: %d of %d pairs kept, %d windows, %d unitigs (%d kept), %d partitions" % (
        case, n - sum(m or []), n, got[0]["windows"], got[0]["unitigs"], got[0]["kept"], got[0]["partitions"]))
    for key in SAME:
        assert got[0][key] == want[0][key], key
    assert got[1] == want[1] and got[2] == want[2]
    assert got[0]["records"] == [n, n] and got[0]["bytes_in"] == [os.path.getsize(p) for p in whole]
    assert got[0]["lost_publications"] == 0
    if parts == "three":
        assert got[0]["partitions"] == 3
    if mname in ("none", "second", "filter") and n == 900:
        assert got[0]["unitigs"] > 0 and len(got[2][0]) > 0


def test_runs_leave_the_pair_untouched(mods, tmp_path):
    """filter at 21, unitigs at 31 under its verdicts, the filter again at 25: each equals its separate run by files"""
    _lib, kf, ug = mods
    recs = records()
    whole = write(tmp_path, "in", recs)
    with kf.Pair(whole[0], whole[1]) as pair:
        f21 = filter_of(kf, tmp_path, "p21", 21, pair=pair)
        v = f21[1]["verdict"]
        u31 = unitigs_of(ug, tmp_path, "p31", 31, pair=pair, dropped=v)
        f25 = filter_of(kf, tmp_path, "p25", 25, pair=pair)
    same_filter(f21, filter_of(kf, tmp_path, "f21", 21, in1=whole[0], in2=whole[1]))
    same_filter(f25, filter_of(kf, tmp_path, "f25", 25, in1=whole[0], in2=whole[1]))
    assert tuple(int(x) for x in v) == verdicts(21) and f21[2][1] == b"".join(r for r, x in zip(recs[0], v) if not x)
    want = unitigs_of(ug, tmp_path, "f31", 31, in_1=os.path.join(str(tmp_path), "p21.1.fq"), in_2=os.path.join(str(tmp_path), "p21.2.fq"))
    for key in SAME:
        assert u31[0][key] == want[0][key], key
    assert u31[1] == want[1] and u31[2] == want[2] and u31[0]["lost_publications"] == 0 and u31[0]["unitigs"] > 0


def test_bad_arguments_are_codes_and_leave_the_pair_usable(mods, tmp_path):
    _lib, kf, ug = mods
    import torch
    recs = records(65)
    whole = write(tmp_path, "in", recs)
    uneven = write(tmp_path, "uneven", (recs[0], recs[1][:64]))
    want = unitigs_of(ug, tmp_path, "files", 21, in_1=whole[0], in_2=whole[1])
    with kf.Pair(whole[0], whole[1]) as pair:
        for m in (bytes(64), bytes(66), b""):  # a wrong n_pairs
            assert unitigs_of(ug, tmp_path, "bad", 21, pair=pair, dropped=m)[0] == _lib.E_ARG
        if torch.cuda.device_count() > 1:  # a pair from another context's device
            L, ctx, res = _lib.lib(), C.c_void_p(), C.c_void_p()
            assert L.msgpu_kf_create(1, C.byref(ctx)) == _lib.OK
            try:
                assert L.msgpu_kf_run_pair(ctx, 21, pair.handle, 0, 0, C.byref(res)) == _lib.E_ARG and not res.value
                assert b"device" in L.msgpu_kf_last_error(ctx)
            finally:
                L.msgpu_kf_destroy(ctx)
        got = unitigs_of(ug, tmp_path, "pair", 21, pair=pair, dropped=bytes(65))
        assert got[1] == want[1] and got[2] == want[2]
    with kf.Pair(uneven[0], uneven[1]) as pair:  # files of unequal record counts take no mask, and the filter rejects them
        assert unitigs_of(ug, tmp_path, "bad", 21, pair=pair, dropped=bytes(65))[0] == _lib.E_ARG
        assert unitigs_of(ug, tmp_path, "bad", 21, pair=pair, dropped=bytes(64))[0] == _lib.E_ARG
        with pytest.raises(kf.KmerFilterError) as e:
            filter_of(kf, tmp_path, "bad", 21, pair=pair)
        assert e.value.code == _lib.E_FORMAT and (e.value.file, e.value.line) == (1, 4 * 64 + 1)
        got = unitigs_of(ug, tmp_path, "pair", 21, pair=pair)
        want = unitigs_of(ug, tmp_path, "files", 21, in_1=uneven[0], in_2=uneven[1])
        assert isinstance(got[0], dict) and got[1] == want[1] and got[2] == want[2] and got[0]["records"] == [65, 64]
    with pytest.raises(kf.KmerFilterError) as e:  # opening judges the files as the run by files does
        with kf.Pair(whole[0], os.path.join(str(tmp_path), "missing.fq")):
            pass
    assert e.value.code == _lib.E_IO and e.value.file == 1
