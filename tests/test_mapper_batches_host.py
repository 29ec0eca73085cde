"""The mapper's batches (rule 9), host side (no GPU): the three new symbols of the C-ABI and the size of msgpu_map_batch, the
properties of msgpu_map_batch_bytes that a greedy cut relies on, a plain-Python restatement of that cut (``greedy_cut``, which
the GPU tests compare the stage's plan with) on hand-made count vectors, the per-record anchors and bases of an input from
the restatement of the rules (``record_counts``), the conditions the GPU tests' budgets rely on, and ``--budget-mb``."""
import ctypes as C
import functools
import os
import re

import pytest

import map_oracle
import mapcases

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def mp():
    import __graft_entry__ as g
    g.build()
    from muchsalsa_amd import mapper
    return mapper


def batch_bytes(exact=0):
    """(anchors, query bases) -> msgpu_map_batch_bytes with the default parameters and this ``exact``"""
    from muchsalsa_amd import _lib
    prm = _lib.MapParams()
    _lib.lib().msgpu_map_default_params(C.byref(prm))
    prm.exact = int(exact)
    return lambda a, b: int(_lib.lib().msgpu_map_batch_bytes(C.byref(prm), a, b))


class RecordTooLarge(Exception):
    """the query record that fits no batch on its own"""

    def __init__(self, record):
        super().__init__(record)
        self.record = record


def greedy_cut(a, b, nbytes, budget):
    """Rule 9's cut.  a[r], b[r]: anchors and bases of query record r; nbytes(anchors, bases): the bytes of a batch.
    -> [(first record, records, anchors, bases)]"""
    out, r = [], 0
    while r < len(a):
        first, sa, sb = r, 0, 0
        while r < len(a) and sa + a[r] < 1 << 31 and nbytes(sa + a[r], sb + b[r]) <= budget:
            sa, sb, r = sa + a[r], sb + b[r], r + 1
        if r == first:
            raise RecordTooLarge(first)
        out.append((first, r - first, sa, sb))
    return out


@functools.lru_cache(maxsize=None)
def _record_counts(name, params):
    p = dict(map_oracle.PARAMS, **dict(params))
    targets, queries = mapcases._records(name)
    if p["ava"]:
        queries = targets
    index = map_oracle.build_index(targets, p["k"], p["w"], p["max_occ"])[0]
    a = [0] * len(queries)
    for (q, _, _), g in map_oracle.anchors(index, queries, p["k"], p["w"], p["ava"]).items():
        a[q] += len(g)
    return tuple(a), tuple(len(s) for _, s in queries)


def record_counts(name, **params):
    """-> (anchors per query record, bases per query record) of an input of mapcases, by rules 1 to 4 of the restatement"""
    if name in mapcases.HAND:
        params = dict(mapcases.hand_cases()[name][2], **params)
    if name.endswith("_ava"):
        params["ava"] = 1
    return _record_counts(name, tuple(sorted(params.items())))


def budgets(name, **params):
    """the GPU tests' budgets (i), (ii), (iii): every record fits; one batch; half-way"""
    a, b = record_counts(name, **params)
    nbytes = batch_bytes(params.get("exact", 0))
    one = nbytes(max(a, default=0), max(b, default=0))
    whole = nbytes(sum(a), sum(b))
    return one, whole, (one + whole) // 2


def test_abi_exports_the_batch_symbols(mp):
    from muchsalsa_amd import _lib
    header = open(os.path.join(ROOT, "include", "msgpu.h")).read()
    bound = {n for n, _, _ in _lib.SYMBOLS}
    for n in ("msgpu_map_batch_bytes", "msgpu_map_result_batches", "msgpu_map_result_budget"):
        assert hasattr(_lib.lib(), n) and n in bound and n + "(" in header, n
    assert C.sizeof(_lib.MapParams) == 48 and C.sizeof(_lib.MapChain) == 48 and C.sizeof(_lib.MapStats) == 424
    body = re.search(r"typedef struct msgpu_map_batch \{(.*?)\} msgpu_map_batch;", header, re.S).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    fields, size = [], 0
    for ctype, names in re.findall(r"(uint32_t|uint64_t)\s+([^;]+);", body):
        for n in names.split(","):
            fields.append(n.strip())
            size += 4 if ctype == "uint32_t" else 8
    assert fields == [f for f, _ in _lib.MapBatch._fields_] and size == C.sizeof(_lib.MapBatch) == 64
    assert "budget_mb" not in mp.DEFAULTS


def test_batch_bytes_is_a_bound_a_greedy_cut_can_use(mp):
    seed, exact = batch_bytes(0), batch_bytes(1)
    sizes = [0, 1, 2, 17, 1000, 230181, (1 << 31) - 1, 1 << 33]
    for f in (seed, exact):
        for a in sizes:
            assert f(a, 0) >= 105 * a  # the estimate it replaces
            for b in sizes:
                assert f(a + 1, b) > f(a, b) and f(a, b + 1) >= f(a, b)
    for a in sizes:
        for b in sizes:
            assert seed(a, b) == seed(a, 0)
            assert exact(a, b + 1) > exact(a, b) and exact(a, b) >= seed(a, b) + 2 * b
    for f in (seed, exact):
        for a1, b1 in ((0, 0), (1, 5), (1000, 3), (1 << 20, 1 << 30)):
            for a2, b2 in ((0, 0), (3, 0), (77, 1 << 20)):
                assert f(a1 + a2, b1 + b2) <= f(a1, b1) + f(a2, b2)
        # a constant plus a multiple of each argument
        assert f(20, 0) - f(10, 0) == f(30, 0) - f(20, 0) and f(5, 200) - f(5, 100) == f(9, 300) - f(9, 200)
    from muchsalsa_amd import _lib
    assert _lib.lib().msgpu_map_batch_bytes(None, 10, 10) == seed(10, 0)


def test_the_greedy_cut_on_hand_made_counts(mp):
    f = batch_bytes(0)
    ones = [10] * 8

    def cut(a, budget, b=None, nbytes=f):
        return greedy_cut(a, (b or ones)[:len(a)], nbytes, budget)

    assert cut([0, 0, 5, 3], f(5, 0)) == [(0, 3, 5, 30), (3, 1, 3, 10)]           # zeros at the front
    assert cut([5, 0, 0, 3], f(5, 0)) == [(0, 3, 5, 30), (3, 1, 3, 10)]           # in the middle: they join the running batch
    assert cut([5, 3, 0, 0], f(5, 0)) == [(0, 1, 5, 10), (1, 3, 3, 30)]           # at the end
    assert cut([0, 0, 0], f(0, 0)) == [(0, 3, 0, 30)]                             # all zeros
    assert cut([], f(0, 0)) == [] and cut([], 1) == []                            # no records, no batches
    assert cut([4], f(4, 0)) == [(0, 1, 4, 10)]                                   # one record
    assert cut([2, 6, 2], f(6, 0)) == [(0, 1, 2, 10), (1, 1, 6, 10), (2, 1, 2, 10)]  # a record exactly at the budget
    assert cut([2, 4, 2], f(6, 0)) == [(0, 2, 6, 20), (2, 1, 2, 10)]
    with pytest.raises(RecordTooLarge) as e:                                      # one byte under
        cut([2, 6, 2], f(6, 0) - 1)
    assert e.value.record == 1
    with pytest.raises(RecordTooLarge) as e:
        cut([0, 0, 0], f(0, 0) - 1)
    assert e.value.record == 0
    huge = f(1 << 40, 0)
    assert cut([(1 << 31) - 1, 1], huge) == [(0, 1, (1 << 31) - 1, 10), (1, 1, 1, 10)]  # fewer than 2^31 anchors per batch
    assert cut([(1 << 30), (1 << 30) - 1, 1], huge) == [(0, 2, (1 << 31) - 1, 20), (2, 1, 1, 10)]
    with pytest.raises(RecordTooLarge) as e:
        cut([3, 1 << 31], huge)
    assert e.value.record == 1
    g = batch_bytes(1)  # exact mode: a record without anchors still brings its bases
    assert cut([5, 0], g(5, 100), b=[100, 100], nbytes=g) == [(0, 1, 5, 100), (1, 1, 0, 100)]
    assert cut([5, 0], g(5, 200), b=[100, 100], nbytes=g) == [(0, 2, 5, 200)]
    assert cut([5, 0], f(5, 0), b=[100, 100]) == [(0, 2, 5, 200)]


def test_the_inputs_meet_the_conditions_of_the_gpu_tests(mp):
    """what keeps the GPU tests of the batches from passing on nothing: budget (i) cuts small and small_ava into at least three
    batches, some batch holds a record without anchors, small has both classes of groups and 16 query records"""
    for name, params in (("small", {}), ("small", dict(exact=1)), ("small_ava", dict(exact=1))):
        a, b = record_counts(name, **params)
        one, whole, half = budgets(name, **params)
        nbytes = batch_bytes(params.get("exact", 0))
        assert sum(a) == mapcases.expected(name, **params)["anchors"]
        assert one < half < whole
        assert len(greedy_cut(a, b, nbytes, one)) >= 3 and len(greedy_cut(a, b, nbytes, whole)) == 1
        assert 1 < len(greedy_cut(a, b, nbytes, half)) < len(greedy_cut(a, b, nbytes, one))
        if not params.get("exact"):  # (seed mode: the bases do not count, so the heaviest record is the one that fails)
            with pytest.raises(RecordTooLarge) as e:
                greedy_cut(a, b, nbytes, one - 1)
            assert e.value.record == a.index(max(a))
    a, b = record_counts("small")
    assert len(a) == 16
    sizes = [g[3] for g in mapcases.expected("small")["groups"]]
    assert min(sizes) <= 16 < max(sizes)
    a, b = record_counts("small_ava", exact=1)
    assert a[-1] == 0 and sum(a) > 0  # (ava: the last record meets no later one)
    a, b = record_counts("short_stretch")
    assert a[0] == 0 and a[1] > 0
    assert record_counts("empty_queries") == ((), ())
    assert len(record_counts("tiny", k=4)[0]) == 4


def test_command_line_takes_a_budget(mp, tmp_path, monkeypatch, capsys):
    p = [str(tmp_path / n) for n in ("t.fa", "q.fa", "out.paf")]
    seen = []

    def fake_run(*args, **kw):
        seen.append((args, kw))
        return {}

    monkeypatch.setattr(mp, "run", fake_run)
    for bad in (["--budget-mb", "0"], ["--budget-mb", "x"], ["--budget-mb"], ["--budget-mb", "-3"], ["--budget-mb", "nan"],
                ["--budget-mb", "inf"]):
        assert mp.main(p + bad) == 2, bad
        assert "--budget-mb" in capsys.readouterr().err
    assert seen == []
    assert mp.main(p + ["--budget-mb", "1.5", "-k", "16"]) == 0
    assert mp.main(p) == 0
    assert [kw["budget_mb"] for _, kw in seen] == [1.5, None] and seen[0][1]["k"] == 16 and seen[0][0] == tuple(p)
    assert "--budget-mb" in mp.__doc__.split("\n\n")[1]
