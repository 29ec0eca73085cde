"""bench.py --dump-outputs: the files dump_outputs writes (no GPU: the tables are made up here)."""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def _tables(n, seed):
    from muchsalsa_amd._lib import EDGE_DTYPE, EM_DTYPE, ORDER_DTYPE
    rng = np.random.default_rng(seed)
    out = {}
    for name, dt in (("edges", EDGE_DTYPE), ("ems", EM_DTYPE), ("orders", ORDER_DTYPE)):
        t = np.zeros(n, dtype=dt)
        t.view(np.uint8)[:] = rng.integers(0, 256, t.nbytes, dtype=np.uint8)
        for f in dt.names:
            if t[f].dtype.kind == "f":
                t[f] = rng.standard_normal(t[f].shape)  # (random bytes would give NaNs)
        out[name] = t
    out["ids"] = rng.integers(0, 1 << 20, 1000).astype("<u4")  # a short table: dumped whole
    return out


def test_dump_is_float64_sampled_alike_every_run_and_within_64_mb(tmp_path):
    import bench
    n = bench.DUMP_ROWS + 1234
    tables = _tables(n, 5)
    bench.dump_outputs(str(tmp_path / "a"), tables)
    bench.dump_outputs(str(tmp_path / "b"), tables)
    files = sorted(os.listdir(tmp_path / "a"))
    assert files == sorted(os.listdir(tmp_path / "b"))
    assert not any("pad" in f for f in files)
    total = 0
    for f in files:
        a, b = np.load(tmp_path / "a" / f), np.load(tmp_path / "b" / f)
        assert a.dtype == np.float64 and a.tobytes() == b.tobytes(), f
        total += os.path.getsize(tmp_path / "a" / f)
    assert total <= 64 << 20
    for name, t in tables.items():
        assert np.load(tmp_path / "a" / (name + "_count.npy")).tolist() == [len(t)]
        keep = np.load(tmp_path / "a" / (name + "_row.npy")).astype(np.int64)
        if len(t) > bench.DUMP_ROWS:
            assert len(keep) == bench.DUMP_ROWS and np.all(np.diff(keep) > 0) and keep[-1] < len(t)
        else:
            assert np.array_equal(keep, np.arange(len(t)))
        if t.dtype.names is None:
            assert np.array_equal(np.load(tmp_path / "a" / (name + ".npy")), t[keep].astype(np.float64))
            continue
        for f in t.dtype.names:
            if f != "pad":
                got = np.load(tmp_path / "a" / ("%s_%s.npy" % (name, f)))
                assert np.array_equal(got, t[f][keep].astype(np.float64)), (name, f)
