"""bench.py --dump-outputs without a GPU: what `dump_outputs` writes for the tables of a sweep -- whole when they fit, a seeded
sample of states that is the same in every run when they do not, and never more than the option allows."""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import bench  # noqa: E402


def _tables(n, T, rng):
    return [(p, rng.standard_normal(n), rng.integers(0, 500, size=n, dtype=np.int32)) for p in range(1, T + 1)]


def _sizes(d):
    return sum(os.path.getsize(os.path.join(d, f)) for f in os.listdir(d))


def test_small_tables_are_written_whole(tmp_path):
    tables = _tables(1000, 3, np.random.default_rng(1))
    bench.dump_outputs(str(tmp_path), tables, {"final_value": [-76.56]})
    assert sorted(os.listdir(tmp_path)) == sorted([f"{k}_p{p}.npy" for p in (1, 2, 3) for k in ("values", "policy")]
                                                  + ["final_value.npy"])
    for p, v, pol in tables:
        gv, gp = np.load(tmp_path / f"values_p{p}.npy"), np.load(tmp_path / f"policy_p{p}.npy")
        assert gv.dtype == np.float64 and np.array_equal(gv, v)
        assert gp.dtype == np.float32 and np.array_equal(gp, pol.astype(np.float32))
    assert np.load(tmp_path / "final_value.npy").tolist() == [-76.56]


def test_large_tables_are_a_fixed_sample_within_the_limit(tmp_path, monkeypatch):
    monkeypatch.setattr(bench, "DUMP_LIMIT_BYTES", 200_000)
    tables = _tables(20000, 4, np.random.default_rng(2))  # 960 kB whole
    a, b = tmp_path / "a", tmp_path / "b"
    bench.dump_outputs(str(a), tables)
    bench.dump_outputs(str(b), [(p, v.copy(), pol.copy()) for p, v, pol in tables])
    assert _sizes(a) <= 200_000 + 128 * len(os.listdir(a))  # (.npy headers)
    assert sorted(os.listdir(a)) == sorted(os.listdir(b))
    for p, v, pol in tables:
        idx = np.load(a / f"states_p{p}.npy")
        assert np.array_equal(idx, np.load(b / f"states_p{p}.npy")), "the sample does not depend on the run"
        assert len(idx) > 1000 and np.all(np.diff(idx) > 0) and idx[-1] < len(v)
        i = idx.astype(np.int64)
        assert np.array_equal(np.load(a / f"values_p{p}.npy"), v[i])
        assert np.array_equal(np.load(a / f"policy_p{p}.npy"), pol[i].astype(np.float32))
    # the periods draw different samples
    assert not np.array_equal(np.load(a / "states_p1.npy"), np.load(a / "states_p2.npy"))


def test_the_headline_grid_fits_the_option(tmp_path):
    """The default workload's tables (6 periods of 1e6 states: 72 MB whole) are cut below 64 MiB."""
    n, T = 1_000_000, 6
    tables = [(p, np.zeros(n), np.zeros(n, dtype=np.int32)) for p in range(1, T + 1)]
    bench.dump_outputs(str(tmp_path), tables)
    assert _sizes(tmp_path) <= 64 << 20
    assert len(os.listdir(tmp_path)) == 3 * T


def test_a_table_the_engine_did_not_keep_is_left_out(tmp_path):
    """Two ping-pong value tables: only V_1 and V_2 outlive the sweep; every policy does."""
    rng = np.random.default_rng(3)
    tables = [(p, rng.standard_normal(50) if p <= 2 else None, rng.integers(0, 9, size=50, dtype=np.int32)) for p in (1, 2, 3)]
    bench.dump_outputs(str(tmp_path), tables)
    assert sorted(os.listdir(tmp_path)) == ["policy_p1.npy", "policy_p2.npy", "policy_p3.npy", "values_p1.npy", "values_p2.npy"]
