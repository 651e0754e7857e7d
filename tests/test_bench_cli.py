"""bench.py's options and output dump, host side only (no GPU): a plain run times exactly --steps steps once, the extra
measurements are behind --full, and --dump-outputs writes float32 / float64 .npy files within a fixed byte budget."""
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import bench  # noqa: E402


def test_plain_run_is_one_block_of_exactly_the_given_steps():
    args = bench.parse_args(["--gpus", "1", "--steps", "7", "--warmup", "3"])
    assert args.steps == 7 and args.warmup == 3
    assert args.min_timed_s == 0.0          # no repeated blocks unless asked for
    assert args.full is False and args.dump_outputs is None
    args = bench.parse_args(["--full", "--dump-outputs", "out"])
    assert args.full is True and args.dump_outputs == "out"
    with pytest.raises(SystemExit):
        bench.parse_args(["--steps", "0"])


def test_dump_writes_every_array_as_float32_or_float64(tmp_path):
    arrays = {"lam": np.arange(10, dtype=np.float64), "w": np.ones((3, 4), np.float32),
              "count": np.array([5], np.int64), "half": np.ones(6, np.float16)}
    names = bench.dump_outputs(arrays, str(tmp_path / "d"))
    assert sorted(names) == ["count.npy", "half.npy", "lam.npy", "w.npy"]
    got = {n[:-4]: np.load(str(tmp_path / "d" / n)) for n in names}
    assert got["lam"].dtype == np.float64 and got["count"].dtype == np.float64
    assert got["w"].dtype == np.float32 and got["half"].dtype == np.float32
    np.testing.assert_array_equal(got["lam"], arrays["lam"])
    np.testing.assert_array_equal(got["w"], arrays["w"])
    assert got["count"][0] == 5.0


def test_dump_past_the_budget_keeps_a_fixed_seeded_sample(tmp_path):
    big = np.random.RandomState(3).standard_normal(20_000).astype(np.float32)
    small = np.arange(4, dtype=np.float64)
    limit = 16_000
    a = bench.dump_outputs({"big": big, "small": small}, str(tmp_path / "a"), limit=limit)
    b = bench.dump_outputs({"big": big, "small": small}, str(tmp_path / "b"), limit=limit)
    assert sorted(a) == sorted(b) == ["big_sample.npy", "small.npy"]
    sa, sb = np.load(str(tmp_path / "a" / "big_sample.npy")), np.load(str(tmp_path / "b" / "big_sample.npy"))
    np.testing.assert_array_equal(sa, sb)                  # the same elements every time
    assert sa.dtype == np.float32 and 0 < sa.size < big.size
    assert np.isin(sa, big).all()
    total = sum(os.path.getsize(str(tmp_path / "a" / n)) - 128 for n in a)     # (128-byte .npy headers)
    assert total <= limit
    np.testing.assert_array_equal(np.load(str(tmp_path / "a" / "small.npy")), small)
    assert bench.DUMP_LIMIT_BYTES == 64 << 20
