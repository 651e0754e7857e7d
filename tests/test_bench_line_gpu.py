"""bench.py's plain line on the device: exactly --steps timed steps in one block, none of the --full measurements, and
--dump-outputs writing the last timed step's results -- the same results from two runs with the same arguments."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

ARGS = ["--steps", "5", "--warmup", "2", "--rows", "40000", "--spin-up-ms", "5"]


def _bench(extra):
    env = dict(os.environ)
    for k in ("RANK", "WORLD_SIZE", "LOCAL_RANK", "MASTER_ADDR", "MASTER_PORT"):
        env.pop(k, None)
    proc = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py")] + extra, env=env,
                          stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=600)
    assert proc.returncode == 0, proc.stderr.decode()[-3000:]
    lines = [l for l in proc.stdout.decode().splitlines() if l.startswith("{")]
    assert len(lines) == 1, proc.stdout.decode()
    return json.loads(lines[0])


@pytest.mark.gpu
def test_plain_line_times_the_given_steps_and_dumps_the_last_step(tmp_path):
    runs = []
    for tag in ("a", "b"):
        out = _bench(ARGS + ["--dump-outputs", str(tmp_path / tag)])
        assert out["full"] is False and out["steps"] == 5 and out["warmup"] == 2
        assert out["timed_blocks"]["n"] == 1 and out["timed_blocks"]["steps_per_block"] == 5
        assert out["ms_per_step"] > 0 and out["higher_is_better"] is True and out["dtype"] == "f32"
        # value = 0.04 1M-row mini-batch equivalents per step / the time of one step
        np.testing.assert_allclose(out["value"], 0.04 / (out["ms_per_step"] * 1e-3), rtol=1e-9)
        assert out["roofline"] is None and out["cpu_baseline"] is None and out["finish_us"] is None
        for key in ("value_same_batch", "value_via_plugin"):
            assert key not in out
        got = {n[:-4]: np.load(str(tmp_path / tag / n)) for n in sorted(os.listdir(str(tmp_path / tag)))}
        assert sorted(got) == ["elbo", "grad", "lam"]
        assert got["lam"].shape == got["grad"].shape == (2 * 256 + 2,) and got["elbo"].shape == (1,)
        assert all(a.dtype == np.float64 and np.isfinite(a).all() for a in got.values())
        np.testing.assert_allclose(got["elbo"][0], out["final_elbo"], rtol=1e-12)
        runs.append(got)
    for name in ("lam", "grad", "elbo"):
        a, b = runs[0][name], runs[1][name]
        np.testing.assert_allclose(a, b, rtol=1e-6, atol=1e-9 * np.abs(a).max())
