"""bench.py's plain run: the one result line a driver parses, and the outputs it dumps for comparing two builds."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.gpu
def test_bench_plain_line_and_dumped_outputs(tmp_path):
    """`bench.py --gpus 1 --steps 3 --warmup 1 --dump-outputs DIR`, twice: a short line with the headline fields only (a driver
    that keeps the tail of the output must get all of it), `--steps` timed steps, and the last step's solution in DIR — the planted
    support of its signal, bit-identical in both runs."""
    dumps = []
    for run in range(2):
        d = tmp_path / ("out%d" % run)
        cmd = [sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", "3", "--warmup", "1", "--dump-outputs", str(d)]
        r = subprocess.run(cmd, cwd=ROOT, stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, timeout=600)
        assert r.returncode == 0, r.stderr[-2000:]
        lines = [ln for ln in r.stdout.splitlines() if ln.startswith("{")]
        assert len(lines) == 1 and len(lines[0]) < 2000, r.stdout[-2000:]
        out = json.loads(lines[0])
        assert out["unit"] == "signals/s" and out["higher_is_better"] is True and out["dtype"] == "f32" and out["steps"] == 3
        assert out["value"] > 0 and abs(out["value"] * out["ms_per_step"] - 1e3) <= 1e-6 * 1e3
        assert out["recovered"]["support_exact"] == 3
        assert not {"roofline", "extras", "batched", "cpu_baseline"} & set(out)
        dumps.append({f: np.load(d / (f + ".npy")) for f in ("x", "iterations", "solution_error")})
    x = dumps[0]["x"]
    assert x.dtype == np.float32 and x.shape == (65536,)
    assert dumps[0]["iterations"].dtype == dumps[0]["solution_error"].dtype == np.float64
    # the last timed signal is seed 1235 + warmup + steps - 1 of bench.make_signal: its support needs no matrix
    sup = np.sort(np.random.default_rng(1235 + 1 + 3 - 1).choice(65536, 64, replace=False))
    assert np.array_equal(np.nonzero(x)[0], sup)
    for f in dumps[0]:
        assert np.array_equal(dumps[0][f], dumps[1][f]), f
