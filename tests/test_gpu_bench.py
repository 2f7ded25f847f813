"""bench.py's plain run: the headline line alone, --steps as the number of timed steps, and
--dump-outputs (the last timed step's decoded columns, a fixed sample above bench.DUMP_ROWS rows)
checked against the synthetic input the frames were encoded from. One small run of the benchmark
in a child process; the --full legs are not run here."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

pytestmark = [pytest.mark.gpu, pytest.mark.timeout(120)]

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_plain_run_and_dump_outputs(tmp_path):
    import bench
    from netidx_amd import synth
    n = bench.DUMP_ROWS + 100_003  # above the sample threshold, no multiple of a tile
    out = tmp_path / "dump"
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", "4",
                        "--warmup", "1", "--records", str(n), "--dump-outputs", str(out)],
                       capture_output=True, text=True, timeout=100)
    assert r.returncode == 0, r.stderr[-2000:]
    lines = [ln for ln in r.stdout.splitlines() if ln.startswith("{")]
    assert len(lines) == 1
    line = json.loads(lines[0])
    assert line["steps"] == 4 and line["warmup"] == 1 and line["full"] is False
    assert line["unit"] == "M updates/s" and line["higher_is_better"] is True
    assert line["ms_per_step"] > 0 and line["value"] > 0
    # value and ms_per_step are the same wall clock: n records per step
    assert line["value"] == pytest.approx(n / (line["ms_per_step"] * 1e-3) / 1e6, rel=0.02)
    for k in ("roofline", "cpu_baseline", "extras", "same_frame", "per_call", "oracle_rows_checked"):
        assert k not in line, k
    got = {f: np.load(out / f"{f}.npy") for f in ("rows", "id", "value_hi32", "value_lo32")}
    assert all(a.dtype == np.float64 and a.shape == (bench.DUMP_ROWS,) for a in got.values())
    assert sum(a.nbytes for a in got.values()) <= 64 << 20
    rows = got["rows"].astype(np.int64)
    assert (np.diff(rows) > 0).all() and rows[0] >= 0 and rows[-1] < n
    ids, bits = synth.f64_columns(n, synth.SEED_F64)
    assert np.array_equal(got["id"], ids[rows].astype(np.float64))
    back = (got["value_hi32"].astype(np.uint64) << np.uint64(32)) | got["value_lo32"].astype(np.uint64)
    assert np.array_equal(back, bits[rows])
