"""bench.py on a MI355X: a plain run prints the headline line and nothing that needs runs of its own (those come with
--full), and --dump-outputs writes the step's result."""
import json
import os
import subprocess
import sys

import pytest

from conftest import ROOT

pytestmark = pytest.mark.gpu

FULL_ONLY = ("roofline", "roofline_all_convolutions", "roofline_delta", "roofline_encode_tail", "kernel_ms_per_step",
             "cpu_baseline", "compression_ratio", "sharded_check", "host_to_host", "lossy_abs2", "decode", "sharded_path",
             "configs", "cfg5_sweep", "cfg4_sharded", "compression_ratio_trained", "host_pipeline", "tz_pa1")


def test_plain_run_prints_the_headline_only(tmp_path):
    out = tmp_path / "dump"
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", "2", "--warmup", "1",
                        "--dump-outputs", str(out)], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-4000:]
    lines = r.stdout.splitlines()
    assert len(lines) == 1, r.stdout[-2000:]
    d = json.loads(lines[0])
    assert d["metric"] == "frames/sec (predict+delta-encode), 512x512 seq" and d["unit"] == "frames/s"
    assert d["higher_is_better"] is True and d["dtype"] == "f32" and d["steps"] == 2 and d["warmup"] == 1
    assert d["value"] > 0 and d["ms_per_step"] > 0
    assert abs(d["value"] * d["ms_per_step"] * 1e-3 - d["config"]["frames_per_step"]) < 1e-6 * d["value"]
    assert not set(d) & set(FULL_ONLY), sorted(set(d) & set(FULL_ONLY))
    assert sorted(os.listdir(out)) == ["key.npy", "payload_frame_sum.npy", "payload_frame_sumsq.npy", "payload_sample.npy",
                                       "table.npy"]
