"""bench.py's plain run: the headline line alone, and --dump-outputs of the last timed step.

A plain run prints the headline fields and none of the --full legs.  --dump-outputs writes the
[44][65536] batch the last timed step transformed in place as the low and high 32 bits of every
residue (float64, exact).  A step is a forward followed by an inverse NTT, so that batch must equal
the seeded input bit for bit."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_plain_run_headline_and_dumped_outputs(tmp_path):
    sys.path.insert(0, ROOT)
    import bench
    import phantom_amd as PA
    out = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", "3", "--warmup", "1",
                          "--dump-outputs", str(tmp_path)], capture_output=True, text=True, timeout=115)
    assert out.returncode == 0, out.stderr[-3000:]
    lines = [l for l in out.stdout.splitlines() if l.startswith("{")]
    assert len(lines) == 1, out.stdout[-2000:]
    line = json.loads(lines[0])
    assert line["steps"] == 3 and line["warmup"] == 1 and line["n_gpus"] == 1
    assert line["unit"] == "GB/s" and line["higher_is_better"] is True and line["dtype"] == "u64"
    assert line["ms_per_step"] > 0
    # value and ms_per_step are the same measurement: bytes of the 3 steps over their time
    assert line["value"] == pytest.approx(2 * bench.BYTES_PER_TRANSFORM / (line["ms_per_step"] * 1e-3) / 1e9, rel=1e-3)
    for leg in ("single_stream", "roofline", "c3", "c4", "c5", "cpu_baseline"):
        assert leg not in line, leg

    files = sorted(os.listdir(tmp_path))
    assert files == ["c2_last_step_hi32.npy", "c2_last_step_lo32.npy"]
    assert sum(os.path.getsize(os.path.join(tmp_path, f)) for f in files) <= 64 << 20
    hi, lo = (np.load(os.path.join(tmp_path, f)) for f in files)
    assert hi.dtype == lo.dtype == np.float64 and hi.shape == lo.shape == (bench.L, bench.N)
    got = (hi.astype(np.uint64) << np.uint64(32)) | lo.astype(np.uint64)
    mods = PA.coeff_modulus_create(bench.N, bench.C3_BITS)[:bench.L]
    rng = np.random.default_rng(0x5EED)
    want = np.stack([rng.integers(0, q, size=bench.N, dtype=np.uint64) for q in mods])
    assert np.array_equal(got, want)
