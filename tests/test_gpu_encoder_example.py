"""examples/encoder_example.cpp `check`: the device encoder's members of PhantomCKKSEncoder against
the host members on the same data, through the C++ façade.  Every check line must be ok, and the
device error at most 4 x the host error wherever both are reported."""
import json
import os
import subprocess

import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BIN = os.path.join(ROOT, "phantom-fhe-boot_amd", "bin", "encoder_example")
CHECKS = ["device_encode_device_decode", "host_encode_device_decode", "device_encode_host_decode",
          "embedding_coefficients", "encode_ext_device_vs_encode_ext", "sparse_device_vs_dense_tiling",
          "overflow_throws"]
RATIO_CHECKS = CHECKS[:4] + ["sparse_device_vs_dense_tiling"]


@pytest.mark.parametrize("log_n", [12, 13])
def test_encoder_example_check(log_n):
    out = subprocess.run([BIN, "check", str(log_n)], capture_output=True, text=True, timeout=100)
    rows = [json.loads(l) for l in out.stdout.splitlines() if l.startswith("{")]
    got = {r["check"]: r for r in rows if "check" in r}
    print(out.stdout)
    assert out.returncode == 0, (rows, out.stderr[-2000:])
    for name in CHECKS:
        assert got[name]["ok"] and got[name]["log_n"] == log_n, got[name]
    for name in RATIO_CHECKS:
        assert got[name]["e_host"] > 0 and got[name]["e_dev"] <= 4 * got[name]["e_host"], got[name]
    ext = got["encode_ext_device_vs_encode_ext"]
    assert ext["e_dev"] <= 1 + 4 * got["embedding_coefficients"]["e_host"] * 2.0**40, ext
    assert rows[-1] == {"done": "encoder_example check", "ok": True}
