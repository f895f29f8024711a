"""examples/encrypt_batch_example.cpp `check`: PhantomSecretKey::encrypt_symmetric_batch and
decrypt_decode_batch against encrypt_symmetric / decrypt per ciphertext, through the C++ façade, with
two for_testing keys of one seed.  Every ciphertext word, recorded seed and save_symmetric byte must be
equal; every check line must be ok and the last line is the `done` record."""
import json
import os
import subprocess

import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BIN = os.path.join(ROOT, "phantom-fhe-boot_amd", "bin", "encrypt_batch_example")
PER_CHAIN = ["ciphertext_words", "recorded_seeds", "metadata", "save_symmetric_bytes", "decrypt_decode_batch",
             "decrypt_batch"]
ONCE = ["decode_two_limbs", "sparse_ciphertext_words", "mixed_batch_throws"]


@pytest.mark.parametrize("log_n", [12, 13])
def test_encrypt_batch_example_check(log_n):
    out = subprocess.run([BIN, "check", str(log_n)], capture_output=True, text=True, timeout=100)
    rows = [json.loads(l) for l in out.stdout.splitlines() if l.startswith("{")]
    print(out.stdout)
    assert out.returncode == 0, (rows, out.stderr[-2000:])
    checks = [r for r in rows if "check" in r]
    for r in checks:
        assert r["ok"] and r["mismatches"] == 0 and r["log_n"] == log_n, r
    names = [r["check"] for r in checks]
    for name in PER_CHAIN:
        assert names.count(name) == 2, (name, names)  # chains 1 and 3
    for name in ONCE:
        assert names.count(name) == 1, (name, names)
    assert all(r["count"] > 32 for r in checks if r["check"] in PER_CHAIN)  # the batch crosses a chunk
    assert rows[-1] == {"done": "encrypt_batch_example check", "ok": True}
