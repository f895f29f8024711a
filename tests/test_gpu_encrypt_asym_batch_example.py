"""examples/encrypt_asym_batch_example.cpp `check`: PhantomPublicKey::encrypt_asymmetric_batch (and its
sparse and strided forms) against encode_device + encrypt_asymmetric per ciphertext, through the C++
façade, with two for_testing secret keys of one seed and their public keys.  Every ciphertext word and
the metadata (is_asymmetric, no seed) must be equal, save_symmetric of a batch output throws as for any
asymmetric ciphertext, decrypt_decode_batch stays within n (alpha (n + 1) + 1.5) / scale (the coefficient
bound of tests/test_encrypt_asym_reference.py plus half a unit of rounding, all n terms of a slot
aligned), and a refused call (chain index 0) followed by a good one still matches the loop.  Every check
line must be ok and the last line is the `done` record."""
import json
import os
import subprocess

import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BIN = os.path.join(ROOT, "phantom-fhe-boot_amd", "bin", "encrypt_asym_batch_example")
PER_CHAIN = ["ciphertext_words", "metadata", "save_symmetric_throws", "decrypt_decode_batch",
             "refused_call_restores_the_stream", "batch_to_words"]
ONCE = ["sparse_ciphertext_words", "ungenerated_key_throws"]
CROSSES_A_CHUNK = ["ciphertext_words", "metadata", "save_symmetric_throws", "decrypt_decode_batch"]


@pytest.mark.parametrize("log_n", [12, 13])
def test_encrypt_asym_batch_example_check(log_n):
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
    assert all(r["count"] > 32 for r in checks if r["check"] in CROSSES_A_CHUNK)  # the batch crosses a chunk
    assert rows[-1] == {"done": "encrypt_asym_batch_example check", "ok": True}
