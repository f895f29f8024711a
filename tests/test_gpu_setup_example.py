"""EvalBootstrapSetup on the device (FHECKKSRNS::UseDeviceSetup) against the host setup:
examples/setup_example.cpp `check` through the C++ façade, and a boot session through Python.

The diagonals both setups encode are equal (test_gpu_ltprep.py), so their plaintexts differ only by the
two encoders' rounding: at most 1 + 4 e_host scale per centred coefficient, the bound
test_gpu_encoder_example.py holds encode_ext_device to against encode_ext (e_host: the host embedding's
error against long double on the same values).  A bootstrap through the device setup must be as
precise as one through the host setup in the same run, less 0.05 bits: a +-1 coefficient at scale
~2^59 moves a slot by less than 2^-40 relative, far below what 0.05 bits of the average resolve.
"""
import json
import os
import subprocess

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BIN = os.path.join(ROOT, "phantom-fhe-boot_amd", "bin", "setup_example")
ONCE = ["option_default_off", "rotation_indices_equal", "find_rotation_indices_equal", "output_chain_equal",
        "dense_device_vs_host", "dense_device_pointer_equals_device_path", "bootstrap_precision"]
PER_LEVEL = ["level_shape_equal", "level_plaintexts_within_encoder_bound", "host_setup_bit_identical"]
MARGIN = 0.05


@pytest.mark.parametrize("args", [("12",), ("12", "256")], ids=["full", "sparse256"])
def test_setup_example_check(args):
    out = subprocess.run([BIN, "check", *args], capture_output=True, text=True, timeout=110)
    print(out.stdout)
    rows = [json.loads(l) for l in out.stdout.splitlines() if l.startswith("{")]
    assert out.returncode == 0, (rows, out.stderr[-2000:])
    checks = [r for r in rows if "check" in r]
    assert all(r["ok"] for r in checks), [r for r in checks if not r["ok"]]
    names = [r["check"] for r in checks]
    for name in ONCE:
        assert names.count(name) == 1, name
    assert names.count("level_count_equal") == 2
    for name in PER_LEVEL:  # levelBudget {2, 2}: two levels in each direction
        got = [r for r in checks if r["check"] == name]
        assert sorted((r["dir"], r["level"]) for r in got) == [("CoeffsToSlots", 0), ("CoeffsToSlots", 1),
                                                               ("SlotsToCoeffs", 0), ("SlotsToCoeffs", 1)], got
    for r in checks:
        if r["check"] == "level_plaintexts_within_encoder_bound":
            assert r["present"] > 0 and r["e_host"] > 0 and r["max_diff"] <= r["bound"], r
            print(f"{r['dir']} level {r['level']}: {r['differing']} of {r['coefficients']} coefficients differ, "
                  f"max {r['max_diff']} (bound {r['bound']})")
        if r["check"] == "host_setup_bit_identical":
            assert r["host_vs_host_differing"] == 0, r
        if r["check"] in PER_LEVEL:  # the fingerprints another build's run is compared by
            assert sorted(r["hash"]) == ["device", "host", "host2"], r
            assert all(len(h) == 16 and int(h, 16) >= 0 for h in r["hash"].values()), r
            assert r["hash"]["host"] == r["hash"]["host2"], r
    dense = [r for r in checks if r["check"] == "dense_device_vs_host"][0]
    assert sorted(dense["hash"]) == ["device", "device_pointer", "host"], dense
    assert dense["hash"]["device"] == dense["hash"]["device_pointer"], dense
    rot = [r for r in rows if r.get("hashes") == "rotation_indices"]
    assert len(rot) == 1 and len(rot[0]["hash"]) == 16, rot
    boot = [r for r in checks if r["check"] == "bootstrap_precision"][0]
    print(f"avg_bits host {boot['avg_bits_host']} device {boot['avg_bits_device']}, outputs bit-identical: "
          f"{boot['outputs_bit_identical']}")
    assert boot["avg_bits_host"] > 9.85, boot
    assert boot["avg_bits_device"] >= boot["avg_bits_host"] - MARGIN, boot
    assert rows[-1] == {"done": "setup_example check", "ok": True}


def test_session_device_setup_through_python():
    """One ciphertext, encrypted once, bootstrapped by a host-setup and a device-setup session made
    from the same seed (so the same keys), each decrypting its own output."""
    import torch
    import phantom_amd as PA
    sessions = {ds: PA.BootSession(bytes(range(32)), log_n=12, device_setup=ds) for ds in (False, True)}
    assert sessions[True].device_setup and not sessions[False].device_setup
    host_sess = sessions[False]
    vals = np.random.default_rng(0xD5).uniform(1.0, 5.0, size=(1, host_sess.slots))
    chain = 26
    sin, sout = host_sess.input_bytes(chain), host_sess.output_bytes()
    assert sessions[True].output_bytes() == sout
    dev_in = torch.empty((1, sin), dtype=torch.uint8, device="cuda")
    assert host_sess.encrypt(vals, chain, dev_in.data_ptr(), sin) == sin
    bits, raw = {}, {}
    for ds, sess in sessions.items():
        dev_out = torch.empty((1, sout), dtype=torch.uint8, device="cuda")
        sess.run(dev_in.data_ptr(), sin, 1, dev_out.data_ptr(), sout, 1)
        torch.cuda.synchronize()
        bits[ds] = PA.bit_precision(vals[0], sess.decrypt(dev_out[0].data_ptr(), sout))
        raw[ds] = dev_out.cpu().numpy().tobytes()
    # the device-setup session's own round trip: encrypt, bootstrap, decrypt (fresh encryption
    # randomness, so it is held to the project's floor, not compared with the host run)
    dev_sess = sessions[True]
    own_in = torch.empty((1, sin), dtype=torch.uint8, device="cuda")
    own_out = torch.empty((1, sout), dtype=torch.uint8, device="cuda")
    assert dev_sess.encrypt(vals, chain, own_in.data_ptr(), sin) == sin
    dev_sess.run(own_in.data_ptr(), sin, 1, own_out.data_ptr(), sout, 1)
    torch.cuda.synchronize()
    own_bits = PA.bit_precision(vals[0], dev_sess.decrypt(own_out[0].data_ptr(), sout))
    assert own_bits > 9.85, own_bits
    for sess in sessions.values():
        sess.close()
    print(f"avg_bits: host setup {bits[False]:.4f}, device setup {bits[True]:.4f}, "
          f"outputs bit-identical: {raw[False] == raw[True]}")
    assert bits[False] > 9.85, bits
    assert bits[True] >= bits[False] - MARGIN, bits
