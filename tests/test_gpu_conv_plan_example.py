"""examples/conv_plan_example.cpp `check`: a prepared layer (DNN::PrepareConv, Conv(plan)) against the
existing DNN::Conv(weight), both through the C++ façade on the same ciphertexts and keys, at
N = 2^12, scale 2^50, width 8, 3 -> 2 channels, K = 3; a second case packs the tensor with slotstr 1
and takes stride 2.  Inputs and weights are uniform in [-1, 1] from a fixed seed.

DNN::Conv(weight) is existing code, so it is the yardstick: its maximum error against the cleartext
convolution must be below 1e-3 (the bound of ckks_example), the prepared layer's at most twice that
(the compact encoding rounds 2 ns coefficients where the full-size one rounds N), for the first
apply and for the same plan reused on a second encrypted input, and the two results' metadata must
be equal.  A `conv_plan_chain` line runs Conv(plan) -> BatchNorm -> Add -> Conv(plan prepared at the
lower level)."""
import json
import os
import subprocess

import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BIN = os.path.join(ROOT, "phantom-fhe-boot_amd", "bin", "conv_plan_example")


@pytest.fixture(scope="module")
def rows():
    out = subprocess.run([BIN, "check"], capture_output=True, text=True, timeout=100)
    print(out.stdout)
    rows = [json.loads(l) for l in out.stdout.splitlines() if l.startswith("{")]
    assert out.returncode == 0, (rows, out.stderr[-2000:])
    assert rows[-1] == {"done": "conv_plan_example check", "ok": True}
    return {r["check"]: r for r in rows if "check" in r}


@pytest.mark.parametrize("name,slotstr,stride", [("conv_plan", 0, 1), ("conv_plan_stride2", 1, 2)])
def test_conv_plan_example_check(rows, name, slotstr, stride):
    r = rows[name]
    print(r["hoisted_max_error"], r["plan_max_error"], r["reuse_hoisted_max_error"], r["reuse_plan_max_error"])
    assert (r["log_n"], r["width"], r["in_ch"], r["out_ch"], r["kernel"]) == (12, 8, 3, 2, 3)
    assert (r["slotstr"], r["stride"]) == (slotstr, stride)
    assert r["metadata_equal"] and r["hoisted"] == r["plan"], (r["hoisted"], r["plan"])
    h = r["plan"]
    assert (h["width"], h["slotstr"], h["num_ch"]) == (8 // stride, slotstr + (stride == 2), 2)
    assert (h["chain_index"], h["degree"], h["size"]) == (1, 2, 2)  # the input's level, degree 1 + 1
    assert abs(h["log2_scale"] - 100.0) < 1e-9  # ct.scale * scale_
    assert r["hoisted_max_error"] < 1e-3
    assert r["plan_max_error"] <= 2 * r["hoisted_max_error"]
    assert r["reuse_hoisted_max_error"] < 1e-3
    assert r["reuse_plan_max_error"] <= 2 * r["reuse_hoisted_max_error"]
    # 8 out_ch in_ch K^2 (Ql + P) 2 ns bytes at chain index 1: 5 + 2 limbs
    assert r["plan_bytes"] == 8 * 2 * 3 * 9 * 7 * 2 * (8 << slotstr) ** 2
    assert r["ok"]


def test_conv_plan_example_chain(rows):
    """Conv(plan) -> BatchNorm -> Add -> Conv(plan2) against the cleartext, within ckks_example's 1e-3:
    every step takes a degree-2 tensor and rescales it first, so the batch norm sits one level down
    and the second convolution, with its plan, two"""
    r = rows["conv_plan_chain"]
    print(r["max_error"])
    assert (r["first_chain_index"], r["second_chain_index"]) == (1, 3)
    assert (r["batchnorm"]["chain_index"], r["batchnorm"]["degree"]) == (2, 2)
    assert (r["second"]["chain_index"], r["second"]["degree"], r["second"]["num_ch"]) == (3, 2, 2)
    assert r["mismatched_plan_refused"]
    assert r["max_error"] < 1e-3
    assert r["ok"]
