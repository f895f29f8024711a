"""examples/conv_example.cpp `check`: DNN::Conv (the hoisted layer) against the per-term sequence it
replaces (encode_sparse -> EvalRotateFused -> EvalMultAutoInplace -> EvalAddAutoInplace for every
output channel, input channel and tap), both through the C++ façade on the same ciphertexts and keys,
at N = 2^12, scale 2^50, width 8, 3 -> 2 channels, K = 3; a second case packs the tensor with
slotstr 1 and takes stride 2.  Inputs and weights are uniform in [-1, 1] from a fixed seed.

The baseline is existing code, so it is the yardstick: its maximum error against the cleartext
convolution must be below 1e-3 (the bound of ckks_example; otherwise the comparison is vacuous), the
hoisted layer's at most twice that (different random rounding; it performs fewer roundings, one
moddown per output instead of one per term), the two results' metadata must be equal, and
EncTensor -> DecTensor round-trips within the same 1e-3.  A `conv_chain` line runs two layers with
BatchNorm and Add between them (the members that chain convolutions)."""
import json
import os
import subprocess

import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BIN = os.path.join(ROOT, "phantom-fhe-boot_amd", "bin", "conv_example")


@pytest.fixture(scope="module")
def rows():
    out = subprocess.run([BIN, "check"], capture_output=True, text=True, timeout=100)
    print(out.stdout)
    rows = [json.loads(l) for l in out.stdout.splitlines() if l.startswith("{")]
    assert out.returncode == 0, (rows, out.stderr[-2000:])
    assert rows[-1] == {"done": "conv_example check", "ok": True}
    return {r["check"]: r for r in rows if "check" in r}


@pytest.mark.parametrize("name,slotstr,stride", [("conv", 0, 1), ("conv_stride2", 1, 2)])
def test_conv_example_check(rows, name, slotstr, stride):
    r = rows[name]
    print(r["hoisted_max_error"], r["baseline_max_error"], r["roundtrip_max_error"])
    assert (r["log_n"], r["width"], r["in_ch"], r["out_ch"], r["kernel"]) == (12, 8, 3, 2, 3)
    assert (r["slotstr"], r["stride"]) == (slotstr, stride)
    assert r["metadata_equal"] and r["hoisted"] == r["baseline"], (r["hoisted"], r["baseline"])
    h = r["hoisted"]
    assert (h["width"], h["slotstr"], h["num_ch"]) == (8 // stride, slotstr + (stride == 2), 2)
    assert (h["chain_index"], h["degree"], h["size"]) == (1, 2, 2)  # the input's level, degree 1 + 1
    assert abs(h["log2_scale"] - 100.0) < 1e-9  # ct.scale * scale_
    assert r["baseline_max_error"] < 1e-3
    assert r["hoisted_max_error"] <= 2 * r["baseline_max_error"]
    assert r["roundtrip_max_error"] < 1e-3
    assert r["ok"]


def test_conv_example_chain(rows):
    """Conv -> BatchNorm -> Add -> Conv against the cleartext, within ckks_example's 1e-3: every step
    takes a degree-2 tensor and rescales it first, so the batch norm sits one level down and the
    second convolution two"""
    r = rows["conv_chain"]
    print(r["max_error"])
    assert (r["batchnorm"]["chain_index"], r["batchnorm"]["degree"]) == (2, 2)
    assert (r["second"]["chain_index"], r["second"]["degree"], r["second"]["num_ch"]) == (3, 2, 2)
    assert r["max_error"] < 1e-3
    assert r["ok"]
