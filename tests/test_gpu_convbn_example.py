"""examples/convbn_example.cpp `check`: the fused layers (DNN::PrepareConvBN, Conv(plan) with the
plan's shift, DNN::ConvAdd) against the sequence they replace, Conv(PrepareConv) -> BatchNorm -> Add,
both through the C++ façade on the same ciphertexts and keys, at N = 2^12, scale 2^50, width 8,
3 -> 2 channels, K = 3; inputs, weights and batch-norm parameters from fixed seeds (var in [0.5, 2],
the rest in [-1, 1]).

The sequence is existing code, so it is the yardstick: its maximum error against the cleartext must
be below 1e-3 (the bound the other example tests use), the fused layer's at most twice that, measured
in the same run (the margin conv_plan_example gives a path that rounds differently; the fused path
has one rescale fewer).  The fused result stays at the input's chain index, the yardstick is one
lower, and a second convolution behind ConvAdd runs at chain index 2 where the sequence needs 3
(tests/test_gpu_conv_plan_example.py::test_conv_plan_example_chain)."""
import json
import os
import subprocess

import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BIN = os.path.join(ROOT, "phantom-fhe-boot_amd", "bin", "convbn_example")


@pytest.fixture(scope="module")
def rows():
    out = subprocess.run([BIN, "check"], capture_output=True, text=True, timeout=100)
    print(out.stdout)
    rows = [json.loads(l) for l in out.stdout.splitlines() if l.startswith("{")]
    assert rows and rows[-1].get("done") == "convbn_example check", (rows, out.returncode, out.stderr[-2000:])
    return {r["check"]: r for r in rows if "check" in r}


def _gates(r, chain, yard_chain):
    print(r["check"], "fused", r["fused_max_error"], "yardstick", r["yardstick_max_error"])
    assert (r["log_n"], r["width"], r["in_ch"], r["out_ch"], r["kernel"]) == (12, 8, 3, 2, 3)
    f, y = r["fused"], r["yardstick"]
    assert (f["chain_index"], f["degree"], f["size"], f["num_ch"]) == (chain, 2, 2, 2)
    assert abs(f["log2_scale"] - 100.0) < 1e-9  # ct.scale * scale_
    assert y["chain_index"] == yard_chain
    assert (f["width"], f["slotstr"]) == (y["width"], y["slotstr"])
    assert r["yardstick_max_error"] < 1e-3
    assert r["fused_max_error"] <= 2 * r["yardstick_max_error"]
    assert r["ok"]


def test_convbn(rows):
    """Conv(PrepareConvBN) against BatchNorm(Conv(PrepareConv))"""
    r = rows["convbn"]
    _gates(r, 1, 2)
    assert (r["slotstr"], r["stride"], r["fused"]["width"]) == (0, 1, 8)


def test_convadd(rows):
    """ConvAdd(x, planBN, r) against Add(BatchNorm(Conv(plan)), r)"""
    r = rows["convadd"]
    _gates(r, 1, 2)
    assert (r["slotstr"], r["stride"], r["fused"]["width"]) == (0, 1, 8)


def test_convadd_stride2(rows):
    """slotstr 1, stride 2, a residual of width 4 and slotstr 2"""
    r = rows["convadd_stride2"]
    _gates(r, 1, 2)
    assert (r["slotstr"], r["stride"]) == (1, 2)
    assert (r["fused"]["width"], r["fused"]["slotstr"]) == (4, 2)


def test_convadd_earlier_residual(rows):
    """accepted: the layer at chain index 2, the residual at 1 (it loses a limb on the way in)"""
    _gates(rows["convadd_earlier_residual"], 2, 3)


def test_resblock_chain(rows):
    """ConvAdd -> Conv(plan2) against the cleartext: the second plan sits at chain index 2"""
    r = rows["resblock_chain"]
    print(r["max_error"])
    assert (r["first_chain_index"], r["second_chain_index"]) == (1, 2)
    assert (r["first"]["chain_index"], r["first"]["degree"]) == (1, 2)
    assert (r["second"]["chain_index"], r["second"]["degree"], r["second"]["num_ch"]) == (2, 2, 2)
    assert r["max_error"] < 1e-3
    assert r["ok"]


def test_refused(rows):
    r = rows["refused"]
    assert r["residual_geometry"] and r["residual_later_chain_index"] and r["bn_vector_length"]
    assert r["residual_channel_count"]
    assert r["ok"]
