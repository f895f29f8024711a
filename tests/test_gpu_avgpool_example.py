"""examples/avgpool_example.cpp `check`: DNN::AvgPoolFullCon (channels mixed first, the T outputs pooled
by hoisted rotate-and-sum launches) against the reference's order of the same layer (per input
channel the log2(width) doubling steps per direction with EvalRotateFused + EvalAddAuto, whole-row
steps; then EvalMultConst / EvalAddAuto / EvalAddConstInPlaceWrap), both through the C++ façade on the
same ciphertexts and keys, at N = 2^12, scale 2^50: width 8, slotstr 0, 3 -> 2 and width 4, slotstr 1,
3 -> 2.  Inputs uniform in [-1, 1], weights uniform in [-1, 1] / width^2, bias in [-1, 1], fixed seed.

The baseline is existing code, so it is the yardstick: its maximum error at pixel (0, 0) against the
cleartext sum_k W[u][k] sum_pixels x + b must be below 1e-3 (the bound of ckks_example and of the
convolution example; above it the comparison is vacuous), the hoisted layer's at most twice that,
the two decodes within the same 1e-3 of each other over all ns slots (both compute the same function
of every slot), the metadata equal to the baseline's and to the reference's rules (src/dnn.cu:447-449
and EvalMultConst: the input's level, degree + 1, scale x sf[level]), and the façade's channel mix
equal to the EvalMultConst / EvalAddAuto loop word for word."""
import json
import os
import subprocess

import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BIN = os.path.join(ROOT, "phantom-fhe-boot_amd", "bin", "avgpool_example")


@pytest.fixture(scope="module")
def rows():
    out = subprocess.run([BIN, "check"], capture_output=True, text=True, timeout=100)
    print(out.stdout)
    rows = [json.loads(l) for l in out.stdout.splitlines() if l.startswith("{")]
    assert out.returncode == 0, (rows, out.stderr[-2000:])
    assert rows[-1] == {"done": "avgpool_example check", "ok": True}
    return {r["check"]: r for r in rows if "check" in r}


@pytest.mark.parametrize("name,width,slotstr", [("avgpool", 8, 0), ("avgpool_slotstr1", 4, 1)])
def test_avgpool_example_check(rows, name, width, slotstr):
    r = rows[name]
    print(r["hoisted_max_error"], r["baseline_max_error"], r["slots_max_difference"])
    assert (r["log_n"], r["width"], r["slotstr"], r["t"], r["T"]) == (12, width, slotstr, 3, 2)
    assert r["metadata_equal"] and r["hoisted"] == r["baseline"], (r["hoisted"], r["baseline"])
    h, i = r["hoisted"], r["input"]
    assert (h["width"], h["slotstr"], h["num_ch"]) == (width, slotstr, 2)  # width_ and slotstr_ stay, num_ch_ = T
    assert (i["chain_index"], i["degree"], i["num_ch"]) == (1, 1, 3)
    assert (h["chain_index"], h["degree"], h["size"], h["ntt"]) == (1, 2, 2, True)  # the input's level, degree 1 + 1
    assert abs(i["log2_scale"] - 50.0) < 1e-9
    assert abs(r["log2_sf_level"] - 50.0) < 1e-3  # the level's scaling factor, next to the 2^50 scale
    assert abs(h["log2_scale"] - (i["log2_scale"] + r["log2_sf_level"])) < 2e-6  # ct.scale * sf[level] (6 digits printed)
    assert r["baseline_max_error"] < 1e-3
    assert r["hoisted_max_error"] <= 2 * r["baseline_max_error"]
    assert r["slots_max_difference"] < 1e-3
    assert r["mix_words_equal"]
    assert r["ok"]
