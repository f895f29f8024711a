"""examples/packboot_example.cpp `check pack`, `check boot` and `check relu`: the channel-packed tensor
bootstrap and the activation layers through the C++ façade at N = 2^12 on the chain of
bootstrapping_example (Q = {60, 29 x 59}, P = 10 x 60, scale 2^59, levelBudget {2, 2}), seeded keys
and encryptions.

Cases (width, slotstr, channels C, pack P): (8, 0, 3, 4); (8, 1, 8, 8), full packing at 2048 slots;
(8, 0, 5, 4), two groups of 4 + 1.  A group that is not full holds its channels at the tree indices
1 .. C (host/pack.h), a full one at 0 .. P - 1; the plain compositions follow that.

pack   DNN::Pack equals MultByMonomialInPlace + add and DNN::Unpack equals EvalRotateFused, add / sub,
       MultByMonomialInPlace word for word; DecTensor(Unpack(Pack(x))) / P is within 1e-6 of x (the bound
       of `bootstrapping_example ops` for a rotation and a monomial multiply at these parameters); the
       metadata is the input's.
boot   inputs uniform in [-4, -1] u [1, 4].  The shift: MultByIntegerInPlace(EvalBootstrap(ct,
       post_shift = g), 2^g) equals EvalBootstrap(ct) word for word (ct a packed ciphertext, so with
       complex slots).  BootStrap(pack = P) has the level, degree and scale() of EvalBootstrap at P ns
       slots.  Yardstick: E_slot, the maximum error of the existing EvalBootstrap on a fresh ciphertext
       of P ns random slots of that range in the same run, must stay below 1e-2 (else the comparison
       says nothing), and the packed path's maximum error over all channels and pixels is at most
       2 E_slot: the tree adds only key-switch noise, far below the bootstrap's error.
       BootStrap(pack = 1)'s error is printed beside them.
       Measured on MI355X (the same on every run: keys and encryptions are seeded), E_slot / packed /
       pack = 1:  (8, 0, 3, 4) 6.5e-5 / 1.1e-5 / 4.7e-5;  (8, 1, 8, 8) 1.1e-4 / 7.0e-5 / 6.3e-4;
       (8, 0, 5, 4) 2.3e-4 / 2.2e-5 / 6.1e-4.  The values near 6e-4 are the bootstrap's slot-0 events
       ("Where the precision goes": a constant offset of coefficient 0 when the raised
       ciphertext's overflow there is near 0; about a quarter of the bootstraps at N = 2^12), here on
       channel 1 of the second case and channel 4 of the third with pack = 1.  Channel 4 is the third
       case's second group alone, the same ciphertext on both paths: a group that is not full leaves
       tree index 0 free (host/pack.h), so the offset falls on a node that is never formed (with the
       channel at index 0 that group measured 6.2e-4).  A full group's channel 0 stays exposed to it.
relu   Sign(k), k = 0, 1, 2, Relu() and ReluDegTwo on 2 channels equal the per-channel
       EvalChebyshevSeries / EvalSquare + EvalAddAuto calls word for word.  ReluComposite on 3 channels
       of width 8 with pack = 1 and pack = 4 against the cleartext composition of the same three
       series (double precision): the pack = 1 path's maximum deviation must be below 0.35 (7 bits of
       bootstrap precision by an injection experiment: an absolute error of 2^-9, 2^-8, 2^-7 at the two
       inner bootstraps deviates the result by at most 0.08, 0.16, 0.34), the pack = 4 path's at most
       twice the pack = 1 path's, and both results carry the same metadata."""
import json
import os
import subprocess

import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BIN = os.path.join(ROOT, "phantom-fhe-boot_amd", "bin", "packboot_example")
CASES = [("w8_c3_p4", 8, 0, 3, 4, 1), ("w8s1_c8_p8", 8, 1, 8, 8, 1), ("w8_c5_p4", 8, 0, 5, 4, 2)]


def _run(mode):
    """the mode's rows by case; every case's test asserts its own row, `ok` included (the exit status
    is 0 iff every row is ok, so one case's miss does not hide the others)"""
    out = subprocess.run([BIN, "check", mode], capture_output=True, text=True, timeout=100)
    print(out.stdout)
    rows = [json.loads(l) for l in out.stdout.splitlines() if l.startswith("{")]
    by_case = {r["check"]: r for r in rows if "check" in r}
    all_ok = all(r["ok"] for r in by_case.values())
    assert out.returncode == (0 if all_ok else 1), (rows, out.stderr[-2000:])
    assert rows[-1] == {"done": "packboot_example check " + mode, "ok": all_ok}
    return by_case


@pytest.fixture(scope="module")
def pack_rows():
    return _run("pack")


@pytest.fixture(scope="module")
def boot_rows():
    return _run("boot")


@pytest.fixture(scope="module")
def relu_rows():
    return _run("relu")


@pytest.mark.parametrize("name,width,slotstr,C,P,groups", CASES)
def test_check_pack(pack_rows, name, width, slotstr, C, P, groups):
    r = pack_rows[name]
    print(r["max_error"])
    assert (r["log_n"], r["width"], r["slotstr"], r["channels"], r["pack"], r["groups"]) == (12, width, slotstr, C, P, groups)
    ns = (width << slotstr) ** 2
    assert r["stride_power"] == 4096 // (2 * P * ns)
    assert r["pack_words_equal"] and r["unpack_words_equal"]
    assert r["max_error"] < 1e-6
    assert r["metadata_equal"] and r["unpacked"] == r["input"], (r["unpacked"], r["input"])
    assert (r["input"]["chain_index"], r["input"]["degree"]) == (1, 1)
    assert r["ok"]


@pytest.mark.parametrize("name,width,slotstr,C,P,groups", CASES)
def test_check_boot(boot_rows, name, width, slotstr, C, P, groups):
    r = boot_rows[name]
    print(r["slot_bootstrap_max_error"], r["packed_max_error"], r["pack1_max_error"])
    ns = (width << slotstr) ** 2
    assert (r["log_n"], r["channels"], r["pack"], r["slots"], r["post_shift"]) == (12, C, P, P * ns, P.bit_length() - 1)
    assert r["post_shift"] <= r["correction"]
    assert r["shift_words_equal"]
    assert r["metadata_equal"] and r["packed"] == r["slot_bootstrap"], (r["packed"], r["slot_bootstrap"])
    assert r["packed"]["degree"] == 1 and r["packed"]["limbs"] > r["input"]["limbs"]
    assert r["slot_bootstrap_max_error"] < 1e-2
    assert r["packed_max_error"] <= 2 * r["slot_bootstrap_max_error"]
    assert r["ok"]


def test_check_relu_layers(relu_rows):
    r = relu_rows["layers"]
    assert (r["log_n"], r["channels"]) == (12, 2)
    assert r["sign_words_equal"] == [True, True, True]
    assert r["relu_words_equal"] and r["relu_deg_two_words_equal"] and r["sign_k3_refused"]
    assert r["ok"]


def test_check_relu_composite(relu_rows):
    r = relu_rows["relu_composite"]
    print(r["pack1_max_deviation"], r["packed_max_deviation"])
    assert (r["log_n"], r["width"], r["channels"], r["pack"]) == (12, 8, 3, 4)
    assert r["pack1_max_deviation"] < 0.35
    assert r["packed_max_deviation"] <= 2 * r["pack1_max_deviation"]
    assert r["metadata_equal"] and r["pack1"] == r["packed"], (r["pack1"], r["packed"])
    assert r["ok"]
