"""examples/packboot_example.cpp `check tree`: the batched same-key rotations and the unpacking tree
built on them, through the C++ façade at N = 2^12 on the chain of bootstrapping_example
(Q = {60, 29 x 59}, P = 10 x 60), seeded keys and encryptions.

rotate   EvalRotateFusedBatch equals EvalRotateFused per ciphertext word for word, metadata included:
         counts 1 and 5 at 30 limbs (beta = 3), the chunk size + 1 at 12 limbs (beta = 2; two chunks),
         every second input with another scale, and 5 inputs once more with the context's unbiased
         moddown on.
tree     unpack_channels_batch equals unpack_channels per group word for word, and DNN::Unpack gives the
         same tensor through either path, for the cases (width, slotstr, channels C, pack P) of
         tests/test_gpu_packboot_example.py and (8, 0, 8, 4), two full groups whose nodes share every
         level's batch.
refusal  inputs at different chain indices, an input not in NTT form, one of three polynomials, a null
         entry and a missing key each throw std::invalid_argument; an empty span gives an empty vector;
         a comparison after them still holds."""
import json
import os
import subprocess

import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BIN = os.path.join(ROOT, "phantom-fhe-boot_amd", "bin", "packboot_example")
TREES = [("tree_w8_c3_p4", 8, 0, 3, 4, 1), ("tree_w8s1_c8_p8", 8, 1, 8, 8, 1), ("tree_w8_c5_p4", 8, 0, 5, 4, 2),
         ("tree_w8_c8_p4", 8, 0, 8, 4, 2)]
REFUSALS = ["different chain indices", "not NTT form", "three polynomials", "null entry", "missing key"]


@pytest.fixture(scope="module")
def rows():
    """every row of the run (the exit status is 0 iff every row is ok, so each test asserts its own)"""
    out = subprocess.run([BIN, "check", "tree"], capture_output=True, text=True, timeout=100)
    print(out.stdout)
    rows = [json.loads(l) for l in out.stdout.splitlines() if l.startswith("{")]
    checks = [r for r in rows if "check" in r]
    all_ok = all(r["ok"] for r in checks)
    assert out.returncode == (0 if all_ok else 1), (rows, out.stderr[-2000:])
    assert rows[-1] == {"done": "packboot_example check tree", "ok": all_ok}
    return checks


def _one(rows, name):
    found = [r for r in rows if r["check"] == name]
    assert len(found) == 1, (name, found)
    return found[0]


@pytest.mark.parametrize("name,count,limbs,unbiased", [("rotate_batch_1", 1, 30, False), ("rotate_batch_5", 5, 30, False),
                                                       ("rotate_batch_chunk_plus_1", None, 12, False),
                                                       ("rotate_batch_unbiased", 5, 12, True),
                                                       ("rotate_batch_after_refusals", 3, 12, False)])
def test_rotate_batch(rows, name, count, limbs, unbiased):
    r = _one(rows, name)
    assert r["log_n"] == 12 and r["limbs"] == limbs and r["unbiased_moddown"] is unbiased
    assert 1 <= r["chunk"] <= 64
    assert r["count"] == (r["chunk"] + 1 if count is None else count)
    assert r["rotate_words_equal"] and r["ok"]


@pytest.mark.parametrize("name,width,slotstr,C,P,groups", TREES)
def test_tree(rows, name, width, slotstr, C, P, groups):
    r = _one(rows, name)
    assert (r["log_n"], r["width"], r["slotstr"], r["channels"], r["pack"], r["groups"]) == (12, width, slotstr, C, P, groups)
    assert r["tree_words_equal"] and r["unpack_words_equal"] and r["ok"]


def test_refusals(rows):
    got = {r["case"]: r for r in rows if r["check"] == "refusal"}
    assert sorted(got) == sorted(REFUSALS)
    assert all(r["thrown"] and r["ok"] for r in got.values()), got
    assert _one(rows, "empty_span")["empty_result"]


def test_every_comparison_row_reports_equality(rows):
    for r in rows:
        for key, value in r.items():
            if key.endswith("_equal") or key == "thrown":
                assert value is True, r
