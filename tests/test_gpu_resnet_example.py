"""examples/resnet_example.cpp: the ResNet inference driver (host/resnet.h) and the .npy weight loader
(host/npy.h) at N = 2^12 on the chain of bootstrapping_example (Q = {60, 29 x 59}, P = 10 x 60, scale 2^59,
levelBudget {2, 2}), seeded keys and encryptions.

wiring     activation kDegTwo (x + x^2, no bootstrap), width 8, 2 input channels, stages {2, 4} with one
           block each, 3 classes: an identity block, a stride-2 block with its 1x1 projection (width 4,
           slotstr 1) and the head.  This file writes the weights and the image as .npy (f4 and f8 mixed)
           and computes the logits itself in float64 with numpy: exact zero-padded convolution, batch
           norm with eps 1e-5, x + x^2, the average and the fully connected layer.  `resnet_example run`
           on that directory, once per schedule:
             - layer by layer: the error against the cleartext logits is below 1e-3 of the largest
               |logit| (plain operations on this chain are good to about 1e-6 and a wiring mistake is
               O(1): a condition with margin, not a measurement);
             - fused: at most twice the layer-by-layer error (the fused layers add only the residual's
               integer-multiple rounding, host/dnn.h);
             - the fused result sits 1 + 2 x blocks = 5 chain indices before the layer-by-layer one, one
               per batch norm folded on the main path;
             - both traces equal the level plan step by step, and the plan is the one DESIGN.md §3
               writes out for this net.
           `resnet_example check wiring` on the same directory, in one process: rotation_indices()
           equals the union of AddRotationIndicesTo(8, 3, 0), (4, 3, 1) and AddAvgPoolRotationsTo(4, 1);
           kStreamed and kResident give the same words, the streamed schedule holding fewer plan bytes.
composite  kComposite on conv1 -> act -> one identity block -> head with 2 channels, width 8, seeded
           synthetic weights (He-scaled, damping 1.0, seed 0x2E5C), against the cleartext net with the
           same three sign series in double.  The fused path (pack 2, 128 slots) must deviate at most
           twice as much as the layer-by-layer pack = 1 path (64 slots), which must stay below a
           quarter of the cleartext logits' spread; one sign series must consume no more levels than
           the plan budgets for it.  The same two gates on a second net with a stride-2 block behind
           it (stages {2, 4}, damping 0.5, packs 2 and 4): there the projected skip sits one rescale
           past the main path after a bootstrap, and the fused schedule drops conv2's input to it.
           Measured on MI355X at N = 2^12 (the same on every run: keys and encryptions are seeded),
           layer by layer / fused / a quarter of the spread: 5.6e-5 / 8.9e-6 / 0.121 and, with the
           projecting block, 1.1e-4 / 6.4e-5 / 0.345; the first series used 5 of its 6 budgeted levels.
           The wiring net's errors: 1.1e-9 layer by layer and 8.5e-11 fused at a largest |logit| of 0.56.
           The condition holds at N = 2^12, so no other ring degree is used.
refuse     every std::invalid_argument of the driver: a width the stages halve below 1, a width that is
           no power of two, no stage, Infer before Prepare, a missing rotation key, weights of another
           spec, a missing projection, fc rows, inputs of another geometry, a chain too short for the
           polynomial net and for the composite one (on a 24-limb chain, refused by the plan alone with
           the pool untouched), a null bootstrapper, a missing bootstrap setup, missing bootstrap keys."""
import json
import os
import subprocess

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BIN = os.path.join(ROOT, "phantom-fhe-boot_amd", "bin", "resnet_example")
SPEC_FLAGS = ["--width", "8", "--in-ch", "2", "--stages", "2,4", "--blocks", "1", "--classes", "3", "--act", "degtwo"]


def _rows(args, timeout):
    out = subprocess.run([BIN, *args], capture_output=True, text=True, timeout=timeout)
    print(out.stdout)
    rows = [json.loads(l) for l in out.stdout.splitlines() if l.startswith("{")]
    assert rows, out.stderr[-2000:]
    return out.returncode, rows, out.stderr


def _check(args, mode, timeout=100):
    """the mode's rows by case; each test asserts its own row (the exit status is 0 iff every row is ok)"""
    code, rows, err = _rows(["check", mode, *args], timeout)
    cases = [r for r in rows if "check" in r]
    all_ok = all(r["ok"] for r in cases)
    assert code == (0 if all_ok else 1), (rows, err[-2000:])
    assert rows[-1] == {"done": "resnet_example check " + mode, "ok": all_ok}
    return cases


# ---- the wiring net in numpy -------------------------------------------------------------------------

def _conv(x, w, stride):
    """x (C, H, W), w (O, C, K, K): zero-padded cross-correlation, every stride-th pixel"""
    O, C, K, _ = w.shape
    p = K // 2
    xp = np.pad(x, ((0, 0), (p, p), (p, p)))
    H = x.shape[1] // stride
    y = np.zeros((O, H, H))
    for i in range(H):
        for j in range(H):
            patch = xp[:, i * stride:i * stride + K, j * stride:j * stride + K]
            y[:, i, j] = np.tensordot(w, patch, axes=([1, 2, 3], [0, 1, 2]))
    return y


def _bn(x, p):
    a = p["weight"] / np.sqrt(p["running_var"] + 1e-5)
    return a[:, None, None] * x + (p["bias"] - a * p["running_mean"])[:, None, None]


def _act(x):
    return x + x * x


@pytest.fixture(scope="module")
def wiring(tmp_path_factory):
    d = tmp_path_factory.mktemp("resnet_wiring")
    rng = np.random.default_rng(0x2E51)
    files = {}

    def conv(name, o, c, k, dtype):
        files[name] = (rng.standard_normal((o, c, k, k)) * 0.6 / np.sqrt(k * k * c)).astype(dtype)

    def bn(prefix, ch, dtype):
        files[prefix + "_weight"] = rng.uniform(0.8, 1.2, ch).astype(dtype)
        files[prefix + "_bias"] = rng.uniform(-0.1, 0.1, ch).astype(dtype)
        files[prefix + "_running_mean"] = rng.uniform(-0.1, 0.1, ch).astype(dtype)
        files[prefix + "_running_var"] = rng.uniform(0.5, 1.5, ch).astype(dtype)

    conv("conv1_weight", 2, 2, 3, np.float32)
    bn("bn1", 2, np.float32)
    conv("layer1_0_conv1_weight", 2, 2, 3, np.float64)
    bn("layer1_0_bn1", 2, np.float64)
    conv("layer1_0_conv2_weight", 2, 2, 3, np.float32)
    bn("layer1_0_bn2", 2, np.float32)
    conv("layer2_0_conv1_weight", 4, 2, 3, np.float32)
    bn("layer2_0_bn1", 4, np.float64)
    conv("layer2_0_conv2_weight", 4, 4, 3, np.float64)
    bn("layer2_0_bn2", 4, np.float32)
    conv("layer2_0_downsample_0_weight", 4, 2, 1, np.float32)
    bn("layer2_0_downsample_1", 4, np.float32)
    files["fc_weight"] = rng.uniform(-1, 1, (3, 4)).astype(np.float32)
    files["fc_bias"] = rng.uniform(-0.5, 0.5, 3)
    for name, a in files.items():
        np.save(d / (name + ".npy"), a)
    images = rng.uniform(-1, 1, (2, 2, 8, 8)).astype(np.float32)
    np.save(d / "images.npy", images)

    f = {k: v.astype(np.float64) for k, v in files.items()}
    bnp = lambda prefix: {k: f[prefix + "_" + k] for k in ("weight", "bias", "running_mean", "running_var")}
    logits = []
    for image in images.astype(np.float64):
        x = _act(_bn(_conv(image, f["conv1_weight"], 1), bnp("bn1")))
        y = _act(_bn(_conv(x, f["layer1_0_conv1_weight"], 1), bnp("layer1_0_bn1")))
        x = _act(_bn(_conv(y, f["layer1_0_conv2_weight"], 1), bnp("layer1_0_bn2")) + x)
        skip = _bn(_conv(x, f["layer2_0_downsample_0_weight"], 2), bnp("layer2_0_downsample_1"))
        y = _act(_bn(_conv(x, f["layer2_0_conv1_weight"], 2), bnp("layer2_0_bn1")))
        x = _act(_bn(_conv(y, f["layer2_0_conv2_weight"], 1), bnp("layer2_0_bn2")) + skip)
        logits.append(f["fc_weight"] @ x.mean(axis=(1, 2)) + f["fc_bias"])
    return d, logits


IMAGE = 1  # the second image of the file: LoadImage's index is exercised


@pytest.fixture(scope="module")
def run_rows(wiring):
    d, _ = wiring
    rows = {}
    for schedule in ("layers", "fused"):
        code, out, err = _rows(["run", "12", str(d), str(d / "images.npy"), str(IMAGE), *SPEC_FLAGS, "--schedule", schedule], 100)
        assert code == 0 and len(out) == 1, (out, err[-2000:])
        rows[schedule] = out[0]
    return rows


@pytest.fixture(scope="module")
def wiring_rows(wiring):
    d, _ = wiring
    return {r["check"]: r for r in _check([str(d), str(d / "images.npy")], "wiring")}


def _steps(trace):
    return [(s["name"], s["kind"], tuple(s["in"]), tuple(s["out"])) for s in trace]


def _error(row, want):
    return float(np.max(np.abs(np.array(row["logits"]) - want)))


def test_wiring_layer_by_layer_matches_cleartext(wiring, run_rows):
    want = wiring[1][IMAGE]
    r = run_rows["layers"]
    err = _error(r, want)
    print("layer-by-layer max error", err, "largest |logit|", np.max(np.abs(want)))
    assert (r["schedule"], r["activation"], r["log_n"]) == ("layers", "degtwo", 12)
    assert err < 1e-3 * np.max(np.abs(want))
    assert r["argmax"] == int(np.argmax(want))
    assert r["ok"]


def test_wiring_fused_within_twice_layer_by_layer(wiring, run_rows):
    want = wiring[1][IMAGE]
    e_layers, e_fused = _error(run_rows["layers"], want), _error(run_rows["fused"], want)
    print("fused max error", e_fused, "layer-by-layer", e_layers)
    assert e_fused <= 2 * e_layers
    assert run_rows["fused"]["ok"]


def test_wiring_fused_is_earlier_by_the_folded_batch_norms(run_rows):
    blocks = 2
    assert run_rows["layers"]["output_chain_index"] - run_rows["fused"]["output_chain_index"] == 1 + 2 * blocks


# DESIGN.md §3 "ResNet driver": (chain index, degree) in -> out, from an input at (1, 1)
FUSED_PLAN = [
    ("conv1", "conv", (1, 1), (1, 2)), ("act0", "act", (1, 2), (2, 2)),
    ("layer1_0_conv1", "conv", (2, 2), (3, 2)), ("layer1_0_act1", "act", (3, 2), (4, 2)),
    ("layer1_0_conv2", "conv", (4, 2), (5, 2)), ("layer1_0_act2", "act", (5, 2), (6, 2)),
    ("layer2_0_down", "conv", (6, 2), (7, 2)), ("layer2_0_conv1", "conv", (6, 2), (7, 2)),
    ("layer2_0_act1", "act", (7, 2), (8, 2)), ("layer2_0_conv2", "conv", (8, 2), (9, 2)),
    ("layer2_0_act2", "act", (9, 2), (10, 2)), ("head", "head", (10, 2), (11, 2)),
]
LAYERS_PLAN = [
    ("conv1", "conv", (1, 1), (1, 2)), ("conv1_bn", "bn", (1, 2), (2, 2)), ("act0", "act", (2, 2), (3, 2)),
    ("layer1_0_conv1", "conv", (3, 2), (4, 2)), ("layer1_0_conv1_bn", "bn", (4, 2), (5, 2)),
    ("layer1_0_act1", "act", (5, 2), (6, 2)),
    ("layer1_0_conv2", "conv", (6, 2), (7, 2)), ("layer1_0_conv2_bn", "bn", (7, 2), (8, 2)),
    ("layer1_0_conv2_add", "add", (8, 2), (8, 2)), ("layer1_0_act2", "act", (8, 2), (9, 2)),
    ("layer2_0_down", "conv", (9, 2), (10, 2)), ("layer2_0_down_bn", "bn", (10, 2), (11, 2)),
    ("layer2_0_conv1", "conv", (9, 2), (10, 2)), ("layer2_0_conv1_bn", "bn", (10, 2), (11, 2)),
    ("layer2_0_act1", "act", (11, 2), (12, 2)),
    ("layer2_0_conv2", "conv", (12, 2), (13, 2)), ("layer2_0_conv2_bn", "bn", (13, 2), (14, 2)),
    ("layer2_0_conv2_add", "add", (14, 2), (14, 2)), ("layer2_0_act2", "act", (14, 2), (15, 2)),
    ("head", "head", (15, 2), (16, 2)),
]


@pytest.mark.parametrize("schedule,plan", [("fused", FUSED_PLAN), ("layers", LAYERS_PLAN)])
def test_wiring_trace_matches_the_level_plan(run_rows, schedule, plan):
    r = run_rows[schedule]
    assert r["trace_matches_plan"]
    assert _steps(r["plan"]) == plan
    assert _steps(r["trace"]) == plan
    assert r["input_chain_index"] == 1 and r["output_chain_index"] == plan[-1][3][0]
    assert all(s["device_ms"] > 0 for s in r["trace"])


def test_wiring_in_process_schedules(wiring, wiring_rows):
    want = wiring[1][0]  # `check wiring` reads image 0
    a, b = wiring_rows["layer_by_layer"], wiring_rows["fused"]
    assert np.max(np.abs(np.array(a["clear_logits"]) - want)) < 1e-12 * max(1.0, np.max(np.abs(want)))  # the example's own cleartext net
    assert _error(a, want) < 1e-3 * np.max(np.abs(want)) and a["trace_matches_plan"] and a["ok"]
    assert _error(b, want) <= 2 * _error(a, want) and b["trace_matches_plan"] and b["ok"]
    assert b["layer_by_layer_chain_index"] - b["output_chain_index"] == b["fused_batch_norms"] == 5


def test_wiring_rotation_indices(wiring_rows, run_rows):
    r = wiring_rows["rotations"]
    assert r["rotation_indices"] == r["expected"] and r["ok"]
    assert run_rows["fused"]["rotation_indices"] == r["expected"] == run_rows["layers"]["rotation_indices"]
    # the 3x3 taps at row lengths 8 (both geometries: 8 and 4 x 2), then what the pooling adds
    taps = {(a * 8 + b) * step for step in (1, 2) for a in (-1, 0, 1) for b in (-1, 0, 1)}
    pool = {i * 2 for i in (1, 2, 3)} | {j * 4 * 4 for j in (1, 2, 3)}
    assert set(r["expected"]) == taps | pool


def test_wiring_streamed_and_resident_plans_give_the_same_words(wiring_rows):
    r = wiring_rows["residency"]
    assert r["words_equal"]
    assert r["resident_plan_bytes_peak"] == r["plan_bytes_total"] > r["streamed_plan_bytes_peak"] > 0
    assert r["ok"]


# ---- composite ---------------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def composite_rows():
    return {r["check"]: r for r in _check([], "composite", timeout=200)}


COMPOSITE = [("composite", [2], [64], [128], [20, 21]), ("composite_projection", [2, 4], [64], [128, 256], [20, 21])]


@pytest.mark.parametrize("name,packs,layer_slots,fused_slots,input_chain", COMPOSITE)
def test_composite_fused_against_layer_by_layer(composite_rows, name, packs, layer_slots, fused_slots, input_chain):
    r = composite_rows[name]
    print("layer-by-layer", r["layer_by_layer_max_deviation"], "fused", r["fused_max_deviation"], "spread", r["spread"])
    assert (r["log_n"], r["packs"], r["layer_by_layer_slot_counts"], r["fused_slot_counts"]) == (12, packs, layer_slots, fused_slots)
    assert r["max_preactivation"] < 10  # inside the sign series' interval after the 0.1
    assert r["layer_by_layer_max_deviation"] < 0.25 * r["spread"]
    assert r["fused_max_deviation"] <= 2 * r["layer_by_layer_max_deviation"]
    assert r["traces_match_plans"] == [True, True]
    assert r["input_chain_index"] == input_chain
    assert r["ok"]


def test_composite_projection_drops_the_layer_to_its_skip(composite_rows):
    """after a bootstrap (chain index 19, degree 1) the projected skip is (19, 2), one rescale past
    the main path's (19, 1): ConvAdd runs at chain index 20, where the layer-by-layer Add already is"""
    steps = {s["name"]: s for s in composite_rows["composite_projection"]["fused_trace"]}
    assert (steps["layer2_0_down"]["in"], steps["layer2_0_down"]["out"]) == ([19, 1], [19, 2])
    assert (steps["layer2_0_conv2"]["in"], steps["layer2_0_conv2"]["out"]) == ([19, 1], [20, 2])
    assert (steps["layer1_0_conv2"]["in"], steps["layer1_0_conv2"]["out"]) == ([19, 1], [19, 2])


def test_composite_series_within_the_plan_budget(composite_rows):
    r = composite_rows["series_budget"]
    print("levels used", r["levels_used"], "budget", r["budget"])
    assert r["budget"] == 6 and r["levels_used"] <= r["budget"]
    assert r["ok"]


# ---- refuse ------------------------------------------------------------------------------------------

REFUSALS = ["width halved below 1", "width not a power of two", "no stage", "infer before prepare", "missing rotation key",
            "weights of another spec", "missing projection", "fc rows differ from the classes", "input of another width",
            "input with other channels", "input at another packing", "chain too short for x + x^2", "null bootstrapper",
            "missing bootstrap setup", "missing bootstrap keys", "chain too short for the composite activation"]


@pytest.fixture(scope="module")
def refuse_rows():
    rows = _check([], "refuse")
    return {r.get("case", r["check"]): r for r in rows}


@pytest.mark.parametrize("case", REFUSALS)
def test_refusal(refuse_rows, case):
    r = refuse_rows[case]
    assert r["thrown"] and r["what"].startswith("ResNet: ") and r["ok"], r
    word = {"missing rotation key": "no key for rotation", "missing bootstrap setup": "no bootstrap setup",
            "missing bootstrap keys": "no keys for", "null bootstrapper": "needs a bootstrapper"}.get(case)
    if case.startswith("chain too short"):
        word = "too short"
    assert word is None or word in r["what"], r


def test_short_chain_is_refused_by_the_plan_alone(refuse_rows):
    assert refuse_rows["deep_plan"]["planned_last_chain_index"] >= refuse_rows["deep_plan"]["size_Q"]
    r = refuse_rows["short_chain_no_allocation"]
    assert r["size_Q"] == 24 and r["pool_unchanged"] and r["ok"]
