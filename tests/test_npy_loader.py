"""phantom-fhe-boot_amd/host/npy.cpp through npytest/npy_check.cpp, a host-compiler program with its own
main (no GPU, no HIP): the .npy reader and the weight-file helpers on top of it.

values    numpy writes f4 and f8 arrays of 1 to 4 dimensions, among them a (2, 3, 3, 3) conv weight and a
          version-2.0 file; npy_check prints the shape and the values as hex doubles, which must equal
          the array's exactly (an f4 value widened).  LoadWeight4D's (out, in, kH, kW) -> [kH][kW][in][out]
          is compared element by element, LoadWeight2D / 1D, LoadBN and LoadImage likewise.
refusals  hand-made files for every refusal of host/npy.h: wrong magic, another version, a header
          length past the end of the file, a dict without one of the three keys, another dtype or byte
          order, Fortran order, 0 or 5 dimensions, a dimension of 0, a shape product that overflows
          size_t, a truncated file and one with trailing bytes; the typed helpers on the wrong number of
          dimensions.  Each must exit with status 1 and print its reason with the file's name: no crash.
sanitized the same cases once more on a build of the same two sources with -fsanitize=address,undefined
          (what `make SAN=address,undefined` builds as bin/npy_check_address), compiled here into a
          temporary directory: a stand-alone program, nothing preloaded.  The statuses must be the
          same and stderr must hold no sanitizer report."""
import os
import shutil
import struct
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "phantom-fhe-boot_amd")
BIN = os.path.join(PKG, "bin", "npy_check")
SOURCES = [os.path.join(PKG, "npytest", "npy_check.cpp"), os.path.join(PKG, "host", "npy.cpp")]


def run(binary, *args):
    out = subprocess.run([binary, *map(str, args)], capture_output=True, text=True, timeout=60)
    return out.returncode, out.stdout, out.stderr


def parse(stdout):
    """{'shape': [..], 'values': [..], ..}: the first word of a line names it"""
    rows = {}
    for line in stdout.splitlines():
        key, *rest = line.split()
        rows[key] = [int(x) for x in rest] if key in ("shape", "item_bytes") else [float.fromhex(x) for x in rest]
    return rows


def header(descr="<f8", fortran=False, shape=(3,), version=(1, 0), text=None, pad=True):
    """the bytes of an .npy header, by hand"""
    if text is None:
        text = "{'descr': '%s', 'fortran_order': %s, 'shape': %s, }" % (descr, fortran, shape)
    body = text.encode("latin1")
    lenfmt = "<H" if version[0] == 1 else "<I"
    if pad:
        total = 6 + 2 + struct.calcsize(lenfmt) + len(body) + 1
        body += b" " * (-total % 64) + b"\n"
    return b"\x93NUMPY" + bytes(version) + struct.pack(lenfmt, len(body)) + body


# ---- the cases: written once per directory, shared by the plain and the sanitizer runs ----------------

def _arrays():
    rng = np.random.default_rng(0x2E5)
    return {
        "f8_1d": rng.standard_normal(5),
        "f4_1d": rng.standard_normal(7).astype(np.float32),
        "f8_2d": rng.standard_normal((3, 4)),
        "f4_3d": rng.standard_normal((2, 3, 5)).astype(np.float32),
        "f4_conv": rng.standard_normal((2, 3, 3, 3)).astype(np.float32),
        "f8_conv": rng.standard_normal((4, 2, 1, 1)),
        "f4_edge": np.array([0.0, -0.0, np.inf, -np.inf, 1e-45, 3.4028235e38, -1.5], dtype=np.float32),
        "f8_image": rng.standard_normal((2, 3, 4, 4)),
    }


REFUSALS = {
    # name: (bytes, a word its reason must contain)
    "magic": (b"\x93NUMPX" + header()[6:] + bytes(24), "magic"),
    "short": (b"\x93NUM", "magic"),
    "empty": (b"", "magic"),
    "version_3_0": (header(version=(3, 0)) + bytes(24), "version"),
    "version_1_1": (header(version=(1, 1)) + bytes(24), "version"),
    "header_past_end": (b"\x93NUMPY\x01\x00" + struct.pack("<H", 4000) + b"{'descr': '<f8'", "header length"),
    "header_past_end_v2": (b"\x93NUMPY\x02\x00" + struct.pack("<I", 0xFFFFFFF0) + b"{}", "header length"),
    "length_bytes_cut": (b"\x93NUMPY\x02\x00\x10", "header length"),
    "no_descr": (header(text="{'fortran_order': False, 'shape': (3,), }") + bytes(24), "lacks"),
    "no_order": (header(text="{'descr': '<f8', 'shape': (3,), }") + bytes(24), "lacks"),
    "no_shape": (header(text="{'descr': '<f8', 'fortran_order': False, }") + bytes(24), "lacks"),
    "dict_cut": (header(text="{'descr': '<f8', 'fortran_order': False, 'shape': (3", pad=False), "malformed"),
    "string_cut": (header(text="{'descr': '<f8", pad=False), "malformed"),
    "not_a_dict": (header(text="hello") + bytes(24), "malformed"),
    "big_endian": (header(descr=">f8") + bytes(24), "dtype"),
    "int32": (header(descr="<i4") + bytes(12), "dtype"),
    "f2": (header(descr="<f2") + bytes(6), "dtype"),
    "native_f8": (header(descr="|f8") + bytes(24), "dtype"),
    "structured": (header(text="{'descr': [('a', '<f8')], 'fortran_order': False, 'shape': (3,), }") + bytes(24), "dtype"),
    "fortran": (header(fortran=True, shape=(2, 2)) + bytes(32), "Fortran"),
    "zero_dims": (header(shape=()) + bytes(8), "dimensions"),
    "five_dims": (header(shape=(1, 1, 1, 1, 2)) + bytes(16), "dimensions"),
    "dimension_0": (header(shape=(3, 0)), "dimension is 0"),
    "product_overflow": (header(shape=(2 ** 40, 2 ** 40)) + bytes(64), "overflow"),
    "bytes_overflow": (header(shape=(2 ** 62,)) + bytes(64), "overflow"),
    "digits_overflow": (header(text="{'descr': '<f8', 'fortran_order': False, 'shape': (99999999999999999999999,), }") + bytes(8), "overflow"),
    "truncated": (header(shape=(3,)) + bytes(23), "truncated"),
    "no_data": (header(shape=(3,)), "truncated"),
    "trailing": (header(shape=(3,)) + bytes(25), "trailing"),
}


@pytest.fixture(scope="module")
def files(tmp_path_factory):
    d = tmp_path_factory.mktemp("npy")
    arrays = _arrays()
    for name, a in arrays.items():
        np.save(d / (name + ".npy"), a)
    # version 2.0, written through numpy's own writer for that version
    with open(d / "v2.npy", "wb") as f:
        np.lib.format.write_array(f, arrays["f8_2d"], version=(2, 0))
    arrays["v2"] = arrays["f8_2d"]
    for i, part in enumerate(("weight", "bias", "running_mean", "running_var")):
        np.save(d / ("bn1_%s.npy" % part), np.arange(4, dtype=np.float32) + 10 * i)
    for name, (data, _) in REFUSALS.items():
        (d / ("bad_%s.npy" % name)).write_bytes(data)
    return d, arrays


@pytest.fixture(scope="module")
def sanitized(tmp_path_factory):
    cxx = shutil.which("g++") or shutil.which("c++")
    assert cxx, "no host C++ compiler"
    out = str(tmp_path_factory.mktemp("npy_san") / "npy_check_address")
    subprocess.run([cxx, "-std=c++20", "-O1", "-g", "-fno-omit-frame-pointer", "-fsanitize=address,undefined",
                    "-fno-sanitize-recover=all", "-o", out, *SOURCES], check=True, timeout=300)
    return out


def _check_values(binary, d, arrays):
    for name, a in arrays.items():
        code, out, err = run(binary, "array", d / (name + ".npy"))
        assert code == 0, (name, out, err)
        rows = parse(out)
        assert rows["shape"] == list(a.shape), name
        assert rows["item_bytes"] == [a.dtype.itemsize], name
        want = a.astype(np.float64).ravel()
        got = np.array(rows["values"])
        assert got.shape == want.shape and np.array_equal(got.view(np.uint64), want.view(np.uint64)), name
        assert err == "", (name, err)


def _check_helpers(binary, d, arrays):
    for name in ("f4_conv", "f8_conv"):
        a = arrays[name].astype(np.float64)
        code, out, err = run(binary, "w4", d / (name + ".npy"))
        assert code == 0 and err == "", (out, err)
        rows = parse(out)
        O, I, H, W = a.shape
        assert rows["shape"] == [H, W, I, O]
        got = np.array(rows["values"]).reshape(H, W, I, O)
        for o in range(O):
            for i in range(I):
                for h in range(H):
                    for w in range(W):
                        assert got[h, w, i, o] == a[o, i, h, w], (name, o, i, h, w)
    code, out, err = run(binary, "w2", d / "f8_2d.npy")
    assert code == 0 and err == "" and parse(out)["shape"] == [3, 4]
    assert np.array_equal(np.array(parse(out)["values"]).reshape(3, 4), arrays["f8_2d"])
    code, out, err = run(binary, "w1", d / "f4_1d.npy")
    assert code == 0 and err == "" and np.array_equal(np.array(parse(out)["values"]), arrays["f4_1d"].astype(np.float64))
    code, out, err = run(binary, "bn", d, "bn1")
    assert code == 0 and err == "", (out, err)
    rows = parse(out)
    for i, key in enumerate(("weight", "bias", "mean", "var")):
        assert rows[key] == [10.0 * i + k for k in range(4)]
    img = arrays["f8_image"]
    for index in range(2):
        code, out, err = run(binary, "image", d / "f8_image.npy", index)
        assert code == 0 and err == "", (out, err)
        rows = parse(out)
        assert rows["shape"] == [4, 4, 3]
        assert np.array_equal(np.array(rows["values"]).reshape(4, 4, 3), img[index].transpose(1, 2, 0))


def _refused(binary, args, word):
    code, out, err = run(binary, *args)
    assert code == 1, (args, code, out, err[-2000:])
    assert out.startswith("refused: ") and word in out, (args, out)
    assert str(args[1]) in out, (args, out)  # the file is named
    assert err == "", (args, err[-2000:])


def _check_refusals(binary, d):
    for name, (_, word) in REFUSALS.items():
        _refused(binary, ("array", d / ("bad_%s.npy" % name)), word)
    _refused(binary, ("array", d / "does_not_exist.npy"), "cannot open")
    # the typed helpers on the wrong number of dimensions, and an image index past the end
    _refused(binary, ("w4", d / "f4_3d.npy"), "expected 4 dimensions")
    _refused(binary, ("w2", d / "f8_1d.npy"), "expected 2 dimensions")
    _refused(binary, ("w1", d / "f8_2d.npy"), "expected 1 dimensions")
    _refused(binary, ("image", d / "f4_3d.npy", 0), "expected 4 dimensions")
    _refused(binary, ("image", d / "f8_image.npy", 2), "out of range")
    code, out, err = run(binary, "bn", d, "bn2")
    assert code == 1 and out.startswith("refused: ") and "bn2_weight.npy" in out and err == ""


def test_values_exact(files):
    _check_values(BIN, *files)


def test_weight_helpers(files):
    _check_helpers(BIN, *files)


@pytest.mark.parametrize("name", sorted(REFUSALS))
def test_refusal(files, name):
    _refused(BIN, ("array", files[0] / ("bad_%s.npy" % name)), REFUSALS[name][1])


def test_helper_refusals(files):
    _check_refusals(BIN, files[0])


def test_all_cases_on_the_sanitizer_build(files, sanitized):
    d, arrays = files
    _check_values(sanitized, d, arrays)
    _check_helpers(sanitized, d, arrays)
    _check_refusals(sanitized, d)
