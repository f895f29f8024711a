"""The hoisted convolution's host-side pieces (no GPU): the C-ABI names, the tap rotations, the
weight slot vectors' host twin against a numpy restatement, and the cleartext identity that pins
the tap / rotation convention (DNN::Conv, src/dnn.cu:99-141):

    sum over terms (k, a, b) of roll(input_k, -rot(a, b)) * slots(h, k, a, b)
        == the zero-padded "same" cross-correlation of the input with W[:, :, :, h]."""
import ctypes
import re

import numpy as np
import pytest

import phantom_amd as PA

NAMES = ["phantom_conv_rotations", "phantom_conv_weight_slots", "phantom_conv_weight_slots_host", "phantom_ext_mac",
         "phantom_conv2d"]


def np_rotations(width, slotstr, K):
    pw, lg = 1 << slotstr, width << slotstr
    return [((a - K // 2) * lg + (b - K // 2)) * pw for a in range(K) for b in range(K)]


def np_weight_slots(shape, W, first, count):
    """terms (h, k, a, b), b fastest -> complex128 [count, ns]"""
    width, slotstr, K, in_ch, out_ch = shape
    pw, lg = 1 << slotstr, width << slotstr
    out = np.zeros((count, lg * lg), dtype=np.complex128)
    for i in range(count):
        term = first + i
        b, term = term % K, term // K
        a, term = term % K, term // K
        k, h = term % in_ch, term // in_ch
        for r in range(width):
            for c in range(width):
                if 0 <= r + a - K // 2 < width and 0 <= c + b - K // 2 < width:
                    out[i, (r * lg + c) * pw] = W[a, b, k, h]
    return out


@pytest.mark.parametrize("name", NAMES)
def test_symbols_declared_and_exported(name):
    assert name in PA.declared_symbols()
    fn = getattr(PA.load(), name)  # AttributeError if the library does not export it
    txt = re.sub(r"/\*.*?\*/", "", open(PA.HEADER_PATH).read(), flags=re.S)
    params = re.search(r"\b%s\s*\(([^)]*)\)" % name, txt).group(1)
    assert fn.restype is ctypes.c_int and len(fn.argtypes) == len(params.split(",")), params


@pytest.mark.parametrize("width,slotstr,K", [(8, 0, 3), (4, 1, 3), (8, 0, 5), (2, 0, 1)])
def test_rotations(width, slotstr, K):
    got = PA.Conv.rotations(width, slotstr, K)
    assert got.tolist() == np_rotations(width, slotstr, K)
    assert got[K * K // 2] == 0  # the centre tap


def test_rotations_refused():
    out = np.zeros(32, dtype=np.int32)
    cnt = PA.sz(0)
    lib = PA.load()
    for width, slotstr, K, cap in [(8, 0, 2, 32), (2, 0, 3, 32), (6, 0, 3, 32), (0, 0, 1, 32), (8, 0, 3, 8)]:
        assert lib.phantom_conv_rotations(width, slotstr, K, out.ctypes.data, cap, ctypes.byref(cnt)) == 1
    assert lib.phantom_conv_rotations(8, 0, 3, None, 32, ctypes.byref(cnt)) == 1
    assert not out.any()


@pytest.mark.parametrize("shape", [(8, 0, 3, 3, 2), (4, 1, 3, 2, 2), (8, 0, 5, 2, 2), (2, 0, 1, 1, 3)])
def test_weight_slots_host(rng, shape):
    width, slotstr, K, in_ch, out_ch = shape
    W = rng.uniform(-1, 1, size=(K, K, in_ch, out_ch))
    terms = out_ch * in_ch * K * K
    want = np_weight_slots(shape, W, 0, terms)
    assert np.array_equal(PA.Conv.weight_slots_host(shape, W, 0, terms), want)
    # a run of terms from the middle
    first, count = terms // 3, terms - terms // 3 - 1
    assert np.array_equal(PA.Conv.weight_slots_host(shape, W, first, count), want[first:first + count])


def test_weight_slots_host_refused():
    lib = PA.load()
    W = np.ones((3, 3, 2, 2))
    out = np.full((36, 64, 2), 7.0)
    bad = [(8, 0, 2, 2, 2, 0, 1), (8, 0, 9, 2, 2, 0, 1), (6, 0, 3, 2, 2, 0, 1), (8, 0, 3, 0, 2, 0, 1),
           (8, 0, 3, 2, 0, 0, 1), (8, 0, 3, 2, 2, 30, 7), (8, 0, 3, 2, 2, 37, 0)]
    for width, slotstr, K, in_ch, out_ch, first, count in bad:
        assert lib.phantom_conv_weight_slots_host(width, slotstr, K, in_ch, out_ch, W.ctypes.data, first, count,
                                                  out.ctypes.data) == 1
    assert lib.phantom_conv_weight_slots_host(8, 0, 3, 2, 2, None, 0, 1, out.ctypes.data) == 1
    assert lib.phantom_conv_weight_slots_host(8, 0, 3, 2, 2, W.ctypes.data, 0, 1, None) == 1
    assert np.all(out == 7.0)


@pytest.mark.parametrize("shape", [(8, 0, 3, 3, 2), (4, 1, 3, 2, 2)])
def test_cleartext_identity(rng, shape):
    """rotations and slot vectors together compute the convolution (rotation by r: slot i takes the
    value of slot i + r, cyclically over the ns slots)"""
    width, slotstr, K, in_ch, out_ch = shape
    pw, lg = 1 << slotstr, width << slotstr
    ns = lg * lg
    x = rng.uniform(-1, 1, size=(in_ch, width, width))
    W = rng.uniform(-1, 1, size=(K, K, in_ch, out_ch))
    packed = np.zeros((in_ch, ns))
    garbage = rng.uniform(-1, 1, size=(in_ch, ns))  # what the gaps of a strided tensor may hold
    for r in range(width):
        for c in range(width):
            packed[:, (r * lg + c) * pw] = x[:, r, c]
    gap = np.ones(ns, dtype=bool)
    gap[[(r * lg + c) * pw for r in range(width) for c in range(width)]] = False
    packed[:, gap] = garbage[:, gap]
    rots = PA.Conv.rotations(width, slotstr, K)
    slots = PA.Conv.weight_slots_host(shape, W, 0, out_ch * in_ch * K * K).real
    pad = np.pad(x, ((0, 0), (K // 2, K // 2), (K // 2, K // 2)))
    for h in range(out_ch):
        got = np.zeros(ns)
        for k in range(in_ch):
            for tap in range(K * K):
                got += np.roll(packed[k], -int(rots[tap])) * slots[(h * in_ch + k) * K * K + tap]
        want = np.zeros((width, width))
        for k in range(in_ch):
            for a in range(K):
                for b in range(K):
                    want += W[a, b, k, h] * pad[k, a:a + width, b:b + width]
        grid = np.array([[got[(r * lg + c) * pw] for c in range(width)] for r in range(width)])
        assert np.allclose(grid, want, rtol=0, atol=1e-12)
        assert not got[gap].any()  # the masks clear every slot between the pixels
