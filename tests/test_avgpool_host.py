"""The hoisted average pooling + fully connected layer's host-side pieces (no GPU): the C-ABI names,
phantom_avgpool_rotations against a numpy statement of the layout, and a numpy model on slot vectors
of what the rotations compute (rotation by r: slot i takes the value of slot i + r, cyclically over
the ns slots):

  * the width - 1 rotations per direction, summed with the identity, put every pixel into slot 0;
  * they agree in every slot with the reference's log2(width) doubling steps per direction when
    the row steps are whole rows (Lg 2^slotstr 2^j);
  * the reference's own row amounts (width 2^slotstr 2^j, src/dnn.cu:334-338, :421) are whole rows
    only for slotstr = 0: at the shape it uses itself (width 8, slotstr 2) they pool two rows."""
import ctypes
import re

import numpy as np
import pytest

import phantom_amd as PA

NAMES = ["phantom_ct_mix", "phantom_rotate_sum_ext", "phantom_avgpool_rotations", "phantom_avgpool_fc"]
SHAPES = [(2, 0), (2, 1), (4, 0), (4, 1), (8, 0), (8, 2), (16, 1), (64, 0)]


def np_rotations(width, slotstr):
    """pixel (r, c) sits at slot (r Lg + c) pow: a column step is pow slots, a row step Lg pow"""
    pw, lg = 1 << slotstr, width << slotstr
    return [i * pw for i in range(1, width)] + [j * lg * pw for j in range(1, width)]


def rotations(width, slotstr, capacity=256):
    out = np.zeros(capacity, dtype=np.int32)
    cnt = PA.sz(0)
    PA.check(PA.load().phantom_avgpool_rotations(width, slotstr, out.ctypes.data, capacity, ctypes.byref(cnt)))
    return out[:cnt.value].tolist()


def packed(rng, width, slotstr):
    """a width x width image in ns slots, the gaps of a strided tensor holding garbage"""
    pw, lg = 1 << slotstr, width << slotstr
    x = rng.uniform(-1, 1, size=(width, width))
    v = rng.uniform(-1, 1, size=lg * lg)
    for r in range(width):
        for c in range(width):
            v[(r * lg + c) * pw] = x[r, c]
    return x, v


def rotate_sum(v, amounts):
    """the identity plus every rotation of v"""
    return v + sum(np.roll(v, -int(a)) for a in amounts)


def doubling(v, steps):
    for s in steps:
        v = v + np.roll(v, -int(s))
    return v


@pytest.mark.parametrize("name", NAMES)
def test_symbols_declared_and_exported(name):
    assert name in PA.declared_symbols()
    fn = getattr(PA.load(), name)  # AttributeError if the library does not export it
    txt = re.sub(r"/\*.*?\*/", "", open(PA.HEADER_PATH).read(), flags=re.S)
    params = re.search(r"\b%s\s*\(([^)]*)\)" % name, txt).group(1)
    assert fn.restype is ctypes.c_int and len(fn.argtypes) == len(params.split(",")), params


@pytest.mark.parametrize("width,slotstr", SHAPES)
def test_rotations(width, slotstr):
    got = rotations(width, slotstr)
    assert got == np_rotations(width, slotstr)
    assert len(got) == 2 * (width - 1) and len(set(got)) == len(got)


def test_rotations_refused():
    out = np.zeros(256, dtype=np.int32)
    cnt = PA.sz(0)
    lib = PA.load()
    for width, slotstr, cap in [(0, 0, 256), (1, 0, 256), (3, 0, 256), (6, 1, 256), (128, 0, 256), (8, 0, 13), (8, 40, 256)]:
        assert lib.phantom_avgpool_rotations(width, slotstr, out.ctypes.data, cap, ctypes.byref(cnt)) == 1
    assert lib.phantom_avgpool_rotations(8, 0, None, 256, ctypes.byref(cnt)) == 1
    assert lib.phantom_avgpool_rotations(8, 0, out.ctypes.data, 256, None) == 1
    assert not out.any()


@pytest.mark.parametrize("width,slotstr", [s for s in SHAPES if s[0] <= 16])
def test_rotations_pool_every_pixel(rng, width, slotstr):
    """columns then rows: slot 0 holds the sum of all pixels, and every slot equals the doubling steps"""
    pw, lg = 1 << slotstr, width << slotstr
    x, v = packed(rng, width, slotstr)
    amounts = rotations(width, slotstr)
    cols, rows = amounts[:width - 1], amounts[width - 1:]
    hoisted = rotate_sum(rotate_sum(v, cols), rows)
    assert abs(hoisted[0] - x.sum()) < 1e-12 * width * width
    log_l = width.bit_length() - 1
    steps = [pw << i for i in range(log_l)] + [(lg * pw) << j for j in range(log_l)]
    assert set(steps) <= set(amounts)  # the baseline's keys are among the layer's
    assert np.allclose(hoisted, doubling(v, steps), rtol=0, atol=1e-12 * width * width)
    # linearity: mixing the channels first and pooling the mix is pooling first and mixing after
    _, v2 = packed(rng, width, slotstr)
    a, b = 0.375, -1.25
    mixed_first = rotate_sum(rotate_sum(a * v + b * v2, cols), rows)
    pooled_first = a * hoisted + b * rotate_sum(rotate_sum(v2, cols), rows)
    assert np.allclose(mixed_first, pooled_first, rtol=0, atol=1e-12 * width * width)


def test_reference_row_amounts():
    """width 2^slotstr 2^j is a row step only for slotstr = 0"""
    rng = np.random.default_rng(0xA76)
    for width, slotstr in [(8, 0), (4, 0)]:
        pw, log_l = 1 << slotstr, width.bit_length() - 1
        ref_rows = [(pw << j) * width for j in range(log_l)]
        assert set(ref_rows) <= set(rotations(width, slotstr)[width - 1:])
    width, slotstr = 8, 2  # AddAvgPoolRotationsTo(vec, 8, 2), the reference's own call
    pw, lg, log_l = 1 << slotstr, width << slotstr, 3
    ref_rows = [(pw << j) * width for j in range(log_l)]
    assert ref_rows == [32, 64, 128] and lg * pw == 128  # rows are 128 slots apart
    x, v = packed(rng, width, slotstr)
    ref = doubling(v, [pw << i for i in range(log_l)] + ref_rows)
    amounts = rotations(width, slotstr)
    ours = rotate_sum(rotate_sum(v, amounts[:width - 1]), amounts[width - 1:])
    assert abs(ours[0] - x.sum()) < 1e-10
    assert abs(ref[0] - x.sum()) > 1e-3  # not the pool
    # what it holds instead: rows 0 and 1, and the slots a quarter and a half row along
    row = lambda r, off: sum(v[r * lg * pw + off + c * pw] for c in range(width))
    assert abs(ref[0] - sum(row(r, off) for r in (0, 1) for off in (0, 32, 64, 96))) < 1e-10
