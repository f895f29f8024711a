"""The bootstrap's linear-transform diagonals built on the device (phantom_ltprep_*, csrc/ltprep.hip)
through the C-ABI, against their host twins (boot::stage / compose / lift_blocks and the giant-step
pre-rotation, the code EvalBootstrapSetup runs on the host).

Equality with the host is exact (numpy ==, so -0 equals +0) at every entry: every entry of a product
of butterfly stages has one non-zero path, so the host's sum is one right-nested product of complex
multiplies plus exact zeros, and the kernels form that product in the same nesting with contraction
off.  A numpy.longdouble restatement of stage / compose pins both to one rounding per product.

Rings: N = 2^12 (2048 slots) for the stage products and the finish, a 512 x 512 matrix for the dense
diagonals.
"""
import ctypes
import math

import numpy as np
import pytest

import phantom_amd as PA
from gpu_util import ptr, stream, torch

pytestmark = pytest.mark.gpu

LOG_N = 12
N = 1 << LOG_N
SLOTS = N // 2
CLD = np.clongdouble

_ctx = {}


def prep():
    if "p" not in _ctx:
        mods = PA.coeff_modulus_create(N, [60, 40, 40, 60])
        _ctx["p"] = PA.LtPrep(PA.Context(N, mods, 1))
    return _ctx["p"]


def dev_c128(a):
    return torch().from_numpy(np.ascontiguousarray(a, dtype=np.complex128)).cuda()


def host(t):
    torch().cuda.synchronize()
    return t.cpu().numpy()


def device_products(ns, inverse, stages, s=None, fill=0.0):
    """(offsets, complex128 [D, ns]) from phantom_ltprep_stage_products"""
    t = torch()
    off = PA.LtPrep.stage_offsets(ns, stages)
    cap = ns  # no product on ns slots has more diagonals
    out = t.full((cap * ns,), fill, dtype=t.complex128, device="cuda")
    scratch = t.full((cap * ns,), fill, dtype=t.complex128, device="cuda")
    prep().stage_products(ns, inverse, stages, ptr(out), ptr(scratch), cap, stream() if s is None else s)
    return off, host(out).reshape(cap, ns)[:len(off)].copy()


# ---- 1. stage products equal the host's ---------------------------------------------------------

def down(a, b):
    return list(range(a, b - 1, -1))


def up(a, b):
    return list(range(a, b + 1))


STAGE_CASES = [
    (2, [1]),                      # one stage = all stages = log2 ns: +h and -h are one key
    (4, [1]), (4, [2]), (4, [2, 1]), (4, [1, 2]),
    (512, [9]), (512, [1]), (512, [5]), (512, down(9, 1)), (512, up(1, 9)), (512, down(9, 5)), (512, up(1, 4)),
    (2048, [11]), (2048, down(11, 1)), (2048, up(1, 11)),
    (2048, down(11, 6)), (2048, down(5, 1)), (2048, up(1, 5)), (2048, up(6, 11)),  # the uneven split 6 + 5
]

_host_products = {}


def host_products(ns, inverse, stages):
    key = (ns, inverse, tuple(stages))
    if key not in _host_products:
        _host_products[key] = PA.LtPrep.stage_products_host(ns, inverse, stages)
    return _host_products[key]


def structural_offsets(ns, stages):
    keys = {0}
    for s in stages:
        h = 1 << (s - 1)
        keys = {(b + a) % ns for b in keys for a in (0, h % ns, (ns - h) % ns)}
    return sorted(keys)


@pytest.mark.parametrize("inverse", [False, True])
@pytest.mark.parametrize("ns,stages", STAGE_CASES)
def test_stage_products_equal_host(ns, stages, inverse):
    off_h, want = host_products(ns, inverse, stages)
    off_d, got = device_products(ns, inverse, stages)
    assert list(off_d) == list(off_h) == structural_offsets(ns, stages)
    assert got.shape == want.shape
    bad = np.argwhere(~((got.real == want.real) & (got.imag == want.imag)))
    assert len(bad) == 0, (len(bad), bad[:4], got[tuple(bad[0])], want[tuple(bad[0])])


# ---- 2. the same products against numpy.longdouble ------------------------------------------------

def stage_ld(ns, s, inverse):
    """boot::stage restated: {offset: longdouble diagonal}; the twiddles are the float64 roots the
    library uses (libm cos / sin of 2 pi e / M in double), carried into long double exactly"""
    m, h, M = 1 << s, 1 << (s - 1), 4 * ns
    pw, p5 = [], 1
    for _ in range(h):
        pw.append(p5)
        p5 = p5 * 5 % (4 * m)
    d0, dp, dm = (np.zeros(ns, dtype=CLD) for _ in range(3))
    for p in range(ns):
        j = p % m
        e = ((ns // m) * pw[j if j < h else j - h]) % M
        a = 2.0 * math.pi * float(e) / float(M)
        t = CLD(complex(math.cos(a), math.sin(a)))
        if j < h:
            d0[p] = 0.5 if inverse else 1.0
            dp[p] = 0.5 if inverse else t
        elif inverse:
            dm[p] = np.conj(t) * np.longdouble(0.5)
            d0[p] = -np.conj(t) * np.longdouble(0.5)
        else:
            d0[p] = -t
            dm[p] = 1.0
    d = {}
    for a, v in ((0, d0), (h % ns, dp), ((ns - h) % ns, dm)):
        d[a] = d[a] + v if a in d else v
    return d


def compose_ld(A, B, ns):
    out = {}
    for a, alpha in A.items():
        for b, beta in B.items():
            k = (a + b) % ns
            out[k] = out.get(k, np.zeros(ns, dtype=CLD)) + alpha * np.roll(beta, -a)
    return out


@pytest.mark.parametrize("inverse", [False, True])
@pytest.mark.parametrize("ns,stages", [(2, [1]), (4, [2, 1]), (512, down(9, 1)), (512, up(1, 4)), (2048, [11]),
                                       (2048, down(11, 6)), (2048, up(1, 5))])
def test_stage_products_within_one_rounding_per_product(ns, stages, inverse):
    T = {0: np.ones(ns, dtype=CLD)}
    for s in stages:
        T = compose_ld(stage_ld(ns, s, inverse), T, ns)
    off = sorted(T)
    want = np.stack([T[a] for a in off])
    off_h, h = host_products(ns, inverse, stages)
    off_d, d = device_products(ns, inverse, stages)
    assert list(off_h) == off and list(off_d) == off
    peak = float(np.max(np.abs(want)))
    bound = len(stages) * 2.0**-52 * peak
    e_dev = float(np.max(np.abs(d.astype(CLD) - want)))
    e_host = float(np.max(np.abs(h.astype(CLD) - want)))
    print(f"ns={ns} stages={stages} inverse={inverse}: e_dev {e_dev:.3e} e_host {e_host:.3e} bound {bound:.3e}")
    assert e_host <= bound
    assert e_dev <= bound


# ---- 3. the finish kernel equals the host twin ----------------------------------------------------

def device_finish(band, ns, band_offsets, stride, dim1, const, mask, s=None):
    """presence -> lifted offsets -> shape -> finish, as a device setup chains them"""
    t = torch()
    s = stream() if s is None else s
    dband = dev_c128(band)
    if ns < SLOTS:
        flags = t.full((2 * len(band_offsets),), 7, dtype=t.int32, device="cuda")
        PA.LtPrep.presence(ptr(dband), ns, band_offsets, ptr(flags), s, const=const)
        keys = PA.LtPrep.lifted_offsets(band_offsets, host(flags), ns, SLOTS)
    else:
        keys = np.asarray(band_offsets, dtype=np.int32)  # compose never drops a key
    shape = PA.LtPrep.shape(SLOTS, keys, stride, dim1)
    out = t.zeros(len(keys) * SLOTS, dtype=t.complex128, device="cuda")
    slots = PA.LtPrep.finish(ptr(dband), ns, SLOTS, band_offsets, keys, shape, ptr(out), s, const=const, mask=mask)
    return shape, keys, slots, host(out).reshape(len(keys), SLOTS)


# (ns, stages, inverse, mask): full packing, and the levels of sparse set-ups with the mask on
# the last CoeffToSlot level and the first SlotToCoeff level
FINISH_CASES = [
    (2048, down(11, 6), True, 0), (2048, up(6, 11), False, 0),
    (2, [1], True, 1), (2, [1], False, 2),
    (256, down(8, 5), True, 0), (256, down(4, 1), True, 1), (256, up(1, 4), False, 2), (256, up(5, 8), False, 0),
]


@pytest.mark.parametrize("dim1", [0, 4, 32])
@pytest.mark.parametrize("const", [None, 0.37, 0.37j])  # no constant, (c, 0), times_i: (0, c)
@pytest.mark.parametrize("ns,stages,inverse,mask", FINISH_CASES)
def test_finish_equals_host_twin(ns, stages, inverse, mask, const, dim1):
    off, band = host_products(ns, inverse, stages)
    stride = 1 << (min(stages) - 1)
    sh_h, keys_h, slots_h, want = PA.LtPrep.finish_host(band, ns, SLOTS, off, stride, dim1, const=const, mask=mask)
    sh_d, keys_d, slots_d, got = device_finish(band, ns, off, stride, dim1, const, mask)
    assert list(sh_d) == list(sh_h)
    assert sorted(keys_d) == sorted(keys_h)  # the presence flags give the host's key set
    # both list the present diagonals in slot order
    assert list(slots_d) == list(slots_h)
    center, D, g = int(sh_h[1]), int(sh_h[2]), int(sh_h[3])
    assert [int((u - center) * stride) % SLOTS for u in slots_h] == [int(k) for k in keys_h]
    if dim1:
        assert g == dim1
    assert got.shape == want.shape and len(want) > 0 and len(want) <= D
    bad = np.argwhere(~((got.real == want.real) & (got.imag == want.imag)))
    assert len(bad) == 0, (len(bad), bad[:4], got[tuple(bad[0])], want[tuple(bad[0])])


def test_finish_lift_drops_and_splits_offsets():
    """the sparse lift really exercises both halves: some offset a appears as a and as a - ns, and
    the masks change values (so the equality above is not comparing trivial data)"""
    ns, stages = 256, down(4, 1)
    off, band = host_products(ns, True, stages)
    _, keys, _, plain = PA.LtPrep.finish_host(band, ns, SLOTS, off, 1, 0, const=None, mask=0)
    _, keys_m, _, masked = PA.LtPrep.finish_host(band, ns, SLOTS, off, 1, 0, const=None, mask=1)
    assert list(keys) == list(keys_m)
    assert any(int(k) >= SLOTS - ns for k in keys) and any(0 < int(k) < ns for k in keys)
    assert not np.array_equal(plain, masked)


# ---- 4. dense diagonals ---------------------------------------------------------------------------

def test_dense_diagonals(rng):
    t = torch()
    slots, scale, k0 = 512, 0.75, 37
    A = rng.uniform(-1, 1, (slots, slots)) + 1j * rng.uniform(-1, 1, (slots, slots))
    p = np.arange(slots)
    A[p, (p + k0) % slots] = 0.0
    out = t.zeros(slots * slots, dtype=t.complex128, device="cuda")
    flags = t.full((slots,), 7, dtype=t.int32, device="cuda")
    PA.LtPrep.dense_diagonals(ptr(dev_c128(A)), slots, scale, ptr(out), ptr(flags), stream())
    got = host(out).reshape(slots, slots)
    want = np.stack([A[p, (p + k) % slots] * scale for k in range(slots)])
    assert np.array_equal(got, want)
    f = host(flags)
    assert f[k0] == 0 and np.all(np.delete(f, k0) == 1)


# ---- 5. bad arguments -----------------------------------------------------------------------------

def test_bad_arguments_enqueue_nothing():
    t = torch()
    lib = PA.load()
    P = prep()
    ns = 8
    sentinel = 123.0
    out = t.full((ns * ns,), sentinel, dtype=t.complex128, device="cuda")
    scratch = t.full((ns * ns,), sentinel, dtype=t.complex128, device="cuda")
    flags = t.full((2 * ns,), 7, dtype=t.int32, device="cuda")
    ok = np.array([1, 2], dtype=np.int32)
    cnt = ctypes.c_size_t(0)
    offs = np.zeros(16, dtype=np.int32)

    def refused(status):
        assert status == 1, status  # PHANTOM_ERR_INVALID_ARGUMENT
        assert lib.phantom_last_error().decode() != ""

    def products(ns_, stages, o=ptr(out), sc=ptr(scratch), ctx=P.ctx.handle):
        st = np.asarray(stages, dtype=np.int32)
        return lib.phantom_ltprep_stage_products(ctx, ns_, 0, st.ctypes.data if len(st) else None, len(st), o, sc, ns,
                                                 stream())

    refused(products(6, ok))            # ns not a power of two
    refused(products(ns, [0]))          # stages out of range
    refused(products(ns, [4]))
    refused(products(ns, []))
    refused(products(ns, ok, o=None))   # null pointers
    refused(products(ns, ok, sc=None))
    refused(products(ns, ok, ctx=None))
    refused(lib.phantom_ltprep_stage_products(P.ctx.handle, ns, 0, None, 2, ptr(out), ptr(scratch), ns, stream()))
    refused(lib.phantom_ltprep_stage_products(P.ctx.handle, ns, 0, ok.ctypes.data, 2, ptr(out), ptr(scratch), 1,
                                              stream()))  # capacity
    refused(lib.phantom_ltprep_stage_offsets(6, ok.ctypes.data, 2, offs.ctypes.data, 16, ctypes.byref(cnt)))
    refused(lib.phantom_ltprep_stage_offsets(ns, ok.ctypes.data, 2, None, 16, ctypes.byref(cnt)))
    refused(lib.phantom_ltprep_presence(None, ns, offs.ctypes.data, 1, 1.0, 0.0, 0, ptr(flags), stream()))
    refused(lib.phantom_ltprep_presence(ptr(out), 6, offs.ctypes.data, 1, 1.0, 0.0, 0, ptr(flags), stream()))
    refused(lib.phantom_ltprep_presence(ptr(out), ns, offs.ctypes.data, 1, 1.0, 0.0, 0, None, stream()))
    shape = np.array([1, 0, 1, 1, 1], dtype=np.int32)
    slots = np.zeros(4, dtype=np.int32)
    fin = lib.phantom_ltprep_finish
    refused(fin(None, ns, ns, offs.ctypes.data, 1, offs.ctypes.data, 1, shape.ctypes.data, 1.0, 0.0, 0, 0, ptr(scratch),
                slots.ctypes.data, stream()))
    refused(fin(ptr(out), 6, ns, offs.ctypes.data, 1, offs.ctypes.data, 1, shape.ctypes.data, 1.0, 0.0, 0, 0,
                ptr(scratch), slots.ctypes.data, stream()))
    refused(fin(ptr(out), ns, ns, offs.ctypes.data, 1, offs.ctypes.data, 1, shape.ctypes.data, 1.0, 0.0, 0, 3,
                ptr(scratch), slots.ctypes.data, stream()))  # unknown mask
    refused(fin(ptr(out), ns, ns, offs.ctypes.data, 1, offs.ctypes.data, 1, None, 1.0, 0.0, 0, 0, ptr(scratch),
                slots.ctypes.data, stream()))
    refused(lib.phantom_ltprep_dense_diagonals(ptr(out), 6, 1.0, ptr(scratch), ptr(flags), stream()))
    refused(lib.phantom_ltprep_dense_diagonals(None, ns, 1.0, ptr(scratch), ptr(flags), stream()))
    refused(lib.phantom_ltprep_dense_diagonals(ptr(out), ns, 1.0, ptr(scratch), None, stream()))
    # nothing was enqueued: every buffer still holds what it was filled with
    assert np.all(host(out) == sentinel) and np.all(host(scratch) == sentinel) and np.all(host(flags) == 7)


# ---- 6. stream independence ------------------------------------------------------------------------

def test_side_stream_gives_identical_bytes(rng):
    t = torch()
    ns, stages = 256, down(4, 1)
    off, band = host_products(ns, True, stages)
    slots = 512
    A = rng.uniform(-1, 1, (slots, slots)) + 1j * rng.uniform(-1, 1, (slots, slots))

    def run(s):
        _, prod = device_products(ns, True, stages, s=s, fill=float("nan"))
        _, _, _, fin = device_finish(band, ns, off, 1, 0, 0.37j, 1, s=s)
        out = t.zeros(slots * slots, dtype=t.complex128, device="cuda")
        flags = t.zeros(slots, dtype=t.int32, device="cuda")
        PA.LtPrep.dense_diagonals(ptr(dev_c128(A)), slots, 1.5, ptr(out), ptr(flags), s)
        return prod.tobytes(), fin.tobytes(), host(out).tobytes(), host(flags).tobytes()

    first = run(stream())
    side = t.cuda.Stream()
    t.cuda.synchronize()
    with t.cuda.stream(side):
        second = run(side.cuda_stream)
    assert first == second
