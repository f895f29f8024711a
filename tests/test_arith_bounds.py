"""The bound arguments the kernels' lazy arithmetic rests on, in exact Python-integer emulation at
the edges those arguments name (phantom-fhe-boot_amd/csrc/arith.h, farith.h; the split partial sums
of ckks.hip lt_bsgs_*, rns.hip ks_rotate_batch_full and bconv_fixed_kernel).  CPU only.

Every device function is restated step by step in wrapping 64-bit arithmetic (FP32 steps in
numpy.float32, FP64 steps in Python floats, which are IEEE doubles) and checked against `% q`, or
against the output range its comment states, at

  * the regime-edge primes of tests/edge_cases.py (30 bits, either side of 2^50 and 2^60, below 2^61),
  * every input bound the comment states, at the bound and one below it
    (ll, hh = 2^62 - 1 and mm = 2^63 - 1; v = k q - 1, k q, k q + 1; |y| = 7.75 q with |w| = q / 2),
  * a few hundred random points.

test_patterns_reach_the_bounds shows that the max / lowmax operand patterns of edge_cases.py drive
the kernels' partial sums to at least half of each stated bound, i.e. that the GPU edge tests
(tests/test_gpu_edges.py) exercise the limits and not the middle of the ranges.
tests/test_int_arith.py keeps its own primes and covers ct_bfly8 / gs_bfly4 / reduce8."""
import random

import numpy as np
import pytest

import edge_cases as E
from test_int_arith import M64, csub, csub_n, hi32, lo32, mulhi_approx

N = 4096
NAMES = dict(zip(E.EDGE_NAMES, E.edge_primes(N)))
P30, P50LO, P50HI, P60LO, P60HI, P61 = (NAMES[k] for k in E.EDGE_NAMES)
INT60 = [P50HI, (1 << 59) - 55, P60LO]  # q < 2^60: the 16q ranges, split_reduce / split_reduce2
INT61 = INT60 + [P60HI, P61]  # q < 2^61: the 8q ranges, split_reduce_exact
FP50 = [P30, (1 << 40) - 87, P50LO]  # q < 2^50: the FP64 path
M30 = E.M30


# ---- arith.h restated ----------------------------------------------------------------------

def mulhi(a, b):
    return (a * b) >> 64


def ratio(q):  # floor(2^128 / q) = {r0, r1}
    r = (1 << 128) // q
    return r & M64, r >> 64


def barrett_reduce_128(lo, hi, q, r0, r1):
    p0 = mulhi(lo, r0)
    p1, p2 = lo * r1, hi * r0
    mid = ((p1 & M64) + p0) & M64
    carry = int(mid < p0)
    mid2 = (mid + (p2 & M64)) & M64
    carry += int(mid2 < mid)
    quot = (hi * r1 + (p1 >> 64) + (p2 >> 64) + carry) & M64
    return csub((lo - quot * q) & M64, q)


def shoup_from_barrett(w, q, r0, r1, rounds=2):
    s = (w * r1 + mulhi(w, r0)) & M64
    low = ((w << 64) // q) - s  # how far the estimate is below the quotient
    for _ in range(rounds):
        p = (s * q) & ((1 << 128) - 1)
        plo, phi = p & M64, p >> 64
        rlo, rhi = (-plo) & M64, (w - phi - int(plo != 0)) & M64
        if rhi != 0 or rlo >= q:
            s = (s + 1) & M64
    return s, low


class SplitRed:
    def __init__(self, q):
        self.q = q
        self.r0, self.r1 = ratio(q)
        self.c30, self.c60 = (1 << 30) % q, (1 << 60) % q
        self.c30s = shoup_from_barrett(self.c30, q, self.r0, self.r1)[0]
        self.c60s = shoup_from_barrett(self.c60, q, self.r0, self.r1)[0]
        self.nq, self.nq2, self.nq4 = (-q) & M64, (-2 * q) & M64, (-4 * q) & M64


def split_reduce(ll, mm, hh, k):
    q, nq = k.q, k.nq
    a = (ll + mulhi_approx(ll, k.r1) * nq) & M64
    b = (mm * k.c30 + mulhi_approx(mm, k.c30s) * nq) & M64
    c = (hh * k.c60 + mulhi_approx(hh, k.c60s) * nq) & M64
    assert a < 4 * q and b < 4 * q and c < 4 * q
    s = a + b + c
    assert s < 12 * q and s < 1 << 64
    s = (s + mulhi_approx(s, k.r1) * nq) & M64
    assert s < 4 * q
    s = csub_n(s, q << 1, k.nq2)
    return csub_n(s, q, nq)


def split_reduce2(ll, mm, hh, k, drop_4q=False):
    q, nq = k.q, k.nq
    L = (ll + ((mm & M30) << 30)) & M64
    H = (hh + (mm >> 30)) & M64
    assert L < 1 << 63 and H < 1 << 63
    a = (L + mulhi_approx(L, k.r1) * nq) & M64
    b = (H * k.c60 + mulhi_approx(H, k.c60s) * nq) & M64
    s = a + b
    assert a < 4 * q and b < 4 * q and s < 1 << 63
    if not drop_4q:
        s = csub_n(s, q << 2, k.nq4)
    s = csub_n(s, q << 1, k.nq2)
    return csub_n(s, q, nq)


def split_reduce_exact(ll, mm, hh, k):
    q = k.q
    a = (ll - mulhi(ll, k.r1) * q) & M64
    b = (mm * k.c30 - mulhi(mm, k.c30s) * q) & M64
    c = (hh * k.c60 - mulhi(hh, k.c60s) * q) & M64
    assert a < 2 * q and b < 2 * q and c < 2 * q
    s = a + b + c
    assert s < 6 * q and s < 1 << 64
    return csub((s - mulhi(s, k.r1) * q) & M64, q)


def mul_shoup_lazy4(a, w, ws, q):
    return (a * w + mulhi_approx(a, ws) * ((-q) & M64)) & M64


def ct_bfly_nored(x, y, w, ws, q):
    t = mul_shoup_lazy4(y, w, ws, q)
    return x + t, x + (q << 2) - t, t  # unwrapped: the caller checks they fit 64 bits


def ct_bfly_c8(x, y, w, ws, q):
    q8 = q << 3
    t = mul_shoup_lazy4(y, w, ws, q)
    u = csub_n(x, q8, (-q8) & M64)
    return u + t, u + (q << 2) - t, t


def gs_bfly8(x, y, w, ws, q, red):
    q8 = q << 3
    d = x + q8 - y
    s = x + y
    assert d < 1 << 64 and s < 1 << 64
    return (csub_n(s, q8, (-q8) & M64) if red else s), mul_shoup_lazy4(d, w, ws, q)


def reduce16(v, q):
    for sh in (3, 2, 1, 0):
        v = csub_n(v, q << sh, (-(q << sh)) & M64)
    return v


def reduce16_est(v, q, margin=0.25):
    """FP32 steps in numpy.float32: hf * rq and the - 1/4 are exact in a double, so one rounding to
    float32 is the fused multiply-add; rq as the kernel forms it (ntt_impl.h: float(2^32 / double(q)))"""
    rq = np.float32(4294967296.0 / float(q))
    hf = np.float32(hi32(v))  # v_cvt_f32_u32: round to nearest even
    est = np.float32(float(hf) * float(rq) - margin)
    k = int(max(est, np.float32(0.0)))
    nq = (-q) & M64
    r = (k * lo32(nq) + v) & M64
    rh = (hi32(r) + ((k * hi32(nq)) & 0xFFFFFFFF)) & 0xFFFFFFFF
    return csub_n((rh << 32) | lo32(r), q, nq), k


# ---- farith.h restated (doubles holding exact integers; Python floats are IEEE doubles) -------

def fmodmul(y, w, q):
    """integers in, integer out; asserts every step the comment calls exact is exact"""
    qinv = 1.0 / float(q)
    h = float(y) * float(w)  # fl(y w)
    l = y * w - int(h)  # fma(y, w, -h): the rounding error of the product
    assert float(l) == l and abs(l) < 1 << 53
    k = round(h * qinv)  # rint: ties to even, as Python's round
    r = int(h) - k * q  # fma(-k, q, h)
    assert abs(r) < 1 << 53
    t = r + l
    assert abs(t) < 1 << 53
    return t


def freduce(v, q):
    k = round(float(v) * (1.0 / float(q)))
    r = v - k * q
    assert abs(r) < 1 << 53
    return r


def f64_to_canonical(v, q):
    r = freduce(v, q)
    if r < 0:
        r += q
    assert 0 <= r < 1 << 52  # the 2^52 magic add holds r in the mantissa
    bits = np.float64(float(r) + 4503599627370496.0).view(np.uint64)
    return int(bits) & 0x000FFFFFFFFFFFFF


# ---- the checks ------------------------------------------------------------------------------

def _around(q, kmax, top):
    """k q - 1, k q, k q + 1 for k = 0 .. kmax, inside [0, top)"""
    return sorted({v for k in range(kmax + 1) for v in (k * q - 1, k * q, k * q + 1) if 0 <= v < top})


def _rand_below(rng, top, count):
    return [rng.randrange(top) for _ in range(count)]


@pytest.mark.parametrize("q", INT61 + FP50)
def test_shoup_from_barrett(q):
    """the estimate is at most 2 low, and two correction rounds make it floor(w 2^64 / q)"""
    rng = random.Random(q)
    r0, r1 = ratio(q)
    ws = [0, 1, 2, q - 1, q - 2, (q - 1) // 2, (q + 1) // 2, (1 << 30) % q, (1 << 60) % q, E.lowmax(q)]
    ws += [(q * k >> 6) for k in range(1, 64)] + [(q * k >> 6) + 1 for k in range(1, 63)]
    worst = 0
    for w in ws + _rand_below(rng, q, 600):
        s, low = shoup_from_barrett(w, q, r0, r1)
        assert 0 <= low <= 2, (q, w, low)
        assert s == (w << 64) // q, (q, w)
        worst = max(worst, low)
    assert worst >= 1 or q < 1 << 50  # the correction is exercised (w / 2^64 is negligible for small q)


@pytest.mark.parametrize("q", INT61 + FP50)
def test_barrett_reduce_128(q):
    rng = random.Random(q + 1)
    r0, r1 = ratio(q)
    top = 1 << 128
    xs = [0, 1, top - 1, top - 2, q * q - 1, (q - 1) ** 2, 32 * (q - 1) ** 2, 64 * (q - 1) ** 2 - 1]
    xs += [(top // q) * q + d for d in (-1, 0, 1) if (top // q) * q + d < top]
    xs += _around(q, 20, top) + [k * q * q + d for k in (1, 15, 16, 31, 32) for d in (-1, 0, 1)]
    for x in xs + _rand_below(rng, top, 400) + _rand_below(rng, 32 * q * q, 200):
        assert barrett_reduce_128(x & M64, x >> 64, q, r0, r1) == x % q, (q, x)


def _split_points(rng, count):
    """(ll, mm, hh) at the stated input bounds (ll, hh < 2^62, mm < 2^63), one below them, and random"""
    b62, b63 = (1 << 62) - 1, (1 << 63) - 1
    pts = [(l, m, h) for l in (0, 1, b62 - 1, b62) for m in (0, b63 - 1, b63, ((1 << 33) - 1) << 30, M30)
           for h in (0, 1, b62 - 1, b62)]
    return pts + [(rng.randrange(1 << 62), rng.randrange(1 << 63), rng.randrange(1 << 62)) for _ in range(count)]


@pytest.mark.parametrize("q", INT60)
def test_split_reduce_and_split_reduce2(q):
    """q < 2^60, approximate quotients: lazy sums below 12q and 8q, canonical results"""
    rng = random.Random(q + 2)
    k = SplitRed(q)
    for ll, mm, hh in _split_points(rng, 400):
        want = (ll + (mm << 30) + (hh << 60)) % q
        assert split_reduce(ll, mm, hh, k) == want, (q, ll, mm, hh)
        assert split_reduce2(ll, mm, hh, k) == want, (q, ll, mm, hh)
    # values within one of a multiple of q: mm and hh at their bounds, ll solved for
    for mm in (0, (1 << 63) - 1, (1 << 63) - 2):
        for hh in (0, (1 << 62) - 1, (1 << 62) - 2):
            for target in (-1, 0, 1):
                for j in range(3):
                    ll = (target - (mm << 30) - (hh << 60)) % q + j * q
                    assert ll < 1 << 62
                    assert split_reduce(ll, mm, hh, k) == target % q, (q, ll, mm, hh)
                    assert split_reduce2(ll, mm, hh, k) == target % q, (q, ll, mm, hh)


def test_split_reduce2_needs_its_three_subtractions():
    """the lazy sum of split_reduce2 passes 4q for partial sums inside the stated bounds (rarely:
    both approximate quotients low at once), so none of the 4q, 2q, q subtractions is spare.  The
    modulus is a 50-bit limb of the mixed chain of tests/test_gpu_edges.py (2^60 mod q generic)."""
    q = 1 << 50
    for _ in range(6):
        q = E.prime_below(q, N)
    assert q == 0x3FFFFFFF46001
    k = SplitRed(q)
    # found by a random search with hh within 2^58 of its bound (about one point in 10^4)
    witnesses = [(0x3532F5883537337C, 0x448D190D4D02C31E, 0x3EFC61C6EB357C78),
                 (0x6E4A03A8DE171, 0x7466AAD08E6393F7, 0x3DDAD68825C76F6F),
                 (0x167B85ADDA38FC23, 0x5EF28DBE4A81C3E4, 0x3FA9539A5E42CFE4)]
    for ll, mm, hh in witnesses:
        assert ll < 1 << 62 and mm < 1 << 63 and hh < 1 << 62
        want = (ll + (mm << 30) + (hh << 60)) % q
        assert split_reduce2(ll, mm, hh, k) == want
        assert split_reduce2(ll, mm, hh, k, drop_4q=True) != want


@pytest.mark.parametrize("q", INT61)
def test_split_reduce_exact(q):
    """q < 2^61, exact high products: any 64-bit partial sums (61-bit moduli reach 2^64 at BETA = 4)"""
    rng = random.Random(q + 3)
    k = SplitRed(q)
    pts = _split_points(rng, 300) + [(M64, M64, M64), (M64 - 1, M64, 0), (0, M64, M64 - 1)]
    pts += [(rng.randrange(1 << 64), rng.randrange(1 << 64), rng.randrange(1 << 64)) for _ in range(300)]
    for ll, mm, hh in pts:
        assert split_reduce_exact(ll, mm, hh, k) == (ll + (mm << 30) + (hh << 60)) % q, (q, ll, mm, hh)


def _ks_sums(dig, key):
    """ks_rotate_batch_full's partial sums of BETA products (wrapping 64-bit adds)"""
    ll = mm = hh = 0
    for d, k in zip(dig, key):
        dl, dh, kl, kh = d & M30, d >> 30, k & M30, k >> 30
        ll = (ll + dl * kl) & M64
        mm = (mm + dl * kh) & M64
        mm = (mm + dh * kl) & M64
        hh = (hh + dh * kh) & M64
    return ll, mm, hh


def _lt_sum(xs, ws, chunk):
    """lt_bsgs_kernel / lt_bsgs_tile / bconv_fixed_kernel: four 64-bit partial sums of `chunk`
    products (wrapping), folded into a 128-bit sum; returns (sum mod 2^128, largest partial sum
    had the adds not wrapped)"""
    acc, peak = 0, 0
    for c0 in range(0, len(xs), chunk):
        ll = m1 = m2 = hh = 0
        for x, w in zip(xs[c0:c0 + chunk], ws[c0:c0 + chunk]):
            xl, xh, wl, wh = x & M30, x >> 30, w & M30, w >> 30
            ll, m1, m2, hh = ll + xl * wl, m1 + xl * wh, m2 + xh * wl, hh + xh * wh
        peak = max(peak, ll, m1, m2, hh)
        ll, m1, m2, hh = ll & M64, m1 & M64, m2 & M64, hh & M64
        acc = (acc + ll + (m1 << 30) + (m2 << 30) + (hh << 60)) & ((1 << 128) - 1)
    return acc, peak


@pytest.mark.parametrize("q", INT61)
@pytest.mark.parametrize("target", [-1, 0, 1])
def test_near_multiple_sums(q, target):
    """sums of products that are -1, 0, 1 modulo q with the other operands at max / lowmax: the
    inner sums (32 products, chunks of 16 / 8 below 2^60 and 4 at 61 bits) and the key-switch sums
    (4 products) through each of their reductions"""
    k = SplitRed(q)
    for fa in ("max", "lowmax"):
        for fb in ("max", "lowmax"):
            a, b = E.near_multiple_operands(q, 32, target, fa, fb)
            for chunk in ((16, 8) if q < 1 << 60 else (4,)):
                acc, peak = _lt_sum(a, b, chunk)
                assert peak < 1 << 64 and acc == sum(x * y for x, y in zip(a, b))
                assert barrett_reduce_128(acc & M64, acc >> 64, q, k.r0, k.r1) == target % q
            d, key = E.near_multiple_operands(q, 4, target, fa, fb)
            ll, mm, hh = _ks_sums(d, key)
            assert ll + (mm << 30) + (hh << 60) == sum(x * y for x, y in zip(d, key))  # nothing wrapped
            assert split_reduce_exact(ll, mm, hh, k) == target % q
            if q < 1 << 60:
                assert ll < 1 << 62 and mm < 1 << 63 and hh < 1 << 62
                assert split_reduce(ll, mm, hh, k) == target % q
                assert split_reduce2(ll, mm, hh, k) == target % q


def test_patterns_reach_the_bounds():
    """max / lowmax operands at the largest primes below 2^60 and 2^61 drive the partial sums to at
    least half of the bound each kernel comment states"""
    q, mx, lm = P60LO, P60LO - 1, E.lowmax(P60LO)
    # lt_bsgs_kernel: 16 products per partial sum below 2^64; lt_bsgs_tile: 8 below 2^63
    for chunk, bound in ((16, 1 << 64), (8, 1 << 63)):
        for a, b in ((mx, mx), (lm, lm), (mx, lm)):
            _, peak = _lt_sum([a] * chunk, [b] * chunk, chunk)
            assert bound // 2 <= peak < bound, (chunk, a, b)
        # each of the four sums on its own: hh by max, ll by lowmax, the cross sums by lowmax
        xl, xh = lm & M30, mx >> 30
        assert chunk * xh * xh >= bound // 2 and chunk * xl * xl >= bound // 2 and chunk * xl * (lm >> 30) >= bound // 2
    # 61-bit moduli: 4 products, the high-half sum below 2^64
    q61 = P61
    _, peak = _lt_sum([q61 - 1] * 4, [q61 - 1] * 4, 4)
    assert 1 << 63 <= peak < 1 << 64
    assert 5 * ((q61 - 1) >> 30) ** 2 >= 1 << 64  # and a fifth product would not fit: kChunk = 4 is tight
    # ks_rotate_batch_full at BETA = 4, q < 2^60: ll, hh < 2^62 and mm < 2^63
    ll, mm, hh = _ks_sums([lm] * 4, [lm] * 4)
    assert 1 << 61 <= ll < 1 << 62 and 1 << 62 <= mm < 1 << 63
    ll, mm, hh = _ks_sums([mx] * 4, [mx] * 4)
    assert 1 << 61 <= hh < 1 << 62
    # ... and at 61 bits the exact form's sums reach past 2^63 without wrapping
    ll, mm, hh = _ks_sums([q61 - 1] * 4, [q61 - 1] * 4)
    assert 1 << 63 <= hh < 1 << 64
    ll, mm, hh = _ks_sums([E.lowmax(q61)] * 4, [E.lowmax(q61)] * 4)
    assert 1 << 63 <= mm < 1 << 64
    # reduce16_est / the 16q lazy ranges: q - 1 inputs put 16 q - 16 inside [8q, 16q)
    assert 8 * q <= 16 * (q - 1) < 16 * q < 1 << 64
    # leaf_combine at kLeafMaxK = 16 terms: one partial sum below 2^60, folds of 4 at 61 bits (a
    # single sum of 16 would wrap: the kernel's leaf_sum<K, 4>)
    for a, b in ((mx, mx), (lm, lm), (mx, lm)):
        acc, peak = _lt_sum([a] * 16, [b] * 16, 16)
        assert 1 << 63 <= peak < 1 << 64 and acc == 16 * a * b
    a = q61 - 1
    acc, peak = _lt_sum([a] * 16, [a] * 16, 4)
    assert 1 << 63 <= peak < 1 << 64 and acc == 16 * a * a
    acc, peak = _lt_sum([a] * 16, [a] * 16, 16)
    assert peak >= 1 << 64 and acc != 16 * a * a


def _primes_below(bound, count):
    out = []
    while len(out) < count:
        bound = E.prime_below(bound, N)
        out.append(bound)
    return out


def _bconv_matrix(ibase, obase):
    """qhat_mod_p as DeviceBaseConverter::init builds it: column j = [prod_{k != i} q_k mod p_j]_i"""
    cols = []
    for p in obase:
        col = []
        for i in range(len(ibase)):
            c = 1
            for kk, qk in enumerate(ibase):
                if kk != i:
                    c = c * qk % p
            col.append(c)
        cols.append(col)
    return cols


def _bconv_peak(ibase, cols, m):
    """largest partial sum of bconv_fixed_kernel over every run of m consecutive input limbs, every
    output column and the inputs max / lowmax (the adds not wrapped), and whether the folded
    128-bit sums are the exact ones"""
    peak, exact = 0, True
    for col in cols:
        for pat in ("max", "lowmax"):
            xs = [q - 1 if pat == "max" else E.lowmax(q) for q in ibase]
            for s0 in range(len(ibase) - m + 1):
                acc, pk = _lt_sum(xs[s0:s0 + m], col[s0:s0 + m], m)
                peak = max(peak, pk)
                exact = exact and acc == sum(x * c for x, c in zip(xs[s0:s0 + m], col[s0:s0 + m]))
    return peak, exact


def _split_terms_from_sums(ibase, obase):
    """how many products fit each of the four partial sums of _lt_sum (ll = lo lo, m1 = lo hi,
    m2 = hi lo, hh = hi hi) for inputs below their ibase modulus and matrix entries below their obase
    modulus: the largest term of each sum, from the largest half on each side"""
    lo = M30
    hx, hc = max((q - 1) >> 30 for q in ibase), max((p - 1) >> 30 for p in obase)
    xl, cl = min(lo, max(ibase) - 1), min(lo, max(obase) - 1)
    return ((1 << 64) - 1) // max(xl * cl, xl * hc, hx * cl, hx * hc)


# (ibase bits, obase bits, products that fit): equal widths, and 61-bit moduli on one side only,
# where the cross sum of the wide side (not the high-by-high sum) is the one that wraps
BCONV_WIDTHS = [(60, 60, 16), (61, 61, 4), (61, 50, 8), (50, 61, 8), (61, 60, 8), (30, 61, 8), (50, 50, 16)]


@pytest.mark.parametrize("ib_bits,ob_bits,terms", BCONV_WIDTHS)
def test_bconv_fixed_sums_at_15_primes(ib_bits, ob_bits, terms):
    """bconv_fixed_kernel's four 64-bit partial sums through the real conversion matrix of 15 input
    primes and 20 output primes, inputs max and lowmax.  Below 2^60 on both sides 15 products fit
    (and reach 2^63); a 61-bit modulus on either side has halves up to 2^31, which enlarges the
    high-by-high sum and that side's cross sum, so that 15 products wrap: only `terms` fit, the
    count rns.hip bconv_split_terms must give so that bconv() sends larger ibases to the 128-bit
    kernel.  The count is derived here from the sums themselves, not from that function."""
    ibase = _primes_below(1 << ib_bits, 15)
    obase = [p for p in _primes_below(1 << ob_bits, 35) if p not in ibase][:20]
    cols = _bconv_matrix(ibase, obase)
    assert _split_terms_from_sums(ibase, obase) == terms
    m = min(terms, 15)
    peak, exact = _bconv_peak(ibase, cols, m)
    assert peak < 1 << 64 and exact
    if terms >= 15:
        assert peak >= 1 << 63 or ib_bits < 60  # the patterns reach half of the 2^64 bound
    else:
        peak, exact = _bconv_peak(ibase, cols, 15)  # the whole ibase in one sum wraps
        assert peak >= 1 << 64 and not exact
        worst = ((P61 - 1) >> 30) * M30  # and `terms` is tight for worst-case matrix entries
        assert (terms + 1) * worst >= 1 << 64 or ib_bits == ob_bits
    assert 16 * M30 ** 2 < 1 << 64 <= 17 * M30 ** 2  # the static_assert IB <= 15 has one to spare


@pytest.mark.parametrize("q", [1 << 50, P50HI, (1 << 55) + 3, (1 << 59) - 55, P60LO, (1 << 60) - 1])
def test_reduce16_est(q):
    """v < 16q -> v mod q for 2^50 <= q < 2^60, the quotient estimate floor(v / q) or one less; the
    worst case of the margin argument is q just above 2^50 (the low word's lo / q = 2^-18)"""
    rng = random.Random(q + 4)
    vs = set(_around(q, 16, 16 * q))
    for k in range(17):  # both ends of the dropped low word around every multiple
        base = k * q
        for v in ((base >> 32) << 32, ((base >> 32) << 32) | 0xFFFFFFFF, (((base >> 32) + 1) << 32),
                  (((base >> 32) + 1) << 32) - 1, base + q // 2, base + q - 2):
            if 0 <= v < 16 * q:
                vs.add(v)
    vs.update([16 * q - 1, 16 * q - 2])
    for v in sorted(vs) + _rand_below(rng, 16 * q, 600):
        got, k = reduce16_est(v, q)
        assert v // q - 1 <= k <= v // q, (q, v, k)
        assert got == v % q, (q, v)


@pytest.mark.parametrize("q", INT60)
def test_reduce16(q):
    rng = random.Random(q + 5)
    for v in _around(q, 16, 16 * q) + _rand_below(rng, 16 * q, 400):
        assert reduce16(v, q) == v % q, (q, v)


def _twiddles(rng, q):
    return [1, 2, q - 1, q - 2, (q - 1) // 2, (q + 1) // 2, E.lowmax(q)] + _rand_below(rng, q, 6)


def _range_points(rng, q, r, count):
    """values of a lazy range [0, r q): its ends, the multiples of q inside it, and random"""
    edges = [0, 1, r * q - 1, r * q - 2] + [k * q + d for k in range(1, r) for d in (-1, 0)]
    return edges + _rand_below(rng, r * q, count)


@pytest.mark.parametrize("q", INT60)
def test_ct_bfly_nored_and_c8(q):
    """q < 2^60: x, y < 12q -> below 16q without a reduction; x < 16q -> below 12q with one"""
    rng = random.Random(q + 6)
    for w in _twiddles(rng, q):
        ws = (w << 64) // q
        for x in _range_points(rng, q, 12, 6):
            for y in _range_points(rng, q, 12, 6) + [16 * q - 1, M64]:
                xo, yo, t = ct_bfly_nored(x, y, w, ws, q)
                assert t < 4 * q and 0 <= yo and xo < 16 * q and yo < 16 * q and xo < 1 << 64 and yo < 1 << 64
                assert (xo - x - y * w) % q == 0 and (yo - x + y * w) % q == 0
        for x in _range_points(rng, q, 16, 6):
            for y in _range_points(rng, q, 16, 6):
                xo, yo, t = ct_bfly_c8(x, y, w, ws, q)
                assert 0 <= yo and xo < 12 * q and yo < 12 * q
                assert (xo - x - y * w) % q == 0 and (yo - x + y * w) % q == 0


@pytest.mark.parametrize("q", INT60)
@pytest.mark.parametrize("red", [True, False])
def test_gs_bfly8(q, red):
    """q < 2^60, inputs below 8q: the sum below 16q (below 8q when RED), the product below 4q"""
    rng = random.Random(q + 7)
    for w in _twiddles(rng, q):
        ws = (w << 64) // q
        for x in _range_points(rng, q, 8, 6):
            for y in _range_points(rng, q, 8, 6):
                xo, yo = gs_bfly8(x, y, w, ws, q, red)
                assert xo < (8 if red else 16) * q and yo < 4 * q
                assert (xo - x - y) % q == 0 and (yo - (x - y) * w) % q == 0


@pytest.mark.parametrize("q", FP50)
def test_fmodmul(q):
    """exact FP64 for q < 2^50: t = y w (mod q) with |t| inside Bound::prod(Y, W) q, at |y| = 7.75 q
    with |w| = q / 2, one below, and small primes (a 30-bit prime: products far below 2^106)"""
    rng = random.Random(q + 8)
    ymax, wmax = (31 * q) // 4, (q - 1) // 2  # 7.75 q and q / 2 (the tables' centred twiddles)
    assert ymax < 1 << 53
    ys = [0, 1, -1, ymax, ymax - 1, -ymax, -(ymax - 1), q, -q, (q - 1) // 2, 7 * q + 1]
    wsx = [0, 1, -1, wmax, wmax - 1, -wmax, -(wmax - 1), E.lowmax(q) % (wmax + 1)]
    ys += [rng.randrange(-ymax, ymax + 1) for _ in range(20)]
    wsx += [rng.randrange(-wmax, wmax + 1) for _ in range(20)]
    for y in ys:
        for w in wsx:
            t = fmodmul(y, w, q)
            assert (t - y * w) % q == 0, (q, y, w)
            assert abs(t) <= (0.51 + 0.4 * 7.75 * 0.5) * q, (q, y, w, t)  # Bound::prod(7.75, 0.5)
            if abs(y) <= q // 2 + 1:  # reduced inputs: Bound::prod(0.51, 0.5)
                assert abs(t) <= (0.51 + 0.4 * 0.51 * 0.5) * q, (q, y, w, t)


@pytest.mark.parametrize("q", FP50)
def test_freduce_and_f64_to_canonical(q):
    """|v| < 2^53 (kernels: below 7.75 q) -> |v'| <= q / 2 + 1, and the canonical residue"""
    rng = random.Random(q + 9)
    top = min((31 * q) // 4, (1 << 53) - 1)
    vs = [0, 1, -1, top, top - 1, -top, -(top - 1)]
    for k in range(8):  # around the multiples and the rounding ties (k + 1/2) q
        for d in (-2, -1, 0, 1, 2):
            vs += [k * q + d, -(k * q) + d, k * q + q // 2 + d, -(k * q + q // 2) + d]
    vs = [v for v in vs if abs(v) <= top] + [rng.randrange(-top, top + 1) for _ in range(400)]
    for v in vs:
        r = freduce(v, q)
        assert (r - v) % q == 0 and 2 * abs(r) <= q + 2, (q, v, r)
        assert f64_to_canonical(v, q) == v % q, (q, v)
    if q < 1 << 40:  # small primes: any |v| < 2^53 (quotients up to 2^23)
        for v in [(1 << 53) - 1, -((1 << 53) - 1)] + [rng.randrange(-(1 << 53) + 1, 1 << 53) for _ in range(300)]:
            assert 2 * abs(freduce(v, q)) <= q + 2 and f64_to_canonical(v, q) == v % q, (q, v)


def test_edge_helpers():
    """edge_cases.py itself: the primes sit where they claim, the patterns are residues"""
    for n in (256, 4096, 1 << 17):
        ps = E.edge_primes(n)
        assert all(E.is_prime(p) and p % (2 * n) == 1 for p in ps)
        assert ps[0] < 1 << 30 and ps[1] < 1 << 50 < ps[2] < ps[3] < 1 << 60 < ps[4] < ps[5] < 1 << 61
        assert ps[0] >> 29 == 1 and ps[1] >> 49 == 1 and ps[2] >> 50 == 1 and ps[4] >> 60 == 1
    assert not E.is_prime((1 << 61) - 3) and E.is_prime((1 << 61) - 1) and not E.is_prime(3215031751)
    mods = E.edge_primes(N)
    for pat in E.PATTERNS:
        a = E.edge_limbs(64, mods, pat).reshape(len(mods), 64)
        for row, q in zip(a, mods):
            assert int(row.max()) < q
    for q in mods[1:]:
        lm = E.lowmax(q)
        assert lm < q and lm & M30 == M30 and lm + (1 << 30) >= q
    st = E.edge_limbs(64, [P60LO], "stripes")
    assert [int(x) for x in st[:9]] == E.stripe_values(P60LO, 0)[:9] and int(st[10]) == 0
