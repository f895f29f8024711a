"""The device CKKS encoder / decoder (phantom_ckks_*, csrc/encode.hip) through the C-ABI.

Yardsticks: Python integers for the integer stages (round / split, compose), a numpy.longdouble
radix-2 embedding for the FP64 stage, and a float64 numpy restatement of the host encoder's own
radix-2 algorithm (PhantomCKKSEncoder::fft) for the error the project accepts today.

Shapes: N = 2^12 and 2^13 with CoeffModulus::Create(N, [60, 40, 40, 60]) (one special prime: chains
of 3, 2 and 1 data limbs); the embedding and the whole encode / decode chain at every N from 2^10
to 2^17 (EMBED_LOG_N: the embedding's single-tile branch up to N = 2048, even and odd splits above).
"""
import random

import numpy as np
import pytest

import oracle_lib as O
import phantom_amd as PA
from gpu_util import ptr, stream, to_dev, to_host, torch

pytestmark = pytest.mark.gpu

BITS = [60, 40, 40, 60]
LD = np.longdouble
CLD = np.clongdouble


# ---- contexts and numpy references, built once per N ------------------------------------------

class Ring:
    def __init__(self, log_n):
        self.n = n = 1 << log_n
        self.log_n = log_n
        self.mods = PA.coeff_modulus_create(n, BITS)
        self.ctx = PA.Context(n, self.mods, 1)
        self.enc = PA.Encoder(self.ctx)
        m = 2 * n
        idx = np.arange(m)
        self.zeta64 = np.cos(2.0 * np.pi * idx / m) + 1j * np.sin(2.0 * np.pi * idx / m)
        pi_ld = 2 * np.arccos(LD(0))
        ang = (2 * pi_ld) * idx.astype(LD) / LD(m)
        self.zeta_ld = (np.cos(ang) + CLD(1j) * np.sin(ang)).astype(CLD)
        p, si = 1, np.zeros(n // 2, dtype=np.int64)
        for j in range(n // 2):
            si[j] = (p - 1) // 2
            p = (p * 5) % m
        self.slot_index = si
        rev = np.zeros(n, dtype=np.int64)
        for b in range(log_n):
            rev |= ((np.arange(n) >> b) & 1) << (log_n - 1 - b)
        self.brev = rev

    def zeta(self, ld):
        return self.zeta_ld if ld else self.zeta64

    def fft(self, a, inverse, ld):
        """the radix-2 transform of PhantomCKKSEncoder::fft, stage by stage, in a's precision"""
        n, z = self.n, self.zeta(ld)
        a = a[self.brev]
        length = 2
        while length <= n:
            h, step = length // 2, 2 * n // length
            w = z[np.arange(h) * step]
            if inverse:
                w = np.conj(w)
            a = a.reshape(n // length, length)
            u, v = a[:, :h], a[:, h:] * w[None, :]
            a = np.concatenate([u + v, u - v], axis=1).reshape(n)
            length *= 2
        return a

    def slots_to_coeffs(self, v, ld):
        a = np.zeros(self.n, dtype=CLD if ld else np.complex128)
        a[self.slot_index[:len(v)]] = v
        a[self.n - 1 - self.slot_index[:len(v)]] = np.conj(v)
        a = self.fft(a, True, ld)
        return (np.conj(self.zeta(ld)[:self.n]) * a).real / (LD(self.n) if ld else float(self.n))

    def coeffs_to_slots(self, c, ld):
        b = self.zeta(ld)[:self.n] * c.astype(LD if ld else np.float64)
        return self.fft(b, False, ld)[self.slot_index]

    def limb_moduli(self, chain, ext):
        q = self.ctx.ql(chain)
        return q + self.mods[self.ctx.size_Q:] if ext else q


_rings = {}


def ring(log_n):
    if log_n not in _rings:
        _rings[log_n] = Ring(log_n)
    return _rings[log_n]


def dev_f64(a):
    return torch().from_numpy(np.ascontiguousarray(a, dtype=np.float64)).cuda()


def dev_c128(a):
    return torch().from_numpy(np.ascontiguousarray(a, dtype=np.complex128)).cuda()


def host(t):
    torch().cuda.synchronize()
    return t.cpu().numpy()


def unit_square(rng, shape):
    return rng.uniform(-1, 1, shape) + 1j * rng.uniform(-1, 1, shape)


def embed_inverse(R, v, sparse_slots=0, count=1, s=None):
    out = torch().zeros(count * R.n, dtype=torch().float64, device="cuda")
    R.enc.embed(False, ptr(dev_c128(v)), ptr(out), stream() if s is None else s, sparse_slots, count)
    return host(out).reshape(count, R.n)


def embed_forward(R, c, sparse_slots=0, count=1):
    ns = sparse_slots or R.n // 2
    out = torch().zeros(count * ns, dtype=torch().complex128, device="cuda")
    R.enc.embed(True, ptr(dev_f64(c)), ptr(out), stream(), sparse_slots, count)
    return host(out).reshape(count, ns)


# ---- FP stage: the embedding -------------------------------------------------------------------

# csrc/encode.hip splits log_n into s1 = (log_n + 1) / 2 and s2: 10 is below its single-tile bound
# (kTile = 2048), 11 equals it, 14 / 15 are an even and an odd split, 17 the largest degree
EMBED_LOG_N = [10, 11, 12, 13, 14, 15, 16, 17]


@pytest.mark.parametrize("log_n", EMBED_LOG_N)
def test_embed_inverse_error_against_longdouble(rng, log_n):
    R = ring(log_n)
    v = unit_square(rng, R.n // 2)
    want = R.slots_to_coeffs(v.astype(CLD), True)
    e_host = float(np.max(np.abs(R.slots_to_coeffs(v, False) - want)))
    e_dev = float(np.max(np.abs(embed_inverse(R, v)[0] - want)))
    print(f"inverse embedding N=2^{log_n}: e_dev {e_dev:.3e} e_host {e_host:.3e} ratio {e_dev / e_host:.3f}")
    assert e_host < 1e-15 * max(1.0, float(np.max(np.abs(want)))) * 16  # the yardstick itself is sane
    assert e_dev <= 4 * e_host


@pytest.mark.parametrize("log_n", EMBED_LOG_N)
def test_embed_forward_error_against_longdouble(rng, log_n):
    R = ring(log_n)
    c = rng.uniform(-1, 1, R.n)
    want = R.coeffs_to_slots(c, True)
    e_host = float(np.max(np.abs(R.coeffs_to_slots(c, False) - want)))
    e_dev = float(np.max(np.abs(embed_forward(R, c)[0] - want)))
    print(f"forward embedding N=2^{log_n}: e_dev {e_dev:.3e} e_host {e_host:.3e} ratio {e_dev / e_host:.3f}")
    assert e_dev <= 4 * e_host


@pytest.mark.parametrize("log_n", [10, 11, 12, 13, 15])
def test_embed_sparse_agrees_with_dense_tiling(rng, log_n):
    R = ring(log_n)
    ns = R.n // 8
    v = unit_square(rng, ns)
    tiled = np.tile(v, R.n // 2 // ns)
    want = R.slots_to_coeffs(tiled.astype(CLD), True)
    e_host = float(np.max(np.abs(R.slots_to_coeffs(tiled, False) - want)))
    got = embed_inverse(R, v, sparse_slots=ns)[0]
    e_dev = float(np.max(np.abs(got - want)))
    print(f"sparse embedding N=2^{log_n} ns={ns}: e_dev {e_dev:.3e} e_host {e_host:.3e}")
    assert e_dev <= 4 * e_host
    # m'(X^(N / 2ns)): only every (N / 2ns)-th coefficient is populated
    stride = R.n // (2 * ns)
    mask = np.ones(R.n, dtype=bool)
    mask[::stride] = False
    assert np.max(np.abs(got[mask])) <= 4 * e_host
    # forward with sparse_slots returns the first ns slots
    back = embed_forward(R, got, sparse_slots=ns)[0]
    assert back.shape == (ns,) and np.max(np.abs(back - v)) < 1e-12


def test_embed_batch_and_stream_are_bit_identical(rng):
    R = ring(12)
    t = torch()
    v = unit_square(rng, (3, R.n // 2))
    batch = embed_inverse(R, v, count=3)
    for i in range(3):
        assert np.array_equal(batch[i], embed_inverse(R, v[i])[0])
    fwd = embed_forward(R, batch, count=3)
    for i in range(3):
        assert np.array_equal(fwd[i], embed_forward(R, batch[i])[0])
    t.cuda.synchronize()
    side = t.cuda.Stream()
    with t.cuda.stream(side):
        other = embed_inverse(R, v, count=3, s=side.cuda_stream)
    assert np.array_equal(other, batch)


# ---- integer stage: round and split ------------------------------------------------------------

SPECIALS = [0.0, 0.5, 1.5, 2.5, 2.0**53 - 1, 2.0**53, 2.0**62, 2.0**63, 2.0**64, 1.2345e30, 2.0**200]


def split_inputs(rng, n, top):
    """the listed magnitudes with both signs (-0.0 included), `top` as the largest one, then random
    normals times 2^k for k in 0..80"""
    sp = [s * x for x in SPECIALS + [top] for s in (1.0, -1.0)]
    k = np.arange(n - len(sp)) % 81
    return np.concatenate([np.array(sp), rng.standard_normal(n - len(sp)) * 2.0**k])


def want_residues(x, scale, moduli):
    r = [int(np.rint(float(v) * scale)) for v in x]  # the double product, rounded half to even, exact
    return np.array([[v % q for v in r] for q in moduli], dtype=np.uint64).reshape(-1)


@pytest.mark.parametrize("scale", [1.0, 2.0**40])
@pytest.mark.parametrize("chain,ext", [(1, False), (2, False), (3, False), (2, True)])
def test_round_rns_is_bit_exact(rng, chain, ext, scale):
    """Every listed input at both scales.  2^999 times 2^40 is past the 2^1000 limit, where residues
    are unspecified, so at scale 2^40 the top magnitude is 2^959: the product is again 2^999."""
    R = ring(12)
    n, t = R.n, torch()
    moduli = R.limb_moduli(chain, ext)
    L = len(moduli)
    assert R.enc.limbs(chain, ext) == L
    base = split_inputs(rng, n, 2.0**999 / scale)
    x3 = np.stack([base, base[::-1], np.roll(base, 7)])
    flag = t.zeros(1, dtype=t.int32, device="cuda")
    for count in (1, 3):
        x = x3[:count]
        out = t.zeros(count * L * n, dtype=t.int64, device="cuda")
        R.enc.round_rns(chain, ptr(dev_f64(x)), scale, ptr(out), stream(), ext=ext, count=count, ntt_form=False,
                        overflow=ptr(flag))
        got = to_host(out).reshape(count, L * n)
        for p in range(count):
            assert np.array_equal(got[p], want_residues(x[p], scale, moduli)), (count, p)
        # NTT form = the forward NTT of the coefficient form
        ntt = t.zeros(count * L * n, dtype=t.int64, device="cuda")
        R.enc.round_rns(chain, ptr(dev_f64(x)), scale, ptr(ntt), stream(), ext=ext, count=count, ntt_form=True)
        got_ntt = to_host(ntt).reshape(count, L * n)
        for p in range(count):
            assert np.array_equal(got_ntt[p], O.ntt_fwd(got[p], n, moduli)), (count, p)
    assert int(host(flag)[0]) == 0


@pytest.mark.parametrize("bad", [np.inf, -np.inf, np.nan, 2.0**1000, -(2.0**1000)])
def test_round_rns_overflow_flag(rng, bad):
    R = ring(12)
    t = torch()
    x = rng.standard_normal(R.n)
    x[R.n // 3] = bad
    out = t.zeros(3 * R.n, dtype=t.int64, device="cuda")
    flag = t.zeros(1, dtype=t.int32, device="cuda")
    R.enc.round_rns(1, ptr(dev_f64(x)), 1.0, ptr(out), stream(), ntt_form=False, overflow=ptr(flag))
    assert int(host(flag)[0]) != 0
    # a null flag is accepted, and the other coefficients are still exact
    R.enc.round_rns(1, ptr(dev_f64(x)), 1.0, ptr(out), stream(), ntt_form=False, overflow=None)
    got = to_host(out).reshape(3, R.n)
    keep = np.arange(R.n) != R.n // 3
    want = want_residues(np.where(keep, x, 0.0), 1.0, R.ctx.ql(1)).reshape(3, R.n)
    assert np.array_equal(got[:, keep], want[:, keep])
    # 2^999 at scale 2^40 overflows as well
    flag.zero_()
    x[R.n // 3] = 2.0**999
    R.enc.round_rns(1, ptr(dev_f64(x)), 2.0**40, ptr(out), stream(), ntt_form=False, overflow=ptr(flag))
    assert int(host(flag)[0]) != 0


# ---- integer stage: compose --------------------------------------------------------------------

@pytest.mark.parametrize("chain", [3, 2, 1])  # L = 1, 2, 3
def test_compose_centred_integers(chain):
    R = ring(12)
    n, t = R.n, torch()
    moduli = R.ctx.ql(chain)
    Q = 1
    for q in moduli:
        Q *= q
    half = (Q - 1) // 2
    py = random.Random(1000 + chain)
    xs = [0, 1, -1, 2**53 - 1, -(2**53 - 1), 2**53 + 1, -(2**53 + 1), half, -half]
    xs += [py.randrange(-half, half + 1) for _ in range(n // 2)]
    while len(xs) < n:  # every magnitude below Q/2 as well
        b = py.randrange(1, half.bit_length())
        xs.append(py.choice((1, -1)) * py.randrange(1 << (b - 1), 1 << b))
    xs = [x for x in xs if -half <= x <= half][:n]
    assert len(xs) == n
    res = np.array([[x % q for x in xs] for q in moduli], dtype=np.uint64).reshape(-1)
    plain = to_dev(O.ntt_fwd(res, n, moduli))
    before = to_host(plain)
    out = t.zeros(n, dtype=t.float64, device="cuda")
    R.enc.compose(chain, ptr(plain), ptr(out), stream())
    got = host(out)
    assert np.array_equal(to_host(plain), before)  # the input is not modified
    want = np.array([float(x) for x in xs])  # correctly rounded
    small = np.array([abs(x) < 2**53 for x in xs])
    assert np.array_equal(got[small], want[small])
    assert np.all(np.abs(got - want) <= np.spacing(np.abs(want)))
    # batched: the same plaintext three times, one call
    plain3 = to_dev(np.tile(before, 3))
    out3 = t.zeros(3 * n, dtype=t.float64, device="cuda")
    R.enc.compose(chain, ptr(plain3), ptr(out3), stream(), count=3)
    assert np.array_equal(host(out3), np.tile(got, 3))


# ---- whole chain -------------------------------------------------------------------------------

@pytest.mark.parametrize("log_n", EMBED_LOG_N)
def test_decode_of_encode_returns_the_input(rng, log_n):
    """max error of decode(encode(v)) at scale 2^40 against 4 x the error of the host algorithm
    (float64 radix-2 embedding, exact rounding and exact integers) on the same v"""
    R = ring(log_n)
    n, t, scale = R.n, torch(), 2.0**40
    count = 2
    v = unit_square(rng, (count, n // 2))
    L = R.enc.limbs(1)
    plain = t.zeros(count * L * n, dtype=t.int64, device="cuda")
    flag = t.zeros(1, dtype=t.int32, device="cuda")
    R.enc.encode(1, ptr(dev_c128(v)), n // 2, scale, ptr(plain), stream(), count=count, overflow=ptr(flag))
    back = t.zeros(count * n // 2, dtype=t.complex128, device="cuda")
    R.enc.decode(1, ptr(plain), scale, ptr(back), stream(), count=count)
    got = host(back).reshape(count, n // 2)
    assert int(host(flag)[0]) == 0
    e_host = max(float(np.max(np.abs(R.coeffs_to_slots(np.rint(R.slots_to_coeffs(v[i], False) * scale) / scale, False)
                                     - v[i]))) for i in range(count))
    e_dev = float(np.max(np.abs(got - v)))
    print(f"decode(encode) N=2^{log_n}: e_dev {e_dev:.3e} e_host {e_host:.3e} ratio {e_dev / e_host:.3f}")
    assert e_dev <= 4 * e_host
    # the plaintext is the NTT of the rounded coefficients of the device's own embedding
    c = embed_inverse(R, v[1])[0]
    assert np.array_equal(to_host(plain).reshape(count, L * n)[1],
                          O.ntt_fwd(want_residues(c, scale, R.ctx.ql(1)), n, R.ctx.ql(1)))


def test_encode_zero_pads_and_ext_and_sparse(rng):
    R = ring(12)
    n, t, scale = R.n, torch(), 2.0**40
    v = unit_square(rng, 100)
    padded = np.concatenate([v, np.zeros(n // 2 - 100, dtype=np.complex128)])

    def encode(values, num, chain, ext=False, sparse=0):
        out = t.zeros(R.enc.limbs(chain, ext) * n, dtype=t.int64, device="cuda")
        R.enc.encode(chain, ptr(dev_c128(values)), num, scale, ptr(out), stream(), ext=ext, sparse_slots=sparse)
        return to_host(out)

    full = encode(padded, n // 2, 2)
    assert np.array_equal(encode(v, 100, 2), full)
    # the extended plaintext: the same data limbs, then the special prime's
    ext = encode(padded, n // 2, 2, ext=True)
    assert np.array_equal(ext[:2 * n], full)
    c = embed_inverse(R, padded)[0]
    assert np.array_equal(ext, O.ntt_fwd(want_residues(c, scale, R.limb_moduli(2, True)), n, R.limb_moduli(2, True)))
    # sparse: 100 values, zero-padded to 512 slots, tiled over every block of 512 slots
    ns = 512
    tiled = np.tile(np.concatenate([v, np.zeros(ns - 100, dtype=np.complex128)]), n // 2 // ns)
    assert np.array_equal(encode(v, 100, 2, sparse=ns), encode(tiled, n // 2, 2))


def test_bad_arguments_are_rejected_with_a_message():
    R = ring(12)
    n, t, lib = R.n, torch(), PA.load()
    vals = t.zeros(n // 2, dtype=t.complex128, device="cuda")
    co = t.zeros(n, dtype=t.float64, device="cuda")
    out = t.zeros(4 * n, dtype=t.int64, device="cuda")
    h, s = R.ctx.handle, stream()
    calls = [
        lambda: lib.phantom_ckks_encode(h, 1, 0, ptr(vals), n // 2, 0, 0.0, 1, ptr(out), None, s),
        lambda: lib.phantom_ckks_encode(h, 1, 0, ptr(vals), n // 2, 0, -1.0, 1, ptr(out), None, s),
        lambda: lib.phantom_ckks_encode(h, 1, 0, ptr(vals), n // 2 + 1, 0, 2.0**40, 1, ptr(out), None, s),
        lambda: lib.phantom_ckks_encode(h, 1, 0, ptr(vals), 4, 3, 2.0**40, 1, ptr(out), None, s),
        lambda: lib.phantom_ckks_encode(h, 1, 0, ptr(vals), 4, n, 2.0**40, 1, ptr(out), None, s),
        lambda: lib.phantom_ckks_encode(h, 1, 0, ptr(vals), 9, 8, 2.0**40, 1, ptr(out), None, s),
        lambda: lib.phantom_ckks_encode(h, 99, 0, ptr(vals), n // 2, 0, 2.0**40, 1, ptr(out), None, s),
        lambda: lib.phantom_ckks_encode(h, 0, 1, ptr(vals), n // 2, 0, 2.0**40, 1, ptr(out), None, s),
        lambda: lib.phantom_ckks_round_rns(h, 1, 0, ptr(co), 0.0, 1, 1, ptr(out), None, s),
        lambda: lib.phantom_ckks_round_rns(h, 0, 1, ptr(co), 1.0, 1, 1, ptr(out), None, s),
        lambda: lib.phantom_ckks_round_rns(h, 5, 0, ptr(co), 1.0, 1, 1, ptr(out), None, s),
        lambda: lib.phantom_ckks_compose(h, 4, ptr(out), 1, ptr(co), s),
        lambda: lib.phantom_ckks_decode(h, 4, ptr(out), 2.0**40, 1, ptr(vals), s),
        lambda: lib.phantom_ckks_decode(h, 1, ptr(out), 0.0, 1, ptr(vals), s),
        lambda: lib.phantom_ckks_embed(h, 0, ptr(vals), ptr(co), 3, 1, s),
        lambda: lib.phantom_ckks_embed(h, 0, ptr(vals), ptr(co), n, 1, s),
        lambda: lib.phantom_ckks_embed(None, 0, ptr(vals), ptr(co), 0, 1, s),
    ]
    for i, call in enumerate(calls):
        assert call() == 1, i
        assert lib.phantom_last_error(), i
    t.cuda.synchronize()
    assert not out.any() and not co.any()  # nothing was launched
