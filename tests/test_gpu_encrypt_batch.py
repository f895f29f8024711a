"""Batched symmetric encryption / decryption on the device (phantom_encrypt_symmetric_batch,
phantom_decrypt_batch, phantom_decrypt_decode_batch, phantom_sample_cbd_small_batch; csrc/encrypt.hip)
through the C-ABI.

All integer arithmetic here has one answer mod q, so every comparison is bit for bit.  Yardsticks:
the one-at-a-time composition of entries that predate the batch (phantom_ckks_encode,
phantom_sample_uniform_seeded, phantom_sample_poly + phantom_nwt_forward_inplace, phantom_poly_op)
and the CPU oracle (tests/encrypt_ref.py, pinned by tests/test_encrypt_reference.py).

Shapes: N = 2^12 and 2^13 with CoeffModulus::Create(N, [60, 40, 40, 60]) (one special prime: chains of
3, 2 and 1 data limbs, so both the FP64 and the integer NTT limbs occur), batches of 1, 3 and one more
than an internal chunk, and one N = 2^16 case on the bootstrap's key chain.
"""
import ctypes

import numpy as np
import pytest

import encrypt_ref as E
import oracle_lib as O
import phantom_amd as PA
from gpu_util import ptr, stream, to_host, torch
from test_capi import SALSA_REJECT_PRIMES

pytestmark = pytest.mark.gpu

BITS = [60, 40, 40, 60]
KEY = np.array([(0x9E3779B9 * (i + 1)) & 0xFFFFFFFF for i in range(8)], dtype=np.uint32)
NONCE0 = (5 << 40) | 3  # above 2^32: a truncated nonce would show
SCALE = 2.0**40
MUL, ADD, NEGATE = 2, 0, 3
CBD, TERNARY = 1, 2


def nonce(p):
    """the error draws a façade key would issue: every other draw of its stream"""
    return NONCE0 + 2 * p + 1


def seed(p):
    return bytes((31 * p + 7 * i + 3) & 0xFF for i in range(64))


def dev_c128(a):
    return torch().from_numpy(np.ascontiguousarray(a, dtype=np.complex128)).cuda()


def zeros_u64(words):
    return torch().zeros(words, dtype=torch().int64, device="cuda")


class Ring:
    """a context, its tables and a ternary secret in NTT form over the data primes"""

    def __init__(self, n, mods, special):
        self.n, self.mods = n, list(mods)
        self.ctx = PA.Context(n, self.mods, special)
        self.tables = PA.NttTables(n, self.mods)
        self.enc = PA.Encoder(self.ctx)
        self.lib, self.h = PA.load(), self.ctx.handle
        self.size_Q = self.ctx.size_Q
        self.sk = zeros_u64(self.size_Q * n)
        PA.check(self.lib.phantom_sample_poly(self.h, TERNARY, KEY.ctypes.data, 0, ptr(self.sk), self.size_Q, stream()))
        PA.check(self.lib.phantom_nwt_forward_inplace(ptr(self.sk), self.tables.handle, self.size_Q, 0, stream()))
        self.cry = PA.Encryptor(self.ctx, ptr(self.sk), KEY)

    def limbs(self, chain):
        return self.size_Q - (chain - 1)

    def op(self, op, a, b, out, L):
        PA.check(self.lib.phantom_poly_op(self.h, op, a, b, out, 0, L, stream()))

    def sequential_ct(self, chain, values, num_values, sparse, p):
        """ciphertext p = (m - (a s + e), a) from the entries that predate the batch"""
        n, L, s = self.n, self.limbs(chain), stream()
        m, a, e, t = (zeros_u64(L * n) for _ in range(4))
        self.enc.encode(chain, ptr(dev_c128(values)), num_values, SCALE, ptr(m), s, sparse_slots=sparse)
        PA.check(self.lib.phantom_sample_uniform_seeded(self.h, seed(p), ptr(a), L, s))
        PA.check(self.lib.phantom_sample_poly(self.h, CBD, KEY.ctypes.data, nonce(p), ptr(e), L, s))
        PA.check(self.lib.phantom_nwt_forward_inplace(ptr(e), self.tables.handle, L, 0, s))
        self.op(MUL, ptr(a), ptr(self.sk), ptr(t), L)
        self.op(ADD, ptr(t), ptr(e), ptr(t), L)
        self.op(NEGATE, ptr(t), None, ptr(t), L)
        self.op(ADD, ptr(t), ptr(m), ptr(t), L)
        return np.concatenate([to_host(t), to_host(a)])

    def batch(self, chain, values, num_values, count, sparse=0, out_stride=0, out=None, overflow=None, first=0):
        """phantom_encrypt_symmetric_batch of ciphertexts first .. first + count - 1; returns the device buffer"""
        words = 2 * self.limbs(chain) * self.n
        if out is None:
            out = zeros_u64(count * (out_stride or words))
        self.cry.encrypt(chain, ptr(dev_c128(values)), num_values, SCALE, [nonce(first + p) for p in range(count)],
                         b"".join(seed(first + p) for p in range(count)), ptr(out), stream(), sparse_slots=sparse,
                         out_stride=out_stride, overflow=overflow)
        return out

    def sequential_decrypt(self, ct, polys, ct_limbs, limbs):
        """c0 + c1 s (+ c2 s^2) over the leading limbs with phantom_poly_op; ct is a device [polys][ct_limbs][n]"""
        n = self.n
        t, u = zeros_u64(limbs * n), zeros_u64(limbs * n)
        poly = lambda i: ptr(ct) + 8 * i * ct_limbs * n
        self.op(MUL, poly(1), ptr(self.sk), ptr(t), limbs)
        self.op(ADD, ptr(t), poly(0), ptr(t), limbs)
        if polys == 3:
            self.op(MUL, ptr(self.sk), ptr(self.sk), ptr(u), limbs)
            self.op(MUL, poly(2), ptr(u), ptr(u), limbs)
            self.op(ADD, ptr(t), ptr(u), ptr(t), limbs)
        return to_host(t)


_rings = {}


def ring(log_n):
    if log_n not in _rings:
        n = 1 << log_n
        _rings[log_n] = Ring(n, PA.coeff_modulus_create(n, BITS), 1)
    return _rings[log_n]


def values_in(rng, shape, lo=-1.0, hi=1.0):
    return rng.uniform(lo, hi, shape) + 1j * rng.uniform(lo, hi, shape)


# ---- encryption -------------------------------------------------------------------------------

@pytest.mark.parametrize("chain", [1, 2, 3])
@pytest.mark.parametrize("log_n", [10, 12, 13, 15])
def test_encrypt_equals_the_sequential_entries(rng, log_n, chain):
    R = ring(log_n)
    n, slots = R.n, R.n // 2
    chunk = R.cry.chunk(chain)
    assert 1 <= chunk <= 32
    total = chunk + 1
    v = values_in(rng, (total, slots))
    want = [R.sequential_ct(chain, v[p], slots, 0, p) for p in range(total)]
    words = want[0].size
    assert words == 2 * R.limbs(chain) * n
    for count in (1, 3, total):
        got = to_host(R.batch(chain, v[:count], slots, count)).reshape(count, words)
        for p in range(count):
            assert np.array_equal(got[p], want[p]), (count, p)


def test_encrypt_out_stride_leaves_the_guard_words(rng):
    R = ring(12)
    chain, count, guard = 2, 3, 6
    words = 2 * R.limbs(chain) * R.n
    v = values_in(rng, (count, R.n // 2))
    out = torch().full((count * (words + guard),), 0x5A5A5A5A5A5A5A5A, dtype=torch().int64, device="cuda")
    R.batch(chain, v, R.n // 2, count, out_stride=words + guard, out=out)
    got = to_host(out).reshape(count, words + guard)
    for p in range(count):
        assert np.array_equal(got[p, :words], R.sequential_ct(chain, v[p], R.n // 2, 0, p)), p
    assert np.all(got[:, words:] == np.uint64(0x5A5A5A5A5A5A5A5A))


def test_encrypt_fewer_values_and_sparse(rng):
    R = ring(12)
    chain, slots = 1, R.n // 2
    words = 2 * R.limbs(chain) * R.n
    v = values_in(rng, (2, 100))
    got = to_host(R.batch(chain, v, 100, 2)).reshape(2, words)
    for p in range(2):
        assert np.array_equal(got[p], R.sequential_ct(chain, v[p], 100, 0, p)), p
    ns = R.n // 8
    v = values_in(rng, (2, ns))
    got = to_host(R.batch(chain, v, ns, 2, sparse=ns)).reshape(2, words)
    for p in range(2):
        assert np.array_equal(got[p], R.sequential_ct(chain, v[p], ns, ns, p)), p
        # and the sparse plaintext is the dense tiling's
        assert np.array_equal(got[p], R.sequential_ct(chain, np.tile(v[p], slots // ns), slots, 0, p)), p


def oracle_ct(R, chain, values, p):
    """the CPU oracle's ciphertext p; only the plaintext m comes from the device"""
    n, L = R.n, R.limbs(chain)
    mods = R.mods[:L]
    m = zeros_u64(L * n)
    R.enc.encode(chain, ptr(dev_c128(values)), values.size, SCALE, ptr(m), stream())
    c0, c1 = E.encrypt(to_host(m), seed(p), KEY, nonce(p), to_host(R.sk)[:L * n], n, mods)
    return np.concatenate([c0, c1])


@pytest.mark.parametrize("chain", [1, 3])
def test_encrypt_equals_the_cpu_oracle(rng, chain):
    R = ring(12)
    count = 2
    v = values_in(rng, (count, R.n // 2))
    got = to_host(R.batch(chain, v, R.n // 2, count)).reshape(count, -1)
    for p in range(count):
        assert np.array_equal(got[p], oracle_ct(R, chain, v[p], p)), p


def test_seed_expansion_rejection_path(rng):
    """primes 3 * 2^58 + k 2^17 + 1 reject a keystream word with probability ~2^-6, so the expansion
    of 3 x 4096 words takes the retry path many times"""
    n = 1 << 12
    R = Ring(n, SALSA_REJECT_PRIMES + O.coeff_modulus_create(n, [60]), 1)
    count = 2
    v = values_in(rng, (count, n // 2))
    got = to_host(R.batch(1, v, n // 2, count)).reshape(count, 2, 3 * n)
    for p in range(count):
        assert np.array_equal(got[p, 1], E.expand_seed(seed(p), n, SALSA_REJECT_PRIMES)), p
        assert np.array_equal(got[p].reshape(-1), oracle_ct(R, 1, v[p], p)), p
    # the first attempt alone would differ: the retries really happen in this expansion
    first = np.zeros(16, dtype=np.uint32)
    rejected = 0
    for t in range(64):
        PA.check(R.lib.phantom_salsa20_block(seed(0), t, first.ctypes.data))
        w = first.astype(np.uint64)
        r = w[0::2] | (w[1::2] << np.uint64(32))
        q = SALSA_REJECT_PRIMES[0]
        rejected += int(np.sum(r > np.uint64(2**64 - 1 - (2**64 - 1) % q - 1)))
    assert rejected > 0


def test_cbd_small_batch_equals_numpy():
    R = ring(12)
    nonces = [nonce(0), nonce(1), 7]
    out = torch().zeros(3 * R.n, dtype=torch().int32, device="cuda")
    R.cry.sample_cbd_small(nonces, ptr(out), stream())
    torch().cuda.synchronize()
    got = out.cpu().numpy().reshape(3, R.n)
    assert np.abs(got).max() <= 21
    for i, nn in enumerate(nonces):
        assert np.array_equal(got[i], E.cbd_signed(KEY, nn, R.n)), i


# ---- decryption -------------------------------------------------------------------------------

def product_of_encryptions(R, rng, count):
    """[count] 3-polynomial ciphertexts at chain 1 (3 limbs): phantom_multiply of two encryptions each"""
    n, words = R.n, 2 * 3 * R.n
    a = R.batch(1, values_in(rng, (count, n // 2)), n // 2, count)
    b = R.batch(1, values_in(rng, (count, n // 2)), n // 2, count, first=count)
    out = zeros_u64(count * 3 * 3 * n)
    for p in range(count):
        PA.check(R.lib.phantom_multiply(R.h, 1, ptr(a) + 8 * p * words, ptr(b) + 8 * p * words,
                                        ptr(out) + 8 * p * 3 * 3 * n, stream()))
    return out


@pytest.mark.parametrize("count", [1, 3])
@pytest.mark.parametrize("polys", [2, 3])
def test_decrypt_equals_the_sequential_entries(rng, polys, count):
    R = ring(12)
    n, t, ct_limbs = R.n, torch(), 3
    if polys == 2:
        cts = R.batch(1, values_in(rng, (count, n // 2)), n // 2, count)
    else:
        cts = product_of_encryptions(R, rng, count)
    words = polys * ct_limbs * n
    for limbs in (3, 2):
        src = cts
        if limbs < ct_limbs:  # the dropped limb must not be read: poison it in every polynomial
            src = cts.clone()
            src.view(count, polys, ct_limbs, n)[:, :, limbs:, :] = 0x7EADBEEF7EADBEEF
        plain = zeros_u64(count * limbs * n)
        R.cry.decrypt(ptr(src), polys, ct_limbs, limbs, count, ptr(plain), stream())
        got = to_host(plain).reshape(count, limbs * n)
        for p in range(count):
            one = cts[p * words:(p + 1) * words]
            assert np.array_equal(got[p], R.sequential_decrypt(one, polys, ct_limbs, limbs)), (limbs, p)
        # decode of that plaintext, double for double, at the chain whose basis is those limbs
        scale = SCALE**(polys - 1)
        chain = R.size_Q - limbs + 1
        vals = t.zeros(count * n // 2, dtype=t.complex128, device="cuda")
        R.cry.decrypt_decode(ptr(src), polys, ct_limbs, limbs, count, scale, ptr(vals), stream())
        want = t.zeros(count * n // 2, dtype=t.complex128, device="cuda")
        R.enc.decode(chain, ptr(plain), scale, ptr(want), stream(), count=count)
        t.cuda.synchronize()
        assert np.array_equal(vals.cpu().numpy().view(np.uint64), want.cpu().numpy().view(np.uint64)), limbs


def test_full_size_bootstrap_chain(rng):
    """N = 2^16 on the bootstrap's key chain, chain index 26 (5 limbs), two ciphertexts"""
    n, chain, count = 1 << 16, 26, 2
    R = Ring(n, PA.coeff_modulus_create(n, [60] + [59] * 29 + [60] * 10), 10)
    L = R.limbs(chain)
    assert L == 5
    v = values_in(rng, (count, n // 2), 1.0, 5.0)
    cts = R.batch(chain, v, n // 2, count)
    got = to_host(cts).reshape(count, 2 * L * n)
    for p in range(count):
        assert np.array_equal(got[p], R.sequential_ct(chain, v[p], n // 2, 0, p)), p
    t = torch()
    plain = zeros_u64(count * L * n)
    R.cry.decrypt(ptr(cts), 2, L, L, count, ptr(plain), stream())
    for p in range(count):
        assert np.array_equal(to_host(plain).reshape(count, L * n)[p],
                              R.sequential_decrypt(cts[p * 2 * L * n:(p + 1) * 2 * L * n], 2, L, L)), p
    vals = t.zeros(count * n // 2, dtype=t.complex128, device="cuda")
    R.cry.decrypt_decode(ptr(cts), 2, L, 2, count, SCALE, ptr(vals), stream())
    t.cuda.synchronize()
    err = float(np.max(np.abs(vals.cpu().numpy().reshape(count, n // 2) - v)))
    print(f"N=2^16 chain 26 round trip through two limbs: max error {err:.3e}")
    # worst case: every coefficient off by |e| <= 21 plus half a unit of rounding, all n aligned
    assert err < 22 * n / SCALE


def test_round_trip_error_against_the_sequential_path(rng):
    R = ring(13)
    n, t, chain, count = R.n, torch(), 1, 3
    L = R.limbs(chain)
    v = values_in(rng, (count, n // 2), 1.0, 5.0)
    vals = t.zeros(count * n // 2, dtype=t.complex128, device="cuda")
    R.cry.decrypt_decode(ptr(R.batch(chain, v, n // 2, count)), 2, L, L, count, SCALE, ptr(vals), stream())
    t.cuda.synchronize()
    e_batch = float(np.max(np.abs(vals.cpu().numpy().reshape(count, n // 2) - v)))
    e_seq = 0.0
    for p in range(count):
        ct = t.from_numpy(R.sequential_ct(chain, v[p], n // 2, 0, p).view(np.int64)).cuda()
        plain = t.from_numpy(R.sequential_decrypt(ct, 2, L, L).view(np.int64)).cuda()
        one = t.zeros(n // 2, dtype=t.complex128, device="cuda")
        R.enc.decode(chain, ptr(plain), SCALE, ptr(one), stream())
        t.cuda.synchronize()
        e_seq = max(e_seq, float(np.max(np.abs(one.cpu().numpy() - v[p]))))
    print(f"round trip: batched error {e_batch:.3e}, sequential error {e_seq:.3e}")
    assert 0 < e_seq < 1e-6
    assert e_batch <= 4 * e_seq


# ---- flags and refusals -----------------------------------------------------------------------

def test_overflow_flag_is_set_and_stays(rng):
    R = ring(12)
    t = torch()
    flag = t.zeros(1, dtype=t.int32, device="cuda")
    v = values_in(rng, (1, R.n // 2))
    R.batch(1, v, R.n // 2, 1, overflow=ptr(flag))
    t.cuda.synchronize()
    assert int(flag.cpu()[0]) == 0
    big = v.copy()
    big[0, 5] = 2.0**999
    R.batch(1, big, R.n // 2, 1, overflow=ptr(flag))
    t.cuda.synchronize()
    assert int(flag.cpu()[0]) != 0
    R.batch(1, v, R.n // 2, 1, overflow=ptr(flag))  # a clean call does not clear it
    t.cuda.synchronize()
    assert int(flag.cpu()[0]) != 0


def test_bad_arguments_are_rejected_before_any_launch():
    R = ring(12)
    n, t, lib, h, s = R.n, torch(), R.lib, R.h, stream()
    vals = t.zeros(2 * n // 2, dtype=t.complex128, device="cuda")
    words = 2 * 3 * n
    out = zeros_u64(2 * words + 8)
    plain = zeros_u64(2 * 3 * n)
    dvals = t.zeros(2 * n // 2, dtype=t.complex128, device="cuda")
    e = t.zeros(2 * n, dtype=t.int32, device="cuda")
    key, sk = KEY.ctypes.data, ptr(R.sk)
    nn = np.array([nonce(0), nonce(1)], dtype=np.uint64)
    nonces, seeds = nn.ctypes.data, seed(0) + seed(1)

    def enc(ctx=h, chain=1, dev_sk=sk, values=ptr(vals), num=n // 2, sparse=0, scale=SCALE, count=2, k=key, no=nonces,
            se=seeds, o=ptr(out), stride=0):
        return lib.phantom_encrypt_symmetric_batch(ctx, chain, dev_sk, values, num, sparse, scale, count, k, no, se, o,
                                                   stride, None, s)

    def dec(ctx=h, dev_sk=sk, src=ptr(out), stride=0, polys=2, ct_limbs=3, limbs=3, count=2, o=ptr(plain)):
        return lib.phantom_decrypt_batch(ctx, dev_sk, src, stride, polys, ct_limbs, limbs, count, o, s)

    def decode(ctx=h, dev_sk=sk, src=ptr(out), stride=0, polys=2, ct_limbs=3, limbs=3, count=2, scale=SCALE,
               o=ptr(dvals)):
        return lib.phantom_decrypt_decode_batch(ctx, dev_sk, src, stride, polys, ct_limbs, limbs, count, scale, o, s)

    c = ctypes.c_size_t(0)
    calls = [
        lambda: enc(ctx=None), lambda: enc(dev_sk=None), lambda: enc(values=None), lambda: enc(k=None),
        lambda: enc(no=None), lambda: enc(se=None), lambda: enc(o=None),
        lambda: enc(count=0), lambda: enc(chain=0), lambda: enc(chain=4), lambda: enc(chain=99),
        lambda: enc(stride=words - 2), lambda: enc(stride=words + 1),
        lambda: enc(scale=0.0), lambda: enc(scale=-1.0), lambda: enc(num=n // 2 + 1),
        lambda: enc(num=4, sparse=3), lambda: enc(num=4, sparse=n), lambda: enc(num=9, sparse=8),
        lambda: dec(ctx=None), lambda: dec(dev_sk=None), lambda: dec(src=None), lambda: dec(o=None),
        lambda: dec(count=0), lambda: dec(limbs=4), lambda: dec(limbs=0), lambda: dec(polys=1), lambda: dec(polys=4),
        lambda: dec(stride=words - 2), lambda: dec(ct_limbs=99, limbs=1),
        lambda: decode(ctx=None), lambda: decode(dev_sk=None), lambda: decode(src=None), lambda: decode(o=None),
        lambda: decode(count=0), lambda: decode(limbs=4), lambda: decode(polys=1), lambda: decode(polys=4),
        lambda: decode(stride=words - 2), lambda: decode(scale=0.0),
        lambda: lib.phantom_sample_cbd_small_batch(None, key, nonces, 2, ptr(e), s),
        lambda: lib.phantom_sample_cbd_small_batch(h, None, nonces, 2, ptr(e), s),
        lambda: lib.phantom_sample_cbd_small_batch(h, key, None, 2, ptr(e), s),
        lambda: lib.phantom_sample_cbd_small_batch(h, key, nonces, 0, ptr(e), s),
        lambda: lib.phantom_sample_cbd_small_batch(h, key, nonces, 2, None, s),
        lambda: lib.phantom_encrypt_batch_chunk(None, 1, ctypes.byref(c)),
        lambda: lib.phantom_encrypt_batch_chunk(h, 0, ctypes.byref(c)),
        lambda: lib.phantom_encrypt_batch_chunk(h, 4, ctypes.byref(c)),
        lambda: lib.phantom_encrypt_batch_chunk(h, 1, None),
    ]
    for i, call in enumerate(calls):
        assert call() == 1, i
        assert lib.phantom_last_error(), i
    t.cuda.synchronize()
    assert not out.any() and not plain.any() and not e.any()  # nothing was launched
    assert not dvals.view(t.float64).any()
