"""Batched public-key encryption on the device (phantom_encrypt_asymmetric_batch,
phantom_sample_small_batch, phantom_encrypt_asymmetric_batch_chunk; csrc/encrypt.hip) through the C-ABI.

All integer arithmetic here has one answer mod q, so every comparison is bit for bit.  Yardsticks: the
one-at-a-time composition of entries that predate the batch (phantom_sample_poly TERNARY / CBD over the
whole key chain, phantom_nwt_forward_inplace, phantom_poly_op against the key, a gather of rows
{0..L-1} u {size_Q..}, phantom_moddown_from_ntt at the chain index, + phantom_ckks_encode) and the CPU
oracle (tests/encrypt_asym_ref.py, pinned by tests/test_encrypt_asym_reference.py).  The public key is
built here as (-(a s + e), a) from the same entries.

Shapes: N = 2^12 and 2^13 with CoeffModulus::Create(N, [60, 40, 40, 60]) (one special prime: chains of
3, 2 and 1 data limbs, so both the FP64 and the integer NTT limbs occur), batches of 1, 3 and one more
than an internal chunk; N = 2^12 with [60, 40, 40, 40, 60, 60] and two special primes (non-contiguous
rows, several P limbs in the conversion); and one N = 2^16 case on the bootstrap's key chain.
"""
import ctypes

import numpy as np
import pytest

import encrypt_asym_ref as A
import phantom_amd as PA
from gpu_util import ptr, stream, to_host, torch

pytestmark = pytest.mark.gpu

BITS = [60, 40, 40, 60]
BITS2 = [60, 40, 40, 40, 60, 60]
KEY = np.array([(0x9E3779B9 * (i + 1)) & 0xFFFFFFFF for i in range(8)], dtype=np.uint32)
NONCE0 = (7 << 40) | 11  # above 2^32: a truncated nonce would show
SCALE = 2.0**40
MUL, ADD, NEGATE = 2, 0, 3
UNIFORM, CBD, TERNARY = 0, 1, 2
GUARD = 0x5A5A5A5A5A5A5A5A


def nonces(p):
    """the draws a façade key would issue for ciphertext p: u, e0, e1"""
    return [NONCE0 + 3 * p + j for j in range(3)]


def dev_c128(a):
    return torch().from_numpy(np.ascontiguousarray(a, dtype=np.complex128)).cuda()


def zeros_u64(words):
    return torch().zeros(words, dtype=torch().int64, device="cuda")


class Ring:
    """a context, its tables, a ternary secret and its public key, NTT form over the whole key chain"""

    def __init__(self, n, mods, special):
        self.n, self.mods, self.alpha = n, list(mods), special
        self.ctx = PA.Context(n, self.mods, special)
        self.tables = PA.NttTables(n, self.mods)
        self.enc = PA.Encoder(self.ctx)
        self.lib, self.h = PA.load(), self.ctx.handle
        self.size_Q, self.size_QP = self.ctx.size_Q, len(self.mods)
        QP, s = self.size_QP, stream()
        self.sk = self.small(TERNARY, 0)
        a, t = zeros_u64(QP * n), zeros_u64(QP * n)
        PA.check(self.lib.phantom_sample_poly(self.h, UNIFORM, KEY.ctypes.data, 1, ptr(a), QP, s))
        e = self.small(CBD, 2)
        self.op(MUL, ptr(a), ptr(self.sk), ptr(t), QP)
        self.op(ADD, ptr(t), ptr(e), ptr(t), QP)
        self.op(NEGATE, ptr(t), None, ptr(t), QP)
        self.pk = torch().cat([t, a])
        self.pub = PA.PublicEncryptor(self.ctx, ptr(self.pk), KEY)
        self.sec = PA.Encryptor(self.ctx, ptr(self.sk), KEY)

    def limbs(self, chain):
        return self.size_Q - (chain - 1)

    def op(self, op, a, b, out, L):
        PA.check(self.lib.phantom_poly_op(self.h, op, a, b, out, 0, L, stream()))

    def small(self, kind, nonce):
        """NTT of a small sample over the whole chain"""
        x = zeros_u64(self.size_QP * self.n)
        PA.check(self.lib.phantom_sample_poly(self.h, kind, KEY.ctypes.data, nonce, ptr(x), self.size_QP, stream()))
        PA.check(self.lib.phantom_nwt_forward_inplace(ptr(x), self.tables.handle, self.size_QP, 0, stream()))
        return x

    def pre_division(self, p):
        """(pk0 u + e0, pk1 u + e1) over the whole chain, as encrypt_asymmetric forms them"""
        n, QP = self.n, self.size_QP
        nu, n0, n1 = nonces(p)
        u, out = self.small(TERNARY, nu), []
        for j, nn in enumerate((n0, n1)):
            x = zeros_u64(QP * n)
            self.op(MUL, ptr(u), ptr(self.pk) + 8 * j * QP * n, ptr(x), QP)
            self.op(ADD, ptr(x), ptr(self.small(CBD, nn)), ptr(x), QP)
            out.append(x)
        return out

    def moddown(self, chain, cx):
        out = zeros_u64(self.limbs(chain) * self.n)
        PA.check(self.lib.phantom_moddown_from_ntt(self.h, chain, ptr(cx), ptr(out), stream()))
        return out

    def sequential_ct(self, chain, values, num_values, sparse, p, divide_at_chain_1=False):
        """ciphertext p from the entries that predate the batch"""
        n, L = self.n, self.limbs(chain)
        halves = []
        for x in self.pre_division(p):
            if divide_at_chain_1:  # the façade's order: divide over all of Q, keep the leading limbs
                halves.append(self.moddown(1, x)[:L * n].clone())
            else:
                rows = list(range(L)) + list(range(self.size_Q, self.size_QP))
                halves.append(self.moddown(chain, x.view(self.size_QP, n)[rows].contiguous().view(-1)))
        m = zeros_u64(L * n)
        self.enc.encode(chain, ptr(dev_c128(values)), num_values, SCALE, ptr(m), stream(), sparse_slots=sparse)
        self.op(ADD, ptr(halves[0]), ptr(m), ptr(halves[0]), L)
        return np.concatenate([to_host(halves[0]), to_host(halves[1])])

    def batch(self, chain, values, num_values, count, sparse=0, out_stride=0, out=None, overflow=None, first=0):
        """phantom_encrypt_asymmetric_batch of ciphertexts first .. first + count - 1; returns the device buffer"""
        words = 2 * self.limbs(chain) * self.n
        if out is None:
            out = zeros_u64(count * (out_stride or words))
        nn = [v for p in range(count) for v in nonces(first + p)]
        self.pub.encrypt(chain, ptr(dev_c128(values)), num_values, SCALE, nn, ptr(out), stream(), sparse_slots=sparse,
                         out_stride=out_stride, overflow=overflow)
        return out


_rings = {}


def ring(log_n, bits=BITS, special=1):
    k = (log_n, len(bits))
    if k not in _rings:
        n = 1 << log_n
        _rings[k] = Ring(n, PA.coeff_modulus_create(n, bits), special)
    return _rings[k]


def values_in(rng, shape, lo=-1.0, hi=1.0):
    return rng.uniform(lo, hi, shape) + 1j * rng.uniform(lo, hi, shape)


@pytest.mark.parametrize("chain", [1, 2, 3])
@pytest.mark.parametrize("log_n", [10, 12, 13, 15])
def test_encrypt_equals_the_sequential_entries(rng, log_n, chain):
    R = ring(log_n)
    n, slots = R.n, R.n // 2
    chunk = R.pub.chunk(chain)
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


@pytest.mark.parametrize("chain", [1, 3])
def test_two_special_primes(rng, chain):
    R = ring(12, BITS2, 2)
    assert R.size_Q == 4 and R.alpha == 2
    count, slots = 3, R.n // 2
    v = values_in(rng, (count, slots))
    got = to_host(R.batch(chain, v, slots, count)).reshape(count, -1)
    for p in range(count):
        assert np.array_equal(got[p], R.sequential_ct(chain, v[p], slots, 0, p)), p


@pytest.mark.parametrize("bits,special,chain", [(BITS, 1, 2), (BITS, 1, 3), (BITS2, 2, 3)])
def test_equals_division_at_chain_1_then_dropping_limbs(rng, bits, special, chain):
    """identity 1 on the device: the façade divides over all of Q and keeps the leading limbs"""
    R = ring(12, bits, special)
    v = values_in(rng, (2, R.n // 2))
    got = to_host(R.batch(chain, v, R.n // 2, 2)).reshape(2, -1)
    for p in range(2):
        assert np.array_equal(got[p], R.sequential_ct(chain, v[p], R.n // 2, 0, p, divide_at_chain_1=True)), p


@pytest.mark.parametrize("bits,special", [(BITS, 1), (BITS2, 2)])
def test_out_stride_leaves_the_guard_words(rng, bits, special):
    R = ring(12, bits, special)
    chain, count, guard = 2, 3, 6
    words = 2 * R.limbs(chain) * R.n
    v = values_in(rng, (count, R.n // 2))
    out = torch().full((count * (words + guard),), GUARD, dtype=torch().int64, device="cuda")
    R.batch(chain, v, R.n // 2, count, out_stride=words + guard, out=out)
    got = to_host(out).reshape(count, words + guard)
    for p in range(count):
        assert np.array_equal(got[p, :words], R.sequential_ct(chain, v[p], R.n // 2, 0, p)), p
    assert np.all(got[:, words:] == np.uint64(GUARD))


def test_fewer_values_and_sparse(rng):
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


@pytest.mark.parametrize("bits,special,chain", [(BITS, 1, 1), (BITS2, 2, 3)])
def test_encrypt_equals_the_cpu_oracle(rng, bits, special, chain):
    """only the plaintext m and the key come from the device"""
    R = ring(12, bits, special)
    n, L, count = R.n, R.limbs(chain), 2
    v = values_in(rng, (count, n // 2))
    got = to_host(R.batch(chain, v, n // 2, count)).reshape(count, -1)
    pk = to_host(R.pk).reshape(2, -1)
    for p in range(count):
        m = zeros_u64(L * n)
        R.enc.encode(chain, ptr(dev_c128(v[p])), n // 2, SCALE, ptr(m), stream())
        c0, c1 = A.encrypt_sequential(to_host(m), pk, KEY, nonces(p), n, R.mods, special, L)
        assert np.array_equal(got[p], np.concatenate([c0, c1])), p


def test_small_batch_equals_numpy():
    import chacha_np as C
    import encrypt_ref as E
    R = ring(12)
    nn = [NONCE0, NONCE0 + 1, 7]
    q = 1 << 40
    for kind in (CBD, TERNARY):
        out = torch().zeros(3 * R.n, dtype=torch().int32, device="cuda")
        R.pub.sample_small(kind, nn, ptr(out), stream())
        torch().cuda.synchronize()
        got = out.cpu().numpy().reshape(3, R.n)
        for i, x in enumerate(nn):
            if kind == CBD:
                want = E.cbd_signed(KEY, x, R.n)
            else:
                t = C.sample_ternary(KEY, x, [q], R.n).astype(np.int64)
                want = np.where(t > q // 2, t - q, t)
            assert np.array_equal(got[i], want), (kind, i)
        assert np.abs(got).max() <= (21 if kind == CBD else 1)


def test_unbiased_moddown_context(rng):
    """the opt-in unbiased division is per limb too: a context of its own, restored afterwards"""
    n = 1 << 12
    R = Ring(n, PA.coeff_modulus_create(n, BITS2), 2)
    R.ctx.set_unbiased_moddown(True)
    try:
        v = values_in(rng, (2, n // 2))
        for chain in (1, 3):
            got = to_host(R.batch(chain, v, n // 2, 2)).reshape(2, -1)
            for p in range(2):
                assert np.array_equal(got[p], R.sequential_ct(chain, v[p], n // 2, 0, p)), (chain, p)
                assert np.array_equal(got[p], R.sequential_ct(chain, v[p], n // 2, 0, p, divide_at_chain_1=True))
        biased = to_host(R.batch(3, v, n // 2, 2)).reshape(2, -1)
    finally:
        R.ctx.set_unbiased_moddown(False)
    plain = to_host(R.batch(3, v, n // 2, 2)).reshape(2, -1)
    assert not np.array_equal(plain, biased)  # the option really was on
    assert np.array_equal(plain[0], R.sequential_ct(3, v[0], n // 2, 0, 0))


def test_full_size_bootstrap_chain(rng):
    """N = 2^16 on the bootstrap's key chain, chain index 26 (5 limbs + 10 special rows), two ciphertexts"""
    n, chain, count, alpha = 1 << 16, 26, 2, 10
    R = Ring(n, PA.coeff_modulus_create(n, [60] + [59] * 29 + [60] * 10), alpha)
    L = R.limbs(chain)
    assert L == 5
    v = values_in(rng, (count, n // 2), 1.0, 5.0)
    cts = R.batch(chain, v, n // 2, count)
    got = to_host(cts).reshape(count, 2 * L * n)
    for p in range(count):
        assert np.array_equal(got[p], R.sequential_ct(chain, v[p], n // 2, 0, p)), p
    t = torch()
    vals = t.zeros(count * n // 2, dtype=t.complex128, device="cuda")
    R.sec.decrypt_decode(ptr(cts), 2, L, L, count, SCALE, ptr(vals), stream())
    t.cuda.synchronize()
    err = float(np.max(np.abs(vals.cpu().numpy().reshape(count, n // 2) - v)))
    bound = n * (alpha * (n + 1) + 1.5) / SCALE
    print(f"N=2^16 chain 26 public-key round trip: max error {err:.3e}, bound {bound:.3e}")
    # the coefficient bound alpha (n + 1) + 1 (tests/test_encrypt_asym_reference.py) plus half a unit of
    # rounding, all n terms of a slot aligned
    assert err < bound


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
    e = t.zeros(2 * n, dtype=t.int32, device="cuda")
    key, pk = KEY.ctypes.data, ptr(R.pk)
    nn = np.array(nonces(0) + nonces(1), dtype=np.uint64)
    nonce_ptr = nn.ctypes.data

    def enc(ctx=h, chain=1, dev_pk=pk, values=ptr(vals), num=n // 2, sparse=0, scale=SCALE, count=2, k=key,
            no=nonce_ptr, o=ptr(out), stride=0):
        return lib.phantom_encrypt_asymmetric_batch(ctx, chain, dev_pk, values, num, sparse, scale, count, k, no, o,
                                                    stride, None, s)

    def small(ctx=h, kind=CBD, k=key, no=nonce_ptr, count=2, o=ptr(e)):
        return lib.phantom_sample_small_batch(ctx, kind, k, no, count, o, s)

    c = ctypes.c_size_t(0)
    calls = [
        lambda: enc(ctx=None), lambda: enc(dev_pk=None), lambda: enc(values=None), lambda: enc(k=None),
        lambda: enc(no=None), lambda: enc(o=None),
        lambda: enc(count=0), lambda: enc(chain=0), lambda: enc(chain=4), lambda: enc(chain=99),
        lambda: enc(stride=words - 2), lambda: enc(stride=words + 1),
        lambda: enc(scale=0.0), lambda: enc(scale=-1.0), lambda: enc(num=n // 2 + 1),
        lambda: enc(num=4, sparse=3), lambda: enc(num=4, sparse=n), lambda: enc(num=9, sparse=8),
        lambda: enc(dev_pk=pk + 8),
        lambda: small(ctx=None), lambda: small(kind=UNIFORM), lambda: small(kind=3), lambda: small(k=None),
        lambda: small(no=None), lambda: small(count=0), lambda: small(o=None),
        lambda: lib.phantom_encrypt_asymmetric_batch_chunk(None, 1, ctypes.byref(c)),
        lambda: lib.phantom_encrypt_asymmetric_batch_chunk(h, 0, ctypes.byref(c)),
        lambda: lib.phantom_encrypt_asymmetric_batch_chunk(h, 4, ctypes.byref(c)),
        lambda: lib.phantom_encrypt_asymmetric_batch_chunk(h, 1, None),
    ]
    for i, call in enumerate(calls):
        assert call() == 1, i
        assert lib.phantom_last_error(), i
    t.cuda.synchronize()
    assert not out.any() and not e.any()  # nothing was launched
