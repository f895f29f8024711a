"""phantom_ct_mix (linear combinations of ciphertexts with per-limb scalars, any K and M) on the GPU,
bit-exact against or_poly_mul_scalar + or_poly_add term by term:

  (K, M) = (1, 1), (5, 3), (33, 10) (a reduction inside the sum), (64, 10) (the ResNet-20 head) and
  (3, 17) (two output tiles), n = 2^12 and 512, with and without the free term;
  on the 61-bit chain with every operand at q - 1: K = 65 and K = 257, the first counts at which a
  128-bit sum that is never reduced on the way overflows (61-bit and 60-bit residues)."""
import numpy as np
import pytest

import edge_cases as E
import oracle_lib as O
import phantom_amd as PA
from gpu_util import ptr, stream, to_dev, to_host, torch

pytestmark = pytest.mark.gpu

CHAINS = {"mixed": ([60] + [50] * 6 + [60] * 3, 3), "q61": ([61] * 10, 2)}


@pytest.fixture(scope="module")
def ctxs():
    made = {}

    def get(kind, n):
        if (kind, n) not in made:
            bits, size_p = CHAINS[kind]
            made[(kind, n)] = PA.Context(n, O.coeff_modulus_create(n, bits), size_p)
        return made[(kind, n)]

    yield get
    for c in made.values():
        c.close()


def _lib():
    return PA.load()


def _vp(ts):
    return PA.ptr_array([ptr(t) for t in ts])


def _mix(ctx, chain, n, ins, coef, cadd, M):
    """runs phantom_ct_mix on ins (host [2][L][n] arrays; repeated arrays share a device copy) and the
    oracle's term-by-term sum; returns (got, want) lists of M arrays"""
    ql = ctx.ql(chain)
    L, K = len(ql), len(ins)
    dev = {}
    for x in ins:
        if id(x) not in dev:
            dev[id(x)] = to_dev(x)
    din = [dev[id(x)] for x in ins]
    douts = [to_dev(np.full(2 * L * n, 7, dtype=np.uint64)) for _ in range(M)]
    PA.check(_lib().phantom_ct_mix(ctx.handle, chain, _vp(din), K, coef.ctypes.data,
                                   cadd.ctypes.data if cadd is not None else None, _vp(douts), M, stream()))
    got = [to_host(d) for d in douts]
    mods2 = O.P(O.arr(ql + ql))
    want = []
    term = np.zeros(2 * L * n, dtype=np.uint64)
    for m in range(M):
        acc = np.zeros(2 * L * n, dtype=np.uint64)
        for k in range(K):
            sc = np.ascontiguousarray(np.tile(coef[m, k], 2))
            O.lib().or_poly_mul_scalar(O.P(ins[k]), O.P(sc), O.P(term), n, 2 * L, mods2)
            O.lib().or_poly_add(O.P(acc), O.P(term), O.P(acc), n, 2 * L, mods2)
        if cadd is not None:  # the free term on c0 only
            q = np.repeat(np.array(ql, dtype=np.uint64), n)
            s = acc[:L * n] + np.repeat(cadd[m], n)  # both below q < 2^61: no wrap
            acc[:L * n] = np.where(s >= q, s - q, s)
        want.append(acc)
    return got, want


def _residues(rng, shape, mods):
    out = np.zeros(shape + (len(mods),), dtype=np.uint64)
    for l, q in enumerate(mods):
        out[..., l] = rng.integers(0, q, size=shape, dtype=np.uint64)
    return out


@pytest.mark.parametrize("with_cadd", [False, True], ids=["plain", "cadd"])
@pytest.mark.parametrize("K,M", [(1, 1), (5, 3), (33, 10), (64, 10), (3, 17)])
@pytest.mark.parametrize("n,chain", [(1 << 12, 1), (1 << 12, 3), (512, 1)])
def test_ct_mix(ctxs, rng, n, chain, K, M, with_cadd):
    ctx = ctxs("mixed", n)
    ql = ctx.ql(chain)
    pool = [np.concatenate([O.random_limbs(rng, n, ql) for _ in range(2)]) for _ in range(min(K, 9))]
    ins = [pool[(5 * k + 1) % len(pool)] for k in range(K)]
    coef = _residues(rng, (M, K), ql)
    cadd = _residues(rng, (M,), ql) if with_cadd else None
    got, want = _mix(ctx, chain, n, ins, coef, cadd, M)
    for m in range(M):
        assert want[m].any() and np.array_equal(got[m], want[m]), (n, chain, K, M, m)


def test_overflow_counts():
    """what the kernel must survive: 65 (257) products of q - 1 do not fit 128 bits, 64 (256) do; a sum
    reduced every 32 terms stays below 2^128"""
    q = E.prime_below(1 << 61, 1 << 12)
    assert 64 * (q - 1) ** 2 < 1 << 128 <= 65 * (q - 1) ** 2
    assert (q - 1) + 32 * (q - 1) ** 2 < 1 << 128
    q = E.prime_below(1 << 60, 1 << 12)
    assert 256 * (q - 1) ** 2 < 1 << 128 <= 257 * (q - 1) ** 2


@pytest.mark.parametrize("K", [64, 65, 256, 257])
@pytest.mark.parametrize("n", [1 << 12, 512])
def test_ct_mix_max_operands(ctxs, n, K):
    """every input word and every coefficient at q - 1 on the 61-bit chain: sum_k (q - 1)^2 = K (mod q)"""
    ctx, chain, M = ctxs("q61", n), 1, 2
    ql = ctx.ql(chain)
    assert min(ql) > 1 << 60
    a = np.concatenate([E.edge_limbs(n, ql, "max")] * 2)
    coef = np.tile(np.array(ql, dtype=np.uint64) - np.uint64(1), (M, K, 1))
    got, want = _mix(ctx, chain, n, [a] * K, coef, None, M)
    for m in range(M):
        assert np.all(want[m] == np.uint64(K))
        assert np.array_equal(got[m], want[m]), (n, K, m)


def test_ct_mix_refused(ctxs, rng):
    """status 1 and the outputs untouched"""
    n, chain = 1 << 12, 1
    ctx = ctxs("mixed", n)
    ql = ctx.ql(chain)
    ins = [to_dev(np.concatenate([O.random_limbs(rng, n, ql) for _ in range(2)])) for _ in range(2)]
    outs = [to_dev(np.full(2 * len(ql) * n, 7, dtype=np.uint64)) for _ in range(2)]
    coef = _residues(rng, (2, 2), ql)
    holes = PA.ptr_array([ptr(ins[0]), 0])
    lib, s = _lib(), stream()

    def call(c=ctx.handle, ch=chain, i=_vp(ins), K=2, cf=coef.ctypes.data, o=_vp(outs), M=2):
        return lib.phantom_ct_mix(c, ch, i, K, cf, None, o, M, s)

    bad = [call(c=None), call(i=None), call(cf=None), call(o=None), call(K=0), call(M=0), call(ch=0),
           call(ch=ctx.size_Q + 1), call(i=holes), call(o=holes)]
    assert bad == [1] * len(bad), bad
    torch().cuda.synchronize()
    for o in outs:
        assert bool((to_host(o) == 7).all())
