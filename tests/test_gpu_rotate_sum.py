"""phantom_rotate_sum_ext (keyswitch_rotate_sum: the hoisted rotate-and-sum in one launch) on the GPU,
bit-exact against the CPU oracle: the value is the modular sum (or_poly_add) of or_fast_rotation_ext
(add_first = 1) per entry and or_keyswitch_ext for the identity term.

  n = 2^12 (four 1024-index blocks) and n = 512 (one block of n indices, the any-size kernel);
  a mixed 60 / 50-bit chain, a 60-bit chain and a 61-bit chain, at the top level and at a lower one
  (the special primes' table rows then differ from their buffer rows);
  beta 1, 2, 3, 4 (the register-resident kernels) and 5 (the generic loop);
  1, 2, 7 and 63 entries, with and without the identity;
  digits and keys at q - 1 and with their low halves all ones (tests/edge_cases.py).

Operands are uniform random residues or edge patterns (parity is a property of the arithmetic, not of
key or ciphertext structure)."""
import ctypes

import numpy as np
import pytest

import edge_cases as E
import oracle_lib as O
import phantom_amd as PA
from gpu_util import ptr, stream, to_dev, to_host

pytestmark = pytest.mark.gpu

CHAINS = {"mixed": ([60] + [50] * 6 + [60] * 3, 3), "q60": ([60] * 10, 2), "q61": ([61] * 10, 2),
          "b5": ([60] * 12, 2)}  # b5: 10 + 2 moduli, five digits at the top level


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


def _vp(addrs):
    return PA.ptr_array(list(addrs))


def _fill(rng, pattern, mods, polys, n):
    if pattern == "random":
        return np.concatenate([O.random_limbs(rng, n, mods) for _ in range(polys)])
    return np.concatenate([E.edge_limbs(n, mods, pattern, rng) for _ in range(polys)])


def _run(rng, ctx, n, chain, count, identity, pair=("random", "random")):
    """phantom_rotate_sum_ext and the oracle's sum; three key sets shared round robin, distinct
    Galois elements, the last a conjugation"""
    ql = ctx.ql(chain)
    em = ql + ctx.moduli[ctx.size_Q:]
    beta, dnum = -(-len(ql) // ctx.size_P), -(-ctx.size_Q // ctx.size_P)
    ct = _fill(rng, pair[0], ql, 2, n)
    digits = _fill(rng, pair[0], em, beta, n)
    keys = [[_fill(rng, pair[1], ctx.moduli, 2, n) for _ in range(dnum)] for _ in range(3)]
    dkeys = [[to_dev(x) for x in ks] for ks in keys]
    elts = [pow(5, 3 * k + 1, 2 * n) for k in range(count)]
    elts[-1] = 2 * n - 1
    key_arrays = [_vp(ptr(x) for x in dkeys[k % 3]) for k in range(count)]
    kk = (ctypes.POINTER(ctypes.c_void_p) * count)(*[ctypes.cast(a, ctypes.POINTER(ctypes.c_void_p)) for a in key_arrays])
    el = (ctypes.c_uint32 * count)(*elts)
    W = 2 * len(em) * n
    dct, ddig, dout = to_dev(ct), to_dev(digits), to_dev(np.full(W, 5, dtype=np.uint64))
    PA.check(_lib().phantom_rotate_sum_ext(ctx.handle, chain, ptr(dct), ptr(ddig), kk, dnum, el, count, identity,
                                           ptr(dout), stream()))
    got = to_host(dout)
    mods, em2 = O.P(O.arr(ctx.moduli)), O.P(O.arr(em + em))
    want = np.zeros(W, dtype=np.uint64)
    if identity:
        O.lib().or_keyswitch_ext(O.P(ct), O.P(want), n, len(ql), ctx.size_Q, ctx.size_P, mods)
    term = np.zeros(W, dtype=np.uint64)
    for k in range(count):
        O.lib().or_fast_rotation_ext(O.P(ct), O.P(digits), O.ptrs(keys[k % 3]), elts[k], 1, O.P(term), n, len(ql),
                                     ctx.size_Q, ctx.size_P, mods)
        O.lib().or_poly_add(O.P(want), O.P(term), O.P(want), n, 2 * len(em), em2)
    return got, want, beta


# (chain kind, n, chain index, beta, entries, identity)
CASES = [("mixed", 1 << 12, 1, 3, 7, 1), ("mixed", 1 << 12, 3, 2, 2, 0), ("mixed", 1 << 12, 3, 2, 63, 1),
         ("q60", 1 << 12, 1, 4, 63, 1), ("q60", 1 << 12, 1, 4, 1, 0), ("q60", 1 << 12, 7, 1, 1, 1),
         ("q60", 1 << 12, 7, 1, 7, 0), ("q61", 1 << 12, 1, 4, 7, 0), ("q61", 1 << 12, 4, 3, 2, 1),
         ("b5", 1 << 12, 1, 5, 7, 1), ("b5", 1 << 12, 2, 5, 2, 0), ("mixed", 512, 1, 3, 63, 1),
         ("mixed", 512, 3, 2, 1, 0), ("q60", 512, 1, 4, 7, 0), ("q60", 512, 7, 1, 2, 1), ("b5", 512, 1, 5, 7, 1)]


@pytest.mark.parametrize("kind,n,chain,beta,count,identity", CASES)
def test_rotate_sum(ctxs, rng, kind, n, chain, beta, count, identity):
    got, want, b = _run(rng, ctxs(kind, n), n, chain, count, identity)
    assert b == beta
    assert want.any() and np.array_equal(got, want), (kind, n, chain, count, identity)


def test_partial_sum_bounds():
    """what the register-resident kernels rely on, in exact integers: with operands split at 30 bits
    (low half below 2^30, high half (q - 1) >> 30 at most), the three partial sums of beta <= 4
    products fit 64 bits for every modulus below 2^61, and the fifth product does not; the exact
    reduction's three lazy residues (each below 2 q) sum below 2^64"""
    n = 1 << 12
    q = E.prime_below(1 << 61, n)
    assert q > 1 << 60
    lo, hi = (1 << 30) - 1, (q - 1) >> 30
    assert hi < 1 << 31
    for beta in (1, 2, 3, 4):
        assert beta * lo * lo < 1 << 64        # ll
        assert beta * 2 * lo * hi < 1 << 64    # mm: two cross products per term
        assert beta * hi * hi < 1 << 64        # hh
    assert 5 * 2 * lo * hi >= 1 << 64          # beta = 5 takes the 128-bit sums
    assert 3 * (2 * q - 1) < 1 << 64
    # the maximal operands reach the bound: q - 1 itself has the maximal high half
    assert (q - 1) >> 30 == hi and E.lowmax(q) & lo == lo
    # the generic kernel's 128-bit sum holds 64 products of 61-bit residues: beta <= 64 there
    assert 64 * (q - 1) ** 2 < 1 << 128


@pytest.mark.parametrize("pair", [("max", "max"), ("lowmax", "lowmax"), ("max", "lowmax")], ids="-".join)
@pytest.mark.parametrize("kind,n,chain", [("q61", 1 << 12, 1), ("q60", 1 << 12, 1), ("mixed", 1 << 12, 1),
                                          ("q61", 512, 1), ("b5", 1 << 12, 1)])
def test_rotate_sum_edges(ctxs, rng, kind, n, chain, pair):
    """digits, ct and keys at q - 1 / low halves all ones: beta = 4 at 61 and 60 bits (sums next to
    2^64), beta = 3 on the mixed chain, the 128-bit sums at n = 512 and at beta = 5"""
    got, want, _ = _run(rng, ctxs(kind, n), n, chain, 7, 1, pair)
    assert np.array_equal(got, want), (kind, n, pair)


def test_rotate_sum_refused(ctxs, rng):
    """status 1 and the output untouched: a null pointer, a null key, 0 or 64 entries, a bad chain
    index, no special prime"""
    t_n, chain, count = 1 << 12, 1, 2
    ctx = ctxs("q60", t_n)
    ql = ctx.ql(chain)
    em = ql + ctx.moduli[ctx.size_Q:]
    beta, dnum = -(-len(ql) // ctx.size_P), -(-ctx.size_Q // ctx.size_P)
    dct, ddig = to_dev(_fill(rng, "random", ql, 2, t_n)), to_dev(_fill(rng, "random", em, beta, t_n))
    dkeys = [to_dev(_fill(rng, "random", ctx.moduli, 2, t_n)) for _ in range(dnum)]
    arr = _vp(ptr(x) for x in dkeys)
    mk = lambda items: (ctypes.POINTER(ctypes.c_void_p) * len(items))(*items)
    cast = ctypes.cast(arr, ctypes.POINTER(ctypes.c_void_p))
    kk, nokey, many = mk([cast] * count), mk([cast, None]), mk([cast] * 64)
    el, el64 = (ctypes.c_uint32 * count)(5, 25), (ctypes.c_uint32 * 64)(*[pow(5, k + 1, 2 * t_n) for k in range(64)])
    dout = to_dev(np.full(2 * len(em) * t_n, 7, dtype=np.uint64))
    nop = PA.Context(t_n, PA.coeff_modulus_create(t_n, [60, 50, 50]), 0)
    last = ctx.size_Q + 1
    lib, s = _lib(), stream()

    def call(c=ctx, ch=chain, ct=ptr(dct), dg=ptr(ddig), keys=kk, e=el, cnt=count, out=ptr(dout)):
        return lib.phantom_rotate_sum_ext(c.handle, ch, ct, dg, keys, dnum, e, cnt, 1, out, s)

    bad = [call(ct=None), call(dg=None), call(keys=None), call(e=None), call(out=None), call(keys=nokey), call(cnt=0),
           call(keys=many, e=el64, cnt=64), call(ch=0), call(ch=last), call(c=nop),
           lib.phantom_rotate_sum_ext(None, chain, ptr(dct), ptr(ddig), kk, dnum, el, count, 1, ptr(dout), s)]
    assert bad == [1] * len(bad), bad
    assert bool((to_host(dout) == 7).all())
    nop.close()
