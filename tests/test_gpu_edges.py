"""GPU kernels at the edges of their lazy-reduction and quotient bounds, bit-exact against the CPU
oracle (every assertion is np.array_equal with the oracle call of that operation).

The rest of the suite draws uniform random residues, which sit around half of every worst case.
Here the operands are the patterns of tests/edge_cases.py (max = q - 1, lowmax = low 30 bits all
ones, stripes, impulse, alt, sums within one of a multiple of q) and the moduli sit at the regime
edges: the largest 60-bit primes (16 / 8 products per split partial sum, the 16q lazy ranges and
the approximate-quotient reductions), 61-bit primes (4 products, the 8q ranges, the exact
reductions), a mixed 60 / 50-bit chain, and for the NTT the primes on either side of 2^50 and 2^60
with a 30-bit one.  tests/test_arith_bounds.py shows on the CPU that these patterns reach at least
half of each stated bound.  N = 4096 unless a kernel needs another size; contexts are 8 + 2 moduli
(the mixed chain 7 + 3) as test_lt_bsgs_moduli builds them."""
import ctypes
import os
import subprocess
import sys

import numpy as np
import pytest

import edge_cases as E
import ks_oracle as KO
import oracle_lib as O
import phantom_amd as PA
from gpu_util import ptr, stream, to_dev, to_host, torch

pytestmark = pytest.mark.gpu

N = 4096
PAIRS = [("max", "max"), ("lowmax", "lowmax"), ("max", "lowmax"), ("stripes", "random")]
PAIR_IDS = ["-".join(p) for p in PAIRS]
NEAR = [("near", "max"), ("near", "lowmax")]
CHAINS = {"q60": ([60] * 10, 2), "q61": ([61] * 10, 2), "mixed": ([60] + [50] * 6 + [60] * 3, 3),
          "wide5": ([61] * 13, 5)}  # 61-bit digits of 5 limbs: more than the 4 products a split sum holds
# chain indices: the top level and a level whose last digit is partial
LEVELS = {"q60": (1, 2), "q61": (1, 2), "mixed": (1, 3)}


@pytest.fixture(scope="module")
def ctxs():
    made = {}

    def get(kind, n=N):
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


def _fill(rng, pattern, mods, polys=1, n=N):
    """[polys][L][n] at `pattern` (an edge_cases pattern or "random")"""
    if pattern == "random":
        return np.concatenate([O.random_limbs(rng, n, mods) for _ in range(polys)])
    return np.concatenate([E.edge_limbs(n, mods, pattern, rng) for _ in range(polys)])


def _rolled(a, n, shift):
    """every limb row rotated by `shift` coefficients (rows keep their modulus)"""
    return np.ascontiguousarray(np.roll(a.reshape(-1, n), shift, axis=1)).reshape(-1)


class _Dev:
    """device copies of host arrays, one per distinct array (constant patterns repeat one array)"""

    def __init__(self):
        self.made = {}

    def __call__(self, a):
        if id(a) not in self.made:
            self.made[id(a)] = (a, to_dev(a))
        return self.made[id(a)][1]


def _lt_operands(rng, em, g, b, pair, n=N):
    """g babies [2][L][n] and g b plaintexts [L][n] (row i: the plaintexts of giant step i)"""
    pa, pb = pair
    if pa == "near":
        # every inner sum is -1, 0 or 1 modulo q (coefficient k: (k mod 3) - 1), the babies and all but
        # the last plaintext of a giant step at max / lowmax, the last plaintext solved for
        baby = _fill(rng, pb, em, 2, n)
        fills = [_fill(rng, f, em, 1, n) for f in ("max", "lowmax")]
        pts = []
        for i in range(b):
            fb = ("max", "lowmax")[i % 2]
            last = np.zeros(len(em) * n, dtype=np.uint64)
            for l, q in enumerate(em):
                for t in (-1, 0, 1):
                    last[l * n + (t + 1):(l + 1) * n:3] = E.near_multiple_operands(q, g, t, pb, fb)[1][-1]
            pts += [fills[i % 2]] * (g - 1) + [last]
        return [baby] * g, pts
    if pa == "stripes":
        base = _fill(rng, pa, em, 2, n)
        babies = [_rolled(base, n, j) for j in range(g)]
    else:
        babies = [_fill(rng, pa, em, 2, n)] * g
    if pb == "random":
        pool = [_fill(rng, pb, em, 1, n) for _ in range(8)]
        pts = [pool[(5 * k + k // g) % 8] for k in range(g * b)]
    else:
        pts = [_fill(rng, pb, em, 1, n)] * (g * b)
    return babies, pts


def _near_check(want, em, n):
    """the oracle's inner sums of a `near` case are the targets themselves"""
    for w in want:
        rows = w.reshape(2, len(em), n)
        for l, q in enumerate(em):
            for t in (-1, 0, 1):
                assert np.all(rows[:, l, (t + 1)::3] == np.uint64(t % q))


# ---- inner sums ----------------------------------------------------------------------------

@pytest.mark.parametrize("pair", PAIRS + NEAR, ids=PAIR_IDS + ["near-max", "near-lowmax"])
@pytest.mark.parametrize("g,b", [(32, 8), (16, 4)])
@pytest.mark.parametrize("kind", ["q60", "q61"])
def test_lt_bsgs_edges(ctxs, rng, kind, g, b, pair):
    """phantom_lt_bsgs (lt_bsgs_tile at g 32, lt_bsgs_kernel at g 16) == or_lt_bsgs with every
    30-bit half at its maximum: 8 / 16 products per partial sum below 2^60, 4 at 61 bits"""
    ctx, chain = ctxs(kind), 1
    em = ctx.ql(chain) + ctx.moduli[ctx.size_Q:]
    babies, pts = _lt_operands(rng, em, g, b, pair)
    dev = _Dev()
    db, dp = [dev(x) for x in babies], [dev(x) for x in pts]
    douts = [to_dev(np.full(2 * len(em) * N, 5, dtype=np.uint64)) for _ in range(b)]
    PA.check(_lib().phantom_lt_bsgs(ctx.handle, chain, _vp(ptr(x) for x in db), g, _vp(ptr(x) for x in dp), b,
                                    _vp(ptr(x) for x in douts), stream()))
    want = [np.zeros(2 * len(em) * N, dtype=np.uint64) for _ in range(b)]
    O.lib().or_lt_bsgs(O.ptrs(babies), g, O.ptrs(pts), b, O.ptrs(want), N, len(ctx.ql(chain)), ctx.size_Q, ctx.size_P,
                       O.P(O.arr(ctx.moduli)))
    if pair[0] == "near":
        _near_check(want, em, N)
    for i in range(b):
        assert np.array_equal(to_host(douts[i]), want[i]), (kind, pair, i)


@pytest.mark.parametrize("pair", PAIRS + NEAR, ids=PAIR_IDS + ["near-max", "near-lowmax"])
@pytest.mark.parametrize("b,group", [(8, 2), (3, 3)])
@pytest.mark.parametrize("kind", ["q60", "q61"])
def test_lt_bsgs_group_edges(ctxs, rng, kind, b, group, pair):
    """phantom_lt_bsgs_group == or_lt_bsgs per ciphertext; ciphertext c takes the baby pattern of
    the pair c places on (the plaintexts are shared)"""
    ctx, chain, g = ctxs(kind), 1, 32
    em = ctx.ql(chain) + ctx.moduli[ctx.size_Q:]
    W = 2 * len(em) * N
    babies = []
    for c in range(group):
        pc = pair if pair[0] == "near" else (PAIRS[(PAIRS.index(pair) + c) % len(PAIRS)][0], pair[1])
        bs, pts_c = _lt_operands(rng, em, g, b, pc)
        babies.append(bs)
        if c == 0:
            pts = pts_c
    dev = _Dev()
    dpts = [dev(x) for x in pts]
    dbabies = [torch().cat([dev(x) for x in bs]) for bs in babies]  # contiguous, stride W
    dacc = [to_dev(np.full(W, 3, dtype=np.uint64)) for _ in range(group)]
    dgiant = [to_dev(np.full(max(b - 1, 1) * W, 9, dtype=np.uint64)) for _ in range(group)]
    PA.check(_lib().phantom_lt_bsgs_group(ctx.handle, chain, group, _vp(ptr(x) for x in dbabies), W, g,
                                          _vp(ptr(x) for x in dpts), b, _vp(ptr(x) for x in dacc),
                                          _vp(ptr(x) for x in dgiant), W, stream()))
    mods = O.P(O.arr(ctx.moduli))
    for c in range(group):
        want = [np.zeros(W, dtype=np.uint64) for _ in range(b)]
        O.lib().or_lt_bsgs(O.ptrs(babies[c]), g, O.ptrs(pts), b, O.ptrs(want), N, len(ctx.ql(chain)), ctx.size_Q,
                           ctx.size_P, mods)
        if pair[0] == "near":
            _near_check(want, em, N)
        assert np.array_equal(to_host(dacc[c]), want[0]), (kind, pair, c, 0)
        giants = to_host(dgiant[c])
        for i in range(1, b):
            assert np.array_equal(giants[(i - 1) * W:i * W], want[i]), (kind, pair, c, i)


# ---- batched rotations -----------------------------------------------------------------------

def _rotation_case(rng, ctx, n, chain, pair, group, count=3):
    """digits, ct at pair[0]; the keys at pair[1]; entry 0 is the identity, the last a conjugation"""
    pa, pb = pair
    ql = ctx.ql(chain)
    em = ql + ctx.moduli[ctx.size_Q:]
    beta = -(-len(ql) // ctx.size_P)
    dnum = -(-ctx.size_Q // ctx.size_P)
    cts = [_rolled(_fill(rng, pa, ql, 2, n), n, 3 * c) for c in range(group)]
    digits = [_rolled(_fill(rng, pa, em, beta, n), n, 5 * c) for c in range(group)]
    keys = [[_fill(rng, pb, ctx.moduli, 2, n) for _ in range(dnum)] for _ in range(2)]
    elts = [pow(5, 3 * k + 1, 2 * n) for k in range(count)]
    elts[-1] = 2 * n - 1
    return ql, em, beta, dnum, cts, digits, keys, elts


def _rotation_want(ctx, n, ql, em, ct, digits, keys, elts, k):
    want = np.zeros(2 * len(em) * n, dtype=np.uint64)
    mods = O.P(O.arr(ctx.moduli))
    if k == 0:
        O.lib().or_keyswitch_ext(O.P(ct), O.P(want), n, len(ql), ctx.size_Q, ctx.size_P, mods)
    else:
        O.lib().or_fast_rotation_ext(O.P(ct), O.P(digits), O.ptrs(keys[k % 2]), elts[k], 1, O.P(want), n, len(ql),
                                     ctx.size_Q, ctx.size_P, mods)
    return want


def _key_table(dkeys, count):
    key_arrays = [None if k == 0 else _vp(ptr(x) for x in dkeys[k % 2]) for k in range(count)]
    kk = (ctypes.POINTER(ctypes.c_void_p) * count)(*[ctypes.cast(a, ctypes.POINTER(ctypes.c_void_p)) if a is not None
                                                     else None for a in key_arrays])
    return key_arrays, kk


@pytest.mark.parametrize("pair", PAIRS, ids=PAIR_IDS)
@pytest.mark.parametrize("shape", ["q60", "q61", "n512"])
def test_fast_rotation_ext_batch_edges(ctxs, rng, shape, pair):
    """phantom_fast_rotation_ext_batch at beta = 4: the full kernel (split sums, exact reduction)
    at 60 and 61 bits, the any-size kernel (128-bit sums) at n = 512; one identity entry"""
    n = 512 if shape == "n512" else N
    ctx = ctxs("q60" if shape == "n512" else shape, n)
    chain, count = 1, 3
    ql, em, beta, dnum, cts, digits, keys, elts = _rotation_case(rng, ctx, n, chain, pair, 1, count)
    assert beta == 4
    dkeys = [[to_dev(x) for x in ks] for ks in keys]
    dct, ddig = to_dev(cts[0]), to_dev(digits[0])
    douts = [to_dev(np.full(2 * len(em) * n, 5, dtype=np.uint64)) for _ in range(count)]
    key_arrays, kk = _key_table(dkeys, count)
    el = (ctypes.c_uint32 * count)(*elts)
    PA.check(_lib().phantom_fast_rotation_ext_batch(ctx.handle, chain, ptr(dct), ptr(ddig), kk, dnum, el, count,
                                                    _vp(ptr(x) for x in douts), stream()))
    for k in range(count):
        want = _rotation_want(ctx, n, ql, em, cts[0], digits[0], keys, elts, k)
        assert np.array_equal(to_host(douts[k]), want), (shape, pair, k)


@pytest.mark.parametrize("pair", PAIRS, ids=PAIR_IDS)
@pytest.mark.parametrize("kind,chain", [("q60", 1), ("q60", 2), ("q61", 1), ("mixed", 1)])
def test_fast_rotation_ext_batch_group_edges(ctxs, rng, kind, chain, pair):
    """phantom_fast_rotation_ext_batch_group: below 2^60 the approximate-quotient reduction
    (split_reduce2: sums up to 2^62, 2^63, 2^62 at beta = 4; the mixed chain's 50-bit limbs have a
    generic 2^60 mod q), at 61 bits the exact one with sums up to 2^64"""
    ctx, group, count = ctxs(kind), 2, 3
    ql, em, beta, dnum, cts, digits, keys, elts = _rotation_case(rng, ctx, N, chain, pair, group, count)
    W = 2 * len(em) * N
    dkeys = [[to_dev(x) for x in ks] for ks in keys]
    dcts, ddig = [to_dev(x) for x in cts], [to_dev(x) for x in digits]
    douts = [to_dev(np.full(count * W, 5, dtype=np.uint64)) for _ in range(group)]
    key_arrays, kk = _key_table(dkeys, count)
    el = (ctypes.c_uint32 * count)(*elts)
    outs = [ptr(douts[c]) + 8 * k * W for c in range(group) for k in range(count)]
    PA.check(_lib().phantom_fast_rotation_ext_batch_group(ctx.handle, chain, group, _vp(ptr(x) for x in dcts),
                                                          _vp(ptr(x) for x in ddig), kk, dnum, el, count, _vp(outs),
                                                          stream()))
    for c in range(group):
        got = to_host(douts[c])
        for k in range(count):
            want = _rotation_want(ctx, N, ql, em, cts[c], digits[c], keys, elts, k)
            assert np.array_equal(got[k * W:(k + 1) * W], want), (kind, pair, c, k)


# ---- key switch and RNS on the mixed and the 61-bit chain ---------------------------------------

KS_CASES = [(kind, lv, pat) for kind in ("mixed", "q61") for lv in (0, 1) for pat in ("max", "stripes", "impulse")]
KS_IDS = [f"{k}-{'top' if lv == 0 else 'partial'}-{p}" for k, lv, p in KS_CASES]


def _ks_setup(ctxs, kind, lv):
    ctx = ctxs(kind)
    chain = LEVELS[kind][lv]
    ql, p = ctx.ql(chain), ctx.moduli[ctx.size_Q:]
    beta = -(-len(ql) // ctx.size_P)
    if lv == 1:
        assert len(ql) % ctx.size_P != 0  # the last digit is partial
    return ctx, chain, ql, p, beta


def _ks_keys(rng, ctx, pat):
    """the keys at the operands' pattern for max (every product at its maximum), random otherwise"""
    dnum = -(-ctx.size_Q // ctx.size_P)
    keys = [_fill(rng, "max" if pat == "max" else "random", ctx.moduli, 2) for _ in range(dnum)]
    return keys, [to_dev(k) for k in keys]


@pytest.mark.parametrize("kind,lv,pat", KS_CASES, ids=KS_IDS)
def test_keyswitch_inner_prod_edges(ctxs, rng, kind, lv, pat):
    ctx, chain, ql, p, beta = _ks_setup(ctxs, kind, lv)
    qlp = ql + p
    tmu = _fill(rng, pat, qlp, beta)
    keys, dkeys = _ks_keys(rng, ctx, pat)
    dt = to_dev(tmu)
    dcx = to_dev(np.zeros(2 * len(qlp) * N, dtype=np.uint64))
    PA.check(_lib().phantom_keyswitch_inner_prod(ctx.handle, chain, ptr(dt), _vp(ptr(k) for k in dkeys), len(dkeys),
                                                 ptr(dcx), stream()))
    want = np.zeros(2 * len(qlp) * N, dtype=np.uint64)
    O.lib().or_keyswitch_inner_prod(O.P(tmu), O.ptrs(keys), O.P(want), N, len(ql), ctx.size_Q, ctx.size_P, beta,
                                    O.P(O.arr(ctx.moduli)))
    assert np.array_equal(to_host(dcx), want)


@pytest.mark.parametrize("kind,lv,pat", KS_CASES, ids=KS_IDS)
def test_relinearize_rescale_edges(ctxs, rng, kind, lv, pat):
    ctx, chain, ql, p, beta = _ks_setup(ctxs, kind, lv)
    L = len(ql)
    ct = _fill(rng, pat, ql, 3)
    keys, dkeys = _ks_keys(rng, ctx, pat)
    d = to_dev(ct)
    dout = to_dev(np.zeros(2 * (L - 1) * N, dtype=np.uint64))
    PA.check(_lib().phantom_relinearize_rescale(ctx.handle, chain, ptr(d), ptr(dout), _vp(ptr(k) for k in dkeys),
                                                len(dkeys), stream()))
    assert np.array_equal(to_host(dout), KO.relinearize_rescale(ctx, chain, ct, keys))


@pytest.mark.parametrize("kind,lv,pat", KS_CASES, ids=KS_IDS)
def test_modup_edges(ctxs, rng, kind, lv, pat):
    ctx, chain, ql, p, beta = _ks_setup(ctxs, kind, lv)
    c2 = _fill(rng, pat, ql)
    d = to_dev(c2)
    dout = to_dev(np.zeros(beta * (len(ql) + len(p)) * N, dtype=np.uint64))
    PA.check(_lib().phantom_modup(ctx.handle, chain, ptr(d), ptr(dout), stream()))
    want = np.zeros(beta * (len(ql) + len(p)) * N, dtype=np.uint64)
    O.lib().or_modup(O.P(c2), O.P(want), N, O.P(O.arr(ql)), len(ql), O.P(O.arr(p)), len(p))
    assert np.array_equal(to_host(dout), want)


@pytest.mark.parametrize("kind,lv,pat", KS_CASES, ids=KS_IDS)
def test_moddown_edges(ctxs, rng, kind, lv, pat):
    """phantom_moddown_from_ntt and phantom_moddown_rescale (the special basis {q_last} u P)"""
    ctx, chain, ql, p, beta = _ks_setup(ctxs, kind, lv)
    cxs = [_rolled(_fill(rng, pat, ql + p), N, 7 * t) for t in range(2)]
    d = to_dev(cxs[0])
    dout = to_dev(np.zeros(len(ql) * N, dtype=np.uint64))
    PA.check(_lib().phantom_moddown_from_ntt(ctx.handle, chain, ptr(d), ptr(dout), stream()))
    want = np.zeros(len(ql) * N, dtype=np.uint64)
    O.lib().or_moddown_from_ntt(O.P(cxs[0].copy()), O.P(want), N, O.P(O.arr(ql)), len(ql), O.P(O.arr(p)), len(p))
    assert np.array_equal(to_host(dout), want)
    d = to_dev(np.concatenate(cxs))
    dout = to_dev(np.zeros(2 * (len(ql) - 1) * N, dtype=np.uint64))
    PA.check(_lib().phantom_moddown_rescale(ctx.handle, chain, ptr(d), ptr(dout), 2, stream()))
    wants = []
    for cx in cxs:
        w = np.zeros((len(ql) - 1) * N, dtype=np.uint64)
        O.lib().or_moddown_from_ntt(O.P(cx.copy()), O.P(w), N, O.P(O.arr(ql[:-1])), len(ql) - 1,
                                    O.P(O.arr([ql[-1]] + list(p))), len(p) + 1)
        wants.append(w)
    assert np.array_equal(to_host(dout), np.concatenate(wants))


@pytest.mark.parametrize("kind,lv,pat", KS_CASES, ids=KS_IDS)
def test_rescale_edges(ctxs, rng, kind, lv, pat):
    ctx, chain, ql, p, beta = _ks_setup(ctxs, kind, lv)
    L = len(ql)
    ct = _fill(rng, pat, ql, 2)
    d = to_dev(ct)
    dout = to_dev(np.zeros(2 * (L - 1) * N, dtype=np.uint64))
    PA.check(_lib().phantom_rescale_to_next(ctx.handle, chain, ptr(d), ptr(dout), 2, stream()))
    want = np.zeros(2 * (L - 1) * N, dtype=np.uint64)
    O.lib().or_rescale_ntt(O.P(ct), O.P(want), N, L, 2, O.P(O.arr(ql)))
    assert np.array_equal(to_host(dout), want)


@pytest.mark.parametrize("pat", ["max", "stripes"])
@pytest.mark.parametrize("chain", [1, 3])
def test_wide_digits_edges(ctxs, rng, chain, pat):
    """a 61-bit chain with digits of 5 limbs (8 + 5 moduli; digits 5 + 3 and 5 + 1): every base
    conversion of the key switch has more 61-bit input limbs than the 4 products a 30-bit-split
    partial sum holds, whichever kernel runs it (the matrix cores by default; the VALU kernels and
    the NTT's fused prologue under the switches of test_knobs_on_61_bit_chains).  modup, moddown,
    moddown + rescale and relinearize + rescale == the oracle."""
    ctx = ctxs("wide5")
    ql, p = ctx.ql(chain), ctx.moduli[ctx.size_Q:]
    L, beta = len(ql), -(-len(ql) // ctx.size_P)
    c2 = _fill(rng, pat, ql)
    d = to_dev(c2)
    dout = to_dev(np.zeros(beta * (L + len(p)) * N, dtype=np.uint64))
    PA.check(_lib().phantom_modup(ctx.handle, chain, ptr(d), ptr(dout), stream()))
    want = np.zeros(beta * (L + len(p)) * N, dtype=np.uint64)
    O.lib().or_modup(O.P(c2), O.P(want), N, O.P(O.arr(ql)), L, O.P(O.arr(p)), len(p))
    assert np.array_equal(to_host(dout), want), "modup"
    cxs = [_rolled(_fill(rng, pat, ql + p), N, 7 * t) for t in range(2)]
    d = to_dev(cxs[0])
    dout = to_dev(np.zeros(L * N, dtype=np.uint64))
    PA.check(_lib().phantom_moddown_from_ntt(ctx.handle, chain, ptr(d), ptr(dout), stream()))
    want = np.zeros(L * N, dtype=np.uint64)
    O.lib().or_moddown_from_ntt(O.P(cxs[0].copy()), O.P(want), N, O.P(O.arr(ql)), L, O.P(O.arr(p)), len(p))
    assert np.array_equal(to_host(dout), want), "moddown"
    d = to_dev(np.concatenate(cxs))
    dout = to_dev(np.zeros(2 * (L - 1) * N, dtype=np.uint64))
    PA.check(_lib().phantom_moddown_rescale(ctx.handle, chain, ptr(d), ptr(dout), 2, stream()))
    wants = []
    for cx in cxs:
        w = np.zeros((L - 1) * N, dtype=np.uint64)
        O.lib().or_moddown_from_ntt(O.P(cx.copy()), O.P(w), N, O.P(O.arr(ql[:-1])), L - 1,
                                    O.P(O.arr([ql[-1]] + list(p))), len(p) + 1)
        wants.append(w)
    assert np.array_equal(to_host(dout), np.concatenate(wants)), "moddown + rescale"
    ct = _fill(rng, pat, ql, 3)
    keys, dkeys = _ks_keys(rng, ctx, pat)
    d = to_dev(ct)
    dout = to_dev(np.zeros(2 * (L - 1) * N, dtype=np.uint64))
    PA.check(_lib().phantom_relinearize_rescale(ctx.handle, chain, ptr(d), ptr(dout), _vp(ptr(k) for k in dkeys),
                                                len(dkeys), stream()))
    assert np.array_equal(to_host(dout), KO.relinearize_rescale(ctx, chain, ct, keys)), "relinearize + rescale"


@pytest.mark.parametrize("knob,select", [
    ("PHX_FUSED_BCONV", "wide_digits_edges or ((modup_edges or moddown_edges or relinearize_rescale_edges) and q61)"),
    ("PHX_BCONV_MFMA", "wide_digits_edges or bconv_edges")], ids=["fused_prologue", "valu_only"])
def test_knobs_on_61_bit_chains(knob, select):
    """the base conversions of the tests above through the code the runtime switches select (each is
    read once per process, so a child process runs them): PHX_FUSED_BCONV=1, the conversion as the
    NTT column pass's prologue, which 61-bit digits of more than 4 limbs must not take (2-limb
    digits do), and PHX_BCONV_MFMA=0, every conversion on the VALU kernels (bconv_fixed_kernel up to
    the number of products its sums hold, the 128-bit kernel above)"""
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    env = dict(os.environ, **{knob: "1" if knob == "PHX_FUSED_BCONV" else "0"})
    cmd = [sys.executable, "-m", "pytest", "-q", "-m", "gpu", "-p", "no:cacheprovider", "tests/test_gpu_edges.py",
           "-k", select]
    out = subprocess.run(cmd, cwd=root, env=env, capture_output=True, text=True, timeout=300)
    tail = (out.stdout + out.stderr)[-3000:]
    assert out.returncode == 0, tail
    assert " passed" in out.stdout and " failed" not in out.stdout, tail


# ---- base conversion ---------------------------------------------------------------------------

def _digit_extremes(q):
    """residues whose bytes are the extreme signed base-256 digits (0x7F: +127, 0x80: -128 and a
    carry), the top byte as large as q allows"""
    out = []
    k = (q.bit_length() - 1) // 8  # whole bytes below the top one
    for byte in (0x7F, 0x80):
        v = int.from_bytes(bytes([byte]) * k, "little") | min(byte, q >> (8 * k)) << (8 * k)
        out.append(v if v < q else v - (1 << (8 * k)))
    return out


# (ibase bits, obase bits): bconv_fixed_kernel at its static limit (obase > 64 keeps the matrix
# cores out), the 128-bit kernel, two matrix-core shapes of test_gpu_bconv.SHAPES, and 61-bit
# moduli, whose 30-bit-split sums hold 4 products on both sides and 8 on one side only (there the
# wide side's cross sum wraps, not the high-by-high one: bconv_split_terms)
BCONV_SHAPES = [([60] * 15, [60] * 65), ([60] * 16, [60] * 65), ([60] * 16, [60] * 64), ([50] * 15, [50] * 45),
                ([61] * 15, [61] * 65), ([61] * 5, [61] * 66), ([61] * 4, [61] * 65), ([61] * 9, [60] * 66),
                ([61] * 15, [50] * 65), ([50] * 15, [61] * 65), ([61] * 8, [50] * 66), ([30] * 9, [61] * 65)]


@pytest.mark.parametrize("prescale", [0, 1])
@pytest.mark.parametrize("ib_bits,ob_bits", BCONV_SHAPES, ids=lambda b: f"{b[0]}x{len(b)}")
def test_bconv_edges(ib_bits, ob_bits, prescale):
    """phantom_fast_bconv and phantom_bconv_run == or_bconv with the converted values t (the
    inputs themselves at prescale = 0, [x qHat^-1] at prescale = 1, x = t qHat chosen so) at
    q - 1, lowmax and the extreme signed digits"""
    mods = O.coeff_modulus_create(N, ib_bits + ob_bits)
    ibase, obase = mods[:len(ib_bits)], mods[len(ib_bits):]
    ib_arr, ob_arr = O.arr(ibase), O.arr(obase)
    t = np.zeros(len(ibase) * N, dtype=np.uint64)
    for i, q in enumerate(ibase):
        vals = [q - 1, E.lowmax(q)] + _digit_extremes(q) + [q - 2, 0, (q - 1) // 2]
        for k, v in enumerate(vals):
            t[i * N + k:(i + 1) * N:len(vals)] = v
    t[:N // 2] = ibase[0] - 1  # and half of the first limb constant
    qhat = []
    for i, q in enumerate(ibase):
        prod = 1
        for k, qk in enumerate(ibase):
            if k != i:
                prod = prod * qk % q
        qhat.append(prod)
    x_oracle = np.zeros_like(t)  # or_bconv prescales by qHat^-1: t qHat gives back t
    O.lib().or_poly_mul_scalar(O.P(t), O.P(O.arr(qhat)), O.P(x_oracle), N, len(ibase), O.P(ib_arr))
    want = np.zeros(len(obase) * N, dtype=np.uint64)
    O.lib().or_bconv(O.P(x_oracle), O.P(want), N, O.P(ib_arr), len(ibase), O.P(ob_arr), len(obase))
    sentinel = np.uint64(0xDEADBEEFCAFEF00D)
    d_in = to_dev(x_oracle if prescale else t)
    d_out = to_dev(np.full((len(obase) + 1) * N, sentinel, dtype=np.uint64))
    lib = _lib()
    PA.check(lib.phantom_fast_bconv(ib_arr.ctypes.data_as(PA.u64p), len(ibase), ob_arr.ctypes.data_as(PA.u64p),
                                    len(obase), ptr(d_in), ptr(d_out), N, prescale, stream()))
    got = to_host(d_out)
    assert np.all(got[len(obase) * N:] == sentinel), "write past obase"
    assert np.array_equal(got[:len(obase) * N], want)
    h = PA.vp()
    PA.check(lib.phantom_bconv_create(ib_arr.ctypes.data_as(PA.u64p), len(ibase), ob_arr.ctypes.data_as(PA.u64p),
                                      len(obase), stream(), ctypes.byref(h)))
    try:
        d_out2 = to_dev(np.full((len(obase) + 1) * N, sentinel, dtype=np.uint64))
        PA.check(lib.phantom_bconv_run(h, ptr(d_in), ptr(d_out2), N, prescale, stream()))
        got2 = to_host(d_out2)
        assert np.all(got2[len(obase) * N:] == sentinel), "write past obase"
        assert np.array_equal(got2[:len(obase) * N], want)
    finally:
        PA.check(lib.phantom_bconv_destroy(h))


# ---- element-wise ------------------------------------------------------------------------------

@pytest.mark.parametrize("pat", ["max", "lowmax"])
@pytest.mark.parametrize("kind", ["q60", "q61"])
def test_multiply_and_tensor_lin_edges(ctxs, rng, kind, pat):
    """phantom_multiply, phantom_tensor_lin and phantom_tensor_lin_batch (factors 2 and 3) with
    operands, factors and constants at q - 1 (`pat`: the operands)"""
    ctx, chain = ctxs(kind), 2
    ql = ctx.ql(chain)
    L = len(ql)
    mods = O.arr(ql)
    a, b = _fill(rng, pat, ql, 2), _fill(rng, "max", ql, 2)
    tl = ctx.ql(chain - 1)  # a term with more limbs than the product
    t = _fill(rng, pat, tl, 2)
    qm1 = O.arr([q - 1 for q in ql])
    da, db, dt = to_dev(a), to_dev(b), to_dev(t)
    dout = to_dev(np.zeros(3 * L * N, dtype=np.uint64))
    PA.check(_lib().phantom_multiply(ctx.handle, chain, ptr(da), ptr(db), ptr(dout), stream()))
    want = np.zeros(3 * L * N, dtype=np.uint64)
    O.lib().or_tensor_prod_2x2(O.P(a), O.P(b), O.P(want), N, L, O.P(mods))
    assert np.array_equal(to_host(dout), want)
    dout = to_dev(np.zeros(3 * L * N, dtype=np.uint64))
    PA.check(_lib().phantom_tensor_lin(ctx.handle, chain, ptr(da), ptr(db), ptr(dout), qm1.ctypes.data, ptr(dt),
                                       len(tl) * N, qm1.ctypes.data, stream()))
    want = np.zeros(3 * L * N, dtype=np.uint64)
    O.lib().or_tensor_lin(O.P(a), O.P(b), O.P(want), N, L, O.P(mods), O.P(qm1), O.P(t), len(tl) * N, O.P(qm1))
    assert np.array_equal(to_host(dout), want)
    jobs = [(2, True, True), (3, True, True), (2, False, True), (3, True, False)]  # factor, term, constant
    cnt = len(jobs)
    douts = [to_dev(np.zeros(3 * L * N, dtype=np.uint64)) for _ in range(cnt)]
    facs = O.arr([f for f, _, _ in jobs])
    PA.check(_lib().phantom_tensor_lin_batch(
        ctx.handle, chain, cnt, _vp([ptr(da)] * cnt), _vp([ptr(db)] * cnt), _vp(ptr(x) for x in douts),
        facs.ctypes.data, _vp(ptr(dt) if jobs[k][1] else 0 for k in range(cnt)), len(tl) * N,
        _vp(qm1.ctypes.data if jobs[k][1] else 0 for k in range(cnt)),
        _vp(qm1.ctypes.data if jobs[k][2] else 0 for k in range(cnt)), stream()))
    for k, (f, with_t, with_c) in enumerate(jobs):
        want = np.zeros(3 * L * N, dtype=np.uint64)
        fr = O.arr([f % q for q in ql])
        O.lib().or_tensor_lin(O.P(a), O.P(b), O.P(want), N, L, O.P(mods), O.P(fr), O.P(t) if with_t else None,
                              len(tl) * N, O.P(qm1) if with_t else None)
        if with_c:
            w0 = want[:L * N].reshape(L, N)
            for l in range(L):
                w0[l] = ((w0[l].astype(object) + (ql[l] - 1)) % ql[l]).astype(np.uint64)
        assert np.array_equal(to_host(douts[k]), want), k


@pytest.mark.parametrize("pat", ["max", "lowmax"])
@pytest.mark.parametrize("kind", ["q60", "q61"])
def test_lin_comb_and_mul_scalar_edges(ctxs, rng, kind, pat):
    ctx, chain = ctxs(kind), 3
    ql = ctx.ql(chain)
    L = len(ql)
    mods = O.arr(ql)
    d = _fill(rng, pat, ql, 2)
    tl = ctx.ql(chain - 2)
    t = _fill(rng, "max", tl, 2)
    qm1 = O.arr([q - 1 for q in ql])
    dd, dtt = to_dev(d), to_dev(t)
    PA.check(_lib().phantom_lin_comb(ctx.handle, chain, ptr(dd), 2, qm1.ctypes.data, ptr(dtt), 2, len(tl) * N,
                                     qm1.ctypes.data, stream()))
    want = d.copy()
    O.lib().or_lin_comb(O.P(want), 2, O.P(qm1), O.P(t), 2, len(tl) * N, O.P(qm1), N, L, O.P(mods))
    assert np.array_equal(to_host(dd), want)
    acc = _fill(rng, pat, ql, 2)
    dacc = to_dev(acc)
    dout = to_dev(np.zeros(2 * L * N, dtype=np.uint64))
    PA.check(_lib().phantom_mul_scalar(ctx.handle, chain, ptr(dtt), len(tl) * N, qm1.ctypes.data, ptr(dacc), ptr(dout),
                                       2, stream()))
    want = np.zeros(2 * L * N, dtype=np.uint64)
    O.lib().or_mul_scalar_acc(O.P(t), len(tl) * N, O.P(qm1), O.P(acc), O.P(want), 2, N, L, O.P(mods))
    assert np.array_equal(to_host(dout), want)


@pytest.mark.parametrize("in_pat,coef_pat", [(a, b) for a in ("max", "lowmax") for b in ("max", "lowmax")])
@pytest.mark.parametrize("kind", ["q60", "q61"])
def test_leaf_combine_edges(ctxs, rng, kind, in_pat, coef_pat):
    """phantom_leaf_combine at its limits K = kLeafMaxK = 16 and M = 8: 16 products of maximal
    residues (and the constant) in one sum"""
    ctx, chain, K, M = ctxs(kind), 3, 16, 8
    ql = ctx.ql(chain)
    L = len(ql)
    ins, strides = [], []
    for k in range(K):
        lk = ctx.ql(chain - (k % 3))  # inputs at the product's level or above
        ins.append(_fill(rng, in_pat, lk, 2))
        strides.append(len(lk) * N)
    cv = (lambda q: q - 1) if coef_pat == "max" else E.lowmax
    coef = O.arr([cv(ql[i % L]) for i in range(M * K * L)])
    cadd = O.arr([ql[i % L] - 1 for i in range(M * L)])
    dins = [to_dev(x) for x in ins]
    douts = [to_dev(np.zeros(2 * L * N, dtype=np.uint64)) for _ in range(M)]
    st = (PA.sz * K)(*strides)
    PA.check(_lib().phantom_leaf_combine(ctx.handle, chain, _vp(ptr(x) for x in dins), st, K, coef.ctypes.data,
                                         cadd.ctypes.data, _vp(ptr(x) for x in douts), M, stream()))
    want = [np.zeros(2 * L * N, dtype=np.uint64) for _ in range(M)]
    ost = (O.sz * K)(*strides)
    O.lib().or_leaf_combine(O.ptrs(ins), ost, K, O.P(coef), O.P(cadd), O.ptrs(want), M, N, L, O.P(O.arr(ql)))
    for m in range(M):
        assert np.array_equal(to_host(douts[m]), want[m]), m


# ---- NTT -----------------------------------------------------------------------------------------

NTT_DATA = ["max", "alt", "impulse", "stripes", "delta", "random"]


def _ntt_data(rng, n, mods, pat):
    if pat == "delta":  # q - 1 at index 0: every forward output is q - 1, one below a multiple of q
        a = np.zeros(len(mods) * n, dtype=np.uint64)
        a[::n] = [q - 1 for q in mods]
        return a
    return _fill(rng, pat, mods, 1, n)


@pytest.mark.parametrize("table", ["all6", "int3", "lazy2"])
@pytest.mark.parametrize("log_n", [8, 12, 14, 16, 17])
def test_ntt_edges(rng, log_n, table):
    """forward == ntt_fwd, inverse of it == the input, inverse of the pattern == ntt_inv, and the
    scaled inverse, at the regime-edge primes in one launch: all six (FP64 limbs, 16q-barred
    integer limbs and a 30-bit prime together), the three integer ones either side of 2^60 (integer
    only, one limb barred from the 16q ranges), and the two below 2^60 (the lazy integer-only
    kernels, reduce16_est at q just above 2^50).  One size per kernel file and the 1-D path."""
    n = 1 << log_n
    ps = E.edge_primes(n)
    mods = {"all6": ps, "int3": [ps[2], ps[3], ps[4]], "lazy2": [ps[2], ps[3]]}[table]
    L = len(mods)
    t = PA.NttTables(n, mods)
    lib = _lib()
    scale = O.arr([q - 1 if i % 2 == 0 else E.lowmax(q) for i, q in enumerate(mods)])
    shoup = O.arr([(int(s) << 64) // q for s, q in zip(scale, mods)])
    ds, dss = to_dev(scale), to_dev(shoup)
    for pat in NTT_DATA:
        a = _ntt_data(rng, n, mods, pat)
        d = to_dev(a)
        PA.check(lib.phantom_nwt_forward_inplace(ptr(d), t.handle, L, 0, stream()))
        assert np.array_equal(to_host(d), O.ntt_fwd(a, n, mods)), (pat, "forward")
        PA.check(lib.phantom_nwt_backward_inplace(ptr(d), t.handle, L, 0, stream()))
        assert np.array_equal(to_host(d), a), (pat, "inverse of forward")
        inv = O.ntt_inv(a, n, mods)
        d2 = to_dev(a)
        PA.check(lib.phantom_nwt_backward_inplace(ptr(d2), t.handle, L, 0, stream()))
        assert np.array_equal(to_host(d2), inv), (pat, "inverse")
        din, dout = to_dev(a), to_dev(np.zeros_like(a))
        PA.check(lib.phantom_nwt_backward_scale(ptr(dout), ptr(din), t.handle, L, 0, ptr(ds), ptr(dss), stream()))
        want = np.zeros_like(a)
        O.lib().or_poly_mul_scalar(O.P(inv), O.P(scale), O.P(want), n, L, O.P(O.arr(mods)))
        assert np.array_equal(to_host(dout), want), (pat, "scaled inverse")
    t.close()
