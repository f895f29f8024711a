"""The fused NTT forms and the key switch at every ring degree, bit-exact against the CPU oracle
(every comparison is np.array_equal with the oracle composition the 2^12 / 2^16 tests use).

The NTT is one templated kernel pair (csrc/ntt_impl.h ntt_col / ntt_row), instantiated per degree
as launch<S1_LOG, S2_LOG>: (5,5) (5,6) (6,6) (6,7) (7,7) (7,8) (8,8) (8,9) for N = 2^10 .. 2^17, and
a 1-D kernel below 2^10.  The rest of the suite runs the fused forms (base-conversion and
broadcast prologues, the moddown / rescale finish, the key-switch inner product in the forward
epilogue and the inverse prologue, modup's copy, skip ranges, batched and grouped maps, the XCD
block re-dealing) at 2^12 and 2^16 only, the symmetric splits (6,6) and (8,8).  Here they run at

  log_n 9             the host drivers' 1-D path (unfused inner product, no fused conversion)
  10, 11, 13, 15, 17  (5,5), (7,7) and every asymmetric split; 17 is the only three-round row pass
  14, 15              the integer-only instantiations with their own launch bounds

on three chains of 7 data + 3 special primes:

  mixed  [60] + [50]*6 + [60]*3   FP64 and integer limbs in one launch, lazy range
  io     [60] + [59]*6 + [60]*3   every modulus in [2^50, 2^60): integer-only at log_n >= 14
  q61    [61]*10                  above 2^60: the non-lazy range and the exact reductions

at chain index 1 (Ql = 7, beta = 3, the last digit partial), 2 (Ql = 6, beta = 2, full digits) and
5 (Ql = 3, beta = 1): BETA = 1, 2, 3 of ks_epilogue_b / ks_prologue_b.  Operands are uniform
random residues; the key-switch operations also run once per degree with operands and keys at
q - 1 (edge_cases "max") on the mixed and the 61-bit chain, as tests/test_gpu_edges.py argues.
tests/test_gpu_knobs.py runs the key-switch tests of this file under the runtime switches."""
import ctypes

import numpy as np
import pytest

import edge_cases as E
import ks_oracle as KO
import oracle_lib as O
import phantom_amd as PA
from gpu_util import ptr, stream, to_dev, to_host

pytestmark = pytest.mark.gpu

DEGREES = [9, 10, 11, 13, 14, 15, 17]
CHAINS = {"mixed": [60] + [50] * 6 + [60] * 3, "io": [60] + [59] * 6 + [60] * 3, "q61": [61] * 10}
SIZE_P = 3
LEVELS = {1: (7, 3, True), 2: (6, 2, False), 5: (3, 1, False)}  # chain index: Ql, beta, last digit partial
# ntt_impl.h RowShape<S1_LOG, S2_LOG>::GROUPS (row groups per limb) by log_n; see
# test_relinearize_rescale_row_deal_branches
GROUPS = {10: 1, 11: 2, 12: 4, 13: 8, 14: 16, 15: 32, 16: 64, 17: 128}
SENTINEL = np.uint64(0xDEADBEEFCAFEF00D)

SWEEP = [(log_n, kind, chain) for log_n in DEGREES for kind in CHAINS for chain in LEVELS]
SWEEP_IDS = [f"logn{log_n}-{kind}-c{chain}" for log_n, kind, chain in SWEEP]
# the key-switch operations: the sweep at random operands, and one run per degree at q - 1
KS_SWEEP = [(log_n, kind, chain, "random") for log_n, kind, chain in SWEEP] + \
           [(log_n, kind, 1, "max") for log_n in DEGREES for kind in ("mixed", "q61")]
KS_IDS = [f"logn{log_n}-{kind}-c{chain}-{pat}" for log_n, kind, chain, pat in KS_SWEEP]


def _lib():
    return PA.load()


def _vp(addrs):
    return PA.ptr_array(list(addrs))


@pytest.fixture(scope="module")
def ctxs():
    made = {}

    def get(kind, log_n):
        if (kind, log_n) not in made:
            n = 1 << log_n
            mods = O.coeff_modulus_create(n, CHAINS[kind])
            assert len(set(mods)) == len(mods)
            # the chain is of the kind its name says
            if kind == "mixed":
                assert min(mods) < 2**50 and max(mods) < 2**60
            elif kind == "io":
                assert all(2**50 <= q < 2**60 for q in mods)
            else:
                assert min(mods) > 2**60
            made[(kind, log_n)] = PA.Context(n, mods, SIZE_P)
        return made[(kind, log_n)]

    yield get
    for c in made.values():
        c.close()


def _level(ctx, chain):
    """ql, p, L, beta of `chain`, the shape checked against LEVELS"""
    ql, p = ctx.ql(chain), ctx.moduli[ctx.size_Q:]
    L, beta = len(ql), -(-len(ql) // ctx.size_P)
    assert (L, beta, L % ctx.size_P != 0) == LEVELS[chain]
    assert len(p) == SIZE_P and ql == ctx.moduli[:L]
    return ql, p, L, beta


def _fill(rng, pat, mods, n, polys=1):
    """[polys][len(mods)][n] residues: uniform, or every one at q - 1"""
    if pat == "random":
        return np.concatenate([O.random_limbs(rng, n, mods) for _ in range(polys)])
    return np.concatenate([E.edge_limbs(n, mods, pat, rng) for _ in range(polys)])


def _keys(rng, ctx, pat):
    dnum = -(-ctx.size_Q // ctx.size_P)
    keys = [_fill(rng, pat, ctx.moduli, ctx.n, 2) for _ in range(dnum)]
    return keys, [to_dev(k) for k in keys]


def _moddown(cx, n, ql, p):
    want = np.zeros(len(ql) * n, dtype=np.uint64)
    O.lib().or_moddown_from_ntt(O.P(cx.copy()), O.P(want), n, O.P(O.arr(ql)), len(ql), O.P(O.arr(p)), len(p))
    return want


def _modup(c2, n, ql, p, beta):
    want = np.zeros(beta * (len(ql) + len(p)) * n, dtype=np.uint64)
    O.lib().or_modup(O.P(c2), O.P(want), n, O.P(O.arr(ql)), len(ql), O.P(O.arr(p)), len(p))
    return want


# ---- base conversions around the NTT --------------------------------------------------------------

@pytest.mark.parametrize("log_n,kind,chain", SWEEP, ids=SWEEP_IDS)
def test_modup_moddown_forms(ctxs, rng, log_n, kind, chain):
    """phantom_moddown_from_ntt, phantom_modup (of the moddown's result: canonical residues),
    phantom_moddown_modup and phantom_moddown_modup_batch (3 polynomials at a padded stride), all
    against one set of oracle results: down_i = moddown(cx_i), up_i = modup(down_i)"""
    ctx = ctxs(kind, log_n)
    n = ctx.n
    ql, p, L, beta = _level(ctx, chain)
    qlp, count = L + len(p), 3
    cxs = [O.random_limbs(rng, n, ql + p) for _ in range(count)]
    downs = [_moddown(cx, n, ql, p) for cx in cxs]
    ups = [_modup(d, n, ql, p, beta) for d in downs]
    d = to_dev(cxs[0])
    dout = to_dev(np.zeros(L * n, dtype=np.uint64))
    PA.check(_lib().phantom_moddown_from_ntt(ctx.handle, chain, ptr(d), ptr(dout), stream()))
    assert np.array_equal(to_host(dout), downs[0]), "moddown"
    d = to_dev(downs[0])
    dout = to_dev(np.zeros(beta * qlp * n, dtype=np.uint64))
    PA.check(_lib().phantom_modup(ctx.handle, chain, ptr(d), ptr(dout), stream()))
    assert np.array_equal(to_host(dout), ups[0]), "modup"
    assert np.array_equal(to_host(d), downs[0]), "modup input"
    d = to_dev(cxs[1])
    dout = to_dev(np.zeros(beta * qlp * n, dtype=np.uint64))
    PA.check(_lib().phantom_moddown_modup(ctx.handle, chain, ptr(d), ptr(dout), stream()))
    assert np.array_equal(to_host(dout), ups[1]), "moddown_modup"
    stride = 2 * qlp * n
    buf = np.zeros(count * stride, dtype=np.uint64)
    for i, cx in enumerate(cxs):
        buf[i * stride:i * stride + cx.size] = cx
    d = to_dev(buf)
    dout = to_dev(np.zeros(count * beta * qlp * n, dtype=np.uint64))
    PA.check(_lib().phantom_moddown_modup_batch(ctx.handle, chain, ptr(d), count, stride, ptr(dout), stream()))
    got = to_host(dout).reshape(count, -1)
    for i in range(count):
        assert np.array_equal(got[i], ups[i]), ("moddown_modup_batch", i)


@pytest.mark.parametrize("log_n,kind,chain", SWEEP, ids=SWEEP_IDS)
def test_moddown_rescale_polys(ctxs, rng, log_n, kind, chain):
    """phantom_moddown_rescale of 1, 2, 3 and 4 polynomials == moddown_from_NTT over the special
    basis {q_last} u P.  Under PHX_FUSED_BCONV=1 the conversion is the column pass's prologue, whose
    tile order bcv_tile re-deals when polys * S2 / 16 is a multiple of 8: 4 polynomials at 2^10,
    2 and 4 at 2^11 (S2 = 32, 64), every count from 2^13 on; 1 and 3 take the identity below that."""
    ctx = ctxs(kind, log_n)
    n = ctx.n
    ql, p, L, beta = _level(ctx, chain)
    cxs = [O.random_limbs(rng, n, ql + p) for _ in range(4)]
    wants = [_moddown(cx, n, ql[:-1], [ql[-1]] + list(p)) for cx in cxs]
    s2 = 1 << (log_n - log_n // 2)
    for polys in (1, 2, 3, 4):
        if log_n == 10:
            assert (polys * s2 // 16 % 8 == 0) == (polys == 4)
        if log_n == 11:
            assert (polys * s2 // 16 % 8 == 0) == (polys in (2, 4))
        d = to_dev(np.concatenate(cxs[:polys]))
        dout = to_dev(np.full(polys * (L - 1) * n + n, SENTINEL, dtype=np.uint64))
        PA.check(_lib().phantom_moddown_rescale(ctx.handle, chain, ptr(d), ptr(dout), polys, stream()))
        got = to_host(dout)
        assert np.array_equal(got[:polys * (L - 1) * n], np.concatenate(wants[:polys])), polys
        assert np.all(got[polys * (L - 1) * n:] == SENTINEL), polys


@pytest.mark.parametrize("log_n,kind,chain", SWEEP, ids=SWEEP_IDS)
def test_rescale_to_next(ctxs, rng, log_n, kind, chain):
    """the broadcast prologue and the finish epilogue (below 2^10 the 1-D kernel's own)"""
    ctx = ctxs(kind, log_n)
    n = ctx.n
    ql, p, L, beta = _level(ctx, chain)
    ct = _fill(rng, "random", ql, n, 2)
    d = to_dev(ct)
    dout = to_dev(np.zeros(2 * (L - 1) * n, dtype=np.uint64))
    PA.check(_lib().phantom_rescale_to_next(ctx.handle, chain, ptr(d), ptr(dout), 2, stream()))
    want = np.zeros(2 * (L - 1) * n, dtype=np.uint64)
    O.lib().or_rescale_ntt(O.P(ct), O.P(want), n, L, 2, O.P(O.arr(ql)))
    assert np.array_equal(to_host(dout), want)
    assert np.array_equal(to_host(d), ct)  # input untouched


# ---- key switch -------------------------------------------------------------------------------------

@pytest.mark.parametrize("log_n,kind,chain,pat", KS_SWEEP, ids=KS_IDS)
def test_keyswitch_and_relinearize(ctxs, rng, log_n, kind, chain, pat):
    """phantom_keyswitch (ct += KeySwitch(c2)) == or_keyswitch_add, and phantom_relinearize of the
    same three polynomials, which is that key switch of c2 into (c0, c1)"""
    ctx = ctxs(kind, log_n)
    n = ctx.n
    ql, p, L, beta = _level(ctx, chain)
    ct3 = _fill(rng, pat, ql, n, 3)
    keys, dkeys = _keys(rng, ctx, pat)
    want = ct3[:2 * L * n].copy()
    O.lib().or_keyswitch_add(O.P(want), O.P(ct3[2 * L * n:].copy()), O.ptrs(keys), n, L, ctx.size_Q, ctx.size_P,
                             O.P(O.arr(ctx.moduli)))
    kp = _vp(ptr(k) for k in dkeys)
    dct, dc2 = to_dev(ct3[:2 * L * n]), to_dev(ct3[2 * L * n:])
    PA.check(_lib().phantom_keyswitch(ctx.handle, chain, ptr(dct), ptr(dc2), kp, len(dkeys), stream()))
    assert np.array_equal(to_host(dct), want), "keyswitch"
    d3 = to_dev(ct3)
    PA.check(_lib().phantom_relinearize(ctx.handle, chain, ptr(d3), kp, len(dkeys), stream()))
    assert np.array_equal(to_host(d3)[:2 * L * n], want), "relinearize"


def _relinearize_rescale_all(ctx, chain, cts, keys, dkeys):
    """phantom_relinearize_rescale of cts[0] and phantom_relinearize_rescale_batch of the first 2 and
    of all 3 (padded strides, the padding at a sentinel) against one oracle result per ciphertext"""
    n, L = ctx.n, len(ctx.ql(chain))
    words = 2 * (L - 1) * n
    wants = []
    for ct in cts:  # equal operands (the max pattern) share one result
        same = [w for c, w in zip(cts, wants) if c is ct]
        wants.append(same[0] if same else KO.relinearize_rescale(ctx, chain, ct, keys))
    kp = _vp(ptr(k) for k in dkeys)
    d = to_dev(cts[0])
    dout = to_dev(np.zeros(words, dtype=np.uint64))
    PA.check(_lib().phantom_relinearize_rescale(ctx.handle, chain, ptr(d), ptr(dout), kp, len(dkeys), stream()))
    assert np.array_equal(to_host(dout), wants[0]), "relinearize_rescale"
    s_in, s_out = 3 * L * n + 5 * n, words + 3 * n
    for count in (2, 3):
        buf = np.zeros(count * s_in, dtype=np.uint64)
        for k in range(count):
            buf[k * s_in:k * s_in + 3 * L * n] = cts[k]
        d = to_dev(buf)
        dout = to_dev(np.full(count * s_out, SENTINEL, dtype=np.uint64))
        PA.check(_lib().phantom_relinearize_rescale_batch(ctx.handle, chain, ptr(d), s_in, count, ptr(dout), s_out, kp,
                                                          len(dkeys), stream()))
        got = to_host(dout)
        for k in range(count):
            assert np.array_equal(got[k * s_out:k * s_out + words], wants[k]), ("batch", count, k)
            assert np.all(got[k * s_out + words:(k + 1) * s_out] == SENTINEL), ("padding", count, k)


@pytest.mark.parametrize("log_n,kind,chain,pat", KS_SWEEP, ids=KS_IDS)
def test_relinearize_rescale_and_batch(ctxs, rng, log_n, kind, chain, pat):
    """the inner product inside the moddown-rescale's INTT prologue and NTT epilogue (below 2^10 the
    unfused kernel), one product and batches of 2 and 3.  The forward row pass covers Ql - 1 limbs
    per polynomial: with the 7-limb chains ks_row_block re-deals at 2^14 for chain index 1 (and 5) and not
    for 2, and always from 2^15 on (test_relinearize_rescale_row_deal_branches has the condition)."""
    ctx = ctxs(kind, log_n)
    ql, p, L, beta = _level(ctx, chain)
    if log_n == 14:  # 6 and 2 limbs fill whole groups of 8 blocks, 5 do not
        assert ((L - 1) * GROUPS[log_n] % 32 == 0) == (chain != 2)
    if log_n >= 15:
        assert GROUPS[log_n] % 32 == 0
    one = _fill(rng, pat, ql, ctx.n, 3)
    cts = [one] * 3 if pat == "max" else [one] + [_fill(rng, pat, ql, ctx.n, 3) for _ in range(2)]
    keys, dkeys = _keys(rng, ctx, pat)
    _relinearize_rescale_all(ctx, chain, cts, keys, dkeys)


# (log_n, data primes, special primes, chain index, blocks per polynomial of the forward row pass or
# None where it keeps the launch order); 50-bit data and 60-bit special primes
ROW_DEAL = [(10, 33, 11, 1, 8), (10, 33, 11, 2, None), (10, 65, 22, 1, 16),
            (11, 17, 6, 1, 8), (11, 17, 6, 2, None), (11, 33, 11, 1, 16),
            (13, 5, 3, 1, 8), (13, 5, 3, 2, None), (13, 9, 3, 1, 16)]


@pytest.mark.parametrize("log_n,size_q,size_p,chain,per", ROW_DEAL,
                         ids=[f"logn{c[0]}-{c[1]}p{c[2]}-c{c[3]}-{'identity' if c[4] is None else f'redeal{c[4]}'}"
                              for c in ROW_DEAL])
def test_relinearize_rescale_row_deal_branches(rng, log_n, size_q, size_p, chain, per):
    """Both branches of ks_row_block (csrc/ntt_impl.h) at the degrees where 7 limbs reach only one.

    A batched row pass of `polys` >= 2 polynomials deals its blocks polynomial-interleaved per XCD
    when every polynomial fills whole groups of 8 blocks:

        limbs_per_poly * GROUPS % (WAVES * 8) == 0,   WAVES = 4 wavefronts (row items) per block,
        GROUPS = S1 / RW row items per limb = 1, 2, 4, 8, 16, 32, 64, 128 for N = 2^10 .. 2^17

    and keeps the launch order otherwise.  Block b = 8 k + x then works on block
    (k % polys) per + (k / polys) 8 + x, per = limbs_per_poly GROUPS / WAVES blocks per polynomial.
    The forward row pass of phantom_relinearize_rescale covers Ql - 1 limbs for each of its 2
    (batch: 2 count) polynomials, so 33, 17 and 5 data primes at 2^10, 2^11 and 2^13 take the
    re-dealing branch at chain index 1 (per = 8) and the next level, one limb fewer, does not.
    With per = 8 the re-dealt order is the launch order again (8 k + x): only per >= 16 moves a
    block, so chains of 65, 33 and 9 data primes (per = 16) run too; a re-dealing that skipped or
    repeated blocks passes the shorter ones.  From 2^15 on GROUPS itself is a multiple of 32: every
    batched row pass re-deals.  Every chain has enough special primes for beta <= kMaxKsBeta = 3
    (above it the driver takes the unfused inner product).  A change to the row tiling changes this
    table."""
    n = 1 << log_n
    ctx = PA.Context(n, O.coeff_modulus_create(n, [50] * size_q + [60] * size_p), size_p)
    try:
        ql = ctx.ql(chain)
        L, beta = len(ql), -(-len(ql) // size_p)
        assert L == size_q - (chain - 1) and beta <= 3
        work = (L - 1) * GROUPS[log_n]  # wavefront items per polynomial
        assert (work % 32 == 0) == (per is not None)
        assert per is None or work // 4 == per
        cts = [_fill(rng, "random", ql, n, 3) for _ in range(3)]
        keys, dkeys = _keys(rng, ctx, "random")
        _relinearize_rescale_all(ctx, chain, cts, keys, dkeys)
    finally:
        ctx.close()


# ---- hoisted rotations --------------------------------------------------------------------------------

@pytest.mark.parametrize("log_n,kind,chain,pat", KS_SWEEP, ids=KS_IDS)
def test_fast_rotation_ext_batch_degrees(ctxs, rng, log_n, kind, chain, pat):
    """one launch of three baby steps: a NULL key (the keyswitch_ext entry), a rotation and the
    conjugation 2n - 1 == or_keyswitch_ext / or_fast_rotation_ext per entry"""
    ctx = ctxs(kind, log_n)
    n, count = ctx.n, 3
    ql, p, L, beta = _level(ctx, chain)
    em = ql + p
    dnum = -(-ctx.size_Q // ctx.size_P)
    ct = _fill(rng, pat, ql, n, 2)
    digits = _fill(rng, pat, em, n, beta)
    keysets = [_keys(rng, ctx, pat) for _ in range(2)]
    elts = [5, pow(5, 3, 2 * n), 2 * n - 1]  # the first is not applied: a NULL key is the identity entry
    dct, ddig = to_dev(ct), to_dev(digits)
    douts = [to_dev(np.full(2 * len(em) * n, 5, dtype=np.uint64)) for _ in range(count)]
    key_arrays = [None] + [_vp(ptr(x) for x in keysets[k % 2][1]) for k in (1, 2)]
    kk = (ctypes.POINTER(ctypes.c_void_p) * count)(*[ctypes.cast(a, ctypes.POINTER(ctypes.c_void_p)) if a is not None
                                                     else None for a in key_arrays])
    el = (ctypes.c_uint32 * count)(*elts)
    PA.check(_lib().phantom_fast_rotation_ext_batch(ctx.handle, chain, ptr(dct), ptr(ddig), kk, dnum, el, count,
                                                    _vp(ptr(x) for x in douts), stream()))
    mods = O.P(O.arr(ctx.moduli))
    for k in range(count):
        want = np.zeros(2 * len(em) * n, dtype=np.uint64)
        if k == 0:
            O.lib().or_keyswitch_ext(O.P(ct), O.P(want), n, L, ctx.size_Q, ctx.size_P, mods)
        else:
            O.lib().or_fast_rotation_ext(O.P(ct), O.P(digits), O.ptrs(keysets[k % 2][0]), elts[k], 1, O.P(want), n, L,
                                         ctx.size_Q, ctx.size_P, mods)
        assert np.array_equal(to_host(douts[k]), want), k


@pytest.mark.parametrize("log_n,kind,chain,pat", KS_SWEEP, ids=KS_IDS)
def test_rotate_ext_accumulate_degrees(ctxs, rng, log_n, kind, chain, pat):
    """a giant step (moddown, modup, inner product, automorphism) stored and accumulated"""
    ctx = ctxs(kind, log_n)
    n = ctx.n
    ql, p, L, beta = _level(ctx, chain)
    em = ql + p
    ext, acc = _fill(rng, pat, em, n, 2), _fill(rng, pat, em, n, 2)
    keys, dkeys = _keys(rng, ctx, pat)
    elt = pow(5, n // 8 + 1, 2 * n)
    for accumulate in (0, 1):
        dext, dacc = to_dev(ext), to_dev(acc)
        PA.check(_lib().phantom_rotate_ext_accumulate(ctx.handle, chain, ptr(dext), _vp(ptr(k) for k in dkeys),
                                                      len(dkeys), elt, ptr(dacc), accumulate, stream()))
        want = acc.copy()
        O.lib().or_rotate_ext_accumulate(O.P(ext.copy()), O.ptrs(keys), elt, O.P(want), accumulate, n, L, ctx.size_Q,
                                         ctx.size_P, O.P(O.arr(ctx.moduli)))
        assert np.array_equal(to_host(dacc), want), accumulate


@pytest.mark.parametrize("log_n", DEGREES)
def test_apply_galois_degrees(ctxs, rng, log_n):
    ctx = ctxs("mixed", log_n)
    n, L = ctx.n, ctx.size_Q
    a = O.random_limbs(rng, n, ctx.moduli[:L])
    for elt in (5, pow(5, n // 4, 2 * n), 2 * n - 1):
        d, dout = to_dev(a), to_dev(np.zeros_like(a))
        PA.check(_lib().phantom_apply_galois_ntt(ctx.handle, elt, ptr(d), ptr(dout), L, stream()))
        want = np.zeros_like(a)
        O.lib().or_apply_galois_ntt(O.P(a), O.P(want), n, L, elt)
        assert np.array_equal(to_host(dout), want), elt


# ---- the NTT launchers, called directly ----------------------------------------------------------------

def _rows(x, n, idx):
    """the limb rows `idx` of a [limbs][n] array, in that order"""
    return np.ascontiguousarray(x.reshape(-1, n)[list(idx)]).reshape(-1)


def _scaled(x, n, mods, scale):
    out = np.zeros_like(x)
    O.lib().or_poly_mul_scalar(O.P(np.ascontiguousarray(x)), O.P(O.arr(scale)), O.P(out), n, len(mods), O.P(O.arr(mods)))
    return out


@pytest.mark.parametrize("log_n", [8] + DEGREES)
def test_ntt_launchers_degrees(rng, log_n):
    """every launcher of include/phantom_amd.h on the mixed chain's tables (tests/test_gpu_ntt.py
    runs them at 2^16 only): out of place with the input preserved, the scaled inverses, the
    special-prime maps with and without a skipped range (in the middle, from limb 0), the inverse
    over the special rows, the moddown finish, and non-zero start_modulus_idx.  Below 2^10 the 1-D
    kernel implements scale, skip and epilogue itself.  One forward and one inverse oracle
    transform of a [10][n] array give every expected value: buffers are rows of it."""
    n = 1 << log_n
    mods = O.coeff_modulus_create(n, CHAINS["mixed"])
    size_QP, size_P = len(mods), SIZE_P
    size_Q = size_QP - size_P
    t = PA.NttTables(n, mods)
    lib = _lib()
    a = O.random_limbs(rng, n, mods)
    fwd, inv = O.ntt_fwd(a, n, mods), O.ntt_inv(a, n, mods)
    sent = lambda limbs: to_dev(np.full(limbs * n, SENTINEL, dtype=np.uint64))
    scale = [int(x) % q for x, q in zip(rng.integers(1, 2**62, size_QP), mods)]
    shoup = lambda vals, qs: O.arr([(int(s) << 64) // q for s, q in zip(vals, qs)])
    try:
        # out of place, all limbs
        din, dout = to_dev(a), sent(size_QP)
        PA.check(lib.phantom_nwt_backward(ptr(dout), ptr(din), t.handle, size_QP, 0, stream()))
        assert np.array_equal(to_host(dout), inv), "backward"
        assert np.array_equal(to_host(din), a), "backward input"
        # scaled, out of place, limbs [2, 7): the scale array starts at the first transformed limb
        start, L = 2, 5
        sub, sc = mods[start:start + L], scale[start:start + L]
        ds, dss = to_dev(O.arr(sc)), to_dev(shoup(sc, sub))
        din, dout = to_dev(a), sent(size_QP)
        PA.check(lib.phantom_nwt_backward_scale(ptr(dout), ptr(din), t.handle, L, start, ptr(ds), ptr(dss), stream()))
        got = to_host(dout)
        assert np.array_equal(got[start * n:(start + L) * n], _scaled(inv[start * n:(start + L) * n], n, sub, sc))
        assert np.all(got[:start * n] == SENTINEL) and np.all(got[(start + L) * n:] == SENTINEL)
        assert np.array_equal(to_host(din), a), "backward_scale input"
        # scaled, in place, limbs [0, 7)
        L = size_Q
        ds, dss = to_dev(O.arr(scale[:L])), to_dev(shoup(scale[:L], mods[:L]))
        d = to_dev(a)
        PA.check(lib.phantom_nwt_backward_inplace_scale(ptr(d), t.handle, L, 0, ptr(ds), ptr(dss), stream()))
        got = to_host(d)
        assert np.array_equal(got[:L * n], _scaled(inv[:L * n], n, mods[:L], scale[:L])), "backward_inplace_scale"
        assert np.array_equal(got[L * n:], a[L * n:])
        # forward over Ql = 4 data limbs and the special limbs
        rows = list(range(4)) + list(range(size_Q, size_QP))
        d = to_dev(_rows(a, n, rows))
        PA.check(lib.phantom_nwt_forward_include_special_mod(ptr(d), t.handle, len(rows), 0, size_QP, size_P, stream()))
        assert np.array_equal(to_host(d), _rows(fwd, n, rows)), "include_special_mod"
        # ... over Ql = 6 with a skipped range in the middle and one from limb 0
        rows = list(range(6)) + list(range(size_Q, size_QP))
        for lo, hi in ((2, 4), (0, 3)):
            d = to_dev(_rows(a, n, rows))
            PA.check(lib.phantom_nwt_forward_include_special_mod_exclude_range(ptr(d), t.handle, len(rows), 0, size_QP,
                                                                               size_P, lo, hi, stream()))
            want = _rows(fwd, n, rows)
            want[lo * n:hi * n] = _rows(a, n, rows)[lo * n:hi * n]
            assert np.array_equal(to_host(d), want), ("exclude_range", lo, hi)
        # ... from start_modulus_idx 1: buffer limbs [1, 9) are table rows 1 .. 5 and the special rows
        start, rows = 1, list(range(1, 6)) + list(range(size_Q, size_QP))
        buf = np.concatenate([a[:n], _rows(a, n, rows)])
        d = to_dev(buf)
        PA.check(lib.phantom_nwt_forward_include_special_mod_exclude_range(ptr(d), t.handle, len(rows), start, size_QP,
                                                                           size_P, 1, 3, stream()))
        want = np.concatenate([a[:n], _rows(fwd, n, rows)])
        want[n:3 * n] = buf[n:3 * n]
        assert np.array_equal(to_host(d), want), "exclude_range from limb 1"
        # inverse of the special limbs of a Ql + P buffer (moddown_from_NTT's first step)
        size_Ql = 4
        rows = list(range(size_Ql)) + list(range(size_Q, size_QP))
        d = to_dev(_rows(a, n, rows))
        PA.check(lib.phantom_nwt_backward_inplace_include_special_mod(ptr(d), t.handle, size_P, size_Ql, size_QP, size_P,
                                                                      stream()))
        want = np.concatenate([a[:size_Ql * n], inv[size_Q * n:]])
        assert np.array_equal(to_host(d), want), "backward include_special_mod"
        # the moddown finish ct = (cx - NTT(delta)) P^-1 over limbs [1, 7): the constants are indexed
        # by the absolute limb
        start, L = 1, 6
        cx = O.random_limbs(rng, n, mods[:size_Q])
        pinv = scale[:size_Q]
        dct, dcx, ddl = sent(size_Q), to_dev(cx), to_dev(a[:size_Q * n])
        dp, dps = to_dev(O.arr(pinv)), to_dev(shoup(pinv, mods[:size_Q]))
        PA.check(lib.phantom_nwt_forward_fuse_moddown(ptr(dct), ptr(dcx), ptr(dp), ptr(dps), ptr(ddl), t.handle, L, start,
                                                      stream()))
        sl = slice(start * n, (start + L) * n)
        sub = mods[start:start + L]
        diff = np.zeros(L * n, dtype=np.uint64)
        O.lib().or_poly_sub(O.P(np.ascontiguousarray(cx[sl])), O.P(np.ascontiguousarray(fwd[sl])), O.P(diff), n, L,
                            O.P(O.arr(sub)))
        got = to_host(dct)
        assert np.array_equal(got[sl], _scaled(diff, n, sub, pinv[start:start + L])), "fuse_moddown"
        assert np.all(got[:start * n] == SENTINEL)
    finally:
        t.close()


@pytest.mark.parametrize("bits", [50, 60])
@pytest.mark.parametrize("batch", [1, 5])
@pytest.mark.parametrize("log_n", [3, 4, 5, 6, 7])
def test_nwt_1d_small_sizes(rng, log_n, batch, bits):
    """phantom_fnwt_1d / phantom_inwt_1d below one wavefront of butterflies (n / 2 < 64 threads, the
    block is 64): forward and inverse == the oracle, the round trip, and the inverse with a scalar.
    The tested limbs are the last rows of the table (start_modulus_idx = num_moduli - batch)."""
    n = 1 << log_n
    mods = O.coeff_modulus_create(n, [110 - bits] + [bits] * batch)
    start, sub = 1, mods[1:]
    t = PA.NttTables(n, mods)
    lib = _lib()
    try:
        a = np.concatenate([O.random_limbs(rng, n, mods[:1]), O.random_limbs(rng, n, sub)])
        fwd, inv = O.ntt_fwd(a[n:], n, sub), O.ntt_inv(a[n:], n, sub)
        d = to_dev(a)
        PA.check(lib.phantom_fnwt_1d(ptr(d), t.handle, batch, start, stream()))
        assert np.array_equal(to_host(d), np.concatenate([a[:n], fwd])), "forward"
        PA.check(lib.phantom_inwt_1d(ptr(d), t.handle, batch, start, None, None, stream()))
        assert np.array_equal(to_host(d), a), "round trip"
        d = to_dev(a)
        PA.check(lib.phantom_inwt_1d(ptr(d), t.handle, batch, start, None, None, stream()))
        assert np.array_equal(to_host(d), np.concatenate([a[:n], inv])), "inverse"
        scale = [q - 1 if i % 2 == 0 else int(x) % q for i, (x, q) in enumerate(zip(rng.integers(1, 2**62, batch), sub))]
        ds = to_dev(O.arr(scale))
        dss = to_dev(O.arr([(int(s) << 64) // q for s, q in zip(scale, sub)]))
        d = to_dev(a)
        PA.check(lib.phantom_inwt_1d(ptr(d), t.handle, batch, start, ptr(ds), ptr(dss), stream()))
        assert np.array_equal(to_host(d), np.concatenate([a[:n], _scaled(inv, n, sub, scale)])), "inverse with a scalar"
    finally:
        t.close()
