"""phantom_avgpool_fc (the hoisted average pooling + fully connected layer on raw ciphertexts) on the
GPU: bit for bit the stages it names, called one by one through the C-ABI

    phantom_ct_mix -> per output phantom_modup + phantom_rotate_sum_ext (columns, identity)
    -> phantom_moddown_from_ntt of every polynomial -> the same over the rows -> the bias on c0

(a full moddown of both polynomials stands between the two directions), and every refused argument
returns status 1 with the outputs untouched.  Operands are uniform random residues."""
import ctypes

import numpy as np
import pytest

import oracle_lib as O
import phantom_amd as PA
from gpu_util import ptr, stream, to_dev, to_host, torch

pytestmark = pytest.mark.gpu

POOL_N = 1 << 12


@pytest.fixture(scope="module")
def pool_ctx():
    ctx = PA.Context(POOL_N, PA.coeff_modulus_create(POOL_N, [60, 50, 50, 50, 60, 60]), 2)
    yield ctx
    ctx.close()


def _lib():
    return PA.load()


def _vp(ts):
    return PA.ptr_array([ptr(t) for t in ts])


def _rotations(width, slotstr):
    out = np.zeros(2 * (width - 1), dtype=np.int32)
    cnt = PA.sz(0)
    PA.check(_lib().phantom_avgpool_rotations(width, slotstr, out.ctypes.data, len(out), ctypes.byref(cnt)))
    assert cnt.value == len(out)
    return out.tolist()


def _key_arrays(keysets, first, count):
    """host array of `count` host arrays of device key-digit pointers (key sets round robin from `first`)"""
    arrays = [_vp(keysets[(first + i) % len(keysets)]) for i in range(count)]
    kk = (ctypes.POINTER(ctypes.c_void_p) * count)(*[ctypes.cast(a, ctypes.POINTER(ctypes.c_void_p)) for a in arrays])
    return kk, arrays


def _residues(rng, shape, mods):
    out = np.zeros(shape + (len(mods),), dtype=np.uint64)
    for l, q in enumerate(mods):
        out[..., l] = rng.integers(0, q, size=shape, dtype=np.uint64)
    return out


def _operands(rng, ctx, chain, shape):
    width, slotstr, t, T = shape
    n, ql = POOL_N, ctx.ql(chain)
    rand = lambda mods, polys=1: np.concatenate([O.random_limbs(rng, n, mods) for _ in range(polys)])
    cts = [to_dev(rand(ql, 2)) for _ in range(t)]
    dnum = -(-ctx.size_Q // ctx.size_P)
    keysets = [[to_dev(rand(ctx.moduli, 2)) for _ in range(dnum)] for _ in range(3)]
    elts = [pow(5, int(r) % (n // 2), 2 * n) for r in _rotations(width, slotstr)]
    return cts, keysets, dnum, elts, _residues(rng, (T, t), ql), _residues(rng, (T,), ql)


def _steps(ctx, chain, shape, cts, keysets, dnum, elts, coef, bias):
    """the layer as the C-ABI entries phantom_avgpool_fc names, one call each"""
    width, slotstr, t, T = shape
    tt, lib, s = torch(), _lib(), stream()
    n, ql = POOL_N, ctx.ql(chain)
    Ql, R = len(ql), width - 1
    QlP, beta = Ql + ctx.size_P, -(-Ql // ctx.size_P)
    zeros = lambda words: tt.zeros(words, dtype=tt.int64, device="cuda")
    cur = [zeros(2 * Ql * n) for _ in range(T)]
    PA.check(lib.phantom_ct_mix(ctx.handle, chain, _vp(cts), t, coef.ctypes.data, None, _vp(cur), T, s))
    digits = zeros(beta * QlP * n)
    for d in range(2):
        kk, keep = _key_arrays(keysets, d * R, R)
        el = (ctypes.c_uint32 * R)(*elts[d * R:(d + 1) * R])
        acc = [zeros(2 * QlP * n) for _ in range(T)]
        for u in range(T):
            PA.check(lib.phantom_modup(ctx.handle, chain, ptr(cur[u]) + 8 * Ql * n, ptr(digits), s))
            PA.check(lib.phantom_rotate_sum_ext(ctx.handle, chain, ptr(cur[u]), ptr(digits), kk, dnum, el, R, 1,
                                                ptr(acc[u]), s))
        nxt = [zeros(2 * Ql * n) for _ in range(T)]
        for u in range(T):
            for p in range(2):
                PA.check(lib.phantom_moddown_from_ntt(ctx.handle, chain, ptr(acc[u]) + 8 * p * QlP * n,
                                                      ptr(nxt[u]) + 8 * p * Ql * n, s))
        cur = nxt
    outs = [to_host(o) for o in cur]
    q = np.repeat(np.array(ql, dtype=np.uint64), n)
    for u in range(T):  # the bias on c0: both below q < 2^61, no wrap
        sm = outs[u][:Ql * n] + np.repeat(bias[u], n)
        outs[u][:Ql * n] = np.where(sm >= q, sm - q, sm)
    return outs


def _layer(ctx, chain, shape, cts, keysets, dnum, elts, coef, bias, contiguous):
    width, slotstr, t, T = shape
    tt = torch()
    words, R = 2 * len(ctx.ql(chain)) * POOL_N, width - 1
    if contiguous:
        whole = tt.full((T * words,), 7, dtype=tt.int64, device="cuda")
        outs = [whole[u * words:(u + 1) * words] for u in range(T)]
    else:
        outs = [tt.full((words,), 7, dtype=tt.int64, device="cuda") for _ in range(T)]
    ck, keep1 = _key_arrays(keysets, 0, R)
    rk, keep2 = _key_arrays(keysets, R, R)
    ce, re_ = (ctypes.c_uint32 * R)(*elts[:R]), (ctypes.c_uint32 * R)(*elts[R:])
    PA.check(_lib().phantom_avgpool_fc(ctx.handle, chain, _vp(cts), t, T, width, slotstr, coef.ctypes.data,
                                       bias.ctypes.data, ck, rk, dnum, ce, re_, _vp(outs), stream()))
    return [to_host(o) for o in outs]


@pytest.mark.parametrize("shape,chain", [((4, 0, 3, 2), 1), ((2, 1, 2, 3), 1), ((4, 0, 3, 2), 2)], ids=str)
def test_avgpool_fc(pool_ctx, rng, shape, chain):
    """the layer == its step-by-step composition, with scattered and with contiguous outputs; chain
    index 2 has 3 + 2 limbs (the last key-switch digit partial)"""
    ops = _operands(rng, pool_ctx, chain, shape)
    want = _steps(pool_ctx, chain, shape, *ops)
    scattered = _layer(pool_ctx, chain, shape, *ops, contiguous=False)
    together = _layer(pool_ctx, chain, shape, *ops, contiguous=True)
    for u in range(shape[3]):
        assert want[u].any()
        assert np.array_equal(scattered[u], want[u]), u
        assert np.array_equal(together[u], want[u]), u


def test_refused_arguments(pool_ctx, rng):
    """every bad argument returns PHANTOM_ERR_INVALID_ARGUMENT (1) and nothing is written"""
    tt, lib, s = torch(), _lib(), stream()
    ctx, chain, n = pool_ctx, 1, POOL_N
    shape = (4, 0, 3, 2)
    width, slotstr, t, T = shape
    cts, keysets, dnum, elts, coef, bias = _operands(rng, ctx, chain, shape)
    Ql, R = len(ctx.ql(chain)), width - 1
    outs = [tt.full((2 * Ql * n,), 7, dtype=tt.int64, device="cuda") for _ in range(T)]
    ck, keep1 = _key_arrays(keysets, 0, 63)  # enough entries for every width tried below
    rk, keep2 = _key_arrays(keysets, 1, 63)
    nokey, keep3 = _key_arrays(keysets, 0, 63)
    nokey[1] = None
    el = (ctypes.c_uint32 * 63)(*[pow(5, k + 1, 2 * n) for k in range(63)])
    nop = PA.Context(n, PA.coeff_modulus_create(n, [60, 50, 50]), 0)  # no special prime
    last = ctx.size_Q + 1  # one past the last chain index
    holes = PA.ptr_array([ptr(cts[0]), 0, ptr(cts[2])])
    out_holes = PA.ptr_array([ptr(outs[0]), 0])

    def pool(c=ctx.handle, ch=chain, cts_=_vp(cts), t_=t, T_=T, w=width, st=slotstr, cf=coef.ctypes.data,
             b=bias.ctypes.data, cols=ck, rows=rk, ce=el, re_=el, outs_=_vp(outs)):
        return lib.phantom_avgpool_fc(c, ch, cts_, t_, T_, w, st, cf, b, cols, rows, dnum, ce, re_, outs_, s)

    bad = [pool(c=None), pool(cts_=None), pool(cf=None), pool(b=None), pool(cols=None), pool(rows=None), pool(ce=None),
           pool(re_=None), pool(outs_=None), pool(cts_=holes), pool(outs_=out_holes), pool(t_=0), pool(T_=0),
           pool(w=0), pool(w=1), pool(w=3), pool(w=6), pool(w=128), pool(w=64), pool(w=4, st=4), pool(w=2, st=40),
           pool(ch=0), pool(ch=last), pool(c=nop.handle), pool(cols=nokey), pool(rows=nokey)]
    assert bad == [1] * len(bad), bad
    tt.cuda.synchronize()
    for o in outs:
        assert bool((o == 7).all())
    nop.close()
