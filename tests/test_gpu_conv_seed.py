"""Batch norm, bias and the residual add fused into a prepared convolution, on the GPU, bit-exact:

  phantom_ext_mac_sub_seeded     == or_lt_bsgs on the expanded plaintexts + P (res m + [p == 0] B) mod q_l
                                 on the limbs of Ql (Python integers), nothing on the limbs of P
  phantom_conv2d_apply_seeded    == phantom_conv2d_apply + (res m + [p == 0] B) mod q_l, word for word:
                                 moddown(x + P v) = moddown(x) + v (tests/test_convbn_host.py)
  phantom_conv2d_prepare_scaled  == phantom_conv2d_prepare on weights scaled on the host in FP64
  refused arguments              status 1, outputs untouched"""
import ctypes

import numpy as np
import pytest

import edge_cases as E
import oracle_lib as O
import phantom_amd as PA
from gpu_util import ptr, stream, to_dev, to_host, torch
from test_gpu_conv import (CONV_N, CONV_SCALE, _conv_operands, _Dev, _ext_mods, _key_arrays, _vp, conv_ctx,  # noqa: F401
                           ctxs)

pytestmark = pytest.mark.gpu

T_, O_ = 33, 17  # one past a term block; one past the 16 waves of a workgroup


def _lib():
    return PA.load()


@pytest.fixture(scope="module")
def mixed_small():
    ctx = PA.Context(512, PA.coeff_modulus_create(512, [60, 50, 50, 50, 60, 60]), 2)
    yield ctx
    ctx.close()


def _expand(pt, L, M, n):
    return np.repeat(pt.reshape(L, M), n // M, axis=1).reshape(-1)


def _oracle_mac(ctx, chain, n, M, ins, pts):
    em = _ext_mods(ctx, chain)
    L = len(em)
    cache = {}
    full = []
    for x in pts:
        if id(x) not in cache:
            cache[id(x)] = _expand(x, L, M, n)
        full.append(cache[id(x)])
    want = [np.zeros(2 * L * n, dtype=np.uint64) for _ in range(O_)]
    O.lib().or_lt_bsgs(O.ptrs(ins), T_, O.ptrs(full), O_, O.ptrs(want), n, len(ctx.ql(chain)), ctx.size_Q, ctx.size_P,
                       O.P(O.arr(ctx.moduli)))
    return want


def _big_p(ctx):
    P = 1
    for p in ctx.moduli[ctx.size_Q:]:
        P *= int(p)
    return P


def _res_term(ctx, chain, n, res, mult):
    """P m res mod q_l over the limbs of Ql and zeros over P, as [2][Ql + P][n], in Python integers
    (object arrays); res [2][Ql][n], mult [Ql]"""
    ql = ctx.ql(chain)
    Ql, QlP, P = len(ql), len(ql) + ctx.size_P, _big_p(ctx)
    out = np.zeros((2, QlP, n), dtype=np.uint64)
    for l, q in enumerate(ql):
        c = (P * int(mult[l])) % int(q)
        out[:, l] = np.array((res.reshape(2, Ql, n)[:, l].astype(object) * c) % int(q), dtype=np.uint64)
    return out.reshape(-1)


def _bias_term(ctx, chain, n, bias_row):
    """P B mod q_l in every word of polynomial 0's limbs of Ql, zeros elsewhere"""
    ql = ctx.ql(chain)
    out = np.zeros((2, len(ql) + ctx.size_P, n), dtype=np.uint64)
    for l, q in enumerate(ql):
        out[0, l] = (_big_p(ctx) * int(bias_row[l])) % int(q)
    return out.reshape(-1)


def _add_mod(a, b, ctx, chain, n):
    q = np.tile(np.repeat(np.array(_ext_mods(ctx, chain), dtype=np.uint64), n), 2)
    s = a + b  # both below q < 2^61: no wrap
    return np.where(s >= q, s - q, s)


def _run_seeded(ctx, chain, M, din, table, res, mult, bias, n):
    """res: list of O_ numpy arrays or None entries, or None; mult: [Ql] array or None; bias: [O_][Ql] or None"""
    QlP = len(_ext_mods(ctx, chain))
    douts = [to_dev(np.full(2 * QlP * n, 5, dtype=np.uint64)) for _ in range(O_)]
    keep = [None if r is None else to_dev(r) for r in res] if res is not None else None
    res_arr = PA.ptr_array([None if k is None else ptr(k) for k in keep]) if keep is not None else None
    m = np.ascontiguousarray(mult, dtype=np.uint64) if mult is not None else None
    b = np.ascontiguousarray(bias, dtype=np.uint64) if bias is not None else None
    PA.check(_lib().phantom_ext_mac_sub_seeded(ctx.handle, chain, _vp(din), T_, ptr(table), M, O_, _vp(douts), res_arr,
                                               m.ctypes.data if m is not None else None,
                                               b.ctypes.data if b is not None else None, stream()))
    return [to_host(d) for d in douts]


@pytest.mark.parametrize("sub", ["128", "N"])
@pytest.mark.parametrize("chain_kind", ["59", "mixed", "61"])
@pytest.mark.parametrize("n", [1 << 12, 1 << 9])
def test_ext_mac_sub_seeded(ctxs, conv_ctx, mixed_small, rng, n, chain_kind, sub):
    """33 terms x 17 outputs in the tile form (N = 2^12) and the plain form (N = 2^9), compact
    plaintexts of 128 words and full-size ones (ext_mac's kernels): random words with a full seed, one
    null residual, bias only, residual only, and every operand, residual word, res_mult and bias at
    q - 1"""
    if chain_kind == "mixed":
        ctx = conv_ctx if n == CONV_N else mixed_small
    else:
        ctx = ctxs(int(chain_kind), n)
    chain = 1
    em, ql = _ext_mods(ctx, chain), ctx.ql(chain)
    Ql, M = len(ql), 128 if sub == "128" else n
    rand = lambda size, mods, polys: np.concatenate([O.random_limbs(rng, size, mods) for _ in range(polys)])

    # random words: one oracle sum shared by the four seed cases
    pin, ppt = [rand(n, em, 2) for _ in range(12)], [rand(M, em, 1) for _ in range(20)]
    ins = [pin[(5 * t + 1) % len(pin)] for t in range(T_)]
    pts = [ppt[(7 * k + k // T_) % len(ppt)] for k in range(T_ * O_)]
    want = _oracle_mac(ctx, chain, n, M, ins, pts)
    dev = _Dev()
    din, dpt = [dev(x) for x in ins], [dev(x) for x in pts]
    table = to_dev(np.array([ptr(x) for x in dpt], dtype=np.uint64))
    res = [rand(n, ql, 2) for _ in range(O_)]
    mult = np.array([int(rng.integers(0, q)) for q in ql], dtype=np.uint64)
    bias = np.array([[int(rng.integers(0, q)) for q in ql] for _ in range(O_)], dtype=np.uint64)
    one_null = list(res)
    one_null[3] = None
    cases = {"full": (res, mult, bias), "one null residual": (one_null, mult, bias), "bias only": (None, None, bias),
             "residual only": (res, mult, None)}
    res_terms = [_res_term(ctx, chain, n, res[o], mult) for o in range(O_)]
    bias_terms = [_bias_term(ctx, chain, n, bias[o]) for o in range(O_)]
    for name, (r, m, b) in cases.items():
        got = _run_seeded(ctx, chain, M, din, table, r, m, b, n)
        for o in range(O_):
            w = want[o]
            if r is not None and r[o] is not None:
                w = _add_mod(w, res_terms[o], ctx, chain, n)
            if b is not None:
                w = _add_mod(w, bias_terms[o], ctx, chain, n)
            assert np.array_equal(got[o], w), (name, o)
        assert not np.array_equal(got[0], want[0]), name

    # the edge: everything at q - 1
    a = np.concatenate([E.edge_limbs(n, em, "max")] * 2)
    w = E.edge_limbs(M, em, "max")
    ins, pts = [a] * T_, [w] * (T_ * O_)
    want = _oracle_mac(ctx, chain, n, M, ins, pts)
    da, dw = to_dev(a), to_dev(w)
    table = to_dev(np.array([ptr(dw)] * (T_ * O_), dtype=np.uint64))
    r = np.concatenate([E.edge_limbs(n, ql, "max")] * 2)
    m = np.array([q - 1 for q in ql], dtype=np.uint64)
    got = _run_seeded(ctx, chain, M, [da] * T_, table, [r] * O_, m, np.tile(m, (O_, 1)), n)
    seed = _add_mod(_res_term(ctx, chain, n, r, m), _bias_term(ctx, chain, n, m), ctx, chain, n)
    for o in range(O_):
        assert np.array_equal(got[o], _add_mod(want[o], seed, ctx, chain, n)), ("edge", o)


# ---- the layer -----------------------------------------------------------------------------------

SHAPE = (8, 0, 3, 3, 2)  # width 8, slotstr 0, K = 3, 3 -> 2 channels


def _apply(ctx, plan, cts, keysets, dnum, elts, seed=None):
    width, slotstr, K, in_ch, out_ch = SHAPE
    t = torch()
    words = 2 * len(ctx.ql(1)) * CONV_N
    outs = [t.full((words,), 7, dtype=t.int64, device="cuda") for _ in range(out_ch)]
    kk, keep = _key_arrays(keysets, K * K)
    el = (ctypes.c_uint32 * (K * K))(*elts)
    if seed is None:
        PA.Conv.apply(ctx, plan, _vp(cts), kk, dnum, el, _vp(outs), stream())
    else:
        res, mult, bias = seed
        PA.Conv.apply_seeded(ctx, plan, _vp(cts), kk, dnum, el, _vp(outs), res, mult, bias, stream())
    return [to_host(o) for o in outs]


def test_conv2d_apply_seeded(conv_ctx, rng):
    """seeded apply == apply + (res m + [p == 0] B) mod q_l on the same inputs, plan and keys: the
    moddown identity; a seed that touched the limbs of P would break it"""
    ctx, chain, n = conv_ctx, 1, CONV_N
    ql = ctx.ql(chain)
    Ql, out_ch = len(ql), SHAPE[4]
    cts, keysets, dnum, elts, W = _conv_operands(rng, ctx, chain, SHAPE)
    plan = PA.Conv.prepare(ctx, chain, SHAPE, W.data_ptr(), CONV_SCALE, stream())
    try:
        base = _apply(ctx, plan, cts, keysets, dnum, elts)
        res = [np.concatenate([O.random_limbs(rng, n, ql) for _ in range(2)]) for _ in range(out_ch)]
        dres = [to_dev(r) for r in res]
        mult = np.array([(1 << 50) % q for q in ql], dtype=np.uint64)
        bias = np.array([[int(rng.integers(0, q)) for q in ql] for _ in range(out_ch)], dtype=np.uint64)
        q = np.tile(np.repeat(np.array(ql, dtype=np.uint64), n), 2)

        def want(h, with_res, with_bias):
            v = np.zeros((2, Ql, n), dtype=object)
            if with_res:
                v = v + res[h].reshape(2, Ql, n).astype(object) * mult.astype(object).reshape(1, Ql, 1)
            if with_bias:
                v[0] = v[0] + bias[h].astype(object).reshape(Ql, 1)
            v = np.array(v % np.array(ql, dtype=object).reshape(1, Ql, 1), dtype=np.uint64).reshape(-1)
            s = base[h] + v
            return np.where(s >= q, s - q, s)

        for with_res, with_bias in [(True, True), (True, False), (False, True)]:
            seed = (_vp(dres) if with_res else None, mult if with_res else None, bias if with_bias else None)
            got = _apply(ctx, plan, cts, keysets, dnum, elts, seed)
            for h in range(out_ch):
                assert np.array_equal(got[h], want(h, with_res, with_bias)), (with_res, with_bias, h)
                assert not np.array_equal(got[h], base[h])
    finally:
        plan.close()


def test_conv2d_prepare_scaled(conv_ctx, rng):
    """out_scale = 1 (and none): the plan's plaintext words are phantom_conv2d_prepare's; out_scale = a:
    they are those of phantom_conv2d_prepare on weights multiplied by a_h on the host in FP64"""
    ctx, chain = conv_ctx, 1
    out_ch = SHAPE[4]
    W = _conv_operands(rng, ctx, chain, SHAPE)[4]
    a = rng.uniform(-1.5, 1.5, size=out_ch)
    before = W.cpu().numpy().copy()
    Wa = torch().from_numpy(before * a.reshape(1, 1, 1, out_ch)).cuda()
    plans = [PA.Conv.prepare(ctx, chain, SHAPE, W.data_ptr(), CONV_SCALE, stream()),
             PA.Conv.prepare_scaled(ctx, chain, SHAPE, W.data_ptr(), np.ones(out_ch), CONV_SCALE, stream()),
             PA.Conv.prepare_scaled(ctx, chain, SHAPE, W.data_ptr(), None, CONV_SCALE, stream()),
             PA.Conv.prepare(ctx, chain, SHAPE, Wa.data_ptr(), CONV_SCALE, stream()),
             PA.Conv.prepare_scaled(ctx, chain, SHAPE, W.data_ptr(), a, CONV_SCALE, stream())]
    try:
        plain, ones, none, host_scaled, dev_scaled = [p.words() for p in plans]
        assert plain.size * 8 == plans[0].bytes and plain.any()
        assert np.array_equal(ones, plain) and np.array_equal(none, plain)
        assert np.array_equal(dev_scaled, host_scaled)
        assert not np.array_equal(dev_scaled, plain)
        assert np.array_equal(W.cpu().numpy(), before)  # dev_W is not modified
    finally:
        for p in plans:
            p.close()


def test_seed_refused_arguments(conv_ctx, rng, request):
    """status 1 and outputs untouched: what the unseeded entries refuse, and a residual without its
    multiplier"""
    t, lib, s = torch(), _lib(), stream()
    ctx, chain, n = conv_ctx, 1, CONV_N
    width, slotstr, K, in_ch, out_ch = SHAPE
    cts, keysets, dnum, elts, W = _conv_operands(rng, ctx, chain, SHAPE)
    ql = ctx.ql(chain)
    Ql, QlP = len(ql), len(ql) + ctx.size_P
    outs = [t.full((2 * Ql * n,), 7, dtype=t.int64, device="cuda") for _ in range(out_ch)]
    kk, keep = _key_arrays(keysets, K * K)
    el = (ctypes.c_uint32 * (K * K))(*elts)
    nokey, keep2 = _key_arrays(keysets, K * K)
    nokey[0] = None
    other = PA.Context(n, ctx.moduli, ctx.size_P)
    nop = PA.Context(n, PA.coeff_modulus_create(n, [60, 50, 50]), 0)  # no special prime
    request.addfinalizer(other.close)
    request.addfinalizer(nop.close)
    last = len(ctx.moduli) - ctx.size_P + 1
    plan = PA.Conv.prepare(ctx, chain, SHAPE, W.data_ptr(), CONV_SCALE, s)
    request.addfinalizer(plan.close)
    res = [t.full((2 * Ql * n,), 3, dtype=t.int64, device="cuda") for _ in range(out_ch)]
    mult = np.full(Ql, 3, dtype=np.uint64)
    bias = np.full((out_ch, Ql), 3, dtype=np.uint64)

    def apply(c=ctx, p=plan.handle, cts_=_vp(cts), keys=kk, e=el, outs_=_vp(outs), r=_vp(res), m=mult.ctypes.data,
              b=bias.ctypes.data):
        return lib.phantom_conv2d_apply_seeded(c.handle if c else None, p, cts_, keys, dnum, e, outs_, r, m, b, s)

    one_null = _vp(cts)
    one_null[1] = None
    bad = [apply(m=None), apply(m=None, b=None), apply(c=other), apply(c=None), apply(p=None), apply(cts_=None),
           apply(keys=None), apply(e=None), apply(outs_=None), apply(keys=nokey), apply(cts_=one_null)]
    assert bad == [1] * len(bad), bad

    def prepare(c=ctx, ch=chain, i=in_ch, o=out_ch, w=width, st=slotstr, k=K, dw=W.data_ptr(), sc=CONV_SCALE, out=True,
                a=np.ones(out_ch)):
        h = ctypes.c_void_p()
        r = lib.phantom_conv2d_prepare_scaled(c.handle if c else None, ch, i, o, w, st, k, dw, a.ctypes.data, sc, None, s,
                                              ctypes.byref(h) if out else None)
        assert r != 0 and not h.value
        return r

    bad = [prepare(dw=None), prepare(out=False), prepare(i=0), prepare(o=0), prepare(k=2), prepare(k=9), prepare(w=6),
           prepare(w=64), prepare(st=3), prepare(ch=0), prepare(ch=last), prepare(c=nop), prepare(c=None),
           prepare(sc=0.0), prepare(sc=-1.0), prepare(w=1, k=1), prepare(a=np.array([1.0, np.inf])),
           prepare(a=np.array([np.nan, 1.0]))]
    assert bad == [1] * len(bad), bad

    M = 2 * PA.Conv.slots(width, slotstr)
    ins = [t.full((2 * QlP * n,), 3, dtype=t.int64, device="cuda") for _ in range(2)]
    pts = [t.full((QlP * M,), 3, dtype=t.int64, device="cuda") for _ in range(4)]
    table = to_dev(np.array([ptr(x) for x in pts], dtype=np.uint64))
    accs = [t.full((2 * QlP * n,), 7, dtype=t.int64, device="cuda") for _ in range(2)]

    def mac(c=ctx, ch=chain, ins_=_vp(ins), T=2, tab=ptr(table), m_=M, O__=2, outs_=_vp(accs), r=_vp(res),
            m=mult.ctypes.data, b=bias.ctypes.data):
        return lib.phantom_ext_mac_sub_seeded(c.handle, ch, ins_, T, tab, m_, O__, outs_, r, m, b, s)

    bad = [mac(m=None), mac(m=None, b=None), mac(ins_=None), mac(tab=None), mac(outs_=None), mac(T=0), mac(O__=0),
           mac(ch=0), mac(ch=last), mac(c=nop), mac(m_=0), mac(m_=96), mac(m_=2 * n)]
    assert bad == [1] * len(bad), bad

    t.cuda.synchronize()
    for o in outs + accs:
        assert bool((o == 7).all())
