"""Prepared convolution layers with compact sparse-packed weights on the GPU, bit-exact:

  phantom_sub_ntt          the size-M subring transform == every g-th word of or_ntt_fwd of the
                           zero-stuffed size-N polynomial (tests/test_sub_ring.py pins that reference)
  phantom_ckks_encode_sub  == a degree-M context's embedding and rounding, zero-stuffed, through
                           or_ntt_fwd; with sub_slots = N/2 == phantom_ckks_encode
  ... accuracy at small M  decode of the expanded plaintext against phantom_ckks_encode(sparse_slots)
  phantom_ext_mac_sub      == or_lt_bsgs on the plaintexts expanded with np.repeat
  phantom_conv2d_apply     == the step-by-step composition of the C-ABI entries it is made of
  refused arguments        status 1, outputs untouched"""
import ctypes

import numpy as np
import pytest

import edge_cases as E
import oracle_lib as O
import phantom_amd as PA
from gpu_util import ptr, stream, to_dev, to_host, torch
from test_gpu_conv import (CONV_N, CONV_SCALE, EDGE_CASES, EDGE_N, _conv_operands, _Dev, _ext_mods, _key_arrays, _vp,
                           conv_ctx, ctxs, edge_ctxs)  # noqa: F401 (fixtures)

pytestmark = pytest.mark.gpu

N = 1 << 12


def _lib():
    return PA.load()


def _expand(pt, L, M, n):
    """compact [L][M] -> full-size [L][n], each word repeated n / M times"""
    return np.repeat(pt.reshape(L, M), n // M, axis=1).reshape(-1)


def _stuffed_ntt(coeffs, L, M, n, mods):
    """[.., L, M] coefficient residues of p' -> every g-th word of NTT_n(p'(X^g)), which is block-constant"""
    lead = coeffs.shape[:-2]
    c = coeffs.reshape(-1, L, M)
    out = np.empty_like(c)
    g = n // M
    for i in range(c.shape[0]):
        full = np.zeros((L, n), dtype=np.uint64)
        full[:, ::g] = c[i]
        f = O.ntt_fwd(full.reshape(-1), n, mods).reshape(L, M, g)
        assert np.all(f == f[:, :, :1])
        out[i] = f[:, :, 0]
    return out.reshape(lead + (L, M))


# ---- 1. the subring transform ------------------------------------------------------------------

@pytest.mark.parametrize("M", [8, 32, 128, 1024, 2048, 4096])
@pytest.mark.parametrize("chain_kind", ["59", "mixed", "61"])
def test_sub_ntt(ctxs, conv_ctx, rng, chain_kind, M):
    """the 1-D path (M < 2^10), the first 2-D size and M = N, over integer and FP64 limbs"""
    ctx = conv_ctx if chain_kind == "mixed" else ctxs(int(chain_kind))
    chain, count = 1, 2
    em = _ext_mods(ctx, chain)
    L = len(em)
    a = np.stack([O.random_limbs(rng, M, em).reshape(L, M) for _ in range(count)])
    want = _stuffed_ntt(a, L, M, N, em)
    d = to_dev(a.reshape(-1))
    PA.check(_lib().phantom_sub_ntt(ctx.handle, chain, 1, M, 0, ptr(d), count, stream()))
    assert np.array_equal(to_host(d).reshape(count, L, M), want)
    PA.check(_lib().phantom_sub_ntt(ctx.handle, chain, 1, M, 1, ptr(d), count, stream()))
    assert np.array_equal(to_host(d).reshape(count, L, M), a)


# ---- 2. the compact encoder, exact -------------------------------------------------------------

@pytest.fixture(scope="module")
def small_ctxs(conv_ctx):
    made = {}

    def get(M):
        if M not in made:
            made[M] = PA.Context(M, conv_ctx.moduli, conv_ctx.size_P)
        return made[M]

    yield get
    for c in made.values():
        c.close()


@pytest.mark.parametrize("ext", [0, 1])
@pytest.mark.parametrize("sub_slots", [512, 1024])
def test_encode_sub_exact(conv_ctx, small_ctxs, rng, sub_slots, ext):
    t, s = torch(), stream()
    ctx, chain, count, M = conv_ctx, 1, 3, 2 * sub_slots
    num = sub_slots - 3  # zero-padded to sub_slots
    mods = _ext_mods(ctx, chain) if ext else ctx.ql(chain)
    L = len(mods)
    vals = rng.uniform(-1, 1, size=(count, num)) + 1j * rng.uniform(-1, 1, size=(count, num))
    dv = t.from_numpy(vals.view(np.float64).copy()).cuda()
    out = t.zeros(count * L * M, dtype=t.int64, device="cuda")
    PA.check(_lib().phantom_ckks_encode_sub(ctx.handle, chain, ext, dv.data_ptr(), num, sub_slots, CONV_SCALE, count,
                                            ptr(out), None, s))
    got = to_host(out).reshape(count, L, M)
    # the degree-M context's coefficients
    small = small_ctxs(M)
    padded = np.zeros((count, sub_slots), dtype=np.complex128)
    padded[:, :num] = vals
    dp = t.from_numpy(padded.view(np.float64).copy()).cuda()
    coeffs = t.zeros(count * M, dtype=t.float64, device="cuda")
    PA.check(_lib().phantom_ckks_embed(small.handle, 0, dp.data_ptr(), coeffs.data_ptr(), 0, count, s))
    res = t.zeros(count * L * M, dtype=t.int64, device="cuda")
    PA.check(_lib().phantom_ckks_round_rns(small.handle, chain, ext, coeffs.data_ptr(), CONV_SCALE, count, 0, ptr(res),
                                           None, s))
    want = _stuffed_ntt(to_host(res).reshape(count, L, M), L, M, N, mods)
    assert got.any()
    assert np.array_equal(got, want)


def test_encode_sub_full_degree_is_encode(rng):
    """sub_slots = N/2: the context's own tables, phantom_ckks_encode bit for bit"""
    t, s = torch(), stream()
    n, count = 1 << 13, 2
    ctx = PA.Context(n, PA.coeff_modulus_create(n, [60, 50, 50, 60]), 1)
    L = len(_ext_mods(ctx, 1))
    vals = rng.uniform(-1, 1, size=(count, n // 2)) + 1j * rng.uniform(-1, 1, size=(count, n // 2))
    dv = t.from_numpy(vals.view(np.float64).copy()).cuda()
    a = t.zeros(count * L * n, dtype=t.int64, device="cuda")
    b = t.zeros(count * L * n, dtype=t.int64, device="cuda")
    PA.check(_lib().phantom_ckks_encode_sub(ctx.handle, 1, 1, dv.data_ptr(), n // 2, n // 2, CONV_SCALE, count, ptr(a),
                                            None, s))
    PA.check(_lib().phantom_ckks_encode(ctx.handle, 1, 1, dv.data_ptr(), n // 2, 0, CONV_SCALE, count, ptr(b), None, s))
    ga, gb = to_host(a), to_host(b)
    ctx.close()
    assert gb.any() and np.array_equal(ga, gb)


# ---- 3. the compact encoder, accuracy at small M ------------------------------------------------

@pytest.mark.parametrize("sub_slots", [16, 64])
def test_encode_sub_accuracy(conv_ctx, rng, sub_slots):
    """decode(expanded compact plaintext) is at most twice as far from the values as the existing
    sparse encode -> decode (the two round different coefficient vectors)"""
    t, s = torch(), stream()
    ctx, chain, count, M, scale = conv_ctx, 1, 8, 2 * sub_slots, float(1 << 40)
    ql = ctx.ql(chain)
    L = len(ql)
    vals = rng.uniform(-1, 1, size=(count, sub_slots)) + 1j * rng.uniform(-1, 1, size=(count, sub_slots))
    dv = t.from_numpy(vals.view(np.float64).copy()).cuda()
    sub = t.zeros(count * L * M, dtype=t.int64, device="cuda")
    PA.check(_lib().phantom_ckks_encode_sub(ctx.handle, chain, 0, dv.data_ptr(), sub_slots, sub_slots, scale, count,
                                            ptr(sub), None, s))
    compact = to_host(sub).reshape(count, L, M)
    full = t.zeros(count * L * N, dtype=t.int64, device="cuda")
    PA.check(_lib().phantom_ckks_encode(ctx.handle, chain, 0, dv.data_ptr(), sub_slots, sub_slots, scale, count,
                                        ptr(full), None, s))

    def decode_error(plain):
        out = t.zeros(count * (N // 2) * 2, dtype=t.float64, device="cuda")
        PA.check(_lib().phantom_ckks_decode(ctx.handle, chain, ptr(plain), scale, count, out.data_ptr(), s))
        t.cuda.synchronize()
        z = out.cpu().numpy().view(np.complex128).reshape(count, N // 2)
        return float(np.abs(z - np.tile(vals, (1, N // 2 // sub_slots))).max())

    expanded = to_dev(np.stack([_expand(compact[p].reshape(-1), L, M, N) for p in range(count)]).reshape(-1))
    e_sub, e_full = decode_error(expanded), decode_error(full)
    print(f"sub_slots={sub_slots}: compact max error {e_sub:.3e}, existing sparse encode {e_full:.3e}")
    assert e_full < 1e-6
    assert e_sub <= 2 * e_full
    # coefficient form over the subring: every limb holds the same centred integer
    PA.check(_lib().phantom_sub_ntt(ctx.handle, chain, 0, M, 1, ptr(sub), count, s))
    r = to_host(sub).reshape(count, L, M)
    q = np.array(ql, dtype=np.uint64).reshape(1, L, 1)
    centred = np.where(r > q // 2, r.astype(np.int64) - q.astype(np.int64), r.astype(np.int64))
    assert np.all(centred == centred[:, :1, :])
    assert centred.any()


# ---- 4. inner sums over compact plaintexts -------------------------------------------------------

def _mac_sub(ctx, chain, n, M, ins, pts, O_, old):
    """phantom_ext_mac_sub with accumulate 0 and 1, and the oracle on the expanded plaintexts;
    returns (got0, got1, want, want + old mod q)"""
    T = len(ins)
    em = _ext_mods(ctx, chain)
    L = len(em)
    dev = _Dev()
    din, dpt = [dev(x) for x in ins], [dev(x) for x in pts]
    table = to_dev(np.array([ptr(x) for x in dpt], dtype=np.uint64))
    got = []
    for accumulate in (0, 1):
        douts = [to_dev(o) for o in old]
        PA.check(_lib().phantom_ext_mac_sub(ctx.handle, chain, _vp(din), T, ptr(table), M, O_, _vp(douts), accumulate,
                                            stream()))
        got.append([to_host(d) for d in douts])
    cache = {}
    full = []
    for x in pts:
        if id(x) not in cache:
            cache[id(x)] = _expand(x, L, M, n)
        full.append(cache[id(x)])
    want = [np.zeros(2 * L * n, dtype=np.uint64) for _ in range(O_)]
    O.lib().or_lt_bsgs(O.ptrs(ins), T, O.ptrs(full), O_, O.ptrs(want), n, len(ctx.ql(chain)), ctx.size_Q, ctx.size_P,
                       O.P(O.arr(ctx.moduli)))
    q = np.tile(np.repeat(np.array(em, dtype=np.uint64), n), 2)
    acc = []
    for o in range(O_):
        sm = want[o] + old[o]  # both below q < 2^61: no wrap
        acc.append(np.where(sm >= q, sm - q, sm))
    return got[0], got[1], want, acc


def _pooled_sub(rng, n, M, em, T, O_):
    rand = lambda size, polys: np.concatenate([O.random_limbs(rng, size, em) for _ in range(polys)])
    pin, ppt = [rand(n, 2) for _ in range(min(T, 12))], [rand(M, 1) for _ in range(min(T * O_, 20))]
    ins = [pin[(5 * t + 1) % len(pin)] for t in range(T)]
    pts = [ppt[(7 * k + k // T) % len(ppt)] for k in range(T * O_)]
    return ins, pts


@pytest.mark.parametrize("log_gap", [0, 1, 5, 6, 7, 8, 9])
@pytest.mark.parametrize("T,O_", [(1, 1), (27, 2), (33, 9), (144, 17)])
@pytest.mark.parametrize("bits", [59, 61])
def test_ext_mac_sub(ctxs, rng, bits, T, O_, log_gap):
    """n = 4096, the tiled kernel: gaps on both sides of a lane's element pair (1 | 2) and of the
    128-element tile (64 | 128); one term, a tail block, a block boundary, and 17 outputs (two
    workgroup rows, the second with one live wave)"""
    n, chain = N, 1
    ctx = ctxs(bits)
    em = _ext_mods(ctx, chain)
    M = n >> log_gap
    ins, pts = _pooled_sub(rng, n, M, em, T, O_)
    old = [np.concatenate([O.random_limbs(rng, n, em) for _ in range(2)]) for _ in range(O_)]
    got0, got1, want, acc = _mac_sub(ctx, chain, n, M, ins, pts, O_, old)
    for o in range(O_):
        assert np.array_equal(got0[o], want[o]), (bits, T, O_, log_gap, o)
        assert np.array_equal(got1[o], acc[o]), (bits, T, O_, log_gap, o, "accumulate")


@pytest.mark.parametrize("log_gap", [3, 8])
@pytest.mark.parametrize("pair", [("max", "max"), ("lowmax", "lowmax"), ("max", "lowmax")], ids="-".join)
@pytest.mark.parametrize("kind,T", EDGE_CASES)
def test_ext_mac_sub_edges(edge_ctxs, kind, T, pair, log_gap):
    """every operand at q - 1 / low 30 bits all ones, on either side of each fold and of the 128-bit
    sum's capacity (tests/test_gpu_conv.py test_ext_mac_edges), n = 1024"""
    ctx, chain, n = edge_ctxs(kind), 1, EDGE_N
    em = _ext_mods(ctx, chain)
    M = n >> log_gap
    a = np.concatenate([E.edge_limbs(n, em, pair[0])] * 2)
    b = E.edge_limbs(M, em, pair[1])
    for O_ in (1, 2):
        old = [np.full(2 * len(em) * n, 5, dtype=np.uint64)] * O_
        got0, got1, want, acc = _mac_sub(ctx, chain, n, M, [a] * T, [b] * (T * O_), O_, old)
        for o in range(O_):
            assert np.array_equal(got0[o], want[o]), (kind, T, pair, log_gap, O_, o)
            assert np.array_equal(got1[o], acc[o]), (kind, T, pair, log_gap, O_, o, "accumulate")


def test_ext_mac_sub_small_n(ctxs, rng):
    """n = 512: the one-element-per-thread form, gap 8, 33 terms x 3 outputs"""
    n, chain, T, O_, log_gap = 512, 1, 33, 3, 3
    ctx = ctxs(50, n)
    em = _ext_mods(ctx, chain)
    M = n >> log_gap
    ins, pts = _pooled_sub(rng, n, M, em, T, O_)
    old = [np.concatenate([O.random_limbs(rng, n, em) for _ in range(2)]) for _ in range(O_)]
    got0, got1, want, acc = _mac_sub(ctx, chain, n, M, ins, pts, O_, old)
    for o in range(O_):
        assert np.array_equal(got0[o], want[o]), o
        assert np.array_equal(got1[o], acc[o]), (o, "accumulate")


# ---- 5. the plan ---------------------------------------------------------------------------------

def _plan_steps(ctx, chain, shape, cts, keysets, dnum, elts, W):
    """the prepared layer as the C-ABI entries phantom_conv2d_prepare / _apply name, one call each"""
    width, slotstr, K, in_ch, out_ch = shape
    t, lib, s = torch(), _lib(), stream()
    n, Ql = CONV_N, len(ctx.ql(chain))
    QlP, K2 = Ql + ctx.size_P, K * K
    T, ns, beta = in_ch * K2, PA.Conv.slots(width, slotstr), -(-Ql // ctx.size_P)
    M = 2 * ns
    zeros = lambda words: t.zeros(words, dtype=t.int64, device="cuda")
    kk, keep = _key_arrays(keysets, K2)
    el = (ctypes.c_uint32 * K2)(*elts)
    rot = [zeros(2 * QlP * n) for _ in range(T)]
    digits = zeros(beta * QlP * n)
    for k in range(in_ch):
        PA.check(lib.phantom_modup(ctx.handle, chain, ptr(cts[k]) + 8 * Ql * n, ptr(digits), s))
        PA.check(lib.phantom_fast_rotation_ext_batch(ctx.handle, chain, ptr(cts[k]), ptr(digits), kk, dnum, el, K2,
                                                     _vp(rot[k * K2:(k + 1) * K2]), s))
    slots = t.zeros((out_ch * T, ns, 2), dtype=t.float64, device="cuda")
    PA.Conv.weight_slots(shape, W.data_ptr(), 0, out_ch * T, slots.data_ptr(), s)
    pts = zeros(out_ch * T * QlP * M)
    PA.check(lib.phantom_ckks_encode_sub(ctx.handle, chain, 1, slots.data_ptr(), ns, ns, CONV_SCALE, out_ch * T,
                                         ptr(pts), None, s))
    table = to_dev(np.array([ptr(pts) + 8 * QlP * M * k for k in range(out_ch * T)], dtype=np.uint64))
    acc = [zeros(2 * QlP * n) for _ in range(out_ch)]
    PA.check(lib.phantom_ext_mac_sub(ctx.handle, chain, _vp(rot), T, ptr(table), M, out_ch, _vp(acc), 0, s))
    outs = [zeros(2 * Ql * n) for _ in range(out_ch)]
    for h in range(out_ch):
        for p in range(2):
            PA.check(lib.phantom_moddown_from_ntt(ctx.handle, chain, ptr(acc[h]) + 8 * p * QlP * n,
                                                  ptr(outs[h]) + 8 * p * Ql * n, s))
    return [to_host(o) for o in outs]


def _apply(ctx, chain, shape, plan, cts, keysets, dnum, elts):
    width, slotstr, K, in_ch, out_ch = shape
    t = torch()
    words = 2 * len(ctx.ql(chain)) * CONV_N
    outs = [t.full((words,), 7, dtype=t.int64, device="cuda") for _ in range(out_ch)]
    kk, keep = _key_arrays(keysets, K * K)
    el = (ctypes.c_uint32 * (K * K))(*elts)
    PA.Conv.apply(ctx, plan, _vp(cts), kk, dnum, el, _vp(outs), stream())
    return [to_host(o) for o in outs]


@pytest.mark.parametrize("chain,shape", [(1, (8, 0, 3, 3, 2)), (1, (4, 1, 3, 4, 3)), (1, (8, 0, 5, 2, 2)),
                                         (2, (4, 0, 3, 2, 2))], ids=str)
def test_conv_plan(conv_ctx, rng, chain, shape):
    """apply == its step-by-step composition, on a second input too, after dev_W has been overwritten"""
    width, slotstr, K, in_ch, out_ch = shape
    ctx = conv_ctx
    cts, keysets, dnum, elts, W = _conv_operands(rng, ctx, chain, shape)
    want = _plan_steps(ctx, chain, shape, cts, keysets, dnum, elts, W)
    plan = PA.Conv.prepare(ctx, chain, shape, W.data_ptr(), CONV_SCALE, stream())
    try:
        QlP = len(ctx.ql(chain)) + ctx.size_P
        assert plan.bytes == 8 * out_ch * in_ch * K * K * QlP * 2 * PA.Conv.slots(width, slotstr)
        got = _apply(ctx, chain, shape, plan, cts, keysets, dnum, elts)
        for h in range(out_ch):
            assert np.array_equal(got[h], want[h]), h
            assert want[h].any()
        cts2 = _conv_operands(rng, ctx, chain, shape)[0]
        want2 = _plan_steps(ctx, chain, shape, cts2, keysets, dnum, elts, W)
        W.fill_(123.0)  # the plan never reads dev_W again
        got2 = _apply(ctx, chain, shape, plan, cts2, keysets, dnum, elts)
        for h in range(out_ch):
            assert np.array_equal(got2[h], want2[h]), h
            assert not np.array_equal(want2[h], want[h])
    finally:
        plan.close()


# ---- 6. refused arguments --------------------------------------------------------------------------

def test_plan_refused_arguments(conv_ctx, rng, request):
    """every bad argument returns PHANTOM_ERR_INVALID_ARGUMENT (1) and nothing is written"""
    t, lib, s = torch(), _lib(), stream()
    ctx, chain, n = conv_ctx, 1, CONV_N
    shape = (8, 0, 3, 2, 2)
    width, slotstr, K, in_ch, out_ch = shape
    cts, keysets, dnum, elts, W = _conv_operands(rng, ctx, chain, shape)
    Ql, QlP = len(ctx.ql(chain)), len(ctx.ql(chain)) + ctx.size_P
    outs = [t.full((2 * Ql * n,), 7, dtype=t.int64, device="cuda") for _ in range(out_ch)]
    kk, keep = _key_arrays(keysets, K * K)
    el = (ctypes.c_uint32 * (K * K))(*elts)
    nokey, keep2 = _key_arrays(keysets, K * K)
    nokey[0] = None  # a tap other than the centre without a key
    nop = PA.Context(n, PA.coeff_modulus_create(n, [60, 50, 50]), 0)  # no special prime
    other = PA.Context(n, ctx.moduli, ctx.size_P)
    request.addfinalizer(nop.close)  # closed however the test ends
    request.addfinalizer(other.close)
    last = len(ctx.moduli) - ctx.size_P + 1  # one past the last chain index

    def prepare(c=ctx, ch=chain, i=in_ch, o=out_ch, w=width, st=slotstr, k=K, dw=W.data_ptr(), sc=CONV_SCALE,
                out=True):
        h = ctypes.c_void_p()
        r = lib.phantom_conv2d_prepare(c.handle if c else None, ch, i, o, w, st, k, dw, sc, None, s,
                                       ctypes.byref(h) if out else None)
        assert r != 0 and not h.value
        return r

    bad = [prepare(dw=None), prepare(out=False), prepare(i=0), prepare(o=0), prepare(k=2), prepare(k=9), prepare(w=6),
           prepare(w=64), prepare(st=3), prepare(ch=0), prepare(ch=last), prepare(c=nop), prepare(c=None),
           prepare(sc=0.0), prepare(sc=-1.0), prepare(w=1, k=1)]  # the last: 2 ns = 2 < 8
    assert bad == [1] * len(bad), bad

    plan = PA.Conv.prepare(ctx, chain, shape, W.data_ptr(), CONV_SCALE, s)
    request.addfinalizer(plan.close)

    def apply(c=ctx, p=plan.handle, cts_=_vp(cts), keys=kk, e=el, outs_=_vp(outs)):
        return lib.phantom_conv2d_apply(c.handle if c else None, p, cts_, keys, dnum, e, outs_, s)

    one_null = _vp(cts)
    one_null[1] = None
    bad = [apply(c=other), apply(c=None), apply(p=None), apply(cts_=None), apply(keys=None), apply(e=None),
           apply(outs_=None), apply(keys=nokey), apply(cts_=one_null)]
    assert bad == [1] * len(bad), bad
    b = ctypes.c_size_t(0)
    assert lib.phantom_conv_plan_bytes(None, ctypes.byref(b)) == 1 and lib.phantom_conv_plan_bytes(plan.handle, None) == 1

    ns = PA.Conv.slots(width, slotstr)
    M = 2 * ns
    ins = [t.full((2 * QlP * n,), 3, dtype=t.int64, device="cuda") for _ in range(2)]
    pts = [t.full((QlP * M,), 3, dtype=t.int64, device="cuda") for _ in range(4)]
    table = to_dev(np.array([ptr(x) for x in pts], dtype=np.uint64))
    accs = [t.full((2 * QlP * n,), 7, dtype=t.int64, device="cuda") for _ in range(2)]

    def mac(c=ctx, ch=chain, ins_=_vp(ins), T=2, tab=ptr(table), m=M, O_=2, outs_=_vp(accs)):
        return lib.phantom_ext_mac_sub(c.handle, ch, ins_, T, tab, m, O_, outs_, 0, s)

    bad = [mac(ins_=None), mac(tab=None), mac(outs_=None), mac(T=0), mac(O_=0), mac(ch=0), mac(ch=last), mac(c=nop),
           mac(m=0), mac(m=96), mac(m=2 * n)]
    assert bad == [1] * len(bad), bad

    vals = t.full((2 * ns,), 0.5, dtype=t.float64, device="cuda")
    enc_out = t.full((QlP * M,), 7, dtype=t.int64, device="cuda")

    def enc(c=ctx, ch=chain, v=vals.data_ptr(), num=ns, sub=ns, sc=CONV_SCALE, out=ptr(enc_out)):
        return lib.phantom_ckks_encode_sub(c.handle, ch, 1, v, num, sub, sc, 1, out, None, s)

    def sub_ntt(c=ctx, ch=chain, m=M, data=ptr(enc_out)):
        return lib.phantom_sub_ntt(c.handle, ch, 1, m, 0, data, 1, s)

    bad = [enc(v=None), enc(out=None), enc(sub=2), enc(sub=48), enc(sub=n), enc(num=ns + 1), enc(ch=0), enc(ch=last),
           enc(sc=0.0), enc(sc=-2.0),
           sub_ntt(m=4), sub_ntt(m=96), sub_ntt(m=2 * n), sub_ntt(data=None), sub_ntt(ch=0), sub_ntt(ch=last)]
    assert bad == [1] * len(bad), bad

    t.cuda.synchronize()
    for o in outs + accs + [enc_out]:
        assert bool((o == 7).all())
