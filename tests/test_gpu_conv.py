"""The hoisted encrypted convolution's kernels and C-ABI on the GPU, bit-exact:

  phantom_ext_mac            general inner sums over the extended basis == or_lt_bsgs(ins, T, pts, O)
                             (the oracle reduces every product; it takes any number of terms)
  ... at the edges           the largest 60-bit prime, the smallest above 2^60 and the largest 61-bit
                             one with every operand at q - 1 / low halves all ones: 65 (257) products
                             overflow a 128-bit sum that is never reduced on the way
  phantom_conv_weight_slots  == its host twin == numpy
  phantom_conv2d             == the step-by-step composition of the C-ABI entries it is made of
  refused arguments          status 1, outputs untouched

Operands of the integer kernels are uniform random residues or edge patterns (parity is a property
of the arithmetic, not of key or ciphertext structure)."""
import ctypes

import numpy as np
import pytest

import edge_cases as E
import oracle_lib as O
import phantom_amd as PA
from gpu_util import ptr, stream, to_dev, to_host, torch
from test_conv_host import np_weight_slots

pytestmark = pytest.mark.gpu


def _lib():
    return PA.load()


def _vp(ts):
    return PA.ptr_array([ptr(t) for t in ts])


def _ext_mods(ctx, chain):
    return ctx.ql(chain) + ctx.moduli[ctx.size_Q:]


class _Dev:
    """device copies of host arrays, one per distinct array (pools and constant patterns repeat)"""

    def __init__(self):
        self.made = {}

    def __call__(self, a):
        if id(a) not in self.made:
            self.made[id(a)] = (a, to_dev(a))
        return self.made[id(a)][1]


def _mac(ctx, chain, n, ins, pts, O_, outs_init, accumulate=0):
    """runs phantom_ext_mac and the oracle; returns (got, want) lists of [2][L][n] arrays"""
    T = len(ins)
    em = _ext_mods(ctx, chain)
    dev = _Dev()
    din, dpt = [dev(x) for x in ins], [dev(x) for x in pts]
    table = to_dev(np.array([ptr(x) for x in dpt], dtype=np.uint64))
    douts = [to_dev(o) for o in outs_init]
    PA.check(_lib().phantom_ext_mac(ctx.handle, chain, _vp(din), T, ptr(table), O_, _vp(douts), accumulate, stream()))
    want = [np.zeros(2 * len(em) * n, dtype=np.uint64) for _ in range(O_)]
    O.lib().or_lt_bsgs(O.ptrs(ins), T, O.ptrs(pts), O_, O.ptrs(want), n, len(ctx.ql(chain)), ctx.size_Q, ctx.size_P,
                       O.P(O.arr(ctx.moduli)))
    return [to_host(d) for d in douts], want


def _pooled(rng, n, em, T, O_):
    """T inputs and T O plaintexts drawn from small pools of distinct random arrays"""
    rand = lambda polys: np.concatenate([O.random_limbs(rng, n, em) for _ in range(polys)])
    pin, ppt = [rand(2) for _ in range(min(T, 12))], [rand(1) for _ in range(min(T * O_, 20))]
    ins = [pin[(5 * t + 1) % len(pin)] for t in range(T)]
    pts = [ppt[(7 * k + k // T) % len(ppt)] for k in range(T * O_)]
    return ins, pts


@pytest.fixture(scope="module")
def ctxs():
    made = {}

    def get(bits, n=1 << 12):
        if (bits, n) not in made:
            made[(bits, n)] = PA.Context(n, O.coeff_modulus_create(n, [bits] * 10), 2)
        return made[(bits, n)]

    yield get
    for c in made.values():
        c.close()


@pytest.mark.parametrize("T,O_", [(1, 1), (27, 2), (33, 9), (144, 3)])
@pytest.mark.parametrize("bits", [59, 61])
def test_ext_mac(ctxs, rng, bits, T, O_):
    """n = 4096, 8 + 2 moduli, the tiled kernel: one term; a tail block; more than 8 outputs (two
    workgroup rows) across a block boundary; 4.5 blocks.  59-bit moduli fold every 8 products, 61-bit
    every 4."""
    n, chain = 1 << 12, 1
    ctx = ctxs(bits)
    em = _ext_mods(ctx, chain)
    ins, pts = _pooled(rng, n, em, T, O_)
    got, want = _mac(ctx, chain, n, ins, pts, O_, [np.full(2 * len(em) * n, 5, dtype=np.uint64)] * O_)
    for o in range(O_):
        assert np.array_equal(got[o], want[o]), (bits, T, O_, o)


def test_ext_mac_small_n(ctxs, rng):
    """n = 512: the one-element-per-thread kernel, 33 terms (a reduction inside the sum) x 3 outputs"""
    n, chain, T, O_ = 512, 1, 33, 3
    ctx = ctxs(50, n)
    em = _ext_mods(ctx, chain)
    ins, pts = _pooled(rng, n, em, T, O_)
    got, want = _mac(ctx, chain, n, ins, pts, O_, [np.full(2 * len(em) * n, 5, dtype=np.uint64)] * O_)
    for o in range(O_):
        assert np.array_equal(got[o], want[o]), o


@pytest.mark.parametrize("n", [1 << 12, 512])
def test_ext_mac_accumulate(ctxs, rng, n):
    """accumulate = 1 adds the residues already in the outputs (both kernels)"""
    chain, T, O_ = 1, 27, 2
    ctx = ctxs(59 if n > 512 else 50, n)
    em = _ext_mods(ctx, chain)
    ins, pts = _pooled(rng, n, em, T, O_)
    old = [np.concatenate([O.random_limbs(rng, n, em) for _ in range(2)]) for _ in range(O_)]
    got, want = _mac(ctx, chain, n, ins, pts, O_, old, accumulate=1)
    q = np.tile(np.repeat(np.array(em, dtype=np.uint64), n), 2)
    for o in range(O_):
        s = want[o] + old[o]  # both below q < 2^61: no wrap
        assert np.array_equal(got[o], np.where(s >= q, s - q, s)), o


# ---- edges -----------------------------------------------------------------------------------

EDGE_N = 1024
EDGE_KINDS = {"<2^60": ("below", 1 << 60), ">2^60": ("above", 1 << 60), "<2^61": ("below", 1 << 61)}
EDGE_T = {"<2^60": [16, 17, 256, 257], ">2^60": [4, 5, 16, 17, 64, 65], "<2^61": [4, 5, 16, 17, 64, 65]}
EDGE_CASES = [(k, t) for k in EDGE_KINDS for t in EDGE_T[k]]


def _edge_chain(kind):
    """2 + 1 distinct primes = 1 (mod 2 n) next to the bound, the nearest first"""
    side, bound = EDGE_KINDS[kind]
    ps = []
    for _ in range(3):
        p = E.prime_below(bound, EDGE_N) if side == "below" else E.prime_above(bound, EDGE_N)
        ps.append(p)
        bound = p if side == "below" else p + 1
    return ps


@pytest.fixture(scope="module")
def edge_ctxs():
    made = {}

    def get(kind):
        if kind not in made:
            made[kind] = PA.Context(EDGE_N, _edge_chain(kind), 1)
        return made[kind]

    yield get
    for c in made.values():
        c.close()


def test_edge_chains():
    assert _edge_chain("<2^60")[0] == E.prime_below(1 << 60, EDGE_N) and max(_edge_chain("<2^60")) < 1 << 60
    assert _edge_chain(">2^60")[0] == E.prime_above(1 << 60, EDGE_N) and min(_edge_chain(">2^60")) > 1 << 60
    assert _edge_chain("<2^61")[0] == E.prime_below(1 << 61, EDGE_N) and min(_edge_chain("<2^61")) > 1 << 60
    # what the kernel must survive: 65 (257) products of q - 1 do not fit 128 bits, 64 (256) do
    q = E.prime_below(1 << 61, EDGE_N)
    assert 64 * (q - 1) ** 2 < 1 << 128 <= 65 * (q - 1) ** 2
    q = E.prime_below(1 << 60, EDGE_N)
    assert 256 * (q - 1) ** 2 < 1 << 128 <= 257 * (q - 1) ** 2


@pytest.mark.parametrize("pair", [("max", "max"), ("lowmax", "lowmax"), ("max", "lowmax")], ids="-".join)
@pytest.mark.parametrize("kind,T", EDGE_CASES)
def test_ext_mac_edges(edge_ctxs, kind, T, pair):
    """every operand at q - 1 / low 30 bits all ones, on either side of each fold (4 | 5, 16 | 17
    products per partial sum) and of the 128-bit sum's capacity (64 | 65, 256 | 257 products)"""
    ctx, chain, n = edge_ctxs(kind), 1, EDGE_N
    em = _ext_mods(ctx, chain)
    a = np.concatenate([E.edge_limbs(n, em, pair[0])] * 2)
    b = E.edge_limbs(n, em, pair[1])
    for O_ in (1, 2):
        got, want = _mac(ctx, chain, n, [a] * T, [b] * (T * O_), O_, [np.full(2 * len(em) * n, 5, dtype=np.uint64)] * O_)
        for o in range(O_):
            assert np.array_equal(got[o], want[o]), (kind, T, pair, O_, o)


@pytest.mark.parametrize("fill", ["max", "lowmax"])
@pytest.mark.parametrize("kind", list(EDGE_KINDS))
def test_ext_mac_near_multiple(edge_ctxs, kind, fill):
    """sums that are -1, 0 and 1 modulo q (coefficient k: (k mod 3) - 1) with every operand but the
    last plaintext at its maximum, one term past the 128-bit sum's capacity"""
    ctx, chain, n = edge_ctxs(kind), 1, EDGE_N
    em = _ext_mods(ctx, chain)
    T = EDGE_T[kind][-1]
    a = np.concatenate([E.edge_limbs(n, em, fill)] * 2)
    pts = []
    for o, fb in enumerate(("max", "lowmax")):
        b = E.edge_limbs(n, em, fb)
        last = np.zeros(len(em) * n, dtype=np.uint64)
        for l, q in enumerate(em):
            for t in (-1, 0, 1):
                last[l * n + (t + 1):(l + 1) * n:3] = E.near_multiple_operands(q, T, t, fill, fb)[1][-1]
        pts += [b] * (T - 1) + [last]
    got, want = _mac(ctx, chain, n, [a] * T, pts, 2, [np.full(2 * len(em) * n, 5, dtype=np.uint64)] * 2)
    for o in range(2):
        rows = want[o].reshape(2, len(em), n)
        for l, q in enumerate(em):
            for t in (-1, 0, 1):
                assert np.all(rows[:, l, (t + 1)::3] == np.uint64(t % q))
        assert np.array_equal(got[o], want[o]), (kind, fill, o)


# ---- weight slot vectors ----------------------------------------------------------------------

@pytest.mark.parametrize("shape", [(8, 0, 3, 3, 2), (4, 1, 3, 2, 2)])
def test_weight_slots(rng, shape):
    width, slotstr, K, in_ch, out_ch = shape
    t = torch()
    W = rng.uniform(-1, 1, size=(K, K, in_ch, out_ch))
    terms, ns = out_ch * in_ch * K * K, PA.Conv.slots(width, slotstr)
    dW = t.from_numpy(W).cuda()
    for first, count in [(0, terms), (terms // 3, terms - terms // 3 - 1)]:
        dout = t.full((count, ns, 2), 7.0, dtype=t.float64, device="cuda")
        PA.Conv.weight_slots(shape, dW.data_ptr(), first, count, dout.data_ptr(), stream())
        t.cuda.synchronize()
        got = dout.cpu().numpy().view(np.complex128).reshape(count, ns)
        host = PA.Conv.weight_slots_host(shape, W, first, count)
        assert np.array_equal(got, host)
        assert np.array_equal(host, np_weight_slots(shape, W, first, count))


# ---- the whole layer --------------------------------------------------------------------------

CONV_N = 1 << 12
CONV_SCALE = float(1 << 40)


@pytest.fixture(scope="module")
def conv_ctx():
    ctx = PA.Context(CONV_N, PA.coeff_modulus_create(CONV_N, [60, 50, 50, 50, 60, 60]), 2)
    yield ctx
    ctx.close()


def _key_arrays(keysets, K2):
    """host array of K2 host arrays of device key-digit pointers, NULL at the centre tap"""
    arrays = [None if k == K2 // 2 else _vp(keysets[k % len(keysets)]) for k in range(K2)]
    kk = (ctypes.POINTER(ctypes.c_void_p) * K2)(*[ctypes.cast(a, ctypes.POINTER(ctypes.c_void_p)) if a is not None
                                                 else None for a in arrays])
    return kk, arrays


def _conv_operands(rng, ctx, chain, shape):
    width, slotstr, K, in_ch, out_ch = shape
    t = torch()
    n, ql = CONV_N, ctx.ql(chain)
    rand = lambda mods, polys=1: np.concatenate([O.random_limbs(rng, n, mods) for _ in range(polys)])
    cts = [to_dev(rand(ql, 2)) for _ in range(in_ch)]
    dnum = -(-ctx.size_Q // ctx.size_P)
    keysets = [[to_dev(rand(ctx.moduli, 2)) for _ in range(dnum)] for _ in range(3)]
    rots = PA.Conv.rotations(width, slotstr, K)
    elts = [pow(5, int(r) % (n // 2), 2 * n) for r in rots]
    W = t.from_numpy(rng.uniform(-1, 1, size=(K, K, in_ch, out_ch))).cuda()
    return cts, keysets, dnum, elts, W


def _conv_steps(ctx, chain, shape, cts, keysets, dnum, elts, W):
    """the layer as the C-ABI entries phantom_conv2d names, one call each"""
    width, slotstr, K, in_ch, out_ch = shape
    t, lib, s = torch(), _lib(), stream()
    n, Ql = CONV_N, len(ctx.ql(chain))
    QlP, K2 = Ql + ctx.size_P, K * K
    T, ns, beta = in_ch * K2, PA.Conv.slots(width, slotstr), -(-Ql // ctx.size_P)
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
    pts = zeros(out_ch * T * QlP * n)
    PA.check(lib.phantom_ckks_encode(ctx.handle, chain, 1, slots.data_ptr(), ns, ns, CONV_SCALE, out_ch * T, ptr(pts),
                                     None, s))
    table = to_dev(np.array([ptr(pts) + 8 * QlP * n * k for k in range(out_ch * T)], dtype=np.uint64))
    acc = [zeros(2 * QlP * n) for _ in range(out_ch)]
    PA.check(lib.phantom_ext_mac(ctx.handle, chain, _vp(rot), T, ptr(table), out_ch, _vp(acc), 0, s))
    outs = [zeros(2 * Ql * n) for _ in range(out_ch)]
    for h in range(out_ch):
        for p in range(2):
            PA.check(lib.phantom_moddown_from_ntt(ctx.handle, chain, ptr(acc[h]) + 8 * p * QlP * n,
                                                  ptr(outs[h]) + 8 * p * Ql * n, s))
    return [to_host(o) for o in outs]


def _conv2d(ctx, chain, shape, cts, keysets, dnum, elts, W, group, contiguous):
    width, slotstr, K, in_ch, out_ch = shape
    t = torch()
    words = 2 * len(ctx.ql(chain)) * CONV_N
    if contiguous:
        whole = t.full((out_ch * words,), 7, dtype=t.int64, device="cuda")
        outs = [whole[h * words:(h + 1) * words] for h in range(out_ch)]
    else:
        outs = [t.full((words,), 7, dtype=t.int64, device="cuda") for _ in range(out_ch)]
    kk, keep = _key_arrays(keysets, K * K)
    el = (ctypes.c_uint32 * (K * K))(*elts)
    PA.check(_lib().phantom_conv2d(ctx.handle, chain, _vp(cts), in_ch, out_ch, width, slotstr, K, W.data_ptr(),
                                   CONV_SCALE, kk, dnum, el, group, _vp(outs), None, stream()))
    return [to_host(o) for o in outs]


@pytest.mark.parametrize("shape", [(8, 0, 3, 3, 2), (4, 1, 3, 4, 3), (8, 0, 5, 2, 2)], ids=str)
def test_conv2d(conv_ctx, rng, shape):
    """the layer == its step-by-step composition; one output channel per pass == the engine's choice
    (27, 36 and 50 terms per output: a tail block, and two blocks of terms)"""
    chain = 1
    ops = _conv_operands(rng, conv_ctx, chain, shape)
    want = _conv_steps(conv_ctx, chain, shape, *ops)
    one = _conv2d(conv_ctx, chain, shape, *ops, group=1, contiguous=False)
    auto = _conv2d(conv_ctx, chain, shape, *ops, group=0, contiguous=True)
    for h in range(shape[4]):
        assert np.array_equal(one[h], want[h]), h
        assert np.array_equal(auto[h], want[h]), h
        assert want[h].any()


@pytest.mark.parametrize("shape", [(4, 0, 3, 2, 2), (16, 0, 11, 1, 1)], ids=str)
def test_conv2d_lower_level(conv_ctx, rng, shape):
    """chain index 2 (3 + 2 limbs, the last key-switch digit partial); K = 11 has 121 rotations, whose
    table is written in two pieces"""
    chain = 2
    ops = _conv_operands(rng, conv_ctx, chain, shape)
    want = _conv_steps(conv_ctx, chain, shape, *ops)
    got = _conv2d(conv_ctx, chain, shape, *ops, group=0, contiguous=False)
    for h in range(shape[4]):
        assert np.array_equal(got[h], want[h]), h


# ---- refused arguments -------------------------------------------------------------------------

def test_refused_arguments(conv_ctx, rng):
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
    last = len(ctx.moduli) - ctx.size_P + 1  # one past the last chain index

    def conv(c=ctx, ch=chain, cts_=_vp(cts), i=in_ch, o=out_ch, w=width, st=slotstr, k=K, dw=W.data_ptr(),
             sc=CONV_SCALE, keys=kk, e=el, outs_=_vp(outs)):
        return lib.phantom_conv2d(c.handle, ch, cts_, i, o, w, st, k, dw, sc, keys, dnum, e, 0, outs_, None, s)

    bad = [conv(cts_=None), conv(dw=None), conv(keys=None), conv(e=None), conv(outs_=None), conv(i=0), conv(o=0),
           conv(k=2), conv(k=9), conv(w=6), conv(w=64), conv(st=3), conv(ch=0), conv(ch=last), conv(c=nop),
           conv(sc=0.0), conv(sc=-1.0), conv(keys=nokey),
           lib.phantom_conv2d(None, chain, _vp(cts), in_ch, out_ch, width, slotstr, K, W.data_ptr(), CONV_SCALE, kk,
                              dnum, el, 0, _vp(outs), None, s)]
    assert bad == [1] * len(bad), bad

    ins = [t.full((2 * QlP * n,), 3, dtype=t.int64, device="cuda") for _ in range(2)]
    pts = [t.full((QlP * n,), 3, dtype=t.int64, device="cuda") for _ in range(4)]
    table = to_dev(np.array([ptr(x) for x in pts], dtype=np.uint64))
    accs = [t.full((2 * QlP * n,), 7, dtype=t.int64, device="cuda") for _ in range(2)]

    def mac(c=ctx, ch=chain, ins_=_vp(ins), T=2, tab=ptr(table), O_=2, outs_=_vp(accs)):
        return lib.phantom_ext_mac(c.handle, ch, ins_, T, tab, O_, outs_, 0, s)

    bad = [mac(ins_=None), mac(tab=None), mac(outs_=None), mac(T=0), mac(O_=0), mac(ch=0), mac(ch=last), mac(c=nop)]
    assert bad == [1] * len(bad), bad

    ns = PA.Conv.slots(width, slotstr)
    dslots = t.full((2 * ns,), 7.0, dtype=t.float64, device="cuda")

    def ws(w=width, st=slotstr, k=K, i=in_ch, o=out_ch, dw=W.data_ptr(), first=0, count=1, out=dslots.data_ptr()):
        return lib.phantom_conv_weight_slots(w, st, k, i, o, dw, first, count, out, s)

    bad = [ws(dw=None), ws(out=None), ws(k=2), ws(k=9), ws(w=6), ws(i=0), ws(o=0), ws(first=36, count=1),
           ws(first=30, count=7)]
    assert bad == [1] * len(bad), bad

    t.cuda.synchronize()
    for o in outs + accs:
        assert bool((o == 7).all())
    assert bool((dslots == 7.0).all())
    nop.close()
