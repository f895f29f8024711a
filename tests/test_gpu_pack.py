"""phantom_ct_pack and phantom_ct_split (channel packing by monomial shifts and one level of its
rotation tree) on the GPU, bit-exact against the CPU oracle in coefficient form:

  pack:   out = ntt_fwd(sum_c negacyclic_shift(ntt_inv(in_c), c D))
  split:  even_k = ntt_fwd(ntt_inv(a_k) + ntt_inv(r_k)),
          odd_k  = ntt_fwd(negacyclic_shift(ntt_inv(a_k) - ntt_inv(r_k), 2N - power))

on two chains: the mixed one of tests/test_gpu_degrees.py (primes below 2^50 beside 60-bit ones), and
the same with one data prime replaced by the prime just below 2^61, the modulus bound.  Each case
runs with uniform random limbs and with every word at q - 1.  pack: n = 2^10 with (C, D) = (4, 8);
n = 2^12 with (2, 1), (8, 4), (7, 4), (32, 1) (the pointer table: C > 16) and (1, 16).  split: count 1,
3 and 16 (the node table: count > 8), one null odd, even aliasing a.  Refused arguments return
status 1 and write nothing."""
import numpy as np
import pytest

import edge_cases as E
import oracle_lib as O
import phantom_amd as PA
from gpu_util import ptr, stream, to_dev, to_host, torch

pytestmark = pytest.mark.gpu

MIXED = [60] + [50] * 6 + [60] * 3
SIZE_P = 3
PACK_CASES = [(10, 4, 8), (12, 2, 1), (12, 8, 4), (12, 7, 4), (12, 32, 1), (12, 1, 16)]


def _chain(kind, n):
    mods = O.coeff_modulus_create(n, MIXED)
    assert min(mods) < 2**50 and max(mods) < 2**60
    if kind == "q61":
        mods[1] = E.prime_below(1 << 61, n)
        assert mods[1] > 2**60 and len(set(mods)) == len(mods)
    return mods


@pytest.fixture(scope="module")
def ctxs():
    made = {}

    def get(kind, log_n):
        if (kind, log_n) not in made:
            made[(kind, log_n)] = PA.Context(1 << log_n, _chain(kind, 1 << log_n), SIZE_P)
        return made[(kind, log_n)]

    yield get
    for c in made.values():
        c.close()


def _vp(ts):
    return PA.ptr_array([ptr(t) if t is not None else 0 for t in ts])


def _fill(rng, pat, ql, n):
    """[2][L][n] residues: uniform, or every word at q - 1"""
    if pat == "random":
        return np.concatenate([O.random_limbs(rng, n, ql) for _ in range(2)])
    return np.concatenate([E.edge_limbs(n, ql, "max")] * 2)


def _rows(x, ql, n):
    return x.reshape(2 * len(ql), n), np.array(ql + ql, dtype=np.uint64)[:, None]


def _shift(c, k, q, n):
    """rows of coefficients times X^k (negacyclic), k in [0, 2n)"""
    idx = (np.arange(n) + k) % (2 * n)
    out = np.zeros_like(c)
    out[:, idx % n] = np.where(idx >= n, (q - c) % q, c)
    return out


def _want_pack(ins, D, ql, n):
    acc = np.zeros((2 * len(ql), n), dtype=np.uint64)
    for c, x in enumerate(ins):
        co, q = _rows(O.ntt_inv(x, n, ql + ql), ql, n)
        acc = (acc + _shift(co, (c * D) % (2 * n), q, n)) % q  # both below q < 2^61: no wrap
    return O.ntt_fwd(acc.reshape(-1), n, ql + ql)


def _want_split(a, r, power, ql, n):
    ca, q = _rows(O.ntt_inv(a, n, ql + ql), ql, n)
    cr, _ = _rows(O.ntt_inv(r, n, ql + ql), ql, n)
    even = (ca + cr) % q
    odd = _shift((ca + q - cr) % q, (2 * n - power) % (2 * n), q, n)
    return O.ntt_fwd(even.reshape(-1), n, ql + ql), O.ntt_fwd(odd.reshape(-1), n, ql + ql)


@pytest.mark.parametrize("pat", ["random", "max"])
@pytest.mark.parametrize("kind,chain", [("mixed", 1), ("q61", 1), ("q61", 3)])
@pytest.mark.parametrize("log_n,C,D", PACK_CASES)
def test_ct_pack(ctxs, rng, log_n, C, D, kind, chain, pat):
    ctx, n = ctxs(kind, log_n), 1 << log_n
    ql = ctx.ql(chain)
    base = [_fill(rng, pat, ql, n) for _ in range(min(C, 5))]  # repeated operands share a device copy
    dev = [to_dev(x) for x in base]
    ins, din = [base[(3 * c + 1) % len(base)] for c in range(C)], [dev[(3 * c + 1) % len(base)] for c in range(C)]
    out = to_dev(np.full(2 * len(ql) * n, 7, dtype=np.uint64))
    PA.check(PA.load().phantom_ct_pack(ctx.handle, chain, _vp(din), C, D, ptr(out), stream()))
    want = _want_pack(ins, D, ql, n)
    assert want.any() and np.array_equal(to_host(out), want)


@pytest.mark.parametrize("pat", ["random", "max"])
@pytest.mark.parametrize("kind,chain", [("mixed", 1), ("q61", 2)])
@pytest.mark.parametrize("count", [1, 3, 16])
def test_ct_split(ctxs, rng, count, kind, chain, pat):
    """node 0's even output aliases its a; the last node's odd output is null"""
    log_n, power = 12, 24
    ctx, n = ctxs(kind, log_n), 1 << log_n
    ql = ctx.ql(chain)
    words = 2 * len(ql) * n
    base = [_fill(rng, "random" if pat == "random" else ("max" if i == 0 else "random"), ql, n) for i in range(4)]
    a = [base[(2 * k) % 4] for k in range(count)]
    r = [base[(2 * k + 1 + (k & 1)) % 4] for k in range(count)]
    if pat == "max":  # a - r = 0 and a + r = 2 (q - 1) at node 0; (q - 1) - x elsewhere
        r[0] = a[0]
    da, dr = [to_dev(x) for x in a], [to_dev(x) for x in r]
    even = [da[0]] + [to_dev(np.full(words, 7, dtype=np.uint64)) for _ in range(count - 1)]
    odd = [to_dev(np.full(words, 7, dtype=np.uint64)) for _ in range(count - 1)] + [None]
    if count == 1:
        odd = [to_dev(np.full(words, 7, dtype=np.uint64))]
    PA.check(PA.load().phantom_ct_split(ctx.handle, chain, _vp(da), _vp(dr), count, power, _vp(even), _vp(odd), stream()))
    for k in range(count):
        want_even, want_odd = _want_split(a[k], r[k], power, ql, n)
        assert np.array_equal(to_host(even[k]), want_even), k
        if odd[k] is not None:
            assert (want_odd.any() or pat == "max") and np.array_equal(to_host(odd[k]), want_odd), k
    # the inputs other than the aliased one are intact
    for k in range(1, count):
        assert np.array_equal(to_host(da[k]), a[k]) and np.array_equal(to_host(dr[k]), r[k])


def test_split_arrays_may_be_null(ctxs, rng):
    """even or odd as a whole may be absent; power 0 multiplies by X^0"""
    ctx, n, chain = ctxs("mixed", 12), 1 << 12, 1
    ql = ctx.ql(chain)
    a, r = _fill(rng, "random", ql, n), _fill(rng, "random", ql, n)
    da, dr = to_dev(a), to_dev(r)
    o = to_dev(np.zeros(2 * len(ql) * n, dtype=np.uint64))
    lib, s = PA.load(), stream()
    want_even, want_odd = _want_split(a, r, 0, ql, n)
    PA.check(lib.phantom_ct_split(ctx.handle, chain, _vp([da]), _vp([dr]), 1, 0, None, _vp([o]), s))
    assert np.array_equal(to_host(o), want_odd)
    PA.check(lib.phantom_ct_split(ctx.handle, chain, _vp([da]), _vp([dr]), 1, 0, _vp([o]), None, s))
    assert np.array_equal(to_host(o), want_even)


def test_refused_arguments(ctxs, rng):
    """every bad argument returns PHANTOM_ERR_INVALID_ARGUMENT (1) before any launch"""
    ctx, n, chain = ctxs("mixed", 12), 1 << 12, 1
    ql = ctx.ql(chain)
    words = 2 * len(ql) * n
    lib, s, tt = PA.load(), stream(), torch()
    ins = [to_dev(_fill(rng, "random", ql, n)) for _ in range(3)]
    keep = [to_host(x) for x in ins]
    outs = [tt.full((words + 2,), 7, dtype=tt.int64, device="cuda") for _ in range(3)]
    o = [x[:words] for x in outs]
    holes = PA.ptr_array([ptr(ins[0]), 0, ptr(ins[2])])
    many = PA.ptr_array([ptr(ins[0])] * 65)
    last = ctx.size_Q + 1

    def pack(c=ctx.handle, ch=chain, i=_vp(ins), C=3, D=4, out=ptr(o[0])):
        return lib.phantom_ct_pack(c, ch, i, C, D, out, s)

    bad = [pack(c=None), pack(i=None), pack(out=None), pack(C=0), pack(i=many, C=65), pack(D=2 * n), pack(ch=0),
           pack(ch=last), pack(i=holes), pack(out=ptr(ins[1])), pack(out=ptr(ins[2]) + 8 * n), pack(out=ptr(outs[0]) + 8)]
    assert bad == [1] * len(bad), bad

    def split(c=ctx.handle, ch=chain, a=_vp(ins[:2]), r=_vp([ins[2], ins[2]]), cnt=2, pw=4, ev=_vp(o[:2]), od=_vp([o[2], None])):
        return lib.phantom_ct_split(c, ch, a, r, cnt, pw, ev, od, s)

    bad = [split(c=None), split(a=None), split(r=None), split(ev=None, od=None), split(cnt=0), split(a=many, r=many, cnt=65),
           split(pw=2 * n), split(ch=0), split(ch=last), split(a=holes), split(r=holes),
           split(ev=_vp([ins[1], o[1]])),           # even[0] aliases a[1], not its own a
           split(ev=_vp([ins[2], o[1]])),           # an output on r
           split(od=_vp([ins[0], None])),           # odd aliases a
           split(ev=_vp([o[0], o[0]])),             # two outputs on one buffer
           split(od=_vp([o[0], None]))]             # odd[0] on even[0]
    assert bad == [1] * len(bad), bad
    assert split(ev=_vp(ins[:2]), od=None) == 0  # even[k] == a[k] is the allowed alias
    tt.cuda.synchronize()
    for x in outs:
        assert bool((x == 7).all())
    assert np.array_equal(to_host(ins[2]), keep[2])
