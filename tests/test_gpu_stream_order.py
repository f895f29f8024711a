"""Every stream-taking C-ABI entry of include/phantom_amd.h on a held side stream.

The protocol is tests/stream_harness.py's: the entry is called on a fresh torch stream whose queue
is held back by a device-side delay while the buffers it reads hold a decoy; the real inputs are
copied in behind the delay, on that stream.  Work issued on any other stream reads the decoy (or
scratch nobody has written) and gives other bytes than a quiet run on the current stream, which
the per-entry test modules pin to the oracle.  An entry documented as not synchronising must return
while the stream is still held; the entries whose header text allows a wait (`blocks`) are only
required to start while it is held.  The check of work left running after the call returns, and
the two-stream test, are opportunistic: NOT deterministic.  Controls A and B show that the harness
can fail and can pass; test_header_entries_are_covered (CPU) keeps the table complete.

Shapes: N = 2^12 on the mixed chain of tests/test_gpu_ckks.py (`small`: FP64 and integer limbs, three
special primes), N = 2^10 for the 1-D NTT, the N = 2^12 rings of the encoder / encryption / DNN
modules.

Delay (stream_harness.Delay): torch.cuda._sleep, calibrated once per module with events; measured
on an MI355X at 2.39 million cycles per millisecond (asked 20 ms, events measured 19.97 ms).  A warm
gated run holds the stream for max(20 ms, 8 x the call's host time on an idle stream), at most
250 ms; the cold run for 60 ms.  Warm host times measured for the entries that must not block:
0.008 ms (multiply) to 0.38 ms (conv2d), 0.004 to 0.13 ms while the stream is held, so every warm run
uses the 20 ms floor, 50 x the slowest call; the entries that may block return after the 20 ms.

Side streams: HIP deals streams round robin onto 4 hardware queues, the null stream's among them; a
side stream on the null stream's queue would hide work issued on stream 0, so the harness passes
such a stream over (stream_harness.fresh_stream).
"""
import ctypes
import os
import re

import numpy as np
import pytest

import ks_oracle as KO
import oracle_lib as O
import phantom_amd as PA
import stream_harness as H
from gpu_util import ptr, torch
from test_gpu_ckks import SMALL_BITS

N = 1 << 12
CASES = {}      # name -> (builder, entries covered, blocks)
VPP = ctypes.POINTER(ctypes.c_void_p)

# entries of the header that take a stream and have no case, each with its reason
EXEMPT = {
    "phantom_bconv_create": "builds host tables and waits for the stream before returning (documented); its tables are "
                            "exercised by the bconv_run case, which creates its converter with it",
}


def case(name, entries, blocks=False):
    def deco(f):
        assert name not in CASES
        CASES[name] = (f, tuple(entries), blocks)
        return f
    return deco


def build(env, name):
    f, _, blocks = CASES[name]
    c = H.Case(name, blocks)
    f(env, c)
    assert c.call is not None
    return c


# ---- helpers ---------------------------------------------------------------------------------------

def ck(status):
    PA.check(status)


def vp(ts):
    return PA.ptr_array([ptr(t) if t is not None else 0 for t in ts])


def rl(rng, n, mods, polys=1):
    return np.concatenate([O.random_limbs(rng, n, mods) for _ in range(polys)])


def residues(rng, mods, *shape):
    out = np.zeros(shape + (len(mods),), dtype=np.uint64)
    for l, q in enumerate(mods):
        out[..., l] = rng.integers(0, q, size=shape, dtype=np.uint64)
    return np.ascontiguousarray(out)


def scales(rng, mods):
    sc = [int(rng.integers(1, q)) for q in mods]
    return O.arr(sc), O.arr([(s << 64) // q for s, q in zip(sc, mods)])


def key_table(arrays):
    """host array of host arrays of device pointers (entries may be None)"""
    return (VPP * len(arrays))(*[ctypes.cast(a, VPP) if a is not None else None for a in arrays])


def on_stream(s):
    """torch's stream context for a raw stream handle"""
    t = torch()
    return t.cuda.stream(t.cuda.ExternalStream(s) if s else t.cuda.default_stream())


class Env:
    def __init__(self, rng):
        self.rng = rng
        self.lib = PA.load()
        self._made = {}

    def get(self, key, make):
        if key not in self._made:
            self._made[key] = make()
        return self._made[key]

    def small_mods(self):
        return self.get("small_mods", lambda: O.coeff_modulus_create(N, SMALL_BITS))

    def small(self):
        return self.get("small", lambda: PA.Context(N, self.small_mods(), 3))

    def fresh_small(self, c):
        """a second context with the same parameters: its lazily built tables do not exist yet"""
        def make():
            ctx = PA.Context(N, self.small_mods(), 3)
            c.cleanup.append(ctx.close)
            return ctx
        return make

    def tables(self):
        return self.get("tables", lambda: PA.NttTables(N, self.small_mods()))

    def conv_ctx(self):
        return self.get("conv", lambda: PA.Context(N, PA.coeff_modulus_create(N, [60, 50, 50, 50, 60, 60]), 2))

    def keys(self, c, ctx, sets=1):
        """`sets` key-switching keys of uniform digits on the device (not gated): [(host, dev, vp)]"""
        dnum = -(-ctx.size_Q // ctx.size_P)
        out = []
        for _ in range(sets):
            host = [rl(self.rng, ctx.n, ctx.moduli, 2) for _ in range(dnum)]
            dev = [c.const(k) for k in host]
            out.append((host, dev, c.hold(vp(dev))))
        return out, dnum


def ext_mods(ctx, chain):
    return ctx.ql(chain) + ctx.moduli[ctx.size_Q:]


def beta_of(ctx, chain):
    return -(-len(ctx.ql(chain)) // ctx.size_P)


# ---- controls ----------------------------------------------------------------------------------------

def _control(env, c, wrong_stream):
    t = torch()
    x = c.inp(env.rng.integers(0, 1 << 60, size=1 << 16, dtype=np.uint64), 1 << 16)
    y = c.out(1 << 16)

    def call(s, ctx):
        if wrong_stream:
            with t.cuda.stream(t.cuda.default_stream()):
                y.copy_(x, non_blocking=True)
        else:
            with on_stream(s):
                y.copy_(x, non_blocking=True)
    c.call = call


# ---- NTT (capi.cpp) -------------------------------------------------------------------------------------

def _ntt_case(env, c, L, fn, want, inplace=True):
    mods = env.small_mods()[:L]
    a = rl(env.rng, N, mods)
    x = c.inp(a, N, inout=inplace)
    t = env.tables()
    c.call = lambda s, ctx: ck(fn(x, t.handle, s))
    c.oracle = lambda: [(0, want(a, mods))]
    return x, a, mods


@case("nwt_forward_inplace", ["phantom_nwt_forward_inplace"])
def _(env, c):
    _ntt_case(env, c, 5, lambda x, t, s: env.lib.phantom_nwt_forward_inplace(ptr(x), t, 5, 0, s),
              lambda a, m: O.ntt_fwd(a, N, m))


@case("nwt_backward_inplace", ["phantom_nwt_backward_inplace"])
def _(env, c):
    _ntt_case(env, c, 5, lambda x, t, s: env.lib.phantom_nwt_backward_inplace(ptr(x), t, 5, 0, s),
              lambda a, m: O.ntt_inv(a, N, m))


@case("nwt_backward", ["phantom_nwt_backward"])
def _(env, c):
    out = c.out(4 * N)
    _ntt_case(env, c, 4, lambda x, t, s: env.lib.phantom_nwt_backward(ptr(out), ptr(x), t, 4, 0, s),
              lambda a, m: O.ntt_inv(a, N, m), inplace=False)


def _scaled_inv(a, mods, sc):
    want = O.ntt_inv(a, N, mods)
    for l, q in enumerate(mods):
        want[l * N:(l + 1) * N] = (want[l * N:(l + 1) * N].astype(object) * int(sc[l]) % q).astype(np.uint64)
    return want


def _gated_scales(env, c, mods):
    sets = [scales(env.rng, mods) for _ in range(3)]
    sc = c.inp(sets[0][0], len(mods), decoys=(sets[1][0], sets[2][0]))
    sh = c.inp(sets[0][1], len(mods), decoys=(sets[1][1], sets[2][1]))
    return sc, sh, sets[0][0]


@case("nwt_backward_scale", ["phantom_nwt_backward_scale"])
def _(env, c):
    L = 3
    out = c.out(L * N)
    sc, sh, host = _gated_scales(env, c, env.small_mods()[:L])
    _ntt_case(env, c, L, lambda x, t, s: env.lib.phantom_nwt_backward_scale(ptr(out), ptr(x), t, L, 0, ptr(sc), ptr(sh), s),
              lambda a, m: _scaled_inv(a, m, host), inplace=False)


@case("nwt_backward_inplace_scale", ["phantom_nwt_backward_inplace_scale"])
def _(env, c):
    L = 3
    sc, sh, host = _gated_scales(env, c, env.small_mods()[:L])
    _ntt_case(env, c, L, lambda x, t, s: env.lib.phantom_nwt_backward_inplace_scale(ptr(x), t, L, 0, ptr(sc), ptr(sh), s),
              lambda a, m: _scaled_inv(a, m, host))


def _special_case(env, c, size_Ql, fn, want_limb):
    """a QlP buffer: size_Ql data limbs, then the three special primes"""
    mods = env.small_mods()
    qlp = mods[:size_Ql] + mods[7:]
    a = rl(env.rng, N, qlp)
    x = c.inp(a, N, inout=True)
    t = env.tables()
    c.call = lambda s, ctx: ck(fn(x, t.handle, s))

    def oracle():
        want = a.copy()
        for i, q in enumerate(qlp):
            want[i * N:(i + 1) * N] = want_limb(i, a[i * N:(i + 1) * N], q)
        return [(0, want)]
    c.oracle = oracle


@case("nwt_forward_include_special_mod", ["phantom_nwt_forward_include_special_mod"])
def _(env, c):
    _special_case(env, c, 4, lambda x, t, s: env.lib.phantom_nwt_forward_include_special_mod(ptr(x), t, 7, 0, 10, 3, s),
                  lambda i, v, q: O.ntt_fwd(v, N, [q]))


@case("nwt_forward_include_special_mod_exclude_range", ["phantom_nwt_forward_include_special_mod_exclude_range"])
def _(env, c):
    _special_case(env, c, 4,
                  lambda x, t, s: env.lib.phantom_nwt_forward_include_special_mod_exclude_range(ptr(x), t, 7, 0, 10, 3, 1,
                                                                                                3, s),
                  lambda i, v, q: v if 1 <= i < 3 else O.ntt_fwd(v, N, [q]))


@case("nwt_backward_inplace_include_special_mod", ["phantom_nwt_backward_inplace_include_special_mod"])
def _(env, c):
    _special_case(env, c, 4,
                  lambda x, t, s: env.lib.phantom_nwt_backward_inplace_include_special_mod(ptr(x), t, 3, 4, 10, 3, s),
                  lambda i, v, q: v if i < 4 else O.ntt_inv(v, N, [q]))


@case("nwt_forward_fuse_moddown", ["phantom_nwt_forward_fuse_moddown"])
def _(env, c):
    L = 4
    mods = env.small_mods()[:L]
    cx, delta = rl(env.rng, N, mods), rl(env.rng, N, mods)
    out = c.out(L * N)
    dcx, ddl = c.inp(cx, N), c.inp(delta, N)
    sc, sh, host = _gated_scales(env, c, mods)
    t = env.tables()
    c.call = lambda s, ctx: ck(env.lib.phantom_nwt_forward_fuse_moddown(ptr(out), ptr(dcx), ptr(sc), ptr(sh), ptr(ddl),
                                                                        t.handle, L, 0, s))

    def oracle():
        nd = O.ntt_fwd(delta, N, mods)
        want = np.zeros_like(cx)
        for l, q in enumerate(mods):
            sl = slice(l * N, (l + 1) * N)
            want[sl] = ((cx[sl].astype(object) - nd[sl].astype(object)) % q * int(host[l]) % q).astype(np.uint64)
        return [(0, want)]
    c.oracle = oracle


def _ntt_1d(env, c, forward):
    n, L = 1 << 10, 3
    mods = env.get("mods_1d", lambda: O.coeff_modulus_create(n, [50] * L))
    t = env.get("tables_1d", lambda: PA.NttTables(n, mods))
    a = rl(env.rng, n, mods)
    x = c.inp(a, n, inout=True)
    if forward:
        c.call = lambda s, ctx: ck(env.lib.phantom_fnwt_1d(ptr(x), t.handle, L, 0, s))
        c.oracle = lambda: [(0, O.ntt_fwd(a, n, mods))]
    else:
        sets = [scales(env.rng, mods) for _ in range(3)]
        sc = c.inp(sets[0][0], L, decoys=(sets[1][0], sets[2][0]))
        sh = c.inp(sets[0][1], L, decoys=(sets[1][1], sets[2][1]))
        c.call = lambda s, ctx: ck(env.lib.phantom_inwt_1d(ptr(x), t.handle, L, 0, ptr(sc), ptr(sh), s))

        def oracle():
            want = O.ntt_inv(a, n, mods)
            for l, q in enumerate(mods):
                want[l * n:(l + 1) * n] = (want[l * n:(l + 1) * n].astype(object) * int(sets[0][0][l]) % q).astype(np.uint64)
            return [(0, want)]
        c.oracle = oracle


@case("fnwt_1d", ["phantom_fnwt_1d"])
def _(env, c):
    _ntt_1d(env, c, True)


@case("inwt_1d", ["phantom_inwt_1d"])
def _(env, c):
    _ntt_1d(env, c, False)


# ---- CKKS (capi_ckks.cpp) -------------------------------------------------------------------------------

@case("multiply", ["phantom_multiply"])
def _(env, c):
    ctx, chain = env.small(), 2
    ql = ctx.ql(chain)
    a, b = rl(env.rng, N, ql, 2), rl(env.rng, N, ql, 2)
    da, db, out = c.inp(a, N), c.inp(b, N), c.out(3 * len(ql) * N)
    c.call = lambda s, x: ck(env.lib.phantom_multiply(ctx.handle, chain, ptr(da), ptr(db), ptr(out), s))

    def oracle():
        want = np.zeros(3 * len(ql) * N, dtype=np.uint64)
        O.lib().or_tensor_prod_2x2(O.P(a), O.P(b), O.P(want), N, len(ql), O.P(O.arr(ql)))
        return [(0, want)]
    c.oracle = oracle


@case("square", ["phantom_square"])
def _(env, c):
    ctx, chain = env.small(), 3
    ql = ctx.ql(chain)
    a = rl(env.rng, N, ql, 2)
    da, out = c.inp(a, N), c.out(3 * len(ql) * N)
    c.call = lambda s, x: ck(env.lib.phantom_square(ctx.handle, chain, ptr(da), ptr(out), s))

    def oracle():
        want = np.zeros(3 * len(ql) * N, dtype=np.uint64)
        O.lib().or_tensor_square_2x2(O.P(a), O.P(want), N, len(ql), O.P(O.arr(ql)))
        return [(0, want)]
    c.oracle = oracle


@case("modup", ["phantom_modup"])
def _(env, c):
    ctx, chain = env.small(), 2
    ql, p = ctx.ql(chain), ctx.moduli[ctx.size_Q:]
    words = beta_of(ctx, chain) * (len(ql) + len(p)) * N
    c2 = rl(env.rng, N, ql)
    d, out = c.inp(c2, N), c.out(words)
    c.call = lambda s, x: ck(env.lib.phantom_modup(ctx.handle, chain, ptr(d), ptr(out), s))

    def oracle():
        want = np.zeros(words, dtype=np.uint64)
        O.lib().or_modup(O.P(c2), O.P(want), N, O.P(O.arr(ql)), len(ql), O.P(O.arr(p)), len(p))
        return [(0, want)]
    c.oracle = oracle


@case("keyswitch_inner_prod", ["phantom_keyswitch_inner_prod"])
def _(env, c):
    ctx, chain = env.small(), 3
    ql = ctx.ql(chain)
    qlp, beta = ext_mods(ctx, chain), beta_of(ctx, chain)
    tmu = rl(env.rng, N, qlp, beta)
    ((keys, dkeys, kp),), dnum = env.keys(c, ctx)
    d, out = c.inp(tmu, N), c.out(2 * len(qlp) * N)
    c.call = lambda s, x: ck(env.lib.phantom_keyswitch_inner_prod(ctx.handle, chain, ptr(d), kp, dnum, ptr(out), s))

    def oracle():
        want = np.zeros(2 * len(qlp) * N, dtype=np.uint64)
        O.lib().or_keyswitch_inner_prod(O.P(tmu), O.ptrs(keys), O.P(want), N, len(ql), ctx.size_Q, ctx.size_P, beta,
                                        O.P(O.arr(ctx.moduli)))
        return [(0, want)]
    c.oracle = oracle


@case("keyswitch", ["phantom_keyswitch"])
def _(env, c):
    ctx, chain = env.small(), 1
    ql = ctx.ql(chain)
    ct, c2 = rl(env.rng, N, ql, 2), rl(env.rng, N, ql)
    ((keys, dkeys, kp),), dnum = env.keys(c, ctx)
    dct, dc2 = c.inp(ct, N, inout=True), c.inp(c2, N)
    c.call = lambda s, x: ck(env.lib.phantom_keyswitch(ctx.handle, chain, ptr(dct), ptr(dc2), kp, dnum, s))

    def oracle():
        want = ct.copy()
        O.lib().or_keyswitch_add(O.P(want), O.P(c2), O.ptrs(keys), N, len(ql), ctx.size_Q, ctx.size_P,
                                 O.P(O.arr(ctx.moduli)))
        return [(0, want)]
    c.oracle = oracle


@case("relinearize", ["phantom_relinearize"])
def _(env, c):
    ctx, chain = env.small(), 4
    ql = ctx.ql(chain)
    ct = rl(env.rng, N, ql, 3)
    ((keys, dkeys, kp),), dnum = env.keys(c, ctx)
    d = c.inp(ct, N, inout=True)
    c.call = lambda s, x: ck(env.lib.phantom_relinearize(ctx.handle, chain, ptr(d), kp, dnum, s))

    def oracle():
        want = ct.copy()
        O.lib().or_relinearize(O.P(want), N, len(ql), ctx.size_Q, ctx.size_P, O.ptrs(keys), O.P(O.arr(ctx.moduli)))
        return [(0, want[:2 * len(ql) * N])]
    c.oracle = oracle


@case("relinearize_rescale", ["phantom_relinearize_rescale"])
def _(env, c):
    ctx, chain = env.small(), 1
    L = len(ctx.ql(chain))
    ct = rl(env.rng, N, ctx.ql(chain), 3)
    ((keys, dkeys, kp),), dnum = env.keys(c, ctx)
    d, out = c.inp(ct, N), c.out(2 * (L - 1) * N)
    c.call = lambda s, x: ck(env.lib.phantom_relinearize_rescale(ctx.handle, chain, ptr(d), ptr(out), kp, dnum, s))
    c.oracle = lambda: [(0, KO.relinearize_rescale(ctx, chain, ct, keys))]


@case("relinearize_rescale_batch", ["phantom_relinearize_rescale_batch"])
def _(env, c):
    ctx, chain, count = env.small(), 5, 3
    L = len(ctx.ql(chain))
    cts = [rl(env.rng, N, ctx.ql(chain), 3) for _ in range(count)]
    s_in, s_out = 3 * L * N + 2 * N, 2 * (L - 1) * N + 2 * N
    buf = np.ones(count * s_in, dtype=np.uint64)
    for k, ct in enumerate(cts):
        buf[k * s_in:k * s_in + ct.size] = ct
    ((keys, dkeys, kp),), dnum = env.keys(c, ctx)
    d, out = c.inp(buf, N), c.out(count * s_out)
    c.call = lambda s, x: ck(env.lib.phantom_relinearize_rescale_batch(ctx.handle, chain, ptr(d), s_in, count, ptr(out),
                                                                       s_out, kp, dnum, s))

    def oracle():
        want = np.full(count * s_out, H.SENTINEL, dtype=np.uint64)
        for k in range(count):
            want[k * s_out:k * s_out + 2 * (L - 1) * N] = KO.relinearize_rescale(ctx, chain, buf[k * s_in:k * s_in + 3 * L * N].copy(), keys)
        return [(0, want)]
    c.oracle = oracle


def _moddown(env, c, unbiased):
    chain = 5
    if unbiased:
        def make():
            ctx = PA.Context(N, env.small_mods(), 3)
            ctx.set_unbiased_moddown(True)
            return ctx
        ctx = env.get("small_unbiased", make)
    else:
        ctx = env.small()
    ql, p = ctx.ql(chain), ctx.moduli[ctx.size_Q:]
    cx = rl(env.rng, N, ql + p)
    d, out = c.inp(cx, N), c.out(len(ql) * N)
    c.call = lambda s, x: ck(env.lib.phantom_moddown_from_ntt(ctx.handle, chain, ptr(d), ptr(out), s))
    if not unbiased:
        def oracle():
            want = np.zeros(len(ql) * N, dtype=np.uint64)
            O.lib().or_moddown_from_ntt(O.P(cx.copy()), O.P(want), N, O.P(O.arr(ql)), len(ql), O.P(O.arr(p)), len(p))
            return [(0, want)]
        c.oracle = oracle


@case("moddown_from_ntt", ["phantom_moddown_from_ntt"])
def _(env, c):
    _moddown(env, c, False)


@case("moddown_from_ntt[unbiased]", ["phantom_moddown_from_ntt"])
def _(env, c):
    _moddown(env, c, True)


def _down_up(ctx, chain, cx):
    ql, p = ctx.ql(chain), ctx.moduli[ctx.size_Q:]
    down = np.zeros(len(ql) * N, dtype=np.uint64)
    O.lib().or_moddown_from_ntt(O.P(cx.copy()), O.P(down), N, O.P(O.arr(ql)), len(ql), O.P(O.arr(p)), len(p))
    want = np.zeros(beta_of(ctx, chain) * (len(ql) + len(p)) * N, dtype=np.uint64)
    O.lib().or_modup(O.P(down), O.P(want), N, O.P(O.arr(ql)), len(ql), O.P(O.arr(p)), len(p))
    return want


@case("moddown_modup", ["phantom_moddown_modup"])
def _(env, c):
    ctx, chain = env.small(), 2
    qlp = ext_mods(ctx, chain)
    cx = rl(env.rng, N, qlp)
    d, out = c.inp(cx, N), c.out(beta_of(ctx, chain) * len(qlp) * N)
    c.call = lambda s, x: ck(env.lib.phantom_moddown_modup(ctx.handle, chain, ptr(d), ptr(out), s))
    c.oracle = lambda: [(0, _down_up(ctx, chain, cx))]


@case("moddown_modup_batch", ["phantom_moddown_modup_batch"])
def _(env, c):
    ctx, chain, count = env.small(), 2, 3
    qlp = ext_mods(ctx, chain)
    stride = (len(qlp) + 1) * N
    cxs = [rl(env.rng, N, qlp) for _ in range(count)]
    buf = np.ones(count * stride, dtype=np.uint64)
    for i, cx in enumerate(cxs):
        buf[i * stride:i * stride + cx.size] = cx
    d, out = c.inp(buf, N), c.out(count * beta_of(ctx, chain) * len(qlp) * N)
    c.call = lambda s, x: ck(env.lib.phantom_moddown_modup_batch(ctx.handle, chain, ptr(d), count, stride, ptr(out), s))
    c.oracle = lambda: [(0, np.concatenate([_down_up(ctx, chain, cx) for cx in cxs]))]


@case("moddown_rescale", ["phantom_moddown_rescale"])
def _(env, c):
    ctx, chain, polys = env.small(), 1, 2
    ql, p = ctx.ql(chain), ctx.moduli[ctx.size_Q:]
    cxs = [rl(env.rng, N, ql + p) for _ in range(polys)]
    d, out = c.inp(np.concatenate(cxs), N), c.out(polys * (len(ql) - 1) * N)
    c.call = lambda s, x: ck(env.lib.phantom_moddown_rescale(ctx.handle, chain, ptr(d), ptr(out), polys, s))

    def oracle():
        want = []
        for cx in cxs:
            w = np.zeros((len(ql) - 1) * N, dtype=np.uint64)
            O.lib().or_moddown_from_ntt(O.P(cx.copy()), O.P(w), N, O.P(O.arr(ql[:-1])), len(ql) - 1,
                                        O.P(O.arr([ql[-1]] + list(p))), len(p) + 1)
            want.append(w)
        return [(0, np.concatenate(want))]
    c.oracle = oracle


@case("rescale_to_next", ["phantom_rescale_to_next"])
def _(env, c):
    ctx, chain = env.small(), 3
    ql = ctx.ql(chain)
    L = len(ql)
    ct = rl(env.rng, N, ql, 2)
    d, out = c.inp(ct, N), c.out(2 * (L - 1) * N)
    c.call = lambda s, x: ck(env.lib.phantom_rescale_to_next(ctx.handle, chain, ptr(d), ptr(out), 2, s))

    def oracle():
        want = np.zeros(2 * (L - 1) * N, dtype=np.uint64)
        O.lib().or_rescale_ntt(O.P(ct), O.P(want), N, L, 2, O.P(O.arr(ql)))
        return [(0, want)]
    c.oracle = oracle


@case("apply_galois_ntt", ["phantom_apply_galois_ntt"])
def _(env, c):
    """the permutation of this element is built on the side stream's first call (a fresh context)"""
    quiet_ctx, L, elt = env.small(), 4, pow(5, 11, 2 * N)
    a = rl(env.rng, N, quiet_ctx.moduli[:L])
    d, out = c.inp(a, N), c.out(L * N)
    c.make_ctx = env.fresh_small(c)
    c.call = lambda s, x: ck(env.lib.phantom_apply_galois_ntt((x or quiet_ctx).handle, elt, ptr(d), ptr(out), L, s))

    def oracle():
        want = np.zeros_like(a)
        O.lib().or_apply_galois_ntt(O.P(a), O.P(want), N, L, elt)
        return [(0, want)]
    c.oracle = oracle


def _poly_op(op):
    def f(env, c):
        ctx, off, L = env.small(), 2, 5
        mods = ctx.moduli[off:off + L]
        a, b = rl(env.rng, N, mods), rl(env.rng, N, mods)
        da, db, out = c.inp(a, N), c.inp(b, N), c.out(L * N)
        c.call = lambda s, x: ck(env.lib.phantom_poly_op(ctx.handle, op, ptr(da), ptr(db), ptr(out), off, L, s))

        def oracle():
            want, m = np.zeros_like(a), O.arr(mods)
            if op < 3:
                [O.lib().or_poly_add, O.lib().or_poly_sub, O.lib().or_poly_mul][op](O.P(a), O.P(b), O.P(want), N, L, O.P(m))
            else:
                O.lib().or_poly_negate(O.P(a), O.P(want), N, L, O.P(m))
            return [(0, want)]
        c.oracle = oracle
    return f


for _op, _name in enumerate(["add", "sub", "mul", "negate"]):
    case(f"poly_op[{_name}]", ["phantom_poly_op"])(_poly_op(_op))


@case("switch_modulus_raise", ["phantom_switch_modulus_raise"])
def _(env, c):
    ctx = env.small()
    L, q0 = ctx.size_Q, ctx.moduli[0]
    v = rl(env.rng, N, [q0])
    d, out = c.inp(v, N), c.out(L * N)
    c.call = lambda s, x: ck(env.lib.phantom_switch_modulus_raise(ctx.handle, ptr(d), ptr(out), L, s))

    def oracle():
        want = np.zeros(L * N, dtype=np.uint64)
        O.lib().or_switch_modulus_raise(O.P(v), O.P(want), N, q0, O.P(O.arr(ctx.moduli)), L)
        return [(0, want)]
    c.oracle = oracle


def _bconv(env, c, kept):
    mods = env.small_mods()
    ib, ob = np.array(mods[:3], dtype=np.uint64), np.array(mods[3:], dtype=np.uint64)
    x = rl(env.rng, N, mods[:3])
    d, out = c.inp(x, N), c.out(len(ob) * N)
    if kept:
        h = PA.vp()
        ck(env.lib.phantom_bconv_create(ib.ctypes.data_as(PA.u64p), 3, ob.ctypes.data_as(PA.u64p), len(ob),
                                        torch().cuda.current_stream().cuda_stream, ctypes.byref(h)))
        c.cleanup.append(lambda: env.lib.phantom_bconv_destroy(h))
        c.call = lambda s, _: ck(env.lib.phantom_bconv_run(h, ptr(d), ptr(out), N, 1, s))
    else:
        c.call = lambda s, _: ck(env.lib.phantom_fast_bconv(ib.ctypes.data_as(PA.u64p), 3, ob.ctypes.data_as(PA.u64p),
                                                            len(ob), ptr(d), ptr(out), N, 1, s))

    def oracle():
        want = np.zeros(len(ob) * N, dtype=np.uint64)
        O.lib().or_bconv(O.P(x), O.P(want), N, O.P(ib), 3, O.P(ob), len(ob))
        return [(0, want)]
    c.oracle = oracle


@case("bconv_run", ["phantom_bconv_run"])
def _(env, c):
    _bconv(env, c, True)


@case("fast_bconv", ["phantom_fast_bconv"], blocks=True)
def _(env, c):
    _bconv(env, c, False)


# ---- the bootstrap's kernels (capi_bootk.cpp) --------------------------------------------------------

@case("keyswitch_ext", ["phantom_keyswitch_ext"])
def _(env, c):
    ctx, chain = env.small(), 2
    ct = rl(env.rng, N, ctx.ql(chain), 2)
    d, out = c.inp(ct, N), c.out(2 * len(ext_mods(ctx, chain)) * N)
    c.call = lambda s, x: ck(env.lib.phantom_keyswitch_ext(ctx.handle, chain, ptr(d), ptr(out), s))


@case("fast_rotation_ext", ["phantom_fast_rotation_ext"])
def _(env, c):
    ctx, chain = env.small(), 1
    em = ext_mods(ctx, chain)
    c0, digits = rl(env.rng, N, ctx.ql(chain)), rl(env.rng, N, em, beta_of(ctx, chain))
    ((_, _, kp),), dnum = env.keys(c, ctx)
    d0, dd, out = c.inp(c0, N), c.inp(digits, N), c.out(2 * len(em) * N)
    elt = pow(5, 77, 2 * N)
    c.call = lambda s, x: ck(env.lib.phantom_fast_rotation_ext(ctx.handle, chain, ptr(d0), ptr(dd), kp, dnum, elt, 1,
                                                               ptr(out), s))


def _rotation_batch(env, c, group):
    """count 3 with the identity at entry 1; group 0 = the one-ciphertext entry"""
    ctx, chain, count = env.small(), 3, 3
    em = ext_mods(ctx, chain)
    W = 2 * len(em) * N
    G = max(group, 1)
    cts = [c.inp(rl(env.rng, N, ctx.ql(chain), 2), N) for _ in range(G)]
    digs = [c.inp(rl(env.rng, N, em, beta_of(ctx, chain)), N) for _ in range(G)]
    keysets, dnum = env.keys(c, ctx, 2)
    kk = c.hold(key_table([keysets[0][2], None, keysets[1][2]]))
    el = (ctypes.c_uint32 * count)(pow(5, 4, 2 * N), 1, 2 * N - 1)
    outs = [c.out(count * W) for _ in range(G)]
    po = c.hold(PA.ptr_array([ptr(o) + 8 * k * W for o in outs for k in range(count)]))
    if group:
        pc, pd = c.hold(vp(cts)), c.hold(vp(digs))
        c.call = lambda s, x: ck(env.lib.phantom_fast_rotation_ext_batch_group(ctx.handle, chain, group, pc, pd, kk, dnum,
                                                                               el, count, po, s))
    else:
        c.call = lambda s, x: ck(env.lib.phantom_fast_rotation_ext_batch(ctx.handle, chain, ptr(cts[0]), ptr(digs[0]), kk,
                                                                         dnum, el, count, po, s))


@case("fast_rotation_ext_batch", ["phantom_fast_rotation_ext_batch"])
def _(env, c):
    _rotation_batch(env, c, 0)


@case("fast_rotation_ext_batch_group", ["phantom_fast_rotation_ext_batch_group"], blocks=True)
def _(env, c):
    _rotation_batch(env, c, 2)


def _rotate_accumulate(env, c, group):
    ctx, chain = env.small(), 2
    em = ext_mods(ctx, chain)
    G = max(group, 1)
    exts = [c.inp(rl(env.rng, N, em, 2), N) for _ in range(G)]  # clobbered: restaged before every call
    accs = [c.inp(rl(env.rng, N, em, 2), N, inout=True) for _ in range(G)]
    ((_, _, kp),), dnum = env.keys(c, ctx)
    elt = pow(5, 1024, 2 * N)
    if group:
        pe, pa = c.hold(vp(exts)), c.hold(vp(accs))
        c.call = lambda s, x: ck(env.lib.phantom_rotate_ext_accumulate_group(ctx.handle, chain, group, pe, kp, dnum, elt,
                                                                             pa, 1, s))
    else:
        c.call = lambda s, x: ck(env.lib.phantom_rotate_ext_accumulate(ctx.handle, chain, ptr(exts[0]), kp, dnum, elt,
                                                                       ptr(accs[0]), 1, s))


@case("rotate_ext_accumulate", ["phantom_rotate_ext_accumulate"])
def _(env, c):
    _rotate_accumulate(env, c, 0)


@case("rotate_ext_accumulate_group", ["phantom_rotate_ext_accumulate_group"])
def _(env, c):
    _rotate_accumulate(env, c, 2)


@case("tensor_lin", ["phantom_tensor_lin"])
def _(env, c):
    ctx, chain = env.small(), 4
    ql, tl = ctx.ql(chain), ctx.ql(chain - 2)
    L = len(ql)
    da, db, dt = c.inp(rl(env.rng, N, ql, 2), N), c.inp(rl(env.rng, N, ql, 2), N), c.inp(rl(env.rng, N, tl, 2), N)
    f, cc = residues(env.rng, ql), residues(env.rng, ql)
    out = c.out(3 * L * N)
    c.call = lambda s, x: ck(env.lib.phantom_tensor_lin(ctx.handle, chain, ptr(da), ptr(db), ptr(out), f.ctypes.data,
                                                        ptr(dt), len(tl) * N, cc.ctypes.data, s))


@case("tensor_lin_batch", ["phantom_tensor_lin_batch"])
def _(env, c):
    ctx, chain, cnt = env.small(), 4, 3
    ql, tl = ctx.ql(chain), ctx.ql(chain - 2)
    L = len(ql)
    A = [c.inp(rl(env.rng, N, ql, 2), N) for _ in range(cnt)]
    B = [c.inp(rl(env.rng, N, ql, 2), N) for _ in range(cnt)]
    T = [c.inp(rl(env.rng, N, tl, 2), N) for _ in range(cnt)]
    C, K = residues(env.rng, ql, cnt), residues(env.rng, ql, cnt)
    outs = [c.out(3 * L * N) for _ in range(cnt)]
    facs = O.arr([1, 2, 3])
    pa, pb, po = vp(A), vp(B), vp(outs)
    pt = vp([T[0], None, T[2]])
    pc = PA.ptr_array([C[0].ctypes.data, 0, C[2].ctypes.data])
    pk = PA.ptr_array([K[0].ctypes.data, K[1].ctypes.data, 0])
    c.hold(pa, pb, po, pt, pc, pk, C, K, facs)
    c.call = lambda s, x: ck(env.lib.phantom_tensor_lin_batch(ctx.handle, chain, cnt, pa, pb, po, facs.ctypes.data, pt,
                                                              len(tl) * N, pc, pk, s))


@case("lin_comb", ["phantom_lin_comb"])
def _(env, c):
    ctx, chain = env.small(), 4
    ql, tl = ctx.ql(chain), ctx.ql(chain - 3)
    d, t = c.inp(rl(env.rng, N, ql, 2), N, inout=True), c.inp(rl(env.rng, N, tl, 2), N)
    ca, cb = residues(env.rng, ql), residues(env.rng, ql)
    c.call = lambda s, x: ck(env.lib.phantom_lin_comb(ctx.handle, chain, ptr(d), 2, ca.ctypes.data, ptr(t), 2,
                                                      len(tl) * N, cb.ctypes.data, s))


@case("mul_scalar", ["phantom_mul_scalar"])
def _(env, c):
    ctx, chain = env.small(), 4
    ql, tl = ctx.ql(chain), ctx.ql(chain - 3)
    t, acc = c.inp(rl(env.rng, N, tl, 2), N), c.inp(rl(env.rng, N, ql, 2), N)
    ca = residues(env.rng, ql)
    out = c.out(2 * len(ql) * N)
    c.call = lambda s, x: ck(env.lib.phantom_mul_scalar(ctx.handle, chain, ptr(t), len(tl) * N, ca.ctypes.data, ptr(acc),
                                                        ptr(out), 2, s))


@case("leaf_combine", ["phantom_leaf_combine"], blocks=True)
def _(env, c):
    ctx, chain, K, M = env.small(), 4, 3, 2
    ql = ctx.ql(chain)
    L = len(ql)
    ins, strides = [], []
    for k in range(K):
        lk = ctx.ql(chain - (k % 3))
        ins.append(c.inp(rl(env.rng, N, lk, 2), N))
        strides.append(len(lk) * N)
    coef, cadd = residues(env.rng, ql, M, K), residues(env.rng, ql, M)
    outs = [c.out(2 * L * N) for _ in range(M)]
    st = (PA.sz * K)(*strides)
    pi, po = c.hold(vp(ins)), c.hold(vp(outs))
    c.call = lambda s, x: ck(env.lib.phantom_leaf_combine(ctx.handle, chain, pi, st, K, coef.ctypes.data, cadd.ctypes.data,
                                                          po, M, s))


@case("lt_bsgs", ["phantom_lt_bsgs"], blocks=True)
def _(env, c):
    ctx, chain, g, b = env.small(), 5, 4, 3
    em = ext_mods(ctx, chain)
    babies = [c.inp(rl(env.rng, N, em, 2), N) for _ in range(g)]
    pts = [c.inp(rl(env.rng, N, em), N) for _ in range(g * b)]
    outs = [c.out(2 * len(em) * N) for _ in range(b)]
    pb, pp, po = c.hold(vp(babies)), c.hold(vp(pts)), c.hold(vp(outs))
    c.call = lambda s, x: ck(env.lib.phantom_lt_bsgs(ctx.handle, chain, pb, g, pp, b, po, s))


@case("lt_bsgs_group", ["phantom_lt_bsgs_group"], blocks=True)
def _(env, c):
    ctx, chain, g, b, group = env.small(), 5, 32, 2, 2
    em = ext_mods(ctx, chain)
    W = 2 * len(em) * N
    babies = [c.inp(rl(env.rng, N, em, 2 * g), N) for _ in range(group)]
    pts = [c.inp(rl(env.rng, N, em), N) for _ in range(g * b)]
    acc = [c.out(W) for _ in range(group)]
    giants = [c.out((b - 1) * W) for _ in range(group)]
    pb, pp, pa, pg = c.hold(vp(babies)), c.hold(vp(pts)), c.hold(vp(acc)), c.hold(vp(giants))
    c.call = lambda s, x: ck(env.lib.phantom_lt_bsgs_group(ctx.handle, chain, group, pb, W, g, pp, b, pa, pg, W, s))


# ---- DNN / packing -------------------------------------------------------------------------------------

@case("ct_mix", ["phantom_ct_mix"])
def _(env, c):
    ctx, chain, K, M = env.small(), 2, 5, 3
    ql = ctx.ql(chain)
    ins = [c.inp(rl(env.rng, N, ql, 2), N) for _ in range(K)]
    coef, cadd = residues(env.rng, ql, M, K), residues(env.rng, ql, M)
    outs = [c.out(2 * len(ql) * N) for _ in range(M)]
    pi, po = c.hold(vp(ins)), c.hold(vp(outs))
    c.call = lambda s, x: ck(env.lib.phantom_ct_mix(ctx.handle, chain, pi, K, coef.ctypes.data, cadd.ctypes.data, po, M, s))


def _ct_pack(C):
    def f(env, c):
        ctx, chain = env.small(), 2
        ql = ctx.ql(chain)
        base = [c.inp(rl(env.rng, N, ql, 2), N) for _ in range(min(C, 5))]
        pi = c.hold(vp([base[(3 * k + 1) % len(base)] for k in range(C)]))
        out = c.out(2 * len(ql) * N)
        c.call = lambda s, x: ck(env.lib.phantom_ct_pack(ctx.handle, chain, pi, C, 4, ptr(out), s))
    return f


case("ct_pack[4]", ["phantom_ct_pack"])(_ct_pack(4))
case("ct_pack[32]", ["phantom_ct_pack"])(_ct_pack(32))


def _ct_split(count):
    def f(env, c):
        ctx, chain = env.small(), 2
        ql = ctx.ql(chain)
        words = 2 * len(ql) * N
        base = [c.inp(rl(env.rng, N, ql, 2), N) for _ in range(4)]
        a = [base[(2 * k) % 4] for k in range(count)]
        r = [base[(2 * k + 1 + (k & 1)) % 4] for k in range(count)]
        even = [c.out(words) for _ in range(count)]
        odd = [c.out(words) for _ in range(count - 1)] + [None]
        pa, pr, pe, po = c.hold(vp(a)), c.hold(vp(r)), c.hold(vp(even)), c.hold(vp(odd))
        c.call = lambda s, x: ck(env.lib.phantom_ct_split(ctx.handle, chain, pa, pr, count, 24, pe, po, s))
    return f


case("ct_split[3]", ["phantom_ct_split"])(_ct_split(3))
case("ct_split[16]", ["phantom_ct_split"])(_ct_split(16))


@case("keyswitch_rotate_many", ["phantom_keyswitch_rotate_many"])
def _(env, c):
    ctx, chain, count = env.small(), 1, 3
    em = ext_mods(ctx, chain)
    cts = [c.inp(rl(env.rng, N, ctx.ql(chain), 2), N) for _ in range(count)]
    digs = [c.inp(rl(env.rng, N, em, beta_of(ctx, chain)), N) for _ in range(count)]
    outs = [c.out(2 * len(em) * N) for _ in range(count)]
    ((_, _, kp),), dnum = env.keys(c, ctx)
    elt = pow(5, 77, 2 * N)
    pc, pd, po = c.hold(vp(cts)), c.hold(vp(digs)), c.hold(vp(outs))
    c.call = lambda s, x: ck(env.lib.phantom_keyswitch_rotate_many(ctx.handle, chain, count, pc, pd, kp, dnum, elt, po, s))


def _rotate_fused(count):
    def f(env, c):
        """the key array is first seen by the side stream's cold call (a fresh context)"""
        quiet_ctx, chain = env.small(), 2
        ql = quiet_ctx.ql(chain)
        cts = [c.inp(rl(env.rng, N, ql, 2), N) for _ in range(count)]
        outs = [c.out(2 * len(ql) * N) for _ in range(count)]
        ((_, _, kp),), dnum = env.keys(c, quiet_ctx)
        elt = pow(5, 9, 2 * N)
        pc, po = c.hold(vp(cts)), c.hold(vp(outs))
        c.make_ctx = env.fresh_small(c)
        c.call = lambda s, x: ck(env.lib.phantom_rotate_fused_batch((x or quiet_ctx).handle, chain, count, pc, kp, dnum,
                                                                    elt, po, s))
    return f


case("rotate_fused_batch[3]", ["phantom_rotate_fused_batch"])(_rotate_fused(3))
case("rotate_fused_batch[9]", ["phantom_rotate_fused_batch"])(_rotate_fused(9))


def _mac(env, c, kind):
    """T = 5 terms, O = 2 outputs; sub: compact plaintexts of 128 words; seeded: residual and bias"""
    ctx, chain, T, Oc = env.conv_ctx(), 1, 5, 2
    em, ql = ext_mods(ctx, chain), ctx.ql(chain)
    M = N if kind == "full" else 128
    ins = [c.inp(rl(env.rng, N, em, 2), N) for _ in range(T)]
    pts = [c.inp(rl(env.rng, M, em), M) for _ in range(T * Oc)]
    table = c.const(np.array([ptr(p) for p in pts], dtype=np.uint64))
    outs = [c.out(2 * len(em) * N) for _ in range(Oc)]
    pi, po = c.hold(vp(ins)), c.hold(vp(outs))
    if kind == "full":
        c.call = lambda s, x: ck(env.lib.phantom_ext_mac(ctx.handle, chain, pi, T, ptr(table), Oc, po, 0, s))
    elif kind == "sub":
        c.call = lambda s, x: ck(env.lib.phantom_ext_mac_sub(ctx.handle, chain, pi, T, ptr(table), M, Oc, po, 0, s))
    else:
        res = [c.inp(rl(env.rng, N, ql, 2), N) for _ in range(Oc)]
        pres = c.hold(vp(res))
        mult, bias = residues(env.rng, ql), residues(env.rng, ql, Oc)
        c.call = lambda s, x: ck(env.lib.phantom_ext_mac_sub_seeded(ctx.handle, chain, pi, T, ptr(table), M, Oc, po, pres,
                                                                    mult.ctypes.data, bias.ctypes.data, s))


@case("ext_mac", ["phantom_ext_mac"], blocks=True)
def _(env, c):
    _mac(env, c, "full")


@case("ext_mac_sub", ["phantom_ext_mac_sub"], blocks=True)
def _(env, c):
    _mac(env, c, "sub")


@case("ext_mac_sub_seeded", ["phantom_ext_mac_sub_seeded"], blocks=True)
def _(env, c):
    _mac(env, c, "seeded")


@case("rotate_sum_ext", ["phantom_rotate_sum_ext"], blocks=True)
def _(env, c):
    ctx, chain, count = env.conv_ctx(), 1, 3
    em = ext_mods(ctx, chain)
    ct, dig = c.inp(rl(env.rng, N, ctx.ql(chain), 2), N), c.inp(rl(env.rng, N, em, beta_of(ctx, chain)), N)
    keysets, dnum = env.keys(c, ctx, 2)
    kk = c.hold(key_table([keysets[k % 2][2] for k in range(count)]))
    el = (ctypes.c_uint32 * count)(5, 25, 2 * N - 1)
    out = c.out(2 * len(em) * N)
    c.call = lambda s, x: ck(env.lib.phantom_rotate_sum_ext(ctx.handle, chain, ptr(ct), ptr(dig), kk, dnum, el, count, 1,
                                                            ptr(out), s))


CONV_SHAPE = (8, 0, 3, 2, 2)  # width 8, 3 x 3, 2 -> 2 channels
CONV_SCALE = float(1 << 40)


@case("conv_weight_slots", ["phantom_conv_weight_slots"])
def _(env, c):
    width, slotstr, K, in_ch, out_ch = CONV_SHAPE
    terms = out_ch * in_ch * K * K
    W = env.rng.uniform(-1, 1, size=(K, K, in_ch, out_ch))
    dW, out = c.inp(W, W.size), c.out(terms * 2 * PA.Conv.slots(width, slotstr))
    c.call = lambda s, x: PA.Conv.weight_slots(CONV_SHAPE, ptr(dW), 0, terms, ptr(out), s)


def _conv_operands(env, c, gate_w):
    ctx, chain = env.conv_ctx(), 1
    width, slotstr, K, in_ch, out_ch = CONV_SHAPE
    ql = ctx.ql(chain)
    cts = [c.inp(rl(env.rng, N, ql, 2), N) for _ in range(in_ch)]
    keysets, dnum = env.keys(c, ctx, 3)
    K2 = K * K
    kk = c.hold(key_table([None if k == K2 // 2 else keysets[k % 3][2] for k in range(K2)]))
    el = (ctypes.c_uint32 * K2)(*[pow(5, int(r) % (N // 2), 2 * N) for r in PA.Conv.rotations(width, slotstr, K)])
    W = env.rng.uniform(-1, 1, size=(K, K, in_ch, out_ch))
    dW = c.inp(W, W.size) if gate_w else c.const(W)
    outs = [c.out(2 * len(ql) * N) for _ in range(out_ch)]
    return ctx, chain, cts, kk, dnum, el, dW, outs


@case("conv2d", ["phantom_conv2d"])
def _(env, c):
    ctx, chain, cts, kk, dnum, el, dW, outs = _conv_operands(env, c, True)
    width, slotstr, K, in_ch, out_ch = CONV_SHAPE
    pc, po = c.hold(vp(cts)), c.hold(vp(outs))
    c.call = lambda s, x: ck(env.lib.phantom_conv2d(ctx.handle, chain, pc, in_ch, out_ch, width, slotstr, K, ptr(dW),
                                                    CONV_SCALE, kk, dnum, el, 0, po, None, s))


def _conv_apply(env, c, seeded):
    ctx, chain, cts, kk, dnum, el, dW, outs = _conv_operands(env, c, False)
    t = torch()
    t.cuda.synchronize()
    plan = PA.Conv.prepare(ctx, chain, CONV_SHAPE, ptr(dW), CONV_SCALE, t.cuda.current_stream().cuda_stream)
    c.cleanup.append(plan.close)
    pc, po = c.hold(vp(cts)), c.hold(vp(outs))
    if seeded:
        ql = ctx.ql(chain)
        res = [c.inp(rl(env.rng, N, ql, 2), N) for _ in range(len(outs))]
        pres = c.hold(vp(res))
        mult, bias = residues(env.rng, ql), residues(env.rng, ql, len(outs))
        c.call = lambda s, x: PA.Conv.apply_seeded(ctx, plan, pc, kk, dnum, el, po, pres, mult, bias, s)
    else:
        c.call = lambda s, x: PA.Conv.apply(ctx, plan, pc, kk, dnum, el, po, s)


@case("conv2d_apply", ["phantom_conv2d_apply"])
def _(env, c):
    _conv_apply(env, c, False)


@case("conv2d_apply_seeded", ["phantom_conv2d_apply_seeded"])
def _(env, c):
    _conv_apply(env, c, True)


def _conv_prepare(env, c, scaled):
    """the output is the plan's words, read back with phantom_conv_plan_read (which waits for the device)"""
    ctx, chain = env.conv_ctx(), 1
    t = torch()
    width, slotstr, K, in_ch, out_ch = CONV_SHAPE
    W = env.rng.uniform(-1, 1, size=(K, K, in_ch, out_ch))
    dW = c.inp(W, W.size)
    words = out_ch * in_ch * K * K * len(ext_mods(ctx, chain)) * 2 * PA.Conv.slots(width, slotstr)
    out = c.out(words)
    sc = np.array([0.75, -1.25]) if scaled else None

    def call(s, x):
        if scaled:
            plan = PA.Conv.prepare_scaled(ctx, chain, CONV_SHAPE, ptr(dW), sc, CONV_SCALE, s)
        else:
            plan = PA.Conv.prepare(ctx, chain, CONV_SHAPE, ptr(dW), CONV_SCALE, s)
        try:
            w = plan.words()
        finally:
            plan.close()
        assert w.size == words
        with on_stream(s):
            out.copy_(t.from_numpy(w.view(np.int64)))
    c.call = call


@case("conv2d_prepare", ["phantom_conv2d_prepare"], blocks=True)
def _(env, c):
    _conv_prepare(env, c, False)


@case("conv2d_prepare_scaled", ["phantom_conv2d_prepare_scaled"], blocks=True)
def _(env, c):
    _conv_prepare(env, c, True)


@case("avgpool_fc", ["phantom_avgpool_fc"])
def _(env, c):
    ctx, chain = env.conv_ctx(), 1
    width, slotstr, t_in, T = 4, 0, 2, 2
    ql = ctx.ql(chain)
    R = width - 1
    cts = [c.inp(rl(env.rng, N, ql, 2), N) for _ in range(t_in)]
    keysets, dnum = env.keys(c, ctx, 3)
    rots = np.zeros(2 * R, dtype=np.int32)
    cnt = PA.sz(0)
    ck(env.lib.phantom_avgpool_rotations(width, slotstr, rots.ctypes.data, len(rots), ctypes.byref(cnt)))
    elts = [pow(5, int(r) % (N // 2), 2 * N) for r in rots]
    colk = c.hold(key_table([keysets[i % 3][2] for i in range(R)]))
    rowk = c.hold(key_table([keysets[(R + i) % 3][2] for i in range(R)]))
    ce, re_ = (ctypes.c_uint32 * R)(*elts[:R]), (ctypes.c_uint32 * R)(*elts[R:])
    coef, bias = residues(env.rng, ql, T, t_in), residues(env.rng, ql, T)
    outs = [c.out(2 * len(ql) * N) for _ in range(T)]
    pc, po = c.hold(vp(cts)), c.hold(vp(outs))
    c.call = lambda s, x: ck(env.lib.phantom_avgpool_fc(ctx.handle, chain, pc, t_in, T, width, slotstr, coef.ctypes.data,
                                                        bias.ctypes.data, colk, rowk, dnum, ce, re_, po, s))


# ---- encoder ------------------------------------------------------------------------------------------

def _ring():
    from test_gpu_encrypt_batch import ring
    return ring(12)


def _complex(rng, *shape):
    return rng.uniform(-1, 1, shape) + 1j * rng.uniform(-1, 1, shape)


ENC_SCALE = 2.0**40


def _embed(forward):
    def f(env, c):
        R, count = _ring(), 2
        if forward:
            x, out = c.inp(env.rng.uniform(-1, 1, (count, N)), N), c.out(count * N)
        else:
            x, out = c.inp(_complex(env.rng, count, N // 2), N // 2), c.out(count * N)
        c.call = lambda s, ctx: R.enc.embed(forward, ptr(x), ptr(out), s, 0, count)
    return f


case("ckks_embed[inverse]", ["phantom_ckks_embed"])(_embed(False))
case("ckks_embed[forward]", ["phantom_ckks_embed"])(_embed(True))


@case("ckks_round_rns", ["phantom_ckks_round_rns"])
def _(env, c):
    R, chain, count = _ring(), 1, 2
    x = c.inp(env.rng.uniform(-1, 1, (count, N)), N)
    out = c.out(count * R.enc.limbs(chain, True) * N)
    c.call = lambda s, ctx: R.enc.round_rns(chain, ptr(x), ENC_SCALE, ptr(out), s, ext=True, count=count)


@case("ckks_compose", ["phantom_ckks_compose"])
def _(env, c):
    R, chain, count = _ring(), 1, 2
    x = c.inp(rl(env.rng, N, R.ctx.ql(chain), count), N)
    out = c.out(count * N)
    c.call = lambda s, ctx: R.enc.compose(chain, ptr(x), ptr(out), s, count=count)


@case("ckks_encode", ["phantom_ckks_encode"])
def _(env, c):
    R, chain, count = _ring(), 1, 2
    x = c.inp(_complex(env.rng, count, N // 2), N // 2)
    out = c.out(count * R.enc.limbs(chain) * N)
    c.call = lambda s, ctx: R.enc.encode(chain, ptr(x), N // 2, ENC_SCALE, ptr(out), s, count=count)


@case("ckks_decode", ["phantom_ckks_decode"])
def _(env, c):
    R, chain, count = _ring(), 2, 2
    ql = R.ctx.ql(chain)
    small = [np.concatenate([(env.rng.integers(-2**30, 2**30, N) % q).astype(np.uint64) for q in ql]) for _ in range(count)]
    x = c.inp(O.ntt_fwd(np.concatenate(small), N, ql * count), N)
    out = c.out(count * N)
    c.call = lambda s, ctx: R.enc.decode(chain, ptr(x), ENC_SCALE, ptr(out), s, count=count)


def _fresh_ring_ctx(c, R):
    def make():
        ctx = PA.Context(R.n, R.mods, 1)
        c.cleanup.append(ctx.close)
        return ctx
    return make


@case("ckks_encode_sub", ["phantom_ckks_encode_sub"])
def _(env, c):
    """the sub-ring tables of this degree are built on the side stream's first call (a fresh context)"""
    R, chain, count, sub = _ring(), 1, 2, 64
    x = c.inp(_complex(env.rng, count, sub), sub)
    out = c.out(count * R.enc.limbs(chain, True) * 2 * sub)
    c.make_ctx = _fresh_ring_ctx(c, R)
    c.call = lambda s, ctx: PA.Encoder(ctx or R.ctx).encode_sub(chain, ptr(x), sub, sub, ENC_SCALE, ptr(out), s, ext=True,
                                                                count=count)


@case("sub_ntt", ["phantom_sub_ntt"])
def _(env, c):
    R, chain, count, M = _ring(), 1, 2, 256
    x = c.inp(rl(env.rng, M, R.ctx.ql(chain), count), M, inout=True)
    c.make_ctx = _fresh_ring_ctx(c, R)
    c.call = lambda s, ctx: PA.Encoder(ctx or R.ctx).sub_ntt(chain, M, ptr(x), s, count=count)


# ---- samplers and encryption ----------------------------------------------------------------------------

@case("sample_uniform_seeded", ["phantom_sample_uniform_seeded"])
def _(env, c):
    R, L = _ring(), 3
    seed = bytes(range(64))
    out = c.out(L * N)
    c.call = lambda s, ctx: ck(env.lib.phantom_sample_uniform_seeded(R.h, seed, ptr(out), L, s))


@case("sample_poly", ["phantom_sample_poly"])
def _(env, c):
    from test_gpu_encrypt_batch import KEY
    R, L = _ring(), 3
    out = c.out(L * N)
    c.call = lambda s, ctx: ck(env.lib.phantom_sample_poly(R.h, 1, KEY.ctypes.data, (5 << 40) | 9, ptr(out), L, s))


@case("sample_cbd_small_batch", ["phantom_sample_cbd_small_batch"])
def _(env, c):
    R = _ring()
    out = c.out(3 * N, 4)
    c.call = lambda s, ctx: R.cry.sample_cbd_small([11, (7 << 40) | 5, 13], ptr(out), s)


@case("sample_small_batch", ["phantom_sample_small_batch"])
def _(env, c):
    from test_gpu_encrypt_asym_batch import ring
    R = ring(12)
    out = c.out(3 * N, 4)
    c.call = lambda s, ctx: R.pub.sample_small(PA.PublicEncryptor.TERNARY, [11, (7 << 40) | 5, 13], ptr(out), s)


@case("encrypt_symmetric_batch", ["phantom_encrypt_symmetric_batch"])
def _(env, c):
    from test_gpu_encrypt_batch import nonce, seed
    R, chain, count = _ring(), 1, 3
    x = c.inp(_complex(env.rng, count, N // 2), N // 2)
    out = c.out(count * 2 * R.limbs(chain) * N)
    nn, seeds = [nonce(p) for p in range(count)], b"".join(seed(p) for p in range(count))
    c.call = lambda s, ctx: R.cry.encrypt(chain, ptr(x), N // 2, ENC_SCALE, nn, seeds, ptr(out), s)


def _decrypt(decode):
    def f(env, c):
        R, polys, limbs, count = _ring(), 2, 3, 2
        x = c.inp(rl(env.rng, N, R.mods[:limbs], polys * count), N)
        if decode:
            out = c.out(count * N)
            c.call = lambda s, ctx: R.cry.decrypt_decode(ptr(x), polys, limbs, limbs, count, ENC_SCALE, ptr(out), s)
        else:
            out = c.out(count * limbs * N)
            c.call = lambda s, ctx: R.cry.decrypt(ptr(x), polys, limbs, limbs, count, ptr(out), s)
    return f


case("decrypt_batch", ["phantom_decrypt_batch"])(_decrypt(False))
case("decrypt_decode_batch", ["phantom_decrypt_decode_batch"])(_decrypt(True))


@case("encrypt_asymmetric_batch", ["phantom_encrypt_asymmetric_batch"])
def _(env, c):
    from test_gpu_encrypt_asym_batch import nonces, ring
    R, chain, count = ring(12), 1, 2
    x = c.inp(_complex(env.rng, count, N // 2), N // 2)
    out = c.out(count * 2 * R.limbs(chain) * N)
    nn = [v for p in range(count) for v in nonces(p)]
    c.call = lambda s, ctx: R.pub.encrypt(chain, ptr(x), N // 2, ENC_SCALE, nn, ptr(out), s)


# ---- linear-transform setup ---------------------------------------------------------------------------
# stage_products, presence and finish upload a small table first and wait for the stream once, as the
# header says ("one wait for `stream`"): they may block.  dense_diagonals has no table.

def _prep():
    from test_gpu_ltprep import prep
    return prep()


@case("ltprep_stage_products", ["phantom_ltprep_stage_products"], blocks=True)
def _(env, c):
    """no device input: checked on the output side only"""
    P, ns, stages = _prep(), 256, [4, 3, 2, 1]
    out, scratch = c.out(2 * ns * ns), c.out(2 * ns * ns)
    c.call = lambda s, ctx: P.stage_products(ns, True, stages, ptr(out), ptr(scratch), ns, s)
    c.outs = [o for o in c.outs if o is not scratch]  # its final content is unspecified


def _band(env):
    from test_gpu_ltprep import host_products
    return host_products(256, True, [4, 3, 2, 1])


@case("ltprep_presence", ["phantom_ltprep_presence"], blocks=True)
def _(env, c):
    ns = 256
    off, band = _band(env)
    # a rotated band may have the same presence flags: the first decoy is the zero band (no flag set)
    x = c.inp(band, ns, decoys=(np.zeros_like(band), H.rolled(band, ns, 1)))
    flags = c.out(2 * len(off), 4)
    c.call = lambda s, ctx: PA.LtPrep.presence(ptr(x), ns, off, ptr(flags), s, const=0.37j)


@case("ltprep_finish", ["phantom_ltprep_finish"], blocks=True)
def _(env, c):
    ns, slots = 256, N // 2
    off, band = _band(env)
    keys = np.sort(PA.LtPrep.finish_host(band, ns, slots, off, 1, 0, const=0.37j, mask=1)[1])
    shape = PA.LtPrep.shape(slots, keys, 1, 0)
    x = c.inp(band, ns)
    out = c.out(2 * len(keys) * slots)
    c.call = lambda s, ctx: PA.LtPrep.finish(ptr(x), ns, slots, off, keys, shape, ptr(out), s, const=0.37j, mask=1)


@case("ltprep_dense_diagonals", ["phantom_ltprep_dense_diagonals"])
def _(env, c):
    slots = 256
    A = _complex(env.rng, slots, slots)
    p = np.arange(slots)
    A[p, (p + 37) % slots] = 0.0
    x = c.inp(A, slots)
    out, flags = c.out(2 * slots * slots), c.out(slots, 4)
    c.call = lambda s, ctx: PA.LtPrep.dense_diagonals(ptr(x), slots, 0.75, ptr(out), ptr(flags), s)


# ---- the tests -----------------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def env(rng):
    e = Env(rng)
    yield e
    torch().cuda.synchronize()


_log = []


def _note(line):
    _log.append(line)
    print(line)


@pytest.mark.gpu
def test_delay_delays(env):
    """the calibrated delay holds a stream for about what was asked (events), within a factor of two"""
    t = torch()
    d = H.delay()
    S = H.fresh_stream()
    a, b = t.cuda.Event(enable_timing=True), t.cuda.Event(enable_timing=True)
    t.cuda.synchronize()
    with t.cuda.stream(S):
        a.record(S)
        d.enqueue(20.0)
        b.record(S)
    queued = not b.query()
    b.synchronize()
    ms = a.elapsed_time(b)
    _note(f"delay: {d.describe()}; asked 20 ms, measured {ms:.2f} ms")
    assert queued and 10.0 <= ms <= 40.0, (d.describe(), ms)


@pytest.mark.gpu
def test_control_a_wrong_stream_is_detected(env):
    """an 'entry' that ignores its stream and copies on the default stream must be reported, as a mismatch of
    the result (it read the decoy): this also shows that side streams do not wait for stream 0"""
    c = H.Case("control A")
    _control(env, c, True)
    with pytest.raises(H.StreamOrderError, match="differ from the quiet run"):
        H.run_case(c)


@pytest.mark.gpu
def test_control_b_right_stream_passes(env):
    c = H.Case("control B")
    _control(env, c, False)
    H.run_case(c, log=_note)


@pytest.mark.gpu
def test_control_c_hidden_wait_is_detected(env):
    """an 'entry' that waits for its stream is reported when it is declared not to block"""
    t = torch()
    c = H.Case("control C")
    _control(env, c, False)
    copy = c.call

    def call(s, ctx):
        copy(s, ctx)
        t.cuda.ExternalStream(s).synchronize()
    c.call = call
    with pytest.raises(H.StreamOrderError, match="opened during a call"):
        H.run_case(c)


_gpu_errors = []


def _guarded(name, f):
    """after an error that is not a verdict of the harness (a HIP error, say) nothing more is started on
    the device by this module: the remaining cases fail at once"""
    if _gpu_errors:
        pytest.fail(f"not run: {_gpu_errors[0]} ended with an error of the runtime or the library")
    try:
        f()
    except AssertionError:
        raise
    except Exception:
        _gpu_errors.append(name)
        raise


@pytest.mark.gpu
@pytest.mark.parametrize("name", list(CASES))
def test_stream_order(env, name):
    _guarded(name, lambda: H.run_case(build(env, name), log=_note))


PAIRS = ["nwt_forward_inplace", "keyswitch", "moddown_rescale", "rotate_fused_batch[3]", "ckks_encode",
         "encrypt_symmetric_batch", "conv2d_apply"]


@pytest.mark.gpu
@pytest.mark.parametrize("name", PAIRS)
def test_two_streams_at_once(env, name):
    """two instances with different inputs on one context, each on its own held stream, four rounds issued
    alternately: every round's bytes equal that instance's quiet run.  Opportunistic: the kernels overlap
    only when the device schedules them so; NOT deterministic."""
    def run():
        a, b = build(env, name), build(env, name)
        a.make_ctx = b.make_ctx = None
        H.run_pair(a, b)
    _guarded(name, run)


# ---- completeness (CPU) ---------------------------------------------------------------------------------

def stream_entries(header=PA.HEADER_PATH):
    """every prototype of the header with a hipStream_t parameter"""
    txt = re.sub(r"/\*.*?\*/", "", open(header).read(), flags=re.S)
    return sorted({m.group(1) for m in re.finditer(r"\b(phantom_[a-z0-9_]+)\s*\(([^;{]*?)\)\s*;", txt, flags=re.S)
                   if "hipStream_t" in m.group(2)})


def test_header_entries_are_covered():
    entries = stream_entries()
    assert len(entries) >= 78 and "phantom_keyswitch" in entries and "phantom_ct_split" in entries
    assert not [e for e in entries if e.startswith("phantom_boot_")]  # the session API takes no stream
    covered = {e for _, es, _ in CASES.values() for e in es}
    assert covered <= set(entries), sorted(covered - set(entries))
    assert not set(EXEMPT) & covered, sorted(set(EXEMPT) & covered)
    assert set(EXEMPT) <= set(entries) and all(len(r) > 20 for r in EXEMPT.values())
    missing = [e for e in entries if e not in covered and e not in EXEMPT]
    assert not missing, f"stream-taking entries without a stream-order case: {missing}"
    assert set(PAIRS) <= set(CASES)
    # the header's list of entries that wait for the stream is the set of cases that may block
    head = open(PA.HEADER_PATH).read()
    listed = head[head.index("wait for `stream` once before they return"):head.index("#ifndef PHANTOM_AMD_H")]
    waits = set(re.findall(r"phantom_[a-z0-9_]+", listed))
    blocking = {e for _, es, b in CASES.values() if b for e in es} | {"phantom_bconv_create"}
    assert waits == blocking, sorted(waits ^ blocking)
