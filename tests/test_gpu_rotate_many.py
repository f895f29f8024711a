"""phantom_keyswitch_rotate_many and phantom_rotate_fused_batch (many ciphertexts rotated under ONE
Galois key) on the GPU, through the C-ABI, bit-exact against the CPU oracle applied to each ciphertext
on its own (oracle/oracle.c restates EvalFastRotationExt with its fused P c0 / automorphism epilogue,
src/evaluate.cu:3660-3755, modup src/rns_bconv.cu:530-628 and moddown_from_NTT :791-843).

The kernel entry, reference or_fast_rotation_ext(ct, digits, keys, elt, add_first = 1) per ciphertext;
shapes are the smallest at which each code path and bound is reached:

  q61     n = 2^12, ten 61-bit moduli, P = 2, chain 1: beta = 4, the exact reduction with split partial
          sums at their bounds; count 3; inputs random, and every word (keys too) at q - 1
  q59     the same n with 59-bit moduli at chain 4: 5 limbs, a partial last digit (beta = 3), the
          approximate-quotient reduction; count 9 (past the lockstep group limit of 8)
  mixed   tests/test_gpu_pack.py's chain ([60] + [50] x 6 + [60] x 3, P = 3), n = 2^12: counts 1 and 64
          (the table's full length; the ciphertext loop split over the grid's second dimension), the
          conjugation element 2n - 1, and chain 5 with Ql = 3 <= P (beta = 1)
  n512    n = 512, below the automorphism block: the fallback to one launch per ciphertext; count 2
  c4      N = 2^16 on tests/test_gpu_group.py's C4 chain at chain index 18 (beta = 2), count 3

Operands are uniform random residues (parity is a property of the arithmetic, not of key or
ciphertext structure).  Every output is pre-filled with a marker and one spare buffer beyond `count`
must keep it.

phantom_rotate_fused_batch, n = 2^10 on the mixed chain, 70 ciphertexts made once: count = chunk + 1
and count = 70 (both cross the 64 of one launch) against or_modup -> or_fast_rotation_ext ->
or_moddown_from_ntt on both polynomials, and against the device composition phantom_modup +
phantom_fast_rotation_ext + phantom_moddown_from_ntt per ciphertext; count 0 returns OK and writes
nothing.  Refused arguments return a non-zero status and leave the marker-filled outputs as they were."""
import numpy as np
import pytest

import edge_cases as E
import oracle_lib as O
import phantom_amd as PA
from gpu_util import ptr, stream, to_dev, to_host, torch

pytestmark = pytest.mark.gpu

MIXED = [60] + [50] * 6 + [60] * 3
C4_BITS = [60] + [59] * 29 + [60] * 10
MARK = 0x5A5A5A5A5A5A5A5A

# name -> (log_n, bit sizes, special primes)
CHAINS = {"q61": (12, [61] * 10, 2), "q59": (12, [59] * 10, 2), "mixed": (12, MIXED, 3), "mixed10": (10, MIXED, 3),
          "n512": (9, [50] * 10, 2), "c4": (16, C4_BITS, 10)}


@pytest.fixture(scope="module")
def ctxs():
    made = {}

    def get(kind):
        if kind not in made:
            log_n, bits, size_p = CHAINS[kind]
            made[kind] = PA.Context(1 << log_n, O.coeff_modulus_create(1 << log_n, bits), size_p)
        return made[kind]

    yield get
    for c in made.values():
        c.close()


def _lib():
    return PA.load()


def _vp(ts):
    return PA.ptr_array([ptr(t) if t is not None else 0 for t in ts])


def _ext(ctx, chain):
    return ctx.ql(chain) + ctx.moduli[ctx.size_Q:]


def _beta(ctx, chain):
    return -(-len(ctx.ql(chain)) // ctx.size_P)


def _limbs(rng, pat, n, mods, polys=1):
    if pat == "random":
        return np.concatenate([O.random_limbs(rng, n, mods) for _ in range(polys)])
    return np.concatenate([E.edge_limbs(n, mods, "max")] * polys)


def _keys(rng, pat, ctx):
    dnum = -(-ctx.size_Q // ctx.size_P)
    keys = [_limbs(rng, pat, ctx.n, ctx.moduli, 2) for _ in range(dnum)]
    return keys, [to_dev(k) for k in keys]


def _marked(words):
    return to_dev(np.full(words, MARK, dtype=np.uint64))


def _untouched(t):
    return bool((to_host(t) == np.uint64(MARK)).all())


KERNEL_CASES = [
    ("q61", 1, 3, "rot", "random"), ("q61", 1, 3, "rot", "max"),
    ("q59", 4, 9, "rot", "random"),
    ("mixed", 1, 1, "rot", "random"), ("mixed", 1, 64, "conj", "random"), ("mixed", 5, 2, "rot", "random"),
    ("n512", 1, 2, "rot", "random"),
    ("c4", 18, 3, "rot", "random"),
]


@pytest.mark.parametrize("kind,chain,count,elt_kind,pat", KERNEL_CASES)
def test_keyswitch_rotate_many(ctxs, rng, kind, chain, count, elt_kind, pat):
    ctx = ctxs(kind)
    n, ql, em, beta = ctx.n, ctx.ql(chain), _ext(ctx, chain), _beta(ctx, chain)
    assert {"q61": beta == 4 and max(ctx.moduli) > 2**60, "q59": beta == 3 and len(ql) % ctx.size_P == 1,
            "mixed": beta == (3 if chain == 1 else 1), "n512": n < 1024, "c4": beta == 2}[kind]
    elt = pow(5, 77, 2 * n) if elt_kind == "rot" else 2 * n - 1
    keys, dkeys = _keys(rng, pat, ctx)
    cts = [_limbs(rng, pat, n, ql, 2) for _ in range(count)]
    digits = [_limbs(rng, pat, n, em, beta) for _ in range(count)]
    dcts, ddig = [to_dev(x) for x in cts], [to_dev(x) for x in digits]
    W = 2 * len(em) * n
    douts = [_marked(W) for _ in range(count + 1)]  # the last one is the spare
    PA.keyswitch_rotate_many(ctx, chain, [ptr(x) for x in dcts], [ptr(x) for x in ddig], _vp(dkeys), len(dkeys), elt,
                             [ptr(x) for x in douts[:count]], stream())
    mods = O.P(O.arr(ctx.moduli))
    for k in range(count):
        want = np.zeros(W, dtype=np.uint64)
        O.lib().or_fast_rotation_ext(O.P(cts[k]), O.P(digits[k]), O.ptrs(keys), elt, 1, O.P(want), n, len(ql),
                                     ctx.size_Q, ctx.size_P, mods)
        assert np.array_equal(to_host(douts[k]), want), k
    assert _untouched(douts[count])
    for x, h in zip(dcts + ddig, cts + digits):  # the inputs are read only
        assert np.array_equal(to_host(x), h)


@pytest.fixture(scope="module")
def fused(ctxs, rng):
    """70 ciphertexts at n = 2^10 with both references, computed once: the oracle composition and the
    device composition of the one-ciphertext entries"""
    ctx, chain, total = ctxs("mixed10"), 1, 70
    n, ql, p, em, beta = ctx.n, ctx.ql(chain), ctx.moduli[ctx.size_Q:], _ext(ctx, chain), _beta(ctx, chain)
    L, QlP = len(ql), len(em)
    elt = pow(5, 9, 2 * n)
    keys, dkeys = _keys(rng, "random", ctx)
    cts = [_limbs(rng, "random", n, ql, 2) for _ in range(total)]
    dcts = [to_dev(x) for x in cts]
    mods = O.P(O.arr(ctx.moduli))
    want, dev = [], []
    ddig, dext, dout = to_dev(np.zeros(beta * QlP * n, dtype=np.uint64)), _marked(2 * QlP * n), _marked(2 * L * n)
    lib = _lib()
    for k in range(total):
        tmu = np.zeros(beta * QlP * n, dtype=np.uint64)
        O.lib().or_modup(O.P(cts[k][L * n:].copy()), O.P(tmu), n, O.P(O.arr(ql)), L, O.P(O.arr(p)), len(p))
        ext = np.zeros(2 * QlP * n, dtype=np.uint64)
        O.lib().or_fast_rotation_ext(O.P(cts[k]), O.P(tmu), O.ptrs(keys), elt, 1, O.P(ext), n, L, ctx.size_Q, ctx.size_P,
                                     mods)
        w = np.zeros(2 * L * n, dtype=np.uint64)
        for t in range(2):
            c = ext[t * QlP * n:(t + 1) * QlP * n].copy()
            O.lib().or_moddown_from_ntt(O.P(c), O.P(w[t * L * n:]), n, O.P(O.arr(ql)), L, O.P(O.arr(p)), len(p))
        want.append(w)
        PA.check(lib.phantom_modup(ctx.handle, chain, ptr(dcts[k]) + 8 * L * n, ptr(ddig), stream()))
        PA.check(lib.phantom_fast_rotation_ext(ctx.handle, chain, ptr(dcts[k]), ptr(ddig), _vp(dkeys), len(dkeys), elt,
                                               1, ptr(dext), stream()))
        for t in range(2):
            PA.check(lib.phantom_moddown_from_ntt(ctx.handle, chain, ptr(dext) + 8 * t * QlP * n,
                                                  ptr(dout) + 8 * t * L * n, stream()))
        dev.append(to_host(dout))
    return dict(ctx=ctx, chain=chain, elt=elt, keys=dkeys, cts=cts, dcts=dcts, want=want, dev=dev, words=2 * L * n)


@pytest.mark.parametrize("count", ["chunk_plus_1", 70, 0])
def test_rotate_fused_batch(fused, count):
    f = fused
    ctx, chain = f["ctx"], f["chain"]
    chunk = PA.rotate_fused_batch_chunk(ctx, chain)
    assert 1 <= chunk <= 64
    count = chunk + 1 if count == "chunk_plus_1" else count
    douts = [_marked(f["words"]) for _ in range(count + 1)]
    PA.rotate_fused_batch(ctx, chain, [ptr(x) for x in f["dcts"][:count]], _vp(f["keys"]), len(f["keys"]), f["elt"],
                          [ptr(x) for x in douts[:count]], stream())
    for k in range(count):
        got = to_host(douts[k])
        assert np.array_equal(got, f["want"][k]), k
        assert np.array_equal(got, f["dev"][k]), k
    assert _untouched(douts[count])
    for x, h in zip(f["dcts"][:count], f["cts"]):
        assert np.array_equal(to_host(x), h)


def test_refusals(ctxs, rng):
    """every refusal of the two launching entries returns a non-zero status before any launch: the
    marker-filled outputs stay as they were"""
    ctx, chain, count = ctxs("mixed10"), 1, 3
    n, ql, em, beta = ctx.n, ctx.ql(chain), _ext(ctx, chain), _beta(ctx, chain)
    elt = pow(5, 9, 2 * n)
    _, dkeys = _keys(rng, "random", ctx)
    dnum = len(dkeys)
    dcts = [to_dev(_limbs(rng, "random", n, ql, 2)) for _ in range(count)]
    ddig = [to_dev(_limbs(rng, "random", n, em, beta)) for _ in range(count)]
    Wx, W = 2 * len(em) * n, 2 * len(ql) * n
    big = _marked(2 * Wx)  # two outputs' worth, for overlapping views
    dext = [_marked(Wx) for _ in range(count)]
    dout = [_marked(W) for _ in range(count)]
    lib, s = _lib(), stream()
    a = lambda ts: [ptr(t) if t is not None else 0 for t in ts]
    pa = PA.ptr_array
    cts, dig, ext, out, kd = a(dcts), a(ddig), a(dext), a(dout), _vp(dkeys)

    def many(chain_=chain, count_=count, cts_=pa(cts), dig_=pa(dig), kd_=kd, dnum_=dnum, outs_=pa(ext)):
        return lib.phantom_keyswitch_rotate_many(ctx.handle, chain_, count_, cts_, dig_, kd_, dnum_, elt, outs_, s)

    def whole(chain_=chain, count_=count, cts_=pa(cts), kd_=kd, dnum_=dnum, outs_=pa(out)):
        return lib.phantom_rotate_fused_batch(ctx.handle, chain_, count_, cts_, kd_, dnum_, elt, outs_, s)

    refused = {
        "many: null cts": many(cts_=None), "many: null digits": many(dig_=None), "many: null keys": many(kd_=None),
        "many: null outs": many(outs_=None), "many: null ct entry": many(cts_=pa([cts[0], 0, cts[2]])),
        "many: null digits entry": many(dig_=pa([dig[0], dig[1], 0])),
        "many: null out entry": many(outs_=pa([0, ext[1], ext[2]])),
        "many: count 65": many(count_=65, cts_=pa([cts[0]] * 65), dig_=pa([dig[0]] * 65), outs_=pa([ext[0]] * 65)),
        "many: count 0": many(count_=0),
        "many: chain 0": many(chain_=0), "many: chain past the end": many(chain_=ctx.size_Q + 1),
        "many: dnum below beta": many(dnum_=beta - 1),
        "many: two outputs overlap": many(outs_=pa([ptr(big), ptr(big) + 8 * (Wx - 2), ext[2]])),
        "many: an output is an input": many(outs_=pa([ext[0], dig[1], ext[2]])),
        "many: an output overlaps a ciphertext": many(cts_=pa([cts[0], ptr(big) + 16, cts[2]]),
                                                      outs_=pa([ext[0], ext[1], ptr(big)])),
        "whole: null cts": whole(cts_=None), "whole: null keys": whole(kd_=None), "whole: null outs": whole(outs_=None),
        "whole: null ct entry": whole(cts_=pa([cts[0], cts[1], 0])),
        "whole: null out entry": whole(outs_=pa([out[0], 0, out[2]])),
        "whole: chain 0": whole(chain_=0), "whole: chain past the end": whole(chain_=ctx.size_Q + 1),
        "whole: dnum below beta": whole(dnum_=beta - 1),
        "whole: two outputs overlap": whole(outs_=pa([ptr(big), ptr(big) + 8 * (W - 2), out[2]])),
        "whole: an output is an input": whole(outs_=pa([out[0], cts[2], out[2]])),
        "whole: the same output twice": whole(outs_=pa([out[0], out[1], out[0]])),
    }
    assert all(rc != 0 for rc in refused.values()), {k: rc for k, rc in refused.items() if rc == 0}
    torch().cuda.synchronize()
    for t in dext + dout + [big]:
        assert _untouched(t)
    assert lib.phantom_rotate_fused_batch_chunk(ctx.handle, 0, None) != 0
    assert whole(count_=0) == 0  # a no-op
    assert all(_untouched(t) for t in dout)
