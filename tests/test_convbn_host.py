"""The algebra behind the fused batch norm / bias / residual of a prepared convolution, on the CPU:

  moddown(x + P v) == moddown(x) + v   word for word, for x over Ql u P and v over Ql: once over exact
                                       Python integers with the moddown formula written out, once
                                       through the oracle's moddown (or_moddown_from_ntt, NTT form)
  phantom_scaled_constant_residues     round(value * scale) mod q_l against Python integers: negative
                                       constants, constants above 2^64 and above 2^100, zero, and
                                       values below 2^53 that round

The seeded inner sum adds P (m res + B) on the Ql limbs and nothing on the P limbs (csrc/conv.h);
this identity is why its moddown equals the unseeded layer's plus m res + B exactly."""
from fractions import Fraction

import numpy as np
import pytest

import oracle_lib as O
import phantom_amd as PA

N = 64
BITS = [40, 30, 30, 30, 40, 40]  # 4 limbs of Q, 2 special primes
SIZE_P = 2


@pytest.fixture(scope="module")
def chain():
    mods = O.coeff_modulus_create(N, BITS)
    return mods[:-SIZE_P], mods[-SIZE_P:]


def _moddown_int(x_q, x_p, ql, p):
    """one word: (x_i - conv_{P -> q_i}([x]_P)) P^-1 mod q_i, the fast base conversion without
    overflow correction (src/rns_bconv.cu:791-843 as host/rns_tool.h describes it)"""
    P = 1
    for pj in p:
        P *= pj
    y = [(xj * pow(P // pj, -1, pj)) % pj for xj, pj in zip(x_p, p)]
    out = []
    for xi, qi in zip(x_q, ql):
        conv = sum(yj * ((P // pj) % qi) for yj, pj in zip(y, p)) % qi
        out.append(((xi - conv) * pow(P % qi, -1, qi)) % qi)
    return out


def test_moddown_shift_exact_integers(chain, rng):
    ql, p = chain
    P = p[0] * p[1]
    edge = [[q - 1 for q in ql], [0] * len(ql), [1] * len(ql)]
    for trial in range(200):
        x_q = [int(rng.integers(0, q)) for q in ql] if trial >= 3 else edge[trial]
        x_p = [int(rng.integers(0, q)) for q in p] if trial >= 3 else [q - 1 for q in p]
        v = [int(rng.integers(0, q)) for q in ql] if trial >= 3 else edge[trial]
        shifted = [(xi + (P % qi) * vi) % qi for xi, vi, qi in zip(x_q, v, ql)]  # the P limbs get 0
        base = _moddown_int(x_q, x_p, ql, p)
        assert _moddown_int(shifted, x_p, ql, p) == [(b + vi) % qi for b, vi, qi in zip(base, v, ql)]


@pytest.mark.parametrize("levels", [4, 2])
def test_moddown_shift_oracle(chain, rng, levels):
    """the oracle's moddown on NTT-form polynomials, at the full level and two limbs down"""
    ql, p = chain
    ql = ql[:levels]
    L = len(ql)
    P = p[0] * p[1]
    x = O.random_limbs(rng, N, list(ql) + list(p))
    v = O.random_limbs(rng, N, ql)
    v[:N] = ql[0] - 1  # a limb of the largest residue
    shifted = x.copy()
    for l, q in enumerate(ql):
        s = [(int(a) + (P % q) * int(b)) % q for a, b in zip(x[l * N:(l + 1) * N], v[l * N:(l + 1) * N])]
        shifted[l * N:(l + 1) * N] = np.array(s, dtype=np.uint64)

    def moddown(c):
        w = np.zeros(L * N, dtype=np.uint64)
        O.lib().or_moddown_from_ntt(O.P(c.copy()), O.P(w), N, O.P(O.arr(ql)), L, O.P(O.arr(p)), len(p))
        return w

    base, got = moddown(x), moddown(shifted)
    q = np.repeat(np.array(ql, dtype=np.uint64), N)
    s = base + v  # both below q < 2^41
    assert np.array_equal(got, np.where(s >= q, s - q, s))
    assert not np.array_equal(got, base)


def _want_residues(value, scale, mods):
    x = value * scale  # the product as the library forms it: one FP64 rounding
    B = int(Fraction(abs(x)) + Fraction(1, 2))  # nearest integer, halves away from zero
    return [(B % q) if x >= 0 else (q - B % q) % q for q in mods]


@pytest.mark.parametrize("value,scale", [
    (0.731, 2.0 ** 100), (-0.731, 2.0 ** 100),  # S_out of a 2^50 x 2^50 layer, above 2^64
    (-1.0, 2.0 ** 100), (1.0, 2.0 ** 118), (-0.3333333333333333, 2.0 ** 80 * 1.0000001),
    (1e-9, 2.0 ** 100), (3.0, 2.0 ** 64), (-2.5, 1.0), (2.5, 1.0), (0.49999, 1.0), (-1234.5678, 2.0 ** 30),
    (0.0, 2.0 ** 100), (-0.0, 2.0 ** 100), (0.1, 2.0 ** 52), (-0.1, 2.0 ** 53),
])
def test_scaled_constant_residues(chain, value, scale):
    ql, p = chain
    mods = list(ql) + [(1 << 61) - 1, 1152921504606830593]  # and two moduli of 61 and 60 bits
    m = np.array(mods, dtype=np.uint64)
    out = np.full(len(mods), 7, dtype=np.uint64)
    PA.check(PA.load().phantom_scaled_constant_residues(value, scale, m.ctypes.data, len(mods), out.ctypes.data))
    assert [int(r) for r in out] == _want_residues(value, scale, mods)
    assert all(int(r) < q for r, q in zip(out, mods))


def test_scaled_constant_residues_refused():
    lib = PA.load()
    m = np.array([97, 0], dtype=np.uint64)
    out = np.full(2, 7, dtype=np.uint64)
    bad = [lib.phantom_scaled_constant_residues(1.0, 2.0 ** 100, None, 1, out.ctypes.data),
           lib.phantom_scaled_constant_residues(1.0, 2.0 ** 100, m.ctypes.data, 1, None),
           lib.phantom_scaled_constant_residues(1.0, 2.0 ** 100, m.ctypes.data, 2, out.ctypes.data),  # a zero modulus
           lib.phantom_scaled_constant_residues(float("nan"), 2.0 ** 100, m.ctypes.data, 1, out.ctypes.data),
           lib.phantom_scaled_constant_residues(1.0, float("inf"), m.ctypes.data, 1, out.ctypes.data),
           lib.phantom_scaled_constant_residues(1.0, -2.0, m.ctypes.data, 1, out.ctypes.data)]
    assert bad == [1] * len(bad), bad
    assert [int(x) for x in out] == [7, 7]
