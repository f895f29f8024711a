"""Operands and moduli at the edges of the kernels' lazy-reduction and quotient bounds (a helper
module for tests/test_arith_bounds.py and tests/test_gpu_edges.py, not a conftest).

Uniform random residues sit around half of every worst case; the patterns here put every 30-bit
half, every lazy range and every quotient estimate at (or next to) its stated limit:

  edge_limbs(n, moduli, pattern)   [L][n] residues: max, lowmax, stripes, impulse, alt
  edge_primes(n)                   primes = 1 (mod 2n) nearest each regime edge (30 bits, 2^50, 2^60, 2^61)
  near_multiple_operands(...)      a sum of m products that is -1, 0 or 1 modulo q, the rest at max / lowmax
"""
import numpy as np

M30 = (1 << 30) - 1
PATTERNS = ("max", "lowmax", "stripes", "impulse", "alt")

# deterministic Miller-Rabin: these bases decide primality for every n < 3.3e24 > 2^64
_MR_BASES = (2, 3, 5, 7, 11, 13, 17, 19, 23, 29, 31, 37)


def is_prime(v):
    if v < 2:
        return False
    for p in _MR_BASES:
        if v % p == 0:
            return v == p
    d, s = v - 1, 0
    while d % 2 == 0:
        d //= 2
        s += 1
    for a in _MR_BASES:
        x = pow(a, d, v)
        if x in (1, v - 1):
            continue
        for _ in range(s - 1):
            x = x * x % v
            if x == v - 1:
                break
        else:
            return False
    return True


def prime_below(bound, n):
    """largest prime q < bound with q = 1 (mod 2n)"""
    m = 2 * n
    v = (bound - 2) // m * m + 1
    while v > m and not is_prime(v):
        v -= m
    assert v > m, "no such prime"
    return v


def prime_above(bound, n):
    """smallest prime q > bound with q = 1 (mod 2n)"""
    m = 2 * n
    v = bound // m * m + 1
    if v <= bound:
        v += m
    while not is_prime(v):
        v += m
    return v


EDGE_NAMES = ("30", "<2^50", ">2^50", "<2^60", ">2^60", "<2^61")


def edge_primes(n):
    """the six regime edges, in EDGE_NAMES order: a 30-bit prime (the largest below 2^30), the
    largest below / smallest above 2^50 (FP64 | integer NTT), below / above 2^60 (16q | 8q lazy
    ranges, 16 | 4 products per split partial sum), and the largest below 2^61 (the modulus bound)"""
    return [prime_below(1 << 30, n), prime_below(1 << 50, n), prime_above(1 << 50, n), prime_below(1 << 60, n),
            prime_above(1 << 60, n), prime_below(1 << 61, n)]


def lowmax(q):
    """the largest v < q whose low 30 bits are all ones (q - 1 of a prime = 1 mod 2n ends in zeros)"""
    v = (q - 1) | M30
    if v >= q:
        v -= 1 << 30
    return v if v >= 0 else q - 1  # q <= 2^30: no such value below q, the maximum instead


def stripe_values(q, rnd):
    """the ten stripes of one modulus (entries above q - 1 are taken modulo q)"""
    return [v % q for v in (0, 1, q - 1, q - 2, lowmax(q), (q - 1) // 2, (q + 1) // 2, M30, M30 + 1, rnd)]


def edge_limbs(n, moduli, pattern, rng=None):
    """[L][n] residues (flat uint64, limb-major like oracle_lib.random_limbs)"""
    assert pattern in PATTERNS, pattern
    rng = rng if rng is not None else np.random.default_rng(0xED6E)
    out = np.zeros(len(moduli) * n, dtype=np.uint64)
    for i, q in enumerate(moduli):
        q = int(q)
        row = out[i * n:(i + 1) * n]
        if pattern == "max":
            row[:] = q - 1
        elif pattern == "lowmax":
            row[:] = lowmax(q)
        elif pattern == "impulse":
            row[0] = q - 1
            row[n - 1] = q - 1
        elif pattern == "alt":
            row[0::2] = q - 1
        else:
            rnd = rng.integers(0, q, size=n, dtype=np.uint64)
            vals = stripe_values(q, 0)
            for k in range(10):
                row[k::10] = rnd[k::10] if k == 9 else vals[k]
    return out


def near_multiple_operands(q, m, target, a_fill="max", b_fill="max"):
    """m operand pairs (a_j, b_j), all below q, with sum_j a_j b_j = target (mod q) for target in
    {-1, 0, 1}: the first m - 1 pairs sit at a_fill / b_fill (max or lowmax), the last a stays there
    and the last b is solved for.  q prime (the fills are units)."""
    fill = {"max": q - 1, "lowmax": lowmax(q)}
    a, b = [fill[a_fill]] * m, [fill[b_fill]] * m
    rest = sum(x * y for x, y in zip(a[:-1], b[:-1]))
    b[-1] = (target - rest) * pow(a[-1], -1, q) % q
    assert sum(x * y for x, y in zip(a, b)) % q == target % q
    return a, b
