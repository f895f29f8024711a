"""The identity the compact sparse plaintexts rest on (CPU, oracle only).

With g = N / M and p(X) = p'(X^g), deg p' < M, the forward NTT of p in the engine's bit-reversed
order is constant on blocks of g, and its value on block i is p' evaluated at psi^(g (2 brv_M(i) + 1)):
the size-M negacyclic transform with root psi_N^g.  The GPU tests of the subring transform, the
compact encoder and the inner sums over compact plaintexts build their expected values from
or_ntt_fwd of the zero-stuffed polynomial, which this pins."""
import numpy as np
import pytest

import oracle_lib as O

N = 256


def brv(x, bits):
    return int(format(x, "0%db" % bits)[::-1], 2) if bits else 0


@pytest.fixture(scope="module")
def primes():
    return O.coeff_modulus_create(N, [50, 59, 60])


@pytest.mark.parametrize("M", [8, 32, 256])
def test_sub_ring_ntt(primes, M):
    rng = np.random.default_rng(0x5AB + M)
    g, logm = N // M, M.bit_length() - 1
    sub = O.random_limbs(rng, M, primes).reshape(len(primes), M)
    full = np.zeros((len(primes), N), dtype=np.uint64)
    full[:, ::g] = sub  # p(X) = p'(X^g)
    got = O.ntt_fwd(full.reshape(-1), N, primes).reshape(len(primes), N)
    for l, q in enumerate(primes):
        blocks = got[l].reshape(M, g)
        assert np.all(blocks == blocks[:, :1]), (M, q)
        tw, _ = O.ntt_tables(N, q)
        psi = int(tw[0][N // 2])  # tw[brv(1)] = psi
        assert pow(psi, N, q) == q - 1
        coeffs = [int(c) for c in sub[l]]
        for i in range(M):
            x = pow(psi, g * (2 * brv(i, logm) + 1), q)
            want = 0
            for c in reversed(coeffs):
                want = (want * x + c) % q
            assert int(blocks[i, 0]) == want, (M, q, i)
        # the subring's twiddle table is the head of the full one: brv_N(k) = g brv_M(k) for k < M
        for k in range(M):
            assert int(tw[0][k]) == pow(psi, g * brv(k, logm), q)
