"""CPU yardstick of symmetric CKKS encryption, from the oracle (oracle/oracle.c) and numpy alone:
the seed expansion, the centered-binomial error (chacha_np), the NTT and the elementwise products.
Test infrastructure only; tests/test_encrypt_reference.py checks it against itself, the GPU tests
compare the device's batched encryption with it."""
import numpy as np

import chacha_np as C
import oracle_lib as O


def expand_seed(seed, n, moduli):
    """`a` of a seed-compressed ciphertext: or_sample_uniform_seeded, [L][n]"""
    out = np.zeros(len(moduli) * n, dtype=np.uint64)
    O.lib().or_sample_uniform_seeded(bytes(seed), O.P(O.arr(moduli)), n, len(moduli), O.P(out))
    return out


def _binary(fn, a, b, n, moduli):
    out = np.zeros(len(moduli) * n, dtype=np.uint64)
    getattr(O.lib(), fn)(O.P(np.ascontiguousarray(a)), O.P(np.ascontiguousarray(b)), O.P(out), n, len(moduli),
                         O.P(O.arr(moduli)))
    return out


def mul(a, b, n, moduli):
    return _binary("or_poly_mul", a, b, n, moduli)


def sub(a, b, n, moduli):
    return _binary("or_poly_sub", a, b, n, moduli)


def add(a, b, n, moduli):
    return _binary("or_poly_add", a, b, n, moduli)


def cbd_signed(key, nonce, n):
    """the centred error e[k] in [-21, 21] of draw `nonce`"""
    q = 1 << 40
    v = C.sample_cbd(key, nonce, [q], n).astype(np.int64)
    return np.where(v > q // 2, v - q, v)


def residues(signed, moduli):
    """[L][n] residues of a signed integer vector (Python integers: any magnitude)"""
    return np.array([[int(v) % q for v in signed] for q in moduli], dtype=np.uint64).reshape(-1)


def encrypt(m_ntt, seed, key, nonce, s_ntt, n, moduli):
    """(c0, c1) = (m - (a s + e), a), NTT form, with e transformed on its own as the one-at-a-time
    path does"""
    a = expand_seed(seed, n, moduli)
    e_ntt = O.ntt_fwd(C.sample_cbd(key, nonce, moduli, n), n, moduli)
    return sub(m_ntt, add(mul(a, s_ntt, n, moduli), e_ntt, n, moduli), n, moduli), a
