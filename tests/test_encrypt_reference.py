"""The CPU yardstick of the batched encryption tests (tests/encrypt_ref.py), checked against itself
at N = 2^10 with the oracle and numpy alone: a ciphertext decrypts to m - e exactly, and subtracting
the error in coefficient form before the one forward NTT gives the same residues as transforming m
and e separately, the identity the device's fused rounding rests on."""
import numpy as np

import chacha_np as C
import encrypt_ref as E
import oracle_lib as O

N = 1 << 10
KEY = [0x01234567 * (i + 1) & 0xFFFFFFFF for i in range(8)]
SEED = bytes((11 * i + 5) & 0xFF for i in range(64))
NONCE = ((5 << 40) | 3) + 1


def setup():
    mods = O.coeff_modulus_create(N, [60, 40, 40])
    rng = np.random.default_rng(77)
    m = rng.integers(-(1 << 45), 1 << 45, size=N)
    s_ntt = O.ntt_fwd(C.sample_ternary(KEY, 0, mods, N), N, mods)
    return mods, m, s_ntt


def test_error_is_small_and_centred():
    e = E.cbd_signed(KEY, NONCE, N)
    assert e.min() >= -21 and e.max() <= 21 and e.min() < 0 < e.max()
    mods = O.coeff_modulus_create(N, [60, 40])
    assert np.array_equal(E.residues(e, mods), C.sample_cbd(KEY, NONCE, mods, N))


def test_ciphertext_decrypts_to_m_minus_e():
    mods, m, s_ntt = setup()
    c0, c1 = E.encrypt(O.ntt_fwd(E.residues(m, mods), N, mods), SEED, KEY, NONCE, s_ntt, N, mods)
    assert np.array_equal(c1, E.expand_seed(SEED, N, mods))
    dec = O.ntt_inv(E.add(c0, E.mul(c1, s_ntt, N, mods), N, mods), N, mods)
    assert np.array_equal(dec, E.residues(m - E.cbd_signed(KEY, NONCE, N), mods))


def test_subtracting_the_error_before_the_ntt_is_exact():
    mods, m, s_ntt = setup()
    c0, c1 = E.encrypt(O.ntt_fwd(E.residues(m, mods), N, mods), SEED, KEY, NONCE, s_ntt, N, mods)
    fused = O.ntt_fwd(E.residues(m - E.cbd_signed(KEY, NONCE, N), mods), N, mods)
    assert np.array_equal(E.sub(fused, E.mul(c1, s_ntt, N, mods), N, mods), c0)
