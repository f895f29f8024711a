"""The CPU yardstick of the batched public-key encryption tests (tests/encrypt_asym_ref.py), pinned with
the oracle and numpy alone at N = 2^10, CoeffModulus [60, 40, 40, 40 | 60, 60] (two special primes), at
L = 4, 2 and 1 limbs:

  * identity 1: the division by P is per limb, so forming only rows {0..L-1} u {size_Q..} and dividing
    at the target level gives the bits of "divide at chain index 1, keep the leading L limbs";
  * identity 2: P m added to the data rows of e0's coefficients comes out of the division as + m;
  * decryption: c0 + c1 s - m, centred, stays within alpha (n + 1) + 1 in every coefficient.  Before the
    division the noise e0 + e1 s - e u is far below P and vanishes; each of the two divisions through
    the fast base conversion leaves a remainder term below 1 and an overflow in [0, alpha - 1], and the
    c1 term is multiplied by the ternary s: at most n (alpha - 1 + 1) + alpha + 1 <= alpha (n + 1) + 1.
"""
import numpy as np
import pytest

import chacha_np as C
import encrypt_asym_ref as A
import encrypt_ref as E
import oracle_lib as O

N = 1 << 10
ALPHA = 2
KEY = [0x01234567 * (i + 1) & 0xFFFFFFFF for i in range(8)]
NONCES = [((5 << 40) | 3) + i for i in range(3)]

_state = {}


def setup():
    if not _state:
        mods = O.coeff_modulus_create(N, [60, 40, 40, 40, 60, 60])
        rng = np.random.default_rng(78)
        s_ntt = O.ntt_fwd(C.sample_ternary(KEY, 0, mods, N), N, mods)
        pk = A.public_key(O.random_limbs(rng, N, mods), s_ntt, KEY, 1, N, mods)
        m = rng.integers(-(1 << 45), 1 << 45, size=N)
        _state.update(mods=mods, s_ntt=s_ntt, pk=pk, m=m)
    return _state["mods"], _state["s_ntt"], _state["pk"], _state["m"]


def m_ntt(m, mods, L):
    return O.ntt_fwd(E.residues(m, mods[:L]), N, mods[:L])


@pytest.mark.parametrize("L", [4, 2, 1])
def test_division_over_the_kept_rows_equals_divide_then_drop(L):
    mods, _, pk, m = setup()
    want = A.encrypt_sequential(m_ntt(m, mods, L), pk, KEY, NONCES, N, mods, ALPHA, L)
    got = A.encrypt_kept_rows(m_ntt(m, mods, L), pk, KEY, NONCES, N, mods, ALPHA, L)
    assert np.array_equal(got[0], want[0]) and np.array_equal(got[1], want[1])


@pytest.mark.parametrize("L", [4, 2, 1])
def test_message_folded_into_e0_equals_the_final_add(L):
    mods, _, pk, m = setup()
    want = A.encrypt_sequential(m_ntt(m, mods, L), pk, KEY, NONCES, N, mods, ALPHA, L)
    got = A.encrypt_folded(m, pk, KEY, NONCES, N, mods, ALPHA, L)
    assert np.array_equal(got[0], want[0]) and np.array_equal(got[1], want[1])


@pytest.mark.parametrize("L", [4, 2, 1])
def test_ciphertext_decrypts_to_the_message_within_the_derived_bound(L):
    mods, s_ntt, pk, m = setup()
    ql = mods[:L]
    c0, c1 = A.encrypt_sequential(m_ntt(m, mods, L), pk, KEY, NONCES, N, mods, ALPHA, L)
    dec = O.ntt_inv(E.add(c0, E.mul(c1, s_ntt[:L * N], N, ql), N, ql), N, ql)
    noise = E.sub(dec, E.residues(m, ql), N, ql).reshape(L, N)
    first = A.centred(noise[0], ql[0])
    worst = max(abs(int(v)) for v in first)
    print(f"L = {L}: worst |c0 + c1 s - m| = {worst}, bound {ALPHA * (N + 1) + 1}")
    assert 0 < worst <= ALPHA * (N + 1) + 1
    for i in range(1, L):  # one small integer, the same in every limb
        assert np.array_equal(A.centred(noise[i], ql[i]), first), i
