"""CPU yardstick of public-key CKKS encryption, from the oracle (oracle/oracle.c) and numpy alone: the
sequential algorithm of PhantomPublicKey::encrypt_asymmetric restated limb by limb, and the two
shortcuts the device's batched path takes (division by P over the kept rows only; the message folded
into e0).  Test infrastructure only; tests/test_encrypt_asym_reference.py pins it, the GPU tests
compare the device's batched encryption with it.

Polynomials are flat uint64 arrays [limbs][n]; `mods` is the key chain (size_Q data primes, then alpha
special primes); a ciphertext at L limbs keeps rows 0 .. L-1."""
import numpy as np

import chacha_np as C
import encrypt_ref as E
import oracle_lib as O


def kept_rows(L, size_Q, size_QP):
    """rows {0 .. L-1} u {size_Q .. size_QP-1} of the key chain"""
    return list(range(L)) + list(range(size_Q, size_QP))


def gather(x, n, rows):
    return np.ascontiguousarray(x.reshape(-1, n)[rows]).reshape(-1)


def public_key(a, s_ntt, key, nonce, n, mods):
    """(-(a s + e), a) over the whole chain, NTT form; a uniform (NTT form), e of draw `nonce`"""
    e = O.ntt_fwd(C.sample_cbd(key, nonce, mods, n), n, mods)
    zero = np.zeros(len(mods) * n, dtype=np.uint64)
    return E.sub(zero, E.add(E.mul(a, s_ntt, n, mods), e, n, mods), n, mods), a


def small_ntt(key, nonces, n, mods):
    """NTT(u), NTT(e0), NTT(e1) over `mods` from the three draws"""
    return (O.ntt_fwd(C.sample_ternary(key, nonces[0], mods, n), n, mods),
            O.ntt_fwd(C.sample_cbd(key, nonces[1], mods, n), n, mods),
            O.ntt_fwd(C.sample_cbd(key, nonces[2], mods, n), n, mods))


def moddown(x, n, ql, p):
    """or_moddown_from_ntt of x [len(ql) + len(p)][n] -> [len(ql)][n]"""
    out = np.zeros(len(ql) * n, dtype=np.uint64)
    O.lib().or_moddown_from_ntt(O.P(np.ascontiguousarray(x.copy())), O.P(out), n, O.P(O.arr(ql)), len(ql),
                                O.P(O.arr(p)), len(p))
    return out


def pre_division(pk, key, nonces, n, mods):
    """(pk0 u + e0, pk1 u + e1) over every limb of `mods`, NTT form"""
    u, e0, e1 = small_ntt(key, nonces, n, mods)
    return (E.add(E.mul(u, pk[0], n, mods), e0, n, mods), E.add(E.mul(u, pk[1], n, mods), e1, n, mods))


def encrypt_sequential(m_ntt, pk, key, nonces, n, mods, alpha, L):
    """encrypt_asymmetric as it runs: everything over the whole chain, the division at chain index 1,
    the leading L limbs kept, then + m (m_ntt [L][n])"""
    size_Q = len(mods) - alpha
    x0, x1 = pre_division(pk, key, nonces, n, mods)
    c0 = moddown(x0, n, mods[:size_Q], mods[size_Q:])[:L * n]
    c1 = moddown(x1, n, mods[:size_Q], mods[size_Q:])[:L * n]
    return E.add(c0, m_ntt, n, mods[:L]), c1


def encrypt_kept_rows(m_ntt, pk, key, nonces, n, mods, alpha, L):
    """identity 1: only the kept rows are formed and the division runs at the target level"""
    size_Q = len(mods) - alpha
    rows = kept_rows(L, size_Q, len(mods))
    sub = [mods[r] for r in rows]
    x0, x1 = pre_division([gather(pk[0], n, rows), gather(pk[1], n, rows)], key, nonces, n, sub)
    return E.add(moddown(x0, n, sub[:L], sub[L:]), m_ntt, n, mods[:L]), moddown(x1, n, sub[:L], sub[L:])


def encrypt_folded(m, pk, key, nonces, n, mods, alpha, L):
    """identities 1 and 2, as the device computes: m (signed integers, the rounded coefficients) enters
    as P m on the data rows of e0's coefficients; no plaintext transform and no final add"""
    size_Q = len(mods) - alpha
    rows = kept_rows(L, size_Q, len(mods))
    sub = [mods[r] for r in rows]
    bigP = 1
    for p in mods[size_Q:]:
        bigP *= p
    e0 = E.cbd_signed(key, nonces[1], n)
    lifted = [[(int(e) + (bigP * int(v) if i < L else 0)) % q for e, v in zip(e0, m)] for i, q in enumerate(sub)]
    x0 = O.ntt_fwd(np.array(lifted, dtype=np.uint64).reshape(-1), n, sub)
    u = O.ntt_fwd(C.sample_ternary(key, nonces[0], sub, n), n, sub)
    e1 = O.ntt_fwd(C.sample_cbd(key, nonces[2], sub, n), n, sub)
    x0 = E.add(E.mul(u, gather(pk[0], n, rows), n, sub), x0, n, sub)
    x1 = E.add(E.mul(u, gather(pk[1], n, rows), n, sub), e1, n, sub)
    return moddown(x0, n, sub[:L], sub[L:]), moddown(x1, n, sub[:L], sub[L:])


def centred(x, q):
    """residues [n] of one limb as signed integers in (-q/2, q/2]"""
    v = x.astype(object)
    return np.array([int(t) - q if int(t) > q // 2 else int(t) for t in v], dtype=object)
