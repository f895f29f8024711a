"""The channel packing's host-side pieces (no GPU): the C-ABI names, phantom_pack_rotations against
the formulas, and a numpy model over exact negacyclic integer polynomials modulo a prime of what
packing and the rotation tree compute.

A channel of ns slots is a polynomial in X^G, G = N / (2 ns).  packed = sum_c X^(c D) m_c with
D = G / P, plus full-ring junk (an encryption's noise is full-ring).  Level t of the tree applies the
automorphism X -> X^e, e = 5^(P ns / 2^(t+1)) mod 2N, to every node a and forms a + a(X^e) and
(a - a(X^e)) X^(2N - D 2^t).  On the subring positions (multiples of D) node c must end as P m_c
exactly, and a node at or above C as zero there.  The junk of the model lies outside the subring of X^D\n(the bootstrap's partial sum projects onto it; what an encryption's noise leaves inside it stays noise).

Shapes (N, ns, P, C): (64,4,4,4), (64,4,8,8), (64,2,16,16) full packing, (128,8,4,3), (256,16,8,5),
(64,4,2,2), (64,4,1,1).  ns = (width 2^slotstr)^2 is a square, so phantom_pack_rotations(width,
slotstr, ..) cannot be asked for ns = 2 or 8: those two shapes run on the formulas alone, and
(128,4,16,16) (full packing) and (256,4,4,3) (C < P) stand in for them at the C-ABI."""
import ctypes
import re

import numpy as np
import pytest

import phantom_amd as PA

NAMES = ["phantom_pack_rotations", "phantom_ct_pack", "phantom_ct_split"]
SHAPES = [(64, 4, 4, 4), (64, 4, 8, 8), (64, 2, 16, 16), (128, 8, 4, 3), (256, 16, 8, 5), (64, 4, 2, 2), (64, 4, 1, 1)]
ABI_SHAPES = [s for s in SHAPES if s[1] in (4, 16)] + [(128, 4, 16, 16), (256, 4, 4, 3)]
Q = (1 << 31) - 1  # products stay below 2^62


def formulas(N, ns, P):
    g = P.bit_length() - 1
    D = N // (2 * P * ns)
    rots = [P * ns >> (t + 1) for t in range(g)]
    return rots, [pow(5, r, 2 * N) for r in rots], [D << t for t in range(g)]


def width_slotstr(ns):
    lg = int(round(ns ** 0.5))
    assert lg * lg == ns
    return (lg, 0) if lg < 4 else (lg // 2, 1)  # ns = 16 as width 2, slotstr 1


def abi(width, slotstr, pack, log_n, capacity=8):
    rot = np.zeros(capacity, dtype=np.int32)
    elt = np.zeros(capacity, dtype=np.uint32)
    pw = np.zeros(capacity, dtype=np.uint32)
    cnt = PA.sz(99)
    st = PA.load().phantom_pack_rotations(width, slotstr, pack, log_n, rot.ctypes.data, elt.ctypes.data, pw.ctypes.data,
                                          capacity, ctypes.byref(cnt))
    return st, cnt.value, rot, elt, pw


@pytest.mark.parametrize("name", NAMES)
def test_symbols_declared_and_exported(name):
    assert name in PA.declared_symbols()
    fn = getattr(PA.load(), name)  # AttributeError if the library does not export it
    txt = re.sub(r"/\*.*?\*/", "", open(PA.HEADER_PATH).read(), flags=re.S)
    params = re.search(r"\b%s\s*\(([^)]*)\)" % name, txt).group(1)
    assert fn.restype is ctypes.c_int and len(fn.argtypes) == len(params.split(",")), params


@pytest.mark.parametrize("N,ns,P,C", ABI_SHAPES, ids=str)
def test_rotations(N, ns, P, C):
    width, slotstr = width_slotstr(ns)
    st, cnt, rot, elt, pw = abi(width, slotstr, P, N.bit_length() - 1)
    rots, elts, powers = formulas(N, ns, P)
    assert st == 0 and cnt == len(rots) == P.bit_length() - 1
    assert rot[:cnt].tolist() == rots == [P * ns // 2 ** (t + 1) for t in range(cnt)]
    assert sorted(rots) == [ns << i for i in range(cnt)]
    assert elt[:cnt].tolist() == elts and pw[:cnt].tolist() == powers
    assert not rot[cnt:].any() and not elt[cnt:].any() and not pw[cnt:].any()


def test_rotations_refused():
    log_n = 12  # width 8: ns = 64, capacity min(4096 / 128, 64) = 32
    assert abi(8, 0, 32, log_n)[0] == 0
    for width, slotstr, pack in [(8, 0, 3), (8, 0, 0), (8, 0, 64), (8, 1, 16), (0, 0, 1), (6, 0, 2), (64, 0, 2), (8, 40, 1)]:
        st, cnt, rot, elt, pw = abi(width, slotstr, pack, log_n)
        assert st == 1 and not rot.any() and not elt.any() and not pw.any(), (width, slotstr, pack)
    assert abi(32, 0, 64, 17)[0] == 0 and abi(16, 0, 128, 17)[0] == 1  # never above 64
    assert abi(8, 0, 4, 0)[0] == 1 and abi(8, 0, 4, 21)[0] == 1
    st, cnt, rot, elt, pw = abi(8, 0, 8, log_n, capacity=2)  # the count is reported, nothing is written
    assert (st, cnt) == (1, 3) and not rot.any()
    lib = PA.load()
    assert lib.phantom_pack_rotations(8, 0, 4, log_n, None, None, None, 8, None) == 1
    cnt = PA.sz(0)
    assert lib.phantom_pack_rotations(8, 0, 4, log_n, None, None, None, 8, ctypes.byref(cnt)) == 0 and cnt.value == 2


def shift(a, k, N):
    """a X^k in Z_Q[X] / (X^N + 1)"""
    k %= 2 * N
    out = np.zeros_like(a)
    idx = (np.arange(N) + k) % (2 * N)
    out[idx % N] = np.where(idx >= N, (Q - a) % Q, a)
    return out


def automorphism(a, e, N):
    """a(X^e)"""
    out = np.zeros_like(a)
    idx = (np.arange(N) * e) % (2 * N)
    out[idx % N] = np.where(idx >= N, (Q - a) % Q, a)
    return out


@pytest.mark.parametrize("N,ns,P,C", SHAPES, ids=str)
def test_tree_recovers_every_channel(N, ns, P, C):
    rng = np.random.default_rng([N, ns, P, C])
    if (N, ns, P, C) in ABI_SHAPES:  # driven by what the library returns
        st, cnt, rot, elt, pw = abi(*width_slotstr(ns), P, N.bit_length() - 1)
        assert st == 0
        elts, powers = elt[:cnt].tolist(), pw[:cnt].tolist()
        assert (elts, powers) == formulas(N, ns, P)[1:]
    else:
        _, elts, powers = formulas(N, ns, P)
    G, D = N // (2 * ns), N // (2 * P * ns)
    on_g, on_d = np.arange(N) % G == 0, np.arange(N) % D == 0
    chans = []
    for c in range(C):  # the message on the multiples of G, junk everywhere outside the subring of X^D
        m = rng.integers(0, Q, size=N, dtype=np.int64)
        m[on_d & ~on_g] = 0
        chans.append(m)
    packed = np.zeros(N, dtype=np.int64)
    for c, m in enumerate(chans):
        packed = (packed + shift(m, c * D, N)) % Q
    assert D == 1 or packed[~on_d].any()  # the junk is there

    def tree(limit):
        """nodes of the tree; a child at or above `limit` is not computed"""
        nodes = {0: packed}
        for t, (e, pw_t) in enumerate(zip(elts, powers)):
            for idx in [i for i in sorted(nodes) if i < 1 << t]:
                a = nodes[idx]
                r = automorphism(a, e, N)
                child = idx | 1 << t
                if child < limit:
                    nodes[child] = shift((a - r) % Q, 2 * N - pw_t, N)
                nodes[idx] = (a + r) % Q
        return nodes

    pruned, full = tree(C), tree(P)
    assert sorted(pruned) == list(range(C)) and sorted(full) == list(range(P))
    for c, m in enumerate(chans):
        want = np.where(on_g, P * m % Q, 0)[on_d]
        assert want.any() and np.array_equal(pruned[c][on_d], want), c
        assert np.array_equal(full[c], pruned[c]), c  # pruning changes no computed node
    for c in range(C, P):  # an unused node is exactly zero on the subring
        assert not full[c][on_d].any(), c


@pytest.mark.parametrize("N,ns,P,C", [(128, 8, 4, 3), (256, 16, 8, 5), (64, 4, 4, 1), (64, 4, 8, 7)], ids=str)
def test_group_that_is_not_full_leaves_index_zero_free(N, ns, P, C):
    """host/pack.h deals a group of C < P channels to the tree indices 1 .. C.  Coefficient 0 and the
    middle coefficient N / 2 of the packed polynomial (where a bootstrap's slot-0 offset lands) belong
    to index 0: an offset there changes node 0 alone, and every channel still comes back as P m_c."""
    rng = np.random.default_rng([N, ns, P, C, 1])
    _, elts, powers = formulas(N, ns, P)
    G, D = N // (2 * ns), N // (2 * P * ns)
    on_g, on_d = np.arange(N) % G == 0, np.arange(N) % D == 0
    chans = [np.where(on_g, rng.integers(0, Q, size=N, dtype=np.int64), 0) for _ in range(C)]
    packed = np.zeros(N, dtype=np.int64)
    for c, m in enumerate(chans):
        packed = (packed + shift(m, (1 + c) * D, N)) % Q
    offset = packed.copy()
    offset[0] = (offset[0] + 12345) % Q
    offset[N // 2] = (offset[N // 2] + 54321) % Q

    def tree(root):
        nodes = {0: root}
        for t, (e, pw_t) in enumerate(zip(elts, powers)):
            for idx in range(1 << t):
                a, r = nodes[idx], automorphism(nodes[idx], e, N)
                nodes[idx | 1 << t] = shift((a - r) % Q, 2 * N - pw_t, N)
                nodes[idx] = (a + r) % Q
        return nodes

    clean, shifted = tree(packed), tree(offset)
    for c, m in enumerate(chans):
        assert m.any() and np.array_equal(clean[1 + c], P * m % Q), c
    for idx in [0] + list(range(1 + C, P)):
        assert not clean[idx].any(), idx
    for idx in range(1, P):
        assert np.array_equal(shifted[idx], clean[idx]), idx
    assert shifted[0][0] == P * 12345 % Q and shifted[0][N // 2] == P * 54321 % Q
