"""Numpy restatement of the many-digit form of the lvl0 -> lvl2 rotation, written from its definition alone.  It shares
the polynomial arithmetic of tests/cb_rotate_ref.py (mul_xr, external_product, linear, digits) and no code with the library.

l = the number of constants mu[0 .. l), 1 <= l <= 4; bw = the smallest integer with 2^bw >= l; s = 20 + bw.  Job on the n + 1 u32 words
w of a lvl0 TLWE, with the torus-domain key bk u64 [n][(k+1) l2][k+1][N2]:
    lin = sign * w + (0, .., 0, off)  (mod 2^32)
    abar_i = (((lin_i + 2^(s-1)) mod 2^32) >> s) << bw;  bbar = (lin_n >> s) << bw         (multiples of 2^bw in [0, 2 N2))
    tv[c] = mu[c mod 2^bw] if (c mod 2^bw) < l else 0, c < N2
    acc = X^(2 N2 - bbar) * (0, tv);  for i < n: acc += bk_i [.] ((X^abar_i - 1) acc)
    out[r] = SampleExtractIndex(acc, r) + (0, .., 0, mu[r]),  r < l
    SampleExtractIndex(acc, r): a_i = acc_a[r - i] for i <= r, a_i = -acc_a[N2 + r - i] for i > r, b = acc_b[r]
"""
import numpy as np

from cb_rotate_ref import L2, M64, N2, external_product, linear, mul_xr


def bw_of(l):
    if not 1 <= l <= 4:
        raise ValueError("l outside [1, 4]")
    return (l - 1).bit_length()


def modswitch(lin, bw):
    """(abar [n], bbar): the a words rounded, the b word truncated, all multiples of 2^bw in [0, 2 N2)"""
    s = 20 + bw
    abar = (((lin[:-1] + (1 << (s - 1))) & 0xFFFFFFFF) >> s) << bw
    return abar, (int(lin[-1]) >> s) << bw


def test_vector(mu, bw):
    tv = np.zeros(N2, dtype=np.uint64)
    for c in range(N2):
        if c % (1 << bw) < len(mu):
            tv[c] = int(mu[c % (1 << bw)]) & M64
    return tv


def extract(acc, r, mu_r):
    """SampleExtractIndex(acc, r) + (0, .., 0, mu_r) of acc u64 [2][N2] -> u64 [N2 + 1]"""
    out = np.zeros(N2 + 1, dtype=np.uint64)
    for i in range(N2):
        out[i] = int(acc[0, r - i]) if i <= r else (-int(acc[0, N2 + r - i])) & M64
    out[N2] = (int(acc[1, r]) + int(mu_r)) & M64
    return out


def accumulator(w, sign, off, mu, bk):
    """the accumulator u64 [2][N2] after the n steps"""
    bw = bw_of(len(mu))
    bk = np.asarray(bk, dtype=np.uint64).reshape(-1, 2 * L2, 2, N2)
    abar, bbar = modswitch(linear(w, sign, off), bw)
    assert bk.shape[0] == abar.size
    tv = np.zeros((2, N2), dtype=np.uint64)
    tv[1] = test_vector(mu, bw)
    acc = mul_xr(tv, (2 * N2 - bbar) % (2 * N2))
    for i in range(abar.size):
        acc = acc + external_product(bk[i], mul_xr(acc, int(abar[i])) - acc)
    return acc


def rotate_job(w, sign, off, mu, bk):
    """-> u64 [l][N2 + 1]"""
    acc = accumulator(w, sign, off, mu, bk)
    return np.stack([extract(acc, r, mu[r]) for r in range(len(mu))])
