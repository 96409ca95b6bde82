"""Numpy restatement of the lvl0 -> lvl2 blind rotation of circuit bootstrapping (N2 = 2048, k = 1, 64-bit torus), written from the
definition alone: schoolbook negacyclic products with u64 wrap-around, the gadget digits, the mod switch and the sample extraction.
It shares no code with the library; every GPU / emulation result is compared with it word for word.

Job on the n + 1 u32 words w of a lvl0 TLWE, with the torus-domain key bk u64 [n][(k+1) l2][k+1][N2]:
    lin = sign * w + (0, .., 0, off)  (mod 2^32);  abar_i = (lin_i + 2^19) >> 20  (mod 2^32 first);  bbar = lin_n >> 20
    acc = X^(2 N2 - bbar) * (0, mu (1 + X + .. + X^(N2-1)));  for i < n: acc += bk_i [.] ((X^abar_i - 1) acc)
    out = SampleExtractIndex(acc, 0), mu added to b
"""
import numpy as np

N2 = 2048
L2, BGBIT2 = 4, 9
M64 = (1 << 64) - 1


def mu_of(r, bgbit1):
    """the test-vector constant of gadget digit r of the lvl1 set: the rotation gives 2 mu = 2^(64 - (r+1) Bgbit1) for a positive phase"""
    return 1 << (63 - (r + 1) * bgbit1)


def linear(w, sign, off):
    lin = (np.asarray(w, dtype=np.uint32).astype(np.int64) * int(sign)) & 0xFFFFFFFF
    lin[-1] = (lin[-1] + int(off)) & 0xFFFFFFFF
    return lin


def modswitch(lin):
    """(abar [n], bbar), both in [0, 2 N2)"""
    abar = ((lin[:-1] + (1 << 19)) & 0xFFFFFFFF) >> 20
    return abar, int(lin[-1]) >> 20


def digits(x, l2=L2, bgbit=BGBIT2):
    """signed digits int64 [l2, ...] of u64 words, most significant first"""
    x = np.asarray(x, dtype=np.uint64)
    bg = 1 << bgbit
    offset = sum((bg // 2) << (64 - j * bgbit) for j in range(1, l2 + 1))
    rnd = 1 << (64 - l2 * bgbit - 1)
    t = x + np.uint64((offset + rnd) & M64)
    return np.stack([((t >> np.uint64(64 - j * bgbit)) & np.uint64(bg - 1)).astype(np.int64) - bg // 2 for j in range(1, l2 + 1)])


def word_of_digits(d, l2=L2, bgbit=BGBIT2, low=0):
    """the word whose digits are d (each in [-Bg/2, Bg/2)), plus `low` below the rounding bit"""
    return (sum(int(v) << (64 - (j + 1) * bgbit) for j, v in enumerate(d)) + int(low)) & M64


def mul_xr(p, r):
    """X^r * p in Z[X] / (X^N + 1), 0 <= r < 2N, u64 wrap-around"""
    n = p.shape[-1]
    ext = np.concatenate([p, np.uint64(0) - p], axis=-1)
    idx = (np.arange(n) - int(r)) % (2 * n)
    return ext[..., idx]


def negacyclic_product(d, q):
    """d * q in Z[X] / (X^N + 1) mod 2^64: the schoolbook convolution (np.convolve on u64 wraps), folded; d signed, q u64"""
    n = d.shape[0]
    c = np.convolve(d.astype(np.int64).view(np.uint64), q)   # 2N - 1 words
    out = c[:n].copy()
    out[: n - 1] -= c[n:]
    return out


def external_product(trgsw, diff):
    """trgsw u64 [(k+1) l2][k+1][N] [.] diff u64 [k+1][N] -> u64 [k+1][N]: row h l2 + j multiplies digit j of polynomial h"""
    n = diff.shape[-1]
    out = np.zeros((2, n), dtype=np.uint64)
    for h in range(2):
        dg = digits(diff[h])
        for j in range(L2):
            if not dg[j].any():
                continue
            for c in range(2):
                out[c] += negacyclic_product(dg[j], trgsw[h * L2 + j, c])
    return out


def rotate_job(w, sign, off, mu, bk):
    """-> u64 [N2 + 1]"""
    bk = np.asarray(bk, dtype=np.uint64).reshape(-1, 2 * L2, 2, N2)
    lin = linear(w, sign, off)
    abar, bbar = modswitch(lin)
    assert bk.shape[0] == abar.size
    tv = np.zeros((2, N2), dtype=np.uint64)
    tv[1] = np.uint64(int(mu) & M64)
    acc = mul_xr(tv, (2 * N2 - bbar) % (2 * N2))
    for i in range(abar.size):
        diff = mul_xr(acc, int(abar[i])) - acc
        acc = acc + external_product(bk[i], diff)
    out = np.zeros(N2 + 1, dtype=np.uint64)
    out[0] = acc[0, 0]
    out[1:N2] = np.uint64(0) - acc[0, :0:-1]
    out[N2:] = acc[1, :1] + np.array([int(mu) & M64], dtype=np.uint64)
    return out


def dft_direct(x, root, P):
    """sum_j x[j] root^(j k) mod P for every k < len(x): python integers"""
    n = len(x)
    pw = [pow(root, e, P) for e in range(n)]
    order_pw = lambda e: pw[e % n] if pow(root, n, P) == 1 else pow(root, e, P)
    return [sum(int(x[j]) * order_pw(j * k) for j in range(n)) % P for k in range(n)]
