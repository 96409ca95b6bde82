"""Cases of the lvl0 -> lvl2 rotation shared by the CPU (emulation) and the GPU tests: chosen keys and lvl0 words, their expected lvl2
TLWEs from the numpy restatement (computed once per process), and the ctypes face of the emulation."""
import ctypes
import functools
import os

import numpy as np

import cb_rotate_ref as ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
N2, L2, BGBIT2 = ref.N2, ref.L2, ref.BGBIT2
_u64p, _u32p, _i32p = ctypes.POINTER(ctypes.c_uint64), ctypes.POINTER(ctypes.c_uint32), ctypes.POINTER(ctypes.c_int32)


@functools.lru_cache(maxsize=None)
def emul():
    L = ctypes.CDLL(os.path.join(ROOT, "iyokan_amd", "lib", "libiyk_emul.so"))
    L.iyk_emul_ntt64.argtypes = [_u64p, ctypes.c_int, _u64p]
    L.iyk_emul_ntt64.restype = None
    L.iyk_emul_cb_ntt.argtypes = [_u64p, ctypes.c_int, _u64p, _u64p]
    L.iyk_emul_cb_ntt.restype = None
    L.iyk_emul_cb_digits.argtypes = [_u64p, ctypes.c_int, ctypes.c_uint32, ctypes.c_uint32, _i32p]
    L.iyk_emul_bk2_ntt.argtypes = [ctypes.c_uint64, _u64p, _u64p]
    L.iyk_emul_bk2_ntt.restype = None
    L.iyk_emul_cb_rotate.argtypes = [ctypes.c_uint32] * 3 + [_u32p, ctypes.c_int32, ctypes.c_uint32, ctypes.c_uint64, _u64p, _u64p]
    return L


def key_ntt(bk):
    """the device form u64 [n][2][8][2][N2] of a torus-domain key, by the emulation of bk2_ntt_kernel"""
    bk = np.ascontiguousarray(bk, dtype=np.uint64).reshape(-1, 2 * L2, 2, N2)
    out = np.zeros((bk.shape[0], 2, 2 * L2, 2, N2), dtype=np.uint64)
    emul().iyk_emul_bk2_ntt(bk.shape[0], bk.ctypes.data_as(_u64p), out.ctypes.data_as(_u64p))
    return out


def emul_rotate(w, sign, off, mu, ntt, l2=L2, bgbit2=BGBIT2):
    w = np.ascontiguousarray(w, dtype=np.uint32)
    out = np.zeros(N2 + 1, dtype=np.uint64)
    rc = emul().iyk_emul_cb_rotate(w.size - 1, l2, bgbit2, w.ctypes.data_as(_u32p), int(sign), int(off) & 0xFFFFFFFF, int(mu) & ref.M64,
                                   ntt.ctypes.data_as(_u64p), out.ctypes.data_as(_u64p))
    if rc != 0:
        raise ValueError(f"iyk_emul_cb_rotate refused its arguments ({rc})")
    return out


def _uniform_key(n, seed):
    return np.random.default_rng(seed).integers(0, 1 << 64, size=(n, 2 * L2, 2, N2), dtype=np.uint64)


def _u32(rng, size):
    return rng.integers(0, 1 << 32, size=size, dtype=np.uint64).astype(np.uint32)


# words whose digits sit at the edges, as (wanted digits, word).  Built from the digits; `carry` has every digit at Bg/2 - 1 and the
# rounding bit set below them, so the rounding carry runs through all four digits and out of the word.
def digit_edge_words():
    bg = 1 << BGBIT2
    lo, hi = -bg // 2, bg // 2 - 1
    words = {"all-min": ([lo] * L2, ref.word_of_digits([lo] * L2)), "all-max": ([hi] * L2, ref.word_of_digits([hi] * L2))}
    for j in range(L2):
        for v in (lo, hi, 1):
            d = [0] * L2
            d[j] = v
            words[f"digit{j}={v}"] = (d, ref.word_of_digits(d))
    words["below-round"] = ([0] * L2, ref.word_of_digits([0] * L2, low=(1 << (64 - L2 * BGBIT2 - 1)) - 1))
    words["at-round"] = ([0, 0, 0, 1], ref.word_of_digits([0] * L2, low=1 << (64 - L2 * BGBIT2 - 1)))
    words["carry"] = ([lo] * L2, ref.word_of_digits([hi] * L2, low=1 << (64 - L2 * BGBIT2 - 1)))   # hi + 1 wraps to lo at every digit
    return words


def _mu_for_difference(word):
    """with abar = N2 (X^N2 = -1) and no rotation of the test vector every coefficient of the first step's difference is -2 mu"""
    assert word % 2 == 0
    return ((-word) & ref.M64) >> 1


@functools.lru_cache(maxsize=None)
def case(name):
    """-> (bk u64 [n][8][2][N2], jobs [(w u32 [n+1], sign, off, mu)])"""
    rng = np.random.default_rng(sum(map(ord, name)))
    if name.startswith("uniform-n"):
        n = int(name[len("uniform-n"):])
        jobs = [(_u32(rng, n + 1), 1, 0, int(rng.integers(0, 1 << 63))), (_u32(rng, n + 1), -1, 0x12345678, int(rng.integers(0, 1 << 63))),
                (_u32(rng, n + 1), 1, 0xFEDCBA98, ref.mu_of(0, 6))]
        return _uniform_key(n, 100 + n), jobs
    if name == "abar-bbar":
        abars = [0, 1, 2047, 2048, 4095]
        jobs = []
        for bbar, low in ((0, 0), (1, (1 << 20) - 1), (2048, 0), (4095, (1 << 20) - 1)):   # b is truncated: the low bits change nothing
            w = np.array([a << 20 for a in abars] + [(bbar << 20) | low], dtype=np.uint32)
            jobs.append((w, 1, 0, int(rng.integers(0, 1 << 63))))
        return _uniform_key(5, 200), jobs
    if name == "threshold":
        # a is rounded: (7 << 20) + 2^19 - 1 -> 7, + 2^19 -> 8; 0xFFF7FFFF -> 4095, 0xFFF80000 -> wraps to 0
        ws = [[(7 << 20) + (1 << 19) - 1, (7 << 20) + (1 << 19), 3 << 20], [0xFFF7FFFF, 0xFFF80000, 0xFFFFFFFF]]
        return _uniform_key(2, 300), [(np.array(w, dtype=np.uint32), s, 0, int(rng.integers(0, 1 << 63))) for w in ws for s in (1, -1)]
    if name == "digit-edges":
        w = np.array([N2 << 20, 0], dtype=np.uint32)
        return _uniform_key(1, 400), [(w, 1, 0, _mu_for_difference(word)) for _, word in digit_edge_words().values() if word % 2 == 0]
    if name.startswith("extreme-"):
        # the exactness bound at its extreme: every key word all ones (both halves 2^32 - 1) or 2^63, every digit of the first step's b
        # polynomial -Bg/2; the second step runs on whatever the first left
        word = {"extreme-ones": 0xFFFFFFFFFFFFFFFF, "extreme-msb": 0x8000000000000000}[name]
        bk = np.full((2, 2 * L2, 2, N2), word, dtype=np.uint64)
        w = np.array([N2 << 20, int(rng.integers(0, 1 << 32)), 0], dtype=np.uint32)
        return bk, [(w, 1, 0, _mu_for_difference(digit_edge_words()["all-min"][1]))]
    raise KeyError(name)


CASES = ["uniform-n1", "uniform-n2", "uniform-n5", "abar-bbar", "threshold", "digit-edges", "extreme-ones", "extreme-msb"]


@functools.lru_cache(maxsize=None)
def expected(name):
    """u64 [jobs][N2 + 1] from the restatement"""
    bk, jobs = case(name)
    return np.stack([ref.rotate_job(w, s, off, mu, bk) for w, s, off, mu in jobs])


# ---- a real key at a small n: the lvl1 sets' mu_r, both bit values, both signs ------------------------------------------------------
REAL_N, ALPHA2 = 8, 2.0 ** -44


class SmallKeys:
    """what client.bk2_rows reads of a KeySet, at a lvl0 dimension of the test's choosing"""

    def __init__(self, n, seed):
        self.s0 = np.random.default_rng(seed).integers(0, 2, size=n).astype(np.uint32)


@functools.lru_cache(maxsize=None)
def real_case(n=REAL_N, seed=5):
    from iyokan_amd import client

    ks = SmallKeys(n, seed)
    s2 = client.keygen_lvl2(N2, seed=seed + 1)
    bk = client.bk2_rows(ks, s2, L2, BGBIT2, ALPHA2, seed=seed + 2)
    return ks, s2, bk


def encrypt_lvl0(s0, bits, mu0=1 << 29, seed=0, noise_bits=18):
    """lvl0 TLWEs of +-mu0 under s0 with a small uniform noise: u32 [len(bits)][n + 1]"""
    rng = np.random.default_rng(seed)
    n = s0.size
    ct = np.zeros((len(bits), n + 1), dtype=np.uint32)
    ct[:, :n] = _u32(rng, (len(bits), n))
    msg = np.where(np.asarray(bits) == 1, mu0, (1 << 32) - mu0).astype(np.uint64)
    noise = rng.integers(-(1 << noise_bits), 1 << noise_bits, size=len(bits)).astype(np.int64).astype(np.uint64)
    ct[:, n] = ((ct[:, :n].astype(np.uint64) * s0.astype(np.uint64)).sum(axis=1) + msg + noise).astype(np.uint32)
    return ct
