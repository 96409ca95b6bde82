"""Cases of the FP64 FFT form of the lvl0 -> lvl2 rotation (csrc/cb_rotate_fft.hpp) shared by the CPU (emulation) and the GPU tests:
cb_rotate_cases' own cases and expected() (the u64 schoolbook restatement, tests/cb_rotate_ref.py), the cases the split of a key word
into four signed 16-bit quarters needs, and the ctypes face of the emulation.

The quarters of a word are taken with carries moving upward, so 0x8000800080008000 splits into (-2^15, -32767, -32767, -32767): the
carry out of each -2^15 raises the next quarter by one.  `quarters-min` keeps that word; `quarters-all-min` is the word whose four
quarters really are -2^15, 0x7FFF7FFF7FFF8000, the norm bound's extreme; `quarters-alt` alternates the SIGN OF EVERY QUARTER from
coefficient to coefficient: even coefficients hold 0x7FFF7FFF7FFF8000 (all four quarters -2^15), odd ones 0x7FFF7FFF7FFF7FFF (all
four quarters +32767, the largest positive quarter), so the transforms' inputs alternate between -32768 and +32767."""
import ctypes
import functools

import numpy as np

import cb_rotate_cases as base
import cb_rotate_ref as ref

N2, L2, BGBIT2 = ref.N2, ref.L2, ref.BGBIT2
QUARTERS, POINTS = 4, N2 // 2
_u64p, _u32p, _i32p = ctypes.POINTER(ctypes.c_uint64), ctypes.POINTER(ctypes.c_uint32), ctypes.POINTER(ctypes.c_int32)
_f64p = ctypes.POINTER(ctypes.c_double)

# the PROVEN bound on |z - rint(z)| of every rounded sum, for any key and any digits
PROVEN_BOUND = 2.0 ** -3.8

WORD_MIN = 0x8000800080008000
WORD_ALL_MIN = 0x7FFF7FFF7FFF8000
WORD_ALL_MAX = 0x7FFF7FFF7FFF7FFF           # every quarter +32767: no carry anywhere
CARRY_WORDS = [0x7FFF800080008000, 0xFFFFFFFFFFFF8000, 0x0000FFFF80007FFF, 0x8000000000008000, 0x7FFF7FFF7FFF7FFF, 0xFFFF7FFFFFFF8000]


@functools.lru_cache(maxsize=None)
def emul():
    L = base.emul()
    L.iyk_emul_fft1024.argtypes = [_f64p, ctypes.c_int, _f64p]
    L.iyk_emul_fft1024.restype = None
    L.iyk_emul_cb_key_quarters.argtypes = [_u64p, ctypes.c_int, _i32p]
    L.iyk_emul_cb_key_quarters.restype = None
    L.iyk_emul_cb_recombine.argtypes = [_f64p, ctypes.c_int, _u64p]
    L.iyk_emul_cb_recombine.restype = None
    L.iyk_emul_bk2_fft.argtypes = [ctypes.c_uint64, _u64p, _f64p]
    L.iyk_emul_bk2_fft.restype = None
    L.iyk_emul_cb_rotate_fft.argtypes = [ctypes.c_uint32] * 3 + [_u32p, ctypes.c_int32, ctypes.c_uint32, ctypes.c_uint64, _f64p, _u64p]
    L.iyk_emul_cb_fft_round_error.argtypes = [ctypes.c_int]
    L.iyk_emul_cb_fft_round_error.restype = ctypes.c_double
    L.iyk_emul_cb_fft_grid.argtypes = [ctypes.c_int64, ctypes.c_int]
    L.iyk_emul_bk2_form_known.argtypes = [ctypes.c_int]
    return L


def key_fft(bk):
    """the device form double [n][4 quarters][8][2][1024][2] of a torus-domain key, by the emulation of bk2_fft_kernel"""
    bk = np.ascontiguousarray(bk, dtype=np.uint64).reshape(-1, 2 * L2, 2, N2)
    out = np.zeros((bk.shape[0], QUARTERS, 2 * L2, 2, POINTS, 2), dtype=np.float64)
    emul().iyk_emul_bk2_fft(bk.shape[0], bk.ctypes.data_as(_u64p), out.ctypes.data_as(_f64p))
    return out


def emul_rotate_fft(w, sign, off, mu, fftkey, l2=L2, bgbit2=BGBIT2):
    w = np.ascontiguousarray(w, dtype=np.uint32)
    out = np.zeros(N2 + 1, dtype=np.uint64)
    rc = emul().iyk_emul_cb_rotate_fft(w.size - 1, l2, bgbit2, w.ctypes.data_as(_u32p), int(sign), int(off) & 0xFFFFFFFF, int(mu) & ref.M64,
                                       fftkey.ctypes.data_as(_f64p), out.ctypes.data_as(_u64p))
    if rc != 0:
        raise ValueError(f"iyk_emul_cb_rotate_fft refused its arguments ({rc})")
    return out


def round_error(reset=True):
    return float(emul().iyk_emul_cb_fft_round_error(1 if reset else 0))


def _min_digit_jobs(rng):
    """the first step's digits of the b polynomial are all -Bg/2 (cb_rotate_cases' extreme cases); the second step runs on what the first
    left; then a job of uniform words with sign = -1 and an offset"""
    w = np.array([N2 << 20, int(rng.integers(0, 1 << 32)), 0], dtype=np.uint32)
    return [(w, 1, 0, base._mu_for_difference(base.digit_edge_words()["all-min"][1])),
            (base._u32(rng, 3), -1, 0x9E3779B9, int(rng.integers(0, 1 << 63)))]


@functools.lru_cache(maxsize=None)
def case(name):
    """-> (bk u64 [n][8][2][N2], jobs [(w u32 [n+1], sign, off, mu)])"""
    if name in base.CASES:
        return base.case(name)
    rng = np.random.default_rng(sum(map(ord, name)))
    if name in ("quarters-min", "quarters-all-min"):
        return np.full((2, 2 * L2, 2, N2), {"quarters-min": WORD_MIN, "quarters-all-min": WORD_ALL_MIN}[name], dtype=np.uint64), _min_digit_jobs(rng)
    if name == "quarters-alt":
        bk = np.full((2, 2 * L2, 2, N2), WORD_ALL_MIN, dtype=np.uint64)
        bk[..., 1::2] = WORD_ALL_MAX
        return bk, _min_digit_jobs(rng)
    if name == "carry-chain":
        words = np.array(CARRY_WORDS, dtype=np.uint64)
        bk = words[rng.integers(0, len(words), size=(2, 2 * L2, 2, N2))]
        bk[..., :len(words)] = words                     # each of them in every polynomial, whatever the draw
        return bk, _min_digit_jobs(rng)
    raise KeyError(name)


SPLIT_CASES = ["quarters-min", "quarters-all-min", "quarters-alt", "carry-chain"]
CASES = list(base.CASES) + SPLIT_CASES


@functools.lru_cache(maxsize=None)
def expected(name):
    """u64 [jobs][N2 + 1] from the restatement"""
    if name in base.CASES:
        return base.expected(name)
    bk, jobs = case(name)
    return np.stack([ref.rotate_job(w, s, off, mu, bk) for w, s, off, mu in jobs])
