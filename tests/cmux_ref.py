"""Exact reference of the CMUX jobs (test support for test_cmux_emulation / test_cmux_plan / test_gpu_cmux): numpy differences,
tests/numpy_tfhe.decompose digits and the oracle's exact negacyclic products on the TORUS-domain TRGSW — never the code under test."""
import copy
import ctypes
import os

import numpy as np

import numpy_tfhe as nt
import oracle_lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
_u32p = ctypes.POINTER(ctypes.c_uint32)
_i32p = ctypes.POINTER(ctypes.c_int32)
M32 = 0xFFFFFFFF


def _neg(fn, d, w):
    d = np.ascontiguousarray(d, dtype=np.int32)
    w = np.ascontiguousarray(w, dtype=np.uint32)
    res = np.zeros(d.size, dtype=np.uint32)
    fn.argtypes = [ctypes.c_uint32, _i32p, _u32p, _u32p]
    fn.restype = None
    fn(d.size, d.ctypes.data_as(_i32p), w.ctypes.data_as(_u32p), res.ctypes.data_as(_u32p))
    return res


def negacyclic_ntt(d, w):
    return _neg(oracle_lib.lib().orc_negacyclic_ntt, d, w)


def negacyclic_schoolbook(d, w):
    return _neg(oracle_lib.lib().orc_negacyclic_schoolbook, d, w)


def difference(p, T, job):
    """D of a job (sel, in0, in1, rot, out): [k+1][N] uint32."""
    _, in0, in1, rot, _ = job
    N = p.N
    a0 = T[in0].reshape(2, N)
    if in1 >= 0:
        return (T[in1].reshape(2, N) - a0).astype(np.uint32)
    return np.stack([((nt.mul_by_xai(a0[c].astype(np.uint64), rot, N) - a0[c]) & M32).astype(np.uint32) for c in range(2)])


def cmux(p, T, trgsw, job, product=negacyclic_ntt):
    """out = in0 + sum_r digits_r(D) (*) TRGSW[sel][r][c'] mod 2^32; trgsw: u32 [slots][(k+1) l][k+1][N] torus.  Returns the 2N words."""
    sel, in0 = job[0], job[1]
    N = p.N
    D = difference(p, T, job)
    digits = np.concatenate([nt.decompose(D[c], p.l, p.Bgbit) for c in range(2)])   # row c l + j
    out = T[in0].reshape(2, N).copy()
    for r in range(2 * p.l):
        for c in range(2):
            out[c] += product(digits[r], trgsw[sel][r][c])
    return out.reshape(2 * N)


def run_jobs(p, T, trgsw, jobs):
    """The jobs one after the other, in place on T (rows of 2N words)."""
    for job in jobs:
        T[job[4]] = cmux(p, T, trgsw, job)
    return T


def sample_extract_index(row, h, N):
    """numpy restatement of SampleExtractIndex: a'[j] = a[h - j] (j <= h), -a[N + h - j] (j > h), b' = b[h]."""
    a, b = row[:N], row[N:]
    j = np.arange(N)
    ap = np.where(j <= h, a[(h - j) % N], (0 - a[(N + h - j) % N].astype(np.int64)) & M32).astype(np.uint32)
    return np.concatenate([ap, b[h : h + 1]]).astype(np.uint32)


def rom_read(p, data, trgsw, addr_width, log2_word_bits):
    """One ROM read through iyokan_amd.cmux.rom_read_plan with the exact CMUX: the result row (bit i of the word at coefficient i)."""
    from iyokan_amd import cmux as plan

    lay = plan.rom_layout(addr_width, log2_word_bits, p.N)
    T = np.concatenate([data, np.zeros((lay.scratch_rows, 2 * p.N), dtype=np.uint32)])
    for jobs in plan.rom_read_plan(addr_width, log2_word_bits, p.N):
        run_jobs(p, T, trgsw, [(j.bit, j.in0, j.in1, j.rot, j.out) for j in jobs])
    return T[lay.result]


def emul():
    em = ctypes.CDLL(os.path.join(ROOT, "iyokan_amd", "lib", "libiyk_emul.so"))
    em.emu_cmux_fft.argtypes = [ctypes.c_int, _u32p, ctypes.c_uint64, ctypes.POINTER(ctypes.c_double), ctypes.c_uint64, _i32p,
                                ctypes.c_uint64]
    em.emu_sample_extract_index.argtypes = [_u32p, ctypes.c_int, _u32p]
    return em


def spectra(em, p, trgsw):
    """The selector store's device layout for torus-domain TRGSWs [slots][(k+1) l][k+1][N], through the existing emulation of
    bk_fft_kernel: a key of `slots` steps is exactly a store of `slots` selectors."""
    trgsw = np.ascontiguousarray(trgsw, dtype=np.uint32)
    q = copy.copy(p)
    q.n = trgsw.shape[0]
    assert trgsw.size == q.bk_words
    out = np.zeros(2 * trgsw.size, dtype=np.float64)
    assert em.iyk_emul_bk_fft(ctypes.byref(q), trgsw.ctypes.data_as(_u32p), out.ctypes.data_as(ctypes.POINTER(ctypes.c_double))) == 0
    return out


def emu_run(em, p, T, spec, slots, jobs):
    T = np.ascontiguousarray(T, dtype=np.uint32).copy()
    jobs = np.ascontiguousarray(jobs, dtype=np.int32).reshape(-1, 5)
    rc = em.emu_cmux_fft(0 if p.l == 3 else 1, T.ctypes.data_as(_u32p), T.shape[0], spec.ctypes.data_as(ctypes.POINTER(ctypes.c_double)),
                         slots, jobs.ctypes.data_as(_i32p), jobs.shape[0])
    assert rc == 0
    return T


def worst_case_trgsw(p, word):
    return np.full((p.trgsw_rows, p.k + 1, p.N), word, dtype=np.uint32)


def extreme_pair(p, rng, top):
    """TRLWE rows (x, y) with every gadget digit of y - x at its extreme: +Bg/2 - 1 (top) or -Bg/2."""
    Bg = 1 << p.Bgbit
    d = (Bg // 2 - 1) if top else -(Bg // 2)
    D = sum(d << (32 - j * p.Bgbit) for j in range(1, p.l + 1)) & M32
    x = rng.integers(0, 1 << 32, size=2 * p.N, dtype=np.uint64).astype(np.uint32)
    y = (x + np.uint32(D)).astype(np.uint32)
    assert np.all(nt.decompose(y - x, p.l, p.Bgbit) == d)
    return x, y
