"""Cases of the many-digit form of the lvl0 -> lvl2 rotation shared by the CPU test (tests/test_cb_many_cases.py) and the
GPU test (tests/test_gpu_cb_many.py), each under the three kernel forms of tests/cb_rotate_edge_cases.py (wg / lat / fft).  Expected
words come from the numpy restatement tests/cb_many_ref.py, computed once per process:

    l1-is-per-digit  n = 19, l = 1: the words of the per-digit restatement (cb_rotate_ref.rotate_job)
    grid-n19         n = 19, uniform key, l = 3 (the mu_r of the 128-bit set) and l = 2 (of the 80-bit set): eight jobs on a 7-slot arena —
                     both signs, three offs, inputs at slot 0, a middle slot and the last slot; the middle row holds words at the
                     rounding edges of the coarser mod switch, and its four jobs put bbar at 0, N2 - 2^bw, N2 and 2 N2 - 2^bw
    extract          cb_epilogue alone on an accumulator of distinct words, r = 0 .. 3
    real-n19         a real small key: every one of the l outputs of the restatement decrypts to 2 mu_r or 0 within decrypt_bound
    row-pass         n = 256, 257, 512, 513 (GPU, against the emulation): the last lane of a pass of 256 / 512 lanes and the first of the next
"""
import ctypes
import functools

import numpy as np

import cb_many_ref as many
import cb_rotate_cases as cases
import cb_rotate_edge_cases as edge
import cb_rotate_ref as ref

N2, L2, BGBIT2 = ref.N2, ref.L2, ref.BGBIT2
FORMS = edge.FORMS
FORM_INDEX = {"wg": 0, "lat": 1, "fft": 2}
_u64p, _u32p, _i32p = ctypes.POINTER(ctypes.c_uint64), ctypes.POINTER(ctypes.c_uint32), ctypes.POINTER(ctypes.c_int32)
MUS = {3: [ref.mu_of(r, 6) for r in range(3)], 2: [ref.mu_of(r, 10) for r in range(2)], 1: [ref.mu_of(1, 6)],
       4: [ref.mu_of(r, 5) for r in range(4)]}


@functools.lru_cache(maxsize=None)
def emul(path=None):
    """libiyk_emul.so, or another build of it at `path` (the mutants of DESIGN.md 6d), with the many-digit entry points declared"""
    L = edge.emul(path)
    L.iyk_emul_cb_rotate_many.argtypes = [ctypes.c_int] + [ctypes.c_uint32] * 3 + [_u32p, ctypes.c_int32, ctypes.c_uint32, ctypes.c_uint32, _u64p,
                                                                                 ctypes.c_void_p, _u64p]
    L.iyk_emul_cb_many_extract.argtypes = [_u64p, ctypes.c_int, ctypes.c_uint32, _u64p, _u64p]
    return L


def rotate(form, w, sign, off, mu, key, lib=None):
    """one many-digit job through the emulation of `form` -> u64 [l][N2 + 1]; key: n = len(w) - 1 steps of a device key of the form"""
    w = np.ascontiguousarray(w, dtype=np.uint32)
    mu = np.array([int(m) & ref.M64 for m in mu], dtype=np.uint64)
    assert key.shape[0] == w.size - 1 and key.flags.c_contiguous
    out = np.zeros((len(mu), N2 + 1), dtype=np.uint64)
    rc = (lib or emul()).iyk_emul_cb_rotate_many(FORM_INDEX[form], w.size - 1, L2, BGBIT2, w.ctypes.data_as(_u32p), int(sign), int(off) & 0xFFFFFFFF,
                                                 len(mu), mu.ctypes.data_as(_u64p), key.ctypes.data, out.ctypes.data_as(_u64p))
    if rc != 0:
        raise ValueError(f"iyk_emul_cb_rotate_many refused its arguments ({rc})")
    return out


def rotate_jobs(form, arena, jobs, mu, key, lib=None):
    """u64 [jobs][l][N2 + 1] of jobs (in, sign, off) on one arena"""
    return np.stack(edge._pool(lambda j: rotate(form, arena[j[0]], j[1], j[2], mu, key, lib), jobs))


def extract(acc, lanes, mu, lib=None):
    acc = np.ascontiguousarray(acc, dtype=np.uint64)
    mu = np.array(mu, dtype=np.uint64)
    out = np.zeros((len(mu), N2 + 1), dtype=np.uint64)
    assert (lib or emul()).iyk_emul_cb_many_extract(acc.ctypes.data_as(_u64p), lanes, len(mu), mu.ctypes.data_as(_u64p), out.ctypes.data_as(_u64p)) == 0
    return out


# ---- grid-n19, l1-is-per-digit ---------------------------------------------------------------------------------------------------------
GRID_N, GRID_SLOTS = edge.MID_N, edge.MID_SLOTS
grid_key = edge.mid_key   # the uniform key of mid-n19: KEYS["mid"], device_key("mid", form)


@functools.lru_cache(maxsize=None)
def grid_case(l):
    """-> (arena u32 [7][20], eight jobs (in, sign, off), mu [l])"""
    bw = many.bw_of(l)
    s = 20 + bw
    arena = cases._u32(np.random.default_rng(1910 + l), (GRID_SLOTS, GRID_N + 1))
    mid = GRID_SLOTS // 2
    # abar 0 against 2^bw, the round-up that wraps to 0, and a word the per-digit shift rounds to an odd abar; b = 0: off alone sets bbar
    arena[mid, :4] = [(1 << (s - 1)) - 1, 1 << (s - 1), (1 << 32) - (1 << (s - 1)), (4 << 20) + (1 << 19)]
    arena[mid, GRID_N] = 0
    low = (1 << s) - 1   # b is truncated: the bits below 2^s change nothing
    jobs = [(mid, 1, low), (mid, 1, (N2 - (1 << bw)) << 20), (mid, 1, N2 << 20), (mid, 1, ((2 * N2 - (1 << bw)) << 20) | low),
            (0, 1, 0), (0, -1, 0x9E3779B9), (GRID_SLOTS - 1, 1, 0xFFF80000), (GRID_SLOTS - 1, -1, 0)]
    return arena, jobs, MUS[l]


def grid_bbars(l):
    """bbar of the four jobs on the middle row"""
    arena, jobs, _ = grid_case(l)
    return [many.modswitch(ref.linear(arena[i], sg, off), many.bw_of(l))[1] for i, sg, off in jobs[:4]]


@functools.lru_cache(maxsize=None)
def grid_expected(l):
    """u64 [8][l][N2 + 1] from the restatement"""
    arena, jobs, mu = grid_case(l)
    return np.stack(edge._pool(lambda j: many.rotate_job(arena[j[0]], j[1], j[2], mu, grid_key()), jobs))


@functools.lru_cache(maxsize=None)
def l1_case():
    """-> (arena, three jobs (in, sign, off), mu [1])"""
    arena, jobs, _ = grid_case(3)
    return arena, [jobs[0], jobs[5], jobs[6]], MUS[1]


@functools.lru_cache(maxsize=None)
def l1_expected():
    """u64 [3][1][N2 + 1] from the PER-DIGIT restatement"""
    arena, jobs, mu = l1_case()
    return np.stack(edge._pool(lambda j: ref.rotate_job(arena[j[0]], j[1], j[2], mu[0], grid_key())[None], jobs))


# ---- extract ---------------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def extract_case():
    """-> (acc u64 [2][N2] of distinct words, mu [4] of distinct words)"""
    acc = (np.arange(2 * N2, dtype=np.uint64) * np.uint64(0x9E3779B97F4A7C15) + np.uint64(0x0123456789ABCDEF)).reshape(2, N2)
    assert np.unique(acc).size == 2 * N2
    return acc, [0x1111111111111111, 0x2222222222222222, 0x4444444444444444, 0x8888888888888888]


# ---- real-n19 --------------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def real_case():
    """-> (s2, bk, ct u32 [2][20] (bit 1, bit 0), jobs (in, sign, off, bit)): a real key of 19 steps (alpha2 = 2^-44)"""
    ks, s2, bk = cases.real_case(GRID_N, 19)
    ct = cases.encrypt_lvl0(ks.s0, [1, 0], seed=191)
    return s2, bk, ct, [(i, sign, 0, bit) for i, bit in ((0, 1), (1, 0)) for sign in (1, -1)]


@functools.lru_cache(maxsize=None)
def real_expected(l):
    """u64 [4][l][N2 + 1] from the restatement"""
    _, bk, ct, jobs = real_case()
    return np.stack(edge._pool(lambda j: many.rotate_job(ct[j[0]], j[1], j[2], MUS[l], bk), jobs))


def real_errors(l, words):
    """the signed distance of every output's phase from (bit if sign == +1 else 1 - bit) * 2 mu_r: python integers [job][r]"""
    from iyokan_amd import client

    s2, _, _, jobs = real_case()
    errs = []
    for (_, sign, _, bit), w in zip(jobs, words):
        ph = client.tlwe2_phases(s2, np.ascontiguousarray(w))
        errs.append([(int(ph[r]) - (bit if sign == 1 else 1 - bit) * 2 * MUS[l][r] + (1 << 63)) % (1 << 64) - (1 << 63) for r in range(l)])
    return errs


# ---- row-pass --------------------------------------------------------------------------------------------------------------------------
ROW_NS = (256, 257, 512, 513)


@functools.lru_cache(maxsize=None)
def row_expected(form, n, l):
    """u64 [1][l][N2 + 1] of edge.row_case(n)'s second job (the last slot, sign -1, an off) from the emulation of `form`"""
    arena, jobs = edge.row_case(n)
    i, sign, off, _ = jobs[1]
    return rotate(form, arena[i], sign, off, MUS[l], edge.device_key("row", form)[:n])[None]


# ---- argument checks: csrc/batch_args.hpp through libiyk_emul.so ------------------------------------------------------------------------
def _check_out():
    msg = ctypes.create_string_buffer(256)
    words = np.zeros(4096, dtype=np.uint32)
    counts = np.zeros(8, dtype=np.uint64)
    return msg, words, counts, (msg, ctypes.c_uint64(256), words.ctypes.data_as(_u32p), ctypes.c_uint64(words.size), counts.ctypes.data_as(_u64p))


def rotate_many_args(tlwe0_slots, tlwe2_slots, count, in_, sign, off, l, mu, out):
    """-> (code, text, words u32, counts) of args::cb_rotate_many_args; the arrays may be shorter than count (an over-cap set)"""
    L = emul()
    a = lambda v, t: np.ascontiguousarray(v, dtype=t)
    in_, sign, out, off, mu = a(in_, np.int32), a(sign, np.int32), a(out, np.int32), a(off, np.uint32), a(mu, np.uint64)
    msg, words, counts, tail = _check_out()
    L.iyk_emul_cb_rotate_many_args.argtypes = [ctypes.c_uint64] * 3 + [_i32p, _i32p, _u32p, ctypes.c_uint32, _u64p, _i32p, ctypes.c_char_p,
                                                                      ctypes.c_uint64, _u32p, ctypes.c_uint64, _u64p]
    code = L.iyk_emul_cb_rotate_many_args(tlwe0_slots, tlwe2_slots, count, in_.ctypes.data_as(_i32p), sign.ctypes.data_as(_i32p),
                                          off.ctypes.data_as(_u32p), l, mu.ctypes.data_as(_u64p), out.ctypes.data_as(_i32p), *tail)
    return code, msg.value.decode(), words, counts


def circuit_bootstrap_many_args(p, bk2_n, privks_n_in, tlwe0_slots, in_, sign, tlwe2_n_in, tlwe2_slots, tlwe2_first, trlwe_slots, trgsw_slots,
                                trgsw_first, bits):
    """-> (code, text, words, counts) of args::circuit_bootstrap_many_args; p: an iyk_params (iyokan_amd.hip)"""
    L = emul()
    in_, sign = np.ascontiguousarray(in_, dtype=np.int32), np.ascontiguousarray(sign, dtype=np.int32)
    msg, words, counts, tail = _check_out()
    u64, u32 = ctypes.c_uint64, ctypes.c_uint32
    L.iyk_emul_circuit_bootstrap_many_args.argtypes = [ctypes.c_void_p, u32, u32, u64, _i32p, _i32p, u32, u64, u64, u64, u64, u64, u64,
                                                       ctypes.c_char_p, u64, _u32p, u64, _u64p]
    code = L.iyk_emul_circuit_bootstrap_many_args(ctypes.addressof(p), bk2_n, privks_n_in, tlwe0_slots, in_.ctypes.data_as(_i32p),
                                                  sign.ctypes.data_as(_i32p), tlwe2_n_in, tlwe2_slots, tlwe2_first, trlwe_slots, trgsw_slots,
                                                  trgsw_first, bits, *tail)
    return code, msg.value.decode(), words, counts
