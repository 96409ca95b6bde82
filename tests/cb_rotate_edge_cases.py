"""Edge cases of the lvl0 -> lvl2 rotation shared by the CPU test (tests/test_cb_rotate_edge_cases.py) and the GPU test
(tests/test_gpu_cb_rotate_edges.py), each run under the three forms: `wg` (cb_rotate_kernel), `lat` (cb_rotate_lat_kernel) and `fft`
(cb_rotate_fft_kernel, a key of form="fft").  A case is an arena of lvl0 TLWEs u32 [slots][n + 1], jobs (in, sign, off, mu) that
address it by slot, and the expected u64 [N2 + 1] words of every job, computed once per process:

    mid-n19     n = 19, six jobs on a 7-slot arena, expected words from the numpy restatement (tests/cb_rotate_ref.py)
    row-pass    n = 255, 256, 257, 511, 512, 513 (the b word on the last lane of a full pass of 256 / 512 lanes and on the first lane of
                the next), prefixes of one uniform key; expected words from the emulation of the form under test
    rounds-n19  CUs + 3 jobs that cycle over mid-n19's six: three workgroups run a second job behind a first
    full-size   n = 636 / 500, a real key (client.bk2_rows), the l rotations of a 1 bit and of a 0 bit under both signs; expected words
                from the emulation, and the decryption of every off = 0 job inside decrypt_bound(n)

The emulation runs one job per call on the n + 1 words it is handed, so a job's row is sliced here (`row`): the kernels' own
`tlwe0 + in * (n + 1)` is what the GPU test adds to that.  `emul(path)` loads another build of the emulation (the mutants of DESIGN.md
§6d were run through it)."""
import ctypes
import functools
import math
from concurrent.futures import ThreadPoolExecutor

import numpy as np

import cb_rotate_cases as cases
import cb_rotate_fft_cases as fft_cases
import cb_rotate_ref as ref
from iyokan_amd import client

N2, L2, BGBIT2 = ref.N2, ref.L2, ref.BGBIT2
FORMS = ("wg", "lat", "fft")
KEY_FORM = {"wg": "ntt", "lat": "ntt", "fft": "fft"}          # the Bk2Key form each kernel form rotates under
ENTRY = {"wg": "iyk_emul_cb_rotate", "lat": "iyk_emul_cb_rotate_lat", "fft": "iyk_emul_cb_rotate_fft"}
_u64p, _u32p, _f64p = ctypes.POINTER(ctypes.c_uint64), ctypes.POINTER(ctypes.c_uint32), ctypes.POINTER(ctypes.c_double)


@functools.lru_cache(maxsize=None)
def emul(path=None):
    """libiyk_emul.so, or another build of it at `path`, with the entry points of the three forms declared"""
    L = ctypes.CDLL(path) if path else cases.emul()
    job = [ctypes.c_uint32] * 3 + [_u32p, ctypes.c_int32, ctypes.c_uint32, ctypes.c_uint64]
    L.iyk_emul_cb_rotate.argtypes = job + [_u64p, _u64p]
    L.iyk_emul_cb_rotate_lat.argtypes = job + [_u64p, _u64p]
    L.iyk_emul_cb_rotate_fft.argtypes = job + [_f64p, _u64p]
    L.iyk_emul_bk2_ntt.argtypes = [ctypes.c_uint64, _u64p, _u64p]
    L.iyk_emul_bk2_ntt.restype = None
    L.iyk_emul_bk2_fft.argtypes = [ctypes.c_uint64, _u64p, _f64p]
    L.iyk_emul_bk2_fft.restype = None
    return L


def _pool(fn, items):
    """fn over items on at most client.MAX_THREADS threads: the emulation's calls release the interpreter lock"""
    items = list(items)
    with ThreadPoolExecutor(max_workers=max(1, min(client._threads(), len(items)))) as ex:
        return list(ex.map(fn, items))


@functools.lru_cache(maxsize=None)
def _device_key(name, key_form):
    """the device form of the torus-domain key KEYS[name]() by the emulation of bk2_ntt_kernel / bk2_fft_kernel, 16 steps per call"""
    bk = KEYS[name]()
    n = bk.shape[0]
    if key_form == "ntt":
        out = np.zeros((n, 2, 2 * L2, 2, N2), dtype=np.uint64)
        fn, ptr = emul().iyk_emul_bk2_ntt, _u64p
    else:
        out = np.zeros((n, fft_cases.QUARTERS, 2 * L2, 2, fft_cases.POINTS, 2), dtype=np.float64)
        fn, ptr = emul().iyk_emul_bk2_fft, _f64p
    _pool(lambda a: fn(min(16, n - a), bk[a:a + 16].ctypes.data_as(_u64p), out[a:a + 16].ctypes.data_as(ptr)), range(0, n, 16))
    return out


def device_key(name, form):
    return _device_key(name, KEY_FORM[form])


def rotate(form, w, sign, off, mu, key, lib=None):
    """one job through the emulation of `form`; key: the first n = len(w) - 1 steps of a device key of KEY_FORM[form]"""
    w = np.ascontiguousarray(w, dtype=np.uint32)
    assert key.shape[0] == w.size - 1 and key.flags.c_contiguous
    out = np.zeros(N2 + 1, dtype=np.uint64)
    fn = getattr(lib or emul(), ENTRY[form])
    rc = fn(w.size - 1, L2, BGBIT2, w.ctypes.data_as(_u32p), int(sign), int(off) & 0xFFFFFFFF, int(mu) & ref.M64,
            key.ctypes.data_as(_f64p if form == "fft" else _u64p), out.ctypes.data_as(_u64p))
    if rc != 0:
        raise ValueError(f"{ENTRY[form]} refused its arguments ({rc})")
    return out


def row(arena, slot, stride=None):
    """the n + 1 words of slot `slot`; stride: the words between two rows, n + 1 unless a mutant says otherwise"""
    width = arena.shape[1]
    at = slot * (width if stride is None else stride)
    return arena.ravel()[at:at + width]


def rotate_jobs(form, arena, jobs, key, lib=None, stride=None):
    """u64 [jobs][N2 + 1] of jobs (in, sign, off, mu) on one arena and key, through the emulation of `form`"""
    return np.stack(_pool(lambda j: rotate(form, row(arena, j[0], stride), j[1], j[2], j[3], key, lib), jobs))


def out_slots(count, slots, seed):
    """a permutation of output slots with slot 0 and the last slot among them"""
    perm = np.random.default_rng(seed).permutation(slots)[:count].tolist()
    if 0 not in perm:
        perm[0] = 0
    if slots - 1 not in perm:
        perm[-1] = slots - 1
    assert len(set(perm)) == count
    return perm


# ---- mid-n19, rounds-n19 ----------------------------------------------------------------------------------------------------------------
MID_N, MID_SLOTS = 19, 7


@functools.lru_cache(maxsize=None)
def mid_key():
    return cases._uniform_key(MID_N, 1900)


@functools.lru_cache(maxsize=None)
def mid_case():
    """-> (arena u32 [7][20], six jobs (in, sign, off, mu)): both signs, off in {0, 0x9E3779B9, 0xFFF80000}, the mu_r of both parameter
    sets and one uniform 63-bit mu, inputs at slot 0, a middle slot and the last slot"""
    rng = np.random.default_rng(1901)
    arena = cases._u32(rng, (MID_SLOTS, MID_N + 1))
    mus = [ref.mu_of(r, 6) for r in range(3)] + [ref.mu_of(r, 10) for r in range(2)] + [int(rng.integers(0, 1 << 63))]
    ins, offs = (0, 3, MID_SLOTS - 1), (0, 0x9E3779B9, 0xFFF80000)
    # g -> in g % 3, sign by g % 2, off (g // 2) % 3: every input under both signs, every off under both signs
    jobs = [(ins[g % 3], 1 if g % 2 == 0 else -1, offs[(g // 2) % 3], mus[g]) for g in range(6)]
    return arena, jobs


@functools.lru_cache(maxsize=None)
def mid_expected():
    """u64 [6][N2 + 1] from the restatement: about 0.6 s per job"""
    arena, jobs = mid_case()
    return np.stack([ref.rotate_job(arena[i], s, off, mu, mid_key()) for i, s, off, mu in jobs])


def rounds_case(cus):
    """-> (arena, jobs (in, sign, off, mu, out), slots, index of each job's tuple in mid_case): CUs + 3 jobs in one batch"""
    arena, six = mid_case()
    count = cus + 3
    slots = count + 2
    out = out_slots(count, slots, seed=cus)
    return arena, [six[g % 6] + (out[g],) for g in range(count)], slots, [g % 6 for g in range(count)]


# ---- row-pass ---------------------------------------------------------------------------------------------------------------------------
ROW_NS = (255, 256, 257, 511, 512, 513)
ROW_SLOTS = 3


@functools.lru_cache(maxsize=None)
def row_key():
    """one uniform key of 513 steps; the key of every n is its first n steps"""
    return cases._uniform_key(max(ROW_NS), 5130)


@functools.lru_cache(maxsize=None)
def row_case(n):
    """-> (arena u32 [3][n + 1] of uniform words, two jobs (in, sign, off, mu)): slot 0 with sign +1, the last slot with sign -1 and an off"""
    rng = np.random.default_rng(5131 + n)
    arena = cases._u32(rng, (ROW_SLOTS, n + 1))
    return arena, [(0, 1, 0, ref.mu_of(2, 6)), (ROW_SLOTS - 1, -1, 0x9E3779B9, int(rng.integers(0, 1 << 63)))]


@functools.lru_cache(maxsize=None)
def row_expected(form):
    """{n: u64 [2][N2 + 1]} from the emulation of `form`, all twelve jobs at once"""
    key = device_key("row", form)
    items = [(n, g) for n in ROW_NS for g in range(2)]

    def one(item):
        n, g = item
        arena, jobs = row_case(n)
        i, s, off, mu = jobs[g]
        return rotate(form, row(arena, i), s, off, mu, key[:n])

    got = _pool(one, items)
    return {n: np.stack([got[items.index((n, g))] for g in range(2)]) for n in ROW_NS}


# ---- full-size --------------------------------------------------------------------------------------------------------------------------
FULL_SLOTS = 3
_FULL = {}


def full_case(name, keys):
    """keys: the KeySet of parameter set `name` ("128" / "80").  -> (s2, bk, arena u32 [3][n + 1], jobs (in, sign, off, mu), bits): a
    real key, the encryption of 1 at slot 0 and of 0 at the last slot (uniform words between them); for each bit and each sign the l
    rotations mu_r with off = 0, then one job with an off.  bits[g]: the bit job g rotates."""
    if name not in _FULL:
        p = keys.params
        s2 = client.keygen_lvl2(N2, seed=631)
        bk = client.bk2_rows(keys, s2, L2, BGBIT2, cases.ALPHA2, seed=632)
        ct = client.encrypt_bits(keys, [1, 0], seed=633)
        arena = cases._u32(np.random.default_rng(634), (FULL_SLOTS, p.n + 1))
        arena[0], arena[FULL_SLOTS - 1] = ct[0], ct[1]
        jobs, bits = [], []
        for bit, slot in ((1, 0), (0, FULL_SLOTS - 1)):
            for sign in (1, -1):
                for r in range(int(p.l)):
                    jobs.append((slot, sign, 0, ref.mu_of(r, int(p.Bgbit))))
                    bits.append(bit)
        jobs.append((FULL_SLOTS - 1, -1, 0x9E3779B9, ref.mu_of(0, int(p.Bgbit))))
        bits.append(0)
        _FULL[name] = (s2, bk, arena, jobs, bits)
        KEYS["full" + name] = lambda: _FULL[name][1]
    return _FULL[name]


@functools.lru_cache(maxsize=None)
def full_expected(name, form, which=None):
    """u64 [jobs][N2 + 1] from the emulation of `form` (full_case(name, keys) first); which: a tuple of job indexes, all by default"""
    _, _, arena, jobs, _ = _FULL[name]
    return rotate_jobs(form, arena, jobs if which is None else [jobs[g] for g in which], device_key("full" + name, form))


def phase_errors(s2, words, jobs, bits):
    """the signed distance of every job's phase from (bit if sign == +1 else 1 - bit) * 2 mu, as python integers"""
    ph = client.tlwe2_phases(s2, words)
    errs = []
    for p_, (_, sign, _, mu), bit in zip(ph, jobs, bits):
        want = (bit if sign == 1 else 1 - bit) * 2 * mu
        errs.append((int(p_) - want + (1 << 63)) % (1 << 64) - (1 << 63))
    return errs


def decrypt_bound(n):
    """The bound on |phase - message| of a rotation's output under a real key of n steps, in units of 2^-64, at 6.5 sigma.

    The output's phase is that of the accumulator's coefficient 0 (sample extraction and `+ mu` are exact), and the accumulator's
    message after n steps is exactly +-mu: the lvl0 noise and the mod switch move the rotation amount, not the amplitude, so as long
    as the lvl0 TLWE decrypts (client.encrypt_bits: +-1/8 against its own noise and a mod-switch error of deviation sqrt(n / 24) / 4096)
    the only error is what n external products add.  One external product acc += BK2_i [.] ((X^abar_i - 1) acc) adds, per coefficient
    of the phase:
      * key noise: every one of the (k+1) l2 = 8 rows is a TRLWE whose phase noise has deviation alpha2 2^64 per coefficient, multiplied
        by a digit polynomial of N2 coefficients.  The digits of a uniform word are uniform in [-Bg/2, Bg/2): energy Bg^2 / 12 each
        (the accumulator is uniform from the first step on whose difference is not zero; before it the digits are fewer and smaller).
        Variance (k+1) l2 N2 (Bg^2 / 12) (alpha2 2^64)^2.
      * the decomposition's rounding: the digits rebuild each word up to eps, uniform in +-2^(64 - l2 Bgbit2 - 1): variance
        2^(2 (64 - l2 Bgbit2)) / 12; the phase takes eps_b - eps_a s2, at most 1 + N2 such terms for a binary s2, and only in the
        steps whose key bit is 1 (all n taken).  Variance (1 + N2) 2^(2 (64 - l2 Bgbit2)) / 12.
    The n steps' errors are independent.  With alpha2 = 2^-44, l2 = 4, Bgbit2 = 9, N2 = 2048: 3.93e20 + 1.23e19 per step;
    sigma = 2^38.89 at n = 636 and 2^38.72 at n = 500 (DESIGN.md 6d measured worst errors of 2^38.5 .. 2^40.0), the bound 2^41.59 and
    2^41.41.  The smallest mu_r / 2 are 2^44 (128-bit set, r = 2) and 2^42 (80-bit set, r = 1): the bound clears both."""
    bg = 1 << BGBIT2
    key_noise = 2 * L2 * N2 * (bg * bg / 12.0) * (cases.ALPHA2 * 2.0 ** 64) ** 2
    rounding = (1 + N2) * 2.0 ** (2 * (64 - L2 * BGBIT2)) / 12.0
    return 6.5 * math.sqrt(n * (key_noise + rounding))


KEYS = {"mid": mid_key, "row": row_key}
