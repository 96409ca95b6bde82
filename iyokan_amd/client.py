"""Key generation / bit encryption / decryption (ctypes over libiyokan_client.so).

Mirrors what `iyokan-packet genkey|genevalkey|enc|dec` does for the reference
(/root/reference/src/iyokan-packet.cpp:144-178); used to make synthetic, non-trivial inputs.

Randomness: `seed=None` (the default) draws keys / masks / noise from a ChaCha20 stream keyed with fresh
getrandom(2) entropy for every call — two encryptions never share a mask.  An explicit integer `seed` selects
a seeded, NON-cryptographic generator: reproducible fixtures for tests and benchmarks only (the same seed
reproduces the same masks, so never encrypt two messages meant to stay secret with one seed).
"""
import ctypes
import os

import numpy as np

from .params import IykParams

_LIB = None
_u32p = ctypes.POINTER(ctypes.c_uint32)
_u8p = ctypes.POINTER(ctypes.c_uint8)


def _lib():
    global _LIB
    if _LIB is None:
        path = os.path.join(os.path.dirname(os.path.abspath(__file__)), "lib", "libiyokan_client.so")
        if not os.path.exists(path):
            raise RuntimeError(f"{path} missing: run `python -c 'import __graft_entry__ as g; g.build()'`")
        lib = ctypes.CDLL(path)
        lib.iyk_client_keygen.argtypes = [ctypes.POINTER(IykParams), ctypes.c_uint64, ctypes.c_int, _u32p, _u32p, _u32p, _u32p]
        lib.iyk_client_encrypt_bits.argtypes = [ctypes.POINTER(IykParams), _u32p, ctypes.c_uint64, ctypes.c_int, _u8p,
                                                ctypes.c_uint64, _u32p]
        lib.iyk_client_decrypt_bits.argtypes = [ctypes.POINTER(IykParams), _u32p, _u32p, ctypes.c_uint64, _u8p]
        lib.iyk_client_phases.argtypes = [ctypes.POINTER(IykParams), _u32p, _u32p, ctypes.c_uint64, _u32p]
        lib.iyk_client_trivial.argtypes = [ctypes.POINTER(IykParams), ctypes.c_int, _u32p]
        lib.iyk_client_encrypt_trlwe.argtypes = [ctypes.POINTER(IykParams), _u32p, ctypes.c_uint64, ctypes.c_int, _u32p,
                                                 ctypes.c_uint64, _u32p]
        lib.iyk_client_trlwe_phases.argtypes = [ctypes.POINTER(IykParams), _u32p, _u32p, ctypes.c_uint64, _u32p]
        u64, _u64p = ctypes.c_uint64, ctypes.POINTER(ctypes.c_uint64)
        lib.iyk_client_keygen_lvl2.argtypes = [ctypes.c_uint32, u64, ctypes.c_int, _u32p]
        lib.iyk_client_encrypt_tlwe2.argtypes = [ctypes.c_uint32, _u32p, u64, ctypes.c_int, ctypes.c_double, _u64p, u64, _u64p]
        lib.iyk_client_tlwe2_phases.argtypes = [ctypes.c_uint32, _u32p, _u64p, u64, _u64p]
        lib.iyk_client_privks_key_rows.argtypes = [ctypes.POINTER(IykParams), _u32p, ctypes.c_uint32, _u32p, ctypes.c_uint32,
                                                   ctypes.c_uint32, u64, u64, u64, ctypes.c_int, ctypes.c_int, _u32p]
        lib.iyk_client_bk2_rows.argtypes = [ctypes.c_uint32, _u32p, ctypes.c_uint32, _u32p, ctypes.c_uint32, ctypes.c_uint32,
                                            ctypes.c_double, u64, u64, u64, ctypes.c_int, ctypes.c_int, _u64p]
        _seedp = ctypes.c_char_p
        lib.iyk_client_chacha20_block.argtypes = [_u32p, _u32p]
        lib.iyk_client_expand_key_masks.argtypes = [ctypes.c_uint32, _seedp, u64, u64, u64, _u32p]
        lib.iyk_client_privks_key_rows_seeded.argtypes = [ctypes.POINTER(IykParams), _u32p, ctypes.c_uint32, _u32p, ctypes.c_uint32,
                                                          ctypes.c_uint32, _seedp, u64, u64, u64, ctypes.c_int, ctypes.c_int, _u32p]
        lib.iyk_client_bk2_rows_seeded.argtypes = [ctypes.c_uint32, _u32p, ctypes.c_uint32, _u32p, ctypes.c_uint32, ctypes.c_uint32,
                                                   ctypes.c_double, _seedp, u64, u64, u64, ctypes.c_int, ctypes.c_int, _u64p]
        _LIB = lib
    return _LIB


def _p32(a):
    return a.ctypes.data_as(_u32p)


class KeySet:
    """SecretKey (s0, s1) + EvalKey material the GPU path needs (bk<lvl01> torus, iksk<lvl10>)."""

    def __init__(self, params, s0, s1, bk, ksk):
        self.params, self.s0, self.s1, self.bk, self.ksk = params, s0, s1, bk, ksk


def keygen(params: IykParams, seed=None) -> KeySet:
    """SecretKey + EvalKey material.  seed=None: OS entropy (CSPRNG); an int: reproducible fixture keys."""
    s0 = np.zeros(params.n, dtype=np.uint32)
    s1 = np.zeros(params.N, dtype=np.uint32)
    bk = np.zeros(params.bk_words, dtype=np.uint32)
    ksk = np.zeros(params.ksk_words, dtype=np.uint32)
    rc = _lib().iyk_client_keygen(ctypes.byref(params), 0 if seed is None else int(seed), int(seed is not None),
                                  _p32(s0), _p32(s1), _p32(bk), _p32(ksk))
    if rc != 0:
        raise RuntimeError(f"iyk_client_keygen failed: {rc}")
    return KeySet(params, s0, s1, bk, ksk)


def encrypt_bits(keys: KeySet, bits, seed=None) -> np.ndarray:
    """bootsSymEncrypt of a bit vector.  seed=None: fresh OS-keyed stream per call; an int: reproducible fixture."""
    bits = np.ascontiguousarray(np.asarray(bits, dtype=np.uint8).ravel())
    out = np.zeros((bits.size, keys.params.n + 1), dtype=np.uint32)
    _lib().iyk_client_encrypt_bits(ctypes.byref(keys.params), _p32(keys.s0), 0 if seed is None else int(seed),
                                   int(seed is not None), bits.ctypes.data_as(_u8p), bits.size, _p32(out))
    return out


def decrypt_bits(keys: KeySet, ct) -> np.ndarray:
    ct = np.ascontiguousarray(ct, dtype=np.uint32).reshape(-1, keys.params.n + 1)
    bits = np.zeros(ct.shape[0], dtype=np.uint8)
    _lib().iyk_client_decrypt_bits(ctypes.byref(keys.params), _p32(keys.s0), _p32(ct), ct.shape[0],
                                   bits.ctypes.data_as(_u8p))
    return bits


def encrypt_trlwe(keys: KeySet, msg, seed=None) -> np.ndarray:
    """trlweSymEncrypt<Lvl1> of message polynomials (count, N) torus words -> (count, 2N): a(X) then b(X)."""
    msg = np.ascontiguousarray(msg, dtype=np.uint32).reshape(-1, keys.params.N)
    out = np.zeros((msg.shape[0], 2 * keys.params.N), dtype=np.uint32)
    _lib().iyk_client_encrypt_trlwe(ctypes.byref(keys.params), _p32(keys.s1), 0 if seed is None else int(seed),
                                    int(seed is not None), _p32(msg), msg.shape[0], _p32(out))
    return out


def trlwe_phases(keys: KeySet, ct) -> np.ndarray:
    """b - a * s1 of TRLWE lvl1 rows (count, 2N) -> (count, N); trlweSymDecrypt is `(int32) phase > 0` per coefficient."""
    ct = np.ascontiguousarray(ct, dtype=np.uint32).reshape(-1, 2 * keys.params.N)
    out = np.zeros((ct.shape[0], keys.params.N), dtype=np.uint32)
    _lib().iyk_client_trlwe_phases(ctypes.byref(keys.params), _p32(keys.s1), _p32(ct), ct.shape[0], _p32(out))
    return out


def encrypt_trgsw(keys: KeySet, bits, seed=None) -> np.ndarray:
    """trgswSymEncrypt<Lvl1> of bits -> u32 [count][(k+1) l][k+1][N], torus domain (the host form of TFHEpp::TRGSW<lvl1param>): row
    c l + j is a fresh encrypt_trlwe of zero plus bit * 2^(32 - (j+1) Bgbit) at coefficient 0 of polynomial c — the layout of one
    step of the bootstrapping key (csrc/client.cpp)."""
    bits = np.asarray(bits, dtype=np.uint8).ravel()
    p = keys.params
    rows = (p.k + 1) * p.l
    out = encrypt_trlwe(keys, np.zeros((bits.size * rows, p.N), dtype=np.uint32), seed).reshape(bits.size, rows, p.k + 1, p.N)
    for c in range(p.k + 1):
        for j in range(p.l):
            out[:, c * p.l + j, c, 0] += bits.astype(np.uint32) << np.uint32(32 - (j + 1) * p.Bgbit)
    return out


def encrypt_ram_trlwe(keys: KeySet, bits, seed=None) -> np.ndarray:
    """encryptRAM (/root/reference/src/packet.hpp:104-118): one TRLWE per bit, +-mu in coefficient 0."""
    bits = np.asarray(bits, dtype=np.uint8).ravel()
    msg = np.zeros((bits.size, keys.params.N), dtype=np.uint32)
    mu = int(keys.params.mu)
    msg[:, 0] = np.where(bits == 1, np.uint32(mu), np.uint32((1 << 32) - mu))
    return encrypt_trlwe(keys, msg, seed)


def decrypt_ram_trlwe(keys: KeySet, ct) -> np.ndarray:
    """decryptRAM (:153-164): coefficient 0 of every TRLWE."""
    return (trlwe_phases(keys, ct)[:, 0].view(np.int32) > 0).astype(np.uint8)


def encrypt_rom_trlwe(keys: KeySet, bits, seed=None) -> np.ndarray:
    """encryptROM (:78-97): N bits per TRLWE, +-mu per coefficient, 0 beyond the last bit."""
    bits = np.asarray(bits, dtype=np.uint8).ravel()
    N = keys.params.N
    count = -(-bits.size // N)
    mu = int(keys.params.mu)
    msg = np.zeros(count * N, dtype=np.uint32)
    msg[: bits.size] = np.where(bits == 1, np.uint32(mu), np.uint32((1 << 32) - mu))
    return encrypt_trlwe(keys, msg.reshape(count, N), seed)


def decrypt_rom_trlwe(keys: KeySet, ct) -> np.ndarray:
    """decryptROM (:172-183): every coefficient of every TRLWE (the padding of the last block decrypts to noise signs)."""
    return (trlwe_phases(keys, ct).view(np.int32) > 0).astype(np.uint8).ravel()


def phases(keys: KeySet, ct) -> np.ndarray:
    ct = np.ascontiguousarray(ct, dtype=np.uint32).reshape(-1, keys.params.n + 1)
    out = np.zeros(ct.shape[0], dtype=np.uint32)
    _lib().iyk_client_phases(ctypes.byref(keys.params), _p32(keys.s0), _p32(ct), ct.shape[0], _p32(out))
    return out


def trivial(params: IykParams, bit: int) -> np.ndarray:
    out = np.zeros(params.n + 1, dtype=np.uint32)
    _lib().iyk_client_trivial(ctypes.byref(params), int(bit), _p32(out))
    return out


# ---- lvl2 (64-bit torus) and the private key-switching key: the client side of circuit bootstrapping's second half ----------------
_u64p = ctypes.POINTER(ctypes.c_uint64)
MAX_THREADS = 16   # row generation never starts more threads than this, whatever the machine has


def _threads():
    try:
        return max(1, min(MAX_THREADS, len(os.sched_getaffinity(0))))
    except AttributeError:
        return 1


def keygen_lvl2(n_in, seed=None) -> np.ndarray:
    """A binary lvl2 secret key s2: u32 [n_in], one word per bit (TFHEpp's key.lvl2 has n_in = 2048)."""
    s2 = np.zeros(int(n_in), dtype=np.uint32)
    _lib().iyk_client_keygen_lvl2(int(n_in), 0 if seed is None else int(seed), int(seed is not None), _p32(s2))
    return s2


def encrypt_tlwe2(s2, msgs_u64, alpha, seed=None) -> np.ndarray:
    """TLWE lvl2 of 64-bit torus messages -> u64 [count][n_in + 1]: a, then b = msg + <a, s2> + Gaussian noise of deviation alpha."""
    s2 = np.ascontiguousarray(s2, dtype=np.uint32)
    msgs = np.ascontiguousarray(np.asarray(msgs_u64, dtype=np.uint64).ravel())
    out = np.zeros((msgs.size, s2.size + 1), dtype=np.uint64)
    _lib().iyk_client_encrypt_tlwe2(s2.size, _p32(s2), 0 if seed is None else int(seed), int(seed is not None), float(alpha),
                                    msgs.ctypes.data_as(_u64p), msgs.size, out.ctypes.data_as(_u64p))
    return out


def tlwe2_phases(s2, ct) -> np.ndarray:
    """b - <a, s2> of TLWE lvl2 rows -> u64 [count]."""
    s2 = np.ascontiguousarray(s2, dtype=np.uint32)
    ct = np.ascontiguousarray(ct, dtype=np.uint64).reshape(-1, s2.size + 1)
    out = np.zeros(ct.shape[0], dtype=np.uint64)
    _lib().iyk_client_tlwe2_phases(s2.size, _p32(s2), ct.ctypes.data_as(_u64p), ct.shape[0], out.ctypes.data_as(_u64p))
    return out


def privks_key_total_rows(params, n_in, t, basebit):
    return (params.k + 1) * (int(n_in) + 1) * int(t) * ((1 << int(basebit)) - 1)


MASK_PRIVKS, MASK_BK2 = 1, 2   # the `kind` of a seeded key's mask stream (csrc/key_expand.hpp)


def new_mask_seed() -> bytes:
    """32 bytes from the OS: the PUBLIC mask seed of ONE seeded key.  Draw a new one for every key: two keys made with one seed share
    their masks row for row."""
    return os.urandom(32)


def chacha20_block(state) -> np.ndarray:
    """The ChaCha20 block function (RFC 8439 §2.3) on a state of 16 u32 words: the one copy the client's generators, the mask
    expansion and the GPU kernel share (csrc/key_expand.hpp)."""
    state = np.ascontiguousarray(state, dtype=np.uint32).reshape(16)
    out = np.zeros(16, dtype=np.uint32)
    if _lib().iyk_client_chacha20_block(_p32(state), _p32(out)) != 0:
        raise ValueError("iyk_client_chacha20_block refused its arguments")
    return out


def _seed32(mask_seed) -> bytes:
    seed = bytes(mask_seed)
    if len(seed) != 32:
        raise ValueError(f"a mask seed is 32 bytes, not {len(seed)}")
    return seed


def expand_key_masks(kind, mask_seed, first_row, row_count, words_per_row) -> np.ndarray:
    """The masks of rows [first_row, first_row + row_count) of a seeded key -> u32 (row_count, words_per_row): kind MASK_PRIVKS with
    words_per_row = N gives the a polynomials of the private key-switching key's rows, kind MASK_BK2 with words_per_row = 2 N2 those of the
    lvl2 bootstrapping key's (`.view(np.uint64)`: a[m] = w[2m] | w[2m+1] << 32).  What the GPU writes in upload_seeded."""
    out = np.zeros((int(row_count), int(words_per_row)), dtype=np.uint32)
    rc = _lib().iyk_client_expand_key_masks(int(kind), _seed32(mask_seed), int(first_row), int(row_count), int(words_per_row), _p32(out))
    if rc != 0:
        raise ValueError(f"iyk_client_expand_key_masks refused its arguments ({rc})")
    return out


def privks_key_rows(keys: KeySet, s2, t, basebit, first_row=0, row_count=None, seed=None, nthreads=None, mask_seed=None) -> np.ndarray:
    """Rows [first_row, first_row + row_count) of the private key-switching key lvl2 -> lvl1, host layout
    u32 [k+1][n_in+1][t][2^basebit-1][k+1][N] flattened over its first four axes -> (row_count, 2N).  Row (c, i, j, u) is a TRLWE of
    zero (noise alpha1) plus sigma_i (u+1) 2^(32 - (j+1) basebit) at coefficient 0 of polynomial c, sigma_i = s2[i], sigma_{n_in} = -1.
    Any window gives the same words as the whole key (an int seed), so a full-size key (2.35 GB) is made and uploaded in chunks.
    mask_seed (32 public bytes, new_mask_seed()): the SEEDED key — only the b halves, (row_count, N), half the bytes; the a half of row R
    is expand_key_masks(MASK_PRIVKS, mask_seed, R, 1, N), and (a, b) has the phase of the unseeded row."""
    s2 = np.ascontiguousarray(s2, dtype=np.uint32)
    p = keys.params
    total = privks_key_total_rows(p, s2.size, t, basebit)
    row_count = total - first_row if row_count is None else int(row_count)
    if mask_seed is not None:
        out = np.zeros((max(row_count, 0), p.N), dtype=np.uint32)
        rc = _lib().iyk_client_privks_key_rows_seeded(ctypes.byref(p), _p32(keys.s1), s2.size, _p32(s2), int(t), int(basebit),
                                                      _seed32(mask_seed), int(first_row), row_count, 0 if seed is None else int(seed),
                                                      int(seed is not None), _threads() if nthreads is None else int(nthreads), _p32(out))
        if rc != 0:
            raise ValueError(f"iyk_client_privks_key_rows_seeded refused its arguments ({rc})")
        return out
    out = np.zeros((row_count, 2 * p.N), dtype=np.uint32)
    rc = _lib().iyk_client_privks_key_rows(ctypes.byref(p), _p32(keys.s1), s2.size, _p32(s2), int(t), int(basebit), int(first_row),
                                           row_count, 0 if seed is None else int(seed), int(seed is not None),
                                           _threads() if nthreads is None else int(nthreads), _p32(out))
    if rc != 0:
        raise ValueError(f"iyk_client_privks_key_rows refused its arguments ({rc})")
    return out


def encrypt_cb_digits(s2, bits, params, alpha, seed=None) -> np.ndarray:
    """What the lvl0 -> lvl2 rotation of circuit bootstrapping outputs, made by the key holder instead: per bit the l TLWE lvl2 of
    bit * 2^(64 - (r+1) Bgbit), r < l -> u64 [len(bits) * l][n_in + 1], TLWE bit * l + r = gadget digit r of that bit."""
    bits = np.asarray(bits, dtype=np.uint64).ravel()
    msgs = np.array([[int(b) << (64 - (r + 1) * params.Bgbit) for r in range(params.l)] for b in bits], dtype=np.uint64)
    return encrypt_tlwe2(s2, msgs.ravel(), alpha, seed)


def bk2_rows(keys: KeySet, s2, l2, Bgbit2, alpha2, first_step=0, step_count=None, seed=None, nthreads=None, mask_seed=None) -> np.ndarray:
    """Steps [first_step, first_step + step_count) of the lvl2 bootstrapping key of the lvl0 -> lvl2 rotation, torus domain:
    u64 [step_count][(k+1) l2][k+1][N2], N2 = len(s2).  Row c l2 + j of step i is a lvl2 TRLWE of zero (noise alpha2) under the ring key s2
    plus s0[i] 2^(64 - (j+1) Bgbit2) at coefficient 0 of polynomial c.  The lvl2 TLWE key the rotation's outputs decrypt under is s2 as
    tlwe2_phases takes it.  Any window gives the same words as the whole key (an int seed); at most MAX_THREADS threads.
    mask_seed (32 public bytes, new_mask_seed()): the SEEDED key — only the b halves, u64 [step_count][(k+1) l2][N2]; the a half of row
    R = step (k+1) l2 + r is expand_key_masks(MASK_BK2, mask_seed, R, 1, 2 N2).view(np.uint64)."""
    s2 = np.ascontiguousarray(s2, dtype=np.uint32)
    s0 = np.ascontiguousarray(keys.s0, dtype=np.uint32)
    step_count = s0.size - first_step if step_count is None else int(step_count)
    if mask_seed is not None:
        out = np.zeros((max(step_count, 0), 2 * int(l2), s2.size), dtype=np.uint64)
        rc = _lib().iyk_client_bk2_rows_seeded(s0.size, _p32(s0), s2.size, _p32(s2), int(l2), int(Bgbit2), float(alpha2), _seed32(mask_seed),
                                               int(first_step), step_count, 0 if seed is None else int(seed), int(seed is not None),
                                               _threads() if nthreads is None else int(nthreads), out.ctypes.data_as(_u64p))
        if rc != 0:
            raise ValueError(f"iyk_client_bk2_rows_seeded refused its arguments ({rc})")
        return out
    out = np.zeros((max(step_count, 0), 2 * int(l2), 2, s2.size), dtype=np.uint64)
    rc = _lib().iyk_client_bk2_rows(s0.size, _p32(s0), s2.size, _p32(s2), int(l2), int(Bgbit2), float(alpha2), int(first_step), step_count,
                                    0 if seed is None else int(seed), int(seed is not None),
                                    _threads() if nthreads is None else int(nthreads), out.ctypes.data_as(_u64p))
    if rc != 0:
        raise ValueError(f"iyk_client_bk2_rows refused its arguments ({rc})")
    return out
