"""Builders for the seeded evaluation keys (tests/test_key_expand.py on the CPU, tests/test_gpu_key_seeded*.py on the GPU): a numpy
restatement of the mask generator of csrc/key_expand.hpp written from RFC 8439 and the state layout DESIGN.md §6c states — nothing of
the library is used by it — small real keys of both kinds in seeded and unseeded form, full rows rebuilt from b halves and masks, and
the ctypes face of the kernel's emulation and of the pure argument check.  No GPU, no handle of the HIP library."""
import ctypes
import functools
import os

import numpy as np

import cb_rotate_cases
import privks_edge_cases as edge
from iyokan_amd import client

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
KIND_PRIVKS, KIND_BK2 = 1, 2
N2, L2, BGBIT2, ALPHA2 = cb_rotate_cases.N2, cb_rotate_cases.L2, cb_rotate_cases.BGBIT2, cb_rotate_cases.ALPHA2
SEED_A = bytes(range(32))                               # public mask seeds of the test keys
SEED_B = bytes((7 * i + 3) & 0xFF for i in range(32))
_u32p, _u64p, _u8p = ctypes.POINTER(ctypes.c_uint32), ctypes.POINTER(ctypes.c_uint64), ctypes.POINTER(ctypes.c_uint8)

# RFC 8439 §2.3.2: key 00 01 .. 1f, counter 1, nonce 00 00 00 09 00 00 00 4a 00 00 00 00
RFC_STATE_TAIL = (1, 0x09000000, 0x4A000000, 0)
RFC_BLOCK = [int(w, 16) for w in ("e4e7f110 15593bd1 1fdd0f50 c47120a3 c7f4d1c7 0368c033 9aaa2204 4e6cd4c3 "
                                  "466482d2 09aa9f07 05d7c214 a2028bd9 d19c12b5 b94e16de e883d0cb 4e3c50a2").split()]


# ---- the generator, restated ---------------------------------------------------------------------------------------------------------

def _rotl(x, k):
    return (x << np.uint32(k)) | (x >> np.uint32(32 - k))


def chacha20_blocks(states):
    """RFC 8439 §2.3 on u32 [count][16] states -> u32 [count][16]: 10 double rounds, then the state is added."""
    st = np.ascontiguousarray(states, dtype=np.uint32).reshape(-1, 16)
    x = [st[:, i].copy() for i in range(16)]

    def qr(a, b, c, d):
        x[a] += x[b]; x[d] = _rotl(x[d] ^ x[a], 16)
        x[c] += x[d]; x[b] = _rotl(x[b] ^ x[c], 12)
        x[a] += x[b]; x[d] = _rotl(x[d] ^ x[a], 8)
        x[c] += x[d]; x[b] = _rotl(x[b] ^ x[c], 7)

    with np.errstate(over="ignore"):
        for _ in range(10):
            for q in ((0, 4, 8, 12), (1, 5, 9, 13), (2, 6, 10, 14), (3, 7, 11, 15), (0, 5, 10, 15), (1, 6, 11, 12), (2, 7, 8, 13), (3, 4, 9, 14)):
                qr(*q)
        return np.stack(x, axis=1) + st


def state_of(key_bytes, w12, w13, w14, w15):
    """the 16 state words: "expand 32-byte k", the key as eight little-endian u32, then words 12 .. 15"""
    key = np.frombuffer(bytes(key_bytes), dtype="<u4")
    return np.concatenate([np.array([0x61707865, 0x3320646E, 0x79622D32, 0x6B206574], dtype=np.uint32), key.astype(np.uint32),
                           np.array([w12, w13, w14, w15], dtype=np.uint32)])


def mask_rows(kind, mask_seed, rows, words):
    """u32 [len(rows)][words]: word 12 = the block inside the row, 13 / 14 = the row index low / high, 15 = the kind"""
    rows = [int(r) for r in rows]
    blocks = -(-words // 16)
    st = np.tile(state_of(mask_seed, 0, 0, 0, kind), (len(rows) * blocks, 1))
    st[:, 12] = np.tile(np.arange(blocks, dtype=np.uint32), len(rows))
    st[:, 13] = np.repeat(np.array([r & 0xFFFFFFFF for r in rows], dtype=np.uint32), blocks)
    st[:, 14] = np.repeat(np.array([r >> 32 for r in rows], dtype=np.uint32), blocks)
    return chacha20_blocks(st).reshape(len(rows), blocks * 16)[:, :words]


def masks_u64(w):
    """the lvl2 key's packing, written out: a[m] = w[2m] | w[2m+1] << 32"""
    w = np.asarray(w, dtype=np.uint32)
    return w[..., 0::2].astype(np.uint64) | (w[..., 1::2].astype(np.uint64) << np.uint64(32))


# ---- small real keys, seeded and unseeded ----------------------------------------------------------------------------------------------

# (n_in, t, basebit): 48 rows; 2040 rows, 255 per (c, i, j); 6120 rows = 12 staging chunks of 512, the smallest shape of this kind whose
# whole-key upload takes more chunks than the ring has slots (9) with (j + 1) basebit <= 32 for every j
PRIVKS_SHAPES = {"small": (3, 2, 2), "wide": (3, 1, 8), "ring": (3, 3, 8)}
PRIVKS_CHUNK, BK2_CHUNK, STAGE_RING = 512, 8, 8           # iyokan_hip.hip: PRIVKS_SEEDED_CHUNK rows, BK2_UPLOAD_CHUNK steps, the ring's slots


@functools.lru_cache(maxsize=None)
def lvl2_key(n_in):
    return client.keygen_lvl2(n_in, seed=31)


def privks_b(keys, shape, mask_seed=SEED_A, **kw):
    n_in, t, bb = PRIVKS_SHAPES[shape]
    return client.privks_key_rows(keys, lvl2_key(n_in), t, bb, seed=32, mask_seed=mask_seed, **kw)


def privks_unseeded(keys, shape, **kw):
    n_in, t, bb = PRIVKS_SHAPES[shape]
    return client.privks_key_rows(keys, lvl2_key(n_in), t, bb, seed=32, **kw)


def privks_full_rows(b, mask_seed, first_row=0):
    """(rows, 2N) as the unseeded upload takes them: the restated mask, then b"""
    b = np.asarray(b, dtype=np.uint32)
    a = mask_rows(KIND_PRIVKS, mask_seed, range(first_row, first_row + b.shape[0]), b.shape[1])
    return np.ascontiguousarray(np.concatenate([a, b], axis=1))


def privks_message(keys, shape, row):
    """The message polynomial of host row `row` as int64 [N] mod 2^32: v on coefficient 0 for c = 1, -v s1(X) for c = 0, with
    v = sigma_i (u + 1) 2^(32 - (j + 1) basebit)."""
    n_in, t, bb = PRIVKS_SHAPES[shape]
    nb = (1 << bb) - 1
    u, j, i, c = row % nb, row // nb % t, row // nb // t % (n_in + 1), row // nb // t // (n_in + 1)
    sh = (j + 1) * bb
    m = ((u + 1) << (32 - sh)) & 0xFFFFFFFF if sh <= 32 else 0
    v = -m if i == n_in else m * int(lvl2_key(n_in)[i])
    N = keys.params.N
    msg = np.zeros(N, dtype=np.int64)
    if c == 1:
        msg[0] = v
    else:
        msg = -v * keys.s1.astype(np.int64)
    return msg & 0xFFFFFFFF


def privks_jobs(shape):
    """(tlwe2 u64 [nb][n_in + 1], jobs (in, c, out)): TLWE g has digit g + 1 at every (i, j), so the nb TLWEs under c = 0 and c = 1 read
    every row of the key exactly once."""
    n_in, t, bb = PRIVKS_SHAPES[shape]
    nb = (1 << bb) - 1
    tl = np.array([[edge.word_of_digits([g + 1] * t, bb)] * (n_in + 1) for g in range(nb)], dtype=np.uint64)
    jobs = [(g, c, 2 * g + c) for g in range(nb) for c in (0, 1)]
    return tl, jobs


def odd_windows(total):
    """three windows cut at odd rows, one of a single row, in the order they are sent: the last, the first, the single row"""
    cut = (total // 2) | 1
    return [(cut + 1, total - cut - 1), (0, cut), (cut, 1)]


def chunk_windows(total, chunk):
    """Three windows of a key of `total` units whose uploads are staged `chunk` units at a time, in the order they are sent: one that
    starts a unit short of a chunk edge and ends on the next edge (a whole chunk at an unaligned destination, then a tail of one unit),
    the rest of the key, the head."""
    assert total > 2 * chunk
    w = [(chunk - 1, chunk + 1), (2 * chunk, total - 2 * chunk), (0, chunk - 1)]
    assert sorted(u for f, c in w for u in range(f, f + c)) == list(range(total))   # they tile [0, total) exactly once
    return w


BK2_N = 3
_S0_SEED = 22   # the generator seed of the lvl0 secrets below: found by search for the properties _s0 asserts, and [1, 0, 1] at n = 3


@functools.lru_cache(maxsize=None)
def _s0(n):
    """The lvl0 secret of the lvl2 test key of n steps, as what client.bk2_rows reads of a KeySet.  Both bit values occur among the first
    staging chunk's steps and among the last chunk's (a last chunk of one step: it and the step before it differ)."""
    ks = cb_rotate_cases.SmallKeys(n, _S0_SEED)
    s0 = [int(v) for v in ks.s0]
    last = s0[BK2_CHUNK * ((n - 1) // BK2_CHUNK):]
    assert len(set(s0[:BK2_CHUNK])) == 2 and len(set(last if len(last) > 1 else s0[-2:])) == 2, (n, s0)
    return ks


_S0 = _s0(BK2_N)   # [1, 0, 1]: the key the n = 3 tests have always used


def bk2_b(mask_seed=SEED_A, n=BK2_N, **kw):
    return client.bk2_rows(_s0(n), lvl2_key(N2), L2, BGBIT2, ALPHA2, seed=33, mask_seed=mask_seed, **kw)


def bk2_unseeded(n=BK2_N, **kw):
    return client.bk2_rows(_s0(n), lvl2_key(N2), L2, BGBIT2, ALPHA2, seed=33, **kw)


REAL_N = 67   # 9 staging chunks, one more than the ring has slots: an upload in one call takes a slot of its own again


@functools.lru_cache(maxsize=None)
def bk2_real(n=REAL_N, seed=5, mask_seed=SEED_A):
    """-> (ks, s2, b halves u64 [n][8][N2]): a real seeded key from the secrets cb_rotate_cases.real_case(n, seed) draws"""
    ks = cb_rotate_cases.SmallKeys(n, seed)
    s2 = client.keygen_lvl2(N2, seed=seed + 1)
    return ks, s2, client.bk2_rows(ks, s2, L2, BGBIT2, ALPHA2, seed=seed + 2, mask_seed=mask_seed)


@functools.lru_cache(maxsize=None)
def bk2_real_jobs(n=REAL_N):
    """-> (ct u32 [2][n + 1]: a 1 and a 0 under bk2_real's lvl0 secret, jobs (in, sign, off, mu), bits): each bit under both signs at the
    three mu_r of the 128-bit set"""
    ct = cb_rotate_cases.encrypt_lvl0(bk2_real(n)[0].s0, [1, 0], seed=671)
    jobs = [(i, sign, 0, cb_rotate_cases.ref.mu_of(r, 6)) for i in (0, 1) for sign in (1, -1) for r in range(3)]
    return ct, jobs, [1 - j[0] for j in jobs]


def bk2_full_steps(b, mask_seed, first_step=0):
    """u64 (steps, (k+1) l2, 2, N2) as the unseeded upload takes them"""
    b = np.asarray(b, dtype=np.uint64)
    rows = 2 * L2
    a = masks_u64(mask_rows(KIND_BK2, mask_seed, range(first_step * rows, (first_step + b.shape[0]) * rows), 2 * N2))
    return np.ascontiguousarray(np.stack([a.reshape(b.shape), b], axis=2))


def bk2_jobs(n=BK2_N):
    """(lvl0 TLWEs u32 [4][n + 1], jobs (in, sign, off, mu, out)): four rotations, both signs, outputs in another order than inputs"""
    rng = np.random.default_rng(34)
    tl = rng.integers(0, 1 << 32, size=(4, n + 1), dtype=np.uint64).astype(np.uint32)
    mus = [1 << (63 - (r + 1) * 6) for r in range(3)] + [1 << 61]
    jobs = [(g, 1 if g & 1 else -1, int(rng.integers(0, 1 << 32)), mus[g], 3 - g) for g in range(4)]
    return tl, jobs


# ---- the emulation library --------------------------------------------------------------------------------------------------------------

@functools.lru_cache(maxsize=None)
def emul():
    L = ctypes.CDLL(os.path.join(ROOT, "iyokan_amd", "lib", "libiyk_emul.so"))
    L.iyk_emul_key_mask_expand.argtypes = [ctypes.c_uint32, ctypes.c_char_p, ctypes.c_uint64, ctypes.c_uint64, ctypes.c_uint32, ctypes.c_int,
                                           _u32p, _u32p]
    L.iyk_emul_key_upload_seeded_args.argtypes = [ctypes.c_uint64] * 4 + [ctypes.c_int] * 4 + [ctypes.c_uint64] * 3 + [
        ctypes.c_char_p, ctypes.c_uint64, _u32p, ctypes.c_uint64, _u64p]
    return L


def emul_expand(kind, mask_seed, first_row, row_count, ring, cus, dst_u32, src_b_u32):
    """key_mask_expand_kernel lane by lane on the CPU, in place on dst_u32 (a view of the window's first destination row)"""
    assert dst_u32.dtype == np.uint32 and src_b_u32.dtype == np.uint32 and src_b_u32.flags.c_contiguous
    return emul().iyk_emul_key_mask_expand(kind, bytes(mask_seed), first_row, row_count, ring, cus, dst_u32.ctypes.data_as(_u32p),
                                           src_b_u32.ctypes.data_as(_u32p))


def check_args(st=1, key=2, mask_seed=3, host_b=4, st_replica=0, key_replica=0, st_ordinal=0, key_ordinal=0, key_units=48, first=0, count=48):
    """(code, text) of args::key_upload_seeded_args; the four handles as integers, 0 = null"""
    msg = ctypes.create_string_buffer(256)
    counts = (ctypes.c_uint64 * 4)()
    rc = emul().iyk_emul_key_upload_seeded_args(st, key, mask_seed, host_b, st_replica, key_replica, st_ordinal, key_ordinal, key_units, first,
                                                count, msg, 256, None, 0, counts)
    return rc, msg.value.decode()


# every refusal of the seeded uploads: name -> (arguments of check_args, the text)
REFUSALS = {
    "null stream": (dict(st=0), "null argument"),
    "null key": (dict(key=0), "null argument"),
    "null seed": (dict(mask_seed=0), "null argument"),
    "null buffer": (dict(host_b=0), "null argument"),
    "another GPU": (dict(key_replica=1, key_ordinal=1), "the stream and the key are on different GPUs"),
    "another replica": (dict(key_replica=1), "the stream and the key belong to different replicas"),
    "empty window": (dict(count=0), "empty window"),
    "window starts past the key": (dict(first=49, count=1), "window outside the key"),
    "window ends past the key": (dict(first=47, count=2), "window outside the key"),
    "window wraps 2^64": (dict(first=(1 << 64) - 1, count=2), "window outside the key"),
}
