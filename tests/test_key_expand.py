"""CPU: the seeded evaluation keys.  The shared ChaCha20 block function (csrc/key_expand.hpp) against RFC 8439 and against a numpy
restatement, client.expand_key_masks against the restatement at the row indices and block edges where the state layout can go wrong,
window independence of the seeded rows, seeded rows as keys (phases and noise), the emulation of key_mask_expand_kernel on a
device-layout buffer with canary rows, and every refusal of the pure argument check."""
import numpy as np
import pytest

import cb_rotate_ref
import key_expand_cases as cases
import privks_edge_cases as edge
import privks_ref
from iyokan_amd import client
from test_privks_ref import _noise_bound   # the bound the existing private-key tests hold a sum of `rows` key rows to


def test_rfc8439_block_vector():
    """§2.3.2 through the client library (the shared header) and through the restatement.  If `cryptography` is importable its
    ChaCha20 decides which of the three is right."""
    st = cases.state_of(bytes(range(32)), *cases.RFC_STATE_TAIL)
    lib = [int(v) for v in client.chacha20_block(st)]
    own = [int(v) for v in cases.chacha20_blocks(st)[0]]
    assert lib == own
    try:
        from cryptography.hazmat.primitives.ciphers import Cipher, algorithms
    except ImportError:
        pass
    else:   # its 16-byte nonce is the little-endian counter then the 12-byte nonce: state words 12 .. 15
        nonce = np.array(cases.RFC_STATE_TAIL, dtype="<u4").tobytes()
        ks = Cipher(algorithms.ChaCha20(bytes(range(32)), nonce), mode=None).encryptor().update(bytes(64))
        assert [int(v) for v in np.frombuffer(ks, dtype="<u4")] == cases.RFC_BLOCK
    assert lib == cases.RFC_BLOCK


@pytest.mark.parametrize("kind,words", [(cases.KIND_PRIVKS, 1024), (cases.KIND_BK2, 4096)], ids=["privks", "bk2"])
def test_masks_equal_the_restatement(kind, words):
    """row indices 0, 1, 2^32 - 1, 2^32, 2^40 + 3: the high word of the row index is used; whole rows: block 0, the last block, and the
    first block of the next row (a window of two rows: no carry from one row into the next)"""
    for first in (0, 1, (1 << 32) - 1, 1 << 32, (1 << 40) + 3):
        got = client.expand_key_masks(kind, cases.SEED_A, first, 2, words)
        want = cases.mask_rows(kind, cases.SEED_A, [first, first + 1], words)
        assert got.shape == (2, words) and np.array_equal(got, want), first
        blocks = words // 16
        last = cases.chacha20_blocks(cases.state_of(cases.SEED_A, blocks - 1, first & 0xFFFFFFFF, first >> 32, kind))[0]
        nxt = cases.chacha20_blocks(cases.state_of(cases.SEED_A, 0, (first + 1) & 0xFFFFFFFF, (first + 1) >> 32, kind))[0]
        assert np.array_equal(got[0, -16:], last) and np.array_equal(got[1, :16], nxt)
    a = client.expand_key_masks(kind, cases.SEED_A, 1 << 32, 1, words)
    assert not np.array_equal(a, client.expand_key_masks(kind, cases.SEED_A, 0, 1, words))          # the high word counts
    assert not np.array_equal(a, client.expand_key_masks(3 - kind, cases.SEED_A, 1 << 32, 1, words))  # the kind counts
    assert not np.array_equal(a, client.expand_key_masks(kind, cases.SEED_B, 1 << 32, 1, words))      # the seed counts
    assert np.array_equal(client.expand_key_masks(kind, cases.SEED_A, 5, 1, 40)[0], cases.mask_rows(kind, cases.SEED_A, [5], 48)[0, :40])
    for bad in (dict(kind=0), dict(kind=3), dict(words_per_row=0)):
        with pytest.raises(ValueError):
            client.expand_key_masks(**{**dict(kind=kind, mask_seed=cases.SEED_A, first_row=0, row_count=1, words_per_row=16), **bad})
    with pytest.raises(ValueError):
        client.expand_key_masks(kind, b"short", 0, 1, 16)


def test_u64_packing_of_the_lvl2_key():
    w = client.expand_key_masks(cases.KIND_BK2, cases.SEED_A, 9, 1, 2 * cases.N2)
    a = cases.masks_u64(w)[0]
    assert a.shape == (cases.N2,) and int(a[5]) == int(w[0, 10]) | int(w[0, 11]) << 32
    assert np.array_equal(a, w.view(np.uint64)[0])   # which is the order of the words in memory


@pytest.mark.parametrize("nthreads", [1, 3])
def test_windows_give_the_whole_seeded_key(keys128, nthreads):
    """cut at rows [0, 1), [1, 8), [8, end), whatever nthreads is; and half the bytes of the unseeded key, exactly"""
    whole = cases.privks_b(keys128, "small", nthreads=2)
    total = whole.shape[0]
    parts = [cases.privks_b(keys128, "small", first_row=f, row_count=c, nthreads=nthreads) for f, c in ((0, 1), (1, 7), (8, total - 8))]
    assert np.array_equal(np.concatenate(parts), whole)
    full = cases.privks_unseeded(keys128, "small")
    assert whole.shape == (48, keys128.params.N) and 2 * whole.nbytes == full.nbytes
    assert not np.array_equal(whole, cases.privks_b(keys128, "small", mask_seed=cases.SEED_B))

    whole2 = cases.bk2_b(nthreads=2)
    parts2 = [cases.bk2_b(first_step=f, step_count=c, nthreads=nthreads) for f, c in ((0, 1), (1, 2))]
    assert np.array_equal(np.concatenate(parts2), whole2)
    # row windows of the lvl2 key are whole steps; inside a step the rows are independent too: one thread against three gave one key
    assert whole2.shape == (cases.BK2_N, 8, cases.N2) and 2 * whole2.nbytes == cases.bk2_unseeded().nbytes
    with pytest.raises(ValueError):
        cases.privks_b(keys128, "small", first_row=total, row_count=1)
    with pytest.raises(ValueError):
        cases.bk2_b(first_step=cases.BK2_N + 1)


def _signed32(x):
    return np.asarray(x, dtype=np.uint32).view(np.int32).astype(np.int64)


@pytest.mark.parametrize("shape", ["small"])
def test_seeded_private_key_rows_are_key_rows(keys128, shape):
    """full rows rebuilt from b halves and expanded masks have the phases of the unseeded key's rows — the message of every row — with
    noise inside the bound of tests/test_privks_ref.py for one row of noise alpha1"""
    p = keys128.params
    b = cases.privks_b(keys128, shape)
    rows = cases.privks_full_rows(b, cases.SEED_A)
    assert np.array_equal(rows[:, : p.N], client.expand_key_masks(cases.KIND_PRIVKS, cases.SEED_A, 0, b.shape[0], p.N))
    ph_seeded = client.trlwe_phases(keys128, rows)
    ph_plain = client.trlwe_phases(keys128, cases.privks_unseeded(keys128, shape))
    bound = _noise_bound(p, 1)
    worst = 0
    for r in range(rows.shape[0]):
        msg = cases.privks_message(keys128, shape, r)
        e_seeded = np.abs(_signed32((ph_seeded[r].astype(np.int64) - msg) & 0xFFFFFFFF)).max()
        e_plain = np.abs(_signed32((ph_plain[r].astype(np.int64) - msg) & 0xFFFFFFFF)).max()
        worst = max(worst, int(e_seeded))
        assert 0 < e_seeded < bound and 0 < e_plain < bound, (r, e_seeded, e_plain, bound)
    print(f"worst phase error of a seeded row {worst}, bound {bound:.0f}")


def _lvl2_row_error(s2, bit, r, row):
    """the largest |phase - message| over the coefficients of row r = c l2 + j of a key step whose lvl0 key bit is `bit`; row: (a, b)"""
    c, j = divmod(r, 4)
    ones = np.flatnonzero(s2)
    m = np.zeros(cases.N2, dtype=np.uint64)
    m[0] = np.uint64(int(bit) << (64 - (j + 1) * 9))
    want = m.copy()
    if c == 0:   # message on a: phase = -s2(X) m
        want = np.zeros(cases.N2, dtype=np.uint64)
        for t in ones:
            want -= cb_rotate_ref.mul_xr(m, int(t))
    a_, b_ = row
    ph = b_.copy()
    for t in ones:
        ph -= cb_rotate_ref.mul_xr(a_, int(t))
    return int(np.abs((ph - want).view(np.int64)).max())


def test_seeded_lvl2_key_rows_are_key_rows():
    """the same for the lvl2 key, by the method and the bound (2^26 for alpha2 = 2^-44) of tests/test_cb_rotate_ref.py"""
    s2 = cases.lvl2_key(cases.N2)
    full = cases.bk2_full_steps(cases.bk2_b(), cases.SEED_A)
    plain = cases.bk2_unseeded()
    assert full.shape == plain.shape == (cases.BK2_N, 8, 2, cases.N2)
    for i, r in ((0, 0), (0, 3), (0, 4), (0, 7), (1, 0), (1, 7), (2, 5)):
        for key in (full, plain):
            err = _lvl2_row_error(s2, cases._S0.s0[i], r, key[i, r])
            assert 0 < err < 1 << 26, (i, r, key is full, err)


def test_real_lvl2_key_of_nine_chunks_is_a_key():
    """the n = 67 key the GPU decrypts under (tests/test_gpu_key_seeded_edges.py): rows of the steps either side of the first chunk edge,
    of the last edge, and the first and the last step, rebuilt from b halves and the restated masks, hold their phases to the same 2^26"""
    ks, s2, b = cases.bk2_real()
    assert b.shape == (cases.REAL_N, 8, cases.N2) and -(-cases.REAL_N // cases.BK2_CHUNK) == cases.STAGE_RING + 1
    full = cases.bk2_full_steps(b, cases.SEED_A)
    assert set(int(ks.s0[i]) for i in (0, 7, 8, 63, 64, 66)) == {0, 1}
    for i, r in ((0, 0), (7, 3), (8, 4), (63, 7), (64, 1), (66, 5)):
        err = _lvl2_row_error(s2, ks.s0[i], r, full[i, r])
        assert 0 < err < 1 << 26, (i, r, err)
    # a window of the seeded key is the whole key's: steps 63 .. 66 made alone
    part = client.bk2_rows(ks, s2, cases.L2, cases.BGBIT2, cases.ALPHA2, seed=7, mask_seed=cases.SEED_A, first_step=63, step_count=4)
    assert np.array_equal(part, b[63:])


def test_default_builders_give_the_keys_they_always_gave():
    """bk2_b() and bk2_jobs() took no n before the edge cases came: their defaults are the n = 3 arrays of then, by SHA-256"""
    import hashlib

    tl, jobs = cases.bk2_jobs()
    assert [int(v) for v in cases._S0.s0] == [1, 0, 1] and cases.bk2_b().shape == (3, 8, cases.N2)
    assert hashlib.sha256(np.ascontiguousarray(cases.bk2_b()).tobytes()).hexdigest() == \
        "2b6125d2a3f900a41876eedd40d1bf14d6a967980fb1034c5dc8eb91f6fc87a9"
    assert hashlib.sha256(np.ascontiguousarray(cases.bk2_unseeded()).tobytes()).hexdigest() == \
        "6e5fdfd74c225c1c3472e09927f22e1cc5c8cd17511edc97b699cf19795b3ace"
    assert hashlib.sha256(tl.tobytes() + repr(jobs).encode()).hexdigest() == "25b2a003f629cb354e1b032b1aa843bbeacfe3bfdd5e642fa3b6999cd58df03f"
    for n in (17, cases.REAL_N):   # the secrets of the longer keys: both bit values in the first chunk and at the last chunk's edge
        s0 = cases._s0(n).s0
        assert s0.size == n and cases.bk2_jobs(n)[0].shape == (4, n + 1)


def test_chunk_windows_tile_their_keys():
    assert cases.chunk_windows(17, 8) == [(7, 9), (16, 1), (0, 7)]
    w = cases.chunk_windows(6120, cases.PRIVKS_CHUNK)
    assert w == [(511, 513), (1024, 5096), (0, 511)]
    for total, chunk in ((17, 8), (6120, 512), (67, 8)):
        seen = np.zeros(total, dtype=np.int64)
        for first, count in cases.chunk_windows(total, chunk):
            seen[first:first + count] += 1
        assert (seen == 1).all()
    assert edge.key_rows(*cases.PRIVKS_SHAPES["ring"]) == 6120 == 12 * cases.PRIVKS_CHUNK - 24 and 12 > cases.STAGE_RING


def test_ring_jobs_read_every_key_row_once():
    """privks_jobs("ring"): 255 TLWEs under c = 0 and c = 1; privks_ref.selected_rows of the 510 jobs is every row index (c, i, j, u) of
    the 6120, each exactly once"""
    n_in, t, bb = cases.PRIVKS_SHAPES["ring"]
    tl, jobs = cases.privks_jobs("ring")
    assert tl.shape == (255, n_in + 1) and len(jobs) == 510 and sorted(j[2] for j in jobs) == list(range(510))
    seen = np.zeros(edge.key_rows(n_in, t, bb), dtype=np.int64)
    for g, c, _ in jobs:
        idx = privks_ref.selected_rows(tl[g], c, t, bb)
        assert idx.size == (n_in + 1) * t
        np.add.at(seen, idx, 1)
    assert (seen == 1).all()


@pytest.mark.parametrize("kind,ring", [(cases.KIND_PRIVKS, 1024), (cases.KIND_BK2, cases.N2)], ids=["privks", "bk2"])
@pytest.mark.parametrize("cus", [1, 256])
def test_emulated_kernel_writes_one_odd_row_and_nothing_else(kind, ring, cus):
    """A window that starts at an odd row and is one row long, in a device-layout buffer of three rows: the middle row becomes the mask
    then the b half, the canary rows either side stay.  cus = 1 caps the grid under the lvl2 row's 256 blocks: the stride loop runs."""
    per = ring if kind == cases.KIND_PRIVKS else 2 * ring      # u32 words of one polynomial
    rng = np.random.default_rng(41)
    buf = rng.integers(0, 1 << 32, size=(3, 2 * per), dtype=np.uint64).astype(np.uint32)
    before = buf.copy()
    b = rng.integers(0, 1 << 32, size=(1, per), dtype=np.uint64).astype(np.uint32)
    first = 7
    assert cases.emul_expand(kind, cases.SEED_A, first, 1, ring, cus, buf[1], b) == 0
    assert np.array_equal(buf[0], before[0]) and np.array_equal(buf[2], before[2])
    assert np.array_equal(buf[1, :per], cases.mask_rows(kind, cases.SEED_A, [first], per)[0])
    assert np.array_equal(buf[1, :per], client.expand_key_masks(kind, cases.SEED_A, first, 1, per)[0])
    assert np.array_equal(buf[1, per:], b[0])
    # three rows from row 2^32 - 1 on: rows either side of the 32-bit line, still inside the buffer
    b3 = rng.integers(0, 1 << 32, size=(3, per), dtype=np.uint64).astype(np.uint32)
    assert cases.emul_expand(kind, cases.SEED_B, (1 << 32) - 1, 3, ring, cus, buf[0], b3) == 0
    want = cases.mask_rows(kind, cases.SEED_B, [(1 << 32) - 1, 1 << 32, (1 << 32) + 1], per)
    assert np.array_equal(buf[:, :per], want) and np.array_equal(buf[:, per:], b3)
    assert cases.emul_expand(kind, cases.SEED_A, 0, 0, ring, cus, buf[0], b3) == -1     # no lanes: no launch
    assert cases.emul_expand(3, cases.SEED_A, 0, 1, ring, cus, buf[0], b3) == -1


def test_emulated_kernel_gives_the_unseeded_keys_layout(keys128):
    """the whole small private key through the emulation is the host-rebuilt key the unseeded upload takes"""
    b = cases.privks_b(keys128, "small")
    dev = np.zeros((b.shape[0], 2 * b.shape[1]), dtype=np.uint32)
    for first, count in cases.odd_windows(b.shape[0]):
        assert cases.emul_expand(cases.KIND_PRIVKS, cases.SEED_A, first, count, b.shape[1], 4, dev[first], np.ascontiguousarray(b[first:first + count])) == 0
    assert np.array_equal(dev, cases.privks_full_rows(b, cases.SEED_A))
    assert cases.odd_windows(48) == [(26, 22), (0, 25), (25, 1)]   # out of order, the single row 25 last


def _chunked(first, count, chunk):
    """the sub-windows (first unit, units, units done before) the seeded uploads' staging loops form of one window"""
    return [(first + done, min(chunk, count - done), done) for done in range(0, count, chunk)]


def test_emulated_private_key_window_in_chunks_is_the_window_whole(keys128):
    """Rows [511, 1025) of the "ring" key, the first of chunk_windows: as the staging loop cuts it (512 rows from 511, then 2 from 1023:
    every chunk's first_row is the window's plus the rows done) and in one call.  One device-layout buffer either way, the rebuilt
    rows; the rows either side of the window stay."""
    first, count = 511, 514
    assert _chunked(first, count, cases.PRIVKS_CHUNK) == [(511, 512, 0), (1023, 2, 512)]
    b = cases.privks_b(keys128, "ring", first_row=first, row_count=count)
    N = b.shape[1]
    rng = np.random.default_rng(43)
    canary = rng.integers(0, 1 << 32, size=(count + 2, 2 * N), dtype=np.uint64).astype(np.uint32)
    chunks, whole = canary.copy(), canary.copy()
    for f, c, done in _chunked(first, count, cases.PRIVKS_CHUNK):
        assert cases.emul_expand(cases.KIND_PRIVKS, cases.SEED_A, f, c, N, 256, chunks[1 + done], np.ascontiguousarray(b[done:done + c])) == 0
    assert cases.emul_expand(cases.KIND_PRIVKS, cases.SEED_A, first, count, N, 256, whole[1], b) == 0
    assert np.array_equal(chunks, whole)
    assert np.array_equal(whole[1:-1], cases.privks_full_rows(b, cases.SEED_A, first_row=first))
    assert np.array_equal(whole[0], canary[0]) and np.array_equal(whole[-1], canary[-1])
    # the chunk that forgets the rows done (first_row = the window's) gives other masks: the GPU test can tell
    wrong = canary.copy()
    assert cases.emul_expand(cases.KIND_PRIVKS, cases.SEED_A, first, 2, N, 256, wrong[1 + 512], np.ascontiguousarray(b[512:])) == 0
    assert not np.array_equal(wrong[513:515, :N], whole[513:515, :N]) and np.array_equal(wrong[513:515, N:], whole[513:515, N:])


def test_emulated_lvl2_window_in_chunks_is_the_window_whole():
    """Nine lvl2 steps from step 7 (the first of chunk_windows(17, 8)): 8 steps from mask row 7 * 8 then one from row 15 * 8, and one
    call over all 72 rows.  The staged torus-domain window u64 [rows][a: N2][b: N2] either way: what the chunk loop must pass as
    first_row is (first_step + done) * 8."""
    first, count, rows = 7, 9, 2 * cases.L2
    assert _chunked(first, count, cases.BK2_CHUNK) == [(7, 8, 0), (15, 1, 8)]
    b = cases.bk2_b(n=17)[first:first + count]
    b32 = np.ascontiguousarray(b).view(np.uint32).reshape(count * rows, 2 * cases.N2)
    rng = np.random.default_rng(44)
    canary = rng.integers(0, 1 << 32, size=(count * rows + 2, 4 * cases.N2), dtype=np.uint64).astype(np.uint32)
    chunks, whole = canary.copy(), canary.copy()
    for f, c, done in _chunked(first, count, cases.BK2_CHUNK):
        src = np.ascontiguousarray(b32[done * rows:(done + c) * rows])
        assert cases.emul_expand(cases.KIND_BK2, cases.SEED_A, f * rows, c * rows, cases.N2, 256, chunks[1 + done * rows], src) == 0
    assert cases.emul_expand(cases.KIND_BK2, cases.SEED_A, first * rows, count * rows, cases.N2, 256, whole[1], b32) == 0
    assert np.array_equal(chunks, whole)
    want = cases.bk2_full_steps(b, cases.SEED_A, first_step=first)
    assert np.array_equal(whole[1:-1].view(np.uint64).reshape(want.shape), want)
    assert np.array_equal(whole[0], canary[0]) and np.array_equal(whole[-1], canary[-1])


@pytest.mark.parametrize("name", list(cases.REFUSALS))
def test_argument_check_refuses(name):
    kw, text = cases.REFUSALS[name]
    assert cases.check_args(**kw) == (-1, text)


def test_argument_check_accepts_up_to_the_whole_key():
    assert cases.check_args() == (0, "")                                   # the largest legal window: the whole key
    assert cases.check_args(first=47, count=1) == (0, "")                  # its last row alone
    assert cases.check_args(first=25, count=1) == (0, "")                  # one odd row
    assert cases.check_args(key_units=(1 << 64) - 1, first=0, count=(1 << 64) - 1) == (0, "")
    assert cases.check_args(st_replica=1, key_replica=1, st_ordinal=0, key_ordinal=0) == (0, "")   # replica 1 on device 0
