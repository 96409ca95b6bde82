"""CPU: the host side of the matrix form of the key switch (csrc/dispatch.hpp, through libiyk_emul.so) — the signed base-256 split of
a key word, the operand's layout function, the predicate that sends a batch to the form, and a numpy restatement of the product
(one-hot digits x planes, recombined, subtracted) against the digit-by-digit sum."""
import ctypes
import os

import numpy as np
import pytest

import ks_words as K

SETS = {"128": (7, 5, 637), "80": (8, 4, 501)}   # t, nc = padded row words / 128, row words n + 1
N = 1024
_i64p = ctypes.POINTER(ctypes.c_int64)
_ip = ctypes.POINTER(ctypes.c_int)


@pytest.fixture(scope="module")
def em():
    L = ctypes.CDLL(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "iyokan_amd", "lib", "libiyk_emul.so"))
    L.iyk_emul_ks_matrix_form.argtypes = [ctypes.c_int] * 4
    L.iyk_emul_ks_matrix_bytes.argtypes = [ctypes.c_int] * 2
    L.iyk_emul_ks_matrix_bytes.restype = ctypes.c_int64
    L.iyk_emul_ks_matrix_offset.argtypes = [ctypes.c_int] * 6
    L.iyk_emul_ks_matrix_offset.restype = ctypes.c_int64
    L.iyk_emul_ks_matrix_offsets_k.argtypes = [ctypes.c_int, _ip, ctypes.c_int, ctypes.c_int, ctypes.c_int, _i64p]
    L.iyk_emul_ks_matrix_offsets_k.restype = None
    L.iyk_emul_ks_signed_planes.argtypes = [ctypes.POINTER(ctypes.c_uint32), ctypes.c_int, ctypes.POINTER(ctypes.c_int8)]
    L.iyk_emul_ks_signed_planes.restype = None
    return L


def _planes(em, words):
    w = np.ascontiguousarray(words, dtype=np.uint32)
    out = np.empty((len(w), 4), dtype=np.int8)
    em.iyk_emul_ks_signed_planes(w.ctypes.data_as(ctypes.POINTER(ctypes.c_uint32)), len(w), out.ctypes.data_as(ctypes.POINTER(ctypes.c_int8)))
    return out


def _offsets_k(em, t, ks, word, plane):
    ks = np.ascontiguousarray(ks, dtype=np.int32)
    out = np.empty(len(ks), dtype=np.int64)
    em.iyk_emul_ks_matrix_offsets_k(t, ks.ctypes.data_as(_ip), word, plane, len(ks), out.ctypes.data_as(_i64p))
    return out


def test_signed_base_256_split(em):
    """Every plane lies in [-128, 127] (it is an int8) and sum s_p 256^p = w mod 2^32, at the carry edges and on 10^5 random words."""
    edges = [0, 0x7F, 0x80, 0xFF, 0x7FFF, 0x8000, 0x7F7F7F7F, 0x80808080, 0x7FFFFFFF, 0x80000000, 0xFFFFFF80, 0xFFFFFFFF]
    w = np.concatenate([np.array(edges, dtype=np.uint32), np.random.default_rng(256).integers(0, 1 << 32, size=100000, dtype=np.uint32)])
    s = _planes(em, w).astype(np.int64)
    assert s.min() >= -128 and s.max() <= 127
    back = (s * (np.int64(256) ** np.arange(4))).sum(axis=1) & K.MASK32
    assert np.array_equal(back, w.astype(np.int64))
    assert s[1].tolist() == [127, 0, 0, 0] and s[2].tolist() == [-128, 1, 0, 0] and s[7].tolist() == [-128, -127, -127, -127]
    assert s[11].tolist() == [-1, 0, 0, 0]   # the top carry is dropped


@pytest.mark.parametrize("which", ["128", "80"])
def test_layout_is_a_bijection_onto_the_operand(em, which):
    """(column k, word, plane) -> byte is one-to-one onto [0, bytes) over k < 4 N t, the nc x 128 padded words and the 4 planes;
    (i, j, u) is column 4 (i t + j) + u + 1, so the padding (columns = 0 mod 4, words past the row) shares no byte with the data;
    16 consecutive k of a column are 16 consecutive bytes at a 16-byte boundary."""
    t, nc, row = SETS[which]
    total = em.iyk_emul_ks_matrix_bytes(t, nc)
    kk = np.arange(4 * N * t, dtype=np.int32)
    assert total == len(kk) * nc * 128 * 4
    f = _offsets_k(em, t, kk, 0, 0)
    marks = np.zeros(total, dtype=np.uint8)
    for word in range(nc * 128):
        for plane in range(4):
            g = em.iyk_emul_ks_matrix_offset(t, 0, 0, 0, word, plane) - f[1]
            if word % 37 == 0 or word == nc * 128 - 1:   # the layout separates: byte(k, word, plane) = f(k) + g(word, plane)
                assert np.array_equal(_offsets_k(em, t, kk, word, plane), f + g)
            off = f + g
            assert off.min() >= 0 and off.max() < total and not marks[off].any()
            marks[off] = 1
    assert int(marks.sum(dtype=np.int64)) == total
    rng = np.random.default_rng(3)
    for i, j, u, word, plane in zip(rng.integers(0, N, 2000), rng.integers(0, t, 2000), rng.integers(0, 3, 2000),
                                    rng.integers(0, row, 2000), rng.integers(0, 4, 2000)):
        k = 4 * (int(i) * t + int(j)) + int(u) + 1
        assert em.iyk_emul_ks_matrix_offset(t, int(i), int(j), int(u), int(word), int(plane)) == f[k] + (
            em.iyk_emul_ks_matrix_offset(t, 0, 0, 0, int(word), int(plane)) - f[1])
    lead = f[::16]
    assert (lead % 16 == 0).all() and np.array_equal(f.reshape(-1, 16), lead[:, None] + np.arange(16))


def test_predicate(em):
    """IYK_HIP_KS_KERNEL=3: the matrix form at any batch size; unset: exactly from KS_MATRIX_MIN_JOBS on; 0 .. 2 keep their meaning;
    t = 5 (no instantiation) and a (t, nc) of neither parameter set never run it."""
    m = em.iyk_emul_ks_matrix_min_jobs()
    assert m > K.TABLE_MIN_JOBS + 1   # the suite's 4 097-gate default batches stay on the table
    for t, nc, _ in SETS.values():
        assert em.iyk_emul_ks_matrix_form(3, 1, t, nc) == 1 and em.iyk_emul_ks_matrix_form(3, 1 << 20, t, nc) == 1
        assert [em.iyk_emul_ks_matrix_form(-1, n, t, nc) for n in (1, m - 1, m, m + 1, 1 << 20)] == [0, 0, 1, 1, 1]
        for kind in (0, 1, 2):
            assert not any(em.iyk_emul_ks_matrix_form(kind, n, t, nc) for n in (1, m, 1 << 20))
    for kind in (-1, 3):
        assert em.iyk_emul_ks_matrix_form(kind, 1 << 20, 5, 5) == 0 and em.iyk_emul_ks_matrix_form(kind, 1 << 20, 7, 4) == 0
    assert em.iyk_emul_ks_matrix_gates(0) == 4 * em.iyk_emul_ks_matrix_gates(1) == 256


@pytest.mark.parametrize("t", [7, 8])
def test_numpy_restatement_of_the_product(em, t):
    """3 gates, 8 coefficients: the operand filled through the layout function from random rows (bytes 0x80 / 0x7F mixed in), the
    one-hot digit matrix read through the same function, plane products recombined with shifts and subtracted from (0, .., 0, b'),
    against the rows subtracted digit by digit as ks_words.digit_list decodes them."""
    rng = np.random.default_rng(40 + t)
    ni, words, gates = 8, 33, 3
    rows = rng.integers(0, 1 << 32, size=(ni, t, 3, words), dtype=np.uint32)
    rows[:, :, :, ::5] = rng.choice(np.array([0x80, 0x7F, 0xFF, 0x00], dtype=np.uint32), size=rows[:, :, :, ::5].shape + (4,)).dot(
        np.array([1, 1 << 8, 1 << 16, 1 << 24], dtype=np.uint32)).astype(np.uint32)
    D = rng.integers(0, 1 << (2 * t), size=(gates, ni))
    D[0, :2], D[1, 0], D[2, 1] = 0, (1 << 2 * t) - 1, 3
    a = np.stack([K.words_from_digits(D[g], rng.integers(0, 1 << (32 - 2 * t), size=ni, dtype=np.uint64), t) for g in range(gates)])
    b = rng.integers(0, 1 << 32, size=gates, dtype=np.uint32)
    want = np.zeros((gates, words), dtype=np.int64)
    want[:, words - 1] = b
    for g in range(gates):
        for j, dj in enumerate(K.digit_list(a[g], t)):
            for i in range(ni):
                if dj[i]:
                    want[g] -= rows[i, j, dj[i] - 1]
    want &= K.MASK32
    # operand bytes and one-hot columns, both addressed by the layout function (word group 0 and 1, the k-steps of 8 coefficients)
    planes = _planes(em, rows.ravel()).reshape(ni, t, 3, words, 4)
    mat = {}
    for i in range(ni):
        for j in range(t):
            for u in range(3):
                for w in range(words):
                    for p in range(4):
                        mat[em.iyk_emul_ks_matrix_offset(t, i, j, u, w, p)] = int(planes[i, j, u, w, p])
    assert len(mat) == ni * t * 3 * words * 4
    got = np.zeros((gates, words), dtype=np.int64)
    for g in range(gates):
        digits = K.digit_list(a[g], t)
        onehot = np.zeros(4 * ni * t, dtype=np.int64)
        for i in range(ni):
            for j in range(t):
                onehot[4 * (i * t + j) + digits[j][i]] = 1
        for w in range(words):
            acc = [sum(mat.get(int(o), 0) for o in _offsets_k(em, t, np.flatnonzero(onehot), w, p)) for p in range(4)]
            assert all(abs(x) < 1 << 21 for x in acc)
            got[g, w] = ((int(b[g]) if w == words - 1 else 0) - sum(acc[p] << (8 * p) for p in range(4))) & K.MASK32
    assert np.array_equal(got, want)
