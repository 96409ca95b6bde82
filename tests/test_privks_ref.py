"""CPU: the private functional key switch lvl2 -> lvl1 restated in numpy (tests/privks_ref.py) against real keys from the client
library — phases, the orientation of the selector rows against client.encrypt_trgsw, a CMUX driven by a restated selector — the digit
edge words, the library's own digit function, dispatch.hpp's split of the i range, and the noise of the end-to-end case that
test_gpu_privks runs on the GPU."""
import ctypes
import os

import numpy as np
import pytest

import cmux_ref
import privks_cases as cases
import privks_ref as ref
from iyokan_amd import client

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
N_IN = 16
T, BB = cases.T_CB, cases.BASEBIT_CB


def _signed(x):
    return np.asarray(x, dtype=np.uint32).view(np.int32).astype(np.int64)


@pytest.fixture(scope="module", params=["128", "80"])
def small(request):
    keys = request.getfixturevalue("keys" + request.param)
    s2 = client.keygen_lvl2(N_IN, seed=3)
    K = client.privks_key_rows(keys, s2, T, BB, seed=4)
    return keys, s2, K


def _noise_bound(p, rows):
    """6.5 standard deviations of a sum of `rows` key rows of noise alpha1, in units of 2^-32, plus the rounding of the input words:
    every word is cut to t basebit = 30 bits, at most 2^-31 off each, (N_IN + 1) words, 2^-32 units -> 2 (N_IN + 1); + 2 for the
    truncation of the expectation itself."""
    return 6.5 * np.sqrt(rows) * p.alpha1 * 2.0 ** 32 + 2 * (N_IN + 1) + 2


def test_key_windows_and_threads(small):
    keys, s2, K = small
    total = client.privks_key_total_rows(keys.params, N_IN, T, BB)
    assert K.shape == (total, 2 * keys.params.N) and total == 2 * 17 * 10 * 7
    assert np.array_equal(client.privks_key_rows(keys, s2, T, BB, 100, 50, seed=4, nthreads=1), K[100:150])
    assert np.array_equal(client.privks_key_rows(keys, s2, T, BB, total - 3, 3, seed=4, nthreads=3), K[-3:])
    assert not np.array_equal(K[0], K[1])
    with pytest.raises(ValueError):
        client.privks_key_rows(keys, s2, T, BB, total, 1, seed=4)
    with pytest.raises(ValueError):
        client.privks_key_rows(keys, s2, 8, 8, seed=4)   # basebit t = 64


def test_tlwe2_round_trip():
    s2 = client.keygen_lvl2(N_IN, seed=3)
    assert set(np.unique(s2)) <= {0, 1} and 0 < s2.sum() < N_IN
    msgs = np.array([0, 1 << 63, 1 << 58, (1 << 64) - (1 << 40)], dtype=np.uint64)
    ct = client.encrypt_tlwe2(s2, msgs, cases.ALPHA2, seed=5)
    err = (client.tlwe2_phases(s2, ct) - msgs).view(np.int64)
    assert np.abs(err).max() < 6.5 * cases.ALPHA2 * 2.0 ** 64 and np.abs(err).max() > 0


def test_phase_is_fc_times_phase2(small):
    """phase(R_c) = f_c phase2 / 2^32: f_1 = 1 (coefficient 0), f_0 = -s1(X)"""
    keys, s2, K = small
    p = keys.params
    rng = np.random.default_rng(6)
    msgs = np.concatenate([rng.integers(0, 1 << 64, size=6, dtype=np.uint64), np.array([0, 1 << 63, 1 << 58], dtype=np.uint64)])
    ct = client.encrypt_tlwe2(s2, msgs, cases.ALPHA2, seed=7)
    ph2 = client.tlwe2_phases(s2, ct)
    worst = 0
    for g in range(len(msgs)):
        m = int(ph2[g]) >> 32
        for c in (0, 1):
            row = ref.switch(ct[g], c, T, BB, ref.key_rows_of(K))
            ph = _signed(client.trlwe_phases(keys, row)[0])
            want = np.zeros(p.N, dtype=np.int64)
            if c == 1:
                want[0] = m
            else:
                want = -m * keys.s1.astype(np.int64)
            err = _signed(((ph - want) & ref.M32).astype(np.uint32))
            worst = max(worst, int(np.abs(err).max()))
    rows = (N_IN + 1) * T
    print(f"worst phase error {worst} = 2^{np.log2(max(worst, 1)):.1f}, bound {_noise_bound(p, rows):.0f}")
    assert worst < _noise_bound(p, rows)


def test_rows_decrypt_like_encrypt_trgsw(small):
    """orientation: the rows made from the l lvl2 TLWEs of a bit have the phases of client.encrypt_trgsw's rows of that bit"""
    keys, s2, K = small
    p = keys.params
    for bit in (0, 1):
        tl = client.encrypt_cb_digits(s2, [bit], p, cases.ALPHA2, seed=8 + bit)
        got = ref.selector_rows(tl, T, BB, ref.key_rows_of(K), p.l).reshape(p.trgsw_rows, 2 * p.N)
        want = client.encrypt_trgsw(keys, [bit], seed=10 + bit).reshape(p.trgsw_rows, 2 * p.N)
        d = _signed(client.trlwe_phases(keys, got) - client.trlwe_phases(keys, want))
        assert np.abs(d).max() < _noise_bound(p, (N_IN + 1) * T + 1), (bit, np.abs(d).max())
        if bit:   # and the rows are not noise: row c l + r carries 2^(32 - (r+1) Bgbit) on polynomial c
            ph = _signed(client.trlwe_phases(keys, got))
            for r in range(p.l):
                assert abs(ph[p.l + r, 0] - (1 << (32 - (r + 1) * p.Bgbit))) < _noise_bound(p, (N_IN + 1) * T)


def test_restated_selector_drives_cmux(small):
    """a selector of 1 picks in1, a selector of 0 picks in0"""
    keys, s2, K = small
    p = keys.params
    tl = client.encrypt_cb_digits(s2, [0, 1], p, cases.ALPHA2, seed=12).reshape(2, p.l, N_IN + 1)
    trgsw = np.stack([ref.selector_rows(tl[b], T, BB, ref.key_rows_of(K), p.l) for b in range(2)])
    bits = np.random.default_rng(13).integers(0, 2, size=(2, p.N)).astype(np.uint8)
    Tr = np.concatenate([client.encrypt_rom_trlwe(keys, bits.ravel(), seed=14), np.zeros((1, 2 * p.N), dtype=np.uint32)])
    for b in range(2):
        out = cmux_ref.cmux(p, Tr, trgsw, (b, 0, 1, 0, 2))
        assert np.array_equal(client.decrypt_rom_trlwe(keys, out), bits[b]), b


def _emul():
    em = ctypes.CDLL(os.path.join(ROOT, "iyokan_amd", "lib", "libiyk_emul.so"))
    em.iyk_emul_privks_plan.argtypes = [ctypes.c_int] * 3 + [ctypes.POINTER(ctypes.c_int)]
    em.iyk_emul_privks_plan.restype = None
    em.iyk_emul_privks_digits.argtypes = [ctypes.POINTER(ctypes.c_uint64), ctypes.c_int, ctypes.c_uint32, ctypes.c_uint32,
                                          ctypes.POINTER(ctypes.c_uint32)]
    em.iyk_emul_privks_digits.restype = None
    return em


@pytest.mark.parametrize("t,bb", [(10, 3), (4, 5), (7, 9 - 1), (63, 1)])
def test_digit_edge_words(t, bb):
    nb = (1 << bb) - 1
    edges = ref.edge_words(t, bb)
    for name, (w, every) in edges.items():
        d = ref.digits(np.array([w], dtype=np.uint64), t, bb)[0]
        if every is not None:
            assert np.all(d == every), (name, d)
        else:
            assert list(d) == [0] * (t - 1) + [1], (name, d)
    # the zero word and the word that wraps select no row: the zero TRLWE
    K = np.random.default_rng(1).integers(0, 1 << 32, size=(2 * 3 * t * nb, 64), dtype=np.uint64).astype(np.uint32)
    for w in (0, edges["smallest that wraps to zero"][0]):
        assert not ref.switch(np.array([w, w, w], dtype=np.uint64), 1, t, bb, ref.key_rows_of(K)).any()
    # all digits at their largest: every (i, j) adds its last row
    full = ref.switch(np.array([edges["largest without wrap"][0]] * 3, dtype=np.uint64), 0, t, bb, ref.key_rows_of(K))
    assert np.array_equal(full, (-(K[: 3 * t * nb].reshape(3 * t, nb, 64)[:, nb - 1].sum(axis=0, dtype=np.int64)) & ref.M32).astype(np.uint32))
    # the library's digit function (csrc/privks.hpp, what privks_kernel runs) on the edges, their neighbours and uniform words
    words = [w for w, _ in edges.values()] + [(w + dw) & ref.M64 for w, _ in edges.values() for dw in (-1, 1)]
    words = np.concatenate([np.array(words, dtype=np.uint64), np.random.default_rng(2).integers(0, 1 << 64, size=200, dtype=np.uint64)])
    got = np.zeros((len(words), t), dtype=np.uint32)
    _emul().iyk_emul_privks_digits(words.ctypes.data_as(ctypes.POINTER(ctypes.c_uint64)), len(words), t, bb,
                                   got.ctypes.data_as(ctypes.POINTER(ctypes.c_uint32)))
    assert np.array_equal(got, ref.digits(words, t, bb))


@pytest.mark.parametrize("n_words", [1, 2, 65, 2049])
def test_split_covers_every_i_once(n_words):
    em = _emul()
    out = (ctypes.c_int * 2)()
    seen = set()
    for cus in (1, 8, 256, 304):
        for njobs in list(range(1, 70)) + [255, 256, 257, 1024, 1025, 5000, 1 << 20]:
            em.iyk_emul_privks_plan(njobs, n_words, cus, out)
            splits, per = out[0], out[1]
            assert 1 <= splits <= n_words and per >= 1
            owner = np.zeros(n_words, dtype=np.int64)
            for s in range(splits):
                lo, hi = s * per, min((s + 1) * per, n_words)
                assert lo < hi, (njobs, cus, s)   # no empty split
                owner[lo:hi] += 1
            assert np.all(owner == 1), (njobs, cus)
            assert njobs * splits < 1 << 31
            seen.add(splits)
    assert 1 in seen and (n_words == 1 or max(seen) > 1)   # both ends of what the function can return were walked


@pytest.mark.parametrize("name", ["128", "80"])
def test_end_to_end_noise_measured(name, request):
    """The end-to-end case (n_in = 64, a real key of noise alpha1, t = 10, basebit = 3, a ROM of 8 rows read at all 8 addresses through
    selectors made from lvl2 TLWEs), on the CPU: selectors restated from the lvl2 TLWEs of every address, the ROM read through cmux_ref's
    exact CMUX.  Every coefficient of every word must decrypt; the worst distance of a result phase from +-mu is printed.

    Measured: 33 866 280 = 2^25.01 (128-bit set), 59 745 644 = 2^25.83 (80-bit set) against mu / 2 = 2^28: 2.99 and 2.17 bits of margin,
    LESS than the 3 bits asked for before the case may be asserted at decrypt level on the GPU.  The figures are the same to the last
    digit with lvl2 input noise 0 instead of 2^-44: the error is the key rows' (about 570 rows of noise alpha1 summed into every selector
    row, 2^-20 against a fresh selector's 2^-25), so lowering the input noise is no remedy.  Hence test_gpu_privks compares this case
    word for word with the restatement and asserts no decryption there; DESIGN.md section 6c has the figures."""
    keys = request.getfixturevalue("keys" + name)
    p = keys.params
    case = cases.e2e_case(name, keys)
    mu = int(p.mu)
    worst = 0
    for addr in range(1 << cases.E2E_ADDR_WIDTH):
        res = cases.e2e_reference_row(case, p, addr)
        ph = _signed(client.trlwe_phases(keys, res)[0])
        want = np.where(case["content"][addr] == 1, mu, -mu)
        worst = max(worst, int(np.abs(ph - want).max()))
        assert np.array_equal((ph > 0).astype(np.uint8), case["content"][addr]), addr
    print(f"set {name}: worst phase error {worst} = 2^{np.log2(worst):.2f}; bound mu/2 = 2^28")
    assert worst < 1 << 28
