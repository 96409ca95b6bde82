"""CPU: the FP64 FFT form of the lvl0 -> lvl2 rotation (csrc/cb_rotate_fft.hpp, csrc/fft1024.hpp) run lane by lane by csrc/emul.cpp —
the split of a key word into signed 16-bit quarters and the 64-bit recombination on their own, the 1024-point transform against a
direct long double evaluation, whole rotation jobs word for word against the numpy restatement (tests/cb_rotate_ref.py) and against
the latency form's emulation, the rounding distance against the bound proven in DESIGN.md §2b, and dispatch::cb_fft_grid."""
import ctypes
import math

import numpy as np
import pytest

import cb_rotate_cases as base
import cb_rotate_fft_cases as cases
import cb_rotate_ref as ref
from test_cb_rotate_lat_emul import emul_rotate_lat

_u64p, _i32p, _f64p = ctypes.POINTER(ctypes.c_uint64), ctypes.POINTER(ctypes.c_int32), ctypes.POINTER(ctypes.c_double)
M64 = ref.M64


def quarters(words):
    w = np.array(words, dtype=np.uint64)
    q = np.zeros((w.size, 4), dtype=np.int32)
    cases.emul().iyk_emul_cb_key_quarters(w.ctypes.data_as(_u64p), w.size, q.ctypes.data_as(_i32p))
    return q


def recombine(z):
    z = np.ascontiguousarray(z, dtype=np.float64).reshape(-1, 4)
    out = np.zeros(z.shape[0], dtype=np.uint64)
    cases.emul().iyk_emul_cb_recombine(z.ctypes.data_as(_f64p), z.shape[0], out.ctypes.data_as(_u64p))
    return out


CHOSEN_WORDS = [0, 1, M64, 0x7FFF, 0x8000, 0xFFFF, 0x10000, 0x7FFF7FFF7FFF7FFF, 0x8000000000000000, 0x7FFFFFFFFFFFFFFF,
                cases.WORD_MIN, cases.WORD_ALL_MIN] + cases.CARRY_WORDS


def test_the_split_into_signed_quarters():
    q = quarters(CHOSEN_WORDS)
    assert q.min() >= -(1 << 15) and q.max() < (1 << 15)
    for w, row in zip(CHOSEN_WORDS, q):
        assert sum(int(v) << (16 * j) for j, v in enumerate(row)) & M64 == w, hex(w)
    by_word = {w: [int(v) for v in row] for w, row in zip(CHOSEN_WORDS, q)}
    assert by_word[cases.WORD_ALL_MIN] == [-(1 << 15)] * 4                                   # the norm bound's extreme
    assert by_word[cases.WORD_ALL_MAX] == [32767] * 4                                        # quarters-alt's other word
    assert by_word[cases.WORD_MIN] ==[-(1 << 15), -32767, -32767, -32767]                   # each carry raises the next quarter
    assert by_word[0xFFFFFFFFFFFF8000] == [-(1 << 15), 0, 0, 0]                              # the carry runs through all and out of the top
    assert by_word[0x7FFF800080008000] == [-(1 << 15), -32767, -32767, -(1 << 15)]           # ... into q3, which wraps to its minimum
    assert by_word[0x0000FFFF80007FFF] == [32767, -(1 << 15), 0, 1]                          # 0xFFFF + carry = 2^16: q2 = 0, q3 = 1
    rng = np.random.default_rng(3)
    words = rng.integers(0, 1 << 64, size=4096, dtype=np.uint64)
    q = quarters(words).astype(object)
    assert [(int(a) + (int(b) << 16) + (int(c) << 32) + (int(d) << 48)) & M64 for a, b, c, d in q] == [int(w) for w in words]


def test_the_recombination_takes_signed_sums():
    lim = 1 << 37                                                      # |R_j| <= 2^37
    rows = [(0, 0, 0, 0), (1, 1, 1, 1), (-1, 0, 0, 0), (0, 0, -1, 0), (0, 0, 0, -1), (lim, -lim, lim, -lim), (-lim, lim, -lim, lim),
            (-(1 << 32), 0, 0, 0), ((1 << 32) + 5, -(1 << 33) - 7, (1 << 36) + 1, -3), (lim - 1, lim - 1, lim - 1, lim - 1)]
    rng = np.random.default_rng(4)
    rows += [tuple(int(v) for v in rng.integers(-lim, lim, size=4)) for _ in range(200)]
    want = [(r0 + (r1 << 16) + (r2 << 32) + (r3 << 48)) & M64 for r0, r1, r2, r3 in rows]
    assert [int(v) for v in recombine(np.array(rows, dtype=np.float64))] == want
    # the rounding: a quarter of a unit either side of an integer, of either sign
    nudged = np.array(rows, dtype=np.float64) + np.where(np.arange(4 * len(rows)).reshape(-1, 4) % 2 == 0, 0.25, -0.25)
    assert [int(v) for v in recombine(nudged)] == want


def _direct(z, inverse):
    """A[k] = sum_j z[j] psi^j W^(jk) (forward) or psi^-j sum_k C[k] W^(-jk) (inverse, unscaled) in long double"""
    n = z.size
    idx = np.arange(n)
    ld = np.longdouble
    pi = ld(math.pi) + ld(1.2246467991473532e-16)                         # pi to long double precision
    ang = lambda e, den: (pi * e.astype(ld)) / ld(den)
    zr, zi = z.real.astype(ld), z.imag.astype(ld)
    out_r, out_i = np.zeros(n, dtype=ld), np.zeros(n, dtype=ld)
    for k in range(n):
        e = (idx * (4 * k + 1)) % 4096 if not inverse else (-(k * (4 * idx + 1))) % 4096    # exponent of psi = exp(i pi / 2048)
        c, s = np.cos(ang(e, 2048)), np.sin(ang(e, 2048))
        out_r[k], out_i[k] = (zr * c - zi * s).sum(), (zr * s + zi * c).sum()
    return out_r, out_i


@pytest.mark.parametrize("inverse", [0, 1])
def test_fft1024_against_direct_long_double_evaluation(inverse):
    rng = np.random.default_rng(21 + inverse)
    z = rng.integers(-256, 256, size=1024).astype(np.float64) + 1j * rng.integers(-256, 256, size=1024).astype(np.float64)
    z[:3] = [256 + 256j, -256, 255j]
    buf = np.ascontiguousarray(np.stack([z.real, z.imag], axis=1))
    out = np.zeros_like(buf)
    cases.emul().iyk_emul_fft1024(buf.ctypes.data_as(_f64p), inverse, out.ctypes.data_as(_f64p))
    want_r, want_i = _direct(z, inverse)
    err = math.sqrt(float(((out[:, 0] - want_r) ** 2 + (out[:, 1] - want_i) ** 2).sum()))
    norm = math.sqrt(float((want_r ** 2 + want_i ** 2).sum()))
    # Lemma 1 of DESIGN.md §2b for this network: rho_F <= 40.2 eps in l2; the long double reference adds ~2^-60 of its own
    print(f"fft1024 inverse={inverse}: l2-relative error {err / norm:.3e} = {err / norm * 2 ** 53:.2f} eps")
    assert err <= 40.2 * 2.0 ** -53 * norm + 2.0 ** -58 * norm
    assert norm > 0


def test_fft1024_round_trip_is_1024_times_the_input():
    rng = np.random.default_rng(23)
    z = np.ascontiguousarray(rng.integers(-(1 << 15), 1 << 15, size=(1024, 2)).astype(np.float64))
    spec, back = np.zeros_like(z), np.zeros_like(z)
    cases.emul().iyk_emul_fft1024(z.ctypes.data_as(_f64p), 0, spec.ctypes.data_as(_f64p))
    cases.emul().iyk_emul_fft1024(spec.ctypes.data_as(_f64p), 1, back.ctypes.data_as(_f64p))
    assert np.array_equal(np.rint(back / 1024.0), z) and np.abs(back / 1024.0 - z).max() < 2.0 ** -20


def test_key_spectra_carry_the_scale_once():
    """a key whose every word is 1: quarter 0 is the polynomial 1 + X + ..., quarters 1 .. 3 are zero; position 0 of a spectrum is
    frequency 0, and |A[0]| of the all-ones polynomial, by the closed form of the geometric sum, is 1 / sin(pi / 4096) — over 1024"""
    bk = np.ones((1, 2 * cases.L2, 2, cases.N2), dtype=np.uint64)
    key = cases.key_fft(bk)
    assert not key[:, 1:].any() and key[:, 0].any()
    a0 = complex(key[0, 0, 0, 0, 0, 0], key[0, 0, 0, 0, 0, 1])
    assert abs(abs(a0) * 1024.0 - 1.0 / math.sin(math.pi / 4096)) < 1e-9 * 1304


@pytest.mark.parametrize("name", cases.CASES)
def test_emulated_fft_form_word_for_word(name):
    bk, jobs = cases.case(name)
    fftkey, ntt = cases.key_fft(bk), base.key_ntt(bk)
    want = cases.expected(name)
    cases.round_error(reset=True)
    for g, (w, sign, off, mu) in enumerate(jobs):
        got = cases.emul_rotate_fft(w, sign, off, mu, fftkey)
        bad = np.flatnonzero(got != want[g])
        assert bad.size == 0, (name, g, bad[:8])
        assert np.array_equal(got, emul_rotate_lat(w, sign, off, mu, ntt)), (name, g)
    assert want.any()
    worst = cases.round_error(reset=True)
    print(f"{name}: largest |z - rint(z)| = {worst:.3e} = 2^{math.log2(worst) if worst else float('-inf'):.1f}")
    assert worst <= cases.PROVEN_BOUND


def test_case_tables_hold_sign_offset_and_both_sides_of_the_modswitch_threshold():
    """A guard on the case TABLES only: it runs none of the code under test (test_emulated_fft_form_word_for_word does, on these
    cases).  Said here so that dropping one from the tables is noticed: sign = -1 and off != 0 (uniform-n*, the split cases' second
    job), a rounded either side of (7 << 20) + 2^19 and at the wrap (threshold)"""
    assert any(s == -1 and off != 0 for n in ("uniform-n1", "uniform-n2", "uniform-n5") + tuple(cases.SPLIT_CASES) for _, s, off, _ in cases.case(n)[1])
    ws = {int(w[0]) for w, _, _, _ in cases.case("threshold")[1]}
    assert {(7 << 20) + (1 << 19) - 1, 0xFFF7FFFF} <= ws
    assert {int(w[1]) for w, _, _, _ in cases.case("threshold")[1]} >= {(7 << 20) + (1 << 19), 0xFFF80000}


def test_refused_arguments():
    bk, jobs = cases.case("uniform-n1")
    fftkey = cases.key_fft(bk)
    w = jobs[0][0]
    for l2, bg, sign in ((3, 9, 1), (4, 10, 1), (4, 9, 0), (4, 9, 2)):
        with pytest.raises(ValueError):
            cases.emul_rotate_fft(w, sign, 0, 1, fftkey, l2, bg)


@pytest.mark.parametrize("cus", [256, 304, 7])
def test_grid_rule(cus):
    grid = cases.emul().iyk_emul_cb_fft_grid
    for count in (1, 2, cus - 1, cus, cus + 1, 2 * cus + 1, 1 << 40):
        assert grid(count, cus) == min(count, cus), count
    assert grid(0, cus) == 0 and grid(-1, cus) == 0 and grid(5, 0) == 0


def test_known_forms():
    known = cases.emul().iyk_emul_bk2_form_known
    assert [known(f) for f in (-1, 0, 1, 2, 3, 255)] == [0, 1, 1, 0, 0, 0]
