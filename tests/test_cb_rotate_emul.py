"""CPU: the device math of the lvl0 -> lvl2 rotation (csrc/cb_rotate.hpp) run lane by lane by csrc/emul.cpp — the 64-point pass, the
N2 = 2048 transform, the digits, the key transform and whole rotation jobs — against direct evaluation mod P and against the numpy
restatement (tests/cb_rotate_ref.py), word for word."""
import ctypes

import numpy as np
import pytest

import cb_rotate_cases as cases
import cb_rotate_ref as ref

P = (1 << 64) - (1 << 32) + 1
_u64p = ctypes.POINTER(ctypes.c_uint64)


def _field(rng, n):
    x = rng.integers(0, 1 << 64, size=n, dtype=np.uint64)
    x[x >= np.uint64(P)] -= np.uint64(P)
    x[:4] = [0, 1, P - 1, P >> 1]
    return x


@pytest.mark.parametrize("inverse", [0, 1])
def test_ntt64_is_the_dft_with_root_8(inverse):
    x = _field(np.random.default_rng(5 + inverse), 64)
    out = np.zeros(64, dtype=np.uint64)
    cases.emul().iyk_emul_ntt64(x.ctypes.data_as(_u64p), inverse, out.ctypes.data_as(_u64p))
    root = pow(8, P - 2, P) if inverse else 8
    assert pow(8, 32, P) == P - 1   # 2^3 has order 64
    want = [sum(int(x[j]) * pow(root, j * k % 64, P) for j in range(64)) % P for k in range(64)]
    assert [int(v) for v in out] == want


def test_n2_transform_against_direct_evaluation_and_round_trip():
    rng = np.random.default_rng(9)
    x = _field(rng, ref.N2)
    X, back, psi = np.zeros(ref.N2, dtype=np.uint64), np.zeros(ref.N2, dtype=np.uint64), ctypes.c_uint64()
    cases.emul().iyk_emul_cb_ntt(x.ctypes.data_as(_u64p), 0, X.ctypes.data_as(_u64p), ctypes.byref(psi))
    psi = psi.value
    assert pow(psi, 64, P) == 8 and pow(psi, 2048, P) == P - 1
    pw = [1] * 4096
    for e in range(1, 4096):
        pw[e] = pw[e - 1] * psi % P
    xs = [int(v) for v in x]
    for k in list(range(0, 2048, 61)) + [1, 31, 32, 63, 64, 2047]:     # X[k] = sum_j x[j] psi^(j (2k+1)), O(N) each
        assert int(X[k]) == sum(xs[j] * pw[j * (2 * k + 1) % 4096] for j in range(2048)) % P, k
    cases.emul().iyk_emul_cb_ntt(X.ctypes.data_as(_u64p), 1, back.ctypes.data_as(_u64p), None)
    assert np.array_equal(back, x)


def test_digits_at_their_edges():
    words = cases.digit_edge_words()
    x = np.array([w for _, w in words.values()], dtype=np.uint64)
    got = np.zeros((len(x), 4), dtype=np.int32)
    assert cases.emul().iyk_emul_cb_digits(x.ctypes.data_as(_u64p), len(x), 4, 9, got.ctypes.data_as(ctypes.POINTER(ctypes.c_int32))) == 0
    for (name, (want, _)), g in zip(words.items(), got):
        assert list(g) == want, name
    rnd = np.random.default_rng(3).integers(0, 1 << 64, size=512, dtype=np.uint64)
    got = np.zeros((512, 4), dtype=np.int32)
    cases.emul().iyk_emul_cb_digits(rnd.ctypes.data_as(_u64p), 512, 4, 9, got.ctypes.data_as(ctypes.POINTER(ctypes.c_int32)))
    assert np.array_equal(got.T, ref.digits(rnd))
    assert cases.emul().iyk_emul_cb_digits(rnd.ctypes.data_as(_u64p), 1, 3, 9, got.ctypes.data_as(ctypes.POINTER(ctypes.c_int32))) == -1


@pytest.mark.parametrize("name", cases.CASES)
def test_emulated_rotation_word_for_word(name):
    bk, jobs = cases.case(name)
    ntt = cases.key_ntt(bk)
    want = cases.expected(name)
    for g, (w, sign, off, mu) in enumerate(jobs):
        got = cases.emul_rotate(w, sign, off, mu, ntt)
        bad = np.flatnonzero(got != want[g])
        assert bad.size == 0, (name, g, bad[:8])
    assert want.any()


def test_extreme_case_is_extreme():
    """every digit of the first step's b polynomial is -Bg/2 and every key half is 2^32 - 1: the sums the bound is about"""
    bk, jobs = cases.case("extreme-ones")
    w, sign, off, mu = jobs[0]
    lin = ref.linear(w, sign, off)
    abar, bbar = ref.modswitch(lin)
    assert abar[0] == ref.N2 and bbar == 0
    tv = np.full(ref.N2, mu, dtype=np.uint64)
    d = ref.digits(ref.mul_xr(tv, ref.N2) - tv)
    assert (d == -256).all() and (bk == np.uint64(ref.M64)).all()


def test_refused_arguments():
    bk, jobs = cases.case("uniform-n1")
    ntt = cases.key_ntt(bk)
    w = jobs[0][0]
    for l2, bg, sign in ((3, 9, 1), (4, 10, 1), (4, 9, 0), (4, 9, 2)):
        with pytest.raises(ValueError):
            cases.emul_rotate(w, sign, 0, 1, ntt, l2, bg)


@pytest.mark.slow
@pytest.mark.parametrize("name", ["128", "80"])
def test_full_size_noise_measured(name, request):
    """n = 636 / 500, a real key of alpha2 = 2^-44, the l rotations of one address bit of each value through the emulation: the worst
    phase error against mu_r, printed (DESIGN.md §6d has the table).  The assertion is the decryption itself: |error| < mu_r."""
    from iyokan_amd import client

    keys = request.getfixturevalue("keys" + name)
    p = keys.params
    s2 = client.keygen_lvl2(ref.N2, seed=31)
    ntt = cases.key_ntt(client.bk2_rows(keys, s2, 4, 9, cases.ALPHA2, seed=32))
    ct = client.encrypt_bits(keys, [0, 1], seed=33)
    for r in range(p.l):
        mu = ref.mu_of(r, p.Bgbit)
        worst = 0
        for bit in (0, 1):
            ph = int(client.tlwe2_phases(s2, cases.emul_rotate(ct[bit], 1, 0, mu, ntt))[0])
            err = (ph - bit * 2 * mu + (1 << 63)) % (1 << 64) - (1 << 63)
            worst = max(worst, abs(err))
        print(f"set {name} r {r}: worst |phase error| 2^{np.log2(max(worst, 1)):.2f}, mu_r 2^{np.log2(mu):.0f}, margin {np.log2(mu / max(worst, 1)):.2f} bits")
        assert worst < mu
