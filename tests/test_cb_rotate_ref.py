"""CPU: the restatement of the lvl0 -> lvl2 rotation (tests/cb_rotate_ref.py) holds what the definition promises, and the words of a
rotation under a real key (client.bk2_rows) decrypt to the gadget digits client.encrypt_cb_digits fakes."""
import numpy as np
import pytest

import cb_rotate_cases as cases
import cb_rotate_ref as ref
import cmux_ref
import privks_ref
from iyokan_amd import client
from iyokan_amd.params import params_128bit, params_80bit


def test_digits_rebuild_the_word():
    rng = np.random.default_rng(1)
    x = rng.integers(0, 1 << 64, size=4096, dtype=np.uint64)
    d = ref.digits(x)
    assert d.min() >= -256 and d.max() <= 255
    back = sum(d[j].astype(np.int64).view(np.uint64) << np.uint64(64 - (j + 1) * 9) for j in range(4))
    err = (x - back).view(np.int64)
    assert np.abs(err).max() <= 1 << 27   # half of the last digit's weight


def test_digit_edges():
    for name, (want, word) in cases.digit_edge_words().items():
        assert list(ref.digits(np.array([word], dtype=np.uint64))[:, 0]) == want, name


def test_negacyclic_product_is_schoolbook():
    rng = np.random.default_rng(2)
    n = 16
    d = rng.integers(-256, 256, size=n)
    q = rng.integers(0, 1 << 64, size=n, dtype=np.uint64)
    want = [0] * n
    for i in range(n):
        for j in range(n):
            k, s = (i + j) % n, -1 if i + j >= n else 1
            want[k] = (want[k] + s * int(d[i]) * int(q[j])) % (1 << 64)
    assert [int(v) for v in ref.negacyclic_product(d, q)] == want


def test_mul_xr():
    p = np.arange(1, 9, dtype=np.uint64)
    assert list(ref.mul_xr(p, 0)) == list(p)
    assert list(ref.mul_xr(p, 8)) == list(np.uint64(0) - p)
    assert list(ref.mul_xr(p, 1)) == [(1 << 64) - 8] + list(range(1, 8))
    assert list(ref.mul_xr(p, 15)) == list(range(2, 9)) + [(1 << 64) - 1]   # X^15 = -X^7


def test_windows_of_bk2_rows_give_the_whole_key():
    ks, s2, bk = cases.real_case()
    a = client.bk2_rows(ks, s2, 4, 9, cases.ALPHA2, first_step=0, step_count=1, seed=7, nthreads=1)
    b = client.bk2_rows(ks, s2, 4, 9, cases.ALPHA2, first_step=1, seed=7, nthreads=3)
    assert np.array_equal(np.concatenate([a, b]), bk) and bk.shape == (cases.REAL_N, 8, 2, 2048)
    assert client.bk2_rows(ks, s2, 4, 9, cases.ALPHA2, first_step=cases.REAL_N, seed=7).shape[0] == 0
    with pytest.raises(ValueError):
        client.bk2_rows(ks, s2, 4, 9, cases.ALPHA2, first_step=cases.REAL_N + 1, seed=7)
    # every row is a lvl2 TRLWE of s0[i] 2^(64 - (j+1) 9) on polynomial c: the phase b - a s2 at coefficient 0, and zero elsewhere
    for i in (0, cases.REAL_N - 1):
        for r in (0, 3, 4, 7):
            a_, b_ = bk[i, r]
            ph = b_.copy()
            for t in np.flatnonzero(s2):
                ph -= ref.mul_xr(a_, int(t))
            c, j = divmod(r, 4)
            msg = np.zeros(2048, dtype=np.uint64)
            if c == 1:
                msg[0] = np.uint64(int(ks.s0[i]) << (64 - (j + 1) * 9))
            else:   # message on a: phase = -s2(X) * m
                m = np.zeros(2048, dtype=np.uint64)
                m[0] = np.uint64(int(ks.s0[i]) << (64 - (j + 1) * 9))
                for t in np.flatnonzero(s2):
                    msg -= ref.mul_xr(m, int(t))
            assert np.abs((ph - msg).view(np.int64)).max() < 1 << 26, (i, r)   # alpha2 = 2^-44: noise around 2^20


@pytest.mark.parametrize("p", [params_128bit(), params_80bit()], ids=["128", "80"])
def test_real_key_outputs_decrypt(p):
    """n = 8, alpha2 = 2^-44: the l rotations of an address bit decrypt to bit * 2 mu_r under tlwe2_phases, for both signs, and the
    emulation of the kernel gives the same words from the same key"""
    ks, s2, bk = cases.real_case()
    l, bg = int(p.l), int(p.Bgbit)
    bits = [1, 0, 1]
    ntt = cases.key_ntt(bk)
    ct = cases.encrypt_lvl0(ks.s0, bits, seed=3)
    tl = np.zeros((2, len(bits) * l, ref.N2 + 1), dtype=np.uint64)
    for si, sign in enumerate((1, -1)):
        for b, bit in enumerate(bits):
            for r in range(l):
                mu = ref.mu_of(r, bg)
                tl[si, b * l + r] = ref.rotate_job(ct[b], sign, 0, mu, bk)
                assert np.array_equal(cases.emul_rotate(ct[b], sign, 0, mu, ntt), tl[si, b * l + r]), (sign, b, r)
                want = (bit if sign == 1 else 1 - bit) * 2 * mu
                ph = int(client.tlwe2_phases(s2, tl[si, b * l + r])[0])
                err = (ph - want + (1 << 63)) % (1 << 64) - (1 << 63)
                assert abs(err) < mu >> 3, (sign, b, r, err)   # 3 bits under mu


def _switch_windowed(keys, s2, tlwes, jobs, t, bb, seed, window=16384):
    """privks_ref's R_c = - (sum of the key rows the digits select) for jobs (TLWE index, c), with the real key made in windows of rows:
    the 2.35 GB key of n_in = 2048 never exists, every window is dropped once its selected rows are added up"""
    total = client.privks_key_total_rows(keys.params, s2.size, t, bb)
    idx = [np.sort(privks_ref.selected_rows(tlwes[i], c, t, bb)) for i, c in jobs]
    acc = np.zeros((len(jobs), 2 * keys.params.N), dtype=np.int64)
    for first in range(0, total, window):
        rows = client.privks_key_rows(keys, s2, t, bb, first_row=first, row_count=min(window, total - first), seed=seed)
        for g, ix in enumerate(idx):
            sel = ix[np.searchsorted(ix, first):np.searchsorted(ix, first + rows.shape[0])] - first
            acc[g] += rows[sel].sum(axis=0, dtype=np.int64)
    return ((-acc) & 0xFFFFFFFF).astype(np.uint32)


@pytest.mark.parametrize("name", ["128", "80"])
def test_rotation_outputs_address_a_rom(name, request):
    """The purpose of the feature, on the CPU: the rotation's words under a real key (n = 8, alpha2 = 2^-44) go through the private key
    switch (a real key of n_in = 2048, t = 10, basebit = 3, restated by privks_ref's row selection) and the selectors they give read a
    3-bit ROM through cmux_ref: the addressed word for sign = +1, the word at the complemented address for sign = -1."""
    keys = request.getfixturevalue("keys" + name)
    p = keys.params
    ks, s2, bk = cases.real_case()
    l, bg, A = int(p.l), int(p.Bgbit), 3
    bits = [1, 0, 1]
    ct = cases.encrypt_lvl0(ks.s0, bits, seed=3)
    tl = np.stack([ref.rotate_job(ct[b], sign, 0, ref.mu_of(r, bg), bk) for sign in (1, -1) for b in range(A) for r in range(l)])
    jobs = [(i, c) for i in range(2 * A * l) for c in range(p.k + 1)]
    rows = _switch_windowed(keys, s2, tl, jobs, 10, 3, seed=41).reshape(2, A, l, p.k + 1, 2, p.N)
    # every selector row is a lvl1 TRLWE of f_c * (phase of its lvl2 TLWE) / 2^32, f_1 = 1, f_0 = -s1(X) (privks.hpp): key noise of
    # (n_in + 1) t rows of deviation alpha1 at 6.5 sigma, the cut of every word to t basebit = 30 bits (at most 2 units per word), 2 for
    # the roundings of this comparison
    sigma_row = np.sqrt((ref.N2 + 1) * 10) * p.alpha1 * 2.0 ** 32
    bound = 6.5 * sigma_row + 2 * (ref.N2 + 1) + 2
    ph2 = client.tlwe2_phases(s2, tl).reshape(2, A, l)
    s1 = keys.s1.astype(np.int64)
    for si in range(2):
        for b in range(A):
            for r in range(l):
                m = (int(ph2[si, b, r]) + (1 << 31)) >> 32
                ph = client.trlwe_phases(keys, rows[si, b, r].reshape(p.k + 1, 2 * p.N)).astype(np.int64)
                want = np.zeros((2, p.N), dtype=np.int64)
                want[0] = -m * s1
                want[1, 0] = m
                d = (ph - want + (1 << 31)) % (1 << 32) - (1 << 31)
                assert np.abs(d).max() < bound, (name, si, b, r, np.abs(d).max(), bound)
    # the read.  Its decryption is asserted at the 128-bit set: l = 3, Bgbit = 6 with t = 10, basebit = 3 are TFHEpp's own circuit
    # bootstrapping parameters, the chain the reference runs.  The 80-bit set (l = 2, Bgbit = 10) multiplies the selector rows' noise
    # by digits 16 times larger: with a key of n_in = 2048 the read does not decrypt (DESIGN.md 6c has 2.17 bits left at n_in = 64, and
    # sqrt(2049 / 65) takes 2.5), whatever made the lvl2 TLWEs.  There the selector rows above are the assertion and the wrong bits of
    # the read are printed.
    content = np.random.default_rng(42).integers(0, 2, size=(1 << A, p.N)).astype(np.uint8)
    data = client.encrypt_rom_trlwe(keys, content.ravel(), seed=43)
    for si, addr in enumerate((0b101, 0b010)):
        trgsw = rows[si].transpose(0, 2, 1, 3, 4).reshape(A, (p.k + 1) * l, 2, p.N)      # row c l + r of every bit's selector
        word = cmux_ref.rom_read(p, data, trgsw, A, int(p.N).bit_length() - 1)
        wrong = int((client.decrypt_rom_trlwe(keys, word) != content[addr]).sum())
        print(f"set {name} sign {(1, -1)[si]}: {wrong} of {p.N} bits of the word read wrong")
        if name == "128":
            assert wrong == 0, (name, si, wrong)
