"""cmux_fft.hpp's phase functions, run lane by lane on the CPU (csrc/emul.cpp: emu_cmux_fft), against the exact reference of
tests/cmux_ref.py — numpy differences, numpy_tfhe.decompose digits, the oracle's exact negacyclic product on the torus-domain TRGSW.
Equality is word for word on both parameter sets."""
import ctypes

import numpy as np
import pytest

import cmux_ref
from iyokan_amd import client

SETS = ["128", "80"]


@pytest.fixture(scope="module")
def em(built):
    return cmux_ref.emul()


@pytest.fixture(scope="module", params=SETS)
def case(request, em):
    """One store of selectors and TRLWE rows per parameter set, and the reference's product anchored once."""
    keys = request.getfixturevalue("keys" + request.param)
    p = keys.params
    rng = np.random.default_rng(2024)
    fresh = client.encrypt_trgsw(keys, [0, 1], seed=11)
    trgsw = np.stack([
        fresh[0], fresh[1],
        np.zeros_like(fresh[0]),                                              # 2: noise-free zero
        rng.integers(0, 1 << 32, size=fresh[0].shape, dtype=np.uint64).astype(np.uint32),   # 3: uniform words
        cmux_ref.worst_case_trgsw(p, 0x7FFF7FFF), cmux_ref.worst_case_trgsw(p, 0x80008000),   # 4, 5
    ])
    msg = rng.integers(0, 1 << 32, size=(4, p.N), dtype=np.uint64).astype(np.uint32)
    rows = [r for r in client.encrypt_trlwe(keys, msg, seed=12)]
    rows += list(cmux_ref.extreme_pair(p, rng, top=False)) + list(cmux_ref.extreme_pair(p, rng, top=True))   # 4, 5 and 6, 7
    T = np.stack(rows + [np.zeros(2 * p.N, dtype=np.uint32)] * 2)            # 8, 9: outputs
    # anchor: the NTT product the reference uses equals the schoolbook one on one job
    job = (3, 0, 1, 0, 8)
    assert np.array_equal(cmux_ref.cmux(p, T, trgsw, job), cmux_ref.cmux(p, T, trgsw, job, product=cmux_ref.negacyclic_schoolbook))
    return keys, p, T, trgsw, cmux_ref.spectra(em, p, trgsw)


def _check(em, case, jobs):
    _, p, T, trgsw, spec = case
    want = cmux_ref.run_jobs(p, T.copy(), trgsw, jobs)
    got = cmux_ref.emu_run(em, p, T, spec, trgsw.shape[0], jobs)
    assert np.array_equal(got, want)
    return got


@pytest.mark.parametrize("sel", [0, 1, 3, 4, 5])
def test_two_row_form_equals_reference(em, case, sel):
    """fresh selectors of 0 and 1, uniform words, the worst-case words 0x7FFF7FFF / 0x80008000 in every coefficient"""
    _check(em, case, [(sel, 0, 1, 0, 8), (sel, 2, 3, 0, 9)])


def test_fresh_selectors_select(em, case):
    keys, p, T, _, _ = case
    got = _check(em, case, [(0, 0, 1, 0, 8), (1, 0, 1, 0, 9)])
    ph = client.trlwe_phases(keys, np.stack([got[8], got[9], T[0], T[1]])).view(np.int32).astype(np.int64)
    # sel = 0 keeps in0, sel = 1 selects in1, up to the product's noise: sqrt(2 l N) (Bg / 2) sigma ~ 2^18.5 / 2^19 per coefficient
    # with sigma = alpha1 2^32 of a fresh selector, plus the decomposition's rounding ~ 2^18 / 2^16: 2^24 is > 30 sigma
    wrap = lambda x: ((x + (1 << 31)) % (1 << 32)) - (1 << 31)
    assert np.abs(wrap(ph[0] - ph[2])).max() < 1 << 24 and np.abs(wrap(ph[1] - ph[3])).max() < 1 << 24


def test_zero_trgsw_returns_in0_exactly(em, case):
    _, p, T, _, _ = case
    got = _check(em, case, [(2, 0, 1, 0, 8), (2, 3, -1, 5, 9)])
    assert np.array_equal(got[8], T[0]) and np.array_equal(got[9], T[3])


@pytest.mark.parametrize("sel", [3, 4, 5])
def test_extreme_digits(em, case, sel):
    """pairs whose difference makes every digit -Bg/2 (rows 4, 5) and +Bg/2 - 1 (rows 6, 7)"""
    _check(em, case, [(sel, 4, 5, 0, 8), (sel, 6, 7, 0, 9)])


def test_rotate_form(em, case):
    _, p, T, _, _ = case
    N = p.N
    for rot in (0, 1, N - 1, N, N + 1, 2 * N - 1):
        got = _check(em, case, [(3, 0, -1, rot, 8), (1, 2, -1, rot, 9)])
        if rot == 0:   # (X^0 - 1) T = 0: every digit is zero
            assert np.array_equal(got[8], T[0]) and np.array_equal(got[9], T[2])


def test_in_place_forms(em, case):
    _check(em, case, [(3, 0, 1, 0, 0)])            # out == in0
    _check(em, case, [(3, 0, 1, 0, 1)])            # out == in1
    _check(em, case, [(4, 2, -1, 77, 2)])          # rotate form in place
    _check(em, case, [(1, 0, 1, 0, 0), (0, 0, 2, 0, 0), (3, 0, -1, 1000, 0)])   # a chain through one row


def test_rounding_margin(em, case):
    """the distance of every inverse-transform output from an integer, worst-case words and digits included, stays below what
    DESIGN.md section 2b proves for any key and digits: 2^-9.0 at the 128-bit set, 2^-5.6 at the 80-bit set"""
    p = case[1]
    em.iyk_emul_fft_round_error.restype = ctypes.c_double
    em.iyk_emul_fft_round_error(1)
    _check(em, case, [(4, 4, 5, 0, 8), (5, 6, 7, 0, 9), (5, 4, 5, 0, 8)])
    worst = em.iyk_emul_fft_round_error(1)
    print(f"emulated CMUX rounding distance, worst-case words and digits: {worst:.3e}")
    assert 0.0 < worst < (2.0 ** -9.0 if p.l == 3 else 2.0 ** -5.6)


def test_selector_spectra_are_the_key_transform(em, case):
    """What iyk_hip_trgsw_upload stores is bk_fft_kernel's output for the TRGSW taken as one step of a key: the emulation of that
    kernel, applied to one selector alone, gives that selector's slot of the store."""
    _, p, _, trgsw, spec = case
    slot = spec.size // trgsw.shape[0]
    for s in (1, 5):
        one = cmux_ref.spectra(em, p, trgsw[s : s + 1])
        assert np.array_equal(one, spec[s * slot : (s + 1) * slot])
    assert slot * 8 == p.trgsw_rows * (p.k + 1) * 2 * 512 * 16   # bytes per slot as include/iyokan_hip.h states them


def test_bad_index_is_refused(em, case):
    _, p, T, trgsw, spec = case
    jobs = np.array([[0, 0, 1, 0, T.shape[0]]], dtype=np.int32)
    Tc = T.copy()
    rc = em.emu_cmux_fft(0 if p.l == 3 else 1, Tc.ctypes.data_as(ctypes.POINTER(ctypes.c_uint32)), T.shape[0],
                         spec.ctypes.data_as(ctypes.POINTER(ctypes.c_double)), trgsw.shape[0],
                         jobs.ctypes.data_as(ctypes.POINTER(ctypes.c_int32)), 1)
    assert rc == -1 and np.array_equal(Tc, T)


@pytest.mark.parametrize("h", [0, 1, 512, 1023])
def test_index_extraction(em, case, h):
    _, p, T, _, _ = case
    out = np.zeros(p.N + 1, dtype=np.uint32)
    u32p = ctypes.POINTER(ctypes.c_uint32)
    assert em.emu_sample_extract_index(T[1].ctypes.data_as(u32p), h, out.ctypes.data_as(u32p)) == 0
    assert np.array_equal(out, cmux_ref.sample_extract_index(T[1], h, p.N))
    if h == 0:   # the existing index-0 extraction
        import numpy_tfhe as nt

        want0 = nt.sample_extract0([T[1][: p.N].astype(np.uint64), T[1][p.N :].astype(np.uint64)], p.N)
        assert np.array_equal(out, np.asarray(want0).astype(np.uint32))


def test_degenerate_jobs_and_last_slot(em, request):
    """The cmux_batch cases of tests/cmux_cases.py (the words test_gpu_cmux_edges.py runs on the GPU): in0 == in1, rot = 0, a job on
    the store's last selector slot, a batch whose jobs all use it.  The closed forms (a zero difference returns T[in0]) hold for
    the reference first, then for the emulation."""
    import cmux_cases

    for which in SETS:
        keys = request.getfixturevalue("keys" + which)
        p = keys.params
        trgsw, T, batches = cmux_cases.cmux_cases(keys)
        spec = cmux_ref.spectra(em, p, trgsw)
        want, got = T.copy(), T.copy()
        for n, jobs in enumerate(batches):
            cmux_ref.run_jobs(p, want, trgsw, jobs)
            got = cmux_ref.emu_run(em, p, got, spec, trgsw.shape[0], jobs)
            if n == 0:
                for out, same in cmux_cases.CMUX_IDENTITIES:
                    assert np.array_equal(want[out], T[same]) and np.array_equal(got[out], T[same]), (which, out, same)
        assert np.array_equal(got, want), which
        assert not np.array_equal(got[20], T[4])   # the last slot's selector did something
