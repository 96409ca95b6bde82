"""cmux_chain_kernel's phase functions, run lane by lane on the CPU (csrc/emul.cpp: emu_cmux_chain), against the exact reference of
tests/cmux_ref.py applied step by step (tests/ram_ref.py: chain).  Equality is word for word on both parameter sets."""
import ctypes

import numpy as np
import pytest

import cmux_cases
import cmux_ref
import ram_ref
from iyokan_amd import client

SETS = ["128", "80"]
# selector slots: five runs of five slots, one per kind, so that a chain of up to five steps stays inside one kind
FRESH, ZERO, UNIFORM, WORST_P, WORST_N = 0, 5, 10, 15, 20
FRESH_BITS = [1, 0, 1, 1, 0]


@pytest.fixture(scope="module")
def em(built):
    return ram_ref.emul()


@pytest.fixture(scope="module", params=SETS)
def case(request, em):
    keys = request.getfixturevalue("keys" + request.param)
    p = keys.params
    rng = np.random.default_rng(2025)
    fresh = client.encrypt_trgsw(keys, FRESH_BITS, seed=21)
    uniform = rng.integers(0, 1 << 32, size=fresh.shape, dtype=np.uint64).astype(np.uint32)
    trgsw = np.concatenate([fresh, np.zeros_like(fresh), uniform, np.stack([cmux_ref.worst_case_trgsw(p, 0x7FFF7FFF)] * 5),
                            np.stack([cmux_ref.worst_case_trgsw(p, 0x80008000)] * 5)])
    msg = rng.integers(0, 1 << 32, size=(4, p.N), dtype=np.uint64).astype(np.uint32)
    rows = [r for r in client.encrypt_trlwe(keys, msg, seed=22)]                                             # 0 .. 3
    rows += list(cmux_ref.extreme_pair(p, rng, top=False)) + list(cmux_ref.extreme_pair(p, rng, top=True))   # 4, 5 and 6, 7
    T = np.stack(rows + [np.zeros(2 * p.N, dtype=np.uint32)] * 2)                                            # 8, 9: outputs
    return keys, p, T, trgsw, cmux_ref.spectra(em, p, trgsw)


def _check(em, case, jobs):
    _, p, T, trgsw, spec = case
    want = ram_ref.run_chains(p, T.copy(), trgsw, jobs)
    got = ram_ref.emu_chain_run(em, p, T, spec, trgsw.shape[0], jobs)
    assert np.array_equal(got, want)
    return got


PATTERNS = {1: [0, 1], 2: [0, 3, 1, 2], 5: [0, 31, 0b01101, 0b10010]}   # all-zero, all-ones, mixed


@pytest.mark.parametrize("steps", [1, 2, 5])
@pytest.mark.parametrize("sel0", [FRESH, ZERO, UNIFORM, WORST_P, WORST_N])
def test_chain_equals_step_by_step_reference(em, case, steps, sel0):
    """every kind of selector, every pattern shape, out a fresh row"""
    jobs = [(sel0, steps, pat, 0, 1, 8 + (n & 1)) for n, pat in enumerate(PATTERNS[steps])]
    _check(em, case, jobs)


def test_chain_equals_cmux_jobs(em, case):
    """the same chain through emu_cmux_fft as dependent CMUX jobs: the two kernels' emulations agree as well"""
    _, p, T, trgsw, spec = case
    job = (UNIFORM, 5, 0b10110, 0, 1, 8)
    got = ram_ref.emu_chain_run(em, p, T, spec, trgsw.shape[0], [job])
    steps = cmux_ref.emu_run(em, p, T, spec, trgsw.shape[0], ram_ref.chain_as_cmux_jobs(job, 9))
    assert np.array_equal(got[8], steps[8])


@pytest.mark.parametrize("sel0", [UNIFORM, WORST_P, WORST_N])
def test_extreme_digits(em, case, sel0):
    """src / mem pairs whose first difference makes every digit -Bg/2 (rows 4, 5) or +Bg/2 - 1 (rows 6, 7), both orientations"""
    _check(em, case, [(sel0, 2, 0, 4, 5, 8), (sel0, 2, 3, 5, 4, 9), (sel0, 5, 0b01010, 6, 7, 8), (sel0, 1, 1, 7, 6, 9)])


def test_in_place_forms(em, case):
    for steps, pat in ((1, 1), (2, 1), (5, 0b11001)):
        _check(em, case, [(UNIFORM, steps, pat, 0, 1, 1)])   # out == mem: the RAM cell
        _check(em, case, [(UNIFORM, steps, pat, 0, 1, 0)])   # out == src
        _check(em, case, [(UNIFORM, steps, pat, 0, 1, 8)])   # a fresh row
    _check(em, case, [(FRESH, 5, 9, 0, 1, 1), (FRESH, 5, 9, 0, 2, 2), (FRESH, 5, 22, 0, 3, 3)])   # one src, three cells


@pytest.mark.parametrize("steps", [1, 2, 5])
def test_zero_trgsw_leaves_acc_or_mem_exactly(em, case, steps):
    """S = 0: a step with pattern bit 0 keeps the accumulator, a step with pattern bit 1 replaces it by T[mem]"""
    _, p, T, _, _ = case
    got = _check(em, case, [(ZERO, steps, 0, 0, 1, 8), (ZERO, steps, 1 << (steps - 1), 0, 1, 9)])
    assert np.array_equal(got[8], T[0]) and np.array_equal(got[9], T[1])
    got = _check(em, case, [(ZERO, steps, (1 << steps) - 1, 2, 3, 8)])
    assert np.array_equal(got[8], T[3])


def test_fresh_selectors_select(em, case):
    """five fresh selectors of FRESH_BITS: the accumulator survives exactly where the pattern equals the encrypted bits"""
    keys, p, T, _, _ = case
    addr = sum(b << j for j, b in enumerate(FRESH_BITS))
    got = _check(em, case, [(FRESH, 5, addr, 0, 1, 8), (FRESH, 5, addr ^ 4, 0, 1, 9)])
    ph = client.trlwe_phases(keys, np.stack([got[8], got[9], T[0], T[1]])).view(np.int32).astype(np.int64)
    wrap = lambda x: ((x + (1 << 31)) % (1 << 32)) - (1 << 31)
    # five products' noise instead of one: the 2^24 of test_cmux_emulation.py (> 30 sigma of one product) times sqrt(5) < 2^26
    assert np.abs(wrap(ph[0] - ph[2])).max() < 1 << 26 and np.abs(wrap(ph[1] - ph[3])).max() < 1 << 26


def test_rounding_margin(em, case):
    """the distance of every inverse-transform output of the chain from an integer, worst-case words and digits included, stays
    below what DESIGN.md section 2b proves for any key and digits: 2^-9.0 at the 128-bit set, 2^-5.6 at the 80-bit set"""
    p = case[1]
    em.iyk_emul_fft_round_error.restype = ctypes.c_double
    em.iyk_emul_fft_round_error(1)
    _check(em, case, [(WORST_P, 5, 0b01010, 4, 5, 8), (WORST_N, 5, 0b10101, 6, 7, 9), (WORST_N, 2, 3, 5, 4, 8)])
    worst = em.iyk_emul_fft_round_error(1)
    print(f"emulated chain rounding distance, worst-case words and digits: {worst:.3e}")
    assert 0.0 < worst < (2.0 ** -9.0 if p.l == 3 else 2.0 ** -5.6)


def test_bad_jobs_are_refused(em, case):
    _, p, T, trgsw, spec = case
    slots = trgsw.shape[0]
    for job in [(0, 0, 0, 0, 1, 8), (0, 33, 0, 0, 1, 8), (slots - 1, 2, 0, 0, 1, 8), (-1, 1, 0, 0, 1, 8), (0, 1, 0, T.shape[0], 1, 8),
                (0, 1, 0, 0, -1, 8), (0, 1, 0, 0, 1, T.shape[0])]:
        Tc = T.copy()
        assert ram_ref.emu_chain_rc(em, p, Tc, spec, slots, [job]) == -1, job
        assert np.array_equal(Tc, T)


# ---- the chosen cases of tests/cmux_cases.py: the words the GPU runs in test_gpu_cmux_edges.py ------------------------------------


@pytest.fixture(scope="module", params=SETS)
def chosen(request, em):
    """The 128-slot selector store of cmux_cases and its spectra, once per parameter set."""
    keys = request.getfixturevalue("keys" + request.param)
    trgsw = cmux_cases.selectors(keys)
    return keys, cmux_ref.spectra(em, keys.params, trgsw)


def _run_chosen(em, chosen, case):
    """The case through emu_cmux_chain, batch by batch, against ram_ref.run_chains.  Returns (T, jobs of all batches, result)."""
    keys, spec = chosen
    p = keys.params
    trgsw, T, batches = case
    want, got = T.copy(), T.copy()
    for jobs in batches:
        ram_ref.run_chains(p, want, trgsw, jobs)
        got = ram_ref.emu_chain_run(em, p, got, spec, trgsw.shape[0], jobs)
    bad = np.flatnonzero((got != want).any(axis=1))
    assert bad.size == 0, f"rows that differ from the reference: {bad[:10]}"
    written = {j[5] for jobs in batches for j in jobs}
    untouched = [r for r in range(T.shape[0]) if r not in written]
    assert np.array_equal(got[untouched], T[untouched])
    return T, [j for jobs in batches for j in jobs], got


@pytest.mark.parametrize("steps", cmux_cases.A_STEPS)
def test_long_chains(em, chosen, steps):
    """case A: 8 (the RAM benchmark's shape), 16, 31 and 32 steps, pattern bits up to 31, sel0 + j up to the store's last slot"""
    keys, spec = chosen
    p = keys.params
    case = cmux_cases.case_a(keys, steps)
    T, jobs, got = _run_chosen(em, chosen, case)
    if steps == 32:   # the same chains through emu_cmux_fft as dependent CMUX jobs
        step_jobs = [s for g, j in enumerate(jobs) for s in ram_ref.chain_as_cmux_jobs(j, cmux_cases.accumulator_row(jobs, g))]
        unfused = cmux_ref.emu_run(em, p, T, spec, case[0].shape[0], step_jobs)
        written = sorted({j[5] for j in jobs})
        assert np.array_equal(unfused[written], got[written])


def test_mixed_steps(em, chosen):
    """case B: steps 1 .. 32 side by side, the top used bit of every pattern set"""
    _run_chosen(em, chosen, cmux_cases.case_b(chosen[0]))


def test_many_jobs(em, chosen):
    """case C cut to 17 jobs (the emulation has no workgroups; the GPU runs all 301)"""
    _run_chosen(em, chosen, cmux_cases.case_c(chosen[0], count=17))


def test_degenerate_chains(em, chosen):
    """case D: src == mem and chains on zero selectors.  The closed forms hold for the REFERENCE first, then for the emulation."""
    keys, _ = chosen
    trgsw, T, batches = cmux_cases.case_d(keys)
    want = ram_ref.run_chains(keys.params, T.copy(), trgsw, batches[0])
    for out, same in cmux_cases.D_IDENTITIES:
        assert np.array_equal(want[out], T[same]), (out, same)
    _, _, got = _run_chosen(em, chosen, (trgsw, T, batches))
    for out, same in cmux_cases.D_IDENTITIES:
        assert np.array_equal(got[out], T[same]), (out, same)


def test_dependent_batches(em, chosen):
    """case E: twelve batches, each on the rows the one before wrote"""
    _run_chosen(em, chosen, cmux_cases.case_e(chosen[0]))
