"""cmux_rotate_chain_kernel's phase functions, run lane by lane on the CPU (csrc/emul.cpp: iyk_emul_cmux_rotate_chain), against the exact
reference of tests/cmux_ref.py applied step by step (tests/rom_chain_cases.py: chain) and against the existing single-CMUX emulation
(emu_cmux_fft), word for word on both parameter sets; and cmux.rom_rotate_chain / Rom.launches_fused against cmux.rom_read_plan."""
import ctypes

import numpy as np
import pytest

import cmux_cases
import cmux_ref
import rom_chain_cases as cases
from iyokan_amd import cmux

SETS = ["128", "80"]
_u32p = ctypes.POINTER(ctypes.c_uint32)
_i32p = ctypes.POINTER(ctypes.c_int32)
_f64p = ctypes.POINTER(ctypes.c_double)


@pytest.fixture(scope="module")
def em(built):
    em = cmux_ref.emul()
    em.iyk_emul_cmux_rotate_chain.argtypes = [ctypes.c_int, _u32p, ctypes.c_uint64, _f64p, ctypes.c_uint64, ctypes.c_int32, _i32p, _i32p,
                                              ctypes.c_int32, ctypes.c_int32]
    em.iyk_emul_fft_round_error.restype = ctypes.c_double
    return em


@pytest.fixture(scope="module", params=SETS)
def chosen(request, em):
    """The 128-slot selector store of cmux_cases and its spectra, once per parameter set."""
    keys = request.getfixturevalue("keys" + request.param)
    return keys, cmux_ref.spectra(em, keys.params, cmux_cases.selectors(keys))


def emu_job_rc(em, p, T, spec, slots, job):
    """one job through the emulation, in place on T; returns its status"""
    steps, sels, rots, src, out = job
    sel, rot = np.asarray(sels, dtype=np.int32), np.asarray(rots, dtype=np.int32)
    return em.iyk_emul_cmux_rotate_chain(0 if p.l == 3 else 1, T.ctypes.data_as(_u32p), T.shape[0], spec.ctypes.data_as(_f64p), slots, steps,
                                         sel.ctypes.data_as(_i32p), rot.ctypes.data_as(_i32p), src, out)


def emu_run(em, chosen, case):
    keys, spec = chosen
    trgsw, T, batches = case
    got = np.ascontiguousarray(T, dtype=np.uint32).copy()
    for jobs in batches:
        for job in jobs:
            assert emu_job_rc(em, keys.params, got, spec, trgsw.shape[0], job) == 0
    return got


def _assert_case(T, batches, got, want):
    bad = np.flatnonzero((got != want).any(axis=1))
    assert bad.size == 0, f"rows that differ from the reference: {bad[:10]}"
    written = {j[4] for jobs in batches for j in jobs}
    untouched = [r for r in range(T.shape[0]) if r not in written]
    assert np.array_equal(got[untouched], T[untouched])


@pytest.mark.parametrize("name", list(cases.CPU_CASES))
def test_emulation_equals_successive_reference_jobs(em, chosen, name):
    """steps = 1, 2, 10 (the ROM's own rotations, descending selectors), 32 (ending on the last slot); rot = 0, N, 2N - 1 in every step;
    the zero selector; worst-case words with every digit of the first difference at -Bg/2.  The closed forms (out == src) hold for the
    REFERENCE first, then for the emulation."""
    keys = chosen[0]
    case, want = cases.expected_of(keys, name)
    _, T, batches = case
    for out, same in cases.IDENTITIES.get(name, ()):
        assert np.array_equal(want[out], T[same]), (out, same)
    got = emu_run(em, chosen, case)
    _assert_case(T, batches, got, want)
    for out, same in cases.IDENTITIES.get(name, ()):
        assert np.array_equal(got[out], T[same]), (out, same)


@pytest.mark.parametrize("name", ["steps1", "steps2", "rom12", "steps32", "rotN", "extreme"])
def test_emulation_equals_single_cmux_emulation(em, chosen, name):
    """the same chains as `steps` successive calls of the existing emulation of cmux_fft_kernel, the accumulator in the out row"""
    keys, spec = chosen
    trgsw, T, batches = cases.CPU_CASES[name](keys)
    got = emu_run(em, chosen, (trgsw, T, batches))
    step_jobs = [j for jobs in batches for launch in cases.as_cmux_launches(jobs) for j in launch]
    unfused = cmux_ref.emu_run(em, keys.params, T, spec, trgsw.shape[0], step_jobs)
    assert np.array_equal(got, unfused)


@pytest.mark.parametrize("mutant", [dict(ascending=True), dict(shift_rot=1), dict(carry=False)], ids=["ascending", "next-rot", "no-carry"])
def test_mutants_differ(em, chosen, mutant):
    """What the comparison above must be able to tell apart, on the (12, 0) tail: the selectors taken ascending, the rot of step j + 1
    used in step j, the accumulator not carried into the next step — each gives other words than the emulation (and than the real
    reference, which the emulation equals)."""
    keys = chosen[0]
    case, want = cases.expected_of(keys, "rom12")
    trgsw, T, batches = case
    wrong = cases.expected(keys.params, T, trgsw, batches, **mutant)
    out = batches[0][0][4]
    assert not np.array_equal(wrong[out], want[out])
    got = emu_run(em, chosen, case)
    assert np.array_equal(got[out], want[out]) and not np.array_equal(got[out], wrong[out])


def test_rounding_margin(em, chosen):
    """the distance of every inverse-transform output from an integer over the 32-step chain, rot = N and the worst-case words and
    digits stays inside what DESIGN.md section 2b proves for any key and digits: 2^-8.5 at the 128-bit set, 2^-5.1 at the 80-bit set"""
    keys = chosen[0]
    em.iyk_emul_fft_round_error(1)
    for name in ("steps32", "rotN", "extreme"):
        emu_run(em, chosen, cases.CPU_CASES[name](keys))
    worst = em.iyk_emul_fft_round_error(1)
    print(f"emulated rotate chain rounding distance, worst-case words and digits: {worst:.3e}")
    assert 0.0 < worst <= (2.0 ** -8.5 if keys.params.l == 3 else 2.0 ** -5.1)


def test_bad_jobs_are_refused(em, chosen):
    keys, spec = chosen
    trgsw, T, _ = cases.one(keys)
    slots, N2 = trgsw.shape[0], 2 * keys.params.N
    for job in [(0, [], [], 0, 2), (33, [0] * 33, [1] * 33, 0, 2), (1, [-1], [1], 0, 2), (1, [slots], [1], 0, 2), (1, [0], [-1], 0, 2),
                (1, [0], [N2], 0, 2), (1, [0], [1], T.shape[0], 2), (1, [0], [1], 0, T.shape[0]), (2, [0, slots], [1, 1], 0, 2)]:
        Tc = T.copy()
        assert emu_job_rc(em, keys.params, Tc, spec, slots, job) == -1, job
        assert np.array_equal(Tc, T)


# ---- cmux.rom_rotate_chain and Rom.launches_fused against rom_read_plan --------------------------------------------------------------

SHAPES = [(3, 3), (8, 3), (9, 3), (12, 0), (2, 10), (1, 0)]
N = 1024


def _rom(aw, lw, max_reads):
    """a cmux.Rom without its device stores: what launches() and launches_fused() read"""
    rom = object.__new__(cmux.Rom)
    rom.addr_width, rom.N, rom.max_reads = aw, N, max_reads
    rom.layout = cmux.rom_layout(aw, lw, N)
    rom.plan = cmux.rom_read_plan(aw, lw, N)
    return rom


@pytest.mark.parametrize("aw,lw", SHAPES)
def test_rom_rotate_chain_is_the_plans_tail(aw, lw):
    plan = cmux.rom_read_plan(aw, lw, N)
    lay = cmux.rom_layout(aw, lw, N)
    chain = cmux.rom_rotate_chain(plan)
    want_steps = min(lay.log2_words, aw)   # one rotate step per low address bit the address has
    if want_steps == 0:
        assert chain is None
        return
    assert chain.steps == want_steps == len(chain.bits) == len(chain.rots)
    upper = len(plan) - chain.steps
    assert upper == max(aw - lay.log2_words, 0) and all(j.in1 >= 0 for jobs in plan[:upper] for j in jobs)
    cur = chain.src
    for s in range(chain.steps):   # expanded step by step: exactly the plan's launches
        assert plan[upper + s] == [cmux.PlanJob(chain.bits[s], cur, -1, chain.rots[s], chain.out)]
        cur = chain.out
    assert chain.out == lay.result and chain.src == (lay.result if upper else 0)
    assert list(chain.bits) == list(range(want_steps - 1, -1, -1))            # descending address bits
    skipped = lay.log2_words - want_steps                                      # an address narrower than W skips the high bits' steps
    assert list(chain.rots) == [2 * N - (N >> bit) for bit in range(skipped + 1, lay.log2_words + 1)]


def test_rotate_chain_shapes():
    """the shapes by hand: (12, 0) is the deepest tail the suite runs, (1, 0) skips nine of ten steps, (2, 10) has none"""
    steps = {s: getattr(cmux.rom_rotate_chain(cmux.rom_read_plan(*s, N)), "steps", 0) for s in SHAPES}
    assert steps == {(3, 3): 3, (8, 3): 7, (9, 3): 7, (12, 0): 10, (2, 10): 0, (1, 0): 1}
    one = cmux.rom_rotate_chain(cmux.rom_read_plan(1, 0, N))
    assert one == cmux.RotateChain(1, (0,), (2 * N - 1,), 0, 1)


@pytest.mark.parametrize("reads", [1, 2, 3])
@pytest.mark.parametrize("aw,lw", SHAPES)
def test_launches_fused_expand_to_the_unfused_launches(aw, lw, reads):
    rom = _rom(aw, lw, 3)
    unfused = rom.launches(reads)
    upper, chain = rom.launches_fused(reads)
    assert upper == unfused[: len(upper)]
    if chain is None:
        assert upper == unfused and cmux.rom_rotate_chain(rom.plan) is None
        return
    steps, sel, rot, src, out = chain
    assert len(steps) == len(src) == len(out) == reads and len(set(steps)) == 1 and len(sel) == len(rot) == sum(steps)
    assert len(upper) + steps[0] == len(unfused)
    first = np.concatenate([[0], np.cumsum(steps)[:-1]])
    for s in range(steps[0]):
        cols = ([sel[f + s] for f in first], list(src) if s == 0 else list(out), [-1] * reads, [rot[f + s] for f in first], list(out))
        assert tuple(cols) == unfused[len(upper) + s], s
    assert len(set(out)) == reads and all(out[g] != src[h] for g in range(reads) for h in range(reads) if g != h)   # one legal batch
