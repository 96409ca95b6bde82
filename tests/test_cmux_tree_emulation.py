"""cmux_tree_kernel's phase functions, run lane by lane on the CPU in the kernel's order and on its strided in-place accumulators
(csrc/emul.cpp: iyk_emul_cmux_tree), against the exact reference of tests/cmux_ref.py applied level by level (tests/cmux_tree_cases.py:
tree) and against the existing single-CMUX emulation (emu_cmux_fft) run as `levels` batches, word for word on both parameter sets; the
argument check cmux_tree_args through iyk_emul_check_cmux_tree_batch; cmux.rom_tree_jobs against cmux.rom_read_plan; and what Rom.read /
Ram.read_port enqueue with and without fused_tree.

Mutants of the EMULATION (one edit of cmux_tree in emul.cpp each, built apart and run against this file):
    partner w + 2^b instead of w + 2^(b-1)
    selector sel0 at every level
    in0 / in1 swapped at the levels >= 1 only (the difference the other way round, the accumulator replaced by in1)
    the two loops exchanged, wave by wave instead of level by level: the barrier's effect dropped, wave 0 reads its partners'
        accumulators as they were before those ran their levels
Each of the four fails, at both parameter sets, test_emulation_equals_successive_reference_levels[uniform, alt, first, last, zig, zag,
in_place, two_groups], every case of test_emulation_equals_single_cmux_emulation, test_mutants_differ (the emulation no longer equals the
reference) and test_rom_tree_jobs_emulated_give_the_unfused_plans_row[2 .. 9]: 42 of the file's 102 tests.  The zero selector's case passes
under the first, second and fourth, as it must — a zero selector keeps in0 whatever in1 and the slot are — and fails under the third."""
import ctypes
import os
import re

import numpy as np
import pytest

import batch_refusal_cases as brc
import cmux_ref
import cmux_tree_cases as cases
from iyokan_amd import client, cmux

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SETS = ["128", "80"]
_u32p = ctypes.POINTER(ctypes.c_uint32)
_i32p = ctypes.POINTER(ctypes.c_int32)
_f64p = ctypes.POINTER(ctypes.c_double)
u64 = ctypes.c_uint64


@pytest.fixture(scope="module")
def em(built):
    em = cmux_ref.emul()
    em.iyk_emul_cmux_tree.argtypes = [ctypes.c_int, _u32p, u64, _f64p, u64, ctypes.c_int32, ctypes.c_int32, ctypes.c_int32, ctypes.c_int32]
    em.iyk_emul_fft_round_error.restype = ctypes.c_double
    return em


@pytest.fixture(scope="module", params=SETS)
def chosen(request, em):
    """The 32-slot selector store of cmux_tree_cases and its spectra, once per parameter set."""
    keys = request.getfixturevalue("keys" + request.param)
    return keys, cmux_ref.spectra(em, keys.params, cases.selectors(keys))


def emu_job_rc(em, p, T, spec, slots, job):
    """one job through the emulation, in place on T; returns its status"""
    sel0, levels, first, out = job
    return em.iyk_emul_cmux_tree(0 if p.l == 3 else 1, T.ctypes.data_as(_u32p), T.shape[0], spec.ctypes.data_as(_f64p), slots, sel0, levels,
                                 first, out)


def emu_run(em, p, spec, slots, T, batches):
    got = np.ascontiguousarray(T, dtype=np.uint32).copy()
    for jobs in batches:
        for job in jobs:   # one after the other: no out is a leaf of another job of its batch
            assert emu_job_rc(em, p, got, spec, slots, job) == 0
    return got


def _assert_case(T, batches, got, want):
    bad = np.flatnonzero((got != want).any(axis=1))
    assert bad.size == 0, f"rows that differ from the reference: {bad[:10]}"
    written = {j[3] for jobs in batches for j in jobs}
    untouched = [r for r in range(T.shape[0]) if r not in written]
    assert np.array_equal(got[untouched], T[untouched])


@pytest.mark.parametrize("name", list(cases.CPU_CASES))
def test_emulation_equals_successive_reference_levels(em, chosen, name):
    """levels 1, 2, 3, 4 side by side on zero selectors (the result is leaf 0 exactly: held for the REFERENCE first), on uniform words
    ending on the store's last slot and on the worst-case words over leaves with every first digit at its extreme; fresh selectors
    whose bits lead to the first leaf, the last leaf and along the two alternating paths, on leaves that encrypt a 1 where the path
    ends and 0 elsewhere (the result decrypts to 1); out == an own leaf; two dependent batches."""
    keys, spec = chosen
    case, want = cases.expected_of(keys, name)
    trgsw, T, batches = case
    for out, same in cases.IDENTITIES.get(name, ()):
        assert np.array_equal(want[out], T[same]), (out, same)
    got = emu_run(em, keys.params, spec, trgsw.shape[0], T, batches)
    _assert_case(T, batches, got, want)
    for out, same in cases.IDENTITIES.get(name, ()):
        assert np.array_equal(got[out], T[same]), (out, same)
    if name in ("first", "last", "zig", "zag"):
        outs = [j[3] for j in batches[0]]
        assert list(client.decrypt_ram_trlwe(keys, got[outs])) == [1] * len(outs)
        hot = [first + cases.selected_leaf(sel0, levels) for sel0, levels, first, _ in batches[0]]
        assert np.flatnonzero(client.decrypt_ram_trlwe(keys, T[: 4 * cases.LEAVES])).tolist() == hot   # the 1 can only have come from there


@pytest.mark.parametrize("name", ["uniform", "alt", "zig", "in_place", "two_groups"])
def test_emulation_equals_single_cmux_emulation(em, chosen, name):
    """the same trees as `levels` successive batches of the existing emulation of cmux_fft_kernel, the candidates in rows of their own"""
    keys, spec = chosen
    trgsw, T, batches = cases.CPU_CASES[name](keys)
    got = emu_run(em, keys.params, spec, trgsw.shape[0], T, batches)
    rows = T.shape[0]
    unfused = T
    for jobs in batches:
        big = np.concatenate([unfused, np.zeros((14 * len(jobs), T.shape[1]), dtype=np.uint32)])
        for launch in cases.as_cmux_launches(jobs, rows):
            big = cmux_ref.emu_run(em, keys.params, big, spec, trgsw.shape[0], launch)
        unfused = big[:rows]
    assert np.array_equal(got, unfused)


MUTANTS = {"far-partner": dict(far_partner=True), "same-selector": dict(same_selector=True), "swap-upper": dict(swap_upper=True),
           "stale-partner": dict(stale_partner=True)}


@pytest.mark.parametrize("mutant", list(MUTANTS))
def test_mutants_differ(em, chosen, mutant):
    """What the comparison above must be able to tell apart, on uniform words: each fault of the wave pattern, restated on the
    reference's candidates, gives other words than the reference for every levels >= 2 — and the same words at levels = 1, where there
    is no level b >= 1 — and the emulation equals the reference, not the mutant."""
    keys, spec = chosen
    case, want = cases.expected_of(keys, "uniform")
    trgsw, T, batches = case
    wrong = cases.expected(keys.params, T, trgsw, batches, **MUTANTS[mutant])
    got = emu_run(em, keys.params, spec, trgsw.shape[0], T, batches)
    for sel0, levels, first, out in batches[0]:
        assert np.array_equal(got[out], want[out])
        assert np.array_equal(wrong[out], want[out]) == (levels == 1), (mutant, levels)


def test_rounding_margin(em, chosen):
    """the distance of every inverse-transform output from an integer over the worst-case words and digits stays inside what DESIGN.md
    section 2b proves for any key and digits: 2^-8.5 at the 128-bit set, 2^-5.1 at the 80-bit set"""
    keys, spec = chosen
    em.iyk_emul_fft_round_error(1)
    for name in ("alt", "uniform"):
        trgsw, T, batches = cases.CPU_CASES[name](keys)
        emu_run(em, keys.params, spec, trgsw.shape[0], T, batches)
    worst = em.iyk_emul_fft_round_error(1)
    print(f"emulated read tree rounding distance, worst-case words and digits: {worst:.3e}")
    assert 0.0 < worst <= (2.0 ** -8.5 if keys.params.l == 3 else 2.0 ** -5.1)


def test_bad_jobs_are_refused(em, chosen):
    keys, spec = chosen
    trgsw, T, _ = cases.single(keys)
    slots, rows = trgsw.shape[0], T.shape[0]
    for job in [(0, 0, 0, 16), (0, 5, 0, 16), (-1, 1, 0, 16), (slots - 3, 4, 0, 16), (slots, 1, 0, 16), (0, 1, -1, 16), (0, 1, rows - 1, 16),
                (0, 4, 2, 16), (0, 1, 0, rows), (0, 1, 0, -1)]:
        Tc = T.copy()
        assert emu_job_rc(em, keys.params, Tc, spec, slots, job) == -1, job
        assert np.array_equal(Tc, T)


# ---- cmux_tree_args (csrc/batch_args.hpp) through iyk_emul_check_cmux_tree_batch: stores of 8 selector slots and 40 rows ------------------

TRGSW, TRLWE = 8, 40
OK, INVALID = 0, -1
T_LEVELS = "levels outside [1, 4]"
T_SEL = "selector index outside the selector store"
T_ROW = "TRLWE index outside the buffer"
T_TWO = "two jobs of one batch write the same TRLWE row"
T_READ = "a job reads a TRLWE row that another job of the batch writes"
T_CAP = "batch too large"
T_STORE = "store larger than an allocation can be"


def check(sel0, levels, first, out, count=None, trgsw_slots=TRGSW, trlwe_slots=TRLWE):
    """(code, text, job words [count][4])"""
    L = brc.emul()
    keep = [np.ascontiguousarray(np.asarray(v, dtype=np.int64).astype(np.int32)) for v in (sel0, levels, first, out)]
    msg = ctypes.create_string_buffer(256)
    words = np.zeros(1024, dtype=np.uint32)
    counts = (u64 * 4)()
    f = L.iyk_emul_check_cmux_tree_batch
    f.restype = ctypes.c_int
    code = f(u64(trgsw_slots), u64(trlwe_slots), u64(len(keep[0]) if count is None else count), *[a.ctypes.data_as(_i32p) for a in keep], msg,
             u64(256), words.ctypes.data_as(_u32p), u64(words.size), counts)
    nj = int(counts[0])
    return code, msg.value.decode(), words.view(np.int32)[: 4 * nj].reshape(nj, 4).tolist()


REFUSED = {
    "levels 0": (dict(sel0=[0], levels=[0], first=[0], out=[20]), T_LEVELS),
    "levels 5": (dict(sel0=[0], levels=[5], first=[0], out=[36]), T_LEVELS),
    "levels -1 in the second job": (dict(sel0=[0, 0], levels=[1, -1], first=[0, 2], out=[20, 21]), T_LEVELS),
    "sel0 -1": (dict(sel0=[-1], levels=[1], first=[0], out=[20]), T_SEL),
    "sel0 == trgsw_slots": (dict(sel0=[TRGSW], levels=[1], first=[0], out=[20]), T_SEL),
    "sel0 + levels == trgsw_slots + 1": (dict(sel0=[TRGSW - 3], levels=[4], first=[0], out=[20]), T_SEL),
    "first -1": (dict(sel0=[0], levels=[1], first=[-1], out=[20]), T_ROW),
    "the last leaf == trlwe_slots": (dict(sel0=[0], levels=[4], first=[TRLWE - 15], out=[0]), T_ROW),
    "first == trlwe_slots": (dict(sel0=[0], levels=[1], first=[TRLWE], out=[0]), T_ROW),
    "out == trlwe_slots": (dict(sel0=[0], levels=[1], first=[0], out=[TRLWE]), T_ROW),
    "out -1": (dict(sel0=[0], levels=[1], first=[0], out=[-1]), T_ROW),
    "out[g] == the first leaf of h": (dict(sel0=[0, 0], levels=[2, 2], first=[0, 4], out=[4, 20]), T_READ),
    "out[g] == the last leaf of h": (dict(sel0=[0, 0], levels=[2, 4], first=[0, 4], out=[19, 20]), T_READ),
    "out[g] == a leaf both jobs share": (dict(sel0=[0, 1], levels=[2, 2], first=[0, 0], out=[1, 20]), T_READ),
    "out[g] == out[h]": (dict(sel0=[0, 1], levels=[1, 2], first=[0, 4], out=[20, 20]), T_TWO),
    "over cap": (dict(sel0=[0], levels=[1], first=[0], out=[20], count=(1 << 24) + 1), T_CAP),
    "selector store over cap": (dict(sel0=[0], levels=[1], first=[0], out=[20], trgsw_slots=(1 << 24) + 1), T_STORE),
    "row store over cap": (dict(sel0=[0], levels=[1], first=[0], out=[20], trlwe_slots=(1 << 28) + 1), T_STORE),
    # two faults at once: which one is reported
    "bad levels and bad row": (dict(sel0=[0], levels=[0], first=[-1], out=[20]), T_LEVELS),
    "bad selector and bad row": (dict(sel0=[TRGSW], levels=[1], first=[0], out=[TRLWE]), T_SEL),
    "two writers and a read of a written row": (dict(sel0=[0, 0, 0], levels=[1, 1, 1], first=[0, 2, 20], out=[20, 21, 21]), T_TWO),
}


@pytest.mark.parametrize("name", list(REFUSED))
def test_refusals(built, name):
    args, text = REFUSED[name]
    code, got, jobs = check(**args)
    assert (code, got) == (INVALID, text)
    assert jobs == []   # a refused set hands nothing to stage


def test_job_words_of_a_legal_batch(built):
    """levels 1 and 4, selectors 0 and ending on trgsw_slots - 1, leaves from row 0 and ending on row trlwe_slots - 1 are all inside"""
    code, text, jobs = check(sel0=[0, TRGSW - 4, TRGSW - 1], levels=[1, 4, 1], first=[0, TRLWE - 16, 2], out=[20, 21, TRLWE - 17])
    assert (code, text) == (OK, "")
    assert jobs == [[0, 1, 0, 20], [TRGSW - 4, 4, TRLWE - 16, 21], [TRGSW - 1, 1, 2, TRLWE - 17]]   # {sel0, levels, first, out}


def test_allowed_aliasings(built):
    """out == the job's own first, inner or last leaf; jobs that share all or some of their leaves; both at once where no out is a
    leaf of ANOTHER job"""
    for out in (0, 5, 15):
        assert check(sel0=[0], levels=[4], first=[0], out=[out])[:2] == (OK, "")
    assert check(sel0=[0, 4], levels=[4, 4], first=[0, 0], out=[20, 21])[:2] == (OK, "")
    assert check(sel0=[0, 1, 2], levels=[3, 2, 1], first=[0, 4, 6], out=[20, 21, 22])[:2] == (OK, "")
    code, _, jobs = check(sel0=[0, 0, 3], levels=[2, 2, 1], first=[0, 0, 8], out=[20, 21, 8])
    assert code == OK and [j[2:] for j in jobs] == [[0, 20], [0, 21], [8, 8]]


def test_a_shared_leaf_may_not_be_written_by_one_of_its_readers(built):
    assert check(sel0=[0, 0], levels=[2, 2], first=[0, 0], out=[0, 21])[:2] == (INVALID, T_READ)


def test_every_refusal_text_has_a_set(built):
    """the string literals of cmux_tree_args in batch_args.hpp == the texts the sets above reach"""
    src = open(os.path.join(ROOT, "iyokan_amd", "csrc", "batch_args.hpp")).read()
    m = re.search(r"^inline Refusal cmux_tree_args\(.*?^}$", src, re.M | re.S)
    assert m
    assert set(re.findall(r'"([^"\n]+)"', m.group(0))) == {text for _, text in REFUSED.values()}


def test_grid(built):
    """dispatch::cmux_tree_grid: one workgroup per job"""
    f = brc.emul().iyk_emul_cmux_tree_grid
    f.restype, f.argtypes = ctypes.c_int64, [ctypes.c_int64]
    assert [f(c) for c in (-1, 0, 1, 8, 9, 301, 1 << 24)] == [0, 0, 1, 8, 9, 301, 1 << 24]


# ---- cmux.rom_tree_jobs against cmux.rom_read_plan ------------------------------------------------------------------------------------

N = 1024
UPPER = list(range(1, 10))


def _expand(groups):
    """the groups as the launches of two-row PlanJobs they stand for, the candidates between a group's levels under names of their own"""
    launches = []
    for jobs, _ in groups:
        for b in range(jobs[0].levels):
            launches.append([(j.bit0 + b, (g, b, 2 * i), (g, b, 2 * i + 1)) for g, j in enumerate(jobs) for i in range(1 << (j.levels - 1 - b))])
    return launches


@pytest.mark.parametrize("upper", UPPER)
@pytest.mark.parametrize("lw", [10, 7])
def test_rom_tree_jobs_cover_the_plans_levels(upper, lw):
    """for 1 .. 9 upper address bits (a RAM's plan, and a ROM's with three rotate steps behind them): groups of 4 levels and a rest, level
    for level the job counts and address bits of the plan; a group's leaves are the data rows or, consecutively, the outs of the group
    before; the regions alternate, no group reads the region it writes, everything stays inside the layout; the last group's one job
    writes layout.result"""
    aw = upper + (10 - lw)
    plan, lay = cmux.rom_read_plan(aw, lw, N), cmux.rom_layout(aw, lw, N)
    groups = cmux.rom_tree_jobs(plan)
    assert [jobs[0].levels for jobs, _ in groups] == [4] * (upper // 4) + ([upper % 4] if upper % 4 else [])
    expanded = _expand(groups)
    assert len(expanded) == upper and all(j.in1 >= 0 for jobs in plan[:upper] for j in jobs) and all(j.in1 < 0 for jobs in plan[upper:] for j in jobs)
    for level, jobs in zip(expanded, plan):
        assert len(level) == len(jobs) and [x[0] for x in level] == [j.bit for j in jobs]
    D = lay.data_rows
    regions = [range(D, D + D // 2), range(D + D // 2, D + D // 2 + D // 4)]
    prev_outs = list(range(D))
    for g, (jobs, region) in enumerate(groups):
        leaves = [j.first + k for j in jobs for k in range(1 << j.levels)]
        assert leaves == prev_outs                                     # consecutive, in order, all of them
        assert len({j.levels for j in jobs}) == 1 and len({j.bit0 for j in jobs}) == 1
        outs = [j.out for j in jobs]
        if g == len(groups) - 1:
            assert region is None and outs == [lay.result]
        else:
            assert region == g & 1 and all(o in regions[region] for o in outs) and not set(outs) & set(leaves)
        assert all(0 <= r < D + lay.scratch_rows for r in outs + leaves)
        prev_outs = outs
    assert cmux.rom_tree_jobs(cmux.rom_read_plan(3, 3, N)) == []   # no upper tree


def test_rom_tree_jobs_by_hand():
    five = cmux.rom_tree_jobs(cmux.ram_read_plan(5, N))
    assert five == [([cmux.TreeJob(0, 4, 0, 32), cmux.TreeJob(0, 4, 16, 33)], 0), ([cmux.TreeJob(4, 1, 32, 32)], None)]
    assert cmux.rom_tree_jobs(cmux.rom_read_plan(9, 3, N)) == [([cmux.TreeJob(7, 2, 0, 4)], None)]
    nine = cmux.rom_tree_jobs(cmux.ram_read_plan(9, N))
    assert [(len(jobs), jobs[0], region) for jobs, region in nine] == [(32, cmux.TreeJob(0, 4, 0, 512), 0), (2, cmux.TreeJob(4, 4, 512, 768), 1),
                                                                      (1, cmux.TreeJob(8, 1, 768, 512), None)]


@pytest.mark.parametrize("upper", UPPER)
def test_rom_tree_jobs_emulated_give_the_unfused_plans_row(em, keys128, upper):
    """a RAM plane of 2^upper uniform rows under the store's last `upper` selector slots (a worst-case one, then uniform ones): the
    groups through the tree emulation and the plan's levels through the single-CMUX emulation leave the same result row"""
    keys = keys128
    p = keys.params
    trgsw = cases.selectors(keys)
    spec = cmux_ref.spectra(em, p, trgsw)
    plan, lay = cmux.ram_read_plan(upper, N), cmux.ram_layout(upper, N)
    rng = np.random.default_rng([11, 0x7F, upper])
    T = np.concatenate([cases._rows(p, rng, lay.data_rows), np.zeros((lay.scratch_rows, 2 * N), dtype=np.uint32)])
    sel = cases.SLOTS - upper
    fused = T.copy()
    for jobs, _ in cmux.rom_tree_jobs(plan):
        for j in jobs:
            assert emu_job_rc(em, p, fused, spec, cases.SLOTS, (sel + j.bit0, j.levels, j.first, j.out)) == 0
    unfused = T
    for jobs in plan:
        unfused = cmux_ref.emu_run(em, p, unfused, spec, cases.SLOTS, [(sel + j.bit, j.in0, j.in1, j.rot, j.out) for j in jobs])
    assert np.array_equal(fused[lay.result], unfused[lay.result])
    assert np.array_equal(fused[: lay.data_rows], T[: lay.data_rows])


# ---- what Rom.read and Ram.read_port enqueue --------------------------------------------------------------------------------------------

class Recorder:
    """a stream that writes down its calls"""

    def __init__(self):
        self.calls = []

    def __getattr__(self, name):
        def call(*args, **kw):
            self.calls.append((name,) + tuple(np.asarray(a).tolist() if isinstance(a, (np.ndarray, list, tuple)) else a for a in args) + ((kw,) if kw else ()))
        return call


def _rom(aw, lw, max_reads):
    """a cmux.Rom without its device stores, on a recording stream"""
    rom = object.__new__(cmux.Rom)
    rom.stream, rom.addr_width, rom.N, rom.max_reads, rom.word_bits = Recorder(), aw, N, max_reads, 1 << lw
    rom.layout, rom.plan = cmux.rom_layout(aw, lw, N), cmux.rom_read_plan(aw, lw, N)
    rom.trgsw, rom.trlwe = "selectors", "rows"
    return rom


def _ram(aw, dw):
    ram = object.__new__(cmux.Ram)
    ram.stream, ram.addr_width, ram.data_width, ram.N, ram.cells_per_plane = Recorder(), aw, dw, N, 1 << aw
    ram.layout, ram.plan = cmux.ram_layout(aw, N), cmux.ram_read_plan(aw, N)
    ram.ncells, ram.plane_scratch = dw << aw, ram.layout.scratch_rows + 2
    ram.trgsw, ram.trlwe = "selectors", "rows"
    return ram


def _lists(args):
    return tuple(list(a) for a in args)


@pytest.mark.parametrize("aw,lw", [(9, 3), (12, 0), (13, 3), (3, 3), (2, 10)])
def test_rom_read_without_fused_tree_enqueues_what_it_did(aw, lw):
    """fused_tree=False (the default, and said aloud): one cmux_batch per launch of launches(reads), then the extraction — call for call
    what Rom.read sent before it had the argument; the same in front of a fused tail.  fused_tree=True: one cmux_tree_batch per group in
    place of the upper launches, every other call unchanged."""
    reads, wb = 2, 1 << lw
    slots = np.arange(reads * wb).reshape(reads, wb)
    rom = _rom(aw, lw, reads)
    extract = ("sample_extract_index_keyswitch_batch", "rows", np.repeat([rom.row(r, rom.layout.result) for r in range(reads)], wb).tolist(),
               np.tile(np.arange(wb), reads).tolist(), slots.ravel().tolist(), "arena")
    parent = [("cmux_batch", "selectors", "rows") + _lists(a) for a in rom.launches(reads)] + [extract]
    got = {}
    for kw in ({}, dict(fused_tree=False), dict(fused_tree=True), dict(fused=True), dict(fused=True, fused_tree=True)):
        rom.stream.calls = []
        rom.read(None, "arena", slots, resident=True, **kw)
        got[tuple(sorted(kw.items()))] = rom.stream.calls
    assert got[()] == parent and got[(("fused_tree", False),)] == parent
    upper = len([jobs for jobs in rom.plan if jobs[0].in1 >= 0])
    trees = [("cmux_tree_batch", "selectors", "rows") + _lists(a) for a in rom.tree_launches(reads)]
    assert len(trees) == -(-upper // 4)
    assert got[(("fused_tree", True),)] == trees + parent[upper:]
    fused_tail = got[(("fused", True),)]
    assert fused_tail[:upper] == parent[:upper] and fused_tail[-1] == extract
    assert got[(("fused", True), ("fused_tree", True))] == trees + fused_tail[upper:]
    assert len(got[(("fused", True), ("fused_tree", True))]) == len(trees) + (1 if lw < 10 else 0) + 1   # tree(s), tail, extraction


@pytest.mark.parametrize("aw,dw", [(1, 1), (5, 2), (8, 1)])
def test_ram_read_port_without_fused_tree_enqueues_what_it_did(aw, dw):
    ram = _ram(aw, dw)
    rdata = list(range(dw))
    extract = ("sample_extract_index_keyswitch_batch", "rows", [ram.row(d, ram.layout.result) for d in range(dw)], [0] * dw, rdata, "arena")
    parent = [("cmux_batch", "selectors", "rows") + _lists(a) for a in ram.read_launches()] + [extract]
    ram.read_port("arena", rdata)
    assert ram.stream.calls == parent
    ram.stream.calls = []
    ram.read_port("arena", rdata, fused_tree=False)
    assert ram.stream.calls == parent
    ram.stream.calls = []
    ram.read_port("arena", rdata, fused_tree=True)
    trees = [("cmux_tree_batch", "selectors", "rows") + _lists(a) for a in ram.tree_launches()]
    assert ram.stream.calls == trees + [extract] and len(trees) == -(-aw // 4)
    assert [len(t[3]) for t in trees] == [dw * len(jobs) for jobs, _ in cmux.rom_tree_jobs(ram.plan)]
