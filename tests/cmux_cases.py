"""Chosen cases of the CMUX kernels (test support for test_ram_emulation / test_cmux_emulation / test_gpu_cmux_edges), the role
tests/ks_words.py plays for the key switch: one selector store and, per case, TRLWE rows and job lists, deterministically from a seed.
Pure numpy apart from client.encrypt_trgsw — no GPU, no emulation, no reference: the CPU emulation tests and the GPU tests run
identical words through the code under test and compare with tests/ram_ref.py / tests/cmux_ref.py themselves.

Selector store: four runs of RUN = 32 consecutive slots, 128 slots in all.
    ZERO     0 ..  31   noise-free zeros: a step keeps the accumulator (pattern bit 0) or takes T[mem] (bit 1) exactly
    FRESH   32 ..  63   fresh encryptions of the bits of ADDRESS, bit j in slot FRESH + j
    ALT     64 ..  95   the worst-case words 0x7FFF7FFF (even slot) and 0x80008000 (odd slot) in every coefficient
    UNIFORM 96 .. 127   uniform words
The run that ends on the store's last slot is the UNIFORM one on purpose: a buffer read past a descriptor's range returns zero, so a
range or offset error at the last slot would read as a ZERO selector — the one kind that could hide it.

Chain jobs are (sel0, steps, pattern, src, mem, out), CMUX jobs (sel, in0, in1, rot, out)."""
import numpy as np

import cmux_ref
from iyokan_amd import client

RUN = 32
ZERO, FRESH, ALT, UNIFORM = 0, 32, 64, 96
RUNS = (ZERO, FRESH, ALT, UNIFORM)
SLOTS = 4 * RUN
ADDRESS = 0xC35A962D
A_STEPS = (8, 16, 31, 32)
A_PATTERNS = (0, 0xFFFFFFFF, 0x80000001, 0xA5A5A5A5, 0x7FFFFFFF)
B_STEPS = (1, 32, 2, 31, 5, 8, 16, 3, 32)
B_RUNS = (ZERO, ALT, FRESH, UNIFORM, ALT, ZERO, FRESH, ALT, UNIFORM)
C_JOBS = 8 * 37 + 5
E_BATCHES = 12

_store = {}


def selectors(keys, seed=7):
    """u32 [SLOTS][(k+1) l][k+1][N], torus domain; computed once per key set and seed, never written by a caller."""
    key = (id(keys), seed)
    if key not in _store:
        p = keys.params
        rng = np.random.default_rng(seed)
        trgsw = np.zeros((SLOTS, p.trgsw_rows, p.k + 1, p.N), dtype=np.uint32)
        trgsw[FRESH : FRESH + RUN] = client.encrypt_trgsw(keys, [(ADDRESS >> j) & 1 for j in range(RUN)], seed=seed + 1)
        trgsw[ALT : ALT + RUN : 2] = 0x7FFF7FFF
        trgsw[ALT + 1 : ALT + RUN : 2] = 0x80008000
        trgsw[UNIFORM:] = rng.integers(0, 1 << 32, size=trgsw[UNIFORM:].shape, dtype=np.uint64).astype(np.uint32)
        trgsw.setflags(write=False)
        _store[key] = (keys, trgsw)   # the key set is kept alive with its entry: an id is never reused under it
    return _store[key][1]


def _rows(p, rng, count):
    return rng.integers(0, 1 << 32, size=(count, 2 * p.N), dtype=np.uint64).astype(np.uint32)


def _chain_rows(p, rng, specs):
    """Chain jobs from (sel0, steps, pattern) on 4 count + 2 rows, the layout of test_gpu_ram._chain_batch.  Row 0 is the src of every
    third job; job g otherwise reads src 1 + g; mem = count + 1 + g; out is the mem row (the RAM cell), a fresh row 2 count + 1 + g,
    or the job's own src (the mem row where the src is shared).  Rows 3 count + 1 .. 4 count hold the accumulators of an unfused
    run; the last row belongs to no job."""
    count = len(specs)
    jobs = []
    for g, (sel0, steps, pattern) in enumerate(specs):
        shared = g % 3 == 0
        src, mem = (0 if shared else 1 + g), count + 1 + g
        out = (mem, 2 * count + 1 + g, mem if shared else src)[(g // 2) % 3]
        jobs.append((sel0, steps, pattern & ((1 << steps) - 1), src, mem, out))
    return jobs, _rows(p, rng, 4 * count + 2)


def _extreme(p, rng, T, jobs, picks):
    """Every digit of the FIRST difference of job g at its extreme: mem - acc where pattern bit 0 is 0, acc - mem where it is 1."""
    for g, top in picks:
        assert jobs[g][3] != 0   # a src of its own
        x, y = cmux_ref.extreme_pair(p, rng, top=top)
        T[jobs[g][3]], T[jobs[g][4]] = (y, x) if jobs[g][2] & 1 else (x, y)


def accumulator_row(jobs, g):
    """Row of the accumulator of job g of a case-A / case-B batch when the chain is sent step by step."""
    return 3 * len(jobs) + 1 + g


def case_a(keys, steps, seed=7):
    """Long chains: one job per pattern of A_PATTERNS (masked to `steps` bits) on each selector run, 20 jobs.  Every chain ends on its
    run's last slot, so the UNIFORM ones have sel0 + steps == SLOTS.  Returns (trgsw, T, [jobs])."""
    assert steps in A_STEPS
    p = keys.params
    rng = np.random.default_rng([seed, 0xA, steps])
    specs = [(run + RUN - steps, steps, pat) for run in RUNS for pat in A_PATTERNS]
    jobs, T = _chain_rows(p, rng, specs)
    _extreme(p, rng, T, jobs, ((4, False), (5, True)))
    assert any(j[0] + j[1] == SLOTS for j in jobs)
    return selectors(keys, seed), T, [jobs]


def case_b(keys, seed=7):
    """Mixed steps in one workgroup (and one wave of the next): 9 jobs with steps B_STEPS, the top used bit of every pattern set,
    selectors from different runs; the chains of odd jobs end on their run's last slot."""
    p = keys.params
    rng = np.random.default_rng([seed, 0xB])
    specs = []
    for g, (steps, run) in enumerate(zip(B_STEPS, B_RUNS)):
        pattern = (1 << (steps - 1)) | (0xA5A5A5A5 >> g)
        specs.append((run + (RUN - steps if g & 1 or steps == RUN else g), steps, pattern))
    jobs, T = _chain_rows(p, rng, specs)
    _extreme(p, rng, T, jobs, ((1, False), (8, True)))   # the two 32-step jobs
    assert all((j[2] >> (j[1] - 1)) & 1 for j in jobs) and jobs[8][0] + jobs[8][1] == SLOTS
    return selectors(keys, seed), T, [jobs]


def case_c(keys, seed=7, count=C_JOBS):
    """Many workgroups: `count` jobs of 3 steps, sel0 cycling over the runs (and inside them), every third job with src row 0; C_JOBS
    = 8 * 37 + 5 ends the grid in a partial workgroup."""
    p = keys.params
    rng = np.random.default_rng([seed, 0xC, count])
    specs = [(RUNS[g % 4] + (g // 4) % (RUN - 2), 3, (g * 5 + g // 8) & 7) for g in range(count)]
    jobs, T = _chain_rows(p, rng, specs)
    return selectors(keys, seed), T, [jobs]


# case D: (out row, the row of the ORIGINAL T it must equal word for word)
D_IDENTITIES = ((6, 1), (2, 2), (7, 3), (5, 4), (8, 4))


def case_d(keys, seed=7):
    """Degenerate chains on 9 rows: src == mem with a fresh out; src == mem == out; chains entirely on ZERO selectors with an
    all-zero pattern (the result is T[src]) and with bit steps - 1 set (the result is T[mem]), at 7 and at 32 steps."""
    p = keys.params
    rng = np.random.default_rng([seed, 0xD])
    T = _rows(p, rng, 9)
    jobs = [(UNIFORM + 20, 5, 0b10110, 1, 1, 6), (ALT + 24, 8, 0xA5, 2, 2, 2), (ZERO, 7, 0, 3, 4, 7), (ZERO + 25, 7, 0x40, 3, 4, 5),
            (ZERO, 32, 0x80000000, 3, 4, 8)]   # only the top bit: were it lost, the result would be T[src]
    return selectors(keys, seed), T, [jobs]


def case_e(keys, seed=7):
    """E_BATCHES dependent chain batches for ONE stream with no sync between them (more than the stream's ring of staging slots): two
    jobs per batch, each with the out row of its predecessor in the previous batch as src.  Rows 0, 1: the first srcs; 2 .. 5: mem
    rows; 6 + 2 b + i: out of job i of batch b."""
    p = keys.params
    rng = np.random.default_rng([seed, 0xE])
    T = _rows(p, rng, 6 + 2 * E_BATCHES)
    batches = []
    for b in range(E_BATCHES):
        steps = 1 + b % 4
        batches.append([(RUNS[(b + i) % 4] + 2 * b + i, steps, (0x2D3 >> (b + i)) & ((1 << steps) - 1), (i if b == 0 else 4 + 2 * b + i),
                         2 + (b + 2 * i) % 4, 6 + 2 * b + i) for i in range(2)])
    return selectors(keys, seed), T, batches


CHAIN_CASES = {"A8": lambda k: case_a(k, 8), "A16": lambda k: case_a(k, 16), "A31": lambda k: case_a(k, 31), "A32": lambda k: case_a(k, 32),
               "B": case_b, "C": case_c, "D": case_d, "E": case_e}


# cmux_batch cases: (out row, the row of the ORIGINAL T it must equal word for word) after the first batch
CMUX_IDENTITIES = ((18, 0), (1, 1), (19, 2), (3, 3))
LAST = SLOTS - 1


def cmux_cases(keys, seed=7):
    """Two cmux_batch launches on 27 rows.  The first: in0 == in1 with a fresh out and with out the row itself; the rotate form with
    rot = 0, fresh out and in place (the difference is zero in all four: the output is T[in0]); one job on the last selector slot.
    The second: nine jobs (a workgroup and one wave) that ALL use the last slot, two-row and rotate forms, g reads rows g and 9 + g
    and writes 18 + g, its in0 or its in1.  Returns (trgsw, T, [jobs, jobs])."""
    p = keys.params
    N = p.N
    rng = np.random.default_rng([seed, 0xF])
    T = _rows(p, rng, 27)
    first = [(FRESH + 1, 0, 0, 0, 18), (UNIFORM + 3, 1, 1, 0, 1), (ALT, 2, -1, 0, 19), (ALT + 1, 3, -1, 0, 3), (LAST, 4, 5, 0, 20)]
    rots = (1, N - 1, 2 * N - 1)
    second = []
    for g in range(9):
        rotate = g % 3 == 2
        out = (18 + g, g, g if rotate else 9 + g)[(g // 3 + g) % 3]
        second.append((LAST, g, -1 if rotate else 9 + g, rots[g // 3] if rotate else 0, out))
    T[6], T[15] = cmux_ref.extreme_pair(p, rng, top=False)
    T[7], T[16] = cmux_ref.extreme_pair(p, rng, top=True)
    return selectors(keys, seed), T, [first, second]
