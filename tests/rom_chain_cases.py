"""Chosen cases of the fused rotate chain of a ROM read (cmux_fft.hpp: cmux_rotate_chain_kernel; test support for
test_rom_chain_emulation / test_gpu_rom_chain), on the selector store of tests/cmux_cases.py: 128 slots — ZERO, FRESH bits, the worst-case
words 0x7FFF7FFF / 0x80008000 (ALT) and UNIFORM words, the run that ends on the store's last slot.  Pure numpy; the expected words come
from tests/cmux_ref.py applied step by step, never from the code under test.

A job is (steps, [sel per step], [rot per step], src, out):  acc = T[src]; per step acc += S[sel] [.] ((X^rot - 1) acc); T[out] = acc.
A case is (trgsw, T, [batch, ...]), a batch a list of jobs for ONE cmux_rotate_chain_batch; batches run one after the other."""
import numpy as np

import cmux_cases
import cmux_ref
import numpy_tfhe as nt
from cmux_cases import ALT, FRESH, RUN, SLOTS, UNIFORM, ZERO

MANY = 8 * 37 + 5    # 301 jobs: the grid ends in a partial workgroup
QUEUED = 12          # dependent batches without a sync: more than a stream's eight staging slots


def _rows(p, rng, count):
    return rng.integers(0, 1 << 32, size=(count, 2 * p.N), dtype=np.uint64).astype(np.uint32)


def _rots(p, rng, steps):
    return [int(r) for r in rng.integers(1, 2 * p.N, size=steps)]


def rom_rots(p, steps):
    """the ROM's own rotations, highest first: 2N - (N >> bit), bit = 1 .. steps (cmux.rom_read_plan)"""
    return [2 * p.N - (p.N >> bit) for bit in range(1, steps + 1)]


def flat(jobs):
    """a batch as the arguments of Stream.cmux_rotate_chain_batch: (steps, sel, rot, src, out)"""
    return ([j[0] for j in jobs], [s for j in jobs for s in j[1]], [r for j in jobs for r in j[2]], [j[3] for j in jobs], [j[4] for j in jobs])


def as_cmux_launches(jobs):
    """The batch as max(steps) dependent cmux_batch launches of rotate-form jobs (sel, in0, -1, rot, out), the accumulator in the job's
    out row between them: what Rom.read(fused=False) sends."""
    launches = []
    for s in range(max(j[0] for j in jobs)):
        launches.append([(j[1][s], j[3] if s == 0 else j[4], -1, j[2][s], j[4]) for j in jobs if s < j[0]])
    return launches


def chain(p, T, trgsw, job, carry=True, shift_rot=0, ascending=False):
    """The exact reference of one job: `steps` successive cmux_ref.cmux rotate jobs.  The three keyword arguments make the MUTANTS
    test_rom_chain_emulation must tell from the real thing: the accumulator not carried into the next step, the rot of step j + 1 used
    in step j, the selectors taken in ascending order."""
    steps, sels, rots, src, _ = job
    sels = sorted(sels) if ascending else list(sels)
    rots = [rots[min(j + shift_rot, steps - 1)] for j in range(steps)]
    two = np.stack([T[src], T[src]])   # row 0: the accumulator, row 1: T[src] as it was
    for j in range(steps):
        two[0] = cmux_ref.cmux(p, two, trgsw, (sels[j], 0 if carry or j == 0 else 1, -1, rots[j], 0))
    return two[0].copy()


def expected(p, T, trgsw, batches, **mutant):
    """every batch, job by job, in place on a copy of T"""
    want = T.copy()
    for jobs in batches:
        for job in jobs:
            want[job[4]] = chain(p, want, trgsw, job, **mutant)
    return want


def extreme_row(p, rng):
    """A TRLWE row whose difference under rot = N, (X^N - 1) acc = -2 acc, has every gadget digit at -Bg/2 in both polynomials."""
    D = sum((-(1 << (p.Bgbit - 1))) << (32 - j * p.Bgbit) for j in range(1, p.l + 1)) & 0xFFFFFFFF
    assert D % 2 == 0
    half = ((1 << 32) - D) >> 1                                                             # -2 half = D mod 2^32
    row = (half + (rng.integers(0, 2, size=2 * p.N, dtype=np.uint64) << 31)).astype(np.uint32)   # the top bit is free
    diff = (0 - 2 * row.astype(np.uint64)).astype(np.uint32)
    assert np.all(nt.decompose(diff, p.l, p.Bgbit) == -(1 << (p.Bgbit - 1)))
    return row


def _case(keys, tag, rows, make):
    p = keys.params
    rng = np.random.default_rng([7, 0x50, tag])
    T = _rows(p, rng, rows)
    return cmux_cases.selectors(keys), T, make(p, rng, T)


def one(keys):
    """steps = 1"""
    return _case(keys, 1, 3, lambda p, rng, T: [[(1, [UNIFORM + 3], _rots(p, rng, 1), 0, 2)]])


def two(keys):
    """steps = 2, selectors of two kinds"""
    return _case(keys, 2, 3, lambda p, rng, T: [[(2, [FRESH + 1, ALT + 2], _rots(p, rng, 2), 0, 2)]])


def rom12(keys):
    """the tail of a (12, 0) read: 10 steps, rot = 2N - (N >> bit), the selectors of address bits 9 .. 0 (descending slots)"""
    return _case(keys, 3, 3, lambda p, rng, T: [[(10, [FRESH + b for b in range(9, -1, -1)], rom_rots(p, 10), 0, 2)]])


def steps32(keys):
    """32 steps on the store's last 32 slots, ending on the last one"""
    def make(p, rng, T):
        jobs = [(32, list(range(SLOTS - RUN, SLOTS)), _rots(p, rng, 32), 0, 2)]
        assert jobs[0][1][-1] == SLOTS - 1
        return [jobs]
    return _case(keys, 4, 3, make)


def rot_fixed(keys, which):
    """the same rot in every step: 0 (the difference is zero: out == src under any selector), N (the difference is -2 acc), 2N - 1"""
    def make(p, rng, T):
        rot = {"0": 0, "N": p.N, "2N-1": 2 * p.N - 1}[which]
        return [[(3, [UNIFORM + 7, ALT + 4, ALT + 5], [rot] * 3, 0, 2), (2, [FRESH + 2, UNIFORM + 31], [rot] * 2, 1, 1)]]
    return _case(keys, 5 + ("0", "N", "2N-1").index(which), 3, make)


def zero_selector(keys):
    """zero selectors: out == src whatever the rotations"""
    return _case(keys, 8, 3, lambda p, rng, T: [[(4, [ZERO + 5, ZERO, ZERO + 31, ZERO + 7], _rots(p, rng, 4), 0, 2)]])


def extreme(keys):
    """worst-case selector words, an accumulator whose first rotated difference has every digit at -Bg/2"""
    def make(p, rng, T):
        T[0], T[1] = extreme_row(p, rng), extreme_row(p, rng)
        return [[(2, [ALT, ALT + 1], [p.N, p.N], 0, 2), (3, [ALT + 1, ALT, ALT + 3], [p.N, 5, p.N], 1, 1)]]
    return _case(keys, 9, 3, make)


def _mixed(p, rng, count, steps_of):
    """`count` jobs on 2 count + 1 rows: row 0 is the src of every third job, job g otherwise reads row 1 + g; out is a fresh row
    count + 1 + g, or — every other job with a src of its own — the src itself.  Selectors cycle over the four kinds."""
    jobs = []
    for g in range(count):
        steps = steps_of(g)
        shared = g % 3 == 0
        src = 0 if shared else 1 + g
        out = src if (g & 1 and not shared) else count + 1 + g
        base = cmux_cases.RUNS[g % 4] + (g // 4) % (RUN - steps + 1)
        jobs.append((steps, [base + (j * 5 + g) % steps for j in range(steps)], _rots(p, rng, steps), src, out))
    return jobs


def workgroup(keys, count):
    """8 jobs with steps 1 .. 8 side by side in one workgroup; 9: one more in a second, partial one.  Shared src, in place, fresh out."""
    return _case(keys, 10 + count, 2 * count + 1, lambda p, rng, T: [_mixed(p, rng, count, lambda g: 1 + g % 8)])


def many(keys, count=MANY):
    """`count` jobs of 1 or 2 steps, every third with the shared src row 0: 38 workgroups at 301, the last one partial"""
    return _case(keys, 30, 2 * count + 1, lambda p, rng, T: [_mixed(p, rng, count, lambda g: 1 + (g >> 1 & 1))])


def queued(keys):
    """QUEUED dependent batches for ONE stream with no sync between them: two jobs per batch, each with the out row of its predecessor
    in the batch before as src.  Rows 0, 1: the first srcs; 2 + 2 b + i: out of job i of batch b."""
    def make(p, rng, T):
        batches = []
        for b in range(QUEUED):
            steps = 1 + b % 3
            batches.append([(steps, [cmux_cases.RUNS[(b + i + j) % 4] + 2 * b + i for j in range(steps)], _rots(p, rng, steps),
                             i if b == 0 else 2 * b + i, 2 + 2 * b + i) for i in range(2)])
        return batches
    return _case(keys, 31, 2 + 2 * QUEUED, make)


# the cases the emulation runs against the reference on both parameter sets, and the rows that must come back as an ORIGINAL row
CPU_CASES = {"steps1": one, "steps2": two, "rom12": rom12, "steps32": steps32, "rot0": lambda k: rot_fixed(k, "0"),
             "rotN": lambda k: rot_fixed(k, "N"), "rot2N-1": lambda k: rot_fixed(k, "2N-1"), "zero": zero_selector, "extreme": extreme}
IDENTITIES = {"rot0": ((2, 0), (1, 1)), "zero": ((2, 0),)}   # case -> (out row, the row of the original T it equals)
# what the GPU runs at the 128-bit set: the batch shapes on top
GPU_CASES = {"one": one, "wg8": lambda k: workgroup(k, 8), "wg9": lambda k: workgroup(k, 9), "many": many, "steps32": steps32,
             "rot0": lambda k: rot_fixed(k, "0"), "rotN": lambda k: rot_fixed(k, "N"), "queued": queued}

_expected = {}


def expected_of(keys, name):
    """(case, expected rows) of a named case, computed once per key set and shared by the tests that need it; never written"""
    key = (id(keys), name)
    if key not in _expected:
        case = {**CPU_CASES, **GPU_CASES}[name](keys)
        want = expected(keys.params, case[1], case[0], case[2])
        want.setflags(write=False)
        case[1].setflags(write=False)
        _expected[key] = (keys, case, want)
    return _expected[key][1], _expected[key][2]
