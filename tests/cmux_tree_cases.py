"""Chosen cases of the fused CMUX read tree (cmux_fft.hpp: cmux_tree_kernel; test support for test_cmux_tree_emulation /
test_gpu_cmux_tree).  Pure numpy apart from the client library's encryptions; the expected words come from tests/cmux_ref.py applied
level by level on a list of candidate rows, never from the code under test.

Selector store, 32 slots:
    ZERO      0 ..  3   noise-free zeros: every level keeps in0, the result is leaf 0 exactly
    F0        4 ..  7   fresh encryptions of 0, 0, 0, 0: the path to the FIRST leaf
    F1        8 .. 11   fresh encryptions of 1, 1, 1, 1: the path to the LAST leaf
    ZIG      12 .. 15   fresh encryptions of 0, 1, 0, 1: a path that alternates in0 / in1
    ZAG      16 .. 19   fresh encryptions of 1, 0, 1, 0: the other alternating path
    ALT      20 .. 23   the worst-case words 0x7FFF7FFF (even slot) and 0x80008000 (odd slot) in every coefficient
    UNIFORM  24 .. 31   uniform words; the run that ends on the store's last slot (a read past a descriptor's range returns zero and would
                        pass for a zero selector: the one kind that could hide it)

A job is (sel0, levels, first, out): the leaves T[first .. first + 2^levels) halved `levels` times, level b with selector slot sel0 + b,
job i of a level the CMUX (in0 = candidate 2 i, in1 = candidate 2 i + 1); T[out] = the row left.  With selector bits s_0 .. s_(n-1) the
tree selects leaf sum(s_b << b).  A case is (trgsw, T, [batch, ...]), a batch a list of jobs for ONE cmux_tree_batch."""
import numpy as np

import cmux_ref
from iyokan_amd import client

ZERO, F0, F1, ZIG, ZAG, ALT, UNIFORM, SLOTS = 0, 4, 8, 12, 16, 20, 24, 32
FRESH_BITS = {F0: (0, 0, 0, 0), F1: (1, 1, 1, 1), ZIG: (0, 1, 0, 1), ZAG: (1, 0, 1, 0)}
LEVELS = (1, 2, 3, 4)   # the only sizes of the wave pattern
LEAVES = 16

_store = {}


def selectors(keys, seed=11):
    """u32 [SLOTS][(k+1) l][k+1][N], torus domain; computed once per key set, never written by a caller."""
    key = (id(keys), seed)
    if key not in _store:
        p = keys.params
        rng = np.random.default_rng(seed)
        trgsw = np.zeros((SLOTS, p.trgsw_rows, p.k + 1, p.N), dtype=np.uint32)
        for run, bits in FRESH_BITS.items():
            trgsw[run : run + 4] = client.encrypt_trgsw(keys, list(bits), seed=seed + run)
        trgsw[ALT : ALT + 4 : 2] = 0x7FFF7FFF
        trgsw[ALT + 1 : ALT + 4 : 2] = 0x80008000
        trgsw[UNIFORM:] = rng.integers(0, 1 << 32, size=trgsw[UNIFORM:].shape, dtype=np.uint64).astype(np.uint32)
        trgsw.setflags(write=False)
        _store[key] = (keys, trgsw)   # the key set is kept alive with its entry: an id is never reused under it
    return _store[key][1]


def selected_leaf(run, levels):
    """the leaf the fresh run's first `levels` bits select"""
    return sum(b << k for k, b in enumerate(FRESH_BITS[run][:levels]))


def _rows(p, rng, count):
    return rng.integers(0, 1 << 32, size=(count, 2 * p.N), dtype=np.uint64).astype(np.uint32)


def tree(p, T, trgsw, job, far_partner=False, same_selector=False, swap_upper=False, stale_partner=False):
    """The exact reference of one job: `levels` rounds of cmux_ref.cmux over the list of candidate rows.  The keyword arguments make
    the MUTANTS the comparisons must tell from the real thing, each a fault of the kernel's wave pattern restated on candidates: at the
    levels b >= 1 in1 taken from the wave 2^b (not 2^(b-1)) further on, i.e. candidate 2 i + 2 (a zero row where there is none); the
    selector sel0 at every level; in0 / in1 swapped at the levels b >= 1 only; in1 at a level b >= 1 as its wave held it BEFORE level
    b - 1 — its in0 of that level — which is what a missing barrier lets a wave read."""
    sel0, levels, first, _ = job
    cand = [T[first + k] for k in range(1 << levels)]
    before = cand
    for b in range(levels):
        nxt = []
        for i in range(len(cand) // 2):
            in0, in1 = cand[2 * i], cand[2 * i + 1]
            if b >= 1:
                if far_partner:
                    in1 = cand[2 * i + 2] if 2 * i + 2 < len(cand) else np.zeros_like(in0)
                if stale_partner:
                    in1 = before[2 * (2 * i + 1)]
                if swap_upper:
                    in0, in1 = in1, in0
            nxt.append(cmux_ref.cmux(p, np.stack([in0, in1]), trgsw, (sel0 if same_selector else sel0 + b, 0, 1, 0, 0)))
        before, cand = cand, nxt
    return cand[0]


def expected(p, T, trgsw, batches, **mutant):
    """every batch in place on a copy of T; the jobs of a batch all read the rows as they were in front of it"""
    want = T.copy()
    for jobs in batches:
        outs = [tree(p, want, trgsw, job, **mutant) for job in jobs]
        for job, row in zip(jobs, outs):
            want[job[3]] = row
    return want


def as_cmux_launches(jobs, scratch):
    """The batch as max(levels) dependent cmux_batch launches of two-row jobs (sel, in0, in1, 0, out): job g keeps the candidates between
    its levels in the 14 rows from scratch + 14 g on (8 + 4 + 2) and writes its out row in its last level.  What Rom.read and
    Ram.read_port send without fused_tree, on rows of their own."""
    launches = [[] for _ in range(max(j[1] for j in jobs))]
    for g, (sel0, levels, first, out) in enumerate(jobs):
        cand = [first + k for k in range(1 << levels)]
        base = scratch + 14 * g
        for b in range(levels):
            outs = [out] if b == levels - 1 else [base + i for i in range(len(cand) // 2)]
            launches[b].extend((sel0 + b, cand[2 * i], cand[2 * i + 1], 0, outs[i]) for i in range(len(outs)))
            base += len(outs)
            cand = outs
    return launches


def _case(keys, tag, rows, make):
    p = keys.params
    rng = np.random.default_rng([11, 0x7E, tag])
    T = _rows(p, rng, rows)
    return selectors(keys), T, make(p, rng, T)


def side_by_side(keys, run):
    """levels 1 .. 4 side by side in one batch on selector run `run`, all four jobs on the leaves 0 .. (sharing them), outs 16 .. 19.
    The UNIFORM run is taken so that every job ends on the store's last slot."""
    def make(p, rng, T):
        return [[(SLOTS - n if run == UNIFORM else run, n, 0, LEAVES + n - 1) for n in LEVELS]]
    return _case(keys, run, LEAVES + 4, make)


def one_hot(keys, run):
    """Fresh selectors on leaves that ENCRYPT a bit each (client.encrypt_ram_trlwe: the bit at coefficient 0): job n - 1 (levels n, leaves
    16 (n - 1) .., out 64 + n - 1) has a 1 in the leaf its path selects and 0 in every other, so its result decrypts to 1."""
    p = keys.params
    bits = np.zeros(4 * LEAVES + 4, dtype=np.uint8)
    for n in LEVELS:
        bits[LEAVES * (n - 1) + selected_leaf(run, n)] = 1
    T = client.encrypt_ram_trlwe(keys, bits, seed=100 + run).reshape(-1, 2 * p.N).copy()
    return selectors(keys), T, [[(run, n, LEAVES * (n - 1), 4 * LEAVES + n - 1) for n in LEVELS]]


def extreme(keys):
    """worst-case selector words on leaves whose first-level differences have every digit at its extreme (-Bg/2 in the pair 0 / 1, +Bg/2
    - 1 in the pair 2 / 3)"""
    def make(p, rng, T):
        T[0], T[1] = cmux_ref.extreme_pair(p, rng, top=False)
        T[2], T[3] = cmux_ref.extreme_pair(p, rng, top=True)
        return [[(ALT, n, 0, LEAVES + n - 1) for n in LEVELS]]
    return _case(keys, 40, LEAVES + 4, make)


def in_place(keys):
    """out == the job's own first leaf (levels 4 on rows 0 .. 15, levels 2 on rows 16 .. 19), and out == its own LAST leaf (levels 1 on
    rows 20, 21)"""
    return _case(keys, 41, 22, lambda p, rng, T: [[(UNIFORM, 4, 0, 0), (ZAG, 2, 16, 16), (UNIFORM + 5, 1, 20, 21)]])


def single(keys):
    """1 job of 4 levels"""
    return _case(keys, 42, LEAVES + 1, lambda p, rng, T: [[(UNIFORM + 1, 4, 0, LEAVES)]])


def nine(keys):
    """9 jobs, one workgroup each, that share their leaves: levels cycle over 1 .. 4, job g starts at leaf (2 g) % 16 rounded down to its
    own size, selectors of every kind, outs 16 .. 24"""
    def make(p, rng, T):
        runs = (UNIFORM, F1, ALT, ZIG, ZERO, UNIFORM + 4, ZAG, F0, UNIFORM + 3)
        jobs = []
        for g, run in enumerate(runs):
            n = LEVELS[g % 4]
            jobs.append((run, n, ((2 * g) % LEAVES) >> n << n, LEAVES + g))
        return [jobs]
    return _case(keys, 43, LEAVES + 9, make)


def two_groups(keys):
    """two dependent batches, cut as cmux.rom_tree_jobs cuts a deep read: four jobs of 2 levels into rows 16 .. 19, then one job of 2
    levels on those rows into row 16, its own first leaf"""
    return _case(keys, 44, LEAVES + 4, lambda p, rng, T: [[(UNIFORM, 2, 4 * i, LEAVES + i) for i in range(4)], [(UNIFORM + 2, 2, LEAVES, LEAVES)]])


CPU_CASES = {"zero": lambda k: side_by_side(k, ZERO), "uniform": lambda k: side_by_side(k, UNIFORM), "alt": extreme,
             "first": lambda k: one_hot(k, F0), "last": lambda k: one_hot(k, F1), "zig": lambda k: one_hot(k, ZIG),
             "zag": lambda k: one_hot(k, ZAG), "in_place": in_place, "two_groups": two_groups}
GPU_CASES = {"single": single, "side_by_side": lambda k: side_by_side(k, UNIFORM), "nine": nine, "in_place": in_place,
             "zero": lambda k: side_by_side(k, ZERO), "last": lambda k: one_hot(k, F1), "two_groups": two_groups}
# case -> (out row, the row of the original T it equals): the zero selector gives leaf 0 exactly
IDENTITIES = {"zero": tuple((LEAVES + n - 1, 0) for n in LEVELS)}

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
