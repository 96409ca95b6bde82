"""The lane batches of the CMUX memories behind tests/test_cmux_lane_jobs.py (CPU: csrc/cmux_lane_jobs.hpp and batch_args.hpp's
*_lanes_args through libiyk_emul.so) and tests/test_gpu_cmux_lanes.py (the four iyk_hip_cmux_*_batch_lanes calls on the GPU).

A case is the argument arrays of ONE lane of one of the four CMUX families, a lane count, a selector stride and a row stride.  Its
reference is the FLAT batch: `lanes` copies of the arrays, copy r with + r * sel_stride on every selector slot and + r * row_stride on
every non-negative row (replicate) — what a caller had to build on the host before these calls, what the parent call runs and what the
parent check (iyk_emul_check_cmux_*) builds its job list from.  Every comparison is word for word.

Families and their arrays, in the order of the C calls:
    0  cmux_batch               sel, in0, in1, rot, out
    1  cmux_chain_batch         sel0, steps, pattern, src, mem, out
    2  cmux_rotate_chain_batch  steps, sel, rot, src, out        (sel / rot: sum(steps) entries)
    3  cmux_tree_batch          sel0, levels, first, out"""
import ctypes
import os

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OK, INVALID = 0, -1
MAX_ROW_BATCH = 1 << 24
CMUX, CHAIN, ROT, TREE = 0, 1, 2, 3
FAMILY_NAME = {CMUX: "cmux_batch", CHAIN: "cmux_chain_batch", ROT: "cmux_rotate_chain_batch", TREE: "cmux_tree_batch"}
JOB_WORDS = {CMUX: 5, CHAIN: 6, ROT: 4, TREE: 4}   # 32-bit words of a CmuxJob / CmuxChainJob / CmuxRotChainJob / CmuxTreeJob
STEP_WORDS = 2                                     # of a CmuxRotStep
# which arrays of a family are selector slots / rows (the rest is the same in every lane)
SEL_ARRAYS = {CMUX: (0,), CHAIN: (0,), ROT: (1,), TREE: (0,)}
ROW_ARRAYS = {CMUX: (1, 2, 4), CHAIN: (3, 4, 5), ROT: (3, 4), TREE: (2, 3)}

_i32p, _u32p, u64 = ctypes.POINTER(ctypes.c_int32), ctypes.POINTER(ctypes.c_uint32), ctypes.c_uint64


def case(name, family, arrays, lanes, sel_stride, row_stride, trgsw_slots=None, trlwe_slots=None):
    """arrays: one lane's, as lists; the stores default to what `lanes` lanes need and nothing more"""
    arrays = tuple(np.array(a, dtype=np.int32) for a in arrays)
    sel_top, row_top = reach(family, arrays)
    return dict(name=name, family=family, arrays=arrays, lanes=lanes, sel_stride=sel_stride, row_stride=row_stride,
                trgsw_slots=sel_top + 1 + (lanes - 1) * sel_stride if trgsw_slots is None else trgsw_slots,
                trlwe_slots=row_top + 1 + (lanes - 1) * row_stride if trlwe_slots is None else trlwe_slots)


def reach(family, arrays):
    """(highest selector slot, highest row) one lane's list touches"""
    a = [np.asarray(x, dtype=np.int64) for x in arrays]
    if family == CMUX:
        return int(a[0].max()), int(max(a[1].max(), a[2].max(), a[4].max()))
    if family == CHAIN:
        return int((a[0] + a[1] - 1).max()), int(max(a[3].max(), a[4].max(), a[5].max()))
    if family == ROT:
        return int(a[1].max()), int(max(a[3].max(), a[4].max()))
    return int((a[0] + a[1] - 1).max()), int(max((a[2] + (1 << a[1]) - 1).max(), a[3].max()))


def replicate(family, arrays, lanes, sel_stride, row_stride):
    """the arrays of all lanes, lane-major: the flat batch a caller built on the host before the _lanes calls"""
    out = []
    for i, a in enumerate(arrays):
        a = np.asarray(a, dtype=np.int64)
        stride = sel_stride if i in SEL_ARRAYS[family] else row_stride if i in ROW_ARRAYS[family] else 0
        copies = [np.where(a < 0, a, a + r * stride) if stride else a for r in range(lanes)]
        out.append(np.concatenate(copies).astype(np.int32))
    return tuple(out)


# ---- one lane's lists ------------------------------------------------------------------------------------------------------------------
# CMUX: 3 jobs, one past nothing yet — with 3 lanes 9 jobs, one past a workgroup's 8.  Job 1 is the rotate form (in1 = -1) beside two-row
# jobs, job 2 writes over its own input.  Rows 0 .. 6.
CMUX3 = ([0, 1, 2], [0, 2, 5], [1, -1, 6], [0, 100, 0], [4, 3, 5])
# CHAIN: the write-back of a 2 x 1 RAM (two cells, one address bit): src = row 2, cells 0 and 1 in place
CHAIN_RAM21 = ([0, 0], [1, 1], [0, 1], [2, 2], [0, 1], [0, 1])
# ROT: two chains of 3 and 1 steps: `first` of the second job is 3, and lane r's jobs start at r * 4
ROT31 = ([3, 1], [0, 1, 2, 1], [2044, 2040, 2032, 1024], [0, 1], [2, 1])
# TREE: a 4-level tree over leaves 0 .. 15 into row 16 and a 1-level tree over leaves 17, 18 into its own leaf 17
TREE41 = ([0, 2], [4, 1], [0, 17], [16, 17])


def _wide(count):
    """`count` two-row CMUX jobs over shared inputs 0, 1: job g writes row 2 + g"""
    g = np.arange(count)
    return (g % 3, np.zeros(count, int), np.ones(count, int), np.zeros(count, int), 2 + g)


def _cases():
    out = []
    for lanes in (1, 2, 5, 7):
        out.append(case(f"cmux3-x{lanes}", CMUX, CMUX3, lanes, 3, 7))
        out.append(case(f"chain-ram21-x{lanes}", CHAIN, CHAIN_RAM21, lanes, 1, 3))
        out.append(case(f"rot31-x{lanes}", ROT, ROT31, lanes, 3, 3))
        out.append(case(f"tree41-x{lanes}", TREE, TREE41, lanes, 4, 19))
    out.append(case("cmux3-x3", CMUX, CMUX3, 3, 3, 7))                                         # 9 jobs: one past a workgroup's 8
    out.append(case("cmux3-wide-stride", CMUX, CMUX3, 5, 3, 11))                               # row_stride larger than the span
    # stage-major selectors: a port at sel_base 5 of a stage of 3 bits per lane — sel_stride 3 < sel_base
    out.append(case("cmux-stage-major", CMUX, ([5, 6, 7], CMUX3[1], CMUX3[2], CMUX3[3], CMUX3[4]), 2, 3, 7))
    out.append(case("chain-stage-major", CHAIN, ([5, 5], [1, 1], [0, 1], [2, 2], [0, 1], [0, 1]), 2, 3, 3))
    out.append(case("rot-stage-major", ROT, ([3, 1], [5, 6, 7, 6], ROT31[2], ROT31[3], ROT31[4]), 2, 3, 3))
    out.append(case("tree-stage-major", TREE, ([5, 7], TREE41[1], TREE41[2], TREE41[3]), 2, 4, 19))
    out.append(case("37x7", CMUX, _wide(37), 7, 3, 39))                                        # 259 jobs: one past a 256-thread block
    out.append(case("rot-37x7", ROT, ([1] * 37, [g % 3 for g in range(37)], [1] * 37, [0] * 37, list(range(1, 38))), 7, 3, 38))
    return {c["name"]: c for c in out}


CASES = _cases()
ONE_LANE = [n for n, c in CASES.items() if c["lanes"] == 1]


# ---- libiyk_emul.so ------------------------------------------------------------------------------------------------------------------
_EMUL = {}


def emul(path=None):
    path = path or os.path.join(ROOT, "iyokan_amd", "lib", "libiyk_emul.so")
    if path not in _EMUL:
        _EMUL[path] = ctypes.CDLL(path)
    return _EMUL[path]


def _p(a):
    return a.ctypes.data_as(_i32p)


def lanes_args(family, arrays, trgsw_slots, trlwe_slots, lanes, sel_stride, row_stride, lib=None):
    """iyk_emul_cmux_lanes_args -> (code, text, jobs [n][W] and steps [ns][2] of ONE lane, a list left non-empty by a refusal)"""
    L = lib or emul()
    arrays = [np.ascontiguousarray(a, dtype=np.int32) for a in arrays]
    count = len(arrays[0])
    ptrs = [_p(a) for a in arrays] + [None] * (6 - len(arrays))
    msg = ctypes.create_string_buffer(256)
    cap = 8 * (sum(len(a) for a in arrays) + 8)
    words = np.zeros(cap, dtype=np.uint32)
    counts = (u64 * 3)()
    L.iyk_emul_cmux_lanes_args.restype = ctypes.c_int
    code = L.iyk_emul_cmux_lanes_args(family, u64(trgsw_slots), u64(trlwe_slots), u64(count), *ptrs, u64(lanes), u64(sel_stride), u64(row_stride),
                                      msg, u64(256), words.ctypes.data_as(_u32p), u64(cap), counts)
    n, ns = int(counts[0]), int(counts[1])
    W = JOB_WORDS[family]
    jobs = words[: n * W].view(np.int32).reshape(n, W).copy()
    steps = words[n * W: n * W + ns * STEP_WORDS].view(np.int32).reshape(ns, STEP_WORDS).copy()
    return code, msg.value.decode(), (jobs, steps), bool(counts[2])


def expand(family, jobs, steps, lanes, sel_stride, row_stride, threads=0, lib=None):
    """iyk_emul_cmux_lane_jobs: the lists of all lanes from those of one; threads > 0: cmux_lane_jobs_kernel's traversal with that many"""
    L = lib or emul()
    W = JOB_WORDS[family]
    words1 = np.concatenate([jobs.ravel(), steps.ravel()]).astype(np.int32).view(np.uint32)
    counts1 = (u64 * 2)(len(jobs), len(steps))
    out = np.full((len(jobs) * W + len(steps) * STEP_WORDS) * lanes, 0xDEADBEEF, dtype=np.uint32)
    L.iyk_emul_cmux_lane_jobs.restype = ctypes.c_int
    assert L.iyk_emul_cmux_lane_jobs(family, words1.ctypes.data_as(_u32p), counts1, u64(lanes), u64(sel_stride), u64(row_stride), u64(threads),
                                     out.ctypes.data_as(_u32p)) == 0
    n = len(jobs) * lanes
    return out[: n * W].view(np.int32).reshape(n, W), out[n * W:].view(np.int32).reshape(len(steps) * lanes, STEP_WORDS)


def parent_lists(family, arrays, trgsw_slots, trlwe_slots, lib=None):
    """The parent check (iyk_emul_check_cmux_*) on flat arrays -> (code, text, (jobs, steps))"""
    L = lib or emul()
    arrays = [np.ascontiguousarray(a, dtype=np.int32) for a in arrays]
    count = len(arrays[0])
    msg = ctypes.create_string_buffer(256)
    cap = 8 * (sum(len(a) for a in arrays) + 8)
    words = np.zeros(cap, dtype=np.uint32)
    counts = (u64 * 2)()
    f = getattr(L, {CMUX: "iyk_emul_check_cmux_batch", CHAIN: "iyk_emul_check_cmux_chain_batch", ROT: "iyk_emul_check_cmux_rotate_chain_batch",
                    TREE: "iyk_emul_check_cmux_tree_batch"}[family])
    f.restype = ctypes.c_int
    code = f(u64(trgsw_slots), u64(trlwe_slots), u64(count), *[_p(a) for a in arrays], msg, u64(256), words.ctypes.data_as(_u32p), u64(cap), counts)
    n, ns = int(counts[0]), int(counts[1]) if family == ROT else 0
    W = JOB_WORDS[family]
    jobs = words[: n * W].view(np.int32).reshape(n, W).copy()
    steps = words[n * W: n * W + ns * STEP_WORDS].view(np.int32).reshape(ns, STEP_WORDS).copy()
    return code, msg.value.decode(), (jobs, steps)


def lane_lists(c, threads=0, lib=None):
    """the expanded lists of a case: *_lanes_args for one lane's lists, then the expansion (lanes == 1: the staged list is the batch)"""
    code, text, (jobs, steps), _ = lanes_args(c["family"], c["arrays"], c["trgsw_slots"], c["trlwe_slots"], c["lanes"], c["sel_stride"], c["row_stride"],
                                              lib=lib)
    assert code == OK, text
    if c["lanes"] == 1:
        return jobs, steps
    return expand(c["family"], jobs, steps, c["lanes"], c["sel_stride"], c["row_stride"], threads=threads, lib=lib)


def flat_lists(c):
    """what the parent check builds from the host-replicated arrays, against the same stores"""
    rep = replicate(c["family"], c["arrays"], c["lanes"], c["sel_stride"], c["row_stride"])
    code, text, lists = parent_lists(c["family"], rep, c["trgsw_slots"], c["trlwe_slots"])
    assert code == OK, text
    return lists


def first_difference(c, lib=None):
    """None, or (list, job index, got, want) of the first word that differs between the expansion and the flat batch"""
    got, want = lane_lists(c, lib=lib), flat_lists(c)
    for which, g, w in zip(("jobs", "steps"), got, want):
        if g.shape != w.shape:
            return which, "shape", g.shape, w.shape
        bad = np.flatnonzero((g != w).any(axis=1)) if len(g) else []
        if len(bad):
            return which, int(bad[0]), g[bad[0]].tolist(), w[bad[0]].tolist()
    return None


# ---- refusals and their accepted neighbours: (name, family, arrays, trgsw_slots, trlwe_slots, lanes, sel_stride, row_stride[, word]) ----
def _with(arrays, **kw):
    return tuple(kw.get(f"a{i}", a) for i, a in enumerate(arrays))


REFUSALS = [
    ("lanes-zero", CMUX, CMUX3, 64, 64, 0, 3, 7, "lanes is zero"),
    ("row-stride-zero", CMUX, CMUX3, 64, 64, 2, 3, 0, "stride is zero"),
    ("sel-stride-zero", TREE, TREE41, 64, 64, 2, 0, 19, "stride is zero"),
    ("lanes-2^31", CMUX, CMUX3, 64, 64, 1 << 31, 3, 7, "count x lanes"),
    ("count-x-lanes-one-more", CMUX, _wide(1 << 12), 1 << 13, 1 << 27, (1 << 12) + 1, 1, 1 << 13, "count x lanes"),
    # the span rule: rows 0 .. 6 span 6; a stride of 6 would put lane 1's row 0 on lane 0's row 6
    ("cmux-span-equals-stride", CMUX, CMUX3, 64, 64, 2, 3, 6, "span row_stride"),
    ("chain-span-equals-stride", CHAIN, CHAIN_RAM21, 64, 64, 2, 1, 2, "span row_stride"),
    ("rot-span-equals-stride", ROT, ROT31, 64, 64, 2, 3, 2, "span row_stride"),
    ("tree-span-equals-stride", TREE, TREE41, 64, 64, 2, 4, 18, "span row_stride"),         # leaves 0 .. 18: the last leaf of job 1 counts
    ("tree-leaves-count", TREE, ([0], [4], [0], [0]), 64, 64, 2, 4, 15, "span row_stride"),   # out over leaf 0: span 15 comes from the leaves
    # the last lane one row / one slot past the store
    ("cmux-last-lane-row", CMUX, CMUX3, 64, 7 + 7 - 1, 2, 3, 7, "outside the TRLWE store"),
    ("chain-last-lane-row", CHAIN, CHAIN_RAM21, 64, 3 * 4 + 2, 5, 1, 3, "outside the TRLWE store"),
    ("rot-last-lane-row", ROT, ROT31, 64, 3 + 2, 2, 3, 3, "outside the TRLWE store"),
    ("tree-last-lane-row", TREE, TREE41, 64, 19 + 18, 2, 4, 19, "outside the TRLWE store"),
    ("cmux-last-lane-sel", CMUX, CMUX3, 3 + 2, 64, 2, 3, 7, "outside the selector store"),
    ("chain-last-lane-sel", CHAIN, CHAIN_RAM21, 4, 64, 5, 1, 3, "outside the selector store"),
    ("rot-last-lane-sel", ROT, ROT31, 5, 64, 2, 3, 3, "outside the selector store"),
    ("tree-last-lane-sel", TREE, TREE41, 4 + 3, 64, 2, 4, 19, "outside the selector store"),
    # the parent's checks still hold, on lane 0's list against the whole stores
    ("parent-bad-row", CMUX, _with(CMUX3, a4=[4, 3, 64]), 64, 64, 2, 3, 7, "TRLWE index outside the buffer"),
    ("parent-two-writers", CMUX, _with(CMUX3, a4=[4, 4, 5]), 64, 64, 2, 3, 7, "two jobs of one batch write"),
    ("parent-steps", ROT, _with(ROT31, a0=[3, 0]), 64, 64, 2, 3, 3, "steps outside"),
    ("parent-levels", TREE, _with(TREE41, a1=[5, 1]), 64, 64, 2, 4, 19, "levels outside"),
]
ACCEPTED = [
    ("lanes-one-ignores-strides", CMUX, CMUX3, 3, 7, 1, 0, 0),
    ("count-x-lanes-at-the-cap", CMUX, _wide(1 << 12), 1 << 13, 1 << 27, 1 << 12, 1, 1 << 13),
    ("cmux-span-one-less", CMUX, CMUX3, 64, 64, 2, 3, 7),
    ("chain-span-one-less", CHAIN, CHAIN_RAM21, 64, 64, 2, 1, 3),
    ("rot-span-one-less", ROT, ROT31, 64, 64, 2, 3, 3),
    ("tree-span-one-less", TREE, TREE41, 64, 64, 2, 4, 19),
    ("tree-leaves-count", TREE, ([0], [4], [0], [0]), 64, 64, 2, 4, 16),
    ("cmux-last-lane-fits", CMUX, CMUX3, 3 + 3, 7 + 7, 2, 3, 7),
    ("chain-last-lane-fits", CHAIN, CHAIN_RAM21, 5, 3 * 4 + 3, 5, 1, 3),
    ("rot-last-lane-fits", ROT, ROT31, 6, 3 + 3, 2, 3, 3),
    ("tree-last-lane-fits", TREE, TREE41, 4 + 4, 19 + 19, 2, 4, 19),
    ("interleaved-selectors", CHAIN, ([5, 5], [3, 3], [0, 1], [2, 2], [0, 1], [0, 1]), 5 + 3 + 1, 6, 2, 1, 3),   # sel_stride 1 < 3 steps
]
