"""The lane batches behind tests/test_lane_jobs.py (CPU: csrc/lane_jobs.hpp and batch_args.hpp's gate_batch_lanes_args through
libiyk_emul.so) and tests/test_gpu_lanes.py (iyk_hip_gate_batch_lanes on the GPU).

A case is the gate descriptors of ONE lane, a lane count and a lane stride.  Its reference is the FLAT batch: `lanes` copies of the
descriptor arrays, copy r with + r * stride on every non-negative index (replicate) — what a caller had to build on the host before
lane batches, what iyk_hip_gate_batch runs and what check_gate_batch builds job lists from.  Every comparison is word for word.

A lane's slots: [0, NIN) hold inputs, gate g writes NIN + g unless the case says otherwise; slots of the stride behind `used` belong to
no gate."""
import ctypes
import os

import numpy as np

from iyokan_amd.params import OPS, params_128bit

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OK, INVALID = 0, -1
MAX_GATE_BATCH = 1 << 30
NIN = 8          # input slots of a lane
ROT_WORDS, KS_WORDS, EW_WORDS = 5, 4, 3   # 32-bit words of a RotJob / KsJob / EwJob

_i32p, _u32p, u64 = ctypes.POINTER(ctypes.c_int32), ctypes.POINTER(ctypes.c_uint32), ctypes.c_uint64


def case(name, gates, lanes, stride=None, used=None):
    """gates: [(kind, in0, in1, in2, out)] of one lane"""
    cols = list(zip(*[(OPS[k], a, b, c, o) for k, a, b, c, o in gates]))
    desc = {k: np.array(c, dtype=np.int32) for k, c in zip(("ops", "in0", "in1", "in2", "out"), cols)}
    top = 1 + max(int(desc[k].max()) for k in ("in0", "in1", "in2", "out"))
    used = top if used is None else used
    stride = used if stride is None else stride
    assert top <= used <= stride
    return dict(name=name, lanes=lanes, stride=stride, used=used, count=len(gates), **desc)


def _random_gates(count, seed):
    """every kind, seeded: inputs among the NIN input slots, gate g writes NIN + g"""
    rng = np.random.default_rng(seed)
    kinds = list(OPS)
    gates = []
    for g in range(count):
        k = kinds[g % len(kinds)] if g < 2 * len(kinds) else kinds[int(rng.integers(len(kinds)))]
        a, b, c = (int(x) for x in rng.integers(0, NIN, size=3))
        nin = 3 if k == "MUX" else 2 if OPS[k] < OPS["MUX"] else 1 if k in ("NOT", "COPY") else 0
        gates.append((k, a if nin > 0 else -1, b if nin > 1 else -1, c if nin > 2 else -1, NIN + g))
    return gates


def wide(name, count, lanes, kind="NAND"):
    """`count` gates of one kind per lane on the NIN shared inputs (jobs may share what they only read): the dispatch threshold cases"""
    return case(name, [(kind, g % NIN, (g + 3) % NIN, -1, NIN + g) for g in range(count)], lanes)


EVERY_OP = [
    ("AND", 0, 1, -1, 8), ("NAND", 1, 2, -1, 9), ("ANDNOT", 2, 3, -1, 10), ("OR", 3, 4, -1, 11), ("NOR", 4, 5, -1, 12), ("ORNOT", 5, 6, -1, 13),
    ("XOR", 6, 7, -1, 14), ("XNOR", 7, 0, -1, 15), ("MUX", 0, 1, 2, 16), ("NOT", 3, -1, -1, 17), ("CONSTONE", -1, -1, -1, 18),
    ("CONSTZERO", -1, -1, -1, 19), ("COPY", 4, -1, -1, 20),
    ("NAND", 21, 5, -1, 21),      # writes over its own input (slot 21 holds an input, too)
    ("MUX", 6, 22, 7, 22),        # a MUX over its own c1
    ("NOT", 23, -1, -1, 23),      # an elementwise gate over its own input
]
OWN_INPUT_SLOTS = (21, 22, 23)    # slots of EVERY_OP that hold inputs besides [0, NIN)

CASES = {c["name"]: c for c in [
    case("one-gate-one-lane", [("NAND", 0, 1, -1, 8)], 1),
    case("one-gate-two-lanes", [("NAND", 0, 1, -1, 8)], 2),
    case("mux-3", [("MUX", 0, 1, 2, 8), ("XOR", 3, 4, -1, 9), ("NOT", 5, -1, -1, 10)], 2),
    case("mux-first-and-last", [("MUX", 0, 1, 2, 8), ("AND", 3, 4, -1, 9), ("MUX", 5, 6, 7, 10)], 5),
    case("every-op-1", EVERY_OP, 1),
    case("every-op-2", EVERY_OP, 2),
    case("every-op-5-wide-stride", EVERY_OP, 5, stride=31),          # 7 slots per lane that no gate names
    case("constants-only", [("CONSTONE", -1, -1, -1, 8), ("CONSTZERO", -1, -1, -1, 9)], 5, stride=13),
    case("37x7", _random_gates(37, seed=37), 7, stride=NIN + 37 + 2),   # 259 gates: one past a 256-thread block
]}
# what tests/test_gpu_lanes.py runs under real keys (the issue's smallest shapes first)
GPU_CASES = ["one-gate-one-lane", "one-gate-two-lanes", "mux-3", "every-op-5-wide-stride", "37x7"]


def input_slots(c):
    """the slots of one lane that hold inputs"""
    return list(range(NIN)) + [s for s in OWN_INPUT_SLOTS if s < c["used"] and c["name"].startswith("every-op")]


def replicate(c, lanes=None, stride=None):
    """the flat batch: (ops, in0, in1, in2, out) of `lanes` copies, copy r shifted by r * stride, negative indexes kept"""
    lanes = c["lanes"] if lanes is None else lanes
    stride = c["stride"] if stride is None else stride
    shift = lambda a: np.concatenate([np.where(a >= 0, a + r * stride, a) for r in range(lanes)]).astype(np.int32)
    return (np.tile(c["ops"], lanes),) + tuple(shift(c[k]) for k in ("in0", "in1", "in2", "out"))


# ---- libiyk_emul.so ---------------------------------------------------------------------------------------------------------------

_EMUL = None


def emul(path=None):
    global _EMUL
    if path is not None:
        return ctypes.CDLL(path)
    if _EMUL is None:
        _EMUL = ctypes.CDLL(os.path.join(ROOT, "iyokan_amd", "lib", "libiyk_emul.so"))
    return _EMUL


def _p(a):
    return a.ctypes.data_as(_i32p)


def _split(words, counts):
    """flat words -> [rot, ks, ew] arrays of shape [jobs, words per job]"""
    out, at = [], 0
    for n, w in zip(counts, (ROT_WORDS, KS_WORDS, EW_WORDS)):
        out.append(words[at: at + n * w].reshape(n, w).copy())
        at += n * w
    return out


def lane_args(desc, arena_slots, lanes, stride, debug=0, lib=None):
    """iyk_emul_gate_batch_lanes_args -> (code, text, [rot, ks, ew] of ONE lane, a list left non-empty by a refusal)"""
    L = lib or emul()
    ops, in0, in1, in2, out = (np.ascontiguousarray(a, dtype=np.int32) for a in desc)
    msg = ctypes.create_string_buffer(256)
    cap = max(1, 2 * ROT_WORDS * len(ops) + KS_WORDS * len(ops))
    words = np.zeros(cap, dtype=np.uint32)
    counts = (u64 * 4)()
    p = params_128bit()
    L.iyk_emul_gate_batch_lanes_args.restype = ctypes.c_int
    code = L.iyk_emul_gate_batch_lanes_args(ctypes.byref(p), debug, u64(arena_slots), u64(len(ops)), _p(ops), _p(in0), _p(in1), _p(in2), _p(out),
                                            u64(lanes), u64(stride), msg, u64(256), words.ctypes.data_as(_u32p), u64(cap), counts)
    n = [int(counts[i]) for i in range(3)]
    return code, msg.value.decode(), _split(words, n), bool(counts[3])


def flat_lists(desc, arena_slots, debug=0):
    """iyk_emul_check_gate_batch (what iyk_hip_gate_batch stages) -> (code, text, [rot, ks, ew])"""
    L = emul()
    ops, in0, in1, in2, out = (np.ascontiguousarray(a, dtype=np.int32) for a in desc)
    msg = ctypes.create_string_buffer(256)
    cap = max(1, 2 * ROT_WORDS * len(ops) + KS_WORDS * len(ops))
    words = np.zeros(cap, dtype=np.uint32)
    counts = (u64 * 4)()
    p = params_128bit()
    L.iyk_emul_check_gate_batch.restype = ctypes.c_int
    code = L.iyk_emul_check_gate_batch(ctypes.byref(p), debug, u64(arena_slots), u64(len(ops)), _p(ops), _p(in0), _p(in1), _p(in2), _p(out), msg, u64(256),
                                       words.ctypes.data_as(_u32p), u64(cap), counts)
    return code, msg.value.decode(), _split(words, [int(counts[i]) for i in range(3)])


def expand(lists1, lanes, stride, threads=0, lib=None):
    """iyk_emul_lane_jobs: the lists of all lanes from those of one; threads > 0: lane_jobs_kernel's traversal with that many threads"""
    L = lib or emul()
    counts1 = (u64 * 3)(*[len(a) for a in lists1])
    words1 = np.ascontiguousarray(np.concatenate([a.reshape(-1) for a in lists1] + [np.zeros(1, dtype=np.uint32)]), dtype=np.uint32)
    n = [len(a) * lanes for a in lists1]
    out = np.zeros(max(1, n[0] * ROT_WORDS + n[1] * KS_WORDS + n[2] * EW_WORDS), dtype=np.uint32)
    assert L.iyk_emul_lane_jobs(words1.ctypes.data_as(_u32p), counts1, u64(lanes), u64(stride), u64(threads), out.ctypes.data_as(_u32p)) == 0
    return _split(out, n)


def lane_lists(c, lib=None, threads=0):
    """a case through the mirror and the emulated expansion: [rot, ks, ew] of all lanes"""
    code, text, lists1, _ = lane_args(tuple(c[k] for k in ("ops", "in0", "in1", "in2", "out")), c["lanes"] * c["stride"], c["lanes"], c["stride"], lib=lib)
    assert code == OK, text
    return expand(lists1, c["lanes"], c["stride"], threads=threads, lib=lib)


def first_difference(c, lib=None):
    """None where the expansion of the case equals the lists of the replicated descriptors, else (list, job)"""
    got = lane_lists(c, lib=lib)
    code, text, want = flat_lists(replicate(c), c["lanes"] * c["stride"])
    assert code == OK, text
    for name, g, w in zip(("rot", "ks", "ew"), got, want):
        if g.shape != w.shape:
            return name, -1
        bad = np.nonzero((g != w).any(axis=1))[0]
        if len(bad):
            return name, int(bad[0])
    return None


# ---- refusals: (name, descriptors of one lane, arena_slots, lanes, stride, a word of the text) -------------------------------------
_G = tuple(CASES["mux-3"][k] for k in ("ops", "in0", "in1", "in2", "out"))       # used: 11 slots


def _with(desc, **kw):
    d = dict(zip(("ops", "in0", "in1", "in2", "out"), (a.copy() for a in desc)))
    for k, (g, v) in kw.items():
        d[k][g] = v
    return tuple(d[k] for k in ("ops", "in0", "in1", "in2", "out"))


_STRIDE1 = tuple(np.array(v, dtype=np.int32) for v in ([OPS["NAND"]] * 3, [0] * 3, [0] * 3, [-1] * 3, [0] * 3))   # every index 0: stride 1
REFUSALS = [
    ("lanes-0", _G, 64, 0, 11, "lanes is zero"),
    ("stride-0", _G, 64, 2, 0, "lane stride is zero"),
    ("out-equal-to-stride", _with(_G, out=(2, 11)), 64, 2, 11, "output slot outside the arena"),
    ("in-equal-to-stride", _with(_G, in1=(0, 11)), 64, 2, 11, "MUX needs three input slots inside the arena"),
    ("in-of-another-lane", _with(_G, in0=(1, 12)), 64, 2, 11, "binary gate needs two input slots inside the arena"),
    ("one-slot-short", _G, 2 * 11 - 1, 2, 11, "do not fit the arena"),              # lanes * stride = arena_slots + 1
    ("lanes-2^40", _G, 64, 1 << 40, 11, "do not fit the arena"),
    ("lanes-2^40-product-wraps", _G, 1 << 20, 1 << 40, 1 << 24, "do not fit the arena"),   # lanes * stride = 2^64 = 0 in 64 bits
    ("beyond-int32-slots", _G, 1 << 33, (1 << 31) // 11 + 1, 11, "2^31 slots"),
    ("count-x-lanes", _STRIDE1, 1 << 29, 1 << 29, 1, "count x lanes"),              # 3 * 2^29 > MAX_GATE_BATCH
    ("unknown-op", _with(_G, ops=(1, 13)), 64, 2, 11, "unknown gate op"),
]
# accepted, next to the refusals above
ACCEPTED = [
    ("exact-fit", _G, 2 * 11, 2, 11),
    ("arena-larger", _G, 2 * 11 + 5, 2, 11),
    ("index-stride-minus-1", _with(_G, out=(2, 10)), 64, 2, 11),
    ("count-x-lanes-at-the-cap", tuple(a[:1] for a in _STRIDE1), 1 << 30, 1 << 30, 1),
]
