"""Chosen cases for the host runtime around the gate kernels (iyokan_amd/csrc/iyokan_hip.hip): arenas past every 32-bit limit of
`arena + (size_t)slot * (n + 1)`, per-stream buffers that grow behind queued work, and batches issued by several host threads.
Plain arrays and integers only, no GPU: tests/test_arena_cases.py checks them on the CPU, tests/test_gpu_gate_edges.py runs them."""
import numpy as np

from iyokan_amd.params import OPS, OP_NAMES, PLAIN

BINARY = ("AND", "NAND", "ANDNOT", "OR", "NOR", "ORNOT", "XOR", "XNOR")

# ---- arenas beyond 16 GiB -------------------------------------------------------------------------------------------------------

# a row's offset cut to: 32 bits of BYTES (word address mod 2^30), a 31-bit WORD index, a 32-bit WORD index
TRUNCATIONS = {"bytes mod 2^32": 1 << 30, "words mod 2^31": 1 << 31, "words mod 2^32": 1 << 32}


def arena_slots(n1):
    """Slots of the arena whose last rows lie past word index 2^32 (17.18 GB at n + 1 = 637 and at 501)."""
    return (1 << 32) // n1 + 3


def boundary_pairs(n1):
    """(limit in words, last slot that starts below it, first slot that starts at or above it) for the three limits."""
    out = []
    for words in (1 << 30, 1 << 31, 1 << 32):          # 2^32 bytes, 2^31 words, 2^32 words
        after = -(-words // n1)
        out.append((words, after - 1, after))
    return out


def boundary_slots(n1):
    """The chosen high slots, ascending: both sides of each limit and the arena's last three slots."""
    s = set()
    for _, before, after in boundary_pairs(n1):
        s.update((before, after))
    top = arena_slots(n1)
    s.update((top - 3, top - 2, top - 1))
    return sorted(s)


def truncated_word(slot, n1, modulus):
    return (slot * n1) % modulus


def aliases(slot, n1):
    """{truncation name: (low slot holding the truncated address, the slot after it)} for every truncation that moves the row of
    `slot`: where a kernel that dropped a cast would read or write instead.  A truncated row starts inside the first of the two slots
    and generally ends in the second."""
    out = {}
    for name, modulus in TRUNCATIONS.items():
        w = truncated_word(slot, n1, modulus)
        if w != slot * n1:
            out[name] = (w // n1, w // n1 + 1)
    return out


def sentinel_slots(n1):
    """Every low slot a truncated access to a chosen high slot touches that is not itself a chosen slot, ascending.  The three limits
    are powers of two, so the slot just below a limit aliases the slot just below a lower limit: those aliases are chosen slots, and
    hold data the GPU test compares after every stage; all the others (slots 0, 1, 2 and at most one more) hold sentinels."""
    chosen = set(boundary_slots(n1))
    s = set()
    for h in chosen:
        for pair in aliases(h, n1).values():
            s.update(pair)
    return sorted(s - chosen)


def sentinel_row(slot, n1):
    """What a sentinel slot holds: word j is 0xA5 in the top byte and (1021 slot + j) mod 2^24 below — it names the slot and its own
    position, and no stage of the test produces such a row (ciphertext words are uniform, trivial rows are zero but for the last
    word)."""
    j = np.arange(n1, dtype=np.uint64)
    return (np.uint64(0xA5000000) | ((np.uint64(slot) * np.uint64(1021) + j) & np.uint64(0xFFFFFF))).astype(np.uint32)


def sentinel_words(row):
    """Words of `row` that continue a sentinel row: top byte 0xA5 and the successor of the word before them.  Two uniform words do that
    with probability 2^-40; a row read through a truncated offset that lands in a sentinel slot does it almost everywhere."""
    row = np.asarray(row, dtype=np.uint32)
    return int(np.sum((row[1:] >> 24 == 0xA5) & (row[:-1] >> 24 == 0xA5) & (row[1:] == row[:-1] + np.uint32(1))))


def low_range(n1, count, start):
    """First `count` consecutive slots at or above `start` that hold neither a sentinel nor a chosen slot (data the test keeps in low
    slots)."""
    sent = sorted(set(sentinel_slots(n1)) | set(boundary_slots(n1)))
    while True:
        hit = [s for s in sent if start <= s < start + count]
        if not hit:
            return start
        start = hit[-1] + 1


# ---- gate levels as arrays ------------------------------------------------------------------------------------------------------

def gate_level(rng, count, sources, out_first, kinds=BINARY + ("MUX",), extra=()):
    """`count` gates of random `kinds` reading random slots of `sources`, then one gate per kind in `extra` (NOT / COPY / CONST*), writing
    consecutive fresh slots from out_first: independent by construction when no source is at or above out_first."""
    sources = np.asarray(sources, dtype=np.int32)
    names = list(rng.choice(list(kinds), size=count)) + list(extra)
    n = len(names)
    ops = np.array([OPS[k] for k in names], dtype=np.int32)
    in0, in1, in2 = (sources[rng.integers(0, len(sources), size=n)].astype(np.int32) for _ in range(3))
    in1 = np.where(ops <= OPS["MUX"], in1, -1).astype(np.int32)
    in2 = np.where(ops == OPS["MUX"], in2, -1).astype(np.int32)
    in0 = np.where((ops == OPS["CONSTONE"]) | (ops == OPS["CONSTZERO"]), -1, in0).astype(np.int32)
    return {"ops": ops, "in0": in0, "in1": in1, "in2": in2, "out": np.arange(out_first, out_first + n, dtype=np.int32)}


def level_args(lv):
    return lv["ops"], lv["in0"], lv["in1"], lv["in2"], lv["out"]


def rotations(lv):
    """Blind rotations of a level: 2 per MUX, 1 per binary gate."""
    return int(np.sum(lv["ops"] < OPS["MUX"]) + 2 * np.sum(lv["ops"] == OPS["MUX"]))


def inputs_of(lv):
    """(gate, slot) for every slot a gate of the level reads."""
    ops = lv["ops"]
    nin = np.where(ops < OPS["MUX"], 2, np.where(ops == OPS["MUX"], 3, np.where((ops == OPS["NOT"]) | (ops == OPS["COPY"]), 1, 0)))
    return [(g, int(a[g])) for k, a in enumerate((lv["in0"], lv["in1"], lv["in2"])) for g in range(len(ops)) if k < nin[g]]


def independent(lv):
    """The contract of include/iyokan_hip.h: outputs pairwise distinct, no gate reads a slot ANOTHER gate of the batch writes."""
    writer = {}
    for g, o in enumerate(lv["out"]):
        if int(o) in writer:
            return False
        writer[int(o)] = g
    return all(writer.get(s, g) == g for g, s in inputs_of(lv))


def simulate_level(lv, bits):
    """Plaintext semantics of a level on `bits` (one per slot, -1 = never written), in place; reads of unwritten slots are an error."""
    new = {}
    for g, op in enumerate(lv["ops"]):
        name = OP_NAMES[int(op)]
        args = [int(bits[lv[k][g]]) for k in ("in0", "in1", "in2") if lv[k][g] >= 0]
        assert all(a in (0, 1) for a in args), (g, name)
        new[int(lv["out"][g])] = PLAIN[name](*args)
    for o, v in new.items():
        bits[o] = v
    return bits


# ---- buffers that grow behind queued batches ------------------------------------------------------------------------------------
# Mirrors of the growth policy of iyokan_hip.hip (ensure_stage, ensure_rot) and of what each call asks them for: the CPU test
# derives from them at which steps of growth_program a buffer is reallocated.  A change of the policy fails that test and shows
# which sizes to move.
STAGE_RING = 8
ROT_JOB_BYTES, KS_JOB_BYTES, EW_JOB_BYTES = 20, 16, 12


def stage_cap_after(nbytes):
    return (nbytes + nbytes // 2 + 4096 + 255) & ~255


def rot_cap_after(jobs):
    return jobs + jobs // 2 + 64


def gate_batch_stage_bytes(lv):
    al = lambda v: (v + 15) & ~15
    nks = int(np.sum(lv["ops"] <= OPS["MUX"]))
    return al(al(rotations(lv) * ROT_JOB_BYTES) + nks * KS_JOB_BYTES) + (len(lv["ops"]) - nks) * EW_JOB_BYTES


def slot_list_stage_bytes(count, n1):
    return ((count * 4 + 15) & ~15) + count * n1 * 4


GROWTH_INPUTS = 16
# 2 binary gates: 2 x 20 + 2 x 16 = 72 bytes -> staging slot (72 + 36 + 4096 + 255) & ~255 = 4352 bytes; 2 jobs -> 2 + 1 + 64 = 67 rows.
# 200 gates, 196 of them with rotations: at least 196 x 36 = 7056 bytes > 4352 and 196 jobs > 67: both grow, staging to at most
#   (196 x 56 + 48) x 1.5 + 4351 < 21 000 bytes, the rotation buffer to 196 + 98 + 64 = 358 .. 392 + 196 + 64 = 652 rows (MUX = 2 jobs).
# 300 uploaded rows: 1200 + 300 x 4 (n + 1) >= 602 400 bytes > 21 000: staging grows again.
# 700 gates, 698 of them with rotations: >= 698 jobs > 652: the rotation buffer grows again; <= 698 x 56 + 24 bytes, far below the
#   staging slot the 300 rows left, so staging stays.
GROWTH_SIZES = (2, 200, 1, 300, 700)
GROWTH_TAIL = (1, 3, 2, 1, 2, 3, 1, 1, 2, 3)      # ten more calls: the ring of eight slots wraps after the last growth


def growth_program(rng):
    """The job list of test_buffers_grow_behind_queued_batches: {"bits": bits of the input slots 0 .. 15, "steps": [...], "final": slots
    of the last download_slots, "slots": arena size}.  A step is ("gates", level) or ("upload_slots", slots, bits of the uploaded
    rows).  Every level reads outputs of the step before it (the first reads the inputs), the 700-gate level also the uploaded rows."""
    nxt = GROWTH_INPUTS
    steps = []
    prev = np.arange(GROWTH_INPUTS)

    def level(count, sources, **kw):
        nonlocal nxt, prev
        lv = gate_level(rng, count, sources, nxt, **kw)
        nxt += len(lv["ops"])
        prev = lv["out"]
        steps.append(("gates", lv))

    level(GROWTH_SIZES[0], prev, kinds=BINARY)
    level(GROWTH_SIZES[1] - 4, np.concatenate([prev, np.arange(GROWTH_INPUTS)]), extra=("NOT", "COPY", "CONSTONE", "CONSTZERO"))
    level(GROWTH_SIZES[2], prev, kinds=BINARY)
    up = np.arange(nxt, nxt + GROWTH_SIZES[3], dtype=np.int32)
    nxt += len(up)
    up = rng.permutation(up).astype(np.int32)
    steps.append(("upload_slots", up, rng.integers(0, 2, size=len(up)).astype(np.uint8)))
    level(GROWTH_SIZES[4] - 2, np.concatenate([prev, steps[1][1]["out"], up]), extra=("NOT", "COPY"))
    for count in GROWTH_TAIL:
        level(count, prev[-8:])
    return {"bits": rng.integers(0, 2, size=GROWTH_INPUTS).astype(np.uint8), "steps": steps, "slots": nxt,
            "final": rng.permutation(np.concatenate([prev, steps[-4][1]["out"], up[:5]])).astype(np.int32)}


def simulate_growth(prog):
    bits = np.full(prog["slots"], -1, dtype=np.int8)
    bits[:GROWTH_INPUTS] = prog["bits"]
    for step in prog["steps"]:
        if step[0] == "gates":
            simulate_level(step[1], bits)
        else:
            assert np.all(bits[step[1]] == -1)
            bits[step[1]] = step[2]
    return bits


def growth_points(prog, n1):
    """(steps at which the staging ring is reallocated, steps at which d_rot / d_abar are) under the mirrored policy."""
    stage_cap = rot_cap = 0
    stage_at, rot_at = [], []
    for k, step in enumerate(prog["steps"]):
        if step[0] == "gates":
            need, jobs = gate_batch_stage_bytes(step[1]), rotations(step[1])
        else:
            need, jobs = slot_list_stage_bytes(len(step[1]), n1), 0
        if need > stage_cap:
            stage_cap = stage_cap_after(need)
            stage_at.append(k)
        if jobs > rot_cap:
            rot_cap = rot_cap_after(jobs)
            rot_at.append(k)
    return stage_at, rot_at


# ---- batches from several host threads ------------------------------------------------------------------------------------------
THREAD_INPUTS = 64
FRESH_GATES = 64          # leading gates of a wide level that read the common inputs only: the oracle needs no earlier level for them
KS_TABLE_MIN = 4097       # smallest batch the key-switch table kernel takes (dispatch.hpp: KS_LUT_MIN_JOBS + 1)
KS_MATRIX_GROUP = 256     # key switches per workgroup of the matrix form (dispatch.hpp: KS_MATRIX_GATES)
KS_MATRIX_EDGE = 2 * KS_MATRIX_GROUP + 1   # two whole workgroups and a third that holds one job
# key-switch jobs of the core gates that write high slots, per batch of the huge-arena test: between them job 0, both sides of the
# boundary between two workgroups, and the last job
KS_MATRIX_AT = {"X": (0, KS_MATRIX_GROUP - 1, KS_MATRIX_GROUP), "Y": (KS_MATRIX_GROUP - 1, KS_MATRIX_GROUP, KS_MATRIX_EDGE - 1)}


def thread_programs(rng, threads, rotation_round=2048):
    """{"bits": bits of the common read-only inputs (slots 0 .. 63), "slots": arena size, "programs": one per thread}.  A program is
    {"range": (first, end) of the slots it writes, "levels": [3, rotation_round + 150, 1, 4097, 17 gates], "rotate": (ia, ib, sa, sb,
    off) of its blind_rotate_batch, "field": the 70-gate level of the second phase}.  The two wide levels hold binary gates only (so
    many rotations exactly: full rounds on one rotation kernel, 150 on the other from job `rotation_round` on; 4 097 key switches) plus
    NOT / COPY gates; their first FRESH_GATES gates read the common inputs only."""
    common = np.arange(THREAD_INPUTS)
    nxt = THREAD_INPUTS
    programs = []
    for _ in range(threads):
        first = nxt
        levels = []

        def level(count, sources, **kw):
            nonlocal nxt
            lv = gate_level(rng, count, sources, nxt, **kw)
            nxt += len(lv["ops"])
            levels.append(lv)
            return lv

        def wide(count, sources, extra):
            nonlocal nxt
            a = gate_level(rng, FRESH_GATES, common, nxt, kinds=BINARY)
            b = gate_level(rng, count - FRESH_GATES, sources, nxt + FRESH_GATES, kinds=BINARY, extra=extra)
            lv = {k: np.concatenate([a[k], b[k]]) for k in a}
            nxt += len(lv["ops"])
            levels.append(lv)
            return lv

        l0 = level(3, common)
        l1 = wide(rotation_round + 150, np.concatenate([common, l0["out"]]), ("NOT", "COPY", "NOT"))
        l2 = level(1, l1["out"][-40:], kinds=BINARY)
        l3 = wide(KS_TABLE_MIN, np.concatenate([l1["out"], l2["out"]]), ("COPY", "NOT"))
        l4 = level(17, l3["out"])
        src = l4["out"]
        rotate = (src[:8].astype(np.int32), np.concatenate([src[8:12], [-1] * 4]).astype(np.int32),
                  np.array([-1, 1, 2, 1, 1, 1, 1, 1], dtype=np.int32), np.array([-1, 1, 2, -1, 0, 0, 0, 0], dtype=np.int32),
                  np.array([1 << 29, 1 << 29, 1 << 30, (1 << 32) - (1 << 29), 0, 0, 0, 0], dtype=np.uint32))
        field = gate_level(rng, 70, np.concatenate([l4["out"], common]), nxt)
        nxt += 70
        programs.append({"range": (first, nxt), "levels": levels, "rotate": rotate, "field": field})
    return {"bits": rng.integers(0, 2, size=THREAD_INPUTS).astype(np.uint8), "slots": nxt, "programs": programs}


def simulate_threads(progs):
    bits = np.full(progs["slots"], -1, dtype=np.int8)
    bits[:THREAD_INPUTS] = progs["bits"]
    for pr in progs["programs"]:
        for lv in pr["levels"] + [pr["field"]]:
            simulate_level(lv, bits)
    return bits
