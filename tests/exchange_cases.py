"""Chosen cases for the replica exchange (iyk_hip_arena_sync_slots / _multi in iyokan_amd/csrc/iyokan_hip.hip): schedules of writes,
exchanges and snapshots over R replica arenas, and the arenas they must leave.  Pure numpy, no GPU, no library: an arena is an array,
an exchange is `dst[slots] = src[slots]`, a snapshot copies a span of an arena into the history region of the same arena, and the
steps apply in program order — the order the events of the exchange have to enforce on the streams, since every arena is touched
by its own replica's stream alone.  tests/test_exchange_cases.py checks on the CPU that the schedules tell a wrong exchange from a
right one; tests/test_gpu_zz_exchange.py runs them.

A step is one of
  ("write", r, slots, g)                 upload_slots of generation g of replica r's own rows: arena r [slots] = rows(r, slots, g)
  ("exchange", src, dsts, slots)         sync_slots_to (one destination) / sync_slots_to_many
  ("snap", r, first, count, to)          arena_copy on r's stream: arena r [to : to + count] = arena r [first : first + count]
  ("gates", r, level)                    gate_batch on replica r (the chained case)
  ("busy", r)                            a round of gates on a scratch arena of replica r's stream: nothing in the model
  ("refused", src, dsts, slots)          an exchange the library must refuse: nothing in the model
  ("check",)                             the GPU test synchronises and compares the arenas here (the arenas past 4 GiB only)
"""
import numpy as np

M32 = np.uint64(0xFFFFFFFF)
HIST_GEN = 127            # what an unwritten history row holds: generation 127 of its own slot
GATE_KINDS = ("NAND", "XOR", "MUX")

# ---- mirrors of iyokan_hip.hip (tests/test_exchange_cases.py reads the originals out of the source text) -------------------------
STAGE_RING = 8
MAX_DST = 64
MAX_COUNT = 1 << 24


def stage_cap_after(nbytes):
    return (nbytes + nbytes // 2 + 4096 + 255) & ~255


def list_stage_bytes(count, n1):
    """What upload_slots and the exchange ask acquire_stage for: the index list padded to 16 bytes, then the rows."""
    return ((count * 4 + 15) & ~15) + count * n1 * 4


# ---- sentinel rows ---------------------------------------------------------------------------------------------------------------

def _bij32(x):
    """A bijection of the 32-bit words (the finaliser of MurmurHash3), on uint64 arrays holding values below 2^32."""
    x = x ^ (x >> np.uint64(16))
    x = (x * np.uint64(0x85EBCA6B)) & M32
    x = x ^ (x >> np.uint64(13))
    x = (x * np.uint64(0xC2B2AE35)) & M32
    return x ^ (x >> np.uint64(16))


def rows(r, slots, g, n1):
    """Generation g of the rows of `slots` on replica r: word w is bij(bij(r, g, slot) + w * odd).  (r, g, slot) pack into 32 bits
    without overlap and both maps are bijections, so two rows of different replica, slot or generation differ in EVERY word, and so
    does a row read or written at a word offset."""
    slots = np.asarray(slots, dtype=np.uint64).reshape(-1)
    assert 0 <= r < 8 and 0 <= g < 128 and (slots.size == 0 or int(slots.max()) < 1 << 22)
    base = _bij32((np.uint64(r) << np.uint64(29)) | (np.uint64(g) << np.uint64(22)) | slots)
    w = np.arange(n1, dtype=np.uint64) * np.uint64(0x9E3779B1)
    return _bij32((base[:, None] + w[None, :]) & M32).astype(np.uint32)


def pseudo_gates(level, arena):
    """The model's stand-in for a level of gates: every output word mixes the same word of the inputs and the gate kind.  (The GPU
    test runs the real gates and hands run() the oracle instead.)"""
    a, b = arena[level["in0"]].astype(np.uint64), arena[level["in1"]].astype(np.uint64)
    c = np.where((level["in2"] >= 0)[:, None], arena[np.maximum(level["in2"], 0)], 0).astype(np.uint64)
    k = level["kind"].astype(np.uint64)[:, None]
    arena[level["out"]] = _bij32((a * np.uint64(3) + b * np.uint64(5) + c * np.uint64(7) + k * np.uint64(11) + np.uint64(1)) & M32).astype(np.uint32)


# ---- schedules -------------------------------------------------------------------------------------------------------------------

def _i32(a):
    return np.asarray(a, dtype=np.int32).reshape(-1)


class _Builder:
    """Arena r: live slots [0, live), history [live, live + hist), then at least one more live slot (the arena's last)."""

    def __init__(self, name, R, live, n1, hist=None, sizes=None):
        self.name, self.R, self.live, self.n1, self.hist, self.sizes = name, R, live, n1, hist, sizes
        self.steps, self.gen, self.used = [], [0] * R, [0] * R

    def write(self, r, slots):
        self.gen[r] += 1
        self.steps.append(("write", r, _i32(slots), self.gen[r]))

    def exchange(self, src, dsts, slots, snap=True):
        self.steps.append(("exchange", src, tuple(dsts), _i32(slots)))
        for d in dsts if snap else ():
            self.snap(d, slots)

    def snap(self, r, slots):
        """One arena_copy per run of consecutive slots among `slots`."""
        s = np.unique(_i32(slots))
        for run in np.split(s, np.flatnonzero(np.diff(s) != 1) + 1) if s.size else ():
            self.steps.append(("snap", r, int(run[0]), len(run), self.live + self.used[r]))
            self.used[r] += len(run)

    def other(self, kind, *args):
        self.steps.append((kind,) + args)

    def done(self, **extra):
        hist = max(self.used) if self.hist is None else self.hist
        assert max(self.used) <= hist and max(self.gen) < HIST_GEN
        sizes = list(self.sizes) if self.sizes else [self.live + hist + 1] * self.R
        assert min(sizes) > self.live + hist
        return dict(name=self.name, R=self.R, live=self.live, hist=hist, sizes=sizes, n1=self.n1, steps=self.steps, tracked=None, **extra)


def _others(r, R):
    return [x for x in range(R) if x != r]


def wrap_case(n1, R=3, ring=STAGE_RING):
    """(a) The source's staging ring wraps behind a slow destination: replica R - 1 is busy first, then replica 0 writes a new
    generation of the same five slots and sends it on, 6 x ring times, to destinations 1 .. R - 1 in turn; every destination
    snapshots what it got.  Staging acquisitions: 12 x ring on the source (upload_slots and gather), 6 x ring / (R - 1) on each destination."""
    b = _Builder("wrap", R, 16, n1)
    slots = [5, 3, 7, 4, 6]
    b.other("busy", R - 1)
    for k in range(6 * ring):
        b.write(0, slots)
        b.exchange(0, (1 + k % (R - 1),), slots)
    return b.done(slow=R - 1)


def all_to_all_case(n1, R=3, rounds=20):
    """(b) Every round, every replica writes a new generation of its own four slots and fans it out to all the others, which snapshot
    it: per round a stream is source once and destination R - 1 times."""
    b = _Builder("all_to_all", R, 4 * R, n1)
    for _ in range(rounds):
        for r in range(R):
            own = np.arange(4 * r, 4 * r + 4)[[2, 0, 3, 1]]
            b.write(r, own)
            b.exchange(r, _others(r, R), own)
    return b.done(rounds=rounds)


def first_over(cap, n1):
    """Smallest list that no longer fits a staging slot of `cap` bytes."""
    c = max(1, cap // (n1 * 4 + 4) - 2)
    while list_stage_bytes(c, n1) <= cap:
        c += 1
    return c


def growth_sizes(n1, small=8, limit=8192):
    """(small, big1, big2): big1 outgrows the staging slot the small lists leave — 16 times the smallest list that does, so that the
    reallocation is no longer a matter of one page — and big2 the slot big1 leaves (8 times), both capped at `limit` rows."""
    big1 = min(limit, 16 * first_over(stage_cap_after(list_stage_bytes(small, n1)), n1))
    big2 = min(limit, 8 * first_over(stage_cap_after(list_stage_bytes(big1, n1)), n1))
    return small, big1, big2


def growth_case(n1, R=3, seed=41):
    """(c) Staging reallocated behind queued exchanges.  Small lists first, every stream source once.  Then list L1 from replica 0:
    0 fills it by uploads that still fit the small staging slot, so 0 grows AS SOURCE; replica 1 has just been the source of a small
    exchange to the busy replica 2 when it grows as destination; 2 grows as destination behind its busy round.  Then L2 from replica 2
    with the roles turned (0 has just sent to the busy 1).  Then 40 rows and more than a ring of small exchanges."""
    rng = np.random.default_rng(seed)
    small, big1, big2 = growth_sizes(n1)
    b = _Builder("growth", R, 40 + big2 + 8, n1)
    s8 = lambda r: 8 * r + rng.permutation(small)          # replicas 0, 1, 2 own slots 0 .. 23
    fit = lambda cap: first_over(cap, n1) - 1
    L1 = 40 + rng.permutation(big1)
    L2 = 40 + rng.permutation(big2)
    for r in range(3):
        b.write(r, s8(r))
        b.exchange(r, _others(r, R), s8(r))
    cap = stage_cap_after(list_stage_bytes(small, n1))
    for at in range(0, big1, fit(cap)):
        b.write(0, L1[at:at + fit(cap)])
    b.other("busy", 2)
    b.write(1, s8(1))
    b.exchange(1, (2,), s8(1))
    b.exchange(0, _others(0, R), L1)
    cap = stage_cap_after(list_stage_bytes(big1, n1))
    for at in range(0, big2, fit(cap)):
        b.write(2, L2[at:at + fit(cap)])
    b.other("busy", 1)
    b.write(0, s8(0))
    b.exchange(0, (1,), s8(0))
    b.exchange(2, _others(2, R), L2)
    L40 = 40 + rng.permutation(big2)[:40]
    b.write(1, L40)
    b.exchange(1, _others(1, R), L40)
    for k in range(STAGE_RING + 4):
        b.write(k % 3, s8(k % 3))
        b.exchange(k % 3, _others(k % 3, R), s8(k % 3))
    return b.done(sizes3=(small, big1, big2))


def stage_growth(case, busy_bytes=0):
    """[(step, stream, "write" / "source" / "destination" / "busy")] for every reallocation of a stream's staging ring under the
    mirrored policy; busy_bytes = what a busy round's gate_batch asks for."""
    cap = [0] * case["R"]
    out = []

    def need(k, r, nbytes, role):
        if nbytes > cap[r]:
            cap[r] = stage_cap_after(nbytes)
            out.append((k, r, role))

    for k, st in enumerate(case["steps"]):
        if st[0] == "write":
            need(k, st[1], list_stage_bytes(len(st[2]), case["n1"]), "write")
        elif st[0] == "exchange" and len(st[2]) and len(st[3]):
            need(k, st[1], list_stage_bytes(len(st[3]), case["n1"]), "source")
            for d in st[2]:
                need(k, d, list_stage_bytes(len(st[3]), case["n1"]), "destination")
        elif st[0] == "busy":
            need(k, st[1], busy_bytes, "busy")
    return out


def acquisitions(case):
    """Staging slots each stream takes over the schedule (upload_slots, gather and scatter sides of the exchanges)."""
    n = [0] * case["R"]
    for st in case["steps"]:
        if st[0] == "write":
            n[st[1]] += 1
        elif st[0] == "exchange" and len(st[2]) and len(st[3]):
            for r in (st[1],) + tuple(st[2]):
                n[r] += 1
    return n


def chain_case(n1, R=3, levels=6, width=48, nin=24, seed=43):
    """(d) Six dependent levels of 48 NAND / XOR / MUX gates dealt round-robin over the replicas; after every level each replica
    fans its outputs out to all the others.  in0 of every gate above the first level is an output of the level below that ANOTHER
    replica produced; the other inputs are any outputs of the level below."""
    rng = np.random.default_rng(seed)
    b = _Builder("chain", R, nin + levels * width, n1, hist=0)
    prev, prev_owner = np.arange(nin), None
    deals = []
    for k in range(levels):
        out = np.arange(nin + k * width, nin + (k + 1) * width)
        owner = (np.arange(width) + k) % R
        kind = rng.integers(0, len(GATE_KINDS), size=width)
        kind[:3] = [0, 1, 2]
        in0, in1, in2 = (prev[rng.integers(0, len(prev), size=width)] for _ in range(3))
        if prev_owner is not None:
            for g in range(width):
                foreign = prev[prev_owner != owner[g]]
                in0[g] = foreign[rng.integers(0, len(foreign))]
        in2 = np.where(kind == GATE_KINDS.index("MUX"), in2, -1)
        for r in range(R):
            m = owner == r
            b.other("gates", r, dict(kind=_i32(kind[m]), in0=_i32(in0[m]), in1=_i32(in1[m]), in2=_i32(in2[m]), out=_i32(out[m])))
        for r in range(R):
            b.exchange(r, _others(r, R), rng.permutation(out[owner == r]), snap=False)
        deals.append(dict(out=out, owner=owner, in0=in0))
        prev, prev_owner = out, owner
    return b.done(nin=nin, deals=deals)


def relay_case(n1):
    """(e) The same slots go 0 -> 1 and at once 1 -> 2; 0 overwrites them the moment its call returns and sends the new generation to
    2; then a third generation goes down the relay again.  1 ends with what 0 sent it, never with what 0 wrote afterwards."""
    b = _Builder("relay", 3, 16, n1)
    L = [9, 2, 11, 3, 10, 4]
    b.write(0, L)
    b.exchange(0, (1,), L, snap=False)
    b.exchange(1, (2,), L)                 # 2 snapshots generation 1
    b.write(0, L)
    b.exchange(0, (2,), L)                 # 2 snapshots generation 2; 1 still holds generation 1
    b.snap(1, L)
    b.write(0, L)
    b.exchange(0, (1,), L, snap=False)
    b.write(0, L)                          # generation 4 never leaves replica 0
    b.exchange(1, (2,), L)
    return b.done()


def shapes_case(n1):
    """(f) Eight replicas of different sizes: a fan-out to seven, a list of one slot, slot 0 with the last slot, repeated slots (every
    copy writes the same row), no destination, no slot, and lists that the smallest destination cannot hold — refused, after which
    the same streams exchange again."""
    live, hist = 16, 40
    T = live + hist + 1
    sizes = [T + 2, T, T + 1, T, T + 3, T, T + 4, T]      # T slots is the smallest; replica 6 has four more
    b = _Builder("shapes", 8, live, n1, hist=hist, sizes=sizes)
    L = [7, 1, 12, 3, 8]
    b.write(0, L)
    b.exchange(0, range(1, 8), L)
    b.write(3, [9])
    b.exchange(3, (4,), [9])
    b.write(1, [0, T - 1])
    b.exchange(1, (0, 2), [T - 1, 0])
    rep = [2, 5, 2, 7, 5, 9, 2, 13]
    b.write(2, np.unique(rep))
    b.exchange(2, (5, 6), rep)
    b.exchange(4, (), L)
    b.exchange(4, (5, 6), [])
    b.write(6, [1, T + 2, T])
    b.other("refused", 6, (5, 7), _i32([1, T + 2]))       # outside both destinations
    b.other("refused", 6, (7, 5), _i32([T, 1]))           # the first slot past the smallest arena
    b.other("refused", 5, (6, 7), _i32([1, T]))           # outside the source
    b.exchange(6, (5, 7), [T - 1, 1])
    b.write(5, [14, 1])
    b.exchange(5, (6, 7), [1, 14])
    return b.done()


def long_case(n1, count=65539):
    """(f) One list of 65 539 slots (more than 2^16 workgroups) between two replicas, slot 0 and a permuted range."""
    rng = np.random.default_rng(47)
    slots = np.concatenate([[0], 3 + rng.permutation(count - 1)])
    b = _Builder("long", 2, count + 5, n1, hist=0)
    b.write(0, slots)
    b.exchange(0, (1,), slots, snap=False)
    return b.done()


def refusal_rounds_case(n1, rounds):
    """(g) `rounds` times: a refused call (made by the GPU test through the C interface), then a valid fan-out on the same streams."""
    b = _Builder("refusals", 3, 12, n1)
    for k in range(rounds):
        b.other("refuse", k)
        r = k % 3
        L = np.arange(4 * r, 4 * r + 4)[[1, 3, 0, 2]]
        b.write(r, L)
        b.exchange(r, _others(r, 3), L)
    return b.done()


def big_arena_slots(n1):
    """Slots of an arena of just over 2^32 bytes."""
    return (1 << 32) // (n1 * 4) + 3


def big_case(n1):
    """(h) Two arenas past 4 GiB; only the tracked slots are modelled (and touched): the exchanged slots — the last slot that starts
    below byte 2^32, the first at or above it, slot 0, the last slot — and slots 1 .. 3, where a byte offset cut to 32 bits lands.
    "check" marks where the GPU test compares every tracked slot of both arenas."""
    slots = big_arena_slots(n1)
    after = -(-(1 << 32) // (n1 * 4))
    before, last = after - 1, slots - 1
    L = [after, 0, last, before]
    steps = [("write", 0, _i32(L), 1), ("check",), ("exchange", 0, (1,), _i32(L)), ("check",),
             ("write", 1, _i32(L[::-1]), 1), ("exchange", 1, (0,), _i32(L[::-1])), ("check",)]
    return dict(name="big", R=2, live=slots, hist=0, sizes=[slots, slots], n1=n1, steps=steps,
                tracked=np.array(sorted({0, 1, 2, 3, before, after, last}), dtype=np.int64), chosen=dict(before=before, after=after, last=last))


def byte_alias_slots(slot, n1):
    """The low slots a row of `slot` touches when its BYTE offset is cut to 32 bits (none when the offset fits)."""
    off = slot * n1 * 4
    if off < 1 << 32:
        return []
    w = (off % (1 << 32)) // 4
    return sorted({w // n1, (w + n1 - 1) // n1})


def small_cases(n1, big_n1=None):
    """Every schedule (the long list apart: long_case); the arenas past 4 GiB need rows of at least 256 words (22-bit slot numbers)."""
    return [wrap_case(n1), all_to_all_case(n1), growth_case(n1), chain_case(n1), relay_case(n1), shapes_case(n1),
            refusal_rounds_case(n1, 4), big_case(big_n1 or n1)]


# ---- the model -------------------------------------------------------------------------------------------------------------------

def _loc(case, slots):
    """Rows of the model arrays that hold `slots` (the identity unless the case models tracked slots only)."""
    slots = np.asarray(slots, dtype=np.int64)
    if case["tracked"] is None:
        return slots
    at = np.searchsorted(case["tracked"], slots)
    assert np.array_equal(case["tracked"][at], slots)
    return at


def initial(case):
    """The arenas before the first step: generation 0 of every live slot, HIST_GEN in the history region."""
    out = []
    for r, size in enumerate(case["sizes"]):
        slots = np.arange(size) if case["tracked"] is None else case["tracked"]
        a = rows(r, slots, 0, case["n1"])
        h = (slots >= case["live"]) & (slots < case["live"] + case["hist"])
        a[h] = rows(r, slots[h], HIST_GEN, case["n1"])
        out.append(a)
    return out


def _touches(step):
    """({replica: slots read}, {replica: slots written}) of a step."""
    k = step[0]
    if k == "write":
        return {}, {step[1]: step[2]}
    if k == "exchange":
        return {step[1]: step[3]}, {d: step[3] for d in step[2]}
    if k == "snap":
        return {step[1]: np.arange(step[2], step[2] + step[3])}, {step[1]: np.arange(step[4], step[4] + step[3])}
    if k == "gates":
        lv = step[2]
        ins = np.concatenate([lv["in0"], lv["in1"], lv["in2"]])
        return {step[1]: ins[ins >= 0]}, {step[1]: lv["out"]}
    return {}, {}


def _conflict(a, b):
    ra, wa = _touches(a)
    rb, wb = _touches(b)
    hit = lambda x, y: any(r in y and np.intersect1d(x[r], y[r]).size for r in x)
    return hit(wa, rb) or hit(wa, wb) or hit(ra, wb)


def mutants(case):
    """Every wrong exchange the model can play, as (kind, step, detail):
      drop     the exchange does nothing                       short    the last row of the list is left out
      late     it happens after the next step it does not commute with (a destination's snapshot, the source's next write, ...)
      stale    it delivers what the source's slots held before they were last written
      future   it delivers what the source's NEXT write puts there (the gather ran after the overwrite)
      shift    row j lands in slot slots[j] + 1               skipdst  one destination of a fan-out gets nothing"""
    steps = case["steps"]
    for k, st in enumerate(steps):
        if st[0] != "exchange" or not len(st[2]) or not len(st[3]):
            continue
        for kind in ("drop", "short", "stale", "shift"):
            yield kind, k, None
        j = next((j for j in range(k + 1, len(steps)) if _conflict(st, steps[j])), None)
        if j is not None:
            yield "late", k, j
        j = next((j for j in range(k + 1, len(steps)) if steps[j][0] == "write" and steps[j][1] == st[1]
                  and np.intersect1d(steps[j][2], st[3]).size), None)
        if j is not None:
            yield "future", k, j
        if len(st[2]) > 1:
            for d in st[2]:
                yield "skipdst", k, d


def run(case, mutant=None, gate_fn=pseudo_gates, arenas=None):
    """The arenas after the schedule, in program order, followed by their copies at every ("check",) step (R arrays each); `mutant`
    (one of mutants(case)) makes one exchange go wrong."""
    n1 = case["n1"]
    arenas = [a.copy() for a in (initial(case) if arenas is None else arenas)]
    before = [np.zeros_like(a) for a in arenas]           # what each row held before it was last written
    kind, at, detail = mutant or (None, None, None)
    steps = list(enumerate(case["steps"]))
    if kind == "late":
        steps = steps[:at] + steps[at + 1:detail + 1] + [steps[at]] + steps[detail + 1:]

    def put(r, where, new):
        # in list order, as the model of a scatter with repeated slots (every copy carries the same row)
        before[r][where] = arenas[r][where]
        arenas[r][where] = new

    checks = []
    for k, st in steps:
        if st[0] == "check":
            checks += [a.copy() for a in arenas]
        elif st[0] == "write":
            put(st[1], _loc(case, st[2]), rows(st[1], st[2], st[3], n1))
        elif st[0] == "snap":
            put(st[1], _loc(case, np.arange(st[4], st[4] + st[3])), arenas[st[1]][_loc(case, np.arange(st[2], st[2] + st[3]))])
        elif st[0] == "gates":
            lv = st[2]
            before[st[1]][lv["out"]] = arenas[st[1]][lv["out"]]
            gate_fn(lv, arenas[st[1]])
        elif st[0] == "exchange":
            src, dsts, slots = st[1], st[2], st[3].astype(np.int64)
            wrong = kind if k == at else None
            if wrong == "drop":
                continue
            data = (before if wrong == "stale" else arenas)[src][_loc(case, slots)].copy()
            if wrong == "future":
                nxt = case["steps"][detail]
                newer = dict(zip(nxt[2].tolist(), rows(src, nxt[2], nxt[3], n1)))
                for j, s in enumerate(slots.tolist()):
                    if s in newer:
                        data[j] = newer[s]
            to = slots
            if wrong == "short":
                to, data = to[:-1], data[:-1]
            if wrong == "shift":
                to = (to + 1) % min(case["sizes"][d] for d in dsts)
            for d in dsts:
                if wrong == "skipdst" and d == detail:
                    continue
                put(d, _loc(case, to), data)
    return arenas + checks


def differ(a, b):
    return any(not np.array_equal(x, y) for x, y in zip(a, b))
