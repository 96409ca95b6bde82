"""Level-synchronous, frontier-sharded evaluation of a netlist over one or more GPUs.

MI355X-first replacement for the reference's scheduling layer around the hot path
(ReadyQueue + 800 one-gate workers + host bounce per gate: /root/reference/src/iyokan.hpp:775-883,
/root/reference/src/iyokan_cufhe.hpp:666-753; multi-GPU there = keys replicated, streams
round-robined over GPUs, every ciphertext through host memory — SURVEY.md §2.4):

  * the per-clock DAG is levelised once (netlist.levelise);
  * every rank holds the SAME device-resident ciphertext arena (slot per node);
  * level by level, the bootstrapped gates of the level are dealt round-robin to the ranks
    (MUX first, so 2-rotation gates spread evenly), each rank evaluates its share with ONE
    iyk_hip_gate_batch, and one all_gather (RCCL over xGMI) of that level's freshly written
    slots makes every arena identical again — the only data-path collective, at level
    boundaries (BASELINE.json north_star);
  * NOT / CONST are not bootstrapped: every rank computes them locally, no exchange;
  * the clock edge (DFF / RAM cell latch) is a local two-phase copy on every rank.

The arithmetic is behind `backend.gate_batch`; `HipBackend` is the product path, and
`PlainBitBackend` (bits instead of ciphertexts, CPU tensors) exists so the sharding /
collective / clocking logic is covered by gloo world_size-2 tests without a GPU.
"""
import numpy as np

from .netlist import BINARY
from .params import OPS


def make_level_cost(table=None):
    """Milliseconds one rank spends on a level of r blind rotations, as the library's dispatch prices it (include/
    iyokan_level_cost.h: iyk_level_cost_ms, restated here for the planner's inner loop; tests/test_netlist.py holds the two equal): full
    rounds on the wave-per-rotation kernel, a remainder of up to max_passes passes of the workgroup-per-rotation kernel (one
    rotation per CU and pass), a larger remainder as one more full round.  The FIGURES are the library's (include/
    iyokan_hip.h: iyk_level_cost; this module holds none): `table` = hip.level_cost_table(gpu) / hip.calibrate(gpu) on a
    GPU, default hip.level_cost_defaults() — the compiled-in MI355X table of the loaded build, readable without a GPU.
    Only the SHAPE matters to the planner (where the steps are), not the milliseconds."""
    if table is None:
        from . import hip

        table = hip.level_cost_defaults()
    rnd, pas, maxp = int(table["round"]), int(table["pass"]), int(table["max_passes"])
    round_ms, pass_ms = float(table["round_ms"]), [float(v) for v in table["pass_ms"]]

    def cost(rotations):
        if rotations <= 0:
            return 0.0
        full, rem = divmod(rotations, rnd)
        t = round_ms * full
        if rem == 0:
            return t
        if rem <= maxp * pas:
            return t + pass_ms[-(-rem // pas) - 1]
        return t + round_ms

    cost.quanta = (rnd, pas)
    cost.table = table
    return cost


class _DefaultCost:
    """make_level_cost() of the library's compiled-in table, resolved at first use (importing this module must not need
    the shared library)."""

    def __init__(self):
        self._f = None

    def _get(self):
        if self._f is None:
            self._f = make_level_cost()
        return self._f

    def __call__(self, rotations):
        return self._get()(rotations)

    @property
    def quanta(self):
        return self._get().quanta

    @property
    def table(self):
        return self._get().table


mi355x_level_cost = _DefaultCost()


def level_rotations(nl, levels, world=1):
    """Rotations per rank and level (binary gate 1, MUX 2; dealt round-robin, MUX first: FrontierPlan)."""
    return [-(-sum(2 if nl.kinds[i] == "MUX" else 1 if nl.kinds[i] in BINARY else 0 for i in lv) // world) for lv in levels]


# What ONE pass of the narrow-frontier kernel costs by how much of it is filled, relative to a full pass: up to a quarter of the
# CUs busy the kernel runs at the part's full clock, with all of them busy it runs into the power limit (profiles/r06_level_gaps.txt:
# 2.466 / 2.497 / 2.554 / 2.635 ms at 64 / 128 / 192 / 256 rotations, steady state; right after narrow levels a full pass starts at
# 3.1 ms).  Every level of a depth-bound netlist costs a pass whatever it holds, so rotations moved out of full passes into the
# half-empty ones behind them are free — if the plan knows that a full pass is the dear one.
SUB_PASS_SHAPE = (0.936, 0.947, 0.969, 1.0)


def with_sub_pass_shape(cost):
    """`cost` with the first pass priced by quarter: the figure plan_levels compares candidate plans by (the table's own
    pass_ms[0] stays what a FULL pass costs; beam_levels / balanced_levels and the C++ planner keep cutting by the plain table)."""
    _, small = getattr(cost, "quanta", (2048, 256))

    def refined(rotations):
        if 0 < rotations <= small:
            return cost(small) * SUB_PASS_SHAPE[min(3, (4 * rotations - 1) // small)]
        return cost(rotations)

    refined.quanta = getattr(cost, "quanta", (2048, 256))
    return refined


def capped_levels(nl, world=1, cap=128):
    """List scheduling with a CAP: level k takes the gates that must run now (ALAP level k) and, by ALAP order, as many of the
    other ready gates as keep it at `cap` rotations per rank.  Same number of levels as levelise(); a netlist whose depth, not its
    width, sets the clock ends up with its rotations spread over all its levels instead of piled into full passes at the front."""
    depth, order, succ, npred0, alap, rot = _slack_graph(nl)
    npred = list(npred0)
    ready = [i for i in order if npred[i] == 0]
    out = []
    for k in range(1, depth + 1):
        this, nxt, boots = [], [], []
        for i in ready:
            if rot[i] == 0:
                this.append(i)
                for s2 in succ[i]:
                    npred[s2] -= 1
                    if npred[s2] == 0:
                        nxt.append(s2)
            else:
                boots.append(i)
        boots.sort(key=lambda i: (alap[i], i))
        acc = 0
        for i in boots:
            if alap[i] <= k or k == depth or acc + rot[i] <= cap * world:
                this.append(i)
                acc += rot[i]
                for s2 in succ[i]:
                    npred[s2] -= 1
                    if npred[s2] == 0:
                        nxt.append(s2)
            else:
                nxt.append(i)
        out.append(this)
        ready = nxt
    assert not ready and sum(len(lv) for lv in out) == len(order)
    return out


def plan_levels(nl, world=1, cost=mi355x_level_cost, spread=True):
    """The cheapest of levelise(), balanced_levels() at three cut granularities, beam_levels() with both of its tie-breaks and —
    round 6 — capped_levels() at eighths of a pass up to a whole one, compared by with_sub_pass_shape(cost).  The greedy is not
    monotone (a deferral can push a later level over a step), so the plain ASAP levels stay a candidate."""
    best, best_t = None, None
    big, small = getattr(cost, "quanta", (2048, 256))
    price = with_sub_pass_shape(cost)
    caps = sorted({max(1, small * e // 8) for e in range(2, 9)}) if spread else []   # spread=False: round 5's candidates only (A/B)
    for quanta in [None, (big, small), (small,), (big,), "id", "fanout"] + [("cap", c) for c in caps]:
        if quanta is None:
            lv = nl.levelise()
        elif isinstance(quanta, str):
            lv = beam_levels(nl, world, cost, tie=quanta)
        elif quanta[0] == "cap":
            lv = capped_levels(nl, world, quanta[1])
        else:
            lv = balanced_levels(nl, world, cost, quanta)
        t = sum(price(r) for r in level_rotations(nl, lv, world))
        if best is None or t < best_t - 1e-9:
            best, best_t = lv, t
    return best


def _slack_graph(nl):
    """(depth, order, succ, npred, alap, rot) of the per-clock DAG: nodes in levelise() order, successor lists and input
    counts restricted to nodes that have a level (sources are ready from the start; OUTPUT wires stand for their driver),
    latest level that does not stretch the critical path, rotations per node."""
    asap = nl.levelise()
    depth = len(asap)
    n = nl.num_nodes
    level = [0] * n
    for k, lv in enumerate(asap):
        for i in lv:
            level[i] = k + 1
    order = [i for lv in asap for i in lv]
    succ = [[] for _ in range(n)]
    npred = [0] * n
    root = nl.roots()
    for i in order:
        for j in nl.ins[i]:
            j = root[j] if nl.kinds[j] == "OUTPUT" else j
            if level[j] > 0:
                succ[j].append(i)
                npred[i] += 1
    alap = [depth] * n
    for i in reversed(order):
        for s2 in succ[i]:
            alap[i] = min(alap[i], alap[s2] - 1)
    rot = [2 if nl.kinds[i] == "MUX" else 1 if nl.kinds[i] in BINARY else 0 for i in range(n)]
    return depth, order, succ, npred, alap, rot


def beam_levels(nl, world=1, cost=mi355x_level_cost, width=6, tie="id"):
    """balanced_levels with the greedy's one choice per level — where to cut the ready set — searched instead: at every
    level each kept partial schedule is continued with every cut (all ready gates; the largest multiples of a round / a
    pass per rank, and one step below each, that still hold the critical gates), and the `width` cheapest by
    (milliseconds so far + the gates not yet run at the throughput kernel's rate) survive.  Deterministic; the greedy's own
    schedule is one of the paths, a wider beam only adds others.  Ready gates of equal slack are taken by node number
    (tie="id") or fewest successors first (tie="fanout"): which of them waits changes what later levels can hold, by 1-3 %
    of a clock on the benchmark netlists, in either direction — plan_levels keeps the cheaper."""
    depth, order, succ, npred0, alap, rot = _slack_graph(nl)
    rank = (lambda i: (alap[i], len(succ[i]), i)) if tie == "fanout" else (lambda i: (alap[i], i))
    big, small = getattr(cost, "quanta", (2048, 256))
    rate = cost(big) / big
    total_rot = sum(rot)
    # a partial schedule: (ms so far, rotations done, npred, ready, levels so far)
    beam = [(0.0, 0, list(npred0), [i for i in order if npred0[i] == 0], [])]
    for k in range(1, depth + 1):
        grown = []
        for ms, done, npred, ready, levels in beam:
            free, boots = [], []
            for i in ready:
                (free if rot[i] == 0 else boots).append(i)
            boots.sort(key=rank)
            total = sum(rot[i] for i in boots)
            must = sum(rot[i] for i in boots if alap[i] <= k)
            cuts = {total}
            if total and k < depth:
                for q in (big * world, small * world):
                    for c in ((total // q) * q, (total // q) * q - q):
                        if c >= must and c > 0:
                            cuts.add(c)
            for cut in sorted(cuts):
                np2 = list(npred)
                nxt, take, acc = [], [], 0
                for i in free:
                    for s2 in succ[i]:
                        np2[s2] -= 1
                        if np2[s2] == 0:
                            nxt.append(s2)
                for i in boots:
                    if alap[i] <= k or acc + rot[i] <= cut:
                        take.append(i)
                        acc += rot[i]
                        for s2 in succ[i]:
                            np2[s2] -= 1
                            if np2[s2] == 0:
                                nxt.append(s2)
                    else:
                        nxt.append(i)
                grown.append((ms + cost(-(-acc // world)), done + acc, np2, nxt, levels + [free + take]))
        grown.sort(key=lambda st: (st[0] + (total_rot - st[1]) * rate / world, -st[1]))
        beam = grown[:width]
    best = min(beam, key=lambda st: st[0])
    assert not best[3] and sum(len(lv) for lv in best[4]) == len(order)
    return best[4]


def balanced_levels(nl, world=1, cost=mi355x_level_cost, quanta=None):
    """The per-clock DAG in as many levels as netlist.levelise() gives (the critical path is not stretched, so the number of
    level-boundary exchanges is the same), with every gate that has SLACK placed where it costs least.

    levelise() puts a gate at its earliest level.  The kernels price a level in steps — 256 rotations per pass of the
    narrow-frontier kernel, 2048 per round of the throughput kernel — so a level of 300 rotations costs two passes where
    256 + 44 deferred would cost one, if 44 of its gates can wait.  A gate can wait until its ALAP level (depth minus its
    longest path to a sink).  Greedy list scheduling, level by level: ready gates sorted by ALAP level; the gates whose
    ALAP level is now MUST run; beyond them the level is cut at the multiple of 256 / 2048 rotations (per rank) that gives
    the lowest time per rotation, and the rest waits.  NOT / CONST cost nothing and run as soon as their input exists.
    Any cut yields a valid schedule (a deferred gate's successors are deferred with it and all have the slack)."""
    if quanta is None:
        quanta = getattr(cost, "quanta", (2048, 256))
    asap = nl.levelise()
    depth = len(asap)
    n = nl.num_nodes
    level = [0] * n
    for k, lv in enumerate(asap):
        for i in lv:
            level[i] = k + 1
    order = [i for lv in asap for i in lv]
    succ = [[] for _ in range(n)]
    npred = [0] * n
    root = nl.roots()
    for i in order:
        for j in nl.ins[i]:
            j = root[j] if nl.kinds[j] == "OUTPUT" else j
            if level[j] > 0:
                succ[j].append(i)
                npred[i] += 1
    alap = [depth] * n
    for i in reversed(order):
        for s2 in succ[i]:
            alap[i] = min(alap[i], alap[s2] - 1)
    rot = [2 if nl.kinds[i] == "MUX" else 1 if nl.kinds[i] in BINARY else 0 for i in range(n)]
    ready = [i for i in order if npred[i] == 0]
    out = []
    for k in range(1, depth + 1):
        this = []

        def release(i, into):
            for s2 in succ[i]:
                npred[s2] -= 1
                if npred[s2] == 0:
                    into.append(s2)

        # free nodes run as soon as they are ready; like levelise(), they count as a level of their own for their
        # consumers (a batch never reads a slot it writes: two chained NOTs cannot share one elementwise batch)
        nxt, boots = [], []
        for i in ready:
            if rot[i] == 0:
                this.append(i)
                release(i, nxt)
            else:
                boots.append(i)
        boots.sort(key=lambda i: (alap[i], i))
        total = sum(rot[i] for i in boots)
        must = sum(rot[i] for i in boots if alap[i] <= k)
        per_rank = lambda r: -(-r // world)
        cands = {total}
        for q in (q0 * world for q0 in quanta):
            c = (total // q) * q
            if c >= must and c > 0:
                cands.add(c)
        if total and k < depth:
            cut = min(cands, key=lambda c: (cost(per_rank(c)) / c, -c))
        else:
            cut = total
        take, rest, acc = [], [], 0
        for i in boots:
            if alap[i] <= k or acc + rot[i] <= cut:
                take.append(i)
                acc += rot[i]
            else:
                rest.append(i)
        nxt.extend(rest)
        for i in take:
            release(i, nxt)
        this.extend(take)
        out.append(this)
        ready = nxt
    assert not ready and sum(len(lv) for lv in out) == len(order)
    return out


# ---- two lanes: a model of running critical levels on a CU subset beside deferrable bulk ---------------
# Upstream's ready queue (/root/reference/src/iyokan.hpp:775-883) starts a gate as soon as its inputs exist and has no level
# barrier; the level plan above has one after every level, so the narrow tail of a clock waits for the wide write-back levels in
# front of it.  Two lanes would own DISJOINT CUs (a rotation workgroup takes a whole CU's registers and LDS: profiles/HISTORY.md):
# lane A runs one batch per level of the plan on `a` CUs of every XCD, lane B runs bulk sets on the rest, ordered against lane A
# only by wait edges.  This is the pricing such a plan would be chosen by; profiles/r07_two_lane_model.txt holds what it says of
# the benchmark netlists (tools/scale_model.py --two-lane).

XCDS = 8                                                       # MI355X: 8 XCDs of 32 CUs; a lane owns the same CUs on every XCD
PENALTY_LOADED = 2.4 / 2.10                                    # narrow pass at the part's 2.4 GHz vs the clock of a busy chip
PENALTY_WORST = 2.4 / 1.97                                     # ... vs the clock a full pass starts at (profiles/r06_level_gaps.txt)


def lane_table(table, cus):
    """The level-cost table of a lane that owns `cus` of the device's CUs: its round is 8 x its CUs and its pass its CUs, at the
    full chip's milliseconds per round / pass (the device table's pass is one rotation on each of the device's CUs)."""
    out = dict(table)
    out["round"] = int(table["round"]) * cus // int(table["pass"])
    out["pass"] = int(cus)
    return out


def _split_ms(cost, rotations):
    """(ms in full rounds, ms in the pass kernel or the partial round) of one batch: the part a clock penalty applies to"""
    full = rotations // cost.quanta[0]
    base = cost(full * cost.quanta[0]) if full else 0.0
    return base, cost(rotations) - base


def simulate_lanes(a_ms, b_ms, after, before, penalty=1.0):
    """Milliseconds from the first batch to the last of a two-lane plan.  a_ms[k] = (ms in full rounds, ms in the pass kernel) of
    lane A's level k, b_ms[j] = ms of lane B's set j.  Each lane runs its batches in order; set j starts once lane A has finished
    level after[j] (-1: at once), level k starts once every set with before[j] <= k has finished.  While lane B is busy, lane A's
    pass kernel runs `penalty` times longer (rounds are priced at the loaded clock already)."""
    nb = len(b_ms)
    need = [-1] * len(a_ms)                                     # last set level k waits for
    for j, m in enumerate(before):
        if m < len(a_ms):
            need[m] = max(need[m], j)
    for k in range(1, len(need)):
        need[k] = max(need[k], need[k - 1])
    ka = jb = 0                                                 # next batch of each lane
    left_a = left_b = None                                      # [round ms, pass ms] / ms still to run of the running batch
    t = 0.0
    while ka < len(a_ms) or jb < nb:
        if left_a is None and ka < len(a_ms) and need[ka] < jb:
            left_a = list(a_ms[ka])
        if left_b is None and jb < nb and after[jb] < ka:
            left_b = b_ms[jb]
        if left_a is None and left_b is None:
            raise ValueError("two-lane plan deadlocks")
        slow = penalty if (left_b is not None and left_a is not None and left_a[0] <= 0.0) else 1.0
        steps = []
        if left_a is not None:
            steps.append(left_a[0] if left_a[0] > 0.0 else left_a[1] * slow)
        if left_b is not None:
            steps.append(left_b)
        dt = min(steps)
        t += dt
        if left_a is not None:
            if left_a[0] > 0.0:
                left_a[0] -= dt
            else:
                left_a[1] -= dt / slow
            if left_a[0] <= 1e-12 and left_a[1] <= 1e-12:
                left_a, ka = None, ka + 1
        if left_b is not None:
            left_b -= dt
            if left_b <= 1e-12:
                left_b, jb = None, jb + 1
    return t


def _rot(nl):
    return [2 if k == "MUX" else 1 if k in BINARY else 0 for k in nl.kinds]


def two_lane_levels(nl, levels, table, lane_cus, horizon=0, slack=1, head=0, xcds=XCDS):
    """A two-lane plan made of the level plan `levels` (plan_levels): every gate keeps its level, on lane A or in lane B's set of
    that level.  To lane B go, from level `head` on:
      * deferred gates: at level >= horizon, at least `slack` levels before their latest level (ALAP in `levels`), and every
        consumer of theirs in the clock deferred too (RAM and register write-backs: their sets end with the clock);
      * split gates: of a level whose remaining rotations take longer on lane A's CUs than split over both lanes, the share that
        evens the two lanes out, latest consumers first.
    NOT / CONST follow the same rules, so a NOT of a deferred gate is deferred with it or read by lane A after a wait edge.
    Returns (lane A's levels, lane B's sets as {"nodes", "level", "after", "before"}): a set reads lane A's outputs up to level
    `after` and lane A's level `before` (len(levels): end of clock) is the first to read its outputs."""
    rot = _rot(nl)
    n, depth = nl.num_nodes, len(levels)
    level = [-1] * n
    for k, lv in enumerate(levels):
        for i in lv:
            level[i] = k
    root = nl.roots()
    src = lambda j: root[j] if nl.kinds[j] == "OUTPUT" else j
    succ = [[] for _ in range(n)]
    for lv in levels:
        for i in lv:
            for j in nl.ins[i]:
                if level[src(j)] >= 0:
                    succ[src(j)].append(i)
    alap = [depth - 1] * n
    on_b = [False] * n
    for k in range(depth - 1, -1, -1):
        for i in levels[k]:
            alap[i] = min([alap[s] - 1 for s in succ[i]], default=depth - 1)
            on_b[i] = k >= max(horizon, head) and alap[i] - k >= slack and all(on_b[s] for s in succ[i])
    dev = int(table["pass"])
    ca = make_level_cost(lane_table(table, lane_cus * xcds))
    cb = make_level_cost(lane_table(table, dev - lane_cus * xcds))
    for k in range(head, depth):
        boots = [i for i in levels[k] if rot[i] and not on_b[i]]
        total = sum(rot[i] for i in boots)
        best, best_t = 0, ca(total)
        for q in ca.quanta:
            for mult in range(total // q + 2):
                ra = min(total, mult * q)
                if max(ca(ra), cb(total - ra)) < best_t - 1e-9:
                    best, best_t = total - ra, max(ca(ra), cb(total - ra))
        boots.sort(key=lambda i: (-min([level[s] for s in succ[i] if not on_b[s]], default=depth), i))
        acc = 0
        for i in boots:
            if acc + rot[i] > best:
                break
            on_b[i] = True
            acc += rot[i]
    a_levels = [[i for i in lv if not on_b[i]] for lv in levels]
    sets = []
    for k, lv in enumerate(levels):
        nodes = [i for i in lv if on_b[i]]
        if nodes:
            after = max([level[src(j)] for i in nodes for j in nl.ins[i] if level[src(j)] >= 0 and not on_b[src(j)]], default=-1)
            before = min([level[s] for i in nodes for s in succ[i] if not on_b[s]], default=depth)
            sets.append({"nodes": nodes, "level": k, "after": after, "before": before})
    return a_levels, sets


def two_lane_price(nl, a_levels, sets, table, lane_cus, penalty=PENALTY_LOADED, head=0, xcds=XCDS, extra_ms=None):
    """Model milliseconds per clock of a two-lane plan (two_lane_levels) by the device cost table `table` rescaled to each lane
    (lane_table): lane A's levels on lane_cus CUs per XCD (the levels before `head` on the whole device, lane B idle), lane B's
    sets on the rest.  A pass on lane A costs `penalty` times more while lane B runs.  extra_ms(gates, cus) adds the per-batch
    milliseconds that are not rotations (key switch, fixed cost) where the caller has them."""
    rot = _rot(nl)
    dev = int(table["pass"])
    whole = with_sub_pass_shape(make_level_cost(table))
    ca = with_sub_pass_shape(make_level_cost(lane_table(table, lane_cus * xcds)))
    cb = make_level_cost(lane_table(table, dev - lane_cus * xcds))
    extra = extra_ms or (lambda gates, cus: 0.0)

    def gates(nodes):
        return sum(1 for i in nodes if rot[i])

    a_ms = []
    for k, lv in enumerate(a_levels):
        r = sum(rot[i] for i in lv)
        base, pas = _split_ms(ca, r) if k >= head else (whole(r), 0.0)
        a_ms.append((base + (extra(gates(lv), dev if k < head else lane_cus * xcds) if r else 0.0), pas))
    b_ms = []
    for s in sets:
        r = sum(rot[i] for i in s["nodes"])
        b_ms.append(cb(r) + (extra(gates(s["nodes"]), dev - lane_cus * xcds) if r else 0.0))
    return simulate_lanes(a_ms, b_ms, [s["after"] for s in sets], [s["before"] for s in sets], penalty)


def two_lane_bound(nl, table, lane_cus, penalties=(PENALTY_LOADED,), levels=None, whole_head=False, xcds=XCDS, extra_ms=None,
                   slacks=(1, 2, 4, 8, 16, 1 << 30)):
    """For each clock penalty in `penalties`, the cheapest two-lane plan of `levels` (default plan_levels by `table`) that
    two_lane_levels makes over every deferral horizon and the minimum slacks `slacks` (1 << 30: nothing deferred, split levels
    only), priced by two_lane_price: a dict of ms, horizon, slack, head, lane A's levels and lane B's sets.  whole_head=True also
    lets the levels before the horizon run on the whole device (a third, full-device stream: an optimistic bound beyond two
    lanes)."""
    if levels is None:
        levels = plan_levels(nl, 1, make_level_cost(table))
    best = [None] * len(penalties)
    for horizon in range(len(levels)):
        for slack in slacks:
            if horizon and not whole_head and slack >= len(levels):
                continue                                        # nothing deferred: the horizon changes nothing
            head = horizon if whole_head else 0
            a_levels, sets = two_lane_levels(nl, levels, table, lane_cus, horizon, slack, head, xcds)
            if not sets:
                continue
            for p, penalty in enumerate(penalties):
                ms = two_lane_price(nl, a_levels, sets, table, lane_cus, penalty, head, xcds, extra_ms)
                if best[p] is None or ms < best[p]["ms"] - 1e-9:
                    best[p] = {"ms": ms, "horizon": horizon, "slack": slack, "head": head, "a_levels": a_levels, "sets": sets}
    return best


def stage_netlist(nl, stages, s):
    """The netlist of ONE stage of a system with CMUX memory ports (system.assign_stages), node numbers kept: every gate of another
    stage becomes a source, so the levels of this netlist hold the gates of stage `s` alone and the slack-moving planners see no
    path that crosses a port."""
    from .netlist import Netlist

    sub = Netlist()
    for i, k in enumerate(nl.kinds):
        keep = k in ("INPUT", "DFF", "OUTPUT") or stages[i] == s
        sub.kinds.append(k if keep else "INPUT")
        sub.ins.append(list(nl.ins[i]) if keep else [])
    return sub


def address_cone(nl, stages, pt):
    """The gates of stage pt.stage that the address of memory port `pt` depends on: the walk backwards from pt.addr stops at DFFs, at
    sources and at nodes of other stages (OUTPUT wires stand for their driver).  In topological order."""
    seen, order = set(), []
    stack = [(a, False) for a in pt.addr]
    while stack:
        i, done = stack.pop()
        if done:
            order.append(i)
            continue
        k = nl.kinds[i]
        if k == "OUTPUT":
            stack.append((nl.ins[i][0], False))
            continue
        if i in seen or k in ("INPUT", "DFF") or stages[i] != pt.stage:
            continue
        seen.add(i)
        stack.append((i, True))
        stack.extend((j, False) for j in nl.ins[i])
    return order


def hoist_cones(nl, stages, s, levels, ports):
    """`levels` (the planned levels of stage s, lists of nodes) with the address cones of the stage's ports moved to the earliest level
    their inputs allow — every gate, bootstrapped or not, one level behind the latest of its inputs of this stage, as levelise()
    places it — and {port name: the number of these levels that hold its cone}.  A cone is closed under the stage's predecessors, so
    the moves need nothing but the cone; a gate outside it keeps its level, which lies behind every cone gate it reads.  The number
    of levels stays: a level that a cone gate leaves still holds the gate of the stage's longest path."""
    root = nl.roots()
    at, ready = {}, {}
    for pt in ports:
        if pt.stage != s:
            continue
        top = 0
        for i in address_cone(nl, stages, pt):
            if i not in at:
                at[i] = 1 + max([at[root[j]] for j in nl.ins[i] if root[j] in at], default=-1)   # the cone holds all it reads
            top = max(top, at[i] + 1)
        ready[pt.name] = top
    if not at:
        return levels, ready
    out = [[i for i in lv if i not in at] for lv in levels]
    for i in sorted(at, key=lambda i: (at[i], i)):
        out[at[i]].append(i)
    assert all(out) and sum(map(len, out)) == sum(map(len, levels))
    return out, ready


class FrontierPlan:
    """Slot assignment + per-level, per-rank gate descriptor arrays.  `balance` (default): gates with slack are placed in
    the level where the kernels' step-shaped cost is lowest (plan_levels; `cost` = make_level_cost(hip.rotation_round()) on
    a GPU other than the 256-CU MI355X the default describes); False: every gate at its earliest level.  `stages` (node -> stage,
    System.stages): the plan is made stage by stage, each from stage_netlist — stage_levels[s] is the range of self.levels that
    stage s owns (possibly empty), and a memory port of stage s runs after it (FrontierExecutor.run(after_stage)).
    `early` (the system's memory ports, with `stages`): the gates a port's address depends on (address_cone) are moved to the earliest
    level of their stage (hoist_cones: the slack-moving planners push exactly these late), and port_ready[name] is the number of
    levels of self.levels, counted from the first, that must be enqueued before the port's address slots are final — the first
    level of its stage where the address depends on no gate of the stage.  A port may then be read beside the rest of its stage
    (FrontierExecutor.run(after_level)).  Without `early` the plan is the one of before the argument and has no port_ready."""

    def __init__(self, nl, world=1, balance=True, cost=mi355x_level_cost, spread=True, stages=None, early=None):
        self.nl, self.world = nl, world
        if early is not None and stages is None:
            raise ValueError("early= names the memory ports of a staged plan: give stages= too")
        if stages is None:
            levels = plan_levels(nl, world, cost, spread) if balance else nl.levelise()
            self.stage_levels = [range(len(levels))]
        else:
            levels, self.stage_levels = [], []
            if early is not None:
                self.port_ready = {}
            for s in range(1 + max(stages)):
                sub = stage_netlist(nl, stages, s)
                lv = [x for x in (plan_levels(sub, world, cost, spread) if balance else sub.levelise()) if x]
                if early is not None:
                    lv, ready = hoist_cones(nl, stages, s, lv, early)
                    self.port_ready.update({name: len(levels) + r for name, r in ready.items()})
                self.stage_levels.append(range(len(levels), len(levels) + len(lv)))
                levels += lv
        n = nl.num_nodes
        slot = [-1] * n
        nslots = 0
        for i, k in enumerate(nl.kinds):                       # sources first
            if k in ("INPUT", "DFF"):
                slot[i] = nslots
                nslots += 1
        self.levels = []
        for lv in levels:
            boot = [i for i in lv if nl.kinds[i] == "MUX"] + [i for i in lv if nl.kinds[i] in BINARY]
            ew = [i for i in lv if nl.kinds[i] in ("NOT", "CONSTONE", "CONSTZERO")]
            B = -(-len(boot) // world) if boot else 0
            base = nslots
            for j, i in enumerate(boot):                       # gate j -> rank j % world, position j // world
                slot[i] = base + (j % world) * B + (j // world)
            nslots += world * B
            for i in ew:
                slot[i] = nslots
                nslots += 1
            self.levels.append({"boot": boot, "ew": ew, "base": base, "B": B})
        root = nl.roots()
        for i, k in enumerate(nl.kinds):                       # OUTPUT-kind wires alias their (ultimate) driver
            if k == "OUTPUT":
                slot[i] = slot[root[i]]
        self.dffs = [i for i, k in enumerate(nl.kinds) if k == "DFF"]
        self.sources = [i for i, k in enumerate(nl.kinds) if k == "INPUT"]
        self.shadow_base = nslots
        nslots += len(self.dffs)
        self.slot, self.num_slots = slot, nslots

        def desc(nodes):
            ops = np.array([OPS[nl.kinds[i]] for i in nodes], dtype=np.int32)
            cols = []
            for c in range(3):
                cols.append(np.array([slot[nl.ins[i][c]] if len(nl.ins[i]) > c else -1 for i in nodes], dtype=np.int32))
            out = np.array([slot[i] for i in nodes], dtype=np.int32)
            return ops, cols[0], cols[1], cols[2], out

        for L in self.levels:
            L["ew_desc"] = desc(L["ew"])
            L["rank_desc"] = [desc(L["boot"][r::world]) for r in range(world)]
        d_in = np.array([slot[nl.ins[i][0]] for i in self.dffs], dtype=np.int32)
        d_sh = np.arange(self.shadow_base, self.shadow_base + len(self.dffs), dtype=np.int32)
        d_out = np.array([slot[i] for i in self.dffs], dtype=np.int32)
        cp = np.full(len(self.dffs), OPS["COPY"], dtype=np.int32)
        neg = np.full(len(self.dffs), -1, dtype=np.int32)
        self.latch_desc = (cp, d_in, neg, neg, d_sh)
        self.commit_desc = (cp, d_sh, neg, neg, d_out)

    def stats(self):
        return {"levels": len(self.levels), "slots": self.num_slots,
                "rotations": self.nl.rotations(),
                "max_rank_gates_per_level": [L["B"] for L in self.levels]}


def _check_lanes(lanes):
    if not isinstance(lanes, (int, np.integer)) or lanes < 1:
        raise ValueError(f"lanes = {lanes!r}: a backend has one lane or more")


def _lane_slots(be, slots, lane):
    """slots of one lane's image -> slots of the backend's arena: + lane * lane_stride.  A slot outside the image, and a lane the
    backend does not have, are refused: lane r owns [r * lane_stride, (r + 1) * lane_stride) and nothing else."""
    if not 0 <= lane < be.lanes:
        raise ValueError(f"lane {lane} of a backend with {be.lanes}")
    s = np.asarray(slots, dtype=np.int64)
    if s.size and (s.min() < 0 or s.max() >= be.lane_stride):
        raise ValueError(f"slot outside the lane's {be.lane_stride} slots")
    return s + lane * be.lane_stride


class PlainBitBackend:
    """Bits instead of ciphertexts: arena = torch.uint8 [slots, 1] on CPU.  Test support.
    lanes > 1: that many copies of the circuit's image in one arena, lane r in slots [r * num_slots, (r + 1) * num_slots); a gate
    batch runs on every lane, the descriptors are one lane's (the bits twin of HipBackend(lanes=))."""

    def __init__(self, num_slots, lanes=1):
        import torch

        _check_lanes(lanes)
        self.lanes, self.lane_stride = lanes, num_slots
        self.arena = torch.zeros((lanes * num_slots, 1), dtype=torch.uint8)

    def gate_batch(self, ops, in0, in1, in2, out):
        for r in range(self.lanes):
            self._lane_batch(self.arena.numpy()[r * self.lane_stride:(r + 1) * self.lane_stride, 0], ops, in0, in1, in2, out)

    @staticmethod
    def _lane_batch(a, ops, in0, in1, in2, out):
        v0 = a[np.maximum(in0, 0)]
        v1 = a[np.maximum(in1, 0)]
        v2 = a[np.maximum(in2, 0)]
        res = np.zeros(len(ops), dtype=np.uint8)
        table = {
            "AND": v0 & v1, "NAND": 1 ^ (v0 & v1), "ANDNOT": v0 & (1 ^ v1), "OR": v0 | v1, "NOR": 1 ^ (v0 | v1),
            "ORNOT": v0 | (1 ^ v1), "XOR": v0 ^ v1, "XNOR": 1 ^ v0 ^ v1, "MUX": np.where(v2 == 1, v1, v0),
            "NOT": 1 ^ v0, "CONSTONE": np.ones_like(v0), "CONSTZERO": np.zeros_like(v0), "COPY": v0,
        }
        for name, code in OPS.items():
            m = ops == code
            if m.any():
                res[m] = table[name][m]
        a[out] = res

    def write(self, slot, value, lane=0):
        self.arena[int(_lane_slots(self, slot, lane)), 0] = int(np.asarray(value).reshape(-1)[0])

    def write_many(self, slots, values, lane=0):
        self.arena.numpy()[_lane_slots(self, slots, lane), 0] = np.asarray(values, dtype=np.uint8).reshape(len(slots))

    def read(self, slot, lane=0):
        return int(self.arena[int(_lane_slots(self, slot, lane)), 0])

    def read_many(self, slots, lane=0):
        return [self.read(s_, lane) for s_ in slots]

    def sync(self):
        pass


class HipBackend:
    """Ciphertexts in HBM: arena = torch.int32 [slots, n+1] on the rank's GPU, kernels through the
    C ABI on torch's current stream (so RCCL collectives issued by torch.distributed order with them).
    lanes > 1: that many copies of the circuit's image in one arena, lane r in slots [r * num_slots, (r + 1) * num_slots); a gate batch
    is ONE Stream.gate_batch(lanes=, lane_stride=num_slots) — one lane's descriptors, count x lanes gates on the GPU."""

    def __init__(self, num_slots, params, device, lanes=1):
        import torch

        from . import hip

        _check_lanes(lanes)
        self.torch, self.hip = torch, hip
        self.lanes, self.lane_stride = lanes, num_slots
        self.arena = torch.zeros((lanes * num_slots, params.n + 1), dtype=torch.int32, device=device)
        self._tstream = torch.cuda.Stream(device=device)
        torch.cuda.synchronize(device)
        self.stream = hip.Stream(0, hip_stream=self._tstream.cuda_stream)
        self._arena = hip.Arena.from_torch(self.arena)
        self.torch_stream = self._tstream

    def gate_batch(self, ops, in0, in1, in2, out):
        if len(ops):
            if self.lanes == 1:
                self.stream.gate_batch(self._arena, ops, in0, in1, in2, out)
            else:
                self.stream.gate_batch(self._arena, ops, in0, in1, in2, out, lanes=self.lanes, lane_stride=self.lane_stride)

    def write(self, slot, tlwe, lane=0):
        t = self.torch.from_numpy(np.ascontiguousarray(tlwe, dtype=np.uint32).view(np.int32))
        with self.torch.cuda.stream(self._tstream):
            self.arena[int(_lane_slots(self, slot, lane))].copy_(t)
        self._tstream.synchronize()

    def write_many(self, slots, tlwe_rows, lane=0):
        rows = np.ascontiguousarray(tlwe_rows, dtype=np.uint32).reshape(len(slots), -1).view(np.int32)
        idx = self.torch.as_tensor(_lane_slots(self, slots, lane), device=self.arena.device)
        with self.torch.cuda.stream(self._tstream):
            self.arena[idx] = self.torch.from_numpy(rows).to(self.arena.device)
        self._tstream.synchronize()

    def read(self, slot, lane=0):
        self._tstream.synchronize()
        return self.arena[int(_lane_slots(self, slot, lane))].cpu().numpy().view(np.uint32)

    def read_many(self, slots, lane=0):
        self._tstream.synchronize()
        idx = self.torch.as_tensor(_lane_slots(self, slots, lane), device=self.arena.device)
        return self.arena[idx].cpu().numpy().view(np.uint32)

    def sync(self):
        self._tstream.synchronize()

    def close(self):
        self.stream.destroy()


class FrontierExecutor:
    def __init__(self, plan, backend, rank=0, world=1, dist=None):
        assert plan.world == world
        if getattr(backend, "lanes", 1) > 1 and world > 1:
            raise ValueError("lanes > 1 with world > 1: the level exchange lists are per slot of ONE image — lanes over several GPUs are not built")
        self.plan, self.be, self.rank, self.world, self.dist = plan, backend, rank, world, dist
        self.collectives = 0

    # ---- host-visible ports (TaskMem::set/get) -------------------------------------------
    # lane: which copy of the image on a backend with lanes (0 on every other: backends without lanes take no such argument)
    def set_input(self, port, bit, value, lane=0):
        self.set_node(self.plan.nl.inputs[(port, bit)], value, lane)

    def get_output(self, port, bit, lane=0):
        return self.get_node(self.plan.nl.outputs[(port, bit)], lane)

    def set_node(self, node, value, lane=0):
        self.be.write(self.plan.slot[node], value, **_lane_kw(lane))

    def get_node(self, node, lane=0):
        return self.be.read(self.plan.slot[node], **_lane_kw(lane))

    # ---- one combinational evaluation -------------------------------------------------------
    def run(self, after_stage=None, after_level=None):
        """after_stage(s): called once the levels of stage s are enqueued (a staged plan's memory ports), on the same stream.
        after_level(i): called with i = 0 before the first level and with every further i up to len(plan.levels) once level i - 1 is
        enqueued (a port whose address is ready there: plan.port_ready) — at a stage's last level in front of after_stage."""
        if after_level is None:
            if after_stage is None:
                return self._run_levels(self.plan.levels)
            for s, rng in enumerate(self.plan.stage_levels):
                self._run_levels(self.plan.levels[rng.start:rng.stop])
                after_stage(s)
            return
        after_level(0)
        for s, rng in enumerate(self.plan.stage_levels):
            self._run_levels(self.plan.levels[rng.start:rng.stop], rng.start, after_level)
            if after_stage is not None:
                after_stage(s)

    def _run_levels(self, levels, first=0, after_level=None):
        be, w = self.be, self.world
        ctx = be.torch.cuda.stream(be.torch_stream) if hasattr(be, "torch_stream") else _null()
        with ctx:
            for k, L in enumerate(levels):
                if k and after_level is not None:
                    after_level(first + k)
                be.gate_batch(*L["ew_desc"])
                if L["B"] == 0:
                    continue
                be.gate_batch(*L["rank_desc"][self.rank])
                if self.dist is not None:
                    # The level's one exchange, IN PLACE on the arena: the slot layout puts rank r's outputs of this level at
                    # [base + r B, base + (r + 1) B), so the rank's block is already where the gathered tensor wants it (RCCL's
                    # in-place all-gather: send buffer = receive buffer + rank * count; no staging copy).  Issued whenever a
                    # process group exists — with ONE rank too, so that the 1-GPU boxes this is developed on execute the very
                    # collective the 8-GPU run depends on (tests/test_gpu_bench_launcher.py asserts it ran).
                    lo, B = L["base"], L["B"]
                    whole = be.arena[lo: lo + w * B]
                    mine = be.arena[lo + self.rank * B: lo + (self.rank + 1) * B]
                    self._all_gather(whole, mine)
                    self.collectives += 1
            if levels and after_level is not None:
                after_level(first + len(levels))

    def _all_gather(self, whole, mine):
        """RCCL all_gather_into_tensor on the device arena.  Test rigs with ONE GPU run the ranks as processes sharing that
        GPU over gloo (RCCL refuses two ranks on one device; gloo has no device all-gather): the same per-level exchange,
        staged through the host — every other line of the sharded path (plans, per-rank batches, slot layout) is the product's."""
        if self.dist.get_backend() == "gloo":
            host = whole.new_empty(whole.shape, device="cpu")
            self.dist.all_gather_into_tensor(host, mine.cpu().clone())
            whole.copy_(host)
        else:
            self.dist.all_gather_into_tensor(whole, mine)

    # ---- clock edge: two-phase latch so DFF -> DFF chains sample the old value ---------------
    def tick(self):
        be = self.be
        ctx = be.torch.cuda.stream(be.torch_stream) if hasattr(be, "torch_stream") else _null()
        with ctx:
            if len(self.plan.dffs):
                be.gate_batch(*self.plan.latch_desc)
                be.gate_batch(*self.plan.commit_desc)

    def sync(self):
        self.be.sync()


def _lane_kw(lane):
    return {"lane": lane} if lane else {}


class _null:
    def __enter__(self):
        return self

    def __exit__(self, *a):
        return False
