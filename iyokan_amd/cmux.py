"""CMUX memories on the GPU: the read tree of a ROM over TRLWE rows (Stream.cmux_batch + index extraction; optionally the upper levels as
one fused Stream.cmux_tree_batch per four levels and the rotate tail as one fused Stream.cmux_rotate_chain_batch), and a RAM — read tree,
MUXwoSE, one fused chain of CMUXes per cell (Stream.cmux_chain_batch) and the refresh of every cell.

Replaces the reference's TaskTFHEppROMUX (UROMUX + LROMUX, /root/reference/src/iyokan_tfhepp.hpp:238-300) followed by one
TaskTFHEppSEI per output bit (:340-352), and its RAM network (:409-787: TaskTFHEppRAMUX, TaskTFHEppGateMUXWoSE, TaskTFHEppRAMCMUXs,
TaskTFHEppRAMGateBootstrapping).

Orientation: a CMUX job computes T[out] = T[in0] + S [.] (T[in1] - T[in0]), so a selector that encrypts 1 selects in1.  The plan
below puts the even row of a pair in in0 and the odd row in in1 and is driven by the address bits AS THEY ARE.  The reference calls
CMUXFFT(out, sel, data[2 i], data[2 i + 1]) (1 selects the EVEN row) and therefore feeds its ROM inverted selectors; with this
interface that is the caller's choice of in0 / in1, not a second kind of selector.
"""
from collections import namedtuple

import numpy as np

# One CMUX of a plan.  bit: the address bit whose selector drives it.  in0 / in1 / out: rows — 0 .. data_rows-1 are the ROM's
# TRLWEs (never written), data_rows .. data_rows+scratch_rows-1 the scratch rows of ONE read.  in1 = -1: rotate form with `rot`.
PlanJob = namedtuple("PlanJob", "bit in0 in1 rot out")
RomLayout = namedtuple("RomLayout", "data_rows scratch_rows result log2_words")


def rom_layout(addr_width, log2_word_bits, N):
    """Rows of one ROM read: data_rows TRLWEs of N / 2^log2_word_bits words each, the scratch rows its plan uses, the scratch row that
    holds the selected word (bit i at coefficient i) after the last launch, and log2 of the words per TRLWE."""
    log2_n = int(N).bit_length() - 1
    assert 1 << log2_n == N and 0 <= log2_word_bits <= log2_n and addr_width >= 1
    log2_words = log2_n - log2_word_bits
    upper = max(addr_width - log2_words, 0)
    data_rows = 1 << upper
    # level b writes 2^(upper-1-b) rows: levels alternate between two regions, so that no job reads what a job of its launch writes
    scratch = (data_rows // 2 + data_rows // 4) if upper >= 2 else 1
    return RomLayout(data_rows, scratch, data_rows, log2_words)


def rom_read_plan(addr_width, log2_word_bits, N):
    """The ordered launches of one ROM read, each a list of PlanJob that are independent of each other (one cmux_batch).

    First the upper tree (UROMUX): with a = addr_width - log2(words per TRLWE) upper address bits, level b < a has 2^(a-1-b) jobs,
    each selected by address bit log2(words per TRLWE) + b, halving the candidate rows.  Then one rotate-form job per low address
    bit (LROMUX), highest first: rot = 2N - (N >> bit) for bit = 1 .. log2(words), selected by address bit log2(words) - bit, in
    place on the result row — it moves the addressed word to coefficient 0."""
    lay = rom_layout(addr_width, log2_word_bits, N)
    D, W = lay.data_rows, lay.log2_words
    upper = max(addr_width - W, 0)
    region = [D, D + D // 2]   # first rows of the two scratch regions
    launches = []
    src = list(range(D))
    for b in range(upper):
        base = lay.result if b == upper - 1 else region[b & 1]   # the last level's one job writes the result row (its own in0 at most)
        jobs = [PlanJob(W + b, src[2 * i], src[2 * i + 1], 0, base + i) for i in range(len(src) // 2)]
        launches.append(jobs)
        src = [j.out for j in jobs]
    cur = src[0]   # one row left: a data row when there is no upper tree
    for bit in range(1, W + 1):
        if W - bit >= addr_width:
            continue
        launches.append([PlanJob(W - bit, cur, -1, 2 * N - (N >> bit), lay.result)])
        cur = lay.result
    return launches   # empty for a one-word ROM: nothing to select


# The rotate tail of a read plan as ONE job of Stream.cmux_rotate_chain_batch: acc = row src; step j is the rotate-form CMUX selected by
# address bit bits[j] with rotation rots[j]; row out = acc.
RotateChain = namedtuple("RotateChain", "steps bits rots src out")


def rom_rotate_chain(plan):
    """The trailing rotate-form launches of a rom_read_plan (LROMUX: one job each, every one but the first in place on the result row)
    as one RotateChain; the len(plan) - steps launches in front of them are the upper tree.  None where the plan has no rotate step:
    every word fills a whole TRLWE."""
    tail = []
    for jobs in reversed(plan):
        if len(jobs) != 1 or jobs[0].in1 >= 0:
            break
        tail.append(jobs[0])
    if not tail:
        return None
    tail.reverse()
    out = tail[-1].out
    assert all(j.out == out for j in tail) and all(j.in0 == out for j in tail[1:])
    return RotateChain(len(tail), tuple(j.bit for j in tail), tuple(j.rot for j in tail), tail[0].in0, out)


# One job of Stream.cmux_tree_batch, in plan rows: the 2^levels leaves first .. are halved `levels` times, level b selected by address
# bit bit0 + b; row out is the one left.
TreeJob = namedtuple("TreeJob", "bit0 levels first out")
TREE_MAX_LEVELS = 4


def rom_tree_jobs(plan):
    """The upper levels of a rom_read_plan (the two-row launches in front of the rotate tail) cut into groups of at most
    TREE_MAX_LEVELS levels, each group ONE cmux_tree_batch: [(jobs, region)], jobs a list of TreeJob that are independent of each other,
    region the scratch region (0 or 1) the group writes, None for the last group, whose one job writes the result row.  A group's
    leaves are the candidates in front of its first level — the data rows, then the outs of the group before, which are consecutive rows
    of one region — so the plan's two regions suffice, alternating per group.  Empty where the plan has no upper tree."""
    upper = [jobs for jobs in plan if jobs[0].in1 >= 0]
    assert upper == plan[: len(upper)]
    if not upper:
        return []
    D = 2 * len(upper[0])
    assert upper[0][0].in0 == 0 and len(upper[-1]) == 1
    result = upper[-1][0].out
    region = [D, D + D // 2]   # rom_read_plan's two scratch regions
    groups, first, lo, g = [], 0, 0, 0
    while lo < len(upper):
        levels = min(TREE_MAX_LEVELS, len(upper) - lo)
        count = len(upper[lo + levels - 1])
        last = lo + levels == len(upper)
        base = result if last else region[g & 1]
        groups.append(([TreeJob(upper[lo][0].bit, levels, first + (i << levels), base + i) for i in range(count)], None if last else g & 1))
        first, lo, g = base, lo + levels, g + 1
    return groups


def selectors_from_tlwe2(stream, key, tlwe2, first, addr_width, trlwe_scratch, trgsw, first_slot=0):
    """The selectors of a whole address from ciphertexts, on the device: TLWE lvl2 slot first + bit l + r of `tlwe2` holds gadget digit r
    of address bit `bit` (bit * 2^(64 - (r+1) Bgbit): client.encrypt_cb_digits, later the lvl0 -> lvl2 rotation).  ONE privks_batch of
    addr_width (k+1) l key switches into rows 0 .. of `trlwe_scratch` (row (bit (k+1) + c) l + r), then ONE trgsw_from_rows into
    selector slots first_slot .. first_slot + addr_width - 1 of `trgsw`.  Replaces the second half of the reference's TaskTFHEppCB in
    front of a ROM / RAM port (/root/reference/src/iyokan_tfhepp.hpp:194-236).  Asynchronous on the stream."""
    from . import hip

    p = hip.current_params()
    l, k1 = int(p.l), int(p.k) + 1
    per = k1 * l
    if trlwe_scratch.slots < addr_width * per:
        raise ValueError(f"{addr_width * per} scratch rows needed, the store has {trlwe_scratch.slots}")
    in_, c, out = [], [], []
    for bit in range(addr_width):
        for cc in range(k1):
            for r in range(l):
                in_.append(first + bit * l + r)
                c.append(cc)
                out.append(bit * per + cc * l + r)
    stream.privks_batch(key, tlwe2, in_, c, trlwe_scratch, out)
    stream.trgsw_from_rows(trgsw, np.arange(first_slot, first_slot + addr_width), trlwe_scratch,
                           np.arange(addr_width * per).reshape(addr_width, per))


def selectors_from_tlwe0(stream, bk2, privks_key, arena, addr_slots, tlwe2, first, trlwe_scratch, trgsw, first_slot=0, invert=False,
                         many=False):
    """The selectors of a whole address from its lvl0 TLWEs in `arena` (slot addr_slots[bit]), on the device: circuit bootstrapping.
    ONE cb_rotate_batch of len(addr_slots) * l rotations under the lvl2 bootstrapping key `bk2` into TLWE lvl2 slots first + bit l + r of
    `tlwe2` (mu = 2^(63 - (r+1) Bgbit), off = 0; invert: sign = -1, the selector of the negated bit — the reference's
    CircuitBootstrappingFFTInv), then selectors_from_tlwe2.  Replaces the reference's TaskTFHEppCB / CBInv in front of a ROM / RAM port
    (/root/reference/src/iyokan_tfhepp.hpp:194-236).  many=True: ONE cb_rotate_many_batch of len(addr_slots) rotations instead — each
    gives the l TLWEs of its bit, into the same slots (the many-digit form; l <= 4).  Asynchronous on the stream."""
    from . import hip

    p = hip.current_params()
    l, bg = int(p.l), int(p.Bgbit)
    addr_slots = [int(s) for s in np.asarray(addr_slots).ravel()]
    if many:
        bits = len(addr_slots)
        stream.cb_rotate_many_batch(bk2, arena, addr_slots, [-1 if invert else 1] * bits, [0] * bits,
                                    np.array([1 << (63 - (r + 1) * bg) for r in range(l)], dtype=np.uint64), tlwe2,
                                    [first + bit * l for bit in range(bits)])
        selectors_from_tlwe2(stream, privks_key, tlwe2, first, bits, trlwe_scratch, trgsw, first_slot)
        return
    in_, mu, out = [], [], []
    for bit, slot in enumerate(addr_slots):
        for r in range(l):
            in_.append(slot)
            mu.append(1 << (63 - (r + 1) * bg))
            out.append(first + bit * l + r)
    count = len(in_)
    stream.cb_rotate_batch(bk2, arena, in_, [-1 if invert else 1] * count, [0] * count, np.array(mu, dtype=np.uint64), tlwe2, out)
    selectors_from_tlwe2(stream, privks_key, tlwe2, first, len(addr_slots), trlwe_scratch, trgsw, first_slot)


def _selector_store(trgsw, sel_base, need):
    """Refuses (ValueError) a selector store and base slot that cannot hold `need` selectors; trgsw=None: the memory's own store, base 0."""
    sel_base = int(sel_base)
    if trgsw is None:
        if sel_base != 0:
            raise ValueError("sel_base needs the selector store it is a slot of (trgsw=...)")
        return 0
    if trgsw.slots < need:
        raise ValueError(f"{need} selector slots needed, the store has {trgsw.slots}")
    if sel_base < 0 or sel_base + need > trgsw.slots:
        raise ValueError(f"selector slots {sel_base} .. {sel_base + need - 1} are outside the store's {trgsw.slots}")
    return sel_base


# ---- lanes: K copies of one memory at fixed strides (csrc/cmux_lane_jobs.hpp) --------------------------------
# A memory's job lists stay ONE lane's.  The four CMUX families go through the Stream.cmux_*_batch calls with lanes / sel_stride /
# row_stride and are expanded on the device; the flat index arrays of the extraction, MUXwoSE, the add and the refresh are replicated
# here, lane-major, with one numpy broadcast.
def lane_flat(a, lanes, stride):
    """Lane 0's index array for all lanes, lane-major: entry r * len(a) + g is a[g] + r * stride; a negative entry ("none") stays."""
    a = np.asarray(a, dtype=np.int64).ravel()
    if lanes == 1:
        return a
    return np.where(a < 0, a, np.add.outer(np.arange(lanes, dtype=np.int64) * int(stride), a)).ravel()


def lane_tile(a, lanes):
    """An array of per-job values that are the same in every lane, lane-major."""
    a = np.asarray(a).ravel()
    return a if lanes == 1 else np.tile(a, lanes)


def _lane_setup(lanes, sel_stride, arena_stride, trgsw, sel_base, sel_need, what):
    """(lanes, sel_stride, arena_stride) of a memory, refused (ValueError) before anything is allocated: lanes > 1 needs arena_stride, and
    a caller's selector store must hold the last lane's slots.  sel_stride None: sel_need, the slots one lane uses."""
    lanes = int(lanes)
    if lanes < 1:
        raise ValueError(f"lanes {lanes}: at least one")
    sel_stride = int(sel_need if sel_stride is None else sel_stride)
    if lanes > 1:
        if arena_stride is None:
            raise ValueError(f"a {what} of {lanes} lanes needs arena_stride: lane r's arena slots are lane 0's + r * arena_stride")
        if sel_stride < 1 or int(arena_stride) < 1:
            raise ValueError("sel_stride and arena_stride of a laned memory are at least 1")
        if trgsw is not None and int(sel_base) + (lanes - 1) * sel_stride + sel_need > trgsw.slots:
            raise ValueError(f"selector slots up to {int(sel_base) + (lanes - 1) * sel_stride + sel_need - 1} needed for {lanes} lanes, "
                             f"the store has {trgsw.slots}")
    return lanes, sel_stride, None if arena_stride is None else int(arena_stride)


class Rom:
    """A ROM of TRLWE rows on one GPU.  read() runs rom_read_plan for R independent reads at once: the jobs of all reads at one
    level go into ONE cmux_batch, each read with its own scratch rows and its own addr_width selectors; then bit i of every read's
    word is extracted at coefficient index i and key-switched into an arena slot.
    trgsw, sel_base: a selector store the caller owns and the first of the addr_width * max_reads slots this ROM uses in it (read r, bit b
    at sel_base + r * addr_width + b); every job list names those slots, uploads go there, and free() leaves the store alone.  Without
    them the ROM allocates and frees a store of its own, slots from 0.
    lanes=K: K copies of the ROM, one per request packet, in one store: lane r's rows are lane 0's + r * row_stride (row_stride the
    one-lane store's rows), its selector slots lane 0's + r * sel_stride (default addr_width * max_reads) and its arena slots lane 0's +
    r * arena_stride.  data_trlwe is one image for every lane or K images, lane-major; upload_lane replaces one lane's.  The job lists
    stay ONE lane's and every read runs all lanes in the same launches (Stream.cmux_*_batch(lanes=...)): lane r's words are those of a
    one-lane ROM with lane r's image and selectors."""

    sel_base, own_trgsw = 0, True   # of a ROM with a selector store of its own
    lanes, sel_stride, arena_stride = 1, None, None

    def __init__(self, stream, data_trlwe, addr_width, log2_word_bits, max_reads=1, trgsw=None, sel_base=0, lanes=1, sel_stride=None,
                 arena_stride=None):
        from . import hip

        p = hip.current_params()
        self.stream, self.addr_width, self.N = stream, int(addr_width), int(p.N)
        self.word_bits = 1 << log2_word_bits
        self.layout = rom_layout(addr_width, log2_word_bits, p.N)
        self.plan = rom_read_plan(addr_width, log2_word_bits, p.N)
        if not self.plan:
            raise ValueError("a ROM of one word has no read tree")
        data = np.ascontiguousarray(data_trlwe, dtype=np.uint32).reshape(-1, 2 * p.N)
        self.max_reads = int(max_reads)
        self.lanes, self.sel_stride, self.arena_stride = _lane_setup(lanes, sel_stride, arena_stride, trgsw, sel_base,
                                                                     self.max_reads * self.addr_width, "ROM")
        if data.shape[0] not in (self.layout.data_rows, self.lanes * self.layout.data_rows):
            raise ValueError(f"expected {self.layout.data_rows} TRLWE rows, got {data.shape[0]}")
        self.sel_base = _selector_store(trgsw, sel_base, self.max_reads * self.addr_width)   # refused before anything is allocated
        self.own_trgsw = trgsw is None
        self.row_stride = self.layout.data_rows + self.max_reads * self.layout.scratch_rows   # the one-lane store
        self.trlwe = hip.Trlwe(self.lanes * self.row_stride, stream.gpu_index)
        self.trgsw = (hip.Trgsw((self.lanes - 1) * self.sel_stride + self.max_reads * self.addr_width, stream.gpu_index)
                      if self.own_trgsw else trgsw)
        images = data.reshape(-1, self.layout.data_rows, 2 * p.N)
        for lane in range(self.lanes):
            self.upload_lane(lane, images[lane if len(images) > 1 else 0])

    def _lanes_kw(self):
        """What the Stream.cmux_*_batch calls get behind ONE lane's lists; one lane: nothing, the call of before lanes."""
        return {} if self.lanes == 1 else dict(lanes=self.lanes, sel_stride=self.sel_stride, row_stride=self.row_stride)

    def upload_lane(self, lane, data_trlwe):
        """Lane `lane`'s image: its data rows, at lane * row_stride.  Asynchronous on the stream."""
        if not 0 <= lane < self.lanes:
            raise ValueError(f"lane {lane} of {self.lanes}")
        data = np.ascontiguousarray(data_trlwe, dtype=np.uint32).reshape(-1, 2 * self.N)
        if data.shape[0] != self.layout.data_rows:
            raise ValueError(f"expected {self.layout.data_rows} TRLWE rows, got {data.shape[0]}")
        self.trlwe.upload(self.stream, lane * self.row_stride, data)

    def row(self, read, plan_row):
        """Row of the TRLWE store that plan row `plan_row` is for read number `read`."""
        D, S = self.layout.data_rows, self.layout.scratch_rows
        return plan_row if plan_row < D else D + read * S + (plan_row - D)

    def launches(self, reads):
        """The cmux_batch argument lists (sel, in0, in1, rot, out) of `reads` simultaneous reads, one tuple per launch."""
        out = []
        for jobs in self.plan:
            cols = [[], [], [], [], []]
            for r in range(reads):
                for j in jobs:
                    vals = (self.sel_base + r * self.addr_width + j.bit, self.row(r, j.in0), -1 if j.in1 < 0 else self.row(r, j.in1), j.rot,
                            self.row(r, j.out))
                    for c, v in zip(cols, vals):
                        c.append(v)
            out.append(tuple(cols))
        return out

    def launches_fused(self, reads):
        """(the cmux_batch argument lists of the upper tree, exactly the first ones of launches(reads); ONE cmux_rotate_chain_batch
        argument tuple (steps, sel, rot, src, out) with one job per read for the rotate tail, None where the plan has none)."""
        chain = rom_rotate_chain(self.plan)
        if chain is None:
            return self.launches(reads), None
        steps, sel, rot, src, out = [], [], [], [], []
        for r in range(reads):
            steps.append(chain.steps)
            sel.extend(self.sel_base + r * self.addr_width + b for b in chain.bits)
            rot.extend(chain.rots)
            src.append(self.row(r, chain.src))
            out.append(self.row(r, chain.out))
        return self.launches(reads)[: len(self.plan) - chain.steps], (steps, sel, rot, src, out)

    def tree_launches(self, reads):
        """The cmux_tree_batch argument lists (sel0, levels, first, out) of the upper tree of `reads` simultaneous reads, one tuple per
        group of rom_tree_jobs: they replace the first sum(levels) tuples of launches(reads)."""
        out = []
        for jobs, _ in rom_tree_jobs(self.plan):
            rows = [(self.sel_base + r * self.addr_width + j.bit0, j.levels, self.row(r, j.first), self.row(r, j.out))
                    for r in range(reads) for j in jobs]
            out.append(tuple(zip(*rows)))
        return out

    def read(self, addr_trgsw, arena, out_slots, resident=False, fused=False, fused_tree=False):
        """addr_trgsw: u32 [R][addr_width][(k+1) l][k+1][N] (client.encrypt_trgsw of every read's address bits, bit 0 first);
        out_slots: [R][word_bits] arena slots.  Asynchronous on the stream.  resident=True: the selectors are in self.trgsw already
        (slot sel_base + read * addr_width + bit, e.g. from selectors_from_tlwe2 on this stream): addr_trgsw is ignored and nothing is uploaded.
        fused=True sends the rotate tail of all reads as ONE cmux_rotate_chain_batch instead of one cmux_batch per step, fused_tree=True
        the upper tree as ONE cmux_tree_batch per four levels instead of one cmux_batch per level: the same words either way.
        lanes > 1: addr_trgsw is [lanes][R][addr_width]..., lane r's selectors uploaded at + r * sel_stride; out_slots stay lane 0's
        [R][word_bits], lane r's results land at + r * arena_stride."""
        K = self.lanes
        if resident:
            out_slots = np.asarray(out_slots, dtype=np.int32).reshape(-1, self.word_bits)
            reads = out_slots.shape[0]
        else:
            sel = np.ascontiguousarray(addr_trgsw, dtype=np.uint32).reshape(-1, self.addr_width, self.trgsw.words)
            if sel.shape[0] % K:
                raise ValueError(f"{sel.shape[0]} addresses for {K} lanes")
            reads = sel.shape[0] // K
            out_slots = np.asarray(out_slots, dtype=np.int32).reshape(reads, self.word_bits)
        if reads > self.max_reads:
            raise ValueError(f"{reads} reads, sized for {self.max_reads}")
        if not resident:
            for lane in range(K):
                self.trgsw.upload(self.stream, self.sel_base + lane * self.sel_stride, sel[lane * reads:(lane + 1) * reads])
        kw = self._lanes_kw()
        upper, chain = self.launches_fused(reads) if fused else (self.launches(reads), None)
        if fused_tree:
            trees = self.tree_launches(reads)
            for args in trees:
                self.stream.cmux_tree_batch(self.trgsw, self.trlwe, *args, **kw)
            upper = upper[sum(args[1][0] for args in trees):]   # what is left of `upper` is the unfused rotate tail
        for args in upper:
            self.stream.cmux_batch(self.trgsw, self.trlwe, *args, **kw)
        if chain is not None:
            self.stream.cmux_rotate_chain_batch(self.trgsw, self.trlwe, *chain, **kw)
        rows = np.repeat([self.row(r, self.layout.result) for r in range(reads)], self.word_bits)
        coeff = np.tile(np.arange(self.word_bits), reads)
        if K == 1:
            self.stream.sample_extract_index_keyswitch_batch(self.trlwe, rows, coeff, out_slots.ravel(), arena)
        else:
            self.stream.sample_extract_index_keyswitch_batch(self.trlwe, lane_flat(rows, K, self.row_stride), lane_tile(coeff, K),
                                                             lane_flat(out_slots, K, self.arena_stride), arena)

    def free(self):
        self.trlwe.free()
        if self.own_trgsw:
            self.trgsw.free()


# ---- RAM ----------------------------------------------------------------------------------------------------------------------
# One chain of CMUXes (Stream.cmux_chain_batch): acc = T[src]; step j < steps with selector slot sel0 + j keeps acc where that selector
# encrypts bit j of pattern and takes T[mem] otherwise; T[out] = acc.
ChainJob = namedtuple("ChainJob", "sel0 steps pattern src mem out")


def ram_layout(addr_width, N):
    """Rows of the read tree of one bit plane of a RAM: 2^addr_width cells of one bit each (at coefficient 0), the scratch rows of
    the plan and the scratch row that holds the addressed cell after the last launch."""
    return rom_layout(addr_width, int(N).bit_length() - 1, N)


def ram_read_plan(addr_width, N):
    """The reference's RAMUX as launches: rom_read_plan at ONE word per TRLWE — level b has 2^(addr_width-1-b) jobs selected by
    address bit b, the even cell in in0 and the odd cell in in1, the address bits as they are (the reference feeds
    CMUXFFT(out, inverted selector, even, odd), :421-443)."""
    return rom_read_plan(addr_width, int(N).bit_length() - 1, N)


def ram_write_jobs(addr_width, src, first_cell=0, sel0=0):
    """The reference's RAMCMUXs of one bit plane, one chain job per cell i < 2^addr_width: pattern = i, steps = addr_width,
    src = the row of the written TRLWE (MUXwoSE's output), mem = out = the cell's row first_cell + i.  Cell i keeps src where every
    selector j encrypts bit j of i — the addressed cell — and gets its old content back otherwise."""
    assert 1 <= addr_width <= 32
    return [ChainJob(sel0, addr_width, i, src, first_cell + i, first_cell + i) for i in range(1 << addr_width)]


def chain_steps(job, acc):
    """A chain job as `steps` dependent cmux_batch jobs (sel, in0, in1, rot, out), one per launch, with the accumulator kept in row
    `acc` between them: what Ram.clock(fused=False) sends."""
    jobs = []
    for j in range(job.steps):
        cur = job.src if j == 0 else acc
        out = job.out if j == job.steps - 1 else acc
        jobs.append((job.sel0 + j, job.mem, cur, 0, out) if (job.pattern >> j) & 1 else (job.sel0 + j, cur, job.mem, 0, out))
    return jobs


class Ram:
    """A RAM of 2^addr_width words of data_width bits on one GPU, one TRLWE per bit (the bit at coefficient 0), as the reference
    keeps it.  One Trlwe store holds the data_width bit planes of 2^addr_width cell rows, then per plane the read tree's scratch
    rows and two rows for MUXwoSE, then one accumulator row per cell for the unfused write-back; one Trgsw store holds the
    addr_width selectors of the current clock; a private arena holds the TLWEs between the write-back and the refresh.
    trgsw, sel_base: a selector store the caller owns and the first of the addr_width slots this RAM uses in it (bit b at sel_base + b);
    every job list names those slots, uploads go there, and free() leaves the store alone.  Without them the RAM allocates and frees a
    store of its own, slots from 0.

    Refresh aside (write_port(refresh_stream=...)).  The refresh of every cell — steps 5 and 6 — is what the NEXT read tree needs and
    nothing in front of it, so it may run on a second stream beside whatever the main stream does until then.  The two sides of the wait:
        refresh side   the cell rows (read by the extraction, written by the rotation back), the RAM's private arena, and the
                       refresh stream's own rotation / key-switch scratch
        main side      between write_port and the next read_port a staged engine runs the DFF copies, the gates of the next clock's
                       first stage and its circuit bootstrapping: the engine's arena, its lvl2 store, its TRLWE scratch rows and the
                       selector store
    The two lists share nothing; that is the whole argument.  It is held at the edges by three waits on the device, none on the host:
    the refresh stream waits for the main stream behind the chain (the extraction reads what the chain wrote), and read_port, write_port,
    cells() and free() — every path that reads or overwrites a cell row or the private arena — first make the main stream wait for a
    pending refresh (order_refresh()).  Whoever else touches the cell rows on the main stream (an upload into them) calls
    order_refresh() first.  The words are those of the one-stream form.  Measured on one MI355X: DESIGN.md section 6e."""

    sel_base, own_trgsw, pending_refresh = 0, True, None   # of a RAM with a selector store of its own and its refresh on its own stream
    lanes, sel_stride, arena_stride = 1, None, None

    def __init__(self, stream, cells_trlwe, addr_width, data_width, trgsw=None, sel_base=0, lanes=1, sel_stride=None, arena_stride=None):
        from . import hip

        p = hip.current_params()
        self.stream, self.addr_width, self.data_width, self.N, self.mu = stream, int(addr_width), int(data_width), int(p.N), int(p.mu)
        self.cells_per_plane = C = 1 << self.addr_width
        self.layout = ram_layout(self.addr_width, p.N)
        self.plan = ram_read_plan(self.addr_width, p.N)
        data = np.ascontiguousarray(cells_trlwe, dtype=np.uint32).reshape(-1, 2 * p.N)
        self.lanes, self.sel_stride, self.arena_stride = _lane_setup(lanes, sel_stride, arena_stride, trgsw, sel_base, self.addr_width, "RAM")
        if data.shape[0] not in (self.data_width * C, self.lanes * self.data_width * C):
            raise ValueError(f"expected {self.data_width} x {C} TRLWE rows, got {data.shape[0]}")
        self.ncells = self.data_width * C
        self.plane_scratch = self.layout.scratch_rows + 2
        self.acc0 = self.ncells + self.data_width * self.plane_scratch
        self.sel_base = _selector_store(trgsw, sel_base, self.addr_width)   # refused before anything is allocated
        self.own_trgsw = trgsw is None
        self.pending_refresh = None   # the stream a refresh was sent to that the main stream is not ordered behind yet
        self.row_stride = self.acc0 + self.ncells   # the one-lane store
        self.trlwe = hip.Trlwe(self.lanes * self.row_stride, stream.gpu_index)
        self.trgsw = hip.Trgsw((self.lanes - 1) * self.sel_stride + self.addr_width, stream.gpu_index) if self.own_trgsw else trgsw
        self.arena = hip.Arena(self.lanes * self.ncells, stream.gpu_index)   # lane r: slots [r * ncells, (r + 1) * ncells)
        images = data.reshape(-1, self.ncells, 2 * p.N)
        for lane in range(self.lanes):
            self.upload_lane(lane, images[lane if len(images) > 1 else 0])

    _lanes_kw = Rom._lanes_kw

    def upload_lane(self, lane, cells_trlwe):
        """Lane `lane`'s image: its cell rows, at lane * row_stride, behind a pending refresh.  Asynchronous on the stream."""
        if not 0 <= lane < self.lanes:
            raise ValueError(f"lane {lane} of {self.lanes}")
        data = np.ascontiguousarray(cells_trlwe, dtype=np.uint32).reshape(-1, 2 * self.N)
        if data.shape[0] != self.ncells:
            raise ValueError(f"expected {self.data_width} x {self.cells_per_plane} TRLWE rows, got {data.shape[0]}")
        self.order_refresh()
        self.trlwe.upload(self.stream, lane * self.row_stride, data)

    def row(self, plane, plan_row):
        """Row of the TRLWE store that row `plan_row` of the read plan is for bit plane `plane`."""
        C = self.cells_per_plane
        return plane * C + plan_row if plan_row < C else self.ncells + plane * self.plane_scratch + (plan_row - C)

    def mux_rows(self, plane):
        """The two MUXwoSE rows of a plane; the first one holds the written TRLWE after the add."""
        base = self.ncells + plane * self.plane_scratch + self.layout.scratch_rows
        return base, base + 1

    def read_launches(self):
        """The cmux_batch argument lists (sel, in0, in1, rot, out) of the read tree, all planes' jobs of a level in one launch."""
        out = []
        for jobs in self.plan:
            rows = [(self.sel_base + j.bit, self.row(d, j.in0), self.row(d, j.in1), 0, self.row(d, j.out))
                    for d in range(self.data_width) for j in jobs]
            out.append(tuple(zip(*rows)))
        return out

    def tree_launches(self):
        """The cmux_tree_batch argument lists (sel0, levels, first, out) of the read tree, all planes' jobs of a group of rom_tree_jobs in
        one launch: together they replace read_launches()."""
        out = []
        for jobs, _ in rom_tree_jobs(self.plan):
            rows = [(self.sel_base + j.bit0, j.levels, self.row(d, j.first), self.row(d, j.out)) for d in range(self.data_width) for j in jobs]
            out.append(tuple(zip(*rows)))
        return out

    def write_jobs(self):
        """One ChainJob per cell of every plane, in place on the cell rows, from the plane's written TRLWE."""
        C = self.cells_per_plane
        return [j for d in range(self.data_width) for j in ram_write_jobs(self.addr_width, self.mux_rows(d)[0], d * C, self.sel_base)]

    def clock(self, addr_trgsw, arena, wren_slot, wdata_slots, rdata_slots, fused=True, resident=False, fused_tree=False):
        """One clock of the reference's RAM network, asynchronous on the stream.  addr_trgsw: u32 [addr_width][(k+1) l][k+1][N]
        (client.encrypt_trgsw of the address bits, bit 0 first); arena holds the TLWEs of wren (one slot) and wdata (data_width
        slots) and receives rdata (data_width slots, the addressed word BEFORE the write).  fused=False sends the write-back as
        addr_width cmux_batch launches instead of one cmux_chain_batch: the same words.  resident=True: the addr_width selectors are in
        self.trgsw already (e.g. from selectors_from_tlwe2 on this stream): addr_trgsw is ignored and nothing is uploaded.
        fused_tree=True sends the read tree as one cmux_tree_batch per four levels (read_port): the same words."""
        self._slots(wdata_slots, rdata_slots)   # both refused before anything is uploaded or enqueued
        if not resident:
            sel = np.ascontiguousarray(addr_trgsw, dtype=np.uint32).reshape(self.lanes, self.addr_width, self.trgsw.words)
            for lane in range(self.lanes):   # lanes > 1: addr_trgsw is [lanes][addr_width]..., lane r's selectors at + r * sel_stride
                self.trgsw.upload(self.stream, self.sel_base + lane * self.sel_stride, sel[lane])
        self.read_port(arena, rdata_slots, fused_tree)
        self.write_port(arena, wren_slot, wdata_slots, rdata_slots, fused)

    def _slots(self, *lists):
        out = [np.asarray(s, dtype=np.int32).ravel() for s in lists]
        if any(len(s) != self.data_width for s in out):
            raise ValueError(f"expected {self.data_width} wdata and {self.data_width} rdata slots")
        return out

    def order_refresh(self):
        """Orders the main stream behind a refresh that is pending on another stream (write_port(refresh_stream=...)): one wait on the
        device, nothing on the host.  Nothing pending: nothing enqueued."""
        if self.pending_refresh is not None:
            self.stream.wait_stream(self.pending_refresh)
            self.pending_refresh = None

    def read_port(self, arena, rdata_slots, fused_tree=False):
        """The read half of a clock (steps 1, 2: RAMUX, SEI(0) + key switch -> rdata) with the selectors that are resident in
        self.trgsw.  Inside a netlist rdata feeds the logic that computes wren / wdata of the same clock, so the two halves are
        enqueued apart: read_port, the gates, write_port.  Together they enqueue what clock(resident=True) enqueues.
        fused_tree=True sends the tree as ONE cmux_tree_batch per four levels instead of one cmux_batch per level: the same words."""
        st, w = self.stream, self.data_width
        rdata_slots, = self._slots(rdata_slots)
        self.order_refresh()   # the tree reads the cell rows
        # 1, 2: RAMUX, SEI(0) + key switch -> rdata
        K, kw = self.lanes, self._lanes_kw()
        if fused_tree:
            for args in self.tree_launches():
                st.cmux_tree_batch(self.trgsw, self.trlwe, *args, **kw)
        else:
            for args in self.read_launches():
                st.cmux_batch(self.trgsw, self.trlwe, *args, **kw)
        result = [self.row(d, self.layout.result) for d in range(w)]
        if K == 1:
            st.sample_extract_index_keyswitch_batch(self.trlwe, result, np.zeros(w, dtype=np.int32), rdata_slots, arena)
        else:
            st.sample_extract_index_keyswitch_batch(self.trlwe, lane_flat(result, K, self.row_stride), np.zeros(K * w, dtype=np.int32),
                                                    lane_flat(rdata_slots, K, self.arena_stride), arena)

    def write_port(self, arena, wren_slot, wdata_slots, rdata_slots, fused=True, refresh_stream=None):
        """The write half of a clock (steps 3 - 6: MUXwoSE, the chain of every cell, extraction, refresh) with the same resident
        selectors; rdata_slots still hold what read_port put there.
        refresh_stream: a second hip.Stream of the same GPU.  Steps 3 and 4 stay on self.stream, refresh_stream waits for them on the
        device, steps 5 and 6 go to refresh_stream, and the RAM remembers that its refresh is pending there (the class docstring has the
        buffers of either side).  The same words."""
        st, w = self.stream, self.data_width
        wdata_slots, rdata_slots = self._slots(wdata_slots, rdata_slots)
        if refresh_stream is st:
            raise ValueError("refresh_stream is the RAM's own stream: leave it out")
        self.order_refresh()   # the chain reads and writes the cell rows
        # 3: HomMUXwoSE: BlindRotate(wren + wdata - mu) + BlindRotate(-wren + rdata - mu), + mu at coefficient 0 of b
        K, kw, A, R = self.lanes, self._lanes_kw(), self.arena_stride, self.row_stride
        m1, m0 = zip(*(self.mux_rows(d) for d in range(w)))
        minus_mu = np.full(2 * w, (-self.mu) & 0xFFFFFFFF, dtype=np.uint32)
        if K == 1:
            st.bootstrap_trlwe_batch(arena, [wren_slot] * (2 * w), np.concatenate([wdata_slots, rdata_slots]), [1] * w + [-1] * w,
                                     [1] * (2 * w), minus_mu, self.trlwe.ptr, trlwe_slots=self.trlwe.slots, trlwe_out=m1 + m0)
            st.trlwe_add_batch(self.trlwe, m1, m0, m1, self.mu)
        else:   # the flat arrays of all lanes, lane-major: slots + r * arena_stride, rows + r * row_stride
            st.bootstrap_trlwe_batch(arena, lane_flat([wren_slot] * (2 * w), K, A), lane_flat(np.concatenate([wdata_slots, rdata_slots]), K, A),
                                     lane_tile([1] * w + [-1] * w, K), lane_tile([1] * (2 * w), K), lane_tile(minus_mu, K), self.trlwe.ptr,
                                     trlwe_slots=self.trlwe.slots, trlwe_out=lane_flat(m1 + m0, K, R))
            st.trlwe_add_batch(self.trlwe, lane_flat(m1, K, R), lane_flat(m0, K, R), lane_flat(m1, K, R), self.mu)
        # 4: RAMCMUXs of every cell, in place
        jobs = self.write_jobs()
        if fused:
            st.cmux_chain_batch(self.trgsw, self.trlwe, *zip(*jobs), **kw)
        else:
            steps = [chain_steps(j, self.acc0 + g) for g, j in enumerate(jobs)]
            for s in range(self.addr_width):
                st.cmux_batch(self.trgsw, self.trlwe, *zip(*(c[s] for c in steps)), **kw)
        # 5, 6: SEI(0) + key switch of every cell, then the blind rotation back into the cell's row
        n = K * self.ncells
        cells = np.arange(self.ncells, dtype=np.int32)
        rows = cells if K == 1 else lane_flat(cells, K, R)           # the cell rows of all lanes
        slots = cells if K == 1 else np.arange(n, dtype=np.int32)    # the private arena: lane r in slots r * ncells ..
        if refresh_stream is not None:
            refresh_stream.wait_stream(st)
            st = refresh_stream
            self.pending_refresh = refresh_stream
        st.sample_extract_index_keyswitch_batch(self.trlwe, rows, np.zeros(n, dtype=np.int32), slots, self.arena)
        st.bootstrap_trlwe_batch(self.arena, slots, np.full(n, -1), np.ones(n), np.zeros(n),
                                 np.zeros(n, dtype=np.uint32), self.trlwe.ptr, trlwe_slots=self.trlwe.slots, trlwe_out=rows)

    def cells(self, lane=0):
        """Lane `lane`'s cell rows: u32 [data_width][2^addr_width][2N] (synchronises the stream, behind a pending refresh)."""
        if not 0 <= lane < self.lanes:
            raise ValueError(f"lane {lane} of {self.lanes}")
        self.order_refresh()
        return self.trlwe.download(self.stream, lane * self.row_stride, self.ncells).reshape(self.data_width, self.cells_per_plane, 2 * self.N)

    def free(self):
        self.order_refresh()   # nothing is freed under a refresh that still runs
        self.trlwe.free()
        if self.own_trgsw:
            self.trgsw.free()
        self.arena.free()
