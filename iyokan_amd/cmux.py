"""CMUX memories on the GPU: the read tree of a ROM over TRLWE rows (Stream.cmux_batch + index extraction).

Replaces the reference's TaskTFHEppROMUX (UROMUX + LROMUX, /root/reference/src/iyokan_tfhepp.hpp:238-300) followed by one
TaskTFHEppSEI per output bit (:340-352).

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


class Rom:
    """A ROM of TRLWE rows on one GPU.  read() runs rom_read_plan for R independent reads at once: the jobs of all reads at one
    level go into ONE cmux_batch, each read with its own scratch rows and its own addr_width selectors; then bit i of every read's
    word is extracted at coefficient index i and key-switched into an arena slot."""

    def __init__(self, stream, data_trlwe, addr_width, log2_word_bits, max_reads=1):
        from . import hip

        p = hip.current_params()
        self.stream, self.addr_width, self.N = stream, int(addr_width), int(p.N)
        self.word_bits = 1 << log2_word_bits
        self.layout = rom_layout(addr_width, log2_word_bits, p.N)
        self.plan = rom_read_plan(addr_width, log2_word_bits, p.N)
        if not self.plan:
            raise ValueError("a ROM of one word has no read tree")
        data = np.ascontiguousarray(data_trlwe, dtype=np.uint32).reshape(-1, 2 * p.N)
        if data.shape[0] != self.layout.data_rows:
            raise ValueError(f"expected {self.layout.data_rows} TRLWE rows, got {data.shape[0]}")
        self.max_reads = int(max_reads)
        self.trlwe = hip.Trlwe(self.layout.data_rows + self.max_reads * self.layout.scratch_rows, stream.gpu_index)
        self.trgsw = hip.Trgsw(self.max_reads * self.addr_width, stream.gpu_index)
        self.trlwe.upload(stream, 0, data)

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
                    vals = (r * self.addr_width + j.bit, self.row(r, j.in0), -1 if j.in1 < 0 else self.row(r, j.in1), j.rot,
                            self.row(r, j.out))
                    for c, v in zip(cols, vals):
                        c.append(v)
            out.append(tuple(cols))
        return out

    def read(self, addr_trgsw, arena, out_slots):
        """addr_trgsw: u32 [R][addr_width][(k+1) l][k+1][N] (client.encrypt_trgsw of every read's address bits, bit 0 first);
        out_slots: [R][word_bits] arena slots.  Asynchronous on the stream."""
        sel = np.ascontiguousarray(addr_trgsw, dtype=np.uint32).reshape(-1, self.addr_width, self.trgsw.words)
        reads = sel.shape[0]
        out_slots = np.asarray(out_slots, dtype=np.int32).reshape(reads, self.word_bits)
        if reads > self.max_reads:
            raise ValueError(f"{reads} reads, sized for {self.max_reads}")
        self.trgsw.upload(self.stream, 0, sel)
        for args in self.launches(reads):
            self.stream.cmux_batch(self.trgsw, self.trlwe, *args)
        rows = np.repeat([self.row(r, self.layout.result) for r in range(reads)], self.word_bits)
        coeff = np.tile(np.arange(self.word_bits), reads)
        self.stream.sample_extract_index_keyswitch_batch(self.trlwe, rows, coeff, out_slots.ravel(), arena)

    def free(self):
        self.trlwe.free()
        self.trgsw.free()
