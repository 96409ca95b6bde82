"""The argument sets behind tests/test_batch_args.py (CPU: csrc/batch_args.hpp through libiyk_emul.so) and tests/test_gpu_batch_refusals.py
(the library itself): per batch entry point one set per refusal its source can give, sets where two faults coincide (they pin WHICH is
reported), and a few legal sets with the job words they must make, written out by hand.  What a set must answer — (code, text) — is
recorded from the PARENT commit's library by tools/record_refusals.py into tests/golden/batch_refusals_parent.json.

Everything is tiny: stores of 4 to 16 slots, count <= 4.  An over-cap set states a huge count over arrays of one entry: every entry point
looks at count before it reads an array (a cap that is checked only after the arrays were read has no set here: UNREACHED).  The 128-bit
set throughout (n = 636, k = 1, l = 3, Bgbit = 6, mu = 2^29); a private key-switching key of (n_in, t, basebit) = (2048, 1, 1)."""
import ctypes
import os

import numpy as np

from iyokan_amd.params import OPS, params_128bit

ARENA, TRLWE, TRGSW, TLWE2 = 8, 16, 4, 8      # slots of the real stores behind the legal sets: no legal set states more
N2 = 2048
MU = 1 << 29
NAND, MUX, NOT, ONE, COPY = OPS["NAND"], OPS["MUX"], OPS["NOT"], OPS["CONSTONE"], OPS["COPY"]
OK, INVALID = 0, -1

# refusals of batch_args.hpp no set reaches, and why
UNREACHED = {
    ("gate_batch", "batch too large: more than 2^31 - 1 rotations"): "needs count + MUXes > 2^31 - 1 under the cap of 2^30 gates: 2^30 descriptors read",
}

# entry point -> (function of batch_args.hpp, words per job of every list it builds)
ENTRY = {
    "arena_upload_slots": ("check_slot_list", ()),
    "gate_batch": ("check_gate_batch", (5, 4, 3)),
    "blind_rotate_batch": ("check_rotate_only", (5,)),
    "bootstrap_trlwe_batch": ("check_rotate_only", (5,)),
    "sample_extract_keyswitch_batch": ("check_sample_extract_keyswitch", (4,)),
    "sample_extract_index_keyswitch_batch": ("check_sample_extract_keyswitch", (4,)),
    "cmux_batch": ("check_cmux_batch", (5,)),
    "cmux_chain_batch": ("check_cmux_chain_batch", (6,)),
    "trlwe_add_batch": ("check_trlwe_add_batch", (3,)),
    "privks_batch": ("check_privks_batch", (3,)),
    "trgsw_from_rows": ("check_trgsw_from_rows", ()),
    "cb_rotate_batch": ("check_cb_rotate_batch", (6,)),
    "circuit_bootstrap_batch": ("check_circuit_bootstrap_batch", (6, 3, 1, 1)),
}
CASES = []


def case(entry, name, words=None, **args):
    """words: None for a set that is refused, else the job lists the set must make ([[job, ...], ...], a job a list of words)"""
    assert entry in ENTRY and not any(c["entry"] == entry and c["name"] == name for c in CASES), (entry, name)
    CASES.append({"entry": entry, "name": name, "id": f"{entry}/{name}", "words": words, "args": args})


def mu_words(r):
    """CbJob::mu of digit level r as (lo, hi): 2^(63 - (r + 1) Bgbit)"""
    m = 1 << (63 - (r + 1) * 6)
    return [m & 0xFFFFFFFF, m >> 32]


# ---- slot-list transfers -----------------------------------------------------------------------------------------------------------
E = "arena_upload_slots"
case(E, "legal", words=[], arena_slots=8, count=2, slots=[1, 3])
case(E, "slot == arena_slots", arena_slots=8, count=2, slots=[0, 8])
case(E, "negative slot", arena_slots=8, count=1, slots=[-1])

# ---- gates ---------------------------------------------------------------------------------------------------------------------------
E = "gate_batch"
G = dict(debug=0, arena_slots=8)
case(E, "legal: NAND, MUX, NOT, CONSTONE", **G, count=4, ops=[NAND, MUX, NOT, ONE], in0=[0, 1, 2, -1], in1=[1, 2, -1, -1], in2=[-1, 3, -1, -1],
     out=[4, 5, 6, 7],
     words=[[[0, 1, -1, -1, MU], [3, 2, 1, 1, -MU], [1, 3, 1, -1, -MU]],      # RotJob: NAND; MUX = BR(cs + c1 - mu), BR(c0 - cs - mu)
            [[0, -1, 0, 4], [1, 2, MU, 5]],                                   # KsJob{rot, -1, 0, out}; MUX: {rot, rot + 1, mu, out}
            [[NOT, 2, 6], [ONE, -1, 7]]])                                     # EwJob{op, in, out}
case(E, "legal: XOR and COPY over their own inputs", **G, count=2, ops=[OPS["XOR"], COPY], in0=[0, 1], in1=[2, 77], in2=[-9, -9], out=[0, 1],
     words=[[[0, 2, 2, 2, 2 * MU]], [[0, -1, 0, 0]], [[COPY, 1, 1]]])
case(E, "over cap", **G, count=(1 << 30) + 1, ops=[NAND], in0=[0], in1=[1], in2=[-1], out=[4])
case(E, "over cap and bad slot", **G, count=(1 << 30) + 1, ops=[NAND], in0=[-1], in1=[1], in2=[-1], out=[4])
case(E, "out == arena_slots", **G, count=1, ops=[NAND], in0=[0], in1=[1], in2=[-1], out=[8])
case(E, "bad out and unknown op", **G, count=1, ops=[13], in0=[0], in1=[1], in2=[-1], out=[-1])
case(E, "binary gate without in1", **G, count=1, ops=[NAND], in0=[0], in1=[-1], in2=[-1], out=[4])
case(E, "binary gate, in0 outside", **G, count=1, ops=[OPS["AND"]], in0=[8], in1=[1], in2=[-1], out=[4])
case(E, "MUX without in2", **G, count=1, ops=[MUX], in0=[0], in1=[1], in2=[-1], out=[4])
case(E, "NOT, in0 outside", **G, count=1, ops=[NOT], in0=[9], in1=[-1], in2=[-1], out=[4])
case(E, "unknown op 13", **G, count=1, ops=[13], in0=[0], in1=[1], in2=[-1], out=[4])
case(E, "unknown op -1", **G, count=1, ops=[-1], in0=[0], in1=[1], in2=[-1], out=[4])
case(E, "bad input at gate 0, bad out at gate 1", **G, count=2, ops=[NAND, NAND], in0=[0, 0], in1=[8, 1], in2=[-1, -1], out=[4, 8])
D = dict(debug=1, arena_slots=8)
case(E, "debug, legal: own input overwritten, unread input is another's out", **D, count=2, ops=[NAND, NOT], in0=[0, 2], in1=[1, 0], in2=[-1, 0],
     out=[0, 2], words=[[[0, 1, -1, -1, MU]], [[0, -1, 0, 0]], [[NOT, 2, 2]]])
case(E, "debug: two writers", **D, count=2, ops=[NAND, NAND], in0=[0, 1], in1=[1, 2], in2=[-1, -1], out=[4, 4])
case(E, "debug: read of written", **D, count=2, ops=[NAND, NAND], in0=[0, 4], in1=[1, 2], in2=[-1, -1], out=[4, 5])
case(E, "debug: MUX selector is another's out", **D, count=2, ops=[NAND, MUX], in0=[0, 1], in1=[1, 2], in2=[-1, 4], out=[4, 5])
case(E, "debug: two writers and a read of written", **D, count=3, ops=[NAND, NAND, NAND], in0=[0, 4, 1], in1=[1, 2, 2], in2=[-1, -1, -1], out=[4, 5, 5])
case(E, "debug: two writers and a bad index after them", **D, count=3, ops=[NAND, NAND, NAND], in0=[0, 1, 8], in1=[1, 2, 2], in2=[-1, -1, -1],
     out=[4, 4, 5])

# ---- rotations only ------------------------------------------------------------------------------------------------------------------
E = "blind_rotate_batch"
R = dict(arena_slots=8)
case(E, "legal: one and two inputs", **R, count=2, ia=[0, 7], ib=[1, -1], sa=[1, -2], sb=[-1, 5], off=[MU, 3],
     words=[[[0, 1, 1, -1, MU], [7, -1, -2, 5, 3]]])
case(E, "over cap", **R, count=(1 << 30) + 1, ia=[0], ib=[1], sa=[1], sb=[1], off=[0])
case(E, "over cap and bad slot", **R, count=(1 << 30) + 1, ia=[-1], ib=[1], sa=[1], sb=[1], off=[0])
case(E, "ia outside", **R, count=2, ia=[0, 8], ib=[1, 1], sa=[1, 1], sb=[1, 1], off=[0, 0])
case(E, "ia negative", **R, count=1, ia=[-1], ib=[1], sa=[1], sb=[1], off=[0])
case(E, "ib outside", **R, count=1, ia=[0], ib=[8], sa=[1], sb=[1], off=[0])
E = "bootstrap_trlwe_batch"
case(E, "legal: rows by index", **R, count=2, ia=[0, 1], ib=[-1, 2], sa=[1, 1], sb=[0, 1], off=[0, MU], trlwe_slots=4, trlwe_out=[2, 0],
     words=[[[0, -1, 1, 0, 0], [1, 2, 1, 1, MU]]])
case(E, "legal: rows in order", **R, count=2, ia=[0, 1], ib=[-1, 2], sa=[1, 1], sb=[0, 1], off=[0, MU], trlwe_slots=2, trlwe_out=None,
     words=[[[0, -1, 1, 0, 0], [1, 2, 1, 1, MU]]])
case(E, "output index == trlwe_slots", **R, count=2, ia=[0, 1], ib=[-1, 2], sa=[1, 1], sb=[0, 1], off=[0, 0], trlwe_slots=4, trlwe_out=[0, 4])
case(E, "bad input and bad output index", **R, count=1, ia=[8], ib=[-1], sa=[1], sb=[0], off=[0], trlwe_slots=4, trlwe_out=[4])
case(E, "bad output index at job 0, bad input at job 1", **R, count=2, ia=[0, 8], ib=[-1, -1], sa=[1, 1], sb=[0, 0], off=[0, 0], trlwe_slots=4,
     trlwe_out=[-1, 0])
case(E, "more jobs than rows", **R, count=3, ia=[0, 1, 2], ib=[-1, -1, -1], sa=[1, 1, 1], sb=[0, 0, 0], off=[0, 0, 0], trlwe_slots=2, trlwe_out=None)
case(E, "bad input and more jobs than rows", **R, count=3, ia=[0, 1, 8], ib=[-1, -1, -1], sa=[1, 1, 1], sb=[0, 0, 0], off=[0, 0, 0], trlwe_slots=2,
     trlwe_out=None)

# ---- extraction + key switch -----------------------------------------------------------------------------------------------------------
E = "sample_extract_keyswitch_batch"
S = dict(trlwe_slots=4, arena_slots=8)
case(E, "legal", **S, count=3, trlwe_index=[3, 0, 3], out_slot=[5, 6, 0], words=[[[0, -1, 0, 5], [1, -1, 0, 6], [2, -1, 0, 0]]])
case(E, "over cap", **S, count=(1 << 30) + 1, trlwe_index=[0], out_slot=[0])
case(E, "over cap and bad slot", **S, count=(1 << 30) + 1, trlwe_index=[-1], out_slot=[0])
case(E, "TRLWE index outside", **S, count=2, trlwe_index=[0, 4], out_slot=[0, 1])
case(E, "out slot outside", **S, count=2, trlwe_index=[0, 1], out_slot=[0, 8])
case(E, "both outside", **S, count=1, trlwe_index=[-1], out_slot=[-1])
E = "sample_extract_index_keyswitch_batch"
case(E, "legal", **S, count=2, trlwe_index=[1, 1], coeff_index=[0, 1023], out_slot=[7, 2], words=[[[0, -1, 0, 7], [1, -1, 0, 2]]])
case(E, "over cap", **S, count=(1 << 30) + 1, trlwe_index=[0], coeff_index=[0], out_slot=[0])
case(E, "TRLWE index outside", **S, count=1, trlwe_index=[4], coeff_index=[0], out_slot=[0])
case(E, "coefficient index == N", **S, count=2, trlwe_index=[0, 1], coeff_index=[0, 1024], out_slot=[0, 1])
case(E, "coefficient index negative", **S, count=1, trlwe_index=[0], coeff_index=[-1], out_slot=[0])
case(E, "out slot outside", **S, count=1, trlwe_index=[0], coeff_index=[5], out_slot=[8])
case(E, "bad TRLWE index and bad coefficient index", **S, count=1, trlwe_index=[4], coeff_index=[1024], out_slot=[8])
case(E, "bad coefficient index and bad out slot", **S, count=1, trlwe_index=[0], coeff_index=[1024], out_slot=[8])

# ---- CMUX memories -------------------------------------------------------------------------------------------------------------------
E = "cmux_batch"
M = dict(trgsw_slots=4, trlwe_slots=8)
case(E, "legal: select form, rotate form, own input overwritten", **M, count=3, sel=[0, 3, 1], in0=[0, 2, 5], in1=[1, -1, -7], rot=[77, 2047, 0],
     out=[0, 3, 4], words=[[[0, 0, 1, 0, 0], [3, 2, -1, 2047, 3], [1, 5, -1, 0, 4]]])   # in1 >= 0: rot forced to 0; in1 < 0: -1, rot kept
case(E, "legal: shared inputs", **M, count=2, sel=[2, 2], in0=[0, 0], in1=[1, 1], rot=[0, 0], out=[6, 7],
     words=[[[2, 0, 1, 0, 6], [2, 0, 1, 0, 7]]])
case(E, "over cap", **M, count=(1 << 24) + 1, sel=[0], in0=[0], in1=[1], rot=[0], out=[2])
case(E, "over cap and bad slot", **M, count=(1 << 24) + 1, sel=[-1], in0=[0], in1=[1], rot=[0], out=[2])
case(E, "over cap and store too large", trgsw_slots=(1 << 24) + 1, trlwe_slots=8, count=(1 << 24) + 1, sel=[0], in0=[0], in1=[1], rot=[0], out=[2])
case(E, "selector store too large", trgsw_slots=(1 << 24) + 1, trlwe_slots=8, count=1, sel=[0], in0=[0], in1=[1], rot=[0], out=[2])
case(E, "TRLWE store too large", trgsw_slots=4, trlwe_slots=(1 << 28) + 1, count=1, sel=[0], in0=[0], in1=[1], rot=[0], out=[2])
case(E, "store too large and bad selector", trgsw_slots=4, trlwe_slots=(1 << 28) + 1, count=1, sel=[4], in0=[0], in1=[1], rot=[0], out=[2])
case(E, "selector outside", **M, count=1, sel=[4], in0=[0], in1=[1], rot=[0], out=[2])
case(E, "in0 outside", **M, count=1, sel=[0], in0=[8], in1=[1], rot=[0], out=[2])
case(E, "out outside", **M, count=1, sel=[0], in0=[0], in1=[1], rot=[0], out=[-1])
case(E, "in1 outside", **M, count=1, sel=[0], in0=[0], in1=[8], rot=[0], out=[2])
case(E, "rot == 2N", **M, count=1, sel=[0], in0=[0], in1=[-1], rot=[2048], out=[2])
case(E, "rot negative", **M, count=1, sel=[0], in0=[0], in1=[-1], rot=[-1], out=[2])
case(E, "bad selector and bad row and bad rot", **M, count=1, sel=[-1], in0=[8], in1=[-1], rot=[-1], out=[2])
case(E, "two writers", **M, count=2, sel=[0, 1], in0=[0, 1], in1=[1, 0], rot=[0, 0], out=[2, 2])
case(E, "read of written", **M, count=2, sel=[0, 1], in0=[0, 2], in1=[1, 0], rot=[0, 0], out=[2, 3])
case(E, "in1 read of written", **M, count=2, sel=[0, 1], in0=[0, 0], in1=[3, 1], rot=[0, 0], out=[2, 3])
case(E, "two writers and a read of written", **M, count=3, sel=[0, 1, 2], in0=[0, 2, 1], in1=[1, 0, 0], rot=[0, 0, 0], out=[2, 3, 3])
case(E, "bad index and second writer in one job", **M, count=2, sel=[0, 4], in0=[0, 1], in1=[1, 0], rot=[0, 0], out=[2, 2])
case(E, "second writer at job 1, bad index at job 2", **M, count=3, sel=[0, 1, 4], in0=[0, 1, 0], in1=[1, 0, 1], rot=[0, 0, 0], out=[2, 2, 3])
case(E, "bad index at job 1, second writer at job 2", **M, count=3, sel=[0, 4, 1], in0=[0, 1, 0], in1=[1, 0, 1], rot=[0, 0, 0], out=[2, 3, 2])
case(E, "bad rot at job 2, second writer at job 3", **M, count=4, sel=[0, 1, 2, 3], in0=[0, 0, 0, 0], in1=[1, 1, -1, 1], rot=[0, 0, 2048, 0],
     out=[2, 3, 4, 4])

E = "cmux_chain_batch"
case(E, "legal", **M, count=2, sel0=[1, 0], steps=[2, 4], pattern=[0b10, 0xFFFFFFFF], src=[0, 1], mem=[0, 2], out=[0, 5],
     words=[[[1, 2, 0b10, 0, 0, 0], [0, 4, 0xFFFFFFFF, 1, 2, 5]]])
case(E, "over cap", **M, count=(1 << 24) + 1, sel0=[0], steps=[1], pattern=[0], src=[0], mem=[1], out=[2])
case(E, "over cap and bad slot", **M, count=(1 << 24) + 1, sel0=[-1], steps=[0], pattern=[0], src=[0], mem=[1], out=[2])
case(E, "selector store too large", trgsw_slots=(1 << 24) + 1, trlwe_slots=8, count=1, sel0=[0], steps=[1], pattern=[0], src=[0], mem=[1], out=[2])
case(E, "TRLWE store too large", trgsw_slots=4, trlwe_slots=(1 << 28) + 1, count=1, sel0=[0], steps=[1], pattern=[0], src=[0], mem=[1], out=[2])
case(E, "steps 0", **M, count=1, sel0=[0], steps=[0], pattern=[0], src=[0], mem=[1], out=[2])
case(E, "steps 33", **M, count=1, sel0=[0], steps=[33], pattern=[0], src=[0], mem=[1], out=[2])
case(E, "bad steps and bad sel0", **M, count=1, sel0=[-1], steps=[33], pattern=[0], src=[0], mem=[1], out=[2])
case(E, "sel0 negative", **M, count=1, sel0=[-1], steps=[1], pattern=[0], src=[0], mem=[1], out=[2])
case(E, "sel0 + steps past the store", **M, count=1, sel0=[2], steps=[3], pattern=[0], src=[0], mem=[1], out=[2])
case(E, "bad sel0 and bad row", **M, count=1, sel0=[4], steps=[1], pattern=[0], src=[8], mem=[1], out=[2])
case(E, "src outside", **M, count=1, sel0=[0], steps=[1], pattern=[0], src=[8], mem=[1], out=[2])
case(E, "mem outside", **M, count=1, sel0=[0], steps=[1], pattern=[0], src=[0], mem=[-1], out=[2])
case(E, "out outside", **M, count=1, sel0=[0], steps=[1], pattern=[0], src=[0], mem=[1], out=[8])
case(E, "two writers", **M, count=2, sel0=[0, 1], steps=[1, 1], pattern=[0, 0], src=[0, 1], mem=[1, 0], out=[2, 2])
case(E, "read of written", **M, count=2, sel0=[0, 1], steps=[1, 1], pattern=[0, 0], src=[0, 1], mem=[1, 2], out=[2, 3])
case(E, "two writers, then a bad row", **M, count=3, sel0=[0, 1, 2], steps=[1, 1, 1], pattern=[0, 0, 0], src=[0, 1, 8], mem=[1, 0, 0], out=[2, 2, 3])

E = "trlwe_add_batch"
case(E, "legal: out is a of its own job", trlwe_slots=8, count=2, a=[0, 1], b=[2, 2], out=[0, 7], words=[[[0, 2, 0], [1, 2, 7]]])
case(E, "over cap", trlwe_slots=8, count=(1 << 24) + 1, a=[0], b=[1], out=[2])
case(E, "over cap and bad slot", trlwe_slots=8, count=(1 << 24) + 1, a=[-1], b=[1], out=[2])
case(E, "store too large", trlwe_slots=(1 << 28) + 1, count=1, a=[0], b=[1], out=[2])
case(E, "a outside", trlwe_slots=8, count=1, a=[8], b=[1], out=[2])
case(E, "b outside", trlwe_slots=8, count=1, a=[0], b=[-1], out=[2])
case(E, "out outside", trlwe_slots=8, count=1, a=[0], b=[1], out=[8])
case(E, "two writers", trlwe_slots=8, count=2, a=[0, 1], b=[1, 0], out=[2, 2])
case(E, "read of written", trlwe_slots=8, count=2, a=[0, 1], b=[1, 2], out=[2, 3])
case(E, "two writers, then a bad row", trlwe_slots=8, count=3, a=[0, 1, 8], b=[1, 0, 0], out=[2, 2, 3])

# ---- circuit bootstrapping and its parts ---------------------------------------------------------------------------------------------
E = "privks_batch"
P = dict(tlwe2_slots=8, trlwe_slots=16)
case(E, "legal", **P, count=3, in_=[0, 0, 7], c=[0, 1, 1], out=[2, 0, 15], words=[[[0, 0, 2], [0, 1, 0], [7, 1, 15]]])
case(E, "over cap", **P, count=(1 << 20) + 1, in_=[0], c=[0], out=[0])
case(E, "over cap and bad slot", **P, count=(1 << 20) + 1, in_=[-1], c=[0], out=[0])
case(E, "lvl2 store too large", tlwe2_slots=(1 << 28) + 1, trlwe_slots=16, count=1, in_=[0], c=[0], out=[0])
case(E, "TRLWE store too large", tlwe2_slots=8, trlwe_slots=(1 << 28) + 1, count=1, in_=[0], c=[0], out=[0])
case(E, "in outside", **P, count=1, in_=[8], c=[0], out=[0])
case(E, "c == k + 1", **P, count=1, in_=[0], c=[2], out=[0])
case(E, "c negative", **P, count=1, in_=[0], c=[-1], out=[0])
case(E, "out outside", **P, count=1, in_=[0], c=[0], out=[16])
case(E, "bad in and bad c and bad out", **P, count=1, in_=[-1], c=[2], out=[-1])
case(E, "bad c and bad out", **P, count=1, in_=[0], c=[2], out=[16])
case(E, "two writers", **P, count=2, in_=[0, 1], c=[0, 0], out=[3, 3])
case(E, "bad index and second writer in one job", **P, count=2, in_=[0, 8], c=[0, 0], out=[3, 3])
case(E, "second writer at job 1, bad index at job 2", **P, count=3, in_=[0, 1, 2], c=[0, 0, 2], out=[3, 3, 4])
case(E, "bad index at job 1, second writer at job 2", **P, count=3, in_=[0, 1, 2], c=[0, 2, 0], out=[3, 4, 3])

E = "trgsw_from_rows"
F = dict(trgsw_slots=4, trlwe_slots=16)
case(E, "legal: a run of slots", **F, count=2, out_slot=[2, 3], rows=[0, 1, 2, 3, 4, 5, 6, 7, 8, 9, 10, 11], words=[])
case(E, "legal: two runs, shared rows", **F, count=2, out_slot=[3, 1], rows=[0, 1, 2, 3, 4, 5, 0, 1, 2, 3, 4, 15], words=[])
case(E, "selector store too large", trgsw_slots=(1 << 24) + 1, trlwe_slots=16, count=1, out_slot=[0], rows=[0, 1, 2, 3, 4, 5])
case(E, "TRLWE store too large", trgsw_slots=4, trlwe_slots=(1 << 28) + 1, count=1, out_slot=[0], rows=[0, 1, 2, 3, 4, 5])
case(E, "store too large and more selectors than slots", trgsw_slots=(1 << 24) + 1, trlwe_slots=16, count=(1 << 24) + 2, out_slot=[0],
     rows=[0, 1, 2, 3, 4, 5])
case(E, "more selectors than slots", **F, count=5, out_slot=[0], rows=[0, 1, 2, 3, 4, 5])
case(E, "more selectors than slots and bad slot", **F, count=5, out_slot=[-1], rows=[0, 1, 2, 3, 4, 5])
case(E, "slot outside", **F, count=1, out_slot=[4], rows=[0, 1, 2, 3, 4, 5])
case(E, "row outside", **F, count=1, out_slot=[0], rows=[0, 1, 2, 3, 4, 16])
case(E, "row negative", **F, count=1, out_slot=[0], rows=[-1, 1, 2, 3, 4, 5])
case(E, "two writers", **F, count=2, out_slot=[1, 1], rows=[0, 1, 2, 3, 4, 5, 6, 7, 8, 9, 10, 11])
case(E, "second writer with a bad row", **F, count=2, out_slot=[1, 1], rows=[0, 1, 2, 3, 4, 5, 6, 7, 8, 9, 10, 16])
case(E, "bad row at selector 0, second writer at selector 1", **F, count=2, out_slot=[1, 1], rows=[0, 1, 16, 3, 4, 5, 6, 7, 8, 9, 10, 11])
case(E, "second writer at selector 1, bad slot at selector 2", **F, count=3, out_slot=[1, 1, 4], rows=list(range(16)) + [0, 1])

E = "cb_rotate_batch"
B = dict(tlwe0_slots=8, tlwe2_slots=8)
case(E, "legal", **B, count=3, in_=[0, 0, 7], sign=[1, -1, 1], off=[0, MU, 5], mu=[1 << 57, 1 << 51, 3], out=[1, 0, 7],
     words=[[[0, 1, 0, 1] + mu_words(0), [0, -1, MU, 0] + mu_words(1), [7, 1, 5, 7, 3, 0]]])
case(E, "over cap", **B, count=(1 << 20) + 1, in_=[0], sign=[1], off=[0], mu=[1], out=[0])
case(E, "over cap and bad slot", **B, count=(1 << 20) + 1, in_=[-1], sign=[1], off=[0], mu=[1], out=[0])
case(E, "lvl0 store too large", tlwe0_slots=(1 << 28) + 1, tlwe2_slots=8, count=1, in_=[0], sign=[1], off=[0], mu=[1], out=[0])
case(E, "lvl2 store too large", tlwe0_slots=8, tlwe2_slots=(1 << 28) + 1, count=1, in_=[0], sign=[1], off=[0], mu=[1], out=[0])
case(E, "in outside", **B, count=1, in_=[8], sign=[1], off=[0], mu=[1], out=[0])
case(E, "sign 0", **B, count=1, in_=[0], sign=[0], off=[0], mu=[1], out=[0])
case(E, "sign 2", **B, count=1, in_=[0], sign=[2], off=[0], mu=[1], out=[0])
case(E, "out outside", **B, count=1, in_=[0], sign=[1], off=[0], mu=[1], out=[8])
case(E, "bad in and bad sign and bad out", **B, count=1, in_=[-1], sign=[0], off=[0], mu=[1], out=[-1])
case(E, "bad sign and bad out", **B, count=1, in_=[0], sign=[0], off=[0], mu=[1], out=[-1])
case(E, "two writers", **B, count=2, in_=[0, 1], sign=[1, 1], off=[0, 0], mu=[1, 1], out=[3, 3])
case(E, "bad index and second writer in one job", **B, count=2, in_=[0, 1], sign=[1, 0], off=[0, 0], mu=[1, 1], out=[3, 3])
case(E, "second writer at job 1, bad index at job 2", **B, count=3, in_=[0, 1, 8], sign=[1, 1, 1], off=[0, 0, 0], mu=[1, 1, 1], out=[3, 3, 4])
case(E, "bad index at job 1, second writer at job 2", **B, count=3, in_=[0, 8, 1], sign=[1, 1, 1], off=[0, 0, 0], mu=[1, 1, 1], out=[3, 4, 3])

E = "circuit_bootstrap_batch"
# bk2 / pk name the key handed over: "ok" = (n = 636) / (n_in = 2048), "other" = (n = 2) / (n_in = 64)
CB = dict(bk2="ok", pk="ok", tlwe0_slots=8, tlwe2_n_in=N2, tlwe2_slots=8, tlwe2_first=1, trlwe_slots=16, trgsw_slots=4, trgsw_first=1)
case(E, "legal: two bits", **CB, bits=2, in_=[1, 0], sign=[1, -1],
     words=[[[1, 1, 0, 1 + r] + mu_words(r) for r in range(3)] + [[0, -1, 0, 4 + r] + mu_words(r) for r in range(3)],   # lvl2 slot first + bit l + r
            [[1 + b * 3 + r, c, b * 6 + c * 3 + r] for b in range(2) for c in range(2) for r in range(3)],             # scratch row (bit (k+1) + c) l + r
            [[row] for row in range(12)], [[1], [2]]])
case(E, "legal: one bit into the last slots", **{**CB, "tlwe2_first": 5, "trgsw_first": 3, "trlwe_slots": 6}, bits=1, in_=[7], sign=[-1],
     words=[[[7, -1, 0, 5 + r] + mu_words(r) for r in range(3)], [[5 + r, c, c * 3 + r] for c in range(2) for r in range(3)],
            [[row] for row in range(6)], [[3]]])
case(E, "over cap", **CB, bits=(1 << 20) // 6 + 1, in_=[0], sign=[1])
case(E, "over cap and bad slot", **CB, bits=(1 << 20) // 6 + 1, in_=[-1], sign=[0])
case(E, "lvl0 store too large", **{**CB, "tlwe0_slots": (1 << 28) + 1}, bits=1, in_=[0], sign=[1])
case(E, "lvl2 store too large", **{**CB, "tlwe2_slots": (1 << 28) + 1}, bits=1, in_=[0], sign=[1])
case(E, "TRLWE store too large", **{**CB, "trlwe_slots": (1 << 28) + 1}, bits=1, in_=[0], sign=[1])
case(E, "selector store too large", **{**CB, "trgsw_slots": (1 << 24) + 1}, bits=1, in_=[0], sign=[1])
case(E, "store too large and wrong n_in", **{**CB, "trgsw_slots": (1 << 24) + 1, "tlwe2_n_in": 64}, bits=1, in_=[0], sign=[1])
case(E, "bootstrapping key of another n", **{**CB, "bk2": "other"}, bits=1, in_=[0], sign=[1])
case(E, "bootstrapping key of another n and wrong n_in", **{**CB, "bk2": "other", "tlwe2_n_in": 64}, bits=1, in_=[0], sign=[1])
case(E, "lvl2 store of n_in 64", **{**CB, "tlwe2_n_in": 64}, bits=1, in_=[0], sign=[1])
case(E, "lvl2 store and key of n_in 64", **{**CB, "tlwe2_n_in": 64, "pk": "other"}, bits=1, in_=[0], sign=[1])
case(E, "key of n_in 64", **{**CB, "pk": "other"}, bits=1, in_=[0], sign=[1])
case(E, "wrong n_in and bad in", **{**CB, "pk": "other"}, bits=1, in_=[8], sign=[1])
case(E, "lvl2 first past the store", **{**CB, "tlwe2_first": 9}, bits=1, in_=[0], sign=[1])
case(E, "lvl2 slots do not fit", **{**CB, "tlwe2_first": 3}, bits=2, in_=[0, 1], sign=[1, 1])
case(E, "lvl2 slots do not fit and scratch too small", **{**CB, "tlwe2_first": 3, "trlwe_slots": 11}, bits=2, in_=[0, 1], sign=[1, 1])
case(E, "scratch too small", **{**CB, "trlwe_slots": 11}, bits=2, in_=[0, 1], sign=[1, 1])
case(E, "scratch too small and selector slots outside", **{**CB, "trlwe_slots": 11, "trgsw_first": 3}, bits=2, in_=[0, 1], sign=[1, 1])
case(E, "selector first past the store", **{**CB, "trgsw_first": 5}, bits=1, in_=[0], sign=[1])
case(E, "selector slots do not fit", **{**CB, "trgsw_first": 3}, bits=2, in_=[0, 1], sign=[1, 1])
case(E, "selector slots do not fit and bad in", **{**CB, "trgsw_first": 3}, bits=2, in_=[8, 1], sign=[1, 1])
case(E, "in outside", **CB, bits=2, in_=[0, 8], sign=[1, 1])
case(E, "sign 0", **CB, bits=2, in_=[0, 1], sign=[1, 0])
case(E, "bad sign at bit 0, bad in at bit 1", **CB, bits=2, in_=[0, 8], sign=[0, 1])
case(E, "bad in and bad sign in one bit", **CB, bits=1, in_=[-1], sign=[0])


# ---- running a set -------------------------------------------------------------------------------------------------------------------

_i32p, _u32p, _u64p = ctypes.POINTER(ctypes.c_int32), ctypes.POINTER(ctypes.c_uint32), ctypes.POINTER(ctypes.c_uint64)
u64 = ctypes.c_uint64


def _arr(v, dtype=np.int32):
    """(array kept alive, pointer): None stays a null pointer; uint32 lists may hold values >= 2^31"""
    if v is None:
        return None, None
    a = np.ascontiguousarray(np.asarray(v, dtype=np.int64).astype(dtype) if dtype == np.int32 else np.asarray(v, dtype=dtype))
    return a, a.ctypes.data_as({np.int32: _i32p, np.uint32: _u32p, np.uint64: _u64p}[dtype])


def expected_words(c):
    """the hand-written job lists of a legal set as one flat uint32 array, and the jobs per list"""
    flat = [w & 0xFFFFFFFF for jobs in c["words"] for job in jobs for w in job]
    return np.array(flat, dtype=np.uint32), [len(jobs) for jobs in c["words"]]


_EMUL = None


def emul():
    global _EMUL
    if _EMUL is None:
        root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
        _EMUL = ctypes.CDLL(os.path.join(root, "iyokan_amd", "lib", "libiyk_emul.so"))
    return _EMUL


def call_emul(c):
    """(code, text, words, jobs per list) of iyk_emul_check_* on the set"""
    a, L, p = c["args"], emul(), params_128bit()
    fn, per_job = ENTRY[c["entry"]]
    keep, P = [], lambda v, dt=np.int32: (keep.append(_arr(v, dt)), keep[-1][1])[1]
    msg = ctypes.create_string_buffer(256)
    words = np.zeros(256, dtype=np.uint32)
    counts = (u64 * 4)()
    tail = [msg, u64(256), words.ctypes.data_as(_u32p), u64(words.size), counts]
    e = c["entry"]
    if e == "arena_upload_slots":
        head = [u64(a["count"]), P(a["slots"]), u64(a["arena_slots"])]
    elif e == "gate_batch":
        head = [ctypes.byref(p), a["debug"], u64(a["arena_slots"]), u64(a["count"])] + [P(a[k]) for k in ("ops", "in0", "in1", "in2", "out")]
    elif e in ("blind_rotate_batch", "bootstrap_trlwe_batch"):
        head = [u64(a["arena_slots"]), u64(a["count"])] + [P(a[k]) for k in ("ia", "ib", "sa", "sb")] + [P(a["off"], np.uint32)]
        head += [u64(a.get("trlwe_slots", 0)), P(a.get("trlwe_out"))]
    elif e in ("sample_extract_keyswitch_batch", "sample_extract_index_keyswitch_batch"):
        head = [u64(a["trlwe_slots"]), u64(a["arena_slots"]), u64(a["count"]), P(a["trlwe_index"]), P(a.get("coeff_index")), P(a["out_slot"])]
    elif e == "cmux_batch":
        head = [u64(a["trgsw_slots"]), u64(a["trlwe_slots"]), u64(a["count"])] + [P(a[k]) for k in ("sel", "in0", "in1", "rot", "out")]
    elif e == "cmux_chain_batch":
        head = [u64(a["trgsw_slots"]), u64(a["trlwe_slots"]), u64(a["count"]), P(a["sel0"]), P(a["steps"]), P(a["pattern"], np.uint32)]
        head += [P(a[k]) for k in ("src", "mem", "out")]
    elif e == "trlwe_add_batch":
        head = [u64(a["trlwe_slots"]), u64(a["count"])] + [P(a[k]) for k in ("a", "b", "out")]
    elif e == "privks_batch":
        head = [ctypes.c_uint32(p.k), u64(a["tlwe2_slots"]), u64(a["trlwe_slots"]), u64(a["count"])] + [P(a[k]) for k in ("in_", "c", "out")]
    elif e == "trgsw_from_rows":
        head = [ctypes.byref(p), u64(a["trgsw_slots"]), u64(a["trlwe_slots"]), u64(a["count"]), P(a["out_slot"]), P(a["rows"])]
    elif e == "cb_rotate_batch":
        head = [u64(a["tlwe0_slots"]), u64(a["tlwe2_slots"]), u64(a["count"]), P(a["in_"]), P(a["sign"]), P(a["off"], np.uint32), P(a["mu"], np.uint64),
                P(a["out"])]
    else:
        head = [ctypes.byref(p), ctypes.c_uint32(p.n if a["bk2"] == "ok" else 2), ctypes.c_uint32(N2 if a["pk"] == "ok" else 64), u64(a["tlwe0_slots"]),
                P(a["in_"]), P(a["sign"]), ctypes.c_uint32(a["tlwe2_n_in"]), u64(a["tlwe2_slots"]), u64(a["tlwe2_first"]), u64(a["trlwe_slots"]),
                u64(a["trgsw_slots"]), u64(a["trgsw_first"]), u64(a["bits"])]
    f = getattr(L, "iyk_emul_" + fn)
    f.restype = ctypes.c_int
    code = f(*head, *tail)
    n = [int(counts[i]) for i in range(len(per_job))]
    return code, msg.value.decode(), words[: sum(k * w for k, w in zip(n, per_job))].copy(), n


class Stores:
    """The real stores and keys behind the sets, on GPU 0 of an initialised library (128-bit set), zero-filled: what a legal set launches
    on.  A refused set never touches them."""

    def __init__(self, hip):
        p = hip.current_params()
        self.hip, self.st = hip, hip.Stream(0)
        self.arena, self.trlwe, self.trgsw, self.tlwe2 = hip.Arena(ARENA), hip.Trlwe(TRLWE), hip.Trgsw(TRGSW), hip.Tlwe2(N2, TLWE2)
        self.st.upload(self.arena, 0, np.zeros((ARENA, p.n + 1), dtype=np.uint32))
        self.trlwe.upload(self.st, 0, np.zeros((TRLWE, 2 * p.N), dtype=np.uint32))
        self.trgsw.upload(self.st, 0, np.zeros((TRGSW, (p.k + 1) * p.l * (p.k + 1) * p.N), dtype=np.uint32))
        self.tlwe2.upload(self.st, 0, np.zeros((TLWE2, N2 + 1), dtype=np.uint64))
        self.bk2 = {"ok": hip.Bk2Key(p.n), "other": hip.Bk2Key(2)}
        self.pk = {"ok": hip.PrivKsKey(N2, 1, 1), "other": hip.PrivKsKey(64, 1, 1)}
        for key in self.bk2.values():                                     # the first upload sends the transform's tables
            key.upload(self.st, 0, np.zeros((1, key.step_words), dtype=np.uint64))
        self.st.sync()

    def free(self):
        self.st.sync()
        for o in [self.arena, self.trlwe, self.trgsw, self.tlwe2, *self.bk2.values(), *self.pk.values()]:
            o.free()
        self.st.destroy()

    def call(self, c):
        """(code, text of iyk_hip_last_error — "" when accepted) of the entry point on the set"""
        a, L, S = c["args"], self.hip.lib(), self
        vp = ctypes.c_void_p
        keep, P = [], lambda v, dt=np.int32: (keep.append(_arr(v, dt)), keep[-1][1])[1]
        if c["words"] is not None:   # a legal set launches: it must fit the real stores
            assert all(a.get(k, 0) <= cap for k, cap in (("arena_slots", ARENA), ("trlwe_slots", TRLWE), ("trgsw_slots", TRGSW), ("tlwe2_slots", TLWE2),
                                                         ("tlwe0_slots", ARENA), ("count", 4), ("bits", 2))), c["id"]
        st, arena, trlwe, trgsw, tlwe2 = S.st.h, vp(S.arena.ptr), vp(S.trlwe.ptr), vp(S.trgsw.ptr), vp(S.tlwe2.ptr)
        e = c["entry"]
        if e == "arena_upload_slots":
            host = np.zeros((min(a["count"], 4), S.hip.current_params().n + 1), dtype=np.uint32)
            rc = L.iyk_hip_arena_upload_slots(st, arena, a["arena_slots"], a["count"], P(a["slots"]), host.ctypes.data_as(_u32p))
        elif e == "gate_batch":
            rc = L.iyk_hip_gate_batch(st, arena, a["arena_slots"], a["count"], *[P(a[k]) for k in ("ops", "in0", "in1", "in2", "out")])
        elif e == "blind_rotate_batch":   # the TRLWE store stands in for the rows of N + 1 words
            rc = L.iyk_hip_blind_rotate_batch(st, arena, a["arena_slots"], a["count"], *[P(a[k]) for k in ("ia", "ib", "sa", "sb")],
                                              P(a["off"], np.uint32), trlwe)
        elif e == "bootstrap_trlwe_batch":
            rc = L.iyk_hip_bootstrap_trlwe_batch(st, arena, a["arena_slots"], a["count"], *[P(a[k]) for k in ("ia", "ib", "sa", "sb")],
                                                 P(a["off"], np.uint32), trlwe, a["trlwe_slots"], P(a["trlwe_out"]))
        elif e == "sample_extract_keyswitch_batch":
            rc = L.iyk_hip_sample_extract_keyswitch_batch(st, trlwe, a["trlwe_slots"], a["count"], P(a["trlwe_index"]), P(a["out_slot"]), arena,
                                                          a["arena_slots"])
        elif e == "sample_extract_index_keyswitch_batch":
            rc = L.iyk_hip_sample_extract_index_keyswitch_batch(st, trlwe, a["trlwe_slots"], a["count"], P(a["trlwe_index"]), P(a["coeff_index"]),
                                                                P(a["out_slot"]), arena, a["arena_slots"])
        elif e == "cmux_batch":
            rc = L.iyk_hip_cmux_batch(st, trgsw, a["trgsw_slots"], trlwe, a["trlwe_slots"], a["count"],
                                      *[P(a[k]) for k in ("sel", "in0", "in1", "rot", "out")])
        elif e == "cmux_chain_batch":
            rc = L.iyk_hip_cmux_chain_batch(st, trgsw, a["trgsw_slots"], trlwe, a["trlwe_slots"], a["count"], P(a["sel0"]), P(a["steps"]),
                                            P(a["pattern"], np.uint32), *[P(a[k]) for k in ("src", "mem", "out")])
        elif e == "trlwe_add_batch":
            rc = L.iyk_hip_trlwe_add_batch(st, trlwe, a["trlwe_slots"], a["count"], *[P(a[k]) for k in ("a", "b", "out")], 0)
        elif e == "privks_batch":
            rc = L.iyk_hip_privks_batch(st, S.pk["ok"].h, tlwe2, a["tlwe2_slots"], a["count"], P(a["in_"]), P(a["c"]), trlwe, a["trlwe_slots"],
                                        P(a["out"]))
        elif e == "trgsw_from_rows":
            rc = L.iyk_hip_trgsw_from_rows(st, trgsw, a["trgsw_slots"], a["count"], P(a["out_slot"]), trlwe, a["trlwe_slots"], P(a["rows"]))
        elif e == "cb_rotate_batch":
            rc = L.iyk_hip_cb_rotate_batch(st, S.bk2["ok"].h, arena, a["tlwe0_slots"], a["count"], P(a["in_"]), P(a["sign"]), P(a["off"], np.uint32),
                                           P(a["mu"], np.uint64), tlwe2, a["tlwe2_slots"], P(a["out"]))
        else:
            rc = L.iyk_hip_circuit_bootstrap_batch(st, S.bk2[a["bk2"]].h, S.pk[a["pk"]].h, arena, a["tlwe0_slots"], P(a["in_"]), P(a["sign"]), tlwe2,
                                                   a["tlwe2_n_in"], a["tlwe2_slots"], a["tlwe2_first"], trlwe, a["trlwe_slots"], trgsw,
                                                   a["trgsw_slots"], a["trgsw_first"], a["bits"])
        return int(rc), (L.iyk_hip_last_error().decode() if rc else "")
