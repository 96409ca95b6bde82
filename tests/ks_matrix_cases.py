"""Chosen cases for the matrix form of the key switch (iyokan_amd/csrc/keyswitch_mfma.hpp) and for the host runtime of its operand
(ensure_ks_matrix in iyokan_amd/csrc/iyokan_hip.hip): keys whose rows carry out of every signed plane, cells with exactly one
non-zero digit at every position of a staging lane, job lists that put a distinctive cell on every accumulator row of every wave,
a gate level with MUX jobs at the edges of every wave, and the thread / stream programs of the runtime tests as data.  Plain arrays
and integers only, no GPU: tests/test_ks_matrix_cases.py checks them on the CPU, tests/test_gpu_keyswitch_matrix.py and
tests/test_gpu_keyswitch_matrix_edges.py run them."""
import numpy as np

import arena_cases as ac
import ks_words as K
from iyokan_amd import client
from iyokan_amd.params import OPS

GATES = 256                 # gates per workgroup of keyswitch_mfma_kernel (dispatch.hpp: KS_MATRIX_GATES)
WAVE_GATES = 64             # gates per wave (KS_MATRIX_WAVE_GATES)
MIN_JOBS = 4608             # the default dispatch takes the form from here on (KS_MATRIX_MIN_JOBS)
EDGE_JOBS = 2 * GATES + 37  # two whole workgroups and a ragged third: a whole wave (64 .. 127 of it never exist) and 37 gates
IB = 16                     # coefficients per digit block of the staging buffer (keyswitch_mfma.hpp: KSM_IB)
SWEEP_BLOCKS = (0, 1, 31, 63)
# bytes of the operand: 4 N t columns x nc 128 words x 4 planes (dispatch.hpp: ks_matrix_bytes)
OPERAND_BYTES = {"128": 73_400_320, "80": 67_108_864}


def nc_of(p):
    """Padded row words / 128: the NC template argument of the key-switch kernels."""
    return (((p.n + 1 + 3) & ~3) + 127) // 128


def operand_bytes(p):
    return 4 * p.N * p.t * nc_of(p) * 128 * 4


# ---- keys ---------------------------------------------------------------------------------------------------------------------------

def carry_keys(keys):
    """The key set with the rows of coefficients 0, 1, 511 and 1023 replaced by words whose four bytes are 0x80 / 0x7F in every
    mix: the signed split carries (or not) out of every plane.  Both kernels get the same key, so they stay comparable."""
    p = keys.params
    ksk = np.array(keys.ksk, dtype=np.uint32).reshape(p.N, p.t, 3, p.n + 1).copy()
    pat = np.array([sum((0x80 if (m >> b) & 1 else 0x7F) << (8 * b) for b in range(4)) for m in range(16)], dtype=np.uint32)
    for i in (0, 1, 511, 1023):
        for j in range(p.t):
            for u in range(3):
                ksk[i, j, u] = pat[(np.arange(p.n + 1) + i + 3 * j + u) % 16]
    return client.KeySet(p, keys.s0, keys.s1, keys.bk, ksk.ravel())


def salted_keys(keys, salt):
    """The key set with every word of the key-switching key XORed with a word stream of `salt`: a key no other test uploads, so an
    operand left in device memory by an earlier initialisation is never the right one.  Outputs no longer decrypt; the oracle made
    from the same KeySet still says what every word is."""
    p = keys.params
    ksk = np.array(keys.ksk, dtype=np.uint32)
    ksk = ksk ^ np.random.default_rng(salt).integers(0, 1 << 32, size=ksk.shape, dtype=np.uint32)
    return client.KeySet(p, keys.s0, keys.s1, keys.bk, ksk)


def ksk_rows(keys):
    """[N][t][3][n + 1]: row (i, j, v - 1) is what digit j of coefficient i subtracts at value v."""
    p = keys.params
    return np.asarray(keys.ksk, dtype=np.uint32).reshape(p.N, p.t, 3, p.n + 1)


# ---- cells --------------------------------------------------------------------------------------------------------------------------

def _t1(a, b, N):
    w = np.empty(N + 1, dtype=np.uint32)
    w[:N] = a
    w[N] = b
    return w


def _low(p, rng):
    return rng.integers(0, 1 << (32 - 2 * p.t), size=p.N, dtype=np.uint64)


def single_digit_t1(p, rng, i, j, v):
    """TLWE1 words whose only non-zero digit is v at coefficient i, level j; random bits below the digit window, random b."""
    D = np.zeros(p.N, dtype=np.int64)
    D[i] = v << (2 * (p.t - 1 - j))
    return _t1(K.words_from_digits(D, _low(p, rng), p.t), rng.integers(0, 1 << 32, dtype=np.uint64), p.N)


NAMED = ("every digit 0", "every digit 3", "a' = 0xFFFFFFFF", "a' = -prec", "digit (0, 0)", "digit (0, t - 1)", "digit (N - 1, 0)",
         "digit (N - 1, t - 1)")


def named_t1(p, rng):
    """The named TLWE1 words (N + 1 each), in the order of NAMED: every digit 0, every digit 3, a' = 0xFFFFFFFF, a' = -prec, one
    non-zero digit at (i, j) in the four corners."""
    N, t = p.N, p.t
    named = []

    def add(a):
        named.append(_t1(a, rng.integers(0, 1 << 32, dtype=np.uint64), N))

    add(K.words_from_digits(np.zeros(N, dtype=np.int64), _low(p, rng), t))
    add(K.words_from_digits(np.full(N, (1 << 2 * t) - 1), _low(p, rng), t))
    add(np.full(N, 0xFFFFFFFF, dtype=np.uint32))
    add(np.full(N, (1 << 32) - K.prec_of(t), dtype=np.uint64).astype(np.uint32))
    for k, (i, j) in enumerate(((0, 0), (0, t - 1), (N - 1, 0), (N - 1, t - 1))):
        D = np.zeros(N, dtype=np.int64)
        D[i] = (1 + k % 3) << (2 * (t - 1 - j))
        add(K.words_from_digits(D, _low(p, rng), t))
    return named


def cells(p, seed, ncells):
    """[ncells][2 N] TRLWE images: first the named cells, then the families of ks_words.chosen_images, then uniform words.
    Returns (cells, number of named cells, number of named + chosen cells, t1[N] of the every-digit-0 cell)."""
    N = p.N
    rng = np.random.default_rng(seed)
    named = named_t1(p, rng)
    imgs, _ = K.chosen_images(p, seed)
    out = np.empty((ncells, 2 * N), dtype=np.uint32)
    for c, w in enumerate(named):
        out[c] = K.image_from_t1(w, rng, N)
    out[len(named):len(named) + len(imgs)] = imgs
    first = len(named) + len(imgs)
    out[first:] = rng.integers(0, 1 << 32, size=(ncells - first, 2 * N), dtype=np.uint32)
    return out, len(named), first, int(named[0][N])


def digit_sweep(p, rng):
    """(images [64 t 3][2 N], digits [64 t 3][3] = (i, j, v)): cells with exactly one non-zero digit, every v in 1 .. 3 at every level
    j < t of coefficient i = 16 blk + c, c = 0 .. 15 (the four coefficient groups of a staging lane and the four positions inside a
    group), blk in SWEEP_BLOCKS.  At t = 7 the 14 digit bits of a coefficient straddle the byte and k-step boundaries of the staging
    buffer, at t = 8 they do not.  The key switch of cell k is (0, .., 0, b') - KSK[i][j][v - 1]."""
    digits = np.array([(IB * blk + c, j, v) for blk in SWEEP_BLOCKS for c in range(IB) for j in range(p.t) for v in (1, 2, 3)], dtype=np.int64)
    imgs = np.stack([K.image_from_t1(single_digit_t1(p, rng, int(i), int(j), int(v)), rng, p.N) for i, j, v in digits])
    return imgs, digits


def single_digit_output(keys, img, i, j, v):
    """What the key switch of a single-digit cell is: (0, .., 0, b') minus one key row."""
    p = keys.params
    out = (np.uint32(0) - ksk_rows(keys)[i, j, v - 1]).astype(np.uint32)
    out[p.n] = np.uint32((int(out[p.n]) + int(img[p.N])) & K.MASK32)
    return out


def position_digit(r, t):
    """(i, j, v) of the distinctive cell of residue r: pairwise different coefficients, every level and every value in turn."""
    return 4 * r + r // 64, r % t, 1 + r % 3


def position_group(r, njobs=EDGE_JOBS):
    """The workgroup whose job r mod 256 holds the distinctive cell: the ragged third takes every third of the residues it has,
    its first and (at EDGE_JOBS) its last job among them."""
    return (r + 2) % 3 if r < njobs - 2 * GATES else r % 2


def position_sweep(p, rng, njobs=EDGE_JOBS):
    """(images [1 + 256][2 N], idx [njobs]): image 0 is an every-digit-0 cell, image 1 + r the single-digit cell position_digit(r).
    Every job is image 0 but one per residue r of the job index mod 256 — one per (wave r // 64, gate tile (r % 64) // 32,
    accumulator row r % 32) —, which sits in workgroup position_group(r): the two whole workgroups and the ragged third all hold
    some."""
    assert 2 * GATES < njobs <= 3 * GATES
    zero = _t1(K.words_from_digits(np.zeros(p.N, dtype=np.int64), _low(p, rng), p.t), rng.integers(0, 1 << 32, dtype=np.uint64), p.N)
    imgs = [K.image_from_t1(zero, rng, p.N)]
    idx = np.zeros(njobs, dtype=np.int32)
    for r in range(GATES):
        imgs.append(K.image_from_t1(single_digit_t1(p, rng, *position_digit(r, p.t)), rng, p.N))
        idx[GATES * position_group(r, njobs) + r] = 1 + r
    return np.stack(imgs), idx


# ---- a gate level ---------------------------------------------------------------------------------------------------------------------

def mux_jobs(njobs=EDGE_JOBS):
    """Key-switch jobs that are MUX gates: the first and the last job of every wave's 64 and the last job of the batch."""
    return sorted({j for w in range(-(-njobs // WAVE_GATES)) for j in (WAVE_GATES * w, WAVE_GATES * w + WAVE_GATES - 1) if j < njobs} | {njobs - 1})


def mux_neighbours(njobs=EDGE_JOBS):
    """The non-MUX jobs beside them, in the same wave."""
    mux = set(mux_jobs(njobs))
    out = set()
    for j in mux:
        for k in (j - 1, j + 1):
            if 0 <= k < njobs and k // WAVE_GATES == j // WAVE_GATES and k not in mux:
                out.add(k)
    return sorted(out)


GATE_EXTRA = ("NOT", "COPY", "CONSTONE", "CONSTZERO", "NOT")


def gate_levels(rng, nin):
    """One gate_batch level {"ops", "in0", "in1", "in2", "out"} of EDGE_JOBS gates with rotations, reading slots 0 .. nin - 1 and
    writing fresh slots from nin on: MUX gates (two rotation rows, off = mu) at mux_jobs(), every binary kind in turn on their
    neighbours and at random elsewhere (a kind's `off` and signs are its own), then GATE_EXTRA.  Gate g < EDGE_JOBS is key-switch
    job g."""
    names = list(rng.choice(list(ac.BINARY), size=EDGE_JOBS))
    for k, j in enumerate(mux_neighbours()):
        names[j] = ac.BINARY[k % len(ac.BINARY)]
    for j in mux_jobs():
        names[j] = "MUX"
    names += list(GATE_EXTRA)
    n = len(names)
    ops = np.array([OPS[k] for k in names], dtype=np.int32)
    in0, in1, in2 = (rng.integers(0, nin, size=n).astype(np.int32) for _ in range(3))
    in1 = np.where(ops <= OPS["MUX"], in1, -1).astype(np.int32)
    in2 = np.where(ops == OPS["MUX"], in2, -1).astype(np.int32)
    in0 = np.where((ops == OPS["CONSTONE"]) | (ops == OPS["CONSTZERO"]), -1, in0).astype(np.int32)
    return {"ops": ops, "in0": in0, "in1": in1, "in2": in2, "out": np.arange(nin, nin + n, dtype=np.int32)}


def oracle_sample():
    """Gates of gate_levels the oracle runs: the MUX jobs, their neighbours and the gates without a rotation (about 40)."""
    return np.array(mux_jobs() + mux_neighbours() + list(range(EDGE_JOBS, EDGE_JOBS + len(GATE_EXTRA))), dtype=np.int64)


# ---- thread and stream programs -----------------------------------------------------------------------------------------------------
# A batch is (trlwe_index [jobs], out_slot [jobs]); a program names which stream runs which batch and in which order, so the serial
# evaluation of the oracle's rows (expected_arena) and the GPU run read the same description.
BATCH_JOBS = 300


def _batches(rng, count, jobs, special, ncells):
    """`count` batches of `jobs` jobs into disjoint, permuted slot ranges of one arena with three free slots between ranges."""
    out = []
    for k in range(count):
        first = k * (jobs + 3)
        out.append((K.job_layout(jobs, special, ncells, rng), (first + rng.permutation(jobs)).astype(np.int32)))
    return out, count * (jobs + 3)


def first_use_program(rng, special, ncells, threads=3):
    """{"slots", "batches", "threads": [[batch, batch]] per host thread}: every thread creates a stream, meets the others at a barrier
    and runs its two batches back to back; it synchronises once, at the end."""
    batches, slots = _batches(rng, 2 * threads, BATCH_JOBS, special, ncells)
    return {"slots": slots, "batches": batches, "threads": [[2 * t, 2 * t + 1] for t in range(threads)]}


# ("create", stream) | ("batch", stream, batch, IYK_HIP_KS_KERNEL) | ("bytes", name) | ("sync",) | ("destroy", stream)
STREAM_STEPS = (
    ("create", "A"), ("create", "B"),
    ("batch", "A", 0, "1"), ("batch", "A", 1, "1"), ("batch", "A", 2, "1"),    # work queued ahead of the build on A's stream
    ("batch", "A", 3, "3"),                                                    # builds the operand behind it
    ("bytes", "first"),
    ("batch", "B", 4, "3"),                                                    # no sync: waits for the build's event
    ("create", "C"), ("batch", "C", 5, "3"),                                   # a stream created after the build
    ("sync",), ("destroy", "A"),
    ("batch", "B", 6, "3"), ("batch", "C", 7, "3"),                            # streams that outlive the builder
    ("sync",), ("bytes", "last"),
)


def stream_program(rng, special, ncells):
    """{"slots", "batches", "steps": STREAM_STEPS}: stream A queues three batches on the wave kernel and then the first batch of the
    matrix form, which builds the operand on A behind them; B follows at once, C is created after the build; A is destroyed; B and C
    run again."""
    nb = 1 + max(s[2] for s in STREAM_STEPS if s[0] == "batch")
    batches, slots = _batches(rng, nb, BATCH_JOBS, special, ncells)
    return {"slots": slots, "batches": batches, "steps": STREAM_STEPS}


def expected_arena(prog, ref, fill):
    """The arena after every batch of `prog`: ref[cell] in every written slot, `fill` everywhere else."""
    want = np.full((prog["slots"], ref.shape[1]), fill, dtype=np.uint32)
    for idx, out_slot in prog["batches"]:
        want[out_slot] = ref[idx]
    return want
