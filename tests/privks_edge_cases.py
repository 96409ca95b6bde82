"""Chosen cases of the private key switch (test support for test_privks_cases / test_gpu_privks_edges / privks_edges_child), the role
tests/cmux_cases.py plays for the CMUX kernels: TLWE stores, job lists and expected rows, deterministically from seeds.  No GPU and no
handle of the HIP library: the expected rows come from tests/privks_ref.py alone.  The only library code used is the emulation library's
iyk_emul_privks_plan (dispatch.hpp's split of a launch, to FIND a batch size of a wanted character) and iyk_emul_privks_digits (checked
against the restatement's digits by the CPU test, never used to build an expectation).

A job is (in, c, out).  Every case is a dict; the CPU test (tests/test_privks_cases.py) proves what the case claims about itself."""
import ctypes
import os

import numpy as np

import privks_ref as ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
WORDS = 2048                       # 2N words of a TRLWE row
FILL = np.uint32(0xA5A5A5A5)       # what a TRLWE store holds before a case runs
ROW_BYTES = WORDS * 4
WG_PER_CU = 4                      # dispatch.hpp: PRIVKS_WG_PER_CU, restated for the `asked` figure of a plan only
UNROLL = 5                         # privks.hpp: PRIVKS_UNROLL, restated to place a digit at the start of the last round

_emul = []


def emul():
    if not _emul:
        em = ctypes.CDLL(os.path.join(ROOT, "iyokan_amd", "lib", "libiyk_emul.so"))
        em.iyk_emul_privks_plan.argtypes = [ctypes.c_int] * 3 + [ctypes.POINTER(ctypes.c_int)]
        em.iyk_emul_privks_plan.restype = None
        em.iyk_emul_privks_digits.argtypes = [ctypes.POINTER(ctypes.c_uint64), ctypes.c_int, ctypes.c_uint32, ctypes.c_uint32,
                                              ctypes.POINTER(ctypes.c_uint32)]
        em.iyk_emul_privks_digits.restype = None
        _emul.append(em)
    return _emul[0]


def plan(njobs, n_words, cus):
    """(splits, i_per_split) of dispatch.hpp: privks_plan."""
    out = (ctypes.c_int * 2)()
    emul().iyk_emul_privks_plan(int(njobs), int(n_words), int(cus), out)
    return out[0], out[1]


def emul_digits(words, t, basebit):
    words = np.ascontiguousarray(words, dtype=np.uint64).ravel()
    got = np.zeros((words.size, t), dtype=np.uint32)
    emul().iyk_emul_privks_digits(words.ctypes.data_as(ctypes.POINTER(ctypes.c_uint64)), words.size, t, basebit,
                                  got.ctypes.data_as(ctypes.POINTER(ctypes.c_uint32)))
    return got


def uniform_rows(seed, rows, words=WORDS):
    return np.random.default_rng(seed).integers(0, 1 << 32, size=(rows, words), dtype=np.uint32)


def formula_rows(idx, words=WORDS):
    """A cheap wrap-around function of (row index, word index): v = row A + x B, v v + row A  (mod 2^32), the rows of a key that is
    never held whole."""
    ra = (np.asarray(idx, dtype=np.uint64) * np.uint64(0x9E3779B1)).astype(np.uint32)
    xb = (np.arange(words, dtype=np.uint64) * np.uint64(0x85EBCA77)).astype(np.uint32)
    v = np.add.outer(ra, xb)
    np.multiply(v, v, out=v)
    v += ra[:, None]
    return v


def key_rows(n_in, t, basebit):
    return 2 * (n_in + 1) * t * ((1 << basebit) - 1)


def word_of_digits(d, basebit, low=0):
    """The 64-bit word whose rounded digits are d (most significant first); `low` fills the bits under the rounding constant."""
    t = len(d)
    h = 1 << (63 - basebit * t)
    assert 0 <= low < h or low == 0
    w = low
    for j, dj in enumerate(d):
        assert 0 <= dj < 1 << basebit
        w |= int(dj) << (64 - (j + 1) * basebit)
    return w


def expected_rows(tlwe2, pairs, t, basebit, row_fn):
    """{(in, c): the 2N words privks_ref.switch gives}, each distinct pair once."""
    return {(i, c): ref.switch(tlwe2[i], c, t, basebit, row_fn) for i, c in sorted(set(pairs))}


def run_jobs(T, jobs, rows_of):
    """The jobs in place on the TRLWE rows T, from the rows of expected_rows: what privks_ref.run_jobs does, each (in, c) summed once."""
    for i, c, out in jobs:
        T[out] = rows_of[(i, c)]
    return T


# ---- 1. launch plans ------------------------------------------------------------------------------------------------------------------

PLAN_N_IN, PLAN_T, PLAN_BB = 12, 10, 3
PLAN_WORDS = PLAN_N_IN + 1
PLAN_TLWES = 64
PLAN_EXTRA_ROWS = 3               # rows of the TRLWE store no job writes


def _asked(count, cus):
    want = WG_PER_CU * max(1, cus)
    return min(max(-(-want // count), 1), PLAN_WORDS)


def _last(splits, per):
    return PLAN_WORDS - (splits - 1) * per


# character -> predicate on (count, cus, splits, per); the figures in the comments are the plans at 256 CUs
CHARACTERS = {
    "one split": lambda n, cus, s, per: s == 1,                                                         # 1024: per = 13
    "two splits, uneven": lambda n, cus, s, per: s == 2 and _last(s, per) < per,                        # 1023: 7 + 6
    "three splits, short tail": lambda n, cus, s, per: s == 3 and 1 < _last(s, per) < per,              # 342: 5 + 5 + 3
    "last split of one word": lambda n, cus, s, per: per > 1 and _last(s, per) == 1 and s == _asked(n, cus),   # 205: per = 3, 5 splits
    "fewer splits than asked": lambda n, cus, s, per: s < _asked(n, cus) and _last(s, per) == 1,        # 100: asks 11, gets 7 of 2
    "finest cut": lambda n, cus, s, per: per == 1 and s == PLAN_WORDS,                                  # 1: 13 splits of 1
}
AT_256_CUS = {"one split": 1024, "two splits, uneven": 1023, "three splits, short tail": 342, "last split of one word": 205,
              "fewer splits than asked": 100, "finest cut": 1}
PLANS_AT_256_CUS = {"one split": (1, 13), "two splits, uneven": (2, 7), "three splits, short tail": (3, 5),
                    "last split of one word": (5, 3), "fewer splits than asked": (7, 2), "finest cut": (13, 1)}


def find_count(character, cus):
    """The batch size at which a device of `cus` CUs gets a plan of this character, or None if it has none: the hand-derived size of
    AT_256_CUS where it fits, else the smallest."""
    ok = CHARACTERS[character]
    for count in [AT_256_CUS[character]] + list(range(1, WG_PER_CU * max(1, cus) + 2)):
        s, per = plan(count, PLAN_WORDS, cus)
        if ok(count, cus, s, per):
            return count
    return None


_plan_store = []


def plan_store():
    """(tlwe2 u64 [64][13], K u32 [1820][2N]): uniform TLWEs, from slot 40 on every edge word of privks_ref.edge_words at i = 0,
    i = n_in - 1 and i = n_in of a uniform TLWE; slot 39 all zeros (no row at all).  Read-only."""
    if not _plan_store:
        tl = np.random.default_rng(1201).integers(0, 1 << 64, size=(PLAN_TLWES, PLAN_WORDS), dtype=np.uint64)
        s = 40
        for w, _ in ref.edge_words(PLAN_T, PLAN_BB).values():
            for pos in (0, PLAN_N_IN - 1, PLAN_N_IN):
                tl[s, pos] = np.uint64(w)
                s += 1
        tl[39] = 0
        K = uniform_rows(1202, key_rows(PLAN_N_IN, PLAN_T, PLAN_BB))
        tl.setflags(write=False)
        K.setflags(write=False)
        _plan_store.append((tl, K))
    return _plan_store[0]


def rows_per_split(tlwe, splits, per, t=PLAN_T, basebit=PLAN_BB):
    """How many key rows each split of a plan reads for one TLWE: int [splits]."""
    nz = (ref.digits(tlwe, t, basebit) != 0).sum(axis=1)
    return np.array([nz[s * per : (s + 1) * per].sum() for s in range(splits)])


_plan_cases = {}


def plan_case(character, cus):
    """The case of one character at `cus` CUs, or None.  `count` jobs in one batch (two batches of one job where count is 1): `in` drawn
    with repeats from the TLWEs that select a row in EVERY split of the plan (the edge TLWEs among them where the plan allows), c
    alternating, `out` a permutation of the store's rows that has row 0 and the last row and leaves PLAN_EXTRA_ROWS rows alone.
    dict(count, splits, per, tlwe2, K, T, batches, want)."""
    if (character, cus) in _plan_cases:
        return _plan_cases[(character, cus)]
    count = find_count(character, cus)
    case = None
    if count is not None:
        tl, K = plan_store()
        splits, per = plan(count, PLAN_WORDS, cus)
        eligible = [g for g in range(PLAN_TLWES) if rows_per_split(tl[g], splits, per).min() > 0]
        rng = np.random.default_rng([1203, count, cus])
        rows = count + PLAN_EXTRA_ROWS
        if count == 1:   # one job cannot write both ends of the store: two batches of one job
            batches = [[(eligible[-1], 1, rows - 1)], [(eligible[0], 0, 0)]]
        else:
            in_ = rng.choice(eligible, size=count)            # with repeats
            in_[: min(count, len(eligible))] = eligible[::-1][:count]   # and every eligible TLWE at least once where they fit, the edge ones first
            inner = rng.permutation(np.arange(1, rows - 1))[: count - 2]
            out = rng.permutation(np.concatenate([[0, rows - 1], inner]))
            batches = [[(int(in_[g]), (g + 1) & 1, int(out[g])) for g in range(count)]]
        T = np.full((rows, WORDS), FILL, dtype=np.uint32)
        jobs = [j for b in batches for j in b]
        rows_of = expected_rows(tl, [j[:2] for j in jobs], PLAN_T, PLAN_BB, ref.key_rows_of(K))
        want = run_jobs(T.copy(), jobs, rows_of)
        case = dict(count=count, splits=splits, per=per, tlwe2=tl, K=K, T=T, batches=batches, want=want, rows_of=rows_of)
    _plan_cases[(character, cus)] = case
    return case


# ---- 2. digit shapes ------------------------------------------------------------------------------------------------------------------

DIGIT_N_IN = 3
DIGIT_SHAPES = [(1, 1), (5, 3), (6, 3), (7, 8), (11, 2), (21, 3), (63, 1), (9, 7)]


def digit_words(t, basebit):
    """[(name, word, digits or None)]: the words of a digit-shape case, each built from the digits it is meant to have (None: uniform,
    or an edge word whose digits privks_ref.edge_words states)."""
    nb = (1 << basebit) - 1
    h = 1 << (63 - basebit * t)
    rng = np.random.default_rng([1301, t, basebit])
    low = lambda: int(rng.integers(0, h))   # bits under the rounding constant: they change no digit
    one = lambda j: [nb - (j % nb) if k == j else 0 for k in range(t)]   # a digit value that is not always the same
    first_of_last_round = UNROLL * ((t - 1) // UNROLL)
    named = [
        ("every digit nb", [nb] * t),
        ("0, nb, 0, nb", [nb * (j & 1) for j in range(t)]),
        ("nb, 0, nb, 0", [nb * (1 - (j & 1)) for j in range(t)]),
        ("only digit t - 1", one(t - 1)),
        ("only the first digit of the last round", one(first_of_last_round)),
        ("only digit 0", one(0)),
    ]
    out = [(name, w, None) for name, (w, _) in ref.edge_words(t, basebit).items()]
    out += [(name, word_of_digits(d, basebit, low()), d) for name, d in named]
    out += [(f"uniform {g}", int(rng.integers(0, 1 << 64, dtype=np.uint64)), None) for g in range(3)]
    return out


_digit_cases = {}


def digit_case(t, basebit):
    """One batch at n_in = 3: TLWE g holds word g of digit_words at all four positions (every i selects other key rows), the last TLWE
    holds four DIFFERENT special words; every TLWE with c = 0 and c = 1.  Uniform key.  dict(tlwe2, K, T, jobs, want)."""
    if (t, basebit) not in _digit_cases:
        words = digit_words(t, basebit)
        tl = np.array([[w] * (DIGIT_N_IN + 1) for _, w, _ in words] + [[words[g][1] for g in (5, 8, 6, 7)]], dtype=np.uint64)
        K = uniform_rows([1302, t, basebit], key_rows(DIGIT_N_IN, t, basebit))
        n = len(tl)
        rows = 2 * n + 2
        out = np.random.default_rng([1303, t]).permutation(rows)[: 2 * n]
        jobs = [(g % n, (g // n + g % n) & 1, int(out[g])) for g in range(2 * n)]
        assert len(set(j[:2] for j in jobs)) == 2 * n
        T = np.full((rows, WORDS), FILL, dtype=np.uint32)
        rows_of = expected_rows(tl, [j[:2] for j in jobs], t, basebit, ref.key_rows_of(K))
        _digit_cases[(t, basebit)] = dict(words=words, tlwe2=tl, K=K, T=T, jobs=jobs, want=run_jobs(T.copy(), jobs, rows_of))
    return _digit_cases[(t, basebit)]


# ---- 3. offsets past 32 bits ----------------------------------------------------------------------------------------------------------

BIG2_N_IN, BIG2_T, BIG2_BB = 8191, 1, 1            # 8 192 words = 64 KiB per TLWE; 16 384 key rows (134 MB)
BIG2_SLOTS = (1 << 18) + 3                           # 17.18 GB
BIG2_HIGH = [(1 << 16) - 1, 1 << 16, (1 << 18) - 1, 1 << 18, (1 << 18) + 2]   # byte offset 2^32 at slot 2^16, u64 word index 2^31 at 2^18


def big2_aliases(slot):
    """The low slots an offset of `slot` cut to 32 bits could land on: slot - 2^16, slot - 2^18, slot mod 2^16 (a 32-bit byte offset)."""
    return sorted({a for a in (slot - (1 << 16), slot - (1 << 18), slot % (1 << 16)) if 0 <= a != slot})


_big2 = []


def big_tlwe2_case():
    """dict(K, high {slot: TLWE}, low {slot: sentinel TLWE}, jobs, T, want, alias_rows {(slot, c, alias slot): the row an aliased read
    would give}).  Every high slot is read with both c; `low` are the sentinels: slots 0, 1, 2 and every alias that is no high slot."""
    if not _big2:
        rng = np.random.default_rng(1401)
        words = BIG2_N_IN + 1
        K = uniform_rows(1402, key_rows(BIG2_N_IN, BIG2_T, BIG2_BB))
        high = {s: rng.integers(0, 1 << 64, size=words, dtype=np.uint64) for s in BIG2_HIGH}
        low_slots = sorted(({0, 1, 2} | {a for s in BIG2_HIGH for a in big2_aliases(s)}) - set(high))   # an alias may be a high slot itself
        low = {s: rng.integers(0, 1 << 64, size=words, dtype=np.uint64) for s in low_slots}
        jobs = [(s, c, 2 * g + c) for g, s in enumerate(BIG2_HIGH) for c in (1, 0)]
        T = np.full((2 * len(BIG2_HIGH) + 1, WORDS), FILL, dtype=np.uint32)
        row_fn = ref.key_rows_of(K)
        want = T.copy()
        for s, c, out in jobs:
            want[out] = ref.switch(high[s], c, BIG2_T, BIG2_BB, row_fn)
        alias_rows = {(s, c, a): ref.switch(low[a] if a in low else high[a], c, BIG2_T, BIG2_BB, row_fn) for s, c, _ in jobs for a in big2_aliases(s)}
        _big2.append(dict(K=K, high=high, low=low, jobs=jobs, T=T, want=want, alias_rows=alias_rows))
    return _big2[0]


BIGT_ROWS = (1 << 21) + 3                            # 17.18 GB of TRLWE rows: byte offset 2^32 at row 2^19, word index 2^31 / 2^32 at 2^20 / 2^21
BIGT_HIGH = [(1 << 19) - 1, 1 << 19, (1 << 20) - 1, 1 << 20, (1 << 21) - 1, 1 << 21, (1 << 21) + 2]
BIGT_LOW = [0, 1, 2]                                 # sentinels: what the high rows alias modulo 2^19, 2^20, 2^21 and are not themselves written


def bigt_aliases(row):
    return sorted({row % m for m in (1 << 19, 1 << 20, 1 << 21)} - {row})


def big_trlwe_case(per):
    """privks jobs of the plan store's key onto the high rows (distinct (in, c), so an aliased write leaves a wrong row), two selectors of
    `per` rows taken from the high rows (the first `per` and the last `per`: rows shared where per > 3), one two-row CMUX job through each.
    dict(tlwe2, K, jobs, want {row: words}, sentinels [3][2N], sel_rows [2][per], cmux_T, cmux_jobs)."""
    tl, K = plan_store()
    jobs = [(3 + 5 * g, g & 1, r) for g, r in enumerate(BIGT_HIGH)]
    rows_of = expected_rows(tl, [j[:2] for j in jobs], PLAN_T, PLAN_BB, ref.key_rows_of(K))
    want = {r: rows_of[(i, c)] for i, c, r in jobs}
    sentinels = uniform_rows(1411, len(BIGT_LOW))
    sel_rows = np.array([BIGT_HIGH[:per], BIGT_HIGH[-per:]])
    cmux_T = uniform_rows(1412, 6)
    cmux_jobs = [(0, 0, 1, 0, 4), (1, 2, 3, 0, 5)]
    return dict(tlwe2=tl, K=K, jobs=jobs, want=want, sentinels=sentinels, sel_rows=sel_rows, cmux_T=cmux_T, cmux_jobs=cmux_jobs)


BIGK_N_IN, BIGK_T, BIGK_BB = 2048, 10, 4            # 614 700 rows, 5.04 GB
BIGK_LIMIT = (1 << 32) // ROW_BYTES                  # row 524 288: byte offset 2^32
BIGK_I = [0, 1445, 1446, 1447, BIGK_N_IN]            # c = 1: rows of i = 1445 under the limit, of 1446 on both sides, of 1447 and n_in over it


def bigk_row(c, i, j, d):
    nb = (1 << BIGK_BB) - 1
    return ((c * (BIGK_N_IN + 1) + i) * BIGK_T + j) * nb + d - 1


_bigk = []


def big_key_case():
    """TLWEs that are zero but at the words BIGK_I: every digit 15 / digits 15, 0, 15, 0 ... / uniform words; both c.  The key is
    formula_rows of the row index, and only `upload` is ever written: all t nb rows of every (c, i) of BIGK_I, and the rows 524 288
    under those of them that lie over the limit (what a byte offset cut to 32 bits reads instead).
    dict(tlwe2, jobs, T, want, upload [(first row, count)], selected {c: rows}, want_aliased)."""
    if not _bigk:
        nb = (1 << BIGK_BB) - 1
        rng = np.random.default_rng(1421)
        tl = np.zeros((3, BIGK_N_IN + 1), dtype=np.uint64)
        tl[0, BIGK_I] = np.uint64(word_of_digits([nb] * BIGK_T, BIGK_BB))
        tl[1, BIGK_I] = np.uint64(word_of_digits([nb * (1 - (j & 1)) for j in range(BIGK_T)], BIGK_BB))
        tl[2, BIGK_I] = rng.integers(0, 1 << 64, size=len(BIGK_I), dtype=np.uint64)
        jobs = [(g, c, 2 * g + c) for g in range(3) for c in (1, 0)]
        T = np.full((7, WORDS), FILL, dtype=np.uint32)
        want = ref.run_jobs(T.copy(), tl, jobs, BIGK_T, BIGK_BB, formula_rows)
        cut = lambda idx: np.asarray(idx) % BIGK_LIMIT          # the row a byte offset cut to 32 bits reads
        want_aliased = ref.run_jobs(T.copy(), tl, jobs, BIGK_T, BIGK_BB, lambda idx: formula_rows(cut(idx)))
        per_i = BIGK_T * nb
        spans = [(bigk_row(c, i, 0, 1), per_i) for c in (0, 1) for i in BIGK_I]
        rows = sorted({r for first, n in spans for r in range(first, first + n)} |
                      {r - BIGK_LIMIT for first, n in spans for r in range(first, first + n) if r >= BIGK_LIMIT})
        upload, start = [], rows[0]   # runs of consecutive rows
        for a, b in zip(rows, rows[1:] + [None]):
            if b != a + 1:
                upload.append((start, a - start + 1))
                start = b
        selected = {c: np.unique(np.concatenate([ref.selected_rows(tl[g], c, BIGK_T, BIGK_BB) for g in range(3)])) for c in (0, 1)}
        _bigk.append(dict(tlwe2=tl, jobs=jobs, T=T, want=want, want_aliased=want_aliased, upload=upload, selected=selected))
    return _bigk[0]


# ---- 4. host runtime ------------------------------------------------------------------------------------------------------------------

QUEUE_BATCHES = 14                # more than the stream's ring of eight staging slots
QUEUE_SELECTORS = (1, 5, 40)      # the stream's selector scratch (capacity n + n / 2 + 2) grows at the second and at the third call
QUEUE_AFTER = (1, 6, 13)          # trgsw_from_rows + cmux_batch follow these privks batches


def queue_case(per):
    """A program for ONE stream with no synchronisation: ("privks", jobs) x 14 with fourteen different job lists (3 + b jobs, c and in
    varying) on a row store R, and after batches 1, 6, 13 ("from_rows", slots, rows [count][per]) + ("cmux", jobs) with 1, 5, 40
    selectors made of rows written so far.  Batch 13 writes again over the rows the first selector was made of.
    dict(tlwe2, K, R0, C0, slots, program); reference: queue_reference."""
    tl, K = plan_store()
    rng = np.random.default_rng([1501, per])
    program, written, first = [], [], 0
    sel_slot0 = {1: 45, 5: 40, 40: 0}
    for b in range(QUEUE_BATCHES):
        n = 3 + b
        if b == QUEUE_BATCHES - 1:
            outs = written[:n]                       # over the rows of batches 0, 1 ...: the first selector's
        else:
            outs = list(range(first, first + n))
            first += n
            written += outs
        program.append(("privks", [(int(rng.integers(0, 39)), (g + b) & 1, out) for g, out in enumerate(outs)]))
        if b in QUEUE_AFTER:
            count = QUEUE_SELECTORS[QUEUE_AFTER.index(b)]
            rows = np.array([rng.choice(written, size=per, replace=False) for _ in range(count)])
            slots = list(range(sel_slot0[count], sel_slot0[count] + count))
            base = {1: 0, 5: 3, 40: 18}[count]       # rows of the CMUX store: in0, in1, out of selector g at base + 3 g ...
            program.append(("from_rows", slots, rows))
            program.append(("cmux", [(slots[g], base + 3 * g, base + 3 * g + 1, 0, base + 3 * g + 2) for g in range(count)]))
    R0 = np.full((first + 2, WORDS), FILL, dtype=np.uint32)
    C0 = uniform_rows([1502, per], 18 + 3 * 40)
    return dict(tlwe2=tl, K=K, R0=R0, C0=C0, slots=46, program=program)


def run_reference(p, case, program, R, C, trgsw):
    """The calls of a program one after the other on numpy copies: R rows (privks_ref), trgsw torus-domain selectors (rows of R as they
    are at the call), C rows (cmux_ref).  In place; returns (R, C)."""
    import cmux_ref

    tl, row_fn = case["tlwe2"], ref.key_rows_of(case["K"])
    memo = {}
    for call in program:
        if call[0] == "privks":
            for i, c, out in call[1]:
                if (i, c) not in memo:
                    memo[(i, c)] = ref.switch(tl[i], c, PLAN_T, PLAN_BB, row_fn)
                R[out] = memo[(i, c)]
        elif call[0] == "from_rows":
            for slot, rows in zip(call[1], call[2]):
                trgsw[slot] = R[rows].reshape(trgsw.shape[1:])
        else:
            cmux_ref.run_jobs(p, C, trgsw, call[1])
    return R, C


SLOT_LISTS = {
    "several runs": [5, 6, 7, 2, 9, 10, 0],          # runs 5-7, 2, 9-10, 0: four launches
    "descending": [3, 2, 1],                         # three launches
    "the last slot inside a run": [9, 10, 11, 4],    # of a store of 12 slots
}
SLOT_STORE = 12


def slot_case(name, per):
    """trgsw_from_rows with the slot list `name` on a store of SLOT_STORE slots: uniform rows, selector g takes `per` rows from all over
    the store and shares its first row with selector g - 1; then one two-row CMUX job through every slot of the list.
    dict(R, slots, rows, C0, jobs)."""
    slots = SLOT_LISTS[name]
    rng = np.random.default_rng([1511, per, len(slots)])
    nrows = len(slots) * per + 3
    R = uniform_rows([1512, per], nrows)
    rows = rng.permutation(nrows)[: len(slots) * per].reshape(len(slots), per)
    for g in range(1, len(slots)):
        rows[g, 0] = rows[g - 1, per - 1]            # one row used by two selectors
    C0 = uniform_rows([1513, per], 3 * len(slots))
    jobs = [(slots[g], 3 * g, 3 * g + 1, 0, 3 * g + 2) for g in range(len(slots))]
    return dict(R=R, slots=slots, rows=rows, C0=C0, jobs=jobs)


TWO_ROUNDS = 5


def two_stream_case(per):
    """Two programs for two streams that share key, lvl2 store, row store, selector store and CMUX rows, on disjoint rows and slots:
    TWO_ROUNDS rounds of privks (2 per jobs) + from_rows (2 selectors) + cmux (2 jobs) each, every round on rows and slots of its own.
    dict(tlwe2, K, R0, C0, slots, programs [2])."""
    tl, K = plan_store()
    rng = np.random.default_rng([1521, per])
    programs = []
    rows_per = 2 * per * TWO_ROUNDS
    for s in range(2):
        prog = []
        for r in range(TWO_ROUNDS):
            r0 = s * rows_per + r * 2 * per
            outs = list(range(r0, r0 + 2 * per))
            prog.append(("privks", [(int(rng.integers(0, 39)), (g + r + s) & 1, out) for g, out in enumerate(outs)]))
            slots = [(s * TWO_ROUNDS + r) * 2 + 1, (s * TWO_ROUNDS + r) * 2]                # descending: two launches
            prog.append(("from_rows", slots, np.array(outs).reshape(2, per)[:, ::-1]))
            c0 = (s * TWO_ROUNDS + r) * 6
            prog.append(("cmux", [(slots[g], c0 + 3 * g, c0 + 3 * g + 1, 0, c0 + 3 * g + 2) for g in range(2)]))
        programs.append(prog)
    R0 = np.full((2 * rows_per + 1, WORDS), FILL, dtype=np.uint32)
    C0 = uniform_rows([1522, per], 2 * TWO_ROUNDS * 6)
    return dict(tlwe2=tl, K=K, R0=R0, C0=C0, slots=4 * TWO_ROUNDS, programs=programs)
