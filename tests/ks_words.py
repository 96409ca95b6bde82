"""Chosen words for the key switch (lvl1 -> lvl0) and a mirror of its launch geometry — test infrastructure only.

A TLWE1 coefficient a'_i is built from the 2 t digit bits D the key switch will decode from a'_i + prec and the bits L below
them:  a'_i = (D << (32 - 2 t)) + L - prec  (mod 2^32),  prec = 2^(31 - 2 t),  so that a'_i + prec carries exactly the digits D.
The TRLWE image the C ABI's SampleExtractAndKeySwitch takes is the inverse of the oracle's orc_sample_extract0:
a[0] = t1[0], a[N - j] = -t1[j], b[0] = t1[N]; b[1 .. N - 1] are ignored by the extraction and filled at random.

Families (each a list of TRLWE images, 2 N words):
  cover   16 cells: coefficient i of cell c takes, at stage s, the pair value (c + 3 i + 5 s) mod 16 (mod 4 for the single last
          digit of an odd t).  Together the 16 cells select every row (i, s, v) of the pair table of keyswitch_lut_kernel,
          zero rows included, and every (i, j, v) KSK row of the other two kernels.
  edges   every digit 0, every digit 3 (pair 15 everywhere), the carry wrap to D = 0 (a' = 2^32 - prec + x, x < prec) and to D all ones
          (a' = 2^32 - prec - 1).
  lbits   the cover family with L = 0, L = 2^(32 - 2 t) - 1, L = prec - 1 and L = prec + 1.
  raw     TRLWE words as they are: all 0, all 0xFFFFFFFF, the sign bit, alternating extremes, uniform.
The b word (t1[N]) cycles through 0, 0xFFFFFFFF and uniform values.
"""
import numpy as np

MASK32 = (1 << 32) - 1
TABLE_MIN_JOBS = 4096     # csrc/dispatch.hpp: KS_LUT_MIN_JOBS
SHARED_MAX_DEFAULT = 4096  # csrc/dispatch.hpp: KS_SHARED_MAX_DEFAULT (IYK_HIP_KS_SHARED_MAX unset)
KSL_GROUP = 128           # csrc/dispatch.hpp: KS_TABLE_GATES (kernels.hpp: KSL_WAVES * KSL_G gates per workgroup of keyswitch_lut_kernel)


def prec_of(t):
    return 1 << (31 - 2 * t)


def rows_per_i(t):
    """Rows of the pair table per coefficient (kernels.hpp: ksl_rows_per_i)."""
    return 16 * (t // 2) + 4 * (t % 2)


def stage_rows(t):
    """Rows of each stage of one coefficient: 16 per digit pair, 4 for the single last digit of an odd t."""
    return [16] * (t // 2) + [4] * (t % 2)


def table_bytes(p):
    """Bytes of the pair table ensure_ks_lut allocates: N rows_per_i + 12 padding rows of NC * 128 words."""
    stride = (p.n + 1 + 3) & ~3
    nc = (stride + 127) // 128
    return (p.N * rows_per_i(p.t) + 12) * nc * 128 * 4


def words_from_digits(D, L, t):
    """a' with a' + prec = (D << (32 - 2 t)) + L (mod 2^32)."""
    D = np.asarray(D, dtype=np.uint64)
    L = np.asarray(L, dtype=np.uint64)
    return (((D << np.uint64(32 - 2 * t)) + L - np.uint64(prec_of(t))) & np.uint64(MASK32)).astype(np.uint32)


def digits_of(words, t):
    """The 2 t digit bits of a' + prec, as orc_keyswitch reads them."""
    w = (np.asarray(words, dtype=np.uint64) + np.uint64(prec_of(t))) & np.uint64(MASK32)
    return (w >> np.uint64(32 - 2 * t)).astype(np.int64)


def digit_list(words, t):
    """[t][len(words)]: digit j of a' + prec = (a' + prec >> (32 - 2 (j + 1))) & 3 — orc_keyswitch's decode."""
    w = (np.asarray(words, dtype=np.uint64) + np.uint64(prec_of(t))) & np.uint64(MASK32)
    return [((w >> np.uint64(32 - 2 * (j + 1))) & np.uint64(3)).astype(np.int64) for j in range(t)]


def table_rows_selected(words, t):
    """[N]-long rows of the pair table each stage selects, from orc_keyswitch's digits: (stage s, row 16 s + (v_2s << 2 | v_2s+1))
    and for an odd t the single last digit's row 16 (t // 2) + v_(t-1).  Returns a list over stages of row arrays."""
    d = digit_list(words, t)
    out = [16 * s + ((d[2 * s] << 2) | d[2 * s + 1]) for s in range(t // 2)]
    if t % 2:
        out.append(16 * (t // 2) + d[t - 1])
    return out


def digits_from_stage_values(vals, t):
    """Stage values (pair values, then the single digit of an odd t) -> D."""
    D = np.zeros_like(np.asarray(vals[0], dtype=np.int64))
    for s in range(t // 2):
        D = D | (np.asarray(vals[s], dtype=np.int64) << (2 * t - 4 * (s + 1)))
    if t % 2:
        D = D | np.asarray(vals[t // 2], dtype=np.int64)
    return D


def image_from_t1(t1, rng, N):
    """A TRLWE image (a[0..N), b[0..N)) whose sample extract of coefficient 0 is t1 (N + 1 words)."""
    t1 = np.asarray(t1, dtype=np.uint32)
    img = np.empty(2 * N, dtype=np.uint32)
    img[0] = t1[0]
    img[N - np.arange(1, N)] = (np.uint32(0) - t1[1:N]).astype(np.uint32)
    img[N] = t1[N]
    img[N + 1:] = rng.integers(0, 1 << 32, size=N - 1, dtype=np.uint64).astype(np.uint32)
    return img


def t1_from_image(img, N):
    """orc_sample_extract0 restated: t1[0] = a[0], t1[j] = -a[N - j], t1[N] = b[0]."""
    out = np.empty(N + 1, dtype=np.uint32)
    out[0] = img[0]
    out[1:N] = (np.uint32(0) - img[N - np.arange(1, N)]).astype(np.uint32)
    out[N] = img[N]
    return out


def cover_stage_values(c, t, N):
    i = np.arange(N, dtype=np.int64)
    vals = [(c + 3 * i + 5 * s) % 16 for s in range(t // 2)]
    if t % 2:
        vals.append((c + 3 * i + 5 * (t // 2)) % 4)
    return vals


def _b_word(k, rng):
    return [0, MASK32, int(rng.integers(0, 1 << 32, dtype=np.uint64))][k % 3]


def chosen_t1(p, seed=0):
    """{family: [t1 words (N + 1)]} for the cover, edges and lbits families (raw words are built as images)."""
    N, t = p.N, p.t
    rng = np.random.default_rng(seed)
    low = 1 << (32 - 2 * t)
    prec = prec_of(t)
    fam = {"cover": [], "edges": [], "lbits": []}
    k = 0

    def t1_of(a, rng):
        nonlocal k
        w = np.empty(N + 1, dtype=np.uint32)
        w[:N] = a
        w[N] = _b_word(k, rng)
        k += 1
        return w

    for c in range(16):
        L = rng.integers(0, low, size=N, dtype=np.uint64)
        fam["cover"].append(t1_of(words_from_digits(digits_from_stage_values(cover_stage_values(c, t, N), t), L, t), rng))
    L = rng.integers(0, low, size=N, dtype=np.uint64)
    fam["edges"].append(t1_of(words_from_digits(np.zeros(N, dtype=np.int64), L, t), rng))                 # every digit 0
    fam["edges"].append(t1_of(words_from_digits(np.full(N, (1 << 2 * t) - 1), L, t), rng))               # every digit 3
    x = rng.integers(0, prec, size=N, dtype=np.uint64)   # a' >= 2^32 - prec: a' + prec carries out of the word, to x < 2^(32 - 2 t)
    x[0], x[1] = 0, prec - 1
    fam["edges"].append(t1_of(((np.uint64(1 << 32) - np.uint64(prec) + x) & np.uint64(MASK32)).astype(np.uint32), rng))  # wraps to D = 0
    fam["edges"].append(t1_of(np.full(N, (1 << 32) - prec - 1, dtype=np.uint64).astype(np.uint32), rng))            # D all ones
    for Lv in (0, low - 1, prec - 1, prec + 1):
        for c in range(16):
            D = digits_from_stage_values(cover_stage_values(c, t, N), t)
            fam["lbits"].append(t1_of(words_from_digits(D, np.full(N, Lv), t), rng))
    return fam


def raw_images(p, seed=0):
    N = p.N
    rng = np.random.default_rng(seed + 1)
    imgs = [np.zeros(2 * N, dtype=np.uint32), np.full(2 * N, MASK32, dtype=np.uint32), np.full(2 * N, 0x80000000, dtype=np.uint32),
            np.where(np.arange(2 * N) % 2 == 0, 0, MASK32).astype(np.uint32),
            rng.integers(0, 1 << 32, size=2 * N, dtype=np.uint64).astype(np.uint32)]
    for k, img in enumerate(imgs):   # the b word: 0, all ones, uniform, in turn (the all-ones image keeps its own)
        if k != 1:
            img[N] = _b_word(k, rng)
    return imgs


def chosen_images(p, seed=0):
    """(images [cells][2 N], family name per cell): cover, edges, lbits, raw — the cells every wide enough case contains."""
    rng = np.random.default_rng(seed + 2)
    fam = chosen_t1(p, seed)
    imgs, names = [], []
    for name in ("cover", "edges", "lbits"):
        for w in fam[name]:
            imgs.append(image_from_t1(w, rng, p.N))
            names.append(name)
    for img in raw_images(p, seed):
        imgs.append(img)
        names.append("raw")
    return np.stack(imgs), names


# ---- launch geometry ----------------------------------------------------------------------------------------------------------

def ks_geometry(kind, shared_max, n, t, cus, shared_wg=None):
    """(form, groups, slices) of the key-switch launch of n jobs at t digits, as ks_plan of iyokan_amd/csrc/dispatch.hpp decides it
    (tests/test_ks_words.py holds this mirror to ks_plan itself, case by case):
      IYK_HIP_KS_KERNEL = kind ('0' .. '2'; anything else: KS_KIND_DEFAULT = 2); kind 2 and n > KS_LUT_MIN_JOBS = 4096 -> the table form:
        ceil(n / 128) groups, slices doubled while < 8 and groups * slices < cus; kind >= 1 -> the wave kernel; else
        keyswitch_kernel: ceil(n / 16) groups, slices doubled while < 64 and groups * slices < 512;
      the wave kernel: n <= IYK_HIP_KS_SHARED_MAX (KS_SHARED_MAX_DEFAULT = 4096) -> the shared form: ceil(n / 16) groups, slices
        doubled while < max_slices (256 / 128 / 64 from 1 / 2 / 4 groups on) and groups * slices < IYK_HIP_KS_SHARED_WG
        (KS_SHARED_WG_DEFAULT = 512); else the wide form: ceil(n / 64) groups, slices doubled while < 256 and groups * slices < 512.
    Forms: 'table' (keyswitch_lut_kernel), 'shared' / 'wide' (keyswitch_wave_kernel, SHARED = true / false), 'kind0'
    (keyswitch_kernel).  The table and the wave kernel exist for t = 7 (128-bit set) and t = 8 (80-bit set) only."""
    kind = int(kind) if kind is not None and str(kind)[:1] in ("0", "1", "2") else 2
    if t not in (7, 8):   # the table and the wave kernel are instantiated for the two parameter sets only
        kind = 0
    if kind == 2 and n > TABLE_MIN_JOBS:
        groups = -(-n // KSL_GROUP)
        slices = 1
        while slices < 8 and groups * slices < cus:
            slices *= 2
        return "table", groups, slices
    if kind >= 1:
        smax = SHARED_MAX_DEFAULT if shared_max is None else int(shared_max)
        if n <= smax:
            min_wg = 512 if shared_wg is None else max(1, int(shared_wg))
            groups = -(-n // 16)
            max_slices = 64 if groups >= 4 else 128 if groups >= 2 else 256
            slices = 1
            while slices < max_slices and groups * slices < min_wg:
                slices *= 2
            return "shared", groups, slices
        groups = -(-n // 64)
        slices = 1
        while slices < 256 and groups * slices < 512:
            slices *= 2
        return "wide", groups, slices
    groups = -(-n // 16)
    slices = 1
    while slices < 64 and groups * slices < 512:
        slices *= 2
    return "kind0", groups, slices


def gates_per_group(form):
    return {"table": KSL_GROUP, "shared": 16, "wide": 64, "kind0": 16}[form]


# (IYK_HIP_KS_KERNEL, IYK_HIP_KS_SHARED_MAX, sizes) of tests/test_gpu_keyswitch.py; the 1-job cases run several chosen cells one by one
BASE_CASES = [
    ("0", None, [1, 17, 256, 512, 1024, 2048, 4097, 8193]),
    ("1", None, [1, 17, 64, 65, 256, 1000, 1024, 2048, 4096, 4097]),
    ("1", "0", [1, 65, 129, 257, 513, 1025, 2049, 4097, 8193, 16385, 32769]),
    ("2", None, [4096, 4097, 4224, 8192, 8193, 16384, 16385, 32768, 32769]),
]


def table_boundary_sizes(cus, t=7):
    """For every slice count of the table form at `cus` CUs: the widest batch with whole workgroups and the widest ragged one."""
    out = set()
    g = TABLE_MIN_JOBS // KSL_GROUP + 1
    last = None
    while True:
        sl = ks_geometry("2", None, g * KSL_GROUP, t, cus)[2]
        if last is not None and sl != last:
            out.update({(g - 1) * KSL_GROUP, (g - 2) * KSL_GROUP + 1})
        if sl == 1:
            out.update({g * KSL_GROUP, g * KSL_GROUP + 1})
            break
        last = sl
        g += 1
    return sorted(n for n in out if n > TABLE_MIN_JOBS)


def cases(cus, t=7):
    """[(kind, shared_max, n)]: BASE_CASES plus the table sizes at either end of each slice count at `cus` CUs."""
    out = [(k, sm, n) for k, sm, ns in BASE_CASES for n in ns]
    have = {n for k, sm, n in out if k == "2"}
    out += [("2", None, n) for n in table_boundary_sizes(cus, t) if n not in have]
    return out


def expected_shapes():
    """(form, slices) every launch form can take at 256 CUs; the table form also with a whole and a ragged last workgroup."""
    shapes = {("kind0", s) for s in (64, 32, 16, 8, 4, 2, 1)}
    shapes |= {("shared", s) for s in (256, 128, 64, 32, 16, 8, 4, 2)}
    shapes |= {("wide", s) for s in (256, 128, 64, 32, 16, 8, 4, 2, 1)}
    shapes |= {("table", s, r) for s in (8, 4, 2, 1) for r in ("whole", "ragged")}
    return shapes


def reached_shapes(case_list, t, cus):
    out = set()
    for kind, smax, n in case_list:
        form, groups, slices = ks_geometry(kind, smax, n, t, cus)
        if form == "table":
            out.add((form, slices, "whole" if n % KSL_GROUP == 0 else "ragged"))
        else:
            out.add((form, slices))
    return out


def job_layout(n, special, ncells, rng):
    """trlwe_index of a case of n jobs: uniform cells, with the `special` cells placed at the first job, ending at the last job and
    straddling a 16-gate wave boundary in the middle (as far as n allows; the copy at the first job is written last, so a case of
    len(special) jobs or more holds all of them)."""
    idx = rng.integers(0, ncells, size=n).astype(np.int32)
    k = len(special)
    if n <= 1:
        return idx
    sp = np.asarray(special, dtype=np.int32)
    if n >= k:
        idx[n - k:] = sp                                           # the last job holds special[-1]
        mid = (n // 2) // 16 * 16                                  # a wave boundary: special[k // 2 - 1] | special[k // 2]
        lo = max(0, mid - k // 2)
        idx[lo:lo + k] = sp[:min(k, n - lo)]
        idx[:k] = sp
    else:
        idx[:] = sp[:n]
    return idx
