"""numpy restatement of the private functional key switch lvl2 -> lvl1 (test support for test_privks_ref / test_gpu_privks): the
digits of a 64-bit word and the sum of the key rows they select, from the published algorithm — never the code under test.

    wbar   = w + 2^(63 - basebit t)                          (mod 2^64)
    d_j(w) = (wbar >> (64 - (j+1) basebit)) & (2^basebit - 1)   j < t
    R_c    = - sum_{i <= n_in} sum_{j < t, d_j(w_i) != 0} K[c][i][j][d_j(w_i) - 1]     (mod 2^32)

The key is only ever asked for the rows a job selects (row_fn: row indices -> u32 [m][2N]), so a full-size key (2.35 GB) is never
materialised here."""
import numpy as np

M32 = 0xFFFFFFFF
M64 = (1 << 64) - 1


def digits(w, t, basebit):
    """u64 words (any shape) -> their t digits, most significant first: uint32 [..., t]."""
    w = np.asarray(w, dtype=np.uint64)
    wbar = np.array([(int(x) + (1 << (63 - basebit * t))) & M64 for x in w.ravel()], dtype=np.uint64).reshape(w.shape)
    out = np.zeros(w.shape + (t,), dtype=np.uint32)
    for j in range(t):
        out[..., j] = ((wbar >> np.uint64(64 - (j + 1) * basebit)) & np.uint64((1 << basebit) - 1)).astype(np.uint32)
    return out


def edge_words(t, basebit):
    """The words at which the digits change character, and what every digit of each must be (None: not all digits alike)."""
    h = 1 << (63 - basebit * t)   # the rounding constant: half of the last digit's unit
    nb = (1 << basebit) - 1
    return {
        "zero": (0, 0),
        "below the rounding threshold": (h - 1, 0),
        "at the rounding threshold": (h, None),           # last digit 1, the others 0
        "largest without wrap": (M64 - h, nb),
        "smallest that wraps to zero": ((1 << 64) - h, 0),
    }


def selected_rows(tlwe, c, t, basebit):
    """Row indices ((c (n_in+1) + i) t + j) nb + d - 1 of the key rows one job adds up, int64 [m]."""
    tlwe = np.asarray(tlwe, dtype=np.uint64).ravel()
    n1, nb = tlwe.size, (1 << basebit) - 1
    d = digits(tlwe, t, basebit).astype(np.int64)
    i, j = np.nonzero(d)
    return ((c * n1 + i) * t + j) * nb + (d[i, j] - 1)


def switch(tlwe, c, t, basebit, row_fn):
    """R_c of one lvl2 TLWE (u64 [n_in + 1]): the 2N words."""
    idx = selected_rows(tlwe, c, t, basebit)
    rows = np.asarray(row_fn(idx), dtype=np.uint32)
    if idx.size == 0:
        return np.zeros(rows.shape[1], dtype=np.uint32)
    total = rows.sum(axis=0, dtype=np.int64)           # < 2^32 * rows: no overflow below 2^31 rows
    return ((-total) & M32).astype(np.uint32)


def key_rows_of(K):
    """row_fn of a key held as an array [..., 2N] in the host layout."""
    flat = np.asarray(K, dtype=np.uint32)
    flat = flat.reshape(-1, flat.shape[-1])
    return lambda idx: flat[idx]


def run_jobs(T, tlwe2, jobs, t, basebit, row_fn):
    """Jobs (in, c, out) in place on the TRLWE rows T."""
    for in_, c, out in jobs:
        T[out] = switch(tlwe2[in_], c, t, basebit, row_fn)
    return T


def selector_rows(tlwe2_digits, t, basebit, row_fn, l, k=1):
    """The (k+1) l rows (row c l + r) of one TRGSW, torus domain [(k+1) l][k+1][N], from the l lvl2 TLWEs of one bit."""
    rows = [switch(tlwe2_digits[r], c, t, basebit, row_fn) for c in range(k + 1) for r in range(l)]
    return np.stack(rows).reshape((k + 1) * l, k + 1, -1)
