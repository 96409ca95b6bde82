"""The chosen cases of tests/ks_matrix_cases.py are what tests/test_gpu_keyswitch_matrix_edges.py takes them for: keys that carry out
of every plane, cells with the one digit they name, job lists that reach every accumulator row in every workgroup, a gate level with
MUX jobs at the edges of every wave, programs whose batches never share a slot.  No GPU."""
import ctypes
import os

import numpy as np
import pytest

import arena_cases as ac
import ks_matrix_cases as M
import ks_words as K
from iyokan_amd.params import OPS, params_128bit, params_80bit

SETS = {"128": params_128bit, "80": params_80bit}
_u32p = ctypes.POINTER(ctypes.c_uint32)


@pytest.fixture(scope="module")
def em():
    L = ctypes.CDLL(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "iyokan_amd", "lib", "libiyk_emul.so"))
    L.iyk_emul_ks_matrix_bytes.argtypes = [ctypes.c_int] * 2
    L.iyk_emul_ks_matrix_bytes.restype = ctypes.c_int64
    L.iyk_emul_ks_signed_planes.argtypes = [_u32p, ctypes.c_int, ctypes.POINTER(ctypes.c_int8)]
    L.iyk_emul_ks_signed_planes.restype = None
    return L


def _digits(img, p):
    """[t][N] digits of the TLWE1 the image extracts to."""
    return np.stack(K.digit_list(K.t1_from_image(img, p.N)[:p.N], p.t))


def test_constants_mirror_the_library(em):
    assert M.GATES == em.iyk_emul_ks_matrix_gates(0) == 256 and M.WAVE_GATES == em.iyk_emul_ks_matrix_gates(1) == 64
    assert M.MIN_JOBS == em.iyk_emul_ks_matrix_min_jobs() == 4608
    assert M.EDGE_JOBS == 549 and 2 * M.GATES < M.EDGE_JOBS and (M.EDGE_JOBS - 2 * M.GATES) % 32 not in (0, 31)   # ragged inside a tile
    for which, (t, nc) in {"128": (7, 5), "80": (8, 4)}.items():
        p = SETS[which]()
        assert (p.t, M.nc_of(p)) == (t, nc)
        assert M.OPERAND_BYTES[which] == M.operand_bytes(p) == 4 * 1024 * t * nc * 128 * 4 == em.iyk_emul_ks_matrix_bytes(t, nc)
    assert M.OPERAND_BYTES == {"128": 73_400_320, "80": 67_108_864}


@pytest.mark.parametrize("which", ["128", "80"])
def test_carry_and_salted_keys(which, request, em):
    keys = request.getfixturevalue("keys" + which)
    p = keys.params
    plain, carry = M.ksk_rows(keys), M.ksk_rows(M.carry_keys(keys))
    doctored = [0, 1, 511, 1023]
    rest = np.setdiff1d(np.arange(p.N), doctored)
    assert np.array_equal(carry[rest], plain[rest])
    rows = carry[doctored]
    by = rows.view(np.uint8)
    assert set(np.unique(by).tolist()) == {0x7F, 0x80}
    mixes = ((rows >> 7) & 1) | ((rows >> 14) & 2) | ((rows >> 21) & 4) | ((rows >> 28) & 8)    # which bytes are 0x80
    assert all(set(np.unique(mixes[k, j, u]).tolist()) == set(range(16)) for k in range(4) for j in range(p.t) for u in range(3))
    # the signed split of these words: a byte 0x80 is -128 and carries, a byte 0x7F above a carry becomes -128 and carries on
    w = np.ascontiguousarray(rows[0, 0, 0])
    planes = np.empty((len(w), 4), dtype=np.int8)
    em.iyk_emul_ks_signed_planes(w.ctypes.data_as(_u32p), len(w), planes.ctypes.data_as(ctypes.POINTER(ctypes.c_int8)))
    assert set(np.unique(planes).tolist()) == {-128, -127, 127}
    assert np.array_equal((planes.astype(np.int64) * (np.int64(256) ** np.arange(4))).sum(axis=1) & K.MASK32, w.astype(np.int64))
    a, b = M.salted_keys(keys, 4), M.salted_keys(keys, 5)
    assert a.bk is keys.bk and a.params is p
    assert all(np.mean(np.asarray(x.ksk) != np.asarray(y.ksk)) > 0.999 for x, y in ((a, keys), (b, keys), (a, b)))
    assert np.array_equal(np.asarray(a.ksk), np.asarray(M.salted_keys(keys, 4).ksk))


@pytest.mark.parametrize("which", ["128", "80"])
def test_named_cells_are_what_their_names_say(which):
    p = SETS[which]()
    t, N = p.t, p.N
    cells, nnamed, nspecial, b0 = M.cells(p, seed=int(which), ncells=120)
    assert nnamed == len(M.NAMED) == 8 and nspecial == nnamed + len(K.chosen_images(p, int(which))[0]) and nspecial <= 120
    assert np.array_equal(cells[nnamed:nspecial], K.chosen_images(p, int(which))[0])
    d = [_digits(cells[c], p) for c in range(nnamed)]
    assert not d[0].any() and int(cells[0][N]) == b0
    assert (d[1] == 3).all()
    t1 = K.t1_from_image(cells[2], N)
    assert (t1[:N] == 0xFFFFFFFF).all() and not d[2].any()                     # a' + prec wraps to prec - 1: every digit 0
    t1 = K.t1_from_image(cells[3], N)
    assert (t1[:N] == np.uint32((1 << 32) - K.prec_of(t))).all() and not d[3].any()    # a' + prec = 0 exactly
    for k, (i, j) in enumerate(((0, 0), (0, t - 1), (N - 1, 0), (N - 1, t - 1))):
        want = np.zeros((t, N), dtype=np.int64)
        want[j, i] = 1 + k % 3
        assert np.array_equal(d[4 + k], want)


@pytest.mark.parametrize("which", ["128", "80"])
def test_digit_sweep_holds_exactly_the_digit_it_names(which, request):
    """64 t 3 cells, every (c, j, v) at every chosen block; each decodes to that one digit; and the oracle's key switch of such a cell
    is (0, .., 0, b') minus the one key row, under the ordinary and under the carrying key."""
    import oracle_lib
    from test_gpu_keyswitch import _reference

    keys = request.getfixturevalue("keys" + which)
    p = keys.params
    t = p.t
    imgs, digits = M.digit_sweep(p, np.random.default_rng(1))
    assert len(imgs) == len(digits) == 64 * t * 3 == {7: 1344, 8: 1536}[t]
    assert {tuple(x) for x in digits.tolist()} == {(16 * blk + c, j, v) for blk in (0, 1, 31, 63) for c in range(16) for j in range(t)
                                                    for v in (1, 2, 3)}
    assert {int(i) % 16 for i in digits[:, 0]} == set(range(16)) and {int(i) // 16 for i in digits[:, 0]} == {0, 1, 31, 63}
    for img, (i, j, v) in zip(imgs, digits):
        d = _digits(img, p)
        assert d[j, i] == v and np.count_nonzero(d) == 1
    low = K.t1_from_image(imgs[0], p.N)[:p.N].astype(np.uint64) + np.uint64(K.prec_of(t))
    assert ((low[1:] & np.uint64((1 << (32 - 2 * t)) - 1)) != 0).any()             # random bits below the digit window
    assert len({int(img[p.N]) for img in imgs}) > len(imgs) - 3                    # random b
    # a staging lane packs the 2 t digit bits of 4 coefficients into t bytes: at t = 7 coefficients start inside a byte
    starts = {(2 * t * c) % 8 for c in range(4)}
    assert starts == ({0, 6, 4, 2} if t == 7 else {0})
    pick = np.arange(0, len(imgs), 7)
    for ks in (keys, M.carry_keys(keys)):
        orc = oracle_lib.Oracle(ks)
        try:
            ref = _reference(orc, np.ascontiguousarray(imgs[pick]))
        finally:
            orc.close()
        for k, c in enumerate(pick):
            assert np.array_equal(ref[k], M.single_digit_output(ks, imgs[c], *(int(x) for x in digits[c])))


@pytest.mark.parametrize("which", ["128", "80"])
def test_position_sweep_reaches_every_accumulator_row(which):
    p = SETS[which]()
    imgs, idx = M.position_sweep(p, np.random.default_rng(2))
    assert len(imgs) == 257 and len(idx) == M.EDGE_JOBS == 2 * 256 + 37 and idx.dtype == np.int32
    assert not _digits(imgs[0], p).any()
    seen = set()
    for r in range(256):
        d = _digits(imgs[1 + r], p)
        i, j, v = M.position_digit(r, p.t)
        assert d[j, i] == v and np.count_nonzero(d) == 1
        seen.add((i, j, v))
    assert len(seen) == 256 and len({i for i, _, _ in seen}) == 256                # distinctive: no two share a coefficient
    jobs = np.flatnonzero(idx)
    assert sorted((jobs % 256).tolist()) == list(range(256))                        # every residue once across the list
    assert np.array_equal(idx[jobs], 1 + jobs % 256)
    classes = {(int(r) // 64, int(r) % 64 // 32, int(r) % 32) for r in jobs % 256}
    assert len(classes) == 4 * 2 * 32
    per_group = np.bincount(jobs // 256, minlength=3)
    assert per_group.tolist() == [121, 122, 13] and jobs.max() < M.EDGE_JOBS
    assert set((jobs[jobs >= 512] - 512).tolist()) == set(range(0, 37, 3))         # the ragged third: both of its tiles
    assert all(jobs[jobs // 256 == g].min() % 256 < 4 and jobs[jobs // 256 == g].max() % 256 > (250 if g < 2 else 33) for g in range(3))


def test_gate_level_puts_mux_jobs_at_the_edges_of_every_wave():
    nin = 16
    lv = M.gate_levels(np.random.default_rng(3), nin)
    ops = lv["ops"]
    n = M.EDGE_JOBS
    assert len(ops) == n + len(M.GATE_EXTRA) and np.all(ops[:n] <= OPS["MUX"]) and np.all(ops[n:] > OPS["MUX"])
    assert ac.rotations(lv) == n + len(M.mux_jobs()) and ac.independent(lv)
    mux = M.mux_jobs()
    assert mux == [0, 63, 64, 127, 128, 191, 192, 255, 256, 319, 320, 383, 384, 447, 448, 511, 512, 548]
    assert np.flatnonzero(ops == OPS["MUX"]).tolist() == mux
    nb = M.mux_neighbours()
    assert nb == [1, 62, 65, 126, 129, 190, 193, 254, 257, 318, 321, 382, 385, 446, 449, 510, 513, 547]
    assert {int(ops[j]) for j in nb} == {OPS[k] for k in ac.BINARY}                 # every binary kind beside a MUX
    assert all(lv["in2"][j] >= 0 for j in mux) and np.all(lv["in2"][np.setdiff1d(np.arange(len(ops)), mux)] == -1)
    assert {ac.OP_NAMES[int(o)] for o in ops[n:]} == {"NOT", "COPY", "CONSTONE", "CONSTZERO"}
    assert lv["out"].tolist() == list(range(nin, nin + len(ops)))
    assert all(0 <= s < nin for _, s in ac.inputs_of(lv))
    sample = M.oracle_sample()
    assert len(sample) == len(set(sample.tolist())) == 41 and set(mux) | set(nb) <= set(sample.tolist())
    bits = np.full(nin + len(ops), -1, dtype=np.int8)
    bits[:nin] = np.arange(nin) % 2
    assert set(np.unique(ac.simulate_level(lv, bits)).tolist()) <= {0, 1}


def _check_batches(prog, ncells, special):
    used = set()
    for idx, out_slot in prog["batches"]:
        assert len(idx) == len(out_slot) == M.BATCH_JOBS and idx.dtype == out_slot.dtype == np.int32
        assert 0 <= idx.min() and idx.max() < ncells and set(special) <= set(idx.tolist())
        assert idx[0] == special[0] and idx[-1] == special[-1]
        slots = set(out_slot.tolist())
        assert len(slots) == len(out_slot) and not slots & used and max(slots) < prog["slots"]
        used |= slots
    assert len(used) < prog["slots"]                                                # slots nobody writes remain
    ref = np.arange(ncells * 5, dtype=np.uint32).reshape(ncells, 5)
    want = M.expected_arena(prog, ref, 0xA5A5A5A5)
    free = np.setdiff1d(np.arange(prog["slots"]), sorted(used))
    assert (want[free] == 0xA5A5A5A5).all()
    for idx, out_slot in prog["batches"]:
        assert np.array_equal(want[out_slot], ref[idx])


def test_first_use_program():
    special = list(range(97))
    prog = M.first_use_program(np.random.default_rng(4), special, 640)
    assert prog["threads"] == [[0, 1], [2, 3], [4, 5]] and len(prog["batches"]) == 6
    _check_batches(prog, 640, special)


def test_stream_program():
    """Every batch runs once, on a stream that exists; the first batch of the matrix form is A's and has unfinished batches of its own
    stream before it; B's follows with no sync between; C is created after it; A is destroyed behind a sync and B and C run after."""
    special = list(range(97))
    prog = M.stream_program(np.random.default_rng(5), special, 640)
    _check_batches(prog, 640, special)
    live, ran, order = set(), [], []
    for step in prog["steps"]:
        order.append(step[0] if step[0] != "batch" else step[0] + step[1] + step[3])
        if step[0] == "create":
            assert step[1] not in live
            live.add(step[1])
        elif step[0] == "destroy":
            assert order[-2] == "sync"
            live.remove(step[1])
        elif step[0] == "batch":
            assert step[1] in live
            ran.append(step[2])
    assert ran == list(range(len(prog["batches"])))
    assert order == ["create", "create", "batchA1", "batchA1", "batchA1", "batchA3", "bytes", "batchB3", "create", "batchC3", "sync",
                     "destroy", "batchB3", "batchC3", "sync", "bytes"]
    assert live == {"B", "C"}
