"""The chosen cases of tests/arena_cases.py are what tests/test_gpu_gate_edges.py takes them for: slots on both sides of every 32-bit
limit, alias slots that a truncated offset really lands in, programs that keep the independence contract and grow the buffers where
the GPU test says they do.  No GPU."""
import numpy as np
import pytest

import arena_cases as ac
from iyokan_amd.params import OPS, params_128bit, params_80bit

N1 = [params_128bit().n + 1, params_80bit().n + 1]


def test_the_figures_of_the_128_bit_set():
    n1 = 637
    assert ac.arena_slots(n1) == 6_742_494 and ac.arena_slots(n1) * n1 * 4 > 17.17e9
    assert [(b, a) for _, b, a in ac.boundary_pairs(n1)] == [(1_685_622, 1_685_623), (3_371_245, 3_371_246), (6_742_491, 6_742_492)]
    assert ac.boundary_slots(n1) == [1_685_622, 1_685_623, 3_371_245, 3_371_246, 6_742_491, 6_742_492, 6_742_493]


@pytest.mark.parametrize("n1", N1)
def test_boundary_pairs_straddle_their_limits(n1):
    slots = ac.arena_slots(n1)
    assert slots <= 1 << 31                                   # what iyk_hip_arena_alloc and the int32 descriptors admit
    for words, before, after in ac.boundary_pairs(n1):
        assert after == before + 1 and after < slots
        assert before * n1 < words <= after * n1              # `before` starts below the limit, `after` at or above it
        assert (before + 1) * n1 >= words                     # and nothing lies between them
    byte_pair, w31, w32 = ac.boundary_pairs(n1)
    assert byte_pair[1] * n1 * 4 < 1 << 32 <= byte_pair[2] * n1 * 4
    chosen = ac.boundary_slots(n1)
    assert chosen == sorted(set(chosen)) and chosen[-3:] == [slots - 3, slots - 2, slots - 1]
    assert (slots - 1) * n1 >= 1 << 32 and slots * n1 * 4 < 17.2e9


@pytest.mark.parametrize("n1", N1)
def test_aliases_are_where_truncation_lands_and_are_watched(n1):
    """Every slot a truncated offset lands in is lower than the slot it stands for and is either a sentinel slot — below the first
    chosen slot, never used for data — or another chosen slot, whose content the GPU test compares after every stage.  (The limits
    are powers of two, so the slot just below one limit aliases the slot just below a lower one, and every slot just above a limit
    aliases slots 0 and 1: the aliases cannot all be distinct from the chosen slots and from each other.)"""
    chosen = ac.boundary_slots(n1)
    sent = ac.sentinel_slots(n1)
    assert set(sent).isdisjoint(chosen) and max(sent) < chosen[0] and sent[:3] == [0, 1, 2] and len(sent) <= 4
    for h in chosen:
        al = ac.aliases(h, n1)
        # the slot below the byte limit is the control: nothing truncates it; every slot from the byte limit on has an alias
        assert bool(al) == (h * n1 * 4 >= 1 << 32)
        for name, (a, b) in al.items():
            w = (h * n1) % ac.TRUNCATIONS[name]
            assert a * n1 <= w < (a + 1) * n1 and b == a + 1 and w + n1 <= (b + 1) * n1    # starts in a, ends in a or b
            assert 0 <= a and b < h
            assert all(s in sent or s in chosen for s in (a, b))
    # byte truncation moves every slot from the byte limit on; the word truncations only those past their limit
    assert set(ac.aliases(chosen[-1], n1)) == set(ac.TRUNCATIONS)
    assert set(ac.aliases(ac.boundary_pairs(n1)[0][2], n1)) == {"bytes mod 2^32"}
    assert set(ac.aliases(ac.boundary_pairs(n1)[1][2], n1)) == {"bytes mod 2^32", "words mod 2^31"}
    # every slot past a limit has at least one alias among the sentinels
    for _, _, after in ac.boundary_pairs(n1):
        assert any(a in sent for pair in ac.aliases(after, n1).values() for a in pair)


@pytest.mark.parametrize("n1", N1)
def test_sentinels_are_recognisable(n1):
    rng = np.random.default_rng(3)
    sent = ac.sentinel_slots(n1)
    chosen = ac.boundary_slots(n1)
    rows = {s: ac.sentinel_row(s, n1) for s in sent}
    assert all(r.dtype == np.uint32 and r.shape == (n1,) and np.all(r >> 24 == 0xA5) for r in rows.values())
    assert all(not np.array_equal(rows[a], rows[b]) for i, a in enumerate(sent) for b in sent[i + 1:])
    assert all(ac.sentinel_words(r) == n1 - 1 for r in rows.values())
    uniform = rng.integers(0, 1 << 32, size=(200, n1), dtype=np.uint64).astype(np.uint32)
    trivial = np.zeros(n1, dtype=np.uint32)
    trivial[-1] = 1 << 29
    assert all(ac.sentinel_words(r) == 0 for r in uniform) and ac.sentinel_words(trivial) == 0
    # a flat model of the arena: sentinels in their slots, uniform words in the chosen slots; a read through a truncated offset
    # that touches a sentinel slot returns a run of sentinel words
    image = {s: rows[s] for s in sent}
    image.update({s: uniform[i] for i, s in enumerate(chosen)})
    for h in chosen:
        for name, (a, b) in ac.aliases(h, n1).items():
            two = np.concatenate([image[a], image[b]])
            off = (h * n1) % ac.TRUNCATIONS[name] - a * n1
            got = two[off:off + n1]
            want = max(0, n1 - off - 1) * (a in sent) + max(0, off - 1) * (b in sent)
            assert ac.sentinel_words(got) == want and not np.array_equal(got, image[h])
    for count, start in ((4200, 3), (16, 0), (3, chosen[0] - 1)):
        lo = ac.low_range(n1, count, start)
        assert lo >= start and not set(range(lo, lo + count)) & (set(sent) | set(chosen))


def test_key_switch_thresholds_mirror_the_library():
    """KS_TABLE_MIN and the matrix form's workgroup are the library's (csrc/dispatch.hpp through libiyk_emul.so), and the jobs the
    huge-arena test gives its high outputs under the matrix form are the first, both sides of a workgroup boundary, and the last."""
    import ctypes
    import os

    import ks_words as K

    em = ctypes.CDLL(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "iyokan_amd", "lib", "libiyk_emul.so"))
    assert ac.KS_TABLE_MIN == K.TABLE_MIN_JOBS + 1 < em.iyk_emul_ks_matrix_min_jobs()
    assert ac.KS_MATRIX_GROUP == em.iyk_emul_ks_matrix_gates(0) and ac.KS_MATRIX_EDGE == 513
    for t, nc in ((7, 5), (8, 4)):
        assert K.ks_geometry("2", None, ac.KS_TABLE_MIN, t, 256)[0] == "table" and K.ks_geometry("2", None, ac.KS_TABLE_MIN - 1, t, 256)[0] != "table"
    at = ac.KS_MATRIX_AT
    assert set(at["X"]) | set(at["Y"]) == {0, 255, 256, 512} and all(len(v) == 3 and max(v) < ac.KS_MATRIX_EDGE for v in at.values())
    assert {j // ac.KS_MATRIX_GROUP for v in at.values() for j in v} == {0, 1, 2}
    assert -(-ac.KS_MATRIX_EDGE // ac.KS_MATRIX_GROUP) == 3 and ac.KS_MATRIX_EDGE % ac.KS_MATRIX_GROUP == 1


def _levels_of_growth(prog):
    return [s[1] for s in prog["steps"] if s[0] == "gates"]


def test_growth_program_contract_and_simulation():
    prog = ac.growth_program(np.random.default_rng(5))
    kinds = [s[0] for s in prog["steps"]]
    assert kinds == ["gates"] * 3 + ["upload_slots", "gates"] + ["gates"] * 10
    sizes = [len(s[1]["ops"]) if s[0] == "gates" else len(s[1]) for s in prog["steps"]]
    assert tuple(sizes[:5]) == ac.GROWTH_SIZES and tuple(sizes[5:]) == ac.GROWTH_TAIL and len(sizes[5:]) > ac.STAGE_RING
    written = set(range(ac.GROWTH_INPUTS))
    prev = set(written)
    for step in prog["steps"]:
        if step[0] == "upload_slots":
            assert not written & set(step[1].tolist()) and len(set(step[1].tolist())) == len(step[1])   # nothing in flight reads them
            written |= set(step[1].tolist())
            uploaded = set(step[1].tolist())
            continue
        lv = step[1]
        assert ac.independent(lv)
        ins = {s for _, s in ac.inputs_of(lv)}
        assert ins <= written and not set(lv["out"].tolist()) & written      # reads what exists, writes fresh slots
        assert ins & prev                                                     # depends on the step before it
        written |= set(lv["out"].tolist())
        prev = set(lv["out"].tolist())
    big = prog["steps"][4][1]
    assert {s for _, s in ac.inputs_of(big)} & uploaded                       # the 700-gate level reads uploaded rows
    assert {int(o) for o in big["ops"]} >= {OPS["MUX"], OPS["NOT"], OPS["COPY"]}
    assert written == set(range(prog["slots"]))
    bits = ac.simulate_growth(prog)
    assert set(np.unique(bits)) <= {0, 1}                                     # every slot written, nothing read before it exists
    assert np.array_equal(bits, ac.simulate_growth(prog))
    assert set(prog["final"].tolist()) <= written and set(prev) <= set(prog["final"].tolist())
    again = ac.growth_program(np.random.default_rng(5))
    assert all(np.array_equal(a[k], b[k]) for a, b in zip(_levels_of_growth(prog), _levels_of_growth(again)) for k in a)


@pytest.mark.parametrize("n1", N1)
def test_growth_program_grows_where_the_gpu_test_says(n1):
    """Under the growth policy of ensure_stage / ensure_rot as mirrored in arena_cases: the first call leaves a 4 352-byte staging slot
    and 67 rotation rows; the 200-gate level outgrows both; the 300 uploaded rows outgrow staging again, the 700-gate level the
    rotation buffer again; nothing else reallocates — and more than a ring of calls follows the last growth."""
    prog = ac.growth_program(np.random.default_rng(5))
    first = prog["steps"][0][1]
    assert ac.stage_cap_after(ac.gate_batch_stage_bytes(first)) == 4352 and ac.rot_cap_after(ac.rotations(first)) == 67
    assert ac.growth_points(prog, n1) == ([0, 1, 3], [0, 1, 4])
    assert len(prog["steps"]) - 1 - 4 > ac.STAGE_RING


def test_thread_programs_contract_and_simulation():
    R = 2048
    progs = ac.thread_programs(np.random.default_rng(6), 3, rotation_round=R)
    assert len(progs["programs"]) == 3
    common = set(range(ac.THREAD_INPUTS))
    ranges = [pr["range"] for pr in progs["programs"]]
    assert ranges[0][0] == ac.THREAD_INPUTS and all(a[1] == b[0] for a, b in zip(ranges, ranges[1:])) and ranges[-1][1] == progs["slots"]
    for pr in progs["programs"]:
        lo, hi = pr["range"]
        own = set()
        sizes = []
        for lv in pr["levels"] + [pr["field"]]:
            assert ac.independent(lv)
            outs = set(lv["out"].tolist())
            ins = {s for _, s in ac.inputs_of(lv)}
            assert all(lo <= o < hi for o in outs) and not outs & own         # writes its own range only, fresh slots
            assert ins <= common | own                                         # reads the common inputs and its own earlier outputs
            own |= outs
            sizes.append((len(lv["ops"]), ac.rotations(lv)))
        assert own == set(range(lo, hi))
        assert [r for _, r in sizes] == [sizes[0][1], R + 150, 1, ac.KS_TABLE_MIN, sizes[4][1], sizes[5][1]]
        assert [n for n, _ in sizes][0::2] == [3, 1, 17] and sizes[5][0] == 70
        assert sizes[1][0] > R + 150 and sizes[3][0] > ac.KS_TABLE_MIN        # NOT / COPY mixed into the two wide levels
        for lv in (pr["levels"][1], pr["levels"][3]):
            assert {s for g, s in ac.inputs_of(lv) if g < ac.FRESH_GATES} <= common
            assert not np.any(lv["ops"] == OPS["MUX"])
        ia, ib, sa, sb, off = pr["rotate"]
        assert len(ia) == len(ib) == len(sa) == len(sb) == len(off) == 8
        assert set(ia.tolist()) | {s for s in ib.tolist() if s >= 0} <= own and np.all(sb[ib < 0] == 0)
    bits = ac.simulate_threads(progs)
    assert set(np.unique(bits)) <= {0, 1}
    assert np.array_equal(bits, ac.simulate_threads(progs))
    # every thread's bits depend on the common inputs alone: a thread's program replayed alone gives the same bits
    for pr in progs["programs"]:
        alone = np.full(progs["slots"], -1, dtype=np.int8)
        alone[:ac.THREAD_INPUTS] = progs["bits"]
        for lv in pr["levels"] + [pr["field"]]:
            ac.simulate_level(lv, alone)
        lo, hi = pr["range"]
        assert np.array_equal(alone[lo:hi], bits[lo:hi])
