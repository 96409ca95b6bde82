"""GPU: the host runtime around the gate kernels (iyokan_amd/csrc/iyokan_hip.hip) where no other test drives it — an arena past every
32-bit limit of `arena + (size_t)slot * (n + 1)`, per-stream buffers reallocated behind queued, unfinished batches, and batches issued
by several host threads on several streams, including the first use of the lazily built key-switch table and field key.  The cases are
tests/arena_cases.py's (checked on the CPU by tests/test_arena_cases.py); every comparison is word for word against the oracle.  Each
test initialises and cleans up the library itself."""
import os
import threading

import numpy as np
import pytest

import arena_cases as ac
from iyokan_amd import client
from iyokan_amd.params import OPS

pytestmark = pytest.mark.gpu

NTHREADS = min(16, os.cpu_count() or 1)     # the oracle's threads: what a GPU box grants a command, not the machine's CPU count


def _default_env(monkeypatch):
    for v in ("IYK_HIP_NTT", "IYK_HIP_DECOMP", "IYK_HIP_ROT_KERNEL", "IYK_HIP_LATENCY_KERNEL", "IYK_HIP_KS_KERNEL", "IYK_HIP_KS_SHARED_MAX",
              "IYK_HIP_KS_SHARED_WG", "IYK_HIP_DEBUG", "IYK_HIP_COALESCE"):
        monkeypatch.delenv(v, raising=False)


def _oracle_levels(orc, rows, levels):
    """The oracle on `levels` (run in order) over the sparse arena {slot: row}: returns {slot: row} of every slot they write."""
    used = sorted(set(rows) | {int(o) for lv in levels for o in lv["out"]})
    index = {s: i for i, s in enumerate(used)}
    remap = lambda a: np.array([index[int(s)] if s >= 0 else -1 for s in a], dtype=np.int32)
    n1 = orc.p.n + 1
    ref = np.zeros((len(used), n1), dtype=np.uint32)
    for s, r in rows.items():
        ref[index[s]] = r
    out = {}
    for lv in levels:
        orc.gate_batch(lv["ops"], remap(lv["in0"]), remap(lv["in1"]), remap(lv["in2"]), remap(lv["out"]), ref, nthreads=NTHREADS)
        out.update({int(o): ref[index[int(o)]].copy() for o in lv["out"]})
    return out


def _level(gates):
    """[(kind, in0, in1, in2, out)] -> level arrays"""
    cols = list(zip(*[(OPS[k], a, b, c, o) for k, a, b, c, o in gates]))
    return dict(zip(("ops", "in0", "in1", "in2", "out"), (np.array(c, dtype=np.int32) for c in cols)))


def _take(lv, idx):
    return {k: v[idx] for k, v in lv.items()}


def _widen(core, filler, at):
    """`core` (gates with rotations first, then NOT / COPY / CONST*) inside `filler` (gates with rotations only): the i-th core gate with a
    rotation becomes key-switch job at[i]; the rest of the core follows the last job."""
    nrot = int(np.sum(core["ops"] <= OPS["MUX"]))
    total = nrot + len(filler["ops"])
    assert len(at) == nrot and np.all(core["ops"][:nrot] <= OPS["MUX"]) and np.all(core["ops"][nrot:] > OPS["MUX"])
    pos = np.full(total, -1, dtype=np.int64)
    pos[list(at)] = np.arange(nrot)
    pos[pos < 0] = np.arange(nrot, total)
    both = {k: np.concatenate([core[k][:nrot], filler[k]])[pos] for k in core}
    return {k: np.concatenate([both[k], core[k][nrot:]]) for k in core}


def test_arena_beyond_16_gib(keys128, oracle128, monkeypatch):
    """One arena of 2^32 // 637 + 3 slots (17.18 GB), never touched but for the rows used: every entry point of the gate path reads
    and writes the chosen high slots of arena_cases.boundary_slots — both sides of byte offset 2^32, of word index 2^31 and of word
    index 2^32, and the last three slots.  A row offset cut to 32 bits anywhere lands in a low row of the same arena (arena_cases.aliases):
    in slots 0, 1, 2, which hold sentinels and must never change, or in a lower chosen slot.  After EVERY stage, before the next one
    writes, every sentinel and every chosen slot is downloaded and compared: with the sentinel rows, with the oracle's words.
      stage 1  upload / download across each limit and at each slot; upload_slots / download_slots of a permuted mix of high and low
               slots; arena_copy high -> low -> high.
      stage 2  gate_batch with inputs and outputs on the high slots, every gate kind (NOT / COPY / CONST* write and read them too), once
               per key-switch form: IYK_HIP_KS_KERNEL=0, =1 with IYK_HIP_KS_SHARED_MAX=0 (wide form), default (shared form), and =2 with
               4 097 key switches (the table kernel; the high outputs are jobs 0, 2 050 and 4 096: its first, a middle and its last
               workgroup), and =3 with 2 x 256 + 1 key switches (the matrix form, keyswitch_mfma_kernel; the high outputs are jobs 0,
               255 and 256 of the first batch and 255, 256 and 512 of the second: the first job, both sides of a workgroup boundary and
               the last job, a workgroup's only one).  The filler gates run on low slots: a 24-gate sample against the oracle, all
               against the same batch under IYK_HIP_KS_KERNEL=1.
      stage 3  blind_rotate_batch reading the high slots; bootstrap_trlwe_batch + sample_extract_keyswitch_batch writing them.
    Left out: iyk_hip_arena_sync_slots wants the same slot range on both arenas, so two such arenas; its two kernels are the ones
    upload_slots / download_slots run.  Arenas above 2^31 slots do not exist (int32 descriptors)."""
    import torch

    from iyokan_amd import hip

    _default_env(monkeypatch)
    keys, orc = keys128, oracle128
    p = keys.params
    n1, N = p.n + 1, p.N
    assert n1 == 637
    H = ac.boundary_slots(n1)
    slots = ac.arena_slots(n1)
    pairs = ac.boundary_pairs(n1)
    sent = ac.sentinel_slots(n1)
    rng = np.random.default_rng(11)
    seeds = iter(range(500, 600))
    fresh = lambda count: client.encrypt_bits(keys, rng.integers(0, 2, size=count).astype(np.uint8), seed=next(seeds))
    # low slots that hold data: none of them a sentinel
    LIN = np.arange(8) + ac.low_range(n1, 8, 3)                     # fresh inputs
    LMIX = np.arange(9) + ac.low_range(n1, 9, int(LIN[-1]) + 1)     # stage 1: the low part of the slot lists
    LCOPY = ac.low_range(n1, 5, int(LMIX[-1]) + 1)                  # stage 1: arena_copy's low range
    LOUT = np.arange(16) + ac.low_range(n1, 16, LCOPY + 5)          # stage 2: low outputs of the core gates
    FILL = ac.low_range(n1, ac.KS_TABLE_MIN, int(LOUT[-1]) + 1)     # stage 2: outputs of the filler gates
    model = {}                                                      # slot -> the words it must hold

    hip.initialize(keys, device_ids=(0,))
    st = arena = None
    try:
        st = hip.Stream(0)
        try:
            arena = hip.Arena(slots)
        except hip.IykHipError as e:
            if "out of memory" in str(e).lower():
                pytest.skip(f"hipMalloc of the {slots * n1 * 4} byte arena: {e}")
            raise

        def put(first, rows):
            rows = np.asarray(rows, dtype=np.uint32).reshape(-1, n1)
            st.upload(arena, first, rows)
            model.update({first + i: r.copy() for i, r in enumerate(rows)})

        def arm():
            for s in sent:
                st.upload(arena, s, ac.sentinel_row(s, n1))

        def check(stage, also=()):
            for s in sent:
                assert np.array_equal(st.download(arena, s, 1)[0], ac.sentinel_row(s, n1)), f"{stage}: sentinel slot {s} was written"
            for s in list(H) + [int(x) for x in also]:
                got = st.download(arena, s, 1)[0]
                assert ac.sentinel_words(got) == 0, f"{stage}: slot {s} returns sentinel words"
                assert np.array_equal(got, model[s]), f"{stage}: slot {s} differs from the reference"

        # ---- stage 1 ----
        arm()
        for _, before, _ in pairs[:2]:
            put(before, fresh(2))                                   # two rows across the limit
        put(slots - 3, fresh(3))                                    # across word 2^32, up to the arena's end
        for _, before, after in pairs:
            got = st.download(arena, before, 2)
            assert np.array_equal(got, np.stack([model[before], model[after]])), f"stage 1a: download across slot {after}"
        check("stage 1a (upload / download across each limit)")
        for s, row in zip(H, fresh(len(H))):
            put(s, row)
        check("stage 1b (upload / download, first = each high slot)")
        mix = rng.permutation(np.concatenate([H, LMIX])).astype(np.int32)
        rows = fresh(len(mix))
        st.upload_slots(arena, mix, rows)
        st.sync()
        model.update({int(s): r.copy() for s, r in zip(mix, rows)})
        check("stage 1c (upload_slots)", also=LMIX)
        mix2 = rng.permutation(mix).astype(np.int32)
        got = st.download_slots(arena, mix2)
        for s, r in zip(mix2, got):
            assert ac.sentinel_words(r) == 0, f"stage 1d (download_slots): slot {s} returns sentinel words"
            assert np.array_equal(r, model[int(s)]), f"stage 1d (download_slots): slot {s} differs"
        check("stage 1d (download_slots)", also=LMIX)
        st.arena_copy(arena, LCOPY, arena, pairs[0][1], 2)          # across byte 2^32 -> low
        st.arena_copy(arena, LCOPY + 2, arena, slots - 3, 3)        # across word 2^32 -> low
        st.sync()
        model.update({LCOPY + i: model[pairs[0][1] + i] for i in range(2)})
        model.update({LCOPY + 2 + i: model[slots - 3 + i] for i in range(3)})
        check("stage 1e (arena_copy high -> low)", also=range(LCOPY, LCOPY + 5))
        st.arena_copy(arena, pairs[1][1], arena, LCOPY + 3, 2)      # low -> across word 2^31
        st.arena_copy(arena, slots - 2, arena, LCOPY, 2)            # low -> the last two slots
        st.sync()
        model.update({pairs[1][1] + i: model[LCOPY + 3 + i] for i in range(2)})
        model.update({slots - 2 + i: model[LCOPY + i] for i in range(2)})
        check("stage 1f (arena_copy low -> high)", also=range(LCOPY, LCOPY + 5))

        # ---- stage 2 ----
        A, B = [H[0], H[2], H[4], H[6]], [H[1], H[3], H[5]]
        lo = iter(int(s) for s in LOUT)
        # X reads A (and low inputs), writes B; Y reads B, writes A; Z: NOT / COPY / CONST* onto H[1] .. H[6] (NOT in place)
        X = _level([("NAND", A[0], A[1], -1, B[0]), ("XOR", A[2], A[3], -1, B[1]), ("MUX", A[3], A[0], A[2], B[2]),
                    ("AND", A[1], LIN[0], -1, next(lo)), ("ANDNOT", A[3], A[2], -1, next(lo)), ("OR", LIN[1], A[0], -1, next(lo)),
                    ("NOR", A[2], A[1], -1, next(lo)), ("ORNOT", A[3], A[3], -1, next(lo)), ("XNOR", A[0], A[2], -1, next(lo)),
                    ("NOT", A[0], -1, -1, next(lo)), ("COPY", A[3], -1, -1, next(lo)), ("CONSTONE", -1, -1, -1, next(lo)),
                    ("CONSTZERO", -1, -1, -1, next(lo))])
        Y = _level([("ORNOT", B[0], B[1], -1, A[1]), ("XNOR", B[2], B[0], -1, A[2]), ("MUX", B[1], B[2], B[0], A[3]),
                    ("AND", B[2], B[1], -1, next(lo)), ("OR", B[0], LIN[2], -1, next(lo)), ("NOR", B[1], B[2], -1, next(lo)),
                    ("NOT", B[0], -1, -1, A[0]), ("COPY", B[1], -1, -1, next(lo))])
        Z = _level([("CONSTONE", -1, -1, -1, H[1]), ("CONSTZERO", -1, -1, -1, H[3]), ("COPY", H[0], -1, -1, H[5]),
                    ("NOT", H[2], -1, -1, H[2]), ("COPY", H[0], -1, -1, H[4]), ("NOT", H[6], -1, -1, H[6])])
        assert all(ac.independent(lv) for lv in (X, Y, Z))
        at = [0, 2050, ac.KS_TABLE_MIN - 1, 1, 2, 3, 4, 5, 6]
        fx = ac.gate_level(rng, ac.KS_TABLE_MIN - 9, np.concatenate([LIN, A]), FILL)
        fy = ac.gate_level(rng, ac.KS_TABLE_MIN - 6, np.concatenate([LIN, B]), FILL)
        X2, Y2 = _widen(X, fx, at), _widen(Y, fy, at[:6])
        assert ac.independent(X2) and ac.independent(Y2) and int(np.sum(X2["ops"] <= OPS["MUX"])) == ac.KS_TABLE_MIN
        for lv, core in ((X2, X), (Y2, Y)):                        # first, a middle and the last 128-gate workgroup of the table kernel
            ks_out = lv["out"][lv["ops"] <= OPS["MUX"]]
            assert len(ks_out) == ac.KS_TABLE_MIN and [ks_out[0], ks_out[2050], ks_out[4096]] == list(core["out"][:3])
        rng3 = np.random.default_rng(13)                           # the matrix form's fillers: their own stream, the draws above stay as they were
        at3 = {"X": list(ac.KS_MATRIX_AT["X"]) + [1, 2, 3, 4, 5, 6], "Y": list(ac.KS_MATRIX_AT["Y"]) + [0, 1, 2]}
        fx3 = ac.gate_level(rng3, ac.KS_MATRIX_EDGE - 9, np.concatenate([LIN, A]), FILL)
        fy3 = ac.gate_level(rng3, ac.KS_MATRIX_EDGE - 6, np.concatenate([LIN, B]), FILL)
        X3, Y3 = _widen(X, fx3, at3["X"]), _widen(Y, fy3, at3["Y"])
        assert ac.independent(X3) and ac.independent(Y3)
        for lv, core, name in ((X3, X, "X"), (Y3, Y, "Y")):         # job 0, jobs 255 | 256 (two workgroups), job 512 (the third's only one)
            ks_out = lv["out"][lv["ops"] <= OPS["MUX"]]
            assert len(ks_out) == ac.KS_MATRIX_EDGE and [ks_out[j] for j in ac.KS_MATRIX_AT[name]] == list(core["out"][:3])
        start = dict(zip(list(H) + [int(s) for s in LIN], fresh(len(H) + len(LIN))))
        after = {}                                                 # the oracle, once: every form starts from the same rows
        state = dict(start)
        for name, lv in (("X", X), ("Y", Y), ("Z", Z)):
            state.update(_oracle_levels(orc, state, [lv]))
            after[name] = dict(state)
        sample = rng.choice(len(fx["ops"]), size=24, replace=False)
        sample3 = rng3.choice(len(fx3["ops"]), size=24, replace=False)
        forms = [("0", None, "keyswitch_kernel", None), ("1", "0", "wave kernel, wide form", None), (None, None, "wave kernel, shared form", None),
                 ("2", None, "table kernel", {"X": (X2, fx), "Y": (Y2, fy), "sample": sample}),
                 ("3", None, "matrix form", {"X": (X3, fx3), "Y": (Y3, fy3), "sample": sample3})]
        for kernel, shared_max, what, wide in forms:
            for var, val in (("IYK_HIP_KS_KERNEL", kernel), ("IYK_HIP_KS_SHARED_MAX", shared_max)):
                monkeypatch.delenv(var, raising=False) if val is None else monkeypatch.setenv(var, val)
            for s, row in start.items():
                put(s, row)
            arm()
            for name, small in (("X", X), ("Y", Y), ("Z", Z)):
                stage = f"stage 2 ({what}, batch {name})"
                lv, fill = wide[name] if wide is not None and name in wide else (small, None)
                st.gate_batch(arena, *ac.level_args(lv))
                st.sync()
                model.update({s: after[name][s] for s in list(H) + [int(o) for o in small["out"]]})
                check(stage, also=[o for o in small["out"] if o not in H])
                if fill is not None:
                    got = st.download(arena, FILL, len(fill["ops"]))
                    monkeypatch.setenv("IYK_HIP_KS_KERNEL", "1")    # the batch writes none of its inputs: run again, same rows
                    st.gate_batch(arena, *ac.level_args(lv))
                    st.sync()
                    monkeypatch.setenv("IYK_HIP_KS_KERNEL", kernel)
                    assert np.array_equal(got, st.download(arena, FILL, len(fill["ops"]))), f"{stage}: filler gates differ from IYK_HIP_KS_KERNEL=1"
                    # the fillers read the low inputs and A (batch X) or B as X left it (batch Y): the rows after X hold both
                    ref = _oracle_levels(orc, {s: after["X"][s] for s in list(H) + [int(x) for x in LIN]}, [_take(fill, wide["sample"])])
                    for o, r in ref.items():
                        assert np.array_equal(got[o - FILL], r), f"{stage}: filler gate writing slot {o} differs from the oracle"
                    check(stage + ", after the second run", also=[o for o in small["out"] if o not in H])
        monkeypatch.delenv("IYK_HIP_KS_KERNEL", raising=False)
        monkeypatch.delenv("IYK_HIP_KS_SHARED_MAX", raising=False)

        # ---- stage 3 ----
        for s, row in zip(H, fresh(len(H))):
            put(s, row)
        arm()
        mu = int(p.mu)
        ib = np.array([H[1], H[0], -1, H[2], H[6], -1, H[5]], dtype=np.int32)
        sa = np.where(ib >= 0, -1, 1).astype(np.int32)
        sb = np.where(ib >= 0, -1, 0).astype(np.int32)
        off = np.where(ib >= 0, mu, 0).astype(np.uint32)
        out = torch.zeros((len(H), N + 1), dtype=torch.int32, device="cuda")
        trl = torch.zeros((len(H), 2 * N), dtype=torch.int32, device="cuda")
        torch.cuda.synchronize()
        st.blind_rotate_batch(arena, H, ib, sa, sb, off, out.data_ptr())
        st.sync()
        got = out.cpu().numpy().view(np.uint32)
        for j, s in enumerate(H):
            lin = model[s].copy() if ib[j] < 0 else (np.uint32(0) - model[s] - model[int(ib[j])]).astype(np.uint32)
            lin[-1] = np.uint32((int(lin[-1]) + int(off[j])) & 0xFFFFFFFF)
            assert np.array_equal(got[j], orc.bootstrap_lvl1(lin)), f"stage 3a (blind_rotate_batch): job {j} reading slot {s}"
        check("stage 3a (blind_rotate_batch)")
        nxt = [H[(j + 1) % len(H)] for j in range(len(H))]         # NAND(H[j], H[j + 1]) -> H[j], the gate in its two halves
        ones = np.full(len(H), -1, dtype=np.int32)
        st.bootstrap_trlwe_batch(arena, H, nxt, ones, ones, np.full(len(H), mu, dtype=np.uint32), trl.data_ptr(), trlwe_slots=len(H))
        st.sample_extract_keyswitch_batch(trl.data_ptr(), np.arange(len(H)), H, arena, trlwe_slots=len(H))
        st.sync()
        model.update({s: orc.gate(OPS["NAND"], model[s], model[t]) for s, t in zip(H, nxt)})
        check("stage 3b (bootstrap_trlwe_batch + sample_extract_keyswitch_batch)")
    finally:
        if arena is not None:
            arena.free()
        if st is not None:
            st.destroy()
        hip.cleanup()


def _growth_case(which, request, monkeypatch, ks_kernel=None):
    """arena_cases.growth_program on one stream with nothing that synchronises between the first upload and the last download, under
    IYK_HIP_KS_KERNEL=ks_kernel (None: unset), and its three assertions: the whole arena equals the oracle's, the download_slots rows
    equal the same rows of the final download, every bit decrypts right."""
    from iyokan_amd import hip

    _default_env(monkeypatch)
    if ks_kernel is not None:
        monkeypatch.setenv("IYK_HIP_KS_KERNEL", ks_kernel)
    keys = request.getfixturevalue("keys" + which)
    orc = request.getfixturevalue("oracle" + which)
    n1 = keys.params.n + 1
    prog = ac.growth_program(np.random.default_rng(5))
    assert ac.growth_points(prog, n1) == ([0, 1, 3], [0, 1, 4])
    inputs = client.encrypt_bits(keys, prog["bits"], seed=71)
    uploads = {k: client.encrypt_bits(keys, s[2], seed=72 + k) for k, s in enumerate(prog["steps"]) if s[0] == "upload_slots"}
    hip.initialize(keys, device_ids=(0,))
    st = arena = None
    try:
        st = hip.Stream(0)
        arena = hip.Arena(prog["slots"])
        st.upload(arena, 0, inputs)                                 # synchronises: the last time before the downloads
        for k, step in enumerate(prog["steps"]):
            if step[0] == "gates":
                st.gate_batch(arena, *ac.level_args(step[1]))
            else:
                st.upload_slots(arena, step[1], uploads[k])
        final = st.download_slots(arena, prog["final"])             # queued behind all of it
        got = st.download(arena, 0, prog["slots"])
    finally:
        if arena is not None:
            arena.free()
        if st is not None:
            st.destroy()
        hip.cleanup()
    ref = np.zeros((prog["slots"], n1), dtype=np.uint32)
    ref[:ac.GROWTH_INPUTS] = inputs
    for k, step in enumerate(prog["steps"]):
        if step[0] == "gates":
            orc.gate_batch(*ac.level_args(step[1]), ref, nthreads=NTHREADS)
        else:
            ref[step[1]] = uploads[k]
    bad = np.flatnonzero((got != ref).any(axis=1))
    assert bad.size == 0, f"slots that differ from the oracle: {bad[:10]} ... ({bad.size})"
    assert np.array_equal(final, got[prog["final"]])
    assert np.array_equal(client.decrypt_bits(keys, got), ac.simulate_growth(prog).astype(np.uint8))


@pytest.mark.parametrize("which", ["128", "80"])
def test_buffers_grow_behind_queued_batches(which, request, monkeypatch):
    """One stream, nothing that synchronises between the first upload and the last download: arena_cases.growth_program queues 2 gates
    (which leave a 4 352-byte staging slot and 67 rotation rows), 200 gates (both buffers are reallocated while the 2 gates may still
    run), 1 gate, upload_slots of 300 rows (staging reallocated again), 700 gates that read those rows (rotation buffer reallocated
    again), ten batches of 1 - 3 gates (the ring of eight staging slots wraps after the growths) and a download_slots behind all of it
    — each step reading what the step before wrote.  tests/test_arena_cases.py derives the reallocations from the growth policy.  The
    whole arena equals the oracle's, the download_slots rows equal the same rows of the final download, every bit decrypts right."""
    _growth_case(which, request, monkeypatch)


def _join(threads, what):
    for t in threads:
        t.start()
    for t in threads:
        t.join(timeout=120)
        assert not t.is_alive(), f"{what}: a host thread never came back"


def _run_thread_programs(hip, keys, progs, inputs, concurrent, monkeypatch):
    """Phase 1: every program's five levels and its blind_rotate_batch; phase 2, under IYK_HIP_ROT_KERNEL=w32: the 70-gate levels.
    concurrent: one host thread and one stream per program, released together, no synchronisation until a thread's last call (phase 2:
    programs 0 and 1 at once, then program 2).  Otherwise one stream, one thread, a sync after every call.
    Returns (arena, rotation outputs per program, resident key bytes before / after phase 1 / after phase 2)."""
    import torch

    P = progs["programs"]
    N = keys.params.N
    errors = []
    arena = hip.Arena(progs["slots"])
    streams = []
    try:
        main = hip.Stream(0)
        streams.append(main)
        main.upload(arena, 0, inputs)
        bufs = [torch.zeros((len(pr["rotate"][0]), N + 1), dtype=torch.int32, device="cuda") for pr in P]
        torch.cuda.synchronize()
        key_bytes = [hip.resident_key_bytes()]

        def guarded(f):
            def run():
                try:
                    f()
                except BaseException as e:   # noqa: BLE001 - reported on the main thread
                    errors.append(repr(e))
            return threading.Thread(target=run)

        def phase1(st, pr, buf, each):
            for lv in pr["levels"]:
                st.gate_batch(arena, *ac.level_args(lv))
                if each:
                    st.sync()
            st.blind_rotate_batch(arena, *pr["rotate"], buf.data_ptr())
            st.sync()

        def phase2(st, pr):
            st.gate_batch(arena, *ac.level_args(pr["field"]))
            st.sync()

        if concurrent:
            mine = [None] * len(P)
            barrier = threading.Barrier(len(P))

            def worker(t):
                mine[t] = hip.Stream(0)
                barrier.wait(timeout=60)
                phase1(mine[t], P[t], bufs[t], False)

            try:
                _join([guarded(lambda t=t: worker(t)) for t in range(len(P))], "phase 1")
            finally:
                streams.extend(s for s in mine if s is not None)
            assert not errors, errors
            key_bytes.append(hip.resident_key_bytes())
            monkeypatch.setenv("IYK_HIP_ROT_KERNEL", "w32")
            barrier2 = threading.Barrier(2)

            def worker2(t):
                barrier2.wait(timeout=60)
                phase2(mine[t], P[t])

            _join([guarded(lambda t=t: worker2(t)) for t in range(2)], "phase 2")
            assert not errors, errors
            for t in range(2, len(P)):
                phase2(mine[t], P[t])
        else:
            for pr, buf in zip(P, bufs):
                phase1(main, pr, buf, True)
            key_bytes.append(hip.resident_key_bytes())
            monkeypatch.setenv("IYK_HIP_ROT_KERNEL", "w32")
            for pr in P:
                phase2(main, pr)
        monkeypatch.delenv("IYK_HIP_ROT_KERNEL")
        key_bytes.append(hip.resident_key_bytes())
        got = main.download(arena, 0, progs["slots"])
        rot = [b.cpu().numpy().view(np.uint32).copy() for b in bufs]
        return got, rot, key_bytes
    finally:
        monkeypatch.delenv("IYK_HIP_ROT_KERNEL", raising=False)
        arena.free()
        for s in streams:
            s.destroy()


def test_concurrent_streams_from_host_threads(keys128, oracle128, monkeypatch):
    """Three host threads, a stream each, one arena (disjoint slot ranges, common read-only inputs), released together right after a
    fresh iyk_hip_init and never synchronised until a thread's last call.  Each runs arena_cases.thread_programs: 3 gates; a full round
    + 150 gates (both rotation kernels, the second from job `round` on); 1 gate; 4 097 gates — every thread's FIRST wide batch, so the
    key-switch table is first asked for by three threads at once; 17 gates; a blind_rotate_batch into a torch buffer; NOT / COPY in the
    two wide levels.  Then, under IYK_HIP_ROT_KERNEL=w32, two threads send a 70-gate level at once: the first use of the field key,
    which the FFT path builds lazily.
    The reference is the same programs on one stream from one thread with a sync after every call, after an initialisation of its own
    (the configuration the rest of the suite pins to the oracle): identical arenas and rotation outputs.  The oracle itself on every
    3-gate level and on 24 gates of each wide level that read the common inputs; every bit decrypts to the plaintext simulation.
    iyk_hip_resident_key_bytes grows by the table in phase 1 and by the field key in phase 2, exactly as in the serial run — it reports
    sizes, not allocations, so a table built twice would show in the arenas or as a fault, not in this figure."""
    from iyokan_amd import hip

    _default_env(monkeypatch)
    keys, orc = keys128, oracle128
    n1 = keys.params.n + 1
    runs = {}
    progs = inputs = None
    for concurrent in (True, False):                                # the concurrent run is the first thing after its initialisation
        hip.initialize(keys, device_ids=(0,))
        try:
            assert hip.ntt_path() == "fft"
            if progs is None:
                progs = ac.thread_programs(np.random.default_rng(6), 3, rotation_round=hip.rotation_round())
                inputs = client.encrypt_bits(keys, progs["bits"], seed=61)
            runs[concurrent] = _run_thread_programs(hip, keys, progs, inputs, concurrent, monkeypatch)
        finally:
            hip.cleanup()
    (got, rot, kb), (serial, serial_rot, serial_kb) = runs[True], runs[False]
    lo = ac.THREAD_INPUTS
    bad = np.flatnonzero((got[lo:] != serial[lo:]).any(axis=1)) + lo
    assert bad.size == 0, f"slots that differ from the serial run: {bad[:10]} ... ({bad.size})"
    assert np.array_equal(got[:lo], inputs)
    assert all(np.array_equal(a, b) for a, b in zip(rot, serial_rot))
    table, field = kb[1] - kb[0], kb[2] - kb[1]
    assert table > 100e6 and field > 50e6 and kb == serial_kb, (kb, serial_kb)
    rng = np.random.default_rng(7)
    checked = []
    for pr in progs["programs"]:
        checked.append(pr["levels"][0])
        for lv in (pr["levels"][1], pr["levels"][3]):
            checked.append(_take(lv, np.sort(rng.choice(ac.FRESH_GATES, size=24, replace=False))))
    ref = np.zeros((progs["slots"], n1), dtype=np.uint32)
    ref[:lo] = inputs
    for lv in checked:
        orc.gate_batch(*ac.level_args(lv), ref, nthreads=NTHREADS)
        assert np.array_equal(got[lv["out"]], ref[lv["out"]])
    assert np.array_equal(client.decrypt_bits(keys, got), ac.simulate_threads(progs).astype(np.uint8))
