"""GPU: the matrix form of the key switch (keyswitch_mfma_kernel) against the CPU oracle, and the host runtime of its operand
(ensure_ks_matrix) at its edges.  The cases are tests/ks_matrix_cases.py's (checked on the CPU by tests/test_ks_matrix_cases.py);
every comparison is word for word on uint32: key-switch cases against orc_sample_extract0 + orc_keyswitch, gate cases against
orc.gate_batch; IYK_HIP_KS_KERNEL=1 stands beside the oracle only as an all-rows cross-check.  The operand's size is derived (4 N t
columns x nc 128 words x 4 planes), not measured.  Each test initialises and cleans up the library itself."""
import contextlib
import ctypes
import os
import threading

import numpy as np
import pytest

import arena_cases as ac
import ks_matrix_cases as M
import ks_words as K
import oracle_lib
import test_gpu_gate_edges as GE
from iyokan_amd import client
from iyokan_amd.params import params_128bit
from test_gpu_keyswitch import FILL, _check_case, _reference, _run_case, _u32p
from test_gpu_keyswitch_matrix import ENV, _emul

pytestmark = pytest.mark.gpu

NCELLS = 640
NTHREADS = min(16, os.cpu_count() or 1)
CAP = "IYK_HIP_KS_MATRIX_MAX_BYTES"
KIND = "IYK_HIP_KS_KERNEL"


def _clear_env(monkeypatch):
    for v in ENV:
        monkeypatch.delenv(v, raising=False)


def _operand(p, which):
    """Bytes of the operand: the literal, the formula and the library's own figure."""
    size = M.OPERAND_BYTES[which]
    assert size == M.operand_bytes(p) == _emul().iyk_emul_ks_matrix_bytes(p.t, M.nc_of(p))
    return size


def _pool_used(hip):
    """Bytes this process holds in GPU 0's stream-ordered memory pool, where the operand lives (hipMallocAsync)."""
    L = hip.lib()
    pool, used = ctypes.c_void_p(), ctypes.c_uint64()
    assert L.hipDeviceGetMemPool(ctypes.byref(pool), 0) == 0
    assert L.hipMemPoolGetAttribute(pool, 7, ctypes.byref(used)) == 0    # hipMemPoolAttrUsedMemCurrent
    return used.value


@contextlib.contextmanager
def _trlwe(hip, st, cells, gpu=0):
    """The cells in a TRLWE buffer of `gpu`, uploaded on `st`: its device pointer."""
    L = hip.lib()
    d = ctypes.c_void_p()
    assert L.iyk_hip_trlwe_alloc(gpu, len(cells), ctypes.byref(d)) == 0
    try:
        assert L.iyk_hip_trlwe_upload(st.h, d, len(cells), 0, len(cells), cells.ctypes.data_as(_u32p)) == 0
        st.sync()
        yield d.value
    finally:
        assert L.iyk_hip_trlwe_free(gpu, d) == 0


def _cells_and_ref(orc, seed, ncells=NCELLS):
    cells, nnamed, nspecial, _ = M.cells(orc.p, seed, ncells)
    return cells, nnamed, nspecial, _reference(orc, cells)


def _batch(hip, st, d_trlwe, ref, nspecial, rng, what, jobs=M.BATCH_JOBS):
    """One key-switch batch of `jobs` jobs (every named and chosen cell in it) on `st`, every word against `ref`."""
    idx = K.job_layout(jobs, list(range(nspecial)), len(ref), rng)
    got, out_slot = _run_case(hip, st, d_trlwe, len(ref), idx, hip.current_params(), rng)
    _check_case(got, out_slot, idx, ref, nspecial, what)
    return got, out_slot, idx


@pytest.mark.parametrize("which", ["128", "80"])
def test_matrix_form_equals_the_oracle(which, request, monkeypatch):
    """IYK_HIP_KS_KERNEL=3 against the oracle, under the ordinary key and under carry_keys (rows of 0x80 / 0x7F bytes: the signed planes
    exist in this form only): each named cell alone; the digit sweep as one batch (a wrong slot names the digit that was misplaced);
    the position sweep (a distinctive cell on every accumulator row of every wave, in two whole workgroups and a ragged third); 2 x 256
    + 1 jobs with every named and chosen cell at the first job, at the last and across the middle.  Every word of every written slot,
    and the fill of every slot no job wrote."""
    from iyokan_amd import hip

    keys0 = request.getfixturevalue("keys" + which)
    p = keys0.params
    _clear_env(monkeypatch)
    size = _operand(p, which)
    rng = np.random.default_rng(1000 + int(which))
    total = 2600
    cells, nnamed, nspecial, _ = M.cells(p, 20 + int(which), total)
    sweep, digits = M.digit_sweep(p, rng)
    pos, pos_idx = M.position_sweep(p, rng)
    s0, p0 = nspecial, nspecial + len(sweep)
    assert p0 + len(pos) < total - 300
    cells[s0:p0], cells[p0:p0 + len(pos)] = sweep, pos
    carry = M.carry_keys(keys0)
    orc_carry = oracle_lib.Oracle(carry)
    try:
        for name, keys, orc in (("ordinary key", keys0, request.getfixturevalue("oracle" + which)), ("carrying key", carry, orc_carry)):
            ref = _reference(orc, cells)
            hip.initialize(keys, device_ids=(0,))
            try:
                st = hip.Stream(0)
                try:
                    with _trlwe(hip, st, cells) as d:
                        bare = hip.resident_key_bytes()
                        monkeypatch.setenv(KIND, "3")
                        what = f"t={p.t}, {name}: "
                        for c in range(nnamed):
                            idx = np.array([c], dtype=np.int32)
                            got, out_slot = _run_case(hip, st, d, total, idx, p, rng)
                            _check_case(got, out_slot, idx, ref, nspecial, what + f"the cell '{M.NAMED[c]}' alone")
                        assert hip.resident_key_bytes() - bare == size
                        idx = np.arange(s0, p0, dtype=np.int32)
                        got, out_slot = _run_case(hip, st, d, total, idx, p, rng)
                        bad = np.flatnonzero((got[out_slot] != ref[idx]).any(axis=1))
                        assert bad.size == 0, what + f"digit sweep: {bad.size} cells differ; (i, j, v) of the first: {digits[bad[:12]].tolist()}"
                        _check_case(got, out_slot, idx, ref, nspecial, what + "digit sweep")
                        idx = (p0 + pos_idx).astype(np.int32)
                        got, out_slot = _run_case(hip, st, d, total, idx, p, rng)
                        bad = np.flatnonzero((got[out_slot] != ref[idx]).any(axis=1))
                        assert bad.size == 0, what + f"position sweep: jobs {bad[:12].tolist()} differ ({bad.size}); job = 256 workgroup + 64 wave + row"
                        _check_case(got, out_slot, idx, ref, nspecial, what + "position sweep")
                        idx = K.job_layout(2 * M.GATES + 1, list(range(nspecial)), total, rng)
                        got, out_slot = _run_case(hip, st, d, total, idx, p, rng)
                        _check_case(got, out_slot, idx, ref, nspecial, what + f"{len(idx)} jobs")
                        assert hip.resident_key_bytes() - bare == size
                finally:
                    st.destroy()
            finally:
                hip.cleanup()
    finally:
        orc_carry.close()


@pytest.mark.parametrize("which", ["128", "80"])
def test_gate_batch_through_the_matrix_form(which, request, monkeypatch):
    """ks_matrix_cases.gate_levels — 2 x 256 + 37 gates with rotations, MUX gates (a second rotation row, off = mu) at the first and
    last job of every wave and at the last job of the ragged workgroup, every binary kind beside them, NOT / COPY / CONST behind —
    under IYK_HIP_KS_KERNEL=3: all of it equals kind 1, the MUX jobs, their neighbours and the gates without a rotation equal
    orc.gate_batch, every output decrypts to the plaintext simulation, the three rows behind the outputs keep their fill."""
    from iyokan_amd import hip

    keys = request.getfixturevalue("keys" + which)
    orc = request.getfixturevalue("oracle" + which)
    p = keys.params
    _clear_env(monkeypatch)
    size = _operand(p, which)
    nin = 16
    rng = np.random.default_rng(2000 + int(which))
    lv = M.gate_levels(rng, nin)
    ng = len(lv["ops"])
    bits = rng.integers(0, 2, size=nin).astype(np.uint8)
    host = np.zeros((nin + ng + 3, p.n + 1), dtype=np.uint32)
    host[:nin] = client.encrypt_bits(keys, bits, seed=2100 + int(which))
    host[nin + ng:] = FILL
    res = {}
    hip.initialize(keys, device_ids=(0,))
    try:
        st = hip.Stream(0)
        try:
            bare = hip.resident_key_bytes()
            for kind in ("3", "1"):
                monkeypatch.setenv(KIND, kind)
                arena = hip.Arena(host.shape[0])
                try:
                    st.upload(arena, 0, host)
                    st.gate_batch(arena, *ac.level_args(lv))
                    st.sync()
                    res[kind] = st.download(arena, 0, host.shape[0])
                finally:
                    arena.free()
            assert hip.resident_key_bytes() - bare == size
        finally:
            st.destroy()
    finally:
        hip.cleanup()
    bad = np.flatnonzero((res["3"] != res["1"]).any(axis=1))
    assert bad.size == 0, f"slots that differ from IYK_HIP_KS_KERNEL=1: {bad[:10].tolist()} ({bad.size}); gate = slot - {nin}"
    assert (res["3"][nin + ng:] == FILL).all() and np.array_equal(res["3"][:nin], host[:nin])
    sample = M.oracle_sample()
    ref = host.copy()
    orc.gate_batch(*ac.level_args(GE._take(lv, sample)), ref, nthreads=NTHREADS)
    outs = lv["out"][sample]
    bad = sample[(res["3"][outs] != ref[outs]).any(axis=1)]
    assert bad.size == 0, f"gates that differ from the oracle: {bad.tolist()} (MUX jobs: {M.mux_jobs()})"
    plain = np.full(nin + ng, -1, dtype=np.int8)
    plain[:nin] = bits
    ac.simulate_level(lv, plain)
    assert np.array_equal(client.decrypt_bits(keys, res["3"][:nin + ng]), plain.astype(np.uint8))


def test_default_dispatch_boundary(keys128, oracle128, monkeypatch):
    """IYK_HIP_KS_KERNEL unset: 4 607 jobs run the table (the resident bytes grow by the table only), 4 608 the matrix form (by the
    operand's 73 400 320 more).  The words of both equal kind 1 on every row and the oracle on every row."""
    from iyokan_amd import hip

    p = keys128.params
    _clear_env(monkeypatch)
    size = _operand(p, "128")
    assert size == 73_400_320
    cells, _, nspecial, ref = _cells_and_ref(oracle128, 31)
    rng = np.random.default_rng(3000)
    hip.initialize(keys128, device_ids=(0,))
    try:
        st = hip.Stream(0)
        try:
            with _trlwe(hip, st, cells) as d:
                bare = hip.resident_key_bytes()
                for n, grown in ((M.MIN_JOBS - 1, K.table_bytes(p)), (M.MIN_JOBS, K.table_bytes(p) + size)):
                    idx = K.job_layout(n, list(range(nspecial)), NCELLS, rng)
                    monkeypatch.delenv(KIND, raising=False)
                    got, out_slot = _run_case(hip, st, d, NCELLS, idx, p, np.random.default_rng(n))
                    assert hip.resident_key_bytes() - bare == grown, n
                    monkeypatch.setenv(KIND, "1")
                    wave, _ = _run_case(hip, st, d, NCELLS, idx, p, np.random.default_rng(n))
                    assert hip.resident_key_bytes() - bare == grown, n
                    bad = np.flatnonzero((got != wave).any(axis=1))
                    assert bad.size == 0, f"{n} jobs, default dispatch: slots {bad[:10].tolist()} differ from IYK_HIP_KS_KERNEL=1 ({bad.size})"
                    _check_case(got, out_slot, idx, ref, nspecial, f"{n} jobs, default dispatch")
        finally:
            st.destroy()
    finally:
        hip.cleanup()


def _ks(st, d, batch, arena):
    st.sample_extract_keyswitch_batch(d, batch[0], batch[1], arena, trlwe_slots=NCELLS)


def _differing(got, want):
    bad = np.flatnonzero((got != want).any(axis=1))
    return f"slots that differ from the oracle: {bad[:10].tolist()} ({bad.size} of {len(got)})"


def test_first_use_from_three_host_threads(keys128, monkeypatch):
    """Right after a fresh initialisation three host threads create a stream each, meet at a barrier and run two batches of 300 jobs
    under IYK_HIP_KS_KERNEL=3 into disjoint slot ranges of one arena, with no sync between the two and one at the end: one of them
    builds the operand, the others wait for its event.  The arena equals the oracle's, the resident bytes grew by one operand.  The
    key is ks_matrix_cases.salted_keys': no operand an earlier test left in device memory is the right one."""
    from iyokan_amd import hip

    keys = M.salted_keys(keys128, 4)
    p = keys.params
    _clear_env(monkeypatch)
    size = _operand(p, "128")
    orc = oracle_lib.Oracle(keys)
    try:
        cells, _, nspecial, ref = _cells_and_ref(orc, 41)
    finally:
        orc.close()
    prog = M.first_use_program(np.random.default_rng(4000), list(range(nspecial)), NCELLS)
    want = M.expected_arena(prog, ref, FILL)
    monkeypatch.setenv(KIND, "3")
    errors, mine = [], [None] * len(prog["threads"])
    barrier = threading.Barrier(len(mine))
    hip.initialize(keys, device_ids=(0,))
    main = arena = None
    try:
        main = hip.Stream(0)
        arena = hip.Arena(prog["slots"])
        main.upload(arena, 0, np.full((prog["slots"], p.n + 1), FILL, dtype=np.uint32))
        with _trlwe(hip, main, cells) as d:
            bare = hip.resident_key_bytes()

            def worker(t):
                try:
                    mine[t] = hip.Stream(0)
                    barrier.wait(timeout=60)
                    for b in prog["threads"][t]:
                        _ks(mine[t], d, prog["batches"][b], arena)
                    mine[t].sync()
                except BaseException as e:   # noqa: BLE001 - reported on the main thread
                    errors.append(repr(e))

            GE._join([threading.Thread(target=worker, args=(t,)) for t in range(len(mine))], "first use of the operand")
            assert not errors, errors
            assert hip.resident_key_bytes() - bare == size
            got = main.download(arena, 0, prog["slots"])
    finally:
        for s in mine + [main]:
            if s is not None:
                s.destroy()
        if arena is not None:
            arena.free()
        hip.cleanup()
    assert np.array_equal(got, want), _differing(got, want)


def test_streams_behind_the_build(keys128, monkeypatch):
    """ks_matrix_cases.STREAM_STEPS: stream A queues three batches on the wave kernel and then its first batch of the matrix form, so
    the operand's build waits on A behind them; with no sync B runs a batch (it must wait for the build's event); C is created after
    the build and runs one; everything syncs, A is destroyed, B and C run again.  All eight outputs equal the oracle, and the resident
    bytes are bare + one operand from A's batch on.  Salted key, as above."""
    from iyokan_amd import hip

    keys = M.salted_keys(keys128, 5)
    p = keys.params
    _clear_env(monkeypatch)
    size = _operand(p, "128")
    orc = oracle_lib.Oracle(keys)
    try:
        cells, _, nspecial, ref = _cells_and_ref(orc, 51)
    finally:
        orc.close()
    prog = M.stream_program(np.random.default_rng(5000), list(range(nspecial)), NCELLS)
    want = M.expected_arena(prog, ref, FILL)
    streams, seen = {}, {}
    hip.initialize(keys, device_ids=(0,))
    main = arena = None
    try:
        main = hip.Stream(0)
        arena = hip.Arena(prog["slots"])
        main.upload(arena, 0, np.full((prog["slots"], p.n + 1), FILL, dtype=np.uint32))
        with _trlwe(hip, main, cells) as d:
            bare = hip.resident_key_bytes()
            for step in prog["steps"]:
                if step[0] == "create":
                    streams[step[1]] = hip.Stream(0)
                elif step[0] == "batch":
                    monkeypatch.setenv(KIND, step[3])
                    _ks(streams[step[1]], d, prog["batches"][step[2]], arena)
                elif step[0] == "bytes":
                    seen[step[1]] = hip.resident_key_bytes() - bare
                elif step[0] == "sync":
                    for s in streams.values():
                        s.sync()
                else:
                    streams.pop(step[1]).destroy()
            got = main.download(arena, 0, prog["slots"])
    finally:
        for s in list(streams.values()) + [main]:
            if s is not None:
                s.destroy()
        if arena is not None:
            arena.free()
        hip.cleanup()
    assert seen == {"first": size, "last": size}
    assert np.array_equal(got, want), _differing(got, want)


def test_operand_follows_key_and_parameter_set(keys128, oracle128, keys80, oracle80, monkeypatch):
    """Seed-1 keys, a batch under IYK_HIP_KS_KERNEL=3: bare + 73 400 320 bytes.  cleanup, seed-2 keys: bare bytes again, the batch equals
    the seed-2 oracle and differs from the seed-1 words on more than half the rows (rows whose digits are all 0 are (0, .., 0, b)
    under any key).  cleanup, the 80-bit keys: the batch equals the 80-bit oracle, the bytes grow by 67 108 864.  After every cleanup
    the process holds no more of the device's stream-ordered pool, where the operand lives, than before the first initialisation."""
    from iyokan_amd import hip

    _clear_env(monkeypatch)
    keys2 = client.keygen(params_128bit(), seed=2)
    orc2 = oracle_lib.Oracle(keys2)
    try:
        cells, _, nspecial, ref1 = _cells_and_ref(oracle128, 61)
        ref2 = _reference(orc2, cells)
    finally:
        orc2.close()
    cells80, _, nspecial80, ref80 = _cells_and_ref(oracle80, 62)
    assert (_operand(keys128.params, "128"), _operand(keys80.params, "80")) == (73_400_320, 67_108_864)
    monkeypatch.setenv(KIND, "3")
    pool0 = _pool_used(hip)
    bare = {}
    for name, keys, c, nsp, ref, size in (("seed 1", keys128, cells, nspecial, ref1, 73_400_320), ("seed 2", keys2, cells, nspecial, ref2, 73_400_320),
                                          ("80-bit", keys80, cells80, nspecial80, ref80, 67_108_864)):
        hip.initialize(keys, device_ids=(0,))
        try:
            bare[name] = hip.resident_key_bytes()
            st = hip.Stream(0)
            try:
                with _trlwe(hip, st, c) as d:
                    got, out_slot, idx = _batch(hip, st, d, ref, nsp, np.random.default_rng(6000), name)
                    assert hip.resident_key_bytes() == bare[name] + size, name
                    if name == "seed 2":
                        differ = (got[out_slot] != ref1[idx]).any(axis=1)
                        key_free = (ref1[idx] == ref2[idx]).all(axis=1)
                        assert (differ | key_free).all() and differ.sum() > len(idx) // 2
            finally:
                st.destroy()
        finally:
            hip.cleanup()
        held = _pool_used(hip)
        print(f"{name}: stream-ordered pool bytes in use after cleanup: {held} (before the first initialisation: {pool0})")
        assert held <= pool0, f"{name}: {held - pool0} bytes of the stream-ordered pool outlive cleanup (an operand is {size})"
    assert bare["seed 2"] == bare["seed 1"]


def test_operand_cap_boundary_and_memory(keys128, oracle128, monkeypatch):
    """IYK_HIP_KS_MATRIX_MAX_BYTES equal to the operand's size: built.  Re-initialised with the cap one byte lower: not built, and the
    batch runs ks_plan's form.  The variable removed: still not built — the device remembers the refusal until it is initialised
    again.  cleanup + initialize: built.  Every step's words equal the oracle's; the stream-ordered pool is given back every time."""
    from iyokan_amd import hip

    p = keys128.params
    _clear_env(monkeypatch)
    size = _operand(p, "128")
    cells, _, nspecial, ref = _cells_and_ref(oracle128, 71)
    rng = np.random.default_rng(7000)
    monkeypatch.setenv(KIND, "3")
    pool0 = _pool_used(hip)
    # (the variable before each batch of this initialisation (None: removed), the operand is resident after the batch)
    rounds = [[(str(size), True)], [(str(size - 1), False), (None, False)], [(None, True)]]
    for k, batches in enumerate(rounds):
        hip.initialize(keys128, device_ids=(0,))
        try:
            st = hip.Stream(0)
            try:
                with _trlwe(hip, st, cells) as d:
                    bare = hip.resident_key_bytes()
                    for cap, built in batches:
                        monkeypatch.delenv(CAP, raising=False) if cap is None else monkeypatch.setenv(CAP, cap)
                        _batch(hip, st, d, ref, nspecial, rng, f"initialisation {k}, {CAP}={cap}")
                        assert hip.resident_key_bytes() - bare == (size if built else 0), (k, cap)
                        assert _pool_used(hip) - pool0 >= (size if built else 0), (k, cap)
            finally:
                st.destroy()
        finally:
            hip.cleanup()
        assert _pool_used(hip) <= pool0, f"initialisation {k}: the stream-ordered pool is not given back"
    monkeypatch.delenv(CAP, raising=False)


def test_two_replicas_one_device(keys128, oracle128, monkeypatch):
    """initialize(keys, device_ids=(0, 0)): replica 1's stream runs a batch under IYK_HIP_KS_KERNEL=3 first — the resident bytes grow
    by one operand —, then replica 0's: the figure is unchanged (it counts the operand once, like the table).  Both outputs equal the
    oracle; cleanup succeeds and the next initialisation reports the bare bytes."""
    from iyokan_amd import hip

    p = keys128.params
    _clear_env(monkeypatch)
    size = _operand(p, "128")
    cells, _, nspecial, ref = _cells_and_ref(oracle128, 81)
    rng = np.random.default_rng(8000)
    idx = K.job_layout(M.BATCH_JOBS, list(range(nspecial)), NCELLS, rng)
    out_slot = rng.permutation(M.BATCH_JOBS + 37)[:M.BATCH_JOBS].astype(np.int32)
    want = np.full((M.BATCH_JOBS + 37, p.n + 1), FILL, dtype=np.uint32)
    want[out_slot] = ref[idx]
    monkeypatch.setenv(KIND, "3")
    hip.initialize(keys128, device_ids=(0, 0))
    try:
        bare = hip.resident_key_bytes()
        sts = [hip.Stream(0), hip.Stream(1)]
        arenas = []
        try:
            with _trlwe(hip, sts[0], cells, 0) as d0, _trlwe(hip, sts[1], cells, 1) as d1:
                for g in (0, 1):
                    arenas.append(hip.Arena(len(want), gpu_index=g))
                    sts[g].upload(arenas[g], 0, np.full_like(want, FILL))
                for g, d in ((1, d1), (0, d0)):
                    _ks(sts[g], d, (idx, out_slot), arenas[g])
                    sts[g].sync()
                    assert hip.resident_key_bytes() - bare == size, f"after replica {g}'s batch"
                    got = sts[g].download(arenas[g], 0, len(want))
                    assert np.array_equal(got, want), f"replica {g}: " + _differing(got, want)
        finally:
            for a in arenas:
                a.free()
            for s in sts:
                s.destroy()
    finally:
        hip.cleanup()
    hip.initialize(keys128, device_ids=(0,))
    try:
        assert hip.resident_key_bytes() == bare
    finally:
        hip.cleanup()


@pytest.mark.parametrize("which", ["128", "80"])
def test_rotation_buffer_grows_behind_queued_matrix_batches(which, request, monkeypatch):
    """arena_cases.growth_program exactly as test_gpu_gate_edges.test_buffers_grow_behind_queued_batches runs it, under
    IYK_HIP_KS_KERNEL=3: keyswitch_mfma_kernel reads the stream's rotation buffer while later batches of the queue reallocate it.  The
    same three assertions: whole arena == oracle, download_slots rows == final download, every bit decrypts."""
    _clear_env(monkeypatch)
    GE._growth_case(which, request, monkeypatch, ks_kernel="3")
