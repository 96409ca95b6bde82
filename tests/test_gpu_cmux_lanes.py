"""GPU: CMUX memories per lane — the four iyk_hip_cmux_*_batch_lanes calls (cmux_lane_jobs_kernel in front of the unchanged CMUX kernels)
and cmux.Rom / cmux.Ram with lanes.

The four calls: the whole TRLWE store, word for word, against ONE parent call with the host-replicated arrays of
tests/cmux_lane_cases.py on a copy of the same store (random rows: the CMUX product is exact on any words); rows no lane's job writes —
the canary rows between the lanes where row_stride is larger than the span, and behind the last lane — come back as uploaded.
Rom / Ram: lane r's arena words, result rows and cells equal a one-lane memory fed lane r's image and selectors."""
import ctypes

import numpy as np
import pytest

import cmux_lane_cases as cc
import cmux_tree_cases as tree_cases
import memory_cases
from iyokan_amd import client, cmux

pytestmark = pytest.mark.gpu

SEL_OFF = 8      # the cases' selector slots moved behind the zero and all-0 runs of the 32-slot store of tests/cmux_tree_cases.py
BEHIND = 3       # canary rows behind the last lane


@pytest.fixture(scope="module")
def gpu(keys128):
    from iyokan_amd import hip

    hip.initialize(keys128, device_ids=(0,))
    yield hip, keys128
    hip.cleanup()


@pytest.fixture(scope="module")
def store(gpu):
    hip, keys = gpu
    st = hip.Stream(0)
    sel = hip.Trgsw(tree_cases.SLOTS)
    sel.upload(st, 0, tree_cases.selectors(keys))
    st.sync()
    yield st, sel
    sel.free()
    st.destroy()


def _moved(c):
    """the case with its selector slots + SEL_OFF"""
    arrays = tuple(a + SEL_OFF if i in cc.SEL_ARRAYS[c["family"]] else a for i, a in enumerate(c["arrays"]))
    assert cc.reach(c["family"], arrays)[0] + (c["lanes"] - 1) * c["sel_stride"] < tree_cases.SLOTS
    return dict(c, arrays=arrays)


def _rows(keys, c, tag):
    rng = np.random.default_rng([11, 0x6F, tag])
    return rng.integers(0, 1 << 32, size=(c["trlwe_slots"] + BEHIND, 2 * keys.params.N), dtype=np.uint64).astype(np.uint32)


def _call(st, sel, trl, family, arrays, **kw):
    getattr(st, cc.FAMILY_NAME[family])(sel, trl, *arrays, **kw)


def _written(c):
    """the rows the jobs of all lanes write"""
    out = np.asarray(c["arrays"][-1], dtype=np.int64)
    return sorted({int(o) + r * c["row_stride"] for r in range(c["lanes"]) for o in out})


GPU_CASES = ["cmux3-x3", "cmux3-wide-stride", "tree41-x2", "chain-ram21-x2", "rot31-x2", "37x7", "rot-37x7", "cmux3-x1", "chain-ram21-x1", "rot31-x1",
             "tree41-x1", "cmux-stage-major", "chain-stage-major", "rot-stage-major", "tree-stage-major"]


@pytest.mark.parametrize("name", GPU_CASES)
def test_lanes_call_equals_one_parent_call_on_replicated_arrays(gpu, store, name):
    hip, keys = gpu
    st, sel = store
    c = _moved(cc.CASES[name])
    T = _rows(keys, c, GPU_CASES.index(name))
    a, b = hip.Trlwe(T.shape[0]), hip.Trlwe(T.shape[0])
    try:
        a.upload(st, 0, T)
        b.upload(st, 0, T)
        _call(st, sel, a, c["family"], c["arrays"], lanes=c["lanes"], sel_stride=c["sel_stride"], row_stride=c["row_stride"])
        _call(st, sel, b, c["family"], cc.replicate(c["family"], c["arrays"], c["lanes"], c["sel_stride"], c["row_stride"]))
        st.sync()
        got, want = a.download(st, 0, T.shape[0]), b.download(st, 0, T.shape[0])
    finally:
        a.free()
        b.free()
    bad = np.flatnonzero((got != want).any(axis=1))
    assert bad.size == 0, f"{name}: rows that differ from the parent call's: {bad[:10]}"
    written = _written(c)
    untouched = [r for r in range(T.shape[0]) if r not in set(written)]
    assert len(untouched) >= BEHIND and np.array_equal(got[untouched], T[untouched])          # canaries between and behind the lanes
    assert (got[written] != T[written]).any(axis=1).all()                                      # and every job of every lane did run


def test_two_laned_batches_on_one_stream_the_second_growing_the_scratch(gpu, store):
    """a fresh stream: 6 expanded jobs, then 259 — more than the first allocation holds — queued behind it without a sync"""
    hip, keys = gpu
    _, sel = store
    st = hip.Stream(0)
    small, large = _moved(cc.CASES["cmux3-x2"]), _moved(cc.CASES["37x7"])
    assert 6 * 20 * 3 // 2 + 4096 < 259 * 20
    stores = []
    try:
        for i, c in enumerate((small, large)):
            T = _rows(keys, c, 100 + i)
            a, b = hip.Trlwe(T.shape[0]), hip.Trlwe(T.shape[0])
            stores.append((c, T, a, b))
            a.upload(st, 0, T)
            b.upload(st, 0, T)
        for c, T, a, b in stores:
            _call(st, sel, a, c["family"], c["arrays"], lanes=c["lanes"], sel_stride=c["sel_stride"], row_stride=c["row_stride"])
        for c, T, a, b in stores:
            _call(st, sel, b, c["family"], cc.replicate(c["family"], c["arrays"], c["lanes"], c["sel_stride"], c["row_stride"]))
        st.sync()
        for c, T, a, b in stores:
            got = a.download(st, 0, T.shape[0])
            assert np.array_equal(got, b.download(st, 0, T.shape[0])) and not np.array_equal(got, T)
    finally:
        for _, _, a, b in stores:
            a.free()
            b.free()
        st.destroy()


def test_refusals_leave_the_store_unchanged(gpu):
    """every refusal of tests/cmux_lane_cases.py whose stated stores fit 64 slots and 64 rows, through the C ABI: IYK_ERR_INVALID with its
    text, nothing staged or launched — the rows come back as uploaded"""
    hip, keys = gpu
    L = hip.lib()
    st = hip.Stream(0)
    sel, trl = hip.Trgsw(64), hip.Trlwe(64)
    rng = np.random.default_rng([11, 0x6F, 200])
    T = rng.integers(0, 1 << 32, size=(64, 2 * keys.params.N), dtype=np.uint64).astype(np.uint32)
    tried = 0
    try:
        trl.upload(st, 0, T)
        for name, family, arrays, trgsw_slots, trlwe_slots, lanes, sel_stride, row_stride, word in cc.REFUSALS:
            if name == "count-x-lanes-one-more":   # its stores are stated far larger than these; the cap is refused before a store is looked at,
                trgsw_slots, trlwe_slots = 64, 64   # so honest sizes give the same refusal (4 096 jobs x 4 097 lanes)
            assert trgsw_slots <= 64 and trlwe_slots <= 64, name
            f = getattr(L, "iyk_hip_" + cc.FAMILY_NAME[family] + "_lanes")
            arrs = [np.ascontiguousarray(a, dtype=np.int32) for a in arrays]
            ptrs = [a.ctypes.data_as(t) for a, t in zip(arrs, f.argtypes[6:6 + len(arrs)])]
            rc = f(st.h, sel.ptr, trgsw_slots, trl.ptr, trlwe_slots, len(arrs[0]), *ptrs, lanes, sel_stride, row_stride)
            assert rc == -1 and word in L.iyk_hip_last_error().decode(), (name, rc, L.iyk_hip_last_error())
            tried += 1
        with pytest.raises(hip.IykHipError, match="span row_stride"):
            st.cmux_batch(sel, trl, *cc.CMUX3, lanes=2, sel_stride=3, row_stride=6)
        st.sync()
        assert tried == len(cc.REFUSALS) and np.array_equal(trl.download(st, 0, 64), T)
    finally:
        sel.free()
        trl.free()
        st.destroy()


# ---- the plain entry point is the lanes == 1 case of the laned one's body, each with its own checker ------------------------------------

@pytest.mark.parametrize("name", ["cmux3-x1", "chain-ram21-x1", "rot31-x1", "tree41-x1"])
def test_plain_call_and_lanes_call_with_one_lane_give_the_same_words(gpu, store, name):
    """iyk_hip_<kernel> against iyk_hip_<kernel>_lanes with lanes = 1 (the strides given, so Stream._cmux_call takes the laned symbol), on
    copies of one store: the same words in every row"""
    hip, keys = gpu
    st, sel = store
    c = _moved(cc.CASES[name])
    T = _rows(keys, c, 500 + GPU_CASES.index(name))
    a, b = hip.Trlwe(T.shape[0]), hip.Trlwe(T.shape[0])
    try:
        a.upload(st, 0, T)
        b.upload(st, 0, T)
        _call(st, sel, a, c["family"], c["arrays"])
        _call(st, sel, b, c["family"], c["arrays"], lanes=1, sel_stride=c["sel_stride"], row_stride=c["row_stride"])
        st.sync()
        plain, laned = a.download(st, 0, T.shape[0]), b.download(st, 0, T.shape[0])
    finally:
        a.free()
        b.free()
    assert np.array_equal(plain, laned)
    written = _written(c)
    assert (plain[written] != T[written]).any(axis=1).all()                                    # every job did run


def test_gate_batch_and_gate_batch_lanes_with_one_lane_give_the_same_words(gpu):
    """four gates, a NOT (elementwise) and a MUX (two rotations) among them, on random arena words (the gates are exact functions of any
    words): iyk_hip_gate_batch against iyk_hip_gate_batch_lanes with lanes = 1 and the arena as the one lane"""
    from iyokan_amd.params import OPS

    hip, keys = gpu
    ops, in0, in1, in2, out = [OPS["NAND"], OPS["NOT"], OPS["MUX"], OPS["XOR"]], [0, 1, 2, 5], [1, -1, 3, 6], [-1, -1, 4, -1], [7, 8, 9, 10]
    rows = np.random.default_rng([11, 0x6F, 600]).integers(0, 1 << 32, size=(12, keys.params.n + 1), dtype=np.uint64).astype(np.uint32)
    st = hip.Stream(0)
    a, b = hip.Arena(len(rows)), hip.Arena(len(rows))
    try:
        st.upload(a, 0, rows)
        st.upload(b, 0, rows)
        st.gate_batch(a, ops, in0, in1, in2, out)
        st.gate_batch(b, ops, in0, in1, in2, out, lanes=1, lane_stride=b.slots)
        st.sync()
        plain, laned = st.download(a, 0, len(rows)), st.download(b, 0, len(rows))
    finally:
        a.free()
        b.free()
        st.destroy()
    assert np.array_equal(plain, laned)
    assert (plain[out] != rows[out]).any(axis=1).all() and np.array_equal(plain[:7], rows[:7]) and np.array_equal(plain[11], rows[11])


def test_too_many_jobs_each_entry_point_refuses_in_its_own_checkers_words(gpu):
    """2^24 + 1 jobs (np.zeros arrays: pages nobody touches — the count is refused before a job is read or anything is staged): the plain
    call answers with check_cmux_batch's text, the laned call with lanes = 1 with cmux_batch_lanes_args'; the store stays as uploaded"""
    hip, keys = gpu
    count = (1 << 24) + 1
    z = np.zeros(count, dtype=np.int32)
    st = hip.Stream(0)
    sel, trl = hip.Trgsw(4), hip.Trlwe(8)
    T = np.random.default_rng([11, 0x6F, 700]).integers(0, 1 << 32, size=(8, 2 * keys.params.N), dtype=np.uint64).astype(np.uint32)
    try:
        trl.upload(st, 0, T)
        with pytest.raises(hip.IykHipError) as plain:
            st.cmux_batch(sel, trl, z, z, z, z, z)
        with pytest.raises(hip.IykHipError) as laned:
            st.cmux_batch(sel, trl, z, z, z, z, z, lanes=1, sel_stride=1, row_stride=1)
        st.sync()
        assert "batch too large" in str(plain.value) and "count x lanes" not in str(plain.value)
        assert "batch too large: count x lanes" in str(laned.value)
        assert np.array_equal(trl.download(st, 0, 8), T)
    finally:
        sel.free()
        trl.free()
        st.destroy()


# ---- Rom / Ram with two lanes-------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("fused", [False, True], ids=["unfused", "fused"])
def test_rom_two_lanes_equal_one_lane_roms(gpu, fused):
    """two reads per lane of a ROM with a two-level upper tree and a rotate tail; lane 1 holds another image (the rows rolled) and reads
    other addresses: arena words and result rows of lane r equal a one-lane ROM with lane r's image and selectors"""
    hip, keys = gpu
    aw, lw = 9, 3
    wb = 1 << lw
    bits, data, addresses, trgsw = memory_cases.rom_case(keys, aw, lw)
    images = [data, np.roll(data, 1, axis=0)]
    slots = np.arange(2 * wb).reshape(2, wb)
    stride = 2 * wb + 3
    want = []
    for lane in range(2):
        st = hip.Stream(0)
        rom, arena = cmux.Rom(st, images[lane], aw, lw, max_reads=2), hip.Arena(2 * wb)
        try:
            rom.read(trgsw[2 * lane: 2 * lane + 2], arena, slots, fused=fused, fused_tree=fused)
            st.sync()
            want.append((st.download(arena, 0, 2 * wb), np.stack([rom.trlwe.download(st, rom.row(r, rom.layout.result), 1)[0] for r in range(2)])))
        finally:
            arena.free()
            rom.free()
            st.destroy()
    st = hip.Stream(0)
    rom, arena = cmux.Rom(st, np.concatenate(images), aw, lw, max_reads=2, lanes=2, arena_stride=stride), hip.Arena(2 * stride)
    try:
        rom.read(trgsw, arena, slots, fused=fused, fused_tree=fused)
        st.sync()
        for lane in range(2):
            assert np.array_equal(st.download(arena, lane * stride, 2 * wb), want[lane][0]), lane
            rows = np.stack([rom.trlwe.download(st, lane * rom.row_stride + rom.row(r, rom.layout.result), 1)[0] for r in range(2)])
            assert np.array_equal(rows, want[lane][1]), lane
    finally:
        arena.free()
        rom.free()
        st.destroy()
    assert not np.array_equal(want[0][0], want[1][0])
    assert np.array_equal(client.decrypt_bits(keys, want[0][0]).reshape(2, wb), np.stack([bits[a * wb: (a + 1) * wb] for a in addresses[:2]]))


@pytest.mark.parametrize("fused", [False, True], ids=["unfused", "fused"])
def test_ram_two_lanes_equal_one_lane_rams(gpu, fused):
    """one clock of a 32 x 2 RAM per lane, the lanes with their own cells, address, wren and wdata: rdata TLWEs and every cell row of
    lane r after the clock equal a one-lane RAM's"""
    hip, keys = gpu
    p = keys.params
    aw, dw = 5, 2
    C = 1 << aw
    rng = np.random.default_rng([11, 0x6F, 300])
    lanes = []
    for lane in range(2):
        content = rng.integers(0, 2, size=dw * C).astype(np.uint8)
        addr = int(rng.integers(0, C))
        lanes.append(dict(cells=client.encrypt_ram_trlwe(keys, content, seed=80 + lane).reshape(dw * C, 2 * p.N),
                          sel=np.ascontiguousarray(client.encrypt_trgsw(keys, [(addr >> k) & 1 for k in range(aw)], seed=90 + lane), dtype=np.uint32),
                          tlwe=client.encrypt_bits(keys, np.array([1, lane, 1 - lane], dtype=np.uint8), seed=95 + lane)))   # wren, wdata
    wren, wdata, rdata = 0, [1, 2], [3, 4]
    stride = 7
    want = []
    for ln in lanes:
        st = hip.Stream(0)
        ram, arena = cmux.Ram(st, ln["cells"], aw, dw), hip.Arena(5)
        try:
            st.upload(arena, 0, ln["tlwe"])
            ram.clock(ln["sel"], arena, wren, wdata, rdata, fused=fused, fused_tree=fused)
            st.sync()
            want.append((st.download(arena, 3, 2), ram.cells()))
        finally:
            arena.free()
            ram.free()
            st.destroy()
    st = hip.Stream(0)
    ram = cmux.Ram(st, np.concatenate([ln["cells"] for ln in lanes]), aw, dw, lanes=2, arena_stride=stride)
    arena = hip.Arena(2 * stride)
    try:
        for lane, ln in enumerate(lanes):
            st.upload(arena, lane * stride, ln["tlwe"])
        ram.clock(np.stack([ln["sel"].reshape(aw, -1) for ln in lanes]), arena, wren, wdata, rdata, fused=fused, fused_tree=fused)
        st.sync()
        for lane in range(2):
            assert np.array_equal(st.download(arena, lane * stride + 3, 2), want[lane][0]), lane
            assert np.array_equal(ram.cells(lane), want[lane][1]), lane
    finally:
        arena.free()
        ram.free()
        st.destroy()
    assert not np.array_equal(want[0][1], want[1][1])


def test_ram_two_lanes_refresh_aside_equals_one_stream(gpu):
    """write_port(refresh_stream=) of a laned RAM: the refresh of all lanes' cells on a second stream — the cells of both lanes after
    read_port + write_port equal the one-stream form's"""
    hip, keys = gpu
    p = keys.params
    aw, dw, stride = 3, 2, 7
    C = 1 << aw
    rng = np.random.default_rng([11, 0x6F, 400])
    cells = [client.encrypt_ram_trlwe(keys, rng.integers(0, 2, size=dw * C).astype(np.uint8), seed=120 + r).reshape(dw * C, 2 * p.N) for r in range(2)]
    sel = np.stack([np.ascontiguousarray(client.encrypt_trgsw(keys, [(a >> k) & 1 for k in range(aw)], seed=130 + a), dtype=np.uint32).reshape(aw, -1)
                    for a in (5, 2)])
    tlwe = [client.encrypt_bits(keys, np.array([1, r, 1 - r], dtype=np.uint8), seed=140 + r) for r in range(2)]
    got = {}
    for aside in (False, True):
        st, second = hip.Stream(0), hip.Stream(0)
        ram, arena = cmux.Ram(st, np.concatenate(cells), aw, dw, lanes=2, arena_stride=stride), hip.Arena(2 * stride)
        try:
            for r in range(2):
                st.upload(arena, r * stride, tlwe[r])
                ram.trgsw.upload(st, r * ram.sel_stride, sel[r])
            ram.read_port(arena, [3, 4])
            ram.write_port(arena, 0, [1, 2], [3, 4], **({"refresh_stream": second} if aside else {}))
            got[aside] = [ram.cells(r) for r in range(2)]
        finally:
            arena.free()
            ram.free()
            second.destroy()
            st.destroy()
    assert all(np.array_equal(a, b) for a, b in zip(got[True], got[False])) and not np.array_equal(got[True][0], got[True][1])


# ---- CmuxLaneEngine, K = 2, against one-lane CmuxCipherEngines ---------------------------------------------------------------------------

@pytest.fixture(scope="module")
def keyed(gpu, tmp_path_factory):
    """the real bk2 and the uniform private key-switching key of tests/test_gpu_cmux_system.py, and section 6e's small system"""
    import cb_rotate_cases
    import cmux_system_cases as small
    from iyokan_amd.system import load_blueprint

    hip, keys = gpu
    st = hip.Stream(0)
    p = keys.params
    bk = client.bk2_rows(keys, client.keygen_lvl2(cb_rotate_cases.N2, seed=31), 4, 9, cb_rotate_cases.ALPHA2, seed=32)
    bk2 = hip.Bk2Key(p.n)
    for first in range(0, p.n, 200):
        bk2.upload(st, first, bk[first:first + 200])
    pk = hip.PrivKsKey(cb_rotate_cases.N2, 1, 1)
    pk.upload(st, 0, np.random.default_rng(92).integers(0, 1 << 32, size=(pk.rows, pk.words), dtype=np.uint64).astype(np.uint32))
    st.sync()
    sysm = load_blueprint(small.write_blueprint(str(tmp_path_factory.mktemp("cmux_lanes_system"))), cmux_memories=True)
    yield bk2, pk, sysm, small
    bk2.free()
    pk.free()
    st.destroy()


def _engine(keys, sysm, bk2, pk, packets, lanes, **kw):
    import torch

    from iyokan_amd import runner
    from iyokan_amd.frontier import FrontierExecutor, FrontierPlan, HipBackend

    plan = FrontierPlan(sysm.nl, 1, stages=sysm.stages)
    be = HipBackend(plan.num_slots, keys.params, torch.device("cuda", 0), **({"lanes": lanes} if lanes > 1 else {}))
    # the same bits give the same ciphertext in every engine and lane: word equality needs equal inputs
    encrypt = lambda bits: client.encrypt_bits(keys, bits, seed=9000 + sum(int(b) << i for i, b in enumerate(bits)) % 4096 + 4096 * len(bits))
    common = (sysm, FrontierExecutor(plan, be), encrypt, lambda rows: client.decrypt_bits(keys, rows), client.trivial(keys.params, 0), bk2, pk)
    try:
        if lanes > 1:
            eng = runner.CmuxLaneEngine(*common, packets=packets, **kw)
        else:
            eng = runner.CmuxCipherEngine(*common, packet=packets[0], **kw)
    except Exception:
        be.close()                                                                  # a refusal leaves no stream behind
        raise
    return eng, be, plan


@pytest.mark.parametrize("flags", [{}, dict(stage_cb=True, refresh_aside=True)], ids=["flags-off", "stage_cb+refresh_aside"])
def test_lane_engine_two_clocks_equal_one_lane_engines(gpu, keyed, flags):
    """two clocks of run_packets on CmuxLaneEngine, K = 2: every arena row of lane r (rdata TLWEs among them) and every RAM cell equal,
    word for word, a one-lane CmuxCipherEngine given the same input ciphertexts and images.  No decryption: the one-lane engine is
    decrypt-tested (tests/test_gpu_cmux_system.py), and word equality carries it."""
    from iyokan_amd import runner
    from iyokan_amd.packet import TFHEPacket

    hip, keys = gpu
    bk2, pk, sysm, small = keyed
    reqs = [small.request(21, 2), small.request(22, 2)]
    packets = [TFHEPacket.encrypt(keys, r, seed=800 + i) for i, r in enumerate(reqs)]
    dummy = lambda rows: [0] * len(rows)
    want = []
    for r in range(2):
        eng, be, plan = _engine(keys, sysm, bk2, pk, [packets[r]], 1, decrypt_ram=dummy, **flags)
        try:
            runner.run_packet(sysm, reqs[r], engine=eng)
            want.append((be.read_many(list(range(plan.num_slots))), eng.ram_rows("ram")))
        finally:
            eng.free()
            be.close()
    eng, be, plan = _engine(keys, sysm, bk2, pk, packets, 2, decrypt_ram=dummy, **flags)
    try:
        runner.run_packets(sysm, reqs, engine=eng)
        for r in range(2):
            assert np.array_equal(be.read_many(list(range(plan.num_slots)), lane=r), want[r][0]), r
            assert np.array_equal(eng.ram_rows("ram", lane=r), want[r][1]), r
    finally:
        eng.free()
        be.close()
    assert not np.array_equal(want[0][1], want[1][1])
