"""CPU: selectors at a base slot of a shared store (cmux.Rom / cmux.Ram(trgsw=, sel_base=)), one circuit bootstrapping per stage
(runner.CmuxCipherEngine(stage_cb=True)), the RAM refresh on a second stream (refresh_aside=True, Ram.write_port(refresh_stream=...)) and
the argument check of iyk_hip_stream_wait_stream — all on recording streams: every call is logged as (stream, name, arguments), a
wait_stream as an ordering edge, and the happens-before relation of a recording is program order per stream plus those edges.

Buffers are attributed per STORE (a RAM's TRLWE store is its cell rows with its scratch rows, its private arena is a store, the engine's
arena, lvl2 store, TRLWE scratch and selector store are one each): coarser than rows and therefore stricter.  The four-port system is
tests/cmux_stage_cases.py; the default engine's recording is held as a digest taken from the commit before the feature."""
import ctypes
import hashlib
import json

import numpy as np
import pytest

import batch_refusal_cases as brc
import cmux_ref
import cmux_stage_cases as cases
import cmux_system_cases as small
import ram_ref
from iyokan_amd import cmux, runner
from iyokan_amd.frontier import FrontierExecutor, FrontierPlan
from iyokan_amd.params import params_128bit
from iyokan_amd.system import load_blueprint

P = params_128bit()
N, L, PER = int(P.N), int(P.l), int(P.trgsw_rows)
# where a call names its selector store and its selector indices
SEL_POS = {"cmux_batch": 2, "cmux_tree_batch": 2, "cmux_rotate_chain_batch": 3, "cmux_chain_batch": 2}
# the recording of 3 clocks of the four-port system with the default engine, taken from the commit before the feature (_digest below)
PARENT_DIGEST = "9a62a2de39dbc56200630bc8a844b227dd6e4f2a5d3dbd289a08c003f8a6a8bc"


def _selectors(name, args):
    """every selector slot a recorded call reads"""
    if name in ("cmux_chain_batch", "cmux_tree_batch"):                             # sel0 and a number of steps / levels
        return [s + j for s, n in zip(args[2], args[3]) for j in range(n)]
    return list(args[SEL_POS[name]])


# ---- the recording rig ----------------------------------------------------------------------------------------------------------------------


class _Store:
    def __init__(self, rig, kind, slots, words=0):
        self.kind, self.slots, self.words = kind, int(slots), words
        self.ptr = self.serial = len(rig.stores)
        rig.stores.append(self)

    def upload(self, stream, first, host):
        stream.store_upload(self, int(first), int(np.asarray(host).reshape(-1, self.words).shape[0]))

    def download(self, stream, first, count):
        stream.store_download(self, int(first), int(count))
        return np.zeros((count, self.words), dtype=np.uint32)

    def free(self):
        self.freed = True

    def __repr__(self):
        return f"{self.kind}#{self.serial}:{self.slots}"


class _Key:
    def __init__(self, name, n=0):
        self.name, self.n = name, n

    def __repr__(self):
        return self.name


class _Stream:
    gpu_index = 0

    def __init__(self, rig):
        self.rig, self.sid = rig, len(rig.streams)
        rig.streams.append(self)

    def wait_stream(self, other):
        self.rig.log.append((self.sid, "wait_stream", [other.sid], []))

    def destroy(self):
        self.destroyed = True

    def __getattr__(self, name):
        def call(*args, **kw):
            flat = [a if isinstance(a, (_Store, _Key, int)) or a is None else np.asarray(a).tolist() for a in args]
            self.rig.log.append((self.sid, name, flat, sorted((k, np.asarray(v).tolist()) for k, v in kw.items())))
        return call


class _Backend:
    """what FrontierExecutor and CipherEngine need of a backend: gate batches and host writes, recorded on the main stream"""

    def __init__(self, rig, num_slots):
        self.stream, self._arena = _Stream(rig), _Store(rig, "Arena", num_slots, int(P.n) + 1)

    def gate_batch(self, ops, in0, in1, in2, out):
        if len(ops):
            self.stream.gate_batch(self._arena, ops, in0, in1, in2, out)

    def write_many(self, slots, rows):
        self.stream.upload_slots(self._arena, [int(s) for s in slots])

    def read_many(self, slots):
        return np.zeros((len(slots), int(P.n) + 1), dtype=np.uint32)

    def sync(self):
        pass


class _Rig:
    def __init__(self, monkeypatch):
        from iyokan_amd import hip

        self.log, self.stores, self.streams = [], [], []
        monkeypatch.setattr(hip, "current_params", lambda: P)
        monkeypatch.setattr(hip, "Trlwe", lambda slots, gpu=0: _Store(self, "Trlwe", slots, 2 * N))
        monkeypatch.setattr(hip, "Trgsw", lambda slots, gpu=0: _Store(self, "Trgsw", slots, PER * (int(P.k) + 1) * N))
        monkeypatch.setattr(hip, "Arena", lambda slots, gpu=0: _Store(self, "Arena", slots, int(P.n) + 1))
        monkeypatch.setattr(hip, "Tlwe2", lambda n_in, slots, gpu=0: _Store(self, "Tlwe2", slots, n_in + 1))
        monkeypatch.setattr(hip, "Stream", lambda gpu=0, hip_stream=None: _Stream(self))


class _Packet:
    """TRLWE images of the right lengths (the recording keeps their row counts only)"""

    def __init__(self, sysm):
        rows = lambda n: np.zeros((n, 2 * N), dtype=np.uint32)
        self.rom = {pt.name: rows(cmux.rom_layout(pt.addr_width, pt.data_width.bit_length() - 1, N).data_rows) for pt in sysm.ports if pt.kind == "rom"}
        self.ram = {pt.name: rows(pt.data_width << pt.addr_width) for pt in sysm.ports if pt.kind == "ram"}


def _engine(monkeypatch, sysm, cls=None, **kw):
    rig = _Rig(monkeypatch)
    plan = FrontierPlan(sysm.nl, 1, stages=sysm.stages)
    be = _Backend(rig, plan.num_slots)
    n1 = int(P.n) + 1
    eng = (cls or runner.CmuxCipherEngine)(sysm, FrontierExecutor(plan, be), lambda bits: np.zeros((len(bits), n1), dtype=np.uint32),
                                           lambda rows: [0] * len(rows), np.zeros(n1, dtype=np.uint32), _Key("bk2", int(P.n)), _Key("pk"),
                                           packet=_Packet(sysm), decrypt_ram=lambda rows: [0] * len(rows), **kw)
    return eng, rig


def _clocks(eng, sysm, n=3, images=True):
    """the order of run_packet: images, the first run, then tick + run per clock; at the end every RAM's image is read"""
    if images:
        for pt in sysm.ports:
            (eng.load_rom if pt.kind == "rom" else eng.load_ram)(pt.name, None)
    eng.run()
    for _ in range(n):
        eng.tick()
        eng.run()
    for pt in sysm.ports:
        if pt.kind == "ram":
            eng.ram_rows(pt.name)


def _digest(log):
    canon = [[sid, name, [repr(a) if isinstance(a, (_Store, _Key)) else a for a in args], kw] for sid, name, args, kw in log]
    return hashlib.sha256(json.dumps(canon, sort_keys=True).encode()).hexdigest()


@pytest.fixture(scope="module")
def four(tmp_path_factory):
    return load_blueprint(cases.write_blueprint(str(tmp_path_factory.mktemp("cmux_stage"))), cmux_memories=True)


@pytest.fixture(scope="module")
def two(tmp_path_factory):
    return load_blueprint(small.write_blueprint(str(tmp_path_factory.mktemp("cmux_stage_small"))), cmux_memories=True)


def test_the_four_port_system_has_three_ports_in_one_stage(four):
    got = [(pt.kind, pt.name, pt.addr_width, pt.data_width, pt.stage) for pt in four.ports]
    assert got == [(k, n, a, w, 1 if n == "ramc" else 0) for k, n, a, w in cases.PORTS]
    assert four.num_stages == 3 and len({pt.addr_width + 10 * pt.data_width for pt in four.ports[:3]}) == 3


# ---- selectors at a base slot -----------------------------------------------------------------------------------------------------------------
BASE = 5


def _shift(log, by):
    """the recording with `by` taken off every selector index a call names, and the selector store's identity dropped"""
    out = []
    for sid, name, args, kw in log:
        args = list(args)
        if name in SEL_POS:
            args[0] = "selectors"
            args[SEL_POS[name]] = [s - by for s in args[SEL_POS[name]]]
        elif name == "store_upload" and args[0].kind == "Trgsw":
            args = ["selectors", args[1] - by, args[2]]
        out.append((sid, name, [f"{a.kind}:{a.slots}" if isinstance(a, _Store) else a for a in args], kw))
    return out


def _pair(monkeypatch, make):
    """a memory with a store of its own and its twin at slot BASE of a larger store the caller owns, each on a rig of its own (the same
    store serials); returns (own, own's rig, shared, shared's rig, the caller's store)"""
    rig0 = _Rig(monkeypatch)
    st0 = _Stream(rig0)
    own = make(st0, {})
    rig1 = _Rig(monkeypatch)
    st1 = _Stream(rig1)
    store = _Store(rig1, "Trgsw", 64, PER * (int(P.k) + 1) * N)
    rig1.stores.pop()                                                               # not counted: the memories' own serials stay comparable
    shared = make(st1, {"trgsw": store, "sel_base": BASE})
    return own, rig0, shared, rig1, store


@pytest.mark.parametrize("shape", [(9, 3), (12, 0)])
@pytest.mark.parametrize("mode", [{}, {"fused": True}, {"fused_tree": True}, {"fused": True, "fused_tree": True}])
def test_rom_job_lists_at_a_base_slot(monkeypatch, shape, mode):
    aw, lw = shape
    rows = cmux.rom_layout(aw, lw, N).data_rows
    own, rig0, shared, rig1, store = _pair(monkeypatch, lambda st, kw: cmux.Rom(st, np.zeros((rows, 2 * N), dtype=np.uint32), aw, lw, max_reads=2, **kw))
    assert shared.trgsw is store and shared.sel_base == BASE and own.sel_base == 0 and own.trgsw is not store
    plus = lambda lists, pos: [tuple([s + BASE for s in a] if i == pos else list(a) for i, a in enumerate(args)) for args in lists]
    same = lambda lists: [tuple(list(a) for a in args) for args in lists]
    assert same(shared.launches(2)) == plus(own.launches(2), 0) and same(shared.tree_launches(2)) == plus(own.tree_launches(2), 0)
    (up0, ch0), (up1, ch1) = own.launches_fused(2), shared.launches_fused(2)
    assert same(up1) == plus(up0, 0) and (ch0 is None) == (ch1 is None)
    if ch0 is not None:
        assert same([ch1]) == plus([ch0], 1)
    arena, out = _Store(rig0, "Arena", 64), np.arange(2 << lw).reshape(2, -1)
    sel = np.zeros((2, aw, own.trgsw.words), dtype=np.uint32)
    for resident in (True, False):
        own.read(sel, arena, out, resident=resident, **mode)
        shared.read(sel, arena, out, resident=resident, **mode)
    assert _shift(rig1.log, BASE) == _shift(rig0.log, 0) and len(rig0.log) > 4
    top = max(max(_selectors(name, args)) for _, name, args, _ in rig1.log if name in SEL_POS)
    assert top == BASE + 2 * aw - 1                                                 # the second read's highest bit: the stride is addr_width
    own.free()
    shared.free()
    assert getattr(own.trgsw, "freed", False) and not getattr(store, "freed", False)


@pytest.mark.parametrize("shape", [(2, 1), (5, 2)])                                # 2-bit address x 1 bit; 32 words x 2 bits: two tree groups
@pytest.mark.parametrize("mode", [{}, {"fused": False}, {"fused_tree": True}])
def test_ram_job_lists_at_a_base_slot(monkeypatch, shape, mode):
    aw, dw = shape
    own, rig0, shared, rig1, store = _pair(monkeypatch, lambda st, kw: cmux.Ram(st, np.zeros((dw << aw, 2 * N), dtype=np.uint32), aw, dw, **kw))
    assert shared.trgsw is store and shared.sel_base == BASE
    plus = lambda lists: [tuple([s + BASE for s in a] if i == 0 else list(a) for i, a in enumerate(args)) for args in lists]
    same = lambda lists: [tuple(list(a) for a in args) for args in lists]
    assert same(shared.read_launches()) == plus(own.read_launches()) and same(shared.tree_launches()) == plus(own.tree_launches())
    assert shared.write_jobs() == [j._replace(sel0=j.sel0 + BASE) for j in own.write_jobs()]
    assert shared.write_jobs() == [j for d in range(dw) for j in cmux.ram_write_jobs(aw, shared.mux_rows(d)[0], d << aw, sel0=BASE)]
    arena = _Store(rig0, "Arena", 64)
    wdata, rdata = list(range(10, 10 + dw)), list(range(20, 20 + dw))
    sel = np.zeros((aw, own.trgsw.words), dtype=np.uint32)
    for resident in (True, False):
        own.clock(sel, arena, 5, wdata, rdata, resident=resident, **mode)
        shared.clock(sel, arena, 5, wdata, rdata, resident=resident, **mode)
    assert _shift(rig1.log, BASE) == _shift(rig0.log, 0) and len(rig0.log) > 8
    own.free()
    shared.free()
    assert getattr(own.trgsw, "freed", False) and not getattr(store, "freed", False)


def test_a_store_that_cannot_hold_the_selectors_is_refused_before_anything_is_allocated(monkeypatch):
    rig = _Rig(monkeypatch)
    st = _Stream(rig)
    store = _Store(rig, "Trgsw", 8)
    before = len(rig.stores)
    rom = lambda **kw: cmux.Rom(st, np.zeros((1, 2 * N), dtype=np.uint32), 3, 3, **kw)
    ram = lambda **kw: cmux.Ram(st, np.zeros((4, 2 * N), dtype=np.uint32), 2, 1, **kw)
    for make, kw in ((rom, dict(trgsw=store, sel_base=6)), (rom, dict(trgsw=store, sel_base=2, max_reads=3)), (rom, dict(trgsw=store, sel_base=-1)),
                     (rom, dict(trgsw=_Store(rig, "Trgsw", 2), sel_base=0)), (rom, dict(sel_base=1)), (ram, dict(trgsw=store, sel_base=7)),
                     (ram, dict(trgsw=store, sel_base=-2)), (ram, dict(trgsw=_Store(rig, "Trgsw", 1))), (ram, dict(sel_base=3))):
        count = len(rig.stores)
        with pytest.raises(ValueError, match="selector|sel_base"):
            make(**kw)
        assert len(rig.stores) == count and not rig.log, kw
    assert len(rig.stores) == before + 2
    rom(trgsw=store, sel_base=5)                                                    # the last three slots
    ram(trgsw=store, sel_base=6)


def test_words_at_a_base_slot_through_the_emulation(monkeypatch, keys128):
    """Ram 2 x 1 and Rom (3, 3): the job lists with the selectors at slot BASE of a store whose slots below hold uniform words, and with
    a store of their own, through the lane emulations of the chain and of the single CMUX: the same rows"""
    from iyokan_amd import client

    em, p = ram_ref.emul(), keys128.params
    rng = np.random.default_rng(41)
    uniform = lambda count: rng.integers(0, 1 << 32, size=(count,) + (PER, int(p.k) + 1, N), dtype=np.uint64).astype(np.uint32)
    # RAM: the read tree and the write chain of one clock
    sel = client.encrypt_trgsw(keys128, [1, 0], seed=5)
    spec = {0: cmux_ref.spectra(em, p, sel), BASE: cmux_ref.spectra(em, p, np.concatenate([uniform(BASE), sel]))}
    own, _, shared, _, _ = _pair(monkeypatch, lambda st, kw: cmux.Ram(st, np.zeros((4, 2 * N), dtype=np.uint32), 2, 1, **kw))
    bits = [1, 1, 0, 1] + [1] + [0] * (own.trlwe.slots - 5)
    rows = client.encrypt_ram_trlwe(keys128, bits, seed=6)
    rows[own.mux_rows(0)[0]] = client.encrypt_ram_trlwe(keys128, [0], seed=7)[0]
    got = {}
    for base, ram in ((0, own), (BASE, shared)):
        T = rows
        for args in ram.read_launches():
            T = cmux_ref.emu_run(em, p, T, spec[base], base + 2, list(zip(*args)))
        got[base] = ram_ref.emu_chain_run(em, p, T, spec[base], base + 2, [tuple(j) for j in ram.write_jobs()])
    assert np.array_equal(got[0], got[BASE]) and not np.array_equal(got[0][:4], rows[:4])
    assert list(client.decrypt_ram_trlwe(keys128, got[BASE][:4])) == [1, 0, 0, 1]  # cell 1 (address bits 1, 0) took the written 0
    # ROM: three rotate-form steps on one row of 128 words of 8 bits
    sel = client.encrypt_trgsw(keys128, [1, 0, 1], seed=8)
    spec = {0: cmux_ref.spectra(em, p, sel), BASE: cmux_ref.spectra(em, p, np.concatenate([uniform(BASE), sel]))}
    own, _, shared, _, _ = _pair(monkeypatch, lambda st, kw: cmux.Rom(st, np.zeros((1, 2 * N), dtype=np.uint32), 3, 3, **kw))
    data = rng.integers(0, 1 << 32, size=(own.trlwe.slots, 2 * N), dtype=np.uint64).astype(np.uint32)
    got = {}
    for base, rom in ((0, own), (BASE, shared)):
        T = data
        for args in rom.launches(1):
            T = cmux_ref.emu_run(em, p, T, spec[base], base + 3, list(zip(*args)))
        got[base] = T
    assert np.array_equal(got[0], got[BASE]) and not np.array_equal(got[0][own.layout.result], data[own.layout.result])


# ---- one circuit bootstrapping per stage ---------------------------------------------------------------------------------------------------------


def test_defaults_enqueue_the_recorded_calls(monkeypatch, four):
    """the engine as every caller has it today — no new keyword — against the digest of the same recording taken from the commit before"""
    eng, rig = _engine(monkeypatch, four)
    _clocks(eng, four)
    eng.free()
    assert not [c for c in rig.log if c[1] == "wait_stream"] and len(rig.streams) == 1
    assert sum(c[1] == "circuit_bootstrap_batch" for c in rig.log) == 4 * 4         # a batch per port and run()
    assert _digest(rig.log) == PARENT_DIGEST


def _check_stage_cb(eng, rig, sysm):
    """every run(): one batch per stage with ports — the concatenated address slots in the order of the ports' base slots, the stage's
    first base slot, stores that hold the batch — and behind it only calls that name the shared store inside their port's slots"""
    slot = eng.ex.plan.slot
    bases = {pt.name: eng.mem[pt.name].sel_base for pt in sysm.ports}
    assert sorted(bases.values()) == list(np.cumsum([0] + [pt.addr_width for pt in sorted(sysm.ports, key=lambda q: bases[q.name])])[:-1])
    stages = sorted({pt.stage for pt in sysm.ports})
    batches = [c for c in rig.log if c[1] == "circuit_bootstrap_batch"]
    assert len(batches) % len(stages) == 0 and len(batches) >= len(stages)
    for k, (_, _, args, _) in enumerate(batches):
        pts = sorted((pt for pt in sysm.ports if pt.stage == stages[k % len(stages)]), key=lambda q: bases[q.name])
        want = [slot[a] for pt in pts for a in pt.addr]
        assert args[3] == want, (k, args[3], want)
        assert args[4] == [1] * len(want) and args[6] == 0
        assert args[8] is eng.trgsw and args[9] == bases[pts[0].name], (k, args[9])
        assert [bases[pt.name] for pt in pts] == [args[9] + sum(q.addr_width for q in pts[:i]) for i in range(len(pts))]   # contiguous
        assert args[5].slots >= len(want) * L and args[7].slots >= len(want) * PER, (k, args[5], args[7])
    owner = {}                                                                      # TRLWE store -> its port
    for pt in sysm.ports:
        owner[eng.mem[pt.name].trlwe] = pt
    used = 0
    for _, name, args, _ in rig.log:
        if name in SEL_POS:
            pt = owner[args[1]]
            idx = _selectors(name, args)
            assert args[0] is eng.trgsw and set(idx) <= set(range(bases[pt.name], bases[pt.name] + pt.addr_width)), (name, pt.name, idx)
            used += 1
    assert used


@pytest.mark.parametrize("fused", [False, True])
def test_stage_cb_is_one_batch_per_stage(monkeypatch, four, fused):
    eng, rig = _engine(monkeypatch, four, stage_cb=True, rom_fused=fused, tree_fused=fused)
    _clocks(eng, four)
    assert [eng.mem[n].sel_base for _, n, _, _ in cases.PORTS] == [0, 3, 4, 6] and eng.trgsw.slots == 7
    assert eng.tlwe2.slots == 6 * L and eng.scratch.slots == 6 * PER                # the widest stage: 3 + 1 + 2 address bits
    assert sum(c[1] == "circuit_bootstrap_batch" for c in rig.log) == 4 * 2         # two stages with ports, four run()s
    _check_stage_cb(eng, rig, four)
    eng.free()
    assert eng.trgsw.freed and sum(s.kind == "Trgsw" for s in rig.stores) == 1 and len(rig.streams) == 1


def test_stage_cb_with_one_port_per_stage_enqueues_todays_calls(monkeypatch, two):
    """the small system (a ROM, then a RAM): the same calls apart from the store's identity and the RAM's base slot"""
    logs = []
    for kw in ({}, {"stage_cb": True}):
        eng, rig = _engine(monkeypatch, two, **kw)
        _clocks(eng, two)
        base = {eng.mem[pt.name].trlwe.serial: eng.mem[pt.name].sel_base for pt in two.ports}
        canon = []
        for sid, name, args, kw2 in rig.log:
            args = list(args)
            if name in SEL_POS:
                args[0], args[SEL_POS[name]] = "selectors", [s - base[args[1].serial] for s in args[SEL_POS[name]]]
            if name == "circuit_bootstrap_batch":
                args[8], args[9] = "selectors", 0
                args[5], args[7] = "lvl2", "scratch"
            canon.append((sid, name, [a.kind if isinstance(a, _Store) else repr(a) if isinstance(a, _Key) else a for a in args], kw2))
        logs.append(canon)
        eng.free()
    assert logs[0] == logs[1]
    assert base == {eng.mem["rom"].trlwe.serial: 0, eng.mem["ram"].trlwe.serial: 3}


class _OtherOrder(runner.CmuxCipherEngine):
    """bases per port as they should be, the batch concatenated the other way round"""

    def _stage_ports(self, s):
        return super()._stage_ports(s)[::-1]


class _WidestPort(runner.CmuxCipherEngine):
    """the lvl2 store and the scratch rows sized as before: for the widest port"""

    def _cb_bits(self):
        return max(pt.addr_width for pt in self.ports)


class _SlotZeroAgain(runner.CmuxCipherEngine):
    """the second stage's batch writes its selectors from slot 0"""

    def _stage_first_slot(self, pts):
        return 0 if pts[0].stage > 0 else super()._stage_first_slot(pts)


@pytest.mark.parametrize("mutant", [_OtherOrder, _WidestPort, _SlotZeroAgain])
def test_each_stage_cb_mistake_is_caught(monkeypatch, four, mutant):
    eng, rig = _engine(monkeypatch, four, cls=mutant, stage_cb=True)
    _clocks(eng, four)
    with pytest.raises(AssertionError):
        _check_stage_cb(eng, rig, four)


# ---- the refresh aside: happens-before ----------------------------------------------------------------------------------------------------------


def _before(log):
    """before[j]: the set (a bit mask) of calls that happen before call j — program order per stream, and a wait_stream behind the
    last call the other stream held when it was enqueued"""
    before, last = [], {}
    for j, (sid, name, args, _) in enumerate(log):
        mask = 0
        preds = [last.get(sid)] + ([last.get(args[0])] if name == "wait_stream" else [])
        for i in preds:
            if i is not None:
                mask |= before[i] | (1 << i)
        before.append(mask)
        last[sid] = j
    return before


def _buffers(rig, call):
    _, name, args, kw = call
    out = {a.serial for a in args if isinstance(a, _Store)}
    if name == "bootstrap_trlwe_batch":                                             # its output rows come as a device pointer
        out.add(rig.stores[args[6]].serial)
    return out


def _unordered(rig):
    """the pairs of calls that touch a common store and are not ordered by happens-before"""
    before = _before(rig.log)
    touch = [_buffers(rig, c) for c in rig.log]
    return [(i, j) for j in range(len(rig.log)) for i in range(j) if touch[i] & touch[j] and not (before[j] >> i) & 1]


def _aside(rig):
    """(the refresh calls, the circuit bootstrapping batches), as positions in the recording"""
    side = [j for j, c in enumerate(rig.log) if c[0] != 0 and c[1] != "wait_stream"]
    return side, [j for j, c in enumerate(rig.log) if c[1] == "circuit_bootstrap_batch"]


@pytest.mark.parametrize("stage_cb", [False, True])
def test_refresh_aside_orders_every_shared_buffer_and_nothing_more(monkeypatch, four, stage_cb):
    eng, rig = _engine(monkeypatch, four, refresh_aside=True, stage_cb=stage_cb)
    _clocks(eng, four)
    assert len(rig.streams) == 2                                                    # one extra stream for three RAMs
    side, batches = _aside(rig)
    assert len(side) == 3 * 3 * 2                                                   # 3 clocks x 3 RAMs x (extraction, rotation back)
    assert {rig.log[j][1] for j in side} == {"sample_extract_index_keyswitch_batch", "bootstrap_trlwe_batch"}
    private = {eng.mem[n].arena.serial for k, n, _, _ in cases.PORTS if k == "ram"}
    cells = {eng.mem[n].trlwe.serial for k, n, _, _ in cases.PORTS if k == "ram"}
    for j in side:                                                                  # the refresh side's buffers: cell rows and private arenas
        assert _buffers(rig, rig.log[j]) <= private | cells, rig.log[j]
    bad = _unordered(rig)
    assert not bad, [(rig.log[i][:2], rig.log[j][:2]) for i, j in bad[:4]]
    # nothing more: every clock's refresh is beside the NEXT run()'s first batch (else nothing was taken aside)
    before = _before(rig.log)
    ticks = sorted({max(b for b in batches if b < j) for j in side})                # the last batch in front of each tick
    assert len(ticks) == 3
    for t in ticks:
        nxt = min(b for b in batches if b > t)
        mine = [j for j in side if t < j < nxt]
        assert len(mine) == 6 and not any((before[nxt] >> j) & 1 for j in mine), t
    # between tick and read tree the main stream touches none of the refresh side's buffers
    for t in ticks:
        nxt = min(b for b in batches if b > t)
        last_side = max(j for j in side if t < j < nxt)
        between = [c for c in rig.log[last_side + 1:nxt + 1] if c[0] == 0 and c[1] != "wait_stream"]
        assert between and all(not _buffers(rig, c) & (private | cells) for c in between)
    waits = len([c for c in rig.log if c[1] == "wait_stream"])
    eng.free()
    assert len([c for c in rig.log if c[1] == "wait_stream"]) == waits and rig.streams[1].destroyed   # cells() had ordered every RAM
    eng2, rig2 = _engine(monkeypatch, four, refresh_aside=True)
    _clocks(eng2, four, n=1)
    eng2.tick()
    eng2.free()                                                                     # with refreshes pending: each RAM waits first
    assert [c[:3] for c in rig2.log[-3:]] == [(0, "wait_stream", [1])] * 3


def test_refresh_aside_moves_calls_and_changes_none(monkeypatch, four):
    """without the waits, and whatever the stream, the recording is the default engine's"""
    plain = []
    for kw in ({}, {"refresh_aside": True}):
        eng, rig = _engine(monkeypatch, four, **kw)
        _clocks(eng, four)
        plain.append([(name, [repr(a) if isinstance(a, (_Store, _Key)) else a for a in args], k) for _, name, args, k in rig.log if name != "wait_stream"])
        eng.free()
    assert plain[0] == plain[1]


def test_load_ram_waits_for_a_pending_refresh(monkeypatch, four):
    eng, rig = _engine(monkeypatch, four, refresh_aside=True)
    _clocks(eng, four, n=1)
    eng.tick()
    mark = len(rig.log)
    eng.load_ram("ramb", None)
    assert [c[:3] for c in rig.log[mark:mark + 1]] == [(0, "wait_stream", [1])] and rig.log[mark + 1][1] == "store_upload"
    assert not _unordered(rig)
    with pytest.raises(ValueError, match="own stream"):
        eng.mem["rama"].write_port(eng.arena, 0, [1], [2], refresh_stream=eng.stream)


class _NoWaitBeforeRead(cmux.Ram):
    def read_port(self, *a, **kw):
        self.pending_refresh = None
        return super().read_port(*a, **kw)


class _Deaf:
    """a refresh stream that does not wait for the chain"""

    def __init__(self, st):
        self.st = st

    def wait_stream(self, other):
        pass

    def __getattr__(self, name):
        return getattr(self.st, name)


class _NoWaitOnTheChain(cmux.Ram):
    def write_port(self, *a, refresh_stream=None, **kw):
        super().write_port(*a, refresh_stream=_Deaf(refresh_stream), **kw)
        self.pending_refresh = refresh_stream


class _CellsWithoutWait(cmux.Ram):
    def cells(self):
        return self.trlwe.download(self.stream, 0, self.ncells).reshape(self.data_width, self.cells_per_plane, 2 * self.N)


@pytest.mark.parametrize("mutant", [_NoWaitBeforeRead, _NoWaitOnTheChain, _CellsWithoutWait])
def test_each_missing_wait_is_caught(monkeypatch, four, mutant):
    monkeypatch.setattr(cmux, "Ram", mutant)
    eng, rig = _engine(monkeypatch, four, refresh_aside=True)
    _clocks(eng, four, images=False)                                                # the read at the end is the last toucher of the cells
    if mutant is _CellsWithoutWait:                                                 # ... behind a tick, so that a refresh is pending
        eng.tick()
        eng.ram_rows("ramb")
    assert _unordered(rig), mutant.__name__


# ---- the argument check of iyk_hip_stream_wait_stream ---------------------------------------------------------------------------------------


def _wait_args(st, other, st_replica=0, other_replica=0, st_ordinal=0, other_ordinal=0):
    f = brc.emul().iyk_emul_stream_wait_args
    f.restype = ctypes.c_int
    u64 = ctypes.c_uint64
    msg = ctypes.create_string_buffer(256)
    words, counts = (ctypes.c_uint32 * 4)(), (u64 * 2)()
    code = f(u64(st), u64(other), ctypes.c_int(st_replica), ctypes.c_int(other_replica), ctypes.c_int(st_ordinal), ctypes.c_int(other_ordinal), msg,
             u64(256), words, u64(4), counts)
    return code, msg.value.decode()


@pytest.mark.parametrize("args,text", [
    ((0, 0x1000), "null stream"), ((0x1000, 0), "null stream"), ((0, 0), "null stream"),
    ((0x1000, 0x1000), "a stream cannot wait for itself"),
    ((0x1000, 0x2000, 0, 1, 0, 1), "the two streams are on different GPUs"),
    ((0x1000, 0x2000, 0, 0, 2, 3), "the two streams are on different GPUs"),
    ((0x1000, 0x2000, 0, 1, 0, 0), "the two streams belong to different replicas"),
    ((0x1000, 0x2000, 3, 1, 2, 2), "the two streams belong to different replicas"),
])
def test_wait_stream_refusals(built, args, text):
    assert _wait_args(*args) == (-1, text)


def test_wait_stream_accepts_two_streams_of_one_replica(built):
    assert _wait_args(0x1000, 0x2000) == (0, "") and _wait_args(0x2000, 0x1000, 3, 3, 1, 1) == (0, "")
    assert _wait_args(0, 0, 0, 1, 0, 1)[1] == "null stream"                        # the handles are looked at first
