"""Run a blueprint system (or a bare netlist) through the reference's clocking protocol.

Mirrors the frontends' `go()` (/root/reference/src/iyokan_plain.cpp:453-555 and, identically for the
GPU backend, /root/reference/src/iyokan_cufhe.cpp:754-832):

    ROM images are in place before anything runs;
    if the system has an @reset input (and reset is not skipped): reset = 1, run the combinational logic;
    for cycle in 0 .. N-1  (N < 0: until @finflag reads 1):
        tick                               # every DFF / RAM cell latches its input
        cycle 0 only: reset = 0, then the request packet's RAM images are written (setInitialRAM)
        @inputs take their bit stream, circularly:  bit (width * cycle + i) mod len   (setCircularInputs)
        run the combinational logic
    result packet = every @output, every RAM image, and the number of cycles run.

The engine behind it is anything with `set_nodes / get_nodes / run / tick` working on BITS: `PlainEngine` (numpy evaluator) or `CipherEngine` (a `FrontierExecutor` whose
values are TLWE ciphertexts, wrapped with an encrypt / decrypt pair — the GPU path).

A system with CMUX memory ports (load_blueprint(cmux_memories=True)) needs an engine that also has `load_rom / load_ram / ram_image`
and runs its plan in stages: `CmuxCipherEngine` (cmux.Rom / cmux.Ram behind circuit bootstrapping, on the GPU) or `StagedBitsEngine`
(the same staging on bits, the memories evaluated in the clear).  The memories clock during the reset cycle like everything else
and the request's cycle-0 RAM image overwrites them afterwards, as the reference's go() does.
"""
import numpy as np

from . import netlist as N
from .packet import PlainPacket
from .snapshot import PARAM_NAMES, EngineState, Snapshot, as_snapshot

MAX_CB_BATCH = 1 << 20   # rotations of one circuit bootstrapping batch (csrc/jobs.hpp)


class PlainEngine(EngineState):
    """lanes: that many independent copies of the circuit's state (run_packets: one request each); run / tick clock them all.
    state() / load_state() (snapshot.EngineState): every node's value, per lane."""

    def __init__(self, nl, lanes=1):
        if lanes < 1:
            raise ValueError(f"lanes = {lanes!r}: an engine has one lane or more")
        self.nl, self.lanes = nl, lanes
        self.sims = [N.PlainSimulator(nl) for _ in range(lanes)]
        self.sim = self.sims[0]

    def set_nodes(self, nids, bits, lane=0):
        for nid, v in zip(nids, bits):
            self.sims[lane].val[nid] = v

    def get_nodes(self, nids, lane=0):
        return [self.sims[lane].node_value(i) for i in nids]

    def run(self):
        for sim in self.sims:
            sim.evaluate()

    def tick(self):
        for sim in self.sims:
            sim.tick()

    # ---- snapshot.EngineState: the "arena" is the simulator's value of every node ----
    def _state_plan_slot(self):
        return None

    def _state_slots(self):
        return list(range(self.nl.num_nodes))

    def _read_slots(self, slots, lane):
        return self.sims[lane].val[slots].astype(np.uint8)

    def _write_slots(self, slots, values, lane):
        self.sims[lane].val[slots] = values


class CipherEngine(EngineState):
    """A FrontierExecutor (ciphertext slots) seen as a bit engine: `encrypt(bits) -> rows`,
    `decrypt(rows) -> bits`.  State cells start as trivial 0 like TaskCUFHEGateDFF's constructor
    (/root/reference/src/iyokan_cufhe.hpp:108-133).
    lanes: the copies of the circuit's image the executor's backend holds (HipBackend / PlainBitBackend(lanes=)); None: whatever
    the backend has.  run / tick clock all lanes at once — every level ONE batch of count x lanes gates — and set_nodes / get_nodes
    address one lane.  The plan is the single-lane plan.
    state() / load_state() (snapshot.EngineState): the words of every slot of the plan, lane by lane through the backend's own lane=."""

    state_kind = "cipher"

    def __init__(self, executor, encrypt, decrypt, zero_row, lanes=None):
        self.ex, self.encrypt, self.decrypt = executor, encrypt, decrypt
        self.nl = executor.plan.nl
        have = getattr(executor.be, "lanes", 1)
        if lanes is not None and lanes != have:
            raise ValueError(f"lanes = {lanes!r}, but the executor's backend holds {have}: give the backend the lane count")
        self.lanes = have
        plan = executor.plan
        cells = list(plan.dffs) + list(plan.sources)   # state cells and not-yet-driven inputs read as 0
        for lane in range(self.lanes if cells else 0):
            executor.be.write_many([plan.slot[i] for i in cells], np.tile(zero_row, (len(cells), 1)), **self._lane(lane))

    @staticmethod
    def _lane(lane):
        return {"lane": lane} if lane else {}   # a backend without lanes takes no such argument

    def set_nodes(self, nids, bits, lane=0):
        if len(nids):
            slot = self.ex.plan.slot
            self.ex.be.write_many([slot[i] for i in nids], self.encrypt([int(b) for b in bits]), **self._lane(lane))

    def get_nodes(self, nids, lane=0):
        if not len(nids):
            return []
        slot = self.ex.plan.slot
        return [int(b) for b in self.decrypt(self.ex.be.read_many([slot[i] for i in nids], **self._lane(lane)))]

    def run(self):
        self.ex.run()

    def tick(self):
        self.ex.tick()

    # ---- snapshot.EngineState ----
    def _state_params(self):
        from . import hip

        p = hip.current_params()
        return {name: int(getattr(p, name)) for name in PARAM_NAMES}

    def _slot_shape(self):
        return (self._state_params()["n"] + 1,)

    def _read_slots(self, slots, lane):
        return np.ascontiguousarray(self.ex.be.read_many(slots, **self._lane(lane)), dtype=np.uint32).reshape(len(slots), -1)

    def _write_slots(self, slots, rows, lane):
        self.ex.be.write_many(slots, rows, **self._lane(lane))


class StagedPorts:
    """run / tick of an engine whose FrontierExecutor has a staged plan and whose memories are ports (system.MemPort): in run(),
    after the levels of stage s every port of stage s turns its address slots into read data (_port_read) on the executor's one
    stream; in tick(), every RAM is written back (_port_write) BEFORE the DFF latch / commit copies — wren / wdata may be DFF
    outputs, which the commit overwrites.  The write uses the address the read saw (the resident selectors).
    read_early (with a plan that has port_ready: FrontierPlan(early=ports)): a port is read once the levels its address depends on are
    enqueued — port_ready of them — not once its whole stage is; the ports that are read together (_read_groups) go out when the
    last of them is ready.  An engine with streams forks there (_fork) and joins (_join) in front of the next stage's first level
    and at the end of run(); on one stream both do nothing and only the program order moves."""

    read_early = False

    def _reads(self, s):
        for pt in self.ports:
            if pt.stage == s:
                self._port_read(pt)

    def run(self):
        if not self.read_early:
            return self.ex.run(after_stage=self._reads)
        self._stage, self._enqueued, self._read = 0, 0, set()
        self.ex.run(after_stage=self._early_stage, after_level=self._early_level)
        self._join()

    def _ready_level(self, pt):
        return self.ex.plan.port_ready[pt.name]

    def _read_groups(self, s):
        """The ports of stage s in the groups that are read together, in port order: here every port alone"""
        return [[pt] for pt in self.ports if pt.stage == s]

    def _read_group(self, pts):
        for pt in pts:
            self._port_read(pt)

    def _fork(self):
        pass

    def _join(self):
        pass

    def _early_level(self, i):
        self._enqueued = i
        self._read_ready()

    def _early_stage(self, s):
        self._join()                # nothing of a later stage runs beside a read of this one: it may read the rdata slots
        self._stage = s + 1
        self._read_ready()          # a port of the next stage whose address depends on no gate of that stage

    def _read_ready(self):
        for pts in self._read_groups(self._stage):
            if pts[0].name not in self._read and max(self._ready_level(pt) for pt in pts) <= self._enqueued:
                self._read.add(pts[0].name)
                self._fork()
                self._read_group(pts)

    def _write_ports(self):
        for pt in self.ports:
            if pt.kind == "ram":
                self._port_write(pt)

    def tick(self):
        self._write_ports()
        self.ex.tick()


def _staged_executor(system, backend_of, balance=True, spread=True, cost=None, read_early=False):
    from . import frontier

    kw = {} if cost is None else {"cost": cost}
    if read_early:
        kw["early"] = system.ports
    plan = frontier.FrontierPlan(system.nl, 1, balance, spread=spread, stages=system.stages, **kw)
    return frontier.FrontierExecutor(plan, backend_of(plan.num_slots))


class StagedBitsEngine(StagedPorts, EngineState):
    """The bits-only twin of CmuxCipherEngine: the staged plan of `system` on a PlainBitBackend, every memory port an array of bits
    read and written in the clear.  What it checks is the ORDER — stages, read before write, write before commit.
    lanes: that many copies of the circuit's image (PlainBitBackend(lanes=)) and of every memory, one request each (run_packets): a
    port's read and write run lane by lane, the lanes share the clock only.
    read_early=True: the plan hoists the address cones (FrontierPlan(early=)) and every port is read at its port_ready level
    (StagedPorts): the program order CmuxCipherEngine(read_early=True) spreads over two streams.
    state() / load_state() (snapshot.EngineState): the bits of every slot of the plan and the image of every memory, per lane; the address
    the last read saw (tick()'s write uses it) is recomputed from the restored address slots."""

    port_lanes = True   # run_packets: the memory ports of this engine have lanes

    def __init__(self, system, balance=True, spread=True, lanes=1, read_early=False):
        from . import frontier

        if lanes < 1:
            raise ValueError(f"lanes = {lanes!r}: an engine has one lane or more")
        self.lanes, self.read_early = lanes, bool(read_early)
        self.ex = _staged_executor(system, (lambda n: frontier.PlainBitBackend(n, lanes=lanes)) if lanes > 1 else frontier.PlainBitBackend, balance,
                                   spread, read_early=self.read_early)
        self.nl, self.ports = system.nl, list(system.ports)
        self.mems = [{pt.name: [0] * (pt.data_width << pt.addr_width) for pt in self.ports} for _ in range(lanes)]
        self.mem = self.mems[0]
        self._addrs = [{} for _ in range(lanes)]
        self._addr = self._addrs[0]

    _lane = staticmethod(CipherEngine._lane)

    def set_nodes(self, nids, bits, lane=0):
        if len(nids):
            slot = self.ex.plan.slot
            self.ex.be.write_many([slot[i] for i in nids], [int(b) for b in bits], **self._lane(lane))

    def get_nodes(self, nids, lane=0):
        slot = self.ex.plan.slot
        return self.ex.be.read_many([slot[i] for i in nids], **self._lane(lane))

    def _port_read(self, pt):
        slot, be = self.ex.plan.slot, self.ex.be
        for lane in range(self.lanes):
            kw = self._lane(lane)
            addr = sum(b << i for i, b in enumerate(be.read_many([slot[a] for a in pt.addr], **kw)))
            self._addrs[lane][pt.name] = addr
            word = self.mems[lane][pt.name][addr * pt.data_width:(addr + 1) * pt.data_width]
            be.write_many([slot[r] for r in pt.rdata], word, **kw)

    def _port_write(self, pt):
        slot, be = self.ex.plan.slot, self.ex.be
        for lane in range(self.lanes):
            kw = self._lane(lane)
            if pt.name in self._addrs[lane] and be.read(slot[pt.wren[0]], **kw):
                addr = self._addrs[lane][pt.name]
                self.mems[lane][pt.name][addr * pt.data_width:(addr + 1) * pt.data_width] = be.read_many([slot[w] for w in pt.wdata], **kw)

    def _load(self, name, image, lane):
        if image is not None:
            cells = self.mems[lane][name]
            if len(image) > len(cells):
                raise ValueError(f"Invalid request packet: the image of {name!r} is longer than the memory")
            cells[:len(image)] = [int(b) for b in image]

    def load_rom(self, name, request, lane=0):
        self._load(name, request.rom.get(name), lane)

    def load_ram(self, name, request, lane=0):
        image = request.ram.get(name)
        if image is not None and len(image) != len(self.mems[lane][name]):
            raise ValueError("Invalid request packet: wrong length of RAM")
        self._load(name, image, lane)

    def ram_image(self, name, lane=0):
        return list(self.mems[lane][name])

    # ---- snapshot.EngineState ----
    def _state_meta(self, done, reset_ran):
        return dict(super()._state_meta(done, reset_ran), ran=[bool(a) for a in self._addrs])   # per lane: whether a read has happened

    def check_state(self, snap):
        super().check_state(snap)
        if len(snap.meta.get("ran", [])) != self.lanes:
            raise ValueError("the snapshot does not say which lanes have read their ports")

    def _read_slots(self, slots, lane):
        return np.asarray(self.ex.be.read_many(slots, **self._lane(lane)), dtype=np.uint8)

    def _write_slots(self, slots, bits, lane):
        self.ex.be.write_many(slots, bits, **self._lane(lane))

    def _mem_shape(self, pt):
        return (pt.data_width << pt.addr_width,)

    def _read_mem(self, pt, lane):
        return np.asarray(self.mems[lane][pt.name], dtype=np.uint8)

    def _write_mem(self, pt, lane, image):
        self.mems[lane][pt.name][:] = [int(b) for b in image]

    def _after_load(self, snap):
        slot, be = self.ex.plan.slot, self.ex.be
        for lane in range(self.lanes):
            self._addrs[lane].clear()
            if snap.meta["ran"][lane]:
                for pt in self.ports:
                    self._addrs[lane][pt.name] = sum(b << i for i, b in enumerate(be.read_many([slot[a] for a in pt.addr], **self._lane(lane))))


class CmuxCipherEngine(StagedPorts, CipherEngine):
    """CipherEngine for a system with CMUX memory ports, on one GPU.  Per port a cmux.Rom / cmux.Ram on the executor's stream; shared
    by all ports the lvl2 bootstrapping key `bk2`, the private key-switching key `privks_key`, one Tlwe2 store and one TRLWE scratch
    store sized for the widest address.  A port's read is ONE Stream.circuit_bootstrap_batch from its address slots into its own
    selector slots, then Rom.read(resident=True) / Ram.read_port into the rdata nodes' slots; nothing synchronises with the host.
    `packet`: the encrypted request (TFHEPacket) whose TRLWE forms `rom` / `ram` fill the memories; `decrypt_ram(rows) -> bits`
    (client.decrypt_ram_trlwe of the caller's keys) reads the result packet's RAM images out of Ram.cells().
    The 80-bit set is refused unless words_only=True: there the restatement of the circuit bootstrapping itself misreads ROM bits
    (DESIGN.md section 6d), so only words may be compared, never decryptions.
    rom_fused=True: the rotate tail of every ROM read is ONE Stream.cmux_rotate_chain_batch (Rom.read(fused=True)): the same words.
    tree_fused=True: the read tree of every ROM and RAM port is ONE Stream.cmux_tree_batch per four levels (fused_tree=True): the same words.
    stage_cb=True: ONE Stream.circuit_bootstrap_batch per STAGE instead of one per port.  The engine owns one selector store; every port
    has its base slot in it (cmux.Rom / cmux.Ram(trgsw=, sel_base=)), the ports of a stage next to each other in port order, so the
    stage's batch takes the concatenated address slots of its ports and writes the selectors from the stage's first base slot on.  The
    lvl2 store and the TRLWE scratch are sized for the widest stage.  A rotation batch costs the same up to 256 rotations
    (DESIGN.md section 6d), so every further port of a stage is free.  The same words.
    refresh_aside=True: every RAM's refresh runs on ONE second stream of the engine (Ram.write_port(refresh_stream=...), whose class
    docstring has the argument), beside the next clock's DFF copies, first-stage gates and circuit bootstrapping; each RAM orders itself
    back in front of its next read, write, cells() or free(), and load_ram in front of its upload.  The same words.
    read_early=True (the executor's plan made with FrontierPlan(early=system.ports)): every memory lives on ONE further stream P of the
    engine and a port is read there as soon as its address is final (plan.port_ready), beside the rest of its stage's gate levels on
    the executor's stream M: P waits for M at the fork; M waits for P in front of the first level of the next stage and at the end of
    run().  With stage_cb the stage's one batch goes out when the last of its ports is ready.  tick(): P waits for M, every RAM's
    write_port on P, M waits for P, then the latch and commit copies.  A read touches the address slots (final at the fork), the rdata
    slots (read by later stages only), the lvl2 store, the TRLWE scratch, the selector store, the memory's rows, a RAM's private arena
    and P's own stream scratch — nothing the gate levels of its stage touch.  The same words.  Measured, it
    pays with rom_fused + tree_fused: a read of more than eight calls makes the host wait for the rotation inside the read (a stream
    stages eight calls ahead), and the gate levels beside it are then not enqueued in time.
    All three are off by default; DESIGN.md section 6e has what each measured.
    state() / load_state() (snapshot.EngineState): the arena's words, every RAM's cell rows and every ROM's rows, per lane; no key.
    lanes: 1.  The memories hold one request: lanes > 1 (here or on the executor's backend) is a ValueError."""

    def __init__(self, system, executor, encrypt, decrypt, zero_row, bk2, privks_key, packet=None, decrypt_ram=None, words_only=False,
                 rom_fused=False, tree_fused=False, stage_cb=False, refresh_aside=False, lanes=1, read_early=False, cb_many=False):
        from . import cmux, hip
        from .params import params_80bit

        if lanes != 1 or getattr(executor.be, "lanes", 1) != 1:
            raise ValueError("CMUX memories have no lanes (lanes > 1 is refused): a cmux.Rom / cmux.Ram holds ONE request's rows and "
                             "selectors — run the lowered (mux-*) form of the system with CipherEngine, or one lane")
        self._setup(system, executor, encrypt, decrypt, zero_row, bk2, privks_key, [packet], decrypt_ram, words_only, rom_fused, tree_fused,
                    stage_cb, refresh_aside, 1, read_early, cb_many)

    def _setup(self, system, executor, encrypt, decrypt, zero_row, bk2, privks_key, packets, decrypt_ram, words_only, rom_fused, tree_fused,
               stage_cb, refresh_aside, K, read_early=False, cb_many=False):
        """The engine for K lanes (CmuxLaneEngine; K = 1: this class).  Lane r's arena slots are lane 0's + r * the backend's lane stride,
        every memory is a cmux.Rom / cmux.Ram(lanes=K), and the lvl2 store and the TRLWE scratch hold K x the widest batch."""
        from . import cmux, hip
        from .params import params_80bit

        p = hip.current_params()
        p80 = params_80bit()
        if (p.n, p.l, p.Bgbit) == (p80.n, p80.l, p80.Bgbit) and not words_only:
            raise ValueError("CMUX memories behind circuit bootstrapping misread bits at the 80-bit set (DESIGN.md 6d): "
                             "pass words_only=True and compare words, not decryptions")
        if executor.world != 1:
            raise ValueError("staged systems run on one GPU")
        if not system.ports or len(executor.plan.stage_levels) != system.num_stages:
            raise ValueError("the executor's plan is not the staged plan of this system (FrontierPlan(stages=system.stages))")
        if bk2.n != p.n:
            raise ValueError(f"the lvl2 bootstrapping key rotates TLWEs of n = {bk2.n}, the arena holds n = {p.n}")
        if read_early and set(getattr(executor.plan, "port_ready", ())) != {pt.name for pt in system.ports}:
            raise ValueError("read_early needs a plan that knows when every port's address is ready (FrontierPlan(stages=, early=system.ports))")
        CipherEngine.__init__(self, executor, encrypt, decrypt, zero_row)
        be = executor.be
        self.stream, self.arena, self.ports = be.stream, be._arena, list(system.ports)
        self.bk2, self.privks_key, self.packets, self.decrypt_ram = bk2, privks_key, list(packets), decrypt_ram
        self.packet = self.packets[0]
        self.rom_fused, self.tree_fused, self.stage_cb = bool(rom_fused), bool(tree_fused), bool(stage_cb)
        self.cb_many = bool(cb_many)   # every circuit bootstrapping is a circuit_bootstrap_many_batch: one rotation per address bit
        self.lanes, self.lane_stride = K, int(getattr(be, "lane_stride", 0))
        N, l, per = int(p.N), int(p.l), int(p.trgsw_rows)
        widest = K * self._cb_bits()
        if widest * l > MAX_CB_BATCH:
            raise ValueError(f"{K} lanes x {widest // K} address bits x {l} digits: more than the {MAX_CB_BATCH} rotations of one circuit bootstrapping")
        self.tlwe2 = hip.Tlwe2(hip.Bk2Key.N2, widest * l, self.stream.gpu_index)
        self.scratch = hip.Trlwe(widest * per, self.stream.gpu_index)
        self.sel_base = self._assign_bases() if self.stage_cb else {}
        self.trgsw = hip.Trgsw(K * sum(pt.addr_width for pt in self.ports), self.stream.gpu_index) if self.stage_cb else None
        self.refresh_stream = hip.Stream(self.stream.gpu_index) if refresh_aside else None   # one per engine, whatever the number of RAMs
        self.read_early, self._reads_pending = bool(read_early), False
        self.port_stream = hip.Stream(self.stream.gpu_index) if self.read_early else None   # P: one per engine, every memory lives on it
        self.mem_stream = self.port_stream if self.read_early else self.stream
        self.mem = {}
        for pt in self.ports:
            shared = {"trgsw": self.trgsw, "sel_base": self.sel_base[pt.name]} if self.stage_cb else {}
            if K > 1:   # stage-major selectors: lane r of a port sits + r * (the bits of the port's stage) from lane 0
                shared.update(lanes=K, arena_stride=self.lane_stride)
                if self.stage_cb:
                    shared["sel_stride"] = sum(q.addr_width for q in self._stage_ports(pt.stage))
            if pt.kind == "rom":
                log2w = pt.data_width.bit_length() - 1
                if 1 << log2w != pt.data_width or pt.data_width > N:
                    raise ValueError(f"ROM {pt.name!r}: a word of {pt.data_width} bits is no power of two up to N")
                rows = cmux.rom_layout(pt.addr_width, log2w, N).data_rows
                self.mem[pt.name] = cmux.Rom(self.mem_stream, np.zeros((rows, 2 * N), dtype=np.uint32), pt.addr_width, log2w, **shared)
            else:
                zero = np.zeros((pt.data_width << pt.addr_width, 2 * N), dtype=np.uint32)
                zero[:, N] = (-int(p.mu)) & 0xFFFFFFFF          # trivial TRLWEs of bit 0, as the DFFs start as trivial 0
                self.mem[pt.name] = cmux.Ram(self.mem_stream, zero, pt.addr_width, pt.data_width, **shared)

    def _stage_ports(self, s):
        """The ports of stage s in the order their address bits are concatenated in the stage's batch: port order."""
        return [pt for pt in self.ports if pt.stage == s]

    def _cb_bits(self):
        """Address bits of the widest circuit bootstrapping batch: the widest stage with stage_cb, else the widest port."""
        if not self.stage_cb:
            return max(pt.addr_width for pt in self.ports)
        return max(sum(pt.addr_width for pt in self.ports if pt.stage == s) for s in {pt.stage for pt in self.ports})

    def _assign_bases(self):
        """{port name: first selector slot (lane 0's)}: stage by stage, inside a stage in port order, a ROM and a RAM addr_width slots
        each (the engine reads one word per clock) — the ports of a stage are contiguous, in the order of _stage_ports.  With lanes the
        store is stage-major: stage s owns lanes x bits_s contiguous slots, lane r's copy of the stage + r * bits_s from lane 0's."""
        bases, nxt = {}, 0
        for s in sorted({pt.stage for pt in self.ports}):
            first = nxt
            for pt in self.ports:
                if pt.stage == s:
                    bases[pt.name] = nxt
                    nxt += pt.addr_width
            nxt = first + self.lanes * (nxt - first)
        return bases

    def _stage_first_slot(self, pts):
        return self.sel_base[pts[0].name]

    def _reads(self, s):
        if not self.stage_cb:
            return StagedPorts._reads(self, s)
        pts = self._stage_ports(s)
        if pts:
            self._stage_read(pts)

    def _stage_read(self, pts):
        self._stage_selectors(pts)
        for pt in pts:
            self._port_tree(pt)

    def _stage_selectors(self, pts):
        addr = self._lane_slots(np.concatenate([self._slots(pt.addr) for pt in pts]))   # lane-major: the stage-major selector slots
        self._cb_call()(self.bk2, self.privks_key, self.arena, addr, [1] * len(addr), self.tlwe2, 0, self.scratch, self.trgsw,
                        self._stage_first_slot(pts))

    def _cb_call(self):
        """The circuit bootstrapping of the memories' stream: per digit, or with cb_many one rotation per bit (the same arguments)."""
        return self.mem_stream.circuit_bootstrap_many_batch if self.cb_many else self.mem_stream.circuit_bootstrap_batch

    # ---- read_early: the reads on the port stream P, beside the executor's stream M (StagedPorts has the program order) ----
    def _read_groups(self, s):
        pts = self._stage_ports(s)
        return ([pts] if pts else []) if self.stage_cb else [[pt] for pt in pts]

    def _read_group(self, pts):
        if self.stage_cb:
            self._stage_read(pts)
        else:
            self._port_read(pts[0])

    def _fork(self):
        self.port_stream.wait_stream(self.stream)   # the address slots are final on M
        self._reads_pending = True

    def _join(self):
        if self._reads_pending:
            self.stream.wait_stream(self.port_stream)
            self._reads_pending = False

    def tick(self):
        if not self.read_early:
            return StagedPorts.tick(self)
        self.port_stream.wait_stream(self.stream)   # wren, wdata and the gate outputs are final
        self._write_ports()
        self.stream.wait_stream(self.port_stream)   # the chain has read wren / wdata / rdata before the commit copies overwrite DFF slots
        self.ex.tick()

    def _slots(self, nodes):
        slot = self.ex.plan.slot
        return np.array([slot[i] for i in nodes], dtype=np.int32)

    def _lane_slots(self, slots):
        """lane 0's arena slots for all lanes, lane-major; one lane: as they are"""
        if self.lanes == 1:
            return slots
        return (np.arange(self.lanes, dtype=np.int32)[:, None] * self.lane_stride + slots[None, :]).ravel().astype(np.int32)

    def _port_read(self, pt):
        self._port_selectors(pt)
        self._port_tree(pt)

    def _port_selectors(self, pt):
        mem = self.mem[pt.name]
        addr = self._lane_slots(self._slots(pt.addr))   # lane r's selectors land at r * addr_width: the memory's own sel_stride
        self._cb_call()(self.bk2, self.privks_key, self.arena, addr, [1] * len(addr), self.tlwe2, 0, self.scratch, mem.trgsw, 0)

    def _port_tree(self, pt):
        mem = self.mem[pt.name]
        if pt.kind == "rom":
            mem.read(None, self.arena, self._slots(pt.rdata).reshape(1, -1), resident=True, fused=self.rom_fused,
                     fused_tree=self.tree_fused)
        else:
            mem.read_port(self.arena, self._slots(pt.rdata), self.tree_fused)

    def _port_write(self, pt):
        aside = {} if self.refresh_stream is None else {"refresh_stream": self.refresh_stream}
        self.mem[pt.name].write_port(self.arena, int(self._slots(pt.wren)[0]), self._slots(pt.wdata), self._slots(pt.rdata), **aside)

    def _rows(self, table, name, lane=0):
        if self.packets[lane] is None:
            if self.lanes > 1:
                raise ValueError(f"CmuxLaneEngine needs the encrypted request of lane {lane} (packets=[TFHEPacket, ...]) for its memory images")
            raise ValueError("CmuxCipherEngine needs the encrypted request (packet=TFHEPacket) for its memory images")
        return getattr(self.packets[lane], table).get(name)

    def load_rom(self, name, request, lane=0):
        rows, rom = self._rows("rom", name, lane), self.mem[name]
        if rows is not None:
            rows = np.ascontiguousarray(rows, dtype=np.uint32).reshape(-1, 2 * rom.N)
            if rows.shape[0] > rom.layout.data_rows:
                raise ValueError(f"Invalid request packet: the image of {name!r} is longer than the memory")
            rom.trlwe.upload(self.mem_stream, lane * getattr(rom, "row_stride", 0), rows)

    def load_ram(self, name, request, lane=0):
        rows, ram = self._rows("ram", name, lane), self.mem[name]
        if rows is not None:
            rows = np.ascontiguousarray(rows, dtype=np.uint32).reshape(-1, 2 * ram.N)
            if rows.shape[0] != ram.ncells:
                raise ValueError("Invalid request packet: wrong length of RAM")
            ram.order_refresh()   # the upload overwrites the cell rows on the memories' stream
            # the packet's order is address * width + bit, the store's one plane of 2^addr_width cells per bit
            ram.trlwe.upload(self.mem_stream, lane * getattr(ram, "row_stride", 0),
                             rows.reshape(ram.cells_per_plane, ram.data_width, -1).transpose(1, 0, 2))

    def ram_rows(self, name, lane=0):
        """The cells of a RAM (lane `lane`'s) in the packet's order, u32 [2^addr_width * width][2N] (synchronises the stream)."""
        cells = self.mem[name].cells(**self._lane(lane))
        return np.ascontiguousarray(cells.transpose(1, 0, 2)).reshape(-1, cells.shape[2])

    def ram_image(self, name, lane=0):
        if self.decrypt_ram is None:
            raise ValueError("CmuxCipherEngine needs decrypt_ram to read a RAM image")
        return [int(b) for b in self.decrypt_ram(self.ram_rows(name, lane))]

    # ---- snapshot.EngineState (the argument for every store that is left out: DESIGN.md section 6e, "Snapshot and resume") ----
    def state(self, done=0, reset_ran=False):
        """CipherEngine's, behind pending device work: the main stream joins a pending early read in front of the arena's download
        (run() has joined already; a state() taken elsewhere still may not race it), Ram.cells() orders itself behind a refresh that
        runs aside, and the ROM rows come back through their store's download on the memories' stream.  No host synchronisation
        but what those downloads do."""
        self._join()
        return CipherEngine.state(self, done, reset_ran)

    def _state_meta(self, done, reset_ran):
        """cb_many is recorded where it is on (a snapshot without the key was taken with it off): the selectors a resume rebuilds, and
        every word after them, are those of the setting the snapshot's words came from."""
        meta = super()._state_meta(done, reset_ran)
        return dict(meta, cb_many=True) if self.cb_many else meta

    def check_state(self, snap):
        super().check_state(snap)
        if bool(snap.meta.get("cb_many", False)) != self.cb_many:
            raise ValueError(f"the snapshot was taken with cb_many={bool(snap.meta.get('cb_many', False))}, this engine has cb_many={self.cb_many}")

    def _mem_shape(self, pt):
        mem = self.mem[pt.name]
        return (mem.layout.data_rows, 2 * mem.N) if pt.kind == "rom" else (mem.data_width, mem.cells_per_plane, 2 * mem.N)

    def _read_mem(self, pt, lane):
        mem = self.mem[pt.name]
        if pt.kind == "ram":
            return mem.cells(**self._lane(lane))
        return mem.trlwe.download(mem.stream, lane * mem.row_stride, mem.layout.data_rows)

    def _write_mem(self, pt, lane, rows):
        self.mem[pt.name].upload_lane(lane, rows)   # a RAM's behind a pending refresh (order_refresh), both on the memories' stream

    def _before_load(self):
        self._join()   # the arena's upload overwrites rdata slots: behind an early read that still writes them

    def _after_load(self, snap):
        """The selectors of every RAM port: the next tick()'s write-back reads them (the address the last read saw) before any run()
        rewrites them.  The same circuit bootstrapping run() sends, from the restored address slots — fork and join as for a read."""
        rams = [pt for pt in self.ports if pt.kind == "ram"]
        if not rams:
            return
        if self.read_early:
            self._fork()
        for s in sorted({pt.stage for pt in rams}):
            if self.stage_cb:
                self._stage_selectors(self._stage_ports(s))
            else:
                for pt in rams:
                    if pt.stage == s:
                        self._port_selectors(pt)
        self._join()

    def free(self):
        if self.port_stream is not None:   # nothing is freed under a read, a chain or a refresh that still runs
            for m in self.mem.values():
                if hasattr(m, "order_refresh"):
                    m.order_refresh()
            self.port_stream.sync()
            self._reads_pending = False
        for m in self.mem.values():
            m.free()
        if self.trgsw is not None:
            self.trgsw.free()
        if self.refresh_stream is not None:
            self.refresh_stream.destroy()
            self.refresh_stream = None
        self.tlwe2.free()
        self.scratch.free()
        if self.port_stream is not None:
            self.port_stream.destroy()
            self.port_stream = None


class CmuxLaneEngine(CmuxCipherEngine):
    """CmuxCipherEngine for K request packets in one widened clock (run_packets): K = the lanes of the executor's backend
    (HipBackend(lanes=K)), `packets` = the K encrypted requests.  Every memory is a cmux.Rom / cmux.Ram(lanes=K): lane r's rows, selector
    slots and arena slots at fixed strides from lane 0's (csrc/cmux_lane_jobs.hpp).  ONE Stream.circuit_bootstrap_batch per port covers the
    address slots of all K lanes — K x addr_width x l rotations in the batch one lane pays for anyway — and with stage_cb ONE per stage,
    into a stage-major selector store (_assign_bases).  The flags are CmuxCipherEngine's; lane r's words are those of a one-lane
    CmuxCipherEngine given request r's ciphertexts.  One GPU."""

    port_lanes = True   # run_packets: the memory ports of this engine have lanes

    def __init__(self, system, executor, encrypt, decrypt, zero_row, bk2, privks_key, packets=None, decrypt_ram=None, words_only=False,
                 rom_fused=False, tree_fused=False, stage_cb=False, refresh_aside=False, read_early=False, cb_many=False):
        K = getattr(executor.be, "lanes", 1)
        packets = [None] * K if packets is None else list(packets)
        if len(packets) != K:
            raise ValueError(f"{len(packets)} packets for a backend with {K} lanes")
        self._setup(system, executor, encrypt, decrypt, zero_row, bk2, privks_key, packets, decrypt_ram, words_only, rom_fused, tree_fused,
                    stage_cb, refresh_aside, K, read_early, cb_many)


def _at_width(system, nl, name):
    widths = getattr(system, "at_widths", None)
    if widths and name in widths:
        return widths[name]
    return nl.port_width(nl.inputs, name)


class _Lane:
    """One lane of a laned engine as the engine run_packet's steps write to and read from.  run / tick do nothing here: the lanes
    share them, and run_packets calls the engine's own once all lanes have taken a step's writes."""

    def __init__(self, engine, lane):
        self.engine, self.lane = engine, lane

    def set_nodes(self, nids, bits):
        self.engine.set_nodes(nids, bits, **({"lane": self.lane} if self.lane else {}))

    def get_nodes(self, nids):
        return self.engine.get_nodes(nids, **({"lane": self.lane} if self.lane else {}))

    def load_rom(self, name, request):
        self.engine.load_rom(name, request, **({"lane": self.lane} if self.lane else {}))

    def load_ram(self, name, request):
        self.engine.load_ram(name, request, **({"lane": self.lane} if self.lane else {}))

    def ram_image(self, name):
        return self.engine.ram_image(name, **({"lane": self.lane} if self.lane else {}))


def _check_request(system, request, cycles):
    """What run_packet refuses in a request, found before anything runs."""
    nl = getattr(system, "nl", system)
    if "reset" in request.bits:
        raise ValueError("@reset cannot be set by user's input")
    if cycles < 0 and ("finflag", 0) not in nl.outputs:
        raise ValueError("the number of cycles is unspecified and the system has no @finflag")
    for name, cells in getattr(system, "ram", {}).items():
        image = request.ram.get(name)
        if image is not None and len(image) != len(cells):
            raise ValueError("Invalid request packet: wrong length of RAM")


def _load_roms(system, engine, request):
    """ROM contents exist from the start"""
    for name, cells in getattr(system, "rom", {}).items():
        image = request.rom.get(name)
        if image is not None:
            order = sorted(cells)
            engine.set_nodes([cells[i] for i in order], [image[i] if i < len(image) else 0 for i in order])
    for pt in getattr(system, "ports", []):
        if pt.kind == "rom":
            engine.load_rom(pt.name, request)


def _load_rams(system, engine, request):
    """setInitialRAM: the request's RAM images, written after the first tick"""
    for name, cells in getattr(system, "ram", {}).items():
        image = request.ram.get(name)
        if image is None:
            continue
        if len(image) != len(cells):
            raise ValueError("Invalid request packet: wrong length of RAM")
        order = sorted(cells)
        engine.set_nodes([cells[i] for i in order], [image[i] for i in order])
    for pt in getattr(system, "ports", []):
        if pt.kind == "ram":
            engine.load_ram(pt.name, request)


def _set_inputs(system, engine, request, done):
    """setCircularInputs: the @inputs of cycle `done`"""
    nl = getattr(system, "nl", system)
    nids, vals = [], []
    for (port, bit), nid in nl.inputs.items():
        stream = request.bits.get(port)
        if stream:
            width = _at_width(system, nl, port)
            nids.append(nid)
            vals.append(stream[(width * done + bit) % len(stream)])
    engine.set_nodes(nids, vals)


def _check_snapshot_args(snapshot_path, snapshot_every):
    if snapshot_every is not None:
        if snapshot_path is None:
            raise ValueError("snapshot_every without snapshot_path: there is no file to save to")
        if int(snapshot_every) < 1:
            raise ValueError(f"snapshot_every = {snapshot_every!r}: every m-th cycle, m at least 1")


def _check_resume(nl, engine, resume, cycles, skip_reset):
    """The Snapshot of run_packet(resume=), refused (ValueError) before the engine is touched where the run cannot continue from it."""
    snap = as_snapshot(resume)
    if 0 <= cycles < snap.done:
        raise ValueError(f"cycles = {cycles} is the total number of cycles, the snapshot has run {snap.done} already")
    if ("reset", 0) in nl.inputs and not skip_reset and not snap.reset_ran:
        raise ValueError("the snapshot says the reset cycle never ran, and this run asks for it (skip_reset=False)")
    if not hasattr(engine, "check_state"):
        raise ValueError(f"{type(engine).__name__} cannot load a snapshot")
    engine.check_state(snap)
    return snap


def _save_due(snapshot_path, snapshot_every, done, last):
    return snapshot_path is not None and (last or (snapshot_every is not None and done % int(snapshot_every) == 0))


def run_packet(system, request, cycles=None, engine=None, skip_reset=False, on_cycle=None, snapshot_path=None, snapshot_every=None,
               resume=None):
    """Run `system` (a `System` from `load_blueprint`, or a bare `Netlist`) on the request packet.
    `cycles`: None -> the packet's own `cycles`, else -1 -> until @finflag.  Returns the result packet.
    snapshot_path: the engine's state (engine.state(), snapshot.Snapshot) is saved there after the last cycle, and with snapshot_every=m
    after every m-th cycle as well (each save replaces the file as a whole).
    resume: a Snapshot or the path of one.  The ROM images, the reset cycle and the cycle-0 RAM images are skipped, the state is loaded
    into `engine` and the run goes on at the snapshot's `done`: `cycles` stays the TOTAL number of cycles (cycles=6 from a snapshot at 3
    runs 3 more), the circular inputs continue where they were, and -1 runs on until @finflag.  The request and the engine's keys are
    supplied as for a new run; a snapshot that does not fit is refused before the engine is touched."""
    nl = getattr(system, "nl", system)
    ports = getattr(system, "ports", [])
    if engine is None:
        if ports:
            raise ValueError("a system with CMUX memory ports needs a staged engine (StagedBitsEngine / CmuxCipherEngine)")
        engine = PlainEngine(nl)
    if cycles is None:
        cycles = request.cycles if request.cycles is not None else -1
    _check_snapshot_args(snapshot_path, snapshot_every)

    def set_input(port, bit, v):
        engine.set_nodes([nl.inputs[(port, bit)]], [v])

    def get_output(port, bit):
        return engine.get_nodes([nl.outputs[(port, bit)]])[0]

    has_finflag = ("finflag", 0) in nl.outputs
    if resume is not None:
        _check_request(system, request, cycles)
        snap = _check_resume(nl, engine, resume, cycles, skip_reset)
        engine.load_state(snap)
        done, reset_ran = snap.done, snap.reset_ran
        negate_reset = reset_ran and done == 0              # a snapshot of the reset cycle itself: cycle 0 is still to come
        finished = cycles < 0 and done > 0 and get_output("finflag", 0) == 1
    else:
        _load_roms(system, engine, request)

        if "reset" in request.bits:
            raise ValueError("@reset cannot be set by user's input")
        has_reset = ("reset", 0) in nl.inputs
        negate_reset = False
        if has_reset and not skip_reset:
            set_input("reset", 0, 1)
            engine.run()
            negate_reset = True

        if cycles < 0 and not has_finflag:
            raise ValueError("the number of cycles is unspecified and the system has no @finflag")
        done, reset_ran, finished = 0, negate_reset, False
    while not finished and (cycles < 0 or done < cycles):
        engine.tick()
        if done == 0:
            if negate_reset:
                set_input("reset", 0, 0)
            _load_rams(system, engine, request)
        _set_inputs(system, engine, request, done)
        engine.run()
        done += 1
        if on_cycle is not None:
            on_cycle(done, engine)
        finished = cycles < 0 and get_output("finflag", 0) == 1
        if _save_due(snapshot_path, snapshot_every, done, finished or done == cycles):
            engine.state(done=done, reset_ran=reset_ran).save(snapshot_path)
    return result_packet(system, engine, done)


def run_packets(system, requests, cycles=None, engine=None, skip_reset=False, snapshot_path=None, snapshot_every=None, resume=None):
    """K request packets of one system in ONE run: request r lives in lane r of `engine` (PlainEngine(nl, lanes=K), or a CipherEngine on
    a backend with lanes=K: every level of every clock is then ONE batch of count x K gates on the GPU).  Lane r goes through
    run_packet's steps with requests[r] — ROM images, the reset cycle, the cycle-0 RAM images, the circular inputs — and result r is what
    run_packet(system, requests[r]) returns alone; the lanes share only the clock.
    So the requests have to agree on what the clock needs: `cycles` (None: each packet's own) is ONE number of cycles, which an
    until-@finflag run (-1) cannot be — lanes finish on their own clocks; requests that disagree, and what run_packet refuses in any
    of them, are refused before anything runs.  CMUX memory ports have no lanes (CmuxCipherEngine): run the lowered (mux-*) system.
    snapshot_path / snapshot_every / resume: run_packet's, all K lanes in one file."""
    nl = getattr(system, "nl", system)
    requests = list(requests)
    if not requests:
        raise ValueError("no request packet")
    if getattr(system, "ports", []) and not getattr(engine, "port_lanes", False):
        raise ValueError("a system with CMUX memory ports runs one request at a time: CMUX memories have no lanes (use the lowered mux-* form)")
    each = [cycles if cycles is not None else (r.cycles if r.cycles is not None else -1) for r in requests]
    if len(set(each)) != 1:
        raise ValueError(f"the request packets disagree on the number of cycles: {each}")
    cycles = each[0]
    if cycles < 0:
        raise ValueError("lanes share one clock: run_packets needs a number of cycles, not a run until @finflag")
    for r in requests:
        _check_request(system, r, cycles)
    if engine is None:
        engine = PlainEngine(nl, lanes=len(requests))
    if getattr(engine, "lanes", 1) != len(requests):
        raise ValueError(f"{len(requests)} request packets for an engine with {getattr(engine, 'lanes', 1)} lanes")
    _check_snapshot_args(snapshot_path, snapshot_every)
    lanes = [_Lane(engine, r) for r in range(len(requests))]

    if resume is not None:
        snap = _check_resume(nl, engine, resume, cycles, skip_reset)
        engine.load_state(snap)
        first, reset_ran = snap.done, snap.reset_ran
        negate_reset = reset_ran and first == 0
    else:
        for lane, request in zip(lanes, requests):
            _load_roms(system, lane, request)
        negate_reset = ("reset", 0) in nl.inputs and not skip_reset
        if negate_reset:
            for lane in lanes:
                lane.set_nodes([nl.inputs[("reset", 0)]], [1])
            engine.run()
        first, reset_ran = 0, negate_reset
    for done in range(first, cycles):
        engine.tick()
        for lane, request in zip(lanes, requests):
            if done == 0:
                if negate_reset:
                    lane.set_nodes([nl.inputs[("reset", 0)]], [0])
                _load_rams(system, lane, request)
            _set_inputs(system, lane, request, done)
        engine.run()
        if _save_due(snapshot_path, snapshot_every, done + 1, done + 1 == cycles):
            engine.state(done=done + 1, reset_ran=reset_ran).save(snapshot_path)
    return [result_packet(system, lane, cycles) for lane in lanes]


def result_packet(system, engine, cycles):
    """makeResPacket (/root/reference/src/iyokan_plain.cpp:174-224): every @output port, every RAM image."""
    nl = getattr(system, "nl", system)
    res = PlainPacket(cycles=cycles)
    keys = sorted(nl.outputs)
    vals = engine.get_nodes([nl.outputs[k] for k in keys])
    for name in sorted({p for (p, _) in keys}):
        res.bits[name] = [0] * nl.port_width(nl.outputs, name)
    for (name, b), v in zip(keys, vals):
        res.bits[name][b] = int(v)
    for name, cells in getattr(system, "ram", {}).items():
        order = sorted(cells)
        res.ram[name] = [int(v) for v in engine.get_nodes([cells[i] for i in order])]
    for pt in getattr(system, "ports", []):
        if pt.kind == "ram":
            res.ram[pt.name] = [int(v) for v in engine.ram_image(pt.name)]
    return res
