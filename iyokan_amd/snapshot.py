"""Snapshot and resume of a run: the state of an engine at a clock edge, as a plain object and as a file.

Replaces the reference's `--snapshot FILE` / `--resume FILE` (/root/reference/src/main.cpp:67-174, which serialises every task with
cereal) for the Python engines of runner.py.  The file formats are NOT compatible: this one is a numpy archive of this project's own
arena and memory layouts.

State is defined AFTER run() of cycle `done` and BEFORE the next tick() — where run_packet calls on_cycle.  Per lane it is
    the arena       every slot of the plan (plan.slot over all nodes; PlainEngine: every node's value): DFF cells, sources, inputs,
                    rdata slots, gate outputs — tick() reads the D side of every DFF and, for a RAM port, wren / wdata / rdata
    every RAM port  its cell rows u32 [data_width][2^addr_width][2N] (cmux.Ram.cells, behind a pending refresh); bits engines: the image
    every ROM port  its TRLWE rows u32 [data_rows][2N], downloaded from the ROM's store; bits engines: the image
and the scalars: done, whether the reset cycle ran, lanes, the parameter set, the engine's class name and kind, a digest of the system.
No key of any kind and nothing of the request packet's input streams: the resuming caller supplies keys and request as for a new run.

What is NOT state is rebuilt before it is read (DESIGN.md section 6e has the list) — with one exception the next tick() reads before any
run() rewrites it: a RAM's write-back uses the selectors of the address the last read saw.  load_state() rebuilds them from the restored
address slots (the same circuit bootstrapping over the same words, hence the same selectors; the bits engines recompute the address).

EngineState is the mixin the engines of runner.py take state() / check_state() / load_state() from; an engine supplies the hooks
(_state_slots, _read_slots, _write_slots, _read_mem, _write_mem, _mem_shape, _state_params, _before_load, _after_load).
"""
import hashlib
import json
import os
import zipfile

import numpy as np

VERSION = 1
PARAM_NAMES = ("n", "N", "k", "l", "Bgbit", "t", "basebit")


def system_digest(nl, ports, slot):
    """sha256 over the netlist's nodes and kinds, its @port tables, the memory ports (name, kind, widths) and plan.slot (None: no plan)"""
    table = lambda t: sorted([str(p), int(b), int(v)] for (p, b), v in t.items())
    what = [list(nl.kinds), [[int(j) for j in ins] for ins in nl.ins], table(nl.inputs), table(nl.outputs),
            [[pt.name, pt.kind, int(pt.addr_width), int(pt.data_width)] for pt in ports], None if slot is None else [int(s) for s in slot]]
    return hashlib.sha256(json.dumps(what).encode()).hexdigest()


class Snapshot:
    """The state of an engine at a clock edge.  meta: the scalars (a dict that JSON holds); slots: the arena slots saved, i32 [S];
    arena: [lanes][S] u8 bits or [lanes][S][n+1] u32 words; ram / rom: {port name: [lanes] + the memory's shape}."""

    def __init__(self, meta, slots, arena, ram, rom):
        self.meta, self.slots, self.arena, self.ram, self.rom = dict(meta), np.asarray(slots, dtype=np.int32), arena, dict(ram), dict(rom)

    done = property(lambda self: int(self.meta["done"]))
    reset_ran = property(lambda self: bool(self.meta["reset_ran"]))
    lanes = property(lambda self: int(self.meta["lanes"]))

    def __eq__(self, other):
        if not isinstance(other, Snapshot):
            return NotImplemented
        same = lambda a, b: a.dtype == b.dtype and a.shape == b.shape and np.array_equal(a, b)
        return (self.meta == other.meta and same(self.slots, other.slots) and same(self.arena, other.arena)
                and all(sorted(a) == sorted(b) and all(same(a[n], b[n]) for n in a) for a, b in ((self.ram, other.ram), (self.rom, other.rom))))

    __hash__ = None

    def _arrays(self):
        meta = dict(self.meta, ram=sorted(self.ram), rom=sorted(self.rom))
        out = {"version": np.array([VERSION], dtype=np.uint32),
               "meta": np.frombuffer(json.dumps(meta, sort_keys=True).encode("utf-8"), dtype=np.uint8), "slots": self.slots, "arena": self.arena}
        out.update({"ram." + n: a for n, a in self.ram.items()})
        out.update({"rom." + n: a for n, a in self.rom.items()})
        return out

    def save(self, path):
        """One uncompressed numpy.savez archive of arrays only, the version first.  Written to path + ".tmp", then os.replace: a writer
        that is killed, or whose replace fails, leaves what was under `path` as it was."""
        path = os.fspath(path)
        tmp = path + ".tmp"
        try:
            with open(tmp, "wb") as f:
                np.savez(f, **self._arrays())
                f.flush()
                os.fsync(f.fileno())
            os.replace(tmp, path)
        finally:
            if os.path.exists(tmp):
                os.remove(tmp)

    @classmethod
    def load(cls, path):
        """Refuses (ValueError) a file that is no archive or a truncated one, an unknown version and a missing array."""
        path = os.fspath(path)
        try:
            with np.load(path, allow_pickle=False) as z:
                if "version" not in z.files:
                    raise ValueError(f"{path}: no snapshot (the archive has no version)")
                version = int(np.asarray(z["version"]).ravel()[0])
                if version != VERSION:
                    raise ValueError(f"{path}: snapshot format version {version}, this build reads version {VERSION}")
                missing = [k for k in ("meta", "slots", "arena") if k not in z.files]
                if not missing:
                    meta = json.loads(bytes(np.asarray(z["meta"], dtype=np.uint8)).decode("utf-8"))
                    names = [(kind, n) for kind in ("ram", "rom") for n in meta.get(kind, [])]
                    missing = [f"{kind}.{n}" for kind, n in names if f"{kind}.{n}" not in z.files]
                if missing:
                    raise ValueError(f"{path}: the snapshot lacks the array(s) {', '.join(missing)}")
                mems = {kind: {n: z[f"{kind}.{n}"] for k, n in names if k == kind} for kind in ("ram", "rom")}
                slots, arena = z["slots"], z["arena"]
        except (zipfile.BadZipFile, EOFError) as e:
            raise ValueError(f"{path}: not a complete snapshot archive ({e})") from e
        for k in ("ram", "rom"):
            meta.pop(k, None)
        return cls(meta, slots, arena, mems["ram"], mems["rom"])


def as_snapshot(resume):
    """run_packet(resume=): a Snapshot as it is, a path loaded"""
    return resume if isinstance(resume, Snapshot) else Snapshot.load(resume)


class EngineState:
    """state() / check_state() / load_state() of an engine, over the hooks named in the module docstring."""

    state_kind = "bits"   # "cipher": the arena holds TLWE words and the memories TRLWE rows

    # ---- hooks, with what an engine on a FrontierExecutor wants ----
    def _state_plan_slot(self):
        return self.ex.plan.slot

    def _state_slots(self):
        """the arena slots that are state: every slot of the plan (an OUTPUT wire shares its driver's)"""
        return sorted(set(int(s) for s in self._state_plan_slot() if s >= 0))

    def _state_ports(self):
        return list(getattr(self, "ports", []))

    def _state_params(self):
        return None

    def _slot_shape(self):
        """the shape of one arena slot: () a bit, (n + 1,) a TLWE"""
        return ()

    def _before_load(self):
        pass

    def _after_load(self, snap):
        pass

    # ---- the three calls ----
    def _state_meta(self, done, reset_ran):
        nl = self.nl
        return {"done": int(done), "reset_ran": bool(reset_ran), "lanes": int(self.lanes), "params": self._state_params(),
                "engine": type(self).__name__, "kind": self.state_kind,
                "digest": system_digest(nl, self._state_ports(), self._state_plan_slot())}

    def state(self, done=0, reset_ran=False):
        """The engine's state as a Snapshot, taken after run() of cycle `done` and before the next tick().  `done` and `reset_ran` are
        the runner's (run_packet passes its own); an engine clocked by hand may leave them out."""
        slots = self._state_slots()
        arena = np.stack([np.asarray(self._read_slots(slots, lane)) for lane in range(self.lanes)])
        ram, rom = {}, {}
        for pt in self._state_ports():
            (ram if pt.kind == "ram" else rom)[pt.name] = np.stack([np.asarray(self._read_mem(pt, lane)) for lane in range(self.lanes)])
        return Snapshot(self._state_meta(done, reset_ran), slots, arena, ram, rom)

    def check_state(self, snap):
        """Refuses (ValueError, naming what disagrees) a snapshot that is not of this engine's kind, parameter set, lane count, system or
        memory shapes.  Touches nothing."""
        mine = self._state_meta(0, False)
        if snap.meta.get("kind") != mine["kind"]:
            raise ValueError(f"the snapshot is of a {snap.meta.get('kind')} engine ({snap.meta.get('engine')}), this engine "
                             f"({mine['engine']}) holds {mine['kind']}")
        if snap.meta.get("params") != mine["params"]:
            raise ValueError(f"the snapshot's parameter set {snap.meta.get('params')} is not this engine's {mine['params']}")
        if snap.meta.get("lanes") != mine["lanes"]:
            raise ValueError(f"the snapshot holds {snap.meta.get('lanes')} lanes, this engine has {mine['lanes']}")
        ports = self._state_ports()
        for pt in ports:
            have = (snap.ram if pt.kind == "ram" else snap.rom).get(pt.name)
            want = (self.lanes,) + tuple(self._mem_shape(pt))
            if have is not None and tuple(have.shape) != want:
                raise ValueError(f"{pt.kind.upper()} {pt.name!r}: the snapshot's shape {tuple(have.shape)} is not this engine's {want}")
        if snap.meta.get("digest") != mine["digest"]:
            raise ValueError(f"the snapshot's system digest {str(snap.meta.get('digest'))[:12]}... is not this engine's {mine['digest'][:12]}... "
                             "(another netlist, port list or slot assignment)")
        for pt in ports:
            if pt.name not in (snap.ram if pt.kind == "ram" else snap.rom):
                raise ValueError(f"the snapshot lacks {pt.kind.upper()} {pt.name!r}")
        slots = self._state_slots()
        if list(snap.slots) != slots or snap.arena.shape[:2] != (self.lanes, len(slots)) or snap.arena.shape[2:] != self._slot_shape():
            raise ValueError(f"the snapshot's arena {snap.arena.shape} over {len(snap.slots)} slots is not this engine's "
                             f"{(self.lanes, len(slots)) + self._slot_shape()}")

    def load_state(self, snap):
        """Writes a Snapshot back, into a fresh engine or over whatever this one holds: checked first (check_state), written second, so a
        refused snapshot leaves the arena and the memories as they were.  Ordered behind pending device work and in front of the next
        tick() by the engine's hooks."""
        self.check_state(snap)
        self._before_load()
        slots = self._state_slots()
        for lane in range(self.lanes):
            self._write_slots(slots, snap.arena[lane], lane)
            for pt in self._state_ports():
                self._write_mem(pt, lane, (snap.ram if pt.kind == "ram" else snap.rom)[pt.name][lane])
        self._after_load(snap)
