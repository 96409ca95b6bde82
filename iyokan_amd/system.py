"""Blueprint -> one flat netlist (the caller side of the hot path needed by BASELINE config #4).

Covers the subset of Iyokan's TOML blueprint that the CAHP-with-MUX-memories systems use
(/root/reference/src/iyokan.hpp:1691-1895; example /root/reference/test/config-toml/cahp-ruby-mux.toml):

  [[file]]    type = "yosys-json" | "iyokanl1-json", path, name
  [[builtin]] type = "mux-rom" (in_addr_width, out_rdata_width)       -> makeROMWithMUX  (:2517-2593)
              type = "mux-ram" (in_addr_width, in_wdata_width = out_rdata_width) -> makeRAMWithMUX (:2595-2762):
                       the precompiled 8/16/16 netlist when its JSON is at hand, else the generated DMUX/MUX form
              type = "rom" / "ram": the reference keeps these in CMUX memories evaluated by TFHEpp on the CPU; they have
                       the same ports and the same observable behaviour as the MUX forms (the reference's fixtures are
                       shared between the two).  load_blueprint(cmux_memories=False), the default, LOWERS them to the
                       MUX forms on the gate path; cmux_memories=True keeps each as a memory PORT (MemPort) for
                       cmux.Rom / cmux.Ram behind circuit bootstrapping (runner.CmuxCipherEngine): address, wren and
                       wdata bits end at sink nodes, rdata bits start at source nodes, and every node gets a STAGE
  [connect]   "dst/port[a:b]" = "src/port[a:b]"   internal edge (dst input <- src output)
              "dst/port"      = "@name[a:b]"      system input  @name drives dst's input port
              "@name[a:b]"    = "src/port[a:b]"   system output @name reads src's output port
              TOGND = ["@name[a:b]", ...]         declares (and thereby widens) @ports that drive nothing

All sub-netlists are merged into ONE `Netlist`, connected inputs become alias wires of their drivers,
so the plaintext simulator, the levelizer and the frontier executor run the whole system as a single
DAG per clock.  ROM cells are INPUT-like nodes (`nl.rom[index]`), RAM cells DFFs (`nl.ram[index]`).
"""
import os
import re
from collections import namedtuple

import tomli

from . import netlist as N

_PORT = re.compile(r"^(?:(?P<node>[^/@\[]+)/|@)(?P<port>[^\[\]/]+)(?:\[(?P<a>\d+)(?::(?P<b>\d+))?\])?$")


def _parse_ports(s):
    m = _PORT.match(s.strip())
    if not m:
        raise ValueError(f"Invalid port string: {s!r}")
    node = m.group("node")  # None for @ports
    port = m.group("port")
    if m.group("a") is None:
        bits = [0]
    elif m.group("b") is None:
        bits = [int(m.group("a"))]
    else:
        a, b = int(m.group("a")), int(m.group("b"))
        if b < a:
            raise ValueError(f"Invalid port range: {s!r}")
        bits = list(range(a, b + 1))
    return node, port, bits


def make_rom_with_mux(in_addr_width, out_rdata_width):
    """MUX-tree ROM: per output bit, 2^aw ROM cells reduced by aw levels of MUX(A=even, B=odd, S=addr[i])."""
    nl = N.Netlist()
    nl.rom = {}
    addr = []
    for i in range(in_addr_width):
        nid = nl.add("INPUT")
        nl.inputs[("addr", i)] = nid
        addr.append(nid)
    for bit in range(out_rdata_width):
        work = []
        for i in range(1 << in_addr_width):
            nid = nl.add("INPUT")
            nl.rom[bit + i * out_rdata_width] = nid
            work.append(nid)
        for i in range(in_addr_width):
            work = [nl.add("MUX", [work[j], work[j + 1], addr[i]]) for j in range(0, len(work), 2)]
        out = nl.add("OUTPUT", [work[0]])
        nl.outputs[("rdata", bit)] = out
    return nl


def make_ram_with_mux(in_addr_width, data_width):
    """MUX RAM, the structure of make1bitRAMWithMUX (/root/reference/src/iyokan.hpp:2648-2762): wren is
    demultiplexed over the address bits (msb first: out0 = ANDNOT(in, a), out1 = AND(in, a)) into one
    write-select per word; cell (addr, bit) = DFF fed by MUX(A = itself, B = wdata[bit], S = select[addr]);
    the read side reduces the 2^aw cells of a bit with aw levels of MUX(even, odd, addr[i]), lsb first.
    The select tree is shared by all data bits (the reference rebuilds it per bit; same function)."""
    nl = N.Netlist()
    addr = []
    for i in range(in_addr_width):
        nid = nl.add("INPUT")
        nl.inputs[("addr", i)] = nid
        addr.append(nid)
    wren = nl.add("INPUT")
    nl.inputs[("wren", 0)] = wren
    sel = [wren]
    for a in reversed(addr):
        nxt = []
        for src in sel:
            nxt.append(nl.add("ANDNOT", [src, a]))
            nxt.append(nl.add("AND", [src, a]))
        sel = nxt
    for bit in range(data_width):
        wdata = nl.add("INPUT")
        nl.inputs[("wdata", bit)] = wdata
        work = []
        for a in range(1 << in_addr_width):
            mux = nl.add("MUX", [0, wdata, sel[a]])     # A patched below: the cell itself
            ram = nl.add("DFF", [mux])
            nl.ins[mux][0] = ram
            nl.ram[a * data_width + bit] = ram
            work.append(ram)
        for i in range(in_addr_width):
            work = [nl.add("MUX", [work[j], work[j + 1], addr[i]]) for j in range(0, len(work), 2)]
        out = nl.add("OUTPUT", [work[0]])
        nl.outputs[("rdata", bit)] = out
    nl.validate()
    return nl


# One CMUX memory of a system (load_blueprint(cmux_memories=True)).  addr / wren / wdata: the sink nodes its inputs end at (bit 0
# first; wren and wdata are empty for a ROM); rdata: the source nodes (kind INPUT, so they own arena slots) its read data starts at;
# stage: the highest stage among the address drivers — rdata and everything downstream of it sit one stage later.
MemPort = namedtuple("MemPort", "kind name addr_width data_width addr wren wdata rdata stage")


def make_memory_port(kind, in_addr_width, data_width):
    """The netlist side of a CMUX memory: nothing but its pins.  Inputs are INPUT nodes (aliases of their drivers once connected),
    rdata bits INPUT nodes that the memory itself writes."""
    nl = N.Netlist()
    for i in range(in_addr_width):
        nl.inputs[("addr", i)] = nl.add("INPUT")
    if kind == "ram":
        nl.inputs[("wren", 0)] = nl.add("INPUT")
        for i in range(data_width):
            nl.inputs[("wdata", i)] = nl.add("INPUT")
    for i in range(data_width):
        nl.outputs[("rdata", i)] = nl.add("INPUT")
    return nl


def assign_stages(nl, ports):
    """(stage of every node, the ports with their stage filled in).  Sources are stage 0, a gate has the highest stage among its
    inputs, a port the highest among its address nodes, its rdata nodes one more.  A port whose address depends on its own rdata,
    directly or through other ports, is a combinational loop: ValueError naming it."""
    n = nl.num_nodes
    nl._topo()                                              # a loop among the gates alone is the netlist's own error
    deps = [[] for _ in range(n)]
    indeg = [0] * n
    for i in range(n):
        if nl.kinds[i] == "DFF":
            continue                                        # a DFF's input belongs to the next clock
        for j in nl.ins[i]:
            deps[j].append(i)
            indeg[i] += 1
    owner = {}
    for k, pt in enumerate(ports):
        for r in pt.rdata:
            owner[r] = k
            for a in pt.addr:
                deps[a].append(r)
                indeg[r] += 1
    stage = [0] * n
    stack = [i for i in range(n) if indeg[i] == 0]
    done = 0
    while stack:
        i = stack.pop()
        done += 1
        if i in owner:
            stage[i] = 1 + max(stage[a] for a in ports[owner[i]].addr)
        elif nl.kinds[i] != "DFF" and nl.ins[i]:
            stage[i] = max(stage[j] for j in nl.ins[i])
        for d in deps[i]:
            indeg[d] -= 1
            if indeg[d] == 0:
                stack.append(d)
    if done != n:
        stuck = sorted({ports[k].name for r, k in owner.items() if indeg[r] > 0})
        raise ValueError("combinational loop: the address of memory port " + ", ".join(repr(s_) for s_ in stuck)
                         + " depends on its own rdata")
    return stage, [pt._replace(stage=max(stage[a] for a in pt.addr)) for pt in ports]


class System:
    """Merged netlist + where the blueprint's named things ended up."""

    def __init__(self, nl, at_inputs, at_outputs, rom, ram, at_widths=None, ram_shapes=None, rom_shapes=None, ports=None, stages=None):
        self.nl = nl
        self.at_inputs = at_inputs      # (name, bit) -> node id (INPUT)
        self.at_outputs = at_outputs    # (name, bit) -> node id
        self.rom = rom                  # builtin name -> {index: node id}
        self.ram = ram                  # builtin name -> {index: node id}
        self.at_widths = at_widths or {}    # @port name -> declared width (incl. TOGND bits)
        self.ram_shapes = ram_shapes or {}  # builtin name -> (addr width, data width)
        self.rom_shapes = rom_shapes or {}
        self.ports = ports or []            # CMUX memories (MemPort), empty unless load_blueprint(cmux_memories=True) found some
        self.stages = stages                # node id -> stage when there are ports, else None
        self.num_stages = 1 + max(stages) if stages else 1

    def at_width(self, table, name):
        if name in self.at_widths:
            return self.at_widths[name]
        return 1 + max(b for (p, b) in table if p == name)


def load_blueprint(path, mux_ram_dir=None, cmux_memories=False):
    """cmux_memories=True: "rom" / "ram" builtins stay memories (System.ports, System.stages) instead of being lowered to the MUX
    forms; "mux-rom" / "mux-ram" are MUX memories either way."""
    base = os.path.dirname(os.path.abspath(path))
    with open(path, "rb") as f:
        bp = tomli.load(f)
    parts = {}
    for fdesc in bp.get("file", []):
        p = fdesc["path"] if os.path.isabs(fdesc["path"]) else os.path.join(base, fdesc["path"])
        if fdesc["type"] == "yosys-json":
            parts[fdesc["name"]] = N.load_yosys_json(p)
        elif fdesc["type"] == "iyokanl1-json":
            parts[fdesc["name"]] = N.load_iyokanl1_json(p)
        else:
            raise ValueError(f"Invalid file type: {fdesc['type']}")
    ram_shapes, rom_shapes, port_shapes = {}, {}, {}
    for b in bp.get("builtin", []):
        if cmux_memories and b["type"] in ("rom", "ram"):
            if b["type"] == "ram" and b["in_wdata_width"] != b["out_rdata_width"]:
                raise ValueError("Invalid RAM size; RAM with different write/read data widths is not implemented")
            parts[b["name"]] = make_memory_port(b["type"], b["in_addr_width"], b["out_rdata_width"])
            port_shapes[b["name"]] = (b["type"], b["in_addr_width"], b["out_rdata_width"])
        elif b["type"] in ("mux-rom", "rom"):
            parts[b["name"]] = make_rom_with_mux(b["in_addr_width"], b["out_rdata_width"])
            rom_shapes[b["name"]] = (b["in_addr_width"], b["out_rdata_width"])
        elif b["type"] in ("mux-ram", "ram"):
            if b["in_wdata_width"] != b["out_rdata_width"]:
                raise ValueError("Invalid RAM size; RAM with different write/read data widths is not implemented")
            # the reference embeds minimised netlists for some shapes (USE_PRECOMPILED_BINARY, iyokan.hpp:2609-2625):
            # use the same file when it is at hand (next to the blueprint, one level up, or in mux_ram_dir)
            fname = "mux-ram-{}-{}-{}.min.json".format(b["in_addr_width"], b["in_wdata_width"], b["out_rdata_width"])
            cands = [os.path.join(d, fname) for d in ([mux_ram_dir] if mux_ram_dir else []) + [base, os.path.dirname(base)]]
            pre = next((c for c in cands if os.path.exists(c)), None)
            if pre:
                parts[b["name"]] = N.load_iyokanl1_json(pre, ram_width=b["in_wdata_width"])
            else:
                parts[b["name"]] = make_ram_with_mux(b["in_addr_width"], b["in_wdata_width"])
            ram_shapes[b["name"]] = (b["in_addr_width"], b["in_wdata_width"])
        else:
            raise ValueError(f"Invalid builtin type: {b['type']}")

    # ---- merge: renumber every part into one node space ---------------------------------------
    nl = N.Netlist()
    offset, rom, ram = {}, {}, {}
    for name, part in parts.items():
        offset[name] = nl.num_nodes
        off = offset[name]
        for k, ins in zip(part.kinds, part.ins):
            nl.kinds.append(k)
            nl.ins.append([i + off for i in ins])
        for nid, v in part.dff_init.items():
            nl.dff_init[nid + off] = v
        if getattr(part, "rom", None):
            rom[name] = {idx: nid + off for idx, nid in part.rom.items()}
        if part.ram:
            ram[name] = {idx: nid + off for idx, nid in part.ram.items()}

    def in_node(node, port, bit):
        try:
            return parts[node].inputs[(port, bit)] + offset[node]
        except KeyError:
            raise ValueError(f"no input port {node}/{port}[{bit}]")

    def out_node(node, port, bit):
        try:
            return parts[node].outputs[(port, bit)] + offset[node]
        except KeyError:
            raise ValueError(f"no output port {node}/{port}[{bit}]")

    at_inputs, at_outputs, at_widths = {}, {}, {}

    def widen(name, bit):
        at_widths[name] = max(at_widths.get(name, 0), bit + 1)

    for dst, src in bp.get("connect", {}).items():
        if dst == "TOGND":
            for port_str in src:
                if not port_str.startswith("@"):
                    raise ValueError(f"Invalid port name for TOGND: {port_str}")
                _, gport, gbits = _parse_ports(port_str)
                for gb in gbits:
                    widen(gport, gb)
            continue
        if not dst or not src or (dst[0] == "@" and src[0] == "@"):
            raise ValueError(f"Invalid connect: {dst} = {src}")
        dnode, dport, dbits = _parse_ports(dst)
        snode, sport, sbits = _parse_ports(src)
        if len(dbits) != len(sbits):
            raise ValueError(f"Invalid connect: {dst} = {src}")
        for db, sb in zip(dbits, sbits):
            if dnode is None:                      # "@out" = "node/port"
                if snode is None:
                    raise ValueError(f"Invalid connect: {dst} = {src}")
                at_outputs.setdefault((dport, db), out_node(snode, sport, sb))
                widen(dport, db)
            elif snode is None:                    # "node/port" = "@in"
                at_inputs.setdefault((sport, sb), in_node(dnode, dport, db))
                widen(sport, sb)
            else:                                  # internal edge: dst input becomes an alias of src output
                d = in_node(dnode, dport, db)
                nl.kinds[d] = "OUTPUT"
                nl.ins[d] = [out_node(snode, sport, sb)]
    # system-level port tables; unconnected sub-net inputs stay plain INPUT nodes (value 0 unless set)
    nl.inputs = dict(at_inputs)
    nl.outputs = dict(at_outputs)
    for name, cells in ram.items():
        nl.ram.update({(name, idx): nid for idx, nid in cells.items()})
    nl.validate()
    if not port_shapes:
        return System(nl, at_inputs, at_outputs, rom, ram, at_widths, ram_shapes, rom_shapes)
    ports = []
    for name, (kind, aw, dw) in port_shapes.items():
        pins = lambda table, port, width: [table[(port, i)] + offset[name] for i in range(width)]
        pi, po = parts[name].inputs, parts[name].outputs
        ports.append(MemPort(kind, name, aw, dw, pins(pi, "addr", aw), pins(pi, "wren", 1) if kind == "ram" else [],
                             pins(pi, "wdata", dw) if kind == "ram" else [], pins(po, "rdata", dw), 0))
    stages, ports = assign_stages(nl, ports)
    return System(nl, at_inputs, at_outputs, rom, ram, at_widths, ram_shapes, rom_shapes, ports, stages)
