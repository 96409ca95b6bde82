#!/usr/bin/env python3
"""Model-predicted 1 / 2 / 4 / 8-GPU table for BASELINE.json's configs #2 - #5, from a CALIBRATED level-cost table
("so the driver's first real SCALE record has something to be checked against").

No GPU needed: the inputs are numbers a 1-GPU box measured (tools/gpu_round.sh writes them to gpurun_out/<tag>_model_inputs.json
with --measure, see below) and the netlists under tests/golden/.  Everything the table assumes is written into the output.

  flat configs (#2: 65 536 NANDs, 128-bit set; #5: the same on the 80-bit set), bench.py --gpus N, "strong" line:
      a rank gets G / N gates:  t(N) = rot(G / N) + ks(G / N) + host_ms      value(N) = G / t(N)
      rot, ks = interpolated between the launches measured on one GPU at 4 096 and 65 536 gates (the calibrated table's
      round_ms x rounds is listed beside it: one round alone is 3-9 % slower than a round inside a long launch);
      no data-path collective.
      "weak" leg (G gates on every rank): value = N * G / t(1).
  netlists (#3: mux-ram-8-16-16, #4: the CAHP system), tools/bench_netlist.py --gpus N, seconds per clock:
      plan = FrontierPlan(netlist, N, cost) — the plan the executor would run;  per level
      t = rot(rotations of the busiest rank) + ks_small(gates of that rank) + level_fixed_ms + (N > 1) * exchange(level bytes)
      exchange = exch_lat_us + bytes / exch_GBps: ONE in-place all_gather of the level's output ciphertexts over RCCL / xGMI.
      exch_* are ASSUMPTIONS (no multi-GPU box has run this yet): 40 us, 45 GB/s (a third of one xGMI link's ~153 GB/s).

  python tools/scale_model.py --inputs profiles/r06_final_model_inputs.json --out profiles/r06_scale_model.json     (the defaults)
  python tools/scale_model.py --measure gpurun_out/r06_model_inputs.json      (on a GPU box: calibrates both parameter sets)
"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, os.path.join(ROOT, "tools"))

G_FLAT = 65536
WORLDS = (1, 2, 4, 8)


def measure(path):
    """On a GPU box: the calibrated cost table, the key switch's per-gate cost on wide and on narrow batches, and the fixed cost
    of a level (events, staging copy, launch gaps) for both parameter sets."""
    import numpy as np
    import torch

    from iyokan_amd import client, hip
    from iyokan_amd.params import OPS, params_80bit, params_128bit

    out = {}
    for name, mk in (("128bit", params_128bit), ("80bit", params_80bit)):
        p = mk()
        keys = client.keygen(p, seed=1)
        hip.initialize(keys, device_ids=(0,))
        table = hip.calibrate(0)
        dev = torch.device("cuda", 0)
        rec = {"cost_table": table, "ks_ms": {}, "step_ms": {}, "rot_ms": {}}
        import time

        for g in (16, 64, 256, 1024, 4096, 65536):
            t = torch.zeros((3 * g, p.n + 1), dtype=torch.int32, device=dev)
            bits = np.random.default_rng(7).integers(0, 2, size=2 * g).astype(np.uint8)
            t[: 2 * g] = torch.from_numpy(client.encrypt_bits(keys, bits, seed=3).view(np.int32)).to(dev)
            arena = hip.Arena.from_torch(t, 0)
            st = hip.Stream(0)
            idx = np.arange(g, dtype=np.int32)
            args = (np.full(g, OPS["NAND"], dtype=np.int32), idx, idx + g, np.full(g, -1, dtype=np.int32), idx + 2 * g)
            best = None
            for rep in range(5):
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                st.gate_batch(arena, *args)
                st.sync()
                dt = (time.perf_counter() - t0) * 1e3
                br, ks = st.last_batch_timing()
                if rep and (best is None or dt < best[0]):
                    best = (dt, br, ks)
            rec["step_ms"][str(g)], rec["rot_ms"][str(g)], rec["ks_ms"][str(g)] = best
            st.destroy()
        hip.cleanup()
        out[name] = rec
    out["device"] = torch.cuda.get_device_name(0)
    out["build_id"] = hip.build_id()
    os.makedirs(os.path.dirname(os.path.abspath(path)), exist_ok=True)
    with open(path, "w") as f:
        json.dump(out, f, indent=1)
    print(json.dumps({k: v if not isinstance(v, dict) else "..." for k, v in out.items()}))


def interp(points, x):
    """Piecewise-linear through measured (size -> ms) points; linear in the size beyond the last one."""
    xs = sorted(int(k) for k in points)
    ys = [points[str(k)] for k in xs]
    if x <= xs[0]:
        return ys[0]
    for (x0, y0), (x1, y1) in zip(zip(xs, ys), zip(xs[1:], ys[1:])):
        if x <= x1:
            return y0 + (y1 - y0) * (x - x0) / (x1 - x0)
    return ys[-1] * x / xs[-1]


def model(inputs, exch_lat_us, exch_gbps):
    from iyokan_amd import netlist as N
    from iyokan_amd.frontier import BINARY, FrontierPlan, level_rotations, make_level_cost, with_sub_pass_shape
    from iyokan_amd.params import params_128bit
    from netlist_util import gold

    import bench_netlist

    res = {"assumptions": {
        "exchange_latency_us": exch_lat_us, "exchange_GBps": exch_gbps,
        "exchange": "one in-place all_gather of a level's output ciphertexts per level at N > 1 (RCCL over xGMI); ASSUMED figures, "
                    "no multi-GPU run exists yet",
        "flat": "t(N) = rot(G/N) + ks(G/N) + host, all three from the 1-GPU measurements in `inputs` (linear interpolation between measured batch sizes)",
        "netlist": "per level: rot(busiest rank) + ks(its gates) + level_fixed + exchange; plan = FrontierPlan(netlist, N, calibrated cost)",
    }, "inputs": inputs, "configs": {}}

    for cfg, name in (("2_flat_nand_128bit", "128bit"), ("5_flat_nand_80bit", "80bit")):
        rec = inputs[name]
        cost = make_level_cost(rec["cost_table"])
        host1 = rec["step_ms"][str(G_FLAT)] - rec["rot_ms"][str(G_FLAT)] - rec["ks_ms"][str(G_FLAT)]
        rows = {}
        for w in WORLDS:
            g = G_FLAT // w
            # the rotation time of a multi-round launch is interpolated between MEASURED launches (a launch of many rounds runs its
            # rounds ~3-9 % faster than round_ms, which is one round alone with its ramp and tail); the table's figure is listed beside it
            t = interp(rec["rot_ms"], g) + interp(rec["ks_ms"], g) + max(host1, 0.0)
            t1 = rec["rot_ms"][str(G_FLAT)] + rec["ks_ms"][str(G_FLAT)] + max(host1, 0.0)
            rows[str(w)] = {"strong_gates_per_s": G_FLAT / t * 1e3, "strong_ms_per_step": t,
                            "weak_gates_per_s": w * G_FLAT / t1 * 1e3, "rot_ms": interp(rec["rot_ms"], g), "rot_ms_by_cost_table": cost(g),
                            "ks_ms": interp(rec["ks_ms"], g)}
        res["configs"][cfg] = {"metric": "gates/s, 65 536 NAND gates per step", "measured_1gpu_ms_per_step": rec["step_ms"][str(G_FLAT)],
                               "by_gpus": rows}

    rec = inputs["128bit"]
    cost = make_level_cost(rec["cost_table"])
    price = with_sub_pass_shape(cost)   # a narrow level by how full its one pass is (round 6: what plan_levels compares plans by)
    p = params_128bit()
    ct_bytes = (p.n + 1) * 4
    # fixed cost of a level = what a narrow step costs beyond its two kernels (staging copy, events, launch gaps)
    fixed = min(rec["step_ms"][k] - rec["rot_ms"][k] - rec["ks_ms"][k] for k in ("16", "64", "256"))
    for cfg, net in (("3_mux_ram_8_16_16", "mux-ram"), ("4_cahp_system", "cahp-system")):
        fname, kind, _pkt = bench_netlist.NETS[net]
        if kind == "blueprint":
            from iyokan_amd.system import load_blueprint

            nl = load_blueprint(gold(fname)).nl
        else:
            nl = (N.load_iyokanl1_json if kind == "l1" else N.load_yosys_json)(gold(fname))
        rows = {}
        for w in WORLDS:
            plan = FrontierPlan(nl, w, balance=True, cost=cost)
            levels = [L["boot"] for L in plan.levels]
            rots = level_rotations(nl, levels, w)
            t_rot = t_ks = t_fix = t_ex = 0.0
            for lv, r in zip(levels, rots):
                gates = sum(1 for i in lv if nl.kinds[i] == "MUX" or nl.kinds[i] in BINARY)
                mine = -(-gates // w)
                if r:
                    t_rot += price(r)
                    t_ks += interp(rec["ks_ms"], mine)
                    t_fix += max(fixed, 0.0)
                if w > 1 and gates:
                    t_ex += exch_lat_us / 1e3 + gates * ct_bytes / (exch_gbps * 1e9) * 1e3
            total = t_rot + t_ks + t_fix + t_ex
            rows[str(w)] = {"s_per_clock": total / 1e3, "rot_ms": t_rot, "ks_ms": t_ks, "level_fixed_ms": t_fix, "exchange_ms": t_ex,
                            "levels": len(levels), "rotations_per_clock": nl.rotations()}
        res["configs"][cfg] = {"metric": "seconds per clock (tools/bench_netlist.py)", "level_fixed_ms_each": fixed, "by_gpus": rows}
    return res


TWO_LANE_CUS = (4, 8, 16)


def two_lane(inputs, lane_cus=TWO_LANE_CUS):
    """One-GPU bounds of configs #3 and #4 with one lane (the plan the executor runs, priced as model() prices it) and with two
    lanes (frontier.two_lane_bound: lane A on `a` CUs per XCD, lane B on the rest) at the clock penalties of a loaded chip and of
    the worst case, each batch charged the key switch (at the lane's share of the chip: a batch of g gates on c of 256 CUs as
    g * 256 / c gates) and the fixed cost of a level, as model() charges a level.  "two_lane" keeps both lanes for the whole
    clock; "whole_head" lets the levels before the deferral horizon run on the whole device (a third stream, beyond the two-lane
    design: an optimistic bound).  Yields one dict per line of the report."""
    from iyokan_amd import frontier as F
    from iyokan_amd import netlist as N
    from netlist_util import gold

    import bench_netlist

    rec = inputs["128bit"]
    table = rec["cost_table"]
    cost = F.make_level_cost(table)
    price = F.with_sub_pass_shape(cost)
    dev = int(table["pass"])
    fixed = max(min(rec["step_ms"][k] - rec["rot_ms"][k] - rec["ks_ms"][k] for k in ("16", "64", "256")), 0.0)

    def extra(gates, cus):
        return interp(rec["ks_ms"], gates * dev / cus) + fixed

    penalties = (("loaded", F.PENALTY_LOADED), ("worst", F.PENALTY_WORST))
    for cfg, net in (("3_mux_ram_8_16_16", "mux-ram"), ("4_cahp_system", "cahp-system")):
        fname, kind, _pkt = bench_netlist.NETS[net]
        if kind == "blueprint":
            from iyokan_amd.system import load_blueprint

            nl = load_blueprint(gold(fname)).nl
        else:
            nl = (N.load_iyokanl1_json if kind == "l1" else N.load_yosys_json)(gold(fname))
        levels = F.plan_levels(nl, 1, cost)
        rot = F._rot(nl)
        one = sum(price(r) + extra(sum(1 for i in lv if rot[i]), dev) for lv, r in zip(levels, F.level_rotations(nl, levels)) if r)
        yield {"config": cfg, "lanes": 1, "ms_per_clock": round(one, 3)}
        for whole_head in (False, True):
            for a in lane_cus:
                best = F.two_lane_bound(nl, table, a, [p for _, p in penalties], levels, whole_head, extra_ms=extra)
                for (pname, pen), b in zip(penalties, best):
                    yield {"config": cfg, "lanes": 2, "mode": "whole_head" if whole_head else "two_lane", "lane_cus_per_xcd": a,
                           "penalty": pname, "penalty_factor": round(pen, 4), "ms_per_clock": round(b["ms"], 3),
                           "vs_one_lane": round(b["ms"] / one - 1.0, 4), "horizon": b["horizon"], "slack": b["slack"],
                           "lane_b_sets": len(b["sets"]), "lane_b_rotations": sum(rot[i] for s in b["sets"] for i in s["nodes"])}


def check(table_path, model_path, tolerance=0.10):
    """A measured scaling table (tools/scale_all.sh's JSON lines, or the driver's SCALE_rNN.json) against the model's prediction.
    Returns a list of (label, measured, predicted, verdict) and prints it; the two numeric targets the round-5 review named are
    judged explicitly: flat batches >= 0.97 efficiency at N = 8, config #4 <= 0.115 s per clock at N = 8."""
    with open(model_path) as f:
        model_ = json.load(f)["configs"]
    lines = []
    with open(table_path) as f:
        text = f.read().strip()
    try:
        doc = json.loads(text)
        lines = doc if isinstance(doc, list) else doc.get("runs") or doc.get("results") or [doc]
    except ValueError:
        lines = [json.loads(line) for line in text.splitlines() if line.strip().startswith("{")]
    rows = []
    flat = {}
    for d in lines:
        if not isinstance(d, dict):
            continue
        d = d.get("parsed", d)
        if "n_gpus" in d and "value" in d:
            cfg = "5_flat_nand_80bit" if "80" in json.dumps(d.get("config", {})) else "2_flat_nand_128bit"
            n = str(d["n_gpus"])
            want = model_[cfg]["by_gpus"].get(n, {}).get("strong_gates_per_s")
            flat.setdefault(cfg, {})[int(n)] = d["value"]
            ok = want is not None and abs(d["value"] / want - 1.0) <= tolerance
            rows.append((f"{cfg} x{n} gates/s", d["value"], want, "ok" if ok else "OFF MODEL"))
        elif "s_per_clock" in d and "net" in d:
            cfg = {"mux-ram": "3_mux_ram_8_16_16", "cahp-system": "4_cahp_system"}.get(d["net"])
            n = str(d.get("gpus", d.get("n_gpus", 1)))
            if cfg:
                want = model_[cfg]["by_gpus"].get(n, {}).get("s_per_clock")
                ok = want is not None and abs(d["s_per_clock"] / want - 1.0) <= tolerance
                rows.append((f"{cfg} x{n} s/clock", d["s_per_clock"], want, "ok" if ok else "OFF MODEL"))
                if cfg == "4_cahp_system" and n == "8":
                    rows.append(("target: config #4 <= 0.115 s per clock at N = 8", d["s_per_clock"], 0.115,
                                 "met" if d["s_per_clock"] <= 0.115 else "MISSED"))
    for cfg, by_n in flat.items():
        if 1 in by_n and 8 in by_n:
            eff = by_n[8] / (8 * by_n[1])
            rows.append((f"target: {cfg} efficiency >= 0.97 at N = 8", eff, 0.97, "met" if eff >= 0.97 else "MISSED"))
    for label, got, want, verdict in rows:
        print(f"{label:58s} measured {got:12.4f}   model/target {want if want is None else round(want, 4)!s:>12}   {verdict}")
    return rows


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--check", default=None, help="a measured table (scale_all.sh's .jsonl or SCALE_rNN.json) to compare with --out's model")
    ap.add_argument("--measure", default=None, help="GPU box: write the model's inputs to this file")
    ap.add_argument("--inputs", default=os.path.join(ROOT, "profiles", "r06_final_model_inputs.json"))
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r06_scale_model.json"))
    ap.add_argument("--exch-lat-us", type=float, default=40.0)
    ap.add_argument("--exch-gbps", type=float, default=45.0)
    ap.add_argument("--two-lane", action="store_true",
                    help="print one- and two-lane bounds of configs #3 and #4 at one GPU (JSON lines; profiles/r07_two_lane_model.txt)")
    args = ap.parse_args()
    if args.two_lane:
        with open(args.inputs) as f:
            inputs = json.load(f)
        for line in two_lane(inputs):
            print(json.dumps(line), flush=True)
        return
    if args.check:
        rows = check(args.check, args.out)
        sys.exit(0 if rows and all(v in ("ok", "met") for *_, v in rows) else 1)
    if args.measure:
        measure(args.measure)
        return
    with open(args.inputs) as f:
        inputs = json.load(f)
    res = model(inputs, args.exch_lat_us, args.exch_gbps)
    with open(args.out, "w") as f:
        json.dump(res, f, indent=1)
    for cfg, rec in res["configs"].items():
        print(cfg, {w: round(r.get("strong_gates_per_s") or r["s_per_clock"], 4) for w, r in rec["by_gpus"].items()})


if __name__ == "__main__":
    main()
