"""CPU: lane batches — csrc/lane_jobs.hpp (the expansion of one lane's job lists to those of all lanes: the functions lane_jobs_kernel
runs) and batch_args.hpp's gate_batch_lanes_args (the checks of iyk_hip_gate_batch_lanes), through libiyk_emul.so.

The reference is the flat batch: what check_gate_batch builds from host-replicated descriptors (lane_cases.replicate).  Everything is
compared job for job, word for word.  The mutants are scratch builds of csrc/lane_emul.hpp alone against a copy of the headers with one
edit in lane_jobs.hpp; each has named cases that must tell it from the real thing."""
import ctypes
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

import lane_cases as lc

ROOT = lc.ROOT


@pytest.mark.parametrize("name", list(lc.CASES))
def test_expansion_equals_the_lists_of_replicated_descriptors(name):
    c = lc.CASES[name]
    assert lc.first_difference(c) is None
    # and in words, for the record: list sizes and the layout rule, lane-major
    rot, ks, ew = lc.lane_lists(c)
    _, _, (rot1, ks1, ew1), _ = lc.lane_args(tuple(c[k] for k in ("ops", "in0", "in1", "in2", "out")), c["lanes"] * c["stride"], c["lanes"], c["stride"])
    assert (len(rot), len(ks), len(ew)) == (len(rot1) * c["lanes"], len(ks1) * c["lanes"], len(ew1) * c["lanes"])
    for r in range(c["lanes"]):
        for j, job in enumerate(ks1.view(np.int32)):
            ra, rb, off, out = (int(x) for x in ks.view(np.int32)[r * len(ks1) + j])
            assert (ra, out) == (job[0] + r * len(rot1), job[3] + r * c["stride"]) and off == job[2]
            assert rb == (job[1] + r * len(rot1) if job[1] >= 0 else -1)


def test_the_case_set_covers_what_it_claims():
    ops = set()
    for c in lc.CASES.values():
        ops |= {int(o) for o in c["ops"]}
    assert ops == set(lc.OPS.values())
    assert {c["lanes"] for c in lc.CASES.values()} >= {1, 2, 5}
    assert any(c["stride"] > c["used"] for c in lc.CASES.values())
    c = lc.CASES["37x7"]
    assert c["count"] * c["lanes"] == 259 == 256 + 3
    e = lc.CASES["every-op-2"]
    assert any(e["out"][g] in (e["in0"][g], e["in1"][g]) for g in range(e["count"]))          # a gate over its own input
    _, _, (rot1, ks1, ew1), _ = lc.lane_args(tuple(e[k] for k in ("ops", "in0", "in1", "in2", "out")), 2 * e["stride"], 2, e["stride"])
    assert (ks1.view(np.int32)[:, 1] >= 0).any() and (ks1.view(np.int32)[:, 1] < 0).any()      # MUX: rb >= 0; binary gates: rb = -1
    assert (ew1.view(np.int32)[:, 1] < 0).any() and len(rot1) > len(ks1)


@pytest.mark.parametrize("threads", [1, 3, 64, 256, 1024])
def test_grid_stride_traversal_writes_every_job_once(threads):
    """lane_jobs_kernel's loop with fewer threads than jobs, as many, and more: the same lists"""
    c = lc.CASES["37x7"]
    want = lc.lane_lists(c)
    got = lc.lane_lists(c, threads=threads)
    assert all(np.array_equal(g, w) for g, w in zip(got, want))


@pytest.mark.parametrize("name,desc,arena_slots,lanes,stride,word", lc.REFUSALS, ids=[r[0] for r in lc.REFUSALS])
def test_refusals(name, desc, arena_slots, lanes, stride, word):
    code, text, lists, left = lc.lane_args(desc, arena_slots, lanes, stride)
    assert code == lc.INVALID and word in text, (code, text)
    assert not left and all(len(a) == 0 for a in lists)          # nothing to stage


@pytest.mark.parametrize("name,desc,arena_slots,lanes,stride", lc.ACCEPTED, ids=[a[0] for a in lc.ACCEPTED])
def test_the_neighbours_of_the_refusals_are_accepted(name, desc, arena_slots, lanes, stride):
    code, text, lists, left = lc.lane_args(desc, arena_slots, lanes, stride)
    assert code == lc.OK and text == "" and not left
    flat = lc.flat_lists(desc, stride)
    assert flat[0] == lc.OK and all(np.array_equal(a, b) for a, b in zip(lists, flat[2]))      # ONE lane's lists, checked against the stride


def test_debug_check_is_one_lane_s():
    """IYK_HIP_DEBUG: the independence contract is verified on one lane — O(count) — and a violation inside a lane is a refusal"""
    g = lc.CASES["mux-3"]
    desc = tuple(g[k] for k in ("ops", "in0", "in1", "in2", "out"))
    assert lc.lane_args(desc, 64, 5, 11, debug=1)[0] == lc.OK
    clash = lc._with(desc, in0=(1, 8))                     # gate 1 reads what gate 0 writes
    code, text, lists, left = lc.lane_args(clash, 64, 5, 11, debug=1)
    assert code == lc.INVALID and text.startswith("debug: a gate reads a slot another gate") and not left and not len(lists[0])
    assert lc.lane_args(clash, 64, 5, 11, debug=0)[0] == lc.OK
    # a huge lane count costs the check nothing: the lists are one lane's
    code, text, lists, _ = lc.lane_args(desc, 1 << 31, (1 << 31) // 11, 11, debug=1)
    assert code == lc.OK and [len(a) for a in lists] == [3, 2, 1]


def _dispatch(nrot, nks, lanes, kind_env=-1, T=7, nc=5, cus=256, round_=2048, max_passes=5):
    L = lc.emul()
    out = (ctypes.c_int * 10)()
    L.iyk_emul_lane_dispatch(lc.u64(nrot), lc.u64(nks), lc.u64(lanes), round_, cus, max_passes, 0, 2, 4096, 512, kind_env, T, nc, cus, out)
    return list(out)


def _flat_dispatch(nrot, nks, kind_env=-1, T=7, nc=5, cus=256, round_=2048, max_passes=5):
    L = lc.emul()
    split = (ctypes.c_int * 5)()
    L.iyk_emul_rot_split(nrot, round_, cus, max_passes, 0, split)
    n = (ctypes.c_int * 1)(nks)
    form, groups, slices, per = ((ctypes.c_int * 1)() for _ in range(4))
    L.iyk_emul_ks_plan(2, 4096, 512, n, 1, T, nc, cus, form, groups, slices, per)
    L.iyk_emul_ks_matrix_form.restype = ctypes.c_int
    return list(split) + [form[0], groups[0], slices[0], per[0], L.iyk_emul_ks_matrix_form(kind_env, nks, T, nc)]


@pytest.mark.parametrize("count,lanes", [(1, 1), (1, 2), (37, 7), (641, 2), (1025, 2), (1025, 4), (1152, 4), (1153, 4), (4607, 1), (16, 256)])
def test_dispatch_takes_the_total(count, lanes):
    """kernel and grid of a lane batch of count x lanes == those of a flat batch of that many gates; below and at each threshold the
    per-lane count alone would have chosen otherwise"""
    assert _dispatch(count, count, lanes) == _flat_dispatch(count * lanes, count * lanes)
    assert _dispatch(2 * count, count, lanes) == _flat_dispatch(2 * count * lanes, count * lanes)     # all MUX


def test_the_threshold_cases_straddle():
    """what tests/test_gpu_lanes.py relies on: per lane below, in total at or above each threshold dispatch.hpp names"""
    one, two = _flat_dispatch(641, 641), _flat_dispatch(1282, 1282)
    assert one[2] == 0 and one[4] == 641 and two[2] == 1282 and two[4] == 0             # narrow-frontier kernel -> one partial round
    one, two = _flat_dispatch(1025, 1025), _flat_dispatch(2050, 2050)
    assert one[2] == 0 and two[2] == 2048 and two[4] == 2                                # -> a full round and a narrow remainder
    one, four = _flat_dispatch(1025, 1025), _flat_dispatch(4100, 4100)
    assert one[5] == 1 and four[5] == 3 and not four[9]                                  # shared form -> table
    one, four = _flat_dispatch(1152, 1152), _flat_dispatch(4608, 4608)
    assert one[5] == 1 and not one[9] and four[9] == 1                                   # -> matrix form, from 4 608 gates


# ---- mutants ------------------------------------------------------------------------------------------------------------------------

_LANE_MINOR = (r"r = \(uint32_t\)\((\w+) / L\.(\w+)\), j = \(uint32_t\)\(\1 % L\.\2\)", r"r = (uint32_t)(\1 % L.lanes), j = (uint32_t)(\1 / L.lanes)", 3)
MUTANTS = {
    # name: ((pattern, replacement, times it must apply), cases that must differ, cases that must not)
    "negative-rb-offset": ((r"return i < 0 \? i : \(int32_t\)", r"return (int32_t)", 1),
                           ["one-gate-two-lanes", "mux-3", "every-op-2", "constants-only", "37x7"], ["one-gate-one-lane", "every-op-1"]),
    "ra-by-count": ((r"lane_ks_job\(L\.ks1\[j\], r, L\.lane_stride, L\.nrot\)", r"lane_ks_job(L.ks1[j], r, L.lane_stride, L.nks)", 1),
                    ["mux-3", "mux-first-and-last", "every-op-2", "every-op-5-wide-stride", "37x7"], ["one-gate-two-lanes", "every-op-1", "constants-only"]),
    "ks-out-without-offset": ((r"lane_index\(j\.rb, r, nrot\), j\.off, lane_index\(j\.out, r, lane_stride\)\}", r"lane_index(j.rb, r, nrot), j.off, j.out}", 1),
                              ["one-gate-two-lanes", "mux-3", "every-op-2", "37x7"], ["one-gate-one-lane", "every-op-1", "constants-only"]),
    "lane-minor": (_LANE_MINOR, ["mux-3", "mux-first-and-last", "every-op-2", "constants-only", "37x7"], ["one-gate-one-lane", "one-gate-two-lanes", "every-op-1"]),
}


def _build_mutant(tmp_path, edit):
    src = tmp_path / "iyokan_amd" / "csrc"
    src.mkdir(parents=True)
    for f in ("lane_jobs.hpp", "lane_emul.hpp", "batch_args.hpp", "dispatch.hpp", "jobs.hpp"):
        shutil.copy(os.path.join(ROOT, "iyokan_amd", "csrc", f), src / f)
    shutil.copytree(os.path.join(ROOT, "include"), tmp_path / "include")
    pattern, repl, times = edit
    text, n = re.subn(pattern, repl, (src / "lane_jobs.hpp").read_text())
    assert n == times, (pattern, n)
    (src / "lane_jobs.hpp").write_text(text)
    (src / "mutant.cpp").write_text('#include "lane_emul.hpp"\n')
    lib = tmp_path / "libmutant.so"
    subprocess.run(["g++", "-O0", "-std=c++17", "-fPIC", "-shared", "-o", str(lib), str(src / "mutant.cpp")], check=True)
    return lc.emul(str(lib))


def test_the_scratch_build_itself_is_the_real_thing(tmp_path):
    lib = _build_mutant(tmp_path, (r"#pragma once", "#pragma once", 1))       # no edit
    assert all(lc.first_difference(c, lib=lib) is None for c in lc.CASES.values())


@pytest.mark.parametrize("name", list(MUTANTS))
def test_each_mutant_fails_its_named_cases(tmp_path, name):
    edit, must_fail, must_pass = MUTANTS[name]
    lib = _build_mutant(tmp_path, edit)
    failing = [n for n, c in lc.CASES.items() if lc.first_difference(c, lib=lib) is not None]
    assert set(must_fail) <= set(failing), (name, failing)
    assert not set(must_pass) & set(failing), (name, failing)
