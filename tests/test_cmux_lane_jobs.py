"""CPU: CMUX memories per lane — csrc/cmux_lane_jobs.hpp (the expansion of one lane's CMUX job list to those of all lanes: the functions
cmux_lane_jobs_kernel runs) and batch_args.hpp's *_lanes_args (the checks of the four iyk_hip_cmux_*_batch_lanes calls), through
libiyk_emul.so.

The reference is the flat batch: what the parent check builds from host-replicated arrays (cmux_lane_cases.replicate).  Everything is
compared job for job, word for word.  The mutants are scratch builds of csrc/cmux_lane_emul.hpp alone against a copy of the headers with
one edit (in cmux_lane_jobs.hpp; "negative-in1-offset" edits lane_jobs.hpp's lane_index, the one function every offset goes through:
MUTANTS names the file of each); each has named cases that must tell it from the real thing and must leave every one-lane case alone."""
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

import cmux_lane_cases as cc

ROOT = cc.ROOT


@pytest.mark.parametrize("name", list(cc.CASES))
def test_expansion_equals_the_list_of_replicated_arrays(name):
    c = cc.CASES[name]
    assert cc.first_difference(c) is None
    jobs, steps = cc.lane_lists(c)
    _, _, (jobs1, steps1), _ = cc.lanes_args(c["family"], c["arrays"], c["trgsw_slots"], c["trlwe_slots"], c["lanes"], c["sel_stride"], c["row_stride"])
    assert (len(jobs), len(steps)) == (len(jobs1) * c["lanes"], len(steps1) * c["lanes"])      # lane-major, every list `lanes` times as long


def test_the_case_set_covers_what_it_claims():
    fams = {f: {c["lanes"] for c in cc.CASES.values() if c["family"] == f} for f in cc.FAMILY_NAME}
    assert all(l >= {1, 2, 5, 7} for l in fams.values())
    in1 = cc.CASES["cmux3-x2"]["arrays"][2]
    assert (in1 < 0).any() and (in1 >= 0).any()                                              # a rotate-form job beside two-row jobs
    a = cc.CASES["cmux3-x2"]["arrays"]
    assert any(a[4][g] in (a[1][g], a[2][g]) for g in range(3))                              # a job over its own input
    assert cc.CASES["rot31-x2"]["arrays"][0].tolist() == [3, 1]                              # `first` moves by r x 4, not r x 2
    assert set(cc.CASES["tree41-x2"]["arrays"][1].tolist()) == {1, 4}
    w = cc.CASES["cmux3-wide-stride"]
    assert w["row_stride"] > 1 + cc.reach(w["family"], w["arrays"])[1]
    s = cc.CASES["cmux-stage-major"]
    assert int(s["arrays"][0].min()) == 5 and s["sel_stride"] == 3
    assert len(cc.CASES["37x7"]["arrays"][0]) * cc.CASES["37x7"]["lanes"] == 259 == 256 + 3
    assert len(cc.CASES["cmux3-x3"]["arrays"][0]) * 3 == 8 + 1


def test_the_words_of_a_lane_by_hand():
    """the rule itself, not only its agreement with the replicated arrays: lane 2 of the rotate chain (3, 1) and of the CMUX list"""
    jobs, steps = cc.lane_lists(cc.CASES["rot31-x5"])
    assert jobs[2 * 2].tolist() == [0 + 2 * 4, 3, 0 + 2 * 3, 2 + 2 * 3] and jobs[2 * 2 + 1].tolist() == [3 + 2 * 4, 1, 1 + 2 * 3, 1 + 2 * 3]
    assert steps[2 * 4: 3 * 4].tolist() == [[0 + 6, 2044], [1 + 6, 2040], [2 + 6, 2032], [1 + 6, 1024]]
    jobs, _ = cc.lane_lists(cc.CASES["cmux3-x5"])
    assert jobs[2 * 3 + 1].tolist() == [1 + 2 * 3, 2 + 2 * 7, -1, 100, 3 + 2 * 7]             # in1 = -1 and rot stay
    jobs, _ = cc.lane_lists(cc.CASES["cmux-stage-major"])
    assert jobs[3:, 0].tolist() == [8, 9, 10]                                                 # 5 + 3: lane 1 sits inside the stage


@pytest.mark.parametrize("threads", [1, 3, 64, 256, 1024])
@pytest.mark.parametrize("name", ["37x7", "rot-37x7"])
def test_grid_stride_traversal_writes_every_job_once(name, threads):
    """cmux_lane_jobs_kernel's loop with fewer threads than entries, as many, and more: the same lists, nothing left unwritten"""
    c = cc.CASES[name]
    want = cc.lane_lists(c)
    got = cc.lane_lists(c, threads=threads)
    assert all(np.array_equal(g, w) for g, w in zip(got, want))
    assert not any((g.view(np.uint32) == 0xDEADBEEF).any() for g in got)


@pytest.mark.parametrize("name,family,arrays,trgsw_slots,trlwe_slots,lanes,sel_stride,row_stride,word", cc.REFUSALS, ids=[r[0] for r in cc.REFUSALS])
def test_refusals(name, family, arrays, trgsw_slots, trlwe_slots, lanes, sel_stride, row_stride, word):
    code, text, lists, left = cc.lanes_args(family, arrays, trgsw_slots, trlwe_slots, lanes, sel_stride, row_stride)
    assert code == cc.INVALID and word in text, (code, text)
    assert not left and all(len(a) == 0 for a in lists)          # nothing to stage


@pytest.mark.parametrize("name,family,arrays,trgsw_slots,trlwe_slots,lanes,sel_stride,row_stride", cc.ACCEPTED, ids=[a[0] for a in cc.ACCEPTED])
def test_the_neighbours_of_the_refusals_are_accepted(name, family, arrays, trgsw_slots, trlwe_slots, lanes, sel_stride, row_stride):
    code, text, lists, left = cc.lanes_args(family, arrays, trgsw_slots, trlwe_slots, lanes, sel_stride, row_stride)
    assert code == cc.OK and text == "" and not left, text
    flat = cc.parent_lists(family, arrays, trgsw_slots, trlwe_slots)
    assert flat[0] == cc.OK and all(np.array_equal(a, b) for a, b in zip(lists, flat[2]))      # ONE lane's list: the parent's


def test_rotate_chain_step_list_keeps_its_32_bit_index():
    """sum(steps) x lanes that would pass 2^31 - 1 is refused: with at most 32 steps per job the cap on count x lanes refuses it first
    (2^24 x 32 = 2^29), so the expanded `first` of a job always fits its int32_t"""
    count = 1 << 11
    arrays = ([32] * count, [0] * (32 * count), [1] * (32 * count), [0] * count, list(range(1, count + 1)))
    lanes = ((1 << 31) - 1) // (32 * count) + 1          # the first lane count whose steps pass 2^31 - 1
    code, text, lists, left = cc.lanes_args(cc.ROT, arrays, 1 << 20, 1 << 28, lanes, 1, count + 1)
    assert code == cc.INVALID and "count x lanes" in text and not left
    assert cc.MAX_ROW_BATCH * 32 < (1 << 31) - 1


# ---- mutants ------------------------------------------------------------------------------------------------------------------------

MUTANTS = {
    # name: ((file, pattern, replacement, times it must apply), cases that must differ)
    "negative-in1-offset": (("lane_jobs.hpp", r"return i < 0 \? i : \(int32_t\)", r"return (int32_t)", 1),
                            ["cmux3-x2", "cmux3-x5", "cmux3-x3", "cmux3-wide-stride", "cmux-stage-major"]),
    "first-by-count": (("cmux_lane_jobs.hpp", r"lane_cmux_rot_chain_job\(L\.job1\[j\], r, L\.nsteps, L\.row_stride\)",
                        r"lane_cmux_rot_chain_job(L.job1[j], r, L.n, L.row_stride)", 1),
                       ["rot31-x2", "rot31-x5", "rot31-x7", "rot-stage-major"]),
    "out-without-offset": (("cmux_lane_jobs.hpp", r"lane_index\(j\.out, r, row_stride\)", r"j.out", 4),
                           ["cmux3-x2", "chain-ram21-x2", "rot31-x2", "tree41-x2", "37x7"]),
    "sel-by-row-stride": (("cmux_lane_jobs.hpp", r"lane_index\(j\.sel, r, sel_stride\)", r"lane_index(j.sel, r, row_stride)", 1),
                          ["cmux3-x2", "cmux3-x7", "cmux-stage-major", "37x7"]),
    "lane-minor": (("cmux_lane_jobs.hpp", r"r = \(uint32_t\)\((\w+) / L\.(\w+)\), j = \(uint32_t\)\(\1 % L\.\2\)",
                    r"r = (uint32_t)(\1 % L.lanes), j = (uint32_t)(\1 / L.lanes)", 2),
                   ["cmux3-x2", "chain-ram21-x5", "rot31-x2", "tree41-x7", "37x7", "rot-37x7"]),
}


def _build_mutant(tmp_path, edit):
    src = tmp_path / "iyokan_amd" / "csrc"
    src.mkdir(parents=True)
    for f in ("cmux_lane_jobs.hpp", "cmux_lane_emul.hpp", "lane_jobs.hpp", "batch_args.hpp", "jobs.hpp"):
        shutil.copy(os.path.join(ROOT, "iyokan_amd", "csrc", f), src / f)
    shutil.copytree(os.path.join(ROOT, "include"), tmp_path / "include")
    name, pattern, repl, times = edit
    text, n = re.subn(pattern, repl, (src / name).read_text())
    assert n == times, (pattern, n)
    (src / name).write_text(text)
    (src / "mutant.cpp").write_text('#include "cmux_lane_emul.hpp"\n')
    lib = tmp_path / "libmutant.so"
    subprocess.run(["g++", "-O0", "-std=c++17", "-fPIC", "-shared", "-o", str(lib), str(src / "mutant.cpp")], check=True)
    return cc.emul(str(lib))


def test_the_scratch_build_itself_is_the_real_thing(tmp_path):
    lib = _build_mutant(tmp_path, ("cmux_lane_jobs.hpp", r"#pragma once", "#pragma once", 1))       # no edit
    assert all(cc.first_difference(c, lib=lib) is None for c in cc.CASES.values())


@pytest.mark.parametrize("name", list(MUTANTS))
def test_each_mutant_fails_its_named_cases(tmp_path, name):
    edit, must_fail = MUTANTS[name]
    lib = _build_mutant(tmp_path, edit)
    failing = [n for n, c in cc.CASES.items() if cc.first_difference(c, lib=lib) is not None]
    assert set(must_fail) <= set(failing), (name, failing)
    assert not set(cc.ONE_LANE) & set(failing), (name, failing)          # no one-lane case changes: lanes == 1 expands nothing
