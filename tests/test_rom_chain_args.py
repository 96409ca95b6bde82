"""CPU: the argument check and job lists of iyk_hip_cmux_rotate_chain_batch (csrc/batch_args.hpp: cmux_rotate_chain_args, a pure function
compiled on the host into libiyk_emul.so as iyk_emul_check_cmux_rotate_chain_batch, as tests/test_batch_args.py does for the older entry
points): one set per refusal, the sets that must be accepted, the job words written out by hand, and every refusal text of the function
held against a set that reaches it.  Stores of 4 selector slots and 16 rows, N = 1024."""
import ctypes
import os
import re

import numpy as np
import pytest

import batch_refusal_cases as brc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TRGSW, TRLWE, N2 = 4, 16, 2048
OK, INVALID = 0, -1
_i32p, _u32p, u64 = ctypes.POINTER(ctypes.c_int32), ctypes.POINTER(ctypes.c_uint32), ctypes.c_uint64

T_STEPS = "steps outside [1, 32]"
T_SEL = "selector index outside the selector store"
T_ROT = "rot outside [0, 2N)"
T_ROW = "TRLWE index outside the buffer"
T_TWO = "two jobs of one batch write the same TRLWE row"
T_READ = "a job reads a TRLWE row that another job of the batch writes"
T_CAP = "batch too large"
T_STORE = "store larger than an allocation can be"


def check(steps, sel, rot, src, out, count=None, trgsw_slots=TRGSW, trlwe_slots=TRLWE):
    """(code, text, job words [count][4], step words [sum steps][2])"""
    L = brc.emul()
    keep = [np.ascontiguousarray(np.asarray(v, dtype=np.int64).astype(np.int32)) for v in (steps, sel, rot, src, out)]
    msg = ctypes.create_string_buffer(256)
    words = np.zeros(1024, dtype=np.uint32)
    counts = (u64 * 4)()
    f = L.iyk_emul_check_cmux_rotate_chain_batch
    f.restype = ctypes.c_int
    code = f(u64(trgsw_slots), u64(trlwe_slots), u64(len(keep[0]) if count is None else count), *[a.ctypes.data_as(_i32p) for a in keep], msg,
             u64(256), words.ctypes.data_as(_u32p), u64(words.size), counts)
    nj, ns = int(counts[0]), int(counts[1])
    w = words.view(np.int32)
    return code, msg.value.decode(), w[: 4 * nj].reshape(nj, 4).tolist(), w[4 * nj : 4 * nj + 2 * ns].reshape(ns, 2).tolist()


REFUSED = {
    "steps 0": (dict(steps=[0], sel=[0], rot=[1], src=[0], out=[1]), T_STEPS),
    "steps 33": (dict(steps=[33], sel=[0] * 33, rot=[1] * 33, src=[0], out=[1]), T_STEPS),
    "steps -1 in the second job": (dict(steps=[1, -1], sel=[0], rot=[1], src=[0, 2], out=[1, 3]), T_STEPS),
    "sel -1": (dict(steps=[2], sel=[0, -1], rot=[1, 1], src=[0], out=[1]), T_SEL),
    "sel == trgsw_slots": (dict(steps=[1], sel=[TRGSW], rot=[1], src=[0], out=[1]), T_SEL),
    "rot -1": (dict(steps=[1], sel=[0], rot=[-1], src=[0], out=[1]), T_ROT),
    "rot == 2N": (dict(steps=[2], sel=[0, 1], rot=[N2 - 1, N2], src=[0], out=[1]), T_ROT),
    "src == trlwe_slots": (dict(steps=[1], sel=[0], rot=[1], src=[TRLWE], out=[1]), T_ROW),
    "out == trlwe_slots": (dict(steps=[1], sel=[0], rot=[1], src=[0], out=[TRLWE]), T_ROW),
    "src -1": (dict(steps=[1], sel=[0], rot=[1], src=[-1], out=[1]), T_ROW),
    "out[g] == src[h]": (dict(steps=[1, 1], sel=[0, 1], rot=[1, 2], src=[0, 5], out=[5, 6]), T_READ),
    "out[g] == out[h]": (dict(steps=[1, 2], sel=[0, 1, 2], rot=[1, 2, 3], src=[0, 1], out=[5, 5]), T_TWO),
    "over cap": (dict(steps=[1], sel=[0], rot=[1], src=[0], out=[1], count=(1 << 24) + 1), T_CAP),
    "selector store over cap": (dict(steps=[1], sel=[0], rot=[1], src=[0], out=[1], trgsw_slots=(1 << 24) + 1), T_STORE),
    "row store over cap": (dict(steps=[1], sel=[0], rot=[1], src=[0], out=[1], trlwe_slots=(1 << 28) + 1), T_STORE),
    # two faults at once: which one is reported
    "bad steps and bad row": (dict(steps=[0], sel=[0], rot=[1], src=[-1], out=[1]), T_STEPS),
    "bad sel and bad rot in one step": (dict(steps=[1], sel=[-1], rot=[-1], src=[0], out=[1]), T_SEL),
    "bad rot and bad row": (dict(steps=[1], sel=[0], rot=[N2], src=[0], out=[TRLWE]), T_ROT),
    "two writers and a read of a written row": (dict(steps=[1, 1, 1], sel=[0, 0, 0], rot=[1, 1, 1], src=[0, 5, 1], out=[5, 6, 6]), T_TWO),
}


@pytest.mark.parametrize("name", list(REFUSED))
def test_refusals(built, name):
    args, text = REFUSED[name]
    code, got, jobs, steps = check(**args)
    assert (code, got) == (INVALID, text)
    assert jobs == [] and steps == []   # a refused set hands nothing to stage


def test_job_words_of_a_legal_batch(built):
    """three jobs of 2, 1 and 3 steps: first = the sum of the steps before; sel = 0 and sel = trgsw_slots - 1, rot = 0 and rot = 2N - 1,
    row 0 and row trlwe_slots - 1 are all inside"""
    code, text, jobs, steps = check(steps=[2, 1, 3], sel=[3, 0, 1, 2, 2, 3], rot=[0, N2 - 1, 1024, 7, 0, 2047], src=[0, 0, TRLWE - 1], out=[1, 2, 3])
    assert (code, text) == (OK, "")
    assert jobs == [[0, 2, 0, 1], [2, 1, 0, 2], [3, 3, TRLWE - 1, 3]]                                     # {first, steps, src, out}
    assert steps == [[3, 0], [0, N2 - 1], [1, 1024], [2, 7], [2, 0], [3, 2047]]                            # {sel, rot}


def test_32_steps_are_accepted(built):
    code, _, jobs, steps = check(steps=[32], sel=[g % TRGSW for g in range(32)], rot=list(range(32)), src=[4], out=[9])
    assert code == OK and jobs == [[0, 32, 4, 9]] and len(steps) == 32 and steps[31] == [3, 31]


def test_in_place_and_shared_src_are_accepted(built):
    """out[g] == src[g]; two jobs with one src; both at once where the shared src is nobody's out"""
    code, _, jobs, _ = check(steps=[1], sel=[0], rot=[1], src=[5], out=[5])
    assert code == OK and jobs == [[0, 1, 5, 5]]
    code, _, jobs, _ = check(steps=[1, 1], sel=[0, 1], rot=[1, 2], src=[5, 5], out=[6, 7])
    assert code == OK and jobs == [[0, 1, 5, 6], [1, 1, 5, 7]]
    code, _, jobs, _ = check(steps=[1, 1, 1], sel=[0, 1, 2], rot=[1, 2, 3], src=[5, 5, 8], out=[6, 7, 8])
    assert code == OK and [j[2:] for j in jobs] == [[5, 6], [5, 7], [8, 8]]


def test_a_shared_src_may_not_be_written_by_one_of_its_readers(built):
    assert check(steps=[1, 1], sel=[0, 1], rot=[1, 2], src=[5, 5], out=[5, 7])[:2] == (INVALID, T_READ)


def test_every_refusal_text_has_a_set(built):
    """the string literals of cmux_rotate_chain_args in batch_args.hpp == the texts the sets above reach"""
    src = open(os.path.join(ROOT, "iyokan_amd", "csrc", "batch_args.hpp")).read()
    m = re.search(r"^inline Refusal cmux_rotate_chain_args\(.*?^}$", src, re.M | re.S)
    assert m
    assert set(re.findall(r'"([^"\n]+)"', m.group(0))) == {text for _, text in REFUSED.values()}


def test_grid(built):
    """dispatch::cmux_rotate_chain_grid: eight jobs per workgroup, the last one partial"""
    f = brc.emul().iyk_emul_cmux_rotate_chain_grid
    f.restype, f.argtypes = ctypes.c_int64, [ctypes.c_int64]
    assert [f(c) for c in (0, 1, 8, 9, 301, 1 << 24)] == [0, 1, 1, 2, 38, 1 << 21]
