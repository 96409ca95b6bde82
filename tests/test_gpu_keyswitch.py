"""GPU: SampleExtractAndKeySwitch on chosen words (tests/ks_words.py) through every key-switch kernel and launch shape — the table
kernel (keyswitch_lut_kernel, 8 / 4 / 2 / 1 slices, whole and ragged last workgroups), both forms of keyswitch_wave_kernel and
keyswitch_kernel — at both parameter sets, every word of every output against the oracle's sample extract + IdentityKeySwitch;
then a second key after cleanup, for the table and for the field key."""
import concurrent.futures
import ctypes
import os

import numpy as np
import pytest

import ks_words as K
import oracle_lib
from iyokan_amd import client
from iyokan_amd.params import OPS, params_128bit

pytestmark = pytest.mark.gpu

CELLS = 32769               # TRLWE cells of the per-set buffer: the chosen ones first, then uniform ones
FILL = np.uint32(0xA5A5A5A5)
KS_ENV = ("IYK_HIP_KS_KERNEL", "IYK_HIP_KS_SHARED_MAX", "IYK_HIP_KS_SHARED_WG", "IYK_HIP_ROT_KERNEL", "IYK_HIP_LATENCY_KERNEL",
          "IYK_HIP_NTT")
_u32p = ctypes.POINTER(ctypes.c_uint32)


def _cells(p, ncells, seed):
    """[ncells][2 N] TRLWE images: the chosen cells of ks_words.chosen_images, then uniform words; and how many are chosen."""
    imgs, _ = K.chosen_images(p, seed)
    rng = np.random.default_rng(seed + 100)
    out = np.empty((ncells, 2 * p.N), dtype=np.uint32)
    out[:len(imgs)] = imgs
    out[len(imgs):] = rng.integers(0, 1 << 32, size=(ncells - len(imgs), 2 * p.N), dtype=np.uint32)
    return out, len(imgs)


def _reference(orc, cells):
    """orc_sample_extract0 + orc_keyswitch of every cell, on up to 16 threads (ctypes calls release the GIL)."""
    p = orc.p
    ref = np.empty((len(cells), p.n + 1), dtype=np.uint32)
    L = oracle_lib.lib()

    def work(lo, hi):
        t1 = np.zeros(p.N + 1, dtype=np.uint32)
        for c in range(lo, hi):
            L.orc_sample_extract0(orc.ctx, cells[c].ctypes.data_as(_u32p), t1.ctypes.data_as(_u32p))
            L.orc_keyswitch(orc.ctx, t1.ctypes.data_as(_u32p), ref[c].ctypes.data_as(_u32p))

    nw = min(16, os.cpu_count() or 1)
    bounds = np.linspace(0, len(cells), 4 * nw + 1).astype(int)
    with concurrent.futures.ThreadPoolExecutor(nw) as ex:
        list(ex.map(lambda k: work(bounds[k], bounds[k + 1]), range(4 * nw)))
    return ref


def _set_ks_env(monkeypatch, kind, shared_max):
    monkeypatch.setenv("IYK_HIP_KS_KERNEL", kind)
    if shared_max is None:
        monkeypatch.delenv("IYK_HIP_KS_SHARED_MAX", raising=False)
    else:
        monkeypatch.setenv("IYK_HIP_KS_SHARED_MAX", shared_max)


def _run_case(hip, st, d_trlwe, ncells, idx, p, rng):
    """Key switch of cells idx[j] into a permutation of slots of an arena larger than the case, pre-filled with 0xA5A5A5A5:
    (whole arena after the batch, slot of job j)."""
    n = len(idx)
    slots = n + 37
    out_slot = rng.permutation(slots)[:n].astype(np.int32)
    arena = hip.Arena(slots)
    try:
        st.upload(arena, 0, np.full((slots, p.n + 1), FILL, dtype=np.uint32))
        st.sample_extract_keyswitch_batch(d_trlwe, idx, out_slot, arena, trlwe_slots=ncells)
        st.sync()
        got = st.download(arena, 0, slots)
    finally:
        arena.free()
    return got, out_slot


def _check_case(got, out_slot, idx, ref, nchosen, what):
    want = np.full_like(got, FILL)
    want[out_slot] = ref[idx]
    bad = np.nonzero((got != want).any(axis=1))[0]
    if len(bad):
        job_of = {int(s): j for j, s in enumerate(out_slot)}
        lines = []
        for s in bad[:8]:
            j = job_of.get(int(s))
            words = np.nonzero(got[s] != want[s])[0]
            where = "unwritten slot" if j is None else f"job {j}, cell {idx[j]}{' (chosen)' if idx[j] < nchosen else ''}"
            lines.append(f"slot {s}: {where}: {len(words)} words differ, first {words[:6].tolist()}")
        pytest.fail(f"{what}: {len(bad)} of {len(got)} slots differ\n" + "\n".join(lines))


@pytest.mark.parametrize("which", ["128", "80"])
def test_key_switch_chosen_words_every_form_and_shape(which, request, monkeypatch):
    """Every case of ks_words.cases(cus): kind 0, kind 1 (shared form up to 4 096 jobs, wide above), kind 1 with
    IYK_HIP_KS_SHARED_MAX=0 (the wide form at every size), kind 2 (the table above 4 096 jobs).  Cases of 89 jobs or more hold all
    chosen cells at the first job, at the last job and across a 16-gate wave boundary (64 .. 88 jobs: the cover and edge cells);
    a 1-job case runs eight chosen cells one at a time.  Every word of every output equals the oracle's, every slot the case did
    not write keeps its fill, and the resident key bytes grow by the table exactly at the first table launch."""
    from iyokan_amd import hip

    keys = request.getfixturevalue("keys" + which)
    orc = request.getfixturevalue("oracle" + which)
    p = keys.params
    for v in KS_ENV:
        monkeypatch.delenv(v, raising=False)
    cells, nchosen = _cells(p, CELLS, seed=int(which))
    ref = _reference(orc, cells)
    special = list(range(nchosen))
    singles = [0, 15, 16, 17, 18, 19, nchosen - 4, nchosen - 1]    # two cover, the four edges, raw all-ones and raw uniform
    rng = np.random.default_rng(4000 + int(which))
    hip.initialize(keys, device_ids=(0,))
    try:
        cus = hip.level_cost_table(0)["pass"]
        st = hip.Stream(0)
        L = hip.lib()
        d_trlwe = ctypes.c_void_p()
        assert L.iyk_hip_trlwe_alloc(0, CELLS, ctypes.byref(d_trlwe)) == 0
        try:
            assert L.iyk_hip_trlwe_upload(st.h, d_trlwe, CELLS, 0, CELLS, cells.ctypes.data_as(_u32p)) == 0
            st.sync()
            bare = hip.resident_key_bytes()
            table_built = False
            case_list = K.cases(cus, p.t)
            assert K.reached_shapes(case_list, p.t, cus) >= {s for s in K.expected_shapes() if s[0] != "table"}
            for kind, smax, n in case_list:
                form, groups, slices = K.ks_geometry(kind, smax, n, p.t, cus)
                _set_ks_env(monkeypatch, kind, smax)
                runs = [np.array([c], dtype=np.int32) for c in singles] if n == 1 else [K.job_layout(n, special, CELLS, rng)]
                for idx in runs:
                    if n >= 64:
                        assert set(special[:20]) <= set(idx.tolist())
                    got, out_slot = _run_case(hip, st, d_trlwe.value, CELLS, idx, p, rng)
                    _check_case(got, out_slot, idx, ref, nchosen,
                                f"t={p.t} IYK_HIP_KS_KERNEL={kind} SHARED_MAX={smax} n={n}: {form} {groups} x {slices}")
                table_built |= form == "table"
                assert hip.resident_key_bytes() - bare == (K.table_bytes(p) if table_built else 0), (kind, smax, n)
            assert table_built
        finally:
            assert L.iyk_hip_trlwe_free(0, d_trlwe) == 0
            st.destroy()
    finally:
        hip.cleanup()


def test_key_switch_table_and_field_key_follow_a_new_key(keys128, oracle128, monkeypatch):
    """Table and field key built with the seed-1 keys, cleanup, initialise with seed-2 keys: the resident bytes are the bare keys
    again, a 4 097-job table case equals the seed-2 oracle word for word (and not the seed-1 words), and a 64-gate batch on the
    field-key rotation kernel (IYK_HIP_ROT_KERNEL=w32) equals the seed-2 oracle."""
    from iyokan_amd import hip

    for v in KS_ENV:
        monkeypatch.delenv(v, raising=False)
    p = keys128.params
    keys2 = client.keygen(params_128bit(), seed=2)
    orc2 = oracle_lib.Oracle(keys2)
    n = 4097
    cells, nchosen = _cells(p, n, seed=7)
    refs = {1: _reference(oracle128, cells), 2: _reference(orc2, cells)}
    rng = np.random.default_rng(77)
    idx = K.job_layout(n, list(range(nchosen)), n, rng)
    ng, nin = 64, 16
    ops = np.array([OPS["NAND"], OPS["MUX"], OPS["XOR"], OPS["ANDNOT"]] * (ng // 4), dtype=np.int32)
    in0, in1, in2 = (rng.integers(0, nin, size=ng).astype(np.int32) for _ in range(3))
    in2 = np.where(ops == OPS["MUX"], in2, -1).astype(np.int32)
    out = np.arange(nin, nin + ng, dtype=np.int32)
    bits = rng.integers(0, 2, size=nin).astype(np.uint8)
    bare = {}
    try:
        for seed, keys, orc in ((1, keys128, oracle128), (2, keys2, orc2)):
            hip.initialize(keys, device_ids=(0,))
            try:
                bare[seed] = hip.resident_key_bytes()
                st = hip.Stream(0)
                L = hip.lib()
                d_trlwe = ctypes.c_void_p()
                assert L.iyk_hip_trlwe_alloc(0, n, ctypes.byref(d_trlwe)) == 0
                try:
                    assert L.iyk_hip_trlwe_upload(st.h, d_trlwe, n, 0, n, cells.ctypes.data_as(_u32p)) == 0
                    monkeypatch.setenv("IYK_HIP_KS_KERNEL", "2")
                    got, out_slot = _run_case(hip, st, d_trlwe.value, n, idx, p, rng)
                    assert hip.resident_key_bytes() == bare[seed] + K.table_bytes(p)
                    _check_case(got, out_slot, idx, refs[seed], nchosen, f"seed {seed}: table, {n} jobs")
                    if seed == 2:
                        differ = (got[out_slot] != refs[1][idx]).any(axis=1)
                        key_free = (refs[1][idx] == refs[2][idx]).all(axis=1)   # every digit 0: (0, .., 0, b) under any key
                        assert (differ | key_free).all() and differ.sum() > n // 2
                    # the field key (built on first use from the host copy of this initialisation's key)
                    monkeypatch.setenv("IYK_HIP_ROT_KERNEL", "w32")
                    host = np.zeros((nin + ng, p.n + 1), dtype=np.uint32)
                    host[:nin] = client.encrypt_bits(keys, bits, seed=70 + seed)
                    arena = hip.Arena(host.shape[0])
                    st.upload(arena, 0, host)
                    st.gate_batch(arena, ops, in0, in1, in2, out)
                    st.sync()
                    gates = st.download(arena, 0, host.shape[0])
                    arena.free()
                    monkeypatch.delenv("IYK_HIP_ROT_KERNEL")
                    field = p.n * 2 * p.l * 2 * p.N * 8
                    assert hip.resident_key_bytes() == bare[seed] + K.table_bytes(p) + field
                    ref = host.copy()
                    orc.gate_batch(ops, in0, in1, in2, out, ref, nthreads=min(16, os.cpu_count() or 1))
                    assert np.array_equal(gates, ref), f"seed {seed}: w32 gates differ from the oracle"
                finally:
                    assert L.iyk_hip_trlwe_free(0, d_trlwe) == 0
                    st.destroy()
            finally:
                hip.cleanup()
    finally:
        orc2.close()
    assert bare[2] == bare[1]
