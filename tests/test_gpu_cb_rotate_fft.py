"""GPU: the FP64 FFT form of the lvl2 bootstrapping key (hip.Bk2Key(form="fft"), iyk_hip_bk2_key_create_form) and the kernel that
rotates under it (cb_rotate_fft_kernel), word for word against the numpy restatement, against the integer key's kernels, through
iyk_hip_circuit_bootstrap_batch and through one clock of runner.CmuxCipherEngine; the key object's form, byte count and refusals; and
the kernel's recorded rounding distance against the bound proven in DESIGN.md §2b."""
import ctypes
import math
import os
import re
import subprocess
import sys

import numpy as np
import pytest

import cb_rotate_fft_cases as cases
import cb_rotate_ref as ref
import cmux_system_cases as system_cases
from test_gpu_cb_rotate import FILL, _arena, _check, _n2_inputs, _n2_jobs, _run

pytestmark = pytest.mark.gpu

N2 = ref.N2
KNOB = "IYK_HIP_CB_KERNEL"
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def key_bytes(n, form):
    """device bytes of one key: the spectra of its steps and the transform's tables behind them"""
    return (n * 2 * 8 * 2 * N2 + 2 * N2) * 8 if form == "ntt" else (n * 4 * 8 * 2 * (N2 // 2) + 2 * (N2 // 2) + 64) * 16


@pytest.fixture(scope="module")
def gpu(request):
    import torch

    from iyokan_amd import hip

    keys = request.getfixturevalue("keys128")
    hip.initialize(keys, device_ids=(0, 0))   # two replicas on one GPU: a key of the other replica can be offered
    st = hip.Stream(0)
    made = {}
    yield hip, keys, st, made, torch
    for key in made.values():
        key.free()
    st.destroy()
    hip.cleanup()


def _fkey(gpu, name, form="fft"):
    """the case's key in the given form, resident once per module, uploaded as one step and then the rest"""
    hip, _, st, made, _ = gpu
    if (name, form) not in made:
        bk, _ = cases.case(name)
        key = hip.Bk2Key(bk.shape[0], form=form)
        key.upload(st, 0, bk[:1])
        if bk.shape[0] > 1:
            key.upload(st, 1, bk[1:])
        made[name, form] = key
    return made[name, form]


_FULL_BK = {}


def _full_key(gpu, form):
    """a uniform key at the initialised n = 636, resident once per module and form, uploaded in windows"""
    hip, keys, st, made, _ = gpu
    if "bk" not in _FULL_BK:
        _FULL_BK["bk"] = np.random.default_rng(636).integers(0, 1 << 64, size=(keys.params.n, 2 * cases.L2, 2, N2), dtype=np.uint64)
    if ("full", form) not in made:
        bk = _FULL_BK["bk"]
        key = hip.Bk2Key(bk.shape[0], form=form)
        for first in range(0, bk.shape[0], 200):
            key.upload(st, first, bk[first:first + 200])
        made["full", form] = key
    return made["full", form]


@pytest.mark.parametrize("name", cases.CASES)
def test_cases_word_for_word(gpu, name):
    bk, jobs = cases.case(name)
    want = cases.expected(name)
    tl = np.stack([j[0] for j in jobs])
    out = list(range(len(jobs)))[::-1]
    got = _run(gpu, _fkey(gpu, name), tl, [(g, s, off, mu, out[g]) for g, (_, s, off, mu) in enumerate(jobs)], len(jobs) + 1)
    for g in range(len(jobs)):
        bad = np.flatnonzero(got[out[g]] != want[g])
        assert bad.size == 0, (name, g, bad[:8])
    assert (got[len(jobs)] == FILL).all()


@pytest.mark.parametrize("count", [1, 3, 27, "2cus+1"])
def test_batch_shapes(gpu, count):
    import torch

    cus = torch.cuda.get_device_properties(0).multi_processor_count
    count = 2 * cus + 1 if count == "2cus+1" else count     # the last: two rounds and one job of a third inside one launch
    slots = count + 3 if count > 1 else 2
    jobs = _n2_jobs(count, slots)
    assert len({j[4] for j in jobs}) == count
    _check(_run(gpu, _fkey(gpu, "uniform-n2"), _n2_inputs(), jobs, slots), jobs, slots)


def test_queued_batches_on_reused_slots_and_two_streams(gpu):
    hip, _, st, _, torch = gpu
    key = _fkey(gpu, "uniform-n2")
    slots = 12
    a, b = _n2_jobs(5, slots), _n2_jobs(7, slots, salt=3)
    arena, s1, s2, s3 = _arena(gpu, _n2_inputs()), hip.Tlwe2(N2, slots), hip.Tlwe2(N2, slots), hip.Tlwe2(N2, slots)
    st2 = hip.Stream(0)
    args = lambda jobs: tuple(zip(*[j[:4] for j in jobs]))
    try:
        fill = np.full((slots, N2 + 1), FILL, dtype=np.uint64)
        for s in (s1, s2, s3):
            s.upload(st, 0, fill)
        st.sync()                                                           # the fills above, before another stream writes s3
        torch.cuda.synchronize()                                            # and the arena's copy, which torch's stream made
        st.cb_rotate_batch(key, arena, *args(a), s1, [j[4] for j in a])     # the same batch twice without a sync
        st.cb_rotate_batch(key, arena, *args(a), s1, [j[4] for j in a])
        st.cb_rotate_batch(key, arena, *args(a), s2, [j[4] for j in a])     # two different batches back to back
        st.cb_rotate_batch(key, arena, *args(b), s2, [j[4] for j in b])
        st2.cb_rotate_batch(key, arena, *args(b), s3, [j[4] for j in b])    # a second stream on the same key
        g1, g2, g3 = s1.download(st, 0, slots), s2.download(st, 0, slots), s3.download(st2, 0, slots)
    finally:
        for s in (s1, s2, s3):
            s.free()
        st2.destroy()
    _check(g1, a, slots)
    _check(g3, b, slots)
    later = {j[4] for j in b}
    assert later & {j[4] for j in a}
    _check(g2, [j for j in a if j[4] not in later] + b, slots)


def test_full_size_both_forms_give_equal_stores(gpu, monkeypatch):
    """one rotation at n = 636 under a uniform key of each form (the integer key under lat, which tests/test_gpu_cb_rotate_lat.py pins
    to the emulation): equal stores, word for word"""
    hip, keys = gpu[0], gpu[1]
    n = keys.params.n
    tl = cases.base._u32(np.random.default_rng(41), (2, n + 1))
    jobs = [(1, -1, 0x9E3779B9, ref.mu_of(1, 6), 1)]
    monkeypatch.setenv(KNOB, "lat")
    stores = {form: _run(gpu, _full_key(gpu, form), tl, jobs, 3) for form in ("ntt", "fft")}
    assert np.array_equal(stores["ntt"], stores["fft"])
    assert (stores["fft"][1] != FILL).all() and (stores["fft"][[0, 2]] == FILL).all()


def test_circuit_bootstrap_batch_gives_the_integer_keys_selector_words(gpu):
    """a 2-bit address at the initialised n = 636: iyk_hip_circuit_bootstrap_batch with a key of either form leaves the same lvl2 TLWEs
    and the same (k+1) l selector rows per bit (the selector slots are trgsw_from_rows of those rows on both sides)"""
    from iyokan_amd import client

    hip, keys, st, made, _ = gpu
    p = keys.params
    A, l, per = 2, int(p.l), int(p.trgsw_rows)
    if "privks" not in made:
        pk = hip.PrivKsKey(N2, 1, 1)
        pk.upload(st, 0, np.random.default_rng(92).integers(0, 1 << 32, size=(pk.rows, pk.words), dtype=np.uint64).astype(np.uint32))
        made["privks"] = pk
    pk = made["privks"]
    arena = hip.Arena(3)
    st.upload(arena, 0, client.encrypt_bits(keys, [1, 0, 1], seed=77))
    forms = ("ntt", "fft")
    t2 = {k: hip.Tlwe2(N2, A * l + 1) for k in forms}
    rows = {k: hip.Trlwe(A * per) for k in forms}
    trgsw = {k: hip.Trgsw(A) for k in forms}
    got = {}
    try:
        for k in forms:
            t2[k].upload(st, 0, np.full((A * l + 1, N2 + 1), FILL, dtype=np.uint64))
            st.circuit_bootstrap_batch(_full_key(gpu, k), pk, arena, [2, 0], [1, -1], t2[k], 1, rows[k], trgsw[k])
            got[k] = (t2[k].download(st, 0, A * l + 1), rows[k].download(st, 0, A * per))
    finally:
        for store in list(t2.values()) + list(rows.values()) + list(trgsw.values()) + [arena]:
            store.free()
    assert np.array_equal(got["ntt"][0], got["fft"][0]) and (got["fft"][0][0] == FILL).all() and (got["fft"][0][1:] != FILL).any()
    assert np.array_equal(got["ntt"][1], got["fft"][1]) and got["fft"][1].any()


def _one_clock(gpu, sysm, bk2, pk):
    """one run() + tick() of the small system from a chosen register state: the rdata TLWEs of both memories and the RAM cells after"""
    from iyokan_amd.packet import TFHEPacket

    keys = gpu[1]
    packet = TFHEPacket.encrypt(keys, system_cases.request(3, 1), seed=500)
    eng, be = system_cases.gpu_engine(keys, sysm, bk2, pk, packet)
    try:
        rom, ram = sysm.ports
        eng.load_rom("rom", None)
        eng.load_ram("ram", None)
        root, slot = sysm.nl.roots(), eng.ex.plan.slot
        eng.set_nodes([root[a] for a in rom.addr] + [root[ram.wren[0]]], [1, 0, 1, 1])      # counter = 5, wren = 1
        cells0 = eng.mem["ram"].cells()
        eng.run()
        read = lambda nodes: be.read_many([slot[i] for i in nodes])
        d_rom, d_ram = read(rom.rdata), read(ram.rdata)
        eng.tick()
        return d_rom, d_ram, eng.mem["ram"].cells(), cells0
    finally:
        eng.free()
        be.close()


def test_one_clock_of_the_small_system_equals_the_integer_keys(gpu, tmp_path):
    from iyokan_amd.system import load_blueprint

    hip, keys, st, made, _ = gpu
    if "privks" not in made:
        pk = hip.PrivKsKey(N2, 1, 1)
        pk.upload(st, 0, np.random.default_rng(92).integers(0, 1 << 32, size=(pk.rows, pk.words), dtype=np.uint64).astype(np.uint32))
        made["privks"] = pk
    sysm = load_blueprint(system_cases.write_blueprint(str(tmp_path)), cmux_memories=True)
    st.sync()
    runs = {form: _one_clock(gpu, sysm, _full_key(gpu, form), made["privks"]) for form in ("ntt", "fft")}
    for part in range(3):
        assert np.array_equal(runs["ntt"][part], runs["fft"][part]), part
    assert (runs["fft"][2] != runs["fft"][3]).any(axis=2).all()                              # every cell was refreshed
    assert runs["fft"][0].any() and runs["fft"][1].any()


def test_form_attribute_and_key_bytes(gpu):
    hip, _, _, made, _ = gpu
    live = lambda: sum(key_bytes(k.n, k.form) for k in made.values() if isinstance(k, hip.Bk2Key))
    assert hip.bk2_key_bytes(0) == live()
    a = hip.Bk2Key(3)
    assert a.form == "ntt" and hip.bk2_key_bytes(0) == live() + key_bytes(3, "ntt")
    b = hip.Bk2Key(5, form="fft")
    assert b.form == "fft" and hip.bk2_key_bytes(0) == live() + key_bytes(3, "ntt") + key_bytes(5, "fft")
    assert key_bytes(5, "fft") == 5 * (1 << 20) + 2112 * 16                                  # 1 MiB per step, then the tables
    c = hip.Bk2Key(2, form="ntt")
    assert c.form == "ntt"
    a.free()
    assert hip.bk2_key_bytes(0) == live() + key_bytes(5, "fft") + key_bytes(2, "ntt")
    b.free()
    c.free()
    assert hip.bk2_key_bytes(0) == live()
    form = ctypes.c_int(7)
    key = _fkey(gpu, "uniform-n2")
    assert hip.lib().iyk_hip_bk2_key_form(key.h, ctypes.byref(form)) == 0 and form.value == 1
    assert hip.lib().iyk_hip_bk2_key_form(None, ctypes.byref(form)) == -1


def test_refusals_leave_the_store_untouched_and_the_stream_usable(gpu, monkeypatch):
    hip, _, st, _, _ = gpu
    key = _fkey(gpu, "uniform-n2")
    bk, _ = cases.case("uniform-n2")
    arena, store = _arena(gpu, _n2_inputs()), hip.Tlwe2(N2, 4)
    fill = np.full((4, N2 + 1), FILL, dtype=np.uint64)
    mu = [1 << 56]
    before = hip.bk2_key_bytes(0)
    other = hip.Bk2Key(2, gpu_index=1, form="fft")
    try:
        store.upload(st, 0, fill)
        h = ctypes.c_void_p()
        for form in (2, 3, -1, 255):                                                        # an unknown form
            assert hip.lib().iyk_hip_bk2_key_create_form(0, 2, 4, 9, form, ctypes.byref(h)) == -1 and not h.value
            assert b"form" in hip.lib().iyk_hip_last_error()
        with pytest.raises(ValueError, match="form"):
            hip.Bk2Key(2, form="fp64")
        for n, l2, bg in ((2, 3, 9), (2, 4, 10), (0, 4, 9), (2048, 4, 9)):                   # (l2, Bgbit2) != (4, 9); n outside the range
            with pytest.raises(hip.IykHipError, match=r"iyk_hip_bk2_key_create_form failed \(-1\): .+"):
                hip.Bk2Key(n, l2, bg, form="fft")
        assert hip.bk2_key_bytes(0) == before
        assert hip.bk2_key_bytes(1) == key_bytes(2, "fft")
        with pytest.raises(hip.IykHipError, match=r"the stream and the key are on different GPUs"):   # a key of another replica
            other.upload(st, 0, bk)
        with pytest.raises(hip.IykHipError, match=r"the stream and the key are on different GPUs"):
            st.cb_rotate_batch(other, arena, [0], [1], [0], mu, store, [0])
        monkeypatch.setenv(KNOB, "nonsense")                                                # an unknown kind, whatever the key
        with pytest.raises(hip.IykHipError, match=r"iyk_hip_cb_rotate_batch failed \(-1\): .*IYK_HIP_CB_KERNEL"):
            st.cb_rotate_batch(key, arena, [1], [1], [0], mu, store, [3])
        with pytest.raises(hip.IykHipError, match=r"iyk_hip_cb_rotate_batch failed \(-1\): .+"):     # the batch's own checks stay
            st.cb_rotate_batch(key, arena, [0, 1], [1, 1], [0, 0], mu * 2, store, [2, 2])
        assert np.array_equal(store.download(st, 0, 4), fill)
        for kind in ("wg", "lat", None):                                                    # wg / lat do not affect a form-1 key
            if kind is None:
                monkeypatch.delenv(KNOB)
            else:
                monkeypatch.setenv(KNOB, kind)
            store.upload(st, 0, fill)
            st.cb_rotate_batch(key, arena, [1], [1], [0], mu, store, [3])
            _check(store.download(st, 0, 4), [(1, 1, 0, mu[0], 3)], 4)
    finally:
        other.free()
        store.free()
    assert hip.bk2_key_bytes(1) == 0


def test_recorded_round_error_is_inside_the_proven_bound():
    """in a fresh process with IYK_HIP_DEBUG=1 (tests/cb_rotate_fft_child.py): `quarters-min` word for word, then iyk_hip_fft_round_error"""
    env = dict(os.environ, IYK_HIP_DEBUG="1")
    env.pop(KNOB, None)
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tests", "cb_rotate_fft_child.py")], capture_output=True, text=True, timeout=300, env=env)
    m = re.search(r"round error (\S+)", r.stdout)
    assert r.returncode == 0 and m, r.stdout + r.stderr
    err = float(m.group(1))
    print(f"quarters-min on the GPU: largest |z - rint(z)| = {err:.3e} = 2^{math.log2(err) if err else float('-inf'):.1f}")
    assert 0.0 < err <= cases.PROVEN_BOUND
