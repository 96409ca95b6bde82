"""GPU: the edge cases of tests/cb_rotate_edge_cases.py on each of the three kernels of the lvl0 -> lvl2 rotation, by name: `wg`
(cb_rotate_kernel, IYK_HIP_CB_KERNEL=wg), `lat` (cb_rotate_lat_kernel, IYK_HIP_CB_KERNEL=lat) and `fft` (cb_rotate_fft_kernel, a key
of form="fft").  Every comparison is word for word on u64 [N2 + 1]; the store is filled with a canary first and the slots no job writes
must come back unchanged.  For the two integer forms hip.cb_rotate_form is asserted before every launch, so a test cannot run another
kernel than its id names.  tests/test_cb_rotate_edge_cases.py holds the emulation these words come from to the numpy restatement."""
import math

import numpy as np
import pytest

import cb_rotate_edge_cases as edge
import cb_rotate_ref as ref
from test_cb_rotate_lat_emul import emul as lat_emul, plan
from test_gpu_cb_rotate import FILL, _arena, _run

pytestmark = pytest.mark.gpu

N2 = ref.N2
KNOB = "IYK_HIP_CB_KERNEL"


@pytest.fixture(scope="module")
def gpu(request):
    import torch

    from iyokan_amd import hip

    keys = request.getfixturevalue("keys128")
    hip.initialize(keys, device_ids=(0,))
    st = hip.Stream(0)
    made = {}
    yield hip, keys, st, made, torch
    for key in made.values():
        key.free()
    st.destroy()
    hip.cleanup()


@pytest.fixture(params=edge.FORMS)
def form(request, monkeypatch):
    """the kernel form of the test's id: the knob for the integer forms; an FP64 key runs its own kernel whatever the knob says"""
    if request.param == "fft":
        monkeypatch.delenv(KNOB, raising=False)
    else:
        monkeypatch.setenv(KNOB, request.param)
    return request.param


def _key(gpu, name, form, bk, windows):
    """the first n steps of a torus-domain key in the form's key form, resident once per module, uploaded in the given windows"""
    hip, _, st, made, _ = gpu
    at = (name, edge.KEY_FORM[form])
    if at not in made:
        key = hip.Bk2Key(bk.shape[0], form=edge.KEY_FORM[form])
        assert windows[0] == 0 and windows[-1] == bk.shape[0] and len(windows) >= 3
        for first, last in zip(windows, windows[1:]):
            key.upload(st, first, bk[first:last])
        made[at] = key
    assert made[at].form == edge.KEY_FORM[form]
    return made[at]


def _assert_form(gpu, form, count):
    """the integer forms: cb_rotate_form is what dispatch::cb_plan answers for the knob's value, and that is the form of the id"""
    if form == "fft":
        return
    hip, _, _, _, torch = gpu
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    rc, want, _ = plan(count, cus, lat_emul().iyk_emul_cb_kind(form.encode(), 1))
    assert rc == 0 and want == {"wg": 0, "lat": 1}[form]
    assert hip.cb_rotate_form(count) == want, (form, count)


def _launch_and_compare(gpu, form, key, arena, jobs, want, slots):
    """jobs (in, sign, off, mu, out), want[g] the words of job g: the whole store after one batch, canary where nothing wrote"""
    _assert_form(gpu, form, len(jobs))
    got = _run(gpu, key, arena, jobs, slots)
    written = {}
    for g, job in enumerate(jobs):
        written[job[4]] = want[g]
    assert len(written) == len(jobs)
    for s in range(slots):
        if s in written:
            bad = np.flatnonzero(got[s] != written[s])
            assert bad.size == 0, (form, s, bad[:8])
        else:
            assert (got[s] == FILL).all(), f"slot {s} that no job writes changed"
    return got


def test_mid_n19(gpu, form):
    arena, six = edge.mid_case()
    slots = len(six) + 2
    out = edge.out_slots(len(six), slots, seed=19)
    key = _key(gpu, "mid", form, edge.mid_key(), [0, 1, edge.MID_N])
    _launch_and_compare(gpu, form, key, arena, [j + (out[g],) for g, j in enumerate(six)], edge.mid_expected(), slots)


def test_row_pass(gpu, form):
    want = edge.row_expected(form)
    for n in edge.ROW_NS:
        arena, two = edge.row_case(n)
        key = _key(gpu, f"row{n}", form, edge.row_key()[:n], [0, 200, n])
        _launch_and_compare(gpu, form, key, arena, [two[0] + (2,), two[1] + (0,)], want[n], 4)


def test_rounds_n19(gpu, form):
    """CUs + 3 jobs of 19 steps in one launch: three workgroups run a second job behind a first"""
    cus = gpu[4].cuda.get_device_properties(0).multi_processor_count
    arena, jobs, slots, which = edge.rounds_case(cus)
    key = _key(gpu, "mid", form, edge.mid_key(), [0, 1, edge.MID_N])
    six = edge.mid_expected()
    _launch_and_compare(gpu, form, key, arena, jobs, [six[w] for w in which], slots)


@pytest.mark.parametrize("name", ["128", "80"])
def test_full_size(gpu, form, name, request):
    """n = 636 / 500 under a real key uploaded in windows of 200 steps: the emulation's words for the form's key, and every off = 0
    output decrypts to (bit if sign == +1 else 1 - bit) * 2 mu_r inside edge.decrypt_bound(n), which is below mu_r / 2 for every r of
    both sets (asserted here and, on the emulation's words, by tests/test_cb_rotate_edge_cases.py)."""
    keys = request.getfixturevalue("keys" + name)
    p = keys.params
    l = int(p.l)
    s2, bk, arena, jobs, bits = edge.full_case(name, keys)
    key = _key(gpu, "full" + name, form, bk, list(range(0, p.n, 200)) + [p.n])
    slots = len(jobs) + 2
    out = edge.out_slots(len(jobs), slots, seed=p.n)
    got = _launch_and_compare(gpu, form, key, arena, [j + (out[g],) for g, j in enumerate(jobs)], edge.full_expected(name, form), slots)
    bound = edge.decrypt_bound(p.n)
    assert all(bound < ref.mu_of(r, int(p.Bgbit)) / 2 for r in range(l))
    errs = edge.phase_errors(s2, got[out[:4 * l]], jobs[:4 * l], bits[:4 * l])
    worst = max(map(abs, errs))
    print(f"set {name} {form}: worst |phase error| of {4 * l} rotations 2^{math.log2(max(worst, 1)):.2f}, bound 2^{math.log2(bound):.2f}")
    assert worst < bound, (name, form, errs, bound)
