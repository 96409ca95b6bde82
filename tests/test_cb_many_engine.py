"""CPU: cb_many on runner.CmuxCipherEngine, on the recording rig of tests/test_cmux_stage_cb.py.  With cb_many=True every circuit
bootstrapping of a clock is a circuit_bootstrap_many_batch with the arguments of the per-digit call; with it off the recording is
today's; a snapshot taken with one setting is refused by an engine of the other."""
import numpy as np
import pytest

import test_cmux_stage_cb as rig_mod
from test_cmux_stage_cb import PARENT_DIGEST, _clocks, _digest, _engine, four  # noqa: F401  (four: the fixture)

PER_DIGIT, MANY = "circuit_bootstrap_batch", "circuit_bootstrap_many_batch"


def _renamed(log):
    return [(sid, PER_DIGIT if name == MANY else name, args, kw) for sid, name, args, kw in log]


@pytest.mark.parametrize("flags", [{}, {"stage_cb": True}, {"stage_cb": True, "refresh_aside": True}, {"rom_fused": True, "tree_fused": True}])
def test_every_circuit_bootstrapping_is_the_many_call_with_the_same_arguments(monkeypatch, four, flags):
    off, rig_off = _engine(monkeypatch, four, **flags)
    _clocks(off, four)
    on, rig_on = _engine(monkeypatch, four, cb_many=True, **flags)
    _clocks(on, four)
    names_on = [c[1] for c in rig_on.log]
    assert PER_DIGIT not in names_on and names_on.count(MANY) == [c[1] for c in rig_off.log].count(PER_DIGIT) > 0
    # slots, first lvl2 slot, first selector slot, the stores and their sizes: the per-digit call's, call for call
    assert _digest(_renamed(rig_on.log)) == _digest(rig_off.log)
    assert (on.tlwe2.slots, on.scratch.slots) == (off.tlwe2.slots, off.scratch.slots)
    off.free()
    on.free()


def test_cb_many_off_is_todays_recording(monkeypatch, four):
    eng, rig = _engine(monkeypatch, four, cb_many=False)
    _clocks(eng, four)
    eng.free()
    assert _digest(rig.log) == PARENT_DIGEST


def test_read_early_sends_the_many_call_on_the_port_stream(monkeypatch, four):
    from iyokan_amd import runner
    from iyokan_amd.frontier import FrontierExecutor, FrontierPlan

    rig = rig_mod._Rig(monkeypatch)
    plan = FrontierPlan(four.nl, 1, stages=four.stages, early=four.ports)
    be = rig_mod._Backend(rig, plan.num_slots)
    n1 = int(rig_mod.P.n) + 1
    eng = runner.CmuxCipherEngine(four, FrontierExecutor(plan, be), lambda bits: np.zeros((len(bits), n1), dtype=np.uint32),
                                  lambda rows: [0] * len(rows), np.zeros(n1, dtype=np.uint32), rig_mod._Key("bk2", int(rig_mod.P.n)),
                                  rig_mod._Key("pk"), packet=rig_mod._Packet(four), decrypt_ram=lambda rows: [0] * len(rows), read_early=True,
                                  cb_many=True)
    _clocks(eng, four)
    calls = [(sid, name) for sid, name, _, _ in rig.log if name in (PER_DIGIT, MANY)]
    assert calls and all(name == MANY and sid == eng.port_stream.sid for sid, name in calls)
    eng.free()


def test_a_snapshot_of_one_setting_is_refused_by_the_other(monkeypatch, four):
    off, _ = _engine(monkeypatch, four)
    on, _ = _engine(monkeypatch, four, cb_many=True)
    snap_off, snap_on = off.state(), on.state()
    assert "cb_many" not in snap_off.meta and snap_on.meta["cb_many"] is True      # off: the metadata of every snapshot taken so far
    with pytest.raises(ValueError, match="cb_many=True, this engine has cb_many=False"):
        off.check_state(snap_on)
    with pytest.raises(ValueError, match="cb_many=False, this engine has cb_many=True"):
        on.check_state(snap_off)
    off.check_state(snap_off)
    on.check_state(snap_on)
    off.free()
    on.free()
