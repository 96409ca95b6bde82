"""GPU: every argument set of tests/batch_refusal_cases.py through the library's entry points gives the code and the text the parent
commit's library gave (tests/golden/batch_refusals_parent.json).  Own library lifetimes: the sets with debug = 1 need IYK_HIP_DEBUG=1 at
iyk_hip_init.  One stream; a refused set launches nothing, a legal one launches one to four jobs on zero-filled stores, and the final
synchronisation would report a fault of theirs."""
import json
import os

import pytest

import batch_refusal_cases as cases

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.parametrize("debug", [0, 1])
def test_refusals_equal_the_parents(keys128, monkeypatch, debug):
    from iyokan_amd import hip

    with open(os.path.join(ROOT, "tests", "golden", "batch_refusals_parent.json")) as f:
        golden = json.load(f)["cases"]
    monkeypatch.setenv("IYK_HIP_DEBUG", str(debug))
    hip.initialize(keys128, device_ids=(0,))
    try:
        stores = cases.Stores(hip)
        mine = [c for c in cases.CASES if c["args"].get("debug", 0) == debug]
        assert mine
        wrong = []
        for c in mine:
            got = list(stores.call(c))
            assert got[0] != -3, (c["id"], got)   # a HIP error: nothing more on this GPU
            if got != golden[c["id"]]:
                wrong.append((c["id"], got, golden[c["id"]]))
        stores.st.sync()
        stores.free()
        assert not wrong, wrong
    finally:
        hip.cleanup()
