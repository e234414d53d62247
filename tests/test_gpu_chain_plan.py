"""GPU: what the pure planner (csrc/wn_plan.h: wn_chain_plan, run on the CPU through tests/chain_plan_lib.py) plans for the device's CU count IS what
wn_create builds -- every planned value wn_get_info reports, on every kernel variant, the slot form, rounds, a padded shape and under each development pin.
No job is launched: handles are created and asked."""
import ctypes

import pytest

import chain_plan_cases as cc
import chain_plan_lib as cl
from mi355_wavenet import _abi

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("label,model,ns,pins,flags", cc.CASES, ids=[c[0] for c in cc.CASES])
def test_live_handle_is_what_the_planner_planned(monkeypatch, label, model, ns, pins, flags):
    for k in cc.PINS:
        monkeypatch.delenv(k, raising=False)
    for k, v in pins.items():
        monkeypatch.setenv(k, v)
    lib = _abi.load_product_library()
    c = _abi.wn_config()
    for f in cc.CONFIG_FIELDS:
        setattr(c, f, model[f])
    c.bias, c.n_streams, c.device_id = (1 if model["bias"] else 0), ns, 0
    c.reserved[0] = flags
    h = ctypes.c_void_p()
    lib.check(lib.dll.wn_create(ctypes.byref(c), ctypes.byref(h)))
    try:
        info = _abi.wn_info()
        lib.check(lib.dll.wn_get_info(h, ctypes.byref(info)))
    finally:
        lib.dll.wn_destroy(h)
    live = {f: int(getattr(info, f)) for f in cc.INFO_FIELDS}
    planned = cl.plan(model, ns, int(info.n_compute_units), pins, flags)["info"]
    print(label, live)
    assert live == planned
    assert int(info.dev_overrides) == (1 if pins else 0)
    if info.n_compute_units == 256:   # the device the parent's values were recorded on
        assert live == cc.PARENT_INFO[label]
