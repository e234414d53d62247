"""CPU: the generation chain's planner (csrc/wn_plan.h: wn_chain_plan) and kernel choice (wn_kernel_slot, wn_slot_column), run through a host-only build
of a harness that includes the real list of instantiated shapes (tests/chain_plan_lib.py).  Ground truth of the plans: what wn_get_info of the library
reported for the same cases BEFORE the planner existed (chain_plan_cases.PARENT_INFO)."""
import itertools
import subprocess

import pytest

import chain_plan_cases as cc
import chain_plan_lib as cl

LDS_MAX = 163840 - 1024   # csrc/wn_plan.h: WN_LDS_MAX_BYTES


@pytest.fixture(scope="module")
def shapes():
    rows = [cl._kv("row " + l) for l in subprocess.check_output([cl.harness(), "shapes"]).decode().splitlines()]
    return rows


def test_the_list_of_shapes_and_their_facts(shapes):
    assert [r["kind"] for r in shapes] == [3] * 7 + [4] * 3 and [r["index"] for r in shapes] == list(range(7)) + list(range(3))
    cfg3 = shapes[0]
    assert (cfg3["R"], cfg3["DC"], cfg3["S"], cfg3["EC"], cfg3["Pm"]) == (128, 32, 512, 32, 4)
    assert (cfg3["pre0"], cfg3["pre1"], cfg3["nwl"], cfg3["nwh"], cfg3["stride"]) == (1120, 2160, 148, 98, 256)   # WnV3Lds<cfg3>::pre, NWL, NWH
    assert [r["has_slots"] for r in shapes] == [1] + [0] * 9 and all(r["has_g2"] or not r["has_slots"] for r in shapes)
    assert all(r["lanes"] == (256 if r["kind"] == 3 else 512) for r in shapes)


@pytest.mark.parametrize("label,model,ns,pins,flags", cc.CASES, ids=[c[0] for c in cc.CASES])
def test_plan_is_what_the_parent_built(shapes, label, model, ns, pins, flags):
    p = cl.plan(model, ns, 256, pins, flags)
    assert p["info"] == cc.PARENT_INFO[label]
    assert p["padded"] == (1 if label == "odd_padded" else 0)
    assert p["config"] == ((16, 16, 256, 32) if p["padded"] else tuple(model[k] for k in ("residual_channels", "dilation_channels", "skip_channels", "end_channels")))
    # the planned values wn_get_info has no field for, against their definitions
    for c in p["chains"]:
        assert c["map_len"] == c["n_blocks"] >= c["n_wg"] and 1 <= c["gate_need"] and c["gate_need"] * 8 >= c["n_wg"]
        if c["variant"] == 1:
            assert c["row"] == -1 and c["allow_plain"] == 0 and c["n_blocks"] == c["n_wg"] and c["n_lw"] == c["NL"] * c["P"]
            continue
        e = shapes[c["row"]]
        assert e["kind"] == c["variant"] and c["gate_need"] <= 32 and c["n_blocks"] % 8 == 0   # the layer-aligned placement: whole rounds over the 8 XCDs
        assert c["allow_plain"] == (0 if pins.get("WN_NO_LOCAL_STORES") == "1" else 1)
        assert c["n_lw"] == (-(-c["NL"] // e["Pm"]) if c["variant"] == 4 else c["NL"] * c["P"])
        assert c["head_blob_off"] == c["n_lw"] * c["LPW"] * e["nwl"] * e["lanes"] and c["blob_floats"] == c["head_blob_off"] + c["PA"] * e["nwh"] * 256
        assert c["start_in_lds"] == (1 if e["smp"] * 4 <= LDS_MAX else 0)
    if len(p["chains"]) > 1:   # rounds: every member the same chain but for its streams
        assert {(c["row"], c["P"], c["PA"], c["blob_floats"]) for c in p["chains"]} == {tuple(p["chains"][0][k] for k in ("row", "P", "PA", "blob_floats"))}
        assert sum(c["n_streams"] for c in p["chains"]) == ns and max(c["n_streams"] for c in p["chains"]) <= 128


def test_pins_that_only_the_cpu_sees():
    lean = cc.LEAN4
    assert cl.plan(lean, 8, 256, {"WN_NO_LOCAL_STORES": "1"})["chains"][0]["allow_plain"] == 0
    a, b = cl.plan(lean, 8), cl.plan(lean, 8)
    assert a == b and a["chains"][0]["map_digest"] != cl.plan(lean, 2)["chains"][0]["map_digest"]   # planning is a function; two samplers fewer: another map
    assert cl.plan(cc.synth.CONFIGS["cfg3"], 300, 256, {"WN_CHAINS": "1"})["info"]["n_chains"] == 1   # WN_CHAINS=1: no rounds
    assert cl.plan(cc.synth.CONFIGS["cfg1"], 4, 256, {"WN_SAMPLERS": "2"})["info"]["n_samplers"] == 2


@pytest.mark.parametrize("label,model,ns", cc.REFUSALS, ids=[r[0] for r in cc.REFUSALS])
def test_refusals_keep_their_code_and_text(label, model, ns):
    p = cl.plan(model, ns)
    assert (p["rc"], p["refused"]) == cc.PARENT_REFUSALS[label]


def test_refusals_of_bad_arguments():
    assert cl.plan(dict(cc.SMALL, kernel_size=0), 1) == {"rc": -1, "refused": "wn_create: kernel_size must be >= 1"}
    assert cl.plan(dict(cc.SMALL, classes=1), 1) == {"rc": -1, "refused": "wn_create: non-positive dimension in wn_config"}
    assert cl.plan(cc.SMALL, 1, flags=2) == {"rc": -1, "refused": "wn_create: negative split / non-zero reserved field"}


# (label, variant, slot form): the kernels a handle can have
HANDLES = [("form0", 3, 0), ("form1", 3, 0), ("slots", 3, 1), ("variant4", 4, 0), ("generic", 1, 0)]
PRODUCT, DIAG, FILTER = 0, 1, 2   # columns of the kernel tables


@pytest.mark.parametrize("label,variant,slot_form", HANDLES, ids=[h[0] for h in HANDLES])
def test_kernel_choice_truth_table(label, variant, slot_form):
    """What a job needs -> slot -> kernel: extras (filter, log-probability, forced samples) outrank stamps / logits dump; the forms 0 / 1 and variant 4 carry
    all of them in the DIAG instantiation, the slot form has ONE kernel for plain and diagnostic jobs and the filter kernel for extras, the generic kernel is one."""
    for stamps, dump, filt, logp, forced in itertools.product((0, 1), repeat=5):
        job = int(subprocess.check_output([cl.harness(), "job", str(stamps), str(dump), "8" if filt else "0", "0", str((2 if logp else 0) | (4 if forced else 0))]).decode())
        extras = filt or logp or forced
        assert job == (2 if extras else 1 if (stamps or dump) else 0)
        slot, col = (int(x) for x in subprocess.check_output([cl.harness(), "slot", str(variant), str(slot_form), str(int(stamps or dump)), str(int(extras))]).decode().split())
        assert slot == job
        if label == "generic":
            assert col == PRODUCT
        elif label == "slots":
            assert col == (FILTER if extras else PRODUCT)
        else:
            assert col == (DIAG if (extras or stamps or dump) else PRODUCT)
    assert int(subprocess.check_output([cl.harness(), "job", "0", "0", "0", "0.9", "0"]).decode()) == 2   # a nucleus filter alone
