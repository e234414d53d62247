"""The configurations the chain planner (csrc/wn_plan.h: wn_chain_plan) is checked on, shared by tests/test_chain_plan_host.py (CPU) and
tests/test_gpu_chain_plan.py (against wn_get_info of a live handle), and what the library reported for them BEFORE the planner existed."""
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "pytorch-wavenet_amd"))
from mi355_wavenet import synth  # noqa: E402

WN_CFG_NO_PADDING = 1   # include/wn_abi.h
SMALL = dict(layers=3, blocks=2, dilation_channels=16, residual_channels=16, skip_channels=256, end_channels=32, classes=256, kernel_size=2, bias=False)
SMALL2 = dict(SMALL, dilation_channels=32)                  # the small test shape split two ways (16 dilation channels per slice)
LEAN4 = dict(synth.CONFIGS["cfg3"], layers=4, blocks=1)     # cfg3's channel shape on a short stack (the tests' stand-in for the slot form)
ODD = dict(SMALL, dilation_channels=10, residual_channels=7, skip_channels=13, end_channels=9)   # zero-padded into the small test shape
K3 = dict(synth.CONFIGS["tiny"], kernel_size=3)

# (label, model, streams, development pins, wn_config.reserved[0])
CASES = [("small_x%d" % n, SMALL, n, {}, 0) for n in (1, 2, 12)] + [("small2_x%d" % n, SMALL2, n, {}, 0) for n in (1, 2, 12)] + [
    ("cfg1_x1", synth.CONFIGS["cfg1"], 1, {}, 0), ("cfg1_x4", synth.CONFIGS["cfg1"], 4, {}, 0),
    ("cfg2_x1", synth.CONFIGS["cfg2"], 1, {}, 0), ("cfg2_x4", synth.CONFIGS["cfg2"], 4, {}, 0),
    ("chaconne_x1", synth.CONFIGS["chaconne"], 1, {}, 0), ("chaconne_x4", synth.CONFIGS["chaconne"], 4, {}, 0),
    ("cfg2_x8", synth.CONFIGS["cfg2"], 8, {}, 0), ("chaconne_x12", synth.CONFIGS["chaconne"], 12, {}, 0),   # past the stacked kernel's stream limit
    ("cfg3_x1", synth.CONFIGS["cfg3"], 1, {}, 0), ("cfg3_x64", synth.CONFIGS["cfg3"], 64, {}, 0), ("cfg3_x96", synth.CONFIGS["cfg3"], 96, {}, 0),
    ("cfg3_x300_rounds", synth.CONFIGS["cfg3"], 300, {}, 0),
    ("k3_generic", K3, 2, {}, 0),
    ("odd_padded", ODD, 2, {}, 0), ("odd_unpadded", ODD, 2, {}, WN_CFG_NO_PADDING),
    ("pin_generic", synth.CONFIGS["cfg1"], 2, {"WN_KERNEL": "generic"}, 0),
    ("pin_v3", synth.CONFIGS["cfg1"], 1, {"WN_KERNEL": "v3"}, 0),
    ("pin_mode3", SMALL2, 4, {"WN_V3_MODE": "3"}, 0),
    ("pin_slots4", LEAN4, 8, {"WN_V3_MODE": "3", "WN_V3_SLOTS": "4"}, 0),
]
PINS = ("WN_KERNEL", "WN_SAMPLERS", "WN_V3_MODE", "WN_V3_SLOTS", "WN_CHAINS", "WN_NO_LOCAL_STORES")
CONFIG_FIELDS = ("layers", "blocks", "dilation_channels", "residual_channels", "skip_channels", "end_channels", "classes", "kernel_size")
# what the planner decides and wn_get_info reports
INFO_FIELDS = ("kernel_variant", "layer_split", "head_split", "n_workgroups", "lds_bytes", "streams_per_item", "head_replicas", "n_samplers",
               "layers_per_workgroup", "skip_lane_slots", "gate_need_per_xcd", "n_chains", "queue_bytes", "handoff_bytes", "weight_bytes")
# configurations wn_create refuses: (label, model, streams)
REFUSALS = [("layers_25", dict(SMALL, layers=25, blocks=1), 1),
            ("chain_too_long", dict(K3, layers=10, blocks=110), 2)]   # 1100 generic layer workgroups: more than 256 CUs x 4 hold
# wn_get_info of a fresh handle for every case, recorded ONCE from the library of commit 1ed2b42 (the parent of the planner: one function planned, allocated and
# queried in one pass) on an MI355X of 256 CUs -- the ground truth of tests/test_chain_plan_host.py and, on such a device, tests/test_gpu_chain_plan.py.  INFO_FIELDS order.
PARENT_INFO = {k: dict(zip(INFO_FIELDS, v)) for k, v in {
    "small_x1": (3, 1, 1, 8, 162816, 1, 1, 1, 1, 0, 8, 1, 1280, 15240, 231424),
    "small_x2": (3, 1, 1, 9, 162816, 1, 1, 2, 1, 0, 9, 1, 2560, 30480, 231424),
    "small_x12": (3, 1, 1, 12, 35008, 1, 2, 4, 1, 0, 12, 1, 15360, 182880, 231424),
    "small2_x1": (3, 2, 1, 14, 162816, 1, 1, 1, 1, 0, 14, 1, 2560, 28296, 378880),
    "small2_x2": (3, 2, 1, 15, 162816, 1, 1, 2, 1, 0, 15, 1, 5120, 56592, 378880),
    "small2_x12": (3, 2, 1, 18, 35008, 1, 2, 4, 1, 0, 18, 1, 30720, 339552, 378880),
    "cfg1_x1": (4, 1, 4, 7, 85632, 1, 1, 1, 5, 0, 7, 1, 9216, 13064, 1384448),
    "cfg1_x4": (3, 1, 4, 18, 162816, 1, 1, 4, 1, 0, 18, 1, 36864, 125984, 1128448),
    "cfg2_x1": (4, 1, 4, 15, 102848, 1, 1, 1, 3, 0, 15, 1, 793344, 34312, 5267456),
    "cfg2_x4": (4, 1, 4, 18, 107456, 1, 1, 4, 3, 0, 18, 1, 3173376, 137248, 5267456),
    "chaconne_x1": (4, 1, 16, 32, 136448, 1, 1, 1, 2, 0, 32, 1, 396672, 159752, 8278016),
    "chaconne_x4": (4, 1, 16, 35, 136448, 1, 1, 4, 2, 0, 28, 1, 1586688, 639008, 8278016),
    "cfg2_x8": (3, 1, 4, 38, 68320, 1, 1, 4, 1, 0, 24, 1, 6346752, 684096, 5113856),
    "chaconne_x12": (3, 2, 16, 80, 136576, 1, 1, 4, 1, 0, 32, 1, 9520128, 6478944, 7602176),
    "cfg3_x1": (3, 4, 8, 209, 162816, 1, 1, 1, 1, 0, 32, 1, 10577920, 1041416, 31244288),
    "cfg3_x64": (3, 4, 8, 220, 135552, 2, 2, 4, 1, 0, 32, 1, 676986880, 66650624, 31244288),
    "cfg3_x96": (3, 4, 8, 220, 135552, 2, 2, 4, 1, 4, 32, 1, 1015480320, 99975936, 31244288),
    "cfg3_x300_rounds": (3, 4, 8, 660, 135552, 2, 2, 4, 1, 4, 32, 3, 3173376000, 312424800, 93732864),
    "k3_generic": (1, 1, 1, 7, 39328, 1, 1, 0, 1, 0, 1, 1, 4352, 8720, 152704),
    "odd_padded": (3, 1, 1, 9, 162816, 1, 1, 2, 1, 0, 9, 1, 2560, 30480, 231424),
    "odd_unpadded": (1, 1, 1, 7, 18624, 1, 1, 0, 1, 0, 1, 1, 1120, 6032, 98352),
    "pin_generic": (1, 1, 4, 14, 134688, 1, 1, 0, 1, 0, 2, 1, 18432, 62480, 1094656),
    "pin_v3": (3, 1, 4, 15, 162816, 1, 1, 1, 1, 0, 15, 1, 9216, 31496, 1128448),
    "pin_mode3": (3, 2, 1, 18, 162816, 1, 2, 4, 1, 0, 18, 1, 10240, 113184, 378880),
    "pin_slots4": (3, 4, 8, 36, 135552, 2, 2, 4, 1, 4, 32, 1, 311296, 794688, 3358720),
}.items()}
# ... and the return code and wn_last_error() of the refused ones
PARENT_REFUSALS = {
    "layers_25": (-2, 'wn_create: layers > 24 (dilation 2^layers overflows the queue)'),
    "chain_too_long": (-2, 'wn_create: the chain needs 1101 co-resident workgroups but the device admits only 1024'),
}
