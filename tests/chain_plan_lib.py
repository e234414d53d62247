"""The chain planner (csrc/wn_plan.h: wn_chain_plan) behind a small host program: it includes the REAL list of instantiated shapes with their facts
(csrc/wn_chain_shapes.h, which needs the device headers but names no kernel) and is compiled host-only, so it runs without a GPU.  plan() returns what
wn_create would build for a configuration -- per chain the raw planned values, and the view wn_get_info gives of them."""
import os
import subprocess
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "pytorch-wavenet_amd", "csrc")
sys.path.insert(0, os.path.join(ROOT, "pytorch-wavenet_amd"))

HARNESS = r"""
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include "wn_chain_shapes.h"
static const char* opt(const char* s) { return strcmp(s, "-") ? s : nullptr; }
static void chain(const WnChainPlan& c) {
    unsigned long long digest = 1469598103934665603ull;   // FNV-1a over the workgroup map
    for (int32_t v : c.wg_map) digest = (digest ^ (unsigned)v) * 1099511628211ull;
    const WnPlan& p = c.pl;
    printf("chain variant=%d row=%d P=%d PA=%d n_wg=%d lds_bytes=%d v3_mode=%d HR=%d n_smp=%d LPW=%d v3_slots=%d gate_need=%d ring_floats=%zu gran_count=%zu "
           "blob_floats=%zu C=%d R=%d NL=%d n_streams=%d n_blocks=%d allow_plain=%d start_in_lds=%d head_blob_off=%lld n_lw=%d map_len=%zu map_digest=%llu\n",
           c.variant, c.row, p.P, p.PA, p.n_wg, c.lds_bytes, c.v3_mode, p.HR, p.n_smp, p.LPW, c.v3_slots, c.gate_need, c.ring_floats, c.gran_count,
           c.blob_floats, p.C, p.R, p.NL, p.n_streams, p.n_blocks, p.allow_plain, p.start_in_lds, (long long)p.head_blob_off, p.n_lw, c.wg_map.size(), digest);
}
int main(int argc, char** argv) {
    const std::vector<WnChainShape>& sh = wn_chain_shapes();
    if (argc >= 2 && !strcmp(argv[1], "shapes")) {   // the facts of every listed shape
        for (const WnChainShape& e : sh)
            printf("kind=%d index=%d R=%d DC=%d S=%d EC=%d Pm=%d nwl=%d lanes=%d nwh=%d has_g2=%d has_slots=%d pre0=%d pre1=%d stride=%d head=%d smp=%d\n", e.kind, e.index,
                   e.R, e.DC, e.S, e.EC, e.Pm, e.nwl, e.lanes, e.nwh, e.has_g2, e.has_slots, e.lds_pre[0], e.lds_pre[1], e.lds_stride, e.lds_head, e.lds_smp);
        return 0;
    }
    if (argc >= 6 && !strcmp(argv[1], "slot")) {   // slot <variant> <slot form> <stamps or dump> <extras>: the slot of the job, the table column it resolves to
        const int slot = wn_kernel_slot(atoi(argv[4]) != 0, atoi(argv[5]) != 0);
        printf("%d %d\n", slot, wn_slot_column(atoi(argv[2]), atoi(argv[3]) != 0, slot));
        return 0;
    }
    if (argc >= 7 && !strcmp(argv[1], "job")) {   // job <prof> <dbg_logits> <top_k> <top_p> <logp>: wn_job_slot of such a WnRun
        WnRun r;
        memset(&r, 0, sizeof(r));
        static long long stamp; static float dump;
        if (atoi(argv[2])) r.prof = &stamp;
        if (atoi(argv[3])) r.dbg_logits = &dump;
        r.top_k = atoi(argv[4]); r.top_p = (float)atof(argv[5]); r.logp = atoi(argv[6]);
        printf("%d\n", wn_job_slot(r));
        return 0;
    }
    // plan <n_cu> <layers blocks D R S E classes k bias streams layer_split head_split reserved0> <WN_KERNEL WN_SAMPLERS WN_V3_MODE WN_V3_SLOTS | -> <WN_CHAINS> <WN_NO_LOCAL_STORES>
    if (argc < 22 || strcmp(argv[1], "plan")) return 2;
    const int n_cu = atoi(argv[2]);
    wn_config c;
    memset(&c, 0, sizeof(c));
    char** a = argv + 3;
    c.layers = atoi(a[0]); c.blocks = atoi(a[1]); c.dilation_channels = atoi(a[2]); c.residual_channels = atoi(a[3]); c.skip_channels = atoi(a[4]);
    c.end_channels = atoi(a[5]); c.classes = atoi(a[6]); c.kernel_size = atoi(a[7]); c.bias = atoi(a[8]); c.n_streams = atoi(a[9]);
    c.layer_split = atoi(a[10]); c.head_split = atoi(a[11]); c.reserved[0] = atoi(a[12]);
    WnPins pins = {};
    pins.kernel = opt(a[13]); pins.samplers = opt(a[14]); pins.v3_mode = opt(a[15]); pins.v3_slots = opt(a[16]);
    pins.no_rounds = a[17][0] == '1'; pins.no_local_stores = a[18][0] == '1';
    WnChainPlan cp;
    std::string why;
    const int rc = wn_config_refusal(c, why);
    if (rc) { printf("refused %d %s\n", rc, why.c_str()); return 0; }
    why = wn_chain_plan(c, n_cu, pins, sh.data(), (int)sh.size(), cp);
    if (!why.empty()) { printf("refused %d %s\n", WN_E_UNSUPPORTED, why.c_str()); return 0; }
    printf("plan padded=%d rounds=%zu R=%d D=%d S=%d E=%d\n", cp.padded ? 1 : 0, cp.rounds.size(), cp.cfg.residual_channels, cp.cfg.dilation_channels,
           cp.cfg.skip_channels, cp.cfg.end_channels);
    if (cp.rounds.empty()) chain(cp);
    for (const WnChainPlan& m : cp.rounds) chain(m);
    return 0;
}
"""

_exe = None
_dir = None


def harness():
    """Path of the compiled harness (built once per process)."""
    global _exe, _dir
    if _exe is None:
        import build as wn_build  # pytorch-wavenet_amd/build.py: where hipcc is
        _dir = tempfile.TemporaryDirectory(prefix="wn_chain_plan_")
        src = os.path.join(_dir.name, "chain_plan_harness.hip")
        with open(src, "w") as fh:
            fh.write(HARNESS)
        exe = os.path.join(_dir.name, "chain_plan_harness")
        subprocess.check_call([wn_build.hipcc_path(), "--offload-arch=gfx950", "--offload-host-only", "-std=c++17", "-O1", "-Wno-unused-function", "-Wno-inline-asm",
                               "-I", CSRC, src, "-o", exe])
        _exe = exe
    return _exe


def _kv(line):
    return {k: int(v) for k, v in (t.split("=") for t in line.split()[1:])}


def plan(model, n_streams, n_cu=256, pins=None, flags=0, layer_split=0, head_split=0):
    """-> {"rc": error code, "refused": the text of wn_last_error()} or {"padded", "config" (R, D, S, E as planned), "chains": [raw values per chain], "info": the wn_get_info view}."""
    pins = pins or {}
    args = [model[f] for f in ("layers", "blocks", "dilation_channels", "residual_channels", "skip_channels", "end_channels", "classes", "kernel_size")]
    args += [1 if model.get("bias") else 0, n_streams, layer_split, head_split, flags]
    args += [pins.get(k, "-") for k in ("WN_KERNEL", "WN_SAMPLERS", "WN_V3_MODE", "WN_V3_SLOTS")] + [pins.get("WN_CHAINS", "0"), pins.get("WN_NO_LOCAL_STORES", "0")]
    lines = subprocess.check_output([harness(), "plan", str(n_cu)] + [str(x) for x in args]).decode().splitlines()
    if lines[0].startswith("refused "):
        return {"rc": int(lines[0].split()[1]), "refused": "wn_create: " + lines[0].split(" ", 2)[2]}
    head = _kv(lines[0])
    chains = [_kv(l) for l in lines[1:]]
    assert len(chains) == max(1, head["rounds"])
    c0 = chains[0]
    info = {   # csrc/wn_runtime.hip: wn_get_info -- member 0's view, sizes and workgroups summed over the rounds
        "kernel_variant": c0["variant"], "layer_split": c0["P"], "head_split": c0["PA"], "lds_bytes": c0["lds_bytes"],
        "streams_per_item": 2 if c0["variant"] == 3 and c0["v3_mode"] & 1 else 1, "head_replicas": c0["HR"], "n_samplers": c0["n_smp"],
        "layers_per_workgroup": c0["LPW"] if c0["variant"] == 4 else 1, "skip_lane_slots": c0["v3_slots"] if c0["variant"] == 3 else 0,
        "gate_need_per_xcd": c0["gate_need"], "n_chains": len(chains),
        "n_workgroups": sum(c["n_wg"] for c in chains), "queue_bytes": sum(c["ring_floats"] * 4 for c in chains),
        "handoff_bytes": sum(c["gran_count"] * 8 for c in chains), "weight_bytes": sum(c["blob_floats"] * 4 + c["C"] * c["R"] * 4 for c in chains)}
    return {"padded": head["padded"], "config": tuple(head[k] for k in "RDSE"), "chains": chains, "info": info}
