"""CPU: layout and packing of the GEMM-ready weight banks (csrc/wn_banks.h, plain C++) compiled with g++ and checked through a small
harness against the torch restatement of the same layout (mi355_wavenet/training.py: StackLayout.sizes / StackLayout.pack):
the offsets are the running sum of the section sizes, the fp32 bank equals the Python pack bit for bit (both are pure copies; bskip_total,
the one computed section, is the fp32 sum of the skip biases taken in layer order), the bf16 bank equals torch's round-to-nearest-even
bfloat16 of the transposed / block-grouped fp32 sections bit for bit."""
import os
import subprocess

import numpy as np
import pytest
import torch

from mi355_wavenet import _abi, training

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "pytorch-wavenet_amd", "csrc")

# banks_harness <layers> <blocks> <R> <D> <S> <E> <C> <bias> <in> <out>
#   in:  the reference's parameters as fp32, stacked over the layers, in the order of ARRAYS below (bias arrays only with bias = 1)
#   stdout: "total fg bfg ... start_b" / "ok G fg res skip w1 w2 total";  out: the fp32 bank, then (ok = 1) the bf16 bank
HARNESS = r"""
#include "wn_banks.h"
#include <cstdio>
#include <cstdlib>
int main(int argc, char** argv) {
    if (argc != 11) return 2;
    const int layers = atoi(argv[1]), blocks = atoi(argv[2]), bias = atoi(argv[8]);
    WnPlan s = {};
    s.layers = layers; s.blocks = blocks; s.NL = layers * blocks; s.k = 2; s.has_bias = bias;
    s.R = atoi(argv[3]); s.D = atoi(argv[4]); s.S = atoi(argv[5]); s.E = atoi(argv[6]); s.C = atoi(argv[7]);
    const size_t NL = s.NL, R = s.R, D = s.D, S = s.S, E = s.E, C = s.C;
    FILE* in = fopen(argv[9], "rb");
    if (!in) return 3;
    std::vector<std::vector<float>> keep;
    auto take = [&](size_t n) -> const float* {
        keep.emplace_back(n);
        if (fread(keep.back().data(), 4, n, in) != n) exit(4);
        return keep.back().data();
    };
    wn_weight_ptrs w = {};
    w.start_w = take(R * C); if (bias) w.start_b = take(R);
    w.filter_w = take(NL * D * R * 2); w.gate_w = take(NL * D * R * 2);
    if (bias) { w.filter_b = take(NL * D); w.gate_b = take(NL * D); }
    w.res_w = take(NL * R * D); if (bias) w.res_b = take(NL * R);
    w.skip_w = take(NL * S * D); if (bias) w.skip_b = take(NL * S);
    w.end1_w = take(E * S); w.end1_b = take(E); w.end2_w = take(C * E); w.end2_b = take(C);
    fclose(in);
    if (!wn_bank_ok(s)) return 5;
    const wn_train_layout o = wn_bank_layout(s);
    printf("%lld %lld %lld %lld %lld %lld %lld %lld %lld %lld %lld %lld %lld %lld\n", (long long)o.total, (long long)o.fg, (long long)o.bfg, (long long)o.res,
           (long long)o.bres, (long long)o.skip, (long long)o.bskip, (long long)o.bskip_total, (long long)o.w1, (long long)o.b1, (long long)o.w2, (long long)o.b2,
           (long long)o.start_t, (long long)o.start_b);
    const WnBf16Layout ob = wn_bank_layout_bf16(s);
    printf("%d %d %zu %zu %zu %zu %zu %zu\n", ob.ok ? 1 : 0, ob.G, ob.fg, ob.res, ob.skip, ob.w1, ob.w2, ob.total);
    const std::vector<float> fw = wn_pack_bank(o, s, &w);
    FILE* out = fopen(argv[10], "wb");
    if (!out || fwrite(fw.data(), 4, fw.size(), out) != fw.size()) return 6;
    if (ob.ok) {
        const std::vector<unsigned short> wb = wn_pack_bank_bf16(ob, o, s, fw, &w);
        if (fwrite(wb.data(), 2, wb.size(), out) != wb.size()) return 7;
    }
    fclose(out);
    return 0;
}
"""

ARRAYS = ("start_w", "start_b", "filter_w", "gate_w", "filter_b", "gate_b", "res_w", "res_b", "skip_w", "skip_b", "end1_w", "end1_b", "end2_w", "end2_b")
BIASES = ("start_b", "filter_b", "gate_b", "res_b", "skip_b")
SHAPES = [(3, 2, 32, 32, 64, 64, 256), (3, 2, 128, 128, 512, 256, 256), (2, 3, 64, 64, 128, 64, 256)]


@pytest.fixture(scope="module")
def harness(tmp_path_factory):
    d = tmp_path_factory.mktemp("banks")
    src = d / "banks_harness.cpp"
    src.write_text(HARNESS)
    exe = d / "banks_harness"
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-I", CSRC, str(src), "-o", str(exe)])
    return str(exe)


def weights(shape, bias, seed):
    layers, blocks, R, D, S, E, C = shape
    NL = layers * blocks
    g = torch.Generator().manual_seed(seed)
    dims = {"start_w": (R, C, 1), "start_b": (R,), "filter_w": (NL, D, R, 2), "gate_w": (NL, D, R, 2), "filter_b": (NL, D), "gate_b": (NL, D),
            "res_w": (NL, R, D, 1), "res_b": (NL, R), "skip_w": (NL, S, D, 1), "skip_b": (NL, S), "end1_w": (E, S, 1), "end1_b": (E,),
            "end2_w": (C, E, 1), "end2_b": (C,)}
    return {k: torch.randn(dims[k], generator=g, dtype=torch.float32) for k in ARRAYS if bias or k not in BIASES}


def runner(shape, bias, total, off):
    """The engine-free half of a StackRunner: pack() and sizes() only need the shape, the layout and a device."""
    layers, blocks, R, D, S, E, C = shape
    return training.StackLayout(layers * blocks, R, D, S, E, C, bias, total, off, torch.device("cpu"))


def bits(t):
    return t.contiguous().view(torch.int32 if t.dtype == torch.float32 else torch.int16).numpy()


@pytest.mark.parametrize("bias", [0, 1])
@pytest.mark.parametrize("shape", SHAPES)
def test_banks_equal_the_python_pack(harness, tmp_path, shape, bias):
    layers, blocks, R, D, S, E, C = shape
    NL = layers * blocks
    p = weights(shape, bias, seed=1000 * R + 10 * layers + bias)
    with open(tmp_path / "in.bin", "wb") as f:
        for k in ARRAYS:
            if k in p:
                f.write(p[k].numpy().tobytes())
    out = subprocess.check_output([harness] + [str(v) for v in shape] + [str(bias), str(tmp_path / "in.bin"), str(tmp_path / "out.bin")]).decode().splitlines()
    lay = [int(v) for v in out[0].split()]
    total, off = lay[0], dict(zip(_abi.TRAIN_SECTIONS, lay[1:]))
    run = runner(shape, bias, total, off)
    # ---- offsets: the running sum of the section sizes, in the order of the ABI struct
    sz, o = run.sizes(), 0
    for name in _abi.TRAIN_SECTIONS:
        assert off[name] == o, name
        o += sz[name]
    assert total == o
    # ---- fp32 bank
    raw = np.fromfile(tmp_path / "out.bin", dtype=np.uint8)
    got = torch.from_numpy(raw[:total * 4].view(np.float32).copy())
    want = run.pack(p)
    if bias:   # the one computed section (the Python pack leaves it zero): the skip biases added up in layer order, in fp32
        acc = torch.zeros(S, dtype=torch.float32)
        for l in range(NL):
            acc = acc + p["skip_b"][l]
        want[off["bskip_total"]:off["bskip_total"] + S] = acc
    else:
        for name in ("bfg", "bres", "bskip", "bskip_total", "start_b"):
            assert not got[off[name]:off[name] + sz[name]].any(), name
    assert np.array_equal(bits(got), bits(want))
    # ---- bf16 bank
    ok, G, *ob = [int(v) for v in out[1].split()]
    assert G == min(layers, NL)
    assert bool(ok) == (R % 64 == 0 and D % 64 == 0 and S % 64 == 0 and E % 64 == 0 and NL % G == 0)
    if not ok:
        assert raw.size == total * 4
        return
    sec = lambda name: want[off[name]:off[name] + sz[name]]   # noqa: E731
    parts = [sec("fg").reshape(NL, 2 * R, 2 * D).transpose(1, 2),                                          # [NL][2D][2R]
             sec("res").reshape(NL, D, R).transpose(1, 2),                                                 # [NL][R][D]
             sec("skip").reshape(NL // G, G, D, S).permute(0, 3, 1, 2),                                    # [block][S][G*D]
             sec("w1").reshape(S, E).t(), sec("w2").reshape(E, C).t()]                                     # [E][S], [C][E]
    o = 0
    for start, part in zip(ob[:5], parts):
        assert start == o
        o += part.numel()
    assert ob[5] == o and raw.size == total * 4 + o * 2
    got16 = raw[total * 4:].view(np.int16)
    want16 = np.concatenate([bits(part.contiguous().bfloat16()).reshape(-1) for part in parts])
    assert np.array_equal(got16, want16)
