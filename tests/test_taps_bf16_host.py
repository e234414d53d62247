"""CPU: the host side of the opt-in bf16 inference path of kernel_size 3 / 4 (csrc/wn_banks.h, compiled with g++ as tests/test_banks_host.py does):
the predicate wn_bank_fwd_bf16_ok, the k-tap filter/gate section [NL][2D][k*R] of the bf16 bank -- layout, every element against numpy's
round-to-nearest-even of the reference's conv weights --, the kernel_size 2 bank byte for byte what it was before the section was generalised
(SHA-256 recorded from that code, as tests/test_params_host.py records synth.init_weights), the older predicates unchanged, and the facade's switch."""
import hashlib
import os
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "pytorch-wavenet_amd", "csrc")

# taps_bf16_harness <layers> <blocks> <R> <D> <S> <E> <C> <bias> <k> [<in> <out>]
#   stdout: "bank_ok fwd_ok fwd_bf16_ok" / "ok G fg res skip w1 w2 total";  with in / out: the bf16 bank of the parameters in `in` (the order of ARRAYS) to `out`
HARNESS = r"""
#include "wn_banks.h"
#include <cstdio>
#include <cstdlib>
int main(int argc, char** argv) {
    if (argc != 10 && argc != 12) return 2;
    const int bias = atoi(argv[8]);
    WnPlan s = {};
    s.layers = atoi(argv[1]); s.blocks = atoi(argv[2]); s.NL = s.layers * s.blocks; s.k = atoi(argv[9]); s.has_bias = bias;
    s.R = atoi(argv[3]); s.D = atoi(argv[4]); s.S = atoi(argv[5]); s.E = atoi(argv[6]); s.C = atoi(argv[7]);
    const size_t NL = s.NL, R = s.R, D = s.D, S = s.S, E = s.E, C = s.C, k = s.k;
    printf("%d %d %d\n", wn_bank_ok(s) ? 1 : 0, wn_bank_fwd_ok(s) ? 1 : 0, wn_bank_fwd_bf16_ok(s) ? 1 : 0);
    const WnBf16Layout ob = wn_bank_layout_bf16(s);
    printf("%d %d %zu %zu %zu %zu %zu %zu\n", ob.ok ? 1 : 0, ob.G, ob.fg, ob.res, ob.skip, ob.w1, ob.w2, ob.total);
    if (argc == 10) return 0;
    if (!wn_bank_fwd_bf16_ok(s) || !ob.ok) return 5;
    FILE* in = fopen(argv[10], "rb");
    if (!in) return 3;
    std::vector<std::vector<float>> keep;
    auto take = [&](size_t n) -> const float* {
        keep.emplace_back(n);
        if (fread(keep.back().data(), 4, n, in) != n) exit(4);
        return keep.back().data();
    };
    wn_weight_ptrs w = {};
    w.start_w = take(R * C); if (bias) w.start_b = take(R);
    w.filter_w = take(NL * D * R * k); w.gate_w = take(NL * D * R * k);
    if (bias) { w.filter_b = take(NL * D); w.gate_b = take(NL * D); }
    w.res_w = take(NL * R * D); if (bias) w.res_b = take(NL * R);
    w.skip_w = take(NL * S * D); if (bias) w.skip_b = take(NL * S);
    w.end1_w = take(E * S); w.end1_b = take(E); w.end2_w = take(C * E); w.end2_b = take(C);
    fclose(in);
    const wn_train_layout o = wn_bank_layout(s);
    const std::vector<float> fw = wn_pack_bank(o, s, &w);
    const std::vector<unsigned short> wb = wn_pack_bank_bf16(ob, o, s, fw, &w);
    FILE* out = fopen(argv[11], "wb");
    if (!out || fwrite(wb.data(), 2, wb.size(), out) != wb.size()) return 7;
    fclose(out);
    return 0;
}
"""

ARRAYS = ("start_w", "start_b", "filter_w", "gate_w", "filter_b", "gate_b", "res_w", "res_b", "skip_w", "skip_b", "end1_w", "end1_b", "end2_w", "end2_b")
BIASES = ("start_b", "filter_b", "gate_b", "res_b", "skip_b")
SHAPES = [(3, 2, 64, 64, 64, 64, 256), (3, 2, 64, 128, 128, 64, 256)]   # (layers, blocks, R, D, S, E, C)

# SHA-256 of the kernel_size 2 bf16 bank of weights(shape, bias, 2), packed by the code as it stood before the filter/gate section took the tap count
# from the plan: (shape index, bias) -> digest
K2_SHA256 = {
    (0, 0): "89815017a12edc0cd00de718a78b11934ed001884fdd14e2303d0697055b65a8",
    (0, 1): "2b03a894932f3e2757c1f6eaf61a8960c3affaf244e34b8d44e49304e0a375a4",
    (1, 0): "60d78d70f07ee9b9c4238737ef6caf65e4654b8574554be0dd1f61cda19af753",
    (1, 1): "c0673d006d2394ad9e825f9e295399c2ce2dfada3a57f2ab50490fabd25c304c",
}


@pytest.fixture(scope="module")
def harness(tmp_path_factory):
    d = tmp_path_factory.mktemp("taps_bf16")
    src = d / "taps_bf16_harness.cpp"
    src.write_text(HARNESS)
    exe = d / "taps_bf16_harness"
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-I", CSRC, str(src), "-o", str(exe)])
    return str(exe)


def weights(shape, bias, k):
    """the reference's parameters stacked over the layers (numpy's legacy generator: the same bits everywhere)"""
    layers, blocks, R, D, S, E, C = shape
    NL = layers * blocks
    rs = np.random.RandomState(1000 * R + 100 * D + 10 * k + bias)
    dims = {"start_w": (R, C, 1), "start_b": (R,), "filter_w": (NL, D, R, k), "gate_w": (NL, D, R, k), "filter_b": (NL, D), "gate_b": (NL, D),
            "res_w": (NL, R, D, 1), "res_b": (NL, R), "skip_w": (NL, S, D, 1), "skip_b": (NL, S), "end1_w": (E, S, 1), "end1_b": (E,),
            "end2_w": (C, E, 1), "end2_b": (C,)}
    return {n: rs.standard_normal(dims[n]).astype(np.float32) for n in ARRAYS if bias or n not in BIASES}


def rne_bits(x):
    """fp32 -> the bit pattern of its bf16 round-to-nearest-even (finite inputs)"""
    b = np.ascontiguousarray(x, dtype=np.float32).view(np.uint32).astype(np.uint64)
    return ((b + 0x7FFF + ((b >> 16) & 1)) >> 16).astype(np.uint16)


def run(exe, shape, bias, k, tmp_path=None, p=None):
    args = [exe] + [str(v) for v in shape] + [str(bias), str(k)]
    if p is not None:
        with open(tmp_path / "in.bin", "wb") as f:
            for n in ARRAYS:
                if n in p:
                    f.write(p[n].tobytes())
        args += [str(tmp_path / "in.bin"), str(tmp_path / "out.bin")]
    out = subprocess.check_output(args).decode().splitlines()
    preds = [int(v) for v in out[0].split()]
    lay = [int(v) for v in out[1].split()]
    bank = np.fromfile(tmp_path / "out.bin", dtype=np.uint16) if p is not None else None
    return preds, lay, bank


def old_predicates(shape, k):
    layers, blocks, R, D, S, E, C = shape
    m32 = not any(c % 32 for c in (R, D, S, E, C))
    return [int(k == 2 and m32), int(2 <= k <= 4 and m32)]


@pytest.mark.parametrize("bias", [0, 1])
@pytest.mark.parametrize("si", range(len(SHAPES)))
@pytest.mark.parametrize("k", [2, 3, 4])
def test_bank_of_k_taps(harness, tmp_path, k, si, bias):
    shape = SHAPES[si]
    layers, blocks, R, D, S, E, C = shape
    NL = layers * blocks
    p = weights(shape, bias, k)
    preds, lay, bank = run(harness, shape, bias, k, tmp_path, p)
    assert preds == old_predicates(shape, k) + [1]
    ok, G, fg, res, skip, w1, w2, total = lay
    assert ok == 1 and G == layers
    # ---- layout: the filter/gate section spans NL * 2D * k*R elements, the later sections follow it
    assert fg == 0 and res == NL * 2 * D * k * R and skip == res + NL * R * D and w1 == skip + NL * D * S and w2 == w1 + E * S and total == w2 + C * E
    assert bank.size == total
    # ---- every element of the filter/gate section: row 64 * (ch / 32) + 32 * gate + ch % 32, column tap * R + r
    sec = bank[fg:res].reshape(NL, 2 * D, k, R)
    ch = np.arange(D)
    for gate, name in ((0, "filter_w"), (1, "gate_w")):
        rows = 64 * (ch // 32) + 32 * gate + ch % 32
        want = rne_bits(p[name]).transpose(0, 1, 3, 2)   # [NL][D][R][k] -> [NL][D][k][R]
        assert np.array_equal(sec[:, rows], want), name
    assert sorted(np.concatenate([64 * (ch // 32) + ch % 32, 64 * (ch // 32) + 32 + ch % 32]).tolist()) == list(range(2 * D))   # (every row checked)
    # ---- the sections behind it are what they were: [NL][R][D], [block][S][G*D], [E][S], [C][E]
    assert np.array_equal(bank[res:skip], rne_bits(p["res_w"]).reshape(-1))
    want_skip = rne_bits(p["skip_w"]).reshape(NL // G, G, S, D).transpose(0, 2, 1, 3)
    assert np.array_equal(bank[skip:w1], want_skip.reshape(-1))
    assert np.array_equal(bank[w1:w2], rne_bits(p["end1_w"]).reshape(-1))
    assert np.array_equal(bank[w2:], rne_bits(p["end2_w"]).reshape(-1))
    if k == 2:   # byte for byte the bank of the code before this section was generalised
        assert hashlib.sha256(bank.tobytes()).hexdigest() == K2_SHA256[(si, bias)]


@pytest.mark.parametrize("k,shape,want", [
    (5, (3, 2, 64, 64, 64, 64, 256), 0),
    (1, (3, 2, 64, 64, 64, 64, 256), 0),
    (3, (3, 2, 32, 64, 64, 64, 256), 0),
    (3, (3, 2, 96, 64, 64, 64, 256), 0),
    (4, (3, 2, 64, 96, 64, 64, 256), 0),
    (3, (3, 2, 64, 64, 32, 64, 256), 0),
    (3, (3, 2, 64, 64, 64, 96, 256), 0),
    (3, (3, 2, 64, 64, 64, 64, 48), 0),
    (2, (3, 2, 32, 32, 64, 64, 256), 0),
    (3, (3, 2, 64, 64, 64, 64, 32), 1),
    (2, (3, 2, 128, 128, 512, 256, 256), 1),
], ids=lambda v: "-".join(str(x) for x in v) if isinstance(v, tuple) else str(v))
def test_predicate(harness, k, shape, want):
    preds, _, _ = run(harness, shape, 0, k)
    assert preds[2] == want
    assert preds[:2] == old_predicates(shape, k)   # (wn_bank_ok and wn_bank_fwd_ok answer as before)


def test_switch_is_off_by_default():
    import wavenet_model
    assert wavenet_model.WaveNetModel.native_taps_bf16 is False
    m = wavenet_model.WaveNetModel(layers=2, blocks=1, dilation_channels=64, residual_channels=64, skip_channels=64, end_channels=64, kernel_size=3)
    assert m.native_taps_bf16 is False and "native_taps_bf16" not in m.__dict__
