"""CPU: the host arithmetic of the kernel_size 3 / 4 inference path (csrc/wn_plan.h: wn_forward_geometry_host with a kernel_size argument;
csrc/wn_banks.h: the k-tap filter/gate bank), compiled with g++ and checked against the module's own torch path and the reference's weight layout.

Geometry.  In absolute time every layer's sequence ends at L; a[l] is the first position of layer l's input.  The module's CPU wavenet() is run with
forward hooks on the filter convs: a conv's input holds (L - a[l]) + pad positions (pad = the left zero padding up to a multiple of the dilation),
its output L - a[l+1].  rows[l] -- the trailing positions the kernels compute -- follow from them: rows[NL] = output_length, rows[l] =
min(rows[l+1] + (k-1) d, L - a[l]).  kernel_size 3 and 4 are served from L = receptive_field + output_length - 1 on, and there no returned position
sees a pad zero (zlo = 0).  Lengths at which the module itself raises (the skip path's un-dilation quirk at a per-row length of 1) must be refused."""
import os
import subprocess

import numpy as np
import pytest
import torch

import wavenet_model

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "pytorch-wavenet_amd", "csrc")

HARNESS = r"""
#include "wn_banks.h"
#include <cstdio>
#include <cstdlib>
int main(int argc, char** argv) {
    if (argc >= 2 && argv[1][0] == 'f') {  // f <layers> <blocks> <L> <out_len> <k | 0: the call without the kernel_size argument>
        const int layers = atoi(argv[2]), blocks = atoi(argv[3]), k = atoi(argv[6]);
        std::vector<int32_t> dil;
        for (int b = 0; b < blocks; ++b) for (int i = 0; i < layers; ++i) dil.push_back(1 << i);
        WnFwdGeom g;
        const std::string why = k ? wn_forward_geometry_host(dil.data(), (int)dil.size(), atoll(argv[4]), atoll(argv[5]), g, k)
                                  : wn_forward_geometry_host(dil.data(), (int)dil.size(), atoll(argv[4]), atoll(argv[5]), g);
        if (!why.empty()) { printf("REFUSED %s\n", why.c_str()); return 0; }
        for (long long v : g.a) printf("%lld ", v); printf("| ");
        for (long long v : g.rows) printf("%lld ", v); printf("| ");
        for (long long v : g.zlo) printf("%lld ", v); printf("\n");
        return 0;
    }
    // b <layers> <blocks> <R> <D> <S> <E> <C> <bias> <k> <in> <out>: the fp32 bank of a k-tap model; stdout: "train_ok fwd_ok total fg bfg res"
    if (argc != 13) return 2;
    const int bias = atoi(argv[9]);
    WnPlan s = {};
    s.layers = atoi(argv[2]); s.blocks = atoi(argv[3]); s.NL = s.layers * s.blocks; s.k = atoi(argv[10]); s.has_bias = bias;
    s.R = atoi(argv[4]); s.D = atoi(argv[5]); s.S = atoi(argv[6]); s.E = atoi(argv[7]); s.C = atoi(argv[8]);
    const size_t NL = s.NL, R = s.R, D = s.D, S = s.S, E = s.E, C = s.C, k = s.k;
    FILE* in = fopen(argv[11], "rb");
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
    printf("%d %d %lld %lld %lld %lld\n", wn_bank_ok(s) ? 1 : 0, wn_bank_fwd_ok(s) ? 1 : 0, (long long)o.total, (long long)o.fg, (long long)o.bfg, (long long)o.res);
    const std::vector<float> fw = wn_pack_bank(o, s, &w);
    FILE* out = fopen(argv[12], "wb");
    if (!out || fwrite(fw.data(), 4, fw.size(), out) != fw.size()) return 6;
    fclose(out);
    return 0;
}
"""


@pytest.fixture(scope="module")
def harness(tmp_path_factory):
    d = tmp_path_factory.mktemp("taps")
    src = d / "taps_harness.cpp"
    src.write_text(HARNESS)
    exe = d / "taps_harness"
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-I", CSRC, str(src), "-o", str(exe)])
    return str(exe)


def geometry(exe, layers, blocks, L, out_len, k):
    out = subprocess.check_output([exe, "f", str(layers), str(blocks), str(L), str(out_len), str(k)]).decode().strip()
    if out.startswith("REFUSED"):
        return out
    return [[int(v) for v in part.split()] for part in out.split("|")]


def module_lengths(layers, blocks, k, L, out_len):
    """(positions of every filter conv's input, of its output) of the module's CPU wavenet() on clips of L samples, or None where it raises"""
    m = wavenet_model.WaveNetModel(layers=layers, blocks=blocks, dilation_channels=2, residual_channels=2, skip_channels=2, end_channels=2, classes=4,
                                   output_length=out_len, kernel_size=k)
    N, seen = 2, []
    hooks = [c.register_forward_hook(lambda mod, inp, out: seen.append((inp[0].shape[0] // N * inp[0].shape[2], out.shape[0] // N * out.shape[2])))
             for c in m.filter_convs]
    x = torch.zeros(N, 4, L)
    x[:, 1, :] = 1.0
    try:
        with torch.no_grad():
            y = m(x)
    except (RuntimeError, AssertionError):
        return None
    finally:
        for h in hooks:
            h.remove()
    assert y.shape == (N * out_len, 4)
    return seen


@pytest.mark.parametrize("out_len", [4, 9])
@pytest.mark.parametrize("layers,blocks", [(3, 2), (4, 1)])
@pytest.mark.parametrize("k", [3, 4])
def test_geometry_equals_the_modules_sequence_lengths(harness, k, layers, blocks, out_len):
    dil = [1 << i for _ in range(blocks) for i in range(layers)]
    NL = len(dil)
    rf = 1 + blocks * (k - 1) * (2 ** layers - 1)
    lo = rf + out_len - 1
    served = 0
    for L in range(lo, lo + 2 * max(dil) + 1):
        g = geometry(harness, layers, blocks, L, out_len, k)
        want = module_lengths(layers, blocks, k, L, out_len)
        if want is None:   # the module itself has no result here
            assert isinstance(g, str) and "un-dilation" in g, (L, g)
            continue
        assert not isinstance(g, str), (L, g)
        a, rows, zlo = g
        assert a[0] == 0 and len(a) == NL + 1 and len(rows) == NL + 1
        for l in range(NL):
            pad = (-(L - a[l])) % dil[l]
            assert want[l] == (L - a[l] + pad, L - a[l + 1]), (L, l, want[l], a)
            assert rows[l] == min(rows[l + 1] + (k - 1) * dil[l], L - a[l]), (L, l)
            assert L - rows[l + 1] - (k - 1) * dil[l] >= a[l], "the oldest tap of the first computed row lies inside the layer's input"
        assert rows[NL] == out_len and zlo == [0] * NL
        served += 1
    assert served >= max(dil), "most lengths of the sweep have a result"
    below = geometry(harness, layers, blocks, lo - 1, out_len, k)
    assert isinstance(below, str) and len(below) > len("REFUSED ") and "receptive_field + output_length - 1" in below


@pytest.mark.parametrize("layers,blocks,out_len", [(3, 2, 4), (4, 1, 1), (5, 2, 16)])
def test_kernel_size_2_is_the_call_without_the_argument(harness, layers, blocks, out_len):
    rf = 1 + blocks * (2 ** layers - 1)
    for L in range(1, rf + out_len + 2 * 2 ** layers):
        assert geometry(harness, layers, blocks, L, out_len, 2) == geometry(harness, layers, blocks, L, out_len, 0), L


@pytest.mark.parametrize("bias", [0, 1])
@pytest.mark.parametrize("k", [3, 4])
def test_tap_j_lands_in_columns_j_R_of_the_layers_wfg(harness, tmp_path, k, bias):
    layers, blocks, R, D, S, E, C = 2, 2, 64, 32, 32, 32, 32
    NL = layers * blocks
    g = torch.Generator().manual_seed(100 * k + bias)
    rnd = lambda *shape: torch.randn(shape, generator=g, dtype=torch.float32)   # noqa: E731
    p = {"start_w": rnd(R, C), "filter_w": rnd(NL, D, R, k), "gate_w": rnd(NL, D, R, k), "res_w": rnd(NL, R, D), "skip_w": rnd(NL, S, D),
         "end1_w": rnd(E, S), "end1_b": rnd(E), "end2_w": rnd(C, E), "end2_b": rnd(C)}
    if bias:
        p.update(start_b=rnd(R), filter_b=rnd(NL, D), gate_b=rnd(NL, D), res_b=rnd(NL, R), skip_b=rnd(NL, S))
    order = ["start_w", "start_b", "filter_w", "gate_w", "filter_b", "gate_b", "res_w", "res_b", "skip_w", "skip_b", "end1_w", "end1_b", "end2_w", "end2_b"]
    with open(tmp_path / "in.bin", "wb") as f:
        for name in order:
            if name in p:
                f.write(p[name].numpy().tobytes())
    out = subprocess.check_output([harness, "b"] + [str(v) for v in (layers, blocks, R, D, S, E, C, bias, k)] + [str(tmp_path / "in.bin"), str(tmp_path / "out.bin")])
    train_ok, fwd_ok, total, fg, bfg, res = [int(v) for v in out.decode().split()]
    assert (train_ok, fwd_ok) == (0, 1), "kernel_size %d: inference only" % k
    assert fg == 0 and bfg == NL * k * R * 2 * D and res == bfg + NL * 2 * D
    bank = np.fromfile(tmp_path / "out.bin", dtype=np.float32)
    assert bank.size == total
    for l in range(NL):
        wfg = bank[fg + l * k * R * 2 * D: fg + (l + 1) * k * R * 2 * D].reshape(k * R, 2 * D).T   # Wfg [2D][k*R]: stored as its transpose
        for ch in range(D):
            nf = 64 * (ch // 32) + ch % 32   # rows [F(32) | G(32)] per group of 32 channels
            for j in range(k):   # tap j (0 = the oldest, conv.weight[:, :, j]) in columns j*R .. (j+1)*R - 1
                assert np.array_equal(wfg[nf, j * R:(j + 1) * R], p["filter_w"][l, ch, :, j].numpy()), (l, ch, j)
                assert np.array_equal(wfg[nf + 32, j * R:(j + 1) * R], p["gate_w"][l, ch, :, j].numpy()), (l, ch, j)
            b = bank[bfg + l * 2 * D: bfg + (l + 1) * 2 * D]
            assert b[nf] == (p["filter_b"][l, ch] if bias else 0.0) and b[nf + 32] == (p["gate_b"][l, ch] if bias else 0.0)
