"""CPU: the host side of the opt-in native training step for kernel_size 3 and 4.

1. mi355_wavenet/training.py: StackLayout(k = 3 | 4) -- unpack(pack(p)) == p bit for bit; the rows of tap j of the filter / gate section hold
   filter_w[..., j] / gate_w[..., j] in the column order [F(32) | G(32)] per 32 channels (restated here with plain loops from include/wn_abi.h:
   wn_train_layout, the formula of csrc/wn_banks.h: wn_pack_bank, which tests/test_banks_host.py holds today's k = 2 pack to); k = 2 gives those bytes.
2. csrc/wn_plan.h (plain C++, compiled with g++): need[] = wn_forward_geometry_host's rows[] for k = 3, 4 and the row windows of the backward's
   input-gradient product (wn_taps_bwd_shift / wn_taps_bwd_src: which row of [dF|dG] view j of an output row reads, or none) against a brute-force
   dependency walk over absolute sample positions, for clip lengths from receptive_field + output_length - 1 on.
3. wavenet_model.py: the switch native_taps_training -- a class attribute, False by default, an instance's value survives pickle, a state without it loads;
   what it gates (which shapes count as natively trainable, train_forward_indices' argument check, the training engine's unpadded shape).
4. The module's torch path on the CPU reproduces the REAL reference's training step for kernel_size 3 / 4 (tests/golden/golden_taps_train_v1.npz, written
   by tests/golden/make_golden_taps_train.py) at the bars of tests/test_gpu_training.py: test_native_gradients_match_the_reference_golden -- the yardstick
   tests/test_gpu_taps_training.py measures the native step with."""
import copy
import os
import pickle
import subprocess
import sys

import numpy as np
import pytest
import torch

import wavenet_model
from mi355_wavenet import _abi, params, synth, training

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "pytorch-wavenet_amd", "csrc")


# ------------------------------------------------------------------------------------------------ 1. StackLayout
def _layout(NL, R, D, S, E, C, bias, k):
    sz = training.StackLayout(NL, R, D, S, E, C, bias, 0, {}, torch.device("cpu"), k=k).sizes()
    off, o = {}, 0
    for name in _abi.TRAIN_SECTIONS:
        off[name] = o
        o += sz[name]
    return training.StackLayout(NL, R, D, S, E, C, bias, o, off, torch.device("cpu"), k=k)


def _params(NL, R, D, S, E, C, bias, k, seed):
    g = torch.Generator().manual_seed(seed)
    cfg = dict(residual_channels=R, dilation_channels=D, skip_channels=S, end_channels=E, classes=C, kernel_size=k)
    out = {}
    for p in params.rows(bias):
        shape = params.shape(p.key, cfg)
        out[p.key] = torch.randn(((NL,) + shape) if p.per_layer else shape, generator=g, dtype=torch.float32)
    return out


def _bits(t):
    return t.contiguous().view(torch.int32).numpy()


@pytest.mark.parametrize("bias", [False, True])
@pytest.mark.parametrize("k", [2, 3, 4])
@pytest.mark.parametrize("shape", [(3, 32, 32, 64, 64, 256), (2, 64, 96, 128, 64, 256)], ids=["32x32", "64x96"])
def test_stack_layout_packs_k_taps(shape, k, bias):
    NL, R, D, S, E, C = shape
    lay = _layout(NL, R, D, S, E, C, bias, k)
    assert lay.sizes()["fg"] == NL * k * R * 2 * D
    p = _params(NL, R, D, S, E, C, bias, k, seed=100 * k + R + int(bias))
    flat = lay.pack(p)
    back = lay.unpack(flat)
    assert set(back) == set(p)
    for key, v in p.items():
        assert np.array_equal(_bits(back[key].reshape(v.shape)), _bits(v)), key
    # the filter / gate section, restated: row tap * R + r of layer l, column 64 (ch // 32) + ch % 32 (+ 32 for the gate)
    fg = flat[lay.off["fg"]:lay.off["fg"] + lay.sizes()["fg"]].reshape(NL, k * R, 2 * D)
    ch = np.arange(D)
    nf = 64 * (ch // 32) + ch % 32
    for tap in range(k):
        rows = fg[:, tap * R:(tap + 1) * R, :]                                  # [NL][R][2D]
        assert np.array_equal(_bits(rows[:, :, nf]), _bits(p["filter_w"][..., tap].transpose(1, 2))), tap
        assert np.array_equal(_bits(rows[:, :, nf + 32]), _bits(p["gate_w"][..., tap].transpose(1, 2))), tap
    if k == 2:   # the bytes of the layout before it took k: the two-tap reshape of the section, written out
        old = torch.stack([p["filter_w"], p["gate_w"]], dim=1).reshape(NL, 2, D // 32, 32, R, 2).permute(0, 5, 4, 2, 1, 3).reshape(-1)
        assert np.array_equal(_bits(flat[lay.off["fg"]:lay.off["fg"] + old.numel()]), _bits(old))
        assert training.StackLayout(NL, R, D, S, E, C, bias, lay.total, lay.off, torch.device("cpu")).sizes() == lay.sizes()   # (k defaults to 2)


# ------------------------------------------------------------------------------------------------ 2. need[] and the backward's row windows
HARNESS = r"""
#include "wn_plan.h"
#include <cstdio>
#include <cstdlib>
int main(int argc, char** argv) {   // <layers> <blocks> <L> <out_len> <k>: "REFUSED ..." or rows[] on one line, then per layer and output row: the k sources
    if (argc != 6) return 2;
    const int layers = atoi(argv[1]), blocks = atoi(argv[2]), k = atoi(argv[5]);
    std::vector<int32_t> dil;
    for (int b = 0; b < blocks; ++b) for (int i = 0; i < layers; ++i) dil.push_back(1 << i);
    WnFwdGeom g;
    const std::string why = wn_forward_geometry_host(dil.data(), (int)dil.size(), atoll(argv[3]), atoll(argv[4]), g, k);
    if (!why.empty()) { printf("REFUSED %s\n", why.c_str()); return 0; }
    for (long long v : g.rows) printf("%lld ", v);
    printf("\n");
    for (size_t l = 0; l < dil.size(); ++l) {
        const long long rows_out = g.rows[l], rows_dfg = g.rows[l + 1], sh = wn_taps_bwd_shift(rows_out, rows_dfg);
        for (long long i = 0; i < rows_out; ++i)
            for (int j = 0; j < k; ++j) printf("%lld ", wn_taps_bwd_src(i, sh, dil[l], k, j, rows_dfg));
        printf("\n");
    }
    return 0;
}
"""


@pytest.fixture(scope="module")
def harness(tmp_path_factory):
    d = tmp_path_factory.mktemp("taps_train")
    src = d / "taps_train_harness.cpp"
    src.write_text(HARNESS)
    exe = d / "taps_train_harness"
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-I", CSRC, str(src), "-o", str(exe)])
    return str(exe)


@pytest.mark.parametrize("out_len", [1, 5])
@pytest.mark.parametrize("layers,blocks", [(3, 2), (4, 1)])
@pytest.mark.parametrize("k", [3, 4])
def test_need_and_backward_windows_against_a_dependency_walk(harness, k, layers, blocks, out_len):
    dil = [1 << i for _ in range(blocks) for i in range(layers)]
    NL = len(dil)
    rf = 1 + blocks * (k - 1) * (2 ** layers - 1)
    lo = rf + out_len - 1
    short = subprocess.check_output([harness, str(layers), str(blocks), str(lo - 1), str(out_len), str(k)]).decode()
    assert short.startswith("REFUSED"), "one sample short of receptive_field + output_length - 1 is not served"
    served = 0
    for L in range(lo, lo + 2 * max(dil) + 2):
        out = subprocess.check_output([harness, str(layers), str(blocks), str(L), str(out_len), str(k)]).decode().splitlines()
        if out[0].startswith("REFUSED"):   # (a length at which the reference itself has no defined result, e.g. the un-dilation quirk at output_length 1)
            assert "zero-padding regime" not in out[0], (L, out[0])
            continue
        served += 1
        rows = [int(v) for v in out[0].split()]
        # the walk: the sample positions of every layer's input the returned outputs depend on
        need = [None] * (NL + 1)
        need[NL] = set(range(L - out_len, L))
        for l in range(NL - 1, -1, -1):
            need[l] = {t - m * dil[l] for t in need[l + 1] for m in range(k)}
            assert min(need[l]) >= 0, "a tap before the clip's start"
        for l in range(NL + 1):   # need[l] trailing positions: the hull of the dependency set (at output_length 1 the set itself is a comb), and tight
            assert min(need[l]) == L - rows[l] and max(need[l]) == L - 1, (L, l)
            need[l] = set(range(L - rows[l], L))   # what the step computes, and what the gradient therefore flows through
        for l in range(NL):
            d, rows_out, rows_dfg = dil[l], rows[l], rows[l + 1]
            # which (tap, output position of the layer) pairs feed the gradient of input position t: tap j of output t' reads x(t' - (k-1-j) d)
            feeds = {t: set() for t in need[l]}
            for t2 in need[l + 1]:
                for j in range(k):
                    feeds[t2 - (k - 1 - j) * d].add((j, t2))
            src = [int(v) for v in out[1 + l].split()]
            assert len(src) == rows_out * k
            for i in range(rows_out):
                t = L - rows_out + i
                got = {(j, L - rows_dfg + src[i * k + j]) for j in range(k) if src[i * k + j] >= 0}
                assert all(-1 <= s < rows_dfg for s in src[i * k:(i + 1) * k])
                assert got == feeds[t], (L, l, i)
    assert served >= max(dil) + 1, "at least every second length from receptive_field + output_length - 1 on is served"


# ------------------------------------------------------------------------------------------------ 3. the facade's switch
def _model(k, ch=(32, 32, 64, 64), classes=256):
    return wavenet_model.WaveNetModel(layers=2, blocks=1, residual_channels=ch[0], dilation_channels=ch[1], skip_channels=ch[2], end_channels=ch[3],
                                      classes=classes, output_length=4, kernel_size=k)


def test_the_switch_is_a_class_attribute_off_by_default_and_travels_with_a_pickle():
    assert wavenet_model.WaveNetModel.native_taps_training is False
    m = _model(3)
    assert m.native_taps_training is False and "native_taps_training" not in m.__dict__
    assert "native_taps_training" not in pickle.loads(pickle.dumps(m)).__dict__          # off: nothing new in a snapshot
    m.native_taps_training = True
    m2 = pickle.loads(pickle.dumps(m))
    assert m2.native_taps_training is True and wavenet_model.WaveNetModel.native_taps_training is False
    # a state without it (a snapshot written before the switch existed; the reference's own pickles) loads, switched off
    state = m.__getstate__()
    state.pop("native_taps_training")
    m3 = wavenet_model.WaveNetModel.__new__(wavenet_model.WaveNetModel)
    m3.__setstate__(state)
    assert m3.native_taps_training is False
    assert torch.equal(m3.start_conv.weight, m.start_conv.weight)
    m4 = copy.deepcopy(m)
    assert m4.native_taps_training is True


def test_what_the_switch_gates():
    idx = torch.zeros(2, 40, dtype=torch.int32)
    for k in (3, 4):
        m = _model(k)
        assert not m._native_taps_trainable() and not m._native_trainable()
        with pytest.raises(ValueError, match="kernel_size 2"):
            m._checked_indices(idx, True, training=True)
        m.native_taps_training = True
        assert m._native_taps_trainable()
        assert m._checked_indices(idx, True, training=True) is not None
        cfg, shape = m._padded_train_config()
        assert shape is None and cfg == m._config()                   # the model's own shape: no zero padding for kernel_size != 2
        odd = _model(k, ch=(48, 40, 80, 72))
        odd.native_taps_training = True
        assert not odd._native_taps_trainable()
        with pytest.raises(ValueError):
            odd._checked_indices(idx, True, training=True)
        odd_classes = _model(k, classes=200)
        odd_classes.native_taps_training = True
        assert not odd_classes._native_taps_trainable()
    for k in (2, 5):   # the switch says nothing about kernel_size 2 (native as before) or 5 (the torch path)
        m = _model(k)
        m.native_taps_training = True
        assert not m._native_taps_trainable()
        assert m._native_trainable() == (k == 2)


# ------------------------------------------------------------------------------------------------ 4. the torch path against the reference's golden step
@pytest.mark.parametrize("case", ["taps_train_k3", "taps_train_k4"])
def test_the_torch_path_reproduces_the_reference_golden_step(case):
    sys.path.insert(0, os.path.join(ROOT, "tests", "golden"))
    import digest as dg
    z = np.load(os.path.join(ROOT, "tests", "golden", "golden_taps_train_v1.npz"))
    wseed, N, out_len, L, rf, k, bias = [int(v) for v in z["grad_%s_meta" % case]]
    cfg = dict(layers=3, blocks=2, dilation_channels=32, residual_channels=32, skip_channels=64, end_channels=64, classes=256, kernel_size=k, bias=bool(bias))
    m = wavenet_model.WaveNetModel(output_length=out_len, **cfg)
    m.load_state_dict({key: torch.from_numpy(v) for key, v in synth.init_weights(cfg, seed=wseed).items()})
    assert m.receptive_field == rf and L >= rf + out_len - 1
    ids = torch.from_numpy(z["grad_%s_ids" % case].astype(np.int64))
    x = torch.zeros(N, 256, L).scatter_(1, ids.view(N, 1, L), 1.0)
    out = m(x)
    loss = torch.nn.functional.cross_entropy(out, torch.from_numpy(z["grad_%s_target" % case].astype(np.int64)))
    loss.backward()
    assert float(np.abs(out.detach().numpy() - z["grad_%s_out" % case]).max()) <= 1e-4
    assert abs(float(loss.detach()) - float(z["grad_%s_loss" % case][0])) <= 1e-5 * max(1.0, abs(float(loss.detach())))
    got = dg.digest({key: (p.grad.numpy() if p.grad is not None else np.zeros(tuple(p.shape), np.float32)) for key, p in m.named_parameters()})
    dg.compare({key: z["grad_%s_d_%s" % (case, key)] for key in got}, got, 2e-5)
    assert m.residual_convs[-1].weight.grad is None
