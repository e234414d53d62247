"""-m gpu: the opt-in native training step for kernel_size 3 and 4 (WaveNetModel.native_taps_training = True), end to end through the facade:
wn_train_forward (wn_fwd_gemm_taps with the gates saved) and wn_train_backward (wn_bwd_gemm_taps for dx, one single-view wn_bwd_gemm_tn per tap for
dWfg) behind model(x) / loss.backward().

Reference of the step: the module's OWN torch path on the CPU in float64 (tests/test_gpu_taps.py: _logits64) plus torch autograd; it shares nothing
with the kernels.  Models as in the existing training tests: seeded default init with every parameter multiplied by 3.0.  Bars, those of
tests/test_gpu_training.py: logits atol = rtol = 1e-4, loss 1e-5 max(1, |loss|), every gradient 2e-5 of its largest element + 1e-9.  The reference's own
fp32 path sits within 1.8e-6 (gradients, of scale), 6e-6 (logits) and 1.6e-6 (loss) of its float64 evaluation for these models and inputs, so the bars
carry a margin of about 10 / 10 / 6 for the difference between the two fp32 evaluations.

Also: the native pack / unpack against StackLayout, the REAL reference's step (tests/golden/golden_taps_train_v1.npz), deterministic gradients, five Adam
steps, the unchanged default, forward() without autograd, what stays refused with the switch on, and the C ABI's answers."""
import copy
import ctypes
import itertools
import os
import sys
import warnings

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import wavenet_model
from mi355_wavenet import _abi, engine, params, synth, training

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SMALL, WIDE = (32, 32, 64, 64), (64, 96, 128, 64)   # residual / dilation / skip / end channels


def _model(k, ch=SMALL, bias=False, layers=3, blocks=2, out_len=16, seed=0, gain=3.0, opt_in=True):
    torch.manual_seed(seed)
    m = wavenet_model.WaveNetModel(layers=layers, blocks=blocks, residual_channels=ch[0], dilation_channels=ch[1], skip_channels=ch[2], end_channels=ch[3],
                                   classes=256, output_length=out_len, kernel_size=k, bias=bias)
    with torch.no_grad():
        for p in m.parameters():
            p.mul_(gain)
    if opt_in:
        m.native_taps_training = True
    return m


def _batch(m, n, extra, seed=1):
    g = torch.Generator().manual_seed(seed)
    L = m.receptive_field + m.output_length - 1 + extra
    idx = torch.randint(0, 256, (n, L), generator=g)
    target = torch.randint(0, 256, (n * m.output_length,), generator=g)
    return idx, target


def _one_hot(idx, dtype=torch.float32):
    return torch.zeros(idx.size(0), 256, idx.size(1), dtype=dtype).scatter_(1, idx.unsqueeze(1), 1.0)


def _step64(m, idx, target):
    """(logits, loss, gradients) of the module's torch path on the CPU in float64"""
    m64 = copy.deepcopy(m).cpu().double()
    m64.dtype = torch.DoubleTensor
    m64.zero_grad(set_to_none=True)
    out = m64(_one_hot(idx, torch.float64))
    loss = F.cross_entropy(out, target)
    loss.backward()
    return out.detach().numpy(), float(loss.detach()), {k: (None if p.grad is None else p.grad.numpy().copy()) for k, p in m64.named_parameters()}


def _native_step(m, x, target):
    """one native step of a CUDA model: the training engine ran, nothing fell back to torch"""
    m.zero_grad(set_to_none=True)
    before, fb = m._wn_train_calls, dict(m._wn_fallbacks)
    out = m(x)
    loss = F.cross_entropy(out, target)
    loss.backward()
    assert m._wn_train_calls == before + 1 and m._wn_fallbacks == fb, m.wn_stats()
    return out.detach().cpu().numpy(), float(loss.detach()), {k: (None if p.grad is None else p.grad.detach().cpu().numpy().copy()) for k, p in m.named_parameters()}


def _check_step(ref, got, label):
    out_r, loss_r, g_r = ref
    out_n, loss_n, g_n = got
    dev = float(np.abs(out_n - out_r).max())
    worst = 0.0
    assert out_n.shape == out_r.shape and out_n.dtype == np.float32
    assert np.allclose(out_n, out_r, atol=1e-4, rtol=1e-4), (label, dev)
    assert abs(loss_n - loss_r) <= 1e-5 * max(1.0, abs(loss_r)), (label, loss_n, loss_r)
    assert set(g_n) == set(g_r)
    for k in g_r:
        if g_r[k] is None:
            assert g_n[k] is None, k   # the last residual conv never reaches the loss (also upstream)
            continue
        assert g_n[k] is not None and g_n[k].shape == g_r[k].shape, k
        scale = float(np.abs(g_r[k]).max())
        err = float(np.abs(g_n[k] - g_r[k]).max())
        worst = max(worst, err / max(scale, 1e-30))
        assert err <= 2e-5 * scale + 1e-9, (label, k, err, scale)
    print("[%s] max |dlogit| %.3g (|logits| %.3g)  |dloss| %.3g  worst gradient deviation %.3g of scale" % (
        label, dev, float(np.abs(out_r).max()), abs(loss_n - loss_r), worst))


# ------------------------------------------------------------------------------------------------ the step against float64
_MODELS = {}


def _cuda_model(k, ch, bias):
    """one model (and one training engine) per (kernel_size, channels, bias): the cases on it differ in their batches"""
    key = (k, ch, bias)
    if key not in _MODELS:
        m = _model(k, ch=ch, bias=bias, seed=10 * k + int(bias))
        _MODELS[key] = (copy.deepcopy(m), m.cuda())
    return _MODELS[key]


STEP_CASES = list(itertools.product((3, 4), (SMALL, WIDE), (False, True), (1, 2, 3), (0, 5)))


@pytest.mark.parametrize("k,ch,bias,n,extra", STEP_CASES, ids=["k%d-%s-b%d-N%d-L+%d" % (c[0], "x".join(map(str, c[1])), c[2], c[3], c[4]) for c in STEP_CASES])
def test_step_matches_float64_autograd(k, ch, bias, n, extra):
    master, m = _cuda_model(k, ch, bias)
    idx, target = _batch(m, n, extra, seed=100 * n + extra + k)
    ref = _step64(master, idx, target)
    got = _native_step(m, _one_hot(idx).cuda(), target.cuda())
    _check_step(ref, got, "k%d %s bias %d N %d L rf+15+%d" % (k, ch, bias, n, extra))
    assert m.residual_convs[-1].weight.grad is None


def test_step_at_four_by_two_layers_and_wider_channels():
    """4 x 2 layers (dilations up to 8), 128 / 128 / 256 / 128 channels, gain 1.5: K = 3 * 256 in the dx product, full 128-column tiles, R % 128 == 0"""
    m = _model(3, ch=(128, 128, 256, 128), bias=True, layers=4, blocks=2, seed=5, gain=1.5)
    idx, target = _batch(m, 2, 0, seed=6)
    ref = _step64(m, idx, target)
    m = m.cuda()
    _check_step(ref, _native_step(m, _one_hot(idx).cuda(), target.cuda()), "4x2 128/128/256/128")
    assert m.residual_convs[-1].weight.grad is None


# ------------------------------------------------------------------------------------------------ 1. native pack / unpack against torch
@pytest.mark.parametrize("bias", [False, True])
@pytest.mark.parametrize("k", [3, 4])
def test_native_pack_and_unpack_equal_the_torch_layout(k, bias):
    m = _model(k, ch=WIDE, bias=bias).cuda()
    eng = engine.Engine(m._config(), dict(m.state_dict()), n_streams=1, device_index=0, pad_channels=False)
    r = training.StackRunner(eng)
    NL = m.layers * m.blocks
    assert r.k == k and r.sizes()["fg"] == NL * k * 64 * 2 * 96
    p = {key: (ts[0].detach() if key in training.SINGLE_KEYS else torch.stack([t.detach() for t in ts])) for key, ts in params.from_module(m).items()}
    flat = r.pack(p)
    ref = r.export_params()   # what wn_load_weights packed on the host (csrc/wn_banks.h)
    torch.cuda.synchronize()
    o, s = r.off, r.sizes()
    ref[o["bskip_total"]:o["bskip_total"] + s["bskip_total"]] = 0   # derived scratch section
    assert torch.equal(flat, ref)
    by_key = {key: ([v.contiguous()] if key in training.SINGLE_KEYS else [t.contiguous() for t in v.unbind(0)]) for key, v in p.items()}
    nflat = r.pack_native(by_key)
    torch.cuda.synchronize()
    assert torch.equal(nflat, flat)
    gback = r.unpack_native(flat, by_key)
    want = r.unpack(flat)
    torch.cuda.synchronize()
    for key, ts in by_key.items():
        for i, t in enumerate(ts):
            if key in ("res_w", "res_b") and i == NL - 1:
                assert gback[key][i] is None
            else:
                assert torch.equal(gback[key][i], t), (key, i)
                assert torch.equal(gback[key][i], (want[key] if key in training.SINGLE_KEYS else want[key][i]).reshape(t.shape)), (key, i)
    eng.close()


# ------------------------------------------------------------------------------------------------ 2. the real reference's step
@pytest.mark.parametrize("case", ["taps_train_k3", "taps_train_k4"])
def test_native_step_reproduces_the_reference_golden(case):
    """tests/golden/golden_taps_train_v1.npz (tests/golden/make_golden_taps_train.py: the imported reference) at the bars of
    tests/test_gpu_training.py: test_native_gradients_match_the_reference_golden"""
    sys.path.insert(0, os.path.join(ROOT, "tests", "golden"))
    import digest as dg
    z = np.load(os.path.join(ROOT, "tests", "golden", "golden_taps_train_v1.npz"))
    wseed, N, out_len, L, rf, k, bias = [int(v) for v in z["grad_%s_meta" % case]]
    cfg = dict(layers=3, blocks=2, dilation_channels=32, residual_channels=32, skip_channels=64, end_channels=64, classes=256, kernel_size=k, bias=bool(bias))
    m = wavenet_model.WaveNetModel(output_length=out_len, **cfg)
    m.load_state_dict({key: torch.from_numpy(v) for key, v in synth.init_weights(cfg, seed=wseed).items()})
    m.native_taps_training = True
    m = m.cuda()
    ids = torch.from_numpy(z["grad_%s_ids" % case].astype(np.int64))
    target = torch.from_numpy(z["grad_%s_target" % case].astype(np.int64)).cuda()
    out_n, loss_n, g_n = _native_step(m, _one_hot(ids).cuda(), target)
    assert float(np.abs(out_n - z["grad_%s_out" % case]).max()) <= 1e-4
    assert abs(loss_n - float(z["grad_%s_loss" % case][0])) <= 1e-5 * max(1.0, abs(loss_n))
    shapes = {key: tuple(p.shape) for key, p in m.named_parameters()}
    got = dg.digest({key: (v if v is not None else np.zeros(shapes[key], np.float32)) for key, v in g_n.items()})
    print(case, "worst gradient digest deviation vs the reference", dg.compare({key: z["grad_%s_d_%s" % (case, key)] for key in got}, got, 2e-5))


# ------------------------------------------------------------------------------------------------ 3. deterministic gradients
@pytest.mark.parametrize("k", [3, 4])
def test_deterministic_gradients_are_bit_equal_and_the_atomic_mode_agrees(k):
    m = _model(k, ch=WIDE, bias=True, seed=4).cuda()
    idx, target = _batch(m, 3, 5, seed=9)
    x, target = _one_hot(idx).cuda(), target.cuda()
    m.deterministic_gradients = True
    a = _native_step(m, x, target)
    b = _native_step(m, x, target)
    assert np.array_equal(a[0], b[0]) and a[1] == b[1]
    for key in a[2]:
        assert (a[2][key] is None) == (b[2][key] is None)
        if a[2][key] is not None:
            assert np.array_equal(a[2][key], b[2][key]), key
    m.deterministic_gradients = False
    c = _native_step(m, x, target)
    assert np.array_equal(a[0], c[0])
    for key, g in a[2].items():
        if g is not None:
            scale = float(np.abs(g).max())
            assert float(np.abs(c[2][key] - g).max()) <= 2e-5 * scale + 1e-9, key


# ------------------------------------------------------------------------------------------------ 4. Adam
def test_a_few_adam_steps_follow_the_torch_trajectory():
    """the criterion of tests/test_gpu_training.py: test_a_few_adam_steps_follow_the_torch_trajectory, kernel_size 3"""
    losses = {}
    for torch_path in (True, False):
        m = _model(3, bias=True, seed=3).cuda()
        opt = torch.optim.Adam(m.parameters(), lr=1e-3)
        idx, target = _batch(m, 2, 0, seed=5)
        x, target = _one_hot(idx).cuda(), target.cuda()
        ls = []
        for _ in range(5):
            if torch_path:
                os.environ["WN_TORCH_BACKWARD"] = "1"
            try:
                opt.zero_grad()
                with warnings.catch_warnings():
                    warnings.simplefilter("ignore", RuntimeWarning)   # (the torch path announces itself)
                    loss = F.cross_entropy(m(x), target)
                loss.backward()
                torch.nn.utils.clip_grad_norm_(m.parameters(), 10.0)
                opt.step()
            finally:
                os.environ.pop("WN_TORCH_BACKWARD", None)
            ls.append(float(loss))
        assert (m._wn_train_calls == 5) == (not torch_path)
        losses[torch_path] = ls
    assert losses[False][-1] < losses[False][0]
    assert np.allclose(losses[True], losses[False], rtol=2e-3), losses


# ------------------------------------------------------------------------------------------------ 5. the default
def test_without_the_switch_everything_is_as_before():
    m = _model(3, opt_in=False).cuda()
    idx, target = _batch(m, 2, 0)
    x = _one_hot(idx).cuda()
    with warnings.catch_warnings(record=True) as said:
        warnings.simplefilter("always")
        for _ in range(2):
            m.zero_grad(set_to_none=True)
            F.cross_entropy(m(x), target.cuda()).backward()
    said = [str(w.message) for w in said if issubclass(w.category, RuntimeWarning)]
    assert len(said) == 1 and "kernel_size 3" in said[0], said
    assert m._wn_train_calls == 0 and m.start_conv.weight.grad is not None
    assert m.wn_stats()["torch_fallbacks"] == {"kernel_size 3 (the matrix-core kernels are written for 2)": 2}
    with pytest.raises(ValueError, match="kernel_size 2"):
        m.train_forward_indices(idx)


# ------------------------------------------------------------------------------------------------ 6. opted in, no autograd
@pytest.mark.parametrize("k", [3, 4])
def test_forward_without_autograd_runs_wn_forward(k):
    m = _model(k, bias=True).cuda()
    idx, _ = _batch(m, 2, 5)
    x = _one_hot(idx).cuda()
    with torch.no_grad():
        y = m(x)
    st = m.wn_stats()
    assert st["native_forward"] == 1 and st["native_train_forward"] == 0 and not st["torch_fallbacks"]
    assert torch.equal(y, m.forward_indices(idx))
    # and the differentiable index-based forward is accepted: the training engine's logits, the same products
    yt = m.train_forward_indices(idx)
    assert yt.requires_grad and m.wn_stats()["native_train_forward"] == 1
    assert torch.allclose(yt.detach(), y, atol=1e-4, rtol=1e-4)


# ------------------------------------------------------------------------------------------------ 7. opted in: what stays on the torch path
def test_short_clips_bf16_and_odd_channels_with_the_switch_on():
    m = _model(3, ch=(64, 64, 64, 64)).cuda()
    short = m.receptive_field + m.output_length - 2   # one sample short: the reference's zero-padding regime
    g = torch.Generator().manual_seed(2)
    idx = torch.randint(0, 256, (2, short), generator=g)
    with warnings.catch_warnings():
        warnings.simplefilter("error", RuntimeWarning)   # counted, not warned: a refusal of ONE call
        out = m(_one_hot(idx).cuda())
        out.sum().backward()
    fb = m.wn_stats()["torch_fallbacks"]
    assert len(fb) == 1 and list(fb.values()) == [1] and "the engine refused this call" in list(fb)[0], fb
    ref = copy.deepcopy(m).cpu()
    ref.native_taps_training = False
    with torch.no_grad():
        want = ref(_one_hot(idx))
    assert out.shape == want.shape and torch.allclose(out.detach().cpu(), want, atol=1e-4, rtol=1e-4)
    assert m.start_conv.weight.grad is not None
    # bf16 operands are not served for kernel_size != 2: the step runs, in fp32, bit for bit
    idx, target = _batch(m, 2, 0, seed=3)
    x, target = _one_hot(idx).cuda(), target.cuda()
    m.deterministic_gradients = True
    a = _native_step(m, x, target)
    m.matrix_precision = "bf16"
    b = _native_step(m, x, target)
    m.matrix_precision = "fp32"
    assert np.array_equal(a[0], b[0]) and all(np.array_equal(a[2][key], b[2][key]) for key in a[2] if a[2][key] is not None)
    # channel counts that are no multiples of 32: the torch path, with a reason of its own (no zero padding for kernel_size != 2)
    odd = _model(3, ch=(40, 48, 80, 72)).cuda()
    idx, target = _batch(odd, 1, 0)
    with pytest.warns(RuntimeWarning, match="not multiples of 32"):
        F.cross_entropy(odd(_one_hot(idx).cuda()), target.cuda()).backward()
    assert odd._wn_train_calls == 0 and odd.start_conv.weight.grad is not None
    assert list(odd.wn_stats()["torch_fallbacks"]) == ["kernel_size 3 with channel counts or classes that are not multiples of 32 (no zero padding for kernel_size != 2)"]


# ------------------------------------------------------------------------------------------------ 8. the C ABI
def test_training_abi_on_a_kernel_size_3_handle():
    m = _model(3, ch=WIDE, bias=True)
    eng = engine.Engine(m._config(), dict(m.state_dict()), n_streams=1, device_index=0, pad_channels=False)
    d = eng.lib.dll
    NL, R, D = 6, 64, 96
    lay = _abi.wn_train_layout()
    assert d.wn_train_get_layout(eng._h, ctypes.byref(lay)) == 0
    assert lay.fg == 0 and lay.bfg - lay.fg == NL * 3 * R * 2 * D
    r = training.StackRunner(eng)
    flat = r.export_params()
    assert lay.total == flat.numel()
    grads = torch.empty_like(flat)
    out_len = m.output_length
    dl = torch.zeros(out_len, 256, device="cuda")
    assert d.wn_train_backward(eng._h, flat.data_ptr(), dl.data_ptr(), grads.data_ptr(), None) == _abi.WN_E_STATE
    assert b"wn_train_forward" in d.wn_last_error()
    short = m.receptive_field + out_len - 2
    idx = torch.zeros(1, short, dtype=torch.int32, device="cuda")
    out = torch.full((out_len * 256 + 512,), float("nan"), device="cuda")
    assert d.wn_train_forward(eng._h, flat.data_ptr(), idx.data_ptr(), 1, short, out_len, out.data_ptr() + 4 * 256, None) == _abi.WN_E_UNSUPPORTED
    assert b"kernel_size 3" in d.wn_last_error() and b"zero-padding" in d.wn_last_error()
    torch.cuda.synchronize()
    assert bool(torch.isnan(out).all()), "a refused call wrote logits"
    assert d.wn_train_backward(eng._h, flat.data_ptr(), dl.data_ptr(), grads.data_ptr(), None) == _abi.WN_E_STATE   # still nothing to differentiate
    with pytest.raises(_abi.WnError) as ei:
        eng.set_forward_precision(True)
    assert ei.value.code == _abi.WN_E_UNSUPPORTED and "kernel_size" in str(ei.value)
    # a full-length clip is served, with the guard bands of the logits untouched
    L = short + 1
    idx = torch.randint(0, 256, (2, L), generator=torch.Generator().manual_seed(1), dtype=torch.int32).cuda()
    out = torch.full((2 * out_len * 256 + 512,), float("nan"), device="cuda")
    assert d.wn_train_forward(eng._h, flat.data_ptr(), idx.data_ptr(), 2, L, out_len, out.data_ptr() + 4 * 256, None) == 0
    torch.cuda.synchronize()
    assert bool(torch.isnan(out[:256]).all()) and bool(torch.isnan(out[-256:]).all()) and bool(torch.isfinite(out[256:-256]).all())
    eng.close()
