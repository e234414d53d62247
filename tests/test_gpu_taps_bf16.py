"""-m gpu: opt-in bf16 matrix operands for kernel_size 3 and 4 inference (WaveNetModel.native_taps_bf16 = True with matrix_precision = "bf16"; C ABI
wn_set_forward_precision(h, WN_PRECISION_BF16_TAPS)), end to end: forward_indices / score_indices / the trainer's native validation on
wn_fwd_gemm_taps_bf16 and the bf16 residual, skip and head products (or score kernels) of kernel_size 2.

Models as tests/test_gpu_taps.py builds them (seeded default init, every parameter times 3.0), 3 x 2 layers, channels 64/64/64/64 and -- for the
128 x 256 tile of the filter/gate product -- 64/128/128/64.

 a. Embedding, bit for bit.  A kernel_size k model whose filter and gate weights are zero on the k - 2 oldest taps computes the function of the
    kernel_size 2 model that has the two newest taps (asserted here on the CPU torch path: max |dlogit| = 0.0).  On the GPU both run bf16 operands; the
    zero taps add exact zeros to the accumulators and the chunk order of the remaining two views is the two-view product's, so the logits are equal bit
    for bit: the new kernel and the k-tap bank are held to the established bf16 path (and through it to its oracle).  (Neither shape is the 128 / 128
    one whose kernel_size 2 layers would run as the one-launch kernel.)
 b. Dense taps against fp32: 0 < max |d| <= 3e-2 |logits32|_inf, the argmax equal on rows whose fp32 top-2 gap exceeds 4 x the deviation (the bars of
    tests/test_gpu_forward.py::test_forward_bf16_operands_close_to_fp32), the fp32 bits back after the switch; the logits also through the C ABI into NaN
    guard bands.
 c. score_indices with the switch, fused and unfused, under the criterion of tests/test_gpu_score.py's bf16 case: the yardstick is the float64
    log-softmax of the same model's bf16 forward_indices logits, spread = max |nll(yardstick) - nll64|, and row_nll may be 1.5 x that far from float64.
    The trainer's native validation under the same criterion against F.cross_entropy on the bf16 logits.
 d. What stays: the switch off, mode 1, the refusals of mode 2, kernel_size 2 under mode 2, short clips, generate_fast, the native_taps_training step."""
import ctypes

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from mi355_wavenet import _abi, engine
from test_gpu_score import Ref, _nll64, _score
from test_gpu_taps import _build, _forward_in_bands

pytestmark = pytest.mark.gpu
NARROW, WIDE = (64, 64, 64, 64), (64, 128, 128, 64)   # residual / dilation / skip / end channels
MODE_TAPS = 2   # include/wn_abi.h: WN_PRECISION_BF16_TAPS


def _on(m):
    m.native_taps_bf16 = True
    m.matrix_precision = "bf16"
    return m


def _idx(n, L, seed):
    return torch.randint(0, 256, (n, L), generator=torch.Generator().manual_seed(seed), dtype=torch.int32)


# ------------------------------------------------------------------------------------------------ a. embedding
@pytest.mark.parametrize("ch", [NARROW, WIDE], ids=["narrow", "wide"])
@pytest.mark.parametrize("k", [3, 4])
def test_zero_old_taps_equal_the_kernel_size_2_bf16_path_bit_for_bit(k, ch):
    out_len, N = 5, 2
    mk = _build(k, out_len, ch=ch, bias=True)
    m2 = _build(2, out_len, ch=ch, bias=True)
    with torch.no_grad():
        for convs in (mk.filter_convs, mk.gate_convs):
            for c in convs:
                c.weight[:, :, :k - 2] = 0
        sd = {n: v.clone() for n, v in mk.state_dict().items()}
        for n in sd:
            if n.startswith(("filter_convs", "gate_convs")) and n.endswith("weight"):
                sd[n] = sd[n][:, :, k - 2:].contiguous()
        m2.load_state_dict(sd)
    L = mk.receptive_field + out_len - 1
    idx = _idx(N, L, 100 * k + len(ch))
    x = F.one_hot(idx.long(), 256).permute(0, 2, 1).float()
    with torch.no_grad():
        ya, yb = mk(x).numpy(), m2(x).numpy()
    assert float(np.abs(ya - yb).max()) == 0.0, "precondition: the two models compute the same function on the CPU torch path"
    mk, m2 = _on(mk.cuda()), m2.cuda()
    m2.matrix_precision = "bf16"
    yk = mk.forward_indices(idx).cpu().numpy()
    y2 = m2.forward_indices(idx).cpu().numpy()
    mk.matrix_precision = "fp32"
    yk32 = mk.forward_indices(idx).cpu().numpy()
    assert np.isfinite(yk).all() and float(np.abs(yk).max()) > 0
    assert not np.array_equal(yk, yk32), "the switch did not change the operands"
    assert np.array_equal(yk, y2)


# ------------------------------------------------------------------------------------------------ b. dense taps against fp32
# (label, channels, bias, N, output_length, samples beyond receptive_field + output_length - 1)
DENSE = [
    ("exact_narrow", NARROW, False, 2, 4, 0),    # the oldest tap of the first output row is row 0 of the clip
    ("exact_wide", WIDE, True, 2, 4, 0),
    ("longer_wide", WIDE, True, 2, 4, 5),        # the first computed row of layer 0 is not the clip's first
    ("ragged_rows", NARROW, True, 3, 129, 0),    # 129 rows per clip: ragged row tiles, a tile spans two clips
    ("one_row", WIDE, False, 2, 1, 3),           # (as tests/test_gpu_taps.py: at L = rf the reference's own shapes break)
]


@pytest.mark.parametrize("label,ch,bias,N,out_len,extra", DENSE, ids=[c[0] for c in DENSE])
@pytest.mark.parametrize("k", [3, 4])
def test_dense_taps_bf16_close_to_fp32(k, label, ch, bias, N, out_len, extra):
    m = _build(k, out_len, ch=ch, bias=bias).cuda()
    m.native_taps_bf16 = True
    L = m.receptive_field + out_len - 1 + extra
    idx = _idx(N, L, 1000 * k + out_len)
    y32 = m.forward_indices(idx).cpu().numpy()
    m.matrix_precision = "bf16"
    y16 = m.forward_indices(idx).cpu().numpy()
    y16b = _forward_in_bands(m._forward_engine(), idx, out_len)   # (the engine is still in the taps mode)
    m.matrix_precision = "fp32"
    again = m.forward_indices(idx).cpu().numpy()
    assert np.array_equal(again, y32) and np.array_equal(y16b, y16)
    scale = float(np.abs(y32).max())
    dev = float(np.abs(y16 - y32).max())
    print("[%s k=%d] bf16 vs fp32 max |dlogit| %.4g  |logits32|_inf %.4g  ratio %.3g" % (label, k, dev, scale, dev / scale))
    assert 0 < dev <= 3e-2 * scale
    top2 = np.sort(y32, axis=1)
    clear = (top2[:, -1] - top2[:, -2]) > 4 * dev
    assert np.array_equal(y16.argmax(1)[clear], y32.argmax(1)[clear])
    st = m.wn_stats()
    assert st["native_forward"] == 3 and not st["torch_fallbacks"]


# ------------------------------------------------------------------------------------------------ c. scoring
_SCORE = {}


def _score_case(k):
    if k not in _SCORE:
        m = _build(k, 37, ch=NARROW if k == 3 else WIDE, bias=k == 4)
        g = torch.Generator().manual_seed(5)
        idx = torch.randint(0, 256, (4, m.receptive_field + 36), generator=g, dtype=torch.int32)
        tgt = torch.randint(0, 256, (4 * 37,), generator=g, dtype=torch.int64)
        ref = Ref(m, idx, tgt.numpy())
        m = m.cuda()
        m.native_taps_bf16 = True
        m.matrix_precision = "bf16"
        lg = m.forward_indices(idx).cpu().numpy()
        m.matrix_precision = "fp32"
        _SCORE[k] = (m, idx, tgt, ref, lg)
    return _SCORE[k]


@pytest.mark.parametrize("fused", [True, False], ids=["fused", "unfused"])
@pytest.mark.parametrize("k", [3, 4])
def test_score_indices_is_as_close_to_float64_as_the_bf16_forward(k, fused):
    m, idx, tgt, ref, lg = _score_case(k)
    yard = _nll64(lg, tgt.numpy())
    spread = float(np.abs(yard - ref.nll).max())
    nll32 = _score(m, idx, tgt, fused=fused, precision="fp32")[0]
    nll, pred, sums = _score(m, idx, tgt, fused=fused, precision="bf16")
    dev = float(np.abs(nll - ref.nll).max())
    print("[k%d %s bf16] max |logits - logits64| %.4g  max |nll - nll64|: yardstick %.4g  score %.4g  (fp32 score %.4g)" % (
        k, "fused" if fused else "unfused", float(np.abs(lg - ref.logits).max()), spread, dev, float(np.abs(nll32 - ref.nll).max())))
    assert spread > 100 * ref.eps, "the yardstick is not a bf16 forward"
    assert not np.array_equal(nll, nll32), "the switch did not reach wn_score"
    assert sums[2] == nll.size and dev <= 1.5 * spread
    assert abs(sums[0] / sums[2] - yard.mean()) <= 1.5 * spread
    assert sums[1] == float((pred == tgt.numpy()).sum())
    if not fused:   # (the two head products of the bf16 forward, then the row kernel over its very logits: the first argmax of every row)
        assert np.array_equal(pred, lg.argmax(1))
    assert not m.wn_stats()["torch_fallbacks"]


def test_trainer_native_validation_with_the_switch(tmp_path):
    import audio_data
    import wavenet_training
    rs = np.random.RandomState(8)
    np.savez(str(tmp_path / "ds.npz"), rs.randint(0, 256, 1500).astype(np.uint8), rs.randint(0, 256, 900).astype(np.uint8))
    m = _build(3, 16, ch=NARROW, seed=2)
    il = m.receptive_field + m.output_length - 1
    ds = audio_data.WavenetDataset(str(tmp_path / "ds.npz"), item_length=il, target_length=m.output_length, test_stride=5)
    ds.train = False
    n_test = len(ds)
    win = torch.stack([torch.as_tensor(ds._stream[ds.sample_index(i):ds.sample_index(i) + il + 1].astype(np.int32)) for i in range(n_test)])
    ds.train = True
    tgt = win[:, -m.output_length:].reshape(-1).numpy().astype(np.int64)
    ref = Ref(m, win[:, :-1], tgt)
    m = _on(m.cuda())
    lg = m.forward_indices(win[:, :-1]).cpu().numpy()
    yard = _nll64(lg, tgt)
    spread = float(np.abs(yard - ref.nll).max())
    off = wavenet_training.WavenetTrainer(m, ds, device_batches=True)
    on = wavenet_training.WavenetTrainer(m, ds, device_batches=True, native_validation=True)
    off.dataloader = on.dataloader = torch.utils.data.DataLoader(ds, batch_size=8)
    loss_off, acc_off = off.validate()   # (forward_indices per batch -- bf16 operands --, F.cross_entropy and torch.max on its logits)
    before = m.wn_stats()["native_forward"]
    loss_on, acc_on = on.validate()
    assert m.wn_stats()["native_forward"] == before + -(-n_test // 8), "score_indices once per batch"
    m.matrix_precision = "fp32"
    loss32, _ = on.validate()
    print("[trainer k3 bf16] loss torch ops %.9g native %.9g (fp32 native %.9g)  accuracy %.6f %.6f  spread %.4g" % (
        loss_off, loss_on, loss32, acc_off, acc_on, spread))
    assert spread > 100 * ref.eps and loss_on != loss32
    assert abs(loss_on - loss_off) <= 1.5 * spread
    # (and far inside it: by default bf16 operands score on the unfused path -- the forward's own head products, then the row kernel over its very
    #  logits --, so the two losses differ by the fp32 evaluation of the log-softmax alone: the 2 eps of the fp32 criterion)
    assert abs(loss_on - loss_off) <= 2 * ref.eps
    top2 = np.sort(lg.astype(np.float64), axis=1)
    close = int(((top2[:, -1] - top2[:, -2]) <= 20 * ref.eps).sum())
    assert abs(acc_on - acc_off) * tgt.size <= close + 1e-9


# ------------------------------------------------------------------------------------------------ d. what stays
def _raw_handle(lib, k, ch, n_streams=1):
    c = _abi.wn_config(3, 2, ch[1], ch[0], ch[2], ch[3], 256, k, 0, n_streams, 0, 0, 0)
    h = ctypes.c_void_p()
    lib.check(lib.dll.wn_create(ctypes.byref(c), ctypes.byref(h)))
    return h


def test_switch_off_and_the_refusals():
    m = _build(3, 4, ch=NARROW).cuda()
    rf = m.receptive_field
    idx = _idx(2, rf + 3, 3)
    y32 = m.forward_indices(idx).cpu().numpy()
    m.matrix_precision = "bf16"   # (the switch is off: fp32 bits, as before)
    y16 = m.forward_indices(idx).cpu().numpy()
    assert np.array_equal(y16, y32) and float(np.abs(y32).max()) > 0
    eng = m._forward_engine()
    d = eng.lib.dll
    with pytest.raises(_abi.WnError) as ei:
        eng.set_forward_precision(True)   # mode 1 on such a handle: refused as before
    assert ei.value.code == _abi.WN_E_UNSUPPORTED and "kernel_size" in str(ei.value)
    assert np.array_equal(m.forward_indices(idx).cpu().numpy(), y32)
    # mode 2: served; a short clip stays refused, with nothing written
    eng.set_forward_precision(True, taps=True)
    yb = _forward_in_bands(eng, idx, 4)
    assert not np.array_equal(yb, y32)
    short = torch.zeros(2, rf + 4 - 2, dtype=torch.int32, device="cuda")
    out = torch.full((2 * 4 * 256 + 512,), float("nan"), device="cuda")
    assert d.wn_forward(eng._h, short.data_ptr(), 2, rf + 2, 4, out.data_ptr() + 4 * 256, None) == _abi.WN_E_UNSUPPORTED
    torch.cuda.synchronize()
    assert bool(torch.isnan(out).all()), "a refused call wrote logits"
    m.native_taps_bf16 = True
    with pytest.raises(ValueError, match=r"receptive_field \+ output_length - 1"):
        m.forward_indices(torch.zeros(2, rf + 2, dtype=torch.int32))
    eng.set_forward_precision(False)
    assert np.array_equal(_forward_in_bands(eng, idx, 4), y32)
    # before the weights; other channel shapes; kernel_size 5
    lib = eng.lib
    h = _raw_handle(lib, 3, NARROW)
    assert d.wn_set_forward_precision(h, MODE_TAPS) == _abi.WN_E_STATE
    assert d.wn_set_forward_precision(h, 0) == 0
    d.wn_destroy(h)
    small = _build(3, 4, ch=(32, 32, 64, 64))
    e2 = engine.Engine(small._config(), dict(small.state_dict()))
    assert d.wn_set_forward_precision(e2._h, MODE_TAPS) == _abi.WN_E_UNSUPPORTED and b"multiples of 64" in d.wn_last_error()
    e2.close()
    small = _on(small.cuda())   # (the facade does not ask for it there: fp32, nothing raised)
    i2 = _idx(2, small.receptive_field + 3, 4)
    a = small.forward_indices(i2).cpu().numpy()
    small.matrix_precision = "fp32"
    assert np.array_equal(small.forward_indices(i2).cpu().numpy(), a)
    k5 = _build(5, 4, ch=NARROW)
    e5 = engine.Engine(k5._config(), dict(k5.state_dict()))
    assert d.wn_set_forward_precision(e5._h, MODE_TAPS) == _abi.WN_E_UNSUPPORTED and b"kernel_size" in d.wn_last_error()
    e5.close()


def test_mode_2_on_a_kernel_size_2_handle_is_mode_1():
    m = _build(2, 8, ch=WIDE, bias=True)
    eng = engine.Engine(m._config(), dict(m.state_dict()))
    idx = _idx(2, m.receptive_field + 7, 9)
    y32 = eng.forward_indices(idx, 8).cpu().numpy()
    eng.set_forward_precision(True)
    y1 = eng.forward_indices(idx, 8).cpu().numpy()
    eng.set_forward_precision(False)
    eng.set_forward_precision(True, taps=True)
    y2 = eng.forward_indices(idx, 8).cpu().numpy()
    eng.set_forward_precision(False)
    assert np.array_equal(eng.forward_indices(idx, 8).cpu().numpy(), y32)
    eng.close()
    assert np.array_equal(y1, y2) and not np.array_equal(y1, y32)


def test_generate_fast_is_untouched_by_the_switch():
    first = np.random.RandomState(62).randint(0, 256, engine.Engine.PRIME_BATCH_MIN + 10)
    runs = []
    for on in (False, True):
        m = _build(3, 8, ch=NARROW, bias=True, seed=61)
        m.matrix_precision = "bf16"
        m.native_taps_bf16 = on
        m.generate_fast(4, first_samples=torch.from_numpy(first), temperature=0)   # (creates the engine that forward_indices then runs on)
        y = m.forward_indices(_idx(2, m.receptive_field + 7, 5)).cpu().numpy()      # (switch on: leaves that engine in the taps mode)
        audio = m.generate_fast(30, first_samples=torch.from_numpy(first), temperature=0)
        assert m._wn_last_prime_batched is True
        queues = [m._wn_engine.export_queue(l, 0) for l in range(6)]
        runs.append((y, audio, queues))
    (y_off, a_off, q_off), (y_on, a_on, q_on) = runs
    assert not np.array_equal(y_off, y_on), "the switch did not reach the generation engine's forward"
    assert np.array_equal(a_off, a_on)
    for (da, ia, oa), (db, ib, ob) in zip(q_off, q_on):
        assert (ia, oa) == (ib, ob) and np.array_equal(da, db) and float(np.abs(da).max()) > 0


def test_the_native_taps_training_step_stays_fp32():
    from test_gpu_taps_training import _batch, _native_step, _one_hot
    torch.manual_seed(7)
    m = _build(3, 16, ch=NARROW, bias=True, seed=7).train()
    m.native_taps_training = True
    m.deterministic_gradients = True
    m = m.cuda()
    idx, target = _batch(m, 2, 0, seed=3)
    x, target = _one_hot(idx).cuda(), target.cuda()
    a = _native_step(m, x, target)
    # the facade never asks the training engine for it
    _on(m)
    b = _native_step(m, x, target)
    # and a handle put into the mode through the C ABI runs the same fp32 step
    eng = m._wn_train_runner.eng
    keep = m._apply_precision
    m._apply_precision = lambda e: None
    try:
        assert eng.lib.dll.wn_set_forward_precision(eng._h, MODE_TAPS) == 0
        c = _native_step(m, x, target)
        yb = eng.forward_indices(idx.to(torch.int32), 16).cpu().numpy()   # (the mode is on: wn_forward of this handle runs bf16 operands)
    finally:
        m._apply_precision = keep
        eng.set_forward_precision(False)
    y32 = eng.forward_indices(idx.to(torch.int32), 16).cpu().numpy()
    assert not np.array_equal(yb, y32)
    for other in (b, c):
        assert np.array_equal(a[0], other[0]) and a[1] == other[1]
        assert all(np.array_equal(a[2][key], other[2][key]) for key in a[2] if a[2][key] is not None)
