"""-m gpu: matrix-core inference for kernel_size 3 and 4 -- forward_indices / score_indices (wn_forward, wn_score) and batched priming (wn_prime) with the
filter/gate product of csrc/wn_forward.h: wn_fwd_gemm_taps.

Reference of checks 1-3: the module's OWN torch path on the CPU in float64 (the reference's algorithm; shares nothing with the kernels).  Models: seeded
default init with every parameter multiplied by 3.0 (as tests/test_gpu_score.py: default init alone gives logits of about 0.2), random indices.
Bars: logits within TOL = 1e-4 of tests/test_gpu_forward.py, relative to max(1, |logits64|_inf); scoring under the criteria of tests/test_gpu_score.py
(eps = LOGIT_RTOL * max(1, |logits64|_inf): row negative log-likelihoods and their mean within 2 eps, the argmax on every row whose float64 top-2 gap
exceeds 20 eps); queues under the criterion of tests/test_gpu_parity.py: test_batched_priming_equals_chain_priming; check 5 pins the logits to the REAL
reference's (tests/golden/golden_taps_v1.npz, tests/golden/make_golden_taps.py) at the absolute 1e-4 of the golden forward fixtures.
Unchanged and out of scope: forward() on a one-hot tensor and training stay on torch ops for kernel_size != 2 (tests/test_gpu_forward.py:
test_the_torch_path_is_never_silent)."""
import copy
import os

import numpy as np
import pytest
import torch

import c_oracle
import wavenet_model
from mi355_wavenet import _abi, engine, synth
from parity_common import LOGIT_RTOL
from test_gpu_forward import TOL
from test_gpu_score import Ref, _check_pred, _env, _score

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BAND = 64 * 256   # guard band of the logits, in floats


def _build(k, out_len, ch=(32, 32, 64, 64), bias=False, layers=3, blocks=2, seed=11, gain=3.0):
    torch.manual_seed(seed)
    m = wavenet_model.WaveNetModel(layers=layers, blocks=blocks, residual_channels=ch[0], dilation_channels=ch[1], skip_channels=ch[2],
                                   end_channels=ch[3], classes=256, output_length=out_len, kernel_size=k, bias=bias)
    with torch.no_grad():
        for p in m.parameters():
            p.mul_(gain)
    return m.eval()


def _logits64(m, idx):
    m64 = copy.deepcopy(m).cpu().double()
    m64.dtype = torch.DoubleTensor
    x = torch.nn.functional.one_hot(idx.long(), m.classes).permute(0, 2, 1).double()
    with torch.no_grad():
        return m64(x).numpy()


def _forward_in_bands(eng, idx, out_len):
    """wn_forward through the C ABI into a buffer whose logits are surrounded by NaN sentinels; returns the logits after checking the bands"""
    dev = eng.mem.device
    idx = idx.to(dev, torch.int32).contiguous()
    N, L = idx.shape
    M = N * out_len
    buf = torch.full((M * 256 + 2 * BAND,), float("nan"), dtype=torch.float32, device=dev)
    rc = eng.lib.dll.wn_forward(eng._h, idx.data_ptr(), N, L, out_len, buf.data_ptr() + 4 * BAND, eng.mem.stream())
    torch.cuda.synchronize()
    assert rc == 0, eng.lib.last_error()
    buf = buf.cpu().numpy()
    assert np.isnan(buf[:BAND]).all() and np.isnan(buf[-BAND:]).all(), "a guard band was written"
    y = buf[BAND:-BAND].reshape(M, 256)
    assert np.isfinite(y).all(), "a logit was left unwritten"
    return y


# ------------------------------------------------------------------------------------------------ check 1: forward_indices against float64
# (label, kernel sizes, channels R/D/S/E, bias, N, output_length, samples beyond receptive_field + output_length - 1)
FWD = [
    ("exact_nobias", (3, 4), (32, 32, 64, 64), False, 2, 4, 0),   # L = rf + 3: the oldest tap of the first output row is row 0 of the clip
    ("exact_bias", (3, 4), (32, 32, 64, 64), True, 2, 4, 0),
    ("longer_bias", (3, 4), (32, 32, 64, 64), True, 2, 4, 5),     # the first computed row of layer 0 is not the clip's first
    ("k192", (3,), (64, 32, 64, 64), False, 2, 4, 0),             # K = 3 * 64 = 192: one and a half times the 128 of the tile's width
    ("ragged_rows", (3, 4), (32, 32, 64, 64), True, 3, 129, 0),   # 129 rows per clip: ragged row tiles, a tile spans two clips
    ("one_row", (3, 4), (32, 32, 64, 64), False, 2, 1, 3),        # (at L = rf the reference's own shapes break: the un-dilation quirk)
]
FWD_CASES = [(c[0], k) + c[2:] for c in FWD for k in c[1]]


@pytest.mark.parametrize("label,k,ch,bias,N,out_len,extra", FWD_CASES, ids=["%s_k%d" % (c[0], c[1]) for c in FWD_CASES])
def test_forward_indices_against_float64(label, k, ch, bias, N, out_len, extra):
    m = _build(k, out_len, ch=ch, bias=bias)
    L = m.receptive_field + out_len - 1 + extra
    g = torch.Generator().manual_seed(1000 * k + out_len)
    idx = torch.randint(0, 256, (N, L), generator=g, dtype=torch.int32)
    ref = _logits64(m, idx)
    m = m.cuda()
    y = m.forward_indices(idx).cpu().numpy()
    eng = m._forward_engine()
    assert eng.info()["forward_native"] == 1
    yb = _forward_in_bands(eng, idx, out_len)
    scale = max(1.0, float(np.abs(ref).max()))
    dev = float(np.abs(y - ref).max())
    print("[%s k=%d] max |dlogit| %.3g  scale %.3g  bound %.3g" % (label, k, dev, scale, TOL * scale))
    assert y.shape == ref.shape and np.array_equal(y, yb)
    assert dev <= TOL * scale
    st = m.wn_stats()
    assert st["native_forward"] == 1 and not st["torch_fallbacks"]


# ------------------------------------------------------------------------------------------------ check 2: what stays refused
def test_short_clips_training_and_bf16_keep_todays_behaviour():
    m = _build(3, 4, ch=(64, 64, 64, 64)).cuda()
    rf = m.receptive_field
    with pytest.raises(ValueError, match=r"receptive_field \+ output_length - 1"):
        m.forward_indices(torch.zeros(2, rf + 4 - 2, dtype=torch.int32))
    with pytest.raises(ValueError, match="kernel_size 2"):
        m.train_forward_indices(torch.zeros(2, rf + 3, dtype=torch.int32))
    idx = torch.randint(0, 256, (2, rf + 3), generator=torch.Generator().manual_seed(3), dtype=torch.int32)
    y32 = m.forward_indices(idx).cpu().numpy()
    m.matrix_precision = "bf16"   # (64-channel shapes: kernel_size 2 would run bf16 operands here)
    y16 = m.forward_indices(idx).cpu().numpy()
    m.matrix_precision = "fp32"
    assert np.array_equal(y16, y32) and np.isfinite(y32).all() and float(np.abs(y32).max()) > 0
    with pytest.raises(_abi.WnError) as ei:
        m._forward_engine().set_forward_precision(True)
    assert ei.value.code == _abi.WN_E_UNSUPPORTED and "kernel_size" in str(ei.value)


# ------------------------------------------------------------------------------------------------ check 3: score_indices, the trainer
@pytest.fixture(scope="module")
def score_case():
    m = _build(3, 37)
    g = torch.Generator().manual_seed(5)
    idx = torch.randint(0, 256, (4, m.receptive_field + 36), generator=g, dtype=torch.int32)
    tgt = torch.randint(0, 256, (4 * 37,), generator=g, dtype=torch.int64)
    return m.cuda(), idx, tgt, Ref(m, idx, tgt.numpy())


@pytest.mark.parametrize("fused", [True, False], ids=["fused", "unfused"])
def test_score_indices_against_float64(score_case, fused):
    m, idx, tgt, ref = score_case
    nll, pred, sums = _score(m, idx, tgt, fused=fused)
    dev = float(np.abs(nll - ref.nll).max())
    mean_dev = abs(sums[0] / sums[2] - ref.nll.mean())
    print("[k3 %s] max |row_nll - nll64| %.3g  |mean - mean64| %.3g  bound %.3g  undecidable rows %d" % (
        "fused" if fused else "unfused", dev, mean_dev, 2 * ref.eps, int((~ref.decidable).sum())))
    assert sums[2] == ref.nll.size
    assert dev <= 2 * ref.eps
    assert mean_dev <= 2 * ref.eps
    _check_pred(pred, sums, tgt.numpy(), ref, "k3")
    assert not m.wn_stats()["torch_fallbacks"]


def test_trainer_native_validation_of_a_kernel_size_3_model(tmp_path):
    import audio_data
    import wavenet_training
    rs = np.random.RandomState(8)
    np.savez(str(tmp_path / "ds.npz"), rs.randint(0, 256, 1500).astype(np.uint8), rs.randint(0, 256, 900).astype(np.uint8))
    m = _build(3, 16, seed=2)
    il = m.receptive_field + m.output_length - 1
    ds = audio_data.WavenetDataset(str(tmp_path / "ds.npz"), item_length=il, target_length=m.output_length, test_stride=5)
    ds.train = False
    n_test = len(ds)
    win = torch.stack([torch.as_tensor(ds._stream[ds.sample_index(i):ds.sample_index(i) + il + 1].astype(np.int32)) for i in range(n_test)])
    ds.train = True
    ref = Ref(m, win[:, :-1], win[:, -m.output_length:].reshape(-1).numpy().astype(np.int64))
    m = m.cuda()
    off = wavenet_training.WavenetTrainer(m, ds, device_batches=True)
    on = wavenet_training.WavenetTrainer(m, ds, device_batches=True, native_validation=True)
    off.dataloader = on.dataloader = torch.utils.data.DataLoader(ds, batch_size=8)
    loss_off, acc_off = off.validate()   # (forward_indices per batch, F.cross_entropy and torch.max on its logits)
    before = m.wn_stats()["native_forward"]
    loss_on, acc_on = on.validate()
    assert m.wn_stats()["native_forward"] == before + -(-n_test // 8), "score_indices once per batch"
    undecidable = int((~ref.decidable).sum())
    print("[trainer k3] loss torch ops %.9g native %.9g  accuracy %.6f %.6f  undecidable rows %d of %d" % (loss_off, loss_on, acc_off, acc_on, undecidable, ref.decidable.size))
    assert abs(loss_on - loss_off) <= 2 * ref.eps
    assert abs(acc_on - acc_off) * ref.decidable.size <= undecidable + 1e-9   # (equal where every row is decidable in float64)


# ------------------------------------------------------------------------------------------------ check 4: batched priming
K3S = dict(layers=3, blocks=2, dilation_channels=32, residual_channels=32, skip_channels=64, end_channels=64, classes=256, kernel_size=3, bias=True)
K4S = dict(K3S, kernel_size=4)


def _facade(cfg, W):
    m = wavenet_model.WaveNetModel(output_length=8, **cfg)
    m.load_state_dict({k: torch.from_numpy(v) for k, v in W.items()})
    return m


@pytest.mark.parametrize("cfg", [K3S, K4S], ids=["k3", "k4"])
def test_generate_fast_primes_in_one_batched_pass(cfg, monkeypatch):
    """The stack of tests/test_gpu_parity.py's K3 (3 x 2, biases) at 32 / 32 / 64 / 64 channels -- K3's own 12 / 8 / 20 / 24 are no multiples of 32, and zero
    padding into a compiled shape exists for kernel_size 2 only (test_the_unpadded_k3_shape_still_primes_through_the_chain) -- and its kernel_size 4 sibling."""
    W = synth.init_weights(cfg, seed=61, gain=3.0)
    NL, n_new = cfg["layers"] * cfg["blocks"], 30
    first = np.random.RandomState(62).randint(0, 256, engine.Engine.PRIME_BATCH_MIN + 10)
    m = _facade(cfg, W)
    audio = m.generate_fast(n_new, first_samples=torch.from_numpy(first), temperature=0)
    assert m._wn_last_prime_batched is True
    qa = [m._wn_engine.export_queue(l, 0) for l in range(NL)]
    m2 = _facade(cfg, W)
    monkeypatch.setattr(engine.Engine, "PRIME_BATCH_MIN", 10 ** 9)   # the same window through the chain, one sample per pass
    audio_chain = m2.generate_fast(n_new, first_samples=torch.from_numpy(first), temperature=0)
    assert m2._wn_last_prime_batched is False
    qb = [m2._wn_engine.export_queue(l, 0) for l in range(NL)]
    for l, ((da, ia, oa), (db, ib, ob)) in enumerate(zip(qa, qb)):
        assert (ia, oa) == (ib, ob), l
        assert da.shape == (cfg["residual_channels"], (cfg["kernel_size"] - 1) * 2 ** (l % cfg["layers"]) + 1)
        assert np.abs(da - db).max() <= 1e-5 * max(1.0, float(np.abs(db).max())), l
        assert np.abs(db).max() > 0
    o_idx, o_log = c_oracle.generate(cfg, W, n_new, first, 0.0, 0.0)
    top2 = np.sort(o_log, axis=1)
    gap, tol = float((top2[:, -1] - top2[:, -2]).min()), LOGIT_RTOL * max(1.0, float(np.abs(o_log).max()))
    print("[prime k=%d] oracle's smallest top-2 gap %.3g, 10 x logit tolerance %.3g" % (cfg["kernel_size"], gap, 10 * tol))
    assert gap > 10 * tol, "the case was chosen so that greedy indices are decidable"
    assert np.array_equal(audio, m._expand_indices(o_idx)) and np.array_equal(audio_chain, audio)


def test_the_unpadded_k3_shape_still_primes_through_the_chain():
    """tests/test_gpu_parity.py's K3 itself (12 / 8 / 20 / 24 channels): no matrix-core form, today's behaviour -- chain priming, the oracle's indices."""
    cfg = dict(synth.CONFIGS["tiny_bias"], kernel_size=3)
    W = synth.init_weights(cfg, seed=63, gain=3.0)
    first = np.random.RandomState(64).randint(0, 256, engine.Engine.PRIME_BATCH_MIN + 10)
    m = _facade(cfg, W)
    audio = m.generate_fast(30, first_samples=torch.from_numpy(first), temperature=0)
    assert m._wn_last_prime_batched is False and m._wn_engine.info()["forward_native"] == 0
    o_idx, o_log = c_oracle.generate(cfg, W, 30, first, 0.0, 0.0)
    top2 = np.sort(o_log, axis=1)
    if float((top2[:, -1] - top2[:, -2]).min()) > 10 * LOGIT_RTOL * max(1.0, float(np.abs(o_log).max())):
        assert np.array_equal(audio, m._expand_indices(o_idx))


# ------------------------------------------------------------------------------------------------ check 5: the real reference's logits
@pytest.mark.parametrize("case", ["taps_k3", "taps_k4"])
def test_forward_indices_reproduces_the_reference_golden(case):
    z = np.load(os.path.join(ROOT, "tests", "golden", "golden_taps_v1.npz"))
    wseed, N, out_len, L, k, bias = [int(v) for v in z[case + "_meta"]]
    cfg = dict(layers=3, blocks=2, dilation_channels=32, residual_channels=32, skip_channels=64, end_channels=64, classes=256, kernel_size=k, bias=bool(bias))
    ids, ref = z[case + "_ids"].astype(np.int64), z[case + "_out"]
    assert ids.shape == (N, L) and L >= synth.receptive_field(cfg) + out_len - 1
    eng = engine.Engine(cfg, synth.init_weights(cfg, seed=wseed))
    y = eng.forward_indices(ids, out_len).cpu().numpy()
    eng.close()
    assert y.shape == ref.shape
    dev = float(np.abs(y - ref).max())
    print(case, "max |dlogit| vs the reference", dev, "scale", float(np.abs(ref).max()))
    assert dev <= TOL
