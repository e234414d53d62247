"""Teacher-forced scoring on the GPU (C ABI wn_score, Engine.score, WaveNetModel.score_indices, WavenetTrainer(native_validation=True)).

Reference of every check: float64 logits of the module's OWN torch path on the CPU (the reference's algorithm; shares nothing with the kernels).
Models: seeded default init with every parameter multiplied by 3.0 (default init alone gives logits of about 0.2 and one predicted class), random
indices, full receptive field.  Cases (layers x blocks, R/D/S/E, N x output_length) and what the float64 reference itself measures on them:
    small   3x2   32/32/64/64     4 x 37     |logits64|_inf 10.2   undecidable rows (float64 top-2 gap <= 20 x the logit tolerance) 1/148 = 0.68 %   33 classes predicted
    mid     6x2   64/64/256/256   3 x 301                  18.7                                                                    6/903 = 0.66 %   65
    large   10x2  128/128/512/512 2 x 500                  30.6                                                                    1/1000 = 0.10 %  103
(model seed 11, data seed 5; measured on the CPU in float64 before the kernels were run, far inside the 2 % cap; printed again by every run: `pytest -s`).

Bounds.  The project's logit tolerance is LOGIT_RTOL = 1e-5 (tests/parity_common.py): eps = 1e-5 * max(1, |logits64|_inf).  An error eps on every
logit moves logsumexp - logit[target] by at most 2 eps, so row_nll and the mean are held to 2 eps.  The argmax is asserted on rows whose float64
top-2 gap exceeds 20 eps; the others may differ only towards the runner-up.

bf16 (test_bf16_*): the yardstick is the bf16 wn_forward's logits scored in float64 on the host; the fused kernel has the same rounding points, only the
order of the sums differs, so its row_nll may be at most 1.5 x as far from float64 as the yardstick's.  Measured on an MI355X, max |nll - nll64| per case,
yardstick / fused / unfused (profiles/r07_score.txt): small 3.951e-06 / 4.016e-06 / 4.016e-06 (32 residual channels: bf16 operands need multiples of 64, the
model runs fp32 there); mid 0.3451 / 0.3451 / 0.3451 (max |logits - logits64| 0.47); large 1.809 / 1.809 / 1.809 (2.11).
"""
import contextlib
import copy
import json
import os
import tempfile

import numpy as np
import pytest
import torch

from parity_common import LOGIT_RTOL

import wavenet_model
from mi355_wavenet import _abi, engine, synth

pytestmark = pytest.mark.gpu

CASES = {
    "small": dict(layers=3, blocks=2, ch=(32, 32, 64, 64), n=4, out=37),
    "mid": dict(layers=6, blocks=2, ch=(64, 64, 256, 256), n=3, out=301),
    "large": dict(layers=10, blocks=2, ch=(128, 128, 512, 512), n=2, out=500),
}
_CACHE = {}


def _build(layers, blocks, ch, out, classes=256, seed=11, gain=3.0):
    torch.manual_seed(seed)
    m = wavenet_model.WaveNetModel(layers=layers, blocks=blocks, residual_channels=ch[0], dilation_channels=ch[1], skip_channels=ch[2],
                                   end_channels=ch[3], classes=classes, output_length=out)
    with torch.no_grad():
        for p in m.parameters():
            p.mul_(gain)
    return m.eval()


def _logits64(m, idx):
    """float64 logits (N*output_length, classes) of the module's torch path on the CPU"""
    m64 = copy.deepcopy(m).cpu().double()
    m64.dtype = torch.DoubleTensor
    x = torch.nn.functional.one_hot(idx.long(), m.classes).permute(0, 2, 1).double()
    with torch.no_grad():
        return m64(x).numpy()


def _nll64(logits, tgt):
    lg = np.asarray(logits, dtype=np.float64)
    mx = lg.max(axis=1)
    lse = mx + np.log(np.exp(lg - mx[:, None]).sum(axis=1))
    return lse - lg[np.arange(lg.shape[0]), tgt]


class Ref:
    def __init__(self, m, idx, tgt):
        self.logits = _logits64(m, idx)
        self.eps = LOGIT_RTOL * max(1.0, float(np.abs(self.logits).max()))
        self.nll = _nll64(self.logits, tgt)
        order = np.argsort(-self.logits, axis=1, kind="stable")
        self.top, self.second = order[:, 0], order[:, 1]
        rows = np.arange(self.logits.shape[0])
        self.gap = self.logits[rows, self.top] - self.logits[rows, self.second]
        self.decidable = self.gap > 20 * self.eps


def _case(name):
    if name not in _CACHE:
        c = CASES[name]
        m = _build(c["layers"], c["blocks"], c["ch"], c["out"])
        g = torch.Generator().manual_seed(5)
        L = m.receptive_field + m.output_length - 1
        idx = torch.randint(0, 256, (c["n"], L), generator=g, dtype=torch.int32)
        tgt = torch.randint(0, 256, (c["n"] * c["out"],), generator=g, dtype=torch.int64)
        ref = Ref(m, idx, tgt.numpy())
        _CACHE[name] = (m.cuda(), idx, tgt, ref)
        print("\n[%s] |logits64|_inf %.2f  eps %.3g  undecidable rows %d/%d  distinct float64 predictions %d" % (
            name, np.abs(ref.logits).max(), ref.eps, int((~ref.decidable).sum()), ref.decidable.size, len(np.unique(ref.top))))
    return _CACHE[name]


@contextlib.contextmanager
def _env(**kv):
    saved = {k: os.environ.get(k) for k in kv}
    for k, v in kv.items():
        if v is None:
            os.environ.pop(k, None)
        else:
            os.environ[k] = v
    try:
        yield
    finally:
        for k, v in saved.items():
            if v is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = v


def _score(m, idx, tgt, fused=True, precision="fp32"):
    """numpy (row_nll, pred, sums) of score_indices on one path; the switch is read on every call"""
    m.matrix_precision = precision
    with _env(WN_NO_FUSED_SCORE="0" if fused else "1"):   # (=0 pins the fused kernel: with bf16 operands the unfused path is the default)
        r = m.score_indices(idx, tgt, want_rows=True, want_pred=True)
        torch.cuda.synchronize()
    m.matrix_precision = "fp32"
    return r.row_nll.cpu().numpy().reshape(-1).astype(np.float64), r.pred.cpu().numpy().reshape(-1), r.sums.cpu().numpy()


def _check_pred(pred, sums, tgt, ref, tag):
    ok = ref.decidable
    assert (~ok).sum() <= 0.02 * ok.size, "%s: %d of %d rows are undecidable in float64" % (tag, (~ok).sum(), ok.size)
    assert np.array_equal(pred[ok], ref.top[ok]), "%s: argmax differs on %d decidable rows" % (tag, int((pred[ok] != ref.top[ok]).sum()))
    other = pred != ref.top
    assert np.array_equal(pred[other], ref.second[other]), "%s: an undecidable row went to a class that is not the runner-up" % tag
    assert sums[1] == float((pred == tgt).sum()), "%s: sums[1] = %r, the written predictions hit %d targets" % (tag, sums[1], (pred == tgt).sum())
    hits_ref = float((ref.top[ok] == tgt[ok]).sum())
    assert hits_ref <= sums[1] <= hits_ref + float((~ok).sum())
    assert len(np.unique(pred)) >= 10, "%s: only %d distinct classes predicted: the accuracy check would be vacuous" % (tag, len(np.unique(pred)))


# ------------------------------------------------------------------------------------------------ checks 1 and 2: fp32 against float64
@pytest.mark.parametrize("fused", [True, False], ids=["fused", "unfused"])
@pytest.mark.parametrize("name", list(CASES))
def test_fp32_rows_sums_and_argmax_against_float64(name, fused):
    m, idx, tgt, ref = _case(name)
    nll, pred, sums = _score(m, idx, tgt, fused=fused)
    dev = float(np.abs(nll - ref.nll).max())
    mean_dev = abs(sums[0] / sums[2] - ref.nll.mean())
    print("[%s %s] max |row_nll - nll64| %.3g  |mean - mean64| %.3g  bound %.3g" % (name, "fused" if fused else "unfused", dev, mean_dev, 2 * ref.eps))
    assert sums[2] == ref.nll.size
    assert dev <= 2 * ref.eps
    assert mean_dev <= 2 * ref.eps
    _check_pred(pred, sums, tgt.numpy(), ref, name)
    assert not m.wn_stats()["torch_fallbacks"]


def test_ties_go_to_the_lower_index():
    """end_conv_2's weights zeroed: every row's logits are the bias, whose maximum sits at classes 70 and 201 (and, second case, at 31 and 32: two lanes
    of one accumulator tile, then two tiles)."""
    for lo, hi in ((70, 201), (31, 32), (5, 37)):
        m = _build(3, 2, (32, 32, 64, 64), 21)
        with torch.no_grad():
            m.end_conv_2.weight.zero_()
            m.end_conv_2.bias.copy_(torch.linspace(-1.0, 1.0, 256))
            m.end_conv_2.bias[lo] = 2.5
            m.end_conv_2.bias[hi] = 2.5
        m = m.cuda()
        idx = torch.randint(0, 256, (2, m.receptive_field + 20), dtype=torch.int32)
        tgt = torch.randint(0, 256, (42,), dtype=torch.int64)
        for fused in (True, False):
            _, pred, _ = _score(m, idx, tgt, fused=fused)
            assert (pred == lo).all(), (lo, hi, fused, np.unique(pred))


# ------------------------------------------------------------------------------------------------ check 3: fused against unfused
def _launches(prof):
    fd, path = tempfile.mkstemp(suffix=".json")
    os.close(fd)
    try:
        prof.export_chrome_trace(path)
        with open(path) as f:
            trace = json.load(f)
    finally:
        os.remove(path)
    return [e["name"] for e in trace.get("traceEvents", []) if e.get("ph") == "X" and "kernel" in str(e.get("cat", "")).lower() and "wn_" in e.get("name", "")]


@pytest.mark.parametrize("precision", ["fp32", "bf16"])
@pytest.mark.parametrize("name", list(CASES))
def test_fused_against_unfused(name, precision):
    m, idx, tgt, ref = _case(name)
    runs = {}
    for fused in (True, False):
        _score(m, idx, tgt, fused=fused, precision=precision)   # (warm: workspace allocations)
        with torch.profiler.profile(activities=[torch.profiler.ProfilerActivity.CUDA]) as prof:
            a = _score(m, idx, tgt, fused=fused, precision=precision)
        b = _score(m, idx, tgt, fused=fused, precision=precision)
        assert a[2].tobytes() == b[2].tobytes(), "sums differ between two runs of the same path: %r %r" % (a[2], b[2])
        assert a[0].tobytes() == b[0].tobytes() and np.array_equal(a[1], b[1])
        runs[fused] = (a, _launches(prof))
    (f, f_names), (u, u_names) = runs[True], runs[False]
    gemms = lambda names: sum("wn_fwd_gemm" in n for n in names)   # noqa: E731
    assert len(f_names) > 0, "torch.profiler recorded no native kernel launches"
    assert any("wn_score_head" in n for n in f_names) and not any("wn_score_rows" in n for n in f_names), f_names
    assert any("wn_score_rows" in n for n in u_names) and not any("wn_score_head" in n for n in u_names), u_names
    assert gemms(u_names) == gemms(f_names) + 2, "the unfused run launches the two head products, the fused run neither: %d vs %d" % (gemms(u_names), gemms(f_names))
    assert any("wn_score_reduce" in n for n in f_names) and any("wn_score_reduce" in n for n in u_names)
    ok = ref.decidable
    assert np.array_equal(f[1][ok], u[1][ok])
    if precision == "fp32":
        assert np.abs(f[0] - u[0]).max() <= 2 * ref.eps


# ------------------------------------------------------------------------------------------------ check 4: bf16
@pytest.mark.parametrize("name", list(CASES))
def test_bf16_fused_is_as_close_to_float64_as_the_bf16_forward(name):
    """Yardstick: the bf16 wn_forward's logits (matrix_precision = "bf16"), scored in float64 on the host.  spread = max |nll(yardstick) - nll64|; the fused
    kernel's row_nll may be 1.5 x that far from float64 (same rounding points, another summation order).  Figures: profiles/r07_score.txt."""
    m, idx, tgt, ref = _case(name)
    m.matrix_precision = "bf16"
    lg = m.forward_indices(idx).cpu().numpy()
    m.matrix_precision = "fp32"
    spread = float(np.abs(_nll64(lg, tgt.numpy()) - ref.nll).max())
    logit_spread = float(np.abs(lg - ref.logits).max())
    fused = float(np.abs(_score(m, idx, tgt, fused=True, precision="bf16")[0] - ref.nll).max())
    unfused = float(np.abs(_score(m, idx, tgt, fused=False, precision="bf16")[0] - ref.nll).max())
    print("[%s bf16] max |logits - logits64| %.4g  max |nll - nll64|: yardstick %.4g  fused %.4g  unfused %.4g" % (name, logit_spread, spread, fused, unfused))
    assert fused <= 1.5 * spread


# ------------------------------------------------------------------------------------------------ check 5: edges
SENT32 = 0x7FC0DEAD
BAND = 64


def _raw(eng, idx, tgt, out_len, want_nll=True, want_pred=True):
    """wn_score through the C ABI with every output inside bands of sentinel values; returns (rc, nll, pred, sums) after checking the bands"""
    dev = eng.mem.device
    idx = idx.to(dev, torch.int32).contiguous()
    tgt = tgt.to(dev, torch.int64).contiguous()
    N, L = idx.shape
    M = N * out_len
    nll = torch.full((M + 2 * BAND,), SENT32, dtype=torch.int32, device=dev)
    pred = torch.full((M + 2 * BAND,), SENT32, dtype=torch.int32, device=dev)
    sums = torch.full((3 + 2 * BAND,), -12345.0, dtype=torch.float64, device=dev)
    rc = eng.lib.dll.wn_score(eng._h, idx.data_ptr(), tgt.data_ptr(), N, L, out_len, nll.data_ptr() + 4 * BAND if want_nll else None,
                              pred.data_ptr() + 4 * BAND if want_pred else None, sums.data_ptr() + 8 * BAND, eng.mem.stream())
    torch.cuda.synchronize()
    nll, pred, sums = nll.cpu().numpy(), pred.cpu().numpy(), sums.cpu().numpy()
    for buf, written in ((nll, want_nll and rc == 0), (pred, want_pred and rc == 0)):
        assert (buf[:BAND] == SENT32).all() and (buf[-BAND:] == SENT32).all(), "a guard band was written"
        if not written:
            assert (buf == SENT32).all()
    assert (sums[:BAND] == -12345.0).all() and (sums[-BAND:] == -12345.0).all()
    return rc, nll[BAND:-BAND].view(np.float32).astype(np.float64), pred[BAND:-BAND], sums[BAND:-BAND]


@pytest.mark.parametrize("fused", [True, False], ids=["fused", "unfused"])
@pytest.mark.parametrize("n,out,short", [(1, 1, False), (3, 43, False), (2, 128, False), (2, 50, True)], ids=["one_row", "ragged_tile", "full_tile", "short_clip"])
def test_edges_rows_tiles_bands_and_null_outputs(n, out, short, fused):
    m = _build(4, 2, (64, 64, 128, 128), out, seed=3)
    L = m.receptive_field + out - 1 + (8 if out == 1 else 0) if not short else m.receptive_field + out - 9   # (short: the reference's zero-padding regime;
    # one row: 8 samples more than the receptive field -- at exactly the receptive field the reference's own shapes break, include/wn_abi.h: wn_forward)
    assert (L < m.receptive_field + out - 1) == short
    assert (n * out) % 128 != 0 or out == 128
    g = torch.Generator().manual_seed(n * 1000 + out)
    idx = torch.randint(0, 256, (n, L), generator=g, dtype=torch.int32)
    tgt = torch.randint(0, 256, (n * out,), generator=g, dtype=torch.int64)
    if n * out >= 4:
        tgt[1], tgt[n * out - 1] = -100, 256   # (F.cross_entropy's ignore_index, and one past the classes)
    ref = Ref(m, idx, np.clip(tgt.numpy(), 0, 255))
    valid = (tgt.numpy() >= 0) & (tgt.numpy() < 256)
    m = m.cuda()
    eng = m._forward_engine()
    with _env(WN_NO_FUSED_SCORE="0" if fused else "1"):   # (=0 pins the fused kernel: with bf16 operands the unfused path is the default)
        rc, nll, pred, sums = _raw(eng, idx, tgt, out)
        assert rc == 0, eng.lib.last_error()
        rc2, _, _, sums2 = _raw(eng, idx, tgt, out, want_nll=False, want_pred=False)
        assert rc2 == 0 and sums2.tobytes() == sums.tobytes(), "NULL row outputs change the sums"
        side = torch.cuda.Stream()
        with torch.cuda.stream(side):
            rc3, nll3, pred3, sums3 = _raw(eng, idx, tgt, out)
        assert rc3 == 0 and sums3.tobytes() == sums.tobytes() and np.array_equal(pred3, pred) and nll3.tobytes() == nll.tobytes(), "a non-default stream"
    assert np.isnan(nll[~valid]).all() and not np.isnan(nll[valid]).any()
    assert np.abs(nll[valid] - ref.nll[valid]).max() <= 2 * ref.eps
    assert sums[2] == valid.sum()
    assert abs(sums[0] - ref.nll[valid].sum()) <= 2 * ref.eps * valid.sum()
    ok = ref.decidable
    assert np.array_equal(pred[ok], ref.top[ok]), "row_pred is written on every row, NaN rows included"
    assert sums[1] == float(((pred == tgt.numpy()) & valid).sum())


def test_a_class_count_of_128_takes_the_unfused_path():
    m = _build(3, 2, (32, 32, 64, 64), 40, classes=128, seed=4)
    idx = torch.randint(0, 128, (2, m.receptive_field + 39), dtype=torch.int32)
    tgt = torch.randint(0, 128, (80,), dtype=torch.int64)
    tgt[7] = 128   # (outside THIS model's classes)
    ref = Ref(m, idx, np.clip(tgt.numpy(), 0, 127))
    m = m.cuda()
    with torch.profiler.profile(activities=[torch.profiler.ProfilerActivity.CUDA]) as prof:
        nll, pred, sums = _score(m, idx, tgt)
    names = _launches(prof)
    assert any("wn_score_rows" in n for n in names) and not any("wn_score_head" in n for n in names), names
    valid = tgt.numpy() < 128
    assert np.isnan(nll[~valid]).all() and sums[2] == valid.sum()
    assert np.abs(nll[valid] - ref.nll[valid]).max() <= 2 * ref.eps
    assert np.array_equal(pred[ref.decidable], ref.top[ref.decidable])


def test_refusals_are_wn_forwards():
    m = _build(3, 2, (32, 32, 64, 64), 16, seed=4).cuda()
    eng = m._forward_engine()
    L = 9   # (16 final positions do not exist)
    idx = torch.zeros(2, L, dtype=torch.int32, device="cuda")
    out = torch.empty(32, 256, device="cuda")
    rc_f = eng.lib.dll.wn_forward(eng._h, idx.data_ptr(), 2, L, 16, out.data_ptr(), None)
    msg_f = eng.lib.last_error()
    rc_s, _, _, _ = _raw(eng, idx, torch.zeros(32, dtype=torch.int64), 16)
    msg_s = eng.lib.last_error()
    assert rc_f == rc_s == _abi.WN_E_UNSUPPORTED
    assert msg_s == msg_f.replace("wn_forward", "wn_score")
    with pytest.raises(ValueError, match="wn_score"):
        m.score_indices(idx, torch.zeros(32, dtype=torch.int64))
    with pytest.raises(ValueError, match="class indices outside"):
        m.score_indices(torch.full((2, m.receptive_field + 15), 256, dtype=torch.int32), torch.zeros(32, dtype=torch.int64))
    with pytest.raises(ValueError, match=r"must be \(N, L\)"):
        m.score_indices(torch.zeros(5, dtype=torch.int32), torch.zeros(32, dtype=torch.int64))


def test_a_handle_with_chains_scores_like_a_single_chain():
    cfg = dict(synth.CONFIGS["cfg3"], layers=3, blocks=2)
    W = synth.init_weights(cfg, seed=21, gain=3.0)
    many = engine.Engine(cfg, W, n_streams=170)
    assert many.info()["n_chains"] >= 2
    one = engine.Engine(cfg, W, n_streams=1)
    idx = torch.randint(0, 256, (2, 200), dtype=torch.int32)
    tgt = torch.randint(0, 256, (2 * 60,), dtype=torch.int64)
    a, b = _raw(many, idx, tgt, 60), _raw(one, idx, tgt, 60)
    assert a[0] == b[0] == 0
    assert a[3].tobytes() == b[3].tobytes() and a[1].tobytes() == b[1].tobytes() and np.array_equal(a[2], b[2])
    assert np.isfinite(a[1]).all() and a[3][2] == 120
    many.close()
    one.close()


def test_the_switch_shows_in_dev_overrides_and_targets_none_cuts_the_dataset_window():
    m, idx, tgt, ref = _case("small")
    out = m.output_length
    window = torch.randint(0, 256, (3, idx.size(1) + 1), dtype=torch.int32)
    a = m.score_indices(window, want_rows=True)
    b = m.score_indices(window[:, :-1], window[:, -out:].long(), want_rows=True)
    assert torch.equal(a.row_nll, b.row_nll) and torch.equal(a.sums, b.sums)
    assert a.row_nll.shape == (3, out) and a.pred is None
    assert float(a.loss) == float(a.sums[0] / a.sums[2]) and int(a.n) == 3 * out
    before = m.wn_stats()["native_forward"]
    m.score_indices(window)
    assert m.wn_stats()["native_forward"] == before + 1
    m2 = _build(3, 2, (32, 32, 64, 64), 8, seed=9).cuda()
    with _env(WN_NO_FUSED_SCORE="1"):
        m2.score_indices(torch.zeros(1, m2.receptive_field + 8, dtype=torch.int32))
        assert m2._forward_engine().info()["dev_overrides"] == 1
    with _env(WN_NO_FUSED_SCORE="1", WN_TESTING="0"):   # (not honoured without WN_TESTING=1)
        with torch.profiler.profile(activities=[torch.profiler.ProfilerActivity.CUDA]) as prof:
            m.score_indices(window)
            torch.cuda.synchronize()
    assert any("wn_score_head" in n for n in _launches(prof))


# ------------------------------------------------------------------------------------------------ check 6: the trainer
def test_trainer_native_validation_matches_the_torch_ops_and_syncs_once(tmp_path, monkeypatch):
    import audio_data
    import wavenet_training
    rs = np.random.RandomState(8)   # (29 test items, 464 rows; measured on the CPU: smallest float64 top-2 gap 183 eps, no undecidable row, 37 classes predicted)
    np.savez(str(tmp_path / "ds.npz"), rs.randint(0, 256, 1500).astype(np.uint8), rs.randint(0, 256, 900).astype(np.uint8))
    m = _build(3, 2, (32, 32, 64, 64), 16, seed=2)
    il = m.receptive_field + m.output_length - 1
    ds = audio_data.WavenetDataset(str(tmp_path / "ds.npz"), item_length=il, target_length=m.output_length, test_stride=5)
    # no undecidable row in the test split: the two paths must then agree on every prediction
    ds.train = False
    n_test = len(ds)
    win = torch.stack([torch.as_tensor(ds._stream[ds.sample_index(i):ds.sample_index(i) + il + 1].astype(np.int32)) for i in range(n_test)])
    ds.train = True
    ref = Ref(m, win[:, :-1], win[:, -m.output_length:].reshape(-1).numpy().astype(np.int64))
    assert ref.decidable.all(), "the dataset was built to have no undecidable row"
    m = m.cuda()
    off = wavenet_training.WavenetTrainer(m, ds, device_batches=True)
    on = wavenet_training.WavenetTrainer(m, ds, device_batches=True, native_validation=True)
    assert off.native_validation is False
    off.dataloader = on.dataloader = torch.utils.data.DataLoader(ds, batch_size=8)   # (validate() takes its batch size from the training loader: 8, 8, 8, 5)
    loss_off, acc_off = off.validate()
    items = []
    real_item = torch.Tensor.item
    monkeypatch.setattr(torch.Tensor, "item", lambda self: (items.append(1), real_item(self))[1])
    real_score = wavenet_model.WaveNetModel.score_indices
    calls = []
    monkeypatch.setattr(wavenet_model.WaveNetModel, "score_indices", lambda self, *a, **k: (calls.append(1), real_score(self, *a, **k))[1])
    with torch.profiler.profile(activities=[torch.profiler.ProfilerActivity.CUDA]) as prof:
        loss_on, acc_on = on.validate()
    monkeypatch.undo()
    assert len(calls) == -(-n_test // 8) == 4 and not items, "score_indices once per batch, no .item() at all"
    names = _launches(prof)
    assert sum("wn_score_head" in n for n in names) == len(calls)
    print("[trainer] loss torch ops %.9g native %.9g  accuracy %.6f %.6f  batches %d" % (loss_off, loss_on, acc_off, acc_on, len(calls)))
    assert abs(loss_on - loss_off) <= 2 * ref.eps
    assert acc_on == acc_off


def test_defaults_fused_with_fp32_operands_unfused_with_bf16():
    """What runs without the switch: measured at config 5's evaluation batch the fused kernel is level or faster with fp32 operands and slower with bf16
    operands (profiles/r07_score.txt), so the bf16 default is the unfused path; both beat the torch ops."""
    m, idx, tgt, _ = _case("mid")
    for precision, want in (("fp32", "wn_score_head"), ("bf16", "wn_score_rows")):
        m.matrix_precision = precision
        with _env(WN_NO_FUSED_SCORE=None):
            with torch.profiler.profile(activities=[torch.profiler.ProfilerActivity.CUDA]) as prof:
                m.score_indices(idx, tgt)
                torch.cuda.synchronize()
        m.matrix_precision = "fp32"
        names = [n for n in _launches(prof) if "wn_score_head" in n or "wn_score_rows" in n]
        assert len(names) == 1 and want in names[0], (precision, names)
