"""Times forward_indices() and score_indices() of a kernel_size 3 or 4 model through the facade with fp32 operands (the default) and with the opt-in bf16
operands (WaveNetModel.native_taps_bf16 = True, matrix_precision = "bf16": wn_fwd_gemm_taps_bf16 and the bf16 residual / skip / head products), same
weights, same clips, same GPU, the four legs alternating round by round in one process.  Times are device events around one call, after warm-up of
every leg; printed as median (min - max) over the rounds.

    python tools/bench_forward_taps.py [--kernel-size=3] [--layers=10] [--blocks=2] [--N=8] [--out-len=4096] [--rounds=9]

Default shape: 10 layers x 2 blocks, 128 / 128 / 512 / 256 channels, N = 8 clips of receptive_field + 4096 samples (the shape tools/bench_train_taps.py
measures).  Needs an MI355X: there is no CPU leg.
"""
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "pytorch-wavenet_amd"))
import numpy as np  # noqa: E402
import torch  # noqa: E402

import wavenet_model  # noqa: E402


def _opt(name, default):
    vals = [a.split("=", 1)[1] for a in sys.argv[1:] if a.startswith("--%s=" % name)]
    return type(default)(vals[0]) if vals else default


def main():
    assert torch.cuda.is_available(), "bench_forward_taps needs the MI355X"
    k, layers, blocks, N, out_len = _opt("kernel-size", 3), _opt("layers", 10), _opt("blocks", 2), _opt("N", 8), _opt("out-len", 4096)
    rounds = max(7, _opt("rounds", 9))
    torch.manual_seed(0)
    m = wavenet_model.WaveNetModel(layers=layers, blocks=blocks, dilation_channels=128, residual_channels=128, skip_channels=512, end_channels=256,
                                   classes=256, output_length=out_len, kernel_size=k, bias=False)
    with torch.no_grad():
        for p in m.parameters():
            p.mul_(3.0)   # (default init alone gives logits of about 0.2)
    m = m.eval().cuda()
    m.native_taps_bf16 = True
    L = m.receptive_field + out_len
    g = torch.Generator().manual_seed(1)
    idx = torch.randint(0, 256, (N, L), generator=g, dtype=torch.int32).cuda()
    tgt = torch.randint(0, 256, (N * out_len,), generator=g).cuda()

    def leg(call, precision):
        def run():
            m.matrix_precision = precision
            return call()
        return run

    fwd = lambda: m.forward_indices(idx, check=False)               # noqa: E731
    score = lambda: m.score_indices(idx, tgt, check=False).sums     # noqa: E731
    legs = [("forward fp32", leg(fwd, "fp32")), ("forward bf16", leg(fwd, "bf16")), ("score fp32", leg(score, "fp32")), ("score bf16", leg(score, "bf16"))]
    out = {}
    for name, fn in legs:   # warm every leg: workspaces, code objects
        fn()
        out[name] = fn()
    torch.cuda.synchronize()
    times = {name: [] for name, _ in legs}
    for _ in range(rounds):
        for name, fn in legs:
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            fn()
            b.record()
            torch.cuda.synchronize()
            times[name].append(a.elapsed_time(b))
    print("kernel_size %d, %d x %d layers, 128/128/512/256 channels, N=%d clips of L=%d (receptive_field %d), output_length %d: %d rows; %d alternating rounds" % (
        k, layers, blocks, N, L, m.receptive_field, out_len, N * out_len, rounds))
    med = {}
    for name, _ in legs:
        t = np.array(times[name])
        med[name] = float(np.median(t))
        print("  %-13s median %8.3f ms  (%.3f - %.3f)" % (name, med[name], t.min(), t.max()))
    print("  bf16 against fp32: forward x %.2f, score x %.2f" % (med["forward fp32"] / med["forward bf16"], med["score fp32"] / med["score bf16"]))
    y32, y16 = out["forward fp32"].float().cpu().numpy(), out["forward bf16"].float().cpu().numpy()
    s32, s16 = out["score fp32"].cpu().numpy(), out["score bf16"].cpu().numpy()
    print("  logits: |logits32|_inf %.4g  max |bf16 - fp32| %.4g (%.3g of the scale)   mean nll fp32 %.6f bf16 %.6f" % (
        np.abs(y32).max(), np.abs(y16 - y32).max(), np.abs(y16 - y32).max() / np.abs(y32).max(), s32[0] / s32[2], s16[0] / s16[2]))
    m.matrix_precision = "fp32"


if __name__ == "__main__":
    main()
