"""Times one training step (model(x); cross_entropy; backward; Adam) of a kernel_size 3 or 4 model through the facade, opted in to the native step
(WaveNetModel.native_taps_training = True: wn_train_forward / wn_train_backward) against not opted in (the torch path: MIOpen conv1d + autograd),
same weights, same batch, same GPU, the two legs alternating in one process.  Times are device events around `--steps` steps, after warm-up of both.

    python tools/bench_train_taps.py [--kernel-size=3] [--layers=10] [--blocks=2] [--N=8] [--out-len=4096] [--steps=5] [--rounds=3] [--only=native|torch]

Default shape: 10 layers x 2 blocks, 128 / 128 / 512 / 256 channels, N = 8 clips of receptive_field + 4096 samples.  The loss is torch's F.cross_entropy
and the optimiser FusedAdam in both legs.  Needs an MI355X: there is no CPU leg.
"""
import os
import sys
import warnings

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "pytorch-wavenet_amd"))
import torch  # noqa: E402
import torch.nn.functional as F  # noqa: E402

import wavenet_model  # noqa: E402


def _opt(name, default):
    vals = [a.split("=", 1)[1] for a in sys.argv[1:] if a.startswith("--%s=" % name)]
    return type(default)(vals[0]) if vals else default


def main():
    assert torch.cuda.is_available(), "bench_train_taps needs the MI355X"
    from mi355_wavenet.optim import FusedAdam
    k, layers, blocks, N, out_len = _opt("kernel-size", 3), _opt("layers", 10), _opt("blocks", 2), _opt("N", 8), _opt("out-len", 4096)
    steps, rounds, only = _opt("steps", 5), _opt("rounds", 3), _opt("only", "")
    torch.manual_seed(0)
    master = wavenet_model.WaveNetModel(layers=layers, blocks=blocks, dilation_channels=128, residual_channels=128, skip_channels=512, end_channels=256,
                                        classes=256, output_length=out_len, kernel_size=k, bias=False)
    L = master.receptive_field + out_len
    g = torch.Generator().manual_seed(1)
    idx = torch.randint(0, 256, (N, L), generator=g)
    x = torch.zeros(N, 256, L).scatter_(1, idx.unsqueeze(1), 1.0).cuda()
    target = torch.randint(0, 256, (N * out_len,), generator=g).cuda()
    legs = {}
    for name in ("native", "torch"):
        if only and name != only:
            continue
        m = wavenet_model.WaveNetModel(layers=layers, blocks=blocks, dilation_channels=128, residual_channels=128, skip_channels=512, end_channels=256,
                                       classes=256, output_length=out_len, kernel_size=k, bias=False)
        m.load_state_dict(master.state_dict())
        m.native_taps_training = name == "native"
        m = m.cuda()
        legs[name] = (m, FusedAdam(m.parameters(), lr=1e-4))

    def step(name):
        m, opt = legs[name]
        opt.zero_grad(set_to_none=True)
        loss = F.cross_entropy(m(x), target)
        loss.backward()
        opt.step()
        return loss

    def timed(name):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        for _ in range(steps):
            loss = step(name)
        b.record()
        torch.cuda.synchronize()
        return a.elapsed_time(b) / steps, float(loss.detach())

    print("kernel_size %d, %d x %d layers, 128/128/512/256 channels, N %d, L %d (receptive field %d), output_length %d" % (
        k, layers, blocks, N, L, master.receptive_field, out_len))
    with warnings.catch_warnings():
        warnings.simplefilter("ignore", RuntimeWarning)   # (the torch leg announces itself)
        for name in legs:
            for _ in range(3):
                step(name)
        torch.cuda.synchronize()
        times = {name: [] for name in legs}
        for r in range(rounds):
            for name in legs:
                ms, loss = timed(name)
                times[name].append(ms)
                print("round %d  %-6s %8.2f ms / step   loss %.5f" % (r, name, ms, loss))
    for name, (m, _) in legs.items():
        st = m.wn_stats()
        assert (st["native_train_forward"] > 0) == (name == "native") and bool(st["torch_fallbacks"]) == (name == "torch"), (name, st)
        ts = sorted(times[name])
        print("%-6s median %.2f ms / step (min %.2f, max %.2f over %d rounds of %d steps)" % (name, ts[len(ts) // 2], ts[0], ts[-1], rounds, steps))
    if len(legs) == 2:
        med = {name: sorted(ts)[len(ts) // 2] for name, ts in times.items()}
        print("torch / native = %.2f" % (med["torch"] / med["native"]))


if __name__ == "__main__":
    main()
