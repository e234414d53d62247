"""Times one scoring batch at BASELINE config 5's evaluation size (layers=10 blocks=5 dil/res=128 skip=512, N=32 one-second 16 kHz clips,
output_length = 16000 - 5116 + 1 = 10885: M = 348 320 rows) three ways, alternating them round by round in one process:

    torch     the parent commit's validate(): forward_indices() + F.cross_entropy + torch.max / eq / sum + two .item()
    unfused   wn_score with WN_NO_FUSED_SCORE=1: the two head products into the workspace + wn_score_rows
    fused     wn_score with WN_NO_FUSED_SCORE=0: wn_score_head (neither ev nor the logits reach HBM)

    python tools/bench_score.py [N] [L] [--bf16] [--end-channels E] [--rounds K]

Prints per path the median, minimum and maximum of the rounds (device-synchronised host clock around each call) and the results' agreement.
"""
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "pytorch-wavenet_amd"))
os.environ.setdefault("WN_TESTING", "1")   # (the A/B switch is honoured only with it)
import numpy as np  # noqa: E402
import torch  # noqa: E402
import torch.nn.functional as F  # noqa: E402

from mi355_wavenet import engine, synth  # noqa: E402


def opt(name, default):
    return type(default)(sys.argv[sys.argv.index(name) + 1]) if name in sys.argv else default


def main():
    pos = []
    skip = False
    for a in sys.argv[1:]:
        if skip:
            skip = False
        elif a in ("--end-channels", "--rounds"):
            skip = True
        elif not a.startswith("--"):
            pos.append(a)
    N = int(pos[0]) if len(pos) > 0 else 32
    L = int(pos[1]) if len(pos) > 1 else 16000
    cfg = dict(synth.CONFIGS["cfg3"])
    cfg["end_channels"] = opt("--end-channels", cfg["end_channels"])
    rounds = opt("--rounds", 7)
    bf16 = "--bf16" in sys.argv
    out_len = L - synth.receptive_field(cfg) + 1
    eng = engine.Engine(cfg, synth.init_weights(cfg, seed=0, gain=3.0))
    eng.set_forward_precision(bf16)
    rs = np.random.RandomState(0)
    ids = torch.from_numpy(rs.randint(0, 256, (N, L))).cuda().int()
    tgt = torch.from_numpy(rs.randint(0, 256, N * out_len)).cuda()

    def torch_path():
        out = eng.forward_indices(ids, out_len)
        loss = F.cross_entropy(out, tgt).item()
        hits = torch.sum(torch.eq(tgt, torch.max(out, 1)[1])).item()
        return loss, hits

    def native(fused):
        def run():
            os.environ["WN_NO_FUSED_SCORE"] = "0" if fused else "1"   # (pins the path whatever the default of the precision is)
            s = eng.score(ids, tgt, out_len)["sums"].tolist()   # (one sync, as the trainer's native validation pays per epoch)
            os.environ.pop("WN_NO_FUSED_SCORE", None)
            return s[0] / s[2], int(s[1])
        return run

    paths = [("torch", torch_path), ("unfused", native(False)), ("fused", native(True))]
    times = {k: [] for k, _ in paths}
    res = {}
    for k, fn in paths:   # warm every path: workspaces, code objects
        fn(); fn()
    torch.cuda.synchronize()
    for _ in range(rounds):
        for k, fn in paths:
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            res[k] = fn()
            torch.cuda.synchronize()
            times[k].append((time.perf_counter() - t0) * 1e3)
    print("config 5 scoring batch: N=%d L=%d output_length=%d rows=%d S=%d E=%d %s, %d alternating rounds" % (
        N, L, out_len, N * out_len, cfg["skip_channels"], cfg["end_channels"], "bf16" if bf16 else "fp32", rounds))
    for k, _ in paths:
        t = np.array(times[k])
        print("  %-8s median %8.3f ms   min %8.3f   max %8.3f   loss %.7f hits %d" % (k, np.median(t), t.min(), t.max(), res[k][0], res[k][1]))
    eng.close()


if __name__ == "__main__":
    main()
