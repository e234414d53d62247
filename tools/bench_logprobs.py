"""Times what the per-sample log-probabilities cost a generation job (Engine.generate(..., logprobs=), C ABI wn_set_logprob_output): the same job plain,
with logprobs="sampling", with logprobs="model" and -- for scale, the only way to the number before -- with want_logits=True plus a host log-softmax
at the drawn classes.  Same engine, same weights, same uniforms, the four legs alternating round by round in one process; wall time around one
synchronous generate() call (uploads, launch, wait, downloads), after warm-up of every leg; printed as median (min - max) over the rounds.  WN_TESTING is
taken out of the environment: the planner chooses the kernel.

    python tools/bench_logprobs.py [--samples=1600] [--rounds=9] [--jobs="cfg3 1;cfg3 64;cfg1 1"]

Needs an MI355X: there is no CPU leg.
"""
import os
import sys
import time

os.environ.pop("WN_TESTING", None)
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "pytorch-wavenet_amd"))
import numpy as np  # noqa: E402
import torch  # noqa: E402

from mi355_wavenet import engine, synth  # noqa: E402


def _opt(name, default):
    vals = [a.split("=", 1)[1] for a in sys.argv[1:] if a.startswith("--%s=" % name)]
    return type(default)(vals[0]) if vals else default


def host_logp(idx, logits):
    """float64 log-softmax of the dumped logits at the drawn classes: what a caller computed before the kernels wrote it"""
    l = logits.astype(np.float64)
    m = l.max(axis=2, keepdims=True)
    lse = np.log(np.exp(l - m).sum(axis=2)) + m[:, :, 0]
    return np.take_along_axis(l, idx[:, :, None].astype(np.int64), axis=2)[:, :, 0] - lse


def bench(cfgname, ns, n, rounds):
    cfg = synth.CONFIGS[cfgname]
    W = synth.init_weights(cfg, seed=7)
    rs = np.random.RandomState(11)
    first = rs.randint(0, 256, (ns, 1))
    u = rs.random_sample((ns, n))
    eng = engine.Engine(cfg, W, n_streams=ns)
    kw = dict(temperature=1.0, uniforms=u, timeout_ms=20000)

    def with_logits():
        idx, logits = eng.generate(n, first, want_logits=True, **kw)
        return idx, host_logp(idx, logits)

    legs = [("plain", lambda: (eng.generate(n, first, **kw), None)),
            ('logprobs="sampling"', lambda: eng.generate(n, first, logprobs="sampling", **kw)),
            ('logprobs="model"', lambda: eng.generate(n, first, logprobs="model", **kw)),
            ("want_logits + host log-softmax", with_logits)]
    out = {}
    for name, fn in legs:   # warm every leg: code objects, allocator
        fn()
        out[name] = fn()
    times = {name: [] for name, _ in legs}
    for _ in range(rounds):
        for name, fn in legs:
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            fn()
            times[name].append(time.perf_counter() - t0)
    info = eng.info()
    print("%s x %d, %d samples, %d alternating rounds (variant %d, %d streams per item, %d slots, %d sampler workgroups)" % (
        cfgname, ns, n, rounds, info["kernel_variant"], info["streams_per_item"], info["skip_lane_slots"], info["n_samplers"]))
    base = float(np.median(times["plain"]))
    for name, _ in legs:
        t = np.array(times[name]) * 1e3
        print("    %-32s median %9.2f ms  (%.2f - %.2f)   %10.0f samples/s   x %.3f of plain" % (
            name, np.median(t), t.min(), t.max(), ns * n / (np.median(t) * 1e-3), np.median(t) * 1e-3 / base))
    same = all(np.array_equal(out[name][0], out["plain"][0]) for name, _ in legs)
    dev = float(np.abs(out['logprobs="model"'][1] - out["want_logits + host log-softmax"][1]).max())
    print("    same indices in all legs: %s;  max |model-mode logp - host log-softmax of the dump| = %.3g" % (same, dev))
    eng.close()


def main():
    assert torch.cuda.is_available(), "bench_logprobs needs the MI355X"
    n, rounds = _opt("samples", 1600), max(7, _opt("rounds", 9))
    for job in _opt("jobs", "cfg3 1;cfg3 64;cfg1 1").split(";"):
        name, ns = job.split()
        bench(name, int(ns), n, rounds)


if __name__ == "__main__":
    main()
