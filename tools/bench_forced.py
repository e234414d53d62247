"""Times what forced samples cost a generation job (Engine.generate(..., forced=), C ABI wn_set_forced_samples): the same job
  unarmed                         -- the product instantiation;
  logprobs="model"                -- armed with log-probabilities alone: the cost of the instantiation the forced fork lives in;
  forced all free                 -- armed with forced samples, every entry -1: the instantiation plus one load per draw;
  forced all free + logprobs      -- both armings, nothing forced;
  every position forced + logprobs="model" -- what WaveNetModel.score_continuation runs (sampled here, so that the legs differ in the fork alone).
Same engine, same weights, same uniforms, the legs alternating round by round in one process; wall time around one synchronous generate() call (uploads,
launch, wait, downloads), after warm-up of every leg; printed as median (min - max) over the rounds.  WN_TESTING is taken out of the environment: the
planner chooses the kernel.

    python tools/bench_forced.py [--samples=1600] [--rounds=9] [--jobs="cfg3 64;cfg3 1;cfg1 1"]

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


def bench(cfgname, ns, n, rounds):
    cfg = synth.CONFIGS[cfgname]
    W = synth.init_weights(cfg, seed=7)
    rs = np.random.RandomState(11)
    first = rs.randint(0, 256, (ns, 1))
    u = rs.random_sample((ns, n))
    eng = engine.Engine(cfg, W, n_streams=ns)
    kw = dict(temperature=1.0, uniforms=u, timeout_ms=20000)
    free = np.full((ns, n), -1, np.int32)
    plain = eng.generate(n, first, **kw)
    every = plain.astype(np.int32)      # (forced to what the stream drew: the same trajectory, so the legs run the same arithmetic)

    legs = [("unarmed", lambda: (eng.generate(n, first, **kw), None)),
            ('logprobs="model"', lambda: eng.generate(n, first, logprobs="model", **kw)),
            ("forced all free", lambda: (eng.generate(n, first, forced=free, **kw), None)),
            ('forced all free + logprobs="model"', lambda: eng.generate(n, first, forced=free, logprobs="model", **kw)),
            ('every position forced + logprobs="model"', lambda: eng.generate(n, first, forced=every, logprobs="model", **kw))]
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
    base = float(np.median(times["unarmed"]))
    for name, _ in legs:
        t = np.array(times[name]) * 1e3
        print("    %-42s median %9.2f ms  (%.2f - %.2f)   %10.0f samples/s   x %.3f of unarmed" % (
            name, np.median(t), t.min(), t.max(), ns * n / (np.median(t) * 1e-3), np.median(t) * 1e-3 / base))
    same = all(np.array_equal(out[name][0], plain) for name, _ in legs)
    lp = [out[name][1] for name, _ in legs if out[name][1] is not None]
    print("    same indices in all legs: %s;  same log-probability bytes in the three legs that write them: %s" % (
        same, all(a.tobytes() == lp[0].tobytes() for a in lp)))
    eng.close()


def main():
    assert torch.cuda.is_available(), "bench_forced needs the MI355X"
    n, rounds = _opt("samples", 1600), max(7, _opt("rounds", 9))
    for job in _opt("jobs", "cfg3 64;cfg3 1;cfg1 1").split(";"):
        name, ns = job.split()
        bench(name, int(ns), n, rounds)


if __name__ == "__main__":
    main()
