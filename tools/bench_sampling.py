"""dev tool: what the sampling filters (wn_set_sampling) cost -- job rates with alternating legs in ONE process, and the samplers alone.

    python tools/bench_sampling.py [--samples 4000] [--rounds 5] [--jobs "cfg3 1;cfg3 64"] [--filter 40,0.95] [--samplers 8] [--other-lib PATH] [--kernels]

Jobs: per (config, streams) one engine; every round runs the legs one after the other -- filter off, filter on, and with --other-lib the unfiltered job
on another build of the library (the parent commit's, for the "unfiltered legs did not move" comparison) -- and the table gives median and min - max of
the rounds in samples/s.  --samplers N adds the same legs on an engine planned with WN_SAMPLERS=N (multi-stream jobs: the sampler workgroups may be what
a filtered job waits for).  --kernels: the two samplers alone through tests/kernels/libwn_kernel_harness.so (one draw per workgroup), time of a
launch of 4096 rows and of 64 rows, filter off / top_k / top_p / both, HIP events, median of 20."""
import argparse
import os
import statistics
import sys
import time

os.environ.setdefault("WN_TESTING", "1")  # dev tool: the WN_SAMPLERS pin is honoured
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "pytorch-wavenet_amd"))
import numpy as np  # noqa: E402
import torch  # noqa: E402

from mi355_wavenet import _abi, engine, synth  # noqa: E402


def _job(eng, first, uni, out, ns, n):
    eng.reset()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    eng.launch(first, 1, n, 1.0, None, uni, out, None, timeout_ms=30000)
    eng.wait()
    return ns * n / (time.perf_counter() - t0)


def _fmt(v):
    return "median %10.0f  min %10.0f  max %10.0f samples/s" % (statistics.median(v), min(v), max(v))


def bench_jobs(args):
    top_k, top_p = args.filter
    other = _abi.Library(os.path.abspath(args.other_lib)) if args.other_lib else None
    for job in args.jobs.split(";"):
        cfgname, ns = job.split()
        ns = int(ns)
        cfg, n = synth.CONFIGS[cfgname], args.samples
        W = synth.init_weights(cfg, seed=0)
        plans = [None] + ([args.samplers] if args.samplers and ns > 1 else [])
        for n_smp in plans:
            if n_smp:
                os.environ["WN_SAMPLERS"] = str(n_smp)
            engines = {"this": engine.Engine(cfg, W, n_streams=ns)}
            if other is not None:
                engines["other"] = engine.Engine(cfg, W, n_streams=ns, lib=other)
            os.environ.pop("WN_SAMPLERS", None)
            mem = engines["this"].mem
            first = mem.upload(np.full((ns, 1), 128, dtype=np.int32))
            uni = mem.upload(np.random.RandomState(1).random_sample((ns, n)))
            out = mem.empty((ns, n), np.int32)
            legs = [("off", "this", (0, 0.0)), ("(%d, %g)" % (top_k, top_p), "this", (top_k, top_p))] + ([("off, other library", "other", None)] if other else [])
            rates = {name: [] for name, _, _ in legs}
            for rnd in range(args.rounds + 1):          # (round 0 warms up)
                for name, which, filt in legs[rnd % len(legs):] + legs[:rnd % len(legs)]:   # (every leg runs behind every other one)
                    eng = engines[which]
                    if filt is not None:
                        eng.set_sampling(*filt)
                    r = _job(eng, first, uni, out, ns, n)
                    if rnd:
                        rates[name].append(r)
            info = engines["this"].info()
            print("%s x %d, %d samples, %d rounds (variant %d, %d sampler workgroups)" % (cfgname, ns, n, args.rounds, info["kernel_variant"], info["n_samplers"]))
            for name, _, _ in legs:
                print("    %-22s %s   (%.2f us per timestep)" % (name, _fmt(rates[name]), 1e6 * ns / statistics.median(rates[name])))
            for e in engines.values():
                e.set_sampling(0, 0.0)
                e.close()


def bench_kernels(args):
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    import kernel_lib
    kf = kernel_lib.build_and_load().dll
    rs = np.random.RandomState(2)
    dev = torch.device("cuda", 0)
    stream = torch.cuda.current_stream(dev).cuda_stream
    for rows in (4096, 64):
        logits = torch.from_numpy((rs.standard_normal((rows, 256)) * 3).astype(np.float32)).to(dev)
        u = torch.from_numpy(rs.random_sample(rows)).to(dev)
        greedy = torch.zeros(rows, dtype=torch.int32, device=dev)
        temp = torch.full((rows,), 0.8, dtype=torch.float32, device=dev)
        out = torch.empty(rows * 64, dtype=torch.int32, device=dev)
        tail = torch.empty(rows * 64, dtype=torch.int32, device=dev)

        def timed(fn):
            ts = []
            for _ in range(23):
                a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                a.record()
                fn()
                b.record()
                b.synchronize()
                ts.append(a.elapsed_time(b) * 1e3)
            return statistics.median(ts[3:]), min(ts[3:]), max(ts[3:])

        print("samplers alone, %d rows (one draw per workgroup), us per launch: median (min - max)" % rows)
        for name, form, k, p in (("wn_sample_1w<false>", 0, 0, 0.0), ("wn_sample_1w<true> off", 1, 0, 0.0), ("wn_sample_1w<true> top_k 40", 1, 40, 0.0),
                                 ("wn_sample_1w<true> top_p .95", 1, 0, 0.95), ("wn_sample_1w<true> (40, .95)", 1, 40, 0.95)):
            m = timed(lambda: kf.kf_sample_1w(stream, form, rows, k, p, logits.data_ptr(), None, u.data_ptr(), greedy.data_ptr(), temp.data_ptr(), out.data_ptr()))
            print("    %-30s %8.1f (%.1f - %.1f)" % ((name,) + m))
        for name, k, p in (("wn_sample off", 0, 0.0), ("wn_sample top_k 40", 40, 0.0), ("wn_sample top_p .95", 0, 0.95), ("wn_sample (40, .95)", 40, 0.95)):
            m = timed(lambda: kf.kf_sample_generic(stream, rows, 256, k, p, logits.data_ptr(), None, u.data_ptr(), greedy.data_ptr(), temp.data_ptr(), out.data_ptr(),
                                                   tail.data_ptr()))
            print("    %-30s %8.1f (%.1f - %.1f)" % ((name,) + m))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--samples", type=int, default=4000)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--jobs", default="cfg3 1;cfg3 64")
    ap.add_argument("--filter", default="40,0.95", type=lambda s: (int(s.split(",")[0]), float(s.split(",")[1])))
    ap.add_argument("--samplers", type=int, default=0)
    ap.add_argument("--other-lib", default=None)
    ap.add_argument("--kernels", action="store_true")
    args = ap.parse_args()
    if args.kernels:
        bench_kernels(args)
    else:
        bench_jobs(args)


if __name__ == "__main__":
    main()
