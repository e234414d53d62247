"""Times the priming of prompts of unequal length: wn_prime_ragged over the streams' own rows against what the library could do before it -- wn_prime
with every row at the longest length (n_streams * max rows) -- and the whole generate_fast() call for a list of prompts against the recipe it
replaces (the common prefix as first_samples, the rest of every prompt as a forced prefix: one chain evaluation per forced position).  Same weights,
same prompts, same GPU, the legs alternating round by round in one process.  The priming legs are device events around wn_reset + the priming call on
resident arguments; the facade legs are wall clock around the call.  Printed as median (min - max) over the rounds, with the launches of both passes
(counted from the layer count), the workspace by its formula and the device memory the first call took.

    python tools/bench_ragged_prime.py [--config=cfg3] [--streams=64] [--shortest=64] [--longest=5115] [--samples=1600] [--rounds=9] [--seed=24]

Needs an MI355X: there is no CPU leg.  WN_TESTING is not needed.
"""
import ctypes
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "pytorch-wavenet_amd"))
import numpy as np  # noqa: E402
import torch  # noqa: E402

import wavenet_model  # noqa: E402
from mi355_wavenet import engine, synth  # noqa: E402


def _opt(name, default):
    vals = [a.split("=", 1)[1] for a in sys.argv[1:] if a.startswith("--%s=" % name)]
    return type(default)(vals[0]) if vals else default


def _fmt(t):
    t = np.array(t)
    return "median %9.3f ms  (%.3f - %.3f)" % (float(np.median(t)), t.min(), t.max())


def _took(fn):
    """device memory the call took (the workspace it grew): bytes, by the driver's free-memory figure"""
    torch.cuda.synchronize()
    free0 = torch.cuda.mem_get_info()[0]
    fn()
    torch.cuda.synchronize()
    return free0 - torch.cuda.mem_get_info()[0]


def main():
    assert torch.cuda.is_available(), "bench_ragged_prime needs the MI355X"
    name, ns, lo, hi = _opt("config", "cfg3"), _opt("streams", 64), _opt("shortest", 64), _opt("longest", 5115)
    samples, rounds, seed = _opt("samples", 1600), max(7, _opt("rounds", 9)), _opt("seed", 24)
    cfg = synth.CONFIGS[name]
    W = synth.init_weights(cfg, seed=7)
    rs = np.random.RandomState(seed)
    lengths = rs.randint(lo, hi + 1, ns).astype(np.int64)   # priming evaluations per stream: the prompts are one sample longer
    prompts = [rs.randint(0, 256, int(v) + 1).astype(np.int64) for v in lengths]
    n, R, D, NL = int(lengths.max()), cfg["residual_channels"], cfg["dilation_channels"], cfg["layers"] * cfg["blocks"]
    d_max = (cfg["kernel_size"] - 1) * 2 ** (cfg["layers"] - 1)
    share = float(lengths.sum()) / (ns * n)
    print("%s, %d streams, priming lengths uniform in [%d, %d] (seed %d): shortest %d, longest %d, sum %d = %.3f of streams x longest; %d generated "
          "samples; %d alternating rounds" % (name, ns, lo, hi, seed, lengths.min(), n, lengths.sum(), share, samples, rounds))
    print("launches per pass: wn_prime_ragged %d (1 clear, 1 table upload, 1 start gather, %d ring fills, %d products) against wn_prime %d (1 clear, %d start "
          "gathers, %d ring fills, %d products)" % (3 + NL + 2 * (NL - 1), NL, 2 * (NL - 1), 1 + ns + NL + 2 * (NL - 1), ns, NL, 2 * (NL - 1)))
    matrix = np.zeros((ns, n), np.int32)    # left-aligned rows for wn_prime_ragged
    full = rs.randint(0, 256, (ns, n)).astype(np.int32)   # every row at the longest length: what wn_prime needs
    for s, p in enumerate(prompts):
        matrix[s, :lengths[s]] = p[:-1]
    c_lengths = (ctypes.c_int64 * ns)(*[int(v) for v in lengths])
    took = {}
    for leg in ("wn_prime", "wn_prime_ragged"):   # a fresh engine per leg: its first call grows the workspace
        eng = engine.Engine(cfg, W, n_streams=ns)
        assert eng.lib.has("wn_prime_ragged")
        dev = eng.mem.upload(full if leg == "wn_prime" else matrix)
        eng.reset()
        if leg == "wn_prime":
            took[leg] = _took(lambda: eng.lib.check(eng.lib.dll.wn_prime(eng._h, dev.data_ptr(), n, n, eng.mem.stream())))
        else:
            took[leg] = _took(lambda: eng.lib.check(eng.lib.dll.wn_prime_ragged(eng._h, dev.data_ptr(), c_lengths, n, eng.mem.stream())))
        eng.close()
        del dev
        torch.cuda.empty_cache()
    eng = engine.Engine(cfg, W, n_streams=ns)
    full_dev, matrix_dev = eng.mem.upload(full), eng.mem.upload(matrix)
    dll, h = eng.lib.dll, eng._h

    def rectangle():
        eng.reset()
        eng.lib.check(dll.wn_prime(h, full_dev.data_ptr(), n, n, eng.mem.stream()))

    def ragged():
        eng.reset()
        eng.lib.check(dll.wn_prime_ragged(h, matrix_dev.data_ptr(), c_lengths, n, eng.mem.stream()))

    m = wavenet_model.WaveNetModel(output_length=16, **cfg)
    m.load_state_dict({k: torch.from_numpy(v) for k, v in W.items()})
    common = int(lengths.min()) + 1   # the recipe: the prompts' first `common` samples as first_samples, the rest of each as a forced prefix
    rest = n + 1 - common
    forced = np.full((ns, rest + samples), -1, np.int64)
    for s, p in enumerate(prompts):
        forced[s, :p.size - common] = p[common:]
    prefix = torch.from_numpy(np.stack([p[:common] for p in prompts]))

    def facade_ragged():
        np.random.seed(3)
        return m.generate_fast(samples, first_samples=prompts)

    def facade_forced():   # every stream's `samples` free positions lie behind its own forced prefix: the job runs rest + samples positions
        np.random.seed(3)
        return m.generate_fast(rest + samples, first_samples=prefix, forced=forced)

    legs = [("(b) wn_prime, rows at the longest", rectangle, True), ("(a) wn_prime_ragged", ragged, True),
            ("(c) generate_fast, forced prefixes", facade_forced, False), ("(c) generate_fast, list of prompts", facade_ragged, False)]
    for _, fn, _ in legs:   # warm every leg: workspaces, code objects, the facade's engine
        fn()
        fn()
    torch.cuda.synchronize()
    assert m._wn_last_prime_batched is True
    times = {label: [] for label, _, _ in legs}
    for _ in range(rounds):
        for label, fn, on_device in legs:
            if on_device:
                a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                a.record()
                fn()
                b.record()
                torch.cuda.synchronize()
                times[label].append(a.elapsed_time(b))
            else:
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                fn()
                times[label].append((time.perf_counter() - t0) * 1e3)
    for label, _, _ in legs:
        print("  %-38s %s" % (label, _fmt(times[label])))
    med = {label: float(np.median(times[label])) for label, _, _ in legs}
    a, b = med[legs[1][0]], med[legs[0][0]]
    spread = max(times[legs[0][0]]) - min(times[legs[0][0]])
    print("  (a) / (b) = %.3f (rows: %.3f);  (a) %s slower than (b) beyond the spread of (b)'s rounds (%.3f ms);  whole call x %.2f" % (
        a / b, share, "IS" if a > b + spread else "is not", spread, med[legs[2][0]] / med[legs[3][0]]))
    formula = 4 * (2 * ns * (n + d_max) * R + ns * n * D)
    print("  workspace (the right-aligned rectangle of both passes) by formula %.1f MB; taken on the first call %.1f MB (wn_prime) / %.1f MB (wn_prime_ragged)" % (
        formula / 1e6, took["wn_prime"] / 1e6, took["wn_prime_ragged"] / 1e6))
    eng.close()


if __name__ == "__main__":
    main()
