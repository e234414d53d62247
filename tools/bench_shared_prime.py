"""Times the priming of a prompt that all streams share: wn_prime over the prompt repeated once per stream (what generate_fast_streams did before
shared priming) against wn_prime_shared over the one row, and the whole generate_fast_streams() call on both paths -- same weights, same prompt, same
GPU, the legs alternating round by round in one process.  The priming legs are device events around wn_reset + the priming call on resident
arguments; the facade legs are wall clock around the call (upload, priming, the generation job, download).  Printed as median (min - max) over the
rounds.  Workspace: the priming workspace by its formula, 2 rows (n + d_max) R + rows n D floats, and the device memory the first call took.

    python tools/bench_shared_prime.py [--config=cfg3] [--given=5116] [--samples=1600] [--streams=1,8,64] [--rounds=9]

Needs an MI355X: there is no CPU leg.  WN_TESTING is not needed.
"""
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
    assert torch.cuda.is_available(), "bench_shared_prime needs the MI355X"
    name, given, samples, rounds = _opt("config", "cfg3"), _opt("given", 5116), _opt("samples", 1600), max(7, _opt("rounds", 9))
    streams = [int(s) for s in _opt("streams", "1,8,64").split(",")]
    cfg = synth.CONFIGS[name]
    W = synth.init_weights(cfg, seed=7)
    prompt = np.random.RandomState(7).randint(0, 256, given).astype(np.int32)
    n, R, D = given - 1, cfg["residual_channels"], cfg["dilation_channels"]
    d_max = (cfg["kernel_size"] - 1) * 2 ** (cfg["layers"] - 1)
    print("%s, prompt of %d given samples (%d priming evaluations), %d generated samples; %d alternating rounds" % (name, given, n, samples, rounds))
    m = wavenet_model.WaveNetModel(output_length=16, **cfg)
    m.load_state_dict({k: torch.from_numpy(v) for k, v in W.items()})
    for ns in streams:
        def formula(rows):
            return 4 * (2 * rows * (n + d_max) * R + rows * n * D)
        took = {}
        for leg in ("wn_prime", "wn_prime_shared"):   # a fresh engine per leg: its first call grows the workspace
            eng = engine.Engine(cfg, W, n_streams=ns)
            dev = eng.mem.upload(np.repeat(prompt[None, :n], ns, axis=0) if leg == "wn_prime" else prompt[:n])
            eng.reset()
            if leg == "wn_prime":
                took[leg] = _took(lambda: eng.lib.check(eng.lib.dll.wn_prime(eng._h, dev.data_ptr(), n, n, eng.mem.stream())))
            else:
                prime_shared = eng._need("wn_prime_shared", eng._STATE_SINCE)   # (looked up and bound on first use: _abi.LAZY_EXPORTS)
                took[leg] = _took(lambda: eng.lib.check(prime_shared(eng._h, dev.data_ptr(), n, eng.mem.stream())))
            eng.close()
            del dev
            torch.cuda.empty_cache()
        eng = engine.Engine(cfg, W, n_streams=ns)
        rows_dev, row_dev = eng.mem.upload(np.repeat(prompt[None, :n], ns, axis=0)), eng.mem.upload(prompt[:n])
        dll, h, prime_shared = eng.lib.dll, eng._h, eng._need("wn_prime_shared", eng._STATE_SINCE)

        def per_stream():
            eng.reset()
            eng.lib.check(dll.wn_prime(h, rows_dev.data_ptr(), n, n, eng.mem.stream()))

        def shared():
            eng.reset()
            eng.lib.check(prime_shared(h, row_dev.data_ptr(), n, eng.mem.stream()))

        temps = [1.0] * ns
        first = torch.from_numpy(prompt.astype(np.int64))

        def facade(flag):
            def run():
                m.SHARED_PRIME = flag
                np.random.seed(3)
                return m.generate_fast_streams(samples, temps, first_samples=first)
            return run

        legs = [("wn_prime, repeated rows", per_stream, True), ("wn_prime_shared", shared, True),
                ("generate_fast_streams, wn_prime", facade(False), False), ("generate_fast_streams, shared", facade(True), False)]
        out = {}
        for label, fn, _ in legs:   # warm every leg: workspaces, code objects, the facade's engine
            fn()
            out[label] = fn()
        torch.cuda.synchronize()
        states = []
        for fn in (per_stream, shared):
            fn()
            states.append(eng.state_save(ns - 1))
        same = states[0].tobytes() == states[1].tobytes() and np.array_equal(out[legs[2][0]], out[legs[3][0]])
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
        print("%d stream%s (queues and audio of the two paths bit-equal: %s)" % (ns, "" if ns == 1 else "s", same))
        for label, _, _ in legs:
            print("  %-34s %s" % (label, _fmt(times[label])))
        med = {label: float(np.median(times[label])) for label, _, _ in legs}
        print("  priming x %.2f, whole call x %.2f;  workspace by formula %.1f MB against %.1f MB, taken on the first call %.1f MB against %.1f MB" % (
            med[legs[0][0]] / med[legs[1][0]], med[legs[2][0]] / med[legs[3][0]], formula(ns) / 1e6, formula(1) / 1e6,
            took["wn_prime"] / 1e6, took["wn_prime_shared"] / 1e6))
        eng.close()
        del rows_dev, row_dev
        torch.cuda.empty_cache()
    m.SHARED_PRIME = True


if __name__ == "__main__":
    main()
