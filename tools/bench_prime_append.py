"""Times batched priming onto a live state: (a) wn_prime_append on queues that hold a history against wn_prime_ragged over the same lengths from
reset -- the price of the history gather and the full ring fill --, (b) the whole generate_fast(samples, continue_from=states, append=rows) call
against the recipe it replaces (the rows as a forced prefix: one chain evaluation per forced position), (c) the workspace and the time of priming
one long prompt per stream in one pass and in pieces (WaveNetModel.prime_piece_samples).  Same weights, same rows, same GPU; the legs of (a) and (b)
alternate round by round in one process.  (a) is device events around the priming call on resident arguments (the ragged leg's wn_reset stands in
front of its events), (b) and (c) are wall clock around the call.  Printed as median (min - max) over the rounds.

    python tools/bench_prime_append.py [--part=abc] [--config=cfg3] [--streams=64] [--shortest=64] [--longest=5115] [--samples=1600] [--rounds=9] [--seed=24]

--part=f runs the forced-prefix recipe alone; it uses nothing this feature added, so the same file measures it on a tree without wn_prime_append.
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


def _model(cfg, W):
    m = wavenet_model.WaveNetModel(output_length=16, **cfg)
    m.load_state_dict({k: torch.from_numpy(v) for k, v in W.items()})
    return m


def _wall(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3


def part_a(cfg, W, ns, lengths, rows, rounds, samples):
    n, NL = int(lengths.max()), cfg["layers"] * cfg["blocks"]
    ragged_launches = 3 + NL + 2 * (NL - 1)
    print("(a) launches per pass: wn_prime_ragged %d (1 clear, 1 table upload, 1 start gather, %d ring fills, %d products); wn_prime_append %d (the same and "
          "%d history gathers)" % (ragged_launches, NL, 2 * (NL - 1), ragged_launches + NL, NL))
    matrix = np.zeros((ns, n), np.int32)
    for s, r in enumerate(rows):
        matrix[s, :r.size] = r
    c_lengths = (ctypes.c_int64 * ns)(*[int(v) for v in lengths])
    fresh, live = engine.Engine(cfg, W, n_streams=ns), engine.Engine(cfg, W, n_streams=ns)
    assert fresh.lib.has("wn_prime_ragged") and live.lib.has("wn_prime_append")   # (has() also binds the argument types: the raw calls below pass 64-bit pointers)
    rs = np.random.RandomState(5)
    live.generate(samples, rs.randint(0, 256, (ns, 1)), temperature=1.0, uniforms=rs.random_sample((ns, samples)))   # the states come from a job
    dev_f, dev_l = fresh.mem.upload(matrix), live.mem.upload(matrix)

    def ragged():
        fresh.lib.check(fresh.lib.dll.wn_prime_ragged(fresh._h, dev_f.data_ptr(), c_lengths, n, fresh.mem.stream()))

    def append():   # (every call appends to what the call before left: the queue time grows, the work does not)
        live.lib.check(live.lib.dll.wn_prime_append(live._h, dev_l.data_ptr(), c_lengths, n, 0, live.mem.stream()))
    legs = [("wn_prime_ragged from reset", ragged, fresh.reset), ("wn_prime_append at queue time >= %d" % samples, append, lambda: None)]
    for _, fn, before in legs:
        for _ in range(2):
            before()
            fn()
    torch.cuda.synchronize()
    times = {label: [] for label, _, _ in legs}
    for _ in range(rounds):
        for label, fn, before in legs:
            before()
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            fn()
            b.record()
            torch.cuda.synchronize()
            times[label].append(a.elapsed_time(b))
    for label, _, _ in legs:
        print("  %-42s %s" % (label, _fmt(times[label])))
    r, a = times[legs[0][0]], times[legs[1][0]]
    state_mb = live.state_floats() * 4 / 1e6
    print("  append / ragged = %.3f; ragged's own spread %.3f ms, the difference of the medians %.3f ms; gather and fill move about 2 x %.1f MB per stream, "
          "%.0f MB for %d streams" % (float(np.median(a)) / float(np.median(r)), max(r) - min(r), float(np.median(a)) - float(np.median(r)), state_mb,
                                     2 * state_mb * ns, ns))
    fresh.close()
    live.close()


def _checkpoint(m, ns, samples):
    np.random.seed(2)
    first = torch.from_numpy(np.random.RandomState(6).randint(0, 256, (ns, 1)))
    return m.generate_fast(samples, first_samples=first, return_state=True)[1]


def part_forced(cfg, W, ns, lengths, rows, rounds, samples):
    """the recipe without append=: every row as a forced prefix of a job of longest + samples positions from the checkpoint"""
    m = _model(cfg, W)
    states = _checkpoint(m, ns, samples)
    n = int(lengths.max())
    forced = np.full((ns, n + samples), -1, np.int64)
    for s, r in enumerate(rows):
        forced[s, :r.size] = r

    def call():
        np.random.seed(3)
        return m.generate_fast(n + samples, continue_from=states, forced=forced)
    call()
    times = [_wall(call) for _ in range(rounds)]
    print("(b) generate_fast(%d + %d, continue_from=, forced=): the rows as forced prefixes   %s" % (n, samples, _fmt(times)))
    return float(np.median(times))


def part_b(cfg, W, ns, lengths, rows, rounds, samples):
    m = _model(cfg, W)
    states = _checkpoint(m, ns, samples)

    def call():
        np.random.seed(3)
        return m.generate_fast(samples, continue_from=states, append=rows)
    call()
    assert m._wn_last_prime_batched is True
    times = [_wall(call) for _ in range(rounds)]
    print("(b) generate_fast(%d, continue_from=, append=): one batched pass                    %s" % (samples, _fmt(times)))
    return float(np.median(times))


def part_c(cfg, W, ns, longest, rounds):
    R, D = cfg["residual_channels"], cfg["dilation_channels"]
    d_max = (cfg["kernel_size"] - 1) * 2 ** (cfg["layers"] - 1)
    first = torch.from_numpy(np.random.RandomState(8).randint(0, 256, (ns, longest + 1)))
    want = None
    for p in (None, 1024, 256):
        m = _model(cfg, W)
        m.prime_piece_samples = p
        m._engine(ns)   # (the engine's own memory is taken before the call that is measured)

        def call():
            return m.generate_fast(0, first_samples=first, return_state=True)[1]
        took = _took(call)
        times = [_wall(call) for _ in range(rounds)]
        state = call()[0].state
        want = state if want is None else want
        piece = longest if p is None else min(p, longest)
        print("(c) %d streams x %d given samples, prime_piece_samples = %-5s workspace by formula %7.1f MB, taken on the first call %7.1f MB;  %s;  "
              "stream 0's state %s" % (ns, longest, p, 4 * (2 * ns * (piece + d_max) * R + ns * piece * D) / 1e6, took / 1e6, _fmt(times),
                                     "is the one pass's, bit for bit" if state.tobytes() == want.tobytes() else "DIFFERS from the one pass's"))
        m._wn_engine.close()
        m._wn_engine = None
        torch.cuda.empty_cache()


def main():
    assert torch.cuda.is_available(), "bench_prime_append needs the MI355X"
    name, ns, lo, hi = _opt("config", "cfg3"), _opt("streams", 64), _opt("shortest", 64), _opt("longest", 5115)
    samples, rounds, seed, parts = _opt("samples", 1600), max(9, _opt("rounds", 9)), _opt("seed", 24), _opt("part", "abc")
    cfg = synth.CONFIGS[name]
    W = synth.init_weights(cfg, seed=7)
    rs = np.random.RandomState(seed)
    lengths = rs.randint(lo, hi + 1, ns).astype(np.int64)
    rows = [rs.randint(0, 256, int(v)).astype(np.int64) for v in lengths]
    print("%s, %d streams, append lengths uniform in [%d, %d] (seed %d): shortest %d, longest %d, sum %d = %.3f of streams x longest; states from a "
          "%d-sample job; %d rounds" % (name, ns, lo, hi, seed, lengths.min(), lengths.max(), lengths.sum(), float(lengths.sum()) / (ns * lengths.max()),
                                         samples, rounds))
    if "a" in parts:
        part_a(cfg, W, ns, lengths, rows, rounds, samples)
    forced = part_forced(cfg, W, ns, lengths, rows, rounds, samples) if "f" in parts else None
    if "b" in parts:
        whole = part_b(cfg, W, ns, lengths, rows, rounds, samples)
        if forced is not None:
            print("  forced prefixes / append = x %.2f" % (forced / whole))
    if "c" in parts:
        part_c(cfg, W, ns, hi, rounds)


if __name__ == "__main__":
    main()
