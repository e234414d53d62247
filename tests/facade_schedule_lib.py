"""TEST INFRASTRUCTURE for the facade's piece schedule (wavenet_model.WaveNetModel.generate_fast -> mi355_wavenet/generation.py): a fake engine put in
place of ``mi355_wavenet.engine.Engine`` -- the facade's only door to the engine -- that records the ``prime_host``, ``generate`` and ``upload_uniforms``
calls and returns zeros; the reference's generate_fast loop (wavenet_model.py:259-311) restated as a trace of callbacks, timing print and RNG
consumption; the same trace taken from the facade and from the pure schedule's steps; and the recorder of the call-log fixture
(tests/golden/facade_pieces_v1.json, written by tests/golden/make_facade_pieces.py).  Nothing here knows how the facade is built inside."""
import contextlib
import hashlib
import itertools
import json
import zlib

import numpy as np
import torch

import wavenet_model
from mi355_wavenet import engine, synth

_REAL_ENGINE = engine.Engine
SEED = 11

# the grid of the schedule tests: 8 x 7 x 6 x 2 x 2 x 2 = 2688 cases
NUM_GIVEN = (1, 2, 5, 64, 65, 66, 70, 101)
NUM_SAMPLES = (0, 1, 7, 99, 100, 101, 130)
INTERVALS = (1, 3, 10, 50, 100, 1000)


def grid():
    """(num_given, num_samples, interval, has_callback, sampled, batched priming accepted)"""
    return list(itertools.product(NUM_GIVEN, NUM_SAMPLES, INTERVALS, (True, False), (True, False), (True, False)))


class _Has:
    path = "<fake>"

    def has(self, name):
        return True


class _Resident:
    def __init__(self, shape):
        self.shape = tuple(shape)


class FakeEngine:
    """What the facade asks of an Engine, computing nothing.  ``log`` and ``accept_prime`` live on the class install() made."""
    PRIME_BATCH_MIN = _REAL_ENGINE.PRIME_BATCH_MIN
    log = None
    accept_prime = True

    def __init__(self, cfg, weights, n_streams=1, device_index=0, **kw):
        self.cfg, self.n_streams, self.classes, self.lib = dict(cfg), int(n_streams), int(cfg.get("classes", 256)), _Has()

    def close(self):
        pass

    def load_weights(self, weights):
        pass

    def reset(self):
        pass

    def set_sampling(self, top_k=0, top_p=0.0):
        pass

    def state_load(self, state, stream_first=0, stream_count=None):
        pass

    def state_save(self, stream=0):
        return np.zeros(1, np.float32)

    def export_queue(self, layer, stream=0):
        d = 2 ** (layer % self.cfg["layers"])
        return np.zeros((self.cfg["residual_channels"], d + 1), np.float32), 0, 0

    def prime_host(self, first_samples):
        self.log.append(["prime_host", list(np.shape(first_samples))])
        return bool(self.accept_prime)

    def upload_uniforms(self, u):
        self.log.append(["upload_uniforms", list(np.shape(u))])
        return _Resident(np.shape(u))

    def generate(self, num_samples, first_samples=None, temperature=1.0, regularize=0.0, uniforms=None, reset=True, while_running=None,
                 logprobs=None, forced=None, **kw):
        resident = isinstance(uniforms, _Resident)
        self.log.append(["generate", int(num_samples), int(np.shape(first_samples)[-1]),
                         None if uniforms is None else list(uniforms.shape), resident,
                         None if forced is None else list(np.shape(forced)) + [int(np.asarray(forced).reshape(-1)[0])], logprobs])
        if while_running is not None:
            while_running()
        out = np.zeros((self.n_streams, num_samples), np.int32)
        return out if logprobs is None else (out, np.zeros((self.n_streams, num_samples), np.float32))


def install(monkeypatch):
    """-> (a tiny model whose engines are FakeEngines, the fake class: its ``log`` list and its ``accept_prime`` switch)"""
    fake = type("FakeEngineInstalled", (FakeEngine,), {"log": [], "accept_prime": True})
    monkeypatch.setattr(engine, "Engine", fake)
    return wavenet_model.WaveNetModel(output_length=8, **synth.CONFIGS["tiny"]), fake


def _rng_mark():
    st = np.random.get_state()
    return [zlib.crc32(st[1].tobytes()), int(st[2])]


def reference_trace(num_given, num_samples, interval, has_callback, sampled):
    """What a caller of the reference's generate_fast can observe of its control flow (wavenet_model.py:259-311), with the model left out: the priming
    callbacks, one random_sample per generated sample when sampled (np.random.choice, :288), the timing print behind generating sample 100, then the
    generation callback; every callback with the RNG's state at that moment, and the final RNG state last."""
    np.random.seed(SEED)
    total = num_given + num_samples
    trace = []
    for i in range(num_given - 1):
        if i % interval == 0 and has_callback:
            trace.append(["callback", i, total, _rng_mark()])
    for i in range(num_samples):
        if sampled:
            np.random.random_sample()
        if i + 1 == 100:
            trace.append(["print"])
        if (i + num_given) % interval == 0 and has_callback:
            trace.append(["callback", i + num_given, total, _rng_mark()])
    trace.append(["end", _rng_mark()])
    return trace


class _PrintsInto:
    """stdout that puts the timing line into the trace, where it happened"""
    def __init__(self, trace):
        self.trace = trace

    def write(self, text):
        if text.startswith("one generating step does take approximately"):
            self.trace.append(["print"])

    def flush(self):
        pass


def facade_trace(model, fake, num_given, num_samples, interval, has_callback, sampled, accept_prime, streams=0, **kw):
    """The same trace from generate_fast on the fake engine (streams > 0: a 2-D prompt of that many rows).  The fake's log is left for the caller."""
    fake.accept_prime = accept_prime
    del fake.log[:]
    np.random.seed(SEED)
    trace = []
    first = torch.zeros((streams, num_given) if streams else (num_given,), dtype=torch.int64)
    with contextlib.redirect_stdout(_PrintsInto(trace)):
        model.generate_fast(num_samples, first_samples=first, temperature=1.0 if sampled else 0., progress_interval=interval,
                            progress_callback=(lambda i, total: trace.append(["callback", i, total, _rng_mark()])) if has_callback else None, **kw)
    trace.append(["end", _rng_mark()])
    return trace


def schedule_trace(steps, num_given, num_samples, n_streams=1):
    """The same trace from the pure schedule's steps alone (mi355_wavenet/generation.py): a piece consumes the RNG as the executor does for it."""
    from mi355_wavenet import generation
    np.random.seed(SEED)
    trace = []
    for st in steps:
        if isinstance(st, generation.Piece):
            for n in (st.draw, st.draw_ahead):
                if n:
                    np.random.random_sample((n_streams, n))
        elif isinstance(st, generation.Callback):
            trace.append(["callback", st.i, num_given + num_samples, _rng_mark()])
        else:
            trace.append(["print"])
    trace.append(["end", _rng_mark()])
    return trace


# ---------------------------------------------------------------- the call-log fixture
FIXTURE = "facade_pieces_v1.json"
_SUBSET = list(itertools.product((1, 66), NUM_SAMPLES, (3, 100), (True, False), (True,), (True, False)))
_FULL_LOGS = list(itertools.product((5, 70), (7, 130), (10,), (True, False), (True,), (True, False)))


def forced_for(num_samples, rows=None):
    """forced[s, g] = g + s: the first value of a slice says where it was cut"""
    g = np.arange(num_samples, dtype=np.int64)
    return g if rows is None else g[None, :] + np.arange(rows)[:, None]


def piece_cases():
    """[(key, case, streams, generate_fast keywords)]: the grid on one stream; a subset on three streams; the subset with log-probabilities and, where
    something is generated, forced samples -- 1-D on one stream, per row on three"""
    cases = [("grid", c, 0, {}) for c in grid()]
    cases += [("streams3", c, 3, {}) for c in _SUBSET]
    for c in _SUBSET:
        cases.append(("forced_logp", c, 0, dict(return_logprobs=True, **({"forced": forced_for(c[1])} if c[1] else {}))))
        cases.append(("forced_rows3", c, 3, dict(return_logprobs="model", **({"forced": forced_for(c[1], 3)} if c[1] else {}))))
    return cases


def piece_log(model, fake, case, streams, kw):
    facade_trace(model, fake, *case, streams=streams, **kw)
    return [list(e) for e in fake.log]


def digest(log):
    return hashlib.sha1(json.dumps(log).encode()).hexdigest()[:8]


def record_pieces(model, fake):
    """-> the fixture: one digest per case in piece_cases() order, and the full logs of a few dozen grid cases to read"""
    logs = [piece_log(model, fake, case, streams, kw) for _, case, streams, kw in piece_cases()]
    full = {json.dumps(c): piece_log(model, fake, c, 0, {}) for c in _FULL_LOGS}
    return {"cases": len(logs), "digests": " ".join(digest(l) for l in logs), "full": full}
