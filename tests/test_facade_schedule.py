"""The facade's piece schedule (mi355_wavenet/generation.py) without a GPU: generate_fast on a fake engine against the reference's own loop, restated as a
trace (tests/facade_schedule_lib.py), over 2688 combinations of prompt length, sample count, callback interval, callback, sampling and batched priming;
the pure schedule against the same traces; the engine calls against a recording made before the schedule was pulled out of the facade; the schedule's
invariants; one end-to-end job on the test double against oracle/restated.py; and the one check of `forced` through both of its callers."""
import io
import json
import os
from contextlib import redirect_stdout

import numpy as np
import pytest
import torch

import facade_schedule_lib as fsl
import wavenet_model
from double_lib import double_backend
from mi355_wavenet import engine, generation, synth

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", fsl.FIXTURE)
_REAL_ENGINE = engine.Engine


def test_the_facade_follows_the_reference_loop(monkeypatch):
    model, fake = fsl.install(monkeypatch)
    cases = fsl.grid()
    assert len(cases) == 2688
    wrong = [c for c in cases if fsl.facade_trace(model, fake, *c) != fsl.reference_trace(*c[:5])]
    assert not wrong, "%d of %d cases, the first: %r" % (len(wrong), len(cases), wrong[:5])


def _steps(num_given, num_samples, interval, has_callback, sampled, accept_prime):
    n_prime = num_given - 1
    primed = n_prime if (accept_prime and n_prime >= engine.Engine.PRIME_BATCH_MIN) else 0
    return generation.generation_schedule(num_given, num_samples, interval, has_callback, primed, sampled), primed


def test_the_pure_schedule_follows_the_reference_loop():
    wrong = [c for c in fsl.grid() if fsl.schedule_trace(_steps(*c)[0], c[0], c[1]) != fsl.reference_trace(*c[:5])]
    assert not wrong, "%d cases, the first: %r" % (len(wrong), wrong[:5])
    steps, _ = _steps(70, 130, 16, True, True, False)      # three streams draw three rows per piece: other RNG states, the same events
    plain = [e[:3] for e in fsl.schedule_trace(steps, 70, 130, n_streams=3)[:-1]]
    assert plain == [e[:3] for e in fsl.reference_trace(70, 130, 16, True, True)[:-1]]


def test_the_pieces_are_those_recorded_before_the_schedule_was_pulled_out(monkeypatch):
    with open(GOLDEN) as f:
        gold = json.load(f)
    assert os.path.getsize(GOLDEN) < 100 * 1024
    model, fake = fsl.install(monkeypatch)
    cases = fsl.piece_cases()
    digests = gold["digests"].split()
    assert gold["cases"] == len(cases) == len(digests) and len(cases) > 2688 + 300
    wrong = [(key, c) for (key, c, streams, kw), d in zip(cases, digests) if fsl.digest(fsl.piece_log(model, fake, c, streams, kw)) != d]
    assert not wrong, "%d of %d cases, the first: %r" % (len(wrong), len(cases), wrong[:5])
    assert len(gold["full"]) >= 16
    for key, log in gold["full"].items():
        assert fsl.piece_log(model, fake, tuple(json.loads(key)), 0, {}) == log, key
    # the recording says what it is meant to pin: draw-ahead uploads, resident uniforms behind them, priming-only pieces, slices of `forced`
    log = fsl.piece_log(model, fake, (5, 130, 1000, False, True, True), 0, {"forced": fsl.forced_for(130), "return_logprobs": True})
    assert log == [["generate", 0, 5, None, False, None, None], ["upload_uniforms", [1, 100]],
                   ["generate", 100, 1, [1, 100], True, [1, 100, 0], "sampling"], ["upload_uniforms", [1, 30]],
                   ["generate", 30, 1, [1, 30], True, [1, 30, 100], "sampling"]], log


def test_schedule_invariants():
    for c in fsl.grid():
        num_given, num_samples, interval, has_callback, sampled, _ = c
        steps, primed = _steps(*c)
        n_prime, n_eval = num_given - 1, num_given - 1 + num_samples
        pieces = [s for s in steps if isinstance(s, generation.Piece)]
        at = primed
        for p in pieces:     # the pieces tile [primed, n_eval) without gap or overlap
            assert p.a == at and p.b > p.a and p.seg_prime + p.n_new == p.b - p.a and p.seg_prime == max(0, min(p.b, n_prime) - p.a), (c, p)
            assert p.from_prompt == (p.a <= n_prime), (c, p)
            at = p.b
        assert at == n_eval or (not pieces and n_eval == primed), c
        assert sum(p.n_new for p in pieces) == num_samples, c
        assert sum(p.draw + p.draw_ahead for p in pieces) == (num_samples if sampled else 0), c
        for k, st in enumerate(steps):     # a draw-ahead never sits at a cut with a callback due, and belongs to the next piece
            if isinstance(st, generation.Piece) and st.draw_ahead:
                nxt = [s for s in steps[k + 1:] if not isinstance(s, generation.TimingPrint)][0]
                assert isinstance(nxt, generation.Piece) and nxt.n_new == st.draw_ahead and nxt.draw == 0, (c, k)
        assert sum(isinstance(s, generation.TimingPrint) for s in steps) == (1 if num_samples >= 100 else 0), c
        assert sum(p.restart_clock for p in pieces) == (1 if num_samples > 0 else 0), c
        calls = [s.i for s in steps if isinstance(s, generation.Callback)]
        assert calls == sorted(set(calls)) and (has_callback or not calls), c
        if primed:     # callbacks after batched priming: up front, in order, each once
            up_front = list(range(0, primed, interval)) if has_callback else []
            assert [s.i for s in steps[:len(up_front)] if isinstance(s, generation.Callback)] == up_front, c
            assert not any(isinstance(s, generation.Callback) and s.i < n_prime for s in steps[len(up_front):]), c


def test_one_job_on_the_double_against_the_restated_reference(monkeypatch):
    import restated
    cfg = synth.CONFIGS["tiny"]
    W = synth.init_weights(cfg, seed=71)
    m = wavenet_model.WaveNetModel(**cfg)
    m.load_state_dict({k: torch.from_numpy(v) for k, v in W.items()})
    monkeypatch.setattr(engine, "Engine", lambda cfg, weights, n_streams=1, device_index=0, **kw:
                        _REAL_ENGINE(cfg, weights, n_streams=n_streams, device_index=device_index, **double_backend(), **kw))
    for num_given in (70, 23):
        first = np.random.RandomState(num_given).randint(0, 256, num_given)
        got, want = [], []
        r = restated.RestatedWaveNet(cfg, W)
        np.random.seed(5)
        with redirect_stdout(io.StringIO()) as out_ref:
            ref = r.generate_fast(130, first_samples=first, temperature=1.0, progress_callback=lambda i, t: want.append((i, t)), progress_interval=16)
        ref_state = np.random.get_state()
        np.random.seed(5)
        with redirect_stdout(io.StringIO()) as out:
            audio = m.generate_fast(130, first_samples=torch.from_numpy(first), temperature=1.0, progress_callback=lambda i, t: got.append((i, t)),
                                    progress_interval=16)
        state = np.random.get_state()
        assert m._wn_last_prime_batched == (num_given == 70)
        assert np.array_equal(audio, ref) and got == want and len(got) > 8
        assert np.array_equal(state[1], ref_state[1]) and state[2:] == ref_state[2:]
        assert out.getvalue().count("one generating step") == out_ref.getvalue().count("one generating step") == 1


def test_forced_is_checked_by_one_function_for_both_callers():
    """the cases of tests/test_forced_host.py's two argument tests"""
    free = np.full((2, 12), -1)
    for rows in (None, 2):
        ok = engine.checked_forced(free, 12, 256, rows)
        assert ok.dtype == np.int32 and ok.shape == (2, 12)
    f = engine.checked_forced(np.arange(12), 12, 256, rows=3)
    assert f.shape == (3, 12) and f.flags.c_contiguous and f.flags.writeable and np.array_equal(f, np.tile(np.arange(12), (3, 1)))
    assert engine.checked_forced(np.arange(12), 12, 256).shape == (12,) and engine.checked_forced(None, 12, 256, 2) is None
    assert np.array_equal(engine.checked_forced(torch.arange(12), 12, 256), np.arange(12))
    engine_cases = [(np.full((2, 11), -1), 12), (np.full((3, 12), -1), 12), (np.full(13, -1), 12), (np.full((2, 12, 1), -1), 12), (np.full((2, 12), -2), 12),
                    (np.full((2, 12), 256), 12), (np.where(np.arange(12) == 5, 300, -1), 12), (np.full((2, 12), -1.0), 12), (np.zeros((2, 0), int), 0)]
    facade_cases = [(np.full(7, -1), 8), (np.full((1, 2, 4), -1), 8), (np.full(8, -2), 8), (np.full(8, 256), 8), (np.full(8, -1.0), 8), (np.zeros(0, int), 0)]
    for forced, n in engine_cases:
        with pytest.raises(ValueError, match="forced"):
            engine.checked_forced(forced, n, 256, rows=2)
    for forced, n in facade_cases:
        with pytest.raises(ValueError, match="forced"):
            engine.checked_forced(forced, n, 256)
    with pytest.raises(ValueError, match="forced"):
        engine.checked_forced(np.full((3, 8), -1), 8, 256, rows=2)
    # both callers, every case: Engine.generate on the test double (rows = its streams), the facade before any engine exists
    cfg = synth.CONFIGS["tiny"]
    eng = engine.Engine(cfg, synth.init_weights(cfg, seed=1), n_streams=2, **double_backend())
    m = wavenet_model.WaveNetModel(**cfg)
    for forced, n in engine_cases + facade_cases:
        with pytest.raises(ValueError, match="forced"):
            eng.generate(n, np.zeros((2, 4), int), temperature=0., forced=forced)
        with pytest.raises(ValueError, match="forced"):
            m.generate_fast(n, first_samples=torch.zeros(2, 3, dtype=torch.int64), forced=forced)
        with pytest.raises(ValueError, match="forced"):
            m.generate_fast_streams(n, [1.0, 0.5], forced=forced)
    assert m._wn_engine is None
    eng.close()
