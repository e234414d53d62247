"""Host side of the forced samples (wn_set_forced_samples): the mask builders the GPU tests use (tests/forced_cases.py), the declaration and the three
binding lists, a library without the symbol (the test double, which stays as it is), Engine.generate's and the facade's argument checks -- which answer
before the missing symbol does --, the per-piece slices the facade hands to Engine.generate, score_continuation's argument errors, and the product
library's argument checks, which answer before any HIP call.  No GPU: what a forced job computes is checked in tests/test_gpu_forced.py."""
import ctypes
import io
import os
import re
import sys
from contextlib import redirect_stdout

import numpy as np
import pytest
import torch

import forced_cases as fz
import wavenet_model
from double_lib import double_backend, double_library
from mi355_wavenet import _abi, engine, synth
from mi355_wavenet.state import GenerationState

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAME = "wn_set_forced_samples"
_REAL_ENGINE = engine.Engine


def test_the_mask_builders():
    m = fz.positions(64)
    assert m[0] and m[7:12].all() and not m[1:7].any() and not m[12:15].any() and m[15] and m[18] and not m[16] and m[63] and 0 < m.sum() < 64
    for ns in (1, 2, 4, 8):
        p = fz.per_stream(ns, 64)
        assert p.shape == (ns, 64) and p.dtype == bool
        if ns > 1:
            assert not p[0].any() and p[1].all()
            assert len({r.tobytes() for r in p}) == ns, "the rows differ"
            assert all(0 < r.sum() < 64 for r in p[2:])
        else:
            assert np.array_equal(p[0], m)
    assert np.array_equal(fz.shared(3, 64), np.tile(m, (3, 1)))
    plain = np.arange(600).reshape(2, 300) % 300
    for C in (256, 300):
        v = fz.shifted_classes(plain % C, C)
        assert v.dtype == np.int32 and v.min() >= 0 and v.max() < C and (v != plain % C).all()
    f = fz.forced_array(fz.per_stream(4, 64), fz.shifted_classes(np.zeros((4, 64), int), 256))
    assert f.dtype == np.int32 and (f[0] == fz.FREE).all() and (f[1] == 128).all() and set(np.unique(f)) == {fz.FREE, 128}
    assert fz.first_forced(fz.per_stream(4, 64)[0]) is None and fz.first_forced(m) == 0 and fz.first_forced(fz.per_stream(4, 64)[2]) is not None
    assert fz.ragged_prefix_lengths(4) == [0, 5, 1, 7] and fz.ragged_prefix_lengths(9)[8] == 0


def test_the_call_is_declared_bound_and_optional():
    hdr = open(os.path.join(ROOT, "include", "wn_abi.h")).read()
    assert re.search(r"\bint wn_set_forced_samples\(wn_handle\* h, const int32_t\* forced, int64_t capacity\);", hdr)
    assert "#define WN_ABI_VERSION 5" in hdr and _abi.ABI_VERSION == 5
    assert NAME in _abi.EXPORTS and NAME in _abi.OPTIONAL_EXPORTS and NAME in _abi.LAZY_EXPORTS and NAME in _abi.Library._LAZY_ARGTYPES
    for doc in ("INTEGRATION.md", "README.md", "DESIGN.md"):
        assert NAME in open(os.path.join(ROOT, doc)).read(), doc


def test_the_double_lacks_the_symbol_and_the_value_errors_come_first():
    lib = double_library()
    assert lib.missing == ("wn_score",)
    assert not lib.has(NAME) and NAME not in lib.missing
    assert NAME not in open(os.path.join(ROOT, "tests", "double", "wn_abi_double.cpp")).read()
    cfg = synth.CONFIGS["tiny"]
    eng = engine.Engine(cfg, synth.init_weights(cfg, seed=1), n_streams=2, **double_backend())
    u = np.random.RandomState(3).random_sample((2, 12))
    kw = dict(temperature=1.0, uniforms=u)
    before = eng.generate(12, None, **kw)
    free = np.full((2, 12), -1)
    for forced in (free, free[0], np.arange(12), np.zeros((2, 12), np.int64)):       # well-formed: the missing symbol answers, and names itself
        with pytest.raises(RuntimeError, match="does not export wn_set_forced_samples.*rebuild it"):
            eng.generate(12, None, forced=forced, **kw)
    with pytest.raises(RuntimeError, match=NAME):
        eng.set_forced_samples(None, 0)
    bad = [np.full((2, 11), -1), np.full((3, 12), -1), np.full(13, -1), np.full((2, 12, 1), -1),      # shapes
           np.full((2, 12), -2), np.full((2, 12), 256), np.where(np.arange(12) == 5, 300, -1),           # values < -1 or >= classes
           np.full((2, 12), -1.0)]                                                                       # not integers
    for forced in bad:
        with pytest.raises(ValueError, match="forced"):
            eng.generate(12, None, forced=forced, **kw)
    with pytest.raises(ValueError, match="forced"):       # nothing is generated: there is no position to force
        eng.generate(0, np.zeros((2, 4), int), forced=np.zeros((2, 0), int), **kw)
    assert np.array_equal(eng.generate(12, None, **kw), before), "a refused call changed nothing"
    eng.close()


def _model(seed=61):
    cfg = synth.CONFIGS["tiny"]
    W = synth.init_weights(cfg, seed=seed)
    m = wavenet_model.WaveNetModel(output_length=8, **cfg)
    m.load_state_dict({k: torch.from_numpy(v) for k, v in W.items()})
    return m


def _inject_recording_double(monkeypatch, record):
    """the facade's engines are built on the test double; Engine.generate records the `forced` it is handed and runs the job without it"""
    def make(cfg, weights, n_streams=1, device_index=0, **kw):
        return _REAL_ENGINE(cfg, weights, n_streams=n_streams, device_index=device_index, **double_backend(), **kw)

    real = _REAL_ENGINE.generate

    def generate(self, num_samples, *a, **kw):
        record.append((num_samples, kw.pop("forced", None), kw.get("logprobs")))
        return real(self, num_samples, *a, **kw)

    monkeypatch.setattr(engine, "Engine", make)
    monkeypatch.setattr(_REAL_ENGINE, "generate", generate)


@pytest.mark.parametrize("interval", [16, 100])
def test_the_facade_hands_every_piece_its_slice(interval, monkeypatch):
    m = _model()
    n = 130
    first = torch.from_numpy(np.random.RandomState(5).randint(0, 256, 6))
    forced = fz.forced_array(fz.positions(n), np.random.RandomState(6).randint(0, 256, n))
    record = []
    _inject_recording_double(monkeypatch, record)
    np.random.seed(4)
    with redirect_stdout(io.StringIO()):
        plain = m.generate_fast(n, first_samples=first, temperature=1.0, progress_callback=lambda s, t: None, progress_interval=interval)
    state = np.random.get_state()
    assert all(f is None for _, f, _ in record)
    pieces_plain = [k for k, _, _ in record]
    del record[:]
    np.random.seed(4)
    calls = []
    with redirect_stdout(io.StringIO()) as out:
        audio = m.generate_fast(n, first_samples=first, temperature=1.0, progress_callback=lambda s, t: calls.append(s), progress_interval=interval,
                                forced=forced)
    after = np.random.get_state()
    assert [k for k, _, _ in record] == pieces_plain and len([k for k in pieces_plain if k > 0]) >= (3 if interval == 16 else 2), "the same pieces"
    assert "one generating step does take approximately" in out.getvalue() and len(calls) >= 1
    slices = [f for k, f, _ in record if k > 0]
    assert all(f is not None and f.shape == (1, k) for (k, f, _) in record if k > 0) and all(f is None for k, f, _ in record if k == 0)
    assert np.array_equal(np.concatenate(slices, axis=1), forced[None, :])
    assert np.array_equal(audio, plain)       # (the recorder dropped the argument: the double ran the plain job)
    assert np.array_equal(after[1], state[1]) and after[2:] == state[2:], "the call with `forced` consumes the global RNG exactly as the one without"
    # two rows, a per-row array and a shared 1-D one
    del record[:]
    first2 = torch.from_numpy(np.random.RandomState(7).randint(0, 256, (2, 6)))
    per_row = fz.forced_array(np.stack([fz.positions(n), ~fz.positions(n)]), 9)
    with redirect_stdout(io.StringIO()):
        m.generate_fast(n, first_samples=first2, temperature=1.0, progress_callback=lambda s, t: None, progress_interval=interval, forced=per_row)
    assert np.array_equal(np.concatenate([f for k, f, _ in record if k > 0], axis=1), per_row)
    del record[:]
    with redirect_stdout(io.StringIO()):
        m.generate_fast(n, first_samples=first2, temperature=1.0, forced=forced)
    assert np.array_equal(np.concatenate([f for k, f, _ in record if k > 0], axis=1), np.tile(forced, (2, 1)))
    del record[:]
    m.generate_fast_streams(20, [1.0, 0.0, 0.5], forced=forced[:20])
    assert len(record) == 1 and np.array_equal(record[0][1], forced[:20])
    del record[:]
    rows = np.stack([forced[:20], forced[20:40], forced[40:60]])
    m.generate_fast_streams(20, [1.0, 0.0, 0.5], forced=rows)
    assert len(record) == 1 and np.array_equal(record[0][1], rows)


def test_the_facade_checks_forced_before_it_touches_an_engine():
    m = _model()
    free = np.full(8, -1)
    calls = [lambda: m.generate_fast(8, forced=np.full(7, -1)), lambda: m.generate_fast(8, forced=np.full((1, 2, 4), -1)),
             lambda: m.generate_fast(8, forced=np.full(8, -2)), lambda: m.generate_fast(8, forced=np.full(8, 256)),
             lambda: m.generate_fast(8, forced=np.full(8, -1.0)), lambda: m.generate_fast(0, forced=np.zeros(0, int)),
             lambda: m.generate_fast(8, first_samples=torch.zeros(2, 3, dtype=torch.int64), forced=np.full((3, 8), -1)),
             lambda: m.generate_fast_streams(8, [1.0, 0.5], forced=np.full((3, 8), -1)), lambda: m.generate_fast_streams(8, [1.0], forced=np.full(9, -1))]
    for call in calls:
        with pytest.raises(ValueError, match="forced"):
            call()
    assert m._wn_engine is None
    with pytest.raises(TypeError):
        m.generate_fast(8, None, 1.0, 0.0, None, 100, 0, 0.0, None, False, False, free)    # keyword only: the positional signature is the reference's
    with pytest.raises(TypeError):
        m.generate_fast_streams(8, [1.0], None, 0.0, 0, 0.0, None, False, free)


def test_score_continuation_argument_errors(monkeypatch):
    m = _model()
    from mi355_wavenet.state import queue_lengths
    state = GenerationState(np.zeros(m.residual_channels * sum(queue_lengths(m.layers, m.blocks, m.kernel_size)), np.float32), 0, 0, layers=m.layers,
                            blocks=m.blocks, residual_channels=m.residual_channels, kernel_size=m.kernel_size, classes=m.classes)
    ok = np.arange(8)
    calls = [lambda: m.score_continuation(np.zeros(0, int)), lambda: m.score_continuation(np.zeros((2, 0), int)),
             lambda: m.score_continuation(np.zeros((1, 2, 3), int)), lambda: m.score_continuation(ok * 0.5),
             lambda: m.score_continuation(ok - 1), lambda: m.score_continuation(ok + 250),                       # -1 is "free" elsewhere: not audio
             lambda: m.score_continuation(ok, continue_from=state, first_samples=torch.zeros(3, dtype=torch.int64)),
             lambda: m.score_continuation(ok, continue_from=[state, state]), lambda: m.score_continuation(np.stack([ok, ok]), continue_from=state),
             lambda: m.score_continuation(np.stack([ok, ok]), continue_from=[state]), lambda: m.score_continuation(ok, continue_from="nonsense"),
             lambda: m.score_continuation(np.stack([ok, ok]), first_samples=torch.zeros(3, dtype=torch.int64)),
             lambda: m.score_continuation(np.stack([ok, ok]), first_samples=torch.zeros(3, 4, dtype=torch.int64)),
             lambda: m.score_continuation(ok, first_samples=torch.zeros(1, 4, dtype=torch.int64))]
    for k, call in enumerate(calls):
        with pytest.raises(ValueError):
            call()
        assert m._wn_engine is None, k
    # on a library without the symbol the request says so, and the numpy RNG was left alone
    monkeypatch.setattr(engine, "Engine", lambda cfg, weights, n_streams=1, device_index=0, **kw:
                        _REAL_ENGINE(cfg, weights, n_streams=n_streams, device_index=device_index, **double_backend(), **kw))
    np.random.seed(2)
    before = np.random.get_state()
    with pytest.raises(RuntimeError, match=NAME):
        m.score_continuation(ok)
    after = np.random.get_state()
    assert np.array_equal(after[1], before[1]) and after[2:] == before[2:]


def test_the_product_library_checks_its_arguments_before_any_hip_call():
    sys.path.insert(0, os.path.join(ROOT, "pytorch-wavenet_amd"))
    import build
    lib = _abi.Library(build.build_hip())
    assert lib.has(NAME) and lib.missing == ()
    buf = np.full(4, -1, np.int32)
    p = ctypes.c_void_p(buf.ctypes.data)
    for args, word in (((None, p, 4), "NULL handle"), ((None, None, 0), "NULL handle"), ((None, p, -1), "capacity")):
        assert lib.dll.wn_set_forced_samples(*args) == _abi.WN_E_BADARG, args
        assert NAME in lib.last_error() and word in lib.last_error(), (args, lib.last_error())
