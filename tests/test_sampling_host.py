"""Host logic of the sampling filters (wn_set_sampling): the declaration and the binding, a library without the symbol (the test double, which stays as
it is), Engine.set_sampling's argument checks, and the facade's set / reset around a job -- also when a progress callback raises.  No GPU: what needs a
library WITH the symbol wraps the double in a recorder (the filter itself runs in tests/test_gpu_sampler_filter_kernels.py and
tests/test_gpu_sampling_filters.py)."""
import os
import re

import numpy as np
import pytest
import torch

import wavenet_model
from double_lib import double_backend, double_library
from mi355_wavenet import _abi, engine, synth

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
_REAL_ENGINE = engine.Engine


def test_wn_set_sampling_is_declared_bound_and_optional():
    hdr = open(os.path.join(ROOT, "include", "wn_abi.h")).read()
    assert re.search(r"\bint wn_set_sampling\(wn_handle\* h, int32_t top_k, float top_p\);", hdr)
    assert "wn_set_sampling" in _abi.EXPORTS and "wn_set_sampling" in _abi.OPTIONAL_EXPORTS and "wn_set_sampling" in _abi.LAZY_EXPORTS
    assert "#define WN_ABI_VERSION 5" in hdr and _abi.ABI_VERSION == 5
    for word in ("top_k", "top_p", "x_i >= tau", "G_i < top_p * T", "u >= 1"):
        assert word in hdr, "the header states the contract: %r" % word
    assert "wn_set_sampling" in open(os.path.join(ROOT, "INTEGRATION.md")).read()


def _engine_on_double(**kw):
    cfg = synth.CONFIGS["tiny"]
    return _REAL_ENGINE(cfg, synth.init_weights(cfg, seed=1), **dict(double_backend(), **kw)), cfg


def test_the_double_lacks_the_symbol_and_a_filter_request_says_so():
    lib = double_library()
    assert not lib.has("wn_set_sampling") and lib.has("wn_generate")
    assert "wn_set_sampling" not in lib.missing        # (looked up on first use, not when the library is loaded)
    assert "wn_set_sampling" not in open(os.path.join(ROOT, "tests", "double", "wn_abi_double.cpp")).read()
    eng, cfg = _engine_on_double()
    u = np.random.RandomState(3).random_sample((1, 12))
    before = eng.generate(12, None, temperature=1.0, uniforms=u)                 # a job without a filter runs as before ...
    with pytest.raises(RuntimeError, match="does not export wn_set_sampling"):
        eng.generate(12, None, temperature=1.0, uniforms=u, top_k=5)
    with pytest.raises(RuntimeError, match="wn_set_sampling"):
        eng.generate(12, None, temperature=1.0, uniforms=u, top_p=0.9)
    with pytest.raises(RuntimeError, match="wn_set_sampling"):
        eng.set_sampling(top_k=3)
    eng.set_sampling(0, 0.0)                                                     # ... and "off" never touches the symbol
    assert np.array_equal(eng.generate(12, None, temperature=1.0, uniforms=u, top_k=0, top_p=0.0), before)
    assert np.array_equal(eng.generate(12, None, temperature=1.0, uniforms=u), before)
    eng.close()


def test_the_product_library_refuses_a_null_handle_before_any_hip_call():
    import sys
    sys.path.insert(0, os.path.join(ROOT, "pytorch-wavenet_amd"))
    import build
    lib = _abi.Library(build.build_hip())
    assert lib.has("wn_set_sampling") and lib.missing == ()
    assert lib.dll.wn_set_sampling(None, 0, 0.0) == _abi.WN_E_BADARG
    assert "wn_set_sampling: NULL handle" in lib.last_error()


# ---------------------------------------------------------------- a library WITH the symbol: the double behind a recorder
class _Dll:
    def __init__(self, dll, events):
        self._dll, self._events = dll, events

    def __getattr__(self, name):
        fn = getattr(self._dll, name)
        if name != "wn_generate":
            return fn

        def generate(*a):
            self._events.append("generate")
            return fn(*a)
        return generate

    def wn_set_sampling(self, h, top_k, top_p):
        self._events.append((top_k, top_p))
        return 0


class _WithSampling:
    def __init__(self):
        self._lib = double_library()
        self.path, self.events = self._lib.path, []
        self.dll = _Dll(self._lib.dll, self.events)

    def has(self, name):
        return name == "wn_set_sampling" or self._lib.has(name)

    def check(self, rc):
        self._lib.check(rc)

    def last_error(self):
        return self._lib.last_error()


def test_set_sampling_checks_its_arguments():
    lib = _WithSampling()
    eng, cfg = _engine_on_double(lib=lib)
    for bad in (dict(top_k=-1), dict(top_k=2.5), dict(top_k=True), dict(top_k=1 << 31), dict(top_p=-0.1), dict(top_p=1.5), dict(top_p=float("nan"))):
        with pytest.raises(ValueError):
            eng.set_sampling(**bad)
    assert lib.events == []
    eng.set_sampling(top_k=300, top_p=1.0)        # the off values are the library's to normalise
    eng.set_sampling(7)
    eng.set_sampling(top_p=0.25)
    eng.set_sampling()
    assert lib.events == [(300, 1.0), (7, 0.0), (0, 0.25), (0, 0.0)]
    u = np.random.RandomState(3).random_sample((1, 4))
    eng.generate(4, None, temperature=1.0, uniforms=u, top_k=9)                  # top_p None: what the handle has
    eng.generate(4, None, temperature=1.0, uniforms=u, top_p=0.5)                # the 9 stayed
    eng.generate(4, None, temperature=1.0, uniforms=u)                           # None, None: the handle is left alone
    assert lib.events[4:] == [(9, 0.0), "generate", (9, 0.5), "generate", "generate"]
    eng.close()


def _model_on(lib, monkeypatch, seed=62):
    cfg = synth.CONFIGS["tiny"]
    W = synth.init_weights(cfg, seed=seed)
    m = wavenet_model.WaveNetModel(**cfg)
    m.load_state_dict({k: torch.from_numpy(v) for k, v in W.items()})

    def make(cfg, weights, n_streams=1, device_index=0, **kw):
        return _REAL_ENGINE(cfg, weights, n_streams=n_streams, device_index=device_index, lib=lib, mem=double_backend()["mem"], **kw)

    monkeypatch.setattr(engine, "Engine", make)
    return m


def test_generate_fast_sets_the_filter_for_every_piece_and_resets_it(monkeypatch):
    lib = _WithSampling()
    m = _model_on(lib, monkeypatch)
    first = torch.from_numpy(np.random.RandomState(62).randint(0, 256, 5))
    np.random.seed(9)
    m.generate_fast(40, first_samples=first, temperature=1.0, progress_callback=lambda s, t: None, progress_interval=10, top_k=6, top_p=0.75)
    ev = lib.events
    assert ev[0] == (6, 0.75) and ev[-1] == (0, 0.0) and ev.count("generate") >= 4 and set(ev[1:-1]) == {"generate"}, ev
    state = np.random.get_state()       # (key words AND position: the keys alone stay the same for up to 312 draws)
    np.random.seed(9)
    del ev[:]
    m.generate_fast(40, first_samples=first, temperature=1.0, progress_callback=lambda s, t: None, progress_interval=10)
    assert set(ev) == {"generate"}, "a call without a filter never touches the symbol"
    after = np.random.get_state()
    assert np.array_equal(after[1], state[1]) and after[2:] == state[2:], "the filtered call consumed the global RNG like the unfiltered one"
    np.random.seed(9)
    np.random.random_sample(40)
    assert np.random.get_state()[2] == state[2], "40 uniforms for 40 samples"
    del ev[:]
    m.generate_fast_streams(8, [1.0, 0.0, 0.5], first_samples=first, top_p=0.9)
    assert ev == [(0, 0.9), "generate", (0, 0.0)]
    with pytest.raises(TypeError):
        m.generate_fast(8, first, 1.0, 0.0, None, 100, 5)                        # keyword only: the positional signature is the reference's


def test_generate_fast_resets_the_filter_when_a_callback_raises(monkeypatch):
    lib = _WithSampling()
    m = _model_on(lib, monkeypatch)
    first = torch.from_numpy(np.random.RandomState(62).randint(0, 256, 5))
    calls = []

    def callback(s, t):
        calls.append(s)
        if len(calls) == 2:
            raise KeyError("stop")

    with pytest.raises(KeyError):
        m.generate_fast(40, first_samples=first, temperature=1.0, progress_callback=callback, progress_interval=10, top_k=4)
    assert len(calls) == 2
    assert lib.events[0] == (4, 0.0) and lib.events[-1] == (0, 0.0) and "generate" in lib.events, lib.events
