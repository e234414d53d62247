"""Host side of the generation state (no GPU): mi355_wavenet.state.GenerationState against the torch restatement of the reference's queues
(oracle/restated.py), its files and checks, the binding of wn_state_floats / wn_state_save / wn_state_load / wn_prime_shared, a library without
them (the test double, which stays as it is), and the facade's argument errors."""
import os
import pickle
import re
import time

import numpy as np
import pytest
import torch

import restated
import wavenet_model
from double_lib import double_backend, double_library
from mi355_wavenet import _abi, engine, synth
from mi355_wavenet.state import GEOMETRY, GenerationState, queue_lengths

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("wn_state_floats", "wn_state_save", "wn_state_load", "wn_prime_shared")
TINY = synth.CONFIGS["tiny"]
TINY3 = dict(TINY, kernel_size=3)
_REAL_ENGINE = engine.Engine
_T0 = time.time()


@pytest.fixture(scope="module", autouse=True)
def _timing():
    yield
    print("\ntest_generation_state_host: %.1f s wall" % (time.time() - _T0))


def _oracle(cfg):
    return restated.RestatedWaveNet(cfg, synth.init_weights(cfg, seed=5))


def _run(m, inputs):
    """teacher-forced evaluations on the oracle's present queues -> the logits of the last one"""
    x = None
    for i in inputs:
        x = m.wavenet_step(m._onehot(i)).squeeze().numpy()
    return x


def _greedy(m, first, n):
    """n greedy evaluations from the present queues, the first on `first` -> the indices drawn"""
    out, nxt = [], int(first)
    for _ in range(n):
        nxt = int(np.argmax(_run(m, [nxt])))
        out.append(nxt)
    return out


@pytest.mark.parametrize("cfg", [TINY, TINY3], ids=["k2", "k3"])
@pytest.mark.parametrize("evals", [3, 5, 40])   # fewer than the largest ring holds, exactly one ring (k = 2: d = 4), wrapped
def test_state_converts_to_and_from_the_reference_queues(cfg, evals):
    m = _oracle(cfg)
    inputs = np.random.RandomState(evals).randint(0, 256, evals)
    _run(m, inputs)
    st = GenerationState.from_reference_queues(m.queues, 17, evals)
    assert st.geometry() == {n: cfg[n] for n in GEOMETRY}
    assert st.state.dtype == np.float32 and st.state.size == st.state_floats() == cfg["residual_channels"] * sum(queue_lengths(cfg["layers"], cfg["blocks"], cfg["kernel_size"]))
    for blk, q in zip(st.blocks_by_layer(), m.queues):   # the newest row is the last push, rows before the stream start are zero
        ml = q.max_length
        assert np.array_equal(blk[-1], q.data[:, (q.in_pos - 1) % ml].numpy())
        if evals < ml:
            assert not blk[:ml - evals].any() and blk[ml - evals:].any()
    same = st.to_reference_queues()
    for (data, in_pos, out_pos), q in zip(same, m.queues):
        assert np.array_equal(data, q.data.numpy()) and in_pos == q.in_pos and out_pos == q.out_pos
    for other in (0, 1, evals + 7, 1000):   # another queue time: the data rolled by the difference
        for (data, in_pos, out_pos), q in zip(st.to_reference_queues(other), m.queues):
            assert in_pos == out_pos == other % q.max_length
            assert np.array_equal(data, np.roll(q.data.numpy(), other - evals, axis=1))
        back = GenerationState.from_reference_queues(st.to_reference_queues(other), 17, evals)
        assert back == st
    # what Engine.export_queue returns converts the same way
    assert GenerationState.from_reference_queues([(q.data.numpy(), q.in_pos, q.out_pos) for q in m.queues], 17, evals) == st


@pytest.mark.parametrize("cfg", [TINY, TINY3], ids=["k2", "k3"])
def test_a_state_put_back_into_a_fresh_oracle_continues_like_the_one_shot_run(cfg):
    m = _oracle(cfg)
    inputs = np.random.RandomState(2).randint(0, 256, 23)
    _run(m, inputs[:-1])
    one_shot = _greedy(m, inputs[-1], 1 + 30)   # evaluation 23 draws the first index, 30 more follow
    st = GenerationState.from_reference_queues(_oracle_at(cfg, inputs).queues, one_shot[0], 23)   # the queues behind evaluation 23, and what it drew
    fresh = _oracle(cfg)
    _run(fresh, [0, 1, 2, 3, 4, 5, 6])   # another queue time: the rotation is not the identity
    for q, (data, in_pos, out_pos) in zip(fresh.queues, st.to_reference_queues(7)):
        q.data, q.in_pos, q.out_pos = torch.from_numpy(data.copy()), in_pos, out_pos
    assert _greedy(fresh, st.last_index, 30) == one_shot[1:]


def _oracle_at(cfg, inputs):
    m = _oracle(cfg)
    _run(m, inputs)
    return m


def _some_state(evals=9):
    m = _oracle_at(TINY, np.arange(evals))
    return GenerationState.from_reference_queues(m.queues, 200, evals)


def test_state_pickles_and_saves(tmp_path):
    st = _some_state()
    assert pickle.loads(pickle.dumps(st)) == st
    path = str(tmp_path / "stream.npz")
    st.save(path)
    back = GenerationState.load(path)
    assert back == st and back.state.dtype == np.float32 and back.last_index == 200 and back.evals == 9
    assert "evals=9" in repr(back)
    other = pickle.loads(pickle.dumps(st))
    other.state[3] += 1
    assert other != st
    with pytest.raises(ValueError, match="values"):
        GenerationState(st.state[:-1], 0, **st.geometry())
    with pytest.raises(ValueError, match="last_index"):
        GenerationState(st.state, 256, **st.geometry())


def test_check_names_the_field_that_does_not_match():
    st = _some_state()
    st.check(dict(TINY))
    st.check(wavenet_model.WaveNetModel(output_length=4, **TINY))
    for name in GEOMETRY:
        with pytest.raises(ValueError, match=name):
            st.check(dict(TINY, **{name: TINY[name] + 1}))
    with pytest.raises(ValueError, match="residual_channels"):
        st.check(wavenet_model.WaveNetModel(output_length=4, **dict(TINY, residual_channels=8)))
    with pytest.raises(ValueError, match="not those of a WaveNet stack"):
        GenerationState.from_reference_queues([(np.zeros((4, 2), np.float32), 0), (np.zeros((4, 4), np.float32), 0)], 0)


# ---------------------------------------------------------------- the binding
def test_the_four_entry_points_are_declared_bound_and_optional():
    hdr = open(os.path.join(ROOT, "include", "wn_abi.h")).read()
    assert re.search(r"\bint wn_state_floats\(wn_handle\* h, int64_t\* out\);", hdr)
    assert re.search(r"\bint wn_state_save\(wn_handle\* h, int32_t stream, float\* state, void\* hip_stream\);", hdr)
    assert re.search(r"\bint wn_state_load\(wn_handle\* h, int32_t stream_first, int32_t stream_count, const float\* state, void\* hip_stream\);", hdr)
    assert re.search(r"\bint wn_prime_shared\(wn_handle\* h, const int32_t\* first_samples, int64_t n_prime, void\* hip_stream\);", hdr)
    assert "#define WN_ABI_VERSION 5" in hdr and _abi.ABI_VERSION == 5
    for n in NAMES:
        assert n in _abi.EXPORTS and n in _abi.OPTIONAL_EXPORTS and n in _abi.LAZY_EXPORTS and n in _abi.Library._LAZY_ARGTYPES
        assert n in open(os.path.join(ROOT, "INTEGRATION.md")).read()


def test_a_library_without_them_loads_as_before_and_the_engine_names_the_symbol():
    lib = double_library()
    assert lib.missing == ("wn_score",)      # what loading found absent: unchanged
    src = open(os.path.join(ROOT, "tests", "double", "wn_abi_double.cpp")).read()
    cfg = TINY
    eng = _REAL_ENGINE(cfg, synth.init_weights(cfg, seed=1), n_streams=2, **double_backend())
    for n in NAMES:
        assert n not in src and not lib.has(n)
    with pytest.raises(RuntimeError, match="does not export wn_state_floats"):
        eng.state_floats()
    with pytest.raises(RuntimeError, match="does not export wn_state_save"):
        eng.state_save(1)
    with pytest.raises(RuntimeError, match="does not export wn_state_load"):
        eng.state_load(np.zeros(4, np.float32))
    with pytest.raises(RuntimeError, match="does not export wn_prime_shared"):
        eng.prime_shared(np.zeros(70, np.int32))
    first = np.tile(np.arange(70), (2, 1))
    with pytest.raises(RuntimeError, match="wn_prime_shared"):
        eng.generate(4, first, temperature=0.0, shared_prompt=True)
    with pytest.raises(ValueError, match="rows of first_samples differ"):
        eng.generate(4, np.stack([np.arange(70), np.arange(70)[::-1]]), temperature=0.0, shared_prompt=True)
    assert np.array_equal(eng.generate(4, first, temperature=0.0), eng.generate(4, np.arange(70), temperature=0.0))   # ... and the job without it runs
    eng.close()


def test_the_product_library_refuses_null_arguments_before_any_hip_call():
    import sys
    sys.path.insert(0, os.path.join(ROOT, "pytorch-wavenet_amd"))
    import build
    lib = _abi.Library(build.build_hip())
    assert lib.missing == () and all(lib.has(n) for n in NAMES)
    buf = np.zeros(8, np.float32)
    n = _abi.ctypes.c_int64()
    assert lib.dll.wn_state_floats(None, _abi.ctypes.byref(n)) == _abi.WN_E_BADARG and "wn_state_floats: NULL argument" in lib.last_error()
    assert lib.dll.wn_state_save(None, 0, buf.ctypes.data, None) == _abi.WN_E_BADARG and "wn_state_save: NULL argument" in lib.last_error()
    assert lib.dll.wn_state_load(None, 0, 1, buf.ctypes.data, None) == _abi.WN_E_BADARG and "wn_state_load: NULL argument" in lib.last_error()
    assert lib.dll.wn_prime_shared(None, buf.ctypes.data, 2, None) == _abi.WN_E_BADARG and "wn_prime_shared: NULL argument" in lib.last_error()


# ---------------------------------------------------------------- the facade's argument errors (raised before an engine exists)
def test_facade_argument_errors():
    m = wavenet_model.WaveNetModel(output_length=4, **TINY)
    st = _some_state()
    with pytest.raises(ValueError, match="first_samples must not be given"):
        m.generate_fast(4, first_samples=torch.zeros(3, dtype=torch.long), continue_from=st)
    with pytest.raises(ValueError, match="first_samples must not be given"):
        m.generate_fast_streams(4, [1.0, 0.5], first_samples=torch.zeros(3, dtype=torch.long), continue_from=st)
    with pytest.raises(ValueError, match="GenerationState"):
        m.generate_fast(4, continue_from=[])
    with pytest.raises(ValueError, match="GenerationState"):
        m.generate_fast(4, continue_from=[st, "no state"])
    with pytest.raises(ValueError, match="ONE state"):
        m.generate_fast_streams(4, [1.0, 0.5], continue_from=[st, st])
    other = wavenet_model.WaveNetModel(output_length=4, **dict(TINY, layers=4))
    with pytest.raises(ValueError, match="layers"):
        other.generate_fast(4, continue_from=st)
    with pytest.raises(ValueError, match="layers"):
        other.generate_fast_streams(4, [1.0], continue_from=st)
    assert m._wn_engine is None and other._wn_engine is None   # nothing was built on the way


def test_facade_on_a_library_without_the_symbols(monkeypatch):
    """generate_fast_streams keeps priming per stream there; return_state / continue_from say which symbol is missing"""
    m = wavenet_model.WaveNetModel(output_length=4, **TINY)
    real = engine.Engine
    monkeypatch.setattr(engine, "Engine", lambda cfg, weights, n_streams=1, device_index=0, **kw: real(cfg, weights, n_streams=n_streams, device_index=device_index,
                                                                                                       **double_backend(), **kw))
    first = torch.from_numpy(np.arange(80) % 256)
    np.random.seed(4)
    a = m.generate_fast_streams(6, [1.0, 0.0], first_samples=first)
    np.random.seed(4)
    b = m.generate_fast(6, first_samples=first, temperature=1.0)
    assert np.array_equal(a[0], b)
    with pytest.raises(RuntimeError, match="wn_state_floats|wn_state_save"):
        m.generate_fast(3, return_state=True)
    with pytest.raises(RuntimeError, match="wn_state_load|wn_state_floats"):
        m.generate_fast(3, continue_from=_some_state())
