"""Host side of the per-sample log-probabilities (wn_set_logprob_output): the float64 statement the GPU tests replay (tests/logprob_cases.py) against
a direct log-softmax, the declaration and the three binding lists, a library without the symbol (the test double, which stays as it is), the
facade's argument check, and the product library's argument checks, which answer before any HIP call.  No GPU: the values themselves are checked in
tests/test_gpu_logprobs.py."""
import ctypes
import math
import os
import re
import sys

import numpy as np
import pytest
import torch

import logprob_cases as lc
import sampler_cases as sc
import sampler_filter_cases as fc
import wavenet_model
from double_lib import double_backend, double_library
from mi355_wavenet import _abi, engine, synth

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAME = "wn_set_logprob_output"


def _rows(seed, C=256):
    rs = np.random.RandomState(seed)
    for s in (0.3, 3.0, 12.0):
        for T in (1.0, 0.05, 1.7):
            yield (rs.standard_normal(C) * s).astype(np.float32), np.float32(T), rs


def _log_softmax64(v):
    v = v.astype(np.float64)
    return v - v.max() - math.log(np.exp(v - v.max()).sum())


def test_logp64_is_the_log_softmax_in_both_modes():
    reg = sc.regularizer(256)
    for logits, T, rs in _rows(41):
        for r in (None, reg):
            x = sc.x32(logits, r, T, False)
            xg = sc.x32(logits, r, T, True)
            for i in rs.randint(0, 256, 6).tolist() + [0, 255, int(np.argmax(logits))]:
                assert abs(lc.logp64(logits, r, T, False, 0, 0.0, i, "model") - _log_softmax64(logits)[i]) <= 1e-12     # no regulariser, no temperature
                assert abs(lc.logp64(logits, r, T, True, 5, 0.5, i, "model") - _log_softmax64(logits)[i]) <= 1e-12
                assert abs(lc.logp64(logits, r, T, False, 0, 0.0, i, "sampling") - _log_softmax64(x)[i]) <= 1e-12
                assert abs(lc.logp64(logits, r, T, True, 5, 0.5, i, "sampling") - _log_softmax64(xg)[i]) <= 1e-12       # greedy: no division, no filter
    with pytest.raises(ValueError):
        lc.logp64(np.zeros(4, np.float32), None, 1.0, False, 0, 0.0, 0, "nonsense")


@pytest.mark.parametrize("top_k,top_p", [(8, 0.0), (0, 0.8), (32, 0.9)])
def test_the_sampling_mode_is_restricted_to_the_kept_set(top_k, top_p):
    n_out = 0
    for logits, T, rs in _rows(43):
        x = sc.x32(logits, None, T, False)
        keep, _ = fc.filter64(x, top_k, top_p)
        assert 0 < keep.sum() < 256
        v = x.astype(np.float64)
        want = v - v.max() - math.log(np.exp(v[keep] - v.max()).sum())
        for i in range(256):
            got = lc.logp64(logits, None, T, False, top_k, top_p, i, "sampling")
            if keep[i]:
                assert abs(got - want[i]) <= 1e-12
            else:
                assert got == -math.inf
                n_out += 1
        assert abs(sum(math.exp(lc.logp64(logits, None, T, False, top_k, top_p, i, "sampling")) for i in range(256)) - 1.0) <= 1e-12
    assert n_out > 0


def test_the_bound_is_the_derived_one():
    assert lc.A_ONE_WAVE == 10 and lc.a_generic(256) == 32 and lc.a_generic(300) == 35 and lc.a_generic(40) == 19
    assert lc.a_of(3, 256) == 10 and lc.a_of(4, 256) == 10 and lc.a_of(1, 256) == 32
    assert lc.bound(-5.0, 256, 10) == 2 * (math.log(256) + 4 + 10) * 2.0 ** -24 + 2.0 ** -21 * 5.0
    assert lc.bound(0.0, 256, 10) < 2.5e-6 and lc.bound(-20.0, 256, 32) < 1.5e-5


def test_the_call_is_declared_bound_and_optional():
    hdr = open(os.path.join(ROOT, "include", "wn_abi.h")).read()
    assert re.search(r"\bint wn_set_logprob_output\(wn_handle\* h, float\* logp, int64_t capacity, int32_t mode\);", hdr)
    assert "#define WN_LOGP_SAMPLING 0" in hdr and "#define WN_LOGP_MODEL 1" in hdr
    assert "#define WN_ABI_VERSION 5" in hdr and _abi.ABI_VERSION == 5
    assert NAME in _abi.EXPORTS and NAME in _abi.OPTIONAL_EXPORTS and NAME in _abi.LAZY_EXPORTS and NAME in _abi.Library._LAZY_ARGTYPES
    assert (_abi.WN_LOGP_SAMPLING, _abi.WN_LOGP_MODEL) == (0, 1)
    assert NAME in open(os.path.join(ROOT, "INTEGRATION.md")).read()


def test_the_double_lacks_the_symbol_and_only_a_request_says_so():
    lib = double_library()
    assert lib.missing == ("wn_score",)                                              # what loading found absent: unchanged
    assert not lib.has(NAME) and lib.has("wn_generate") and NAME not in lib.missing
    assert NAME not in open(os.path.join(ROOT, "tests", "double", "wn_abi_double.cpp")).read()
    cfg = synth.CONFIGS["tiny"]
    eng = engine.Engine(cfg, synth.init_weights(cfg, seed=1), **double_backend())
    u = np.random.RandomState(3).random_sample((1, 12))
    before = eng.generate(12, None, temperature=1.0, uniforms=u)                     # a job without log-probabilities runs as before
    assert isinstance(before, np.ndarray) and before.shape == (1, 12)
    for mode in lc.MODES:
        with pytest.raises(RuntimeError, match="does not export wn_set_logprob_output.*rebuild it"):
            eng.generate(12, None, temperature=1.0, uniforms=u, logprobs=mode)
    with pytest.raises(ValueError, match="logprobs"):
        eng.generate(12, None, temperature=1.0, uniforms=u, logprobs="nonsense")
    assert np.array_equal(eng.generate(12, None, temperature=1.0, uniforms=u), before)
    eng.close()


def test_the_facade_checks_return_logprobs_before_it_touches_an_engine():
    m = wavenet_model.WaveNetModel(**synth.CONFIGS["tiny"])
    for call in (lambda: m.generate_fast(4, return_logprobs="nonsense"), lambda: m.generate_fast_streams(4, [1.0], return_logprobs="nonsense"),
                 lambda: m.generate_fast(4, return_logprobs=2)):
        with pytest.raises(ValueError, match="return_logprobs"):
            call()
    assert m._wn_engine is None
    f = wavenet_model.WaveNetModel._logprob_mode
    assert (f(False), f(None), f(True), f("sampling"), f("model")) == (None, None, "sampling", "sampling", "model")
    with pytest.raises(TypeError):
        m.generate_fast(4, None, 1.0, 0.0, None, 100, 0, 0.0, None, False, "model")    # keyword only: the positional signature is the reference's


def test_the_product_library_checks_its_arguments_before_any_hip_call():
    sys.path.insert(0, os.path.join(ROOT, "pytorch-wavenet_amd"))
    import build
    lib = _abi.Library(build.build_hip())
    assert lib.has(NAME) and lib.missing == ()
    buf = np.zeros(4, np.float32)
    p = ctypes.c_void_p(buf.ctypes.data)
    for args, word in (((None, p, 4, 0), "NULL handle"), ((None, None, 0, 1), "NULL handle"), ((None, p, -1, 0), "capacity"), ((None, p, 4, 2), "mode"),
                       ((None, p, 4, -1), "mode")):
        assert lib.dll.wn_set_logprob_output(*args) == _abi.WN_E_BADARG, args
        assert NAME in lib.last_error() and word in lib.last_error(), (args, lib.last_error())
    assert not buf.any()
