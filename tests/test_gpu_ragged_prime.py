"""-m gpu: prompts of unequal length primed in one batched pass (C ABI wn_prime_ragged, Engine.prime_ragged, generate_fast(first_samples=[p0, p1, ...])).
Engine level: after the ragged pass every stream's saved state is BIT for bit that of a one-stream engine primed (wn_prime) with that row alone, and a
job from there equals the job of the same engine with those states loaded.  Facade: where the ragged job meets per-prompt one-stream calls -- another
kernel form, chain priming instead of the products -- the cases are chosen on the CPU so that the oracle decides them: every sampled draw at least 1e-5
from a CDF boundary (the convention of tests/test_gpu_generation_state.py), every greedy step's top-2 gap above ten times the logit tolerance."""
import ctypes
import time

import numpy as np
import pytest
import torch

import c_oracle
import ragged_cases as rc
import wavenet_model
from mi355_wavenet import _abi, engine, synth
from parity_common import LOGIT_RTOL
from test_gpu_generation_state import TINY3, _decided, _padded_cfg
from test_gpu_parity import MINI3
from test_gpu_taps import K3S, K4S

pytestmark = pytest.mark.gpu
_T0 = time.time()
N_JOB = 20


@pytest.fixture(scope="module", autouse=True)
def _timing():
    yield
    print("\ntest_gpu_ragged_prime: %.1f s wall" % (time.time() - _T0))


def _prompts(seed, lengths):
    rs = np.random.RandomState(seed)
    return [rs.randint(0, 256, n).astype(np.int64) for n in lengths]


def _references(cfg, W, rows):
    """every row primed ALONE on a one-stream engine (wn_prime) -> its saved state; equal rows are primed once"""
    one = engine.Engine(cfg, W, n_streams=1)
    memo, out = {}, []
    for r in rows:
        key = r.tobytes()
        if key not in memo:
            one.reset()
            if r.size:
                assert one.prime_host(r[None, :]) is True and one.info()["evals_done"] == r.size
            memo[key] = one.state_save(0)
            assert memo[key].any() == (r.size > 0), "a reference state must be non-trivial (a zero-length prompt: all zero)"
        out.append(memo[key])
    one.close()
    return out


def _ragged_equals_alone(cfg, seed, lengths, check=None, timeout_ms=0):
    ns = len(lengths)
    W = synth.init_weights(cfg, seed=seed)
    rows = _prompts(seed + 1, lengths)
    refs = _references(cfg, W, rows)
    rs = np.random.RandomState(seed + 2)
    last, uu = rs.randint(0, 256, (ns, 1)), rs.random_sample((ns, N_JOB))
    eng = engine.Engine(cfg, W, n_streams=ns)
    eng.reset()
    assert eng.prime_ragged(rows) is True
    assert eng.info()["evals_done"] == max(lengths)
    for s in (range(ns) if check is None else check):
        assert eng.state_save(s).tobytes() == refs[s].tobytes(), "stream %d (length %d)" % (s, lengths[s])
    job = eng.generate(N_JOB, last, temperature=1.0, uniforms=uu, reset=False, timeout_ms=timeout_ms)
    eng.reset()
    for s in range(ns):
        eng.state_load(refs[s], s, 1)
    want = eng.generate(N_JOB, last, temperature=1.0, uniforms=uu, reset=False, timeout_ms=timeout_ms)
    for s in range(ns):
        assert np.array_equal(job[s], want[s]), "stream %d (length %d)" % (s, lengths[s])
    return eng


@pytest.mark.parametrize("order", ["ascending", "reversed"])
def test_mini3_seams_inside_a_tile(order):
    """the GEMM row tile is 128: seams inside a tile, a stream shorter than a tile, one exactly a tile, one spanning tiles"""
    lengths = rc.MINI3_LENGTHS if order == "ascending" else rc.MINI3_LENGTHS[::-1]
    _ragged_equals_alone(MINI3, 401, lengths).close()


def test_cfg1_around_its_largest_ring():
    _ragged_equals_alone(synth.CONFIGS["cfg1"], 402, [16, 17, 18, 200]).close()   # ring 17, receptive field 63


@pytest.mark.parametrize("cfg", [K3S, K4S], ids=["k3", "k4"])
def test_kernel_size_3_and_4(cfg):
    _ragged_equals_alone(cfg, 403, [0, 1, 8, 9, 140]).close()


def test_a_padded_shape():
    _ragged_equals_alone(_padded_cfg("pad_to_cfg3_shape"), 404, [0, 1, 9, 8, 40]).close()


def test_two_rounds_with_the_longest_stream_in_the_second():
    ns = 170
    cycle = [3, 0, 17, 64, 129]
    lengths = [cycle[s % len(cycle)] for s in range(ns)]
    lengths[120] = 200
    W = synth.init_weights(MINI3, seed=405)
    distinct = {n: p for n, p in zip(cycle + [200], _prompts(406, cycle + [200]))}
    rows = [distinct[n] for n in lengths]
    refs = _references(MINI3, W, rows)
    rs = np.random.RandomState(407)
    last, uu = rs.randint(0, 256, (ns, 1)), rs.random_sample((ns, N_JOB))
    eng = engine.Engine(MINI3, W, n_streams=ns)
    assert eng.info()["n_chains"] == 2
    eng.reset()
    assert eng.prime_ragged(rows) is True and eng.info()["evals_done"] == 200 and max(lengths[:85]) < 200
    for s in (0, 85, 86, 169, 120):
        assert eng.state_save(s).tobytes() == refs[s].tobytes(), "stream %d (length %d)" % (s, lengths[s])
    job = eng.generate(N_JOB, last, temperature=1.0, uniforms=uu, reset=False, timeout_ms=8000)
    eng.reset()
    for s in range(ns):
        eng.state_load(refs[s], s, 1)
    want = eng.generate(N_JOB, last, temperature=1.0, uniforms=uu, reset=False, timeout_ms=8000)
    eng.close()
    assert np.array_equal(job, want)


def test_equal_lengths_are_wn_prime():
    W = synth.init_weights(MINI3, seed=408)
    rows = _prompts(409, [150, 150, 150])
    eng = engine.Engine(MINI3, W, n_streams=3)
    eng.reset()
    assert eng.prime_host(np.stack(rows)) is True
    want = [eng.state_save(s) for s in range(3)]
    eng.reset()
    assert eng.prime_ragged(rows) is True and eng.info()["evals_done"] == 150
    for s in range(3):
        assert want[s].any() and eng.state_save(s).tobytes() == want[s].tobytes()
    eng.reset()
    assert eng.prime_ragged([rows[0][:0]] * 3) is True and eng.info()["evals_done"] == 0   # all lengths 0: nothing happens
    assert not any(eng.state_save(s).any() for s in range(3))
    eng.close()


def test_error_codes_on_a_live_handle():
    W = synth.init_weights(MINI3, seed=410)
    eng = engine.Engine(MINI3, W, n_streams=3)
    d, h, st = eng.lib.dll, eng._h, eng.mem.stream()
    assert eng.lib.has("wn_prime_ragged")
    dev = eng.mem.upload(np.zeros((3, 8), np.int32))
    p = eng.mem.ptr(dev)
    eng.reset()
    for bad in ([4, -1, 2], [4, 9, 2]):   # a negative length, one above row_stride = 8
        assert d.wn_prime_ragged(h, p, (ctypes.c_int64 * 3)(*bad), 8, st) == _abi.WN_E_BADARG and "wn_prime_ragged" in eng.lib.last_error()
        assert eng.info()["evals_done"] == 0 and not any(eng.state_save(s).any() for s in range(3))
    assert d.wn_prime_ragged(h, None, (ctypes.c_int64 * 3)(1, 2, 3), 8, st) == _abi.WN_E_BADARG
    assert d.wn_prime_ragged(h, p, None, 8, st) == _abi.WN_E_BADARG
    # queues that are not fresh: nothing moves
    eng.generate(2, np.full((3, 1), 7), temperature=0.0, reset=False)
    evals, before = eng.info()["evals_done"], [eng.state_save(s) for s in range(3)]
    assert evals > 0 and before[0].any()
    assert d.wn_prime_ragged(h, p, (ctypes.c_int64 * 3)(1, 2, 3), 8, st) == _abi.WN_E_STATE
    with pytest.raises(_abi.WnError) as e:
        eng.prime_ragged([[1], [2, 3], [4, 5, 6]])
    assert e.value.code == _abi.WN_E_STATE
    assert eng.info()["evals_done"] == evals and all(eng.state_save(s).tobytes() == before[s].tobytes() for s in range(3))
    eng.close()


def test_unsupported_where_wn_prime_is():
    eng = engine.Engine(TINY3, synth.init_weights(TINY3, seed=2), n_streams=2)
    row = np.arange(100) % 256
    assert eng.prime_host(np.stack([row, row])) is False
    assert eng.prime_ragged([row, row[:40]]) is False
    dev = eng.mem.upload(np.stack([row, row]).astype(np.int32))
    rc_ = eng.lib.dll.wn_prime_ragged(eng._h, eng.mem.ptr(dev), (ctypes.c_int64 * 2)(100, 40), 100, eng.mem.stream())
    assert rc_ == _abi.WN_E_UNSUPPORTED and "wn_prime_ragged" in eng.lib.last_error()
    assert eng.info()["evals_done"] == 0
    eng.close()


# ---------------------------------------------------------------- the facade
CFG1 = synth.CONFIGS["cfg1"]
LENGTHS = [3, 70, 1, 130]   # below and above Engine.PRIME_BATCH_MIN: the one-stream calls prime through the chain and through the products


def _model(cfg, W):
    m = wavenet_model.WaveNetModel(output_length=8, **cfg)
    m.load_state_dict({k: torch.from_numpy(v) for k, v in W.items()})
    return m


def _greedy_decided(cfg, W, prompts, n):
    """the oracle's greedy indices per prompt, or None when a step's top-2 gap is within ten times the logit tolerance"""
    out = []
    for p in prompts:
        o_idx, o_log = c_oracle.generate(cfg, W, n, p, 0.0, 0.0)
        top2 = np.sort(o_log, axis=1)
        if float((top2[:, -1] - top2[:, -2]).min()) <= 10 * LOGIT_RTOL * max(1.0, float(np.abs(o_log).max())):
            return None
        out.append(o_idx)
    return np.stack(out)


def _greedy_case(cfg, lengths, n, seed0):
    for seed in range(seed0, seed0 + 50):
        W = synth.init_weights(cfg, seed=seed, gain=3.0)
        prompts = _prompts(seed + 1, lengths)
        want = _greedy_decided(cfg, W, prompts, n)
        if want is not None:
            return W, prompts, want
    raise AssertionError("no seed of 50 gives prompts whose greedy continuations the oracle decides")


def test_generate_fast_greedy_rows_are_the_one_stream_calls():
    W, prompts, want = _greedy_case(CFG1, LENGTHS, 30, 420)
    m = _model(CFG1, W)
    audio = m.generate_fast(30, first_samples=[prompts[0], torch.from_numpy(prompts[1]), prompts[2].tolist(), prompts[3]], temperature=0)
    assert m._wn_last_prime_batched is True and audio.shape == (4, 30)
    assert np.array_equal(audio, m._expand_indices(want))
    one = _model(CFG1, W)
    for s, p in enumerate(prompts):
        assert np.array_equal(one.generate_fast(30, first_samples=torch.from_numpy(p), temperature=0), audio[s]), "prompt %d" % s


def test_generate_fast_sampled_rows_state_and_logprobs(monkeypatch):
    N = 30
    W = synth.init_weights(CFG1, seed=430)
    prompts = _prompts(431, LENGTHS)
    decided = [_decided(CFG1, W, N, p, lambda rs: rs.random_sample(N), "prompt %d" % s) for s, p in enumerate(prompts)]
    U, want = np.stack([d[0] for d in decided]), np.stack([d[1] for d in decided])
    feed = []
    monkeypatch.setattr(np.random, "random_sample", lambda size=None: feed.pop(0).copy().reshape(size))
    m = _model(CFG1, W)
    feed[:] = [U]   # ONE draw of (streams, n): the 2-D call's consumption
    audio, states = m.generate_fast(N, first_samples=prompts, return_state=True)
    assert not feed and np.array_equal(audio, m._expand_indices(want))
    assert [st.evals for st in states] == [p.size - 1 + N for p in prompts] and [st.last_index for st in states] == [int(w[-1]) for w in want]
    one = _model(CFG1, W)
    for s, p in enumerate(prompts):
        feed[:] = [U[s]]
        assert np.array_equal(one.generate_fast(N, first_samples=torch.from_numpy(p)), audio[s]), "prompt %d" % s
    # return_state, then continue_from: the one call
    n1 = 12
    feed[:] = [U[:, :n1]]
    a, sts = m.generate_fast(n1, first_samples=prompts, return_state=True)
    feed[:] = [U[:, n1:]]
    b = m.generate_fast(N - n1, continue_from=sts)
    assert np.array_equal(np.concatenate([a, b], axis=1), audio)
    # the model's log-probabilities of a ragged job are score_continuation's of the same rows
    feed[:] = [U]
    audio2, logp = m.generate_fast(N, first_samples=prompts, return_logprobs="model")
    assert not feed and np.array_equal(audio2, audio) and logp.shape == (4, N) and np.isfinite(logp).all()
    greedy, logp_g = m.generate_fast(N, first_samples=prompts, temperature=0, return_logprobs="model")   # (a greedy job, as score_continuation's is)
    table = m._expand_indices(np.arange(256))
    drawn = np.searchsorted(table, greedy)
    assert np.array_equal(table[drawn], greedy)
    scored = m.score_continuation(drawn, first_samples=prompts)
    assert scored.shape == (4, N) and scored.tobytes() == logp_g.tobytes()
    # top_k and forced compose: they concern generated positions only
    forced = np.full((4, N), -1, np.int64)
    forced[:, :5] = want[:, :5]
    feed[:] = [U]
    assert np.array_equal(m.generate_fast(N, first_samples=prompts, forced=forced), audio)


def test_generate_fast_streams_takes_one_prompt_per_temperature(monkeypatch):
    N = 30
    W = synth.init_weights(CFG1, seed=440)
    prompts = _prompts(441, [5, 90, 2])
    temps = [1.0, 0.0, 1.0]
    d0 = _decided(CFG1, W, N, prompts[0], lambda rs: rs.random_sample(N), "prompt 0")
    d2 = _decided(CFG1, W, N, prompts[2], lambda rs: rs.random_sample(N), "prompt 2")
    feed = []
    monkeypatch.setattr(np.random, "random_sample", lambda size=None: feed.pop(0).copy().reshape(size))
    m = _model(CFG1, W)
    feed[:] = [d0[0], d2[0]]   # the sampled rows' draws, in the order of `temperatures`
    rows = m.generate_fast_streams(N, temps, first_samples=prompts)
    assert not feed and rows.shape == (3, N) and m._wn_last_prime_batched is True
    assert np.array_equal(rows[0], m._expand_indices(d0[1])) and np.array_equal(rows[2], m._expand_indices(d2[1]))
    assert m.dilated_queues[0].data.shape[0] == CFG1["residual_channels"]   # (the deferred queues load: the last stream's)
    o_idx, o_log = c_oracle.generate(CFG1, W, N, prompts[1], 0.0, 0.0)
    top2 = np.sort(o_log, axis=1)
    if float((top2[:, -1] - top2[:, -2]).min()) > 10 * LOGIT_RTOL * max(1.0, float(np.abs(o_log).max())):
        assert np.array_equal(rows[1], m._expand_indices(o_idx))
    feed[:] = [d0[0], d2[0]]   # a 1-D prompt stays shared
    shared = m.generate_fast_streams(N, temps, first_samples=torch.from_numpy(prompts[1]))
    assert shared.shape == (3, N) and not feed


def test_fallback_where_the_batched_pass_does_not_apply():
    """TINY3 (kernel_size 3, 16 channels): no matrix-core form; every prompt is primed alone and its state loaded"""
    W, prompts, want = _greedy_case(TINY3, [4, 70, 1], 25, 450)
    m = _model(TINY3, W)
    audio = m.generate_fast(25, first_samples=prompts, temperature=0)
    assert m._wn_last_prime_batched is False and m._wn_engine.info()["forward_native"] == 0
    assert np.array_equal(audio, m._expand_indices(want))
    one = _model(TINY3, W)
    for s, p in enumerate(prompts):
        assert np.array_equal(one.generate_fast(25, first_samples=torch.from_numpy(p), temperature=0), audio[s]), "prompt %d" % s
