"""-m gpu: batched priming onto queues that hold a history (C ABI wn_prime_append, Engine.prime_append, the facade's append= / advance_state /
prime_piece_samples).  Engine level: wherever a row is cut, priming its head and appending its tail leaves BIT for bit the state of a one-stream engine
primed (wn_prime) with the whole row; the result does not depend on the queue time; a stream that appends nothing keeps its bytes.  Against the chain
(another summation order) the queues agree to the bound of test_batched_priming_equals_chain_priming, and the jobs behind them on cases the oracle
decides (the convention of tests/test_gpu_generation_state.py: every sampled draw at least 1e-5 from a CDF boundary)."""
import ctypes
import time

import numpy as np
import pytest
import torch

import append_cases as ac
from mi355_wavenet import _abi, engine, synth
from test_gpu_generation_state import _decided, _padded_cfg
from test_gpu_parity import MINI3
from test_gpu_ragged_prime import N_JOB, _model, _prompts, _references
from test_gpu_taps import K3S, K4S

pytestmark = pytest.mark.gpu
_T0 = time.time()
CFG1 = synth.CONFIGS["cfg1"]
K5S = dict(K3S, kernel_size=5)   # above the matrix-core forms: wn_prime and its siblings answer WN_E_UNSUPPORTED


@pytest.fixture(scope="module", autouse=True)
def _timing():
    yield
    print("\ntest_gpu_prime_append: %.1f s wall" % (time.time() - _T0))


def _same_job(eng, refs, last, uu, job, check=None, timeout_ms=0):
    """the job that was run from the appended queues equals the job of the same engine with the reference states loaded"""
    eng.reset()
    for s, ref in enumerate(refs):
        eng.state_load(ref, s, 1)
    want = eng.generate(N_JOB, last, temperature=1.0, uniforms=uu, reset=False, timeout_ms=timeout_ms)
    for s in (range(len(refs)) if check is None else check):
        assert np.array_equal(job[s], want[s]), "stream %d" % s


def _head_then_tail(cfg, seed, heads, tails, check=None, timeout_ms=0):
    """prime_ragged over every row's head, prime_append over its tail -> the states of the whole rows primed alone, then the same job"""
    ns = len(heads)
    W = synth.init_weights(cfg, seed=seed)
    rows = _prompts(seed + 1, [h + t for h, t in zip(heads, tails)])
    refs = _references(cfg, W, rows)
    rs = np.random.RandomState(seed + 2)
    last, uu = rs.randint(0, 256, (ns, 1)), rs.random_sample((ns, N_JOB))
    eng = engine.Engine(cfg, W, n_streams=ns)
    eng.reset()
    assert eng.prime_ragged([r[:h] for r, h in zip(rows, heads)]) is True and eng.info()["evals_done"] == max(heads)
    assert eng.prime_append([r[h:] for r, h in zip(rows, heads)]) is True
    assert eng.info()["evals_done"] == max(heads) + max(tails)
    for s in (range(ns) if check is None else check):
        assert eng.state_save(s).tobytes() == refs[s].tobytes(), "stream %d (head %d, tail %d)" % (s, heads[s], tails[s])
    job = eng.generate(N_JOB, last, temperature=1.0, uniforms=uu, reset=False, timeout_ms=timeout_ms)
    _same_job(eng, refs, last, uu, job, check, timeout_ms)
    return eng


# ---------------------------------------------------------------- 1. split invariance
@pytest.mark.parametrize("order", ["ascending", "reversed"])
def test_mini3_split_invariance(order):
    lengths = ac.SPLIT_LENGTHS if order == "ascending" else ac.SPLIT_LENGTHS[::-1]
    cuts = ac.split_cuts(lengths)
    assert {0, 1} <= set(cuts) and any(c == n for c, n in zip(cuts, lengths) if n > 1) and any(c == n - 1 for c, n in zip(cuts, lengths) if n > 2)
    _head_then_tail(MINI3, 501, cuts, [n - c for n, c in zip(lengths, cuts)]).close()


# ---------------------------------------------------------------- 2, 3. a live state at a non-zero queue time
LIVE_N, LIVE_APPEND = 37, [0, 1, 5, 200]


@pytest.fixture(scope="module")
def live():
    """4 streams of MINI3 generate 37 samples through the chain -- uniforms the oracle decides --, their states S are saved, rows of 0, 1, 5 and 200
    samples are appended at queue time 37"""
    W = synth.init_weights(MINI3, seed=510)
    rs = np.random.RandomState(511)
    first = rs.randint(0, 256, (4, 1))
    decided = [_decided(MINI3, W, LIVE_N, first[s], lambda r: r.random_sample(LIVE_N), "the live job, stream %d" % s) for s in range(4)]
    U, want = np.stack([d[0] for d in decided]), np.stack([d[1] for d in decided])
    rows = _prompts(512, LIVE_APPEND)
    eng = engine.Engine(MINI3, W, n_streams=4)
    idx = eng.generate(LIVE_N, first, temperature=1.0, uniforms=U, reset=True, batched_prime=False)
    assert np.array_equal(idx, want) and eng.info()["evals_done"] == LIVE_N
    S = [eng.state_save(s) for s in range(4)]
    assert eng.prime_append(rows) is True and eng.info()["evals_done"] == LIVE_N + max(LIVE_APPEND)
    after = [eng.state_save(s) for s in range(4)]
    yield dict(W=W, first=first, want=want, rows=rows, eng=eng, S=S, after=after)
    eng.close()


def test_live_state_does_not_depend_on_the_queue_time(live):
    fresh = engine.Engine(MINI3, live["W"], n_streams=4)
    fresh.reset()
    for s in range(4):
        fresh.state_load(live["S"][s], s, 1)
    assert fresh.info()["evals_done"] == 0
    assert fresh.prime_append(live["rows"]) is True and fresh.info()["evals_done"] == max(LIVE_APPEND)
    for s in range(4):
        assert live["after"][s].any() and fresh.state_save(s).tobytes() == live["after"][s].tobytes(), "stream %d" % s
    fresh.close()


def test_live_state_against_the_chain(live):
    """the same engine from S runs every row as a forced prefix: one chain evaluation per sample, another fp32 summation order"""
    eng = engine.Engine(MINI3, live["W"], n_streams=4)
    for s, row in enumerate(live["rows"]):
        if not row.size:
            continue
        eng.reset()
        eng.state_load(live["S"][s])
        eng.generate(row.size, np.full((4, 1), row[0]), temperature=0.0, forced=np.concatenate([row[1:], [0]]), reset=False)   # inputs row[0 .. size-1]
        assert eng.info()["evals_done"] == row.size
        got, want = live["after"][s], eng.state_save(s)
        err, bound = float(np.abs(got - want).max()), 1e-5 * max(1.0, float(np.abs(want).max()))
        print("[append against the chain] stream %d (%d samples): max |diff| %.3g, bound %.3g" % (s, row.size, err, bound))
        assert err <= bound
    eng.close()


def test_live_state_then_a_job_the_oracle_decides(live):
    """the job behind the append draws what the oracle draws after the stream's whole input history"""
    n = 20
    last = np.random.RandomState(513).randint(0, 256, (4, 1))
    cases = []
    for s in range(4):   # inputs so far: the first sample, 36 of the 37 drawn ones (the last was never fed), the appended row; then `last`
        history = np.concatenate([live["first"][s], live["want"][s][:LIVE_N - 1], live["rows"][s], last[s]])
        cases.append(_decided(MINI3, live["W"], n, history, lambda r: r.random_sample(n), "the job behind the append, stream %d" % s))
    U, want = np.stack([c[0] for c in cases]), np.stack([c[1] for c in cases])
    eng = live["eng"]
    assert eng.info()["evals_done"] == LIVE_N + max(LIVE_APPEND)
    assert np.array_equal(eng.generate(n, last, temperature=1.0, uniforms=U, reset=False), want)


def test_a_stream_that_appends_nothing_keeps_its_bytes(live):
    assert LIVE_APPEND[0] == 0 and live["S"][0].any()
    assert live["after"][0].tobytes() == live["S"][0].tobytes()   # all rows of every block, the dead oldest one included
    assert live["after"][1].tobytes() != live["S"][1].tobytes()


# ---------------------------------------------------------------- 4, 5. ring edges, kernel_size 3 and 4, a padded shape
@pytest.mark.parametrize("turn", range(4))
def test_cfg1_around_its_largest_ring(turn):
    """ring 17, receptive field 63: histories below / at / above the ring and beyond the field, each with an append of 1, 16, 17 and 64"""
    tails = [1, 16, 17, 64]
    _head_then_tail(CFG1, 520 + turn, [16, 17, 18, 200], tails[turn:] + tails[:turn]).close()


@pytest.mark.parametrize("cfg", [K3S, K4S, _padded_cfg("pad_to_cfg3_shape")], ids=["k3", "k4", "padded"])
def test_kernel_size_3_and_4_and_a_padded_shape(cfg):
    _head_then_tail(cfg, 530, [3, 0, 9, 40, 1], [0, 1, 8, 9, 140]).close()


# ---------------------------------------------------------------- 6. the shared form
def _shared_case(seed, n_head=50, n_tail=130):
    W = synth.init_weights(MINI3, seed=seed)
    row = _prompts(seed + 1, [n_head + n_tail])[0]
    head, whole = _references(MINI3, W, [row[:n_head], row])
    return W, row[n_head:], head, whole


def test_shared_form_equals_the_per_stream_append():
    W, tail, head, whole = _shared_case(540)
    eng = engine.Engine(MINI3, W, n_streams=5)
    eng.reset()
    eng.state_load(head)
    assert eng.prime_append([tail] * 5) is True and eng.info()["evals_done"] == 130
    per_stream = [eng.state_save(s) for s in range(5)]
    eng.reset()
    eng.state_load(head)
    assert eng.prime_append(tail, shared=True) is True and eng.info()["evals_done"] == 130
    for s in range(5):
        assert eng.state_save(s).tobytes() == per_stream[s].tobytes() == whole.tobytes(), "stream %d" % s
    eng.close()


def test_shared_form_through_two_rounds():
    W, tail, head, whole = _shared_case(541)
    eng = engine.Engine(MINI3, W, n_streams=170)
    assert eng.info()["n_chains"] == 2
    eng.reset()
    eng.state_load(head)
    assert eng.prime_append(tail, shared=True) is True and eng.info()["evals_done"] == 130
    for s in (0, 85, 86, 169):
        assert eng.state_save(s).tobytes() == whole.tobytes(), "stream %d" % s
    eng.close()


# ---------------------------------------------------------------- 7. two rounds, ragged
def test_two_rounds_ragged_with_the_longest_append_in_the_second():
    ns = 170
    cycle, head_cycle = [3, 0, 17, 64, 129], [5, 0, 40]
    tails = [cycle[s % len(cycle)] for s in range(ns)]
    tails[120] = 200
    heads = [head_cycle[s % len(head_cycle)] for s in range(ns)]
    W = synth.init_weights(MINI3, seed=550)
    head_row = {n: p for n, p in zip(head_cycle, _prompts(551, head_cycle))}
    tail_row = {n: p for n, p in zip(cycle + [200], _prompts(552, cycle + [200]))}
    rows = [np.concatenate([head_row[h], tail_row[t]]) for h, t in zip(heads, tails)]
    refs = _references(MINI3, W, rows)
    rs = np.random.RandomState(553)
    last, uu = rs.randint(0, 256, (ns, 1)), rs.random_sample((ns, N_JOB))
    eng = engine.Engine(MINI3, W, n_streams=ns)
    assert eng.info()["n_chains"] == 2 and max(tails[:85]) < 200
    eng.reset()
    assert eng.prime_ragged([head_row[h] for h in heads]) is True and eng.info()["evals_done"] == 40
    assert eng.prime_append([tail_row[t] for t in tails]) is True and eng.info()["evals_done"] == 240
    for s in (0, 85, 86, 169, 120):
        assert eng.state_save(s).tobytes() == refs[s].tobytes(), "stream %d (head %d, tail %d)" % (s, heads[s], tails[s])
    job = eng.generate(N_JOB, last, temperature=1.0, uniforms=uu, reset=False, timeout_ms=8000)
    _same_job(eng, refs, last, uu, job, timeout_ms=8000)
    eng.close()


# ---------------------------------------------------------------- 8. error codes through raw ctypes
def test_error_codes_on_a_live_handle():
    W = synth.init_weights(MINI3, seed=560)
    eng = engine.Engine(MINI3, W, n_streams=3)
    d, h, st = eng.lib.dll, eng._h, eng.mem.stream()
    assert eng.lib.has("wn_prime_append") and eng.lib.has("wn_prime_ragged")
    dev = eng.mem.upload(np.zeros((3, 8), np.int32))
    p = eng.mem.ptr(dev)
    eng.generate(2, np.full((3, 1), 7), temperature=0.0, reset=True)
    evals, before = eng.info()["evals_done"], [eng.state_save(s) for s in range(3)]
    assert evals == 2 and before[0].any()

    def untouched():
        return eng.info()["evals_done"] == evals and all(eng.state_save(s).tobytes() == before[s].tobytes() for s in range(3))
    for bad in ([4, -1, 2], [4, 9, 2]):   # a negative length, one above row_stride = 8
        assert d.wn_prime_append(h, p, (ctypes.c_int64 * 3)(*bad), 8, 0, st) == _abi.WN_E_BADARG and "wn_prime_append" in eng.lib.last_error()
    assert d.wn_prime_append(h, p, (ctypes.c_int64 * 1)(9), 8, 1, st) == _abi.WN_E_BADARG   # the shared form's one length
    assert d.wn_prime_append(h, None, (ctypes.c_int64 * 3)(1, 2, 3), 8, 0, st) == _abi.WN_E_BADARG
    assert d.wn_prime_append(h, p, None, 8, 0, st) == _abi.WN_E_BADARG
    assert d.wn_prime_append(None, p, (ctypes.c_int64 * 3)(1, 2, 3), 8, 0, st) == _abi.WN_E_BADARG
    assert untouched()
    assert d.wn_prime_append(h, p, (ctypes.c_int64 * 3)(0, 0, 0), 8, 0, st) == _abi.WN_OK and untouched()   # all lengths 0: nothing happens
    assert d.wn_prime_ragged(h, p, (ctypes.c_int64 * 3)(1, 2, 3), 8, st) == _abi.WN_E_STATE and untouched()   # the fresh-queue forms keep their check
    assert d.wn_prime_append(h, p, (ctypes.c_int64 * 3)(1, 2, 3), 8, 0, st) == _abi.WN_OK and eng.info()["evals_done"] == evals + 3
    eng.close()
    # before wn_load_weights
    c = _abi.wn_config(MINI3["layers"], MINI3["blocks"], MINI3["dilation_channels"], MINI3["residual_channels"], MINI3["skip_channels"], MINI3["end_channels"],
                       256, 2, 0, 2, 0, 0, 0)
    raw = ctypes.c_void_p()
    assert d.wn_create(ctypes.byref(c), ctypes.byref(raw)) == 0
    try:
        row = torch.zeros(16, dtype=torch.int32, device="cuda")
        assert d.wn_prime_append(raw, row.data_ptr(), (ctypes.c_int64 * 2)(8, 3), 8, 0, st) == _abi.WN_E_STATE and "wn_load_weights" in eng.lib.last_error()
    finally:
        d.wn_destroy(raw)


def test_unsupported_where_wn_prime_is():
    eng = engine.Engine(K5S, synth.init_weights(K5S, seed=561), n_streams=2)
    eng.generate(3, np.full((2, 1), 9), temperature=0.0, reset=True)
    evals, before = eng.info()["evals_done"], [eng.state_save(s) for s in range(2)]
    assert evals == 3 and before[0].any()
    row = np.arange(100) % 256
    assert eng.prime_append([row, row[:40]]) is False and eng.prime_append(row, shared=True) is False
    dev = eng.mem.upload(np.stack([row, row]).astype(np.int32))
    rc_ = eng.lib.dll.wn_prime_append(eng._h, eng.mem.ptr(dev), (ctypes.c_int64 * 2)(100, 40), 100, 0, eng.mem.stream())
    assert rc_ == _abi.WN_E_UNSUPPORTED and "wn_prime_append" in eng.lib.last_error()
    assert eng.info()["evals_done"] == evals and all(eng.state_save(s).tobytes() == before[s].tobytes() for s in range(2))
    eng.close()


# ---------------------------------------------------------------- 9. the facade
def _same_state(a, b):
    return a.state.tobytes() == b.state.tobytes() and a.evals == b.evals and a.last_index == b.last_index


def test_generate_fast_append_is_the_concatenated_prompt():
    N = 30
    W = synth.init_weights(CFG1, seed=570)
    A, B = _prompts(571, [80, 50])
    m = _model(CFG1, W)
    np.random.seed(5)
    audio, logp, state = m.generate_fast(N, first_samples=torch.from_numpy(np.concatenate([A, B])), return_logprobs="model", return_state=True)
    assert m._wn_last_prime_batched is True and state.evals == 129 + N
    _, st_a = m.generate_fast(0, first_samples=torch.from_numpy(A), return_state=True)
    assert st_a.evals == 79 and st_a.last_index == int(A[-1])
    np.random.seed(5)
    audio2, logp2, state2 = m.generate_fast(N, continue_from=st_a, append=B, return_logprobs="model", return_state=True)
    assert m._wn_last_prime_batched is True and audio2.shape == (N,)
    assert np.array_equal(audio2, audio) and logp2.tobytes() == logp.tobytes() and _same_state(state2, state)
    # advance_state: a state and samples -> a state; nothing is drawn
    _, st_ab = m.generate_fast(0, first_samples=torch.from_numpy(np.concatenate([A, B])), return_state=True)
    before = np.random.get_state()[1].copy()
    assert _same_state(m.advance_state(st_a, B), st_ab) and np.array_equal(np.random.get_state()[1], before)
    assert _same_state(m.advance_state(st_a, B[:0]), st_a)
    # score_continuation composes: the clip behind the appended audio
    clip = _prompts(572, [12])[0]
    assert m.score_continuation(clip, continue_from=st_a, append=B).tobytes() == m.score_continuation(clip, continue_from=st_ab).tobytes()


def test_generate_fast_append_on_a_list_of_states_and_streams():
    N = 30
    W = synth.init_weights(CFG1, seed=573)
    heads, tails = _prompts(574, [80, 70, 100]), _prompts(575, [0, 5, 66])
    whole = [np.concatenate([a, b]) for a, b in zip(heads, tails)]
    m = _model(CFG1, W)
    np.random.seed(6)
    audio, states = m.generate_fast(N, first_samples=whole, return_state=True)
    _, st_heads = m.generate_fast(0, first_samples=heads, return_state=True)
    np.random.seed(6)
    audio2, states2 = m.generate_fast(N, continue_from=st_heads, append=[t.tolist() for t in tails], return_state=True)
    assert m._wn_last_prime_batched is True and audio2.shape == (3, N) and np.array_equal(audio2, audio)
    assert all(_same_state(a, b) for a, b in zip(states2, states)) and [st.evals for st in states2] == [w.size - 1 + N for w in whole]
    assert all(_same_state(a, b) for a, b in zip(m.advance_state(st_heads, tails), m.generate_fast(0, first_samples=whole, return_state=True)[1]))
    # generate_fast_streams: ONE state, ONE sequence, the shared form
    temps = [1.0, 0.0, 0.7]
    np.random.seed(7)
    rows = m.generate_fast_streams(N, temps, first_samples=torch.from_numpy(whole[2]))
    np.random.seed(7)
    rows2 = m.generate_fast_streams(N, temps, continue_from=st_heads[2], append=tails[2])
    assert m._wn_last_prime_batched is True and rows2.shape == (3, N) and np.array_equal(rows2, rows)


def test_prime_piece_samples_gives_the_bytes_of_one_pass():
    W = synth.init_weights(CFG1, seed=576)
    prompts = _prompts(577, [300, 65, 64, 129, 10])
    m = _model(CFG1, W)
    _, one_pass = m.generate_fast(0, first_samples=prompts, return_state=True)
    shared = m.generate_fast_streams(20, [0.0, 0.0], first_samples=torch.from_numpy(prompts[0]))
    rect = m.generate_fast(20, first_samples=torch.from_numpy(np.stack([prompts[0], prompts[0][::-1].copy()])), temperature=0)
    m.prime_piece_samples = 64
    _, pieces = m.generate_fast(0, first_samples=prompts, return_state=True)
    assert m._wn_last_prime_batched is True and all(_same_state(a, b) for a, b in zip(pieces, one_pass))
    assert np.array_equal(m.generate_fast_streams(20, [0.0, 0.0], first_samples=torch.from_numpy(prompts[0])), shared)
    assert np.array_equal(m.generate_fast(20, first_samples=torch.from_numpy(np.stack([prompts[0], prompts[0][::-1].copy()])), temperature=0), rect)


def test_fallback_where_the_batched_pass_does_not_apply():
    """kernel_size 5: the state is loaded and [last_index, *append] primed through the chain -- the audio of the concatenated prompt"""
    W = synth.init_weights(K5S, seed=578, gain=3.0)
    A, B, A2 = _prompts(579, [20, 30, 9])
    m = _model(K5S, W)
    audio = m.generate_fast(25, first_samples=torch.from_numpy(np.concatenate([A, B])), temperature=0)
    assert m._wn_last_prime_batched is False
    _, st_a = m.generate_fast(0, first_samples=torch.from_numpy(A), return_state=True)
    assert np.array_equal(m.generate_fast(25, continue_from=st_a, append=B, temperature=0), audio) and m._wn_last_prime_batched is False
    both = m.generate_fast(25, first_samples=[np.concatenate([A, B]), A2], temperature=0)
    _, sts = m.generate_fast(0, first_samples=[A, A2], return_state=True)
    assert np.array_equal(m.generate_fast(25, continue_from=sts, append=[B, []], temperature=0), both) and np.array_equal(both[0], audio)
