"""-m gpu: the per-sample log-probabilities of the sampler kernels (include/wn_abi.h wn_set_logprob_output) through whole jobs of the persistent chain,
on every kernel that draws -- the wave-specialised kernel in its one- and two-streams-per-item forms, the slot re-use form's filter kernel, the stacked
kernel, the generic kernel at 256 classes and at 300.

1. Whole jobs on random weights: every job is run with the logits dump AND the log-probabilities, and every draw is replayed on the job's own float32
   logits through the float64 statement of the contract (logprob_cases.logp64) for the class the kernel returned: |logp - logp64| <= logprob_cases.bound,
   which is derived, not measured.  A draw whose filter membership the float64 replay cannot decide (sampler_filter_cases.filter64) is left out; at most
   2 % of a job's draws may be.  Indices are those of the job without log-probabilities, the values those of the job without the dump, bit for bit.
2. Exact rows: end_conv_2.weight = 0 makes every step's logits end_conv_2.bias.
3. A job of two rounds.  4. Model mode against the oracle's teacher-forced logits.  5. Error codes on a live handle.  6. The facade.
The shapes, pins, N = 64 after 3 given and the seed style are tests/test_gpu_sampling_filters.py's."""
import ctypes
import math

import numpy as np
import pytest
import torch

import logprob_cases as lc
import sampler_cases as sc
import sampler_filter_cases as fc
from mi355_wavenet import _abi, engine, synth
from parity_common import LOGIT_RTOL, check_engine, make_case, oracle_run
from test_gpu_parity import MINI3
from test_gpu_sampling_filters import FILTERS, N, N_GIVEN, SHAPES, TEMPS

pytestmark = pytest.mark.gpu

UNDECIDED_CAP = 0.02
TINY300 = dict(synth.CONFIGS["tiny"], classes=300)       # 16 chunks of 19 classes, the last one short: the generic kernel at another class count
LP_SHAPES = SHAPES + [("tiny300_generic", TINY300, 2, {"WN_KERNEL": "generic"}, 1)]
KW = dict(batched_prime=False, timeout_ms=8000)


class Worst:
    """the largest err / bound seen, per label"""
    def __init__(self):
        self.seen = {}

    def add(self, label, ratio):
        self.seen[label] = max(self.seen.get(label, 0.0), ratio)


def _check(got, want, C, A, what):
    """one value against the float64 statement -> err / bound"""
    if want == -math.inf:
        assert got == -math.inf, "%s: %r, the class is outside the kept set" % (what, got)
        return 0.0
    b = lc.bound(want, C, A)
    err = abs(float(got) - want)
    assert err <= b, "%s: logp %r, logp64 %r, error %.3g > bound %.3g" % (what, float(got), want, err, b)
    return err / b


def _replay(idx, logits, logp, reg, temps, top_k, top_p, mode, A, label, worst):
    """every draw of the job against logp64 on the job's own logits; temps: one temperature per stream (<= 0: greedy) -> membership-undecided draws"""
    C = logits.shape[2]
    undecided = 0
    assert logp.shape == idx.shape and logp.dtype == np.float32
    for s in range(idx.shape[0]):
        greedy = not temps[s] > 0
        for t in range(idx.shape[1]):
            if mode == "sampling" and not lc.kept64(logits[s, t], reg, temps[s], greedy, top_k, top_p)[2]:
                undecided += 1
                continue
            want = lc.logp64(logits[s, t], reg, temps[s], greedy, top_k, top_p, idx[s, t], mode)
            worst.add("%s %s" % (label.split(" ")[0], mode), _check(logp[s, t], want, C, A, "%s stream %d step %d" % (label, s, t)))
    assert undecided <= UNDECIDED_CAP * idx.size, "%s: %d of %d draws membership-undecided" % (label, undecided, idx.size)
    return undecided


def _engine_for(label, cfgname, ns, env, variant, monkeypatch, seed):
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    cfg, W, first, u = make_case(cfgname, seed, ns, N_GIVEN, N)
    eng = engine.Engine(cfg, W, n_streams=ns)
    assert eng.info()["kernel_variant"] == variant, eng.info()
    if "WN_V3_SLOTS" in env:
        assert eng.info()["skip_lane_slots"] == int(env["WN_V3_SLOTS"]), eng.info()
    return eng, cfg, W, first, u


# ---------------------------------------------------------------- 1. whole jobs on random weights
@pytest.mark.parametrize("label,cfgname,ns,env,variant", LP_SHAPES, ids=[s[0] for s in LP_SHAPES])
def test_whole_jobs(label, cfgname, ns, env, variant, monkeypatch):
    eng, cfg, W, first, u = _engine_for(label, cfgname, ns, env, variant, monkeypatch, 131)
    C = cfg.get("classes", 256)
    A = lc.a_of(variant, C)
    kw = dict(KW, uniforms=u)
    worst = Worst()
    before = {T: eng.generate(N, first, temperature=T, **kw) for T in TEMPS}
    undecided = []
    for top_k, top_p in ((0, 0.0),) + FILTERS:
        for T in TEMPS:
            plain = eng.generate(N, first, temperature=T, top_k=top_k, top_p=top_p, **kw)       # (the handle keeps the filter for the jobs below)
            for mode in lc.MODES:
                tag = "%s (%d, %g) T=%g %s" % (label, top_k, top_p, T, mode)
                idx, logits, logp = eng.generate(N, first, temperature=T, want_logits=True, logprobs=mode, **kw)
                assert np.array_equal(idx, plain), tag + ": the indices of the job without log-probabilities"
                undecided.append(_replay(idx, logits, logp, None, [T] * ns, top_k, top_p, mode, A, tag, worst))
                idx2, logp2 = eng.generate(N, first, temperature=T, logprobs=mode, **kw)
                assert np.array_equal(idx2, plain) and logp2.tobytes() == logp.tobytes(), tag + ": the job without the logits dump"
    # the regulariser enters the sampling mode's row and not the model mode's
    reg = engine.regularizer_array(C, sc.REGULARIZE)
    eng.set_sampling(0, 0.0)
    for mode in lc.MODES:
        idx, logits, logp = eng.generate(N, first, temperature=1.0, regularize=sc.REGULARIZE, want_logits=True, logprobs=mode, **kw)
        _replay(idx, logits, logp, reg, [1.0] * ns, 0, 0.0, mode, A, "%s regulariser %s" % (label, mode), worst)
    # every second stream (the only one of a single-stream job) greedy by its temperature: the greedy statement there, the sampled one next to it
    temps = np.array([0.0 if (s % 2 == 1 or ns == 1) else 1.0 for s in range(ns)], dtype=np.float32)
    for mode in lc.MODES:
        idx, logits, logp = eng.generate(N, first, temperature=temps, want_logits=True, logprobs=mode, top_k=8, top_p=0.0, **kw)
        _replay(idx, logits, logp, None, temps, 8, 0.0, mode, A, "%s per-stream temperatures %s" % (label, mode), worst)
    # a greedy job (no uniforms) is armed like any other
    g_plain = eng.generate(N, first, temperature=0.0, **KW)
    for mode in lc.MODES:
        idx, logits, logp = eng.generate(N, first, temperature=0.0, want_logits=True, logprobs=mode, **KW)
        assert np.array_equal(idx, g_plain)
        _replay(idx, logits, logp, None, [0.0] * ns, 8, 0.0, mode, A, "%s greedy job %s" % (label, mode), worst)
    # after the armed jobs a plain job returns what it returned before, and the engine still agrees with the oracle
    eng.set_sampling(0, 0.0)
    for T in TEMPS:
        assert np.array_equal(eng.generate(N, first, temperature=T, **kw), before[T]), "%s: a plain job after the armed ones, T = %g" % (label, T)
    check_engine(eng, cfg, W, N, first, 1.0, 0.0, u, label + " after the log-probabilities")
    eng.close()
    print(label, "worst err / bound:", {k: round(v, 3) for k, v in sorted(worst.seen.items())}, "membership-undecided draws per job:", undecided)


# ---------------------------------------------------------------- 2. exact rows through the product kernels
PEAK = np.float32(20.0)
TIES = (2, 3, 63, 64, 255)     # inside a lane (classes 0-3), across the seam of two 16-lane rows (classes 60-63 | 64-67), the last class


def _flat():
    return np.zeros(256, np.float32)


def _peak(shift=0.0):
    x = np.full(256, np.float32(shift), np.float32)
    x[0] = np.float32(shift) + PEAK
    return x


def _ramp():
    return (np.float32(0) - np.float32(0.05) * np.arange(256, dtype=np.float32)).astype(np.float32)      # (class 0: +0.0, as the head's sum gives it)


def _tied():
    x = np.full(256, np.float32(-0.7), np.float32)
    x[list(TIES)] = np.float32(0)
    return x


def _mid(bias, T, top_k, top_p, classes):
    """the midpoints of the float64 CDF intervals of `classes`: the uniforms that land on them"""
    x = sc.x32(bias, None, T, False)
    cdf = fc.cdf64_filtered(x, fc.filter64(x, top_k, top_p)[0])
    return [0.5 * ((cdf[i - 1] if i else 0.0) + cdf[i]) for i in classes]


# (name, end_conv_2.bias, temperature, (top_k, top_p), the uniforms of every stream or None for a greedy job, the classes they land on or None)
def _exact_rows():
    rows = [("flat", _flat(), 1.0, (0, 0.0), [(j + 0.5) / 256 for j in (0, 3, 4, 63, 64, 128, 200, 255)], [0, 3, 4, 63, 64, 128, 200, 255])]
    # one class at +20: the peak holds 1 - 5.3e-7 of the mass.  u = 1 - 1e-7 lies 4.3e-7 behind the peak's CDF value -- the fp32 roundings of 1 / sum and
    # of mass * (1 / sum) move that value by 1.2e-7 at most -- and the tail's steps are 2e-9 wide: no uniform there is BAND from a boundary, so the tail
    # draws are asserted to be tail classes, not one class; the class the kernel returned is the one scored (about -20)
    for name, shift in (("peak", 0.0), ("peak-30", -30.0), ("peak+30", 30.0)):
        rows.append((name, _peak(shift), 1.0, (0, 0.0), [0.3, 1 - 1e-7, 0.5, 0.999, 1 - 1e-7, 0.01, 0.7, 1 - 1e-7], [0, None, 0, 0, None, 0, 0, None]))
    kept8 = list(range(8))
    rows.append(("ramp top_k 8", _ramp(), 1.0, (8, 0.0), _mid(_ramp(), 1.0, 8, 0.0, kept8), kept8))
    x = sc.x32(_ramp(), None, 1.0, False)
    nucleus = np.nonzero(fc.filter64(x, 0, 0.5)[0])[0].tolist()
    assert fc.filter64(x, 0, 0.5)[1] and 8 < len(nucleus) < 40
    pick = nucleus[:3] + nucleus[len(nucleus) // 2:len(nucleus) // 2 + 2] + nucleus[-3:]
    rows.append(("ramp top_p 0.5", _ramp(), 1.0, (0, 0.5), _mid(_ramp(), 1.0, 0, 0.5, pick), pick))
    order = [2, 255, 63, 64, 3, 2, 64, 255]
    rows.append(("ties top_k 3", _tied(), 1.0, (3, 0.0), [(TIES.index(c) + 0.5) / len(TIES) for c in order], order))
    rows.append(("ties greedy", _tied(), 0.0, (0, 0.0), None, [2] * 8))
    sharp = [0, 1, 2, 0, 3, 1, 0, 5]
    rows.append(("ramp T 0.05", _ramp(), 0.05, (0, 0.0), _mid(_ramp(), 0.05, 0, 0.0, sharp), sharp))
    for name, bias, T, (top_k, top_p), us, lands in rows:      # every uniform at least BAND from a boundary of the float64 CDF (the tail draws: see above)
        if us is not None:
            x = sc.x32(bias, None, T, False)
            cdf = fc.cdf64_filtered(x, fc.filter64(x, top_k, top_p)[0])
            for u, c in zip(us, lands):
                assert c is None or (sc.margin(cdf, u) >= sc.BAND and sc.pick(cdf, u) == c), (name, u, c)
    return rows


EXACT_SHAPES = [s for s in SHAPES if s[0] in ("lean4_ns4", "cfg1_ns1_v4", "tiny_generic")]


@pytest.mark.parametrize("label,cfgname,ns,env,variant", EXACT_SHAPES, ids=[s[0] for s in EXACT_SHAPES])
def test_exact_rows(label, cfgname, ns, env, variant, monkeypatch):
    eng, cfg, W, first, _ = _engine_for(label, cfgname, ns, env, variant, monkeypatch, 142)
    A = lc.a_of(variant, 256)
    worst = Worst()
    W = dict(W)
    W["end_conv_2.weight"] = np.zeros_like(W["end_conv_2.weight"])
    n = 8
    values_peak = None
    for name, bias, T, (top_k, top_p), us, lands in _exact_rows():
        W["end_conv_2.bias"] = bias
        eng.load_weights(W)
        u = np.tile(np.asarray(us, np.float64), (ns, 1)) if us is not None else None
        values = {}
        for mode in lc.MODES:
            tag = "%s %s %s" % (label, name, mode)
            idx, logits, logp = eng.generate(n, first, temperature=T, uniforms=u, want_logits=True, logprobs=mode, top_k=top_k, top_p=top_p, **KW)
            assert logits.tobytes() == np.broadcast_to(bias, logits.shape).tobytes(), tag + ": every step's logits are end_conv_2.bias"
            for s in range(ns):
                for t in range(n):
                    if lands[t] is None:
                        assert idx[s, t] != 0, tag + ": u = 1 - 1e-7 lands behind the peak"
                    else:
                        assert idx[s, t] == lands[t], "%s stream %d step %d: class %d, expected %d" % (tag, s, t, idx[s, t], lands[t])
            _replay(idx, logits, logp, None, [T] * ns, top_k, top_p, mode, A, tag, worst)
            values[mode] = logp
        kept = lambda v: np.abs(values["sampling"] - v).max() <= lc.bound(v, 256, A)  # noqa: E731
        if name == "flat":
            assert kept(-math.log(256))
        if name == "ties top_k 3":
            assert kept(-math.log(len(TIES)))
        if name == "ties greedy":      # the T = 1 log-softmax value of the whole row, the same in both modes
            assert kept(-math.log(len(TIES) + (256 - len(TIES)) * math.exp(float(np.float32(-0.7)))))
            assert np.abs(values["model"] - values["sampling"]).max() <= 2 * lc.bound(values["model"].min(), 256, A)
        if name.startswith("peak"):
            tail = np.array([c is None for c in lands])
            assert np.abs(values["model"][:, tail] + 20.0).max() < 1e-4 and np.abs(values["model"][:, ~tail]).max() < 1e-5
            if name == "peak":
                values_peak = values
            for mode in lc.MODES:      # the shifted rows: the same values inside the bound (each is within it of the same float64 value)
                assert np.abs(values[mode] - values_peak[mode]).max() <= 2 * lc.bound(-20.0, 256, A), "%s %s against the unshifted row" % (label, name)
    eng.set_sampling(0, 0.0)
    eng.close()
    print(label, "exact rows, worst err / bound:", {k: round(v, 3) for k, v in sorted(worst.seen.items())})


# ---------------------------------------------------------------- armed by hand: a caller's own buffer
def _armed(eng, buf, capacity, mode, num_samples, first, **kw):
    """one job that writes its log-probabilities into the caller's device tensor `buf`"""
    eng.set_logprob_output(buf, capacity, mode)
    return eng.generate(num_samples, first, **kw)


# ---------------------------------------------------------------- 3. rounds
def test_rounds_write_every_members_slice():
    ns, n = 170, 8
    cfg, W, first, u = make_case(MINI3, 143, ns, N_GIVEN, n)
    eng = engine.Engine(cfg, W, n_streams=ns)
    assert eng.info()["n_chains"] == 2 and eng.info()["kernel_variant"] == 3
    buf = torch.full((ns, n), float("nan"), dtype=torch.float32, device=eng.mem.device)
    idx, logits = _armed(eng, buf, ns * n, "model", n, first, temperature=1.0, uniforms=u, want_logits=True, timeout_ms=8000)
    logp = buf.cpu().numpy()
    assert not np.isnan(logp).any(), "every float of the array is written: %d NaN left" % int(np.isnan(logp).sum())
    worst = Worst()
    for s in (0, 85, 86, 169):        # the first round's first and last stream, the second round's
        _replay(idx[s:s + 1], logits[s:s + 1], logp[s:s + 1], None, [1.0], 0, 0.0, "model", lc.A_ONE_WAVE, "rounds stream %d" % s, worst)
    assert np.array_equal(eng.generate(n, first, temperature=1.0, uniforms=u, timeout_ms=8000), idx)
    eng.close()
    print("rounds worst err / bound:", worst.seen)


# ---------------------------------------------------------------- 4. model mode against the oracle
ORACLE_SHAPES = [s for s in SHAPES if s[0] in ("lean4_ns4", "cfg1_ns1_v4")]


@pytest.mark.parametrize("label,cfgname,ns,env,variant", ORACLE_SHAPES, ids=[s[0] for s in ORACLE_SHAPES])
def test_model_mode_against_the_oracle(label, cfgname, ns, env, variant, monkeypatch):
    eng, cfg, W, first, u = _engine_for(label, cfgname, ns, env, variant, monkeypatch, 144)
    idx, logp = eng.generate(N, first, temperature=1.0, uniforms=u, logprobs="model", **KW)
    eng.close()
    worst = 0.0
    for s in range(ns):
        _, o_log = oracle_run(cfg, W, N, first[s], 1.0, 0.0, u[s], forced=idx[s])
        tol = 2 * LOGIT_RTOL * max(1.0, float(np.abs(o_log).max()))      # check_engine's logit tolerance, once for l_i and once for the log-sum
        for t in range(N):
            want = lc.logp64(o_log[t], None, 1.0, False, 0, 0.0, idx[s, t], "model")
            err, b = abs(float(logp[s, t]) - want), tol + lc.bound(want, 256, lc.A_ONE_WAVE)
            worst = max(worst, err / b)
            assert err <= b, "%s stream %d step %d: logp %r, the oracle's %r, error %.3g > %.3g" % (label, s, t, float(logp[s, t]), want, err, b)
    print(label, "model mode against the oracle, worst err / (logit tolerance + bound): %.3f" % worst)


# ---------------------------------------------------------------- 5. error codes on a live handle
def test_error_codes_on_a_live_handle():
    ns, n = 2, 8
    cfg, W, first, u = make_case("tiny", 145, ns, N_GIVEN, n)
    eng = engine.Engine(cfg, W, n_streams=ns)
    kw = dict(temperature=1.0, uniforms=u, batched_prime=False)
    plain = eng.generate(n, first, **kw)
    sentinel = lambda: torch.full((ns, n), -7.0, dtype=torch.float32, device=eng.mem.device)  # noqa: E731
    intact = lambda b: bool((b == -7.0).all().item())  # noqa: E731
    buf = sentinel()
    with pytest.raises(_abi.WnError) as e:            # one float short: refused, nothing launched
        _armed(eng, buf, ns * n - 1, "model", n, first, **kw)
    assert e.value.code == _abi.WN_E_BADARG and "log-probability" in str(e.value)
    assert np.array_equal(eng.generate(n, first, **kw), plain) and intact(buf), "the refused job ran nothing, and its arming is consumed"
    eng.set_logprob_output(buf, ns * n, "sampling")   # arm, disarm, run
    eng.set_logprob_output(None, 0, "sampling")
    assert np.array_equal(eng.generate(n, first, **kw), plain) and intact(buf)
    d, h = eng.lib.dll, eng._h
    for mode in (2, -1):
        assert d.wn_set_logprob_output(h, ctypes.c_void_p(buf.data_ptr()), ns * n, mode) == _abi.WN_E_BADARG and "wn_set_logprob_output" in eng.lib.last_error()
    assert d.wn_set_logprob_output(h, ctypes.c_void_p(buf.data_ptr()), -1, 0) == _abi.WN_E_BADARG
    assert np.array_equal(eng.generate(n, first, **kw), plain) and intact(buf), "a refused call armed nothing"
    idx = _armed(eng, buf, ns * n, "sampling", n, first, **kw)          # exactly enough: written, once
    assert np.array_equal(idx, plain) and not (buf == -7.0).any().item()
    written = buf.clone()
    eng.generate(n, first, temperature=0.5, uniforms=u, batched_prime=False)
    assert torch.equal(buf, written), "the job after an armed one writes nothing"
    eng.close()


# ---------------------------------------------------------------- 6. the facade
def _model(seed):
    import wavenet_model
    cfg = synth.CONFIGS["cfg1"]
    W = synth.init_weights(cfg, seed=seed)
    m = wavenet_model.WaveNetModel(output_length=8, **cfg)
    m.load_state_dict({k: torch.from_numpy(v) for k, v in W.items()})
    return m, cfg, W


def test_facade_logprobs_and_rng_consumption():
    m, cfg, W = _model(146)
    np.random.seed(5)
    plain = m.generate_fast(64, temperature=1.)
    state = np.random.get_state()
    np.random.seed(5)
    out = m.generate_fast(64, temperature=1., return_logprobs="model")
    after = np.random.get_state()
    assert isinstance(out, tuple) and len(out) == 2
    audio, logp = out
    assert np.array_equal(audio, plain) and logp.shape == audio.shape and logp.dtype == np.float32 and np.isfinite(logp).all() and (logp < 0).all()
    assert np.array_equal(after[1], state[1]) and after[2:] == state[2:], "a call with log-probabilities consumes the global RNG exactly as one without"
    # across callback cuts: the concatenated pieces are the one-piece result's bits
    calls = []
    np.random.seed(5)
    audio_c, logp_c = m.generate_fast(64, temperature=1., progress_callback=lambda s, t: calls.append(s), progress_interval=16, return_logprobs="model")
    assert len(calls) >= 3 and np.array_equal(audio_c, plain) and logp_c.tobytes() == logp.tobytes()
    np.random.seed(5)
    audio_s, logp_s, st = m.generate_fast(64, temperature=1., return_logprobs="model", return_state=True)
    from mi355_wavenet.state import GenerationState
    assert np.array_equal(audio_s, plain) and logp_s.tobytes() == logp.tobytes() and isinstance(st, GenerationState)
    np.random.seed(5)
    a_true, l_true = m.generate_fast(64, temperature=1., return_logprobs=True)
    np.random.seed(5)
    a_smp, l_smp = m.generate_fast(64, temperature=1., return_logprobs="sampling")
    assert l_true.tobytes() == l_smp.tobytes() and np.array_equal(a_true, plain), 'True means "sampling"'
    assert np.abs(l_smp - logp).max() <= 2 * lc.bound(float(logp.min()), 256, lc.A_ONE_WAVE), "T = 1, no filter, no regulariser: the two modes state the same value"


def test_facade_streams_and_best_of_n():
    m, cfg, W = _model(147)
    np.random.seed(6)
    rows, logp = m.generate_fast_streams(64, [1.0, 0.0], return_logprobs="sampling")
    assert rows.shape == (2, 64) and logp.shape == (2, 64) and logp.dtype == np.float32
    np.random.seed(6)
    assert np.array_equal(m.generate_fast_streams(64, [1.0, 0.0]), rows)
    eng = m._engine(2)
    first = np.full((2, 1), 128)
    g_idx, g_logits = eng.generate(64, first, temperature=0.0, want_logits=True)
    assert np.array_equal(m._expand_indices(g_idx[1]), rows[1])
    for t in range(64):      # row 1 is the greedy statement
        _check(logp[1, t], lc.logp64(g_logits[1, t], None, 0.0, True, 0, 0.0, g_idx[1, t], "sampling"), 256, lc.A_ONE_WAVE, "greedy row, step %d" % t)
    # best of N, as the README shows it: fan a state out into four temperatures and rank by the model's log-likelihood
    temps = [1.0, 0.9, 0.8, 0.7]
    np.random.seed(7)
    _, state = m.generate_fast(32, temperature=1., return_state=True)
    np.random.seed(8)
    audio, logp = m.generate_fast_streams(64, temps, continue_from=state, return_logprobs="model")
    ranking = np.argsort(-logp.sum(axis=1))
    best = audio[ranking[0]]
    assert best.shape == (64,)
    # ... against the same job with the logits dump and a host log-softmax
    np.random.seed(8)
    u = np.stack([np.random.random_sample(64) for _ in temps])
    eng = m._engine(4)
    eng.reset()
    eng.state_load(state.state)
    idx, logits = eng.generate(64, np.full((4, 1), state.last_index), temperature=np.asarray(temps, np.float32), uniforms=u, reset=False, want_logits=True)
    assert np.array_equal(m._expand_indices(idx), audio)
    host = np.array([[lc.logp64(logits[s, t], None, 1.0, False, 0, 0.0, idx[s, t], "model") for t in range(64)] for s in range(4)])
    assert np.array_equal(np.argsort(-host.sum(axis=1)), ranking), (host.sum(axis=1), logp.sum(axis=1))
    assert np.abs(host - logp).max() <= lc.bound(float(host.min()), 256, lc.A_ONE_WAVE)
