"""-m gpu: forced samples in the sampler kernels (include/wn_abi.h wn_set_forced_samples) through whole jobs of the persistent chain, on every kernel that
draws -- the wave-specialised kernel in its one- and two-streams-per-item forms, the slot re-use form's filter kernel, the stacked kernel (WIDE sampler), the
generic kernel at 256 classes and at 300.  N = 64 generated samples after 3 given, the shapes and pins of tests/test_gpu_sampling_filters.py.

1. An armed job whose entries are all free is the job that was not armed, bit for bit.           2. Forcing a stream to what it drew anyway changes nothing.
3. Real forcing: the forced class is written, enters the network (oracle, teacher-forced on the job's output), free positions are still the draw of the
   float64 statement on the job's own logits, and every log-probability -- forced or drawn -- is logprob_cases.logp64 at the class written, inside the
   derived bound; a forced class the filter dropped is exactly -inf.                           4. A forced prefix is a longer prompt: indices, logits, state.
5. Exact rows (end_conv_2.weight = 0).   6. Rounds.   7. Error codes on a live handle.   8. The facade and score_continuation."""
import ctypes
import math

import numpy as np
import pytest
import torch

import forced_cases as fz
import logprob_cases as lc
import sampler_cases as sc
import sampler_filter_cases as fc
from mi355_wavenet import _abi, engine, synth
from parity_common import LOGIT_RTOL, check_engine, make_case, oracle_run
from test_gpu_generation_state import _decided
from test_gpu_parity import MINI3
from test_gpu_sampling_filters import FILTERS, N, N_GIVEN, SHAPES, TEMPS

pytestmark = pytest.mark.gpu

UNDECIDED_CAP = 0.02
TINY300 = dict(synth.CONFIGS["tiny"], classes=300)
F_SHAPES = SHAPES + [("tiny300_generic", TINY300, 2, {"WN_KERNEL": "generic"}, 1)]
IDS = [s[0] for s in F_SHAPES]
KW = dict(batched_prime=False, timeout_ms=8000)


class Worst:
    """the largest err / bound seen, per label"""
    def __init__(self):
        self.seen = {}

    def add(self, label, ratio):
        self.seen[label] = max(self.seen.get(label, 0.0), ratio)


def _check(got, want, C, A, what):
    """one log-probability against the float64 statement -> err / bound"""
    if want == -math.inf:
        assert got == -math.inf, "%s: %r, the class is outside the kept set" % (what, got)
        return 0.0
    b = lc.bound(want, C, A)
    err = abs(float(got) - want)
    assert err <= b, "%s: logp %r, logp64 %r, error %.3g > bound %.3g" % (what, float(got), want, err, b)
    return err / b


def _engine_for(label, cfgname, ns, env, variant, monkeypatch, seed):
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    cfg, W, first, u = make_case(cfgname, seed, ns, N_GIVEN, N)
    eng = engine.Engine(cfg, W, n_streams=ns)
    assert eng.info()["kernel_variant"] == variant, eng.info()
    if "WN_V3_SLOTS" in env:
        assert eng.info()["skip_lane_slots"] == int(env["WN_V3_SLOTS"]), eng.info()
    return eng, cfg, W, first, u


def _greedy_temps(ns):
    """every second stream (the only one of a single-stream job) greedy by its temperature"""
    return np.array([0.0 if (s % 2 == 1 or ns == 1) else 1.0 for s in range(ns)], dtype=np.float32)


# ---------------------------------------------------------------- 1. all free
@pytest.mark.parametrize("label,cfgname,ns,env,variant", F_SHAPES, ids=IDS)
def test_an_armed_job_with_every_entry_free_is_the_plain_job(label, cfgname, ns, env, variant, monkeypatch):
    eng, cfg, W, first, u = _engine_for(label, cfgname, ns, env, variant, monkeypatch, 151)
    kw = dict(KW, uniforms=u)
    free = np.full((ns, N), fz.FREE, np.int32)
    before = {T: eng.generate(N, first, temperature=T, **kw) for T in TEMPS}
    for T in TEMPS:
        assert np.array_equal(eng.generate(N, first, temperature=T, forced=free, **kw), before[T]), "%s T=%g: armed, all free" % (label, T)
        assert np.array_equal(eng.generate(N, first, temperature=T, forced=free[0], **kw), before[T]), "%s T=%g: a 1-D array is every stream's" % (label, T)
        for mode in lc.MODES:
            idx0, logp0 = eng.generate(N, first, temperature=T, logprobs=mode, **kw)
            idx1, logp1 = eng.generate(N, first, temperature=T, logprobs=mode, forced=free, **kw)
            assert np.array_equal(idx0, before[T]) and np.array_equal(idx1, before[T]), "%s T=%g %s" % (label, T, mode)
            assert logp1.tobytes() == logp0.tobytes(), "%s T=%g %s: the log-probabilities of the job armed for them alone" % (label, T, mode)
    g0 = eng.generate(N, first, temperature=0.0, **KW)
    assert np.array_equal(eng.generate(N, first, temperature=0.0, forced=free, **KW), g0), label + ": a greedy job, armed, all free"
    for T in TEMPS:
        assert np.array_equal(eng.generate(N, first, temperature=T, **kw), before[T]), "%s: a plain job after the armed ones, T = %g" % (label, T)
    check_engine(eng, cfg, W, N, first, 1.0, 0.0, u, label + " after the forced samples")
    eng.close()


# ---------------------------------------------------------------- 2. self-forcing
@pytest.mark.parametrize("label,cfgname,ns,env,variant", F_SHAPES, ids=IDS)
def test_forcing_what_the_stream_drew_changes_nothing(label, cfgname, ns, env, variant, monkeypatch):
    eng, cfg, W, first, u = _engine_for(label, cfgname, ns, env, variant, monkeypatch, 152)
    kw = dict(KW, uniforms=u, want_logits=True)
    for k, (T, mode) in enumerate(((1.0, "sampling"), (0.05, "model"), (_greedy_temps(ns), "sampling"))):
        idx, logits, logp = eng.generate(N, first, temperature=T, logprobs=mode, **kw)
        for name, mask in (("shared", fz.shared(ns, N)), ("per stream", fz.per_stream(ns, N)), ("all", np.ones((ns, N), bool))):
            f_idx, f_logits, f_logp = eng.generate(N, first, temperature=T, logprobs=mode, forced=fz.forced_array(mask, idx), **kw)
            tag = "%s case %d, mask %s" % (label, k, name)
            assert np.array_equal(f_idx, idx), tag
            assert f_logits.tobytes() == logits.tobytes(), tag + ": the logits dump"
            assert f_logp.tobytes() == logp.tobytes(), tag + ": the log-probabilities"
    eng.close()


# ---------------------------------------------------------------- 3. real forcing, replayed on the job's own logits
def _replay_forced(idx, logits, logp, u, temps, top_k, top_p, mode, mask, forced, A, label, worst):
    """-> (undecided free draws, membership-undecided log-probabilities)"""
    C = logits.shape[2]
    assert logp.shape == idx.shape and logp.dtype == np.float32
    assert np.array_equal(idx[mask], forced[mask]), label + ": out_idx holds the forced classes on the mask"
    und_draw = und_logp = 0
    for s in range(idx.shape[0]):
        greedy = not temps[s] > 0
        for t in range(idx.shape[1]):
            x, keep, member = lc.kept64(logits[s, t], None, temps[s], greedy, top_k, top_p)
            got = int(idx[s, t])
            what = "%s stream %d step %d" % (label, s, t)
            if not mask[s, t]:       # a free position: the draw of the float64 statement, where the existing tests decide it
                if greedy:
                    assert got == int(np.argmax(x)), what + ": the argmax"
                else:
                    cdf = fc.cdf64_filtered(x, keep)
                    if member and sc.margin(cdf, u[s, t]) > fc.BAND:
                        assert got == sc.pick(cdf, u[s, t]), "%s: class %d, the float64 draw %d (u = %r)" % (what, got, sc.pick(cdf, u[s, t]), u[s, t])
                    else:
                        und_draw += 1
                        assert fc.allowed_filtered(x, top_k, top_p, u[s, t], got), what + ": class %d is not allowed on this undecided draw" % got
            if mode == "sampling" and not member:
                und_logp += 1
                continue
            want = lc.logp64(logits[s, t], None, temps[s], greedy, top_k, top_p, got, mode)
            if mask[s, t] and mode == "sampling" and not keep[got]:
                assert want == -math.inf
            worst.add("%s %s %s" % (label.split(" ")[0], mode, "forced" if mask[s, t] else "free"), _check(logp[s, t], want, C, A, what))
    assert und_draw <= UNDECIDED_CAP * idx.size, "%s: %d of %d draws undecided" % (label, und_draw, idx.size)
    assert und_logp <= UNDECIDED_CAP * idx.size, "%s: %d of %d log-probabilities membership-undecided" % (label, und_logp, idx.size)
    return und_draw, und_logp


@pytest.mark.parametrize("label,cfgname,ns,env,variant", F_SHAPES, ids=IDS)
def test_real_forcing(label, cfgname, ns, env, variant, monkeypatch):
    eng, cfg, W, first, u = _engine_for(label, cfgname, ns, env, variant, monkeypatch, 153)
    C = cfg.get("classes", 256)
    A = lc.a_of(variant, C)
    kw = dict(KW, uniforms=u, want_logits=True)
    mask = fz.per_stream(ns, N)
    worst = Worst()
    undecided, dropped, oracle_seen = [], 0, {}
    for top_k, top_p in ((0, 0.0),) + FILTERS:
        for T in TEMPS + ("mixed",):
            if T == "mixed" and (top_k, top_p) not in ((0, 0.0), (8, 0.0)):
                continue
            temps = _greedy_temps(ns) if T == "mixed" else np.full(ns, T, np.float32)
            temperature = temps if T == "mixed" else T
            plain, plain_logits = eng.generate(N, first, temperature=temperature, top_k=top_k, top_p=top_p, **kw)     # (the handle keeps the filter for the jobs below)
            forced = fz.forced_array(mask, fz.shifted_classes(plain, C))
            for mode in lc.MODES:
                tag = "%s (%d, %g) T=%s %s" % (label, top_k, top_p, T, mode)
                idx, logits, logp = eng.generate(N, first, temperature=temperature, logprobs=mode, forced=forced, **kw)
                undecided.append(_replay_forced(idx, logits, logp, u, temps, top_k, top_p, mode, mask, forced, A, tag, worst))
                dropped += int(np.isneginf(logp[mask]).sum())
                for s in range(ns):
                    p = fz.first_forced(mask[s])
                    if p is None:
                        assert np.array_equal(idx[s], plain[s]) and logits[s].tobytes() == plain_logits[s].tobytes(), tag + ": an all-free stream next to forced ones"
                        continue
                    assert np.array_equal(idx[s, :p], plain[s, :p]) and idx[s, p] != plain[s, p], tag
                    if p + 1 < N:      # non-vacuity: the forced class entered the network
                        assert logits[s, p + 1].tobytes() != plain_logits[s, p + 1].tobytes(), "%s stream %d: the logits behind the first forced position" % (tag, s)
                    key = (s, idx[s].tobytes())
                    if key not in oracle_seen:      # (the teacher-forced logits depend on the sequence alone)
                        oracle_seen[key] = oracle_run(cfg, W, N, first[s], 1.0, 0.0, u[s], forced=idx[s])[1]
                    o_log = oracle_seen[key]
                    tol = LOGIT_RTOL * max(1.0, float(np.abs(o_log).max()))
                    dev = float(np.abs(logits[s] - o_log).max())
                    assert dev <= tol, "%s stream %d: logits deviate %.3g > %.3g from the oracle forced to the job's output" % (tag, s, dev, tol)
    assert dropped > 0, "no forced class fell outside a filter's kept set: the -inf branch was not seen"
    eng.set_sampling(0, 0.0)
    eng.close()
    print(label, "worst err / bound:", {k: round(v, 3) for k, v in sorted(worst.seen.items())}, "undecided (draws, log-probabilities) per job:", undecided)


# ---------------------------------------------------------------- 4. a forced prefix is a longer prompt
@pytest.mark.parametrize("label,cfgname,ns,env,variant", F_SHAPES, ids=IDS)
def test_a_forced_prefix_is_a_longer_prompt(label, cfgname, ns, env, variant, monkeypatch):
    eng, cfg, W, first, u = _engine_for(label, cfgname, ns, env, variant, monkeypatch, 154)
    C = cfg.get("classes", 256)
    m = fz.ragged_prefix_lengths(ns)
    if ns == 1:
        m = [5]
    prefix = np.random.RandomState(154).randint(0, C, (ns, max(m)))
    forced = np.full((ns, N), fz.FREE, np.int32)
    for s in range(ns):
        forced[s, :m[s]] = prefix[s, :m[s]]
    idx_a, logits_a = eng.generate(N, first, temperature=1.0, uniforms=u, want_logits=True, forced=forced, **KW)
    state_a = [eng.state_save(s) for s in range(ns)]
    for s in range(ns):       # job B: every stream runs stream s's longer prompt; row s is compared (the same stream slot as in job A)
        prompt = np.concatenate([first[s], prefix[s, :m[s]]])
        n_b = N - m[s]
        idx_b, logits_b = eng.generate(n_b, prompt, temperature=1.0, uniforms=np.tile(u[s, m[s]:], (ns, 1)), want_logits=True, **KW)
        assert np.array_equal(idx_a[s, :m[s]], prefix[s, :m[s]])
        assert np.array_equal(idx_a[s, m[s]:], idx_b[s]), "%s stream %d (prefix %d): the samples behind the prefix" % (label, s, m[s])
        assert logits_a[s, m[s]:].tobytes() == logits_b[s].tobytes(), "%s stream %d (prefix %d): the logits behind the prefix" % (label, s, m[s])
        assert eng.state_save(s).tobytes() == state_a[s].tobytes(), "%s stream %d (prefix %d): the state behind the job" % (label, s, m[s])
    eng.close()


def test_a_forced_prefix_against_the_batched_priming_pass():
    """job B's prompt is long enough for the batched pass (another arithmetic: matrix-core GEMMs): the uniforms are chosen on the CPU so that every draw
    of the oracle lies 1e-5 from a CDF boundary, and the comparison is plain equality (the rule of tests/test_gpu_generation_state.py)"""
    ns, m, n_free = 2, engine.Engine.PRIME_BATCH_MIN + 2, 20
    cfg, W, first, _ = make_case("cfg1", 155, ns, N_GIVEN, 1)
    prefix = np.random.RandomState(155).randint(0, 256, (ns, m))
    prompts = np.concatenate([first, prefix], axis=1)
    u_b, o_idx = zip(*[_decided(cfg, W, n_free, prompts[s], lambda rs: rs.random_sample(n_free), "stream %d" % s) for s in range(ns)])
    u_b = np.stack(u_b)
    eng = engine.Engine(cfg, W, n_streams=ns)
    eng.reset()
    assert eng.prime_host(prompts[:, :-1]), "the batched priming pass serves this shape"
    idx_b = eng.generate(n_free, prompts, temperature=1.0, uniforms=u_b, batched_prime=True, timeout_ms=8000)
    forced = np.concatenate([prefix, np.full((ns, n_free), fz.FREE)], axis=1).astype(np.int32)
    u_a = np.concatenate([np.zeros((ns, m)), u_b], axis=1)
    idx_a = eng.generate(m + n_free, first, temperature=1.0, uniforms=u_a, forced=forced, **KW)
    eng.close()
    for s in range(ns):
        assert np.array_equal(idx_b[s], o_idx[s]) and np.array_equal(idx_a[s, m:], idx_b[s]) and np.array_equal(idx_a[s, :m], prefix[s]), "stream %d" % s


# ---------------------------------------------------------------- 5. exact rows through the product path
PEAK = np.float32(20.0)
TIES = (2, 3, 63, 64, 255)


def _flat():
    return np.zeros(256, np.float32)


def _ramp():
    return (np.float32(0) - np.float32(0.05) * np.arange(256, dtype=np.float32)).astype(np.float32)


def _tied():
    x = np.full(256, np.float32(-0.7), np.float32)
    x[list(TIES)] = np.float32(0)
    return x


def _peak():
    x = np.zeros(256, np.float32)
    x[0] = PEAK
    return x


def _mid(bias, T, top_k, top_p, classes):
    """the midpoints of the float64 CDF intervals of `classes`: the uniforms that land on them"""
    x = sc.x32(bias, None, T, False)
    cdf = fc.cdf64_filtered(x, fc.filter64(x, top_k, top_p)[0])
    return [0.5 * ((cdf[i - 1] if i else 0.0) + cdf[i]) for i in classes]


F = fz.FREE


# (name, end_conv_2.bias, temperature (0: a greedy job), (top_k, top_p), uniforms or None, forced row, the classes written)
def _exact_rows():
    rows = []
    # top_k = 8 keeps classes 0-7 of the ramp: 100 and 8 are outside, 7 is the last one inside; the free positions land where their uniforms say
    lands = [100, 3, 8, 7, 0, 5, 255, 1]
    forced = [100, F, 8, 7, F, F, 255, F]
    us = [0.5 if f != F else _mid(_ramp(), 1.0, 8, 0.0, [c])[0] for f, c in zip(forced, lands)]
    rows.append(("ramp top_k 8", _ramp(), 1.0, (8, 0.0), us, forced, lands))
    # five classes tied at the threshold of top_k = 3 all stay: a forced tied class is kept and finite
    lands = [64, 2, 255, 63, 3, 200, 64, 2]
    forced = [64, F, 255, 63, F, 200, F, 2]
    us = [0.5 if f != F else (TIES.index(c) + 0.5) / len(TIES) for f, c in zip(forced, lands)]
    rows.append(("ties top_k 3", _tied(), 1.0, (3, 0.0), us, forced, lands))
    # T = 0.05 without a filter: x = -i, the fp32 mass of class 255 (and of 120) is 0.0 -- kept all the same, and finite
    lands = [255, 0, 120, 1, 104, 0, 103, 2]
    forced = [255, F, 120, F, 104, F, 103, F]
    us = [0.5 if f != F else _mid(_ramp(), 0.05, 0, 0.0, [c])[0] for f, c in zip(forced, lands)]
    rows.append(("ramp T 0.05", _ramp(), 0.05, (0, 0.0), us, forced, lands))
    # a greedy job forced off its argmax (class 2: the first of the tied maxima), to an untied class, the last class and class 0
    rows.append(("ties greedy", _tied(), 0.0, (0, 0.0), None, [200, F, 255, 0, F, 64, F, 3], [200, 2, 255, 0, 2, 64, 2, 3]))
    # the flat row: class 255 and class 0 forced; u EXACTLY on a boundary of the CDF (j / 256, exact in every precision: searchsorted side='right' gives
    # class j) at the free position behind a forced one
    lands = [255, 64, 0, 1, 128, 255, 0, 200]
    forced = [255, F, 0, F, F, F, 0, F]
    us = [0.3, 64 / 256, 0.9, 1 / 256, 128.5 / 256, 255 / 256, 0.1, 200.5 / 256]
    rows.append(("flat", _flat(), 1.0, (0, 0.0), us, forced, lands))
    # one class at +20 holds all but 5.3e-7 of the mass: forced into the tail, and onto the peak
    rows.append(("peak", _peak(), 1.0, (0, 0.0), [0.3] * 8, [17, F, 255, 0, F, 1, F, 128], [17, 0, 255, 0, 0, 1, 0, 128]))
    for name, bias, T, (top_k, top_p), us, forced, lands in rows:
        assert len(forced) == len(lands) == 8 and all(f == F or f == c for f, c in zip(forced, lands)), name
        if us is not None and name != "flat":      # every free uniform at least BAND from a boundary of the float64 CDF
            x = sc.x32(bias, None, T, False)
            cdf = fc.cdf64_filtered(x, fc.filter64(x, top_k, top_p)[0])
            for uu, f, c in zip(us, forced, lands):
                assert f != F or (sc.margin(cdf, uu) >= sc.BAND and sc.pick(cdf, uu) == c), (name, uu, c)
    return rows


EXACT_SHAPES = [s for s in SHAPES if s[0] in ("lean4_ns4", "lean4_ns8_mode3_slots4", "cfg1_ns1_v4", "tiny_generic")]


@pytest.mark.parametrize("label,cfgname,ns,env,variant", EXACT_SHAPES, ids=[s[0] for s in EXACT_SHAPES])
def test_exact_rows(label, cfgname, ns, env, variant, monkeypatch):
    eng, cfg, W, first, _ = _engine_for(label, cfgname, ns, env, variant, monkeypatch, 156)
    A = lc.a_of(variant, 256)
    worst = Worst()
    W = dict(W)
    W["end_conv_2.weight"] = np.zeros_like(W["end_conv_2.weight"])
    n = 8
    for name, bias, T, (top_k, top_p), us, forced_row, lands in _exact_rows():
        W["end_conv_2.bias"] = bias
        eng.load_weights(W)
        u = np.tile(np.asarray(us, np.float64), (ns, 1)) if us is not None else None
        forced = np.tile(np.asarray(forced_row, np.int32), (ns, 1))
        mask = forced != F
        values = {}
        for mode in lc.MODES:
            tag = "%s %s %s" % (label, name, mode)
            idx, logits, logp = eng.generate(n, first, temperature=T, uniforms=u, want_logits=True, logprobs=mode, forced=forced, top_k=top_k, top_p=top_p, **KW)
            assert logits.tobytes() == np.broadcast_to(bias, logits.shape).tobytes(), tag + ": every step's logits are end_conv_2.bias"
            assert np.array_equal(idx, np.tile(lands, (ns, 1))), "%s: classes %r, expected %r" % (tag, idx.tolist(), lands)
            for s in range(ns):
                for t in range(n):
                    want = lc.logp64(bias, None, T, not T > 0, top_k, top_p, idx[s, t], mode)
                    kind = "forced" if mask[s, t] else "free"
                    worst.add("%s %s" % (mode, kind), _check(logp[s, t], want, 256, A, "%s stream %d step %d (%s)" % (tag, s, t, kind)))
            values[mode] = logp
        smp, mdl = values["sampling"], values["model"]
        near = lambda got, v: np.abs(got - v).max() <= lc.bound(v, 256, A)  # noqa: E731
        if name == "ramp top_k 8":      # forced outside top_k = 8: -inf under "sampling", finite under "model"; the last class inside is finite
            assert np.isneginf(smp[:, [0, 2, 6]]).all() and np.isfinite(smp[:, [1, 3, 4, 5, 7]]).all() and np.isfinite(mdl).all()
            lse = math.log(np.exp(_ramp().astype(np.float64)).sum())
            assert near(mdl[:, 0], float(_ramp()[100]) - lse) and near(mdl[:, 6], float(_ramp()[255]) - lse)
        if name == "ties top_k 3":      # the tied classes are all kept: -log 5 each; 200 is below the threshold
            assert near(smp[:, [0, 1, 2, 3, 4, 6, 7]], -math.log(len(TIES))) and np.isneginf(smp[:, 5]).all() and np.isfinite(mdl).all()
        if name == "ramp T 0.05":       # x = -i: the fp32 mass underflows below about -104; the value is (x_i - gm) - log(tot) all the same
            x = sc.x32(_ramp(), None, 0.05, False).astype(np.float64)
            assert float(np.exp(np.float32(x[120]))) == 0.0 and float(np.exp(np.float32(x[255]))) == 0.0
            lse = math.log(np.exp(x - x.max()).sum())
            for t, c in ((0, 255), (2, 120), (4, 104), (6, 103)):
                assert np.isfinite(smp[:, t]).all() and near(smp[:, t], (x[c] - x.max()) - lse), "%s: class %d" % (label, c)
        if name == "ties greedy":       # forced off the argmax: the log-softmax of the whole row at the forced class, the same in both modes
            lse = math.log(len(TIES) + (256 - len(TIES)) * math.exp(float(np.float32(-0.7))))
            assert near(smp[:, [1, 2, 4, 5, 6, 7]], -lse) and near(smp[:, [0, 3]], float(np.float32(-0.7)) - lse)
            assert np.abs(mdl - smp).max() <= 2 * lc.bound(float(mdl.min()), 256, A)
        if name == "flat":
            assert near(smp, -math.log(256)) and near(mdl, -math.log(256))
        if name == "peak":
            tail = np.array([c != 0 for c in lands])
            assert np.abs(mdl[:, tail] + 20.0).max() < 1e-4 and np.abs(mdl[:, ~tail]).max() < 1e-5 and np.abs(smp - mdl).max() <= 2 * lc.bound(-20.0, 256, A)
    eng.set_sampling(0, 0.0)
    eng.close()
    print(label, "exact rows, worst err / bound:", {k: round(v, 3) for k, v in sorted(worst.seen.items())})


# ---------------------------------------------------------------- armed by hand: a caller's own buffer
def _dev(eng, a):
    return torch.from_numpy(np.ascontiguousarray(a, dtype=np.int32)).to(eng.mem.device)


def _armed(eng, buf, capacity, num_samples, first, **kw):
    eng.set_forced_samples(buf, capacity)
    return eng.generate(num_samples, first, **kw)


# ---------------------------------------------------------------- 6. rounds
def test_rounds_read_every_members_slice():
    ns, n = 170, 8
    cfg, W, first, u = make_case(MINI3, 157, ns, N_GIVEN, n)
    eng = engine.Engine(cfg, W, n_streams=ns)
    assert eng.info()["n_chains"] == 2 and eng.info()["kernel_variant"] == 3
    kw = dict(KW, temperature=1.0, uniforms=u)
    plain = eng.generate(n, first, **kw)
    forced = np.full((ns, n), fz.FREE, np.int32)
    rows = (0, 85, 86, 169)           # the first round's first and last stream, the second round's
    for k, s in enumerate(rows):
        forced[s] = (plain[s] + 31 * (k + 1) + np.arange(n)) % 256
    assert len({forced[s].tobytes() for s in rows}) == 4 and all((forced[s] != plain[s]).any() for s in rows)
    buf = _dev(eng, forced)
    assert buf.numel() == ns * n      # exactly the capacity: the last member's slice ends at the buffer's end
    idx = _armed(eng, buf, ns * n, n, first, **kw)
    for s in range(ns):
        assert np.array_equal(idx[s], forced[s] if s in rows else plain[s]), "stream %d" % s
    assert np.array_equal(eng.generate(n, first, **kw), plain)
    with pytest.raises(_abi.WnError):     # one short: refused before any member ran
        _armed(eng, buf, ns * n - 1, n, first, **kw)
    assert np.array_equal(eng.generate(n, first, **kw), plain)
    eng.close()


# ---------------------------------------------------------------- 7. error codes on a live handle
def test_error_codes_on_a_live_handle():
    ns, n = 2, 8
    cfg, W, first, u = make_case("tiny", 158, ns, N_GIVEN, n)
    eng = engine.Engine(cfg, W, n_streams=ns)
    kw = dict(KW, temperature=1.0, uniforms=u)
    plain = eng.generate(n, first, **kw)
    fives = _dev(eng, np.full((ns, n), 5))
    out = torch.full((ns, n), -7, dtype=torch.int32, device=eng.mem.device)
    first_dev, u_dev = eng.mem.upload(np.ascontiguousarray(first, dtype=np.int32)), eng.mem.upload(np.ascontiguousarray(u, dtype=np.float64))
    a = _abi.wn_generate_args(eng.mem.ptr(first_dev), N_GIVEN, n, 1.0, 0, None, eng.mem.ptr(u_dev), out.data_ptr(), None, eng.mem.stream(), 8000, 0, None)
    eng.reset()
    eng.set_forced_samples(fives, ns * n - 1)         # one int short: refused, nothing launched -- the caller's output keeps its sentinel
    assert eng.lib.dll.wn_generate(eng._h, ctypes.byref(a)) == _abi.WN_E_BADARG and "forced" in eng.lib.last_error()
    eng.wait()
    assert bool((out == -7).all().item()), "the refused job wrote nothing"
    assert np.array_equal(eng.generate(n, first, **kw), plain), "the refused job consumed its arming: the next job is plain"
    # armed with BOTH, the log-probability output one float short: refused for that, and the forced arming is consumed with it -- the next job is plain
    lp = torch.full((ns, n), -7.0, dtype=torch.float32, device=eng.mem.device)
    eng.set_logprob_output(lp, ns * n - 1, "model")
    eng.set_forced_samples(fives, ns * n)
    assert eng.lib.dll.wn_generate(eng._h, ctypes.byref(a)) == _abi.WN_E_BADARG and "log-probability" in eng.lib.last_error()
    eng.wait()
    assert bool((out == -7).all().item()) and bool((lp == -7.0).all().item()), "the refused job wrote nothing"
    assert np.array_equal(eng.generate(n, first, **kw), plain), "refused for its log-probability output, the job consumed its forced samples too"
    eng.set_logprob_output(lp, ns * n, "model")       # ... and the other way round
    eng.set_forced_samples(fives, ns * n - 1)
    assert eng.lib.dll.wn_generate(eng._h, ctypes.byref(a)) == _abi.WN_E_BADARG and "forced" in eng.lib.last_error()
    eng.wait()
    assert np.array_equal(eng.generate(n, first, **kw), plain) and bool((lp == -7.0).all().item()), "refused for its forced samples, the job consumed its log-probability output too"
    eng.set_forced_samples(fives, ns * n)             # arm, disarm, run
    eng.set_forced_samples(None, 0)
    assert np.array_equal(eng.generate(n, first, **kw), plain)
    d, h = eng.lib.dll, eng._h
    assert d.wn_set_forced_samples(h, ctypes.c_void_p(fives.data_ptr()), -1) == _abi.WN_E_BADARG and "wn_set_forced_samples" in eng.lib.last_error()
    assert np.array_equal(eng.generate(n, first, **kw), plain), "a refused call armed nothing"
    # every value outside [0, classes) is a free position
    junk = np.array([-1, 256, 1 << 30, -(1 << 31), -2, 257, 0x7fffffff, -256], dtype=np.int64)
    assert np.array_equal(_armed(eng, _dev(eng, np.tile(junk, (ns, 1)).astype(np.int32)), ns * n, n, first, **kw), plain)
    mixed = np.tile(junk, (ns, 1)).astype(np.int32)
    mixed[:, 3] = 255
    mixed[1, 6] = 0
    got = _armed(eng, _dev(eng, mixed), ns * n, n, first, **kw)
    assert (got[:, 3] == 255).all() and got[1, 6] == 0 and np.array_equal(got[:, :3], plain[:, :3])
    # exactly enough: forced, once -- and the job after an armed one reads nothing
    assert (_armed(eng, fives, ns * n, n, first, **kw) == 5).all()
    assert np.array_equal(eng.generate(n, first, **kw), plain), "the job after an armed one is plain"
    # the host checks of Engine.generate answer before anything is armed
    for bad in (np.full((ns, n), -2), np.full((ns, n), 256), np.full((ns, n + 1), -1)):
        with pytest.raises(ValueError, match="forced"):
            eng.generate(n, first, forced=bad, **kw)
    assert np.array_equal(eng.generate(n, first, **kw), plain)
    eng.close()


# ---------------------------------------------------------------- 8. the facade
def _model(seed, output_length=8):
    import wavenet_model
    cfg = synth.CONFIGS["cfg1"]
    W = synth.init_weights(cfg, seed=seed)
    m = wavenet_model.WaveNetModel(output_length=output_length, **cfg)
    m.load_state_dict({k: torch.from_numpy(v) for k, v in W.items()})
    return m, cfg, W


def _same_rng(a, b):
    return np.array_equal(a[1], b[1]) and a[2:] == b[2:]


def test_facade_forced_and_rng_consumption():
    m, cfg, W = _model(159)
    mask = fz.positions(64)
    np.random.seed(5)
    plain = m.generate_fast(64, temperature=1.)
    state = np.random.get_state()
    classes = np.random.RandomState(9).randint(0, 256, 64)
    forced = fz.forced_array(mask, classes)
    np.random.seed(5)
    audio = m.generate_fast(64, temperature=1., forced=forced)
    assert _same_rng(np.random.get_state(), state), "a call with `forced` consumes the global RNG exactly as one without"
    assert audio.shape == (64,) and np.array_equal(audio[mask], m._expand_indices(classes[mask])) and not np.array_equal(audio, plain)
    calls = []
    np.random.seed(5)
    audio_c, logp_c = m.generate_fast(64, temperature=1., progress_callback=lambda s, t: calls.append(s), progress_interval=16, forced=forced,
                                      return_logprobs="model")
    np.random.seed(5)
    audio_1, logp_1 = m.generate_fast(64, temperature=1., forced=forced, return_logprobs="model")
    assert len(calls) >= 3 and np.array_equal(audio_c, audio) and np.array_equal(audio_1, audio) and logp_c.tobytes() == logp_1.tobytes()
    assert np.isfinite(logp_1).all()
    # return_state, then continue_from, is the one-shot call; with a filter, which is off again afterwards
    np.random.seed(5)
    one = m.generate_fast(64, temperature=1., forced=forced, top_k=8, return_logprobs="sampling")
    np.random.seed(5)
    a, la, st = m.generate_fast(32, temperature=1., forced=forced[:32], top_k=8, return_logprobs="sampling", return_state=True)
    b, lb = m.generate_fast(32, temperature=1., forced=forced[32:], top_k=8, return_logprobs="sampling", continue_from=st)
    assert np.array_equal(np.concatenate([a, b]), one[0]) and np.concatenate([la, lb]).tobytes() == one[1].tobytes()
    assert np.isneginf(one[1][mask]).any() and np.isfinite(one[1][~mask]).all(), "top_k = 8 drops some of 20 random forced classes, and no drawn one"
    np.random.seed(5)
    assert np.array_equal(m.generate_fast(64, temperature=1.), plain)
    # streams: a shared 1-D array, and one row per temperature
    temps = [1.0, 0.0, 0.7]
    np.random.seed(6)
    rows_plain = m.generate_fast_streams(64, temps)
    state = np.random.get_state()
    np.random.seed(6)
    rows = m.generate_fast_streams(64, temps, forced=forced)
    assert _same_rng(np.random.get_state(), state)
    assert rows.shape == (3, 64) and all(np.array_equal(r[mask], m._expand_indices(classes[mask])) for r in rows)
    per_row = np.stack([forced, np.full(64, fz.FREE), fz.forced_array(~mask, classes)]).astype(np.int32)
    np.random.seed(6)
    rows2, logp2 = m.generate_fast_streams(64, temps, forced=per_row, return_logprobs="model")
    assert np.array_equal(rows2[0], rows[0]) and np.array_equal(rows2[1], rows_plain[1]) and np.array_equal(rows2[2][~mask], m._expand_indices(classes[~mask]))
    assert logp2.shape == (3, 64) and np.isfinite(logp2).all()


def test_score_continuation():
    out = 64
    m, cfg, W = _model(160, output_length=out)
    rf = m.receptive_field
    window = torch.from_numpy(np.random.RandomState(160).randint(0, 256, (2, rf + out))).to(torch.int32)
    ref = m.score_indices(window, want_rows=True)
    row_nll = ref.row_nll.cpu().numpy()
    prompt, clip = window[:, :rf].long(), window[:, rf:].numpy()
    np.random.seed(3)
    before = np.random.get_state()
    logp = m.score_continuation(clip, first_samples=prompt)
    assert _same_rng(np.random.get_state(), before), "score_continuation draws nothing"
    assert logp.shape == (2, out) and logp.dtype == np.float32
    _, logits = m._engine(2).generate(out, prompt.numpy(), temperature=0.0, want_logits=True, forced=clip, **KW)
    tol = 2 * LOGIT_RTOL * max(1.0, float(np.abs(logits).max()))
    worst = 0.0
    for s in range(2):
        for t in range(out):
            want = -float(row_nll[s, t])
            err, b = abs(float(logp[s, t]) - want), tol + lc.bound(want, 256, lc.A_ONE_WAVE)
            worst = max(worst, err / b)
            assert err <= b, "stream %d step %d: %r, -row_nll %r, error %.3g > %.3g" % (s, t, float(logp[s, t]), want, err, b)
    # one row, and chunked: four calls of 16 through return_state are the single call's bytes
    one = m.score_continuation(clip[0], first_samples=prompt[0])
    assert one.shape == (out,) and np.abs(one - logp[0]).max() <= tol + 2 * lc.bound(float(logp[0].min()), 256, lc.A_ONE_WAVE)   # (another kernel form)
    whole, st_whole = m.score_continuation(clip[0], first_samples=prompt[0], return_state=True)
    assert whole.tobytes() == one.tobytes()
    parts, st = [], None
    for k in range(4):
        kw = dict(first_samples=prompt[0]) if st is None else dict(continue_from=st)
        lp, st = m.score_continuation(clip[0, 16 * k:16 * k + 16], return_state=True, **kw)
        parts.append(lp)
    assert np.concatenate(parts).tobytes() == whole.tobytes() and st.state.tobytes() == st_whole.state.tobytes() and st.last_index == int(clip[0, -1])
    # two rows from a list of states
    _, sts = m.score_continuation(clip[:, :16], first_samples=prompt, return_state=True)
    two = m.score_continuation(clip[:, 16:32], continue_from=sts)
    assert two.tobytes() == logp[:, 16:32].tobytes()
    assert _same_rng(np.random.get_state(), before)
    print("score_continuation against -score_indices row losses, worst err / (logit tolerance + bound): %.3f" % worst)
