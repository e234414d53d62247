"""-m gpu: the sampling filters (top-k, nucleus: include/wn_abi.h wn_set_sampling) through whole jobs of the persistent chain, on every kernel that
draws -- the wave-specialised kernel in its one- and two-streams-per-item forms, the stacked kernel, the generic kernel.

Every filtered job is run with the logits dump, and every one of its draws is replayed on the host from the dumped float32 logits through the
float64 statement of the contract (sampler_filter_cases.draw64_filtered): equality on every decided draw (sampler_filter_cases has the rule); on an
undecided one the class must be allowed by a membership inside the band; at most 2 % of a job's draws may be undecided -- a condition on seeds and
shapes, which the replay alone has to meet.  The same job without the dump returns the same indices; a stream made greedy by its temperature ignores
the filter; top_k = 1 is the greedy job (random weights: no exact logit ties); after set_sampling(0, 0) the handle does what it did before any filter
was set, bit for bit, and still agrees with the oracle.  64 generated samples after 3 given, as tests/test_gpu_lean_kernels.py (whose shapes and
pins these are); temperatures 1.0 (random weights: nearly flat rows) and 0.05 (sharp rows)."""
import ctypes

import numpy as np
import pytest
import torch

import sampler_cases as sc
import sampler_filter_cases as fc
from mi355_wavenet import _abi, engine, synth
from parity_common import check_engine, make_case

pytestmark = pytest.mark.gpu

LEAN4 = dict(synth.CONFIGS["cfg3"], layers=4, blocks=1)
N, N_GIVEN = 64, 3
FILTERS = ((8, 0.0), (0, 0.8), (32, 0.9))
TEMPS = (1.0, 0.05)
UNDECIDED_CAP = 0.02
# (label, config, streams, pins, kernel variant).  The slot re-use form has its filter in a kernel of its own (wn_generate_kernel_v3m_filter): 8 streams
# with two per item plan it (pinned in the third shape), 4 streams with two per item do not.
SHAPES = [
    ("lean4_ns4", LEAN4, 4, {"WN_KERNEL": "v3"}, 3),
    ("lean4_ns8_mode3", LEAN4, 8, {"WN_KERNEL": "v3", "WN_V3_MODE": "3"}, 3),
    ("lean4_ns8_mode3_slots4", LEAN4, 8, {"WN_KERNEL": "v3", "WN_V3_MODE": "3", "WN_V3_SLOTS": "4"}, 3),
    ("lean4_ns4_mode3", LEAN4, 4, {"WN_KERNEL": "v3", "WN_V3_MODE": "3"}, 3),
    ("cfg1_ns2_v3", "cfg1", 2, {"WN_KERNEL": "v3"}, 3),
    ("cfg1_ns1_v4", "cfg1", 1, {"WN_KERNEL": "v4"}, 4),
    ("tiny_generic", "tiny", 2, {"WN_KERNEL": "generic"}, 1),
]


def _replay(idx, logits, u, T, top_k, top_p, label):
    """every draw of the job against draw64_filtered on the job's own logits -> number of undecided draws"""
    undecided = 0
    for s in range(idx.shape[0]):
        for t in range(idx.shape[1]):
            x = sc.x32(logits[s, t], None, T, False)
            keep, member = fc.filter64(x, top_k, top_p)
            cdf = fc.cdf64_filtered(x, keep)
            got = int(idx[s, t])
            if member and sc.margin(cdf, u[s, t]) > fc.BAND:
                want = sc.pick(cdf, u[s, t])
                assert got == want, "%s stream %d step %d: class %d, draw64_filtered %d (u = %r, %d classes kept)" % (label, s, t, got, want, u[s, t], int(keep.sum()))
                assert keep[got]
            else:
                undecided += 1
                assert fc.allowed_filtered(x, top_k, top_p, u[s, t], got), "%s stream %d step %d: class %d is not allowed on this undecided draw" % (label, s, t, got)
    assert undecided <= UNDECIDED_CAP * idx.size, "%s: %d of %d draws undecided" % (label, undecided, idx.size)
    return undecided


@pytest.mark.parametrize("label,cfgname,ns,env,variant", SHAPES, ids=[s[0] for s in SHAPES])
def test_filtered_jobs(label, cfgname, ns, env, variant, monkeypatch):
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    cfg, W, first, u = make_case(cfgname, 131, ns, N_GIVEN, N)
    eng = engine.Engine(cfg, W, n_streams=ns)
    assert eng.info()["kernel_variant"] == variant, eng.info()
    if "WN_V3_SLOTS" in env:
        assert eng.info()["skip_lane_slots"] == int(env["WN_V3_SLOTS"]), eng.info()
    if label == "lean4_ns4_mode3":
        assert eng.info()["skip_lane_slots"] == 0 and eng.info()["streams_per_item"] == 2, eng.info()
    kw = dict(uniforms=u, batched_prime=False, timeout_ms=8000)
    before = {T: eng.generate(N, first, temperature=T, **kw) for T in TEMPS}
    greedy = eng.generate(N, first, temperature=0.0, batched_prime=False, timeout_ms=8000)
    record = []
    for top_k, top_p in FILTERS:
        for T in TEMPS:
            tag = "%s (%d, %g) T=%g" % (label, top_k, top_p, T)
            idx, logits = eng.generate(N, first, temperature=T, want_logits=True, top_k=top_k, top_p=top_p, **kw)
            record.append((top_k, top_p, T, _replay(idx, logits, u, T, top_k, top_p, tag), int((idx != before[T]).sum())))
            assert np.array_equal(eng.generate(N, first, temperature=T, **kw), idx), tag + ": the job without the logits dump"     # (the handle keeps the filter)
    assert sum(r[4] for r in record) > 0, "no filter changed a single draw: %r" % (record,)
    print(label, "undecided / changed draws per (top_k, top_p, T):", record)
    # one stream (every second; the only one of a single-stream job) made greedy by its temperature: it ignores the filter, its neighbours do not
    temps = np.array([0.0 if (s % 2 == 1 or ns == 1) else 1.0 for s in range(ns)], dtype=np.float32)
    mixed = eng.generate(N, first, temperature=temps, top_k=8, top_p=0.0, **kw)
    only8 = eng.generate(N, first, temperature=1.0, top_k=8, top_p=0.0, **kw)
    for s in range(ns):
        assert np.array_equal(mixed[s], greedy[s] if temps[s] == 0 else only8[s]), "%s: stream %d of the job with per-stream temperatures" % (label, s)
    # top_k = 1 keeps the maximum alone
    assert np.array_equal(eng.generate(N, first, temperature=1.0, top_k=1, top_p=0.0, **kw), greedy), label + ": top_k = 1 against the greedy job"
    assert np.array_equal(eng.generate(N, first, temperature=1.0, top_k=0, top_p=1e-6, **kw), greedy), label + ": a vanishing top_p against the greedy job"
    # off again: the handle does what it did before any filter was set
    eng.set_sampling(0, 0.0)
    for T in TEMPS:
        assert np.array_equal(eng.generate(N, first, temperature=T, **kw), before[T]), "%s: after set_sampling(0, 0), T = %g" % (label, T)
    check_engine(eng, cfg, W, N, first, 1.0, 0.0, u, label + " after the filters")
    # the off values of the ABI are off
    eng.set_sampling(cfg.get("classes", 256) + 7, 1.0)
    assert np.array_equal(eng.generate(N, first, temperature=1.0, **kw), before[1.0]), label + ": top_k above the class count, top_p = 1"
    eng.close()


def test_error_codes_on_a_live_handle():
    cfg, W, first, u = make_case("tiny", 132, 1, N_GIVEN, 8)
    eng = engine.Engine(cfg, W, n_streams=1)
    assert eng.lib.has("wn_set_sampling")      # (binds the symbol: the binding resolves it on first use)
    d, h = eng.lib.dll, eng._h
    for top_k, top_p in ((-1, 0.0), (0, -0.5), (0, 1.5), (0, float("nan")), (-3, 0.5)):
        assert d.wn_set_sampling(h, top_k, ctypes.c_float(top_p)) == _abi.WN_E_BADARG, (top_k, top_p)
        assert "wn_set_sampling" in eng.lib.last_error()
    plain = eng.generate(8, first, temperature=1.0, uniforms=u, batched_prime=False)        # a refused call changed nothing
    for top_k, top_p in ((0, 1.0), (300, 0.0), (0x7fffffff, 1.0), (0, 0.0)):
        assert d.wn_set_sampling(h, top_k, ctypes.c_float(top_p)) == _abi.WN_OK, (top_k, top_p)
        assert np.array_equal(eng.generate(8, first, temperature=1.0, uniforms=u, batched_prime=False), plain)
    eng.close()


def test_facade_filters_and_rng_consumption():
    import wavenet_model
    cfg = synth.CONFIGS["cfg1"]
    W = synth.init_weights(cfg, seed=133)
    m = wavenet_model.WaveNetModel(output_length=8, **cfg)
    m.load_state_dict({k: torch.from_numpy(v) for k, v in W.items()})
    np.random.seed(5)
    one = m.generate_fast(64, temperature=1., top_k=1)
    state = np.random.get_state()       # (key words AND position: the keys alone stay the same for up to 312 draws)
    assert np.array_equal(one, m.generate_fast(64, temperature=0))
    np.random.seed(5)
    plain = m.generate_fast(64, temperature=1.)
    after = np.random.get_state()
    assert np.array_equal(after[1], state[1]) and after[2:] == state[2:], "a filtered call consumes the global RNG exactly as an unfiltered one"
    np.random.seed(5)
    np.random.random_sample(64)
    assert np.random.get_state()[2] == state[2], "64 uniforms for 64 samples"
    np.random.seed(5)
    nucleus = m.generate_fast(64, temperature=1., top_p=0.5)
    assert not np.array_equal(nucleus, plain)
    np.random.seed(5)
    assert np.array_equal(m.generate_fast(64, temperature=1.), plain), "the filter is off again after the filtered call"
    np.random.seed(5)
    rows = m.generate_fast_streams(64, [1.0, 0.0], top_k=1)
    assert np.array_equal(rows[0], one) and np.array_equal(rows[1], one)
