"""-m gpu: a stream's generation state saved, loaded and fanned out through Engine (wn_state_save / wn_state_load / wn_prime_shared) and through the
facade (generate_fast(continue_from=, return_state=), generate_fast_streams(continue_from=)).  Pure copies are held to BIT equality; where two
kernel forms or the oracle meet, the seeds are chosen on the CPU so that every draw of the oracle lies at least 1e-5 from a CDF boundary
(parity_common.softmax_cdf): no draw is undecided and the comparison is plain equality.  Queues across forms: the existing bar, 1e-5 of scale;
against the torch restatement: the existing 2e-6."""
import ctypes
import pickle
import time

import numpy as np
import pytest
import torch

import c_oracle
import restated
import wavenet_model
from mi355_wavenet import _abi, engine, synth
from mi355_wavenet.state import GenerationState, queue_lengths
from parity_common import make_case, softmax_cdf
from test_gpu_parity import MINI3, PADDED

pytestmark = pytest.mark.gpu
TINY = synth.CONFIGS["tiny"]
TINY3 = dict(TINY, kernel_size=3)
N2 = 41
_T0 = time.time()


@pytest.fixture(scope="module", autouse=True)
def _timing():
    yield
    print("\ntest_gpu_generation_state: %.1f s wall" % (time.time() - _T0))


def _padded_cfg(label):
    _, chans, depth, bias, _ = [c for c in PADDED if c[0] == label][0]
    return dict(layers=depth[0], blocks=depth[1], dilation_channels=chans[0], residual_channels=chans[1], skip_channels=chans[2],
                end_channels=chans[3], classes=256, kernel_size=2, bias=bias)


def _roll_check(dst_q, src_q, shift, tol=0.0):
    """the destination's exported queue = the source's, rolled by the difference of the queue times"""
    (dd, di, do), (sd, si, so) = dst_q, src_q
    ml = sd.shape[1]
    assert di == do == (si + shift) % ml
    want = np.roll(sd, shift, axis=1)
    if tol == 0.0:
        assert np.array_equal(dd, want)
    else:
        assert np.abs(dd - want).max() <= tol * max(1.0, float(np.abs(want).max()))


def _resume_equals_one_shot(cfg, ns, N1, seed, variant=None, check=None):
    cfg, W, first, u = make_case(cfg, seed, ns, 6, N1 + N2)
    src = engine.Engine(cfg, W, n_streams=ns)
    info = src.info()
    if variant is not None:
        assert info["kernel_variant"] == variant, info
    if check is not None:
        check(info)
    full = src.generate(N1 + N2, first, temperature=1.0, uniforms=u)
    a = src.generate(N1, first, temperature=1.0, uniforms=u[:, :N1])
    t_src = src.info()["evals_done"]
    assert t_src == 5 + N1
    states = [src.state_save(s) for s in range(ns)]
    assert all(st.dtype == np.float32 and st.shape == (src.state_floats(),) for st in states)
    assert src.state_floats() == cfg["residual_channels"] * sum(queue_lengths(cfg["layers"], cfg["blocks"], cfg["kernel_size"]))
    NL = cfg["layers"] * cfg["blocks"]
    probes = [(l, s) for l in sorted(set((0, cfg["layers"] - 1, NL - 1))) for s in sorted(set((0, ns - 1)))]
    src_q = {p: src.export_queue(*p) for p in probes}
    dst = engine.Engine(cfg, W, n_streams=ns)
    assert dst.info()["kernel_variant"] == info["kernel_variant"] and dst.info()["streams_per_item"] == info["streams_per_item"]
    dst.generate(7, None, temperature=0.0)   # another queue time: the rotation is not the identity
    t_dst = dst.info()["evals_done"]
    assert t_dst == 7
    for s in range(ns):
        dst.state_load(states[s], s, 1)
    assert dst.info()["evals_done"] == t_dst
    for s in range(ns):
        assert dst.state_save(s).tobytes() == states[s].tobytes(), "stream %d: the saved state of the destination differs" % s
    for p in probes:
        _roll_check(dst.export_queue(*p), src_q[p], t_dst - t_src)
    b = dst.generate(N2, a[:, -1:], temperature=1.0, uniforms=u[:, N1:], reset=False)
    src.close()
    dst.close()
    assert np.array_equal(np.concatenate([a, b], axis=1), full)


FORMS = [("tiny_generic", TINY, 1, "generic", 1, None),
         ("tiny_k3", TINY3, 1, None, 1, None),
         ("cfg1_x2_stacked", "cfg1", 2, None, 4, None),
         ("mini3_x1", MINI3, 1, None, 3, lambda i: i["streams_per_item"] == 1),
         ("mini3_x12", MINI3, 12, None, 3, lambda i: i["streams_per_item"] == 2 and i["head_replicas"] == 2)]


@pytest.mark.parametrize("N1", [3, 23])   # less than the largest ring holds, and wrapped
@pytest.mark.parametrize("label,cfg,ns,pin,variant,form", FORMS, ids=[f[0] for f in FORMS])
def test_resume_equals_one_shot_same_kernel_form(label, cfg, ns, pin, variant, form, N1, monkeypatch):
    if pin:
        monkeypatch.setenv("WN_KERNEL", pin)

    def check(info):
        assert form is None or form(info), info
    _resume_equals_one_shot(cfg, ns, N1, 301, variant, check)


def _decided(cfg, W, N, first, make_u, what):
    """uniforms (N,) for which every draw of the oracle lies at least 1e-5 from a CDF boundary: tries seeds until one is"""
    for seed in range(50):
        u = make_u(np.random.RandomState(7000 + seed))
        o_idx, o_log = c_oracle.generate(cfg, W, N, first, 1.0, 0.0, u)
        if min(float(np.abs(softmax_cdf(o_log[t], 1.0, None) - u[t]).min()) for t in range(N)) >= 1e-5:
            return u, o_idx
    raise AssertionError("%s: no seed of 50 keeps every draw 1e-5 from a CDF boundary" % what)


def test_across_forms_and_stream_counts_and_fan_out(monkeypatch):
    N1 = 23
    cfg, W, first, _ = make_case("cfg1", 302, 5, 6, N1 + N2)
    u_one, o_one = _decided(cfg, W, N1 + N2, first[0], lambda rs: rs.random_sample(N1 + N2), "first continuation")
    u_two, o_two = _decided(cfg, W, N1 + N2, first[0], lambda rs: np.concatenate([u_one[:N1], rs.random_sample(N2)]), "second continuation")
    assert np.array_equal(o_one[:N1], o_two[:N1])
    src = engine.Engine(cfg, W, n_streams=1)
    assert src.info()["kernel_variant"] == 4
    a = src.generate(N1, first[:1], temperature=1.0, uniforms=u_one[None, :N1])
    assert np.array_equal(a[0], o_one[:N1])
    state = src.state_save(0)
    monkeypatch.setenv("WN_KERNEL", "v3")
    dst = engine.Engine(cfg, W, n_streams=5)
    assert dst.info()["kernel_variant"] == 3
    rs = np.random.RandomState(11)
    own = dst.generate(9, first, temperature=1.0, uniforms=rs.random_sample((5, 9)))   # every stream has a history of its own
    keep = {s: dst.state_save(s) for s in (0, 4)}
    dst.state_load(state, 1, 3)
    for s in (0, 4):
        assert dst.state_save(s).tobytes() == keep[s].tobytes(), "stream %d lost its own state" % s
    for s in (1, 2, 3):
        assert dst.state_save(s).tobytes() == state.tobytes()
    nxt = own[:, -1:].copy()
    nxt[1:4, 0] = a[0, -1]
    u = rs.random_sample((5, N2))
    u[1] = u[2] = u_one[N1:]
    u[3] = u_two[N1:]
    b = dst.generate(N2, nxt, temperature=1.0, uniforms=u, reset=False)
    assert np.array_equal(b[1], b[2]) and not np.array_equal(b[1], b[3])
    assert np.array_equal(b[1], o_one[N1:]) and np.array_equal(b[3], o_two[N1:])
    src.generate(N2, a[:, -1:], temperature=1.0, uniforms=u_one[None, N1:], reset=False)   # the source goes the same way: queues to the cross-variant bar
    shift = dst.info()["evals_done"] - src.info()["evals_done"]
    for l in (0, 4, 9):
        _roll_check(dst.export_queue(l, 1), src.export_queue(l, 0), shift, tol=1e-5)
    src.close()
    dst.close()


def test_from_the_oracles_queues():
    cfg, W = TINY, synth.init_weights(TINY, seed=303)
    inputs = np.random.RandomState(303).randint(0, 256, 24)   # 23 evaluations, and the input of the next
    u, o_idx = _decided(cfg, W, N2, inputs, lambda rs: rs.random_sample(N2), "oracle continuation")
    m = restated.RestatedWaveNet(cfg, W)
    for i in inputs[:23]:
        m.wavenet_step(m._onehot(i))
    st = GenerationState.from_reference_queues(m.queues, int(inputs[23]), 23)
    eng = engine.Engine(cfg, W, n_streams=1)
    eng.reset()
    eng.state_load(st.state)
    for l, (data, in_pos, out_pos) in enumerate(st.to_reference_queues(0)):
        got, gi, go = eng.export_queue(l, 0)
        assert (gi, go) == (in_pos, out_pos) == (0, 0) and np.abs(got - data).max() <= 2e-6
        assert np.array_equal(np.roll(got, 23, axis=1), m.queues[l].data.numpy())
    out = eng.generate(N2, np.asarray([[st.last_index]]), temperature=1.0, uniforms=u[None], reset=False)
    eng.close()
    assert np.array_equal(out[0], o_idx)


@pytest.mark.parametrize("label", ["pad_to_cfg1_shape", "odd_counts"])
def test_padded_and_odd_shapes(label):
    cfg = _padded_cfg(label)
    eng = engine.Engine(cfg, synth.init_weights(cfg, seed=1), n_streams=2)
    assert eng.state_floats() == cfg["residual_channels"] * sum(queue_lengths(cfg["layers"], cfg["blocks"], 2))   # the caller's channels
    eng.close()
    for N1 in (3, 23):
        _resume_equals_one_shot(cfg, 2, N1, 304)


def test_rounds_load_across_the_seam():
    ns = 170
    cfg, W, first, u = make_case(MINI3, 305, ns, 3, 15)
    eng = engine.Engine(cfg, W, n_streams=ns)
    assert eng.info()["n_chains"] == 2
    own = eng.generate(5, first, temperature=1.0, uniforms=u[:, :5], timeout_ms=8000)
    state = eng.state_save(3)
    keep = {s: eng.state_save(s) for s in (83, 88)}
    assert keep[83].tobytes() != state.tobytes()
    eng.state_load(state, 84, 4)   # 84, 85: the first round's last streams; 86, 87: the second round's first
    for s in range(84, 88):
        assert eng.state_save(s).tobytes() == state.tobytes(), s
    for s in (83, 88):
        assert eng.state_save(s).tobytes() == keep[s].tobytes(), s
    nxt = own[:, -1:].copy()
    nxt[84:88, 0] = own[3, -1]
    uu = u[:, 5:].copy()
    uu[84:88] = uu[3]
    out = eng.generate(10, nxt, temperature=1.0, uniforms=uu, reset=False, timeout_ms=8000)
    eng.close()
    for s in range(84, 88):
        assert np.array_equal(out[s], out[3]), s
    assert not np.array_equal(out[83], out[84]) and not np.array_equal(out[88], out[87])


@pytest.mark.parametrize("label,cfg,ns", [("cfg1_x3", "cfg1", 3), ("mini3_x12", MINI3, 12)], ids=["cfg1_x3", "mini3_x12"])
def test_shared_priming_is_bit_equal_to_priming_every_stream(label, cfg, ns):
    """the gate for generate_fast_streams: wn_prime_shared leaves what wn_prime leaves on repeated rows, in every stream"""
    cfg, W, first, u = make_case(cfg, 306, 1, 201, 20)
    rows = np.repeat(first, ns, axis=0)
    uu = np.random.RandomState(306).random_sample((ns, 20))
    eng = engine.Engine(cfg, W, n_streams=ns)
    eng.reset()
    assert eng.prime_host(rows[:, :200]) and eng.info()["evals_done"] == 200
    per_stream = [eng.state_save(s) for s in range(ns)]
    job = eng.generate(20, rows[:, -1:], temperature=1.0, uniforms=uu, reset=False)
    eng.reset()
    assert eng.prime_shared(first[0, :200]) is True and eng.info()["evals_done"] == 200
    for s in range(ns):
        assert eng.state_save(s).tobytes() == per_stream[s].tobytes(), "stream %d" % s
    assert per_stream[0].any() and all(p.tobytes() == per_stream[0].tobytes() for p in per_stream)
    assert np.array_equal(eng.generate(20, rows[:, -1:], temperature=1.0, uniforms=uu, reset=False), job)
    with pytest.raises(_abi.WnError) as e:   # queues that are not fresh
        eng.prime_shared(first[0, :200])
    assert e.value.code == _abi.WN_E_STATE
    assert np.array_equal(eng.generate(20, rows, temperature=1.0, uniforms=uu, shared_prompt=True), eng.generate(20, rows, temperature=1.0, uniforms=uu))
    eng.close()


def test_shared_priming_fills_every_round():
    """170 streams in two rounds: the products run once (on the first round's handle), both rounds' rings are filled from that result"""
    ns = 170
    cfg, W, first, _ = make_case(MINI3, 309, 1, 201, 8)
    rows = np.repeat(first, ns, axis=0)
    uu = np.random.RandomState(309).random_sample((ns, 8))
    eng = engine.Engine(cfg, W, n_streams=ns)
    assert eng.info()["n_chains"] == 2
    eng.reset()
    assert eng.prime_host(rows[:, :200])
    per_stream = {s: eng.state_save(s) for s in (0, 85, 86, 169)}
    job = eng.generate(8, rows[:, -1:], temperature=1.0, uniforms=uu, reset=False, timeout_ms=8000)
    eng.reset()
    assert eng.prime_shared(first[0, :200]) is True and eng.info()["evals_done"] == 200
    for s, st in per_stream.items():
        assert st.any() and eng.state_save(s).tobytes() == st.tobytes(), "stream %d" % s
    assert np.array_equal(eng.generate(8, rows[:, -1:], temperature=1.0, uniforms=uu, reset=False, timeout_ms=8000), job)
    eng.close()


def test_shared_priming_answers_unsupported_where_wn_prime_does():
    W = synth.init_weights(TINY3, seed=2)
    eng = engine.Engine(TINY3, W, n_streams=2)
    row = np.arange(100) % 256
    assert eng.prime_host(np.stack([row, row])) is False
    assert eng.prime_shared(row) is False
    rc = eng.lib.dll.wn_prime_shared(eng._h, eng.mem.ptr(eng.mem.upload(row.astype(np.int32))), 100, eng.mem.stream())
    assert rc == _abi.WN_E_UNSUPPORTED and "wn_prime_shared" in eng.lib.last_error()
    assert eng.info()["evals_done"] == 0
    eng.close()


def _model(cfg, W):
    m = wavenet_model.WaveNetModel(output_length=8, **cfg)
    m.load_state_dict({k: torch.from_numpy(v) for k, v in W.items()})
    return m


def test_facade_continue_from_and_return_state(monkeypatch):
    cfg = synth.CONFIGS["cfg1"]
    W = synth.init_weights(cfg, seed=307)
    m = _model(cfg, W)
    first = torch.from_numpy(np.random.RandomState(307).randint(0, 256, 10))
    n1, n2 = 30, 50
    np.random.seed(5)
    full = m.generate_fast(n1 + n2, first_samples=first)
    after_full = np.random.random_sample()
    np.random.seed(5)
    a, st = m.generate_fast(n1, first_samples=first, return_state=True)
    assert isinstance(st, GenerationState) and st.evals == 9 + n1 and st.geometry()["residual_channels"] == 32
    b = m.generate_fast(n2, continue_from=st)
    assert np.random.random_sample() == after_full, "the RNG was consumed differently"
    assert np.array_equal(np.concatenate([a, b]), full)
    # callbacks: at the positions of first_samples=[last_index]
    calls_a, calls_b = [], []
    np.random.seed(6)
    ref = m.generate_fast(n2, first_samples=torch.tensor([st.last_index]), progress_callback=lambda i, n: calls_a.append((i, n)), progress_interval=7)
    np.random.seed(6)
    b2, st2 = m.generate_fast(n2, continue_from=st, progress_callback=lambda i, n: calls_b.append((i, n)), progress_interval=7, return_state=True)
    assert calls_a == calls_b and len(calls_a) >= 5
    assert ref.shape == b2.shape
    assert st2.evals == st.evals + n2
    # a pickled state in a fresh model; a list of states is a 2-D job
    m2 = _model(cfg, W)
    np.random.seed(6)
    assert np.array_equal(m2.generate_fast(n2, continue_from=pickle.loads(pickle.dumps(st))), b2)
    np.random.seed(6)
    two, sts = m2.generate_fast(n2, continue_from=[st, st], return_state=True)
    assert two.shape == (2, n2) and isinstance(sts, list) and len(sts) == 2
    assert all(x.evals == st.evals + n2 and x.state.size == st.state.size for x in sts)
    # N variations of a checkpoint: equal temperature and equal uniforms give equal rows
    fixed = np.random.RandomState(9).random_sample(n2)
    monkeypatch.setattr(np.random, "random_sample", lambda size=None: fixed.copy().reshape(size))
    rows = m.generate_fast_streams(n2, [1.0, 1.0, 0.5, 0.0], continue_from=st)
    one = m.generate_fast(n2, continue_from=st, temperature=1.0)
    assert rows.shape == (4, n2) and np.array_equal(rows[0], rows[1]) and not np.array_equal(rows[0], rows[2])
    assert np.array_equal(rows[0], one)
    assert np.array_equal(rows[3], m.generate_fast(n2, continue_from=st, temperature=0.0))


def test_generate_fast_streams_without_a_state_returns_what_it_returned():
    cfg = synth.CONFIGS["cfg1"]
    m = _model(cfg, synth.init_weights(cfg, seed=308))
    first = torch.from_numpy(np.random.RandomState(308).randint(0, 256, 130))
    temps = [1.0, 0.7, 0.0]
    assert m.SHARED_PRIME is True
    np.random.seed(8)
    new = m.generate_fast_streams(40, temps, first_samples=first)
    m.SHARED_PRIME = False   # the per-stream pass over repeated rows
    np.random.seed(8)
    old = m.generate_fast_streams(40, temps, first_samples=first)
    assert np.array_equal(new, old)
    np.random.seed(8)
    assert np.array_equal(m.generate_fast(40, first_samples=first, temperature=1.0), new[0])


def test_error_codes_on_a_live_handle():
    eng = engine.Engine(TINY, synth.init_weights(TINY, seed=1), n_streams=3)
    d, h, st = eng.lib.dll, eng._h, eng.mem.stream()
    assert eng.lib.has("wn_state_load") and eng.lib.has("wn_state_save") and eng.lib.has("wn_state_floats") and eng.lib.has("wn_prime_shared")
    buf = eng.mem.empty((eng.state_floats(),), np.float32)
    p = eng.mem.ptr(buf)
    assert d.wn_state_floats(h, None) == _abi.WN_E_BADARG
    assert d.wn_state_save(h, 0, None, st) == _abi.WN_E_BADARG and d.wn_state_load(h, 0, 1, None, st) == _abi.WN_E_BADARG
    assert d.wn_prime_shared(h, None, 4, st) == _abi.WN_E_BADARG
    for s in (-1, 3):
        assert d.wn_state_save(h, s, p, st) == _abi.WN_E_BADARG and "stream" in eng.lib.last_error()
    for s0, cnt in ((-1, 1), (0, 0), (0, -1), (0, 4), (2, 2), (3, 1)):
        assert d.wn_state_load(h, s0, cnt, p, st) == _abi.WN_E_BADARG, (s0, cnt)
    assert d.wn_state_load(h, 0, 3, p, st) == 0 and d.wn_state_load(h, 2, 1, p, st) == 0
    eng.close()
    # before wn_load_weights: the state calls serve the zero queues, priming needs the weights
    c = _abi.wn_config(TINY["layers"], TINY["blocks"], TINY["dilation_channels"], TINY["residual_channels"], TINY["skip_channels"], TINY["end_channels"],
                       256, 2, 0, 2, 0, 0, 0)
    raw = ctypes.c_void_p()
    assert d.wn_create(ctypes.byref(c), ctypes.byref(raw)) == 0
    try:
        n = ctypes.c_int64()
        assert d.wn_state_floats(raw, ctypes.byref(n)) == 0 and n.value == 16 * sum(queue_lengths(3, 2, 2))
        ones = torch.ones(n.value, dtype=torch.float32, device="cuda")
        out = torch.full((n.value,), 7.0, dtype=torch.float32, device="cuda")
        assert d.wn_state_save(raw, 1, out.data_ptr(), st) == 0
        torch.cuda.synchronize()
        assert not out.cpu().numpy().any()   # the zeros of a fresh handle
        assert d.wn_state_load(raw, 1, 1, ones.data_ptr(), st) == 0
        assert d.wn_state_save(raw, 1, out.data_ptr(), st) == 0
        torch.cuda.synchronize()
        assert (out.cpu().numpy() == 1.0).all()
        assert d.wn_state_save(raw, 0, out.data_ptr(), st) == 0
        torch.cuda.synchronize()
        assert not out.cpu().numpy().any()   # the other stream keeps its zero history
        row = torch.zeros(8, dtype=torch.int32, device="cuda")
        assert d.wn_prime_shared(raw, row.data_ptr(), 8, st) == _abi.WN_E_STATE
    finally:
        d.wn_destroy(raw)
