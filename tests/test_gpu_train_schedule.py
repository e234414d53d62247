"""The training step's stream schedule and A/B switches, end to end (pytorch-wavenet_amd/csrc/wn_train.inl).

wn_train_backward runs the weight gradients on a side stream ordered by events ([dF|dG] double-buffered by layer parity, dx a ping-pong
buffer, one partial-tile workspace per stream in deterministic mode), and the forward runs its grouped skip products there too.  A missing or
misplaced wait gives a wrong gradient only sometimes, which a tolerance test can pass by luck.  So the checker here is the SERIAL REFERENCE:
deterministic gradients (ordered reduction of the row splits) with WN_TRAIN_ONE_STREAM=1, every product in order on the caller's stream.
It uses exactly the default step's arithmetic, so

  class A -- a switch that only moves work between queues (or replaces fused kernels by their two-launch forms, which the kernel tests show
             to be bit-equal) must reproduce it BIT FOR BIT: logits, loss and every gradient;
  class B -- a switch that changes a weight-gradient product's tile or split plan changes only the order of fp32 sums inside the weight
             gradients: logits and loss bit-equal, every gradient within 2e-5 of its tensor's largest element, two runs bit-equal;
  class C -- WN_TRAIN_SKIP_BLOCK changes the forward's arithmetic (layers per grouped skip product): fp32 against torch autograd through the
             facade's CPU graph (test_gpu_training.py's bounds); bf16 against the default G under the bounds of
             test_bf16_step_reproduces_its_oracle_exactly_when_shallow, and no further from oracle/bf16_step.py than the default G;
  atomics -- the default step (fp32 atomics) against the serial reference: forward bit-equal, gradients within 2e-5.

Every switched run also carries a WITNESS that the switch took effect -- else a misspelt variable passes class A for free: the step's
kernel launches, recorded with torch.profiler as (name, stream, grid) from the trace's kernel events.  The `race` model (config 5's stack on
four one-second clips: products of hundreds of workgroups) makes real concurrency of the two streams the normal case.
"""
import collections
import contextlib
import json
import os
import sys
import tempfile

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "pytorch-wavenet_amd"))

pytestmark = pytest.mark.gpu

SWITCHES = ("WN_TRAIN_ONE_STREAM", "WN_TRAIN_SKIP_MAIN", "WN_TRAIN_RES_MAIN", "WN_TRAIN_SKIP_BLOCK", "WN_NO_TALL_WFG", "WN_TALL_SKIP",
            "WN_NO_FUSED_BWD", "WN_NO_FUSED_LAYER", "WN_NO_DSKIP_SHADOW", "WN_TN_WANT", "WN_TN_WANT_WIDE", "WN_TALL_WANT", "WN_DETERMINISTIC",
            "WN_TORCH_BACKWARD", "WN_TORCH_LOSS")
SERIAL = {"WN_TRAIN_ONE_STREAM": "1"}

W128 = dict(dilation_channels=128, residual_channels=128, skip_channels=512, end_channels=256, classes=256, kernel_size=2)
W32 = dict(dilation_channels=32, residual_channels=32, skip_channels=64, end_channels=64, classes=256, kernel_size=2)
# id: (config, N, output_length, clip length as receptive_field + output_length - 1 + this; None: the 16 000-sample clips of config 5)
MODELS = {
    "fused": (dict(layers=3, blocks=2, bias=True, **W128), 2, 24, 3),     # fused layer kernels, 256-column tiles, the bf16 shadows
    "short": (dict(layers=3, blocks=2, bias=True, **W128), 2, 24, -6),    # zero-padding regime: need[l] < L, sh < d, zlo rows
    "narrow": (dict(layers=3, blocks=2, bias=True, **W32), 2, 16, 2),     # 128-column forms, the two-tap weight gradient
    "narrow_nobias": (dict(layers=3, blocks=2, bias=False, **W32), 2, 16, 2),
    "race": (dict(layers=10, blocks=5, bias=False, **W128), 4, None, None),
}
_CACHE = {}


def _model(kind, precision):
    """One model (and so one training handle and workspace) per (kind, precision) for the whole module, with its seeded inputs."""
    key = (kind, precision)
    if key not in _CACHE:
        import wavenet_model
        from mi355_wavenet import synth
        cfg, n, out_len, extra = MODELS[kind]
        rf = synth.receptive_field(cfg)
        L = 16000 if extra is None else rf + out_len - 1 + extra
        out_len = L - rf + 1 if out_len is None else out_len
        m = wavenet_model.WaveNetModel(output_length=out_len, **cfg)
        m.load_state_dict({k: torch.from_numpy(v) for k, v in synth.init_weights(cfg, seed=17 + len(kind)).items()})
        m = m.cuda()
        m.matrix_precision = precision
        rs = np.random.RandomState(23)
        ids = torch.from_numpy(rs.randint(0, 256, (n, L)))
        target = torch.from_numpy(rs.randint(0, 256, (n * out_len,)))
        _CACHE[key] = (m, ids, target)
    return _CACHE[key]


class Step:
    def __init__(self, logits, loss, grads, launches):
        self.logits, self.loss, self.grads, self.launches = logits, loss, grads, launches

    def names(self):
        return collections.Counter(n for n, _, _ in self.launches)

    def streams(self):
        return set(s for _, s, _ in self.launches)

    def caller(self):
        """the caller's stream: the one the forward's first product (wn_fwd_start) ran on"""
        ss = [s for n, s, _ in self.launches if "wn_fwd_start" in n]
        assert len(ss) == 1, ss
        return ss[0]

    def on(self, stream):
        return sum(1 for _, s, _ in self.launches if s == stream)


def _launches(prof):
    """(kernel name, stream, grid) of every native kernel the profiled step launched, in start order"""
    fd, path = tempfile.mkstemp(suffix=".json")
    os.close(fd)
    try:
        prof.export_chrome_trace(path)
        with open(path) as f:
            trace = json.load(f)
    finally:
        os.remove(path)
    evs = [e for e in trace.get("traceEvents", []) if e.get("ph") == "X" and "kernel" in str(e.get("cat", "")).lower() and "wn_" in e.get("name", "")]
    evs.sort(key=lambda e: e["ts"])
    out = []
    for e in evs:
        args = e.get("args") or {}
        out.append((e["name"], args.get("stream", e.get("tid")), tuple(args.get("grid", ()))))
    return out


def _run(m, ids, target, env=None, det=True, stream=None, record=True):
    """One native training step (forward on class indices, the engine's fused loss, backward) with the given switches set for both its
    forward and its backward; the switches are read on every call.  Returns logits, loss, every gradient (numpy) and the launches."""
    from mi355_wavenet import training
    env = dict(env or {})
    saved = {k: os.environ.pop(k) for k in SWITCHES if k in os.environ}
    os.environ.update(env)
    try:
        m.deterministic_gradients = det
        m.zero_grad(set_to_none=True)
        torch.cuda.synchronize()
        prof = torch.profiler.profile(activities=[torch.profiler.ProfilerActivity.CUDA]) if record else contextlib.nullcontext()
        with prof:
            with (torch.cuda.stream(stream) if stream is not None else contextlib.nullcontext()):
                logits = m.train_forward_indices(ids.cuda())
                loss = training.cross_entropy(m._wn_train_runner, logits, target.cuda())
                loss.backward()
            torch.cuda.synchronize()
        assert not m.wn_stats()["torch_fallbacks"]
        grads = {k: (None if p.grad is None else p.grad.detach().cpu().numpy()) for k, p in m.named_parameters()}
        return Step(logits.detach().cpu().numpy(), loss.detach().cpu().numpy(), grads, _launches(prof) if record else None)
    finally:
        for k in env:
            os.environ.pop(k, None)
        os.environ.update(saved)


def _serial(kind, precision):
    key = ("serial", kind, precision)
    if key not in _CACHE:
        _CACHE[key] = _run(*_model(kind, precision), env=SERIAL)
        assert len(_CACHE[key].launches) > 0, "torch.profiler recorded no native kernel launches"
        assert len(_CACHE[key].streams()) == 1, _CACHE[key].streams()
    return _CACHE[key]


def _scrub(kind, precision):
    """One serial step of the same model on other clips and targets: every buffer the next step reads before it writes it (or reads too early)
    then holds another step's values -- a repeat of the same step would find the right bits left over from the last one."""
    m, ids, target = _model(kind, precision)
    _run(m, (ids + 1) % 256, (target + 1) % 256, env=SERIAL, record=False)


def _default(kind, precision):
    """the default two-stream schedule, deterministic mode"""
    key = ("default", kind, precision)
    if key not in _CACHE:
        _CACHE[key] = _run(*_model(kind, precision))
    return _CACHE[key]


def _bits(a):
    return a.view(np.uint32)


def _assert_forward_equal(got, ref, tag):
    assert np.array_equal(_bits(got.logits), _bits(ref.logits)), "%s: logits differ in %d elements" % (tag, int((got.logits != ref.logits).sum()))
    assert np.array_equal(_bits(got.loss), _bits(ref.loss)), (tag, float(got.loss), float(ref.loss))


def _assert_grads_equal(got, ref, tag):
    assert set(got.grads) == set(ref.grads)
    differ = {}
    for k, r in ref.grads.items():
        g = got.grads[k]
        assert (g is None) == (r is None), (tag, k)
        if r is not None and not np.array_equal(_bits(g), _bits(r)):
            scale = float(np.abs(r).max())
            differ[k] = (int((g != r).sum()), float(np.abs(g - r).max()) / max(scale, 1e-30))
    assert not differ, "%s: gradients not bit-equal to the serial reference (tensor: elements, largest deviation / max): %s" % (tag, differ)


def _assert_grads_close(got, ref, tag, tol=2e-5):
    worst = (0.0, None)
    for k, r in ref.grads.items():
        g = got.grads[k]
        assert (g is None) == (r is None), (tag, k)
        if r is None:
            continue
        scale = float(np.abs(r).max())
        err = float(np.abs(g.astype(np.float64) - r).max())
        assert err <= tol * scale + 1e-9, (tag, k, err, scale)
        worst = max(worst, (err / max(scale, 1e-30), k), key=lambda w: w[0])
    return worst


# ---------------------------------------------------------------------------------------------------- class A: same kernels, another queue
CLASS_A = {
    "two_streams": {},
    "skip_main": {"WN_TRAIN_SKIP_MAIN": "1"},
    "res_main_1": {"WN_TRAIN_RES_MAIN": "1"},
    "res_main_2": {"WN_TRAIN_RES_MAIN": "2"},     # lines up with the [dF|dG] buffer parity
    "res_main_3": {"WN_TRAIN_RES_MAIN": "3"},     # does not
    "skip_main_res_main_2": {"WN_TRAIN_SKIP_MAIN": "1", "WN_TRAIN_RES_MAIN": "2"},
    "caller_stream": {},                          # the default step on a non-default torch stream
    "no_fused_bwd": {"WN_NO_FUSED_BWD": "1"},
    "no_fused_layer": {"WN_NO_FUSED_LAYER": "1"},
    "no_dskip_shadow": {"WN_NO_DSKIP_SHADOW": "1"},
}
BF16_ONLY = ("no_fused_bwd", "no_fused_layer", "no_dskip_shadow")   # (the fused kernels and the dskip shadow exist at the 128 / 128 bf16 shape)
MODELS_A = [("fused", "bf16"), ("fused", "fp32"), ("short", "bf16"), ("narrow", "fp32"), ("narrow_nobias", "fp32"), ("race", "bf16"), ("race", "fp32")]
CASES_A = [(k, p, c) for k, p in MODELS_A for c in CLASS_A if p == "bf16" or c not in BF16_ONLY]


@pytest.mark.parametrize("kind,precision,case", CASES_A)
def test_class_a_bit_equal_to_the_serial_reference(kind, precision, case):
    m, ids, target = _model(kind, precision)
    ref = _serial(kind, precision)
    if case == "two_streams":   # run twice in one process: the events and workspaces are reused between forward and backward, and between steps
        _scrub(kind, precision)
        first = _default(kind, precision)
        _scrub(kind, precision)
        got = _run(m, ids, target)
        for tag, s in (("first two-stream run", first), ("second two-stream run", got)):
            _assert_forward_equal(s, ref, tag)
            _assert_grads_equal(s, ref, tag)
    else:
        _scrub(kind, precision)
        got = _run(m, ids, target, env=CLASS_A[case], stream=torch.cuda.Stream() if case == "caller_stream" else None)
        _assert_forward_equal(got, ref, case)
        _assert_grads_equal(got, ref, case)
    # the witness
    dflt = _default(kind, precision)
    assert len(got.streams()) == 2, got.streams()
    if case in ("no_fused_bwd", "no_fused_layer"):
        assert len(got.launches) > len(ref.launches) and got.names() != ref.names()
        return
    if case == "no_dskip_shadow":   # the same launches; the skip weight gradient takes its form with an fp32 A operand
        assert len(got.launches) == len(ref.launches) and got.names() != ref.names()
        return
    assert got.names() == ref.names()
    if case.startswith("skip_main") or case.startswith("res_main"):
        assert got.on(got.caller()) > dflt.on(dflt.caller()), (case, got.on(got.caller()), dflt.on(dflt.caller()))
    if case == "caller_stream":
        assert got.caller() != dflt.caller() and got.on(got.caller()) == dflt.on(dflt.caller())


# ---------------------------------------------------------------------------------------------------- class B: another tile or split plan
CASES_B = [
    ("fused", "bf16", {"WN_NO_TALL_WFG": "1"}),
    ("race", "bf16", {"WN_NO_TALL_WFG": "1"}),
    ("race", "bf16", {"WN_TALL_SKIP": "1"}),
    ("race", "bf16", {"WN_TN_WANT_WIDE": "16"}),
    ("race", "bf16", {"WN_TN_WANT_WIDE": "8192"}),
    ("race", "bf16", {"WN_TALL_WANT": "16"}),
    ("race", "bf16", {"WN_TALL_WANT": "2048"}),
    ("race", "bf16", {"WN_TN_WANT": "16"}),   # (a large value changes nothing here: every bf16 product this switch plans is at the M / 256 cap already)
    ("race", "fp32", {"WN_TN_WANT": "16"}),
    ("race", "fp32", {"WN_TN_WANT": "8192"}),
]


@pytest.mark.parametrize("kind,precision,env", CASES_B, ids=["%s-%s-%s" % (k, p, "-".join("%s=%s" % kv for kv in e.items())) for k, p, e in CASES_B])
def test_class_b_another_split_plan(kind, precision, env):
    m, ids, target = _model(kind, precision)
    ref = _serial(kind, precision)
    _scrub(kind, precision)
    a = _run(m, ids, target, env=env)
    _scrub(kind, precision)
    b = _run(m, ids, target, env=env, record=False)
    _assert_forward_equal(a, ref, str(env))
    worst = _assert_grads_close(a, ref, str(env))
    _assert_grads_equal(b, a, "%s, second run" % env)
    print("%s %s %s: gradients within %.1e of a tensor's max of the serial reference (%s)" % (kind, precision, env, worst[0], worst[1]))
    dflt = _default(kind, precision)
    assert a.launches != dflt.launches   # the witness: another kernel or grid


# ---------------------------------------------------------------------------------------------------- class C: layers per grouped skip product
def _torch_reference(kind):
    """torch autograd through the facade's graph on the CPU (the reference's conv1d / dilate graph), the model's fp32 weights"""
    key = ("torch", kind)
    if key not in _CACHE:
        import wavenet_model
        m, ids, target = _model(kind, "fp32")
        cfg = MODELS[kind][0]
        ref = wavenet_model.WaveNetModel(output_length=m.output_length, **cfg)
        ref.load_state_dict({k: v.detach().cpu() for k, v in m.state_dict().items()})
        n, L = ids.shape
        x = torch.zeros(n, 256, L).scatter_(1, ids.view(n, 1, L), 1.0)
        out = ref(x)
        loss = torch.nn.functional.cross_entropy(out, target)
        loss.backward()
        _CACHE[key] = Step(out.detach().numpy(), loss.detach().numpy(),
                           {k: (None if p.grad is None else p.grad.numpy()) for k, p in ref.named_parameters()}, None)
    return _CACHE[key]


@pytest.mark.parametrize("kind", ["fused", "narrow"])
@pytest.mark.parametrize("g", [1, 2, 4, 11])   # NL = 6: 2 divides it, 4 leaves a 2-layer remainder block, 11 = NL + 5 is clipped to NL
def test_class_c_skip_block_fp32_against_torch_autograd(kind, g):
    m, ids, target = _model(kind, "fp32")
    ref = _torch_reference(kind)
    got = _run(m, ids, target, env={"WN_TRAIN_SKIP_BLOCK": str(g)})
    dl = float(np.abs(got.logits - ref.logits).max())
    assert dl <= 1e-4 * max(1.0, float(np.abs(ref.logits).max())), dl
    assert abs(float(got.loss) - float(ref.loss)) <= 1e-5 * max(1.0, abs(float(ref.loss)))
    worst = _assert_grads_close(got, ref, "WN_TRAIN_SKIP_BLOCK=%d" % g)
    print("%s fp32, %d layers per grouped skip product: logits %.2e, gradients %.1e of a tensor's max (%s) from torch autograd" % (kind, g, dl, worst[0], worst[1]))
    assert got.launches != _default(kind, "fp32").launches


# (layers, blocks, g): g = 2 and g = 4 leave a remainder block of 1 and 2 layers; g = NL + 5 is clipped to NL
BF16_C = [(2, 1, 1), (3, 1, 2), (3, 2, 4), (1, 2, 7)]


def _digest_devs(ref, got):
    """per tensor: the largest relative deviation of the digest (tests/golden/digest.py) of `got` from that of `ref`"""
    out = []
    for k, r in ref.items():
        if r[0] > 0:
            q = got[k]
            out.append(max(abs(q[0] - r[0]) / r[0], abs(q[1] - r[1]) / r[1], float(np.abs(q[2:6] - r[2:6]).max()) / r[1], float(np.abs(q[6:] - r[6:]).max()) / r[0]))
    return np.array(out)


@pytest.mark.parametrize("layers,blocks,g", BF16_C)
def test_class_c_skip_block_bf16_against_its_oracle(layers, blocks, g):
    """bf16: the forward's grouped skip product of a block reads the block's skip weights from the transposed bf16 bank, which the forward
    converts per block -- the last, shorter block included (before that fix it read whatever the workspace held: every logit row off).
    Another G changes only the fp32 order of the skip sum, so against the default G of the same model the criteria of
    test_bf16_step_reproduces_its_oracle_exactly_when_shallow hold (at most 2 logit rows with a flipped rounding, loss 2e-4, gradient digests 3e-3);
    against oracle/bf16_step.py the step may be no further than the default G's step is (beyond two layers a rounding flip in an early layer
    reaches every output row of its receptive field, so the exact criteria are not decidable there -- oracle/bf16_step.py)."""
    sys.path.insert(0, os.path.join(ROOT, "oracle"))
    sys.path.insert(0, os.path.join(ROOT, "tests", "golden"))
    import bf16_step
    import digest as dg
    import wavenet_model
    from mi355_wavenet import synth
    cfg = dict(layers=layers, blocks=blocks, dilation_channels=128, residual_channels=128, skip_channels=256, end_channels=256, classes=256,
               kernel_size=2, bias=True)
    W = synth.init_weights(cfg, seed=61 + 10 * layers + blocks)
    out_len, N = 8, 2
    m = wavenet_model.WaveNetModel(output_length=out_len, **cfg)   # (a fresh model: a workspace no earlier step of it wrote)
    m.load_state_dict({k: torch.from_numpy(v) for k, v in W.items()})
    m = m.cuda()
    m.matrix_precision = "bf16"
    rs = np.random.RandomState(5)
    ids = rs.randint(0, 256, (N, m.receptive_field + out_len - 1 + 16))
    target = rs.randint(0, 256, (N * out_len,))
    got = _run(m, torch.from_numpy(ids), torch.from_numpy(target), env={"WN_TRAIN_SKIP_BLOCK": str(g)})
    dflt = _run(m, torch.from_numpy(ids), torch.from_numpy(target))
    assert got.launches != dflt.launches
    lo, ls, gr = bf16_step.step(cfg, W, ids, target, out_len, round_operands=True)
    lo32, _, _ = bf16_step.step(cfg, W, ids, target, out_len, round_operands=False)
    scale = max(1.0, float(np.abs(lo).max()))
    moved = float(np.abs(lo - lo32).max())
    assert moved > 20e-5 * scale                                   # (the roundings are really in it)
    full = dict(m.named_parameters())

    def digest(s):
        return dg.digest({k: (v if v is not None else np.zeros(tuple(full[k].shape), np.float32)) for k, v in s.grads.items()})

    row_self = np.abs(got.logits - dflt.logits).max(axis=1)
    flipped = int((row_self > 1e-5 * scale).sum())
    dev_self = _digest_devs(digest(dflt), digest(got))
    dev_o, dev_o_d = float(np.abs(got.logits - lo).max()), float(np.abs(dflt.logits - lo).max())
    dg_o, dg_o_d = float(_digest_devs(dg.digest(gr), digest(got)).max()), float(_digest_devs(dg.digest(gr), digest(dflt)).max())
    print("bf16, %d x %d layers, %d per grouped skip product: vs the default G -- %d of %d logit rows off (largest %.2e), loss %.6f vs %.6f, gradient digests %.2e; "
          "vs the oracle (the roundings move the logits %.2e) -- logits %.2e (default G: %.2e), loss %.6f, gradient digests %.2e (default G: %.2e)" % (
              layers, blocks, g, flipped, len(row_self), float(row_self.max()), float(got.loss), float(dflt.loss), float(dev_self.max()), moved, dev_o, dev_o_d,
              ls, dg_o, dg_o_d))
    assert flipped <= 2 and float(row_self.max()) <= 0.5 * moved, (flipped, row_self)
    assert abs(float(got.loss) - float(dflt.loss)) <= 2e-4 * max(1.0, abs(float(dflt.loss)))
    assert float(dev_self.max()) <= 3e-3, dev_self
    assert dev_o <= max(dev_o_d, 0.5 * moved) and abs(float(got.loss) - ls) <= 2e-4 * max(1.0, abs(ls))
    assert dg_o <= max(1.5 * dg_o_d, 3e-3), (dg_o, dg_o_d)


# ---------------------------------------------------------------------------------------------------- atomics
@pytest.mark.parametrize("precision", ["bf16", "fp32"])
def test_atomics_two_streams_against_the_serial_reference(precision):
    m, ids, target = _model("race", precision)
    ref = _serial("race", precision)
    _scrub("race", precision)
    got = _run(m, ids, target, det=False)
    _assert_forward_equal(got, ref, "atomics")
    worst = _assert_grads_close(got, ref, "atomics")
    print("race %s, fp32 atomics on two streams: gradients within %.1e of a tensor's max of the serial reference (%s)" % (precision, worst[0], worst[1]))
    assert len(got.streams()) == 2 and got.launches != _default("race", precision).launches   # (no ordered reductions)
