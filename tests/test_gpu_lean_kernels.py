"""-m gpu: the two instantiations of the generation kernels against the C oracle and against each other.

The chain kernels (csrc/wn_kernel_v3.h, wn_kernel_v4.h) exist twice: the product ("lean") instantiation, and the DIAG one that carries the
wall-clock stamps and the sampler's logits dump; the host launches DIAG for a job with `profile_next` or `want_logits` (wn_chain_launch).
(The slot re-use form exists in the DIAG instantiation alone: profiles/r12_lean_item_loops.txt.)  Every publication takes one of two store
flavours, L2-resident or write-through, by a workgroup-uniform flag tested outside the store's lane predicate; WN_NO_LOCAL_STORES=1 pins the second.

`check_engine` asks for the logits, so what it holds against the oracle is the DIAG instantiation; every case therefore also runs the same job
WITHOUT logits (the lean instantiation) and requires identical indices -- the two differ in diagnostics only, never in arithmetic.

Shape: cfg3's channels (128 / 128 / 512 / 256, 256 classes) on layers=4, blocks=1: first, middle and last layer; dilations 1, 2, 4, 8, so at 4-8
streams the queue group's `near` (d = 2) and `late` (d = 4, 8) paths both occur next to d = 1; 48 samples = three receptive fields, so the
dilation queues wrap.  WN_TESTING=1 (tests/conftest.py) lets the pins through."""
import numpy as np
import pytest

from mi355_wavenet import engine, synth
from parity_common import check_engine, make_case

pytestmark = pytest.mark.gpu

LEAN4 = dict(synth.CONFIGS["cfg3"], layers=4, blocks=1)
N, N_GIVEN = 48, 3

# (label, streams, environment pins, expected streams per item, head replicas, skip-lane slots)
FORMS = [
    ("ns4_default", 4, {}, 1, 1, 0),
    ("ns4_mode3", 4, {"WN_V3_MODE": "3"}, 2, 2, 0),
    ("ns8_mode3_slots4", 8, {"WN_V3_MODE": "3", "WN_V3_SLOTS": "4"}, 2, 2, 4),
]


def _engine(monkeypatch, cfg, W, ns, env):
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    return engine.Engine(cfg, W, n_streams=ns)


def _lean_equals_diag(eng, first, uniforms, label):
    """The job without logits (lean instantiation) and with them (DIAG): identical indices, sampled and greedy."""
    n = uniforms.shape[1]
    lean_s = eng.generate(n, first, temperature=1.0, uniforms=uniforms, batched_prime=False, timeout_ms=8000)
    diag_s, _ = eng.generate(n, first, temperature=1.0, uniforms=uniforms, want_logits=True, batched_prime=False, timeout_ms=8000)
    assert np.array_equal(lean_s, diag_s), (label, "sampled", int(np.argmax((lean_s != diag_s).any(axis=0))))
    lean_g = eng.generate(n, first, temperature=0.0, batched_prime=False, timeout_ms=8000)
    diag_g, _ = eng.generate(n, first, temperature=0.0, want_logits=True, batched_prime=False, timeout_ms=8000)
    assert np.array_equal(lean_g, diag_g), (label, "greedy", int(np.argmax((lean_g != diag_g).any(axis=0))))
    return lean_s


@pytest.mark.parametrize("plain", [False, True], ids=["local_stores", "write_through"])
@pytest.mark.parametrize("label,ns,env,g,hr,slots", FORMS, ids=[f[0] for f in FORMS])
def test_forms_and_store_flavours(label, ns, env, g, hr, slots, plain, monkeypatch):
    env = dict(env, WN_KERNEL="v3", **({"WN_NO_LOCAL_STORES": "1"} if plain else {}))
    cfg, W, first, uniforms = make_case(LEAN4, 120, ns, N_GIVEN, N)
    eng = _engine(monkeypatch, cfg, W, ns, env)
    info = eng.info()
    assert info["kernel_variant"] == 3 and info["n_chains"] == 1, info
    assert info["streams_per_item"] == g and info["head_replicas"] == hr and info["skip_lane_slots"] == slots, info
    _lean_equals_diag(eng, first, uniforms, label)
    s = check_engine(eng, cfg, W, N, first, 1.0, 0.0, uniforms, label + " sampled")
    gr = check_engine(eng, cfg, W, N, first, 0.0, 0.0, None, label + " greedy")
    print(label, "plain" if plain else "local", s, gr)
    eng.close()


OTHER = [("cfg1_ns2_v3", "cfg1", 2, "v3", 3), ("cfg1_ns1_v4", "cfg1", 1, "v4", 4)]


@pytest.mark.parametrize("label,cfgname,ns,pin,variant", OTHER, ids=[o[0] for o in OTHER])
def test_other_kernel_paths(label, cfgname, ns, pin, variant, monkeypatch):
    """cfg1 x 2 on the wave-specialised kernel: the unsplit stack (P = 1), ONE input granule per lane in every layer; cfg1 x 1 on the stacked kernel."""
    n = 64
    cfg, W, first, uniforms = make_case(cfgname, 121, ns, N_GIVEN, n)
    eng = _engine(monkeypatch, cfg, W, ns, {"WN_KERNEL": pin})
    assert eng.info()["kernel_variant"] == variant, eng.info()
    _lean_equals_diag(eng, first, uniforms, label)
    check_engine(eng, cfg, W, n, first, 1.0, 0.0, uniforms, label + " sampled")
    check_engine(eng, cfg, W, n, first, 0.0, 0.0, None, label + " greedy")
    eng.close()


def test_profiled_job_runs_the_diag_instantiation_and_the_next_one_is_lean_again(monkeypatch):
    label, ns = "ns4_default profiled", 4
    cfg, W, first, uniforms = make_case(LEAN4, 120, ns, N_GIVEN, N)
    eng = _engine(monkeypatch, cfg, W, ns, {"WN_KERNEL": "v3"})
    info = eng.info()
    P, PA, NL, HR = info["layer_split"], info["head_split"], info["n_layers"], info["head_replicas"]
    assert info["streams_per_item"] == 1 and HR == 1, info
    plain = eng.generate(N, first, temperature=1.0, uniforms=uniforms, batched_prime=False, timeout_ms=8000)
    n_eval = N_GIVEN - 1 + N
    n_items = n_eval * ns
    eng.profile_next(n_items)
    prof = eng.generate(N, first, temperature=1.0, uniforms=uniforms, batched_prime=False, timeout_ms=8000)
    raw = eng.profile_read(n_items)
    assert np.array_equal(prof, plain), label
    n_lw, n_smp = NL * P, min(4, ns)
    assert raw.shape == (n_lw + PA * HR + n_smp, n_items, 8)
    m40 = (1 << 40) - 1
    # layer workgroups, items of evaluations >= 1 (layer 0 takes evaluation 0's input from the given samples: no "input in registers" stamp):
    # start, input in registers, barrier A, barrier B, x' published, done -- slots 0, 4, 1, 5, 2, 3, all of thread 0
    lay = raw[:n_lw, ns:, :][:, :, [0, 4, 1, 5, 2, 3]]
    assert (lay > 0).all(), label
    assert (np.diff(lay, axis=2) >= 0).all(), label
    # ... the skip group's word (slot 6: its barrier B | chunk length << 40) and the queue group's (slot 7: its barrier A | lengths)
    for k in (6, 7):
        t0 = raw[:n_lw, ns:, k] & m40
        assert (t0 > 0).all() and (t0 >= (raw[:n_lw, ns:, 0] & m40)).all(), (label, k)
    head = raw[n_lw:n_lw + PA * HR, :, :4]     # start, skip lanes staged, logits published, done
    assert (head > 0).all() and (np.diff(head, axis=2) >= 0).all(), label
    for j in range(n_smp):                     # sampler j serves the streams j mod n_smp: wait, logits complete, row published
        smp = raw[n_lw + PA * HR + j, j::n_smp, :3]
        assert (smp > 0).all() and (np.diff(smp, axis=1) >= 0).all(), (label, j)
    # the next job on the same handle, without profile_next: the lean instantiation again, same samples, still the oracle's
    again = eng.generate(N, first, temperature=1.0, uniforms=uniforms, batched_prime=False, timeout_ms=8000)
    assert np.array_equal(again, plain), label
    check_engine(eng, cfg, W, N, first, 1.0, 0.0, uniforms, label)
    eng.close()
