"""-m gpu: the layer role's input poll with the LDS store of x inside the hand-scheduled blocks (csrc/wn_kernel_v3.h: wn_ap_*_stage,
wn_v3_fetch_input).

A polling wave's block stores the lane's input sum at its served exit -- the tail of a successful first look, label 2 of a spin -- and the C++
side stores only where no poll runs (layer 0's first evaluation, a given sample).  What can go wrong is therefore per form of the block
(P = 1, 2, 4 partials), per exit (first look fresh / stale), per lane mask (a partly filled polling wave) and per streams-per-item form
(G = 1, 2: with two streams all four critical waves poll, waves 0-1 for stream a and 2-3 for stream b); the cases below walk those.

Shape: cfg3's channels on layers=4, blocks=1 (a first, a middle and a last layer; queues wrap inside 48 samples), as tests/test_gpu_lean_kernels.py.
Every case holds the indices against the C oracle, sampled and greedy, and the lean instantiation against the DIAG one.  WN_TESTING=1
(tests/conftest.py) lets the pins through.  No case provokes a timeout: the bounded wait's give-up is not exercised here."""
import numpy as np
import pytest

from mi355_wavenet import engine, synth
from parity_common import check_engine, make_case

pytestmark = pytest.mark.gpu

LEAN4 = dict(synth.CONFIGS["cfg3"], layers=4, blocks=1)
N, N_GIVEN = 48, 3


def _engine(monkeypatch, cfg, W, ns, env):
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    return engine.Engine(cfg, W, n_streams=ns)


def _generate(eng, n, first, temperature, uniforms, **kw):
    return eng.generate(n, first, temperature=temperature, uniforms=uniforms, batched_prime=False, timeout_ms=8000, **kw)


def _check(eng, cfg, W, n, first, uniforms, label):
    """lean == DIAG (sampled and greedy), then the DIAG job against the oracle (indices and logits)."""
    for temp, u, what in ((1.0, uniforms, "sampled"), (0.0, None, "greedy")):
        lean = _generate(eng, n, first, temp, u)
        diag, _ = _generate(eng, n, first, temp, u, want_logits=True)
        assert np.array_equal(lean, diag), (label, what, int(np.argmax((lean != diag).any(axis=0))))
        check_engine(eng, cfg, W, n, first, temp, 0.0, u, "%s %s" % (label, what))


# (label, streams, pins, streams per item)
FORMS = [
    ("p4_g1_ns4", 4, {}, 1),
    ("p4_g2_ns4", 4, {"WN_V3_MODE": "3"}, 2),
    ("p4_g2_ns8", 8, {"WN_V3_MODE": "3", "WN_V3_SLOTS": "0"}, 2),   # (a stack this short would take the slot re-use form at 8 streams: it keeps the C++ store)
]


@pytest.mark.parametrize("plain", [False, True], ids=["local_stores", "write_through"])
@pytest.mark.parametrize("label,ns,env,g", FORMS, ids=[f[0] for f in FORMS])
def test_four_partials_both_item_forms_both_store_flavours(label, ns, env, g, plain, monkeypatch):
    """P = 4.  Write-through publications become visible later than L2-resident ones, so the consumer's first look is stale more often and the
    spin's exit stores; with L2-resident stores and tokens queued (8 streams) the look's tail does."""
    env = dict(env, WN_KERNEL="v3", **({"WN_NO_LOCAL_STORES": "1"} if plain else {}))
    cfg, W, first, uniforms = make_case(LEAN4, 170, ns, N_GIVEN, N)
    eng = _engine(monkeypatch, cfg, W, ns, env)
    info = eng.info()
    assert info["kernel_variant"] == 3 and info["layer_split"] == 4 and info["streams_per_item"] == g and info["skip_lane_slots"] == 0, info
    _check(eng, cfg, W, N, first, uniforms, label)
    eng.close()


def test_one_granule_per_lane_and_a_partly_filled_poll_wave(monkeypatch):
    """cfg1 (R = 32) x 2 on the wave-specialised kernel: P = 1, and 32 polling lanes in a wave of 64 -- the block's store runs under the lane mask."""
    n = 64
    cfg, W, first, uniforms = make_case("cfg1", 171, 2, N_GIVEN, n)
    eng = _engine(monkeypatch, cfg, W, 2, {"WN_KERNEL": "v3"})
    info = eng.info()
    assert info["kernel_variant"] == 3 and info["layer_split"] == 1 and info["streams_per_item"] == 1, info
    _check(eng, cfg, W, n, first, uniforms, "cfg1_ns2_v3")
    eng.close()


def test_two_partials(monkeypatch):
    """The train_script.py channel shape (32 / 32 / 1024 / 512, bias), split two ways: P = 2."""
    small = dict(synth.CONFIGS["chaconne"], layers=4, blocks=1)
    cfg, W, first, uniforms = make_case(small, 172, 2, N_GIVEN, N)
    eng = _engine(monkeypatch, cfg, W, 2, {"WN_KERNEL": "v3"})
    info = eng.info()
    assert info["kernel_variant"] == 3 and info["layer_split"] == 2, info
    _check(eng, cfg, W, N, first, uniforms, "chaconne4_ns2_v3")
    eng.close()


@pytest.mark.parametrize("n_given", [1, 3])
def test_given_input_next_to_the_first_polled_evaluation(n_given, monkeypatch):
    """Layer 0 stages evaluation 0 in C++ (the given sample's start_conv row) and evaluation 1 from the poll block, into the two x buffers.
    n_given = 1: evaluation 1's input is already a sampled one; n_given = 3: two more primed evaluations first."""
    ns = 4
    cfg, W, first, uniforms = make_case(LEAN4, 173, ns, n_given, N)
    eng = _engine(monkeypatch, cfg, W, ns, {"WN_KERNEL": "v3"})
    assert eng.info()["kernel_variant"] == 3, eng.info()
    _check(eng, cfg, W, N, first, uniforms, "n_given=%d" % n_given)
    eng.close()


def test_first_job_of_a_fresh_handle_equals_its_repeat(monkeypatch):
    """One stream, straight after engine creation: the ring is slow (nothing queued, cold caches and clocks), spins run long and the bounded wait's
    first iterations can run.  The same job again must return the same samples, and both are the oracle's."""
    cfg, W, first, uniforms = make_case(LEAN4, 174, 1, N_GIVEN, N)
    eng = _engine(monkeypatch, cfg, W, 1, {"WN_KERNEL": "v3"})
    assert eng.info()["kernel_variant"] == 3, eng.info()
    cold = _generate(eng, N, first, 1.0, uniforms)
    again = _generate(eng, N, first, 1.0, uniforms)
    assert np.array_equal(cold, again)
    _check(eng, cfg, W, N, first, uniforms, "fresh_handle_ns1")
    eng.close()
