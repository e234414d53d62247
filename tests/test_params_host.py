"""CPU: mi355_wavenet/params.py -- the one table of the model's 14 parameter arrays -- held to what it was NOT derived from: a real module's
state_dict, the literal argument order of training.StackFunction, the struct orders of _abi.py, the module's own nn.Parameter objects, and the
weights synth.init_weights produced before the table existed."""
import hashlib

import numpy as np
import pytest
import torch

import wavenet_model
from mi355_wavenet import _abi, params, synth, training

# The argument order of training.StackFunction (what training.PARAM_ORDER was as a literal before params.py): written out, not imported.
TRAVELLING_ORDER = ("start_w", "filter_w", "gate_w", "res_w", "skip_w", "end1_w", "end1_b", "end2_w", "end2_b",
                    "start_b", "filter_b", "gate_b", "res_b", "skip_b")


def model(bias, kernel_size=2, channels=(32, 32, 64, 64)):
    R, D, S, E = channels
    return wavenet_model.WaveNetModel(layers=2, blocks=2, dilation_channels=D, residual_channels=R, skip_channels=S, end_channels=E,
                                      classes=256, kernel_size=kernel_size, bias=bias)


@pytest.mark.parametrize("kernel_size", [2, 3])
@pytest.mark.parametrize("bias", [False, True])
def test_names_shapes_and_registration_order_are_a_state_dicts(bias, kernel_size):
    m = model(bias, kernel_size)
    want = [(n, tuple(t.shape)) for n, t in m.state_dict().items()]
    cfg = m._config()
    assert [(n, params.shape(k, cfg)) for n, k in params.entries(cfg)] == want
    assert list(synth.param_shapes(cfg).items()) == want
    # key -> name, a few written out (the table's module column against the reference's attribute names)
    assert params.name("filter_w", 1) == "filter_convs.1.weight" and params.name("gate_w", 0) == "gate_convs.0.weight"
    assert params.name("res_b", 3) == "residual_convs.3.bias" and params.name("skip_w", 2) == "skip_convs.2.weight"
    assert params.name("start_w") == "start_conv.weight" and params.name("end1_b") == "end_conv_1.bias" and params.name("end2_w") == "end_conv_2.weight"


def test_key_order_is_the_argument_order_of_the_stack_function():
    assert params.order(True) == TRAVELLING_ORDER == training.PARAM_ORDER
    assert params.order(False) == tuple(k for k in TRAVELLING_ORDER if k.endswith("_w") or k in ("end1_b", "end2_b"))
    assert set(training.SINGLE_KEYS) == {"start_w", "start_b", "end1_w", "end1_b", "end2_w", "end2_b"}


def test_keys_and_per_layerness_equal_the_abi_structs():
    keys = {p.key for p in params.TABLE}
    assert len(params.TABLE) == 14 == len(keys)
    assert keys == set(_abi.WEIGHT_FIELDS) and len(_abi.WEIGHT_FIELDS) == 14
    assert keys == set(_abi.TRAIN_TENSOR_ARRAYS + _abi.TRAIN_TENSOR_SINGLES) and len(_abi.TRAIN_TENSOR_ARRAYS + _abi.TRAIN_TENSOR_SINGLES) == 14
    assert {p.key for p in params.TABLE if p.per_layer} == set(_abi.TRAIN_TENSOR_ARRAYS)
    assert {p.key for p in params.TABLE if not p.per_layer} == set(_abi.TRAIN_TENSOR_SINGLES)


@pytest.mark.parametrize("bias", [False, True])
def test_from_module_returns_the_parameters_themselves(bias):
    m = model(bias)
    NL = m.layers * m.blocks
    named = dict(m.named_parameters())
    by_key = params.from_module(m)
    assert tuple(by_key) == params.order(bias)
    for key, ts in by_key.items():
        per_layer = key in _abi.TRAIN_TENSOR_ARRAYS
        assert len(ts) == (NL if per_layer else 1), key
        for i, t in enumerate(ts):
            assert isinstance(t, torch.nn.Parameter) and t is named[params.name(key, i if per_layer else None)], (key, i)
    assert sum(len(ts) for ts in by_key.values()) == len(named)
    # ... and the stacked arrays (by name) are the same parameters' values, in layer order
    st = params.stacked(m.state_dict(), m._config())
    assert tuple(st) == params.order(bias)
    for key, ts in by_key.items():
        want = np.stack([t.detach().numpy() for t in ts]) if key in _abi.TRAIN_TENSOR_ARRAYS else ts[0].detach().numpy()
        assert st[key].dtype == np.float32 and st[key].flags["C_CONTIGUOUS"] and np.array_equal(st[key], want), key


@pytest.mark.parametrize("bias", [False, True])
def test_padding_fills_the_leading_block_and_zeros_elsewhere(bias):
    m = model(bias, channels=(48, 40, 300, 200))
    sd = {n: t.numpy() for n, t in m.state_dict().items()}
    same = params.padded(sd, m._config())
    assert list(same) == list(sd) and all(np.array_equal(same[n], sd[n]) and same[n].dtype == np.float32 for n in sd)   # the identity
    big = dict(m._config(), residual_channels=64, dilation_channels=64, skip_channels=320, end_channels=256)
    pad = params.padded(m.state_dict(), big)   # (torch tensors in: numpy out)
    assert [(n, a.shape) for n, a in pad.items()] == list(synth.param_shapes(big).items())
    for n, a in pad.items():
        block = tuple(slice(0, s) for s in sd[n].shape)
        assert np.array_equal(a[block], sd[n]), n
        rest = a.copy()
        rest[block] = 0
        assert not rest.any(), n
        assert (a.size > sd[n].size) == (n != "end_conv_2.bias"), n   # (only the class count is not padded)


def test_init_weights_is_bit_stable():
    """SHA-256 over (name, bytes) of every array in key order.  The expected values were recorded by running synth.init_weights of the commit
    before params.py existed (synth.param_shapes then spelled the names and shapes out in four loops); the golden fixtures under tests/golden
    depend on this consumption order of the seeded RNG."""
    want = {("cfg1", 7): "9fad6ea7834fe09398bb8be453435a75c3b4387b7f856899d0cad0231194a5be",
            ("tiny_bias", 5): "647f395437fadb00be9fda0df8497ad50981f290b61b5ea14c6fdab2dd3cf438"}
    for (name, seed), digest in want.items():
        h = hashlib.sha256()
        for n, a in synth.init_weights(synth.CONFIGS[name], seed=seed).items():
            h.update(n.encode())
            h.update(a.tobytes())
        assert h.hexdigest() == digest, (name, seed)
