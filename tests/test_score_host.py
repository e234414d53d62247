"""Host logic of teacher-forced scoring: wn_score's argument errors (codes before any HIP call, as tests/test_abi.py checks the other entry points), the
binding's handling of a library that lacks the symbol (the unchanged test double), and the trainer's keyword."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

from mi355_wavenet import _abi, engine, synth

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_wn_score_is_declared_bound_and_optional():
    hdr = open(os.path.join(ROOT, "include", "wn_abi.h")).read()
    assert re.search(r"\bint wn_score\(wn_handle\* h, const int32_t\* indices, const int64_t\* targets,", hdr)
    assert "wn_score" in _abi.EXPORTS and "wn_score" in _abi.OPTIONAL_EXPORTS
    assert "#define WN_ABI_VERSION 5" in hdr and _abi.ABI_VERSION == 5


def test_the_binding_loads_the_unchanged_double_and_engine_score_says_what_is_missing():
    from double_lib import double_backend, double_library
    lib = double_library()
    assert not lib.has("wn_score") and lib.has("wn_forward") and lib.missing == ("wn_score",)
    assert "wn_score" not in open(os.path.join(ROOT, "tests", "double", "wn_abi_double.cpp")).read()
    cfg = synth.CONFIGS["tiny"] if "tiny" in synth.CONFIGS else synth.CONFIGS["cfg1"]
    eng = engine.Engine(cfg, synth.init_weights(cfg, seed=1), **double_backend())
    with pytest.raises(RuntimeError, match="does not export wn_score"):
        eng.score(np.zeros((1, 8), dtype=np.int32), np.zeros(4, dtype=np.int64), 4)
    eng.close()


def test_a_library_missing_a_required_symbol_is_still_refused(monkeypatch):
    from double_lib import double_library
    monkeypatch.setattr(_abi, "EXPORTS", _abi.EXPORTS + ["wn_no_such_function"])
    with pytest.raises(RuntimeError, match="does not export wn_no_such_function"):
        _abi.Library(double_library().path)


def test_argument_errors_come_before_any_hip_call():
    """NULL arguments and a handle without weights are refused on the host: no device is needed (the product library loads without one)."""
    import sys
    sys.path.insert(0, os.path.join(ROOT, "pytorch-wavenet_amd"))
    import build
    lib = _abi.Library(build.build_hip())
    assert lib.has("wn_score") and lib.missing == ()
    d = lib.dll
    buf = (ctypes.c_char * 64)()
    p = ctypes.addressof(buf)
    assert d.wn_score(None, p, p, 1, 8, 4, None, None, p, None) == _abi.WN_E_BADARG
    assert "wn_score: NULL argument" in lib.last_error()
    h = ctypes.c_void_p(p)   # (never dereferenced: the NULL checks come first)
    assert d.wn_score(h, None, p, 1, 8, 4, None, None, p, None) == _abi.WN_E_BADARG
    assert d.wn_score(h, p, None, 1, 8, 4, None, None, p, None) == _abi.WN_E_BADARG
    assert d.wn_score(h, p, p, 1, 8, 4, p, p, None, None) == _abi.WN_E_BADARG


def test_native_validation_is_off_by_default_and_off_means_the_torch_ops(monkeypatch):
    import inspect
    import wavenet_model
    import wavenet_training
    sig = inspect.signature(wavenet_training.WavenetTrainer.__init__)
    assert sig.parameters["native_validation"].default is False

    class Data:   # the slice of the dataset's interface validate() touches
        train = True
        def __len__(self):
            return 3

    m = wavenet_model.WaveNetModel(layers=2, blocks=1, dilation_channels=8, residual_channels=8, skip_channels=8, end_channels=8, output_length=4)
    called = []
    monkeypatch.setattr(wavenet_model.WaveNetModel, "score_indices", lambda self, *a, **k: called.append(1))
    g = torch.Generator().manual_seed(0)
    batches = [(torch.randint(0, 256, (2, m.receptive_field + 3), generator=g), torch.randint(0, 256, (8,), generator=g)) for _ in range(2)]

    def epoch(self, batch_size, shuffle):
        for idx, tgt in batches:   # CPU batches: one-hot through the module's torch path, the reference's route
            yield "onehot", torch.nn.functional.one_hot(idx, 256).permute(0, 2, 1).float(), tgt

    monkeypatch.setattr(wavenet_training.WavenetTrainer, "_epoch", epoch)
    monkeypatch.setattr(wavenet_training.WavenetTrainer, "_loader", lambda self, bs, train: (None, None))
    tr = wavenet_training.WavenetTrainer(m, Data())
    loss, acc = tr.validate()
    # the reference's arithmetic on the same batches
    want_loss, hits = 0.0, 0
    with torch.no_grad():
        for idx, tgt in batches:
            out = m(torch.nn.functional.one_hot(idx, 256).permute(0, 2, 1).float())
            want_loss += torch.nn.functional.cross_entropy(out, tgt).item()
            hits += int((out.max(1)[1] == tgt).sum())
    assert not called and loss == want_loss / 2 and acc == hits / 16
    # on, but the batches are not class indices: still the torch ops
    tr2 = wavenet_training.WavenetTrainer(m, Data(), native_validation=True)
    assert tr2.validate() == (loss, acc) and not called
