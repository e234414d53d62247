"""Generates tests/golden/golden_taps_train_v1.npz: one training step of the REAL reference (imported through oracle/ref_shim.py, as make_golden.py
does) for kernel_size 3 and 4 -- forward, F.cross_entropy, backward --, the fixture tests/test_gpu_taps_training.py pins the opt-in native step of
those kernel sizes to and tests/test_taps_train_host.py pins the module's own torch path to.

    python tests/golden/make_golden_taps_train.py

Stored per case (taps_train_k3, taps_train_k4), in the form of the training fixtures of make_golden.py: grad_<case>_meta = (weight seed, N,
output_length, L, receptive field, kernel_size, bias), grad_<case>_ids (N, L) int16 class indices, grad_<case>_target (N * output_length,) int16,
grad_<case>_out (N * output_length, 256) float32 logits, grad_<case>_loss (1,) float64, grad_<case>_d_<parameter name>: the gradient's digest
(tests/golden/digest.py).  Weights are not stored: mi355_wavenet.synth.init_weights(cfg, seed) is bit-stable; the data seed is the weight seed + 1.
Stack: 3 layers x 2 blocks, 32 / 32 / 64 / 64 channels, N = 2, output_length 16, clips of receptive_field + output_length - 1 + 5 samples."""
import os
import sys

import numpy as np
import torch
import torch.nn.functional as F

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.join(ROOT, "oracle"))
sys.path.insert(0, os.path.join(ROOT, "pytorch-wavenet_amd"))

import digest as dg  # noqa: E402
import ref_shim  # noqa: E402
from mi355_wavenet import synth  # noqa: E402

BASE = dict(layers=3, blocks=2, dilation_channels=32, residual_channels=32, skip_channels=64, end_channels=64, classes=256)
# case -> (kernel_size, bias, weight seed, N, output_length, samples beyond receptive_field + output_length - 1)
CASES = {"taps_train_k3": (3, True, 401, 2, 16, 5), "taps_train_k4": (4, False, 402, 2, 16, 5)}


def case_config(k, bias):
    return dict(BASE, kernel_size=k, bias=bias)


def main():
    mdl, _, _ = ref_shim.load()
    out = {}
    for case, (k, bias, wseed, N, out_len, extra) in CASES.items():
        cfg = case_config(k, bias)
        m = mdl.WaveNetModel(output_length=out_len, **cfg)
        m.load_state_dict({key: torch.from_numpy(v) for key, v in synth.init_weights(cfg, seed=wseed).items()})
        L = m.receptive_field + out_len - 1 + extra
        assert m.receptive_field == synth.receptive_field(cfg)
        rs = np.random.RandomState(wseed + 1)
        ids = rs.randint(0, 256, (N, L))
        target = rs.randint(0, 256, (N * out_len,))
        x = torch.zeros(N, 256, L).scatter_(1, torch.from_numpy(ids).view(N, 1, L), 1.)
        y = m(x)                                                      # wavenet_model.py:186-196
        loss = F.cross_entropy(y.squeeze(), torch.from_numpy(target))  # wavenet_training.py:69
        loss.backward()
        out["grad_%s_ids" % case] = ids.astype(np.int16)
        out["grad_%s_target" % case] = target.astype(np.int16)
        out["grad_%s_out" % case] = y.detach().numpy().astype(np.float32)
        out["grad_%s_loss" % case] = np.array([float(loss)], dtype=np.float64)
        out["grad_%s_meta" % case] = np.array([wseed, N, out_len, L, m.receptive_field, k, int(bias)], dtype=np.int64)
        named = {key: (p.grad.numpy() if p.grad is not None else np.zeros(tuple(p.shape), dtype=np.float32)) for key, p in m.named_parameters()}
        for key, v in dg.digest(named).items():
            out["grad_%s_d_%s" % (case, key)] = v
        print(case, "L", L, "rf", m.receptive_field, "loss", float(loss), "params", len(named), "|logits|max", float(y.abs().max()))
    path = os.path.join(HERE, "golden_taps_train_v1.npz")
    np.savez_compressed(path, **out)
    print("wrote", path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
