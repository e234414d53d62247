"""Generates tests/golden/golden_taps_v1.npz: forward() of the REAL reference (imported through oracle/ref_shim.py, as make_golden.py does) for
kernel_size 3 and 4 -- the fixture tests/test_gpu_taps.py pins the matrix-core inference path of those kernel sizes to.

    python tests/golden/make_golden_taps.py

Stored per case (taps_k3, taps_k4): <case>_meta = (weight seed, N, output_length, L, kernel_size, bias), <case>_ids (N, L) int16 class indices,
<case>_out (N * output_length, 256) float32 logits.  Weights are not stored: mi355_wavenet.synth.init_weights(cfg, seed) is bit-stable.
Stack: 3 layers x 2 blocks, 32 / 32 / 64 / 64 channels, N = 2, clips of receptive_field + output_length - 1 + 5 samples."""
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, os.path.join(ROOT, "oracle"))
sys.path.insert(0, os.path.join(ROOT, "pytorch-wavenet_amd"))

import ref_shim  # noqa: E402
from mi355_wavenet import synth  # noqa: E402

BASE = dict(layers=3, blocks=2, dilation_channels=32, residual_channels=32, skip_channels=64, end_channels=64, classes=256)
# case -> (kernel_size, bias, weight seed, data seed, N, output_length, samples beyond receptive_field + output_length - 1)
CASES = {"taps_k3": (3, True, 301, 311, 2, 6, 5), "taps_k4": (4, False, 302, 312, 2, 6, 5)}
GAIN = 1.0   # (as every golden forward fixture: the bar of tests/test_gpu_forward.py on them is an ABSOLUTE 1e-4, sized for logits of order 1)


def case_config(k, bias):
    return dict(BASE, kernel_size=k, bias=bias)


def main():
    mdl, _, _ = ref_shim.load()
    out = {}
    for name, (k, bias, wseed, dseed, N, out_len, extra) in CASES.items():
        cfg = case_config(k, bias)
        m = mdl.WaveNetModel(output_length=out_len, **cfg)
        W = synth.init_weights(cfg, seed=wseed, gain=GAIN)
        m.load_state_dict({key: torch.from_numpy(v) for key, v in W.items()})
        L = m.receptive_field + out_len - 1 + extra
        assert m.receptive_field == synth.receptive_field(cfg)
        ids = np.random.RandomState(dseed).randint(0, 256, (N, L))
        x = torch.zeros(N, 256, L).scatter_(1, torch.from_numpy(ids).view(N, 1, L), 1.)
        with torch.no_grad():
            y = m(x).numpy()
        assert y.shape == (N * out_len, 256) and y.dtype == np.float32
        out[name + "_meta"] = np.array([wseed, N, out_len, L, k, int(bias)], dtype=np.int64)
        out[name + "_ids"] = ids.astype(np.int16)
        out[name + "_out"] = y
        print(name, "L", L, "receptive field", m.receptive_field, "|logits|max", float(np.abs(y).max()))
    path = os.path.join(HERE, "golden_taps_v1.npz")
    np.savez_compressed(path, **out)
    print("wrote", path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
