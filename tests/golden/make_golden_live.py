"""Generates tests/golden/golden_v7.npz with the REAL reference (authoring container only): what four tests used to ask the live reference
tree, recorded once so that the suite runs from the repository alone.

  live_sampled_audio          tiny model, weights seed 31, 25 given samples, generate_fast(150, temperature=0.9, regularize=0.003) after
                              np.random.seed(7)                                       (tests/test_oracle_pinning.py)
  geom_<layers>_<blocks>_<out_len>_<N>
                              for every clip length L = 2 .. receptive_field + out_len + 2 (index L - 2): 1 where the reference's forward()
                              returns (N * output_length, classes) logits for an all-zero-class clip, 0 where it raises or returns another
                              shape                                                   (tests/test_plan_host.py)
  ds_s<k>_<train|test>_*      the reference's WavenetDataset on make_golden_dataset.files(), EVERY item: len, start_samples, the class of
                              every one-hot column (x) and the target (t)             (tests/test_training_host.py)
  mulaw_x, mulaw_quantized, mulaw_expanded
                              the reference's quantize_data(x, 256) (int64 classes) and mu_law_expansion(x, 256) of
                              x = RandomState(0).uniform(-1, 1, 1000)                 (tests/test_training_host.py)
  loop_losses, loop_<param>   three optimiser steps of the reference's training loop body on its own WaveNetModel (the tiny model of
                              tests/test_training_host.py, torch.manual_seed(0) init, DataLoader shuffled under torch.manual_seed(11)):
                              the losses and the parameters after the third step     (tests/test_training_host.py)

    python tests/golden/make_golden_live.py
"""
import os
import sys
import tempfile

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
for p in (os.path.join(ROOT, "oracle"), os.path.join(ROOT, "pytorch-wavenet_amd"), HERE):
    if p not in sys.path:
        sys.path.insert(0, p)

GEOMETRY_CASES = ((3, 2, 4, 2), (4, 2, 3, 1), (5, 1, 6, 3))   # (layers, blocks, output_length, N)
LOOP = {"lr": 0.01, "clip": 1.0, "batch": 4, "steps": 3, "seed": 11, "out_len": 8, "test_stride": 5}


def sampled(mdl, out):
    from mi355_wavenet import synth
    cfg = synth.CONFIGS["tiny"]
    W = synth.init_weights(cfg, seed=31)
    m = mdl.WaveNetModel(output_length=4, **cfg)
    m.load_state_dict({k: torch.from_numpy(v) for k, v in W.items()})
    first = torch.from_numpy(np.random.RandomState(31).randint(0, 256, 25))
    np.random.seed(7)
    out["live_sampled_audio"] = np.asarray(m.generate_fast(150, first_samples=first, temperature=0.9, regularize=0.003), dtype=np.float64)


def geometry(mdl, out):
    for layers, blocks, out_len, N in GEOMETRY_CASES:
        m = mdl.WaveNetModel(layers=layers, blocks=blocks, dilation_channels=4, residual_channels=4, skip_channels=8, end_channels=8,
                             classes=16, output_length=out_len)
        ok = []
        for L in range(2, m.receptive_field + out_len + 3):
            x = torch.zeros(N, 16, L)
            x[:, 0, :] = 1.
            try:
                with torch.no_grad():
                    y = m(x)
                ok.append(tuple(y.shape) == (N * out_len, 16))
            except Exception:   # noqa: BLE001 -- whatever the reference raises there
                ok.append(False)
        out["geom_%d_%d_%d_%d" % (layers, blocks, out_len, N)] = np.asarray(ok, dtype=np.int8)


def dataset(ad, path, out):
    from make_golden_dataset import SETTINGS
    for k, (il, tl, stride) in enumerate(SETTINGS):
        for train in (True, False):
            ds = ad.WavenetDataset(path, item_length=il, target_length=tl, train=train, test_stride=stride)
            tag = "ds_s%d_%s" % (k, "train" if train else "test")
            xs, ts = [], []
            for i in range(len(ds)):
                one_hot, target = ds[i]
                x = one_hot.argmax(0)
                assert one_hot.dtype == torch.float32 and torch.equal(one_hot, torch.nn.functional.one_hot(x, 256).t().float())
                assert target.dtype == torch.int64 and tuple(target.shape) == (1, tl)
                xs.append(x.numpy())
                ts.append(target.numpy().reshape(-1))
            out[tag + "_len"] = np.int64(len(ds))
            out[tag + "_start"] = np.asarray(ds.start_samples, dtype=np.int64)
            out[tag + "_x"] = np.asarray(xs, dtype=np.int16).reshape(len(ds), il)
            out[tag + "_t"] = np.asarray(ts, dtype=np.int16).reshape(len(ds), tl)


def mu_law(ad, out):
    x = np.random.RandomState(0).uniform(-1, 1, 1000)
    out["mulaw_x"] = x
    out["mulaw_quantized"] = np.asarray(ad.quantize_data(x, 256), dtype=np.int64)
    out["mulaw_expanded"] = np.asarray(ad.mu_law_expansion(x, 256), dtype=np.float64)


def reference_loop(model, ds, lr, clip, batch, steps, seed):
    """The reference's loop body (wavenet_training.py:64-77, its two legacy `.data[0]` reads dropped): (losses, model after `steps` steps)."""
    opt = torch.optim.Adam(params=model.parameters(), lr=lr, weight_decay=0)
    model.train()
    torch.manual_seed(seed)
    loader = torch.utils.data.DataLoader(ds, batch_size=batch, shuffle=True, num_workers=0, pin_memory=False)
    losses = []
    for step, (x, target) in enumerate(iter(loader), 1):
        x = x.type(torch.FloatTensor)
        target = target.view(-1).type(torch.LongTensor)
        output = model(x)
        loss = torch.nn.functional.cross_entropy(output.squeeze(), target.squeeze())
        opt.zero_grad()
        loss.backward()
        torch.nn.utils.clip_grad_norm_(model.parameters(), clip)
        opt.step()
        losses.append(loss.item())
        if step == steps:
            break
    return losses


def loop(mdl, ad, path, out):
    torch.manual_seed(0)
    ref = mdl.WaveNetModel(layers=3, blocks=2, dilation_channels=8, residual_channels=8, skip_channels=16, end_channels=16,
                           classes=256, output_length=LOOP["out_len"], kernel_size=2, bias=True)
    import wavenet_model
    torch.manual_seed(0)   # the same init the test's _tiny_model() draws
    twin = wavenet_model.WaveNetModel(layers=3, blocks=2, dilation_channels=8, residual_channels=8, skip_channels=16, end_channels=16,
                                      classes=256, output_length=LOOP["out_len"], kernel_size=2, bias=True)
    ref.load_state_dict(twin.state_dict())
    il = ref.receptive_field + ref.output_length - 1
    rds = ad.WavenetDataset(path, item_length=il, target_length=LOOP["out_len"], test_stride=LOOP["test_stride"])
    losses = reference_loop(ref, rds, LOOP["lr"], LOOP["clip"], LOOP["batch"], LOOP["steps"], LOOP["seed"])
    out["loop_losses"] = np.asarray(losses, dtype=np.float64)
    for k, v in ref.state_dict().items():
        out["loop_" + k] = v.detach().numpy().copy()


def main():
    import ref_shim
    from make_golden_dataset import files
    mdl, _, ad = ref_shim.load()
    out = {}
    sampled(mdl, out)
    geometry(mdl, out)
    with tempfile.TemporaryDirectory() as tmp:
        path = os.path.join(tmp, "ds.npz")
        np.savez(path, *files())
        dataset(ad, path, out)
        mu_law(ad, out)
        loop(mdl, ad, path, out)
    np.savez_compressed(os.path.join(HERE, "golden_v7.npz"), **out)
    print("wrote", len(out), "arrays")


if __name__ == "__main__":
    main()
