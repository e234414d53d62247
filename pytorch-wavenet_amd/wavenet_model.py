"""Drop-in for the reference's ``wavenet_model`` module: ``WaveNetModel``, ``load_latest_model_from``,
``load_to_cpu`` -- same constructor, parameter names, attributes and method signatures
(/root/reference/wavenet_model.py:8-346), so ``from wavenet_model import *`` callers, reference
``state_dict``s and pickled snapshots keep working.

What is different underneath:
  * ``generate_fast()`` does not run the Python per-sample loop.  It hands the whole job to the MI355X
    engine (mi355_wavenet.engine -> C ABI include/wn_abi.h -> HIP kernels csrc/wn_kernel_v3.h / wn_kernel.h): one persistent
    kernel launch per call (per progress interval when a callback is given).  Where the job is cut into such pieces, and what runs between
    them (callbacks, the timing print, the draws), is decided by mi355_wavenet/generation.py: generation_schedule plans, pure; run_schedule
    executes.  generate_fast, generate_fast_streams and score_continuation share one prologue and one epilogue (see _finish).  There is NO CPU
    fallback: without a gfx950 GPU and the built library it raises.
  * the global numpy RNG is consumed exactly as the reference does (one ``random_sample`` per generated
    sample when ``temperature > 0``: ``np.random.choice``, wavenet_model.py:288) -- the draws are made on the
    host and shipped to the kernel, which performs the same float64 inverse-CDF lookup.
  * extension: ``first_samples`` may be 2-D ``(streams, n_given)``; the result is then ``(streams, num_samples)``.
  * the priming window (``first_samples`` of length n > 64) is evaluated as one batched matrix-core pass (wn_prime).
  * ``forward()`` on a CUDA one-hot batch runs natively on the matrix cores (wn_forward; wn_train_forward / wn_train_backward
    behind a torch.autograd.Function when gradients are wanted) -- including clips shorter than receptive_field +
    output_length - 1, where the reference left-pads the layers' activations with zeros (wavenet_modules.py:24-27: per-layer row
    windows in the kernels).  The reference's algorithm with torch ops remains for: CPU tensors, inputs that are not one-hot,
    gradients w.r.t. the input, kernel_size != 2 (kernel_size 3 and 4 run natively where ``native_taps_training`` is switched on: see the class), a class count that is not a multiple of 32 under autograd (channel counts that are not
    multiples of 32 run natively, zero-padded: with and, since round 6, under autograd), and the input lengths for which the reference itself has no defined result (its error, or its shapes, are reproduced).
"""
import collections
import contextlib
import itertools
import os
import os.path
import time

from wavenet_modules import *  # noqa: F401,F403  (the reference re-exports these names, wavenet_model.py:4)
from audio_data import *  # noqa: F401,F403       (and these, :5)

import numpy as np
import torch
import torch.nn as nn
import torch.nn.functional as F

# What WaveNetModel.score_indices returns: device tensors (see there).
ScoreResult = collections.namedtuple("ScoreResult", ["loss", "accuracy", "n", "row_nll", "pred", "sums"])


def _wn_defaults():
    """What a module carries besides the reference's attributes: set by __init__, and by __setstate__ where a snapshot lacks them."""
    return {
        "_wn_engine": None, "_wn_engine_key": None, "_wn_train_runner": None,
        "_wn_forward_calls": 0, "_wn_train_calls": 0, "_wn_fallbacks": {},     # wn_stats()
        "_wn_forward_unsupported": None,   # the _forward_shape_key() this device's library has no native forward for
        "_wn_expansion": None,             # (classes, table) of _expand_indices
        # Extension: operand precision of the native matrix-core forward / backward GEMMs: "fp32" (default: equals the
        # reference's fp32 graph to rounding) or "bf16" (bf16 operands, fp32 accumulation and fp32 residual stream;
        # needs channel counts that are multiples of 64, otherwise fp32 is used)
        "matrix_precision": "fp32",
        # Extension: True = the native backward's weight / bias gradients are bit-reproducible from run to run (ordered reduction of the row splits'
        # partial tiles instead of fp32 atomics: C ABI wn_train_set_deterministic); None = the library's default (off, or WN_DETERMINISTIC=1)
        "deterministic_gradients": None,
    }


class WaveNetModel(nn.Module):
    """
    A Complete Wavenet Model (constructor arguments as in the reference, wavenet_model.py:28-39)

    Args:
        layers (Int):               Number of layers in each block
        blocks (Int):               Number of wavenet blocks of this model
        dilation_channels (Int):    Number of channels for the dilated convolution
        residual_channels (Int):    Number of channels for the residual connection
        skip_channels (Int):        Number of channels for the skip connections
        end_channels (Int):         Number of channels of the penultimate 1x1 convolution
        classes (Int):              Number of possible values each sample can have
        output_length (Int):        Number of samples that are generated for each input
        kernel_size (Int):          Size of the dilation kernel
        dtype:                      Parameter type of this model (legacy tensor type object or torch.dtype)
        bias (Bool):                Whether the stack convolutions carry a bias
    """

    # Extension, opt-in: True = forward() on a one-hot CUDA tensor and train_forward_indices() of a kernel_size 3 or 4 model whose channel counts and
    # class count are multiples of 32 run on the matrix cores too (fp32: wn_forward without autograd, wn_train_forward / wn_train_backward with it)
    # instead of the torch path.  A CLASS attribute, so that reference pickles and snapshots written before it existed load unchanged; set it on the
    # class or on an instance (an instance's value travels with its pickle).  False: every path, message and warning is as before.
    native_taps_training = False

    # Extension, opt-in: True = with matrix_precision "bf16", forward_indices() / score_indices() (and so the trainer's native validation) of a
    # kernel_size 3 or 4 model whose channel counts are multiples of 64 run on bf16 matrix operands (C ABI wn_set_forward_precision,
    # WN_PRECISION_BF16_TAPS).  Inference only: priming, generate_fast() and the native_taps_training step stay fp32.  A class attribute like
    # native_taps_training.  False: matrix_precision is ignored for such a model, as before.
    native_taps_bf16 = False

    def __init__(self, layers=10, blocks=4, dilation_channels=32, residual_channels=32, skip_channels=256,
                 end_channels=256, classes=256, output_length=32, kernel_size=2, dtype=torch.FloatTensor, bias=False):
        super(WaveNetModel, self).__init__()
        self.layers = layers
        self.blocks = blocks
        self.dilation_channels = dilation_channels
        self.residual_channels = residual_channels
        self.skip_channels = skip_channels
        self.end_channels = end_channels
        self.classes = classes
        self.kernel_size = kernel_size
        self.dtype = dtype
        self.bias = bias

        self.dilations = []        # (dilation, previous dilation) per layer  (wavenet_model.py:75)
        self.dilated_queues = []   # plain list on the module, not in state_dict (:56-57, :78-81)
        self.filter_convs = nn.ModuleList()
        self.gate_convs = nn.ModuleList()
        self.residual_convs = nn.ModuleList()
        self.skip_convs = nn.ModuleList()
        self.start_conv = nn.Conv1d(classes, residual_channels, kernel_size=1, bias=bias)

        receptive_field = 1
        previous = 1
        for _ in range(blocks):
            span = kernel_size - 1
            d = 1
            for _ in range(layers):
                self.dilations.append((d, previous))
                self.dilated_queues.append(DilatedQueue(max_length=(kernel_size - 1) * d + 1,
                                                        num_channels=residual_channels, dilation=d, dtype=dtype))
                self.filter_convs.append(nn.Conv1d(residual_channels, dilation_channels, kernel_size, bias=bias))
                self.gate_convs.append(nn.Conv1d(residual_channels, dilation_channels, kernel_size, bias=bias))
                self.residual_convs.append(nn.Conv1d(dilation_channels, residual_channels, 1, bias=bias))
                self.skip_convs.append(nn.Conv1d(dilation_channels, skip_channels, 1, bias=bias))
                receptive_field += span
                span *= 2
                previous = d
                d *= 2
        self.end_conv_1 = nn.Conv1d(skip_channels, end_channels, 1, bias=True)
        self.end_conv_2 = nn.Conv1d(end_channels, classes, 1, bias=True)
        self.output_length = output_length
        self.receptive_field = receptive_field
        self.__dict__.update(_wn_defaults())

    # ------------------------------------------------------------------ training path (torch ops)
    def wavenet(self, input, dilation_func):
        """The residual stack (wavenet_model.py:125-171) with a pluggable dilation function."""
        x = self.start_conv(input)
        skip = None
        for i in range(self.blocks * self.layers):
            dilation, init_dilation = self.dilations[i]
            residual = dilation_func(x, dilation, init_dilation, i)
            x = torch.tanh(self.filter_convs[i](residual)) * torch.sigmoid(self.gate_convs[i](residual))
            s = x
            if x.size(2) != 1:
                s = dilate(x, 1, init_dilation=dilation)
            s = self.skip_convs[i](s)
            # right-aligned crop-add (the reference gets skip=0 on the first layer through a bare except)
            skip = s if skip is None else s + skip[:, :, -s.size(2):]
            x = self.residual_convs[i](x)
            x = x + residual[:, :, (self.kernel_size - 1):]
        x = F.relu(skip)
        x = F.relu(self.end_conv_1(x))
        return self.end_conv_2(x)

    def wavenet_dilate(self, input, dilation, init_dilation, i):
        return dilate(input, dilation, init_dilation)

    def queue_dilate(self, input, dilation, init_dilation, i):
        queue = self.dilated_queues[i]
        queue.enqueue(input.data[0])
        return queue.dequeue(num_deq=self.kernel_size, dilation=dilation).unsqueeze(0)

    def _native_supported(self):
        """Shapes the matrix-core kernels cover (wn_forward / wn_train_*): kernel_size 2, channel counts multiples of 32."""
        return self.kernel_size == 2 and not any(c % 32 for c in (self.residual_channels, self.dilation_channels, self.skip_channels,
                                                                  self.end_channels, self.classes))

    def _native_indices_supported(self):
        """Shapes the index-based inference extensions cover (forward_indices / score_indices: wn_forward / wn_score): kernel_size 2, 3 or 4,
        channel counts multiples of 32.  forward() on a one-hot tensor and training stay on torch ops for kernel_size != 2 unless native_taps_training is on."""
        return self.kernel_size in (2, 3, 4) and not any(c % 32 for c in (self.residual_channels, self.dilation_channels, self.skip_channels,
                                                                            self.end_channels, self.classes))

    def _native_trainable(self):
        """Shapes the native training step covers by default (kernel_size 3 and 4 are opt-in: _native_taps_trainable): kernel_size 2 and a class count that is a multiple of 32 -- channel counts that are not multiples
        of 32 are zero-padded up to multiples of 64 for it (round 6: mi355_wavenet/training.py StackRunner.pad_tensors, shapes from mi355_wavenet/params.py; same logits, same gradients)."""
        return self.kernel_size == 2 and self.classes % 32 == 0

    def _native_taps_trainable(self):
        """Opted in (native_taps_training) and a shape the k-tap training step covers: kernel_size 3 or 4, channel counts and classes multiples of 32
        (no zero padding for kernel_size != 2)."""
        return bool(self.native_taps_training) and self.kernel_size in (3, 4) and self._native_indices_supported()

    def _padded_train_config(self):
        """(config, model shape) of the training engine: the model's own when its channel counts are multiples of 32, else padded to multiples of 64
        (so that the bf16 step's kernels apply as well)."""
        cfg = self._config()
        if self._native_supported() or self._native_taps_trainable():
            return cfg, None
        shape = (self.residual_channels, self.dilation_channels, self.skip_channels, self.end_channels)
        up = lambda c: (c + 63) // 64 * 64  # noqa: E731
        cfg.update(residual_channels=up(shape[0]), dilation_channels=up(shape[1]), skip_channels=up(shape[2]), end_channels=up(shape[3]))
        return cfg, shape

    def _fallback(self, reason, warn=True):
        """forward() on a CUDA tensor is about to run the reference's algorithm in torch ops (MIOpen conv1d + autograd) instead of the
        native kernels: counted per reason (wn_stats()) and said out loud ONCE per reason -- the dual path is never silent."""
        stats = self._wn_fallbacks
        stats[reason] = stats.get(reason, 0) + 1
        if warn and stats[reason] == 1:
            import warnings
            warnings.warn("WaveNetModel.forward(): torch path instead of the MI355X matrix-core kernels: %s "
                          "(said once per reason; model.wn_stats() counts every call)" % reason, RuntimeWarning, stacklevel=4)
        return None

    def wn_stats(self):
        """Extension: which path forward() / model(x) calls of this module took so far: {'native_forward', 'native_train_forward',
        'torch_fallbacks': {reason: calls}} -- CPU tensors are not fallbacks (the reference's own path), everything else on a CUDA
        tensor that did not reach wn_forward / wn_train_* is."""
        return {"native_forward": int(self._wn_forward_calls), "native_train_forward": int(self._wn_train_calls),
                "torch_fallbacks": dict(self._wn_fallbacks)}

    def _native_forward(self, input):
        """Matrix-core forward (C ABI wn_forward, or wn_train_forward + wn_train_backward behind a torch.autograd.Function
        when gradients are wanted) when it applies: CUDA input that is exactly one-hot, shapes the GEMM kernels support.  Returns
        None otherwise -- the caller then runs the torch path, and on a CUDA tensor that is counted and warned about (_fallback).
        Short clips (the reference's zero-padding regime) are served natively; the engine answers WN_E_UNSUPPORTED only for lengths
        at which the reference has no defined result, and the torch path then reproduces what the reference does there.  A library
        that is not built is NOT a reason to fall back: on a CUDA tensor that raises (the product must not run silently without its
        kernels)."""
        if not input.is_cuda:
            return None   # the reference's own path: nothing to report
        if input.dim() != 3 or input.size(1) != self.classes:
            return self._fallback("input is not (N, classes, L)")
        taps = self._native_taps_trainable()
        if self.kernel_size != 2 and not taps:
            if self.native_taps_training and self.kernel_size in (3, 4):
                return self._fallback("kernel_size %d with channel counts or classes that are not multiples of 32 (no zero padding for kernel_size != 2)"
                                      % self.kernel_size)
            return self._fallback("kernel_size %d (the matrix-core kernels are written for 2)" % self.kernel_size)
        want_grad = torch.is_grad_enabled() and any(p.requires_grad for p in self.parameters())
        # Without autograd the engine decides: a channel shape that is not a multiple of 32 may still run natively, zero-padded into a
        # compiled shape (include/wn_abi.h: wn_create); with autograd the handle keeps the model's own shape and needs the multiples.
        no_native = self._wn_forward_unsupported == self._forward_shape_key(input.device)
        if want_grad and not taps and not self._native_trainable():
            return self._fallback("a class count that is not a multiple of 32 under autograd")
        if not want_grad and no_native and not taps and not self._native_supported():
            return self._fallback("channel counts that are not multiples of 32 and fit no compiled shape")
        if torch.is_grad_enabled() and input.requires_grad:
            return self._fallback("a gradient with respect to the one-hot input is wanted")
        if want_grad and input.dtype != torch.float32:
            return self._fallback("autograd on a %s input" % str(input.dtype).replace("torch.", ""))
        if want_grad and os.environ.get("WN_TORCH_BACKWARD") == "1":
            return self._fallback("WN_TORCH_BACKWARD=1")
        vals, idx = input.max(dim=1)
        if not bool(((vals == 1) & (input.sum(dim=1) == 1)).all()):
            return self._fallback("the input is not a one-hot batch (start_conv is a real contraction)")
        from mi355_wavenet import _abi
        try:
            if want_grad:
                return self._native_train_forward(idx)
            eng = self._forward_engine()
            if not eng.info()["forward_native"]:
                # THIS channel shape has no native forward on this device (not zero-padded into a compiled shape): do not ask again.
                # Keyed on what the engine REPORTS (wn_info.forward_native), not on the wording of an error.
                self._wn_forward_unsupported = self._forward_shape_key(input.device)
                return self._fallback("channel counts that are not multiples of 32 and fit no compiled shape")
            self._apply_precision(eng)
            out = eng.forward_indices(idx, self.output_length)
        except _abi.WnError as e:
            if e.code == _abi.WN_E_UNSUPPORTED:
                # (refusals of ONE call -- N*L >= 2^31 rows, a clip length the reference has no result for -- say nothing about the next call;
                #  the torch path reproduces what the reference does there: its error, or its shapes)
                return self._fallback("the engine refused this call: %s" % e, warn=False)
            raise
        self._wn_forward_calls += 1
        return out.to(input.dtype)

    def _forward_shape_key(self, device):
        return (str(device), self.residual_channels, self.dilation_channels, self.skip_channels, self.end_channels, self.classes)

    def _forward_engine(self):
        """The engine forward() runs on: the generation engine when it holds the current parameters -- whatever its stream count, so that a
        validation forward between two generate_fast() calls leaves it (and its deferred queues) alone --, else a one-stream engine."""
        if self._wn_engine is not None and self._wn_engine_key is not None and self._wn_engine_key[1:] == self._parameters_key():
            return self._wn_engine
        return self._engine(1)

    def _parameters_key(self):
        """(device index, (address, version) of every parameter): what an engine's copy of the weights was made from."""
        plist = list(self.parameters())   # (every state_dict entry of this module is a parameter)
        dev = plist[0].device
        index = dev.index if dev.type == "cuda" and dev.index is not None else int(os.environ.get("WN_DEVICE", "0"))
        return index, tuple((v.data_ptr(), v._version) for v in plist)

    def _apply_precision(self, eng):
        want = self.matrix_precision == "bf16"
        c = eng.cfg   # (the ENGINE's channel shape: the training engine of a model with odd channel counts is zero-padded to multiples of 64)
        if want and any(c[k] % 64 for k in ("residual_channels", "dilation_channels", "skip_channels", "end_channels")):
            want = False
        taps = False
        if c.get("kernel_size", 2) != 2:
            # (kernel_size 3 and 4: fp32 unless opted in, and then on the forward engine alone -- the training step of such a model is fp32)
            runner = self._wn_train_runner
            taps = want = (want and bool(self.native_taps_bf16) and c["kernel_size"] in (3, 4) and not (runner is not None and eng is runner.eng))
        eng.set_forward_precision(want, taps=taps)

    def _native_train_forward(self, idx):
        """model(x) with a native backward: see mi355_wavenet/training.py."""
        from mi355_wavenet import engine, params, training
        runner = self._wn_train_runner
        dev = next(self.parameters()).device
        if runner is None or runner.device != dev:
            cfg, shape = self._padded_train_config()
            weights = dict(self.state_dict())
            if shape is not None:   # (the handle is created on zero-padded weights of ITS shape; the step's parameters are passed per call)
                weights = params.padded(weights, cfg)
            eng = engine.Engine(cfg, weights, n_streams=1, device_index=dev.index or 0, pad_channels=False)
            runner = training.StackRunner(eng, model_shape=shape)  # the handle only provides plan, layout and workspace: parameters are passed per call
            self._wn_train_runner = runner
        by_key = params.from_module(self)
        self._wn_train_calls += 1
        self._apply_precision(runner.eng)
        if self.deterministic_gradients is not None:
            runner.set_deterministic(bool(self.deterministic_gradients))
        return training.StackFunction.apply(runner, idx, self.output_length, tuple((k, len(ts)) for k, ts in by_key.items()),
                                            *itertools.chain.from_iterable(by_key.values()))

    def _checked_indices(self, indices, check, training=False):
        idx = torch.as_tensor(indices)
        if idx.dim() != 2:
            raise ValueError("indices must be (N, L) class indices")
        if training and (self._native_trainable() or self._native_taps_trainable()):
            pass   # (kernel_size 2: the training engine pads odd channel counts itself; 3, 4: opted in, multiples of 32)
        elif training and self.kernel_size != 2:
            raise ValueError("the index-based training forward needs kernel_size 2 (kernel_size %d: inference only, forward_indices / "
                             "score_indices)" % self.kernel_size)
        elif not self._native_indices_supported():
            raise ValueError("the index-based forward needs kernel_size 2, 3 or 4 and channel counts that are multiples of 32 "
                             "(kernel_size %d, residual %d, dilation %d, skip %d, end %d, classes %d)" % (
                                 self.kernel_size, self.residual_channels, self.dilation_channels, self.skip_channels, self.end_channels, self.classes))
        if idx.size(1) < 2:
            raise ValueError("items of %d sample(s): forward() needs at least two" % idx.size(1))
        if check and idx.numel() and (int(idx.min()) < 0 or int(idx.max()) >= self.classes):
            raise ValueError("class indices outside [0, %d)" % self.classes)  # they address rows of start_conv^T on the GPU
        return idx

    def forward_indices(self, indices, check=True):
        """Extension: forward() on class indices (N, L) instead of a one-hot (N, classes, L) tensor -- what the
        dataset holds before audio_data.py:119-121 inflates it 256x.  Inference only (matrix-core path, no autograd).
        ``check=False`` skips the range check of the indices (one device sync) when the producer guarantees it."""
        idx = self._checked_indices(indices, check)
        return self._on_forward_engine(lambda eng: eng.forward_indices(idx, self.output_length))

    def score_indices(self, indices, targets=None, check=True, want_rows=False, want_pred=False):
        """Extension: teacher-forced scoring on class indices -- what WavenetTrainer.validate() computes per batch (wavenet_training.py:89-112) and
        the log-likelihood of audio under the model -- on the engine (C ABI wn_score): the logits never reach memory.  ``indices`` (N, L) and
        ``targets`` (N, output_length) or (N*output_length,): the class each output position should predict.  ``targets=None``: ``indices`` is the
        dataset's own window of L + 1 samples per item (audio_data.py: item_indices); the input is its first L samples and the targets are its last
        output_length, as WavenetDataset.__getitem__ cuts them.  Returns a ScoreResult of DEVICE tensors (nothing is synchronised until the caller
        reads one): loss (mean negative log-likelihood in nats = F.cross_entropy), accuracy, n (rows counted), with want_rows / want_pred row_nll float32 /
        pred int32 (N, output_length) (else None),
        sums (float64 (3,): sum of row_nll, hits, n).  A target outside [0, classes) gives a NaN row_nll and is left out of loss, accuracy and n.
        Same checks and errors as forward_indices; ``check=False`` skips the range check of the indices."""
        idx = torch.as_tensor(indices)
        if targets is None:
            if idx.dim() != 2:
                raise ValueError("indices must be (N, L) class indices")
            if idx.size(1) < self.output_length + 1:
                raise ValueError("windows of %d sample(s): targets=None needs at least output_length + 1 = %d" % (idx.size(1), self.output_length + 1))
            targets = idx[:, -self.output_length:]
            idx = idx[:, :-1]
        idx = self._checked_indices(idx, check)
        tgt = torch.as_tensor(targets)
        if tgt.numel() != idx.size(0) * self.output_length:
            raise ValueError("targets hold %d values, %d items x output_length %d need %d" % (
                tgt.numel(), idx.size(0), self.output_length, idx.size(0) * self.output_length))
        out = self._on_forward_engine(lambda eng: eng.score(idx, tgt, self.output_length, want_rows=want_rows, want_pred=want_pred))
        sums = out["sums"]
        return ScoreResult(loss=sums[0] / sums[2], accuracy=sums[1] / sums[2], n=sums[2], row_nll=out["row_nll"], pred=out["row_pred"], sums=sums)

    def _on_forward_engine(self, call):
        """One index-based inference call on the forward engine, at the model's precision; counted in wn_stats()."""
        eng = self._forward_engine()
        self._apply_precision(eng)
        out = self._index_call(lambda: call(eng))
        self._wn_forward_calls += 1
        return out

    @staticmethod
    def _index_call(fn):
        """The index-based extensions have no torch path to fall back to: a clip length the engine refuses (one the reference has no
        defined result for either, include/wn_abi.h: wn_forward) is the caller's ValueError, with the engine's reason."""
        from mi355_wavenet import _abi
        try:
            return fn()
        except _abi.WnError as e:
            if e.code == _abi.WN_E_UNSUPPORTED:
                raise ValueError(str(e)) from e
            raise

    def train_forward_indices(self, indices, check=True):
        """Extension: the differentiable forward() on class indices (N, L) -- the training-time sibling of forward_indices:
        logits (N*output_length, classes) whose backward runs natively (see _native_train_forward).  MI355X only."""
        idx = self._checked_indices(indices, check, training=True)
        return self._index_call(lambda: self._native_train_forward(idx))

    def forward(self, input):
        """(N, classes, L) one-hot -> (N*output_length, classes) logits (wavenet_model.py:186-196)."""
        native = self._native_forward(input)
        if native is not None:
            return native
        x = self.wavenet(input, dilation_func=self.wavenet_dilate)
        n, c, _ = x.size()
        l = self.output_length
        x = x[:, :, -l:].transpose(1, 2).contiguous()
        return x.view(n * l, c)

    def generate(self, num_samples, first_samples=None, temperature=1.):
        raise NotImplementedError("WaveNetModel.generate() is dead code upstream (undefined self.scope, "
                                  "wavenet_model.py:209); use generate_fast()")

    # ------------------------------------------------------------------ generation path (HIP engine)
    def _config(self):
        return dict(layers=self.layers, blocks=self.blocks, dilation_channels=self.dilation_channels,
                    residual_channels=self.residual_channels, skip_channels=self.skip_channels,
                    end_channels=self.end_channels, classes=self.classes, kernel_size=self.kernel_size,
                    bias=self.start_conv.bias is not None)

    def _engine(self, n_streams):
        """The MI355X engine holding this module's current parameters (rebuilt when they change)."""
        from mi355_wavenet import engine
        key = (n_streams,) + self._parameters_key()
        index = key[1]
        if self._wn_engine is None or self._wn_engine_key != key:
            params = list(self.state_dict().items())
            if self._wn_engine is not None and self._wn_engine_key[:2] == key[:2]:
                self._wn_engine.load_weights(dict(params))
            else:
                if self._wn_engine is not None:
                    self._flush_queues()  # their loaders read the engine that is about to go
                    self._wn_engine.close()
                self._wn_engine = engine.Engine(self._config(), dict(params), n_streams=n_streams, device_index=index)
            self._wn_engine_key = key
        return self._wn_engine

    def generate_fast(self, num_samples, first_samples=None, temperature=1., regularize=0.,
                      progress_callback=None, progress_interval=100, *, top_k=0, top_p=0., continue_from=None, return_state=False,
                      return_logprobs=False, forced=None, append=None):
        """Same contract as wavenet_model.py:237-315; returns float64 ndarray (num_samples,).
        Extension (keyword only): top_k / top_p truncate every sampled draw inside the sampler kernels (include/wn_abi.h: wn_set_sampling); one
        uniform per sample is drawn from the global numpy RNG as without them, and the engine's filter is off again when the call returns or raises.
        continue_from: a ``mi355_wavenet.state.GenerationState`` (or a list of them, one per stream: the result is then 2-D) -- the call behaves as
        ``generate_fast(first_samples=[state.last_index])`` except that the dilation queues are LOADED from the state instead of reset: callbacks,
        the timing print and the RNG's consumption are those of that call.  Together with first_samples it is a ValueError.
        return_state=True: returns (audio, state) -- the stream's state behind the last generated sample (a list of states for a 2-D prompt or a
        list given as continue_from), to continue from later, in another process (it pickles; ``state.save(path)``) or on other stream counts.
        return_logprobs="sampling" | "model" (True: "sampling"): the result gains a float32 array shaped like the audio, directly behind it -- (audio,
        logp) or (audio, logp, state) -- with the log-probability of every generated sample, written by the sampler kernels (include/wn_abi.h:
        wn_set_logprob_output): of the distribution the draw was made from (temperature and filters applied), or of the model's own logits.  The RNG's
        consumption, the callbacks and the queues left behind are those of the call without it.
        forced: an int array shaped like the audio (1-D, or 2-D with the prompt's rows) -- a class index in [0, classes) is what the stream emits at
        that position, -1 leaves the position to the draw (include/wn_abi.h: wn_set_forced_samples).  A forced sample enters the network and the
        state like a drawn one and gets its log-probability like one; its uniform is drawn and not used, so the RNG's consumption, the callbacks and the
        timing print are those of the call without it.
        Ragged prompts: first_samples may be a list or tuple of 1-D sequences or tensors, one prompt per stream, of ANY lengths >= 1 (a list of plain
        integers stays one 1-D prompt).  The result is (len(prompts), num_samples), row s being generate_fast(num_samples, first_samples=prompts[s]) of
        a one-stream call given the same uniforms; the RNG's consumption is that of the 2-D call, (streams, n_new) uniforms per piece, and rows of
        equal length ARE the 2-D call.  All prompts are primed in one batched pass over the streams' own samples (Engine.prime_ragged: no length
        threshold), the streams right-aligned in time; callbacks, the timing print and the piece cuts are those of a call with num_given = the longest
        prompt whose priming the batched pass covered.  return_state: state s counts evals = len(prompts[s]) - 1 + num_samples.  forced stays
        (streams, num_samples).  Where the batched pass does not apply (kernel_size above 4, the unpadded kernel_size 3 and 4 shapes, an older
        library) every prompt is primed ALONE on a one-stream engine and its state loaded into the job's engine: correct for every shape, and slow.
        append: given audio that CONTINUES the checkpoint, valid only with continue_from (else a ValueError) -- one 1-D sequence of class indices for
        one state, a list of 1-D sequences for a list of states (any lengths, an empty one included).  The stream's inputs continue
        state.last_index, append[0], ..., append[-1]: the len(append) evaluations on all but the last of them are teacher-forced in ONE batched pass
        onto the loaded queues (Engine.prime_append: no uniform is drawn for them), generation starts from append[-1].  Callbacks, piece cuts and the
        timing print are those of generate_fast(first_samples=[last_index, *append]) with its priming covered by the batched pass; return_state
        counts evals = state.evals + len(append) + num_samples.  Where the batched pass does not apply the state is loaded and [last_index, *append]
        primed through the chain -- for a list, stream by stream on a one-stream engine whose state is then loaded: correct for every shape, and slow."""
        logprobs = self._logprob_mode(return_logprobs)
        forced = self._checked_forced(forced, num_samples)
        states, first_samples, appended = self._continuation("generate_fast", continue_from, first_samples, append)
        return self._generate_fast(num_samples, first_samples, temperature, regularize, progress_callback, progress_interval, top_k, top_p,
                                   states, return_state, logprobs, forced, appended=appended)

    def advance_state(self, states, samples):
        """A state and some given audio -> the state behind that audio: ``generate_fast(0, continue_from=states, append=samples,
        return_state=True)[1]`` without the timing print.  One GenerationState and one 1-D sequence, or a list of each; nothing is drawn."""
        states, first_samples, appended = self._continuation("advance_state", states, None, samples, need_append=True)
        return self._generate_fast(0, first_samples, 1., 0., None, 100, 0, 0., states, True, None, None, timing_print=False, appended=appended)[1]

    # Opt-in piecewise priming: None -- every prompt is primed in ONE batched pass, whose workspace grows with the longest prompt --, or an integer
    # p >= 1: the first p columns of every stream's prompt are primed as before (Engine.prime_host / prime_ragged / prime_shared), the following ones
    # in pieces of at most p through Engine.prime_append.  The workspace is then a piece's; states and audio are those of the one pass, bit for bit.
    prime_piece_samples = None

    def _prime_pieces(self, eng, given, first_pass, shared=False):
        """``given``: one array per stream (shared: ONE array) of teacher-forced inputs for freshly reset queues.  first_pass(rows) -> bool primes
        such rows in one batched pass.  Returns its answer: with prime_piece_samples = None for all of ``given`` -- the call as it always was --,
        else for the first columns, the rest following in prime_append passes."""
        p = self.prime_piece_samples
        longest = max(g.size for g in given)
        if p is None or longest <= p or not eng.lib.has("wn_prime_append"):
            return first_pass(given)
        if int(p) != p or p < 1:
            raise ValueError("prime_piece_samples must be None or an integer >= 1, got %r" % (p,))
        if not first_pass([g[:p] for g in given]):
            return False
        for a in range(p, longest, p):
            piece = [g[a:a + p] for g in given]
            if not eng.prime_append(piece[0] if shared else piece, shared=shared):
                raise RuntimeError("the engine primed the first %d columns in a batched pass and refuses to append the next piece" % p)
        return True

    @staticmethod
    def _logprob_mode(return_logprobs):
        """return_logprobs of the facade -> Engine.generate's logprobs: None, "sampling" or "model" """
        if return_logprobs is False or return_logprobs is None:
            return None
        if return_logprobs is True:
            return "sampling"
        if return_logprobs in ("sampling", "model"):
            return return_logprobs
        raise ValueError('return_logprobs must be False, True, "sampling" or "model", got %r' % (return_logprobs,))

    # ---- what generate_fast, generate_fast_streams and score_continuation share: the prologue (arguments -> checked `forced`, states, prompt: every
    #      argument error before an engine is touched), the filter around the job, and the epilogue (_finish)
    def _checked_forced(self, forced, num_samples, rows=None):
        from mi355_wavenet import engine
        return engine.checked_forced(forced, num_samples, self.classes, rows)

    def _continuation(self, caller, continue_from, first_samples, append=None, need_append=False):
        """-> (None, first_samples, None) without continue_from; else (the states as a list, checked against this model; the first_samples that stand
        for them: 1-D for a single state, else 2-D; None, or -- ``append`` -- every stream's row [last_index, *append] as int64 arrays) --
        continue_from and first_samples exclude each other, append needs continue_from"""
        if continue_from is None:
            if append is not None:
                raise ValueError("%s: append continues a checkpoint and needs continue_from" % caller)
            return None, first_samples, None
        if first_samples is not None:
            raise ValueError("%s: continue_from carries the next input (last_index); first_samples must not be given with it" % caller)
        from mi355_wavenet.state import GenerationState
        single = isinstance(continue_from, GenerationState)
        states = [continue_from] if single else list(continue_from)
        if not states or not all(isinstance(st, GenerationState) for st in states):
            raise ValueError("continue_from must be a GenerationState or a non-empty list of them")
        for st in states:
            st.check(self)
        last = np.asarray([[st.last_index] for st in states], dtype=np.int64)
        appended = None
        if append is not None or need_append:
            from mi355_wavenet import engine
            if append is None or (not single and not isinstance(append, (list, tuple))):
                raise ValueError("%s: append is one 1-D sequence for one state, a list of them for a list of states" % caller)
            rows = engine.ragged_rows([append] if single else append, self.classes, min_length=0)[0]
            if len(rows) != len(states):
                raise ValueError("%s: append holds %d sequence(s) for %d state(s)" % (caller, len(rows), len(states)))
            appended = [np.concatenate([last[s], r]) for s, r in enumerate(rows)]
        return states, torch.from_numpy(last[0] if single else last), appended

    def _stream_state(self, eng, stream, last_index, evals):
        from mi355_wavenet.state import GenerationState
        return GenerationState(eng.state_save(stream), last_index, evals, layers=self.layers, blocks=self.blocks, residual_channels=self.residual_channels,
                               kernel_size=self.kernel_size, classes=self.classes)

    def _ragged_prompt(self, first_samples):
        """A list / tuple of rows (one prompt per stream) -> its checked rows, int64 arrays of length >= 1; None for every other first_samples.  Such a
        list never reaches torch.as_tensor."""
        from mi355_wavenet import engine
        if not engine.is_ragged_prompt(first_samples):
            return None
        return engine.ragged_rows(first_samples, self.classes, min_length=1)[0]

    def _prime_ragged(self, eng, rows):
        """Fresh queues on ``eng``, then every stream primed with all but the last sample of its row: ONE batched pass (Engine.prime_ragged), or --
        where the engine cannot -- every prompt alone on a one-stream engine (its batched pass or its chain, whichever it takes) whose saved state is
        loaded into the stream; slow, and right for every shape.  Returns the right-aligned (streams, longest) matrix of the rows: its last column is
        every stream's next input."""
        from mi355_wavenet import engine
        eng.reset()
        batched = self._prime_pieces(eng, [r[:-1] for r in rows], eng.prime_ragged)
        if not batched:
            states = []
            if any(r.size > 1 for r in rows):
                one = engine.Engine(self._config(), dict(self.state_dict()), n_streams=1, device_index=self._parameters_key()[0])
                try:
                    for r in rows:
                        if r.size > 1:
                            one.generate(0, r[None, :], reset=True)   # (num_samples 0: the priming evaluations alone)
                        states.append(one.state_save(0) if r.size > 1 else None)
                finally:
                    one.close()
            for s, st in enumerate(states):
                if st is not None:
                    eng.state_load(st, s, 1)
        self._wn_last_prime_batched = bool(batched)
        return engine.right_aligned(rows)

    def _prime_append(self, eng, rows, states, shared=False):
        """``eng`` holds the states (loaded at queue time 0); every stream is teacher-forced through all but the last sample of its row
        [last_index, *append]: ONE batched pass onto the loaded queues (Engine.prime_append; shared: one row, every stream holds states[0]), or --
        where the engine cannot -- through the chain: on ``eng`` itself where its streams all take the one row, else stream by stream on a
        one-stream engine that loads the state, primes and hands its state back.  Returns the right-aligned (streams, longest) matrix of the rows."""
        from mi355_wavenet import engine
        given = [r[:-1] for r in rows]
        batched = eng.prime_append(given[0] if shared else given, shared=shared)
        if not batched and any(g.size for g in given):
            if shared or len(rows) == 1:
                eng.generate(0, rows[0], reset=False)   # (num_samples 0: the priming evaluations alone)
            else:
                one = engine.Engine(self._config(), dict(self.state_dict()), n_streams=1, device_index=self._parameters_key()[0])
                try:
                    for s, r in enumerate(rows):
                        if r.size > 1:
                            one.reset()
                            one.state_load(states[s].state)
                            one.generate(0, r[None, :], reset=False)
                            eng.state_load(one.state_save(0), s, 1)
                finally:
                    one.close()
        self._wn_last_prime_batched = bool(batched)
        return engine.right_aligned(rows)

    def _prompt(self, first_samples):
        """first_samples (None: the one sample classes // 2, wavenet_model.py:245-247) -> (int64 (n_streams, num_given), whether it came as 2-D rows)"""
        if first_samples is None:
            first_samples = torch.LongTensor(1).zero_() + (self.classes // 2)
        first = torch.as_tensor(first_samples).detach().cpu().numpy().astype(np.int64)
        return first.reshape(first.shape[0] if first.ndim == 2 else 1, -1), first.ndim == 2

    @contextlib.contextmanager
    def _sampling_filter(self, eng, top_k, top_p):
        """top_k / top_p on the engine's handle for the jobs inside (every piece carries it), off again behind them -- also when one raises"""
        try:
            if top_k or top_p:
                eng.set_sampling(top_k, top_p)
            yield
        finally:
            if top_k or top_p:
                eng.set_sampling(0, 0.)

    def _finish(self, eng, idx, logp, squeeze=False, stream=0, state=None):
        """The engine's class indices (n_streams, n) -> what the caller gets, audio[, logp][, state()] (a tuple as soon as there is more than the
        audio; squeeze: the one row of a 1-D call), with model.dilated_queues deferred to ``stream``'s final state and the module back in train()
        (wavenet_model.py:313)."""
        self._defer_queues(eng, stream)
        self.train()
        result = [self._expand_indices(idx)] + ([logp] if logp is not None else [])  # :296, :314
        if squeeze:
            result = [r[0] for r in result]
        if state is not None:
            result.append(state())
        return result[0] if len(result) == 1 else tuple(result)

    def _generate_fast(self, num_samples, first_samples, temperature, regularize, progress_callback, progress_interval, top_k, top_p,
                       states=None, return_state=False, logprobs=None, forced=None, timing_print=True, appended=None):
        """normalise, reset, load the states, prime, plan, execute, finish: where the job is cut into pieces and what runs between them is
        mi355_wavenet/generation.py's"""
        from mi355_wavenet import generation
        self.eval()
        ragged = appended if appended is not None else self._ragged_prompt(first_samples)
        if appended is None and ragged is not None and len({r.size for r in ragged}) == 1:   # rows of one length: the 2-D call
            first_samples, ragged = torch.from_numpy(np.stack(ragged)), None
        if ragged is not None:
            first, batched = None, appended is None or first_samples.ndim == 2   # (append onto ONE state: the 1-D result)
            n_streams, num_given = len(ragged), max(r.size for r in ragged)
        else:
            first, batched = self._prompt(first_samples)
            n_streams, num_given = first.shape
        forced = self._checked_forced(forced, num_samples, rows=n_streams)
        for queue in self.dilated_queues:  # :250-251
            queue.reset()
        eng = self._engine(n_streams)
        eng.reset()
        for s, st in enumerate(states or ()):   # (queue time 0 again: the canonical form does not depend on it)
            eng.state_load(st.state, s, 1)
        with self._sampling_filter(eng, top_k, top_p):
            # priming (:259-269): all n_prime teacher-forced evaluations as ONE batched pass over the given window (C ABI wn_prime: the stack as
            # matrix-core GEMMs over all positions, queues filled from the result); shapes it does not cover take the per-sample chain
            n_prime = num_given - 1
            if ragged is not None:   # prompts of unequal length: all of the priming is behind us either way, the job starts from the last column
                first = self._prime_append(eng, ragged, states) if appended is not None else self._prime_ragged(eng, ragged)
                primed = n_prime
            else:
                primed = n_prime if n_prime >= eng.PRIME_BATCH_MIN and self._prime_pieces(eng, list(first[:, :n_prime]), lambda g: eng.prime_host(np.stack(g))) else 0
                self._wn_last_prime_batched = primed > 0
            steps = generation.generation_schedule(num_given, num_samples, progress_interval, progress_callback is not None, primed, temperature > 0)
            idx, logp = generation.run_schedule(steps, eng, first, temperature, regularize, forced, logprobs, progress_callback, timing_print)

            def state():   # behind the last generated sample, whose index is the input of the next step
                nxt = idx[:, -1] if idx.shape[1] else first[:, -1]
                before = [st.evals for st in states] if states is not None else [0] * n_streams
                given = [r.size - 1 for r in ragged] if ragged is not None else [n_prime] * n_streams   # (a stream's own priming evaluations)
                out = [self._stream_state(eng, s, int(nxt[s]), before[s] + given[s] + num_samples) for s in range(n_streams)]
                return out if batched else out[0]
            return self._finish(eng, idx, logp, squeeze=not batched, state=state if return_state else None)

    def _expand_indices(self, idx):
        """Class indices -> float64 audio: ``o = idx / classes * 2 - 1`` (wavenet_model.py:296) then ``mu_law_expansion(o)``
        (:314, audio_data.py:156-158).  Both are elementwise, so the 256 possible results are computed once with the very
        same numpy expressions and looked up (10 ms -> 0.3 ms per 128 k samples); the table is checked once against the
        elementwise evaluation on a probe that puts every class at shifted array positions."""
        classes = self.classes
        tab = self._wn_expansion
        if tab is None or tab[0] != classes:
            every = np.arange(classes, dtype=np.int64)
            table = mu_law_expansion((every / classes) * 2. - 1, classes)
            probe = np.concatenate([every[3:], every[::-1], every[:5]])
            ok = bool(np.array_equal(table[probe], mu_law_expansion((probe / classes) * 2. - 1, classes)))
            tab = self._wn_expansion = (classes, table if ok else None)
        idx = np.asarray(idx).astype(np.int64)
        if tab[1] is None:
            return mu_law_expansion((idx / classes) * 2. - 1, classes)
        return tab[1][idx]

    def _defer_queues(self, eng, stream=0):
        """The reference leaves model.dilated_queues in their final state (wavenet_model.py:177-184).  Here that state is on
        the GPU: every queue gets a loader that downloads its ring on first access (wn_export_queue); nothing is copied
        for callers that never look."""
        for layer, queue in enumerate(self.dilated_queues):
            queue._defer(lambda layer=layer: eng.export_queue(layer, stream))

    def _flush_queues(self):
        for queue in self.dilated_queues:
            if getattr(queue, "_lazy", None) is not None:
                queue._sync()

    # generate_fast_streams primes its shared prompt ONCE (Engine.prime_shared) instead of once per stream: every stream's queues are bit for bit those
    # of the per-stream pass (tests/test_gpu_generation_state.py), the products run over 1 / n_streams of the rows (profiles/r16_generation_state.txt)
    SHARED_PRIME = True

    def generate_fast_streams(self, num_samples, temperatures, first_samples=None, regularize=0., *, top_k=0, top_p=0., continue_from=None,
                              return_logprobs=False, forced=None, append=None):
        """Extension: one generate_fast() per entry of ``temperatures`` -- the reference's generate_audio loop
        (wavenet_training.py:115-124) -- as parallel streams of ONE persistent-kernel job.  Returns float64
        (len(temperatures), num_samples), row k equal to ``generate_fast(num_samples, first_samples, temperatures[k])``
        of sequential calls: sampled rows consume the global numpy RNG in the order of ``temperatures`` (one draw per
        sample), greedy rows (temperature <= 0, wavenet_model.py:290-294) consume none.  top_k / top_p as in generate_fast (greedy rows ignore them).
        continue_from: ONE ``GenerationState`` that every temperature continues from (N variations of a checkpoint) -- as first_samples=[last_index]
        with the queues loaded into every stream instead of reset; together with first_samples it is a ValueError.
        append (with continue_from only): ONE 1-D sequence of given audio that continues the state for all temperatures, as in generate_fast; it is
        teacher-forced once for all streams (the shared form of Engine.prime_append).
        return_logprobs as in generate_fast: returns (audio, logp), logp float32 (len(temperatures), num_samples); a greedy row holds the log-softmax
        value of its argmax.
        forced as in generate_fast: (num_samples,) shared by all rows, or (len(temperatures), num_samples); -1 is a free position.
        first_samples as a list or tuple of len(temperatures) 1-D sequences (of any lengths >= 1): one prompt per temperature, all primed in one batched
        pass (generate_fast's ragged prompts); a 1-D prompt stays shared and is primed once.  The rows' draws and the deferred dilated_queues (the
        last stream's) are as without it."""
        logprobs = self._logprob_mode(return_logprobs)
        self._checked_forced(forced, num_samples, rows=len(temperatures))   # (checked here, before an engine is touched; Engine.generate makes the rows)
        if continue_from is not None and isinstance(continue_from, (list, tuple)) and len(continue_from) != 1:
            raise ValueError("generate_fast_streams: continue_from is ONE state that all temperatures share")
        if isinstance(continue_from, (list, tuple)) and append is not None:
            append = [append]
        states, first_samples, appended = self._continuation("generate_fast_streams", continue_from, first_samples, append)
        if states is not None and len(states) != 1:
            raise ValueError("generate_fast_streams: continue_from is ONE state that all temperatures share")
        ragged = self._ragged_prompt(first_samples)
        if ragged is not None and len(ragged) != len(temperatures):
            raise ValueError("generate_fast_streams: a list of prompts holds one per temperature (%d), got %d" % (len(temperatures), len(ragged)))
        self.eval()
        temps = [float(t) for t in temperatures]
        first = None if ragged is not None else np.repeat(self._prompt(first_samples)[0].reshape(1, -1), len(temps), axis=0)
        for queue in self.dilated_queues:
            queue.reset()
        eng = self._engine(len(temps))
        uniforms = np.zeros((len(temps), num_samples), dtype=np.float64)
        for k, t in enumerate(temps):   # row by row, sampled rows only: the draws of sequential calls
            if t > 0:
                uniforms[k] = np.random.random_sample(num_samples)
        with self._sampling_filter(eng, top_k, top_p):
            if states is not None:
                eng.reset()
                eng.state_load(states[0].state)   # one state, every stream
            if appended is not None:   # the given audio once for all streams, the job starts from its last sample
                first = np.repeat(self._prime_append(eng, appended, states, shared=True)[:, -1:], len(temps), axis=0)
            if ragged is not None:   # one prompt per temperature: primed here, the job starts from every stream's last given sample
                first = self._prime_ragged(eng, ragged)[:, -1:]
            shared_prompt = self.SHARED_PRIME and states is None and ragged is None and eng.lib.has("wn_prime_shared")
            reset = states is None and ragged is None
            if shared_prompt and self.prime_piece_samples is not None and first.shape[1] - 1 >= eng.PRIME_BATCH_MIN:   # the shared prompt in pieces
                eng.reset()
                if self._prime_pieces(eng, [first[0, :-1]], lambda g: eng.prime_shared(g[0]), shared=True):
                    first, reset, shared_prompt = first[:, -1:], False, False
            out = eng.generate(num_samples, first, temperature=np.asarray(temps, dtype=np.float32), regularize=regularize,
                               uniforms=uniforms if any(t > 0 for t in temps) else None, reset=reset, logprobs=logprobs,
                               forced=forced, shared_prompt=shared_prompt)
        idx, logp = out if logprobs is not None else (out, None)
        return self._finish(eng, idx, logp, stream=len(temps) - 1)  # sequential calls would leave the LAST temperature's queues

    def score_continuation(self, indices, continue_from=None, first_samples=None, return_state=False, *, append=None):
        """The model's log-likelihood of audio that CONTINUES a stream: float32 shaped like ``indices`` (class indices, 1-D or 2-D), entry g being
        log p(indices[g] | the prompt or state, indices[:g]) in nats -- the negative of score_indices' row losses, computed by the generation kernels
        in constant memory: a greedy job (no uniform is drawn: the numpy RNG is left alone) in which every position is forced
        (include/wn_abi.h: wn_set_forced_samples) under return_logprobs="model".  Any length, any kernel_size the generation kernels serve.
        continue_from: a GenerationState (a list of them, one per row, for 2-D indices), or first_samples as in generate_fast (default: classes // 2).
        append (with continue_from only): given audio between the state and ``indices``, as in generate_fast -- teacher-forced in one batched pass, not
        scored (its log-probabilities are score_continuation's of that audio as ``indices``).
        return_state=True: returns (logp, state) with the state behind the last sample -- chunked scoring: score a long clip piece by piece, each
        piece continuing from the state the piece before returned, for the same values as the single call."""
        idx = indices.detach().cpu().numpy() if torch.is_tensor(indices) else np.asarray(indices)
        if idx.dtype.kind not in "iu" or idx.ndim not in (1, 2) or idx.shape[-1] < 1:
            raise ValueError("score_continuation: indices must be a non-empty integer array, 1-D or (streams, n); got %s %r" % (idx.dtype, idx.shape))
        if idx.min() < 0 or idx.max() >= self.classes:
            raise ValueError("score_continuation: indices outside [0, classes)")
        states, first_samples, appended = self._continuation("score_continuation", continue_from, first_samples, append)
        if states is not None:
            if first_samples.ndim != idx.ndim or (idx.ndim == 2 and len(states) != idx.shape[0]):
                raise ValueError("score_continuation: one GenerationState for 1-D indices, a list of one per row for 2-D indices")
        elif self._ragged_prompt(first_samples) is not None:   # one prompt per row, of any lengths
            if idx.ndim != 2 or len(first_samples) != idx.shape[0]:
                raise ValueError("score_continuation: a list of prompts needs 2-D indices with one row per prompt")
        elif first_samples is not None and idx.ndim == 2:
            rows = torch.as_tensor(first_samples)
            if rows.ndim != 2 or rows.shape[0] != idx.shape[0]:
                raise ValueError("score_continuation: 2-D indices need first_samples with the same number of rows")
        elif first_samples is None and idx.ndim == 2:
            first_samples = torch.full((idx.shape[0], 1), self.classes // 2, dtype=torch.int64)
        elif first_samples is not None and torch.as_tensor(first_samples).ndim != 1:
            raise ValueError("score_continuation: 1-D indices need 1-D first_samples")
        out = self._generate_fast(idx.shape[-1], first_samples, 0., 0., None, 100, 0, 0., states, return_state, "model", idx.astype(np.int32),
                                  timing_print=False, appended=appended)
        return (out[1], out[2]) if return_state else out[1]

    # ------------------------------------------------------------------ bookkeeping
    def parameter_count(self):
        return sum(int(np.prod(list(p.size()))) for p in self.parameters())

    def cpu(self, type=torch.FloatTensor):
        self.dtype = type
        for q in self.dilated_queues:
            q.dtype = self.dtype
        return super().cpu()

    def __getstate__(self):  # the engine handle is not picklable and is rebuilt on demand
        self._flush_queues()
        state = self.__dict__.copy()
        state["_wn_engine"] = None
        state["_wn_engine_key"] = None
        state["_wn_train_runner"] = None
        state.pop("_wn_expansion", None)
        state.pop("_wn_forward_unsupported", None)   # (an answer about THIS device's library: not part of the model)
        return state

    def __setstate__(self, state):
        """Also accepts snapshots pickled by the REFERENCE's class (torch.save(model), wavenet_training.py:84-88 -- its only
        checkpoint format): their __dict__ has no end_channels / bias / engine fields (wavenet_model.py:42-56)."""
        super().__setstate__(state)   # nn.Module back-fills the hook / buffer attributes that a snapshot of an older torch lacks
        d = self.__dict__
        for k, v in _wn_defaults().items():
            d.setdefault(k, v)
        if "end_channels" not in d:
            d["end_channels"] = self.end_conv_1.out_channels
        if "bias" not in d:
            d["bias"] = self.start_conv.bias is not None


def load_latest_model_from(location, use_cuda=True):
    """Newest file (by ctime) in ``location`` -> model (wavenet_model.py:330-340)."""
    files = [location + "/" + f for f in os.listdir(location)]
    newest_file = max(files, key=os.path.getctime)
    print("load model " + newest_file)
    if use_cuda:
        model = torch.load(newest_file, weights_only=False)
    else:
        model = load_to_cpu(newest_file)
    return model


def load_to_cpu(path):
    model = torch.load(path, map_location=lambda storage, loc: storage, weights_only=False)
    model.cpu()
    return model
