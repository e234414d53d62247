"""Host-side driver of the MI355X generation engine (C ABI: include/wn_abi.h).

``Engine`` owns one ``wn_handle``: a planned chain of persistent workgroups with the weights of one
WaveNet packed for LDS residency.  It mirrors what ``WaveNetModel.generate_fast`` needs
(/root/reference/wavenet_model.py:237-315) for one or many independent streams.  PyTorch is used only
for device memory and the current HIP stream.
"""
import ctypes

import numpy as np

from . import _abi, params


def regularizer_array(classes, regularize):
    """(c - classes/2)^2 * regularize evaluated like the reference does (wavenet_model.py:273-274):
    a float32 tensor times a python scalar."""
    import torch
    r = torch.pow(torch.arange(classes) - classes / 2., 2)
    return (r.squeeze() * regularize).numpy().astype(np.float32)


def checked_forced(forced, num_samples, classes, rows=None):
    """The ``forced`` argument of Engine.generate and of the facade (generate_fast, generate_fast_streams), checked in this one place: None, or
    integers shaped like the audio -- (num_samples,) or (streams, num_samples) -- in [-1, classes), -1 being a free position; ValueError for anything
    else.  rows=None -> an int32 array of the shape given.  rows=n: a 2-D array must have n rows, a 1-D one is shared by them -> a writable C-ordered
    int32 (n, num_samples) copy."""
    if forced is None:
        return None
    if num_samples < 1:
        raise ValueError("forced: the job generates no sample")
    f = np.asarray(forced.detach().cpu() if hasattr(forced, "detach") else forced)
    if f.dtype.kind not in "iu" or f.ndim not in (1, 2) or f.shape[-1] != num_samples or (f.ndim == 2 and rows is not None and f.shape[0] != rows):
        raise ValueError("forced must be an integer array shaped like the audio, (%d,) or (%s, %d); got %s %r" % (
            num_samples, "streams" if rows is None else rows, num_samples, f.dtype, f.shape))
    if f.min() < -1 or f.max() >= classes:
        raise ValueError("forced outside [-1, classes): -1 is a free position, 0 .. classes - 1 a forced class")
    if rows is None:
        return f.astype(np.int32)
    return np.array(np.broadcast_to(f.reshape(-1, num_samples), (rows, num_samples)), dtype=np.int32, order="C")


def _host_array(v):
    return np.asarray(v.detach().cpu() if hasattr(v, "detach") else v)


def is_ragged_prompt(first_samples):
    """True for a non-empty list / tuple of ROWS (sequences, arrays, tensors): one prompt per stream, of any lengths.  A list of plain integers is
    the 1-D prompt it always was; arrays and tensors are never ragged."""
    if not isinstance(first_samples, (list, tuple)) or not first_samples:
        return False
    return not all(_host_array(v).ndim == 0 for v in first_samples)


def ragged_rows(prompts, classes, min_length=1):
    """A list / tuple of 1-D integer sequences or tensors -> ([int64 arrays], int64 array of their lengths).  ValueError for anything else: a row
    that is not 1-D or not of integers, one shorter than min_length, a class index outside [0, classes)."""
    if not isinstance(prompts, (list, tuple)):
        raise ValueError("prompts must be a list or tuple of 1-D integer sequences, got %s" % type(prompts).__name__)
    rows = []
    for s, p in enumerate(prompts):
        a = _host_array(p)
        if a.ndim != 1:
            raise ValueError("prompt %d is not a 1-D sequence (shape %r)" % (s, a.shape))
        if a.size and a.dtype.kind not in "iu":
            raise ValueError("prompt %d holds %s values, class indices are integers" % (s, a.dtype))
        if a.size < min_length:
            raise ValueError("prompt %d holds %d sample(s), at least %d needed" % (s, a.size, min_length))
        a = a.astype(np.int64)
        if a.size and (a.min() < 0 or a.max() >= classes):
            raise ValueError("prompt %d outside [0, classes)" % s)
        rows.append(a)
    return rows, np.asarray([r.size for r in rows], dtype=np.int64)


def right_aligned(rows):
    """The rows as an int64 (len(rows), longest) matrix, each row ending in the last column (zeros in front of it)"""
    out = np.zeros((len(rows), max(r.size for r in rows)), dtype=np.int64)
    for s, r in enumerate(rows):
        if r.size:
            out[s, out.shape[1] - r.size:] = r
    return out


class _TorchMem:
    """Device memory, streams and transfers through PyTorch-ROCm (the memory provider of every product Engine)."""
    def __init__(self, device_index):
        import torch
        self.torch = torch
        self.device = torch.device("cuda", device_index)

    def upload(self, a):
        return self.torch.from_numpy(np.ascontiguousarray(a)).to(self.device)

    def empty(self, shape, dtype):
        td = {np.int32: self.torch.int32, np.float32: self.torch.float32, np.float64: self.torch.float64}[dtype]
        return self.torch.empty(shape, dtype=td, device=self.device)

    def ptr(self, a):
        return a.data_ptr() if a is not None else None

    def download(self, a):
        return a.cpu().numpy()

    def stream(self):
        return self.torch.cuda.current_stream(self.device).cuda_stream


class _Resident:
    """uniforms already uploaded (Engine.upload_uniforms)"""
    def __init__(self, dev, shape):
        self.dev, self.shape = dev, tuple(shape)


class Engine:
    def __init__(self, cfg, weights, n_streams=1, device_index=0, layer_split=0, head_split=0, lib=None, mem=None, pad_channels=True):
        """lib / mem: the loaded C-ABI library and the memory provider (upload / empty / ptr / download / stream); the defaults are
        the HIP library and torch device memory.  (Dependency injection for the host-logic tests, which pass a test double of the C
        ABI together with ITS memory provider -- tests/double_lib.py; nothing in this package knows about it.)
        pad_channels=False: no zero padding of a channel shape the fast kernel is not compiled for (include/wn_abi.h: wn_create)."""
        self.lib = lib if lib is not None else _abi.load_product_library()
        self.cfg = dict(cfg)
        self.n_streams = int(n_streams)
        self.classes = int(cfg.get("classes", 256))
        if mem is not None:
            self.mem = mem
        else:
            import torch
            if not torch.cuda.is_available():
                raise RuntimeError("mi355_wavenet: no HIP device visible; the generation engine needs an MI355X "
                                   "(there is no CPU fallback)")
            self.mem = _TorchMem(device_index)
        c = _abi.wn_config(cfg["layers"], cfg["blocks"], cfg["dilation_channels"], cfg["residual_channels"],
                           cfg["skip_channels"], cfg["end_channels"], self.classes, cfg.get("kernel_size", 2),
                           int(bool(cfg.get("bias", False))), self.n_streams, device_index, layer_split, head_split)
        if not pad_channels:  # WN_CFG_NO_PADDING: plan the model's own channel shape (a handle that serves wn_train_* must)
            c.reserved[0] = 1
        self._sampling = (0, 0.0)   # what set_sampling last put on the handle
        self._h = ctypes.c_void_p()
        self.lib.check(self.lib.dll.wn_create(ctypes.byref(c), ctypes.byref(self._h)))
        self.load_weights(weights)

    # -- lifetime
    def close(self):
        if getattr(self, "_h", None) is not None and self._h:
            self.lib.dll.wn_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    # -- ABI calls
    def _need(self, symbol, since):
        """The optional export ``symbol`` (_abi.OPTIONAL_EXPORTS), or the one error for a library built before ``since``."""
        if not self.lib.has(symbol):
            raise RuntimeError("mi355_wavenet: %s does not export %s (a library built before %s): rebuild it with pytorch-wavenet_amd/build.py"
                               % (self.lib.path, symbol, since))
        return getattr(self.lib.dll, symbol)

    def load_weights(self, weights):
        st = params.stacked(weights, self.cfg)   # (host arrays, alive until wn_load_weights has copied them)
        w = _abi.wn_weight_ptrs(*[st[n].ctypes.data if n in st else None for n in _abi.WEIGHT_FIELDS])
        self.lib.check(self.lib.dll.wn_load_weights(self._h, ctypes.byref(w)))

    def info(self):
        i = _abi.wn_info()
        self.lib.check(self.lib.dll.wn_get_info(self._h, ctypes.byref(i)))
        return {n: getattr(i, n) for n, _ in i._fields_}

    def reset(self):
        """DilatedQueue.reset() of every layer and stream (wavenet_model.py:250-251)."""
        self.lib.check(self.lib.dll.wn_reset(self._h, self.mem.stream()))

    def export_queue(self, layer, stream=0):
        """(data (R, (k-1)d+1) float32, in_pos, out_pos) like the reference's DilatedQueue fields."""
        k = self.cfg.get("kernel_size", 2)
        d = 2 ** (layer % self.cfg["layers"])
        R = self.cfg["residual_channels"]
        data = np.zeros((R, (k - 1) * d + 1), dtype=np.float32)
        ip, op = ctypes.c_int32(), ctypes.c_int32()
        self.lib.check(self.lib.dll.wn_export_queue(self._h, layer, stream, data.ctypes.data, ctypes.byref(ip), ctypes.byref(op)))
        return data, ip.value, op.value

    def set_forward_precision(self, bf16, taps=False):
        """bf16 operands (fp32 accumulation) for forward_indices / score; fp32 is the parity default.  taps=True asks for WN_PRECISION_BF16_TAPS: the same
        on a kernel_size 2 engine, and the only bf16 mode a kernel_size 3 or 4 engine takes (wn_forward / wn_score alone; include/wn_abi.h)."""
        self.lib.check(self.lib.dll.wn_set_forward_precision(self._h, (2 if taps else 1) if bf16 else 0))

    def set_sampling(self, top_k=0, top_p=0.0):
        """top-k / nucleus (top-p) truncation of every sampled draw of every later job, inside the sampler kernels (C ABI wn_set_sampling; the
        contract is in include/wn_abi.h).  top_k: 0 or >= classes is off; top_p: 0 or 1 is off; (0, 0) restores the unfiltered draw.  Greedy streams
        ignore both.  With both off a library that lacks the symbol is left alone; asking it for a filter raises."""
        if isinstance(top_k, bool) or int(top_k) != top_k:
            raise ValueError("top_k must be an integer, got %r" % (top_k,))
        top_k, top_p = int(top_k), float(top_p)
        if top_k < 0 or top_k > 0x7fffffff:
            raise ValueError("top_k must be >= 0 (0 and >= classes: off), got %d" % top_k)
        if not (0.0 <= top_p <= 1.0):
            raise ValueError("top_p must lie in [0, 1] (0 and 1: off), got %r" % top_p)
        if top_k == 0 and top_p == 0.0 and not self.lib.has("wn_set_sampling"):
            return   # nothing was ever set on such a library
        self.lib.check(self._need("wn_set_sampling", "the sampling filters were added")(self._h, top_k, top_p))
        self._sampling = (top_k, top_p)

    def forward_indices(self, indices, output_length):
        """WaveNetModel.forward() on class indices: int tensor/array (N, L) -> float32 (N*output_length, classes) on the
        engine's device (a torch tensor; numpy for the emulator is not available: GPU only).  Asynchronous."""
        import torch
        idx = torch.as_tensor(indices).to(self.mem.device, torch.int32).contiguous()
        N, L = idx.shape
        out = torch.empty(N * output_length, self.classes, dtype=torch.float32, device=self.mem.device)
        self.lib.check(self.lib.dll.wn_forward(self._h, idx.data_ptr(), N, L, int(output_length), out.data_ptr(), self.mem.stream()))
        return out

    def score(self, indices, targets, output_length, want_rows=False, want_pred=False):
        """Teacher-forced scoring (C ABI wn_score): indices int (N, L), targets int (N*output_length,) or (N, output_length) -> dict with
        'sums' (float64 (3,) device tensor: sum of the rows' negative log-likelihoods in nats, rows whose argmax equals the target, rows counted)
        and, on request, 'row_nll' float32 / 'row_pred' int32 of shape (N, output_length).  A target outside [0, classes) gives a NaN row_nll and
        leaves the row out of the sums.  Device tensors, asynchronous: nothing is synchronised here."""
        score = self._need("wn_score", "teacher-forced scoring was added")
        import torch
        idx = torch.as_tensor(indices).to(self.mem.device, torch.int32).contiguous()
        N, L = idx.shape
        M = N * int(output_length)
        tgt = torch.as_tensor(targets).to(self.mem.device, torch.int64).reshape(-1).contiguous()
        if tgt.numel() != M:
            raise ValueError("targets hold %d values, %d items x output_length %d need %d" % (tgt.numel(), N, output_length, M))
        sums = torch.empty(3, dtype=torch.float64, device=self.mem.device)
        rows = torch.empty(N, int(output_length), dtype=torch.float32, device=self.mem.device) if want_rows else None
        pred = torch.empty(N, int(output_length), dtype=torch.int32, device=self.mem.device) if want_pred else None
        self.lib.check(score(self._h, idx.data_ptr(), tgt.data_ptr(), N, L, int(output_length), self.mem.ptr(rows), self.mem.ptr(pred), sums.data_ptr(),
                             self.mem.stream()))
        return {"sums": sums, "row_nll": rows, "row_pred": pred}

    def profile_next(self, n_items):
        self.lib.check(self.lib.dll.wn_profile_next(self._h, int(n_items)))

    def profile_read(self, n_items):
        """int64 (n_workgroups, n_items, 8) wall-clock stamps (100 MHz ticks) of the last profiled job."""
        info = self.info()
        n_wg = info["n_workgroups"] // max(1, info["n_chains"])  # stamps of the first chain
        out = np.zeros((n_wg, n_items, 8), dtype=np.int64)
        self.lib.check(self.lib.dll.wn_profile_read(self._h, out.ctypes.data, out.size))
        return out

    LOGPROB_MODES = {"sampling": _abi.WN_LOGP_SAMPLING, "model": _abi.WN_LOGP_MODEL}

    def set_logprob_output(self, logp_dev, capacity, mode):
        """Arms the NEXT job alone to write the log-probability of every generated sample into logp_dev, float32 (n_streams, num_samples) on the device
        (C ABI wn_set_logprob_output; the contract is in include/wn_abi.h).  mode: "sampling" -- of the distribution the draw was made from -- or "model"
        -- of the step's own logits.  logp_dev None disarms.  A library without the symbol raises."""
        if mode not in self.LOGPROB_MODES:
            raise ValueError('logprobs must be "sampling" or "model", got %r' % (mode,))
        arm = self._need("wn_set_logprob_output", "the per-sample log-probabilities were added")
        self.lib.check(arm(self._h, self.mem.ptr(logp_dev), int(capacity), self.LOGPROB_MODES[mode]))

    _FORCED = ("wn_set_forced_samples", "forced samples were added")   # _need()'s arguments

    def set_forced_samples(self, forced_dev, capacity):
        """Arms the NEXT job alone to read forced samples from forced_dev, int32 (n_streams, num_samples) on the device: a value in [0, classes) is what
        the stream emits at that position, anything else (canonically -1) leaves the draw alone (C ABI wn_set_forced_samples; the contract is in
        include/wn_abi.h).  forced_dev None disarms.  A library without the symbol raises."""
        self.lib.check(self._need(*self._FORCED)(self._h, self.mem.ptr(forced_dev), int(capacity)))

    def launch(self, first_dev, n_given, num_samples, temperature, reg_dev, uni_dev, out_dev, logits_dev, timeout_ms=0,
               temps_dev=None):
        """Enqueue one job on the current stream (asynchronous).  temps_dev: optional fp32 (n_streams,) per-stream temperatures."""
        a = _abi.wn_generate_args(self.mem.ptr(first_dev), n_given, num_samples, float(temperature), 0,
                                  self.mem.ptr(reg_dev), self.mem.ptr(uni_dev), self.mem.ptr(out_dev),
                                  self.mem.ptr(logits_dev), self.mem.stream(), int(timeout_ms), 0, self.mem.ptr(temps_dev))
        self.lib.check(self.lib.dll.wn_generate(self._h, ctypes.byref(a)))

    def wait(self):
        self.lib.check(self.lib.dll.wn_wait(self._h))

    def prime(self, first_dev, n_prime, row_stride):
        """Batched teacher-forced priming of freshly reset queues (wn_prime).  Returns False when the engine cannot
        (shape limits / emulator): the caller then primes through wn_generate, one chain pass per sample."""
        rc = self.lib.dll.wn_prime(self._h, self.mem.ptr(first_dev), int(n_prime), int(row_stride), self.mem.stream())
        if rc == _abi.WN_E_UNSUPPORTED:
            return False
        self.lib.check(rc)
        return True

    def prime_host(self, first_samples):
        """prime() on a host array (n_streams, n_prime) of class indices: all of them are teacher-forced inputs."""
        fs = np.ascontiguousarray(np.asarray(first_samples), dtype=np.int32)
        if fs.ndim != 2 or fs.shape[0] != self.n_streams:
            raise ValueError("first_samples must be (n_streams, n_prime)")
        if fs.size and (fs.min() < 0 or fs.max() >= self.classes):
            raise ValueError("first_samples outside [0, classes)")
        if fs.shape[1] == 0:
            return True
        return self.prime(self.mem.upload(fs), fs.shape[1], fs.shape[1])

    # -- the generation state as data (include/wn_abi.h: wn_state_*; mi355_wavenet/state.py holds it on the host)
    _STATE_SINCE = "the generation state could be saved and loaded"

    def state_floats(self):
        """float32 values of ONE stream's canonical state: the caller's residual channels x the sum of the layers' queue lengths."""
        n = ctypes.c_int64()
        self.lib.check(self._need("wn_state_floats", self._STATE_SINCE)(self._h, ctypes.byref(n)))
        return int(n.value)

    def state_save(self, stream=0):
        """The canonical, time-free state of one stream's dilation queues: float32 ndarray (state_floats(),) -- per layer (k-1)d+1 rows of R values,
        oldest first (wn_state_save).  Waits for the job in flight."""
        save = self._need("wn_state_save", self._STATE_SINCE)
        dev = self.mem.empty((self.state_floats(),), np.float32)
        self.lib.check(save(self._h, int(stream), self.mem.ptr(dev), self.mem.stream()))
        return np.ascontiguousarray(self.mem.download(dev), dtype=np.float32)

    def state_load(self, state, stream_first=0, stream_count=None):
        """Writes ONE canonical state into every stream of [stream_first, stream_first + stream_count) (default: up to the last stream), at the
        engine's present queue time, which it leaves alone (wn_state_load).  The other streams keep their queues."""
        load = self._need("wn_state_load", self._STATE_SINCE)
        a = np.ascontiguousarray(np.asarray(state), dtype=np.float32).reshape(-1)
        if a.size != self.state_floats():
            raise ValueError("the state holds %d values, this engine's streams hold %d" % (a.size, self.state_floats()))
        if stream_count is None:
            stream_count = self.n_streams - int(stream_first)
        dev = self.mem.upload(a)
        self.lib.check(load(self._h, int(stream_first), int(stream_count), self.mem.ptr(dev), self.mem.stream()))

    def prime_shared(self, first_row):
        """prime() for a prompt every stream shares: ONE row of teacher-forced class indices, the stack's products once, the result into every
        stream's queues (wn_prime_shared).  Returns False when the engine cannot (wn_prime's shape limits)."""
        prime = self._need("wn_prime_shared", self._STATE_SINCE)
        row = np.ascontiguousarray(np.asarray(first_row), dtype=np.int32).reshape(-1)
        if row.size and (row.min() < 0 or row.max() >= self.classes):
            raise ValueError("first_samples outside [0, classes)")
        if row.size == 0:
            return True
        dev = self.mem.upload(row)
        rc = prime(self._h, self.mem.ptr(dev), int(row.size), self.mem.stream())
        if rc == _abi.WN_E_UNSUPPORTED:
            return False
        self.lib.check(rc)
        return True

    def prime_ragged(self, prompts):
        """prime() for prompts of DIFFERENT lengths (wn_prime_ragged): ``prompts`` is a list of n_streams 1-D integer sequences, all of them
        teacher-forced inputs (a stream may have none).  One batched pass over the streams' own rows; the streams are right-aligned in time, the queue
        time afterwards is the longest length.  Returns False when the library lacks the symbol or the engine cannot (wn_prime's shape limits): the
        caller primes some other way.  ValueError, before any call: not n_streams rows, a row that is not 1-D, a class index out of range."""
        rows, lengths = ragged_rows(prompts, self.classes, min_length=0)
        if len(rows) != self.n_streams:
            raise ValueError("prompts must hold one row per stream (%d), got %d" % (self.n_streams, len(rows)))
        if not self.lib.has("wn_prime_ragged"):
            return False
        stride = max(1, int(lengths.max()))
        fs = np.zeros((self.n_streams, stride), dtype=np.int32)
        for s, row in enumerate(rows):
            fs[s, :row.size] = row
        dev = self.mem.upload(fs)   # (held until the launches are enqueued: the stream orders the rest)
        n = (ctypes.c_int64 * self.n_streams)(*[int(v) for v in lengths])
        rc = self.lib.dll.wn_prime_ragged(self._h, self.mem.ptr(dev), n, stride, self.mem.stream())
        if rc == _abi.WN_E_UNSUPPORTED:
            return False
        self.lib.check(rc)
        return True

    def prime_append(self, prompts, shared=False):
        """prime_ragged() onto queues that hold a history, at any queue time (wn_prime_append): ``prompts`` is a list of n_streams 1-D integer
        sequences (a stream may have none: it keeps its state), all of them teacher-forced inputs that CONTINUE the streams -- after a job, a
        ``state_load``, an earlier priming call.  The streams are right-aligned at the new queue time, the old one plus the longest length.
        shared=True: ``prompts`` is ONE sequence for all streams, which hold the same state; the products run once.  Returns False when the library
        lacks the symbol or the engine cannot (wn_prime's shape limits): the caller appends some other way.  ValueError, before any call: not
        n_streams rows, a row that is not 1-D, a class index out of range."""
        rows, lengths = ragged_rows([prompts] if shared else prompts, self.classes, min_length=0)
        if len(rows) != (1 if shared else self.n_streams):
            raise ValueError("prompts must hold one row per stream (%d), got %d" % (self.n_streams, len(rows)))
        if not self.lib.has("wn_prime_append"):
            return False
        stride = max(1, int(lengths.max()))
        fs = np.zeros((len(rows), stride), dtype=np.int32)
        for s, row in enumerate(rows):
            fs[s, :row.size] = row
        dev = self.mem.upload(fs)   # (held until the launches are enqueued: the stream orders the rest)
        n = (ctypes.c_int64 * len(rows))(*[int(v) for v in lengths])
        rc = self.lib.dll.wn_prime_append(self._h, self.mem.ptr(dev), n, stride, 1 if shared else 0, self.mem.stream())
        if rc == _abi.WN_E_UNSUPPORTED:
            return False
        self.lib.check(rc)
        return True

    def upload_uniforms(self, u):
        """float64 (n_streams, n) uniforms -> a resident handle ``generate(uniforms=...)`` accepts"""
        u = np.ascontiguousarray(np.asarray(u, dtype=np.float64))
        return _Resident(self.mem.upload(u), u.shape)

    # -- convenience: one synchronous generate_fast-shaped job
    PRIME_BATCH_MIN = 64  # given samples from which the GEMM priming path beats the per-sample chain passes

    def generate(self, num_samples, first_samples=None, temperature=1.0, regularize=0.0, uniforms=None,
                 want_logits=False, reset=True, timeout_ms=0, batched_prime=True, while_running=None, top_k=None, top_p=None, shared_prompt=False,
                 logprobs=None, forced=None):
        """first_samples: (n_streams, n_given) or (n_given,) ints (broadcast to every stream) or None -> classes//2.
        uniforms: float64 (n_streams, num_samples) (np.random.random_sample draws) or None -> greedy.
        temperature: a number, or one per stream (a stream with temperature <= 0 is greedy and ignores its uniforms row).
        uniforms may also be what ``upload_uniforms`` returned (already resident: drawn and uploaded while an earlier job ran).
        while_running: optional callable, invoked after the job has been enqueued and before this call waits for it -- host work
        that overlaps the kernel (the facade draws and uploads the NEXT piece's uniforms there).
        top_k / top_p: ``set_sampling`` before the job -- the values STAY on the handle for later jobs; None leaves what the handle has.
        shared_prompt: the streams share their given samples (a 1-D first_samples, or identical rows -- anything else is a ValueError): the batched
        priming runs once over the one row and fills every stream's queues (``prime_shared``).
        logprobs: None, "sampling" or "model" -- the log-probability of every generated sample, written by the sampler kernels (``set_logprob_output``).
        forced: None, or ints (n_streams, num_samples) or (num_samples,) (broadcast to every stream) -- a value in [0, classes) is what the stream emits at
        that position (it enters the network like a drawn sample; its log-probability is reported like one), -1 leaves the draw alone
        (``set_forced_samples``).  ``uniforms`` keeps its shape: the uniform of a forced position is not used.
        Returns indices int32 (n_streams, num_samples) [, logits float32 (n_streams, num_samples, classes)] [, logp float32 (n_streams, num_samples)]:
        a tuple as soon as there is more than the indices, the log-probabilities last."""
        ns, C = self.n_streams, self.classes
        if logprobs is not None and logprobs not in self.LOGPROB_MODES:
            raise ValueError('logprobs must be None, "sampling" or "model", got %r' % (logprobs,))
        if forced is not None:
            forced = checked_forced(forced, num_samples, C, rows=ns)
            self._need(*self._FORCED)   # (before anything is reset or enqueued)
        if top_k is not None or top_p is not None:
            self.set_sampling(self._sampling[0] if top_k is None else top_k, self._sampling[1] if top_p is None else top_p)
        if first_samples is None:
            first_samples = np.full((ns, 1), C // 2, dtype=np.int32)  # wavenet_model.py:245-247
        fs = np.asarray(first_samples)
        if fs.ndim == 1:
            fs = np.broadcast_to(fs[None, :], (ns, fs.shape[0]))
        if fs.shape[0] != ns or fs.shape[1] < 1:
            raise ValueError("first_samples must be (n_streams, n_given>=1)")
        if fs.min() < 0 or fs.max() >= C:
            raise ValueError("first_samples outside [0, classes)")
        fs = np.ascontiguousarray(fs, dtype=np.int32)
        if shared_prompt and not (fs == fs[:1]).all():
            raise ValueError("shared_prompt: the rows of first_samples differ")
        temps_dev = None
        if np.ndim(temperature) > 0:
            temps = np.ascontiguousarray(np.asarray(temperature, dtype=np.float32).reshape(ns))
            temps_dev = self.mem.upload(temps)
            temperature = float(temps.max())
        greedy = not (temperature > 0) or uniforms is None
        uni_dev = None
        if not greedy:
            if isinstance(uniforms, _Resident):
                if uniforms.shape != (ns, num_samples):
                    raise ValueError("resident uniforms have shape %r, the job needs %r" % (uniforms.shape, (ns, num_samples)))
                uni_dev = uniforms.dev
            else:
                uni_dev = self.mem.upload(np.ascontiguousarray(np.asarray(uniforms, dtype=np.float64).reshape(ns, num_samples)))
        reg_dev = self.mem.upload(regularizer_array(C, regularize)) if regularize else None
        first_dev = self.mem.upload(fs)
        out_dev = self.mem.empty((ns, max(num_samples, 1)), np.int32)
        logits_dev = self.mem.empty((ns, max(num_samples, 1), C), np.float32) if want_logits else None
        n_given = fs.shape[1]
        if reset:
            self.reset()
            if batched_prime and n_given - 1 >= self.PRIME_BATCH_MIN and (self.prime_shared(fs[0, :-1]) if shared_prompt else self.prime(first_dev, n_given - 1, n_given)):
                first_dev = self.mem.upload(np.ascontiguousarray(fs[:, -1:]))  # the last given sample is the next input
                n_given = 1
        logp_dev = None
        if logprobs is not None:
            logp_dev = self.mem.empty((ns, max(num_samples, 1)), np.float32)
            self.set_logprob_output(logp_dev, ns * max(num_samples, 1), logprobs)   # (armed right before the job that consumes it)
        if forced is not None:
            forced_dev = self.mem.upload(forced)   # (held until the wait below)
            self.set_forced_samples(forced_dev, forced.size)
        self.launch(first_dev, n_given, num_samples, temperature, reg_dev, uni_dev, out_dev, logits_dev, timeout_ms, temps_dev)
        if while_running is not None:
            while_running()
        self.wait()
        out = [self.mem.download(out_dev)[:, :num_samples]]
        if want_logits:
            out.append(self.mem.download(logits_dev)[:, :num_samples])
        if logprobs is not None:
            out.append(self.mem.download(logp_dev)[:, :num_samples])
        return out[0] if len(out) == 1 else tuple(out)
