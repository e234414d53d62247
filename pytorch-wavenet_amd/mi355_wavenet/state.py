"""A stream's generation state as host data.

Between two generation jobs a stream is the input rings of its layers and the index it drew last.  ``GenerationState`` holds
the rings in the canonical, time-free form of the C ABI (include/wn_abi.h: wn_state_save / wn_state_load) -- for the layers in
order a block of ``(kernel_size - 1) * dilation + 1`` rows of ``residual_channels`` float32, oldest row first -- together with the
geometry it belongs to.  Plain numpy: it pickles, saves to one .npz, and converts to and from the reference's ``DilatedQueue``
fields (``data`` of shape (R, max_length) and ``in_pos``: what ``Engine.export_queue`` returns).  Nothing here touches a device.
"""
import numpy as np

GEOMETRY = ("layers", "blocks", "residual_channels", "kernel_size", "classes")


def queue_lengths(layers, blocks, kernel_size):
    """max_length of every layer's queue, in layer order (wavenet_model.py:72-78)"""
    return [(kernel_size - 1) * 2 ** i + 1 for _ in range(blocks) for i in range(layers)]


def _queue_fields(q):
    if hasattr(q, "data") and hasattr(q, "in_pos"):
        data, in_pos = q.data, q.in_pos
    else:
        data, in_pos = q[0], q[1]
    if hasattr(data, "detach"):
        data = data.detach().cpu().numpy()
    return np.asarray(data, dtype=np.float32), int(in_pos)


class GenerationState:
    def __init__(self, state, last_index, evals=0, *, layers, blocks, residual_channels, kernel_size=2, classes=256):
        """state: float32 (state_floats,) in the canonical form; last_index: the input of the next step; evals: evaluations the stream
        has seen (informational: the form does not depend on it)."""
        self.layers, self.blocks, self.residual_channels = int(layers), int(blocks), int(residual_channels)
        self.kernel_size, self.classes = int(kernel_size), int(classes)
        self.state = np.ascontiguousarray(np.asarray(state), dtype=np.float32).reshape(-1)
        self.last_index = int(last_index)
        self.evals = int(evals)
        if self.state.size != self.state_floats():
            raise ValueError("state: %d values, the geometry holds %d" % (self.state.size, self.state_floats()))
        if not 0 <= self.last_index < self.classes:
            raise ValueError("last_index %d outside [0, %d)" % (self.last_index, self.classes))

    # -- geometry
    def geometry(self):
        return {n: getattr(self, n) for n in GEOMETRY}

    def queue_lengths(self):
        return queue_lengths(self.layers, self.blocks, self.kernel_size)

    def state_floats(self):
        return self.residual_channels * sum(self.queue_lengths())

    def blocks_by_layer(self):
        """views (max_length, R) of the layers' blocks: row j = the layer's input ``max_length - j`` steps before the next evaluation"""
        out, off, R = [], 0, self.residual_channels
        for ml in self.queue_lengths():
            out.append(self.state[off:off + ml * R].reshape(ml, R))
            off += ml * R
        return out

    def check(self, model):
        """Raises ValueError naming the first field of the geometry that ``model`` (a WaveNetModel, an object with those attributes, or a
        config dict) does not share."""
        for n in GEOMETRY:
            if isinstance(model, dict):
                theirs = model.get(n, {"kernel_size": 2, "classes": 256}.get(n))
            else:
                theirs = getattr(model, n, None)
            if theirs is None or int(theirs) != getattr(self, n):
                raise ValueError("GenerationState: %s is %d, the model has %r" % (n, getattr(self, n), theirs))

    def __eq__(self, other):
        return (isinstance(other, GenerationState) and self.geometry() == other.geometry() and self.last_index == other.last_index
                and self.evals == other.evals and self.state.tobytes() == other.state.tobytes())

    __hash__ = None

    # -- the reference's DilatedQueue layout
    @classmethod
    def from_reference_queues(cls, queues, last_index, evals=0, *, classes=256):
        """queues: one per layer, objects with ``data`` (R, max_length) and ``in_pos`` (the reference's DilatedQueue, oracle/restated.py's Queue)
        or tuples (data, in_pos, ...) as Engine.export_queue returns.  The slot a push lands in is ``in_pos``, so the oldest column is the one
        at ``in_pos`` and row j of a block is column ``(in_pos + j) mod max_length``.  The geometry is read off the queue lengths."""
        fields = [_queue_fields(q) for q in queues]
        if not fields:
            raise ValueError("from_reference_queues: no queues")
        R = fields[0][0].shape[0]
        lengths = [f[0].shape[1] for f in fields]
        k = lengths[0]   # dilation 1: max_length = (k - 1) + 1
        if k < 2:
            raise ValueError("from_reference_queues: kernel_size 1 queues carry no geometry")
        dil = [(ml - 1) // (k - 1) for ml in lengths]
        layers = dil.index(1, 1) if 1 in dil[1:] else len(dil)
        blocks = len(dil) // layers
        if lengths != queue_lengths(layers, blocks, k) or any(f[0].shape[0] != R for f in fields):
            raise ValueError("from_reference_queues: queue shapes %r are not those of a WaveNet stack" % ([f[0].shape for f in fields],))
        parts = [np.roll(data.T, -in_pos, axis=0) for data, in_pos in fields]
        return cls(np.concatenate([p.reshape(-1) for p in parts]), last_index, evals, layers=layers, blocks=blocks, residual_channels=R,
                   kernel_size=k, classes=classes)

    def to_reference_queues(self, evals=None):
        """-> [(data (R, max_length) float32, in_pos, out_pos)] per layer, as the queues stand at queue time ``evals`` (default: this state's):
        in_pos = out_pos = evals mod max_length, block row j in column (evals + j) mod max_length."""
        t = self.evals if evals is None else int(evals)
        out = []
        for blk in self.blocks_by_layer():
            ml = blk.shape[0]
            out.append((np.ascontiguousarray(np.roll(blk, t % ml, axis=0).T), t % ml, t % ml))
        return out

    # -- files
    def save(self, path):
        with open(path, "wb") as f:
            np.savez(f, state=self.state, last_index=np.int64(self.last_index), evals=np.int64(self.evals),
                     geometry=np.asarray([getattr(self, n) for n in GEOMETRY], dtype=np.int64))

    @classmethod
    def load(cls, path):
        with np.load(path, allow_pickle=False) as z:
            geo = dict(zip(GEOMETRY, (int(v) for v in z["geometry"])))
            return cls(z["state"], int(z["last_index"]), int(z["evals"]), **geo)

    def __repr__(self):
        return "GenerationState(%s, last_index=%d, evals=%d)" % (", ".join("%s=%d" % (n, getattr(self, n)) for n in GEOMETRY), self.last_index, self.evals)
