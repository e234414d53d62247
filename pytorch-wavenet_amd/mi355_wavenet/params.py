"""The model's 14 parameter arrays, stated once: key (the field names of include/wn_abi.h: wn_weight_ptrs / wn_train_tensors), where the
reference's module keeps it (wavenet_model.py:59-119: ``<module>[.<layer>].<attr>`` in a ``state_dict``), whether it exists once or once per
layer, and its Conv1d shape in letters: R, D, S, E = residual / dilation / skip / end channels, C = classes, k = kernel_size.  The rows stand
in travelling order -- the argument order of training.StackFunction -- with the arrays that exist only with ``bias=True`` last.  Pure Python
and numpy: no torch at import."""
import collections
import operator

import numpy as np

Param = collections.namedtuple("Param", ["key", "module", "attr", "per_layer", "shape"])

TABLE = (
    Param("start_w", "start_conv", "weight", False, "RC1"),
    Param("filter_w", "filter_convs", "weight", True, "DRk"),
    Param("gate_w", "gate_convs", "weight", True, "DRk"),
    Param("res_w", "residual_convs", "weight", True, "RD1"),
    Param("skip_w", "skip_convs", "weight", True, "SD1"),
    Param("end1_w", "end_conv_1", "weight", False, "ES1"),
    Param("end1_b", "end_conv_1", "bias", False, "E"),      # (the end convolutions always carry a bias, wavenet_model.py:111-119)
    Param("end2_w", "end_conv_2", "weight", False, "CE1"),
    Param("end2_b", "end_conv_2", "bias", False, "C"),
    Param("start_b", "start_conv", "bias", False, "R"),
    Param("filter_b", "filter_convs", "bias", True, "D"),
    Param("gate_b", "gate_convs", "bias", True, "D"),
    Param("res_b", "residual_convs", "bias", True, "R"),
    Param("skip_b", "skip_convs", "bias", True, "S"),
)
N_ALWAYS = 9   # rows of TABLE a model without bias has
BY_KEY = {p.key: p for p in TABLE}
PARAM_ORDER = tuple(p.key for p in TABLE)
SINGLE_KEYS = tuple(p.key for p in TABLE if not p.per_layer)
# the order in which the reference's constructor registers the modules, hence the order of a state_dict (ModuleLists first)
MODULES = ("filter_convs", "gate_convs", "residual_convs", "skip_convs", "start_conv", "end_conv_1", "end_conv_2")


def rows(bias):
    """The table's rows of a model with / without bias, in travelling order."""
    return TABLE if bias else TABLE[:N_ALWAYS]


def order(bias):
    return PARAM_ORDER if bias else PARAM_ORDER[:N_ALWAYS]


def name(key, layer=None):
    """The ``state_dict`` name of (key, layer); ``layer`` only for the per-layer keys."""
    p = BY_KEY[key]
    return "%s.%d.%s" % (p.module, layer, p.attr) if p.per_layer else "%s.%s" % (p.module, p.attr)


def shape(key, cfg):
    """Shape of one array of ``key`` (one layer's, for the per-layer keys) under a configuration (WaveNetModel's constructor arguments)."""
    d = {"R": cfg["residual_channels"], "D": cfg["dilation_channels"], "S": cfg["skip_channels"], "E": cfg["end_channels"],
         "C": cfg["classes"], "k": cfg.get("kernel_size", 2), "1": 1}
    return tuple(d[c] for c in BY_KEY[key].shape)


def entries(cfg):
    """(state_dict name, key) of every array of a configuration, in ``state_dict`` order: module by module, layer by layer, weight before bias."""
    nl = cfg["layers"] * cfg["blocks"]
    for module in MODULES:
        ps = [p for p in rows(bool(cfg.get("bias", False))) if p.module == module]   # (a module's weight row stands before its bias row)
        for layer in (range(nl) if ps[0].per_layer else (None,)):
            for p in ps:
                yield name(p.key, layer), p.key


def from_module(model):
    """{key: [the module's own nn.Parameters]} in travelling order (one per layer, in layer order, for the per-layer keys)."""
    out = {}
    for p in rows(model.start_conv.bias is not None):
        m, get = getattr(model, p.module), operator.attrgetter(p.attr)
        out[p.key] = list(map(get, m)) if p.per_layer else [get(m)]   # (runs every training step: no Python-level loop per tensor)
    return out


def _array(x):
    if hasattr(x, "detach"):
        x = x.detach().cpu().numpy()
    return np.ascontiguousarray(np.asarray(x), dtype=np.float32)


def stacked(weights, cfg):
    """name -> array (reference Conv1d layouts; numpy or torch) -> {key: fp32 host array}, the per-layer keys stacked over the layers: the arrays
    of wn_weight_ptrs."""
    nl = cfg["layers"] * cfg["blocks"]
    return {p.key: np.ascontiguousarray(np.stack([_array(weights[name(p.key, i)]) for i in range(nl)])) if p.per_layer
            else _array(weights[name(p.key)]) for p in rows(bool(cfg.get("bias", False)))}


def padded(weights, cfg):
    """name -> array -> the same mapping for the channel shape of ``cfg``: every array in the leading block of a zero-filled one."""
    out = collections.OrderedDict()
    for n, key in entries(cfg):
        a = _array(weights[n])
        buf = np.zeros(shape(key, cfg), dtype=np.float32)
        buf[tuple(slice(0, s) for s in a.shape)] = a
        out[n] = buf
    return out
