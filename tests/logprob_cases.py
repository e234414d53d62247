"""The float64 statement of the per-sample log-probabilities (include/wn_abi.h: wn_set_logprob_output) and the bound the kernels are held to; numpy
only, no GPU.  tests/test_logprob_host.py checks the statement itself, tests/test_gpu_logprobs.py replays whole jobs through it.

  logp64(logits32, reg32, T32, greedy, top_k, top_p, idx, mode): what the contract writes for the class idx the sampler returned, in float64 on the
    float32 inputs the kernels see.
      "model":    l = the step's summed float32 logits; l_i - max(l) - log(sum_j exp(l_j - max(l))).  No regulariser, temperature or filter.
      "sampling": x = sampler_cases.x32 (fl32(logit - reg), then fl32(x / T) unless greedy); K = sampler_filter_cases.filter64's kept set (all classes
                  on a greedy row, which ignores the filters); x_i - max(x) - log(sum_{j in K} exp(x_j - max(x))), -inf for a class outside K.
  bound(logp, C, A) = 2 * (ln C + 4 + A) * 2^-24 + 2^-21 * |logp|: both terms derived, a factor 2 on top -- not a measured number.
      The first is the relative error of the kernels' fp32 kept-mass sum `tot` (logf turns it into an absolute one): the rounding of x_j - max, whose
      mass-weighted mean is at most ln C (units of 2^-24 relative to the mass); an expf of at most 2 ulp (4 units); the summation, A = the longest chain
      of fp32 additions behind one mass: A_ONE_WAVE for the one-wave sampler (3 inside a lane, 4 across a row, 2 over the rows' totals: 9, taken as
      10), a_generic(C) = ceil(C / 16) + 16 for the generic one (a chunk, then the 16 chunks' partials).
      The second covers the roundings of x_i - gm, logf and the final subtraction, each at most 2^-23 of a term no larger than |logp|."""
import math

import numpy as np

import sampler_cases as sc
import sampler_filter_cases as fc

MODES = ("sampling", "model")
A_ONE_WAVE = 10


def a_generic(C):
    return (C + sc.GROUPS - 1) // sc.GROUPS + sc.GROUPS


def a_of(variant, C):
    """A of the kernel variant a handle reports (wn_info.kernel_variant: 3 and 4 draw with the one-wave sampler, 1 is the generic kernel)"""
    return A_ONE_WAVE if variant in (3, 4) else a_generic(C)


def _logsoftmax_at(v32, keep, idx):
    v = np.asarray(v32, dtype=np.float32).astype(np.float64)
    if not keep[idx]:
        return -math.inf
    m = float(v.max())
    return float(v[idx] - m - math.log(np.exp(v[keep] - m).sum()))


def kept64(logits32, reg32, T32, greedy, top_k, top_p):
    """-> (x, keep mask, membership decided) of the sampling mode's row"""
    x = sc.x32(logits32, reg32, T32, greedy)
    if greedy:
        return x, np.ones(len(x), bool), True
    keep, decided = fc.filter64(x, top_k, top_p)
    return x, keep, decided


def logp64(logits32, reg32, T32, greedy, top_k, top_p, idx, mode):
    if mode == "model":
        l = np.asarray(logits32, dtype=np.float32)
        return _logsoftmax_at(l, np.ones(len(l), bool), int(idx))
    if mode != "sampling":
        raise ValueError("mode must be one of %r, got %r" % (MODES, mode))
    x, keep, _ = kept64(logits32, reg32, T32, greedy, top_k, top_p)
    return _logsoftmax_at(x, keep, int(idx))


def bound(logp, C, A):
    return 2.0 * (math.log(C) + 4.0 + A) * 2.0 ** -24 + 2.0 ** -21 * abs(logp)
