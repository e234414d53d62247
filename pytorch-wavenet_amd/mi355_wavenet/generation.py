"""How ``WaveNetModel.generate_fast`` cuts one job into engine calls: ``generation_schedule`` decides (pure arithmetic: no torch, no engine, no model --
tests/test_facade_schedule.py holds it against the reference's loop over thousands of combinations), ``run_schedule`` executes.

The job is evaluations ev = 0 .. n_eval-1: num_given-1 priming evaluations, then num_samples generating ones.  The reference runs them one by one
(its wavenet_model.py:259-311) and lets its caller see three things in between: the progress callback, after priming evaluation i when
i % interval == 0 (:266-269) and after generating step i when (i + num_given) % interval == 0 (:308-311); its timing print behind generating step 99
(:304-306), of a stopwatch started where generation starts (:275); and the global numpy RNG, one random_sample per generated sample when
temperature > 0 (np.random.choice, :288).  Here one persistent kernel launch runs a whole PIECE of evaluations, so the job is cut exactly where the
caller could look, and the RNG is never ahead of the reference at such a moment."""
import collections
import time

import numpy as np

# One engine call over evaluations [a, b): seg_prime priming evaluations, then n_new generated samples.  from_prompt: the head is
# first[:, a:a+seg_prime+1], else the last generated column.  restart_clock: the reference's stopwatch starts here.  draw: uniforms per stream to draw
# right before the piece (0: greedy, nothing generated, or the piece before drew them ahead); draw_ahead: the NEXT piece's uniforms, drawn and
# uploaded while this piece's kernel runs.
Piece = collections.namedtuple("Piece", ["a", "b", "seg_prime", "n_new", "from_prompt", "restart_clock", "draw", "draw_ahead"])
Callback = collections.namedtuple("Callback", ["i"])     # progress_callback(i, total_samples)
TimingPrint = collections.namedtuple("TimingPrint", [])  # the reference's "one generating step does take approximately" line


def generation_schedule(num_given, num_samples, interval, has_callback, primed, sampled):
    """The whole job as an ordered list of Piece / Callback / TimingPrint steps.  primed: priming evaluations a batched pass already covered, 0 or
    num_given - 1 (their callbacks are delivered up front, in order, each once).  There is a cut at the end of the job; at n_prime when the chain does
    the priming (generation, and the stopwatch, start there); behind generating step 99 when it exists; and behind every evaluation the reference
    calls back after."""
    n_prime = num_given - 1
    n_eval = n_prime + num_samples

    def due(ev):   # the callback's argument when the reference calls back after evaluation ev, else None
        i = ev if ev < n_prime else ev - n_prime + num_given
        return i if has_callback and i % interval == 0 else None

    def n_generated(a, b):
        return (b - a) - max(0, min(b, n_prime) - a)

    cuts = {n_eval, n_prime}
    if num_samples >= 100:
        cuts.add(n_prime + 100)
    if has_callback:   # behind priming evaluation i, and behind generating step i = evaluation n_prime + i, where the callback's argument is a multiple
        cuts.update(i + 1 for i in range(-(-primed // interval) * interval, n_prime, interval))
        cuts.update(range(-(-num_given // interval) * interval, num_given + num_samples, interval))
    cuts = sorted(c for c in cuts if c > primed)

    steps = [Callback(i) for i in range(0, primed, interval)] if has_callback else []
    a, drawn_ahead = primed, False
    for k, b in enumerate(cuts):
        n_new = n_generated(a, b)
        # Nothing of the caller's runs between two pieces when no callback is due at the cut (e.g. the cut that exists only for the timing print):
        # the next piece's uniforms are then drawn while this piece's kernel runs -- same draws, same order.
        ahead = n_generated(b, cuts[k + 1]) if sampled and k + 1 < len(cuts) and due(b - 1) is None else 0
        steps.append(Piece(a, b, (b - a) - n_new, n_new, a <= n_prime, a == n_prime, 0 if drawn_ahead or not sampled else n_new, ahead))
        if b == n_prime + 100:   # ahead of a callback due at the same evaluation, as in the reference
            steps.append(TimingPrint())
        if due(b - 1) is not None:
            steps.append(Callback(due(b - 1)))
        a, drawn_ahead = b, ahead > 0
    return steps


def run_schedule(steps, eng, first, temperature, regularize, forced=None, logprobs=None, progress_callback=None, timing_print=True):
    """Walks the steps on an Engine.  first: the prompt, int (n_streams, num_given); forced: None or int (n_streams, num_samples), each piece gets its
    slice; logprobs: Engine.generate's mode.  One uniform per stream and generated sample comes from the GLOBAL numpy RNG, (n_streams, n_new) per piece.
    Returns (indices int32 (n_streams, num_samples), log-probabilities float32 of the same shape or None).  A piece that generates nothing still runs
    (priming through the chain), with neither log-probabilities nor forced samples."""
    n_streams, num_given = first.shape
    total_samples = num_given + sum(st.n_new for st in steps if isinstance(st, Piece))
    idx, logp = [np.zeros((n_streams, 0), np.int32)], [np.zeros((n_streams, 0), np.float32)]
    done = 0          # generated samples behind us
    drawn = None      # this piece's uniforms, where the piece before drew them ahead: already resident
    tic = time.time()
    for st in steps:
        if isinstance(st, Callback):
            progress_callback(st.i, total_samples)
        elif isinstance(st, TimingPrint):
            if timing_print:
                print("one generating step does take approximately " + str((time.time() - tic) * 0.01) + " seconds)")
        else:
            if st.restart_clock:
                tic = time.time()
            u, drawn = drawn, None
            if st.draw:
                u = np.random.random_sample((n_streams, st.draw))
            overlap = None
            if st.draw_ahead:
                def overlap(n=st.draw_ahead):
                    nonlocal drawn
                    drawn = eng.upload_uniforms(np.random.random_sample((n_streams, n)))
            new = st.n_new > 0
            out = eng.generate(st.n_new, first[:, st.a:st.a + st.seg_prime + 1] if st.from_prompt else idx[-1][:, -1:].astype(np.int64),
                               temperature=temperature, regularize=regularize, uniforms=u, reset=False, while_running=overlap,
                               logprobs=logprobs if new else None, forced=forced[:, done:done + st.n_new] if (new and forced is not None) else None)
            if new and logprobs is not None:
                out, lp = out
                logp.append(lp)
            if new:
                idx.append(out)
                done += st.n_new
    return np.concatenate(idx, axis=1), np.concatenate(logp, axis=1) if logprobs is not None else None
