"""Yardsticks for the transition posteriors of a flip-flop CRF (test infrastructure, numpy only).

The quantity: with alpha_0 = beta_n = 0 for all 8 states, the log-posterior of transition i of block t is
alpha_t[from(i)] + score_t[i] + beta_{t+1}[to(i)] minus the log-sum-exp of those 40 values.  Index b*8+s goes from
state s into flip b; index 32+s goes into flop: from flip s to flop s+4 for s < 4, from flop s to itself otherwise.

  posteriors_f64          float64, np.logaddexp.reduce: the reference value.
  posteriors_flappie_f32  the operation order of flappie's transpost_crf_flipflop + log_row_normalise_inplace in np.float32:
                          pairwise max + log1p(exp(-|d|)) in its sequence of sources, unscaled forward and backward
                          vectors (they grow by about 5 per block), the 40 entries of a block summed one after the other.
                          What a float32 implementation of the textbook order loses against float64: the error the GPU
                          kernels are measured against.
  posteriors_scaled_f32   the same order, the same pairwise folds and the same 40-entry normalisation in np.float32, with the
                          textbook per-step rescaling: the maximum of the previous forward (backward) vector is taken off it
                          before each forward (backward) step -- a constant per block that the normalisation removes -- so the
                          values stay those of a few scores and the error does not grow with the read.  The tight yardstick
                          for long reads.  It is not a restatement of the kernels (those take the maximum of the candidates,
                          one expf per candidate and one logf per state); it must not become one.

All work on a batch: a list of [nblk_i, 40] arrays, processed together (one numpy operation per step for all reads).
"""
import numpy as np

FROM = np.array([i % 8 for i in range(32)] + list(range(8)))
TO = np.array([i // 8 for i in range(32)] + [4, 5, 6, 7, 4, 5, 6, 7])


def _stack(scores, dtype):
    scores = [np.asarray(s, dtype=np.float32).reshape(-1, 40) for s in scores]
    lens = np.array([s.shape[0] for s in scores], dtype=np.int64)
    n = int(lens.max()) if len(scores) else 0
    x = np.zeros((len(scores), n, 40), dtype)
    for i, s in enumerate(scores):
        x[i, :s.shape[0]] = s
    return x, lens


def _unstack(post, lens):
    return [post[i, :int(n)].copy() for i, n in enumerate(lens)]


def posteriors_f64_batch(scores):
    x, lens = _stack(scores, np.float64)
    R, n, _ = x.shape
    with np.errstate(all="ignore"):
        alpha = np.zeros((R, n + 1, 8))
        for t in range(n):
            cand = x[:, t, :] + alpha[:, t, FROM]                  # [R, 40]
            nxt = np.empty((R, 8))
            nxt[:, :4] = np.logaddexp.reduce(cand[:, :32].reshape(R, 4, 8), axis=2)
            nxt[:, 4:] = np.logaddexp(cand[:, 36:40], cand[:, 32:36])
            alpha[:, t + 1] = nxt
        post = np.zeros_like(x)
        beta = np.zeros((R, 8))
        for t in range(n, 0, -1):
            beta = np.where((t < lens)[:, None], beta, 0.0)       # a read's backward vector starts at its own end
            e = x[:, t - 1, :] + beta[:, TO]
            p = alpha[:, t - 1, FROM] + e
            post[:, t - 1] = p - np.logaddexp.reduce(p, axis=1, keepdims=True)
            nb = np.empty((R, 8))
            flips = np.logaddexp.reduce(e[:, :32].reshape(R, 4, 8), axis=1)      # over the flip targets, per source
            nb[:] = np.logaddexp(flips, e[:, 32:40])
            beta = nb
    return _unstack(post, lens)


def posteriors_f64(scores):
    return posteriors_f64_batch([scores])[0]


def _lse32(a, b):
    """fmaxf(x, y) + log1pf(expf(-fabsf(x - y))), every operation rounded to float32.  expf and log1pf are evaluated in
    float64 and rounded once: glibc's expf is correctly rounded in all but a handful of arguments and its log1pf stays
    below one unit, while numpy's own float32 exp is a SIMD kernel of up to 2.5 units whose bits depend on the CPU it
    dispatches to.  With numpy's float32 functions here, 31 of 20 520 entries of a 513-block read differed from the
    compiled flappie and the all-zero 9-block case came out 26 % further from float64 than flappie is; evaluated this way,
    2 entries of all recorded cases differ (tests/test_flappie_pin.py)."""
    f, d = np.float32, np.float64
    e = np.exp((-np.abs((a - b).astype(f))).astype(d)).astype(f)
    return (np.maximum(a, b) + np.log1p(e.astype(d)).astype(f)).astype(f)


def posteriors_flappie_f32_batch(scores):
    f = np.float32
    x, lens = _stack(scores, f)
    R, n, _ = x.shape
    with np.errstate(all="ignore"):
        fwd = np.zeros((R, n + 1, 8), f)
        for t in range(n):
            prev = fwd[:, t]
            cur = np.empty((R, 8), f)
            # flop: stay, then the move from flip
            cur[:, 4:] = _lse32((prev[:, 4:] + x[:, t, 36:40]).astype(f), (prev[:, :4] + x[:, t, 32:36]).astype(f))
            # flip: source 0, then sources 1..7 folded in one at a time
            tf = x[:, t, :32].reshape(R, 4, 8)
            acc = (tf[:, :, 0] + prev[:, None, 0]).astype(f)
            for s in range(1, 8):
                acc = _lse32(acc, (tf[:, :, s] + prev[:, None, s]).astype(f))
            cur[:, :4] = acc
            fwd[:, t + 1] = cur
        post = np.zeros_like(x)
        back = np.zeros((R, 8), f)
        for t in range(n, 0, -1):
            back = np.where((t < lens)[:, None], back, f(0))
            xt = x[:, t - 1]
            a = fwd[:, t - 1]
            tp = np.empty((R, 40), f)
            # (fwd + prev) + trans, left to right
            tp[:, :32] = ((a[:, None, :] + back[:, :4, None]).astype(f) + xt[:, :32].reshape(R, 4, 8)).astype(f).reshape(R, 32)
            tp[:, 36:40] = ((a[:, 4:] + back[:, 4:]).astype(f) + xt[:, 36:40]).astype(f)
            tp[:, 32:36] = ((a[:, :4] + back[:, 4:]).astype(f) + xt[:, 32:36]).astype(f)
            # backward vector: the flop terms first, then the flip targets 0..3 folded in one at a time
            cur = np.empty((R, 8), f)
            cur[:, 4:] = (back[:, 4:] + xt[:, 36:40]).astype(f)
            cur[:, :4] = (back[:, 4:] + xt[:, 32:36]).astype(f)
            for b in range(4):
                cur = _lse32(cur, (xt[:, b * 8:b * 8 + 8] + back[:, b, None]).astype(f))
            back = cur
            post[:, t - 1] = tp
        # log_row_normalise_inplace: the 40 entries of a block one after the other (all blocks at once)
        tot = post[:, :, 0].copy()
        for i in range(1, 40):
            tot = _lse32(tot, post[:, :, i])
        post = (post - tot[:, :, None]).astype(f)
    return _unstack(post, lens)


def posteriors_flappie_f32(scores):
    return posteriors_flappie_f32_batch([scores])[0]


def posteriors_scaled_f32_batch(scores):
    f = np.float32
    x, lens = _stack(scores, f)
    R, n, _ = x.shape
    with np.errstate(all="ignore"):
        fwd = np.zeros((R, n, 8), f)                                 # the rescaled vector before block t
        cur = np.zeros((R, 8), f)
        for t in range(n):
            prev = (cur - cur.max(axis=1, keepdims=True)).astype(f)
            fwd[:, t] = prev
            cur = np.empty((R, 8), f)
            cur[:, 4:] = _lse32((prev[:, 4:] + x[:, t, 36:40]).astype(f), (prev[:, :4] + x[:, t, 32:36]).astype(f))
            tf = x[:, t, :32].reshape(R, 4, 8)
            acc = (tf[:, :, 0] + prev[:, None, 0]).astype(f)
            for s in range(1, 8):
                acc = _lse32(acc, (tf[:, :, s] + prev[:, None, s]).astype(f))
            cur[:, :4] = acc
        post = np.zeros_like(x)
        back = np.zeros((R, 8), f)
        for t in range(n, 0, -1):
            back = np.where((t < lens)[:, None], back, f(0))
            back = (back - back.max(axis=1, keepdims=True)).astype(f)
            xt = x[:, t - 1]
            a = fwd[:, t - 1]
            tp = np.empty((R, 40), f)
            tp[:, :32] = ((a[:, None, :] + back[:, :4, None]).astype(f) + xt[:, :32].reshape(R, 4, 8)).astype(f).reshape(R, 32)
            tp[:, 36:40] = ((a[:, 4:] + back[:, 4:]).astype(f) + xt[:, 36:40]).astype(f)
            tp[:, 32:36] = ((a[:, :4] + back[:, 4:]).astype(f) + xt[:, 32:36]).astype(f)
            cur = np.empty((R, 8), f)
            cur[:, 4:] = (back[:, 4:] + xt[:, 36:40]).astype(f)
            cur[:, :4] = (back[:, 4:] + xt[:, 32:36]).astype(f)
            for b in range(4):
                cur = _lse32(cur, (xt[:, b * 8:b * 8 + 8] + back[:, b, None]).astype(f))
            back = cur
            post[:, t - 1] = tp
        tot = post[:, :, 0].copy()
        for i in range(1, 40):
            tot = _lse32(tot, post[:, :, i])
        post = (post - tot[:, :, None]).astype(f)
    return _unstack(post, lens)


def posteriors_scaled_f32(scores):
    return posteriors_scaled_f32_batch([scores])[0]


def brute_force(scores):
    """every one of the 8^(n+1) state sequences of a tiny example, in float64"""
    import itertools
    x = np.asarray(scores, dtype=np.float64).reshape(-1, 40)
    n = x.shape[0]
    idx = {}
    for i in range(40):
        idx[(int(FROM[i]), int(TO[i]))] = i
    w = np.zeros((n, 40))
    total = 0.0
    for path in itertools.product(range(8), repeat=n + 1):
        steps = [idx.get((path[t], path[t + 1])) for t in range(n)]
        if None in steps:
            continue
        p = np.exp(sum(x[t, i] for t, i in enumerate(steps)))
        total += p
        for t, i in enumerate(steps):
            w[t, i] += p
    return np.log(w / total)
