"""The read simulator's definition in numpy: message -> oligo -> strand -> channel -> flip-flop path
and dwells -> transition scores, every draw a word of a counter-based generator, so that a read depends on (seed, read number)
alone.  csrc/sim_kernels.hip computes the same on the device and is held to this file bit for bit (tests/test_gpu_simulate.py);
nothing here touches a GPU.

Generator: Philox4x32-10, key = the 64-bit seed (low word, high word), counter = (item, sub, read number, stream).  A
probability p takes part only as `word < floor(p * 2^32)`; no floating-point number is compared in any decision.

stream 0, message   item = i >> 7: bit i of the message is bit (i & 31) of word (i >> 5) & 3.
stream 1, channel   item = source position i in 0..n, sub 0 -> A, sub 1 -> B.  Insertions: the leading k in 0..3 with
                    A[k] < ins, inserted base k = bits 2k, 2k+1 of B[0].  Then for i < n: deleted if B[1] < del, else
                    substituted if B[2] < sub by base (s + 1 + mulhi(B[3], 3)) & 3, else the base itself
                    (helper.simulate_indelsubs: insertion loop, then deletion, then substitution; at most 4 insertions).
stream 2, dwell     item = j >> 2: emitted base j takes word j & 3; extra blocks d = the first d with word < dwell_cdf[d], else K.
stream 3, noise     item = block t of the read, sub = 2 * quad + h (quad = entry >> 2, h = 0, 1): entry 4 * quad + 2 * h + r sums
                    the four 16-bit halves of words 2r and 2r + 1.
stream 4, lead and flanks   item 0: word 0 -> the leading block's state (first + 1 + mulhi(word, 3)) & 3, words 1 and 2 -> the
                    lengths of the 5' and 3' flank, lo + mulhi(word, hi - lo + 1); item 1 + (i >> 6): the flank base at strand
                    position i (before the reverse complement) is bits 2 (i & 15).. of word (i >> 4) & 3.
stream 6, source    only with a pool (reference_reads(pool=...): the read's message is one of n_pool given messages instead of
                    stream 0's).  item 0, sub 0: word 0 -> the pool entry, src = mulhi(word, n_pool), or with pool_cdf (uint32
                    [n_pool], non-decreasing, last entry 0xFFFFFFFF: weights_to_cdf) the first k with word < pool_cdf[k], else
                    n_pool - 1 -- an entry equal to its predecessor is never drawn; word 1 -> rc_mode 3, the strand is
                    reverse-complemented iff word >> 31.  Every other draw of the read is what it is without a pool.
"""
import math

import numpy as np

from .decoder import code_info, encode
from .philox import STREAM_CHANNEL, STREAM_DWELL, STREAM_LEAD, STREAM_MESSAGE, STREAM_NOISE, STREAM_SOURCE, philox
from .synth import SCORE_CLIP, bases_from_str

MAX_PROB = 0.25             # every channel probability; the insertion loop stops after MAX_INS bases
MAX_INS = 4
MAX_DWELL_TABLE = 64
MAX_FLANK = 256
MAX_STRAND = 1024           # flanks + barcodes + oligo
MAX_POOL = 1 << 24          # messages of a pool; n_pool * msg_len < 2^31
_U32 = 0xFFFFFFFF


def threshold(p):
    """floor(p * 2^32) of a channel probability, the only form in which it is used"""
    if not 0.0 <= p <= MAX_PROB:
        raise ValueError("channel probability %r outside [0, %g]" % (p, MAX_PROB))
    return int(math.floor(p * 4294967296.0))


def poisson_dwell_cdf(mean=3.4, entries=24):
    """uint32 [entries]: floor(P(Poisson(mean) <= d) * 2^32), float64, for the inversion of the extra dwell"""
    pmf, cdf, out = math.exp(-mean), 0.0, []
    for d in range(entries):
        cdf += pmf
        out.append(min(int(math.floor(cdf * 4294967296.0)), _U32))
        pmf = pmf * mean / (d + 1)
    return np.array(out, dtype=np.uint32)


def weights_to_cdf(weights):
    """uint32 [n_pool]: floor(P(entry <= k) * 2^32) of non-negative weights, float64, the last entry 0xFFFFFFFF: the pool_cdf
    by which a read's pool entry is drawn.  A weight of 0 repeats its predecessor's entry: never drawn."""
    w = np.asarray(weights, dtype=np.float64)
    if w.ndim != 1 or len(w) < 1 or not np.isfinite(w).all() or (w < 0).any() or not w.sum() > 0:
        raise ValueError("weights: at least one, finite, none negative, not all zero")
    c = np.minimum(np.floor(np.cumsum(w) / w.sum() * 4294967296.0), float(_U32)).astype(np.uint32)
    c[-1] = _U32
    return c


def pool_arrays(pool, msg_len, pool_cdf=None):
    """a pool as both sides take it -> (uint8 [n_pool, msg_len] of 0/1, uint32 [n_pool] | None), or ValueError"""
    pool = np.ascontiguousarray(pool, dtype=np.uint8)
    if pool.ndim != 2 or pool.shape[1] != msg_len or not 1 <= len(pool) <= MAX_POOL or len(pool) * msg_len >= 1 << 31:
        raise ValueError("pool: uint8 [n_pool, msg_len], 1 <= n_pool <= 2^24, n_pool * msg_len < 2^31")
    if pool.max() > 1:
        raise ValueError("pool: bits 0 / 1")
    if pool_cdf is None:
        return pool, None
    cdf = np.ascontiguousarray(pool_cdf, dtype=np.uint32)
    if cdf.shape != (len(pool),) or (np.diff(cdf.astype(np.int64)) < 0).any() or int(cdf[-1]) != _U32:
        raise ValueError("pool_cdf: uint32 [n_pool], non-decreasing, last entry 0xFFFFFFFF")
    return pool, cdf


def call_parameters(msg_len, pool, pool_cdf, kw):
    """parameters(**kw) of a call that may have a pool -> (q, pool, pool_cdf).  parameters() keeps refusing rc_mode 3, which
    only a pool's draw can serve: with a pool the mode is judged here."""
    if pool is None:
        if pool_cdf is not None:
            raise ValueError("pool_cdf without a pool")
        return parameters(**kw), None, None
    kw = dict(kw)
    mode = kw.pop("rc_mode", 0)
    if mode not in (0, 1, 2, 3):
        raise ValueError("rc_mode: 0 = none, 1 = all, 2 = odd read numbers, 3 = a coin per read")
    return (dict(parameters(**kw), rc_mode=int(mode)),) + pool_arrays(pool, msg_len, pool_cdf)


def pool_draws(n, seed, first_read, n_pool, pool_cdf=None, rc_mode=0):
    """stream 6 of reads first_read .. first_read + n - 1 -> (source int32 [n], rc uint8 [n])"""
    if rc_mode not in (0, 1, 2, 3):
        raise ValueError("rc_mode: 0 = none, 1 = all, 2 = odd read numbers, 3 = a coin per read")
    R = first_read + np.arange(n, dtype=np.int64)
    W = philox(0, 0, R, STREAM_SOURCE, int(seed) & 0xFFFFFFFFFFFFFFFF).reshape(n, 4)
    if pool_cdf is None:
        src = _mulhi(W[:, 0], n_pool)
    else:
        src = np.minimum(np.searchsorted(np.asarray(pool_cdf, dtype=np.uint32), W[:, 0], side="right"), n_pool - 1)
    rc = [np.zeros(n, bool), np.ones(n, bool), (R & 1).astype(bool), (W[:, 1] >> np.uint32(31)).astype(bool)][rc_mode]
    return src.astype(np.int32), rc.astype(np.uint8)


def dwell_mean(dwell_cdf):
    """the mean extra dwell a table gives (d = len(table) where no entry is above the word)"""
    c = np.maximum.accumulate(np.concatenate([[0], np.asarray(dwell_cdf, dtype=np.float64)])) / 4294967296.0
    p = np.diff(np.concatenate([c, [1.0]]))
    return float((p * np.arange(len(p))).sum())


def score_scale(sigma):
    """float32(sigma * sqrt(3) / 65536): the sum of four uniform 16-bit halves has standard deviation 65536 / sqrt(3)"""
    return np.float32(sigma * math.sqrt(3.0) / 65536.0)


def parameters(sub=0.0, dele=0.0, ins=0.0, margin=6.0, sigma=1.5, clip=SCORE_CLIP, dwell_cdf=None, start_barcode=None,
               end_barcode=None, flank=(10, 40), rc_mode=0):
    """What both sides are handed, worked out once: thresholds, float32 scale / margin / clip, the dwell table, barcodes"""
    cdf = poisson_dwell_cdf() if dwell_cdf is None else np.ascontiguousarray(dwell_cdf, dtype=np.uint32)
    if cdf.ndim != 1 or not 1 <= len(cdf) <= MAX_DWELL_TABLE:
        raise ValueError("dwell_cdf: 1..%d uint32 entries" % MAX_DWELL_TABLE)
    if (start_barcode is None) != (end_barcode is None):
        raise ValueError("give both barcodes or neither")
    if rc_mode not in (0, 1, 2):
        raise ValueError("rc_mode: 0 = none, 1 = all, 2 = odd read numbers")
    if not float(clip) > 0.0:
        raise ValueError("clip must be positive")
    lo, hi = int(flank[0]), int(flank[1])
    if start_barcode is not None and not 0 <= lo <= hi <= MAX_FLANK:
        raise ValueError("flank: 0 <= lo <= hi <= %d" % MAX_FLANK)
    return dict(sub=threshold(sub), dele=threshold(dele), ins=threshold(ins), scale=score_scale(sigma), margin=np.float32(margin),
                clip=np.float32(clip), cdf=cdf, start_barcode=start_barcode, end_barcode=end_barcode, flank=(lo, hi),
                rc_mode=int(rc_mode))


def _transition_index(frm, to):
    return np.where(to < 4, to * 8 + frm, 32 + frm)


def _mulhi(w, k):
    return (w.astype(np.uint64) * np.uint64(k)) >> np.uint64(32)


def _read(R, key, oligo, q, rc=None):
    """read number R -> (emitted bases uint8, true transition index per block uint8); rc: the orientation where a pool's
    draw decided it, None: q's rc_mode"""
    L = philox(0, 0, R, STREAM_LEAD, key).astype(np.uint64)
    strand = oligo
    if q["start_barcode"] is not None:
        lo, hi = q["flank"]
        f5, f3 = lo + int(_mulhi(L[1], hi - lo + 1)), lo + int(_mulhi(L[2], hi - lo + 1))
        sb, eb = bases_from_str(q["start_barcode"]), bases_from_str(q["end_barcode"])
        n = f5 + len(sb) + len(oligo) + len(eb) + f3
        i = np.arange(n)
        words = philox(1 + np.arange((n + 63) // 64), 0, R, STREAM_LEAD, key).reshape(-1)
        strand = ((words[i >> 4] >> (2 * (i & 15)).astype(np.uint32)) & 3).astype(np.uint8)
        strand[f5:n - f3] = np.concatenate([sb, oligo, eb])
    if (q["rc_mode"] == 1 or (q["rc_mode"] == 2 and R & 1)) if rc is None else rc:
        strand = (3 - strand)[::-1]
    n = len(strand)
    if n > MAX_STRAND:
        raise ValueError("strand of %d bases (at most %d)" % (n, MAX_STRAND))
    # channel
    i = np.arange(n + 1)
    A, B = philox(i, 0, R, STREAM_CHANNEL, key), philox(i, 1, R, STREAM_CHANNEL, key)
    n_ins = np.cumprod(A < q["ins"], axis=1).sum(axis=1)
    s = np.concatenate([strand, [0]]).astype(np.uint64)
    own = np.where(B[:, 2] < q["sub"], (s + 1 + _mulhi(B[:, 3], 3)) & 3, s)
    keep = (B[:, 1] >= q["dele"]) & (i < n)
    cand = np.concatenate([(B[:, :1] >> (2 * np.arange(MAX_INS, dtype=np.uint32))[None, :]) & 3, own[:, None]], axis=1)
    mask = np.concatenate([np.arange(MAX_INS)[None, :] < n_ins[:, None], keep[:, None]], axis=1)
    em = cand[mask].astype(np.int64)
    nb = len(em)
    # flip-flop states (synth.state_path): a repeated base toggles flip <-> flop
    j = np.arange(nb)
    start = np.ones(nb, dtype=bool)
    start[1:] = em[1:] != em[:-1]
    run = np.maximum.accumulate(np.where(start, j, 0)) if nb else j
    st = em + 4 * ((j - run) & 1)
    lead = ((int(em[0]) if nb else 0) + 1 + int(_mulhi(L[0], 3))) & 3
    # dwell
    w = philox(np.arange((nb + 3) // 4), 0, R, STREAM_DWELL, key).reshape(-1)[:nb]
    below = w[:, None] < q["cdf"][None, :]
    d = np.where(below.any(axis=1), below.argmax(axis=1), len(q["cdf"])) if nb else np.zeros(0, np.int64)
    # true transitions (synth.true_transitions): a leading stay block, then per base one transition and d stays
    prev = np.concatenate([[lead], st[:-1]]) if nb else st
    body = np.repeat(_transition_index(st, st), 1 + d)
    body[np.cumsum(1 + d) - (1 + d)] = _transition_index(prev, st)
    true_idx = np.concatenate([[lead * 9], body]).astype(np.uint8)
    return em.astype(np.uint8), true_idx


def read_scores(R, key, true_idx, scale, margin, clip):
    """float32 [nblk, 40] of read number R: every operation a separately rounded float32 operation"""
    nblk = len(true_idx)
    P = philox(np.arange(nblk)[:, None], np.arange(20)[None, :], R, STREAM_NOISE, key)            # [nblk, 20, 4]
    s = ((P & 0xFFFF).astype(np.int32) + (P >> 16).astype(np.int32)).reshape(nblk, 20, 2, 2).sum(axis=3).reshape(nblk, 40)
    v = (s - 131070).astype(np.float32) * np.float32(scale)
    t = np.arange(nblk)
    v[t, true_idx] = v[t, true_idx] + np.float32(margin)
    return np.minimum(np.maximum(v, -np.float32(clip)), np.float32(clip)).astype(np.float32)


def reference_reads(mem_conv, rate, msg_len, n, seed, first_read=0, scores=True, pool=None, pool_cdf=None, **kw):
    """n reads, numbers first_read .. first_read + n - 1, of the (mem_conv, rate, msg_len) code under `seed`; the keywords
    are parameters()'s.  -> dict(msgs uint8 [n, msg_len], bases uint8 [sum], base_offsets int64 [n + 1], row_offsets int64
    [n + 1], true_idx uint8 [blocks], scores float32 [blocks, 40] (scores=False: absent)).
    pool (uint8 [n_pool, msg_len] of 0 / 1): every read's message is a pool entry drawn by stream 6, uniformly or by pool_cdf
    (weights_to_cdf); rc_mode may then be 3, a coin per read; the result gains source int32 [n] and rc uint8 [n]."""
    src = flip = None
    q, pool, pool_cdf = call_parameters(msg_len, pool, pool_cdf, kw)
    code_info(mem_conv, rate, msg_len)
    if n < 0 or first_read < 0 or first_read + n > 1 << 32:
        raise ValueError("read numbers are 32-bit")
    key = int(seed) & 0xFFFFFFFFFFFFFFFF
    if pool is None:
        msgs = np.zeros((n, msg_len), np.uint8)
        i = np.arange(msg_len)
        for r in range(n):
            words = philox(np.arange((msg_len + 127) // 128), 0, first_read + r, STREAM_MESSAGE, key).reshape(-1)
            msgs[r] = (words[i >> 5] >> (i & 31).astype(np.uint32)) & 1
        oligos = encode(mem_conv, rate, msg_len, msgs) if n else np.zeros((0, 0), np.uint8)
    else:
        src, flip = pool_draws(n, key, first_read, len(pool), pool_cdf, q["rc_mode"])
        msgs = pool[src]
        oligos = encode(mem_conv, rate, msg_len, pool)[src]        # every entry encoded once
    bases, idx = [], []
    for r in range(n):
        b, t = _read(first_read + r, key, oligos[r], q, None if flip is None else bool(flip[r]))
        bases.append(b)
        idx.append(t)
    base_off, row_off = np.zeros(n + 1, np.int64), np.zeros(n + 1, np.int64)
    base_off[1:] = np.cumsum([len(b) for b in bases])
    row_off[1:] = np.cumsum([len(t) for t in idx])
    out = dict(msgs=msgs, bases=np.concatenate(bases + [np.zeros(0, np.uint8)]), base_offsets=base_off, row_offsets=row_off,
               true_idx=np.concatenate(idx + [np.zeros(0, np.uint8)]))
    if pool is not None:
        out.update(source=src, rc=flip)
    if scores:
        out["scores"] = np.concatenate([read_scores(first_read + r, key, idx[r], q["scale"], q["margin"], q["clip"])
                                        for r in range(n)] + [np.zeros((0, 40), np.float32)], axis=0)
    return out
