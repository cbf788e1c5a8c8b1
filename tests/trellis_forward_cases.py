"""What the forward-score tests share (tests/test_trellis_forward_host.py, tests/test_gpu_trellis_forward.py): the three case
classes of rule (A) with their float64 values and float32 restatements (computed once, never changed), the error measure, the
single-path posteriors, and a float64 enumeration of the full flip-flop trellis.  numpy and the package only: no GPU."""
import functools

import numpy as np

from nanopore_dna_storage_amd import synth
from nanopore_dna_storage_amd import trellis_score as T

NEG = -np.inf
OFF = 1 << 12                                                # a max_deviation above every sequence here: the band is off


def err(got, want):
    """max |got - want| over all entries, in float64; both -inf counts as 0, one -inf and the other finite (or a NaN) as inf"""
    got, want = np.asarray(got, np.float64).reshape(-1), np.asarray(want, np.float64).reshape(-1)
    both = np.isneginf(got) & np.isneginf(want)
    with np.errstate(invalid="ignore"):
        d = np.where(both, 0.0, np.abs(got - want))
    d[np.isnan(d)] = np.inf
    return float(d.max()) if len(d) else 0.0


def wrong_message(msg, k):
    out = np.array(msg, np.uint8)
    out[(7 * k + 3) % len(out)] ^= 1
    return out


def _s1():
    """8 synthetic reads of the m = 11, r = 5, msg_len = 180 code, each paired with its true message and one wrong message,
    decoder band 20"""
    code = (11, 5, 180)
    reads = [synth.make_read(*code, 700 + i, margin=4.5, sub=0.01, dele=0.01, ins=0.005) for i in range(8)]
    msgs = np.array([x["msg"] for x in reads] + [wrong_message(x["msg"], i) for i, x in enumerate(reads)], np.uint8)
    pairs = [(i, i) for i in range(8)] + [(i, 8 + i) for i in range(8)]
    return dict(code=code, posts=[x["post"] for x in reads], msgs=msgs, seqs=list(T.message_bases(*code, msgs)), pairs=pairs, md=20)


def _s2():
    """sequences of 63, 64, 65 and 129 bases on reads of len + 2, 200 and 257 blocks, band off: the 64-lane pass boundaries"""
    rng = np.random.default_rng(41)
    seqs = [rng.integers(0, 4, n).astype(np.uint8) for n in (63, 64, 65, 129)]
    posts, pairs = [], []
    for s, seq in enumerate(seqs):
        for nblk in (len(seq) + 2, 200, 257):
            logits = rng.normal(0.0, 1.5, size=(nblk, 40))
            posts.append((logits - np.logaddexp.reduce(logits, axis=1, keepdims=True)).astype(np.float32))
            pairs.append((len(posts) - 1, s))
    return dict(posts=posts, seqs=seqs, pairs=pairs, md=OFF)


def _s3():
    """one sequence of 1024 bases on a read of 2 200 blocks, band 20 (the read goes on a little beyond the sequence, as a
    window cut from a longer read does)"""
    rng = np.random.default_rng(43)
    seq = rng.integers(0, 4, 1024 + 60).astype(np.uint8)
    post = synth.posteriors_from_bases(seq, rng, margin=4.5, mean_extra_dwell=1.1)
    assert post.shape[0] >= 2200
    return dict(posts=[np.ascontiguousarray(post[:2200])], seqs=[seq[:1024]], pairs=[(0, 0)], md=20)


@functools.lru_cache(maxsize=None)
def klass(name):
    """-> dict(posts, seqs, pairs, md, f64 [n_pairs, 2], f32 [n_pairs, 2], e_f32): a case class with the definition's value and
    its float32 restatement for every pair, and the restatement's error"""
    c = dict(S1=_s1, S2=_s2, S3=_s3)[name]()
    c["f64"] = np.array([T.reference_forward(c["posts"][r], c["seqs"][s], c["md"]) for r, s in c["pairs"]], np.float64)
    c["f32"] = np.array([T.reference_forward(c["posts"][r], c["seqs"][s], c["md"], dtype=np.float32) for r, s in c["pairs"]], np.float32)
    c["e_f32"] = err(c["f32"], c["f64"])
    return c


@functools.lru_cache(maxsize=None)
def narrow():
    """a 40-base sequence on a 90-block read for max_deviation 1 and 2: a band narrower than a pass, cells entering and leaving
    it at every block -- where never-cleared buffers and the cleared band part ways -> (post, seq)"""
    rng = np.random.default_rng(47)
    seq = rng.integers(0, 4, 40).astype(np.uint8)
    return np.ascontiguousarray(synth.posteriors_from_bases(seq, rng, margin=3.0, mean_extra_dwell=1.2)[:90]), seq


SINGLE_PATH_SIZES =((1, 3), (5, 17), (64, 66), (70, 100))   # (bases, blocks)


@functools.lru_cache(maxsize=None)
def single_path(n_bases, nblk, seed=5):
    """Posteriors that are -inf except along ONE path: the best path (band off) of a random sequence on a random read.  A
    transition index names its two states, a change of state is a step and no change a stay, so no other path of the sequence
    is finite.  -> dict(post, seq, score = reference_score's two values on `post`, end_state)"""
    rng = np.random.default_rng(seed + 1000 * n_bases + nblk)
    seq = rng.integers(0, 4, n_bases).astype(np.uint8)
    full = rng.normal(-3.0, 1.0, size=(nblk, 40)).astype(np.float32)
    tr = T.reference_trace(full, seq, OFF)
    assert tr["end_state"] >= 0 and tr["n_stale"] == 0
    at = T.positions_after(tr["enter"], nblk)
    post = np.full((nblk, 40), NEG, np.float32)
    state = int(tr["start_state"])
    for t in range(nblk):
        p = int(at[t])
        to = state if p == 0 else int(seq[p - 1]) + 4 * int(tr["kind"][p - 1])
        i = synth.transition_index(state, to)
        post[t, i] = full[t, i]
        state = to
    return dict(post=post, seq=seq, score=T.reference_score(post, seq, OFF), end_state=int(tr["end_state"]))


def brute_force(post, seq, max_deviation=None):
    """(flip, flop) in float64 by enumeration: the log-sum over every state sequence s_-1 .. s_(nblk - 1) of the full 8-state
    flip-flop trellis (any state -> flip b: entry b * 8 + s; flip s -> flop s + 4 and flop s -> itself: entry 32 + s) that
    spells `seq` -- a change of state calls the new state's base, no change calls nothing -- ending in a flip or in a flop.
    max_deviation: paths whose position (the bases called so far) leaves the band of any block are dropped."""
    post = np.asarray(post, np.float64).reshape(-1, 40)
    seq = [int(b) for b in seq]
    nblk, npos = len(post), len(seq) + 1
    bands = None if max_deviation is None else T.band_table(nblk, npos, max_deviation)
    ends = ([], [])

    def walk(t, state, p, w):
        if t == nblk:
            if p == npos - 1:
                ends[int(state >= 4)].append(w)
            return
        nxt = [(b, b * 8 + state) for b in range(4)]                   # into a flip
        nxt.append((state + 4, 32 + state) if state < 4 else (state, 32 + state))
        for to, i in nxt:
            q = p + (to != state)
            if q >= npos or (to != state and to % 4 != seq[q - 1]):
                continue
            if bands is not None and not bands[t, 0] <= q < bands[t, 1]:
                continue
            if post[t, i] == NEG:
                continue
            walk(t + 1, to, q, w + post[t, i])

    for s in range(8):
        walk(0, s, 0, 0.0)
    return tuple(float(np.logaddexp.reduce(e)) if e else NEG for e in ends)
