"""What a GIVEN message scores on a read: the reference trellis restricted to one message.

The decoder answers "which list_size messages score best on this read".  This stage answers the question that follows:
"what would this message have scored?" -- for a read whose list misses the truth it tells a list that was too short from a
band (max_deviation) that cut the truth's path off.

A path of decode_post_conv_parallel_LVA (viterbi_convolutional_code.cpp:589-858) that carries message M walks M's
convolutional states, so of the trellis only (position, flip-flop state) is left, and of the eight flip-flop states of a
position only two can be reached: flip b and flop b + 4 with b the base that M's oligo has there.  What remains is a chain of
single float32 additions and maxima over a band of positions -- a forced alignment of the read's posteriors to M's base
sequence under the decoder's band, the decoder's two parity buffers that are never cleared included (a position outside a
block's band keeps what it held two blocks earlier, and the reference reads it again when the band returns: the "stale band"
lists of tests/golden/m8_r3_L8_edge*).  Every score of a decoded list is one of the two values this returns for the listed
message, bit for bit (tests/test_trellis_score_host.py holds reference_score to the oracle on that).

  reference_score   the definition, plain numpy (this file is to csrc/sc_kernels.hip what read_map.py is to mp_kernels.hip;
                    the three kernels are one frame, csrc/sc_frame.h, under three cell rules -- the definitions stay three);
  message_bases     the base sequence that a decode with a given rc flag walks for a message;
  Decoder.score_bases / score_bases_resident / score_messages (decoder.py)   the same on the device, bit for bit;
  reference_trace   the definition of the traceback (csrc/st_kernels.hip): the best path of a sequence on a read, as the block
                    at which each position is entered; deviation_needed, left_band_at: what a band does to such a path;
  Decoder.trace_bases / trace_bases_resident / trace_messages   the same on the device, byte for byte;
  reference_forward the definition of the forward score (csrc/fw_kernels.hip): the same trellis with a log-sum-exp for every
                    maximum and every cell outside its block's band at -inf -- the log-weight of ALL alignments inside the
                    band; forward_total, list_posterior, forward_order: the posterior of a list's entries given the read;
  Decoder.forward_bases / forward_bases_resident / forward_messages   the same on the device, a float32 stage held to twice
                    the error of the definition's float32 restatement;
  verdicts, main    the use: why did the list of a read miss the truth, and which max_deviation would have kept it?
  list_rows         and: how much of the read's weight does each list entry hold, and which entry leads by likelihood?

    python -m nanopore_dna_storage_amd.trellis_score --simulate 2000 --seed 1 --mem_conv 11 --rate 5 --msg_len 180 \
        --list_size 8 --max_deviation 20 --out run        # -> run.truth.tsv and a summary line; --trace: run.trace.tsv too;
                                                          #    --forward: fwd_truth, fwd_first, fwd_best, conf_first too
"""
import argparse
import sys
from fractions import Fraction

import numpy as np

from . import decoder as _dec

VERDICTS = ("in_list", "list_too_short", "band", "short_read")      # the tool's, in the order of its summary line
NEG = np.float32(-np.inf)


def _band(t, nblk, npos, max_deviation):
    """[lo, hi) of block t (:677-679), as lva_band_table gives it for a code of npos positions: the centre is ONE fused
    multiply-subtract in double (the reference's build contracts it), truncated, clamped at 0; the end in uint32 arithmetic"""
    q = np.float64(t) / np.float64(nblk)
    centre = float(Fraction(float(q)) * npos - max_deviation)          # float(Fraction) rounds to nearest even, once
    lo = max(int(centre), 0)                                           # int() truncates toward zero, as the cast does
    hi = min((lo + 2 * max_deviation) & 0xFFFFFFFF, npos)
    return lo, hi


def band_table(nblk, npos, max_deviation):
    """int64 [nblk, 2]: the band of every block for a sequence of npos - 1 bases; for a code's own npos this is
    decoder.band_table(...)[0] (tests/test_trellis_score_host.py)"""
    return np.array([_band(t, nblk, npos, int(max_deviation)) for t in range(nblk)], dtype=np.int64).reshape(nblk, 2)


def _trellis_inputs(post, bases, max_deviation):
    """What the three definitions below start from, and what they refuse (ValueError): post as float32 [nblk, 40], the base
    codes, npos = len(bases) + 1, nblk, the posterior index of every state's stay at position 0, band_table"""
    post = np.ascontiguousarray(post, dtype=np.float32).reshape(-1, 40)
    seq = as_codes(bases)
    npos, nblk = len(seq) + 1, post.shape[0]
    if len(seq) < 1:
        raise ValueError("npos = len(bases) + 1, and at least one base")
    if nblk < npos + 1:
        raise ValueError("Too small post matrix: %d blocks for %d positions" % (nblk, npos))
    if np.isnan(post).any() or np.isposinf(post).any():
        raise ValueError("posteriors are finite or -inf")
    stay = np.array([k * 8 + k for k in range(4)] + [32 + k for k in range(4, 8)])
    return post, seq, npos, nblk, stay, band_table(nblk, npos, max_deviation)


def reference_score(post, bases, max_deviation, npos=None):
    """The two scores (flip, flop; float32) with which the reference trellis ends on the base sequence `bases` (uint8 codes
    0..3, or the characters ACGT) for a read of posteriors `post` (float32 [nblk, 40], .post layout).

    Restated from the reference's recurrence restricted to one base sequence, npos = len(bases) + 1 positions:
      buffers    two of [npos][8], all -inf; cur[0][k] = 0 for the eight states; the two swap at the start of every block;
                 a block updates the positions of its band only (band_table) and nothing is ever cleared;
      position 0 stays only: cur[0][k] = prev[0][k] + post[k * 8 + k] for a flip k, + post[32 + k] for a flop k;
      p > 0      with b = bases[p - 1]: flip b = max(prev[p][b] + post[b * 8 + b], prev[p - 1][s] + post[b * 8 + s] over every
                 s != b); flop b + 4 = max(prev[p][b + 4] + post[32 + b + 4], prev[p - 1][b] + post[32 + b]); the other six
                 states of the position stay -inf;
      result     (cur[npos - 1][b_last], cur[npos - 1][b_last + 4]) after the last block.
    Every addition is one float32 addition and every maximum is exact, so there is no order to choose.
    Refuses (ValueError) nblk < npos + 1 as the reference does ("Too small post matrix"), an empty sequence and a base code
    above 3.  Posteriors are finite or -inf: NaN and +inf are outside the definition (the reference's heap and its
    `!= -inf` tests give them a meaning that depends on the list size; tests/golden/*_nan*, *_posinf* pin the decoder there,
    not this function)."""
    given = npos
    post, seq, npos, nblk, stay, bands = _trellis_inputs(post, bases, max_deviation)
    if given is not None and given != npos:
        raise ValueError("npos = len(bases) + 1, and at least one base")
    buf = np.full((2, npos, 8), NEG, dtype=np.float32)
    buf[0, 0, :] = 0
    for t in range(nblk):
        prev, cur = buf[t & 1], buf[(t + 1) & 1]
        row = post[t]
        lo, hi = bands[t]
        for p in range(lo, hi):
            if p == 0:
                cur[0] = prev[0] + row[stay]
                continue
            b = int(seq[p - 1])
            flip = prev[p, b] + row[b * 8 + b]
            for s in range(8):
                if s != b:
                    flip = max(flip, prev[p - 1, s] + row[b * 8 + s])
            cur[p, b] = flip
            cur[p, b + 4] = max(prev[p, b + 4] + row[32 + b + 4], prev[p - 1, b] + row[32 + b])
    last = buf[nblk & 1, npos - 1]
    b = int(seq[-1])
    return np.float32(last[b]), np.float32(last[b + 4])


def reference_trace(post, bases, max_deviation, end=-1):
    """The best path of the base sequence `bases` on a read: reference_score's recurrence (same buffers, bands, float32
    additions, parity buffers that are never cleared) with, for every cell a block writes, the predecessor that won -- and
    the walk back from the last position after the last block.  The definition of csrc/st_kernels.hip.

    Tie rule: a later candidate replaces an earlier one only if it is strictly greater.  The candidates of a flip: the stay,
    then the states s of the position below, ascending; of a flop: the stay, then the step from the flip below; position 0
    only stays.
    Walk: from the last position, in flip (end = 0), flop (end = 1) or the larger of the two, flip on a tie (end = -1).
    With (t, p) the cell of position p after block t: p inside block t's band follows the recorded choice -- a stay to
    (t - 1, p), an entry to (t - 1, p - 1) in the recorded state; p outside the band holds what it held two blocks earlier:
    to (t - 2, p), one stale hop.  The walk ends at t = -1, at position 0 in one of the eight start states.
    -> dict(score = (flip, flop), reference_score's bits; enter int32 [len]: at [p - 1] the block whose transition moved the
    path into position p; kind uint8 [len]: 0 the position was entered and held as flip, 1 as flop; start_state 0..7;
    end_state 0 or 1; n_stale).  A chosen end score of -inf is no path: enter -1, kind 255, both states -1, n_stale 0.
    Refuses what reference_score refuses, and an end outside -1..1."""
    if end not in (-1, 0, 1):
        raise ValueError("end is 0 (flip), 1 (flop) or -1 (the larger)")
    post, seq, npos, nblk, stay, bands = _trellis_inputs(post, bases, max_deviation)
    buf = np.full((2, npos, 8), NEG, dtype=np.float32)
    buf[0, 0, :] = 0
    won = np.zeros((nblk, npos, 2), np.uint8)              # [t, p] = (flip: 0 stay, 1 + s from state s; flop: 0 stay, 1 step)
    for t in range(nblk):
        prev, cur = buf[t & 1], buf[(t + 1) & 1]
        row = post[t]
        lo, hi = bands[t]
        for p in range(lo, hi):
            if p == 0:
                cur[0] = prev[0] + row[stay]
                continue
            b = int(seq[p - 1])
            flip, choice = prev[p, b] + row[b * 8 + b], 0
            for s in range(8):
                if s != b:
                    v = prev[p - 1, s] + row[b * 8 + s]
                    if v > flip:
                        flip, choice = v, 1 + s
            flop, step = prev[p, b + 4] + row[32 + b + 4], prev[p - 1, b] + row[32 + b]
            won[t, p, 0] = choice
            if step > flop:
                flop, won[t, p, 1] = step, 1
            cur[p, b], cur[p, b + 4] = flip, flop
    last = buf[nblk & 1, npos - 1]
    b = int(seq[-1])
    score = (np.float32(last[b]), np.float32(last[b + 4]))
    k = int(score[1] > score[0]) if end < 0 else end
    out = dict(score=score, enter=np.full(npos - 1, -1, np.int32), kind=np.full(npos - 1, 255, np.uint8), start_state=-1,
               end_state=-1, n_stale=0)
    if score[k] == NEG:
        return out
    out["end_state"] = k
    t, p = nblk - 1, npos - 1
    while t >= 0:
        lo, hi = bands[t]
        if not lo <= p < hi:
            out["n_stale"] += 1
            t -= 2
            continue
        choice = int(won[t, p, k])
        if p > 0 and choice:
            out["enter"][p - 1], out["kind"][p - 1] = t, k
            state = int(seq[p - 1]) if k else choice - 1   # a flop is entered from the flip of the same base below
            if p == 1:
                out["start_state"] = state
            k = int(state >= 4)
            p -= 1
        t -= 1
    assert t == -1 and p == 0 and out["start_state"] >= 0    # a finite score has a path of finite cells back to the start
    return out


def _lse(f, *terms):
    """log-sum-exp of `terms` (arrays of dtype f, one shape) in their order: m + log(((e_1 + e_2) + ...) + e_k) with
    e_i = exp(x_i - m), m the largest term; -inf where every term is -inf.  Every subtraction, addition and maximum is rounded
    to f; exp and log are evaluated in float64 and rounded once (tests/transpost_ref.py, _lse32: numpy's float32 exp differs
    from CPU to CPU).  The largest term's e is exactly 1 and a term of -inf adds exactly 0."""
    with np.errstate(all="ignore"):
        m = terms[0]
        for x in terms[1:]:
            m = np.maximum(m, x)
        dead = np.isneginf(m)
        mm = np.where(dead, f(0), m)
        s = None
        for x in terms:
            e = np.exp((x - mm).astype(np.float64)).astype(f)
            s = e if s is None else s + e
        return np.where(dead, f(-np.inf), m + np.log(s.astype(np.float64)).astype(f))


def reference_forward(post, bases, max_deviation, dtype=np.float64):
    """The forward score (flip, flop) of the base sequence `bases` on a read: reference_score's trellis -- the same positions,
    states, transitions, posterior entries, start (the eight states of position 0 at 0) and band_table -- with two differences:
      sum for max   where reference_score takes the maximum of terms prev + post, this takes their log-sum-exp (_lse) in the
                    order: a flip at p >= 2 -- the stay, from flip b2 (if b2 != b), from flop b2 + 4; a flip at p = 1 -- the
                    stay, then the seven other states of position 0 ascending; a flop -- the stay, the step from flip b (if
                    b2 = b or p = 1).  Position 0 only stays: a plain addition;
      cleared band  a cell outside its block's band is -inf: when block t reads prev[p] or prev[p - 1], a position outside the
                    band of block t - 1 counts as -inf (for t = 0, prev is the initial state).  reference_score's buffers
                    that are never cleared belong to the reference's Viterbi decoder; a sum over paths that reads a value
                    of two blocks earlier again has no meaning.
    So the result is the log of the total weight of all alignments of the read to the sequence that stay inside the band at
    every block; with the band off (max_deviation >= npos) the plain forward algorithm.  The definition of
    csrc/fw_kernels.hip.  dtype float64 is the value; dtype float32 is the restatement the device is measured beside: the same
    term order with every addition, subtraction and maximum rounded to float32 (the kernel follows this order).
    Vectorised over the positions of a block: its cells depend on the block before alone.  Refuses what reference_score
    refuses.  -> two scalars of dtype."""
    f = np.dtype(dtype).type
    if f not in (np.float64, np.float32):
        raise ValueError("dtype is float64 (the value) or float32 (the restatement)")
    post, seq, npos, nblk, stay, bands = _trellis_inputs(post, bases, max_deviation)
    neg = f(-np.inf)
    post, seq, bands = post.astype(f), seq.astype(np.int64), bands.tolist()
    # per position p (index 0 unused): its base b, the base b2 below (p = 1 has none), and the posterior entries of its terms
    b = np.concatenate([[0], seq])
    b2 = np.concatenate([[0, 0], seq[:-1]])
    same = b2 == b
    i_stay, i_flip, i_flop, i_hold, i_step = b * 8 + b, b * 8 + b2, b * 8 + b2 + 4, 32 + b + 4, 32 + b
    b1 = int(seq[0])
    others = np.array([s for s in range(8) if s != b1])
    zero = np.zeros(8, f)                                   # position 0, every state
    flip, flop = np.full(npos, neg, f), np.full(npos, neg, f)    # [p] for p >= 1: flip b, flop b + 4; outside the band: -inf
    for t in range(nblk):
        row = post[t]
        lo, hi = bands[t]
        nzero, nflip, nflop = np.full(8, neg, f), np.full(npos, neg, f), np.full(npos, neg, f)
        if lo == 0 and hi > 0:
            nzero = zero + row[stay]
        if lo <= 1 < hi:                                    # p = 1: every state of position 0
            nflip[1] = _lse(f, flip[1] + row[b1 * 8 + b1], *(zero[others] + row[b1 * 8 + others]))
            nflop[1] = _lse(f, flop[1] + row[32 + b1 + 4], zero[b1] + row[32 + b1])
        a = max(lo, 2)
        if a < hi:
            p, q = slice(a, hi), slice(a - 1, hi - 1)       # the positions and the ones below
            below = flip[q]
            nflip[p] = _lse(f, flip[p] + row[i_stay[p]], np.where(same[p], neg, below) + row[i_flip[p]], flop[q] + row[i_flop[p]])
            nflop[p] = _lse(f, flop[p] + row[i_hold[p]], np.where(same[p], below, neg) + row[i_step[p]])
        zero, flip, flop = nzero, nflip, nflop
    return f(flip[npos - 1]), f(flop[npos - 1])


def forward_total(ff):
    """float64 [n]: logaddexp(flip, flop) per row of forward scores [n, 2] -- the forward score of the sequence"""
    ff = np.asarray(ff, dtype=np.float64).reshape(-1, 2)
    return np.logaddexp(ff[:, 0], ff[:, 1])


def list_posterior(totals):
    """exp(totals - logsumexp(totals)): the posterior of each entry of one read's list given the read, restricted to the list.
    Sums to 1; an entry with total -inf gets 0; all NaN if every total is -inf"""
    totals = np.asarray(totals, dtype=np.float64).reshape(-1)
    if not len(totals):
        return totals.copy()
    with np.errstate(invalid="ignore"):
        return np.exp(totals - np.logaddexp.reduce(totals))


def forward_order(totals):
    """the entry indices by total descending, list order on ties"""
    return np.argsort(-np.asarray(totals, dtype=np.float64).reshape(-1), kind="stable")


def positions_after(enter, nblk):
    """int64 [nblk]: the position p_t at which a path stands after block t -- the number of positions with enter <= t"""
    enter = np.asarray(enter, dtype=np.int64)
    return np.searchsorted(np.sort(enter), np.arange(nblk), side="right")


def band_contains(enter, nblk, max_deviation):
    """does the band of max_deviation hold the path at every block: lo(t) <= p_t < hi(t), npos = len(enter) + 1?"""
    bands = band_table(nblk, len(enter) + 1, max_deviation)
    at = positions_after(enter, nblk)
    return bool(((bands[:, 0] <= at) & (at < bands[:, 1])).all())


def deviation_needed(enter, nblk):
    """The smallest max_deviation D >= 1 whose band contains a path without stale hops (enter as reference_trace gives it, every
    entry >= 0).  Containment is monotone in D -- lo falls and hi rises with D -- and D = len(enter) + 1 contains every path
    (lo = 0, hi = npos): a bisection."""
    if len(enter) < 1 or np.min(enter) < 0:
        raise ValueError("a path enters every position")
    lo, hi = 1, len(enter) + 1                               # the answer is in [lo, hi]
    while lo < hi:
        mid = (lo + hi) // 2
        if band_contains(enter, nblk, mid):
            hi = mid
        else:
            lo = mid + 1
    return lo


def left_band_at(enter, nblk, max_deviation):
    """the first block at which the path lies outside the band of max_deviation, or -1"""
    bands = band_table(nblk, len(enter) + 1, max_deviation)
    at = positions_after(enter, nblk)
    out = np.flatnonzero((at < bands[:, 0]) | (at >= bands[:, 1]))
    return int(out[0]) if len(out) else -1


def as_codes(bases):
    """a base sequence as uint8 codes 0..3: codes, or the characters ACGT (str, bytes or their byte values)"""
    if isinstance(bases, str):
        bases = bases.encode("ascii")
    a = np.frombuffer(bases, dtype=np.uint8) if isinstance(bases, (bytes, bytearray)) else np.asarray(bases, dtype=np.uint8)
    a = a.reshape(-1).copy()
    for code, ch in enumerate(b"ACGT"):
        a[a == ch] = code
    if (a > 3).any():
        raise ValueError("a base is A, C, G, T or a code 0..3")
    return a


def message_bases(mem_conv, rate, msg_len, msgs, rc=False, sync_marker="", sync_period=0):
    """The base sequence that a decode with this rc flag walks for each message: uint8 [n, oligo_len] (or [oligo_len]).
    Forward it is encode().  A reverse-complement decode (:359-386: mirrored generators, complemented output bits, the
    message's bits consumed from the far end and written back reversed, :826-836) reads the other strand: the forward
    oligo reversed, every base complemented (3 - b) -- held to the oracle's lists on the _rc fixtures by
    tests/test_trellis_score_host.py.  The messages are given as decode() returns them, in encode()'s bit order, whatever rc.
    A sync marker does not change the sequence: its bits are part of the message (the decoder returns them in place), and
    the encoder treats them like any other; the arguments only check that the code exists."""
    _dec.code_info(mem_conv, rate, msg_len, rc, sync_marker, sync_period)
    fwd = _dec.encode(mem_conv, rate, msg_len, msgs)
    if not rc:
        return fwd
    return np.ascontiguousarray((3 - fwd)[..., ::-1])


# ---------------------------------------------------------------------------------------------------------------
# the use: why did a read's list miss the truth?
# ---------------------------------------------------------------------------------------------------------------

def verdict(rank, banded, unbanded, list_scores, list_size):
    """One read.  rank: place of the truth in the list or -1; banded, unbanded: max(flip, flop) of the truth under the
    decoder's band and with the band off (None, None: the read was too short to score); list_scores: the list's scores.
    The first that applies:
      short_read       the read has fewer blocks than the code's positions + 1: neither the decoder nor the score takes it;
      in_list          rank >= 0;
      band             the band cost the truth its path: the banded score is -inf, or below the unbanded one;
      list_too_short   the band changed nothing for the truth and it lost on score: a finite score, at most the last entry's
                       of a FULL list, so a longer list reaches it;
      band             what is left -- a finite score that a list with room to spare does not hold, or one above a full list's
                       last entry: an exact list decoder cannot lose such a message, only the band's buffers that are never
                       cleared can (a position outside the band keeps what it held), so the band decides here too."""
    if banded is None:
        return "short_read"
    if rank >= 0:
        return "in_list"
    if banded == NEG or banded < unbanded:
        return "band"
    if len(list_scores) == list_size and banded <= list_scores[-1]:
        return "list_too_short"
    return "band"


def truth_rank(msgs, truth):
    """place of `truth` (uint8 [msg_len]) among the rows of msgs (uint8 [count, msg_len]), or -1"""
    if isinstance(msgs, int) or len(msgs) == 0:
        return -1
    hit = np.flatnonzero((np.asarray(msgs) == np.asarray(truth, dtype=np.uint8)[None, :]).all(axis=1))
    return int(hit[0]) if len(hit) else -1


def _forward_totals(dec, dev, first_block, n_blocks, msgs_of, rc):
    """One forward_bases_resident call under the decoder's band over (read, message) pairs: msgs_of[i] the messages (uint8
    [k_i, msg_len], k_i may be 0) to weigh on read i, in the orientation of its rc flag -> [float64 [k_i]], forward_total of
    each.  A read with fewer blocks than the code's positions + 1 is not paired: its totals are empty."""
    n = len(msgs_of)
    sync = (dec._sync.decode() if dec._sync else "", dec._sync_period)
    info = _dec.code_info(dec.mem_conv, dec.rate, dec.msg_len, False, *sync)
    rc = np.zeros(n, bool) if rc is None else np.asarray(rc, dtype=bool)
    seqs, pairs, at = [], [], []
    for i in range(n):
        k = len(msgs_of[i]) if int(n_blocks[i]) >= info.nstate_pos + 1 else 0
        at.append((len(seqs), k))
        if k:
            enc = message_bases(dec.mem_conv, dec.rate, dec.msg_len, np.asarray(msgs_of[i], np.uint8), bool(rc[i]), *sync)
            pairs += [(i, len(seqs) + j) for j in range(k)]
            seqs += list(enc)
    if not pairs:
        return [np.zeros(0) for _ in range(n)]
    tot = forward_total(dec.forward_bases_resident(dev, first_block, n_blocks, seqs, pairs))
    return [tot[a:a + k] for a, k in at]


def _entries(res, msg_len):
    """the messages of a decode result as uint8 [count, msg_len]; an error code or an empty list: no rows"""
    msgs = () if isinstance(res, int) else res[0]
    return np.asarray(msgs, np.uint8).reshape(-1, msg_len) if len(msgs) else np.zeros((0, msg_len), np.uint8)


def _list_row(totals):
    return dict(totals=totals, posterior=list_posterior(totals), order=forward_order(totals))


def list_rows(dec, dev, first_block, n_blocks, results, rc):
    """The forward score of every entry of every decoded list, in ONE forward_bases_resident call over (read, entry) pairs on
    the buffer the decode read, under the decoder's band.  Per read -> dict(totals float64 [count]: forward_total of each
    entry; posterior: list_posterior(totals), the weight of each entry given the read, restricted to the list; order:
    forward_order(totals), the entries by likelihood).  A read whose decode returned an error code, an empty list or that is a
    short_read gets empty arrays."""
    tot = _forward_totals(dec, dev, first_block, n_blocks, [_entries(r, dec.msg_len) for r in results], rc)
    return [_list_row(t) for t in tot]


def truth_rows(dec, dev, first_block, n_blocks, results, truth_msgs, rc, forward=False):
    """The table of the tool for reads that are resident on the device (windows first_block / n_blocks of the buffer `dev`),
    their decode results and their true messages: two score_bases_resident calls on the buffer the decode read, one under the
    decoder's band and one with the band off, and one trace_bases_resident call with the band off -- where the truth's best
    path runs.  -> [dict(rank, banded, unbanded, first, last, verdict, dev_needed, left_band_at, trace)]: dev_needed the
    smallest max_deviation whose band holds that path (deviation_needed; nan for a short read and a truth without a path),
    left_band_at the first block at which the path lies outside the decoder's band or -1, trace = dict(start_state,
    end_state, enter) of the path or None.
    forward: one forward_bases_resident call more, over every list entry and the truth of every read under the decoder's
    band, and four keys more per row: fwd_truth (the truth's forward total; nan for a short read), fwd_first (the total of the
    list's first entry; nan for no list), fwd_best (the list place of the entry with the largest total, -1 for no list) and
    conf_first (the posterior of the first entry, list_posterior; nan for no list)."""
    n = len(results)
    sync = (dec._sync.decode() if dec._sync else "", dec._sync_period)
    info = _dec.code_info(dec.mem_conv, dec.rate, dec.msg_len, False, *sync)
    rc = np.zeros(n, bool) if rc is None else np.asarray(rc, dtype=bool)
    ok = [i for i in range(n) if int(n_blocks[i]) >= info.nstate_pos + 1]
    banded, unbanded, path = {}, {}, {}
    if ok:
        seqs = [message_bases(dec.mem_conv, dec.rate, dec.msg_len, truth_msgs[i], bool(rc[i]), *sync) for i in ok]
        pairs = [(i, k) for k, i in enumerate(ok)]
        a = dec.score_bases_resident(dev, first_block, n_blocks, seqs, pairs)
        off_band = dec.msg_len + dec.mem_conv + 1
        b = dec.score_bases_resident(dev, first_block, n_blocks, seqs, pairs, max_deviation=off_band)
        tr = dec.trace_bases_resident(dev, first_block, n_blocks, seqs, pairs, max_deviation=off_band)
        md = dec.max_deviation if dec.max_deviation is not None else off_band
        for k, i in enumerate(ok):
            banded[i], unbanded[i] = np.float32(a[k].max()), np.float32(b[k].max())
            if tr["end_state"][k] >= 0 and tr["n_stale"][k] == 0:
                enter, nblk = tr["enter"][k, :len(seqs[k])], int(n_blocks[i])
                path[i] = dict(dev_needed=deviation_needed(enter, nblk), left_band_at=left_band_at(enter, nblk, md),
                               trace=dict(start_state=int(tr["start_state"][k]), end_state=int(tr["end_state"][k]), enter=enter))
    rows = []
    for i, res in enumerate(results):
        msgs, scores = ((), ()) if isinstance(res, int) else res
        rank = truth_rank(msgs, truth_msgs[i])
        rows.append(dict(rank=rank, banded=banded.get(i), unbanded=unbanded.get(i),
                         first=float(scores[0]) if len(scores) else float("nan"),
                         last=float(scores[-1]) if len(scores) else float("nan"),
                         verdict=verdict(rank, banded.get(i), unbanded.get(i), scores, dec.list_size),
                         **path.get(i, dict(dev_needed=float("nan"), left_band_at=-1, trace=None))))
    if forward:                                              # the lists and the truths in one call: the truth last per read
        truth = np.asarray(truth_msgs, np.uint8).reshape(n, dec.msg_len)
        both = [np.concatenate([_entries(res, dec.msg_len), truth[i:i + 1]]) for i, res in enumerate(results)]
        for row, tot in zip(rows, _forward_totals(dec, dev, first_block, n_blocks, both, rc)):
            lst = _list_row(tot[:-1])
            have = len(lst["totals"]) > 0
            row.update(fwd_truth=float(tot[-1]) if len(tot) else float("nan"),
                       fwd_first=float(lst["totals"][0]) if have else float("nan"),
                       fwd_best=int(lst["order"][0]) if have else -1,
                       conf_first=float(lst["posterior"][0]) if have else float("nan"))
    return rows


def count_verdicts(rows):
    return {v: sum(r["verdict"] == v for r in rows) for v in VERDICTS}


def simulate_rows(dec, n, seed, first_read=0, forward=False, **kw):
    """Decoder.simulate_and_decode with the truth scored on the buffer the decode read, before it is freed: the reads never
    leave the device -> (truth, results, rows); forward: truth_rows' flag"""
    def after(dev, off, truth, results, rc):
        return truth_rows(dec, dev, off[:-1], np.diff(off), results, truth["msgs"], rc, forward=forward)
    return dec.simulate_and_decode(n, seed, first_read, after=after, **kw)


def write_table(rows, path):
    """P.truth.tsv: the seven columns of the scores, and after them dev_needed and left_band_at where the rows carry the trace
    of the truth (truth_rows' do), and after those fwd_truth, fwd_first, fwd_best and conf_first where the rows carry the forward
    scores (truth_rows(forward=True))"""
    traced = bool(rows) and all("dev_needed" in r for r in rows)
    fwd = bool(rows) and all("fwd_best" in r for r in rows)
    with open(path, "w") as f:
        f.write("read\trank\tbanded\tunbanded\tfirst\tlast\tverdict" + ("\tdev_needed\tleft_band_at" if traced else "")
                + ("\tfwd_truth\tfwd_first\tfwd_best\tconf_first" if fwd else "") + "\n")
        for i, r in enumerate(rows):
            sc = lambda v: "nan" if v is None else repr(float(v))
            f.write("%d\t%d\t%s\t%s\t%r\t%r\t%s" % (i, r["rank"], sc(r["banded"]), sc(r["unbanded"]), r["first"], r["last"],
                                                  r["verdict"]))
            if traced:
                f.write("\t%s\t%d" % ("nan" if r["dev_needed"] != r["dev_needed"] else "%d" % r["dev_needed"], r["left_band_at"]))
            if fwd:
                f.write("\t%r\t%r\t%d\t%r" % (r["fwd_truth"], r["fwd_first"], r["fwd_best"], r["conf_first"]))
            f.write("\n")


def write_trace(rows, path):
    """P.trace.tsv, one row per read: read, start_state, end_state and the block at which the truth's unbanded path enters each
    position, comma-separated (a read without a path: -1, -1 and nothing)"""
    with open(path, "w") as f:
        f.write("read\tstart_state\tend_state\tenter\n")
        for i, r in enumerate(rows):
            t = r.get("trace")
            f.write("%d\t%d\t%d\t%s\n" % ((i, t["start_state"], t["end_state"], ",".join(map(str, t["enter"].tolist()))) if t
                                        else (i, -1, -1, "")))


def band_dev_needed(rows):
    """the largest dev_needed among the reads with verdict band whose truth has a path (0: no such read): the max_deviation
    that would have kept every one of them"""
    need = [r["dev_needed"] for r in rows if r["verdict"] == "band" and r.get("dev_needed", float("nan")) == r.get("dev_needed")]
    return int(max(need)) if need else 0


def forward_counts(rows):
    """(reads whose list is led by another entry by forward total than by best path: fwd_best > 0; reads whose truth is in the
    list, not first by best path, and first by forward total: rank > 0 and fwd_best == rank) of rows that carry the forward
    scores"""
    return sum(r["fwd_best"] > 0 for r in rows), sum(r["rank"] > 0 and r["fwd_best"] == r["rank"] for r in rows)


def summary_line(rows, dev_needed=False, forward=False):
    """the count per verdict; dev_needed: and the largest dev_needed among the reads with verdict band (band_dev_needed);
    forward: and forward_counts"""
    c = count_verdicts(rows)
    line = "truth score: %d reads, " % len(rows) + ", ".join("%s %d" % (v, c[v]) for v in VERDICTS)
    line += ", band dev_needed %d" % band_dev_needed(rows) if dev_needed else ""
    return line + (", fwd_best != 0 %d, truth first by forward only %d" % forward_counts(rows) if forward else "")


def build_parser():
    p = argparse.ArgumentParser(description="Score the true message of every read on the decoder's trellis: why did a list miss it?")
    p.add_argument("--mem_conv", type=int, default=11)
    p.add_argument("--rate", type=int, default=5)
    p.add_argument("--msg_len", type=int, default=180)
    p.add_argument("--list_size", type=int, default=8)
    p.add_argument("--max_deviation", type=int, default=20)
    p.add_argument("--device", type=int, default=0)
    p.add_argument("--out", "-P", default="trellis_score", help="prefix P: the table goes to P.truth.tsv")
    p.add_argument("--simulate", type=int, default=0, metavar="N", help="N reads of the device simulator (Decoder.simulate)")
    p.add_argument("--seed", type=int, default=0)
    p.add_argument("--sub", type=float, default=None)
    p.add_argument("--dele", type=float, default=None)
    p.add_argument("--ins", type=float, default=None)
    p.add_argument("--trace", action="store_true",
                   help="also write P.trace.tsv (the truth's unbanded path per read: start_state, end_state, the block at which "
                        "each position is entered) and add the largest dev_needed among the band reads to the summary line")
    p.add_argument("--forward", action="store_true",
                   help="also weigh every list entry and the truth by ALL their alignments (the forward score): four columns "
                        "more in P.truth.tsv (fwd_truth, fwd_first, fwd_best, conf_first), and in the summary line the reads "
                        "with fwd_best != 0 and those whose truth is in the list, not first by best path, first by forward total")
    p.add_argument("--manifest", help="a text file, one read per line: <posterior file (.post)> <true message as 0/1> [rc: 0/1]")
    return p


def main(argv=None, out=sys.stdout):
    args = build_parser().parse_args(argv)
    if bool(args.manifest) == bool(args.simulate):
        raise SystemExit("give --manifest FILE or --simulate N")
    with _dec.Decoder(args.mem_conv, args.rate, args.msg_len, list_size=args.list_size, max_deviation=args.max_deviation,
                      device=args.device) as dec:
        if args.simulate:
            kw = {k: getattr(args, k) for k in ("sub", "dele", "ins") if getattr(args, k) is not None}
            _, _, rows = simulate_rows(dec, args.simulate, args.seed, forward=args.forward, **kw)
        else:
            posts, msgs, rc = [], [], []
            for ln in open(args.manifest):
                w = ln.split()
                if not w:
                    continue
                posts.append(np.fromfile(w[0], dtype="<f4").reshape(-1, 40))
                msgs.append(_dec.str_to_bits(w[1]))
                rc.append(len(w) > 2 and w[2] == "1")
            with dec.resident(posts) as (dev, off):
                results = dec.decode_resident(dev, off, rc)
                rows = truth_rows(dec, dev, off[:-1], np.diff(off), results, np.array(msgs, dtype=np.uint8), rc,
                                  forward=args.forward)
    write_table(rows, args.out + ".truth.tsv")
    if args.trace:
        write_trace(rows, args.out + ".trace.tsv")
    print(summary_line(rows, dev_needed=args.trace, forward=args.forward), file=out)
    return 0


if __name__ == "__main__":
    sys.exit(main())
