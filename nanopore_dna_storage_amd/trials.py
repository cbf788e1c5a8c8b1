"""Reading-cost trials (DESIGN.md section 1, row N4'): how often the outer code recovers the file from a random sample
of the reads, for several sample sizes at once.  This file is the definition in numpy -- which reads a trial draws and in
which order, and what a trial is -- and the call into the device path (lva_rs_trials, csrc/tr_kernels.hip), which is held
to reference_trials bit for bit (tests/test_gpu_trials.py).  Nothing above run_trials touches a GPU unless rs_decode does.

Order of a trial.  Trial t (a 32-bit trial number) orders the n read numbers by a permutation sigma_t of [0, n); the
sample of size u is sigma_t(0) .. sigma_t(u - 1) in that order (the vote breaks ties by who came first), so the samples
of one trial are nested.  sigma_t is a keyed Feistel network with cycle walking:

  h = max(1, ceil(ceil(log2 n) / 2)) bits per half, domain D = 4^h >= n (and D < 4 n: fewer than 4 passes on average)
  one pass E_t(x):  l, r = x >> h, x & (2^h - 1);  for i = 0 .. 7:  l, r = r, l ^ (F(t, i, r) & (2^h - 1));  -> l << h | r
  F(t, i, r) = word 0 of Philox4x32-10 under the 64-bit seed, counter (r, i, t, 5)      (stream 5 of the table in DESIGN.md)
  sigma_t(j):      x = j;  do x = E_t(x) while x >= n
  sigma_t^-1(q):   the same walk with E_t^-1;  read q is in the sample of size u iff sigma_t^-1(q) < u

A trial at sample size u.  The sample's reads in order, those with index >= 0 kept (`passed` of them), rs_code.consensus
over their (index, payload) in that order (`present` indices get a vote), then rs_code.MainDecoder: absent oligos are
erasures, a column the decoder gives up on is ASCII '0'.  success = present > 0 and the first len(original) bytes of the
joined data payloads equal original; columns_ok = the columns the decoder did not give up on, 0 when present = 0 (where
the reference dies in MainDecoder).
"""
import numpy as np

from . import rs_code
from ._lib import check, load_library
from .philox import STREAM_TRIAL, philox

ROUNDS = 8
MAX_POINTS = 64
STAT_FIELDS = ("passed", "present", "columns_ok", "success")


def half_bits(n):
    """h: bits per half of the Feistel network over [0, n)"""
    return max(1, ((int(n) - 1).bit_length() + 1) // 2)


def _round_table(seed, ts, n):
    """F(t, i, r) & (2^h - 1) for every t in ts, round i and half r: int64 [len(ts), ROUNDS, 2^h].  (A pass looks F up
    at 2^h <= 2 sqrt(2 n) different r only; the device computes the same words where it needs them.)"""
    h = half_bits(n)
    ts = np.asarray(ts, dtype=np.uint64).reshape(-1)
    w = philox(np.arange(1 << h)[None, None, :], np.arange(ROUNDS)[None, :, None], ts[:, None, None], STREAM_TRIAL,
               int(seed) & 0xFFFFFFFFFFFFFFFF)[..., 0]
    return (w & np.uint32((1 << h) - 1)).astype(np.int64), h


def _pass(tab, h, ti, x, inverse):
    """E_t (or its inverse) of x, element k under trial row ti[k] of the table"""
    l, r = x >> h, x & ((1 << h) - 1)
    if inverse:
        for i in range(ROUNDS - 1, -1, -1):
            l, r = r ^ tab[ti, i, l], l
    else:
        for i in range(ROUNDS):
            l, r = r, l ^ tab[ti, i, r]
    return (l << h) | r


def _walk(seed, ts, n, inverse):
    """sigma_t (or its inverse) of every element of [0, n), for every t in ts: int64 [len(ts), n]"""
    if not 1 <= n < 1 << 31:
        raise ValueError("n must be in [1, 2^31)")
    tab, h = _round_table(seed, ts, n)
    T = tab.shape[0]
    ti = np.repeat(np.arange(T), n)
    x = _pass(tab, h, ti, np.tile(np.arange(n, dtype=np.int64), T), inverse)
    todo = np.nonzero(x >= n)[0]
    while len(todo):
        x[todo] = _pass(tab, h, ti[todo], x[todo], inverse)
        todo = todo[x[todo] >= n]
    return x.reshape(T, n)


def trial_orders(seed, ts, n):
    """sigma_t for several trial numbers at once: int64 [len(ts), n]"""
    return _walk(seed, ts, n, False)


def trial_places(seed, ts, n):
    """sigma_t^-1 for several trial numbers at once: int64 [len(ts), n]"""
    return _walk(seed, ts, n, True)


def trial_order(seed, t, n):
    """sigma_t as an array: entry j = the read number at place j of trial t"""
    return _walk(seed, [t], n, False)[0]


def trial_place(seed, t, n):
    """sigma_t^-1 as an array: entry q = the place of read number q in trial t"""
    return _walk(seed, [t], n, True)[0]


def _arguments(index, payload, original, bytes_per_oligo, num_oligos_RS, num_oligos, reads_to_use, num_trials, first_trial):
    index = np.ascontiguousarray(index, dtype=np.int32)
    payload = np.ascontiguousarray(payload, dtype=np.uint8)
    if index.ndim != 1 or payload.shape != (len(index), bytes_per_oligo):
        raise ValueError("index must be [n] and payload [n, bytes_per_oligo]")
    points = np.ascontiguousarray(np.atleast_1d(reads_to_use), dtype=np.int32)
    if points.ndim != 1 or not 1 <= len(points) <= MAX_POINTS:
        raise ValueError("reads_to_use: 1..%d sample sizes" % MAX_POINTS)
    if (np.diff(points) < 0).any() or (len(index) and (points[0] < 0 or points[-1] > len(index))):
        raise ValueError("reads_to_use: ascending, within [0, number of reads]")
    if num_trials < 0 or first_trial < 0 or first_trial + num_trials > 1 << 32:
        raise ValueError("trial numbers are 32-bit")
    if bytes_per_oligo < 2 or bytes_per_oligo % 2 or not 1 <= num_oligos_RS < num_oligos:
        raise ValueError("bytes_per_oligo even and >= 2, 1 <= num_oligos_RS < num_oligos")
    if not 1 <= len(original) <= (num_oligos - num_oligos_RS) * bytes_per_oligo:
        raise ValueError("original: 1 .. (num_oligos - num_oligos_RS) * bytes_per_oligo bytes")
    return index, payload, points


def reference_trials(index, payload, original, bytes_per_oligo, num_oligos_RS, num_oligos, reads_to_use, num_trials, seed,
                     first_trial=0, rs_decode=rs_code.MainDecoder, return_consensus=False):
    """The definition, one trial at a time through the existing functions.  index int32 [n] / payload uint8 [n, bytes_per_oligo]:
    list_ops.filter_lists' outputs for all n read numbers (-1: no list, or no entry passed); reads_to_use: K ascending sample
    sizes; trials first_trial .. first_trial + num_trials - 1.  rs_decode(reads, redundancy, total, return_ok=True) ->
    (payloads, ok per column): rs_code.MainDecoder, or a CPU stand-in.
    -> int32 [K, num_trials, 4] = (passed, present, columns_ok, success); with return_consensus also the vote's result,
    present uint8 [K, num_trials, num_oligos] and payload uint8 [K, num_trials, num_oligos, bytes_per_oligo] (zeros: absent)."""
    index, payload, points = _arguments(index, payload, original, bytes_per_oligo, num_oligos_RS, num_oligos, reads_to_use,
                                        num_trials, first_trial)
    original = bytes(original)
    K, n = len(points), len(index)
    stats = np.zeros((K, num_trials, 4), np.int32)
    c_present = np.zeros((K, num_trials, num_oligos), np.uint8)
    c_payload = np.zeros((K, num_trials, num_oligos, bytes_per_oligo), np.uint8)
    rows = [payload[q].tobytes() for q in range(n)]
    for j in range(num_trials if n else 0):
        order = trial_order(seed, first_trial + j, n)
        for k, u in enumerate(points):
            decoded = [(int(index[q]), rows[q]) for q in order[:u] if index[q] >= 0]
            cons = rs_code.consensus(decoded)
            for x, p in cons:
                c_present[k, j, x] = 1
                c_payload[k, j, x] = np.frombuffer(p, np.uint8)
            if not cons:
                continue
            dec, ok = rs_decode(cons, num_oligos_RS, num_oligos, return_ok=True)
            stats[k, j] = (len(decoded), len(cons), int(np.sum(ok)), int(b"".join(dec)[:len(original)] == original))
    return (stats, c_present, c_payload) if return_consensus else stats


def run_trials(index, payload, original, bytes_per_oligo, num_oligos_RS, num_oligos, reads_to_use, num_trials, seed,
               first_trial=0, device=0, chunk_trials=0, return_consensus=False):
    """reference_trials on the device, all sample sizes and all trials in one call (lva_rs_trials): the same integers.
    chunk_trials: trials per pass over the device buffers, 0 = as many as fit 1 GiB; the result does not depend on it."""
    index, payload, points = _arguments(index, payload, original, bytes_per_oligo, num_oligos_RS, num_oligos, reads_to_use,
                                        num_trials, first_trial)
    orig = np.frombuffer(bytes(original), np.uint8)
    K = len(points)
    stats = np.zeros((K, num_trials, 4), np.int32)
    c_present = np.zeros((K, num_trials, num_oligos), np.uint8) if return_consensus else None
    c_payload = np.zeros((K, num_trials, num_oligos, bytes_per_oligo), np.uint8) if return_consensus else None
    check(load_library().lva_rs_trials(device, index.ctypes.data, payload.ctypes.data, len(index), bytes_per_oligo, num_oligos,
                                        num_oligos_RS, orig.ctypes.data, len(orig), points.ctypes.data, K,
                                        int(seed) & 0xFFFFFFFFFFFFFFFF, first_trial, num_trials, chunk_trials, stats.ctypes.data,
                                        c_present.ctypes.data if return_consensus else None,
                                        c_payload.ctypes.data if return_consensus else None))
    return (stats, c_present, c_payload) if return_consensus else stats
