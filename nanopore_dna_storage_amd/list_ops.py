"""What happens to a decoded list, on the GPU (csrc/ls_kernels.hip through the C ABI's
lva_list_filter / lva_list_consensus / lva_list_stats).  Device counterparts of

  helper.decode_list_CRC_index (helper.py:371-388)            filter_lists
  rs_code.consensus (decode_RS_from_decoded_lists.py:37-51)   consensus
  the first-seen rule of helper.py:326-329                    consensus(..., first_only=True)
  the per-trial statistics of simulator.py:92-110             list_stats

on the dense arrays the decoder hands out -- msgs uint8 [n, list_size, msg_len] of 0/1 and counts int32 [n] -- with
lists_to_array / array_to_lists for the `list_<i>` files' lists of '0'/'1' strings.  Results are integers and equal the
host functions' exactly.  No CPU fallback: without the HIP library or a GPU the calls raise.
"""
import ctypes

import numpy as np

from . import _lib
from ._lib import check, load_library

STAT_FIELDS = ("top_correct", "list_correct", "hamming", "hamming8", "hamming16", "edit")
STAT_DTYPE = np.dtype([(k, np.int32) for k in STAT_FIELDS])


def bits_of(s):
    """'0'/'1' string -> uint8 array of 0/1"""
    a = np.frombuffer(s.encode("ascii"), dtype=np.uint8) - 48
    if a.size and a.max() > 1:
        raise ValueError("not a string of '0' and '1': %r" % (s,))
    return a


def lists_to_array(lists, msg_len=None, list_size=None):
    """lists: per read a list of '0'/'1' strings of one common length, best first (what a list_<i> file holds; a read
    without a list: an empty list).  -> (msgs uint8 [n, list_size, msg_len], counts int32 [n]); rows past a read's count
    are zero.  list_size: default the longest list (at least 1), longer lists are cut; msg_len: default the entries' length."""
    lists = [list(lst) for lst in lists]
    if list_size is None:
        list_size = max([len(lst) for lst in lists] + [1])
    if msg_len is None:
        msg_len = next((len(e) for lst in lists for e in lst), 1)
    msgs = np.zeros((len(lists), list_size, msg_len), np.uint8)
    counts = np.zeros(len(lists), np.int32)
    for i, lst in enumerate(lists):
        lst = lst[:list_size]
        if any(len(e) != msg_len for e in lst):
            raise ValueError("read %d: entries must have %d bits" % (i, msg_len))
        counts[i] = len(lst)
        if lst:
            msgs[i, :len(lst)] = bits_of("".join(lst)).reshape(len(lst), msg_len)
    return msgs, counts


def array_to_lists(msgs, counts):
    """the inverse of lists_to_array: -> per read the list of its first counts[i] entries as '0'/'1' strings"""
    msgs = np.asarray(msgs, dtype=np.uint8)
    out = []
    for i, c in enumerate(np.asarray(counts)):
        c = min(max(int(c), 0), msgs.shape[1])
        out.append([(msgs[i, k] + 48).tobytes().decode("ascii") for k in range(c)])
    return out


def results_to_array(results, list_size, msg_len):
    """what Decoder.decode returns -- per read (msgs [count, msg_len], scores) or a negative error code -- as the dense
    pair (msgs, counts); an error code stays in counts"""
    msgs = np.zeros((len(results), list_size, msg_len), np.uint8)
    counts = np.zeros(len(results), np.int32)
    for i, res in enumerate(results):
        if isinstance(res, (int, np.integer)):
            counts[i] = int(res)
        else:
            counts[i] = len(res[0])
            msgs[i, :len(res[0])] = res[0]
    return msgs, counts


def _dense(msgs, counts):
    msgs = np.ascontiguousarray(msgs, dtype=np.uint8)
    counts = np.ascontiguousarray(counts, dtype=np.int32)
    if msgs.ndim != 3 or counts.shape != (msgs.shape[0],):
        raise ValueError("msgs must be [n, list_size, msg_len] and counts [n]")
    return msgs, counts


def filter_lists(msgs, counts, bytes_per_oligo, num_oligos, pad=False, list_size=None, device=0):
    """helper.decode_list_CRC_index on every read: the first of the first min(counts[i], list_size) entries whose CRC-8
    checks and whose index is < num_oligos.  list_size: None = all entries of the array.
    -> (index int32 [n] (-1: none), rank int32 [n] (-1: none), payload uint8 [n, bytes_per_oligo] (zeros: none))"""
    msgs, counts = _dense(msgs, counts)
    n, L, msg_len = msgs.shape
    use = 0 if list_size is None else min(int(list_size), L)
    if list_size is not None and use < 1:
        raise ValueError("list_size must be at least 1")
    index = np.full(n, -1, np.int32)
    rank = np.full(n, -1, np.int32)
    payload = np.zeros((n, bytes_per_oligo), np.uint8)
    check(load_library().lva_list_filter(device, msgs.ctypes.data, counts.ctypes.data, n, L, msg_len, use, bytes_per_oligo,
                                          num_oligos, int(bool(pad)), index.ctypes.data, rank.ctypes.data, payload.ctypes.data))
    return index, rank, payload


def consensus_arrays(index, payload, num_oligos, first_only=False, device=0):
    """-> (present bool [num_oligos], payload uint8 [num_oligos, bytes_per_oligo], votes int32 [num_oligos])"""
    index = np.ascontiguousarray(index, dtype=np.int32)
    payload = np.ascontiguousarray(payload, dtype=np.uint8)
    if payload.ndim != 2 or index.shape != (payload.shape[0],):
        raise ValueError("index must be [n] and payload [n, bytes_per_oligo]")
    present = np.zeros(num_oligos, np.uint8)
    out = np.zeros((num_oligos, payload.shape[1]), np.uint8)
    votes = np.zeros(num_oligos, np.int32)
    check(load_library().lva_list_consensus(device, index.ctypes.data, payload.ctypes.data, len(index), payload.shape[1], num_oligos,
                                             int(bool(first_only)), present.ctypes.data, out.ctypes.data, votes.ctypes.data))
    return present.astype(bool), out, votes


def consensus(index, payload, num_oligos, first_only=False, device=0):
    """rs_code.consensus over filter_lists' outputs (reads with index -1 have no vote): per index the payload seen most
    often, among equal counts the one that reached the count first in read order; first_only: the first payload seen.
    -> [[index, payload_bytes]] in ascending index order (rs_code.MainDecoder does not depend on the order)"""
    present, out, _ = consensus_arrays(index, payload, num_oligos, first_only, device)
    return [[int(k), out[k].tobytes()] for k in np.nonzero(present)[0]]


def list_stats(msgs, counts, truth, device=0):
    """simulator.run's per-trial statistics for every read: truth uint8 [n, msg_len] of 0/1.
    -> structured array [n] with the int32 fields STAT_FIELDS; all -1 for a read without a list"""
    msgs, counts = _dense(msgs, counts)
    truth = np.ascontiguousarray(truth, dtype=np.uint8)
    n, L, msg_len = msgs.shape
    if truth.shape != (n, msg_len):
        raise ValueError("truth must be [n, msg_len]")
    out = np.zeros(n, STAT_DTYPE)
    assert out.itemsize == ctypes.sizeof(_lib.ListStat)
    check(load_library().lva_list_stats(device, msgs.ctypes.data, counts.ctypes.data, truth.ctypes.data, n, L, msg_len, out.ctypes.data))
    return out
