"""Python face of the C ABI: code description, encoder, batched GPU list decoding.

Mirrors the reference's operator surface for this path:
  * `encode`  <->  `viterbi_nanopore.out -m encode`  (viterbi_convolutional_code.cpp:215-225)
  * `Decoder.decode`  <->  `viterbi_nanopore.out -m decode` per read (:226-254), batched.
"""
import ctypes
from contextlib import contextmanager
from dataclasses import dataclass

import numpy as np

from . import _lib
from ._lib import LvaError, check, load_library

_BASES = np.frombuffer(b"ACGT", dtype=np.uint8)


def _sm(sync_marker):
    return sync_marker.encode() if sync_marker else None


def _dist(d):
    """INT32_MAX of the C ABI = the reference's np.inf: no such distance"""
    return float("inf") if d == 0x7FFFFFFF else d


@dataclass
class CodeInfo:
    mem_conv: int
    rate: int
    msg_len: int
    nstate_pos: int
    nstate_conv: int
    oligo_len: int
    msg_words: int
    initial_state: int
    final_state: int
    g: tuple
    pattern: tuple


def code_info(mem_conv, rate, msg_len, rc=False, sync_marker="", sync_period=0):
    """set_conv_params (:264-415): raises LvaError for parameters the reference rejects."""
    L = load_library()
    s = _lib.CodeInfoStruct()
    check(L.lva_code_describe(mem_conv, rate, msg_len, int(bool(rc)), _sm(sync_marker), sync_period, ctypes.byref(s)), detail=None)
    return CodeInfo(mem_conv, rate, msg_len, s.nstate_pos, s.nstate_conv, s.oligo_len, s.msg_words,
                    s.initial_state, s.final_state, (s.g0, s.g1), tuple(s.pattern[:s.pattern_len]))


def code_tables(mem_conv, rate, msg_len, rc=False, sync_marker="", sync_period=0):
    """The per-position / per-conv-state tables the kernels index (for inspection and tests)."""
    info = code_info(mem_conv, rate, msg_len, rc, sync_marker, sync_period)
    L = load_library()
    pos2msg = np.zeros(info.nstate_pos, np.uint32)
    ptype = np.zeros(info.nstate_pos, np.uint8)
    vmask = np.zeros(info.nstate_pos, np.uint32)
    vval = np.zeros(info.nstate_pos, np.uint32)
    predtab = np.zeros((4, info.nstate_conv), np.uint16)
    check(L.lva_code_tables(mem_conv, rate, msg_len, int(bool(rc)), _sm(sync_marker), sync_period,
                            pos2msg.ctypes.data, ptype.ctypes.data, vmask.ctypes.data, vval.ctypes.data,
                            predtab.ctypes.data), detail=None)
    return dict(pos2msg=pos2msg, ptype=ptype, vmask=vmask, vval=vval, predtab=predtab)


def code_fingerprint(mem_conv, rate, msg_len, msg_bits, n_bits=None, rc=False, sync_marker="", sync_period=0):
    """The 32-bit fingerprint the step kernels hold for a path that has consumed the first n_bits (default: all, and then the
    terminating bits too) of the message `msg_bits` (msg_len values 0/1 in encode()'s order; a reverse complement consumes
    them from the far end): lva_code_fingerprint, for inspection and tests."""
    msg = np.ascontiguousarray(msg_bits, dtype=np.uint8)
    if msg.shape != (msg_len,):
        raise LvaError(-10, "Message length does not match msg_len parameter.")
    out = ctypes.c_uint32(0)
    check(load_library().lva_code_fingerprint(mem_conv, rate, msg_len, int(bool(rc)), _sm(sync_marker), sync_period,
                                              msg.ctypes.data, msg_len if n_bits is None else int(n_bits), ctypes.byref(out)),
          detail=None)
    return out.value


STEP_KERNELS = ("exact", "wave", "wave_wide", "acs", "fast", "lazy", "big", "big_rec")     # LVA_STEP_* of include/lva_decoder.h
FIXUP_KERNELS = ("none", "wave", "lazy")                                                    # LVA_FIXUP_*


def kernel_plan(mem_conv, rate, msg_len, list_size=1, max_deviation=None, sync_marker="", sync_period=0, kernel=0):
    """What a Decoder of these arguments runs, decided without a device (lva_kernel_plan): dict(mode = the kernel mode that
    profile()["kernel"] reports, dominant and fixup = names out of STEP_KERNELS / FIXUP_KERNELS, lazy / rec / cmp = the layout
    flags, ring_positions, instance).  Raises the LvaError the Decoder would raise before it looks for a GPU."""
    cfg = _lib.Config(mem_conv, rate, msg_len, list_size, _lib.MAX_DEVIATION_DEFAULT if max_deviation is None else max_deviation,
                      _sm(sync_marker), sync_period, 0, 0, kernel, 0)
    s = _lib.KernelPlanInfo()
    check(load_library().lva_kernel_plan(ctypes.byref(cfg), ctypes.byref(s)), detail=None)
    return dict(mode=s.mode, dominant=STEP_KERNELS[s.dominant], fixup=FIXUP_KERNELS[s.fixup], lazy=s.lazy, rec=s.rec, cmp=s.cmp,
                ring_positions=s.ring_positions, instance=s.instance)


def band_table(mem_conv, rate, msg_len, nblk, max_deviation=None, rc=False, sync_marker="", sync_period=0):
    """-> (reference, working): int arrays [nblk, 2] of [lo, hi) per time step -- the reference's band (:677-679) and the band the
    kernels work on (without positions whose lists cannot reach the output; include/lva_decoder.h lva_band_table)."""
    L = load_library()
    ref = np.zeros((nblk, 2), np.uint32)
    work = np.zeros((nblk, 2), np.uint32)
    md = 0xFFFFFFFF if max_deviation is None else int(max_deviation)
    check(L.lva_band_table(mem_conv, rate, msg_len, int(bool(rc)), _sm(sync_marker), sync_period, int(nblk), md,
                           ref.ctypes.data, work.ctypes.data), detail=None)
    return ref.astype(np.int64), work.astype(np.int64)


def encode(mem_conv, rate, msg_len, msgs):
    """msgs: array [n, msg_len] (or [msg_len]) of 0/1 -> uint8 array [n, oligo_len] of 0..3 (A,C,G,T)."""
    msgs = np.ascontiguousarray(msgs, dtype=np.uint8)
    single = msgs.ndim == 1
    if single:
        msgs = msgs[None, :]
    if msgs.shape[1] != msg_len:
        raise LvaError(-10, "Message length does not match msg_len parameter.")   # :219-222
    info = code_info(mem_conv, rate, msg_len)
    out = np.zeros((msgs.shape[0], info.oligo_len), np.uint8)
    check(load_library().lva_encode(mem_conv, rate, msg_len, msgs.ctypes.data, msgs.shape[0], out.ctypes.data), detail=None)
    return out[0] if single else out


def bases_to_str(bases):
    return _BASES[np.asarray(bases, dtype=np.uint8)].tobytes().decode()


def str_to_bits(s):
    return np.frombuffer(s.encode(), dtype=np.uint8) - ord("0")


def algorithmic_bytes(mem_conv, rate, msg_len, nblk, list_size, max_deviation=None, rc=False,
                      sync_marker="", sync_period=0):
    """sum_t [2 R(t) L (4+4W) + 160] for one read of nblk blocks."""
    out = ctypes.c_double(0)
    md = _lib.MAX_DEVIATION_DEFAULT if max_deviation is None else max_deviation
    check(load_library().lva_algorithmic_bytes(mem_conv, rate, msg_len, int(bool(rc)), _sm(sync_marker), sync_period,
                                               nblk, list_size, md, ctypes.byref(out)), detail=None)
    return out.value


class Decoder:
    """A list-Viterbi decoder bound to one GPU.  Fails loudly without a GPU (no CPU path).

    kernel: 0 = default (the fastest mode for the configuration: 4 for list sizes 2 / 4 / 8,
    else 2 for list sizes up to 64, the thread-per-target exact kernel beyond), 1 = thread-per-target exact kernel,
    2 = fast kernel + exact fix-up, 3 = wavefront-per-target exact kernel (list sizes 2..256; above 64 entries it is the one
    alternative to mode 1 and has to be asked for), 4 = fast kernel with lazy messages
    (materialised every second time step); kernel_plan(...) tells what a configuration resolves to.  All modes give the
    reference's lists bit for bit; they differ in speed only."""

    def __init__(self, mem_conv, rate, msg_len, list_size=1, max_deviation=None, sync_marker="", sync_period=0,
                 device=0, max_slots=0, kernel=0, mem_budget_bytes=0):
        self._L = load_library()
        self._sync = _sm(sync_marker)
        cfg = _lib.Config(mem_conv, rate, msg_len, list_size,
                          _lib.MAX_DEVIATION_DEFAULT if max_deviation is None else max_deviation,
                          self._sync, sync_period, device, max_slots, kernel, mem_budget_bytes)
        h = ctypes.c_void_p()
        check(self._L.lva_decoder_create(ctypes.byref(cfg), ctypes.byref(h)))
        self._h = h
        self.mem_conv, self.rate, self.msg_len, self.list_size = mem_conv, rate, msg_len, list_size
        self.max_deviation = max_deviation               # None: the band is off
        self.device = device
        self._sync_period = sync_period

    def close(self):
        if getattr(self, "_h", None):
            self._L.lva_decoder_destroy(self._h)
            self._h = None

    def __del__(self):
        self.close()

    def __enter__(self):
        return self

    def __exit__(self, *a):
        self.close()

    _check = staticmethod(check)       # a status of the library: LvaError with lva_last_hip_error's text unless it is 0

    @staticmethod
    def _pack(posts):
        posts = [np.ascontiguousarray(p, dtype=np.float32).reshape(-1, 40) for p in posts]
        off = np.zeros(len(posts) + 1, np.int64)
        off[1:] = np.cumsum([p.shape[0] for p in posts])
        flat = np.concatenate(posts, axis=0) if posts else np.zeros((0, 40), np.float32)
        return np.ascontiguousarray(flat), off

    def _outputs(self, n):
        return (np.zeros((n, self.list_size, self.msg_len), np.uint8), np.zeros((n, self.list_size), np.float32),
                np.zeros(n, np.int32))

    def _unpack(self, n, msgs, scores, counts):
        out = []
        for i in range(n):
            c = int(counts[i])
            out.append((msgs[i, :c].copy(), scores[i, :c].copy()) if c >= 0 else c)
        return out

    def decode(self, posts, rc=None):
        """posts: list of float32 [nblk_i, 40] matrices (.post layout).  rc: optional bool per read.
        -> list of (msgs uint8[count, msg_len], scores float32[count]) or a negative error code per read."""
        flat, off = self._pack(posts)
        return self.decode_packed(flat, off, rc)

    pack = _pack

    def decode_packed(self, flat, off, rc=None):
        """decode() on a host buffer that is already in the C ABI's form: `flat` float32 [sum nblk, 40] (all reads
        back to back), `off` int64 [n+1] block offsets.  The host->device copy happens inside the call."""
        return self._unpack(len(off) - 1, *self._decode_packed_dense(flat, off, rc))

    def _decode_call(self, fn, n, rc, *where):
        """The one decode call: `where` is what the entry point takes between the decoder and n_reads (the buffer and its row
        offsets, or the buffer and its windows) -> the outputs as the C ABI fills them: msgs uint8 [n, list_size, msg_len],
        scores float32 [n, list_size], counts int32 [n]"""
        rcf = None if rc is None else np.ascontiguousarray(rc, dtype=np.uint8)
        msgs, scores, counts = self._outputs(n)
        self._check(fn(self._h, *where, n, None if rcf is None else rcf.ctypes.data,
                       msgs.ctypes.data, scores.ctypes.data, counts.ctypes.data))
        return msgs, scores, counts

    def _decode_packed_dense(self, flat, off, rc=None):
        """decode_packed's outputs as the C ABI fills them: msgs uint8 [n, list_size, msg_len], scores, counts"""
        assert flat.dtype == np.float32 and flat.flags.c_contiguous and off.dtype == np.int64
        return self._decode_call(self._L.lva_decode_batch, len(off) - 1, rc, flat.ctypes.data, off.ctypes.data)

    def decode_payloads(self, posts, rc, bytes_per_oligo, num_oligos, pad=False):
        """decode() followed by the CRC-8 / index filter (helper.decode_list_CRC_index, helper.py:371-388) on the arrays
        the decode filled, without a list of strings in between (list_ops.filter_lists: csrc/ls_kernels.hip).
        -> dict(index int32 [n] (-1: no entry passed), rank int32 [n], payload uint8 [n, bytes_per_oligo], counts int32 [n])"""
        from . import list_ops
        flat, off = self._pack(posts)
        msgs, _, counts = self._decode_packed_dense(flat, off, rc)
        index, rank, payload = list_ops.filter_lists(msgs, counts, bytes_per_oligo, num_oligos, pad=pad, device=self.device)
        return dict(index=index, rank=rank, payload=payload, counts=counts)

    # --- inputs resident in HBM (bench.py) ---------------------------------------------------
    def upload(self, posts):
        flat, off = self._pack(posts)
        p = self.alloc(flat.nbytes)
        self._check(self._L.lva_device_upload(self._h, p, flat.ctypes.data, flat.nbytes))
        return p, off

    def free(self, dev_ptr):
        self._L.lva_device_free(self._h, dev_ptr)

    @contextmanager
    def resident(self, data, offsets=None):
        """A buffer in HBM for the length of a `with` block, freed on every way out of it -> (device pointer, offsets).
        data: a list of float32 [nblk_i, 40] matrices, packed and uploaded as upload() does; or with `offsets` (int64 [n + 1])
        one array that holds them back to back already; or a number of bytes, left as allocated (alloc())."""
        flat, off = None, offsets
        if not isinstance(data, (int, np.integer)):
            flat, off = self._pack(data) if offsets is None else (
                np.ascontiguousarray(data, dtype=np.float32).reshape(-1, 40), np.ascontiguousarray(offsets, dtype=np.int64))
        dev = self.alloc(data if flat is None else flat.nbytes)
        try:
            if flat is not None:
                self._check(self._L.lva_device_upload(self._h, dev, flat.ctypes.data, flat.nbytes))
            yield dev, off
        finally:
            self.free(dev)

    def decode_resident(self, dev_ptr, off, rc=None):
        n = len(off) - 1
        return self._unpack(n, *self._decode_call(self._L.lva_decode_batch_device, n, rc, dev_ptr, off.ctypes.data))

    def decode_windows_resident(self, dev_ptr, first_block, n_blocks, rc=None):
        """decode windows [first_block[i], first_block[i] + n_blocks[i]) of a resident posterior buffer in place
        (helper.truncate_post_file + the decode call of generate_decoded_lists.py:80-89, without the copy)"""
        fb = np.ascontiguousarray(first_block, dtype=np.int64)
        nb = np.ascontiguousarray(n_blocks, dtype=np.int64)
        return self._unpack(len(fb), *self._decode_call(self._L.lva_decode_windows_device, len(fb), rc, dev_ptr,
                                                        fb.ctypes.data, nb.ctypes.data))

    def decode_located(self, dev_ptr, off, loc, subset=None):
        """The windows that were found, decoded where they are: `loc` holds one dict per read of the resident buffer, as
        locate_payload or demux give them (ok, start_pos, end_pos, rc are read); subset: the read indices to consider
        (default: all).  One decode_windows_resident call for the reads whose `ok` is set, none when there is no such read.
        -> [(loc[i], decode result | None)] for every read; None: not found, or not in the subset"""
        good = [i for i in (range(len(loc)) if subset is None else subset) if loc[i]["ok"]]
        out = [(lc, None) for lc in loc]
        if good:
            dec = self.decode_windows_resident(dev_ptr, [int(off[i]) + loc[i]["start_pos"] for i in good],
                                               [loc[i]["end_pos"] - loc[i]["start_pos"] + 1 for i in good],
                                               rc=[loc[i]["rc"] for i in good])
            for i, r in zip(good, dec):
                out[i] = (loc[i], r)
        return out

    # --- what a given sequence or message scores on a read (trellis_score.py is the definition) -----
    @staticmethod
    def _score_args(seqs, pairs, max_deviation):
        """what the score and the trace entry points take after n_reads, up to max_deviation: (the arguments, the arrays they
        point into, the sequence lengths, the number of pairs)"""
        from .trellis_score import as_codes
        seqs = [as_codes(s) for s in seqs]
        lens = np.array([len(s) for s in seqs], dtype=np.int32)
        first = np.zeros(len(seqs), np.int64)
        first[1:] = np.cumsum(lens[:-1], dtype=np.int64)
        bases = np.concatenate(seqs + [np.zeros(1, np.uint8)])
        pr = np.ascontiguousarray(pairs, dtype=np.int32).reshape(-1, 2)
        md = _lib.MAX_DEVIATION_DEFAULT if max_deviation is None else int(max_deviation)
        args = (bases.ctypes.data, first.ctypes.data, lens.ctypes.data, len(seqs), pr.ctypes.data, len(pr), md)
        return args, (bases, first, pr), lens, len(pr)

    def _score(self, fn, where, n_reads, seqs, pairs, max_deviation):
        """the one score call: `where` is what the entry point takes between the decoder and n_reads"""
        args, _keep, _, n = self._score_args(seqs, pairs, max_deviation)
        out = np.zeros((n, 2), np.float32)
        self._check(fn(self._h, *where, n_reads, *args, out.ctypes.data))
        return out

    def _trace(self, fn, where, n_reads, seqs, pairs, max_deviation, end, scratch_limit):
        """the one trace call, after _score"""
        args, _keep, lens, n = self._score_args(seqs, pairs, max_deviation)
        stride = int(lens.max()) if len(lens) else 1
        score, info = np.zeros((n, 2), np.float32), np.zeros((n, 4), np.int32)
        enter, kind = np.full((n, stride), -1, np.int32), np.full((n, stride), 255, np.uint8)
        self._check(fn(self._h, *where, n_reads, *args, int(end), int(scratch_limit), stride, score.ctypes.data, enter.ctypes.data,
                       kind.ctypes.data, info.ctypes.data))
        return dict(score=score, enter=enter, kind=kind, end_state=info[:, 0].copy(), start_state=info[:, 1].copy(),
                    n_stale=info[:, 2].copy())

    def score_bases(self, posts, seqs, pairs, max_deviation=None):
        """The reference trellis restricted to one base sequence, per (read, sequence) pair: posts as decode() takes them,
        seqs a list of base sequences (codes 0..3 or ACGT; any lengths from 1 to 1024, the code does not constrain them),
        pairs [(read, sequence)] in any order, max_deviation None: the decoder's.  -> float32 [n_pairs, 2] = (flip, flop),
        bit for bit trellis_score.reference_score(posts[r], seqs[s], max_deviation).  Raises LvaError for an index out of
        range and for a read shorter than its sequence's positions + 1 (LVA_ERR_POST_TOO_SHORT)."""
        flat, off = self._pack(posts)
        return self._score(self._L.lva_score_bases, (flat.ctypes.data, off.ctypes.data), len(off) - 1, seqs, pairs, max_deviation)

    def score_bases_resident(self, dev_ptr, first_block, n_blocks, seqs, pairs, max_deviation=None):
        """score_bases() on windows [first_block[i], first_block[i] + n_blocks[i]) of a resident posterior buffer, as
        decode_windows_resident reads them: a decode and the scores of its entries read the same memory"""
        fb = np.ascontiguousarray(first_block, dtype=np.int64)
        nb = np.ascontiguousarray(n_blocks, dtype=np.int64)
        return self._score(self._L.lva_score_bases_device, (dev_ptr, fb.ctypes.data, nb.ctypes.data), len(fb), seqs, pairs,
                           max_deviation)

    def score_messages(self, posts, msgs, pairs, rc=None):
        """What messages score on reads under this decoder's code and max_deviation: msgs uint8 [n_msgs, msg_len] in
        encode()'s bit order (rows of a decoded list as they are), pairs [(read, message)], rc an optional bool per READ (the
        flag its decode takes; a message is encoded for the orientation of every read it is paired with).
        -> float32 [n_pairs, 2]; every score of decode()'s list for a read is one of the two values of its message."""
        return self.score_bases(posts, *self._message_pairs(posts, msgs, pairs, rc))

    def _message_pairs(self, posts, msgs, pairs, rc):
        """(sequences, pairs into them) of score_messages' and trace_messages' arguments"""
        from .trellis_score import message_bases
        msgs = np.ascontiguousarray(msgs, dtype=np.uint8).reshape(-1, self.msg_len)
        pr = np.array(pairs, dtype=np.int32).reshape(-1, 2)          # a copy: the message indices become sequence indices below
        sync = self._sync.decode() if self._sync else ""
        if len(pr) and (pr[:, 1].min() < 0 or pr[:, 1].max() >= len(msgs)):
            raise LvaError(-10, "a pair names a message that is not there")
        flip = np.zeros(len(pr), bool)
        if rc is not None and len(posts):
            if len(rc) != len(posts):
                raise ValueError("rc: one flag per read")
            flip = np.asarray(rc, dtype=bool)[np.clip(pr[:, 0], 0, len(posts) - 1)]       # (an index out of range: the call refuses it)
        seqs = []
        for want in (False, True):                       # forward sequences first, then the reverse complements that are asked for
            use = np.unique(pr[flip == want, 1])
            if len(use):
                enc = message_bases(self.mem_conv, self.rate, self.msg_len, msgs[use], want, sync, self._sync_period)
                at = dict(zip(use.tolist(), range(len(seqs), len(seqs) + len(use))))
                seqs += list(enc)
                pr[flip == want, 1] = [at[m] for m in pr[flip == want, 1].tolist()]
        return seqs, pr

    # --- the forward score of the same trellis (trellis_score.reference_forward is the definition; csrc/fw_kernels.hip) ---
    def forward_bases(self, posts, seqs, pairs, max_deviation=None):
        """The forward score of a base sequence on a read, per (read, sequence) pair: the log of the total weight of all
        alignments inside the band, where score_bases gives the best one's; arguments and refusals as score_bases.
        -> float32 [n_pairs, 2] = (flip, flop); trellis_score.forward_total adds the two.  A floating-point stage: within twice
        the float32 restatement's error of trellis_score.reference_forward(posts[r], seqs[s], max_deviation), not its bits."""
        flat, off = self._pack(posts)
        return self._score(self._L.lva_forward_bases, (flat.ctypes.data, off.ctypes.data), len(off) - 1, seqs, pairs, max_deviation)

    def forward_bases_resident(self, dev_ptr, first_block, n_blocks, seqs, pairs, max_deviation=None):
        """forward_bases() on windows of a resident posterior buffer, as score_bases_resident reads them"""
        fb = np.ascontiguousarray(first_block, dtype=np.int64)
        nb = np.ascontiguousarray(n_blocks, dtype=np.int64)
        return self._score(self._L.lva_forward_bases_device, (dev_ptr, fb.ctypes.data, nb.ctypes.data), len(fb), seqs, pairs,
                           max_deviation)

    def forward_messages(self, posts, msgs, pairs, rc=None):
        """forward_bases() for messages under this decoder's code and max_deviation; msgs, pairs and rc as score_messages"""
        return self.forward_bases(posts, *self._message_pairs(posts, msgs, pairs, rc))

    # --- the traceback of the same trellis (trellis_score.reference_trace is the definition; csrc/st_kernels.hip) --------
    def trace_bases(self, posts, seqs, pairs, max_deviation=None, end=-1, scratch_limit=0):
        """The best path of a base sequence on a read, per (read, sequence) pair; arguments as score_bases, end: the state of
        the last position the walk starts in (0 flip, 1 flop, -1 the larger score, flip on a tie), scratch_limit: bytes of
        back-pointers on the device at a time (0: 1 GiB; the result does not depend on it).
        -> dict of arrays, byte for byte trellis_score.reference_trace(posts[r], seqs[s], max_deviation, end):
        score float32 [n_pairs, 2] (score_bases' bits); enter int32 [n_pairs, longest sequence], PADDED with -1: enter[k, p - 1]
        is the block whose transition moved the path of pair k into position p, for p up to the length of the pair's sequence;
        kind uint8, padded with 255 (0: the position is held as flip, 1: as flop); start_state, end_state, n_stale int32
        [n_pairs].  A pair without a path (an end score of -inf) has enter -1, kind 255 and both states -1."""
        flat, off = self._pack(posts)
        return self._trace(self._L.lva_trace_bases, (flat.ctypes.data, off.ctypes.data), len(off) - 1, seqs, pairs, max_deviation,
                           end, scratch_limit)

    def trace_bases_resident(self, dev_ptr, first_block, n_blocks, seqs, pairs, max_deviation=None, end=-1, scratch_limit=0):
        """trace_bases() on windows of a resident posterior buffer, as score_bases_resident reads them"""
        fb = np.ascontiguousarray(first_block, dtype=np.int64)
        nb = np.ascontiguousarray(n_blocks, dtype=np.int64)
        return self._trace(self._L.lva_trace_bases_device, (dev_ptr, fb.ctypes.data, nb.ctypes.data), len(fb), seqs, pairs,
                           max_deviation, end, scratch_limit)

    def trace_messages(self, posts, msgs, pairs, rc=None, end=-1, scratch_limit=0):
        """trace_bases() for messages under this decoder's code and max_deviation; msgs, pairs and rc as score_messages"""
        return self.trace_bases(posts, *self._message_pairs(posts, msgs, pairs, rc), end=end, scratch_limit=scratch_limit)

    # --- basecall of the posterior matrix + barcode localisation ------------
    def _basecall(self, fn, src, off):
        n = len(off) - 1
        T = max(int(off[-1]), 1)
        bases, trans, nb = np.zeros(T, np.uint8), np.zeros(T, np.uint32), np.zeros(max(n, 1), np.int32)
        self._check(fn(self._h, src, off.ctypes.data, n, bases.ctypes.data, trans.ctypes.data, nb.ctypes.data))
        return [(bases[off[i]:off[i] + nb[i]].tobytes().decode("ascii"), trans[off[i]:off[i] + nb[i]].astype(np.int64))
                for i in range(n)]

    def basecall(self, posts):
        """flappie's basecall of each posterior matrix (flappie.c:273-285): [(base string, trans positions)]"""
        flat, off = self._pack(posts)
        return self._basecall(self._L.lva_basecall_batch, flat.ctypes.data, off)

    def basecall_resident(self, dev_ptr, off):
        return self._basecall(self._L.lva_basecall_batch_device, dev_ptr, off)

    @staticmethod
    def _pack_bases(basecalls, trans_lists):
        """(basecall, trans list) pairs in the C ABI's form -> (bases uint8, trans uint32, base offsets int64 [n + 1]); of a
        trans list the first len(basecall) entries count; an empty batch leaves one placeholder element in each array"""
        off = np.zeros(len(basecalls) + 1, np.int64)
        off[1:] = np.cumsum([len(b) for b in basecalls])
        for b, t in zip(basecalls, trans_lists):
            if len(t) < len(b):
                raise ValueError("trans list shorter than the basecall")
        bases = np.frombuffer("".join(basecalls).encode("ascii") or b"\0", dtype=np.uint8).copy()
        trans = np.concatenate([np.asarray(t, dtype=np.uint32)[:len(b)] for b, t in zip(basecalls, trans_lists)]
                               + [np.zeros(1, np.uint32)])
        return bases, trans, off

    @staticmethod
    def _payload_out(res, n):
        return [dict(ok=bool(r.ok), start_pos=r.start_pos, end_pos=r.end_pos, rc=bool(r.rc),
                     dist_start=_dist(r.dist_start), dist_end=_dist(r.dist_end)) for r in res[:n]]

    def find_barcode(self, basecalls, trans_lists, start_barcode, end_barcode):
        """helper.find_barcode_pos_in_post (helper.py:157-210) for a batch of (basecall, trans list) pairs"""
        n = len(basecalls)
        bases, trans, off = self._pack_bases(basecalls, trans_lists)
        res = (_lib.PayloadPos * max(n, 1))()
        self._check(self._L.lva_find_barcode_batch(self._h, bases.ctypes.data, trans.ctypes.data, off.ctypes.data, n,
                                                   start_barcode.encode(), end_barcode.encode(), res))
        return self._payload_out(res, n)

    def _locate(self, fn, src, off, start_barcode, end_barcode):
        n = len(off) - 1
        res = (_lib.PayloadPos * max(n, 1))()
        self._check(fn(self._h, src, off.ctypes.data, n, start_barcode.encode(), end_barcode.encode(),
                       self.mem_conv + self.msg_len + 1, res))
        return self._payload_out(res, n)

    def locate_payload(self, posts, start_barcode, end_barcode):
        """generate_decoded_lists.py:68-79 per read: basecall, barcode search in both orientations, choice.
        -> [dict(ok, start_pos, end_pos, rc, dist_start, dist_end)]"""
        flat, off = self._pack(posts)
        return self._locate(self._L.lva_locate_payload_batch, flat.ctypes.data, off, start_barcode, end_barcode)

    def locate_payload_resident(self, dev_ptr, off, start_barcode, end_barcode):
        return self._locate(self._L.lva_locate_payload_batch_device, dev_ptr, off, start_barcode, end_barcode)

    # --- DESIGN.md row N3': demultiplexing a pooled run ------------------------------------------
    def _demux(self, fn, n, where, experiments, max_dist, min_margin, all):
        """the one demux call: `where` is what the entry point takes between the decoder and n_reads"""
        from .helper import experiment_barcodes
        exps = [experiment_barcodes(e) for e in experiments]
        k = len(exps)
        arr = (_lib.ExperimentBarcodes * max(k, 1))()
        for a, (sb, eb, min_len) in zip(arr, exps):
            a.start_barcode, a.end_barcode, a.min_len = sb.encode(), eb.encode(), min_len
        res = (_lib.DemuxPos * max(n, 1))()
        table = (_lib.PayloadPos * max(n * k, 1))() if all else None
        self._check(fn(self._h, *where, n, arr, k, -1 if max_dist is None or max_dist < 0 else int(max_dist), int(min_margin),
                       res, table))
        out = self._payload_out([r.pos for r in res[:n]], n)
        for r, d in zip(res[:n], out):
            d.update(experiment=r.experiment, reason=r.reason, runner_up=r.runner_up, runner_up_dist=_dist(r.runner_up_dist))
        if not all:
            return out
        return out, [self._payload_out(table[i * k:(i + 1) * k], k) for i in range(n)]

    def demux(self, posts, experiments, max_dist=None, min_margin=0, all=False):
        """Which experiment of a pooled run each read belongs to: one basecall per read, one search over every experiment's
        barcodes, one decision (helper.demux_barcodes is the host counterpart).  experiments: (start_barcode, end_barcode,
        min_len) tuples or dicts (helper.experiment_barcodes), 1..64 of them.
        -> [dict(locate_payload's fields of the winner, experiment, reason, runner_up, runner_up_dist)];
        all=True: -> (that, [[locate_payload dict per experiment] per read])."""
        flat, off = self._pack(posts)
        return self._demux(self._L.lva_demux_batch, len(posts), (flat.ctypes.data, off.ctypes.data),
                           experiments, max_dist, min_margin, all)

    def demux_resident(self, dev_ptr, off, experiments, max_dist=None, min_margin=0, all=False):
        """demux() on a resident posterior buffer (upload(), posteriors_resident())"""
        off = np.ascontiguousarray(off, dtype=np.int64)
        return self._demux(self._L.lva_demux_batch_device, len(off) - 1, (dev_ptr, off.ctypes.data),
                           experiments, max_dist, min_margin, all)

    def demux_bases(self, basecalls, trans_lists, experiments, max_dist=None, min_margin=0, all=False):
        """demux() on given (basecall, trans list) pairs, as find_barcode takes them, in both orientations"""
        bases, trans, off = self._pack_bases(basecalls, trans_lists)
        return self._demux(self._L.lva_demux_bases_batch, len(basecalls), (bases.ctypes.data, trans.ctypes.data, off.ctypes.data),
                           experiments, max_dist, min_margin, all)

    def decode_with_barcodes(self, posts, start_barcode, end_barcode):
        """The real-data chain of generate_decoded_lists.py:68-89 on the device: posteriors are uploaded once,
        payload windows located, then decoded in place.  -> [(locate dict, decode result or None)]"""
        with self.resident(posts) as (dev, off):
            return self._decode_chain_resident(dev, off, None, start_barcode, end_barcode)

    # --- transition posteriors from a network's transition scores ---------------
    def posteriors(self, scores):
        """scores: list of float32 [nblk_i, 40] transition-score matrices of a flip-flop CRF (flappie's `trans` layout,
        which is the .post layout) -> list of float32 [nblk_i, 40] log-posteriors, what flappie writes to a .post file
        (transpost_crf_flipflop, flappie/src/decode.c:377-497)"""
        flat, off = self._pack(scores)
        out = np.empty_like(flat)
        self._check(self._L.lva_transpost_batch(self._h, flat.ctypes.data, off.ctypes.data, len(off) - 1, out.ctypes.data))
        return [out[off[i]:off[i + 1]].copy() for i in range(len(off) - 1)]

    def posteriors_resident(self, dev_ptr, off, out_ptr=None):
        """posteriors of a resident score buffer (upload()); out_ptr=None: in place, the scores are overwritten"""
        off = np.ascontiguousarray(off, dtype=np.int64)
        self._check(self._L.lva_transpost_batch_device(self._h, dev_ptr, off.ctypes.data, len(off) - 1,
                                                       dev_ptr if out_ptr is None else out_ptr))

    def alloc(self, nbytes):
        p = ctypes.c_void_p()
        self._check(self._L.lva_device_alloc(self._h, int(nbytes), ctypes.byref(p)))
        return p

    def download(self, dev_ptr, off):
        """a resident [off[-1], 40] float32 buffer -> list of host matrices"""
        flat = np.empty((int(off[-1]), 40), np.float32)
        self._check(self._L.lva_device_download(self._h, flat.ctypes.data, dev_ptr, flat.nbytes))
        return [flat[off[i]:off[i + 1]].copy() for i in range(len(off) - 1)]

    def _decode_chain_resident(self, dev, off, rc, start_barcode, end_barcode):
        if start_barcode is None and end_barcode is None:
            return self.decode_resident(dev, off, rc)
        if start_barcode is None or end_barcode is None or rc is not None:
            raise ValueError("give both barcodes (the orientation is then found, not passed), or neither")
        return self.decode_located(dev, off, self.locate_payload_resident(dev, off, start_barcode, end_barcode))

    def decode_from_scores(self, scores, rc=None, start_barcode=None, end_barcode=None, offsets=None):
        """scores -> posteriors -> (barcode localisation ->) decoded lists without leaving the device: the scores are
        uploaded once, turned into posteriors in place and decoded where they are.  Returns what decode() returns, or with
        both barcodes what decode_with_barcodes() returns.
        scores: a list of float32 [nblk_i, 40] matrices, or ONE contiguous float32 torch tensor [total_blocks, 40] on the
        decoder's device with `offsets` (int64 [n + 1] block offsets): its memory is read where it is and not modified --
        the posteriors go to a buffer of the decoder's.  (A process that uses torch and this library initialises torch's
        device first: INTEGRATION.md section 2.)"""
        if isinstance(scores, (list, tuple, np.ndarray)):
            with self.resident(scores, offsets) as (dev, off):
                self.posteriors_resident(dev, off)
                return self._decode_chain_resident(dev, off, rc, start_barcode, end_barcode)
        import torch                              # only here: the package imports without torch
        if not isinstance(scores, torch.Tensor):
            raise TypeError("scores: a list of [nblk, 40] arrays or one torch tensor with offsets")
        if offsets is None:
            raise ValueError("a score tensor needs offsets")
        if scores.dtype != torch.float32 or not scores.is_contiguous() or scores.dim() != 2 or scores.shape[1] != 40:
            raise ValueError("score tensor: float32, contiguous, [total_blocks, 40]")
        if not scores.is_cuda or scores.device.index != self.device:
            raise ValueError("score tensor is on %s, the decoder on device %d" % (scores.device, self.device))
        off = np.ascontiguousarray(offsets.cpu().numpy() if isinstance(offsets, torch.Tensor) else offsets, dtype=np.int64)
        if int(off[-1]) != scores.shape[0]:
            raise ValueError("offsets end at %d, the tensor has %d blocks" % (int(off[-1]), scores.shape[0]))
        torch.cuda.current_stream(scores.device).synchronize()     # the decoder works on a stream of its own
        with self.resident(scores.shape[0] * 160) as (dev, _):
            self.posteriors_resident(ctypes.c_void_p(scores.data_ptr()), off, out_ptr=dev)
            return self._decode_chain_resident(dev, off, rc, start_barcode, end_barcode)

    # --- reads made on the device (simulate.py is the definition) ----------------
    @contextmanager
    def simulate(self, n, seed, first_read=0, pool=None, pool_cdf=None, **kw):
        """n simulated reads of this decoder's code, numbers first_read .. first_read + n - 1 under `seed`, as transition
        scores in HBM for the length of a `with` block -> (device pointer, row_offsets, truth); truth: dict(msgs uint8
        [n, msg_len], bases uint8, base_offsets int64 [n + 1], true_idx uint8 [blocks]).  Keywords (simulate.parameters): sub,
        dele, ins, margin, sigma, clip, dwell_cdf, start_barcode, end_barcode, flank, rc_mode.  Bit for bit what
        simulate.reference_reads gives for the same arguments; a read depends on (seed, read number) alone.
        pool (uint8 [n_pool, msg_len] of 0 / 1): every read's message is a pool entry, drawn uniformly or by pool_cdf
        (simulate.weights_to_cdf); rc_mode may then be 3, a coin per read; truth gains source int32 [n] and rc uint8 [n]."""
        from . import simulate as sim
        q, pool, pool_cdf = sim.call_parameters(self.msg_len, pool, pool_cdf, kw)
        if n < 0 or first_read < 0 or first_read + n > 1 << 32:
            raise ValueError("read numbers are 32-bit")
        cdf = q["cdf"]
        bc = [None if b is None else b.encode() for b in (q["start_barcode"], q["end_barcode"])]
        shared = (self._h, int(seed) & 0xFFFFFFFFFFFFFFFF, int(first_read), int(n), q["sub"], q["dele"], q["ins"], cdf.ctypes.data,
                  len(cdf), bc[0], bc[1], q["flank"][0], q["flank"][1], q["rc_mode"])
        plan, fill, drawn, more = self._L.lva_simulate_plan, self._L.lva_simulate_fill_device, (), {}
        if pool is not None:                      # the pool pair: the same arguments, the pool behind them, two more outputs
            plan, fill = self._L.lva_simulate_pool_plan, self._L.lva_simulate_pool_fill_device
            shared += (pool.ctypes.data, len(pool), None if pool_cdf is None else pool_cdf.ctypes.data)
            more = dict(source=np.zeros(n, np.int32), rc=np.zeros(n, np.uint8))
            drawn = (more["source"].ctypes.data, more["rc"].ctypes.data)
        row, base = np.zeros(max(n, 0) + 1, np.int64), np.zeros(max(n, 0) + 1, np.int64)
        self._check(plan(*shared, row.ctypes.data, base.ctypes.data))
        msgs = np.zeros((n, self.msg_len), np.uint8)
        bases, true_idx = np.zeros(max(int(base[-1]), 1), np.uint8), np.zeros(max(int(row[-1]), 1), np.uint8)
        with self.resident(max(int(row[-1]), 1) * 160) as (dev, _):
            self._check(fill(*shared, float(q["scale"]), float(q["margin"]), float(q["clip"]), row.ctypes.data, base.ctypes.data,
                             dev, msgs.ctypes.data, bases.ctypes.data, true_idx.ctypes.data, *drawn))
            yield dev, row, dict(msgs=msgs, bases=bases[:int(base[-1])], base_offsets=base, true_idx=true_idx[:int(row[-1])],
                                 **more)

    def simulate_and_decode(self, n, seed, first_read=0, pool=None, pool_cdf=None, after=None, **kw):
        """simulate -> posteriors in place -> decode (with both barcodes: locate_payload_resident -> decode_located) without
        the scores leaving the device -> (truth, results); results as decode() / decode_with_barcodes() give them.  Without
        barcodes the orientation of every read is passed to the decoder as the simulator chose it (rc_mode; with a pool,
        truth's rc, as drawn).  after (without barcodes): a function (dev_ptr, row_offsets, truth, results, rc) that is called
        while the posteriors are still resident -- what it returns is returned third (trellis_score.simulate_rows scores the
        truth there)."""
        with self.simulate(n, seed, first_read, pool=pool, pool_cdf=pool_cdf, **kw) as (dev, off, truth):
            self.posteriors_resident(dev, off)
            if kw.get("start_barcode") is not None:
                if after is not None:
                    raise ValueError("after: reads without barcodes")
                return truth, self._decode_chain_resident(dev, off, None, kw["start_barcode"], kw["end_barcode"])
            mode = kw.get("rc_mode", 0)
            rc = [mode == 1 or (mode == 2 and bool((first_read + i) & 1)) for i in range(n)] if pool is None else truth["rc"]
            results = self.decode_resident(dev, off, rc)
            return (truth, results) if after is None else (truth, results, after(dev, off, truth, results, rc))

    # --- decode stream: reads go in one at a time, results come out as they finish -------------
    def stream(self, queue_cap=None):
        """A DecodeStream on this decoder (a context manager).  queue_cap: reads that may wait for a slot before submit()
        reports back-pressure (default: the slot count).  While it is open decode() and the other batch methods raise."""
        return DecodeStream(self, queue_cap)

    def decode_iter(self, posts, rc=None):
        """Generator: submits from the iterable `posts` (and `rc`, an iterable of bools, or None) as back-pressure allows and
        yields (index, result) as reads finish -- result as decode() gives it; the next matrices are fetched from the iterable
        while earlier reads decode."""
        rcs = None if rc is None else iter(rc)
        it = enumerate(posts)
        with self.stream() as st:
            held = None
            more = True
            while more or held is not None or st.outstanding:
                while more or held is not None:
                    if held is None:
                        try:
                            i, p = next(it)
                        except StopIteration:
                            more = False
                            break
                        held = (i, p, bool(next(rcs)) if rcs is not None else False)
                    if not st.submit(held[1], rc=held[2], tag=held[0]):
                        break                                  # queue full: hand out what has finished first
                    held = None
                # block only when nothing more can go in before a read comes out
                for tag, res in st.poll(wait=held is not None or not more):
                    yield tag, res

    def set_launch_events(self, on=True):
        """HIP events around every trellis-step launch of later decode calls (profile(): dominant_kernel_ms, step_pair_ms)"""
        self._check(self._L.lva_decoder_set_launch_events(self._h, int(bool(on))))

    def profile(self):
        p = _lib.Profile()
        self._L.lva_decoder_profile(self._h, ctypes.byref(p))
        d = {k: getattr(p, k) for k, _ in _lib.Profile._fields_}
        d["fixup_reason"] = list(p.fixup_reason)
        return d


class DecodeStream:
    """lva_stream_* of include/lva_decoder.h.  submit() hands one read in, poll() drives the device and hands finished reads out
    (in the order they finish).  Tags are the caller's names of the reads: any Python object (default: a running number)."""

    def __init__(self, dec, queue_cap=None):
        self._dec, self._L = dec, dec._L
        self.slots = dec.profile()["slots"]
        self.queue_cap = int(self.slots if queue_cap is None else queue_cap)
        h = ctypes.c_void_p()
        dec._check(self._L.lva_stream_open(dec._h, self.queue_cap, ctypes.byref(h)))
        self._h = h
        self._tags = {}
        self._next = 0
        n = self._cap = max(16, min(self.slots, 1024))
        self._otags = np.zeros(n, np.uint64)
        self._msgs, self._scores, self._counts = dec._outputs(n)

    @property
    def outstanding(self):
        """reads submitted and not yet handed out by poll()"""
        return len(self._tags)

    def submit(self, post, rc=False, tag=None):
        """One read: float32 [nblk, 40] (.post layout), copied before the call returns.  -> True, or False when queue_cap reads
        already wait for a slot (nothing was taken: poll(), then submit again)."""
        p = np.ascontiguousarray(post, dtype=np.float32).reshape(-1, 40)
        key = self._next
        st = self._L.lva_stream_submit(self._h, p.ctypes.data, p.shape[0], int(bool(rc)), key)
        if st == _lib.ERR_BUSY:
            return False
        self._dec._check(st)
        self._next += 1
        self._tags[key] = key if tag is None else tag
        return True

    def poll(self, wait=False):
        """-> [(tag, (msgs, scores) | negative code)] of reads that have finished.  wait=False never blocks on the device;
        wait=True returns as soon as at least one read is finished or nothing is pending."""
        out = []
        while True:
            n = ctypes.c_int32(0)
            self._dec._check(self._L.lva_stream_poll(self._h, int(bool(wait)) if not out else 0, self._cap, self._otags.ctypes.data,
                                                     self._msgs.ctypes.data, self._scores.ctypes.data, self._counts.ctypes.data,
                                                     ctypes.byref(n)))
            for k, res in enumerate(self._dec._unpack(n.value, self._msgs, self._scores, self._counts)):
                out.append((self._tags.pop(int(self._otags[k])), res))
            if n.value < self._cap:
                return out

    def pending(self):
        """-> dict(queued, in_slots, finished): waiting for a slot / being decoded / ready for poll()"""
        q, a, f = ctypes.c_int32(0), ctypes.c_int32(0), ctypes.c_int32(0)
        self._dec._check(self._L.lva_stream_pending(self._h, ctypes.byref(q), ctypes.byref(a), ctypes.byref(f)))
        return dict(queued=q.value, in_slots=a.value, finished=f.value)

    def close(self):
        """drains the device, drops reads that were not handed out; the decoder takes batch calls again"""
        if self._h is not None and getattr(self._dec, "_h", None):
            h, self._h = self._h, None
            self._tags.clear()
            self._dec._check(self._L.lva_stream_close(h))
        self._h = None

    def __enter__(self):
        return self

    def __exit__(self, *a):
        self.close()

    def __del__(self):
        try:
            self.close()
        except Exception:  # pragma: no cover
            pass
