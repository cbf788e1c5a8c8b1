"""The contract every decoder-bound stage entry point keeps (csrc/lva_stages.cpp), through the C ABI on the GPU: ONE table of
the ten entry points -- basecall, locate_payload, transpost and demux, each from host and from device memory, find_barcode and
demux_bases -- and the same refusals, no-op, state and precedence checks over all of them.  Refusals are LVA_ERR_ARG (-10)
from the offsets alone; what a good call returns afterwards is bit-equal to what it returned before, and to its twin.

The batch limit (2^31 blocks) is exercised for the posterior-side entry points only: an implementation that went ahead there
would fail in a 343 GB allocation.  For find_barcode / demux_bases a wrong implementation COULD allocate (10 GB) and would run
32-bit offsets past their range on the device, so that case is not written; their limit is checked by reading -- all ten entry
points validate through the one function check_offsets, the only place the limit appears."""

import numpy as np
import pytest

import nanopore_dna_storage_amd as pkg
from nanopore_dna_storage_amd import _lib, synth

pytestmark = pytest.mark.gpu

ARG, BUSY = -10, -13
SB, EB = "CACCTGTGCTGCGTCAGGCTGTGTC", "GCTGTCCGTTCCGCATTGACACGGC"
SB2, EB2 = "TTGACCGTAAGCTTCGGATACCAGT", "AGGTCAACTGCGTATTCCGGATCAA"
MAX_BLOCKS = 1 << 20


def _ptr(a):
    return None if a is None else a.ctypes.data


def _exps(pairs):
    arr = (_lib.ExperimentBarcodes * len(pairs))()
    for a, (sb, eb) in zip(arr, pairs):
        a.start_barcode, a.end_barcode, a.min_len = sb.encode(), eb.encode(), 0
    return arr


class Src:
    """where a call's input lies: posteriors (or scores) on the host, the same on the device (dev_out: where the device
    transposition writes), called bases + their block positions.  Src(): every data pointer null"""

    def __init__(self, post=None, dev=None, dev_out=None, bases=None, trans=None):
        self.post, self.dev, self.dev_out, self.bases, self.trans = _ptr(post), dev, dev_out, _ptr(bases), _ptr(trans)
        self._arrays = (post, bases, trans)            # the pointers above stay valid as long as this object lives


class Out:
    """host output buffers for n reads of T blocks (bases) in all and k experiments; Out(): every output pointer null"""
    FIELDS = ("bases", "trans", "nb", "pos", "demux", "table", "post")

    def __init__(self, T=None, n=0, k=1):
        self.T = T
        if T is None:
            for f in self.FIELDS:
                setattr(self, f, None)
            return
        self.bases, self.trans, self.nb = np.zeros(max(T, 1), np.uint8), np.zeros(max(T, 1), np.uint32), np.zeros(max(n, 1), np.int32)
        self.pos, self.demux, self.table = (np.zeros(max(c, 1) * w, np.int32) for c, w in ((n, 6), (n, 10), (n * k, 6)))
        self.post = np.zeros((max(T, 1), 40), np.float32)

    def result(self, fields, off):
        if "nb" in fields:                    # a basecall defines nb[i] bases from off[i] on, nothing between the reads
            live = np.zeros(len(self.bases), bool)
            for i, c in enumerate(self.nb[:len(off) - 1]):
                live[off[i]:off[i] + c] = True
            self.bases[~live], self.trans[~live] = 0, 0
        return b"".join(getattr(self, f).tobytes() for f in fields)


class Bar:
    """the barcodes of a call: one pair and a table"""

    def __init__(self, sb=SB, eb=EB, pairs=((SB2, EB2), (SB, EB))):
        self.sb, self.eb, self.k = sb.encode(), eb.encode(), len(pairs)
        self.exps = _exps(pairs)


def _transpost_device(L, h, s, off, n, o, b):
    st = L.lva_transpost_batch_device(h, s.dev, off, n, s.dev_out)
    if st == 0 and o.T:                       # a good call: its result comes back for the comparison
        assert L.lva_device_download(h, _ptr(o.post), s.dev_out, o.T * 160) == 0
    return st


# name -> (side of the input, the call, the output fields that make its result).  THE table of the ten entry points.
STAGES = {
    "lva_basecall_batch": ("post", lambda L, h, s, off, n, o, b:
                           L.lva_basecall_batch(h, s.post, off, n, _ptr(o.bases), _ptr(o.trans), _ptr(o.nb)), ("bases", "trans", "nb")),
    "lva_basecall_batch_device": ("post", lambda L, h, s, off, n, o, b:
                                  L.lva_basecall_batch_device(h, s.dev, off, n, _ptr(o.bases), _ptr(o.trans), _ptr(o.nb)), ("bases", "trans", "nb")),
    "lva_locate_payload_batch": ("post", lambda L, h, s, off, n, o, b:
                                 L.lva_locate_payload_batch(h, s.post, off, n, b.sb, b.eb, 0, _ptr(o.pos)), ("pos",)),
    "lva_locate_payload_batch_device": ("post", lambda L, h, s, off, n, o, b:
                                        L.lva_locate_payload_batch_device(h, s.dev, off, n, b.sb, b.eb, 0, _ptr(o.pos)), ("pos",)),
    "lva_transpost_batch": ("post", lambda L, h, s, off, n, o, b: L.lva_transpost_batch(h, s.post, off, n, _ptr(o.post)), ("post",)),
    "lva_transpost_batch_device": ("post", _transpost_device, ("post",)),
    "lva_demux_batch": ("post", lambda L, h, s, off, n, o, b:
                        L.lva_demux_batch(h, s.post, off, n, b.exps, b.k, -1, 0, _ptr(o.demux), _ptr(o.table)), ("demux", "table")),
    "lva_demux_batch_device": ("post", lambda L, h, s, off, n, o, b:
                               L.lva_demux_batch_device(h, s.dev, off, n, b.exps, b.k, -1, 0, _ptr(o.demux), _ptr(o.table)), ("demux", "table")),
    "lva_find_barcode_batch": ("bases", lambda L, h, s, off, n, o, b:
                               L.lva_find_barcode_batch(h, s.bases, s.trans, off, n, b.sb, b.eb, _ptr(o.pos)), ("pos",)),
    "lva_demux_bases_batch": ("bases", lambda L, h, s, off, n, o, b:
                              L.lva_demux_bases_batch(h, s.bases, s.trans, off, n, b.exps, b.k, -1, 0, _ptr(o.demux), _ptr(o.table)),
                              ("demux", "table")),
}
TWINS = [(n, n + "_device") for n in ("lva_basecall_batch", "lva_locate_payload_batch", "lva_transpost_batch", "lva_demux_batch")]
BOTH_STRANDS = [n for n in STAGES if "locate" in n or "demux" in n]      # these form reverse complements: "ACGU" has none


def test_the_table_is_the_headers_stage_entry_points():
    import os
    import re
    with open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "lva_decoder.h")) as f:
        named = set(re.findall(r"\bint (lva_(?:basecall|locate_payload|find_barcode|transpost|demux)\w*)\(", f.read()))
    assert named == set(STAGES) and len(STAGES) == 10


@pytest.fixture(scope="module")
def dec():
    with pkg.Decoder(6, 1, 20, list_size=1, max_slots=1) as d:
        yield d


def _call(dec, name, src, off, n, out, bar=None):
    return STAGES[name][1](dec._L, dec._h, src, off.ctypes.data, n, out, bar or Bar())


@pytest.fixture(scope="module")
def good(dec):
    """four reads of 0, 1, 3 and 300 blocks, 25-base barcodes around a short payload on the last; on the host, on the device,
    and as the device's own basecalls.  run(name) -> (status, result bytes) of a good call, every call on fresh output buffers"""
    rng = np.random.default_rng(2200)
    strand = np.concatenate([rng.integers(0, 4, 5), synth.bases_from_str(SB), rng.integers(0, 4, 40), synth.bases_from_str(EB),
                             rng.integers(0, 4, 30)]).astype(np.uint8)
    long = synth.posteriors_from_bases(strand, rng, margin=6.0, mean_extra_dwell=2.0)      # (the end barcode ends before block 300)
    assert long.shape[0] >= 304
    posts = [long[:0], long[300:301], long[301:304], long[:300]]
    flat, off = dec._pack(posts)
    assert off.tolist() == [0, 0, 1, 4, 304]
    T, n = 304, 4
    dev, _ = dec.upload(posts)
    dev_out = dec.alloc(T * 160)
    calls = dec.basecall(posts)
    boff = np.zeros(n + 1, np.int64)
    boff[1:] = np.cumsum([len(c[0]) for c in calls])
    bases = np.frombuffer("".join(c[0] for c in calls).encode("ascii"), dtype=np.uint8).copy()
    trans = np.concatenate([c[1].astype(np.uint32) for c in calls])
    src = Src(post=flat, dev=dev, dev_out=dev_out, bases=bases, trans=trans)

    def run(name, bar=None):
        offsets = off if STAGES[name][0] == "post" else boff
        o = Out(int(offsets[-1]), n, 2)
        st = _call(dec, name, src, offsets, n, o, bar)
        return st, o.result(STAGES[name][2], offsets)

    first = {name: run(name) for name in STAGES}
    assert all(st == 0 for st, _ in first.values()), {k: v[0] for k, v in first.items()}
    # the batch is not trivial: both barcodes of the last read are found, forward, by locate and by the table's second pair
    pos = np.frombuffer(first["lva_locate_payload_batch"][1], np.int32).reshape(n, 6)
    assert pos[3].tolist() == [82, 201, 0, 0, 0, 1] and pos[0, 0] == -1       # (what the CPU oracle's locate_payload gives)
    dm = np.frombuffer(first["lva_demux_batch"][1][:n * 40], np.int32).reshape(n, 10)
    assert dm[3, 6] == 1 and dm[3, 7] == 0 and dm[3, :6].tolist() == pos[3].tolist()
    yield run, first
    dec.free(dev)
    dec.free(dev_out)


def test_twins_agree(good):
    _, first = good
    for host, device in TWINS:
        assert first[host][1] == first[device][1], host


def _same_as_before(good):
    run, first = good
    for name in STAGES:
        assert run(name) == first[name], name


@pytest.fixture(scope="module")
def oversize(dec):
    """one read of 2^20 + 1 blocks whose buffers are really that large -- zeros on the host, zeros on the device (one buffer for
    every device variant, input and output of the transposition), 2^20 + 1 zero bases -- and outputs of that size"""
    T = MAX_BLOCKS + 1
    post = np.zeros((T, 40), np.float32)
    dev = dec.alloc(post.nbytes)
    assert dec._L.lva_device_upload(dec._h, dev, post.ctypes.data, post.nbytes) == 0
    bases, trans = np.zeros(T, np.uint8), np.zeros(T, np.uint32)
    yield Src(post=post, dev=dev, dev_out=dev, bases=bases, trans=trans)
    dec.free(dev)


@pytest.mark.parametrize("name", sorted(STAGES))
def test_offsets_are_refused(dec, good, oversize, name):
    small = np.zeros((8, 40), np.float32)
    dev = dec.alloc(small.nbytes)
    try:
        assert dec._L.lva_device_upload(dec._h, dev, small.ctypes.data, small.nbytes) == 0
        src = Src(post=small, dev=dev, dev_out=dev, bases=np.zeros(8, np.uint8), trans=np.zeros(8, np.uint32))
        for offsets in ([1, 5], [0, 7, 5]):
            off = np.array(offsets, np.int64)
            assert _call(dec, name, src, off, len(offsets) - 1, Out(8, 2, 2)) == ARG, offsets
        big = np.array([0, MAX_BLOCKS + 1], np.int64)
        assert _call(dec, name, oversize, big, 1, Out(MAX_BLOCKS + 1, 1, 2)) == ARG
        if STAGES[name][0] == "post":
            # 2 049 reads of 2^20 blocks: 2^31 + 2^20 blocks in all
            many = np.arange(2050, dtype=np.int64) * MAX_BLOCKS
            assert _call(dec, name, src, many, 2049, Out(8, 2049, 2)) == ARG
    finally:
        dec.free(dev)
    run, first = good
    assert run(name) == first[name]


def test_good_calls_after_all_the_refusals(good):
    _same_as_before(good)


def test_no_reads_is_a_no_op(dec, good):
    off = np.zeros(1, np.int64)
    for name in STAGES:
        assert _call(dec, name, Src(), off, 0, Out()) == 0, name
    _same_as_before(good)


def test_an_argument_error_wins_over_an_open_stream(dec, good):
    run, first = good
    with dec.stream():
        for name in STAGES:
            assert run(name)[0] == BUSY, name
        for name in BOTH_STRANDS:
            assert run(name, Bar(sb="ACGU", pairs=((SB2, EB2), ("ACGU", EB))))[0] == ARG, name
    assert len(BOTH_STRANDS) == 5
    _same_as_before(good)
