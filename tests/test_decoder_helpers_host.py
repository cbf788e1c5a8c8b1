"""The pure parts of the Python host layer, without a GPU: the packer of (basecall, trans list) pairs behind find_barcode
and demux_bases, and the window arithmetic of Decoder.decode_located with a stub in place of the decode call."""
import numpy as np
import pytest

from nanopore_dna_storage_amd import Decoder


def test_pack_bases_of_an_empty_batch_leaves_placeholders():
    bases, trans, off = Decoder._pack_bases([], [])
    assert off.dtype == np.int64 and off.tolist() == [0]
    assert bases.dtype == np.uint8 and bases.tolist() == [0]             # one element each: a pointer the library may be handed
    assert trans.dtype == np.uint32 and trans.tolist() == [0]


def test_pack_bases_cuts_a_longer_trans_list_and_refuses_a_shorter_one():
    bases, trans, off = Decoder._pack_bases(["ACG", "", "TT"], [[5, 6, 7, 8, 9], [3], np.array([1, 2], np.int64)])
    assert off.dtype == np.int64 and off.tolist() == [0, 3, 3, 5]
    assert bases.dtype == np.uint8 and bases.tobytes() == b"ACGTT" and bases.flags.writeable
    assert trans.dtype == np.uint32 and trans.tolist() == [5, 6, 7, 1, 2, 0]      # cut to the basecalls, then the placeholder
    with pytest.raises(ValueError, match="trans list shorter than the basecall"):
        Decoder._pack_bases(["ACG", "TT"], [[5, 6, 7], [1]])


class _Stub(Decoder):
    """decode_located on a decoder without a device: decode_windows_resident records its calls and names each window"""

    def __init__(self):
        self.calls = []

    def decode_windows_resident(self, dev_ptr, first_block, n_blocks, rc=None):
        self.calls.append((dev_ptr, list(first_block), list(n_blocks), list(rc)))
        return [("window", f, n, r) for f, n, r in zip(first_block, n_blocks, rc)]


def _loc(ok, start=-1, end=-1, rc=False):
    return dict(ok=ok, start_pos=start, end_pos=end, rc=rc, dist_start=0, dist_end=0)


OFF = np.array([0, 100, 250, 250, 400, 1000], np.int64)
LOC = [_loc(True, 10, 79, True), _loc(False), _loc(False, 0, 5), _loc(True, 0, 149), _loc(True, 7, 7, True)]


def test_decode_located_decodes_the_found_windows_in_one_call():
    dec = _Stub()
    out = dec.decode_located("buffer", OFF, LOC)
    assert dec.calls == [("buffer", [10, 250, 407], [70, 150, 1], [True, False, True])]
    assert all(type(f) is int for f in dec.calls[0][1] + dec.calls[0][2])
    assert [lc for lc, _ in out] == LOC and all(a is b for (a, _), b in zip(out, LOC))
    assert [r for _, r in out] == [("window", 10, 70, True), None, None, ("window", 250, 150, False), ("window", 407, 1, True)]


def test_decode_located_on_a_subset():
    dec = _Stub()
    out = dec.decode_located("buffer", OFF, LOC, subset=[4, 1, 0])             # in the subset's order, not-found reads left out
    assert dec.calls == [("buffer", [407, 10], [1, 70], [True, True])]
    assert [r for _, r in out] == [("window", 10, 70, True), None, None, None, ("window", 407, 1, True)]
    assert dec.decode_located("buffer", OFF, LOC, subset=[]) == [(lc, None) for lc in LOC] and len(dec.calls) == 1


def test_decode_located_makes_no_call_when_nothing_was_found():
    dec = _Stub()
    loc = [_loc(False), _loc(False, 3, 90)]
    assert dec.decode_located("buffer", OFF[:3], loc) == [(loc[0], None), (loc[1], None)]
    assert dec.decode_located("buffer", OFF[:1], []) == []
    assert dec.decode_located("buffer", OFF, LOC, subset=[1, 2]) == [(lc, None) for lc in LOC]
    assert dec.calls == []
