"""Host side of the stages beside the decoder without a GPU: every decoder-bound stage entry point refuses a null decoder
with LVA_ERR_ARG instead of crashing, and the build covers the files that hold them.  (The list consumers take a device
ordinal, not a decoder: their refusals are in test_list_ops_host.py.)"""
import os
import re

import numpy as np
import pytest

from nanopore_dna_storage_amd import _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OFF = np.zeros(2, np.int64)                 # n_reads = 0 and n_reads = 1 (one empty read) both read valid memory
BUF = np.zeros(64, np.uint8)
EXPS = (_lib.ExperimentBarcodes * 1)(_lib.ExperimentBarcodes(b"ACGT", b"TGCA", 0))
P, O = BUF.ctypes.data, OFF.ctypes.data

# name -> arguments after the decoder, every pointer valid: only the decoder is missing
STAGE_CALLS = {
    "lva_basecall_batch": (P, O, 1, P, P, P),
    "lva_basecall_batch_device": (P, O, 1, P, P, P),
    "lva_locate_payload_batch": (P, O, 1, b"ACGT", b"TGCA", 0, P),
    "lva_locate_payload_batch_device": (P, O, 1, b"ACGT", b"TGCA", 0, P),
    "lva_find_barcode_batch": (P, P, O, 1, b"ACGT", b"TGCA", P),
    "lva_transpost_batch": (P, O, 1, P),
    "lva_transpost_batch_device": (P, O, 1, P),
    "lva_demux_batch": (P, O, 1, EXPS, 1, -1, 0, P, None),
    "lva_demux_batch_device": (P, O, 1, EXPS, 1, -1, 0, P, None),
    "lva_demux_bases_batch": (P, P, O, 1, EXPS, 1, -1, 0, P, None),
}


@pytest.mark.parametrize("name", sorted(STAGE_CALLS))
def test_null_decoder_is_an_argument_error(name):
    fn = getattr(_lib.load_library(), name)
    args = STAGE_CALLS[name]
    assert fn(None, *args) == -10
    # and with nothing at all behind the other pointers: the decoder is looked at first
    nulls = tuple(None if isinstance(a, int) and a in (P, O) else a for a in args)
    assert fn(None, *nulls) == -10


def test_every_stage_entry_point_of_the_header_is_in_the_table():
    with open(os.path.join(ROOT, "include", "lva_decoder.h")) as f:
        header = f.read()
    named = set(re.findall(r"\bint (lva_(?:basecall|locate_payload|find_barcode|transpost|demux)\w*)\(", header))
    assert named == set(STAGE_CALLS)
    for name in named:
        assert name in _lib.EXPORTS


def test_build_id_covers_the_stage_files():
    with open(os.path.join(ROOT, "nanopore_dna_storage_amd", "csrc", "Makefile")) as f:
        mk = f.read()
    assert re.search(r"^SRC\s*=.*\blva_api\.cpp\b.*\blva_stages\.cpp\b", mk, re.M)
    assert re.search(r"^HDR\s*=.*\blva_host\.h\b", mk, re.M)
    for name in ("lva_stages.cpp", "lva_host.h"):
        assert os.path.exists(os.path.join(ROOT, "nanopore_dna_storage_amd", "csrc", name))
