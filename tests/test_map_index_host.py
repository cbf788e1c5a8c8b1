"""The device-built read-mapping index without a GPU: every refusal of lva_map_index_create_device before a device is looked
for and the device ordinal after them, lva_map_index_tables on a host-built index against read_map.ReferenceIndex expanded
to the direct table, and the declarations."""
import ctypes
import os
import re

import numpy as np
import pytest

from nanopore_dna_storage_amd import _lib, read_map as rm
from nanopore_dna_storage_amd.error_profile import MAX_REF

import map_index_util as U

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "nanopore_dna_storage_amd", "csrc")
ERR_ARG, ERR_NO_DEVICE = -10, -11


def test_create_device_refusals_come_before_the_device():
    L = _lib.load_library()
    refs = np.zeros(40, np.uint8)
    off = np.array([0, 20, 40], np.int64)
    h = ctypes.c_void_p()

    def create(device=9999, r=refs.ctypes.data, o=off.ctypes.data, n=2, k=10, max_occ=64, out=ctypes.byref(h)):
        return L.lva_map_index_create_device(device, r, o, n, k, max_occ, out)
    # every bad argument of tests/test_read_map_host.py::test_index_create_refusals
    for kw in (dict(k=5), dict(k=13), dict(max_occ=0), dict(max_occ=65536), dict(n=0), dict(r=None), dict(out=None), dict(o=None), dict(n=-1)):
        assert create(**kw) == ERR_ARG, kw
        assert create(device=0, **kw) == ERR_ARG, kw
    for bad in ([1, 20, 40], [0, 20, 19], [0, 0, 40], [0, 20, 20], [0, MAX_REF + 1, MAX_REF + 2], [0, 20, 2 ** 31]):
        o = np.array(bad, np.int64)
        assert create(o=o.ctypes.data) == ERR_ARG, bad
    assert create() == ERR_NO_DEVICE                      # arguments pass: now the device ordinal is refused
    assert create(device=-1) == ERR_NO_DEVICE
    assert h.value is None
    with pytest.raises(_lib.LvaError) as e:
        rm.MapIndex(np.zeros((2, 20), np.uint8), device=9999)
    assert e.value.code == ERR_NO_DEVICE
    with pytest.raises(ValueError):
        rm.MapIndex(np.zeros((2, 20), np.uint8), k=13, device=9999)


def test_tables_refusals_and_null_outputs():
    L = _lib.load_library()
    assert L.lva_map_index_tables(None, None, None, None) == ERR_ARG
    with rm.MapIndex(np.zeros((2, 20), np.uint8)) as idx:
        assert L.lva_map_index_tables(idx.handle, None, None, None) == 0           # each may be NULL
        offsets = np.full(4 ** 10 + 1, 7, np.uint32)
        assert L.lva_map_index_tables(idx.handle, offsets.ctypes.data, None, None) == 0
        assert offsets[0] == 0 and offsets[1] == offsets[-1] == 2                  # the one k-mer AAAAAAAAAA, held by both oligos
        assert idx.device is None
    with pytest.raises(ValueError):
        idx.tables()                                                                # closed


def test_map_reads_refuses_an_index_of_another_device_before_the_library():
    class Elsewhere(rm.MapIndex):
        def __init__(self, refs):
            super().__init__(refs)
            self.device = 3
    with Elsewhere(np.zeros((2, 20), np.uint8)) as idx:
        with pytest.raises(ValueError):
            rm.map_reads(np.zeros(30, np.uint8), [[0, 30]], idx, device=0)


@pytest.mark.parametrize("k", [6, 12])
def test_tables_of_a_host_index_on_ragged_lengths(k):
    oligos = U.ragged(k)
    with rm.MapIndex(oligos, k) as idx:
        got, info = idx.tables(), idx.info()
    want = U.direct_tables(oligos, k, 64)
    U.same_tables(got, want[:3], "ragged k=%d" % k)
    assert info == want[3] and got[0][-1] == info[1] and got[2].shape == (len(oligos), 2, 4, 16)


@pytest.mark.parametrize("k", [6, 12])
@pytest.mark.parametrize("where", U.N_WHERE)
def test_tables_of_a_host_index_with_n(k, where):
    oligos = U.with_n(k, where)
    with rm.MapIndex(oligos, k) as idx:
        got, info = idx.tables(), idx.info()
    want = U.direct_tables(oligos, k, 64)
    U.same_tables(got, want[:3], "N %s k=%d" % (where, k))
    assert info == want[3] and (info == (0, 0, 0)) == (where == "every k")


def test_tables_of_a_host_index_with_drops():
    refs = U.shared_prefix()[:300]
    for max_occ in (299, 300, 8):
        with rm.MapIndex(refs, 6, max_occ) as idx:
            got, info = idx.tables(), idx.info()
        want = U.direct_tables(refs, 6, max_occ)
        U.same_tables(got, want[:3], "max_occ %d" % max_occ)
        assert info == want[3] and (info[2] >= 15) == (max_occ < 300)


def test_declarations():
    with open(os.path.join(ROOT, "include", "lva_decoder.h")) as f:
        header = f.read()
    assert "#define LVA_ABI_VERSION 5" in header and _lib.ABI_VERSION == 5
    flat = re.sub(r"\s+", " ", re.sub(r"/\*.*?\*/", " ", header, flags=re.S))
    for proto in ("int lva_map_index_create_device(int32_t device, const uint8_t *refs, const int64_t *ref_off , int32_t n_refs, int32_t k, "
                  "int32_t max_occ, lva_map_index **out);",
                  "int lva_map_index_tables(const lva_map_index *idx, uint32_t *offsets , int32_t *lists , uint64_t *masks );"):
        assert proto in flat, proto
    at = _lib.EXPORTS.index("lva_map_index_create_pooled")
    assert _lib.EXPORTS[at - 2:at] == ["lva_map_index_create_device", "lva_map_index_tables"] and at == len(_lib.EXPORTS) - 6
    L = _lib.load_library()
    assert L.lva_map_index_create_device.argtypes and L.lva_map_index_tables.argtypes
    with open(os.path.join(CSRC, "Makefile")) as f:
        make = f.read()
    assert re.search(r"^SRC\s*=.*\bmi_kernels\.hip\b", make, re.M) and re.search(r"^HDR\s*=.*\bmi_kernels\.h\b", make, re.M)
    p = rm.build_parser()
    assert p.parse_args(["--oligos", "o", "--post_manifest", "m", "--out_prefix", "p"]).index == "host"
    assert p.parse_args(["--oligos", "o", "--post_manifest", "m", "--out_prefix", "p", "--index", "device"]).index == "device"
