"""What the gfx950 code objects of the index-building kernels must keep (no GPU needed: hipcc cross-compiles), from the
kernels' metadata alone: csrc/mi_kernels.hip holds exactly the eight kernels of its header's steps, none of them uses scratch
memory, and each one's LDS is the constant mi_kernels.h names for it -- the oligo as codes and a k-mer per position for
mi_count and mi_fill (5 KiB, so that LDS never limits the wavefronts of a CU), a partial sum per wavefront for the scan."""
import os
import re
import subprocess

import pytest

from nanopore_dna_storage_amd.error_profile import MAX_REF

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "nanopore_dna_storage_amd", "csrc")
HIPCC = "/opt/rocm/bin/hipcc"
# kernel -> the header's constant for its LDS (None: none)
KERNELS = {"mi_masks": None, "mi_count": "kMiOligoLdsBytes", "mi_fill": "kMiOligoLdsBytes", "mi_clip": "kMiClipLdsBytes",
           "mi_scan_sums": "kMiScanLdsBytes", "mi_scan_top": "kMiScanLdsBytes", "mi_scan_add": "kMiScanLdsBytes", "mi_rank": None}


@pytest.fixture(scope="module")
def meta(tmp_path_factory):
    if not os.path.exists(HIPCC):
        pytest.skip("no hipcc")
    out = str(tmp_path_factory.mktemp("asm") / "mi_k.s")
    subprocess.run([HIPCC, "--offload-arch=gfx950", "-O3", "-std=c++17", "-ffp-contract=off", "-fno-fast-math", "--cuda-device-only",
                    "-S", "-o", out, os.path.join(CSRC, "mi_kernels.hip")], check=True, cwd=CSRC)
    res = {}
    for b in open(out).read().split("- .agpr_count:")[1:]:
        g = lambda k: re.search(r"\.%s:\s+(\S+)" % k, b).group(1)
        name = re.search(r"\d+(mi_[a-z_]+?)E", g("name")).group(1)             # the mangled name holds <length><name>E
        assert name not in res, name
        res[name] = dict(vgpr=int(g("vgpr_count")), agpr=int(b.split()[0]), lds=int(g("group_segment_fixed_size")),
                         scratch=int(g("private_segment_fixed_size")))
    return res


@pytest.fixture(scope="module")
def const():
    with open(os.path.join(CSRC, "mi_kernels.h")) as f:
        text = f.read()
    return lambda name: int(re.search(r"constexpr int %s = (\d+);" % name, text).group(1))


def test_the_kernels_are_the_eight_expected_and_none_uses_scratch(meta):
    assert sorted(meta) == sorted(KERNELS), list(meta)
    for name, got in meta.items():
        print(name, got)
        assert got["scratch"] == 0, (name, got)


@pytest.mark.parametrize("name", sorted(KERNELS))
def test_lds_is_what_the_header_says(meta, const, name):
    assert meta[name]["lds"] == (const(KERNELS[name]) if KERNELS[name] else 0), (name, meta[name])


def test_the_header_constants_are_what_the_kernels_need(const):
    assert const("kMiOligoLdsBytes") == MAX_REF + 4 * MAX_REF             # a code per base, a k-mer per position
    assert const("kMiScanLdsBytes") == 4 * (const("kMiThreads") // 64) and const("kMiClipLdsBytes") == 2 * const("kMiScanLdsBytes")
    assert const("kMiScanTile") == 16 * const("kMiThreads") and 4 ** 6 % const("kMiScanTile") == 0      # every table is whole tiles
    assert 160 * 1024 // const("kMiOligoLdsBytes") >= 32                   # a wavefront per workgroup: LDS admits all 32 of a CU
