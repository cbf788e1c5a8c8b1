"""What the gfx950 code objects of the demultiplexing kernels must keep (no GPU needed: hipcc cross-compiles).
bc_search_multi / bc_demux_finalize (csrc/bc_kernels.hip): nothing in scratch memory -- the window's characters and the
recurrence stay in registers -- and at most 128 registers, so that four wavefronts per SIMD stay possible."""
import os
import re
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HIPCC = "/opt/rocm/bin/hipcc"


@pytest.fixture(scope="module")
def meta(tmp_path_factory):
    if not os.path.exists(HIPCC):
        pytest.skip("no hipcc")
    out = str(tmp_path_factory.mktemp("asm") / "bc_k.s")
    src = os.path.join(ROOT, "nanopore_dna_storage_amd", "csrc", "bc_kernels.hip")
    subprocess.run([HIPCC, "--offload-arch=gfx950", "-O3", "-std=c++17", "-ffp-contract=off", "-fno-fast-math", "--cuda-device-only",
                    "-S", "-o", out, src], check=True, cwd=os.path.dirname(src))
    res = {}
    for b in open(out).read().split("- .agpr_count:")[1:]:
        g = lambda k: re.search(r"\.%s:\s+(\S+)" % k, b).group(1)
        res[g("name")] = dict(vgpr=int(g("vgpr_count")), sgpr=int(g("sgpr_count")), lds=int(g("group_segment_fixed_size")),
                              scratch=int(g("private_segment_fixed_size")))
    return res


@pytest.mark.parametrize("kernel", ["bc_search_multi", "bc_demux_finalize"])
def test_no_scratch_and_at_most_128_vgprs(meta, kernel):
    got = [v for k, v in meta.items() if kernel in k]
    assert len(got) == 1, (kernel, list(meta))
    print(kernel, got[0])
    assert got[0]["scratch"] == 0 and got[0]["vgpr"] <= 128, (kernel, got[0])


def test_search_multi_lds_fits_many_workgroups(meta):
    """peq masks of 128 patterns, their minima, ranges and lengths: a few KB, far below what would limit occupancy"""
    got = [v for k, v in meta.items() if "bc_search_multi" in k][0]
    assert 0 < got["lds"] <= 8192, got
