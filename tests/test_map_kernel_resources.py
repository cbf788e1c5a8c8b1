"""What the gfx950 code objects of the mapping kernels must keep (no GPU needed: hipcc cross-compiles).  mp_vote / mp_verify
(csrc/mp_kernels.hip): nothing in scratch memory; the LDS of mp_vote is the window, uint16 counters [2][VOTE_RANGE], the
running top list and one minimum per wavefront, so that seven workgroups share a CU's 160 KiB; the register form of the
distance for oligos of at most 128 bases stays within 64 registers (eight wavefronts per SIMD), the one for at most 256
bases within 128 (four)."""
import os
import re
import subprocess

import pytest

from nanopore_dna_storage_amd import read_map as rm
from nanopore_dna_storage_amd.error_profile import MAX_READ

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HIPCC = "/opt/rocm/bin/hipcc"


@pytest.fixture(scope="module")
def meta(tmp_path_factory):
    if not os.path.exists(HIPCC):
        pytest.skip("no hipcc")
    out = str(tmp_path_factory.mktemp("asm") / "mp_k.s")
    src = os.path.join(ROOT, "nanopore_dna_storage_amd", "csrc", "mp_kernels.hip")
    subprocess.run([HIPCC, "--offload-arch=gfx950", "-O3", "-std=c++17", "-ffp-contract=off", "-fno-fast-math", "--cuda-device-only",
                    "-S", "-o", out, src], check=True, cwd=os.path.dirname(src))
    res = {}
    for b in open(out).read().split("- .agpr_count:")[1:]:
        g = lambda k: re.search(r"\.%s:\s+(\S+)" % k, b).group(1)
        res[g("name")] = dict(vgpr=int(g("vgpr_count")), agpr=int(b.split()[0]), lds=int(g("group_segment_fixed_size")),
                              scratch=int(g("private_segment_fixed_size")))
    return res


def kernel(meta, part):
    got = [v for k, v in meta.items() if part in k]
    assert len(got) == 1, (part, list(meta))
    print(part, got[0])
    return got[0]


def test_the_kernels_are_the_four_expected_and_none_uses_scratch(meta):
    names = [k for k in meta if "mp_" in k]
    assert len(names) == len(meta) == 4, list(meta)
    for k in names:
        assert meta[k]["scratch"] == 0, (k, meta[k])


def test_vote_lds_is_what_the_range_implies(meta):
    lds = kernel(meta, "mp_vote")["lds"]
    assert lds == MAX_READ + 2 * 2 * rm.VOTE_RANGE + 8 * rm.MAX_CANDS + 8 * 4
    assert 160 * 1024 // lds == 7


@pytest.mark.parametrize("form, bound", [("mp_verifyILi2E", 64), ("mp_verifyILi4E", 128), ("mp_verifyILi0E", 64)])
def test_verify_registers(meta, form, bound):
    got = kernel(meta, form)
    assert got["vgpr"] + got["agpr"] <= bound, got
    assert got["lds"] <= (24 if form.endswith("0E") else 8) * 1024, got
