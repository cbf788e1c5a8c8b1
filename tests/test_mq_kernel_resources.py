"""What the gfx950 code objects of the pooled mapping kernels must keep (no GPU needed: hipcc cross-compiles), after
tests/test_map_kernel_resources.py.  csrc/mq_kernels.hip alone holds mq_flank and the three forms of mq_verify; nothing is in
scratch memory; with every lane's oligo at its own length the register forms stay in the occupancy classes of their mp_verify
counterparts -- at most 64 registers for oligos of at most 128 bases (eight wavefronts per SIMD), at most 128 for at most 256
(four) -- and the LDS of a form is mp_verify's."""
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
    out = str(tmp_path_factory.mktemp("asm") / "mq_k.s")
    src = os.path.join(ROOT, "nanopore_dna_storage_amd", "csrc", "mq_kernels.hip")
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
    names = [k for k in meta if "mq_" in k]
    assert len(names) == len(meta) == 4, list(meta)
    assert sum("mq_verify" in k for k in names) == 3 and sum("mq_flank" in k for k in names) == 1
    for k in names:
        assert meta[k]["scratch"] == 0, (k, meta[k])


@pytest.mark.parametrize("form, bound", [("mq_verifyILi2E", 64), ("mq_verifyILi4E", 128), ("mq_verifyILi0E", 64)])
def test_verify_registers(meta, form, bound):
    got = kernel(meta, form)
    assert got["vgpr"] + got["agpr"] <= bound, got
    assert got["lds"] <= (24 if form.endswith("0E") else 8) * 1024, got


def test_flank_is_small(meta):
    got = kernel(meta, "mq_flank")
    assert got["vgpr"] + got["agpr"] <= 32 and got["lds"] == 0, got
