"""What the gfx950 assembly of the simulator's pool kernel must keep (no GPU needed: hipcc cross-compiles).  sim_strand_pool
(csrc/sim_pool_kernels.hip) is sim_strand's body (csrc/sim_strand.h) with the message taken from a pool: nothing in scratch
memory and no LDS beyond what sim_strand (csrc/sim_kernels.hip) has."""
import os
import re
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HIPCC = "/opt/rocm/bin/hipcc"


def _meta(tmp, name):
    out = str(tmp / (name + ".s"))
    src = os.path.join(ROOT, "nanopore_dna_storage_amd", "csrc", name + ".hip")
    subprocess.run([HIPCC, "--offload-arch=gfx950", "-O3", "-std=c++17", "-ffp-contract=off", "-fno-fast-math", "--cuda-device-only",
                    "-S", "-o", out, src], check=True, cwd=os.path.dirname(src))
    res = {}
    for b in open(out).read().split("- .agpr_count:")[1:]:
        g = lambda k: re.search(r"\.%s:\s+(\S+)" % k, b).group(1)
        res[g("name")] = dict(vgpr=int(g("vgpr_count")), sgpr=int(g("sgpr_count")), lds=int(g("group_segment_fixed_size")),
                              scratch=int(g("private_segment_fixed_size")))
    return res


@pytest.fixture(scope="module")
def kernels(tmp_path_factory):
    if not os.path.exists(HIPCC):
        pytest.skip("no hipcc")
    tmp = tmp_path_factory.mktemp("asm")
    return _meta(tmp, "sim_kernels"), _meta(tmp, "sim_pool_kernels")


def test_the_pool_kernel_has_no_scratch_and_the_lds_of_sim_strand(kernels):
    plain, pooled = kernels
    assert len(pooled) == 1 and "sim_strand_pool" in next(iter(pooled)), list(pooled)
    base = [v for k, v in plain.items() if "sim_strand" in k]
    assert len(base) == 1, list(plain)
    got = next(iter(pooled.values()))
    print("sim_strand", base[0])
    print("sim_strand_pool", got)
    assert got["scratch"] == 0 and base[0]["scratch"] == 0
    assert got["lds"] == base[0]["lds"] > 0
    assert got["vgpr"] <= 128
