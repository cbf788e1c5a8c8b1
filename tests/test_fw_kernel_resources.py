"""What the gfx950 code object of the forward-score kernel must keep (no GPU needed: hipcc cross-compiles), after
tests/test_mq_kernel_resources.py and tests/test_sc_kernel_resources.py.  csrc/fw_kernels.hip holds fw_forward alone; nothing is
in scratch memory; all its LDS is dynamic -- the static figure is 0 -- and what a launch asks for is fw_lds_bytes of the
header, evaluated by a host program compiled from it: sc_score's 5.9 KB at 187 bases and 20 KB at the longest sequence, far
below the 64 KB at which two workgroups still fit a CU.  Resource figures only: what the kernel computes is
tests/test_gpu_trellis_forward.py's."""
import os
import re
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HIPCC = "/opt/rocm/bin/hipcc"
CSRC = os.path.join(ROOT, "nanopore_dna_storage_amd", "csrc")
FLAGS = ["-O3", "-std=c++17", "-ffp-contract=off", "-fno-fast-math"]

PROBE = """#include <cstdio>
#include "fw_kernels.h"
int main() {
  std::printf("%zu %zu %zu %zu\\n", lva::fw_lds_bytes(187), lva::fw_lds_bytes(1024), lva::sc_lds_bytes(187), lva::sc_lds_bytes(1024));
  return 0;
}
"""


@pytest.fixture(scope="module")
def meta(tmp_path_factory):
    if not os.path.exists(HIPCC):
        pytest.skip("no hipcc")
    out = str(tmp_path_factory.mktemp("asm") / "fw_k.s")
    subprocess.run([HIPCC, "--offload-arch=gfx950", *FLAGS, "--cuda-device-only", "-S", "-o", out,
                    os.path.join(CSRC, "fw_kernels.hip")], check=True, cwd=CSRC)
    text = open(out).read()
    res = {}
    for b in text.split("- .agpr_count:")[1:]:
        g = lambda k: re.search(r"\.%s:\s+(\S+)" % k, b).group(1)
        res[g("name")] = dict(vgpr=int(g("vgpr_count")), agpr=int(b.split()[0]), sgpr=int(g("sgpr_count")),
                              lds=int(g("group_segment_fixed_size")), scratch=int(g("private_segment_fixed_size")))
    return res, text


def test_one_kernel_without_scratch_and_without_static_lds(meta):
    res, _ = meta
    assert len(res) == 1 and "fw_forward" in list(res)[0], list(res)
    got = list(res.values())[0]
    print(got)
    assert got["scratch"] == 0
    assert got["lds"] == 0, got                  # every byte is dynamic: nothing static in front of the 16-byte aligned base
    assert got["vgpr"] + got["agpr"] <= 512 and got["sgpr"] <= 102, got


def test_dynamic_lds_of_a_launch(tmp_path):
    if not os.path.exists(HIPCC):
        pytest.skip("no hipcc")
    src, exe = str(tmp_path / "probe.cpp"), str(tmp_path / "probe")
    with open(src, "w") as f:
        f.write(PROBE)
    subprocess.run([HIPCC, "-std=c++17", "-I", CSRC, "-o", exe, src], check=True)
    fw187, fw1024, sc187, sc1024 = map(int, subprocess.run([exe], check=True, capture_output=True, text=True).stdout.split())
    lds = lambda n: 16 * 160 + 64 + ((n + 1 + 15) & ~15) * 17          # staged rows, position 0, (flip, flop) x 2 + a base byte
    assert (fw187, fw1024) == (lds(187), lds(1024)) == (sc187, sc1024)
    assert fw187 % 16 == 0 and fw1024 % 16 == 0
    assert fw1024 <= 64 * 1024 and (160 * 1024) // fw1024 >= 2             # at least two workgroups of the longest sequence per CU
    with open(os.path.join(CSRC, "fw_kernels.hip")) as f:
        hip = f.read()
    assert "fw_lds_bytes(max_len)" in hip.split("hipLaunchKernelGGL(fw_forward", 1)[1].split(";", 1)[0]
