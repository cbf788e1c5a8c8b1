"""What the gfx950 code object of the one-message trellis kernel must keep (no GPU needed: hipcc cross-compiles), after
tests/test_mq_kernel_resources.py.  csrc/sc_kernels.hip holds sc_score alone; nothing is in scratch memory; a wavefront stays
within 64 vector registers (eight wavefronts per SIMD: the kernel is a chain of dependent LDS round trips, and other
wavefronts are what hides them) and within the scalar registers of a wave; all its LDS is dynamic -- the static figure is 0,
so the dynamic base is 16-byte aligned -- and what a launch asks for is the header's formula: 5.9 KB at the 187 positions of
m = 6, rate 1, msg_len 180, 20 KB for the longest sequence: 27 and 8 workgroups per CU."""
import os
import re
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HIPCC = "/opt/rocm/bin/hipcc"
CSRC = os.path.join(ROOT, "nanopore_dna_storage_amd", "csrc")


@pytest.fixture(scope="module")
def meta(tmp_path_factory):
    if not os.path.exists(HIPCC):
        pytest.skip("no hipcc")
    out = str(tmp_path_factory.mktemp("asm") / "sc_k.s")
    subprocess.run([HIPCC, "--offload-arch=gfx950", "-O3", "-std=c++17", "-ffp-contract=off", "-fno-fast-math", "--cuda-device-only",
                    "-S", "-o", out, os.path.join(CSRC, "sc_kernels.hip")], check=True, cwd=CSRC)
    text = open(out).read()
    res = {}
    for b in text.split("- .agpr_count:")[1:]:
        g = lambda k: re.search(r"\.%s:\s+(\S+)" % k, b).group(1)
        res[g("name")] = dict(vgpr=int(g("vgpr_count")), agpr=int(b.split()[0]), sgpr=int(g("sgpr_count")),
                              lds=int(g("group_segment_fixed_size")), scratch=int(g("private_segment_fixed_size")))
    return res, text


def test_one_kernel_without_scratch_within_the_register_classes(meta):
    res, _ = meta
    assert len(res) == 1 and "sc_score" in list(res)[0], list(res)
    got = list(res.values())[0]
    print(got)
    assert got["scratch"] == 0
    assert got["vgpr"] + got["agpr"] <= 64, got
    assert got["sgpr"] <= 102, got
    assert got["lds"] == 0, got                  # every byte is dynamic: nothing static in front of the 16-byte aligned base


def test_arithmetic_is_add_and_compare_select(meta):
    _, text = meta
    assert "v_add_f32" in text and "v_cmp_lt_f32" in text and not re.search(r"\bv_(fma|fmac|mad|mac)_f32", text)


def test_lds_of_a_launch():
    with open(os.path.join(CSRC, "sc_kernels.h")) as f:
        h = f.read()
    stage = int(re.search(r"kScStage = (\d+);", h).group(1))
    assert "(size_t)kScStage * 40 * 4 + 2 * 8 * 4 + sc_lds_positions(max_len) * (2 * 8 + 1)" in h
    assert "((size_t)max_len + 1 + 15) & ~(size_t)15" in h
    lds = lambda n: stage * 160 + 64 + ((n + 1 + 15) & ~15) * 17
    assert lds(186) == 5888 and lds(1024) == 20304 and lds(1) % 16 == 0 and lds(1024) % 16 == 0
    assert (160 * 1024) // lds(186) == 27 and (160 * 1024) // lds(1024) == 8
