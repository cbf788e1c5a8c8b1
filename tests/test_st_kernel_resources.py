"""What the gfx950 code object of the traceback kernels must keep (no GPU needed: hipcc cross-compiles), after
tests/test_sc_kernel_resources.py.  csrc/st_kernels.hip holds st_fill and st_walk; nothing is in scratch memory; st_fill, which
is the frame sc_score runs (csrc/sc_frame.h) with a byte store per cell, stays within 64 vector registers (eight wavefronts
per SIMD hide its chain of dependent LDS round trips) and st_walk too; all LDS is dynamic -- st_fill's is sc_score's formula,
st_walk's a run of kStRun rows of kStRun bytes and their band words -- and the arithmetic is add and compare/select, no FMA.
The shared frame is a function, not a kernel: csrc/sc_kernels.hip still compiles to sc_score alone."""
import os
import re
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HIPCC = "/opt/rocm/bin/hipcc"
CSRC = os.path.join(ROOT, "nanopore_dna_storage_amd", "csrc")


def compiled(tmp, name):
    out = str(tmp / (name + ".s"))
    subprocess.run([HIPCC, "--offload-arch=gfx950", "-O3", "-std=c++17", "-ffp-contract=off", "-fno-fast-math", "--cuda-device-only",
                    "-S", "-o", out, os.path.join(CSRC, name + ".hip")], check=True, cwd=CSRC)
    text = open(out).read()
    res = {}
    for b in text.split("- .agpr_count:")[1:]:
        g = lambda k: re.search(r"\.%s:\s+(\S+)" % k, b).group(1)
        res[g("name")] = dict(vgpr=int(g("vgpr_count")), agpr=int(b.split()[0]), sgpr=int(g("sgpr_count")),
                              lds=int(g("group_segment_fixed_size")), scratch=int(g("private_segment_fixed_size")))
    return res, text


@pytest.fixture(scope="module")
def meta(tmp_path_factory):
    if not os.path.exists(HIPCC):
        pytest.skip("no hipcc")
    return compiled(tmp_path_factory.mktemp("asm"), "st_kernels")


def kernel(res, name):
    hit = [v for k, v in res.items() if name in k]
    assert len(hit) == 1, (name, list(res))
    return hit[0]


def test_two_kernels_without_scratch_within_the_register_classes(meta):
    res, _ = meta
    assert len(res) == 2, list(res)
    for name in ("st_fill", "st_walk"):
        got = kernel(res, name)
        print(name, got)
        assert got["scratch"] == 0
        assert got["vgpr"] + got["agpr"] <= 64, got
        assert got["sgpr"] <= 102, got
        assert got["lds"] == 0, got                  # every byte is dynamic


def test_arithmetic_is_add_and_compare_select(meta):
    _, text = meta
    assert "v_add_f32" in text and "v_cmp_lt_f32" in text and not re.search(r"\bv_(fma|fmac|mad|mac)_f(16|32|64)", text)
    assert "global_store_byte" in text               # the back-pointers: one byte per cell


def test_lds_of_a_launch():
    with open(os.path.join(CSRC, "st_kernels.h")) as f:
        h = f.read()
    with open(os.path.join(CSRC, "st_kernels.hip")) as f:
        k = f.read()
    run = int(re.search(r"kStRun = (\d+);", h).group(1))
    assert "(size_t)kStRun * kStRun + (size_t)kStRun * 4" in h
    assert run == 64 and run * run + run * 4 == 4352                     # 37 workgroups of st_walk per CU by LDS
    # st_fill is launched with sc_score's LDS, st_walk with its own formula
    assert re.search(r"hipLaunchKernelGGL\(st_fill, dim3\(n_pairs\), dim3\(64\), sc_lds_bytes\(max_len\)", k)
    assert re.search(r"hipLaunchKernelGGL\(st_walk, dim3\(n_pairs\), dim3\(kStRun\), st_walk_lds_bytes\(\)", k)
    assert "__shared__" not in re.sub(r"extern __shared__", "", k)       # no static LDS


def test_sc_kernels_still_holds_sc_score_alone(tmp_path_factory):
    if not os.path.exists(HIPCC):
        pytest.skip("no hipcc")
    res, _ = compiled(tmp_path_factory.mktemp("asm_sc"), "sc_kernels")
    assert len(res) == 1 and "sc_score" in list(res)[0], list(res)
