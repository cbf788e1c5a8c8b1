"""What the gfx950 assembly of the wide wavefront-per-target kernel must keep (no GPU needed: hipcc cross-compiles).
lva_step_wave_wide<R>, R = 2, 3, 4 register rows (list sizes 65..256): 16 R candidate registers + 3 R for the accepted entries on
top of the narrow kernel's ~50 -- within 128 registers at R = 4 (four wavefronts per SIMD; the launch bounds hold every instance
there), nothing in scratch memory, and the 8 R candidate requests of a flip target issued back to back.  The narrow kernels keep
their names: one symbol each."""
import os
import re
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HIPCC = "/opt/rocm/bin/hipcc"
VGPR_BOUND = {2: 128, 3: 128, 4: 128}


@pytest.fixture(scope="module")
def asm(tmp_path_factory):
    if not os.path.exists(HIPCC):
        pytest.skip("no hipcc")
    out = str(tmp_path_factory.mktemp("asm") / "lva_k.s")
    src = os.path.join(ROOT, "nanopore_dna_storage_amd", "csrc", "lva_kernels.hip")
    subprocess.run([HIPCC, "--offload-arch=gfx950", "-O3", "-std=c++17", "-ffp-contract=off", "-fno-fast-math", "--cuda-device-only",
                    "-S", "-o", out, src], check=True, cwd=os.path.dirname(src))
    return open(out).read()


def _meta(asm):
    res = {}
    for b in asm.split("- .agpr_count:")[1:]:
        g = lambda k: re.search(r"\.%s:\s+(\S+)" % k, b).group(1)
        res[g("name")] = dict(vgpr=int(g("vgpr_count")), lds=int(g("group_segment_fixed_size")), scratch=int(g("private_segment_fixed_size")))
    return res


def test_three_wide_instances_within_budget(asm):
    meta = _meta(asm)
    wide = {k: v for k, v in meta.items() if "lva_step_wave_wide" in k}
    assert len(wide) == 3, list(wide)
    for R in (2, 3, 4):
        got = {k: v for k, v in wide.items() if re.search(r"lva_step_wave_wideILi%dE" % R, k)}
        assert len(got) == 1, (R, list(got))
        for k, v in got.items():
            print(k, v)
            assert v["vgpr"] <= VGPR_BOUND[R] and v["scratch"] == 0 and v["lds"] == 0, (k, v)


def test_narrow_kernels_keep_their_names(asm):
    meta = _meta(asm)
    for pat in (r"lva_step_waveE", r"lva_step_fixup_waveE"):
        assert len([k for k in meta if re.search(pat, k)]) == 1, pat


@pytest.mark.parametrize("R", [2, 3, 4])
def test_candidate_rows_are_requested_at_once(asm, R):
    """8 R eight-byte requests in a row without a wait on the memory queue between them"""
    m = re.search(r"^(_ZN3lva18lva_step_wave_wideILi%dE\S*):" % R, asm, re.M)
    body = asm[m.start():asm.index(".Lfunc_end", m.start())]
    run = best = 0
    for ln in body.split("\n"):
        ln = ln.strip()
        if ln.startswith("global_load_dwordx2"):
            run += 1
        elif ln.startswith("s_waitcnt") and "vmcnt" in ln:
            run = 0
        best = max(best, run)
    assert best >= 8 * R, best
