"""What the gfx950 assembly of the transition-posterior kernels must keep (no GPU needed: hipcc cross-compiles).
tp_forward / tp_backward (csrc/tp_kernels.hip): nothing in scratch memory, at most 128 registers (four wavefronts per SIMD stay
possible), and in the forward loop the row requests of a prefetch chunk -- two 16-byte requests per block, four blocks -- go out
without a full wait on the memory queue between them."""
import os
import re
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HIPCC = "/opt/rocm/bin/hipcc"
CHUNK_REQUESTS = 8          # kTpChunk = 4 blocks x 2 dwordx4


@pytest.fixture(scope="module")
def asm(tmp_path_factory):
    if not os.path.exists(HIPCC):
        pytest.skip("no hipcc")
    out = str(tmp_path_factory.mktemp("asm") / "tp_k.s")
    src = os.path.join(ROOT, "nanopore_dna_storage_amd", "csrc", "tp_kernels.hip")
    subprocess.run([HIPCC, "--offload-arch=gfx950", "-O3", "-std=c++17", "-ffp-contract=off", "-fno-fast-math", "--cuda-device-only",
                    "-S", "-o", out, src], check=True, cwd=os.path.dirname(src))
    return open(out).read()


def _meta(asm):
    res = {}
    for b in asm.split("- .agpr_count:")[1:]:
        g = lambda k: re.search(r"\.%s:\s+(\S+)" % k, b).group(1)
        res[g("name")] = dict(vgpr=int(g("vgpr_count")), sgpr=int(g("sgpr_count")), lds=int(g("group_segment_fixed_size")),
                              scratch=int(g("private_segment_fixed_size")))
    return res


def _body(asm, pat):
    m = re.search(r"^(_ZN3lva\d+%s\S*):" % pat, asm, re.M)
    assert m, pat
    return asm[m.start():asm.index(".Lfunc_end", m.start())]


def test_two_kernels_within_budget(asm):
    meta = _meta(asm)
    assert len(meta) == 2, list(meta)
    for pat in ("tp_forward", "tp_backward"):
        got = [v for k, v in meta.items() if pat in k]
        assert len(got) == 1, pat
        print(pat, got[0])
        assert got[0]["scratch"] == 0 and got[0]["lds"] == 0 and got[0]["vgpr"] <= 128, (pat, got[0])


def test_forward_chunk_is_requested_at_once(asm):
    """in the forward loop the 16-byte row requests come in runs of a whole chunk: no wait on the memory queue and no branch
    inside a run, and nowhere in the loop a wait that drains the queue (vmcnt(0)) -- the other chunk's rows stay in flight"""
    body = _body(asm, "tp_forward")
    lines = [ln.split(";")[0].strip() for ln in body.split("\n")]
    labels = {ln[:-1]: i for i, ln in enumerate(lines) if re.match(r"^\.LBB\d+_\d+:$", ln)}
    loops = []
    for i, ln in enumerate(lines):
        m = re.match(r"^s_c?branch\w*\s+(\.LBB\d+_\d+)$", ln)
        if m and m.group(1) in labels and labels[m.group(1)] < i:
            loops.append((labels[m.group(1)], i))
    assert loops, "no loop found"
    lo, hi = min(p[0] for p in loops), max(p[1] for p in loops)
    loop = lines[lo:hi]
    runs, run = [], 0
    for ln in loop:
        if ln.startswith("global_load_dwordx4"):
            run += 1
        elif (ln.startswith("s_waitcnt") and "vmcnt" in ln) or ln.startswith("s_cbranch") or ln.startswith("s_branch"):
            if run:
                runs.append(run)
            run = 0
    if run:
        runs.append(run)
    print("runs of row requests in the forward loop:", runs)
    assert runs and all(r == CHUNK_REQUESTS for r in runs), runs
    assert not [ln for ln in loop if ln.startswith("s_waitcnt") and re.search(r"vmcnt\(0\)", ln)], "the loop drains the memory queue"


def test_no_scalar_memory_writes(asm):
    for pat in ("tp_forward", "tp_backward"):
        body = _body(asm, pat)
        assert not re.search(r"^\s*s_(buffer_|scratch_)?(store|atomic)", body, re.M)
