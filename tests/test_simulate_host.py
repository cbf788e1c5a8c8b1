"""The read simulator's definition (nanopore_dna_storage_amd/simulate.py), without a GPU: the generator's known answers, what a
clean channel must give, the channel's rates, the dwell and noise moments, the refusals, the independence of a read from its
batch -- and, from the gfx950 assembly, what the two kernels of csrc/sim_kernels.hip must keep.

The rates are read off the OUTPUT, one probability at a time, so that each count is a plain binomial:
  sub alone  emitted bases that differ from the oligo / source positions;
  del alone  missing bases / source positions;
  ins alone  inserted bases / insertion trials.  The loop draws again after every success, so trials = source positions (n + 1
             per read) + successes, less one per position that reached the cap of 4 (probability p^4 = 6e-6: under one
             position in this sample, against a 4-sigma band of some 330).
With all three at once only their sum shows in the output: there the mean length is held to its expectation."""
import math
import os
import re
import subprocess

import numpy as np
import pytest

from nanopore_dna_storage_amd import _lib, simulate as S
from nanopore_dna_storage_amd.decoder import code_info, encode

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HIPCC = "/opt/rocm/bin/hipcc"
M, R, MSG = 6, 1, 60
P = 0.05
READS = 2000


def test_philox_known_answers():
    assert [int(x) for x in S.philox(0, 0, 0, 0, 0)] == [0x6627E8D5, 0xE169C58D, 0xBC57AC4C, 0x9B00DBD8]
    got = S.philox(0x243F6A88, 0x85A308D3, 0x13198A2E, 0x03707344, 0x299F31D0A4093822)          # key words a4093822 299f31d0
    assert [int(x) for x in got] == [0xD16CFE09, 0x94FDCCEB, 0x5001E420, 0x24126EA1]
    both = S.philox(np.array([0, 0x243F6A88]), 0, 0, 0, 0)                                       # counters broadcast
    assert [int(x) for x in both[0]] == [0x6627E8D5, 0xE169C58D, 0xBC57AC4C, 0x9B00DBD8] and both.shape == (2, 4)


def _dwell_of(ref, seed, first_read, cdf):
    """the extra dwell of every emitted base, restated from the dwell stream alone"""
    out = []
    for r in range(len(ref["msgs"])):
        nb = int(ref["base_offsets"][r + 1] - ref["base_offsets"][r])
        w = S.philox(np.arange((nb + 3) // 4), 0, first_read + r, S.STREAM_DWELL, seed).reshape(-1)[:nb]
        out.append(np.array([next((d for d, c in enumerate(cdf) if x < c), len(cdf)) for x in w], dtype=np.int64))
    return out


@pytest.mark.parametrize("rc_mode", [0, 1, 2])
def test_clean_channel_gives_the_oligo_and_the_dwell_sum(rc_mode):
    n, seed = 7, 11
    ref = S.reference_reads(M, R, MSG, n, seed, first_read=2, rc_mode=rc_mode, scores=False)
    oligos = encode(M, R, MSG, ref["msgs"])
    dwell = _dwell_of(ref, seed, 2, S.poisson_dwell_cdf())
    for r in range(n):
        bases = ref["bases"][ref["base_offsets"][r]:ref["base_offsets"][r + 1]]
        rc = rc_mode == 1 or (rc_mode == 2 and (2 + r) & 1)
        assert np.array_equal(bases, (3 - oligos[r])[::-1] if rc else oligos[r])
        assert ref["row_offsets"][r + 1] - ref["row_offsets"][r] == 1 + int((1 + dwell[r]).sum())
    assert set(np.unique(ref["msgs"])) == {0, 1}


def test_the_path_is_synths_path():
    """states and true transitions as synth.state_path / synth.true_transitions give them for the same bases, lead and dwells"""
    from nanopore_dna_storage_amd import synth
    seed = 5
    ref = S.reference_reads(M, R, MSG, 3, seed, sub=0.1, dele=0.1, ins=0.1, scores=False)
    dwell = _dwell_of(ref, seed, 0, S.poisson_dwell_cdf())
    for r in range(3):
        bases = ref["bases"][ref["base_offsets"][r]:ref["base_offsets"][r + 1]]
        got = ref["true_idx"][ref["row_offsets"][r]:ref["row_offsets"][r + 1]]
        lead = int(got[0]) // 9
        assert got[0] == lead * 9 and lead < 4 and lead != bases[0]
        want, cur = [synth.transition_index(lead, lead)], lead
        for st, d in zip(synth.state_path(bases), dwell[r]):
            want += [synth.transition_index(cur, int(st))] + [synth.transition_index(int(st), int(st))] * int(d)
            cur = int(st)
        assert np.array_equal(got, want)


@pytest.fixture(scope="module")
def oligos_of_sample():
    ref = S.reference_reads(M, R, MSG, READS, 1, scores=False)
    return encode(M, R, MSG, ref["msgs"])


def _within(observed, p, trials):
    bound = 4 * math.sqrt(p * (1 - p) / trials)
    print("observed %.5f, p %.3f, 4 sigma %.5f over %d" % (observed, p, bound, trials))
    return abs(observed - p) <= bound


def test_substitution_rate(oligos_of_sample):
    ref = S.reference_reads(M, R, MSG, READS, 1, sub=P, scores=False)
    got = ref["bases"].reshape(READS, -1)
    assert got.shape == oligos_of_sample.shape
    assert _within((got != oligos_of_sample).mean(), P, got.size)


def test_deletion_rate(oligos_of_sample):
    ref = S.reference_reads(M, R, MSG, READS, 1, dele=P, scores=False)
    N = oligos_of_sample.size
    assert _within((N - len(ref["bases"])) / N, P, N)


def test_insertion_rate(oligos_of_sample):
    ref = S.reference_reads(M, R, MSG, READS, 1, ins=P, scores=False)
    inserted = len(ref["bases"]) - oligos_of_sample.size
    trials = READS * (oligos_of_sample.shape[1] + 1) + inserted
    assert _within(inserted / trials, P, trials)


def test_all_three_at_once_and_the_dwell_mean(oligos_of_sample):
    """length: per source position -del + sum_k p^k insertions, and the latter once more behind the last"""
    ref = S.reference_reads(M, R, MSG, READS, 1, sub=P, dele=P, ins=P, scores=False)
    n = oligos_of_sample.shape[1]
    m1 = sum(P ** k for k in range(1, 5))                                   # insertions per position: mean ...
    m2 = sum((2 * k - 1) * P ** k for k in range(1, 5))                     # ... and second moment (P(count >= k) = p^k)
    mean = READS * (n * (1 - P) + (n + 1) * m1)
    var = READS * (n * P * (1 - P) + (n + 1) * (m2 - m1 * m1))
    print("bases %d, expected %.1f, 4 sigma %.1f" % (len(ref["bases"]), mean, 4 * math.sqrt(var)))
    assert abs(len(ref["bases"]) - mean) <= 4 * math.sqrt(var)
    lengths = np.diff(ref["base_offsets"])
    assert lengths.min() < n < lengths.max()
    # dwell: (blocks - 1 - bases) / bases against the table's mean
    cdf = S.poisson_dwell_cdf()
    c = np.concatenate([[0.0], cdf / 4294967296.0, [1.0]])
    p = np.diff(c)
    mu = float((p * np.arange(len(p))).sum())
    sd = math.sqrt(float((p * np.arange(len(p)) ** 2).sum()) - mu * mu)
    nb = len(ref["bases"])
    got = (int(ref["row_offsets"][-1]) - READS - nb) / nb
    print("dwell mean %.4f, table %.4f (Poisson 3.4), 4 standard errors %.4f" % (got, mu, 4 * sd / math.sqrt(nb)))
    assert abs(mu - S.dwell_mean(cdf)) < 1e-12 and abs(mu - 3.4) < 1e-6
    assert abs(got - mu) <= 4 * sd / math.sqrt(nb)


def test_noise_standard_deviation():
    sigma, blocks = 1.5, 25000                                              # 10^6 entries
    v = S.read_scores(3, 99, np.zeros(blocks, np.uint8), S.score_scale(sigma), 0.0, 100.0)
    sd = float(v.astype(np.float64).std())
    print("standard deviation %.4f over %d entries, mean %.5f" % (sd, v.size, float(v.mean())))
    assert v.shape == (blocks, 40) and abs(sd - sigma) <= 0.01 * sigma
    assert float(np.abs(v).max()) <= 2 * math.sqrt(3.0) * sigma < S.SCORE_CLIP + 0.2     # support +-3.46 sigma


def test_scores_are_three_float32_operations():
    """margin on the true transition only, then the clip; a fused multiply-add of scale and margin would differ in some entry"""
    true_idx = (np.arange(4000) % 40).astype(np.uint8)
    scale, margin, clip = S.score_scale(1.5), np.float32(2.7), np.float32(3.1)
    v = S.read_scores(0, 1, true_idx, scale, margin, clip)
    raw = S.read_scores(0, 1, true_idx, scale, 0.0, 1e9)
    want = raw.copy()
    t = np.arange(4000)
    want[t, true_idx] = raw[t, true_idx] + margin                            # float32 + float32
    assert np.array_equal(v, np.clip(want, -clip, clip)) and (np.abs(want) > clip).any()
    s = np.rint(raw[t, true_idx].astype(np.float64) / float(scale))          # the integer the entry was drawn as
    fused = (s * float(scale) + float(margin)).astype(np.float32)            # one rounding instead of two
    assert (fused != want[t, true_idx]).any()


def test_insertion_cap_and_refusals():
    q = S.parameters(ins=S.MAX_PROB)
    assert q["ins"] == 1 << 30
    q["ins"] = 1 << 32                                                      # every trial succeeds: the loop must stop at 4
    oligo = encode(M, R, MSG, np.zeros(MSG, np.uint8))
    bases, true_idx = S._read(0, 1, oligo, q)
    assert len(bases) == len(oligo) + S.MAX_INS * (len(oligo) + 1)
    assert np.array_equal(bases[S.MAX_INS::S.MAX_INS + 1], oligo)
    for kw in (dict(ins=0.2500001), dict(sub=0.3), dict(dele=0.26), dict(sub=-0.1), dict(dwell_cdf=np.zeros(65, np.uint32)),
               dict(dwell_cdf=np.zeros(0, np.uint32)), dict(start_barcode="ACGT"), dict(rc_mode=3), dict(clip=0.0),
               dict(start_barcode="ACGT", end_barcode="ACGT", flank=(5, 4)), dict(start_barcode="ACGT", end_barcode="ACGT", flank=(0, 257))):
        with pytest.raises(ValueError):
            S.reference_reads(M, R, MSG, 1, 0, scores=False, **kw)
    with pytest.raises(ValueError):
        S.reference_reads(M, R, MSG, 2, 0, first_read=(1 << 32) - 1, scores=False)
    L = _lib.load_library()                                                 # no decoder: refused before anything else
    cdf, off = S.poisson_dwell_cdf(), np.full(2, 77, np.int64)
    assert L.lva_simulate_plan(None, 1, 0, 1, 0, 0, 0, cdf.ctypes.data, len(cdf), None, None, 0, 0, 0, off.ctypes.data, off.ctypes.data) == -10
    assert L.lva_simulate_fill_device(None, 1, 0, 1, 0, 0, 0, cdf.ctypes.data, len(cdf), None, None, 0, 0, 0, 1.0, 0.0, 5.0,
                                      off.ctypes.data, off.ctypes.data, None, None, None, None) == -10
    assert list(off) == [77, 77]


KEYS = ("msgs", "bases", "true_idx", "scores")


def test_a_read_depends_on_seed_and_number_alone():
    kw = dict(sub=0.1, dele=0.1, ins=0.1, start_barcode="CACCTGTGCTGCGTCAGGCTGTGTC", end_barcode="GCTGTCCGTTCCGCATTGACACGGC", rc_mode=2)
    big = S.reference_reads(M, R, MSG, 20, 42, **kw)
    part = S.reference_reads(M, R, MSG, 10, 42, first_read=5, **kw)
    for key, off in (("bases", "base_offsets"), ("true_idx", "row_offsets"), ("scores", "row_offsets")):
        assert np.array_equal(part[key].view(np.uint32 if key == "scores" else np.uint8),
                              big[key][big[off][5]:big[off][15]].view(np.uint32 if key == "scores" else np.uint8)), key
        assert np.array_equal(part[off], big[off][5:16] - big[off][5])
    assert np.array_equal(part["msgs"], big["msgs"][5:15])
    other = S.reference_reads(M, R, MSG, 10, 43, first_read=5, **kw)
    assert not np.array_equal(other["msgs"], part["msgs"])


def test_barcoded_strand_layout():
    sb, eb = "CACCTGTGCTGCGTCAGGCTGTGTC", "GCTGTCCGTTCCGCATTGACACGGC"
    ref = S.reference_reads(M, R, MSG, 40, 8, start_barcode=sb, end_barcode=eb, flank=(3, 9), scores=False)
    oligos = encode(M, R, MSG, ref["msgs"])
    core = [S.bases_from_str(sb), None, S.bases_from_str(eb)]
    flanks = set()
    for r in range(40):
        strand = ref["bases"][ref["base_offsets"][r]:ref["base_offsets"][r + 1]]
        core[1] = oligos[r]
        body = np.concatenate(core)
        hits = [k for k in range(3, 10) if np.array_equal(strand[k:k + len(body)], body) and 3 <= len(strand) - k - len(body) <= 9]
        assert hits, r
        flanks.add((hits[0], len(strand) - hits[0] - len(body)))
    assert len(flanks) > 10 and len({a for a, _ in flanks}) == 7            # every length of the range occurs


# ---- the kernels' assembly (hipcc cross-compiles without a GPU) ----------------------------------------------------------

@pytest.fixture(scope="module")
def asm(tmp_path_factory):
    if not os.path.exists(HIPCC):
        pytest.skip("no hipcc")
    out = str(tmp_path_factory.mktemp("asm") / "sim_k.s")
    src = os.path.join(ROOT, "nanopore_dna_storage_amd", "csrc", "sim_kernels.hip")
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
    m = re.search(r"^(_ZN3lva\S*%s\S*):" % pat, asm, re.M)
    assert m, pat
    return asm[m.start():asm.index(".Lfunc_end", m.start())]


def test_two_kernels_without_scratch(asm):
    meta = _meta(asm)
    assert len(meta) == 2, list(meta)
    for pat in ("sim_strand", "sim_scores"):
        got = [v for k, v in meta.items() if pat in k]
        assert len(got) == 1, pat
        print(pat, got[0])
        assert got[0]["scratch"] == 0 and got[0]["vgpr"] <= 128, (pat, got[0])
    assert [v for k, v in meta.items() if "sim_scores" in k][0]["lds"] == 0


def test_scores_kernel_stores_whole_quads_and_fuses_nothing(asm):
    body = _body(asm, "sim_scores")
    stores = re.findall(r"^\s*((?:global|flat|buffer)_store_\w+)", body, re.M)
    print("stores of sim_scores:", stores)
    assert stores and all(s == "global_store_dwordx4" for s in stores), stores
    assert not re.search(r"^\s*global_atomic|^\s*flat_atomic", asm, re.M)
    assert not re.search(r"^\s*v_(pk_)?(fma|fmac|mad|mac)_f", body, re.M), "scale and margin must stay two float32 operations"
    assert re.search(r"^\s*v_mul_f32", body, re.M) and re.search(r"^\s*v_add_f32", body, re.M)
