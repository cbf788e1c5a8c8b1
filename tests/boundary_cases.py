"""The shapes of the plane-boundary tests, in one place: test_plane_boundaries_host.py asserts what this list covers,
test_gpu_plane_boundaries.py decodes it.  A candidate's message is a shift register of T = msg_len + mem_conv bits in
ceil(T / 64) 64-bit planes (newest bit = bit 0), and a trellis position moves max(1, ceil(nbits[pos] / 64)) of them; the
totals below end on, just below and just above a plane (64, 128, 192, 256) or a 32-bit output word (96, 160, 224).

At a punctured rate a position may consume two bits, so nbits either lands on a boundary or steps over it; which of the
two is fixed by the rate's block pattern.  Rates 3 and 5 between them step over all of 64, 128 and 192; rate 1 lands on
every one.  A length that does not end on a base boundary is refused by code_info (LVA_ERR_MSG_LEN): such totals are left
out here, at collection time, and only at the punctured rates."""
import nanopore_dna_storage_amd as pkg
from nanopore_dna_storage_amd import synth

M = 6                                  # the smallest trellis: the plane arithmetic does not depend on mem_conv
MEMS = (6, 8, 11, 14)
RATES = (1, 2, 3, 4, 5, 7)             # every rate of the code tables; 1 = rate 1/2, one bit per position
PUNCTURED = RATES[1:]
BOUNDARIES = (64, 128, 192)
PLANE_TOTALS = (63, 64, 65, 127, 128, 129, 191, 192, 193, 255)
WORD_TOTALS = (96, 97, 160, 161, 224, 225)
STEP_OVER_RATES = (3, 5)
FULL = 256                             # the documented maximum of msg_len + mem_conv
MAX_DEV = 5                            # a narrow band keeps the CPU oracle cheap; the plane arithmetic does not depend on it


def accepted(m, r, msg_len):
    try:
        pkg.code_info(m, r, msg_len)
    except pkg.LvaError:
        return False
    return True


def total(code):
    return code[0] + code[2]


def planes(code):
    return -(-total(code) // 64)


# (mem_conv, rate, msg_len)
RATE1 = [(M, 1, T - M) for T in PLANE_TOTALS]
STEP_OVER = [(M, r, T - M) for r in STEP_OVER_RATES for T in PLANE_TOTALS if accepted(M, r, T - M)]
FULL_ALL = [(m, r, FULL - m) for m in MEMS for r in PUNCTURED if accepted(m, r, FULL - m)]     # the host tests: every memory
FULL_GPU = [c for c in FULL_ALL if c[0] == M]
WORDS = [(M, 1, T - M) for T in WORD_TOTALS]
PRODUCTION = [(11, 1, 53), (11, 1, 181)]     # a full first and a full third plane on the 32-tile trellis
HOST_CODES = RATE1 + STEP_OVER + FULL_ALL + WORDS + PRODUCTION

# name -> (kernel requested, list size, the step kernel that must serve it); big32 is lva_step_big_rec at three planes
KERNELS = {
    "acs1": (0, 1, "acs"), "lazy2": (4, 2, "lazy"), "lazy8": (4, 8, "lazy"), "fast4": (2, 4, "fast"), "big12": (2, 12, "big"),
    "big32": (2, 32, "big"), "wave4": (3, 4, "wave"), "exact4": (1, 4, "exact"), "wide65": (3, 65, "wave_wide"),
}
ALL_BUT_WIDE = [k for k in KERNELS if k != "wide65"]
WIDE_TOTALS = (64, 65, 192, 193)


def dominant(kernel, code):
    return "big_rec" if kernel == "big32" and planes(code) == 3 else KERNELS[kernel][2]


# what the GPU test runs: (kernel name, code)
RUNS = [(k, c) for k in ALL_BUT_WIDE for c in RATE1 + STEP_OVER + FULL_GPU]
RUNS += [("wide65", c) for c in RATE1 if total(c) in WIDE_TOTALS]
RUNS += [(k, c) for k in ("lazy8", "exact4") for c in WORDS]          # the output path behind the gather is shared
PRODUCTION_RUNS = [("lazy8", c) for c in PRODUCTION]
# whole-step redo (a 4-entry work list) at a full last plane
OVERFLOW_RUNS = [(k, (M, 1, T - M)) for T in (64, 192) for k in ("lazy8", "big12", "big32")]


def nbits_of(ptypes):
    """bits consumed on arrival at each position, from the block type of the step into it (type 0: one bit, 1..3: two)"""
    out = [0]
    for t in list(ptypes)[1:]:
        out.append(out[-1] + (1 if int(t) == 0 else 2))
    return out


def alignment(nbits, boundary):
    """'hits': a position has consumed exactly `boundary` bits; 'over': a two-bit step went from boundary - 1 to boundary + 1;
    None: the code ends below the boundary"""
    if boundary in nbits:
        return "hits"
    return "over" if nbits[-1] > boundary else None


def reads_for(code, n=3):
    """n = 3: one forward read, one reverse complement, one on a 0.5 grid (exact score ties: the fix-up and exact paths, the heap
    replay); n = 2, where the oracle is slow: the forward read and the tie read as a reverse complement.  The second read loses
    its last block where that is what it takes to have odd and even block counts."""
    m, r, msg_len = code
    seed = 40000 + 1000 * r + 10 * total(code) + m
    reads = [synth.make_read(m, r, msg_len, seed, rc=False, margin=3.0)]
    if n == 3:
        reads.append(synth.make_read(m, r, msg_len, seed + 1, rc=True, margin=4.0))
    reads.append(synth.make_read(m, r, msg_len, seed + 2, rc=n == 2 or bool(total(code) & 1), margin=2.5, quantum=0.5))
    if len({x["post"].shape[0] & 1 for x in reads}) == 1:
        reads[1]["post"] = reads[1]["post"][:-1].copy()
    return reads
