"""One decode per arm of launch_step's switch (lva_kernels.hip), at the smallest shape that takes it: m = 6 is one tile of 64 conv
states, so a wrong grid, block or template instance shows at once.  The decoder must run the mode that the host-only plan
(kernel_plan: csrc/lva_plan.h) names, and give the lists and scores of kernel mode 1 bit for bit."""
import functools

import numpy as np
import pytest

import nanopore_dna_storage_amd as pkg
from nanopore_dna_storage_amd import synth

pytestmark = pytest.mark.gpu

M, R, MD, SLOTS = 6, 1, 20, 2


@functools.lru_cache(maxsize=None)
def _reads(msg_len):
    reads = [synth.make_read(M, R, msg_len, 5100 + i, rc=bool(i & 1), margin=2.5 + i) for i in range(3)]
    if len({x["post"].shape[0] & 1 for x in reads}) == 1:        # odd and even block counts: the lazy kernels end on either instance
        reads[2]["post"] = reads[2]["post"][:-1].copy()
    return reads


def _decode(msg_len, L, kernel):
    reads = _reads(msg_len)
    with pkg.Decoder(M, R, msg_len, list_size=L, max_deviation=MD, max_slots=SLOTS, kernel=kernel) as dec:
        got = dec.decode([x["post"] for x in reads], rc=[x["rc"] for x in reads])
        return got, dec.profile()["kernel"]


@functools.lru_cache(maxsize=None)
def _exact(msg_len, L):
    """the same configuration on kernel mode 1: computed once per shape, read by every row that shares it"""
    got, mode = _decode(msg_len, L, 1)
    assert mode == 1
    return got


# (request, list size, msg_len) -> the family the plan must name
ROWS = [(1, 8, 60, "exact"), (3, 8, 60, "wave"), (3, 100, 60, "wave_wide"), (0, 1, 60, "acs"), (2, 8, 60, "fast"), (0, 8, 60, "lazy"),
        (0, 16, 60, "big"), (0, 64, 60, "big"), (0, 32, 150, "big_rec"), (0, 64, 150, "big_rec")]


@pytest.mark.parametrize("request_,L,msg_len,family", ROWS)
def test_the_planned_kernel_runs_and_agrees_with_mode_1(request_, L, msg_len, family):
    plan = pkg.kernel_plan(M, R, msg_len, list_size=L, max_deviation=MD, kernel=request_)
    assert plan["dominant"] == family
    got, mode = _decode(msg_len, L, request_)
    assert mode == plan["mode"]
    want = _exact(msg_len, L)
    assert len(got) == len(want) == 3
    for i, (g, w) in enumerate(zip(got, want)):
        assert not isinstance(g, int) and not isinstance(w, int), "read %d: error %r / %r" % (i, g, w)
        assert len(w[0]) > 0, "read %d: empty list" % i
        assert np.array_equal(g[0], w[0]), "read %d: list differs from kernel mode 1" % i
        assert np.array_equal(g[1].view(np.uint32), w[1].view(np.uint32)), "read %d: scores differ from kernel mode 1" % i
