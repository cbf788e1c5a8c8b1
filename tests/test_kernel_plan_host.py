"""The kernel plan (csrc/lva_plan.h plan_kernels, seen through lva_kernel_plan) against the table of DESIGN.md section 4, written
out below as data: every request 0..4 at list sizes on both sides of every class boundary, at one to four message planes.  No
device is opened: lva_kernel_plan is host code, and lva_decoder_create decides the same before it looks for a device."""
import pytest

import nanopore_dna_storage_amd as pkg

ARG, NO_DEVICE, UNSUPPORTED = -10, -11, -12


def _fam(mode, dominant, fixup, flags, ring_extra, instance=0):
    return dict(mode=mode, dominant=dominant, fixup=fixup, lazy=flags[0], rec=flags[1], cmp=flags[2], ring_extra=ring_extra, instance=instance)


EXACT = _fam(1, "exact", "none", (0, 0, 0), 1)
WAVE = _fam(3, "wave", "none", (0, 0, 0), 1)
WIDE = {r: _fam(3, "wave_wide", "none", (0, 0, 0), 1, r) for r in (2, 3, 4)}
LAZY = _fam(4, "lazy", "lazy", (1, 0, 1), 2)
ACS = _fam(2, "acs", "none", (0, 0, 1), 1)
FAST = _fam(2, "fast", "wave", (0, 0, 0), 1)
BIG = {ll: _fam(2, "big", "wave", (0, 0, 1), 1, ll) for ll in (16, 32, 64)}
REC = {ll: _fam(2, "big_rec", "wave", (0, 1, 0), 1, ll) for ll in (32, 64)}
NO = UNSUPPORTED


def _p3(rec, otherwise):
    """the record layout at three message planes, the plane layout at one, two and four"""
    return {1: otherwise, 2: otherwise, 3: rec, 4: otherwise}


# list size -> what the requests 0, 1, 2, 3, 4 resolve to
TABLE = {
    1:     (ACS, EXACT, ACS, NO, NO),
    2:     (LAZY, EXACT, FAST, WAVE, LAZY),
    3:     (BIG[16], EXACT, BIG[16], WAVE, NO),
    4:     (LAZY, EXACT, FAST, WAVE, LAZY),
    8:     (LAZY, EXACT, FAST, WAVE, LAZY),
    12:    (BIG[16], EXACT, BIG[16], WAVE, NO),
    16:    (BIG[16], EXACT, BIG[16], WAVE, NO),
    17:    (BIG[32], EXACT, BIG[32], WAVE, NO),
    31:    (BIG[32], EXACT, BIG[32], WAVE, NO),
    32:    (_p3(REC[32], BIG[32]), EXACT, _p3(REC[32], BIG[32]), WAVE, NO),
    33:    (BIG[64], EXACT, BIG[64], WAVE, NO),
    36:    (_p3(REC[64], BIG[64]), EXACT, _p3(REC[64], BIG[64]), WAVE, NO),
    64:    (_p3(REC[64], BIG[64]), EXACT, _p3(REC[64], BIG[64]), WAVE, NO),
    65:    (EXACT, EXACT, NO, WIDE[2], NO),
    128:   (EXACT, EXACT, NO, WIDE[2], NO),
    256:   (EXACT, EXACT, NO, WIDE[4], NO),
    257:   (EXACT, EXACT, NO, NO, NO),
    65535: (EXACT, EXACT, NO, NO, NO),
}

# (mem_conv, rate, msg_len, message planes): one to four planes at m = 6, then the two large trellises
CODES = [(6, 1, 40, 1), (6, 1, 100, 2), (6, 1, 150, 3), (6, 1, 230, 4), (11, 5, 180, 3), (14, 1, 100, 2)]
MD = 5          # ring = 2 * MD + ring_extra positions, below nstate_pos of every code above


@pytest.mark.parametrize("m,r,msg_len,planes", CODES)
def test_every_request_at_every_list_size_class(m, r, msg_len, planes):
    assert planes == -(-(msg_len + m) // 64)
    npos = pkg.code_info(m, r, msg_len).nstate_pos
    assert 2 * MD + 2 < npos
    for L, row in TABLE.items():
        for request, want in enumerate(row):
            if isinstance(want, dict) and "mode" not in want:
                want = want[planes]
            if want == UNSUPPORTED:
                with pytest.raises(pkg.LvaError) as e:
                    pkg.kernel_plan(m, r, msg_len, list_size=L, max_deviation=MD, kernel=request)
                assert e.value.code == UNSUPPORTED, (request, L)
                continue
            want = dict(want)
            want["ring_positions"] = 2 * MD + want.pop("ring_extra")
            assert pkg.kernel_plan(m, r, msg_len, list_size=L, max_deviation=MD, kernel=request) == want, (request, L)


def test_the_ring_is_never_longer_than_the_trellis():
    npos = pkg.code_info(6, 1, 40).nstate_pos
    for L in (1, 8, 100):                      # unbanded: max_deviation = msg_len + mem_conv + 1
        assert pkg.kernel_plan(6, 1, 40, list_size=L)["ring_positions"] == npos
    assert pkg.kernel_plan(6, 1, 40, list_size=8, max_deviation=0)["ring_positions"] == 2       # lazy: two below an empty band
    assert pkg.kernel_plan(6, 1, 40, list_size=8, max_deviation=0, kernel=1)["ring_positions"] == 1


@pytest.mark.parametrize("what,kw", [("kernel", dict(kernel=-1)), ("kernel", dict(kernel=5)),
                                     ("list_size", dict(list_size=0)), ("list_size", dict(list_size=65536))])
def test_values_outside_the_domain_are_argument_errors(what, kw):
    for call in (pkg.kernel_plan, pkg.Decoder):
        with pytest.raises(pkg.LvaError) as e:
            call(6, 1, 60, **kw)
        assert e.value.code == ARG, what


# (request, list size, msg_len): the three refusals, on both sides where there are two
REFUSED = [(2, 65, 60), (3, 1, 60), (3, 257, 60), (4, 1, 60), (4, 3, 60), (4, 16, 60)]
# one accepted plan of each family
ACCEPTED = [(1, 8, 60, "exact"), (3, 8, 60, "wave"), (3, 100, 60, "wave_wide"), (0, 1, 60, "acs"), (2, 8, 60, "fast"),
            (0, 8, 60, "lazy"), (0, 16, 60, "big"), (0, 32, 150, "big_rec")]


@pytest.mark.parametrize("request_,L,msg_len", REFUSED)
def test_create_refuses_before_it_looks_for_a_device(request_, L, msg_len):
    """LVA_ERR_UNSUPPORTED with or without a GPU: the plan is made first"""
    with pytest.raises(pkg.LvaError) as e:
        pkg.Decoder(6, 1, msg_len, list_size=L, max_deviation=20, kernel=request_)
    assert e.value.code == UNSUPPORTED


@pytest.mark.parametrize("request_,L,msg_len,family", ACCEPTED)
def test_create_of_an_accepted_plan_then_asks_for_the_device(request_, L, msg_len, family):
    assert pkg.kernel_plan(6, 1, msg_len, list_size=L, max_deviation=20, kernel=request_)["dominant"] == family
    import torch
    if torch.cuda.is_available():
        pytest.skip("a GPU is present")
    with pytest.raises(pkg.LvaError) as e:
        pkg.Decoder(6, 1, msg_len, list_size=L, max_deviation=20, kernel=request_)
    assert e.value.code == NO_DEVICE
