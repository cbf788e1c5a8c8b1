"""The list consumers (csrc/ls_kernels.hip, lva_list_filter / lva_list_consensus / lva_list_stats) without a GPU: the
library, header and binding carry the entry points, every argument check answers before a device is looked for, the
string <-> array converters round-trip, the drivers take their new options, and the kernels keep out of scratch memory."""
import os
import re
import subprocess

import numpy as np
import pytest

from nanopore_dna_storage_amd import (_lib, compute_error_rate_from_decoded_lists, decode_RS_from_decoded_lists, helper, list_ops,
                                      simulator)
import nanopore_dna_storage_amd as pkg

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HIPCC = "/opt/rocm/bin/hipcc"
API = ["lva_list_filter", "lva_list_consensus", "lva_list_stats"]
OK, ERR_ARG = 0, -10


def test_header_library_and_binding_carry_the_entry_points():
    with open(os.path.join(ROOT, "include", "lva_decoder.h")) as f:
        header = f.read()
    lib = _lib.load_library()
    for name in API:
        assert re.search(r"\bint %s\(" % name, header), name
        assert hasattr(lib, name) and getattr(lib, name).argtypes, name
        assert name in _lib.EXPORTS
    assert "#define LVA_ABI_VERSION 5" in header and lib.lva_abi_version() == 5
    assert [f[0] for f in _lib.ListStat._fields_] == list(list_ops.STAT_FIELDS) and list_ops.STAT_DTYPE.itemsize == 24
    assert callable(pkg.Decoder.decode_payloads)
    with open(os.path.join(ROOT, "nanopore_dna_storage_amd", "csrc", "Makefile")) as f:
        mk = f.read()
    assert re.search(r"^SRC\s*=.*\bls_kernels\.hip\b", mk, re.M) and re.search(r"^HDR\s*=.*\bls_kernels\.h\b", mk, re.M)


class _Args:
    """valid arguments of the three calls for 2 reads, lists of 3, 18 bytes per oligo; `over` replaces some"""

    def __init__(self, bpo=18, pad=0, n=2, L=3):
        self.msg_len = 20 + 8 * bpo + pad
        self.keep = dict(msgs=np.zeros((max(n, 1), L, self.msg_len), np.uint8), counts=np.zeros(max(n, 1), np.int32),
                         truth=np.zeros((max(n, 1), self.msg_len), np.uint8), index=np.zeros(max(n, 1), np.int32),
                         payload=np.zeros((max(n, 1), bpo), np.uint8), o1=np.zeros(4096 * 64, np.uint8), o2=np.zeros(4096 * 64, np.uint8),
                         o3=np.zeros(4096 * 64, np.uint8))
        p = {k: v.ctypes.data for k, v in self.keep.items()}
        self.filter = dict(device=0, msgs=p["msgs"], counts=p["counts"], n_reads=n, list_size=L, msg_len=self.msg_len, use_entries=0,
                           bytes_per_oligo=bpo, num_oligos=72, pad=pad, out_index=p["o1"], out_rank=p["o2"], out_payload=p["o3"])
        self.consensus = dict(device=0, index=p["index"], payload=p["payload"], n_reads=n, bytes_per_oligo=bpo, num_oligos=72,
                              first_only=0, out_present=p["o1"], out_payload=p["o2"], out_votes=p["o3"])
        self.stats = dict(device=0, msgs=p["msgs"], counts=p["counts"], truth=p["truth"], n_reads=n, list_size=L, msg_len=self.msg_len,
                          out=p["o1"])

    def call(self, which, **over):
        a = dict(getattr(self, which))
        assert set(over) <= set(a), over
        a.update(over)
        return getattr(_lib.load_library(), "lva_list_" + which)(*a.values())


POINTERS = {"filter": ["msgs", "counts", "out_index", "out_rank", "out_payload"],
            "consensus": ["index", "payload", "out_present", "out_payload", "out_votes"],
            "stats": ["msgs", "counts", "truth", "out"]}


@pytest.mark.parametrize("which", ["filter", "consensus", "stats"])
def test_null_pointers_and_negative_batches_are_refused(which):
    a = _Args()
    for name in POINTERS[which]:
        assert a.call(which, **{name: None}) == ERR_ARG, name
    assert a.call(which, n_reads=-1) == ERR_ARG


@pytest.mark.parametrize("which", ["filter", "stats"])
def test_list_shape_is_checked(which):
    a = _Args()
    assert a.call(which, list_size=0) == ERR_ARG
    assert a.call(which, list_size=-3) == ERR_ARG
    for msg_len in (0, 256, 1000):
        assert a.call(which, msg_len=msg_len) == ERR_ARG, msg_len
    if which == "stats":      # n_reads * list_size * msg_len = 2^31 exactly (checked before anything is read)
        assert a.call(which, n_reads=2 ** 17, list_size=2 ** 7, msg_len=128) == ERR_ARG
    else:                     # the first n_reads with n_reads * 164 >= 2^31, in the shape the filter accepts
        assert 13094413 * a.msg_len >= 2 ** 31 > 13094412 * a.msg_len
        assert a.call(which, n_reads=13094413, list_size=1) == ERR_ARG
    assert a.call(which, n_reads=2 ** 31 - 1, list_size=2 ** 31 - 1) == ERR_ARG


def test_filter_arguments_are_checked():
    a = _Args()
    assert a.call("filter", use_entries=4) == ERR_ARG          # > list_size
    assert a.call("filter", use_entries=-1) == ERR_ARG
    for bad in (a.msg_len - 1, a.msg_len + 1, a.msg_len + 8):    # not 12 + 8 + 8 * bytes_per_oligo (+ 1 with pad)
        assert a.call("filter", msg_len=bad) == ERR_ARG, bad
    assert a.call("filter", pad=1) == ERR_ARG                   # same length, now one bit short
    assert a.call("filter", bytes_per_oligo=17) == ERR_ARG and a.call("filter", bytes_per_oligo=0, msg_len=20) == ERR_ARG
    for num_oligos in (0, -1, 4097):
        assert a.call("filter", num_oligos=num_oligos) == ERR_ARG, num_oligos
    assert _Args(pad=1).call("filter", pad=0) == ERR_ARG


def test_consensus_arguments_are_checked():
    a = _Args()
    for num_oligos in (0, -1, 4097):
        assert a.call("consensus", num_oligos=num_oligos) == ERR_ARG, num_oligos
    assert a.call("consensus", bytes_per_oligo=0) == ERR_ARG
    a.keep["index"][:] = [3, 72]
    assert a.call("consensus") == ERR_ARG                       # an index >= num_oligos
    a.keep["index"][:] = [3, 4095]
    assert a.call("consensus") == ERR_ARG


@pytest.mark.parametrize("which", ["filter", "consensus", "stats"])
def test_an_empty_batch_succeeds_and_touches_nothing(which):
    a = _Args(n=0)
    for k in ("o1", "o2", "o3"):
        a.keep[k][:] = 0xAB
    assert a.call(which) == OK
    assert all((a.keep[k] == 0xAB).all() for k in ("o1", "o2", "o3"))
    if which == "filter":
        assert a.call(which, msg_len=a.msg_len + 1) == ERR_ARG  # still checked


def test_python_wrappers_on_empty_batches():
    index, rank, payload = list_ops.filter_lists(np.zeros((0, 8, 164), np.uint8), np.zeros(0, np.int32), 18, 72)
    assert index.shape == (0,) and rank.shape == (0,) and payload.shape == (0, 18)
    assert list_ops.consensus(index, payload, 72) == []
    assert list_ops.list_stats(np.zeros((0, 8, 164), np.uint8), np.zeros(0, np.int32), np.zeros((0, 164), np.uint8)).shape == (0,)
    with pytest.raises(_lib.LvaError):
        list_ops.filter_lists(np.zeros((1, 8, 165), np.uint8), np.zeros(1, np.int32), 18, 72)


def test_string_array_converters_round_trip():
    rng = np.random.default_rng(4)
    lists = []
    for n in (0, 1, 5, 3, 0, 8):
        lists.append(["".join(rng.choice(["0", "1"], size=37)) for _ in range(n)])
    msgs, counts = list_ops.lists_to_array(lists)
    assert msgs.shape == (6, 8, 37) and msgs.dtype == np.uint8 and counts.tolist() == [0, 1, 5, 3, 0, 8] and counts.dtype == np.int32
    assert msgs.max() == 1 and not msgs[2, 5:].any()
    assert "".join(map(str, msgs[3, 2])) == lists[3][2]
    assert list_ops.array_to_lists(msgs, counts) == lists
    # a cut: the first list_size entries stay, like lst[:list_size]
    m4, c4 = list_ops.lists_to_array(lists, list_size=4)
    assert m4.shape == (6, 4, 37) and list_ops.array_to_lists(m4, c4) == [lst[:4] for lst in lists]
    # counts of reads without a list (negative error codes) give no entries
    assert list_ops.array_to_lists(msgs[:2], np.array([-6, 1])) == [[], lists[1]]
    # Decoder.decode's results
    res = [(msgs[2, :5].copy(), np.zeros(5, np.float32)), -6, (msgs[1, :1].copy(), np.zeros(1, np.float32))]
    m, c = list_ops.results_to_array(res, 8, 37)
    assert c.tolist() == [5, -6, 1] and np.array_equal(m[0], msgs[2]) and not m[1].any() and np.array_equal(m[2], msgs[1])
    assert list_ops.lists_to_array([])[0].shape == (0, 1, 1) and list_ops.lists_to_array([[]])[1].tolist() == [0]
    with pytest.raises(ValueError):
        list_ops.lists_to_array([["0101", "011"]])
    with pytest.raises(ValueError):
        list_ops.lists_to_array([["0121"]])


def test_drivers_take_their_options():
    p = simulator.build_parser()
    assert p.parse_args([]).stats == "host" and p.parse_args(["--stats", "device"]).stats == "device"
    with pytest.raises(SystemExit):
        p.parse_args(["--stats", "gpu"])
    base = ["--decoded_lists_dir", "d", "--conv_input_file", "c"]
    p = compute_error_rate_from_decoded_lists.build_parser()
    assert p.parse_args(base).list_ops == "host" and p.parse_args(base + ["--list_ops", "device"]).list_ops == "device"
    base = ["--num_reads_total", "4", "--num_reads_to_use", "2", "--decoded_lists_dir", "d", "--original_file", "o"]
    p = decode_RS_from_decoded_lists.build_parser()
    assert p.parse_args(base).list_ops == "host" and p.parse_args(base + ["--list_ops", "device"]).list_ops == "device"
    from nanopore_dna_storage_amd import rs_code
    with pytest.raises(ValueError):
        rs_code.decode_from_lists([], 18, 16, 72, list_ops="gpu")
    # the host paths are what they were
    conv_in = [helper.attach_index_crc(i, bytes([i] * 4)) for i in range(3)]
    t = helper.tally_decoded_lists([["0" * 52, conv_in[0]], ["0" * 52]], conv_in, 4, False, 8)
    assert t == dict(num_reads=2, num_correct=1, num_erasure_CRC_index=1, num_error_CRC_index=0)


@pytest.fixture(scope="module")
def kernel_meta(tmp_path_factory):
    if not os.path.exists(HIPCC):
        pytest.skip("no hipcc")
    out = str(tmp_path_factory.mktemp("asm") / "ls_k.s")
    src = os.path.join(ROOT, "nanopore_dna_storage_amd", "csrc", "ls_kernels.hip")
    subprocess.run([HIPCC, "--offload-arch=gfx950", "-O3", "-std=c++17", "-ffp-contract=off", "-fno-fast-math", "--cuda-device-only",
                    "-S", "-o", out, src], check=True, cwd=os.path.dirname(src))
    res = {}
    for b in open(out).read().split("- .agpr_count:")[1:]:
        g = lambda k: re.search(r"\.%s:\s+(\S+)" % k, b).group(1)
        res[g("name")] = dict(vgpr=int(g("vgpr_count")), sgpr=int(g("sgpr_count")), lds=int(g("group_segment_fixed_size")),
                              scratch=int(g("private_segment_fixed_size")))
    return res


def test_kernels_use_no_scratch(kernel_meta):
    """six kernels, none with a private segment, each within 128 registers (four wavefronts per SIMD stay possible); the
    Myers recurrence keeps its 256-bit words in registers"""
    names = ["ls_filter", "ls_bucket_count", "ls_bucket_scan", "ls_consensus", "ls_stats", "ls_edit"]
    assert len(kernel_meta) == len(names), list(kernel_meta)
    for pat in names:
        got = [v for k, v in kernel_meta.items() if re.search(r"\d%sE" % pat, k)]
        assert len(got) == 1, pat
        print(pat, got[0])
        assert got[0]["scratch"] == 0 and got[0]["vgpr"] <= 128, (pat, got[0])
