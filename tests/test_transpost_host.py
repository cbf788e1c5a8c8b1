"""Host side of the transition posteriors without a GPU: header, library and binding carry the entry points, the CLI knows
`-m posterior` as an extension, the decode server answers it (stand-in decoder), the drivers take their new options."""
import io
import os
import re

import numpy as np
import pytest

import nanopore_dna_storage_amd as pkg
from nanopore_dna_storage_amd import _lib, decode_client, decode_server, generate_decoded_lists, viterbi_nanopore
from test_stream_server import _Srv

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW_API = ["lva_transpost_batch", "lva_transpost_batch_device", "lva_device_download"]


def test_header_library_and_binding_carry_the_entry_points():
    with open(os.path.join(ROOT, "include", "lva_decoder.h")) as f:
        header = f.read()
    lib = _lib.load_library()
    for name in NEW_API:
        assert re.search(r"\bint %s\(" % name, header), name
        assert hasattr(lib, name) and getattr(lib, name).argtypes, name
        assert name in _lib.EXPORTS
    assert "#define LVA_ABI_VERSION 5" in header and lib.lva_abi_version() == 5
    for method in ("posteriors", "posteriors_resident", "decode_from_scores"):
        assert callable(getattr(pkg.Decoder, method))
    off = np.zeros(1, np.int64)
    assert lib.lva_transpost_batch(None, None, off.ctypes.data, 0, None) == -10
    assert lib.lva_transpost_batch_device(None, None, off.ctypes.data, 0, None) == -10
    assert lib.lva_device_download(None, None, None, 0) == -10
    with open(os.path.join(ROOT, "nanopore_dna_storage_amd", "csrc", "Makefile")) as f:
        mk = f.read()
    assert re.search(r"^SRC\s*=.*\btp_kernels\.hip\b", mk, re.M) and re.search(r"^HDR\s*=.*\btp_kernels\.h\b", mk, re.M)


def test_package_imports_without_torch():
    import subprocess, sys
    code = ("import sys; sys.modules['torch'] = None; import nanopore_dna_storage_amd as p; "
            "from nanopore_dna_storage_amd import decoder, synth, helper, generate_decoded_lists; print('ok')")
    r = subprocess.run([sys.executable, "-c", code], cwd=ROOT, capture_output=True, text=True)
    assert r.returncode == 0 and r.stdout.strip() == "ok", r.stderr


def test_cli_knows_the_posterior_mode_as_an_extension():
    usage = viterbi_nanopore.USAGE
    assert usage.index("-h, --help") < usage.index("Extension") < usage.index("-m posterior")
    code, job = viterbi_nanopore.front(["-m", "posterior", "-i", "a.scores", "-o", "a.post"], io.StringIO(), cwd="/x")
    assert code is None and job[0].mode == "posterior" and job[0].infile == "/x/a.scores" and job[1] is False
    out = io.StringIO()
    assert viterbi_nanopore.front(["-m", "posteriors", "-i", "a", "-o", "b"], out)[0] == 255 and "Invalid mode." in out.getvalue()
    # the reference's modes still ask for their code parameters
    out = io.StringIO()
    assert viterbi_nanopore.front(["-m", "decode", "-i", "a", "-o", "b"], out)[0] == 255


def test_generate_decoded_lists_takes_input_kind():
    base = ["--post_manifest", "m", "--out_prefix", "o", "--info_file", "i", "--mem_conv", "6", "--msg_len", "60", "--rate_conv", "1", "--list_size", "4"]
    p = generate_decoded_lists.build_parser()
    assert p.parse_args(base).input_kind == "post" and p.parse_args(base + ["--input_kind", "scores"]).input_kind == "scores"
    with pytest.raises(SystemExit):
        p.parse_args(base + ["--input_kind", "logits"])


def test_server_answers_the_posterior_mode(tmp_path, monkeypatch):
    """with the stand-in decoder (its `posteriors` is a per-block normalisation): before any configuration is resident, and
    between the decodes of a resident one"""
    srv = _Srv({"LVA_SERVER_DECODER": "fake"}, ["--max-slots", "4"])
    monkeypatch.setenv(decode_client.ENV, srv.sock)
    try:
        fake = decode_server.FakeDecoder(6, 1, 60)
        for k in range(3):
            x = np.random.default_rng(k).normal(0, 2, (50 + k, 40)).astype("<f4")
            x.tofile(tmp_path / ("s%d.scores" % k))
            assert viterbi_nanopore.main(["-m", "posterior", "-i", str(tmp_path / ("s%d.scores" % k)), "-o", str(tmp_path / ("s%d.post" % k))],
                                         out=io.StringIO()) == 0
            got = np.fromfile(tmp_path / ("s%d.post" % k), dtype="<f4").reshape(-1, 40)
            assert np.array_equal(got, fake.posteriors([x])[0])
            if k == 0:                      # a decode in between: the resident configuration changes, the stream reopens
                argv = ["-m", "decode", "-i", str(tmp_path / "s0.post"), "-o", str(tmp_path / "s0.dec"), "--mem-conv", "6",
                        "--msg-len", "8", "-l", "2", "--max-deviation", "20"]
                assert viterbi_nanopore.main(argv, out=io.StringIO()) == 0 and (tmp_path / "s0.dec").exists()
        assert viterbi_nanopore.main(["-m", "posterior", "-i", str(tmp_path / "none.scores"), "-o", str(tmp_path / "n.post")],
                                     out=io.StringIO()) == 134
        assert srv.stop() == 0
    finally:
        srv.finalise()
