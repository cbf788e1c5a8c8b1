"""The decode stream's interface (header, exports, binding) and the decode server's protocol, without a GPU: the server runs a
stand-in decoder (decode_server.FakeDecoder, honoured only with LVA_TESTING=1) whose lists are a function of the posterior
bytes; everything else -- the socket, the thin client, the launcher, list files, exit codes, stdout text -- is the real code."""
import io
import json
import os
import re
import shutil
import signal
import subprocess
import sys
import tempfile
import threading
import time

import numpy as np
import pytest

import nanopore_dna_storage_amd as pkg
from nanopore_dna_storage_amd import _lib, decode_client, decode_server, viterbi_nanopore
from golden_util import GOLDEN, encode_cases

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
STREAM_API = ["lva_stream_open", "lva_stream_close", "lva_stream_submit", "lva_stream_poll", "lva_stream_pending"]
NEW_SOURCES = ["nanopore_dna_storage_amd/decode_server.py", "nanopore_dna_storage_amd/decode_client.py",
               "nanopore_dna_storage_amd/csrc/lva_api.cpp", "include/lva_decoder.h", "nanopore_dna_storage_amd/decoder.py",
               "nanopore_dna_storage_amd/_lib.py", "nanopore_dna_storage_amd/viterbi_nanopore.py", "viterbi/viterbi_nanopore.out",
               "tests/test_stream_server.py", "tests/test_gpu_stream.py", "tests/test_gpu_server.py"]


def test_header_library_and_binding_carry_the_stream():
    with open(os.path.join(ROOT, "include", "lva_decoder.h")) as f:
        header = f.read()
    lib = _lib.load_library()
    for name in STREAM_API:
        assert re.search(r"\bint %s\(" % name, header), name
        assert hasattr(lib, name) and getattr(lib, name).argtypes, name
        assert name in _lib.EXPORTS
    assert re.search(r"#define LVA_ERR_BUSY \(-13\)", header) and "#define LVA_ABI_VERSION 5" in header
    assert _lib.ERRORS[-13] == "LVA_ERR_BUSY" and _lib.ERR_BUSY == -13
    assert lib.lva_strerror(-13).decode().startswith("busy") and lib.lva_strerror(-14) == b"unknown error"
    assert lib.lva_abi_version() == 5
    for method in ("stream", "decode_iter"):
        assert callable(getattr(pkg.Decoder, method))
    # without a device nothing can be opened, and a null handle is an argument error, not a crash
    assert lib.lva_stream_open(None, 4, None) == -10 and lib.lva_stream_close(None) == -10
    assert lib.lva_stream_pending(None, None, None, None) == -10


# ---- the server with the stand-in decoder ----------------------------------------------------------------------------------

class _Srv:
    def __init__(self, extra_env=None, args=()):
        self.dir = tempfile.mkdtemp(prefix="lva")               # short: a socket path holds about 100 bytes
        self.sock = os.path.join(self.dir, "s")
        env = dict(os.environ, LVA_TESTING="1", PYTHONPATH=ROOT + os.pathsep + os.environ.get("PYTHONPATH", ""))
        env.pop(decode_client.ENV, None)
        env.update(extra_env or {})
        self.log = open(os.path.join(self.dir, "log"), "w+")
        self.proc = subprocess.Popen([sys.executable, "-m", "nanopore_dna_storage_amd.decode_server", "--socket", self.sock, *args],
                                     env=env, stderr=self.log, stdout=self.log, cwd=self.dir)
        t0 = time.monotonic()
        while not os.path.exists(self.sock):
            assert self.proc.poll() is None, "the server died: " + self.log_text()
            assert time.monotonic() - t0 < 60, "the server did not come up"
            time.sleep(0.02)

    def log_text(self):
        self.log.flush()
        with open(self.log.name) as f:
            return f.read()

    def stop(self, timeout=60):
        if self.proc.poll() is None:
            self.proc.send_signal(signal.SIGTERM)
            try:
                self.proc.wait(timeout)
            except subprocess.TimeoutExpired:
                self.proc.kill()
                self.proc.wait(10)
                raise
        return self.proc.returncode

    def finalise(self):
        try:
            if self.proc.poll() is None:
                self.proc.kill()
                self.proc.wait(10)
        finally:
            self.log.close()
            shutil.rmtree(self.dir, ignore_errors=True)


@pytest.fixture
def fake_server(monkeypatch):
    srv = _Srv({"LVA_SERVER_DECODER": "fake"}, ["--max-slots", "4"])
    monkeypatch.setenv(decode_client.ENV, srv.sock)
    yield srv
    srv.finalise()                                             # whatever the test did


def _post(path, nblk, seed):
    np.random.default_rng(seed).normal(0, 1, (nblk, 40)).astype("<f4").tofile(path)
    return np.fromfile(path, dtype="<f4").reshape(-1, 40)


def _argv(post, out, m=6, msg_len=60, L=4, rate=1, rc=""):
    # helper.py:305's wording of the command, after the executable's name
    return ["-m", "decode", "-i", str(post), "-o", str(out), "--mem-conv", str(m), "--msg-len", str(msg_len), "-l", str(L), "-t", "8",
            "-r", str(rate), rc, "--max-deviation", "20"]


def _want(post, rc, m=6, msg_len=60, L=4, rate=1):
    msgs, _ = decode_server.FakeDecoder(m, rate, msg_len, list_size=L, max_deviation=20).one(post, rc)
    return "".join("".join("1" if b else "0" for b in row) + "\n" for row in msgs)


def test_sixteen_concurrent_clients_get_their_own_lists(fake_server, tmp_path):
    results = [None] * 16

    def client(i):
        rc = "--rc" if i % 3 == 0 else ""                      # '' in the argument vector is ignored (simulator.py:82-85)
        out = io.StringIO()
        got = []
        for k in range(3):
            post = _post(tmp_path / ("c%d_%d.post" % (i, k)), 120 + 7 * i + k, 100 * i + k)
            code = viterbi_nanopore.main(_argv(tmp_path / ("c%d_%d.post" % (i, k)), tmp_path / ("c%d_%d.dec" % (i, k)), rc=rc), out=out)
            got.append((code, (tmp_path / ("c%d_%d.dec" % (i, k))).read_text() == _want(post, bool(rc))))
        results[i] = (got, out.getvalue())

    threads = [threading.Thread(target=client, args=(i,)) for i in range(16)]
    for t in threads:
        t.start()
    for t in threads:
        t.join(120)
    for i, (got, text) in enumerate(results):
        assert got == [(0, True)] * 3, (i, got)
        assert text == ("Reverse complement flag detected.\n" * 3 if i % 3 == 0 else "")
    # a second configuration behind the first
    post = _post(tmp_path / "b.post", 200, 5)
    assert viterbi_nanopore.main(_argv(tmp_path / "b.post", tmp_path / "b.dec", m=8, msg_len=100, L=8, rate=3), out=io.StringIO()) == 0
    assert (tmp_path / "b.dec").read_text() == _want(post, False, m=8, msg_len=100, L=8, rate=3)
    assert fake_server.stop() == 0
    log = fake_server.log_text()
    assert "reads=48" in log and log.count("resident") == 2 and log.rstrip().endswith("stopped")


def test_errors_are_the_reference_s(fake_server, tmp_path):
    _post(tmp_path / "a.post", 150, 1)
    out = io.StringIO()
    assert viterbi_nanopore.main(_argv(tmp_path / "a.post", tmp_path / "a.dec", m=7), out=out) == 255
    assert out.getvalue() == "Invalid mem_conv (allowed: 6, 8, 11, 14)\n" + viterbi_nanopore.USAGE + "\n" and not (tmp_path / "a.dec").exists()
    out = io.StringIO()
    assert viterbi_nanopore.main(["-m", "decode", "-i", "x"], out=out) == 255 and out.getvalue().startswith("Invalid options.\n")
    out = io.StringIO()
    assert viterbi_nanopore.main(_argv(tmp_path / "a.post", tmp_path / "a.dec", rate=6), out=out) == 255
    assert out.getvalue().startswith("Invalid rate parameter")
    assert viterbi_nanopore.main(["--no-such-option"], out=io.StringIO()) == 134
    assert viterbi_nanopore.main(_argv(tmp_path / "missing.post", tmp_path / "o"), out=io.StringIO()) == 134
    assert "resident" not in fake_server.log_text()            # none of these made a decoder
    # a matrix that is too short: abort, no output file (the golden the reference itself refused)
    assert viterbi_nanopore.main(["-m", "decode", "-i", os.path.join(GOLDEN, "err_short_post.post"), "-o", str(tmp_path / "o"),
                                  "--mem-conv", "6", "--msg-len", "60", "-l", "2", "--max-deviation", "20"], out=io.StringIO()) == 134
    assert not (tmp_path / "o").exists()


def test_encode_through_the_server_is_the_in_process_encoder(fake_server, tmp_path, monkeypatch):
    case = encode_cases()["cases"][0]
    (tmp_path / "msg.txt").write_text("".join(m + "\n" for m in case["msgs"]))
    argv = ["-m", "encode", "-i", "msg.txt", "-o", "%s", "--mem-conv", str(case["mem_conv"]), "--msg-len", str(case["msg_len"]),
            "-r", str(case["rate"])]
    monkeypatch.chdir(tmp_path)                                # relative paths are the caller's
    assert viterbi_nanopore.main([a % "via_server.txt" if a == "%s" else a for a in argv], out=io.StringIO()) == 0
    monkeypatch.delenv(decode_client.ENV)
    assert viterbi_nanopore.main([a % "direct.txt" if a == "%s" else a for a in argv], out=io.StringIO()) == 0
    assert (tmp_path / "via_server.txt").read_text() == (tmp_path / "direct.txt").read_text() != ""
    assert "resident" not in fake_server.log_text()


def test_missing_socket_is_one_line_and_exit_1(tmp_path, monkeypatch, capfd):
    monkeypatch.setenv(decode_client.ENV, str(tmp_path / "nobody"))
    assert viterbi_nanopore.main(_argv(tmp_path / "a.post", tmp_path / "a.dec"), out=io.StringIO()) == 1
    err = capfd.readouterr().err
    assert err.count("\n") == 1 and "decode server" in err and not (tmp_path / "a.dec").exists()


def test_sigterm_removes_the_socket(fake_server):
    assert os.path.exists(fake_server.sock)
    assert fake_server.stop() == 0
    assert not os.path.exists(fake_server.sock)


def test_idle_exit():
    srv = _Srv({"LVA_SERVER_DECODER": "fake"}, ["--idle-exit", "0.3"])
    try:
        assert srv.proc.wait(30) == 0 and not os.path.exists(srv.sock)
    finally:
        srv.finalise()


def test_stand_in_decoder_needs_the_testing_switch(tmp_path):
    """LVA_SERVER_DECODER alone must not put a stand-in into a user's server: without LVA_TESTING=1 the real decoder is used,
    which on a machine without a GPU answers exit code 1 and a message instead of a list"""
    if shutil.which("rocminfo") and os.path.exists("/dev/kfd"):
        pytest.skip("a GPU is present: the real decoder would decode")
    srv = _Srv({"LVA_SERVER_DECODER": "fake", "LVA_TESTING": "0"})
    try:
        _post(tmp_path / "a.post", 150, 1)
        code = decode_client.request(_argv(tmp_path / "a.post", tmp_path / "a.dec"), out=io.StringIO(), path=srv.sock, timeout=120)
        assert code == 1 and not (tmp_path / "a.dec").exists()
    finally:
        srv.finalise()


# ---- the client process imports the standard library only --------------------------------------------------------------------

_CHILD = """
import importlib.util, json, sys
spec = importlib.util.spec_from_file_location("decode_client", sys.argv[1])
mod = importlib.util.module_from_spec(spec); spec.loader.exec_module(mod)
code = mod.request(json.loads(sys.argv[2]))
print(json.dumps({"code": code, "modules": sorted(sys.modules)}))
"""


def test_client_imports_neither_numpy_nor_the_binding(fake_server, tmp_path):
    post = _post(tmp_path / "a.post", 150, 9)
    env = dict(os.environ)
    env.pop("PYTHONPATH", None)
    r = subprocess.run([sys.executable, "-c", _CHILD, os.path.join(ROOT, "nanopore_dna_storage_amd", "decode_client.py"),
                        json.dumps(_argv(tmp_path / "a.post", tmp_path / "a.dec", rc="--rc"))], env=env, capture_output=True, text=True,
                       timeout=120, cwd=str(tmp_path))
    assert r.returncode == 0, r.stderr
    lines = r.stdout.splitlines()
    assert lines[0] == "Reverse complement flag detected."
    ans = json.loads(lines[-1])
    assert ans["code"] == 0 and (tmp_path / "a.dec").read_text() == _want(post, True)
    loaded = [m for m in ans["modules"] if m.split(".")[0] in ("numpy", "ctypes", "_ctypes", "torch", "nanopore_dna_storage_amd")]
    assert loaded == []


def test_launcher_forwards_to_the_server(fake_server, tmp_path):
    post = _post(tmp_path / "tmp.x.post", 150, 10)
    exe = os.path.join(ROOT, "viterbi", "viterbi_nanopore.out")
    # helper.py:305, word for word (relative file names, '' for a forward read)
    r = subprocess.run([exe, "-m", "decode", "-i", "tmp.x.post", "-o", "tmp.x.dec", "--mem-conv", "6", "--msg-len", "60", "-l", "4", "-t", "8",
                        "-r", "1", "", "--max-deviation", "20"], capture_output=True, text=True, timeout=120, cwd=str(tmp_path))
    assert (r.returncode, r.stdout, r.stderr) == (0, "", "")
    assert (tmp_path / "tmp.x.dec").read_text() == _want(post, False)
    r = subprocess.run([exe, "-m", "decode", "-i", "tmp.x.post", "-o", "tmp.y.dec", "--mem-conv", "7", "--msg-len", "60"],
                       capture_output=True, text=True, timeout=120, cwd=str(tmp_path))
    assert r.returncode == 255 and r.stdout.startswith("Invalid mem_conv") and not (tmp_path / "tmp.y.dec").exists()


def test_new_sources_name_nothing_that_is_off_limits_on_the_gpu_machines():
    words = ["s_" + "store_dword", "s_buffer_" + "store", "s_scratch_" + "store", "s_" + "atomic", "s_buffer_" + "atomic", "s_dcache_" + "wb",
             "s_dcache_" + "discard", "HSA_" + "XNACK", "xnack" + "+", "roc" + "gdb", "DEBUG_HIP_FORCE_" + "GRAPH_QUEUES", "os.exec" + "v",
             "-fsanitize=" + "address"]
    for rel in NEW_SOURCES:
        path = os.path.join(ROOT, rel)
        if not os.path.exists(path):
            continue
        with open(path) as f:
            text = f.read().lower()
        for w in words:
            assert w.lower() not in text, (rel, w)
