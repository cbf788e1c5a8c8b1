"""Real server, real decoder: sixteen client processes, worded as helper.py:305 words the command, against one decode_server on
the GPU; list files byte for byte the reference's, launches shared between the callers."""
import os
import re
import shutil
import subprocess

import pytest

from golden_util import GOLDEN, manifest
from test_stream_server import ROOT, _Srv

pytestmark = pytest.mark.gpu

NAMES = ["m11_r5_L8_clean", "m11_r5_L8_noisy", "m11_r5_L8_clean"]        # one forward configuration per client, three reads each
RC_NAMES = ["m11_r5_L8_clean_rc", "m11_r5_L8_noisy_rc", "m11_r5_L8_clean_rc"]


def _command(name, out):
    m = manifest()[name]
    # helper.py:305
    return [os.path.join(ROOT, "viterbi", "viterbi_nanopore.out"), "-m", "decode", "-i", name + ".post", "-o", out, "--mem-conv", str(m["mem_conv"]),
            "--msg-len", str(m["msg_len"]), "-l", str(m["list_size"]), "-t", "8", "-r", str(m["rate"]), "--rc" if m["rc"] else "",
            "--max-deviation", str(m["max_deviation"])]


def test_sixteen_client_processes_share_one_resident_decoder(tmp_path):
    for n in set(NAMES + RC_NAMES + ["m6_r1_L4_rc"]):
        shutil.copy(os.path.join(GOLDEN, n + ".post"), tmp_path / (n + ".post"))
    srv = _Srv(args=["--max-slots", "16"])
    try:
        env = dict(os.environ, LVA_DECODE_SERVER=srv.sock)
        # each client: three calls one after the other (sh runs them in turn and stops at the first failure)
        procs = []
        for c in range(16):
            names = RC_NAMES if c % 4 == 3 else NAMES
            script = " && ".join(" ".join("''" if a == "" else a for a in _command(n, "c%d_%d.dec" % (c, k))) for k, n in enumerate(names))
            procs.append(subprocess.Popen(["sh", "-c", script], cwd=str(tmp_path), env=env, stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True))
        try:
            for c, p in enumerate(procs):
                out, err = p.communicate(timeout=240)
                assert (p.returncode, err) == (0, ""), (c, p.returncode, out, err)
                assert out == ("Reverse complement flag detected.\n" * 3 if c % 4 == 3 else "")
        finally:
            for p in procs:
                if p.poll() is None:
                    p.kill()
        blocks = 0
        for c in range(16):
            for k, n in enumerate(RC_NAMES if c % 4 == 3 else NAMES):
                with open(os.path.join(GOLDEN, n + ".list"), "rb") as f:
                    assert (tmp_path / ("c%d_%d.dec" % (c, k))).read_bytes() == f.read(), (c, k)
                blocks += os.path.getsize(os.path.join(GOLDEN, n + ".post")) // 160
        # a second configuration afterwards: the decoder is replaced
        r = subprocess.run(_command("m6_r1_L4_rc", "second.dec"), cwd=str(tmp_path), env=env, capture_output=True, text=True, timeout=240)
        assert (r.returncode, r.stdout, r.stderr) == (0, "Reverse complement flag detected.\n", "")
        with open(os.path.join(GOLDEN, "m6_r1_L4_rc.list"), "rb") as f:
            assert (tmp_path / "second.dec").read_bytes() == f.read()
        assert srv.stop(120) == 0 and not os.path.exists(srv.sock)
        log = srv.log_text()
        first = re.search(r"configuration \(11, 5, .*closed: reads=(\d+) blocks=(\d+) launches=(\d+)", log)
        assert first, log
        reads, logged_blocks, launches = (int(x) for x in first.groups())
        print("server: %d reads, %d blocks, %d launches" % (reads, logged_blocks, launches))
        assert reads == 48 and logged_blocks == blocks
        assert 0 < launches < blocks, "the callers' reads did not share launches"
        assert log.count("resident") == 2
    finally:
        srv.finalise()
