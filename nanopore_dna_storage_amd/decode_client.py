"""Thin client of decode_server: forwards one `viterbi_nanopore.out` command line to the resident decoder and returns its
answer.  Standard library only and self-contained, so that the launcher viterbi/viterbi_nanopore.out can start it BY FILE
PATH (python3 decode_client.py ...): neither the package's __init__ (numpy) nor the ctypes binding nor anything that opens
the GPU is imported by a client process.

The environment variable LVA_DECODE_SERVER names the server's Unix-domain socket.  One request = one connection:
    -> {"argv": [...], "cwd": "..."}\\n        <- {"code": N, "stdout": "...", "stderr": "..."}\\n
If the socket is absent or refuses, one line goes to stderr and the exit code is 1: the caller asked for the server, so
there is no silent fall-back to a decoder of its own.
"""
import json
import os
import socket
import sys

ENV = "LVA_DECODE_SERVER"


def request(argv, out=None, path=None, timeout=None):
    """-> exit code; the server's stdout text is written to `out` (default sys.stdout), its stderr text to sys.stderr"""
    out = sys.stdout if out is None else out
    path = path or os.environ.get(ENV, "")
    s = socket.socket(socket.AF_UNIX, socket.SOCK_STREAM)
    try:
        s.settimeout(timeout)
        try:
            s.connect(path)
            s.sendall(json.dumps({"argv": list(argv), "cwd": os.getcwd()}).encode() + b"\n")
            buf = b""
            while not buf.endswith(b"\n"):
                part = s.recv(65536)
                if not part:
                    break
                buf += part
            if not buf.endswith(b"\n"):
                raise ConnectionError("the server closed the connection without an answer")
            ans = json.loads(buf.decode())
        except (OSError, ValueError) as e:
            print("viterbi_nanopore: decode server %r (%s): %s" % (path, ENV, e), file=sys.stderr)
            return 1
    finally:
        s.close()
    if ans.get("stdout"):
        out.write(ans["stdout"])
    if ans.get("stderr"):
        sys.stderr.write(ans["stderr"])
    return int(ans.get("code", 1))


if __name__ == "__main__":
    sys.exit(request(sys.argv[1:]))
