"""Resident decode server: one process per GPU that serves the `viterbi_nanopore.out` command line over a Unix-domain socket.

    python -m nanopore_dna_storage_amd.decode_server --socket PATH [--device N] [--max-slots S] [--idle-exit SECONDS]

The reference's scripts spawn the executable once per read (helper.py:305, simulator.py:85, generate_decoded_lists.py:90).
With LVA_DECODE_SERVER=PATH in their environment every such call becomes a thin client (decode_client.py) of this
process, which keeps ONE decoder and ONE decode stream (Decoder.stream) for the configuration in use -- mem_conv, rate,
msg_len, list size, max deviation, sync marker and period -- so a call pays neither HIP initialisation nor tables nor a
trellis allocation, and the reads of many concurrent callers share launches.

A request is the argument vector plus the caller's working directory.  The server reads the .post file, decodes, writes the
list file exactly as viterbi_nanopore.main does -- completely, before it answers, because the caller opens it as soon as
the client exits -- and answers with the reference's exit code and stdout text.  Parameter errors and `-m encode` (host
only) are answered at once, without a decoder.

One configuration is resident at a time: a request for another one (and every request behind it) waits until the current
stream is empty, then the decoder is replaced.  Start the server as a fresh child process, one per GPU; it never replaces a
running program.  SIGTERM / SIGINT: stream and decoder are closed, the socket is removed.
"""
import argparse
import collections
import hashlib
import io
import json
import os
import selectors
import signal
import socket
import sys
import time

import numpy as np

from . import helper, viterbi_nanopore
from ._lib import LvaError
from .decoder import Decoder, code_info


class _FakeStream:
    def __init__(self, dec, queue_cap):
        self._dec, self._cap, self._q = dec, queue_cap, collections.deque()

    @property
    def outstanding(self):
        return len(self._q)

    def submit(self, post, rc=False, tag=None):
        if len(self._q) >= self._cap:
            return False
        self._q.append((tag, self._dec.one(post, rc)))
        self._dec.launches += 1
        return True

    def poll(self, wait=False):
        out = list(self._q)
        self._q.clear()
        return out

    def close(self):
        self._q.clear()


class FakeDecoder:
    """Stand-in for tests of the protocol on machines without a GPU (honoured only with LVA_TESTING=1, see main): the list is a
    deterministic function of the posterior bytes, the orientation and the configuration."""

    def __init__(self, mem_conv, rate, msg_len, list_size=1, max_deviation=None, sync_marker="", sync_period=0, device=0,
                 max_slots=0):
        self.key = repr((mem_conv, rate, msg_len, list_size, max_deviation, sync_marker, sync_period)).encode()
        self.npos = code_info(mem_conv, rate, msg_len, False, sync_marker, sync_period).nstate_pos
        self.msg_len, self.list_size, self.slots, self.launches = msg_len, list_size, max_slots or 16, 0

    def one(self, post, rc):
        post = np.ascontiguousarray(post, dtype=np.float32)
        if post.shape[0] < self.npos + 1:
            return -6
        seed = hashlib.sha256(self.key + (b"rc" if rc else b"fw") + post.tobytes()).digest()
        rng = np.random.default_rng(int.from_bytes(seed[:8], "little"))
        return rng.integers(0, 2, (self.list_size, self.msg_len), dtype=np.uint8), np.zeros(self.list_size, np.float32)

    def stream(self, queue_cap=None):
        return _FakeStream(self, queue_cap or self.slots)

    def posteriors(self, scores):
        out = []
        for s in scores:
            s = np.ascontiguousarray(s, dtype=np.float32).reshape(-1, 40)
            out.append((s - np.logaddexp.reduce(s.astype(np.float64), axis=1, keepdims=True)).astype(np.float32))
        return out

    def profile(self):
        return dict(step_launches=self.launches, slots=self.slots)

    def close(self):
        pass


def _config(a):
    return (a.mem_conv, a.rate, a.msg_len, a.list_size, a.max_deviation, a.sync_marker, a.sync_period)


class Server:
    def __init__(self, path, device=0, max_slots=0, idle_exit=None, decoder_cls=Decoder, log=sys.stderr):
        self.path, self.device, self.max_slots, self.idle_exit, self.decoder_cls, self.log = path, device, max_slots, idle_exit, decoder_cls, log
        self.sel = selectors.DefaultSelector()
        self.listener = socket.socket(socket.AF_UNIX, socket.SOCK_STREAM)
        self.listener.bind(path)
        self.listener.listen(128)
        self.listener.setblocking(False)
        self.sel.register(self.listener, selectors.EVENT_READ, None)
        self.config = self.dec = self.stream = None
        self.jobs = {}                       # tag -> (connection, options, stdout text so far): reads in the stream
        self.backlog = collections.deque()   # [connection, options, rc, stdout text, matrix once read]: not yet in the stream, in arrival order
        self.next_tag = 0
        self.reads = self.blocks = 0         # of the resident configuration
        self.stop = False
        self.last_work = time.monotonic()

    def say(self, text):
        print("decode_server: " + text, file=self.log, flush=True)

    # --- connections ---------------------------------------------------------------------------
    def answer(self, conn, code, stdout="", stderr=""):
        try:
            conn.setblocking(True)
            conn.sendall(json.dumps({"code": code, "stdout": stdout, "stderr": stderr}).encode() + b"\n")
        except OSError:
            pass                             # the caller went away; its list file, if any, is written
        finally:
            conn.close()

    def accept(self):
        while True:
            try:
                conn, _ = self.listener.accept()
            except BlockingIOError:
                return
            conn.setblocking(False)
            self.sel.register(conn, selectors.EVENT_READ, bytearray())

    def readable(self, conn, buf):
        try:
            part = conn.recv(65536)
        except BlockingIOError:
            return
        except OSError:
            part = b""
        buf += part
        if part and not buf.endswith(b"\n"):
            return
        self.sel.unregister(conn)
        if not buf.endswith(b"\n"):
            conn.close()
            return
        self.last_work = time.monotonic()
        try:
            req = json.loads(buf.decode())
            argv, cwd = [str(x) for x in req["argv"]], str(req["cwd"])
        except (ValueError, KeyError, TypeError):
            self.answer(conn, 1, stderr="decode_server: malformed request\n")
            return
        self.request(conn, argv, cwd)

    def request(self, conn, argv, cwd):
        out = io.StringIO()
        try:
            code, job = viterbi_nanopore.front(argv, out, cwd=cwd)
        except SystemExit as e:              # an unknown option: cxxopts throws, the reference aborts
            code, job = int(e.code or 0), None
        except OSError:                      # (-m encode with an unreadable input: the reference aborts on it too)
            code, job = 134, None
        if code is not None:
            self.answer(conn, code, out.getvalue())
            return
        self.backlog.append([conn, job[0], job[1], out.getvalue(), None])

    # --- the resident decoder -------------------------------------------------------------------
    def close_decoder(self):
        if self.stream is not None:
            self.stream.close()
        if self.dec is not None:
            self.say("configuration %r closed: reads=%d blocks=%d launches=%d" % (self.config, self.reads, self.blocks,
                                                                               self.dec.profile()["step_launches"]))
            self.dec.close()
        self.config = self.dec = self.stream = None
        self.reads = self.blocks = 0

    def open_decoder(self, a):
        mc, rate, msg_len, L, md, sm, sp = _config(a)
        self.dec = self.decoder_cls(mc, rate, msg_len, list_size=L, max_deviation=md, sync_marker=sm, sync_period=sp,
                                    device=self.device, max_slots=self.max_slots)
        self.stream = self.dec.stream()
        self.config = _config(a)
        self.say("configuration %r resident: %d slots" % (self.config, self.dec.profile()["slots"]))

    def posterior(self, conn, a, text, scores):
        """-m posterior: scores -> .post on whatever decoder is resident (the code plays no part); its stream is empty and is
        closed for the call, as lva_transpost_batch asks"""
        try:
            if self.dec is None:
                mc, rate, msg_len = viterbi_nanopore.POSTERIOR_CODE
                self.dec = self.decoder_cls(mc, rate, msg_len, device=self.device, max_slots=1)
                self.config = (mc, rate, msg_len, 1, None, "", 0)
                self.say("configuration %r resident for -m posterior" % (self.config,))
            elif self.stream is not None:
                self.stream.close()
            self.stream = None
            post = self.dec.posteriors([scores])[0]
            self.stream = self.dec.stream()
            viterbi_nanopore.write_post(a.outfile, post)
        except (LvaError, OSError) as e:
            if self.dec is not None and self.stream is None:
                try:
                    self.stream = self.dec.stream()
                except LvaError:
                    self.close_decoder()
            self.answer(conn, 1, text, "viterbi_nanopore: %s\n" % e)
            return
        self.reads += 1
        self.blocks += int(scores.shape[0])
        self.last_work = time.monotonic()
        self.answer(conn, 0, text)

    def feed(self):
        """backlog -> stream, in arrival order; a request for another configuration waits (and holds back those behind it)
        until the stream is empty"""
        while self.backlog:
            conn, a, rc, text, post = self.backlog[0]
            if post is None:                 # (before any decoder is made for it, as the executable does)
                try:
                    post = self.backlog[0][4] = helper.read_post_file(a.infile)
                except OSError:
                    self.backlog.popleft()
                    self.answer(conn, 134, text)
                    continue
            if a.mode == "posterior":        # (extension) answered by the resident decoder, between streams
                if self.jobs:
                    return                   # the batch entry points are busy while reads are in the stream
                self.backlog.popleft()
                self.posterior(conn, a, text, post)
                continue
            if self.config != _config(a):
                if self.jobs:
                    return
                self.close_decoder()
                try:
                    self.open_decoder(a)
                except LvaError as e:
                    self.close_decoder()
                    self.backlog.popleft()
                    # runtime_error -> abort (:595-597, :604-605); anything else the reference cannot have: exit code 1
                    self.answer(conn, 134 if e.code in (-5, -7) else 1, text, "" if e.code in (-5, -7) else "viterbi_nanopore: %s\n" % e)
                    continue
            tag = self.next_tag
            if not self.stream.submit(post, rc=rc, tag=tag):
                return                       # back-pressure: after the next poll
            self.backlog.popleft()
            self.next_tag += 1
            self.jobs[tag] = (conn, a, text)
            self.reads += 1
            self.blocks += int(post.shape[0])

    def collect(self):
        for tag, res in self.stream.poll(wait=False):
            conn, a, text = self.jobs.pop(tag)
            if isinstance(res, (int, np.integer)):
                self.answer(conn, 134, text)                 # "Too small post matrix": abort, no output file
                continue
            try:
                viterbi_nanopore.write_list(a.outfile, res[0])
            except OSError as e:
                self.answer(conn, 1, text, "viterbi_nanopore: %s\n" % e)
                continue
            self.answer(conn, 0, text)
        self.last_work = time.monotonic()

    # --- main loop ------------------------------------------------------------------------------
    def serve(self):
        self.say("listening on %s (device %d)" % (self.path, self.device))
        try:
            while not self.stop:
                # while reads are in flight the loop only glances at the sockets: the stream wants its next launches
                for key, _ in self.sel.select(0.0005 if self.jobs else 0.2):
                    if key.data is None:
                        self.accept()
                    else:
                        self.readable(key.fileobj, key.data)
                self.feed()
                if self.jobs:
                    self.collect()
                    self.feed()
                elif self.idle_exit is not None and not self.backlog and time.monotonic() - self.last_work > self.idle_exit:
                    self.say("idle for %g s: leaving" % self.idle_exit)
                    break
        finally:
            self.shutdown()

    def shutdown(self):
        try:
            self.close_decoder()
        finally:
            for conn, *_ in list(self.jobs.values()) + [tuple(b) for b in self.backlog]:
                self.answer(conn, 1, stderr="viterbi_nanopore: the decode server was stopped\n")
            self.jobs.clear(); self.backlog.clear()
            self.sel.close()
            self.listener.close()
            try:
                os.unlink(self.path)
            except OSError:
                pass
            self.say("stopped")


def main(argv=None):
    p = argparse.ArgumentParser(description="resident list-Viterbi decode server (one per GPU)")
    p.add_argument("--socket", required=True, help="path of the Unix-domain socket to listen on (LVA_DECODE_SERVER of the callers)")
    p.add_argument("--device", type=int, default=0)
    p.add_argument("--max-slots", type=int, default=0, help="reads in flight on the device; 0 = the decoder's default")
    p.add_argument("--idle-exit", type=float, default=None, help="leave after this many seconds without a request")
    args = p.parse_args(argv)
    # tests of the protocol on machines without a GPU: a stand-in decoder, only together with LVA_TESTING=1
    fake = os.environ.get("LVA_TESTING") == "1" and os.environ.get("LVA_SERVER_DECODER") == "fake"
    srv = Server(args.socket, args.device, args.max_slots, args.idle_exit, FakeDecoder if fake else Decoder)

    def on_signal(signum, frame):
        srv.stop = True
    signal.signal(signal.SIGTERM, on_signal)
    signal.signal(signal.SIGINT, on_signal)
    srv.serve()
    return 0


if __name__ == "__main__":
    sys.exit(main())
