"""Philox4x32-10 in numpy: the counter-based generator of the read simulator (simulate.py) and of the trial order
(trials.py).  Key = a 64-bit seed (low word, high word), counter = (item, sub, number, stream); the stream table is in
DESIGN.md section 1.  csrc/philox.h is the same function on the device."""
import numpy as np

M0, M1 = 0xD2511F53, 0xCD9E8D57
W0, W1 = 0x9E3779B9, 0xBB67AE85
STREAM_MESSAGE, STREAM_CHANNEL, STREAM_DWELL, STREAM_NOISE, STREAM_LEAD, STREAM_TRIAL, STREAM_SOURCE = range(7)
_U32 = 0xFFFFFFFF


def philox(c0, c1, c2, c3, key):
    """Philox4x32-10 of counters (c0, c1, c2, c3) (broadcast against each other) under the 64-bit key -> uint32 [..., 4]"""
    c = [np.asarray(x).astype(np.uint64) for x in np.broadcast_arrays(c0, c1, c2, c3)]
    k0, k1 = int(key) & _U32, (int(key) >> 32) & _U32
    lo = np.uint64(_U32)
    for _ in range(10):
        p0, p1 = c[0] * np.uint64(M0), c[2] * np.uint64(M1)
        c = [(p1 >> np.uint64(32)) ^ c[1] ^ np.uint64(k0), p1 & lo, (p0 >> np.uint64(32)) ^ c[3] ^ np.uint64(k1), p0 & lo]
        k0, k1 = (k0 + W0) & _U32, (k1 + W1) & _U32
    return np.stack(c, axis=-1).astype(np.uint32)
