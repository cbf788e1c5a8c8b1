"""What the traceback tests share (tests/test_trellis_trace_host.py, tests/test_gpu_trellis_trace.py): a fixture's true base
sequence, the sum of a path, and the comparison of a device trace with the definition."""
import numpy as np

from nanopore_dna_storage_amd import str_to_bits
from nanopore_dna_storage_amd import trellis_score as T


def truth_seq(c):
    """the base sequence that the decode of fixture c (trellis_score_cases.case) walks for the fixture's true message"""
    return T.message_bases(*c["code"], str_to_bits(c["m"]["message"]), c["rc"], **c["sync"])


def path_sum(post, seq, tr):
    """A path without stale hops, added up: from float32 0 the posterior of the path's transition in every block, in block
    order, one float32 addition per block.  tr: start_state, enter, kind as reference_trace gives them."""
    post = np.asarray(post, np.float32).reshape(-1, 40)
    total, state, p = np.float32(0), int(tr["start_state"]), 0
    for t in range(post.shape[0]):
        if p < len(seq) and int(tr["enter"][p]) == t:
            b = int(seq[p])
            if tr["kind"][p]:
                assert state == b                            # a flop is entered from the flip of its base
                at, state = 32 + b, b + 4
            else:
                assert state != b
                at, state = b * 8 + state, b
            p += 1
        else:
            at = state * 8 + state if state < 4 else 32 + state
        total = np.float32(total + post[t, at])
    assert p == len(seq)
    return total


def same_trace(got, k, want, n):
    """is pair k of a device result (Decoder.trace_*: padded arrays) the definition's dict `want` for a sequence of n bases,
    byte for byte, padding included?"""
    stride = got["enter"].shape[1]
    return (np.asarray(got["score"][k], np.float32).tobytes() == np.asarray(want["score"], np.float32).tobytes()
            and got["enter"].dtype == np.int32 and got["kind"].dtype == np.uint8
            and np.array_equal(got["enter"][k], np.concatenate([want["enter"], np.full(stride - n, -1, np.int32)]))
            and np.array_equal(got["kind"][k], np.concatenate([want["kind"], np.full(stride - n, 255, np.uint8)]))
            and int(got["start_state"][k]) == want["start_state"] and int(got["end_state"][k]) == want["end_state"]
            and int(got["n_stale"][k]) == want["n_stale"])
