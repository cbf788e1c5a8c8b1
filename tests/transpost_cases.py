"""The fixed seeded clean score reads the CPU oracle test and the GPU chain tests share (test infrastructure).
test_transpost_ref.py holds the oracle to every one of them: the oracle, fed the float32 cast of the float64
posteriors, decodes the encoded message as the top entry.  A seed that fails there is replaced here."""
from nanopore_dna_storage_amd import synth

CLEAN_CASES = [
    dict(mem_conv=8, rate=3, msg_len=164, list_size=4, max_deviation=10, margin=6.0, seeds=(100, 101)),
    dict(mem_conv=6, rate=1, msg_len=60, list_size=4, max_deviation=20, margin=6.0, seeds=(200, 201, 202, 203)),
]


def clean_reads(case):
    """odd seeds are reverse-complement reads"""
    return [synth.make_read_scores(case["mem_conv"], case["rate"], case["msg_len"], sd, rc=bool(sd & 1), margin=case["margin"])
            for sd in case["seeds"]]
