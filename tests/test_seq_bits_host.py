"""csrc/seq_bits.h on the host, without a GPU: the one bit-vector edit-distance step that bc_search, bc_search_multi, ls_edit
and mp_verify go through, and the one reading of a byte as a base, in a stand-alone program (tests/seq_bits_check.cpp, its
own main, built with the host compiler under AddressSanitizer and UndefinedBehaviorSanitizer) against a plain DP: every
bit of every column, the delta passed from word to word and the score, for pattern lengths at and around the word
boundaries, texts of 0, 1 and about the pattern's length that hold N, entering with hin = +1 (the whole-string distance)
and hin = 0 (free text ends, the minimum over columns and its first column)."""
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

from nanopore_dna_storage_amd import error_profile as ep

HERE = os.path.dirname(os.path.abspath(__file__))
CSRC = os.path.join(os.path.dirname(HERE), "nanopore_dna_storage_amd", "csrc")
PATTERN_LENS = (1, 63, 64, 65, 127, 128, 129, 255, 256, 1024)


@pytest.fixture(scope="module")
def report(tmp_path_factory):
    cxx = next((c for c in (os.environ.get("CXX"), "c++", "g++", "clang++") if c and shutil.which(c)), None)
    if cxx is None:
        pytest.skip("no host C++ compiler")
    exe = str(tmp_path_factory.mktemp("seq_bits") / "seq_bits_check")
    subprocess.run([cxx, "-std=c++17", "-O1", "-g", "-Wall", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                    "-I", CSRC, "-o", exe, os.path.join(HERE, "seq_bits_check.cpp")], check=True)
    p = subprocess.run([exe] + [str(m) for m in PATTERN_LENS], stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, timeout=300)
    print(p.stdout[-400:], p.stderr[-2000:])
    assert p.returncode == 0, (p.returncode, p.stdout[-400:], p.stderr[-2000:])
    return p.stdout


def test_the_step_equals_the_plain_dp_bit_for_bit(report):
    cases, columns, diffs = (int(v) for v in re.search(r"^cases (\d+) columns (\d+) differences (\d+)$", report, re.M).groups())
    assert diffs == 0
    # per pattern length: six text lengths, four kinds of text, two entry conditions; the texts about as long as the pattern
    assert cases == len(PATTERN_LENS) * 6 * 4 * 2 and columns > 2 * 4 * 3 * sum(PATTERN_LENS)


def test_every_byte_reads_as_the_definition_reads_it(report):
    codes = np.array(re.search(r"^base_code((?: \d+){256})$", report, re.M).group(1).split(), dtype=np.uint8)
    assert np.array_equal(codes, ep._CODE)
    assert codes[ord("A")] == 0 and codes[ord("T")] == 3 and codes[3] == 3 and codes[ord("N")] == ep.N == 4 and codes[ord("a")] == 4
    comp = [int(v) for v in re.search(r"^complement_code((?: \d+){5})$", report, re.M).group(1).split()]
    assert comp == [3, 2, 1, 0, ep.N]                      # the other strand's base; N stays N
