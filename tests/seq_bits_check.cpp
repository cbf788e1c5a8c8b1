// seq_bits_check.cpp -- the stand-alone program of tests/test_seq_bits_host.py: csrc/seq_bits.h on the host, against a
// plain column-by-column DP.  Arguments: the pattern lengths.  For every length, texts of 0, 1 and about the pattern's
// length over {A C G T} with N sprinkled in and over two symbols (ties everywhere), random and a mutated copy of the
// pattern, under both entry conditions: hin = +1 (D[0][j] = j, the whole-string distance of bc_search and ls_edit) and
// hin = 0 (D[0][j] = 0, the text's ends free, the minimum over columns and its first column, as mp_verify keeps them).
// After every column, every bit of pv / mv / ph / mh of every word, the delta leaving every word and the score are
// compared with the DP (rows past the pattern's end match nothing).  Prints the byte table of base_code and
// complement_code, then "cases C columns K differences D"; exit status 1 if D > 0.
#include <algorithm>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "seq_bits.h"

using namespace lva;

static uint64_t g_state = 0x9E3779B97F4A7C15ull;
static uint32_t rnd(uint32_t n) {                        // splitmix64, top bits
  uint64_t z = (g_state += 0x9E3779B97F4A7C15ull);
  z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
  z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
  z ^= z >> 31;
  return (uint32_t)((z >> 33) % n);
}

static long g_columns = 0;

static long check(const std::vector<uint8_t>& p, const std::vector<uint8_t>& t, int hin) {
  const int m = (int)p.size(), n = (int)t.size(), W = (m + 63) / 64, M = 64 * W;
  std::vector<uint64_t> peq((size_t)4 * W, 0), pv((size_t)W, ~0ull), mv((size_t)W, 0);
  for (int i = 0; i < m; ++i)
    if (p[i] < kBaseN) peq[(size_t)p[i] * W + (i >> 6)] |= 1ull << (i & 63);
  std::vector<int> prev((size_t)M + 1), cur((size_t)M + 1);
  for (int i = 0; i <= M; ++i) prev[i] = i;
  const int wl = (m - 1) >> 6, bit = (m - 1) & 63;
  int score = m, best = m, arg = 0, want_best = m, want_arg = 0;
  long diffs = 0;
  for (int j = 1; j <= n; ++j, ++g_columns) {
    const uint32_t c = t[j - 1];
    cur[0] = hin ? j : 0;
    for (int i = 1; i <= M; ++i) {
      const bool same = i <= m && c < kBaseN && p[i - 1] == c;
      cur[i] = std::min(prev[i - 1] + (same ? 0 : 1), std::min(prev[i], cur[i - 1]) + 1);
    }
    int h = hin;
    for (int w = 0; w < W; ++w) {
      uint64_t ph, mh;
      h = bv_step_word(pv[w], mv[w], c < kBaseN ? peq[(size_t)c * W + w] : 0ull, h, ph, mh);
      if (w == wl) score += bv_row_delta(ph, mh, bit);
      for (int b = 0; b < 64; ++b) {
        const int i = 64 * w + b + 1, dv = cur[i] - cur[i - 1], dh = cur[i] - prev[i];
        diffs += ((pv[w] >> b) & 1ull) != (uint64_t)(dv == 1);
        diffs += ((mv[w] >> b) & 1ull) != (uint64_t)(dv == -1);
        diffs += ((ph >> b) & 1ull) != (uint64_t)(dh == 1);
        diffs += ((mh >> b) & 1ull) != (uint64_t)(dh == -1);
      }
      diffs += h != cur[64 * (w + 1)] - prev[64 * (w + 1)];
    }
    diffs += score != cur[m];
    if (score < best) { best = score; arg = j; }
    if (cur[m] < want_best) { want_best = cur[m]; want_arg = j; }
    prev.swap(cur);
  }
  return diffs + (best != want_best) + (arg != want_arg);
}

int main(int argc, char** argv) {
  printf("base_code");
  for (int b = 0; b < 256; ++b) printf(" %u", base_code((uint8_t)b));
  printf("\ncomplement_code");
  for (uint32_t c = 0; c <= kBaseN; ++c) printf(" %u", complement_code(c));
  printf("\n");
  long cases = 0, diffs = 0;
  for (int a = 1; a < argc; ++a) {
    const int m = atoi(argv[a]);
    if (m < 1 || m > kMaxRef) return 2;
    const int lens[] = {0, 1, m - 1, m, m + 1, m + m / 8 + 3};
    for (int n : lens) {
      for (int kind = 0; kind < 4; ++kind) {             // bit 0: two symbols; bit 1: the text is a mutated copy
        const uint32_t sym = (kind & 1) ? 2 : 4;
        std::vector<uint8_t> p((size_t)m), t((size_t)std::max(n, 0));
        for (auto& x : p) x = (uint8_t)(rnd(50) == 0 ? kBaseN : rnd(sym));
        for (size_t j = 0; j < t.size(); ++j) {
          const bool copy = (kind & 2) && j < p.size() && rnd(10) != 0;
          t[j] = copy ? p[j] : (uint8_t)(rnd(20) == 0 ? kBaseN : rnd(sym));
        }
        if ((kind & 2) && t.size() > 4) t.erase(t.begin() + rnd((uint32_t)t.size()));      // and an indel: the rest shifts
        if (!t.empty()) t[rnd((uint32_t)t.size())] = (uint8_t)kBaseN;                       // every text holds an N
        for (int hin = 0; hin <= 1; ++hin, ++cases) diffs += check(p, t, hin);
      }
    }
  }
  printf("cases %ld columns %ld differences %ld\n", cases, g_columns, diffs);
  return diffs ? 1 : 0;
}
