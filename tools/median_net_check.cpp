// median_net_check.cpp -- proves the selection network of csrc/median_net.h on the host (no GPU): a network of min / max
// exchanges selects the median of every input iff it does so for every input of zeros and ones (0/1 principle), so all
// 2^N inputs of N = 3, 9, 27 are run, 64 per machine word (min = and, max = or), and the result is compared with the
// majority bit.  A few seconds.
//   c++ -O2 -std=c++17 -I bodyct-dram-emph-subtype_amd/csrc tools/median_net_check.cpp -o build/median_net_check && build/median_net_check
#include <cstdint>
#include <cstdio>

static inline uint64_t med_min(uint64_t a, uint64_t b) { return a & b; }
static inline uint64_t med_max(uint64_t a, uint64_t b) { return a | b; }
#define MED_FN static inline
#include "median_net.h"

// wire j of input number n carries bit j of n; word w holds the inputs 64 w .. 64 w + 63
template <int N>
static long long check() {
  static const uint64_t low[6] = {0xaaaaaaaaaaaaaaaaull, 0xccccccccccccccccull, 0xf0f0f0f0f0f0f0f0ull,
                                  0xff00ff00ff00ff00ull, 0xffff0000ffff0000ull, 0xffffffff00000000ull};
  const uint64_t inputs = 1ull << N, words = inputs < 64 ? 1 : inputs / 64;
  const uint64_t valid = inputs < 64 ? (1ull << inputs) - 1 : ~0ull;
  long long bad = 0;
  for (uint64_t w = 0; w < words; ++w) {
    uint64_t v[N], ones[5] = {0, 0, 0, 0, 0};                     // ones: the bit-sliced count of set wires (< 32)
    for (int j = 0; j < N; ++j) {
      v[j] = j < 6 ? low[j] : ((w >> (j - 6)) & 1 ? ~0ull : 0ull);
      uint64_t carry = v[j];
      for (int b = 0; b < 5; ++b) {
        const uint64_t t = ones[b] & carry;
        ones[b] ^= carry;
        carry = t;
      }
    }
    // majority: count >= N/2 + 1, by a bit-sliced comparison with the constant
    const int need = N / 2 + 1;
    uint64_t gt = 0, eq = ~0ull;
    for (int b = 4; b >= 0; --b) {
      const uint64_t c = (need >> b) & 1 ? ~0ull : 0ull;
      gt |= eq & ones[b] & ~c;
      eq &= ~(ones[b] ^ c);
    }
    const uint64_t want = gt | eq;
    const uint64_t got = median_net::select_median<0>(v);
    bad += __builtin_popcountll((got ^ want) & valid);
  }
  std::printf("N = %2d: %llu inputs, %lld wrong\n", N, (unsigned long long)inputs, bad);
  return bad;
}

int main() {
  const long long bad = check<3>() + check<9>() + check<27>();
  std::puts(bad ? "FAILED" : "ok: the network selects the median for 3, 9 and 27 samples");
  return bad ? 1 : 0;
}
