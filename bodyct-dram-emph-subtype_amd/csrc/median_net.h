// median_net.h -- the selection network of median.hip, over any value type T with med_min(T, T) / med_max(T, T) declared
// before this file is included (median.hip: packed int16 pairs; tools/median_net_check.cpp: 64 inputs of 0 / 1 per word,
// min = and, max = or, which by the 0/1 principle decides the network for every input).  MED_FN: the function qualifiers.
#pragma once

namespace median_net {

template <typename T>
MED_FN void cx(T& a, T& b) {                                      // a <- min, b <- max
  const T lo = med_min(a, b), hi = med_max(a, b);
  a = lo;
  b = hi;
}

// the minimum of v[S .. S+K-1] to v[S], the maximum to v[S+K-1]; the set is kept: ceil(3K/2) - 2 exchanges
template <int S, int K, typename T, int NV>
MED_FN void minmax(T (&v)[NV]) {
  constexpr int M = (K - 1) / 2;                                  // last index of the lower half (K odd: the middle)
#pragma unroll
  for (int i = 0; i < K / 2; ++i) cx(v[S + i], v[S + K - 1 - i]);
#pragma unroll
  for (int i = M; i > 0; --i) cx(v[S + i - 1], v[S + i]);
#pragma unroll
  for (int i = K - 1 - M; i < K - 1; ++i) cx(v[S + i], v[S + i + 1]);
}

// Forgetful selection of the median of v[0 .. N-1], N odd (3, 9, 27); v is scratch.  The set in play is v[S .. E] with
// E = N/2 + 1: after minmax v[S] and v[E] are forgotten, the next sample v[E + 1 + S] moves into v[E], and S advances
// until three are left.
template <int S, typename T, int N>
MED_FN T select_median(T (&v)[N]) {
  constexpr int E = N / 2 + 1, K = E - S + 1;
  if constexpr (K == 3) {
    return med_max(med_min(v[S], v[S + 1]), med_min(med_max(v[S], v[S + 1]), v[S + 2]));
  } else {
    minmax<S, K>(v);
    v[E] = v[E + 1 + S];
    return select_median<S + 1>(v);
  }
}

}  // namespace median_net
