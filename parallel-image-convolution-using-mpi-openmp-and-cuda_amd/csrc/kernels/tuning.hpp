// Host-side helpers shared by the kernel translation units: run-time value ->
// template argument dispatch, and the first-use tuner's measuring loop.
#pragma once

#include <hip/hip_runtime_api.h>

#include <algorithm>
#include <cstddef>
#include <type_traits>
#include <utility>
#include <vector>

#include "pconv/common.hpp"
#include "pconv/device.hpp"
#include "pconv/kernels.hpp"

namespace pconv {

// f(std::integral_constant<int, bytes per pixel>) for the channel layout.
template <class F>
decltype(auto) with_channels(Channels ch, F&& f) {
  switch (ch) {
    case Channels::Grey: return f(std::integral_constant<int, 1>{});
    case Channels::Rgb: return f(std::integral_constant<int, 3>{});
    case Channels::Rgba: break;
  }
  return f(std::integral_constant<int, 4>{});
}

// f(std::integral_constant<size_t, i>) for a run-time i < N; false (f not
// called) for any other i.  A kernel family's constexpr shape table goes
// through this: f is compiled for every row, so a row IS an instantiation, and
// a shape outside the table has nothing to dispatch to.
template <class F, size_t... I>
bool with_index(size_t i, F&& f, std::index_sequence<I...>) {
  return ((i == I && (f(std::integral_constant<size_t, I>{}), true)) || ...);
}
template <size_t N, class F>
bool with_index(size_t i, F&& f) {
  return with_index(i, f, std::make_index_sequence<N>{});
}

constexpr int kTuneRepeats = 3;
constexpr int kTunePasses = 2;

// Index of the fastest of n candidates (the first of equals); launch(i)
// enqueues candidate i on `stream`.  The candidates run the REAL launch (same
// src -> dst, so the repeats are harmless: every run writes the same bytes).
// Two interleaved passes, each candidate's best kept: a single pass in a
// fixed order mis-ranked large launches (the first candidates ran while
// clocks and caches were still settling; 32768^2 grey picked a shape 7 %
// slower than the best).
template <class Launch>
size_t fastest_candidate(size_t n, hipStream_t stream, Launch&& launch) {
  if (n <= 1) return 0;
  Event e0 = Event::create(true), e1 = Event::create(true);
  std::vector<float> t(n, 1e30f);
  for (int pass = 0; pass < kTunePasses; ++pass) {
    for (size_t i = 0; i < n; ++i) {
      if (pass == 0) launch(i);  // warm (code object, caches)
      e0.record(stream);
      for (int r = 0; r < kTuneRepeats; ++r) launch(i);
      e1.record(stream);
      PCONV_HIP_CHECK(hipEventSynchronize(e1.get()));
      t[i] = std::min(t[i], Event::elapsed_ms(e0, e1));
    }
  }
  return static_cast<size_t>(std::min_element(t.begin(), t.end()) - t.begin());
}

}  // namespace pconv
