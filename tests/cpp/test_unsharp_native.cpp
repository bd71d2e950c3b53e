// Native unit tests for the CPU twin of the unsharp mask (no GPU, no HIP
// calls): cpu_unsharp and cpu_unsharp_convolve against a scalar loop in 64-bit
// integers, into heap buffers of EXACTLY the image's size, so that
// AddressSanitizer sees any byte written or read past an edge; serial against
// OpenMP, in place and out of place, both depths, and hand-made pairs on every
// boundary of the formula.  Built by `make -C <pkg>/csrc test-native` with
// AddressSanitizer + UndefinedBehaviorSanitizer next to test_native.cpp.
#include <algorithm>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <string>
#include <vector>

#include "pconv/cpu_stencil.hpp"
#include "pconv/image.hpp"

using namespace pconv;

namespace {

int g_failures = 0, g_checks = 0;

#define EXPECT(cond)                                                         \
  do {                                                                       \
    ++g_checks;                                                              \
    if (!(cond)) {                                                           \
      ++g_failures;                                                          \
      std::fprintf(stderr, "%s:%d: EXPECT failed: %s\n", __FILE__, __LINE__, #cond); \
    }                                                                        \
  } while (0)

template <typename F>
std::string thrown(F&& f) {
  try {
    f();
  } catch (const std::exception& e) {
    return e.what();
  }
  return "";
}

bool has(const std::string& s, const char* what) { return s.find(what) != std::string::npos; }

// The definition, in 64-bit integers with an explicit floor division.
int64_t formula(int64_t x, int64_t b, int64_t k, int64_t t, int64_t top) {
  const int64_t d = x - b;
  if ((d < 0 ? -d : d) < t) return x;
  const int64_t num = x * (16 + k) - b * k + 8;
  int64_t q = num / 16;
  if (num % 16 != 0 && num < 0) --q;  // floor
  return q < 0 ? 0 : q > top ? top : q;
}

// Samples of either depth as host-order values in a byte buffer of exact size.
struct Samples {
  int depth;
  std::vector<uint8_t> bytes;
  Samples(int depth_, size_t n) : depth(depth_), bytes(n * static_cast<size_t>(depth_ / 8)) {}
  size_t count() const { return bytes.size() / static_cast<size_t>(depth / 8); }
  int64_t get(size_t i) const {
    if (depth == 8) return bytes[i];
    uint16_t v;
    std::memcpy(&v, bytes.data() + 2 * i, 2);
    return v;
  }
  void set(size_t i, int64_t v) {
    if (depth == 8) {
      bytes[i] = static_cast<uint8_t>(v);
    } else {
      const uint16_t s = static_cast<uint16_t>(v);
      std::memcpy(bytes.data() + 2 * i, &s, 2);
    }
  }
};

void fill_random(Samples& s, uint32_t seed) {
  uint32_t x = seed * 2654435761u + 12345u;
  for (auto& b : s.bytes) {
    x = x * 1664525u + 1013904223u;
    b = static_cast<uint8_t>(x >> 24);
  }
}

void test_argument_checks() {
  EXPECT(unsharp_k(0.0625) == 1 && unsharp_k(1.0) == 16 && unsharp_k(1.5) == 24 && unsharp_k(15.9375) == 255);
  for (const double bad : {0.0, 0.03, 16.0, 1.01, -1.0})
    EXPECT(has(thrown([&] { unsharp_k(bad); }), "unsharp amount must be a multiple of 1/16 in [0.0625, 15.9375], got"));
  EXPECT(thrown([] { check_unsharp(1, 0, 8); }).empty() && thrown([] { check_unsharp(255, 255, 8); }).empty());
  EXPECT(thrown([] { check_unsharp(255, 65535, 16); }).empty());
  EXPECT(has(thrown([] { check_unsharp(16, 256, 8); }), "unsharp threshold must be an integer in [0, 255]"));
  EXPECT(has(thrown([] { check_unsharp(16, 65536, 16); }), "unsharp threshold must be an integer in [0, 65535]"));
  EXPECT(has(thrown([] { check_unsharp(16, -1, 8); }), "unsharp threshold"));
  EXPECT(has(thrown([] { check_unsharp(0, 0, 8); }), "unsharp amount"));
  EXPECT(has(thrown([] { check_unsharp(256, 0, 8); }), "unsharp amount"));
}

// Hand-made pairs on every boundary, with the value each must give.
void test_boundaries() {
  for (const int depth : {8, 16}) {
    const int64_t top = depth == 8 ? 255 : 65535;
    struct Case {
      int64_t x, b;
      int k, t;
      int64_t want;
    };
    const int t = static_cast<int>(top / 8);
    const Case cases[] = {
        {0, top, 16, 0, 0},              // the most negative numerator of amount 1
        {0, top, 255, 0, 0},             // ... and of the largest amount
        {top, 0, 16, 0, top},            // 2 top + ..., clamped
        {top, 0, 255, 0, top},           // the largest numerator
        {0, 9, 1, 0, 0},                 // numerator -1: floor gives -1, clamped to 0
        {0, 8, 1, 0, 0},                 // numerator 0
        {top, top - 7, 1, 0, top},       // numerator 16 top + 15: exactly top
        {top, top - 8, 1, 0, top},       // numerator 16 top + 16: top + 1, clamped
        {1, 9 + 17, 1, 0, 0},            // numerator -1 away from x = 0
        {t, 0, 24, t, formula(t, 0, 24, t, top)},          // |d| = t: sharpened
        {0, t, 24, t, 0},                                  // d = -t: sharpened (clamps at 0)
        {t - 1, 0, 24, t, t - 1},                          // |d| = t - 1: kept
        {0, t - 1, 24, t, 0},                              // d = -(t - 1): kept
        {top, top - t, 24, t, top},                        // |d| = t at the top: clamps at max
        {top - (t - 1), top, 24, t, top - (t - 1)},        // kept
        {top, 0, 16, static_cast<int>(top), formula(top, 0, 16, top, top)},  // |d| = t = max: sharpened
        {top - 1, 0, 16, static_cast<int>(top), top - 1},  // t = max keeps everything below
        {7, 7, 255, 0, 7},                                 // d = 0: unchanged at any amount
    };
    for (const auto& c : cases) {
      EXPECT(formula(c.x, c.b, c.k, c.t, top) == c.want);
      for (const CpuBackend be : {CpuBackend::Serial, CpuBackend::OpenMP}) {
        // the pair alone in a 1 x 1 image: exact-size buffers of one sample
        const ImageGeom one{1, 1, Channels::Grey, depth};
        Samples x(depth, 1), b(depth, 1), out(depth, 1);
        x.set(0, c.x);
        b.set(0, c.b);
        out.set(0, 0x5A);
        cpu_unsharp(one, x.bytes.data(), b.bytes.data(), out.bytes.data(), c.k, c.t, be, 2);
        EXPECT(out.get(0) == c.want);
        cpu_unsharp(one, x.bytes.data(), b.bytes.data(), b.bytes.data(), c.k, c.t, be, 2);  // in place
        EXPECT(b.get(0) == c.want);
      }
    }
  }
}

void test_cpu_unsharp_random() {
  const Channels chans[] = {Channels::Grey, Channels::Rgb, Channels::Rgba};
  const int64_t shapes[][2] = {{1, 1}, {9, 1}, {1, 9}, {21, 13}, {64, 37}};
  for (const int depth : {8, 16}) {
    const int64_t top = depth == 8 ? 255 : 65535;
    const int pairs[][2] = {{1, 0}, {16, 0}, {255, 0}, {24, static_cast<int>(top / 8)}, {16, static_cast<int>(top)}};
    for (const Channels ch : chans)
      for (const auto& wh : shapes) {
        const ImageGeom g{wh[0], wh[1], ch, depth};
        const size_t n = static_cast<size_t>(g.bytes()) / static_cast<size_t>(depth / 8);
        Samples x(depth, n), b(depth, n);
        fill_random(x, static_cast<uint32_t>(wh[0] * 31 + wh[1] + depth));
        fill_random(b, static_cast<uint32_t>(wh[0] * 17 + wh[1] * 3 + depth));
        for (size_t i = 0; i < n; i += 3) b.set(i, std::min<int64_t>(top, x.get(i) + static_cast<int64_t>(i % 9)));
        for (const auto& kt : pairs) {
          Samples want(depth, n);
          for (size_t i = 0; i < n; ++i) want.set(i, formula(x.get(i), b.get(i), kt[0], kt[1], top));
          Samples serial(depth, n), omp(depth, n);
          std::memset(serial.bytes.data(), 0xA5, serial.bytes.size());
          std::memset(omp.bytes.data(), 0xA5, omp.bytes.size());
          cpu_unsharp(g, x.bytes.data(), b.bytes.data(), serial.bytes.data(), kt[0], kt[1], CpuBackend::Serial);
          cpu_unsharp(g, x.bytes.data(), b.bytes.data(), omp.bytes.data(), kt[0], kt[1], CpuBackend::OpenMP, 3);
          EXPECT(serial.bytes == want.bytes);
          EXPECT(omp.bytes == serial.bytes);
          Samples inplace = b;  // out == blurred
          cpu_unsharp(g, x.bytes.data(), inplace.bytes.data(), inplace.bytes.data(), kt[0], kt[1], CpuBackend::OpenMP, 3);
          EXPECT(inplace.bytes == want.bytes);
        }
      }
  }
}

void test_cpu_unsharp_convolve() {
  const int64_t shapes[][2] = {{1, 1}, {21, 13}, {64, 37}};
  for (const int depth : {8, 16}) {
    const int64_t top = depth == 8 ? 255 : 65535;
    for (const Border border : {Border::Zero, Border::Replicate})
      for (const auto& wh : shapes) {
        const ImageGeom g{wh[0], wh[1], Channels::Rgb, depth};
        const size_t n = static_cast<size_t>(g.bytes()) / static_cast<size_t>(depth / 8);
        Samples x(depth, n), blurred(depth, n), want(depth, n);
        fill_random(x, static_cast<uint32_t>(wh[0] + 7 * wh[1] + depth));
        cpu_convolve(Filter::gaussian(), g, x.bytes.data(), blurred.bytes.data(), 3, CpuBackend::Serial, 0, border);
        const int k = 24, t = static_cast<int>(top / 64);
        for (size_t i = 0; i < n; ++i) want.set(i, formula(x.get(i), blurred.get(i), k, t, top));
        for (const CpuBackend be : {CpuBackend::Serial, CpuBackend::OpenMP}) {
          Samples out(depth, n);
          cpu_unsharp_convolve(Filter::gaussian(), g, x.bytes.data(), out.bytes.data(), 3, k, t, be, 3, border);
          EXPECT(out.bytes == want.bytes);
          Samples inplace = x;  // out == in
          cpu_unsharp_convolve(Filter::gaussian(), g, inplace.bytes.data(), inplace.bytes.data(), 3, k, t, be, 3, border);
          EXPECT(inplace.bytes == want.bytes);
          Samples same(depth, n);  // reps = 0: b = x, out = x
          cpu_unsharp_convolve(Filter::gaussian(), g, x.bytes.data(), same.bytes.data(), 0, k, t, be, 3, border);
          EXPECT(same.bytes == x.bytes);
        }
      }
  }
}

}  // namespace

int main() {
  test_argument_checks();
  test_boundaries();
  test_cpu_unsharp_random();
  test_cpu_unsharp_convolve();
  std::printf("test_unsharp_native: %d checks, %d failures\n", g_checks, g_failures);
  return g_failures == 0 ? 0 : 1;
}
