// Native unit tests for the CPU twin of decimated results (no GPU, no HIP
// calls): HostFrames::copy_out_decimated and cpu_convolve's `decimate` argument
// against a scalar loop, into heap buffers of EXACTLY the decimated size, so
// that AddressSanitizer sees any byte written or read past an edge — factors
// above the width and the height included.  Built by `make -C <pkg>/csrc
// test-native` with AddressSanitizer + UndefinedBehaviorSanitizer next to
// test_native.cpp.
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

std::string thrown(int factor) {
  try {
    check_decimate(factor);
  } catch (const std::exception& e) {
    return e.what();
  }
  return "";
}

std::vector<uint8_t> random_bytes(size_t n, uint32_t seed) {
  std::vector<uint8_t> v(n);
  uint32_t x = seed * 2654435761u + 12345u;
  for (auto& b : v) {
    x = x * 1664525u + 1013904223u;
    b = static_cast<uint8_t>(x >> 24);
  }
  return v;
}

void test_extents_and_range() {
  EXPECT(decimated_extent(1, 64) == 1 && decimated_extent(64, 64) == 1 && decimated_extent(65, 64) == 2);
  EXPECT(decimated_extent(21, 2) == 11 && decimated_extent(13, 7) == 2 && decimated_extent(9, 1) == 9);
  EXPECT(thrown(1).empty() && thrown(64).empty());
  EXPECT(thrown(0).find("outside [1, 64]") != std::string::npos);
  EXPECT(thrown(65).find("outside [1, 64]") != std::string::npos);
  const ImageGeom g{21, 13, Channels::Rgb, 16};
  const ImageGeom og = decimated_geom(g, 3);
  EXPECT(og.width == 7 && og.height == 5 && og.depth == 16 && og.bytes() == 7 * 5 * 6);
}

void test_cpu_convolve_decimate() {
  const Channels chans[] = {Channels::Grey, Channels::Rgb, Channels::Rgba};
  const int64_t shapes[][2] = {{1, 1}, {9, 1}, {1, 9}, {21, 13}, {64, 64}};
  const int factors[] = {1, 2, 3, 7, 64};
  for (const CpuBackend be : {CpuBackend::Serial, CpuBackend::OpenMP})
    for (const int depth : {8, 16})
      for (const Channels ch : chans)
        for (const auto& wh : shapes) {
          const ImageGeom g{wh[0], wh[1], ch, depth};
          const std::vector<uint8_t> in = random_bytes(static_cast<size_t>(g.bytes()), static_cast<uint32_t>(wh[0] * 31 + wh[1]));
          std::vector<uint8_t> full(static_cast<size_t>(g.bytes()));
          cpu_convolve(Filter::gaussian(), g, in.data(), full.data(), 3, be, 2, Border::Replicate);
          for (const int s : factors) {
            const ImageGeom og = decimated_geom(g, s);
            std::vector<uint8_t> got(static_cast<size_t>(og.bytes()), 0xA5), want(static_cast<size_t>(og.bytes()));
            const int64_t pb = g.pixel_bytes();
            for (int64_t y = 0; y < og.height; ++y)
              for (int64_t x = 0; x < og.width; ++x)
                std::memcpy(want.data() + (y * og.width + x) * pb, full.data() + ((y * s) * g.width + x * s) * pb,
                            static_cast<size_t>(pb));
            cpu_convolve(Filter::gaussian(), g, in.data(), got.data(), 3, be, 2, Border::Replicate, s);
            EXPECT(got == want);
          }
        }
}

}  // namespace

int main() {
  test_extents_and_range();
  test_cpu_convolve_decimate();
  std::printf("test_decimate_native: %d checks, %d failures\n", g_checks, g_failures);
  return g_failures == 0 ? 0 : 1;
}
