// Native unit tests of the 16-bit CPU stencil (no GPU, no HIP calls): cpu_step,
// cpu_fused_launch and cpu_convolve at depth 16 against a scalar per-sample
// loop written here, serial and OpenMP, both borders, on sizes around the row
// kernels' edges.  Built by `make -C <pkg>/csrc test-native` with
// AddressSanitizer + UndefinedBehaviorSanitizer next to test_native.cpp.
#include <algorithm>
#include <cstdio>
#include <cstring>
#include <functional>
#include <string>
#include <vector>

#include "pconv/cpu_stencil.hpp"

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

std::string thrown(const std::function<void()>& f) {
  try {
    f();
  } catch (const std::exception& e) {
    return e.what();
  }
  return "";
}

bool has(const std::string& s, const char* part) { return s.find(part) != std::string::npos; }

uint64_t g_rng = 0x9e3779b97f4a7c15ull;
uint16_t next_sample() {
  g_rng ^= g_rng << 13;
  g_rng ^= g_rng >> 7;
  g_rng ^= g_rng << 17;
  const uint32_t v = static_cast<uint32_t>(g_rng >> 20);
  // full range with saturated and empty samples planted
  return v % 11 == 0 ? 65535 : v % 13 == 0 ? 0 : static_cast<uint16_t>(v);
}

// One repetition, sample by sample: out = (sum w p) >> 4, taps outside the
// image read 0 (zero) or the nearest image sample (replicate).
std::vector<uint16_t> scalar_step(const std::vector<uint16_t>& in, int64_t w, int64_t h, int c, Border border) {
  static const int k[3] = {1, 2, 1};
  std::vector<uint16_t> out(in.size());
  for (int64_t y = 0; y < h; ++y)
    for (int64_t x = 0; x < w; ++x)
      for (int ch = 0; ch < c; ++ch) {
        uint32_t acc = 0;
        for (int dy = -1; dy <= 1; ++dy)
          for (int dx = -1; dx <= 1; ++dx) {
            int64_t yy = y + dy, xx = x + dx;
            if (border == Border::Replicate) {
              yy = std::min(std::max<int64_t>(yy, 0), h - 1);
              xx = std::min(std::max<int64_t>(xx, 0), w - 1);
            } else if (yy < 0 || yy >= h || xx < 0 || xx >= w) {
              continue;
            }
            acc += static_cast<uint32_t>(k[dy + 1] * k[dx + 1]) * in[static_cast<size_t>((yy * w + xx) * c + ch)];
          }
        out[static_cast<size_t>((y * w + x) * c + ch)] = static_cast<uint16_t>(acc >> 4);
      }
  return out;
}

const int64_t kSizes[][2] = {{1, 1}, {1, 5}, {5, 1}, {3, 3}, {2, 16}, {17, 16}, {31, 100}, {64, 65}};  // (H, W)

void test_cpu_convolve() {
  const Filter f = Filter::gaussian();
  for (const auto& hw : kSizes)
    for (const Channels chn : {Channels::Grey, Channels::Rgb, Channels::Rgba})
      for (const Border border : {Border::Zero, Border::Replicate})
        for (const CpuBackend be : {CpuBackend::Serial, CpuBackend::OpenMP}) {
          ImageGeom g;
          g.width = hw[1];
          g.height = hw[0];
          g.channels = chn;
          g.depth = 16;
          EXPECT(g.row_bytes() == g.width * channel_count(chn) * 2);
          std::vector<uint16_t> img(static_cast<size_t>(g.bytes() / 2));
          for (auto& v : img) v = next_sample();
          std::vector<uint16_t> ref = img;
          for (const int reps : {1, 2, 7}) {
            // ref advances 1 -> 2 -> ... cumulatively: recompute from img each time
            ref = img;
            for (int t = 0; t < reps; ++t) ref = scalar_step(ref, g.width, g.height, channel_count(chn), border);
            std::vector<uint16_t> out(img.size());
            cpu_convolve(f, g, reinterpret_cast<const uint8_t*>(img.data()), reinterpret_cast<uint8_t*>(out.data()),
                         reps, be, 3, border);
            EXPECT(out == ref);
          }
        }
}

// cpu_fused_launch on a band frame: g_row0 above, at and below the image
// edges, garbage in the ghost rows beyond the image (replicate border: never
// read; the zero border reads the frame's zeros there), against scalar steps of
// the whole image.
void test_fused_launch() {
  const Filter f = Filter::gaussian();
  const int64_t W = 21, H = 19;
  for (const Channels chn : {Channels::Grey, Channels::Rgb, Channels::Rgba})
    for (const Border border : {Border::Zero, Border::Replicate})
      for (const int steps : {1, 2, 3}) {
        const int c = channel_count(chn);
        std::vector<uint16_t> img(static_cast<size_t>(W * H * c));
        for (auto& v : img) v = next_sample();
        std::vector<uint16_t> ref = img;
        for (int t = 0; t < steps; ++t) ref = scalar_step(ref, W, H, c, border);
        const int64_t rb = W * c * 2;
        // bands: the top (ghost rows above the image), the middle, the bottom
        const int64_t bands[][2] = {{0, 6}, {6, 7}, {13, 6}, {0, H}};  // (y0, rows)
        for (const auto& b : bands) {
          const int64_t y0 = b[0], rows = b[1], halo = steps;
          const FrameLayout lay = FrameLayout::make(rb, rows, halo);
          std::vector<uint8_t> src(static_cast<size_t>(lay.bytes()), 0), dst(static_cast<size_t>(lay.bytes()), 0xAB);
          for (int64_t r = -halo; r < rows + halo; ++r) {
            const int64_t gy = y0 + r;
            uint8_t* p = src.data() + lay.offset(r);
            if (gy >= 0 && gy < H)
              std::memcpy(p, img.data() + gy * W * c, static_cast<size_t>(rb));
            else if (border == Border::Replicate)
              std::memset(p, 0xFF, static_cast<size_t>(rb));  // never read: garbage (zero border: the frame's zeros)
          }
          const std::vector<uint8_t> dst0 = dst;
          cpu_fused_launch(f, chn, lay, src.data(), dst.data(), 0, rows, steps, y0, H, CpuBackend::Serial, border, 16);
          bool rows_ok = true, rest_untouched = true;
          for (int64_t r = 0; r < rows; ++r)
            rows_ok = rows_ok && std::memcmp(dst.data() + lay.offset(r), ref.data() + (y0 + r) * W * c,
                                             static_cast<size_t>(rb)) == 0;
          std::vector<uint8_t> a = dst, z = dst0;
          for (int64_t r = 0; r < rows; ++r) {
            std::memset(a.data() + lay.offset(r), 0, static_cast<size_t>(rb));
            std::memset(z.data() + lay.offset(r), 0, static_cast<size_t>(rb));
          }
          rest_untouched = a == z;
          EXPECT(rows_ok);
          EXPECT(rest_untouched);
        }
      }
}

void test_named_errors() {
  ImageGeom g;
  g.width = 4;
  g.height = 4;
  g.depth = 16;
  std::vector<uint16_t> img(16, 7), out(16);
  const auto in8 = reinterpret_cast<const uint8_t*>(img.data());
  const auto out8 = reinterpret_cast<uint8_t*>(out.data());
  EXPECT(has(thrown([&] { cpu_convolve(Filter::box(), g, in8, out8, 1, CpuBackend::Serial); }), "depth 16"));
  EXPECT(has(thrown([&] { cpu_convolve_until_stable(Filter::gaussian(), g, in8, out8, 4, 2, CpuBackend::Serial); }),
             "depth 16"));
  g.depth = 12;
  EXPECT(has(thrown([&] { g.validate(); }), "depth"));
  // saturation: a constant 65535 image stays 65535 under replicate
  g.depth = 16;
  std::fill(img.begin(), img.end(), 65535);
  cpu_convolve(Filter::gaussian(), g, in8, out8, 20, CpuBackend::Serial, 0, Border::Replicate);
  EXPECT(std::all_of(out.begin(), out.end(), [](uint16_t v) { return v == 65535; }));
}

}  // namespace

int main() {
  test_cpu_convolve();
  test_fused_launch();
  test_named_errors();
  std::printf("test_depth16_native: %d checks, %d failures\n", g_checks, g_failures);
  return g_failures == 0 ? 0 : 1;
}
