// Native unit tests for the host side of mixed-size batches (no GPU, no HIP
// calls): the extents table BatchEngine::upload_sized builds, the packed
// buffer's size, the launch guards of StencilLaunch::dims and the tuners'
// live-workgroup count.  Built by `make -C <pkg>/csrc test-native` with
// AddressSanitizer + UndefinedBehaviorSanitizer next to test_native.cpp.
#include <cstdio>
#include <functional>
#include <string>
#include <vector>

#include "pconv/batch_engine.hpp"
#include "pconv/kernels.hpp"
#include "tuning.hpp"

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

// The message of the exception f() throws ("" when it does not throw).
std::string thrown(const std::function<void()>& f) {
  try {
    f();
  } catch (const std::exception& e) {
    return e.what();
  }
  return "";
}

bool has(const std::string& s, const char* part) { return s.find(part) != std::string::npos; }

void test_dims_table() {
  const ImageGeom env{77, 61, Channels::Rgb};
  const std::vector<ImageSize> sizes = {{77, 61}, {1, 1}, {40, 61}, {77, 2}};
  const std::vector<ImageDims> t = image_dims_table(env, 4, sizes);
  EXPECT(t.size() == 4);
  EXPECT(t[0].row_bytes == 231 && t[0].height == 61);
  EXPECT(t[1].row_bytes == 3 && t[1].height == 1);
  EXPECT(t[2].row_bytes == 120 && t[2].height == 61);
  EXPECT(t[3].row_bytes == 231 && t[3].height == 2);
  EXPECT(packed_bytes(env, sizes) == 231 * 61 + 3 + 120 * 61 + 231 * 2);
  EXPECT(image_dims_table(env, 4, {}).empty() && packed_bytes(env, {}) == 0);
  EXPECT(has(thrown([&] { image_dims_table(env, 3, sizes); }), "exceed the capacity 3"));
  for (const ImageSize z : {ImageSize{78, 1}, ImageSize{1, 62}, ImageSize{0, 1}, ImageSize{1, 0}, ImageSize{-1, 5}})
    EXPECT(has(thrown([&] { image_dims_table(env, 4, {{5, 5}, z}); }), "image 1"));
}

StencilLaunch envelope(const std::vector<ImageDims>& host) {
  static const ImageDims device_table[8] = {};  // only its address is looked at
  StencilLaunch a;
  a.pitch = 384;
  a.row_bytes = 231;
  a.r0 = 0;
  a.r1 = 61;
  a.frame_lo = -8;
  a.frame_hi = 69;
  a.steps = 8;
  a.g_row0 = 0;
  a.height = 61;
  a.batch = static_cast<int>(host.size());
  a.batch_stride = 384 * 77;
  a.dims = device_table;
  a.dims_host = host.data();
  return a;
}

void test_guards() {
  const std::vector<ImageDims> good = {{231, 61}, {3, 1}, {120, 61}};
  StencilLaunch a = envelope(good);
  EXPECT(thrown([&] { check_dims("t", a, 3); }).empty());
  StencilLaunch none;  // no dims at all: nothing to check
  EXPECT(thrown([&] { check_dims("t", none, 3); }).empty());
  {
    StencilLaunch b = a;
    b.dims_host = nullptr;
    EXPECT(has(thrown([&] { check_dims("t", b, 3); }), "given together"));
    b = a;
    b.dims = nullptr;
    EXPECT(has(thrown([&] { check_dims("t", b, 3); }), "given together"));
  }
  for (int k = 0; k < 3; ++k) {
    StencilLaunch b = a;
    (k == 0 ? b.g_row0 : k == 1 ? b.r0 : b.r1) = k == 2 ? 60 : 1;
    EXPECT(has(thrown([&] { check_dims("t", b, 3); }), "whole images"));
  }
  for (const ImageDims d : {ImageDims{0, 1}, ImageDims{2, 1}, ImageDims{232, 1}, ImageDims{234, 1}, ImageDims{-3, 1}}) {
    const std::vector<ImageDims> bad = {{231, 61}, d};
    const StencilLaunch b = envelope(bad);
    EXPECT(has(thrown([&] { check_dims("t", b, 3); }), "dims[1].row_bytes"));
  }
  for (const ImageDims d : {ImageDims{3, 0}, ImageDims{3, 62}, ImageDims{3, -1}}) {
    const std::vector<ImageDims> bad = {d};
    const StencilLaunch b = envelope(bad);
    EXPECT(has(thrown([&] { check_dims("t", b, 3); }), "dims[0].height"));
  }
}

void test_live_workgroups() {
  // tile {4, 8, 8} at 8 steps, RGB: 208 x 48 bytes x rows of output, strips in pairs
  const std::vector<ImageDims> host = {{231, 61}, {3, 1}, {208, 48}, {209, 49}};
  const StencilLaunch a = envelope(host);
  // envelope: 2 strips -> 1 strip pair, 2 row tiles
  EXPECT(live_workgroups(a, 208, 48, 2) == 2 + 1 + 1 + 2);
  // unfolded (the float kernel's columns): 2 x 2, 1, 1, 2 x 2
  EXPECT(live_workgroups(a, 208, 48, 1) == 4 + 1 + 1 + 4);
  StencilLaunch none;
  EXPECT(live_workgroups(none, 208, 48, 2) == 0);
  EXPECT(live_workgroups(a, 0, 48, 2) == 0);
}

}  // namespace

int main() {
  test_dims_table();
  test_guards();
  test_live_workgroups();
  std::printf("ragged native tests: %d checks, %d failures\n", g_checks, g_failures);
  return g_failures ? 1 : 0;
}
