// Native unit tests for the host side of a launch's image set (no GPU, no HIP
// calls): the extents table BatchEngine::upload_sized builds, the packed
// buffer's size, the launch guards of StencilLaunch::images and their order,
// the guards they share with launch_decimate and launch_unsharp (ImageTables),
// the kernels' image-set arguments and the tuners' live-workgroup count.  Built by `make -C <pkg>/csrc test-native` with
// AddressSanitizer + UndefinedBehaviorSanitizer next to test_native.cpp.
#include <cstdio>
#include <functional>
#include <string>
#include <vector>

#include "pconv/batch_engine.hpp"
#include "pconv/kernels.hpp"
#include "image_set.hpp"

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
  a.images.frames = static_cast<int>(host.size());
  a.images.stride = 384 * 77;
  a.images.dims = device_table;
  a.images.dims_host = host.data();
  return a;
}

// The envelope's frames without extents, `table` naming the grid's images.
StencilLaunch with_table(int frames, const std::vector<int32_t>& table) {
  static const int32_t device_table[8] = {};  // only its address is looked at
  StencilLaunch a = envelope({});
  a.images.frames = frames;
  a.images.dims = nullptr;
  a.images.dims_host = nullptr;
  a.images.active = device_table;
  a.images.active_host = table.data();
  a.images.count = static_cast<int>(table.size());
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
    b.images.dims_host = nullptr;
    EXPECT(has(thrown([&] { check_dims("t", b, 3); }), "given together"));
    b = a;
    b.images.dims = nullptr;
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

void test_active_guards() {
  const std::vector<int32_t> good = {1, 3};
  const StencilLaunch a = with_table(4, good);
  EXPECT(thrown([&] { check_active("t", a); }).empty());
  EXPECT(thrown([&] { check_image_set("t", a, 3); }).empty());
  EXPECT(a.images.has_table() && a.images.images() == 2 && a.images.frame_of(0) == 1 && a.images.frame_of(1) == 3);
  StencilLaunch none;  // no table at all: nothing to check, image k is frame k
  EXPECT(thrown([&] { check_active("t", none); }).empty());
  EXPECT(!none.images.has_table() && none.images.images() == 1 && none.images.frame_of(0) == 0 && none.images.single());
  {
    StencilLaunch b = a;
    b.images.active_host = nullptr;
    EXPECT(has(thrown([&] { check_active("t", b); }), "t: active and active_host must be given together"));
    b = a;
    b.images.active = nullptr;
    EXPECT(has(thrown([&] { check_active("t", b); }), "t: active and active_host must be given together"));
  }
  {
    const StencilLaunch b = with_table(1, good);
    EXPECT(has(thrown([&] { check_active("t", b); }), "t: active holds 2 entries, more than batch_frames 1"));
    StencilLaunch e = a;  // a table of no entries
    e.images.count = 0;
    EXPECT(has(thrown([&] { check_active("t", e); }), "t: active needs batch >= 1 entries"));
    EXPECT(has(thrown([&] { check_image_set("t", e, 3); }), "t: batch must be >= 1"));
  }
  {
    const std::vector<int32_t> neg = {-1, 2}, big = {1, 4};
    EXPECT(has(thrown([&] { check_active("t", with_table(4, neg)); }), "t: active[0] = -1 is outside [0, batch_frames 4)"));
    EXPECT(has(thrown([&] { check_active("t", with_table(4, big)); }), "t: active[1] = 4 is outside [0, batch_frames 4)"));
    const std::vector<int32_t> equal = {1, 1}, down = {2, 0};
    EXPECT(has(thrown([&] { check_active("t", with_table(4, equal)); }),
               "t: active[1] = 1 does not exceed the entry before it (the table must be strictly increasing)"));
    EXPECT(has(thrown([&] { check_active("t", with_table(4, down)); }),
               "t: active[1] = 0 does not exceed the entry before it (the table must be strictly increasing)"));
  }
  {
    // the stride rules are the FRAMES': 4 frames, whatever the single entry
    const std::vector<int32_t> one = {3};
    StencilLaunch b = with_table(4, one);
    EXPECT(thrown([&] { check_image_set("t", b, 3); }).empty());
    b.images.stride = 384 * 77 + 8;
    EXPECT(has(thrown([&] { check_image_set("t", b, 3); }), "t: batch_stride must be a multiple of 16"));
    b.images.stride = 384 * 77 - 16;
    EXPECT(has(thrown([&] { check_image_set("t", b, 3); }), "is smaller than a frame (29568 bytes): frames would overlap"));
    b.images.frames = 1;  // one frame has no stride to obey, but the table no longer fits
    EXPECT(has(thrown([&] { check_image_set("t", b, 3); }), "t: active[0] = 3 is outside [0, batch_frames 1)"));
  }
}

// check_image_set reports the frames first, then the table, then the extents.
void test_guard_order() {
  const std::vector<ImageDims> bad_dims = {{231, 61}, {2, 1}, {231, 61}, {231, 61}};
  const std::vector<int32_t> bad_table = {2, 2};
  static const int32_t device_table[8] = {};
  StencilLaunch a = envelope(bad_dims);
  a.images.active = device_table;
  a.images.active_host = bad_table.data();
  a.images.count = 2;
  a.images.stride = 384 * 77 + 8;
  EXPECT(has(thrown([&] { check_image_set("t", a, 3); }), "multiple of 16"));  // all three are wrong
  a.images.stride = 384 * 77;
  EXPECT(has(thrown([&] { check_image_set("t", a, 3); }), "active[1] = 2 does not exceed"));
  const std::vector<int32_t> table = {0, 2};  // the bad extent is frame 1's: checked although no grid slot names it
  a.images.active_host = table.data();
  EXPECT(has(thrown([&] { check_image_set("t", a, 3); }), "dims[1].row_bytes"));
  const std::vector<ImageDims> good_dims = {{231, 61}, {3, 1}, {231, 61}, {231, 61}};
  a.images.dims_host = good_dims.data();
  EXPECT(thrown([&] { check_image_set("t", a, 3); }).empty());
  // "not supported by kernel": the first present feature of the list
  EXPECT(has(thrown([&] { check_temporal_only("t", "int9", {{"active", false}, {"dims", true}, {"batch", true}}); }),
             "t: dims not supported by kernel 'int9' (temporal and float_temporal only)"));
  EXPECT(thrown([&] { check_temporal_only("t", "int9", {{"active", false}, {"dims", false}}); }).empty());
}

// The shared guards as launch_decimate and launch_unsharp call them: on bare
// ImageTables, with the launch's own envelope, unit and noun.
void test_pointwise_guards() {
  static const ImageDims device_dims[4] = {};  // only the addresses are looked at
  static const int32_t device_active[4] = {};
  const std::vector<ImageDims> good = {{240, 10}, {6, 1}, {12, 10}};
  ImageTables t;
  t.frames = 3;
  EXPECT(thrown([&] { check_extents("t", t, 240, 10, 6, "pixels"); }).empty());  // no table: nothing to check
  EXPECT(!t.has_dims() && !t.has_table() && t.images() == 3 && t.dims_entries() == 3);
  t.dims_host = good.data();
  EXPECT(has(thrown([&] { check_extents("t", t, 240, 10, 6, "pixels"); }),
             "t: dims and dims_host must be given together (the device table and its host copy)"));
  t.dims_host = nullptr;
  t.dims = device_dims;
  EXPECT(has(thrown([&] { check_extents("t", t, 240, 10, 2, "samples"); }), "t: dims and dims_host must be given together"));
  t.dims_host = good.data();
  EXPECT(thrown([&] { check_extents("t", t, 240, 10, 6, "pixels"); }).empty());
  EXPECT(thrown([&] { check_extents("t", t, 240, 10, 2, "samples"); }).empty());
  // whole images, in the words of the launch that asks (launch_decimate: g_row0 = 0), after the pair, before the entries
  EXPECT(has(thrown([&] { check_extents("t", t, 240, 10, 6, "pixels", false, "g_row0 = 0"); }),
             "t: dims needs whole images (g_row0 = 0)"));
  const auto with_entry = [&](int at, ImageDims d) {
    std::vector<ImageDims> v = good;
    v[at] = d;
    return v;
  };
  // unit 2, "samples" (launch_unsharp at depth 16): odd, none, beyond the envelope, negative
  for (const int rb : {5, 0, 1, 242, -2}) {
    const std::vector<ImageDims> bad = with_entry(1, {rb, 1});
    t.dims_host = bad.data();
    EXPECT(has(thrown([&] { check_extents("t", t, 240, 10, 2, "samples"); }),
               ("t: dims[1].row_bytes " + std::to_string(rb) + " is no whole number of samples inside the envelope's 240")
                   .c_str()));
  }
  // unit 6, "pixels" (launch_decimate, 16-bit rgb): half a pixel, a whole sample but no pixel, beyond the envelope
  for (const int rb : {3, 8, 0, 246}) {
    const std::vector<ImageDims> bad = with_entry(2, {rb, 1});
    t.dims_host = bad.data();
    EXPECT(has(thrown([&] { check_extents("t", t, 240, 10, 6, "pixels"); }),
               ("t: dims[2].row_bytes " + std::to_string(rb) + " is no whole number of pixels inside the envelope's 240")
                   .c_str()));
  }
  const std::vector<ImageDims> four_samples = with_entry(2, {8, 1});  // no 6-byte pixels, but whole 2-byte samples
  t.dims_host = four_samples.data();
  EXPECT(thrown([&] { check_extents("t", t, 240, 10, 2, "samples"); }).empty());
  for (const int h : {0, 11, -1}) {
    const std::vector<ImageDims> bad = with_entry(0, {240, h});
    t.dims_host = bad.data();
    EXPECT(has(thrown([&] { check_extents("t", t, 240, 10, 6, "pixels"); }),
               ("t: dims[0].height " + std::to_string(h) + " is outside [1, the envelope's 10]").c_str()));
  }
  // the first bad entry is the one reported, its row bytes before its height
  const std::vector<ImageDims> two = {{240, 10}, {7, 0}, {0, 0}};
  t.dims_host = two.data();
  EXPECT(has(thrown([&] { check_extents("t", t, 240, 10, 6, "pixels"); }), "dims[1].row_bytes 7"));

  // an active table, by either pointer
  ImageTables a;
  a.frames = 2;
  EXPECT(thrown([&] { check_no_active("t", a, "decimated"); }).empty());
  const std::vector<int32_t> table = {0, 1};
  a.active_host = table.data();
  EXPECT(has(thrown([&] { check_no_active("t", a, "decimated"); }),
             "t: an active table is not supported (every frame of the set is decimated)"));
  a.active_host = nullptr;
  a.active = device_active;
  EXPECT(has(thrown([&] { check_no_active("t", a, "sharpened"); }),
             "t: an active table is not supported (every frame of the set is sharpened)"));

  // the flat grid: blocks per image and images x blocks per image both below 2^31
  EXPECT(thrown([&] { check_flat_grid("t", 64, 64, (int64_t(1) << 19) - 1); }).empty());
  EXPECT(thrown([&] { check_flat_grid("t", 1, (int64_t(1) << 31) - 1, 1); }).empty());
  EXPECT(has(thrown([&] { check_flat_grid("t", 1, int64_t(1) << 12, int64_t(1) << 20); }),
             "t: too many workgroups for one grid"));
  EXPECT(has(thrown([&] { check_flat_grid("t", int64_t(1) << 16, int64_t(1) << 15, 1); }),
             "t: too many workgroups for one grid"));

  // frames at least a frame apart
  const int64_t frame = 9 * 384 + 240;
  EXPECT(thrown([&] { check_frames_apart("t", "dst_stride", frame, "an output frame", frame); }).empty());
  EXPECT(has(thrown([&] { check_frames_apart("t", "dst_stride", frame - 1, "an output frame", frame); }),
             "t: dst_stride 3695 is smaller than an output frame (3696 bytes): frames would overlap"));
  EXPECT(has(thrown([&] { check_frames_apart("t", "orig_stride", 0, "a frame", frame); }),
             "t: orig_stride 0 is smaller than a frame (3696 bytes): frames would overlap"));
}

void test_batch_kernel_args() {
  StencilLaunch lone;  // stride 0 whatever the field holds: the kernels add nothing to the base pointers
  lone.images.stride = 4096;
  BatchKernelArgs k = batch_kernel_args(lone);
  EXPECT(k.stride == 0 && k.dims == nullptr && k.active == nullptr && k.last_frame == 0u);
  const std::vector<ImageDims> three = {{231, 61}, {3, 1}, {120, 61}};
  const StencilLaunch batch = envelope(three);
  k = batch_kernel_args(batch);
  EXPECT(k.stride == 384 * 77 && k.dims == batch.images.dims && k.active == nullptr && k.last_frame == 0u);
  const std::vector<int32_t> table = {1, 3};
  const StencilLaunch some = with_table(4, table);
  k = batch_kernel_args(some);
  EXPECT(k.stride == 384 * 77 && k.dims == nullptr && k.active == some.images.active && k.last_frame == 3u);
  const std::vector<int32_t> one = {0};  // a table over ONE frame keeps the stride too
  k = batch_kernel_args(with_table(1, one));
  EXPECT(k.stride == 384 * 77 && k.last_frame == 0u);
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
  // with a table only the frames it names count, and dims stays indexed by frame
  const std::vector<int32_t> table = {1, 3};
  static const int32_t device_table[8] = {};
  StencilLaunch t = a;
  t.images.active = device_table;
  t.images.active_host = table.data();
  t.images.count = 2;
  EXPECT(t.images.dims_entries() == 4 && t.images.images() == 2);
  EXPECT(thrown([&] { check_image_set("t", t, 1); }).empty());
  EXPECT(live_workgroups(t, 208, 48, 2) == 1 + 2);
  EXPECT(live_workgroups(t, 208, 48, 1) == 1 + 4);
}

}  // namespace

int main() {
  test_dims_table();
  test_guards();
  test_active_guards();
  test_guard_order();
  test_pointwise_guards();
  test_batch_kernel_args();
  test_live_workgroups();
  std::printf("ragged native tests: %d checks, %d failures\n", g_checks, g_failures);
  return g_failures ? 1 : 0;
}
