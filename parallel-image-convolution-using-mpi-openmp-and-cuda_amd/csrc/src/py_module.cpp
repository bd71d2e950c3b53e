// Python bindings (pybind11) for the native engine: module `_pconv_native`.
//
// Buffers cross the boundary either as Python buffer-protocol objects (numpy
// arrays, host memory) or as raw integer addresses (torch.Tensor.data_ptr()
// of CUDA tensors or pinned host tensors) — no torch C++ ABI dependency.
#include <omp.h>
#include <pybind11/pybind11.h>
#include <pybind11/stl.h>

#include <cstring>

#include "pconv/app.hpp"
#include "pconv/batch_engine.hpp"
#include "pconv/cpu_stencil.hpp"
#include "pconv/device.hpp"
#include "pconv/engine.hpp"
#include "pconv/ipc_halo.hpp"
#include "pconv/kernels.hpp"
#include "pconv/partition.hpp"
#include "pconv/selftest.hpp"
#include "pconv/raw_io.hpp"
#include "pconv/rccl_comm.hpp"
#include "pconv/schedule.hpp"
#include "../kernels/swar.hpp"

namespace py = pybind11;
using namespace pconv;

namespace {

struct HostView {
  uint8_t* ptr;
  int64_t size;
};

HostView host_view(py::buffer b, bool writable) {
  py::buffer_info info = b.request(writable);
  PCONV_CHECK(info.itemsize == 1, "expected a uint8 buffer");
  // Must be C-contiguous.
  int64_t expect = 1;
  for (int i = info.ndim - 1; i >= 0; --i) {
    PCONV_CHECK(info.strides[i] == expect, "expected a C-contiguous buffer");
    expect *= info.shape[i];
  }
  return {static_cast<uint8_t*>(info.ptr), static_cast<int64_t>(info.size)};
}

ImageGeom make_geom(int64_t w, int64_t h, const std::string& ch, int depth = 8) {
  ImageGeom g;
  g.width = w;
  g.height = h;
  g.channels = parse_channels(ch);
  g.depth = depth;
  g.validate();
  return g;
}

KernelVariant parse_variant(const std::string& s) {
  if (s == "auto") return KernelVariant::Auto;
  if (s == "binomial") return KernelVariant::Binomial;
  if (s == "temporal") return KernelVariant::Temporal;
  if (s == "int9") return KernelVariant::Int9;
  if (s == "float9") return KernelVariant::Float9;
  if (s == "float_temporal") return KernelVariant::FloatTemporal;
  PCONV_FAIL("unknown kernel variant '" + s + "'");
}

Filter make_filter(py::object f) {
  if (py::isinstance<py::str>(f)) return Filter::by_name(f.cast<std::string>());
  return f.cast<Filter>();
}

// Halo transport implemented in Python (e.g. host-staged gloo messages for
// several ranks sharing one GPU in tests).  The Python subclass implements
// exchange_rows(row0_ptr, pitch, rows, up, down, depth, stream): fill ghost
// rows [-depth, 0) / [rows, rows+depth) of the frame whose owned row 0 starts
// at row0_ptr (pitch-aligned, pads included) and send the matching owned rows,
// enqueued on (or synchronised with) `stream`.
class PyHaloTransport : public HaloTransport {
 public:
  void exchange(BandEngine& e, int64_t depth, hipStream_t stream) override {
    py::gil_scoped_acquire gil;
    py::function f = py::get_override(static_cast<const HaloTransport*>(this), "exchange_rows");
    PCONV_CHECK(static_cast<bool>(f), "HaloTransport subclass must implement exchange_rows()");
    f(reinterpret_cast<uintptr_t>(e.src_frame() - kPadLeft), e.layout().pitch, e.band().rows, e.band().up,
      e.band().down, depth, reinterpret_cast<uintptr_t>(stream));
  }
  const char* name() const override { return "python"; }
};

// Diagnostics of the raw-pointer launch bindings: `timed` launches, each
// between two timing events on stream `s`; synchronises the stream (also when
// timed = 0) and returns the ms of each.
template <class Launch>
std::vector<double> time_launches(int timed, hipStream_t s, Launch&& launch) {
  std::vector<Event> ev;
  for (int i = 0; i < 2 * timed; ++i) ev.push_back(Event::create(true));
  for (int i = 0; i < timed; ++i) {
    ev[2 * i].record(s);
    launch();
    ev[2 * i + 1].record(s);
  }
  PCONV_HIP_CHECK(hipStreamSynchronize(s));
  std::vector<double> ms;
  for (int i = 0; i < timed; ++i) ms.push_back(Event::elapsed_ms(ev[2 * i], ev[2 * i + 1]));
  return ms;
}

}  // namespace

PYBIND11_MODULE(_pconv_native, m) {
  m.doc() = "pconv native engine: CDNA4 HIP stencil kernels, HIP runtime, RCCL halos, CPU oracle";

  py::register_exception<Error>(m, "NativeError", PyExc_RuntimeError);

  // ---------------------------------------------------------------- filters
  py::class_<Filter>(m, "Filter")
      .def_static("gaussian", &Filter::gaussian)
      .def_static("box", &Filter::box)
      .def_static("edge", &Filter::edge)
      .def_static("by_name", &Filter::by_name)
      .def_static("custom", &Filter::custom, py::arg("taps"), py::arg("divisor"), py::arg("name") = "custom")
      .def_readonly("name", &Filter::name)
      .def_readonly("taps", &Filter::taps)
      .def_readonly("divisor", &Filter::divisor)
      .def_readonly("weights", &Filter::weights)
      .def_readonly("int_exact", &Filter::int_exact)
      .def_readonly("shift", &Filter::shift)
      .def_readonly("binomial121", &Filter::binomial121)
      .def("__repr__", [](const Filter& f) { return "Filter(" + f.name + "/" + std::to_string(f.divisor) + ")"; });

  // ---------------------------------------------------------------- geometry
  m.def(
      "frame_layout",
      [](int64_t row_bytes, int64_t rows, int64_t halo) {
        const FrameLayout l = FrameLayout::make(row_bytes, rows, halo);
        return py::dict(py::arg("row_bytes") = l.row_bytes, py::arg("rows") = l.rows, py::arg("halo") = l.halo,
                        py::arg("pitch") = l.pitch, py::arg("bytes") = l.bytes(), py::arg("pad_left") = kPadLeft);
      },
      py::arg("row_bytes"), py::arg("rows"), py::arg("halo"));

  py::class_<Band>(m, "Band")
      .def(py::init<>())
      .def_readwrite("rank", &Band::rank)
      .def_readwrite("world", &Band::world)
      .def_readwrite("y0", &Band::y0)
      .def_readwrite("rows", &Band::rows)
      .def_readwrite("up", &Band::up)
      .def_readwrite("down", &Band::down)
      .def("__repr__", [](const Band& b) {
        return "Band(rank=" + std::to_string(b.rank) + ", y0=" + std::to_string(b.y0) + ", rows=" +
               std::to_string(b.rows) + ", up=" + std::to_string(b.up) + ", down=" + std::to_string(b.down) + ")";
      });
  m.def("row_band", &row_band, py::arg("height"), py::arg("world"), py::arg("rank"));
  m.def("row_bands", &row_bands, py::arg("height"), py::arg("world"));
  m.def("reference_rows_division", &reference_rows_division);

  // ---------------------------------------------------------------- schedule
  py::class_<LaunchSpec>(m, "LaunchSpec")
      .def_readonly("steps", &LaunchSpec::steps)
      .def_readonly("lo", &LaunchSpec::lo)
      .def_readonly("hi", &LaunchSpec::hi)
      .def_readonly("after_halo", &LaunchSpec::after_halo);
  py::class_<Phase>(m, "Phase")
      .def_readonly("exchange_depth", &Phase::exchange_depth)
      .def_readonly("steps", &Phase::steps)
      .def_readonly("launches", &Phase::launches);
  m.def(
      "plan_band",
      [](const Band& b, int reps, int halo_depth, int fuse, bool overlap, bool halo_preloaded) {
        PlanConfig c;
        c.halo_depth = halo_depth;
        c.fuse = fuse;
        c.overlap = overlap;
        c.halo_preloaded = halo_preloaded;
        return plan_band(b, reps, c);
      },
      py::arg("band"), py::arg("reps"), py::arg("halo_depth") = 1, py::arg("fuse") = 1, py::arg("overlap") = true,
      py::arg("halo_preloaded") = false);
  m.def(
      "normalize_plan",
      [](int halo_depth, int fuse, int64_t min_band_rows, int max_fuse) {
        PlanConfig c;
        c.halo_depth = halo_depth;
        c.fuse = fuse;
        c = normalize_plan_config(c, min_band_rows, max_fuse);
        return py::make_tuple(c.halo_depth, c.fuse);
      },
      py::arg("halo_depth"), py::arg("fuse"), py::arg("min_band_rows"), py::arg("max_fuse") = kMaxFusedSteps);
  m.def("describe_plan", &describe_plan);
  m.attr("MAX_FUSED_STEPS") = kMaxFusedSteps;
  py::class_<StreamChunk>(m, "StreamChunk")
      .def_readonly("up_lo", &StreamChunk::up_lo)
      .def_readonly("up_hi", &StreamChunk::up_hi)
      .def_readonly("launches", &StreamChunk::launches)
      .def_readonly("levels", &StreamChunk::levels)
      .def_readonly("down_lo", &StreamChunk::down_lo)
      .def_readonly("down_hi", &StreamChunk::down_hi);
  py::class_<StreamPlan>(m, "StreamPlan")
      .def_readonly("levels", &StreamPlan::levels)
      .def_readonly("chunks", &StreamPlan::chunks);
  m.def("streamable", &streamable, py::arg("plan"));
  m.def("stream_cuts", &stream_cuts, py::arg("in_lo"), py::arg("in_hi"), py::arg("chunks"));
  m.def("stream_cuts_weighted", &stream_cuts_weighted, py::arg("in_lo"), py::arg("in_hi"), py::arg("weights"));
  m.def("plan_streamed", &plan_streamed, py::arg("plan"), py::arg("in_lo"), py::arg("in_hi"), py::arg("owned_rows"),
        py::arg("cuts"));

  // ---------------------------------------------------------------- CPU oracle
  m.def(
      "cpu_convolve",
      [](py::buffer in, py::buffer out, int64_t w, int64_t h, const std::string& ch, int reps, py::object filter,
         bool omp, int threads, const std::string& border, int depth, int decimate) {
        const ImageGeom g = make_geom(w, h, ch, depth);
        const Border bd = parse_border(border);
        const HostView a = host_view(in, false), b = host_view(out, true);
        PCONV_CHECK(a.size == g.bytes() && b.size == decimated_geom(g, decimate).bytes(),
                    "buffer size does not match the image geometry");
        const Filter f = make_filter(filter);
        py::gil_scoped_release nogil;
        cpu_convolve(f, g, a.ptr, b.ptr, reps, omp ? CpuBackend::OpenMP : CpuBackend::Serial, threads, bd, decimate);
      },
      py::arg("src"), py::arg("dst"), py::arg("width"), py::arg("height"), py::arg("channels"), py::arg("reps"),
      py::arg("filter") = "gaussian", py::arg("omp") = false, py::arg("threads") = 0, py::arg("border") = "zero",
      py::arg("depth") = 8, py::arg("decimate") = 1);
  m.attr("MAX_DECIMATE") = kMaxDecimate;
  m.def(
      "cpu_unsharp",
      [](py::buffer orig, py::buffer blurred, py::buffer out, int64_t w, int64_t h, const std::string& ch, int k,
         int64_t threshold, bool omp, int threads, int depth) {
        const ImageGeom g = make_geom(w, h, ch, depth);
        const HostView a = host_view(orig, false), b = host_view(blurred, false), c = host_view(out, true);
        PCONV_CHECK(a.size == g.bytes() && b.size == g.bytes() && c.size == g.bytes(),
                    "buffer size does not match the image geometry");
        check_unsharp(k, threshold, depth);
        py::gil_scoped_release nogil;
        cpu_unsharp(g, a.ptr, b.ptr, c.ptr, k, static_cast<int>(threshold),
                    omp ? CpuBackend::OpenMP : CpuBackend::Serial, threads);
      },
      py::arg("orig"), py::arg("blurred"), py::arg("dst"), py::arg("width"), py::arg("height"), py::arg("channels"),
      py::arg("k"), py::arg("threshold") = 0, py::arg("omp") = false, py::arg("threads") = 0, py::arg("depth") = 8,
      "Unsharp mask of two tight images: dst = x + (k / 16)(x - b) per sample, exact integers (dst may be blurred).");
  m.def(
      "cpu_unsharp_convolve",
      [](py::buffer in, py::buffer out, int64_t w, int64_t h, const std::string& ch, int reps, int k,
         int64_t threshold, py::object filter, bool omp, int threads, const std::string& border, int depth) {
        const ImageGeom g = make_geom(w, h, ch, depth);
        const Border bd = parse_border(border);
        const HostView a = host_view(in, false), b = host_view(out, true);
        PCONV_CHECK(a.size == g.bytes() && b.size == g.bytes(), "buffer size does not match the image geometry");
        check_unsharp(k, threshold, depth);
        const Filter f = make_filter(filter);
        py::gil_scoped_release nogil;
        cpu_unsharp_convolve(f, g, a.ptr, b.ptr, reps, k, static_cast<int>(threshold),
                             omp ? CpuBackend::OpenMP : CpuBackend::Serial, threads, bd);
      },
      py::arg("src"), py::arg("dst"), py::arg("width"), py::arg("height"), py::arg("channels"), py::arg("reps"),
      py::arg("k"), py::arg("threshold") = 0, py::arg("filter") = "gaussian", py::arg("omp") = false,
      py::arg("threads") = 0, py::arg("border") = "zero", py::arg("depth") = 8,
      "cpu_convolve followed by cpu_unsharp against the input.");
  m.def("unsharp_k", &unsharp_k, py::arg("amount"), "amount x 16 as an exact integer in [1, 255], or an error");
  m.def("default_cpu_threads", &default_cpu_threads,
        "OpenMP team size used when none is set: affinity CPUs capped by the cgroup quota, minus one");
  m.def(
      "set_cpu_threads",
      [](int n) {
        omp_set_num_threads(std::max(1, n));
        return omp_get_max_threads();
      },
      py::arg("n"), "OpenMP team size of this process's CPU stencil (returns the size now in effect)");
  m.def("cpu_threads", []() { return omp_get_max_threads(); }, "OpenMP team size in effect");
  m.def("configure_cpu_threads", &configure_cpu_threads, py::arg("share") = 1,
        "Size the OpenMP team (unless OMP_NUM_THREADS is set) for `share` processes on this node");
  m.def(
      "cpu_fused_launch",
      [](py::object filter, const std::string& ch, int64_t row_bytes, int64_t rows, int64_t halo, py::buffer src,
         py::buffer dst, int64_t lo, int64_t hi, int steps, int64_t g_row0, int64_t height, bool omp,
         const std::string& border, int depth) {
        const Border bd = parse_border(border);
        const FrameLayout lay = FrameLayout::make(row_bytes, rows, halo);
        const HostView a = host_view(src, false), b = host_view(dst, true);
        PCONV_CHECK(a.size == lay.bytes() && b.size == lay.bytes(), "frame buffer size mismatch");
        const Filter f = make_filter(filter);
        py::gil_scoped_release nogil;
        cpu_fused_launch(f, parse_channels(ch), lay, a.ptr, b.ptr, lo, hi, steps, g_row0, height,
                         omp ? CpuBackend::OpenMP : CpuBackend::Serial, bd, depth);
      },
      py::arg("filter"), py::arg("channels"), py::arg("row_bytes"), py::arg("rows"), py::arg("halo"), py::arg("src"),
      py::arg("dst"), py::arg("lo"), py::arg("hi"), py::arg("steps"), py::arg("g_row0"), py::arg("height"),
      py::arg("omp") = false, py::arg("border") = "zero", py::arg("depth") = 8);
  m.def(
      "cpu_residual",
      [](py::buffer in, int64_t w, int64_t h, const std::string& ch, py::object filter, bool omp, int threads,
         const std::string& border) {
        const ImageGeom g = make_geom(w, h, ch);
        const Border bd = parse_border(border);
        const HostView a = host_view(in, false);
        PCONV_CHECK(a.size == g.bytes(), "buffer size does not match the image geometry");
        const Filter f = make_filter(filter);
        py::gil_scoped_release nogil;
        return cpu_image_residual(f, g, a.ptr, omp ? CpuBackend::OpenMP : CpuBackend::Serial, threads, bd);
      },
      py::arg("src"), py::arg("width"), py::arg("height"), py::arg("channels"), py::arg("filter") = "gaussian",
      py::arg("omp") = false, py::arg("threads") = 0, py::arg("border") = "zero",
      "bytes of the image that one more repetition would change (0: a fixed point)");
  m.def(
      "cpu_frame_residual",
      [](py::object filter, const std::string& ch, int64_t row_bytes, int64_t rows, int64_t halo, py::buffer src,
         int64_t r0, int64_t r1, int64_t g_row0, int64_t height, bool omp, const std::string& border) {
        const Border bd = parse_border(border);
        const FrameLayout lay = FrameLayout::make(row_bytes, rows, halo);
        const HostView a = host_view(src, false);
        PCONV_CHECK(a.size == lay.bytes(), "frame buffer size mismatch");
        const Filter f = make_filter(filter);
        py::gil_scoped_release nogil;
        return cpu_residual(f, parse_channels(ch), lay, a.ptr, r0, r1, omp ? CpuBackend::OpenMP : CpuBackend::Serial, bd,
                            g_row0, height);
      },
      py::arg("filter"), py::arg("channels"), py::arg("row_bytes"), py::arg("rows"), py::arg("halo"), py::arg("src"),
      py::arg("r0"), py::arg("r1"), py::arg("g_row0"), py::arg("height"), py::arg("omp") = false,
      py::arg("border") = "zero", "cpu_residual on a band frame (cpu_fused_launch's frame arguments)");
  m.def(
      "cpu_convolve_until_stable",
      [](py::buffer in, py::buffer out, int64_t w, int64_t h, const std::string& ch, int max_reps, int check_every,
         py::object filter, bool omp, int threads, const std::string& border) {
        const ImageGeom g = make_geom(w, h, ch);
        const Border bd = parse_border(border);
        const HostView a = host_view(in, false), b = host_view(out, true);
        PCONV_CHECK(a.size == g.bytes() && b.size == g.bytes(), "buffer size does not match the image geometry");
        const Filter f = make_filter(filter);
        StableStats st;
        {
          py::gil_scoped_release nogil;
          st = cpu_convolve_until_stable(f, g, a.ptr, b.ptr, max_reps, check_every,
                                         omp ? CpuBackend::OpenMP : CpuBackend::Serial, threads, bd);
        }
        return py::make_tuple(st.reps_done, st.converged, st.residual, st.checks);
      },
      py::arg("src"), py::arg("dst"), py::arg("width"), py::arg("height"), py::arg("channels"), py::arg("max_reps"),
      py::arg("check_every"), py::arg("filter") = "gaussian", py::arg("omp") = false, py::arg("threads") = 0,
      py::arg("border") = "zero", "(reps_done, converged, residual, checks); dst = the image after reps_done");
  m.def("border_names", []() { return std::vector<std::string>{border_name(Border::Zero), border_name(Border::Replicate)}; },
        "border modes every backend takes (the first is the default and the reference's)");

  // ---------------------------------------------------------------- raw I/O
  m.def("output_path_for", &output_path_for, py::arg("path"), py::arg("prefix") = "blur_");
  m.def(
      "read_raw",
      [](const std::string& path, py::buffer dst, int64_t w, int64_t h, const std::string& ch, int depth) {
        const ImageGeom g = make_geom(w, h, ch, depth);
        const HostView b = host_view(dst, true);
        PCONV_CHECK(b.size == g.bytes(), "buffer size does not match the image geometry");
        read_image(path, g, b.ptr);
      },
      py::arg("path"), py::arg("dst"), py::arg("width"), py::arg("height"), py::arg("channels"),
      py::arg("depth") = 8);
  m.def(
      "read_raw_rows",
      [](const std::string& path, py::buffer dst, int64_t w, int64_t h, const std::string& ch, int64_t y0,
         int64_t rows) {
        const ImageGeom g = make_geom(w, h, ch);
        const HostView b = host_view(dst, true);
        PCONV_CHECK(b.size >= rows * g.row_bytes(), "buffer too small");
        validate_input_file(path, g);
        read_rows(path, g, y0, rows, b.ptr, g.row_bytes());
      },
      py::arg("path"), py::arg("dst"), py::arg("width"), py::arg("height"), py::arg("channels"), py::arg("y0"),
      py::arg("rows"));
  m.def(
      "write_raw",
      [](const std::string& path, py::buffer src, int64_t w, int64_t h, const std::string& ch, int depth) {
        const ImageGeom g = make_geom(w, h, ch, depth);
        const HostView b = host_view(src, false);
        PCONV_CHECK(b.size == g.bytes(), "buffer size does not match the image geometry");
        write_image(path, g, b.ptr);
      },
      py::arg("path"), py::arg("src"), py::arg("width"), py::arg("height"), py::arg("channels"),
      py::arg("depth") = 8);
  m.def(
      "create_output",
      [](const std::string& path, int64_t w, int64_t h, const std::string& ch) {
        create_output(path, make_geom(w, h, ch));
      },
      py::arg("path"), py::arg("width"), py::arg("height"), py::arg("channels"));
  m.def(
      "write_raw_rows",
      [](const std::string& path, py::buffer src, int64_t w, int64_t h, const std::string& ch, int64_t y0,
         int64_t rows) {
        const ImageGeom g = make_geom(w, h, ch);
        const HostView b = host_view(src, false);
        PCONV_CHECK(b.size >= rows * g.row_bytes(), "buffer too small");
        write_rows(path, g, y0, rows, b.ptr, g.row_bytes());
      },
      py::arg("path"), py::arg("src"), py::arg("width"), py::arg("height"), py::arg("channels"), py::arg("y0"),
      py::arg("rows"));
  m.def(
      "synth_rows",
      [](py::buffer dst, int64_t w, int64_t h, const std::string& ch, uint64_t seed, int64_t y0, int64_t rows,
         int depth) {
        const ImageGeom g = make_geom(w, h, ch, depth);
        const HostView b = host_view(dst, true);
        PCONV_CHECK(b.size >= rows * g.row_bytes(), "buffer too small");
        py::gil_scoped_release nogil;
        synth_rows(g, seed, y0, rows, b.ptr, g.row_bytes());
      },
      py::arg("dst"), py::arg("width"), py::arg("height"), py::arg("channels"), py::arg("seed"), py::arg("y0"),
      py::arg("rows"), py::arg("depth") = 8);

  // ---------------------------------------------------------------- CLI
  m.def("conv_main", [](std::vector<std::string> argv) {
    std::vector<char*> ptrs;
    for (auto& s : argv) ptrs.push_back(s.data());
    py::gil_scoped_release nogil;
    return conv_main(static_cast<int>(ptrs.size()), ptrs.data());
  });

  // ---------------------------------------------------------------- device
  m.def("device_count", &device_count);
  m.def("device_name", &device_name);
  m.def("set_device", &set_device);
  m.def("device_pci_bus_id", &device_pci_bus_id);
  m.def("copy_pair_floor_ms", &copy_pair_floor_ms, py::arg("device"), py::arg("row_bytes"), py::arg("rows_in"),
        py::arg("rows_out"), py::arg("iters") = 8,
        "ms per pitched H2D + D2H pair issued concurrently on two streams (the pipeline's PCIe floor)");
  m.def(
      "page_nodes", [](uintptr_t p, size_t bytes) { return page_nodes(reinterpret_cast<const void*>(p), bytes); },
      py::arg("ptr"), py::arg("bytes"), "NUMA node -> pages of a host range (move_pages query; negative: -errno)");
  m.def("device_numa_node", &device_numa_node, py::arg("device"));
  m.def(
      "flush_host_cache",
      [](uintptr_t p, size_t bytes) {
        py::gil_scoped_release nogil;
        flush_host_cache(reinterpret_cast<const void*>(p), bytes);
      },
      py::arg("ptr"), py::arg("bytes"), "clflush a host range out of every CPU cache (staging written by the CPU)");
  m.def(
      "copy_floor_on",
      [](int device, uintptr_t host_in, uintptr_t host_out, int64_t row_bytes, int64_t rows_in, int64_t rows_out,
         int iters) {
        py::gil_scoped_release nogil;
        const CopyFloor f = copy_floor_on(device, reinterpret_cast<uint8_t*>(host_in),
                                          reinterpret_cast<uint8_t*>(host_out), row_bytes, rows_in, rows_out, iters);
        return std::make_tuple(f.h2d_ms, f.d2h_ms, f.pair_ms);
      },
      py::arg("device"), py::arg("host_in"), py::arg("host_out"), py::arg("row_bytes"), py::arg("rows_in"),
      py::arg("rows_out"), py::arg("iters") = 8,
      "(H2D alone, D2H alone, concurrent pair) ms with the given pinned host buffers (0: fresh ones)");
  py::class_<CopyProbe>(m, "CopyProbe")
      .def(py::init([](int device, int64_t row_bytes, int64_t rows_in, int64_t rows_out) {
             py::gil_scoped_release nogil;
             return std::make_unique<CopyProbe>(device, nullptr, nullptr, row_bytes, rows_in, rows_out);
           }),
           py::arg("device"), py::arg("row_bytes"), py::arg("rows_in"), py::arg("rows_out"))
      .def("run", &CopyProbe::run, py::arg("n"), py::arg("up") = true, py::arg("down") = true,
           py::call_guard<py::gil_scoped_release>(),
           "ms per copy (pair) over n pitched H2D and / or D2H copies issued on two streams");
  m.def("bind_to_device_numa", &bind_to_device_numa,
        "Restrict this process to the CPUs local to the GPU (returns the CPUs kept; 0: unchanged)");

  py::class_<PinnedBuffer>(m, "PinnedBuffer", py::buffer_protocol())
      .def(py::init<size_t>())
      .def_property_readonly("ptr", [](const PinnedBuffer& b) { return reinterpret_cast<uintptr_t>(b.data()); })
      .def("__len__", &PinnedBuffer::size)
      .def_buffer([](PinnedBuffer& b) -> py::buffer_info {
        return py::buffer_info(b.data(), 1, py::format_descriptor<uint8_t>::format(), 1,
                               {static_cast<py::ssize_t>(b.size())}, {1});
      });

  // A launch's images from the launch bindings' keyword arguments; the vectors
  // hold the tables' host copies for the duration of the call.
  //   dims / dims_ptr: the extents as a list of one (row_bytes, height) pair per
  // FRAME (the host copy) and the device table's address.  active / active_ptr:
  // the table of open images, as a list of frame indices and the device
  // table's address.
  //   batch / batch_stride (the ImageSet of launch_stencil and launch_residual*):
  // the images of the grid and the bytes between frames; the active list holds
  // `batch` indices, and the frames at the stride then number `batch_frames`,
  // without a table `batch`.
  struct ImageSetArgs {
    std::vector<int32_t> active_host;
    std::vector<ImageDims> dims_host;
    // The dims list must hold dims_n pairs (`dims_holds` says so), the active
    // list active_n indices (below 0: any number, for the launches that refuse it).
    void fill(ImageTables& s, int frames, const py::object& dims, uintptr_t dims_ptr, int64_t dims_n,
              const char* dims_holds, const py::object& active, uintptr_t active_ptr, int64_t active_n = -1) {
      s.frames = frames;
      if (!active.is_none()) {
        active_host = active.cast<std::vector<int32_t>>();
        PCONV_CHECK(active_n < 0 || static_cast<int64_t>(active_host.size()) == active_n,
                    "active: the list must hold `batch` frame indices");
        s.active_host = active_host.data();
        s.count = static_cast<int>(active_host.size());
      }
      s.active = reinterpret_cast<const int32_t*>(active_ptr);
      if (!dims.is_none()) {
        for (const auto& d : dims.cast<std::vector<std::pair<int32_t, int32_t>>>())
          dims_host.push_back(ImageDims{d.first, d.second});
        PCONV_CHECK(static_cast<int64_t>(dims_host.size()) == dims_n,
                    std::string("dims: ") + dims_holds + " (row_bytes, height) pairs");
        s.dims_host = dims_host.data();
      }
      s.dims = reinterpret_cast<const ImageDims*>(dims_ptr);
    }
    void fill(ImageSet& s, int batch, int64_t batch_stride, const py::object& dims, uintptr_t dims_ptr,
              const py::object& active = py::none(), uintptr_t active_ptr = 0, int batch_frames = 1) {
      const bool listed = !active.is_none(), table = listed || active_ptr != 0;
      fill(static_cast<ImageTables&>(s), table ? batch_frames : batch, dims, dims_ptr, listed ? batch_frames : batch,
           listed ? "with an active table the list must hold `batch_frames`" : "the list must hold `batch`", active,
           active_ptr, batch);
      s.stride = batch_stride;
      s.count = table ? batch : 0;
    }
  };
  m.def(
      "launch_stencil",
      [](py::object filter, const std::string& ch, uintptr_t src, uintptr_t dst, int64_t pitch, int64_t row_bytes,
         int64_t r0, int64_t r1, int64_t frame_lo, int64_t frame_hi, int steps, int64_t g_row0, int64_t height,
         uintptr_t stream, const std::string& variant, const std::string& border, int batch, int64_t batch_stride,
         py::object dims, uintptr_t dims_ptr, py::object active, uintptr_t active_ptr, int batch_frames, int depth) {
        StencilLaunch a;
        ImageSetArgs images;
        a.border = parse_border(border);
        a.depth = depth;
        images.fill(a.images, batch, batch_stride, dims, dims_ptr, active, active_ptr, batch_frames);
        a.src = reinterpret_cast<const uint8_t*>(src);
        a.dst = reinterpret_cast<uint8_t*>(dst);
        a.pitch = pitch;
        a.row_bytes = row_bytes;
        a.r0 = r0;
        a.r1 = r1;
        a.frame_lo = frame_lo;
        a.frame_hi = frame_hi;
        a.steps = steps;
        a.g_row0 = g_row0;
        a.height = height;
        launch_stencil(make_filter(filter), parse_channels(ch), a, reinterpret_cast<hipStream_t>(stream),
                       parse_variant(variant));
      },
      py::arg("filter"), py::arg("channels"), py::arg("src"), py::arg("dst"), py::arg("pitch"), py::arg("row_bytes"),
      py::arg("r0"), py::arg("r1"), py::arg("frame_lo"), py::arg("frame_hi"), py::arg("steps") = 1,
      py::arg("g_row0") = 0, py::arg("height") = (int64_t(1) << 40), py::arg("stream") = 0,
      py::arg("variant") = "auto", py::arg("border") = "zero", py::arg("batch") = 1, py::arg("batch_stride") = 0,
      py::arg("dims") = py::none(), py::arg("dims_ptr") = 0, py::arg("active") = py::none(),
      py::arg("active_ptr") = 0, py::arg("batch_frames") = 1, py::arg("depth") = 8);
  m.def(
      "launch_residual",
      [](py::object filter, const std::string& ch, uintptr_t src, int64_t pitch, int64_t row_bytes, int64_t r0,
         int64_t r1, int64_t frame_lo, int64_t frame_hi, int64_t g_row0, int64_t height, uintptr_t stream,
         const std::string& border, py::object dims, uintptr_t dims_ptr) {
        StencilLaunch a;
        ImageSetArgs images;
        images.fill(a.images, 1, 0, dims, dims_ptr);
        a.border = parse_border(border);
        a.src = reinterpret_cast<const uint8_t*>(src);
        a.pitch = pitch;
        a.row_bytes = row_bytes;
        a.r0 = r0;
        a.r1 = r1;
        a.frame_lo = frame_lo;
        a.frame_hi = frame_hi;
        a.g_row0 = g_row0;
        a.height = height;
        const Filter f = make_filter(filter);
        const Channels c = parse_channels(ch);
        hipStream_t s = reinterpret_cast<hipStream_t>(stream);
        py::gil_scoped_release nogil;
        DeviceBuffer counter(16);
        PCONV_HIP_CHECK(hipMemsetAsync(counter.data(), 0, 16, s));
        launch_residual(f, c, a, reinterpret_cast<uint64_t*>(counter.data()), s);
        uint64_t n = 0;
        PCONV_HIP_CHECK(hipMemcpyAsync(&n, counter.data(), sizeof(n), hipMemcpyDeviceToHost, s));
        PCONV_HIP_CHECK(hipStreamSynchronize(s));
        return n;
      },
      py::arg("filter"), py::arg("channels"), py::arg("src"), py::arg("pitch"), py::arg("row_bytes"), py::arg("r0"),
      py::arg("r1"), py::arg("frame_lo"), py::arg("frame_hi"), py::arg("g_row0") = 0,
      py::arg("height") = (int64_t(1) << 40), py::arg("stream") = 0, py::arg("border") = "zero",
      py::arg("dims") = py::none(), py::arg("dims_ptr") = 0,
      "Residual kernel on a frame (launch_stencil's geometry arguments): bytes of rows [r0, r1) that one more "
      "repetition would change; synchronises the stream.");
  m.def(
      "launch_residual_batch",
      [](py::object filter, const std::string& ch, uintptr_t src, int64_t pitch, int64_t row_bytes, int64_t r0,
         int64_t r1, int64_t frame_lo, int64_t frame_hi, uintptr_t counters, int batch, int64_t batch_stride,
         int64_t g_row0, int64_t height, uintptr_t stream, const std::string& border, py::object dims,
         uintptr_t dims_ptr, py::object active, uintptr_t active_ptr, int batch_frames) {
        StencilLaunch a;
        ImageSetArgs images;
        a.border = parse_border(border);
        images.fill(a.images, batch, batch_stride, dims, dims_ptr, active, active_ptr, batch_frames);
        a.src = reinterpret_cast<const uint8_t*>(src);
        a.pitch = pitch;
        a.row_bytes = row_bytes;
        a.r0 = r0;
        a.r1 = r1;
        a.frame_lo = frame_lo;
        a.frame_hi = frame_hi;
        a.g_row0 = g_row0;
        a.height = height;
        const Filter f = make_filter(filter);
        const Channels c = parse_channels(ch);
        hipStream_t s = reinterpret_cast<hipStream_t>(stream);
        py::gil_scoped_release nogil;
        launch_residual(f, c, a, reinterpret_cast<uint64_t*>(counters), s);
        PCONV_HIP_CHECK(hipStreamSynchronize(s));
      },
      py::arg("filter"), py::arg("channels"), py::arg("src"), py::arg("pitch"), py::arg("row_bytes"), py::arg("r0"),
      py::arg("r1"), py::arg("frame_lo"), py::arg("frame_hi"), py::arg("counters"), py::arg("batch"),
      py::arg("batch_stride"), py::arg("g_row0") = 0, py::arg("height") = (int64_t(1) << 40), py::arg("stream") = 0,
      py::arg("border") = "zero", py::arg("dims") = py::none(), py::arg("dims_ptr") = 0,
      py::arg("active") = py::none(), py::arg("active_ptr") = 0, py::arg("batch_frames") = 1,
      "Residual kernel on `batch` frames batch_stride bytes apart in one launch: image b's count is ADDED to "
      "counters[b] (a device pointer to at least `batch` uint64 of the caller's, neither zeroed nor read here); "
      "with an active table, on the `batch` frames it names out of `batch_frames`, each adding to its frame's "
      "counter; synchronises the stream.");
  m.attr("RESIDUAL_BLOCK_ROWS") = kResidualBlockRows;
  m.def(
      "launch_decimate",
      [](uintptr_t src, int64_t src_pitch, int64_t row_bytes, int64_t rows, uintptr_t dst, int64_t dst_pitch,
         int64_t dst_bytes, int pixel_bytes, int factor, int64_t g_row0, int frames, int64_t src_stride,
         int64_t dst_stride, uintptr_t stream, py::object dims, uintptr_t dims_ptr, py::object active,
         uintptr_t active_ptr, int timed) {
        DecimateLaunch a;
        a.src = reinterpret_cast<const uint8_t*>(src);
        a.src_pitch = src_pitch;
        a.row_bytes = row_bytes;
        a.rows = rows;
        a.g_row0 = g_row0;
        a.dst = reinterpret_cast<uint8_t*>(dst);
        a.dst_pitch = dst_pitch;
        a.dst_bytes = dst_bytes;
        a.pixel_bytes = pixel_bytes;
        a.factor = factor;
        a.src_stride = src_stride;
        a.dst_stride = dst_stride;
        ImageSetArgs images;
        images.fill(a.images, frames, dims, dims_ptr, frames, "the list must hold `frames`", active, active_ptr);
        hipStream_t s = reinterpret_cast<hipStream_t>(stream);
        py::gil_scoped_release nogil;
        launch_decimate(a, s);
        return time_launches(timed, s, [&] { launch_decimate(a, s); });
      },
      py::arg("src"), py::arg("src_pitch"), py::arg("row_bytes"), py::arg("rows"), py::arg("dst"),
      py::arg("dst_pitch"), py::arg("dst_bytes"), py::arg("pixel_bytes"), py::arg("factor"), py::arg("g_row0") = 0,
      py::arg("frames") = 1, py::arg("src_stride") = 0, py::arg("dst_stride") = 0, py::arg("stream") = 0,
      py::arg("dims") = py::none(), py::arg("dims_ptr") = 0, py::arg("active") = py::none(),
      py::arg("active_ptr") = 0, py::arg("timed") = 0,
      "Decimation kernel on raw pointers: every factor-th pixel of the source frame's rows on a kept global row "
      "into the pitched destination (dst_bytes: the size of what dst points into); `frames` frames at the two "
      "strides in one launch, dims / dims_ptr: their SOURCE extents; an active table is refused; synchronises the "
      "stream.  timed = k: k further launches of the same arguments, returns the ms of each (stream events).");
  m.attr("DECIMATE_BLOCK_ROWS") = kDecimateBlockRows;
  m.def(
      "launch_unsharp",
      [](uintptr_t orig, int64_t orig_pitch, uintptr_t blur, int64_t blur_pitch, uintptr_t dst, int64_t dst_pitch,
         int64_t row_bytes, int64_t rows, int depth, int k, int threshold, int frames, int64_t orig_stride,
         int64_t blur_stride, int64_t dst_stride, uintptr_t stream, py::object dims, uintptr_t dims_ptr,
         py::object active, uintptr_t active_ptr, int timed) {
        UnsharpLaunch a;
        a.orig = reinterpret_cast<const uint8_t*>(orig);
        a.orig_pitch = orig_pitch;
        a.blur = reinterpret_cast<const uint8_t*>(blur);
        a.blur_pitch = blur_pitch;
        a.dst = reinterpret_cast<uint8_t*>(dst);
        a.dst_pitch = dst_pitch;
        a.row_bytes = row_bytes;
        a.rows = rows;
        a.depth = depth;
        a.k = k;
        a.threshold = threshold;
        a.orig_stride = orig_stride;
        a.blur_stride = blur_stride;
        a.dst_stride = dst_stride;
        ImageSetArgs images;
        images.fill(a.images, frames, dims, dims_ptr, frames, "the list must hold `frames`", active, active_ptr);
        hipStream_t s = reinterpret_cast<hipStream_t>(stream);
        py::gil_scoped_release nogil;
        launch_unsharp(a, s);
        return time_launches(timed, s, [&] { launch_unsharp(a, s); });
      },
      py::arg("orig"), py::arg("orig_pitch"), py::arg("blur"), py::arg("blur_pitch"), py::arg("dst"),
      py::arg("dst_pitch"), py::arg("row_bytes"), py::arg("rows"), py::arg("depth") = 8, py::arg("k") = 16,
      py::arg("threshold") = 0, py::arg("frames") = 1, py::arg("orig_stride") = 0, py::arg("blur_stride") = 0,
      py::arg("dst_stride") = 0, py::arg("stream") = 0, py::arg("dims") = py::none(), py::arg("dims_ptr") = 0,
      py::arg("active") = py::none(), py::arg("active_ptr") = 0, py::arg("timed") = 0,
      "Unsharp-mask kernel on raw pointers: dst = x + (k / 16)(x - b) per sample of three pitched frames (dst may "
      "be blur: in place); `frames` frames at the three strides in one launch, dims / dims_ptr: their extents; an "
      "active table is refused; synchronises the stream.  timed = n: n further launches of the same arguments "
      "(out of place only: in place they would sharpen again), returns the ms of each (stream events).");
  m.attr("UNSHARP_BLOCK_ROWS") = kUnsharpBlockRows;
  m.def(
      "time_copy_rows",
      [](uintptr_t src, int64_t sp, uintptr_t dst, int64_t dp, int64_t row_bytes, int64_t rows, int timed) {
        const uint8_t* s = reinterpret_cast<const uint8_t*>(src);
        uint8_t* d = reinterpret_cast<uint8_t*>(dst);
        py::gil_scoped_release nogil;
        launch_copy_rows(s, sp, d, dp, row_bytes, rows, nullptr);
        return time_launches(timed, nullptr, [&] { launch_copy_rows(s, sp, d, dp, row_bytes, rows, nullptr); });
      },
      py::arg("src"), py::arg("src_pitch"), py::arg("dst"), py::arg("dst_pitch"), py::arg("row_bytes"),
      py::arg("rows"), py::arg("timed") = 0,
      "Diagnostics: the row-copy kernel between two pitched device buffers, one launch and `timed` timed ones "
      "(stream events on the default stream); the ms of each.");
  m.def("set_swar_shape", &set_swar_shape, py::arg("lw") = 0, py::arg("m") = 0, py::arg("nw") = 0,
        "Force the SWAR temporal tile shape (lw=0: back to the latency model).");
  m.def("swar_shapes", []() {
    py::list out;
    for (const auto& s : swar_shapes()) out.append(py::make_tuple(s.lw, s.m, s.nw));
    return out;
  });
  m.def("set_swar16_shape", &set_swar16_shape, py::arg("lw") = 0, py::arg("m") = 0, py::arg("nw") = 0,
        "Force the 16-bit temporal kernel's tile (lw samples per lane; lw=0: back to the pick / tuner).");
  m.def("swar16_shapes", []() {
    py::list out;
    for (const auto& s : swar16_shapes()) out.append(py::make_tuple(s.lw, s.m, s.nw));
    return out;
  });
  m.def("swar16_tuned", []() {
    py::list out;
    for (const auto& kv : swar16_tuned())
      out.append(py::make_tuple(py::cast(kv.first), py::make_tuple(kv.second.lw, kv.second.m, kv.second.nw)));
    return out;
  });
  m.def(
      "swar_model",
      [](int steps, const std::string& ch, int64_t rows, int64_t row_bytes, int batch) {
        PCONV_CHECK(batch >= 1, "swar_model: batch must be >= 1");
        const SwarShape s = pick_swar_shape(steps, channel_count(parse_channels(ch)), rows, row_bytes, batch);
        return py::make_tuple(py::make_tuple(s.lw, s.m, s.nw),
                              swar_launch_cycles(s, steps, channel_count(parse_channels(ch)), rows, row_bytes, batch));
      },
      py::arg("steps"), py::arg("channels"), py::arg("rows"), py::arg("row_bytes"), py::arg("batch") = 1);
  m.def("set_autotune", &set_shape_tuning, py::arg("on"),
        "Time the model's best tile shapes on first use of a launch geometry (default on); returns the previous "
        "setting.");
  m.def("clear_swar_tuning", &clear_swar_tuning);
  m.def("swar_tuned", []() {
    py::list out;
    for (const auto& kv : swar_tuned())
      out.append(py::make_tuple(py::cast(kv.first), py::make_tuple(kv.second.lw, kv.second.m, kv.second.nw)));
    return out;
  });
  m.def("set_prefetch_mode", &set_prefetch_mode, py::arg("mode"),
        "Buffer-op tile kernel: -1 tuned against the others (default), 0 never, 1 forced (with a set_swar_shape "
        "shape it instantiates, that shape)");
  m.def("set_tune_candidates", &set_tune_candidates, py::arg("n"),
        "How many of the latency model's best SWAR tile shapes the tuner times (default 6).");
  m.def("set_float_shape", &set_float_shape, py::arg("m") = 0, py::arg("nw") = 0,
        "Force the float temporal kernel's tile (m rows per wave, nw waves; m=0: model / tuner).");
  m.def("float_shapes", []() {
    py::list out;
    for (const auto& s : float_shapes()) out.append(py::make_tuple(s.m, s.nw));
    return out;
  });
  m.def("float_tuned", []() {
    py::list out;
    for (const auto& kv : float_tuned())
      out.append(py::make_tuple(py::cast(kv.first), py::make_tuple(kv.second.m, kv.second.nw)));
    return out;
  });
  m.def("swar_prefetch_shapes", []() {
    py::list out;
    for (const auto& s : swar_prefetch_shapes()) out.append(py::make_tuple(s.lw, s.m, s.nw));
    return out;
  });
  m.def("last_swar_launch", []() {
    const SwarLaunchInfo l = last_swar_launch();
    return py::make_tuple(l.kern, l.shape.lw, l.shape.m, l.shape.nw, l.form);
  }, "(kern, lw, m, nw, form) of the most recent launch issued to k_swar (kern 0) or k_swar_pf (kern 1); "
     "kern -1 before the first.");
  m.def("last_float_launch", []() {
    const FloatShape s = last_float_launch();
    return py::make_tuple(s.m, s.nw);
  }, "(m, nw) of the most recent launch issued to k_float_temporal; (0, 0) before the first.");
  m.def("set_swar_alt", &set_swar_alt, py::arg("mode"),
        "SWAR step form: -1 tuned (default), 0 truncate every step, 1 pairs of steps with a x16 intermediate.");
  m.def("set_xcd_swizzle", &set_xcd_swizzle, py::arg("on"),
        "XCD-aware (bijective, per-XCD contiguous) tile order of the SWAR kernel.");
  m.def(
      "swar_model_table",
      [](int steps, const std::string& ch, int64_t rows, int64_t row_bytes, int batch) {
        // every shape: (lw, m, nw, vgpr, lds, measured, predicted cycles)
        PCONV_CHECK(batch >= 1, "swar_model_table: batch must be >= 1");
        const int c = channel_count(parse_channels(ch));
        py::list out;
        for (const auto& s : swar_shapes()) {
          const SwarResources r = swar_resources(s, c);
          out.append(py::make_tuple(s.lw, s.m, s.nw, r.vgpr, r.lds, r.measured,
                                    swar_launch_cycles(s, steps, c, rows, row_bytes, batch)));
        }
        return out;
      },
      py::arg("steps"), py::arg("channels"), py::arg("rows"), py::arg("row_bytes"), py::arg("batch") = 1);
  m.def("auto_fuse",
        [](py::object filter, const std::string& v, int64_t frame_bytes, int channels, int depth) {
          return auto_fuse(make_filter(filter), parse_variant(v), frame_bytes, channels, depth);
        },
        py::arg("filter"), py::arg("variant"), py::arg("frame_bytes"), py::arg("channels") = 0, py::arg("depth") = 8,
        "Default repetitions per launch for a band frame of `frame_bytes` with `channels` bytes per pixel");
  m.def("supports_fusion",
        [](py::object filter, const std::string& v) { return supports_fusion(make_filter(filter), parse_variant(v)); },
        py::arg("filter"), py::arg("variant") = "auto");

  // ---------------------------------------------------------------- engine
  py::class_<RunStats>(m, "RunStats")
      .def_readonly("loop_ms", &RunStats::loop_ms)
      .def_readonly("wall_ms", &RunStats::wall_ms)
      .def_readonly("launches", &RunStats::launches)
      .def_readonly("exchanges", &RunStats::exchanges)
      .def_readonly("image_launches", &RunStats::image_launches);

  py::class_<HaloTransport, PyHaloTransport, std::shared_ptr<HaloTransport>>(m, "HaloTransport")
      .def(py::init<>())
      .def_property_readonly("name", &HaloTransport::name);

  m.def(
      "memcpy_async",
      [](uintptr_t dst, uintptr_t src, int64_t nbytes, const std::string& kind, uintptr_t stream) {
        hipMemcpyKind k = kind == "h2d" ? hipMemcpyHostToDevice
                          : kind == "d2h" ? hipMemcpyDeviceToHost
                          : kind == "d2d" ? hipMemcpyDeviceToDevice
                                          : hipMemcpyDefault;
        PCONV_HIP_CHECK(hipMemcpyAsync(reinterpret_cast<void*>(dst), reinterpret_cast<const void*>(src),
                                       static_cast<size_t>(nbytes), k, reinterpret_cast<hipStream_t>(stream)));
      },
      py::arg("dst"), py::arg("src"), py::arg("nbytes"), py::arg("kind"), py::arg("stream") = 0);
  m.def(
      "stream_synchronize",
      [](uintptr_t stream) { PCONV_HIP_CHECK(hipStreamSynchronize(reinterpret_cast<hipStream_t>(stream))); },
      py::arg("stream"), py::call_guard<py::gil_scoped_release>());

  py::class_<BandEngine>(m, "BandEngine")
      .def(py::init([](int64_t w, int64_t h, const std::string& ch, py::object filter, int rank, int world,
                       int device, int halo, int fuse, bool overlap, bool graph, const std::string& variant,
                       bool kernel_copies, int stream_chunks, const std::string& border, int depth) {
             EngineOptions o;
             o.border = parse_border(border);
             o.stream_chunks = stream_chunks;
             o.kernel_copies = kernel_copies;
             o.device = device;
             o.halo_depth = halo;
             o.fuse = fuse;
             o.overlap = overlap;
             o.use_graph = graph;
             o.variant = parse_variant(variant);
             const ImageGeom g = make_geom(w, h, ch, depth);
             return std::make_unique<BandEngine>(g, row_band(h, world, rank), make_filter(filter), o);
           }),
           py::arg("width"), py::arg("height"), py::arg("channels"), py::arg("filter") = "gaussian",
           py::arg("rank") = 0, py::arg("world") = 1, py::arg("device") = 0, py::arg("halo") = 1, py::arg("fuse") = 1,
           py::arg("overlap") = true, py::arg("graph") = false, py::arg("variant") = "auto",
           py::arg("kernel_copies") = false, py::arg("stream_chunks") = 0, py::arg("border") = "zero",
           py::arg("depth") = 8)
      .def_property_readonly("depth", [](const BandEngine& e) { return e.geom().depth; })
      .def_property_readonly("border", [](const BandEngine& e) { return std::string(border_name(e.options().border)); })
      .def_property_readonly("band", &BandEngine::band)
      .def("stream_plan", &BandEngine::stream_plan, py::arg("reps"), py::arg("in_r0"), py::arg("in_r1"))
      .def_property_readonly("halo", [](const BandEngine& e) { return e.layout().halo; })
      .def_property_readonly("fuse", [](const BandEngine& e) { return e.options().fuse; })
      .def_property_readonly("cached_graphs", &BandEngine::cached_graphs)
      .def_property_readonly("cached_step_graphs", &BandEngine::cached_step_graphs)
      .def_property_readonly_static("max_cached_graphs", [](py::object) { return BandEngine::kMaxCachedGraphs; })
      .def_property_readonly("pitch", [](const BandEngine& e) { return e.layout().pitch; })
      .def_property_readonly("row_bytes", [](const BandEngine& e) { return e.layout().row_bytes; })
      .def_property_readonly("compute_stream",
                             [](const BandEngine& e) { return reinterpret_cast<uintptr_t>(e.compute_stream()); })
      .def_property_readonly("comm_stream",
                             [](const BandEngine& e) { return reinterpret_cast<uintptr_t>(e.comm_stream()); })
      .def_property_readonly("src_ptr", [](const BandEngine& e) { return reinterpret_cast<uintptr_t>(e.src_frame()); })
      .def("plan", &BandEngine::plan, py::arg("reps"))
      .def(
          "upload",
          [](BandEngine& e, py::buffer host, int64_t r_begin, int64_t r_end) {
            const HostView v = host_view(host, false);
            PCONV_CHECK(v.size >= (r_end - r_begin) * e.layout().row_bytes, "host buffer too small");
            e.upload_rows(v.ptr, e.layout().row_bytes, r_begin, r_end);
          },
          py::arg("host"), py::arg("r_begin"), py::arg("r_end"))
      .def(
          "upload_ptr",
          [](BandEngine& e, uintptr_t ptr, int64_t pitch, int64_t r_begin, int64_t r_end, bool device) {
            if (device)
              e.upload_rows_device(reinterpret_cast<const uint8_t*>(ptr), pitch, r_begin, r_end);
            else
              e.upload_rows(reinterpret_cast<const uint8_t*>(ptr), pitch, r_begin, r_end);
          },
          py::arg("ptr"), py::arg("pitch"), py::arg("r_begin"), py::arg("r_end"), py::arg("device") = false)
      .def(
          "download",
          [](BandEngine& e, py::buffer host, int64_t r_begin, int64_t r_end) {
            const HostView v = host_view(host, true);
            PCONV_CHECK(v.size >= (r_end - r_begin) * e.layout().row_bytes, "host buffer too small");
            e.download_rows(v.ptr, e.layout().row_bytes, r_begin, r_end);
          },
          py::arg("host"), py::arg("r_begin"), py::arg("r_end"))
      .def(
          "download_ptr",
          [](BandEngine& e, uintptr_t ptr, int64_t pitch, int64_t r_begin, int64_t r_end, bool device) {
            if (device)
              e.download_rows_device(reinterpret_cast<uint8_t*>(ptr), pitch, r_begin, r_end);
            else
              e.download_rows(reinterpret_cast<uint8_t*>(ptr), pitch, r_begin, r_end);
          },
          py::arg("ptr"), py::arg("pitch"), py::arg("r_begin"), py::arg("r_end"), py::arg("device") = false)
      .def(
          "download_decimated",
          [](BandEngine& e, py::buffer host, int factor) {
            const HostView v = host_view(host, true);
            PCONV_CHECK(v.size >= e.decimated_rows(factor) * e.decimated_row_bytes(factor), "host buffer too small");
            e.download_rows_decimated(v.ptr, e.decimated_row_bytes(factor), factor);
          },
          py::arg("host"), py::arg("factor"),
          "every factor-th pixel of the owned rows on a kept global row of the newest frame, tight rows: one "
          "decimation launch into device staging and one D2H of the decimated bytes")
      .def(
          "download_decimated_ptr",
          [](BandEngine& e, uintptr_t ptr, int64_t pitch, int factor, bool device) {
            if (device)
              e.download_rows_decimated_device(reinterpret_cast<uint8_t*>(ptr), pitch, factor);
            else
              e.download_rows_decimated(reinterpret_cast<uint8_t*>(ptr), pitch, factor);
          },
          py::arg("ptr"), py::arg("pitch"), py::arg("factor"), py::arg("device") = false)
      .def("decimated_rows", &BandEngine::decimated_rows, py::arg("factor"))
      .def("decimated_row_bytes", &BandEngine::decimated_row_bytes, py::arg("factor"))
      .def("upload_decimated_from", &BandEngine::upload_decimated_from, py::arg("src"), py::arg("factor"),
           "src's newest frame, decimated, becomes this engine's current frame (device to device, one launch)")
      .def("snapshot_original", &BandEngine::snapshot_original,
           "copy the current frame's owned rows into the engine's third device buffer (after the upload, before run)")
      .def("apply_unsharp", &BandEngine::apply_unsharp, py::arg("k"), py::arg("threshold") = 0,
           "newest frame = x + (k / 16)(x - newest frame), x the snapshot: one launch, in place")
      .def("set_halo_valid", &BandEngine::set_halo_valid)
      .def("wait_stream", [](BandEngine& e, uintptr_t s) { e.wait_stream(reinterpret_cast<hipStream_t>(s)); })
      .def("signal_stream", [](BandEngine& e, uintptr_t s) { e.signal_stream(reinterpret_cast<hipStream_t>(s)); })
      .def("run", &BandEngine::run, py::arg("reps"), py::call_guard<py::gil_scoped_release>())
      .def("synchronize", &BandEngine::synchronize, py::call_guard<py::gil_scoped_release>())
      .def("residual", &BandEngine::residual, py::call_guard<py::gil_scoped_release>(),
           "bytes of this band's owned rows that one more repetition would change (collective over the bands)")
      .def(
          "run_until_stable",
          [](BandEngine& e, int max_reps, int check_every, py::object reduce) {
            std::function<uint64_t(uint64_t)> red;
            if (!reduce.is_none())
              red = [reduce](uint64_t local) {
                py::gil_scoped_acquire gil;
                return reduce(local).cast<uint64_t>();
              };
            StableStats st;
            {
              py::gil_scoped_release nogil;
              st = e.run_until_stable(max_reps, check_every, red);
            }
            return py::make_tuple(st.reps_done, st.converged, st.residual, st.checks);
          },
          py::arg("max_reps"), py::arg("check_every"), py::arg("reduce") = py::none(),
          "(reps_done, converged, residual, checks); reduce(local count) -> sum over the ranks for a band with "
          "neighbours")
      .def("time_residual", &BandEngine::time_residual, py::arg("launches"), py::call_guard<py::gil_scoped_release>(),
           "diagnostics: ms of each of `launches` residual launches on the current frame (stream events)")
      .def("clear", &BandEngine::clear)
      .def_property_readonly("stats", &BandEngine::last_stats)
      .def(
          "process",
          [](BandEngine& e, uintptr_t in_ptr, int64_t in_r0, int64_t in_r1, uintptr_t out_ptr, int reps) {
            // Serving step: H2D (rows [in_r0, in_r1), ghost rows allowed), reps, D2H of
            // the owned rows; host pointers pinned.  Releases the GIL throughout.
            py::gil_scoped_release nogil;
            const int64_t rb = e.layout().row_bytes;
            e.upload_rows(reinterpret_cast<const uint8_t*>(in_ptr), rb, in_r0, in_r1);
            e.set_halo_valid(in_r0 < 0 || in_r1 > e.band().rows);
            e.run(reps);
            e.download_rows(reinterpret_cast<uint8_t*>(out_ptr), rb, 0, e.band().rows);
            e.synchronize();
          },
          py::arg("in_ptr"), py::arg("in_r0"), py::arg("in_r1"), py::arg("out_ptr"), py::arg("reps"))
      .def(
          "process_graph",
          [](BandEngine& e, uintptr_t in_ptr, int64_t in_r0, int64_t in_r1, uintptr_t out_ptr, int reps) {
            py::gil_scoped_release nogil;
            e.process_graph(reinterpret_cast<const uint8_t*>(in_ptr), in_r0, in_r1, reinterpret_cast<uint8_t*>(out_ptr),
                            reps);
          },
          py::arg("in_ptr"), py::arg("in_r0"), py::arg("in_r1"), py::arg("out_ptr"), py::arg("reps"))
      .def("exchange_free", &BandEngine::exchange_free, py::arg("reps"), py::arg("halo_preloaded"))
      .def("input_preloaded", &BandEngine::input_preloaded, py::arg("in_r0"), py::arg("in_r1"))
      .def(
          "exchange_now",
          [](BandEngine& e, uintptr_t stream) { e.exchange_now(reinterpret_cast<hipStream_t>(stream)); },
          py::arg("stream") = 0, "Fill the whole ghost zone now (transport on `stream`, 0 = the comm stream)")
      .def(
          "read_frame",
          [](BandEngine& e, py::buffer host, int64_t r_begin, int64_t r_end) {
            const HostView v = host_view(host, true);
            PCONV_CHECK(v.size >= (r_end - r_begin) * e.layout().row_bytes, "host buffer too small");
            py::gil_scoped_release nogil;
            e.read_frame_rows(v.ptr, r_begin, r_end);
          },
          py::arg("host"), py::arg("r_begin"), py::arg("r_end"),
          "Copy source-frame rows [r_begin, r_end), ghost rows included (tests / debugging)")
      .def_static(
          "for_band",
          [](int64_t w, int64_t h, const std::string& ch, py::object filter, const Band& band, int device, int halo,
             int fuse, bool overlap, const std::string& variant, bool graph, bool capture_exchanges,
             const std::string& border, int depth) {
            // An explicit band (tests: e.g. a single rank whose up/down
            // neighbour is itself, to drive RCCL send/recv-to-self).
            EngineOptions o;
            o.border = parse_border(border);
            o.device = device;
            o.halo_depth = halo;
            o.fuse = fuse;
            o.overlap = overlap;
            o.variant = parse_variant(variant);
            o.use_graph = graph;
            o.capture_exchanges = capture_exchanges;
            return std::make_unique<BandEngine>(make_geom(w, h, ch, depth), band, make_filter(filter), o);
          },
          py::arg("width"), py::arg("height"), py::arg("channels"), py::arg("filter"), py::arg("band"),
          py::arg("device") = 0, py::arg("halo") = 1, py::arg("fuse") = 1, py::arg("overlap") = true,
          py::arg("variant") = "auto", py::arg("graph") = false, py::arg("capture_exchanges") = false,
          py::arg("border") = "zero", py::arg("depth") = 8)
      .def("set_stream_trace", &BandEngine::set_stream_trace, py::arg("on"),
           "diagnostics: time the next streamed images chunk by chunk (stream_trace())")
      .def("stream_trace", &BandEngine::stream_trace, py::call_guard<py::gil_scoped_release>(),
           "latest streamed image: [chunk, upload end, launches end, download end] ms from its start")
      .def("attach_rccl",
           [](BandEngine& e, std::shared_ptr<RcclComm> c) {
             e.set_transport(std::make_shared<RcclTransport>(std::move(c)));
           })
      .def("attach_transport", [](BandEngine& e, std::shared_ptr<HaloTransport> t) { e.set_transport(std::move(t)); },
           py::keep_alive<1, 2>())
      .def("attach_null_transport",
           [](BandEngine& e) { e.set_transport(std::make_shared<NullTransport>()); });

  // Up to `capacity` whole images of one geometry, one fused launch per
  // `fuse` repetitions for all of them (batch_engine.hpp).
  static const auto to_sizes = [](const std::vector<std::pair<int64_t, int64_t>>& sizes) {
    std::vector<ImageSize> out;
    for (const auto& z : sizes) out.push_back(ImageSize{z.first, z.second});
    return out;
  };
  py::class_<BatchEngine>(m, "BatchEngine")
      .def(py::init([](int64_t w, int64_t h, const std::string& ch, int capacity, py::object filter, int device,
                       int fuse, const std::string& variant, const std::string& border, int depth) {
             EngineOptions o;
             o.border = parse_border(border);
             o.device = device;
             o.fuse = fuse;
             o.variant = parse_variant(variant);
             return std::make_unique<BatchEngine>(make_geom(w, h, ch, depth), make_filter(filter), capacity, o);
           }),
           py::arg("width"), py::arg("height"), py::arg("channels"), py::arg("capacity"),
           py::arg("filter") = "gaussian", py::arg("device") = 0, py::arg("fuse") = 1, py::arg("variant") = "auto",
           py::arg("border") = "zero", py::arg("depth") = 8)
      .def_property_readonly("depth", [](const BatchEngine& e) { return e.geom().depth; })
      .def_property_readonly("capacity", &BatchEngine::capacity)
      .def_property_readonly("border", [](const BatchEngine& e) { return std::string(border_name(e.options().border)); })
      .def_property_readonly("fuse", [](const BatchEngine& e) { return e.options().fuse; })
      .def_property_readonly("halo", [](const BatchEngine& e) { return e.layout().halo; })
      .def_property_readonly("pitch", [](const BatchEngine& e) { return e.layout().pitch; })
      .def_property_readonly("row_bytes", [](const BatchEngine& e) { return e.layout().row_bytes; })
      .def_property_readonly("batch_stride", &BatchEngine::batch_stride)
      .def_property_readonly("compute_stream",
                             [](const BatchEngine& e) { return reinterpret_cast<uintptr_t>(e.compute_stream()); })
      .def(
          "upload",
          [](BatchEngine& e, py::buffer host, int n) {
            const HostView v = host_view(host, false);
            PCONV_CHECK(n >= 0 && v.size >= n * e.geom().bytes(), "host buffer too small");
            e.upload(v.ptr, n);
          },
          py::arg("host"), py::arg("n"))
      .def(
          "upload_ptr",
          [](BatchEngine& e, uintptr_t ptr, int n, bool device) {
            e.upload(reinterpret_cast<const uint8_t*>(ptr), n, device);
          },
          py::arg("ptr"), py::arg("n"), py::arg("device") = false)
      .def(
          "download",
          [](BatchEngine& e, py::buffer host, int n) {
            const HostView v = host_view(host, true);
            PCONV_CHECK(n >= 0 && v.size >= n * e.geom().bytes(), "host buffer too small");
            e.download(v.ptr, n);
          },
          py::arg("host"), py::arg("n"))
      .def(
          "download_ptr",
          [](BatchEngine& e, uintptr_t ptr, int n, bool device) { e.download(reinterpret_cast<uint8_t*>(ptr), n, device); },
          py::arg("ptr"), py::arg("n"), py::arg("device") = false)
      .def(
          "upload_sized",
          [](BatchEngine& e, py::buffer host, const std::vector<std::pair<int64_t, int64_t>>& sizes) {
            const HostView v = host_view(host, false);
            const std::vector<ImageSize> sz = to_sizes(sizes);
            (void)image_dims_table(e.geom(), e.capacity(), sz);  // the sizes are checked before the buffer's
            PCONV_CHECK(v.size >= packed_bytes(e.geom(), sz), "host buffer too small");
            e.upload_sized(v.ptr, sz);
          },
          py::arg("host"), py::arg("sizes"),
          "mixed sizes: `host` holds the images of `sizes` [(width, height)] back to back with tight rows, each "
          "within the engine's width x height (the envelope); lasts until the next plain upload")
      .def(
          "upload_sized_ptr",
          [](BatchEngine& e, uintptr_t ptr, const std::vector<std::pair<int64_t, int64_t>>& sizes, bool device) {
            e.upload_sized(reinterpret_cast<const uint8_t*>(ptr), to_sizes(sizes), device);
          },
          py::arg("ptr"), py::arg("sizes"), py::arg("device") = false)
      .def(
          "download_sized",
          [](BatchEngine& e, py::buffer host) {
            const HostView v = host_view(host, true);
            PCONV_CHECK(v.size >= packed_bytes(e.geom(), e.sizes()), "host buffer too small");
            e.download_sized(v.ptr);
          },
          py::arg("host"))
      .def(
          "download_sized_ptr",
          [](BatchEngine& e, uintptr_t ptr, bool device) { e.download_sized(reinterpret_cast<uint8_t*>(ptr), device); },
          py::arg("ptr"), py::arg("device") = false)
      .def(
          "download_decimated",
          [](BatchEngine& e, py::buffer host, int n, int factor) {
            const HostView v = host_view(host, true);
            PCONV_CHECK(n >= 0 && v.size >= n * decimated_geom(e.geom(), factor).bytes(), "host buffer too small");
            e.download_decimated(v.ptr, n, factor);
          },
          py::arg("host"), py::arg("n"), py::arg("factor"),
          "images [0, n) decimated by `factor` in ONE launch, packed back to back with tight rows")
      .def(
          "download_decimated_ptr",
          [](BatchEngine& e, uintptr_t ptr, int n, int factor, bool device) {
            e.download_decimated(reinterpret_cast<uint8_t*>(ptr), n, factor, device);
          },
          py::arg("ptr"), py::arg("n"), py::arg("factor"), py::arg("device") = false)
      .def(
          "download_sized_decimated",
          [](BatchEngine& e, py::buffer host, int factor) {
            const HostView v = host_view(host, true);
            check_decimate(factor);
            PCONV_CHECK(v.size >= decimated_packed_bytes(e.geom(), e.sizes(), factor), "host buffer too small");
            e.download_sized_decimated(v.ptr, factor);
          },
          py::arg("host"), py::arg("factor"),
          "the current mixed-size upload's images, each decimated by `factor` (ONE launch), packed back to back")
      .def(
          "download_sized_decimated_ptr",
          [](BatchEngine& e, uintptr_t ptr, int factor, bool device) {
            e.download_sized_decimated(reinterpret_cast<uint8_t*>(ptr), factor, device);
          },
          py::arg("ptr"), py::arg("factor"), py::arg("device") = false)
      .def_property_readonly("sizes",
                             [](const BatchEngine& e) {
                               std::vector<std::pair<int64_t, int64_t>> out;
                               for (const auto& z : e.sizes()) out.emplace_back(z.width, z.height);
                               return out;
                             })
      .def("snapshot_original", &BatchEngine::snapshot_original, py::arg("n"),
           "copy the current frames' rows of images [0, n) into the engine's third allocation (ONE launch)")
      .def("apply_unsharp", &BatchEngine::apply_unsharp, py::arg("k"), py::arg("threshold"), py::arg("n"),
           "newest frames of images [0, n) = x + (k / 16)(x - newest), x the snapshot: ONE launch, in place")
      .def("wait_stream", [](BatchEngine& e, uintptr_t s) { e.wait_stream(reinterpret_cast<hipStream_t>(s)); })
      .def("signal_stream", [](BatchEngine& e, uintptr_t s) { e.signal_stream(reinterpret_cast<hipStream_t>(s)); })
      .def("run", &BatchEngine::run, py::arg("reps"), py::arg("n"), py::call_guard<py::gil_scoped_release>())
      .def("synchronize", &BatchEngine::synchronize, py::call_guard<py::gil_scoped_release>())
      .def("residual", &BatchEngine::residual, py::arg("n"), py::call_guard<py::gil_scoped_release>(),
           "per-image bytes of the newest frames of images [0, n) that one more repetition would change (one launch)")
      .def(
          "run_until_stable",
          [](BatchEngine& e, int max_reps, int check_every, int n, bool compact) {
            std::vector<StableStats> st;
            {
              py::gil_scoped_release nogil;
              st = e.run_until_stable(max_reps, check_every, n, compact);
            }
            py::list out;
            for (const auto& s : st) out.append(py::make_tuple(s.reps_done, s.converged, s.residual, s.checks));
            return out;
          },
          py::arg("max_reps"), py::arg("check_every"), py::arg("n"), py::arg("compact") = false,
          "[(reps_done, converged, residual, checks)] of images [0, n), each as a single-image run would report it; "
          "compact: converged images are retired from the launches that follow (same results, fewer image_launches)")
      .def("time_residual", &BatchEngine::time_residual, py::arg("launches"), py::arg("n"),
           py::call_guard<py::gil_scoped_release>(),
           "diagnostics: ms of each of `launches` residual launches over images [0, n) (stream events)")
      .def_property_readonly("stats", &BatchEngine::last_stats);

  py::class_<BandPipeline>(m, "BandPipeline")
      .def(py::init([](int64_t w, int64_t h, const std::string& ch, py::object filter, int rank, int world,
                       int device, int halo, int fuse, bool overlap, const std::string& variant, int slots,
                       int concurrent, bool graphs, bool step_graphs, py::object band, bool slot_comm,
                       int stream_chunks, bool cu_mask_queues, bool head_on_slot_streams,
                       int64_t stream_min_bytes, bool head_alt_uploads, std::vector<int> stream_weights,
                       bool lazy_head, const std::string& border) {
             EngineOptions o;
             o.border = parse_border(border);
             o.lazy_head = lazy_head;
             o.head_alt_uploads = head_alt_uploads;
             o.stream_chunks = stream_chunks;
             PCONV_CHECK(stream_weights.empty() || static_cast<int>(stream_weights.size()) == stream_chunks,
                         "stream_weights: one weight per chunk (stream_chunks of them)");
             o.stream_weights = std::move(stream_weights);
             o.stream_min_bytes = stream_min_bytes;
             o.cu_mask_queues = cu_mask_queues;
             o.head_on_slot_streams = head_on_slot_streams;
             o.device = device;
             o.halo_depth = halo;
             o.fuse = fuse;
             o.overlap = overlap;
             o.variant = parse_variant(variant);
             const ImageGeom g = make_geom(w, h, ch);
             // band: an explicit Band (tests: a self-neighbour band on a 1-rank communicator)
             const Band b = band.is_none() ? row_band(h, world, rank) : band.cast<Band>();
             return std::make_unique<BandPipeline>(g, b, make_filter(filter), o, slots, concurrent, graphs,
                                                   step_graphs, slot_comm);
           }),
           py::arg("width"), py::arg("height"), py::arg("channels"), py::arg("filter") = "gaussian",
           py::arg("rank") = 0, py::arg("world") = 1, py::arg("device") = 0, py::arg("halo") = 1, py::arg("fuse") = 1,
           py::arg("overlap") = true, py::arg("variant") = "auto", py::arg("slots") = 2, py::arg("concurrent") = -1,
           py::arg("graphs") = false, py::arg("step_graphs") = true,
           py::arg("band") = py::none(), py::arg("slot_comm") = false, py::arg("stream_chunks") = 0,
           py::arg("cu_mask_queues") = true, py::arg("head_on_slot_streams") = true,
           py::arg("stream_min_bytes") = EngineOptions{}.stream_min_bytes, py::arg("head_alt_uploads") = true,
           py::arg("stream_weights") = std::vector<int>{}, py::arg("lazy_head") = EngineOptions{}.lazy_head,
           py::arg("border") = "zero")
      .def_property_readonly("slots", &BandPipeline::slots)
      .def("slot", &BandPipeline::slot, py::return_value_policy::reference_internal)
      .def("attach_rccl",
           [](BandPipeline& p, std::shared_ptr<RcclComm> c) {
             p.set_transport(std::make_shared<RcclTransport>(std::move(c)));
           })
      .def("attach_transport", [](BandPipeline& p, std::shared_ptr<HaloTransport> t) { p.set_transport(std::move(t)); },
           py::keep_alive<1, 2>())
      .def("attach_slot_rccl",
           [](BandPipeline& p, int k, std::shared_ptr<RcclComm> c) {
             p.set_slot_transport(k, std::make_shared<RcclTransport>(std::move(c)));
           })
      .def("attach_slot_transport",
           [](BandPipeline& p, int k, std::shared_ptr<HaloTransport> t) { p.set_slot_transport(k, std::move(t)); },
           py::keep_alive<1, 3>())
      .def(
          "submit",
          [](BandPipeline& p, uintptr_t in_ptr, int64_t in_r0, int64_t in_r1, uintptr_t out_ptr, int reps) {
            py::gil_scoped_release nogil;
            p.submit(reinterpret_cast<const uint8_t*>(in_ptr), in_r0, in_r1, reinterpret_cast<uint8_t*>(out_ptr), reps);
          },
          py::arg("in_ptr"), py::arg("in_r0"), py::arg("in_r1"), py::arg("out_ptr"), py::arg("reps"))
      .def("drain", &BandPipeline::drain, py::call_guard<py::gil_scoped_release>())
      .def("ready", &BandPipeline::ready, py::arg("slot"), "slot-stream mode: the slot's latest image is done")
      .def("wait_image", &BandPipeline::wait_image, py::arg("slot"), py::call_guard<py::gil_scoped_release>(),
           "slot-stream mode: block until the slot's latest image is done")
      .def("enable_marks", &BandPipeline::enable_marks, py::arg("images"),
           "Completion marks of the next `images` submits (a diagnostic pass; see marks()).")
      .def("marks", &BandPipeline::marks, py::call_guard<py::gil_scoped_release>(),
           "Drain, then per marked image [slot, ms from the first image's issue to its completion, head-streamed].")
      .def_property_readonly("submitted", &BandPipeline::submitted)
      .def_property_readonly("concurrent", &BandPipeline::concurrent)
      .def_property_readonly("graphs", &BandPipeline::graphs)
      .def_property_readonly("streamed_heads", &BandPipeline::streamed_heads)
      .def_property_readonly("step_graphs", &BandPipeline::step_graphs)
      .def_property_readonly("options",
                             [](BandPipeline& p) {
                               const EngineOptions& o = p.slot(0).options();
                               py::dict d;
                               d["stream_chunks"] = o.stream_chunks;
                               d["stream_weights"] = o.stream_weights;
                               d["lazy_head"] = o.lazy_head;
                               d["stream_min_bytes"] = o.stream_min_bytes;
                               d["head_alt_uploads"] = o.head_alt_uploads;
                               d["cu_mask_queues"] = o.cu_mask_queues;
                               d["head_on_slot_streams"] = o.head_on_slot_streams;
                               return d;
                             })
      .def("enable_trace", &BandPipeline::enable_trace, py::arg("images"),
           "Time the stages of the next `images` submits (directly issued pipelines only)")
      .def("trace", &BandPipeline::trace, py::call_guard<py::gil_scoped_release>(),
           "Per traced image: [slot, H2D start, H2D end, reps end, D2H end] in ms");

  py::class_<LocalCluster>(m, "LocalCluster")
      .def(py::init([](int64_t w, int64_t h, const std::string& ch, py::object filter, int bands, int device, int halo,
                       int fuse, const std::string& variant, bool overlap, const std::string& border) {
             EngineOptions o;
             o.border = parse_border(border);
             o.device = device;
             o.halo_depth = halo;
             o.fuse = fuse;
             o.overlap = overlap;
             o.variant = parse_variant(variant);
             return std::make_unique<LocalCluster>(make_geom(w, h, ch), bands, make_filter(filter), o);
           }),
           py::arg("width"), py::arg("height"), py::arg("channels"), py::arg("filter") = "gaussian",
           py::arg("bands") = 2, py::arg("device") = 0, py::arg("halo") = 1, py::arg("fuse") = 1,
           py::arg("variant") = "auto", py::arg("overlap") = true, py::arg("border") = "zero")
      .def("upload",
           [](LocalCluster& c, py::buffer host, bool preload_halo) {
             c.upload(host_view(host, false).ptr, preload_halo);
           },
           py::arg("host"), py::arg("preload_halo") = false)
      .def("run", &LocalCluster::run, py::arg("reps"), py::arg("device_async") = false,
           py::call_guard<py::gil_scoped_release>(),
           "device_async: every band through the production phase path (comm stream || interior, event-ordered)")
      .def("download", [](LocalCluster& c, py::buffer host) { c.download(host_view(host, true).ptr); })
      .def("exchanges", [](LocalCluster& c) { return c.engine(0).last_stats().exchanges; })
      .def_property_readonly("size", &LocalCluster::size);

  // ---------------------------------------------------------------- HIP IPC halos
  m.def("ipc_create_segment", &ipc_create_segment, py::arg("name"), py::arg("world"), py::arg("slots"),
        "create the zeroed shared flag segment of an IPC halo job (one rank)");
  m.def("ipc_pull_probe", &ipc_pull_probe, py::arg("form"), py::arg("bytes"), py::arg("host_source"),
        py::arg("iters") = 50, py::arg("device") = 0, py::arg("workgroups") = 0,
        py::call_guard<py::gil_scoped_release>(),
        "ms per IPC exchange of one pull form (grid|single|sdma), `bytes` per side from a pinned host buffer "
        "(host_source: stand-in for a peer GPU behind xGMI) or this GPU's HBM; self-neighbour flag protocol");
  m.def("ipc_grid_workgroups", &ipc_grid_workgroups, py::arg("bytes"));
  m.def("ipc_unlink_segment", &ipc_unlink_segment, py::arg("name"),
        "remove the segment's name (mappings stay valid; call once every rank has mapped it)");
  py::class_<IpcHaloTransport, HaloTransport, std::shared_ptr<IpcHaloTransport>>(m, "IpcHaloTransport")
      .def(py::init([](BandEngine& e, const std::string& segment, int slot, int slots, double timeout_s,
                       const std::string& pull) {
             return std::make_shared<IpcHaloTransport>(e, segment, slot, slots, timeout_s, parse_ipc_pull(pull));
           }),
           py::arg("engine"), py::arg("segment"), py::arg("slot") = 0, py::arg("slots") = 1,
           py::arg("timeout_s") = 30.0, py::arg("pull") = "grid", py::keep_alive<1, 2>())
      .def_property_readonly("pull", [](const IpcHaloTransport& t) { return std::string(ipc_pull_name(t.pull())); })
      .def("local_handles", [](const IpcHaloTransport& t) {
        const auto v = t.local_handles();
        return py::bytes(reinterpret_cast<const char*>(v.data()), v.size());
      })
      .def("connect",
           [](IpcHaloTransport& t, py::bytes up, py::bytes down) {
             const std::string u = up, d = down;
             t.connect(std::vector<uint8_t>(u.begin(), u.end()), std::vector<uint8_t>(d.begin(), d.end()));
           },
           py::arg("up"), py::arg("down"))
      .def_property_readonly("connected", &IpcHaloTransport::connected)
      .def("self_test", &IpcHaloTransport::self_test, py::arg("timeout_s") = 5.0,
           py::call_guard<py::gil_scoped_release>(),
           "collective: one exchange of sentinel rows with the neighbours, compared; raises a named error")
      .def_property_readonly("self_tested", &IpcHaloTransport::self_tested)
      .def_property_readonly("mailbox_kind", &IpcHaloTransport::mailbox_kind)
      .def("peer_device", &IpcHaloTransport::peer_device, py::arg("side"))
      .def_property_readonly("enqueued", &IpcHaloTransport::enqueued)
      .def_property_readonly("device_count", &IpcHaloTransport::device_count)
      .def("check", &IpcHaloTransport::check, "raise if a wait of this rank timed out (after the stream drained)");

  // ---------------------------------------------------------------- RCCL
  m.def("rccl_unique_id", []() {
    const auto v = rccl_unique_id();
    return py::bytes(reinterpret_cast<const char*>(v.data()), v.size());
  });
  m.def("rccl_version", &rccl_version);
  m.def("rccl_loaded", &rccl_loaded, "True once librccl is mapped (loaded lazily on the first RCCL call)");
  m.def("install_crash_handler", &install_crash_handler,
        "print a native backtrace on SIGSEGV/SIGBUS/SIGILL/SIGFPE/SIGABRT, then chain to the previous handler");
  m.def("rccl_capture_probe", &rccl_capture_probe, py::arg("op") = "sendrecv", py::arg("mode") = "relaxed",
        py::arg("bytes") = 4096, py::arg("device") = 0, py::arg("launches") = 3,
        py::call_guard<py::gil_scoped_release>());
  m.def("rccl_selftest_exchange", &rccl_selftest_exchange, py::arg("device") = 0,
        py::call_guard<py::gil_scoped_release>());
  m.def("rccl_selftest_multicomm", &rccl_selftest_multicomm, py::arg("device") = 0, py::arg("slots") = 3,
        py::arg("images") = 60, py::arg("timeout_s") = 60.0, py::call_guard<py::gil_scoped_release>());
  m.def("rccl_library_path", &rccl_library_path, "path of the mapped librccl ('' while none is mapped)");
  m.def(
      "runtime_info",
      []() {
        const HipRuntimeInfo h = hip_runtime_info();
        py::dict d;
        d["hip_runtime_version"] = h.runtime_version;
        d["hip_driver_version"] = h.driver_version;
        d["hip_runtime_path"] = h.runtime_path;
        d["hip_compiled_version"] = h.compiled_version;
        const bool loaded = rccl_loaded();
        d["rccl_version"] = loaded ? py::object(py::str(rccl_version())) : py::object(py::none());
        d["rccl_path"] = loaded ? py::object(py::str(rccl_library_path())) : py::object(py::none());
        return d;
      },
      "the HIP runtime / RCCL this process actually runs on (versions and library paths)");
  py::class_<RcclComm, std::shared_ptr<RcclComm>>(m, "RcclComm")
      .def(py::init([](py::bytes id, int rank, int world, int device) {
             const std::string s = id;
             std::vector<uint8_t> v(s.begin(), s.end());
             py::gil_scoped_release nogil;
             return std::make_shared<RcclComm>(v, rank, world, device);
           }),
           py::arg("unique_id"), py::arg("rank"), py::arg("world"), py::arg("device"))
      .def_property_readonly("rank", &RcclComm::rank)
      .def_property_readonly("world", &RcclComm::world)
      .def("allreduce_max", &RcclComm::allreduce_max, py::call_guard<py::gil_scoped_release>())
      .def("allreduce_sum", &RcclComm::allreduce_sum, py::call_guard<py::gil_scoped_release>())
      .def("barrier", &RcclComm::barrier, py::call_guard<py::gil_scoped_release>())
      .def(
          "wait",
          [](RcclComm& c, uintptr_t stream, double timeout_s) { c.wait(reinterpret_cast<hipStream_t>(stream), timeout_s); },
          py::arg("stream"), py::arg("timeout_s"), py::call_guard<py::gil_scoped_release>(),
          "Wait for a stream while polling RCCL async errors; aborts the communicator and raises on timeout.");

  m.def("set_error_rank", &set_error_rank);
}
