// Device side of ImageTables (pconv/kernels.hpp) for the kernels on a flat,
// image-major grid: k_residual, k_decimate and k_unsharp.  (The temporal
// kernels decode another grid — tiles, XCD swizzle, blockIdx.z — themselves.)
#pragma once

#include <hip/hip_runtime.h>

#include "pconv/kernels.hpp"

namespace pconv {

// Where a workgroup of the flat grid works.  The grid is images x
// blocks_per_image workgroups, image-major: the row's blocks fastest (blocks_x
// of them), then the block rows, then the images, so a workgroup never spans
// two images.  All scalar, from the workgroup id.  `img` is the grid's slot:
// the kernel moves its base pointers by img * stride, in 64 bits, before
// anything else (after an active table's remap, where it has one).
struct ImageBlock {
  unsigned img;
  int bx, by;
};
__device__ __forceinline__ ImageBlock image_block(int blocks_x, int blocks_per_image) {
  const unsigned img = blockIdx.x / static_cast<unsigned>(blocks_per_image);
  const unsigned blk = blockIdx.x - img * static_cast<unsigned>(blocks_per_image);
  return {img, static_cast<int>(blk % static_cast<unsigned>(blocks_x)),
          static_cast<int>(blk / static_cast<unsigned>(blocks_x))};
}

// An entry of the extents table inside the envelope of row_bytes x rows:
// whatever the device table holds, the image stays inside its frame (and an
// entry below zero leaves the workgroup nothing, so it exits before its first
// load).
__device__ __forceinline__ ImageDims clamp_extent(ImageDims d, int row_bytes, int rows) {
  return {min(max(d.row_bytes, 0), row_bytes), min(max(d.height, 0), rows)};
}

}  // namespace pconv
