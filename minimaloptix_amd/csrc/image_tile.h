// image_tile.h -- the image-space kernels' pixel mapping (denoisekernel.hip, temporalkernel.hip, adaptivekernel.hip; no trace kernel
// includes this): a lane per pixel, a 256-thread workgroup covers 16x16 pixels as four 8x8 tiles, one per wave.  A wave's tile is a tile
// of the trace kernels' slot numbering (megakernel.h item_to_pixel), and its taps fall on 8-row blocks that neighbouring lanes share.
#pragma once
#include <hip/hip_runtime.h>

namespace pt {

constexpr int kImageBlockThreads = 256;

inline dim3 image_grid(int width, int height) { return dim3((width + 15) / 16, (height + 15) / 16); }

// This lane's pixel and the 8x8 tile (tx, ty) of its wave; false outside the frame.
__device__ __forceinline__ bool image_pixel(int width, int height, int& x, int& y, int& tx, int& ty) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  tx = blockIdx.x * 2 + (wave & 1); ty = blockIdx.y * 2 + (wave >> 1);
  x = tx * 8 + (lane & 7); y = ty * 8 + (lane >> 3);
  return x < width && y < height;
}
__device__ __forceinline__ bool image_pixel(int width, int height, int& x, int& y) {
  int tx, ty;
  return image_pixel(width, height, x, y, tx, ty);
}

}  // namespace pt
