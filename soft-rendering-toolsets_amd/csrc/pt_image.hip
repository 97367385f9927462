// The image kernels that never see a scene: the gathered tiles of all ranks to a row-major image, Pathtracer::accumulate, and
// HDR_Image::tonemap_to.  Reference paths are relative to the reference's src/, as in pt.hip.
#include <hip/hip_runtime.h>

#include "pt_context.h"
#include "pt_device.h"

namespace srt {

__global__ void pt_untile_kernel(TileMap T, uint32_t w, uint32_t h, uint32_t tiles_per_rank,
                                 const float* __restrict__ gathered, float* __restrict__ image) {
  const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= w * h) return;
  const uint32_t x = i % w, y = i / w;
  const uint32_t tile = (y / T.tile_h) * T.tiles_x + (x / T.tile_w);
  const uint32_t rank = tile % T.world, local = tile / T.world;
  const size_t src = (((size_t)rank * tiles_per_rank + local) * (T.tile_w * T.tile_h) + (size_t)(y % T.tile_h) * T.tile_w +
                      (x % T.tile_w)) * 3;
  image[3 * (size_t)i] = gathered[src];
  image[3 * (size_t)i + 1] = gathered[src + 1];
  image[3 * (size_t)i + 2] = gathered[src + 2];
}

// Pathtracer::accumulate: s += (n - s) * (1.0f / accumulator_samples)
__global__ void pt_accumulate_kernel(float* __restrict__ acc, const float* __restrict__ epoch, size_t n, float inv) {
  const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i < n) acc[i] += (epoch[i] - acc[i]) * inv;
}

// HDR_Image::tonemap_to (util/hdr_image.cpp:161-187): output row j is image row h-1-j; per channel
// 1 - exp(-c * exposure), Spectrum::to_srgb, (unsigned char)round(c * 255); alpha 255.  One lane per pixel, one packed
// 32-bit store (consecutive lanes: consecutive pixels of an output row, 12-byte loads / 4-byte stores, fully coalesced).
__global__ void pt_tonemap_kernel(const float* __restrict__ rgb, uint32_t w, uint32_t h, float exposure, uint32_t* __restrict__ rgba) {
  const size_t p = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (p >= (size_t)w * h) return;
  const uint32_t j = (uint32_t)(p / w), i = (uint32_t)(p % w);
  const float* s = rgb + 3 * ((size_t)(h - j - 1) * w + i);
  uint32_t px = 0xff000000u;
#pragma unroll
  for (int c = 0; c < 3; c++) px |= srgb_byte(to_srgb(1.0f - srt_expf(-s[c] * exposure))) << (8 * c);
  rgba[p] = px;
}

}  // namespace srt

using namespace srt;

extern "C" {

int srt_pt_untile_device(srt_pt* pt, void* stream, const float* d_gathered, float* d_image) {
  int st = need_ready(pt, "srt_pt_untile_device");
  if (st != SRT_OK) return st;
  if (!d_gathered || !d_image) return srt::fail(SRT_ERR_INVALID, "srt_pt_untile_device: NULL buffer");
  hipStream_t s = (hipStream_t)stream;  // exactly the caller's stream; NULL is the HIP default stream
  const uint32_t n = pt->w * pt->h;
  pt_untile_kernel<<<dim3((n + 255) / 256), dim3(256), 0, s>>>(pt->tiles, pt->w, pt->h, pt->tiles_per_rank, d_gathered, d_image);
  SRT_HIP(hipGetLastError());
  return SRT_OK;
}

int srt_pt_accumulate_device(srt_pt* pt, void* stream, float* d_accumulator, const float* d_epoch, size_t nfloats,
                             uint32_t accumulator_samples) {
  int st = need_device(pt, "srt_pt_accumulate_device");
  if (st != SRT_OK) return st;
  if (!d_accumulator || !d_epoch || !accumulator_samples) return srt::fail(SRT_ERR_INVALID, "srt_pt_accumulate_device: bad argument");
  hipStream_t s = (hipStream_t)stream;  // exactly the caller's stream; NULL is the HIP default stream
  pt_accumulate_kernel<<<dim3((unsigned)((nfloats + 255) / 256)), dim3(256), 0, s>>>(d_accumulator, d_epoch, nfloats,
                                                                                 1.0f / accumulator_samples);
  SRT_HIP(hipGetLastError());
  return SRT_OK;
}

int srt_pt_tonemap_device(srt_pt* pt, void* stream, const float* d_rgb, uint32_t width, uint32_t height, float exposure, uint8_t* d_rgba) {
  int st = need_device(pt, "srt_pt_tonemap_device");
  if (st != SRT_OK) return st;
  if (!d_rgb || !d_rgba) return srt::fail(SRT_ERR_INVALID, "srt_pt_tonemap_device: NULL argument");
  if (!(exposure > 0.0f)) return srt::fail(SRT_ERR_INVALID, "srt_pt_tonemap_device: exposure must be positive (got %g)", (double)exposure);
  if ((reinterpret_cast<uintptr_t>(d_rgba) & 3u) != 0) return srt::fail(SRT_ERR_INVALID, "srt_pt_tonemap_device: rgba must be 4-byte aligned");
  const size_t px = (size_t)width * height;
  if (!px) return SRT_OK;
  hipStream_t s = static_cast<hipStream_t>(stream);      // exactly the caller's stream; NULL is the HIP default stream, as for every *_device call
  pt_tonemap_kernel<<<dim3((unsigned)((px + 255) / 256)), dim3(256), 0, s>>>(d_rgb, width, height, exposure, reinterpret_cast<uint32_t*>(d_rgba));
  SRT_HIP(hipGetLastError());
  return SRT_OK;
}

int srt_pt_tonemap(srt_pt* pt, const float* rgb, uint32_t width, uint32_t height, float exposure, uint8_t* rgba_out) {
  int st = need_device(pt, "srt_pt_tonemap");
  if (st != SRT_OK) return st;
  if (!rgb || !rgba_out) return srt::fail(SRT_ERR_INVALID, "srt_pt_tonemap: NULL argument");
  if (!(exposure > 0.0f)) return srt::fail(SRT_ERR_INVALID, "srt_pt_tonemap: exposure must be positive (got %g)", (double)exposure);
  const size_t px = (size_t)width * height;
  if (!px) return SRT_OK;
  DeviceBuffer<float> d_in; DeviceBuffer<uint8_t> d_out;
  if ((st = d_in.ensure(3 * px)) || (st = d_out.ensure(4 * px))) return st;
  if (hipMemcpyAsync(d_in, rgb, px * 12, hipMemcpyHostToDevice, pt->stream) != hipSuccess) st = srt::fail(SRT_ERR_HIP, "srt_pt_tonemap: upload failed");
  if (st == SRT_OK) st = srt_pt_tonemap_device(pt, (void*)pt->stream, d_in, width, height, exposure, d_out);
  if (st == SRT_OK && (hipMemcpyAsync(rgba_out, d_out, px * 4, hipMemcpyDeviceToHost, pt->stream) != hipSuccess ||
                       hipStreamSynchronize(pt->stream) != hipSuccess))
    st = srt::fail(SRT_ERR_HIP, "srt_pt_tonemap: download failed");
  return st;
}

}  // extern "C"
