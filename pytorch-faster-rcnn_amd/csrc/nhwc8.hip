// frh_nchw_to_nhwc8: an NCHW f32 image batch of 1 .. 8 channels as NHWC with the channels
// zero-padded to 8, the input of VGG16's first conv on frh_conv3x3_bias_act (cin % 8 == 0; the
// zero channels add exact zeros to every Winograd sum).  One thread per pixel: c plane reads
// (a wave reads 256 contiguous bytes of each plane) and two 16-byte stores (a wave writes 2 KB
// contiguous).  Bytes per pixel: 4 c read, 32 written: HBM-bound.
#include "common.h"

namespace frh {
namespace {

__global__ void __launch_bounds__(256) nchw_to_nhwc8_kernel(const float* __restrict__ x, float* __restrict__ y,
                                                            int64_t pixels, int64_t plane, int c) {
  const int64_t p = (int64_t)blockIdx.x * 256 + threadIdx.x;  // (image, y, x) flat
  if (p >= pixels) return;
  const int64_t img = p / plane;
  const float* xp = x + img * c * plane + (p - img * plane);
  float v[8];
#pragma unroll
  for (int k = 0; k < 8; ++k) v[k] = k < c ? xp[k * plane] : 0.0f;
  float4* yp = reinterpret_cast<float4*>(y + p * 8);
  yp[0] = make_float4(v[0], v[1], v[2], v[3]);
  yp[1] = make_float4(v[4], v[5], v[6], v[7]);
}

}  // namespace
}  // namespace frh

using namespace frh;

extern "C" int32_t frh_nchw_to_nhwc8(const float* x, float* y, int64_t n, int32_t c, int32_t h, int32_t w,
                                     void* stream) {
  FRH_REQUIRE(n >= 0 && h >= 0 && w >= 0 && c >= 1 && c <= 8, "nchw_to_nhwc8: 1 to 8 channels, sizes >= 0");
  const int64_t plane = (int64_t)h * w, pixels = n * plane;
  if (pixels == 0) return FRH_OK;
  FRH_REQUIRE(pixels < ((int64_t)1 << 38), "nchw_to_nhwc8: too many pixels");
  FRH_REQUIRE(x && y, "null pointer argument");
  FRH_REQUIRE_ALIGNED16(x, y);
  FRH_REQUIRE(!ranges_overlap(y, pixels * 32, x, pixels * c * 4), "y must not alias x");
  hipLaunchKernelGGL(nchw_to_nhwc8_kernel, dim3((unsigned)((pixels + 255) / 256)), dim3(256), 0, as_stream(stream), x,
                     y, pixels, plane, c);
  return check_launch("frh_nchw_to_nhwc8");
}
