// Search on gfx950: the response of every pixel of a key map to up to RW_KEY_RESPONSE_MAX_KEYS query keys
// (ProgressiveGanRewriter.ranking_for_key, rewrite/ganrewrite.py:582-594, and the heat maps of render_image*,
// :610-650), heat[b][k][p] = sum_c keys[k][c] * a[b][c][p], and the per-image maximum the ranking sorts by.
//
// The key map is the only large operand (the resident index of rewrite/search.py is tens of GB) and is read ONCE for
// all K keys, NCHW as the generator left it: a lane owns V consecutive pixels of one image (V = 4: one 16-byte load per
// channel, a wave reads 1 KiB of consecutive addresses; V = 1 where hw % 4 != 0 or a pointer is not 16-byte aligned),
// keeps K x V sums in registers and walks the channels 0 .. C-1 in order, one fused multiply-add per (key, pixel).  The
// key values are wave-uniform and come through the scalar cache.  (image, pixel group) is flattened over the grid, so
// 4x4 and 8x8 maps fill their waves with several images.
//
// The sum of a pixel is the same chain of C fmaf's in every form: it does not depend on images, on n_keys, on the slot
// a key sits in, on V or on the chip.  A row of heat is therefore bit-identical alone or inside any launch.
// peak is a second small launch over heat (1/C of the first pass's traffic): a plain maximum, so peak == max_p heat bit
// for bit.  No atomics, no memset, no partial slots.
#include "rw_common.h"

#include <math.h>

#define KR_BLOCK 256
#define KR_UNROLL 8       // channels whose loads are issued before the first of them is used

template <int V> struct kr_vec;
template <> struct kr_vec<4> { typedef rw_f32x4 type; };
template <> struct kr_vec<1> { typedef float type; };
__device__ __forceinline__ float kr_at(const rw_f32x4& v, int j) { return v[j]; }
__device__ __forceinline__ float kr_at(const float& v, int) { return v; }

// groups = images * (hw / V) pixel groups of V pixels; gpi = hw / V groups per image
template <int K, int V>
__global__ void __launch_bounds__(KR_BLOCK) key_response_kernel(const float* __restrict__ a, const float* __restrict__ keys,
                                                                float* __restrict__ heat, int64_t groups, int channels,
                                                                int hw, int gpi) {
  typedef typename kr_vec<V>::type vec;
  const int64_t g = (int64_t)blockIdx.x * KR_BLOCK + threadIdx.x;
  if (g >= groups) return;
  const int64_t img = g / gpi;
  const int p0 = (int)(g - img * gpi) * V;
  const float* src = a + img * channels * (int64_t)hw + p0;      // + c * hw: channels * hw fits 31 bits (checked by the entry)

  float acc[K][V];
#pragma unroll
  for (int k = 0; k < K; ++k)
#pragma unroll
    for (int j = 0; j < V; ++j) acc[k][j] = 0.f;

  int c = 0;
  for (; c + KR_UNROLL <= channels; c += KR_UNROLL) {
    vec x[KR_UNROLL];
#pragma unroll
    for (int u = 0; u < KR_UNROLL; ++u) x[u] = *reinterpret_cast<const vec*>(src + (c + u) * hw);
#pragma unroll
    for (int u = 0; u < KR_UNROLL; ++u)
#pragma unroll
      for (int k = 0; k < K; ++k) {
        const float kv = keys[k * channels + c + u];
#pragma unroll
        for (int j = 0; j < V; ++j) acc[k][j] = __builtin_fmaf(kv, kr_at(x[u], j), acc[k][j]);
      }
  }
  for (; c < channels; ++c) {
    const vec x = *reinterpret_cast<const vec*>(src + c * hw);
#pragma unroll
    for (int k = 0; k < K; ++k) {
      const float kv = keys[k * channels + c];
#pragma unroll
      for (int j = 0; j < V; ++j) acc[k][j] = __builtin_fmaf(kv, kr_at(x, j), acc[k][j]);
    }
  }

  float* dst = heat + img * K * (int64_t)hw + p0;                 // + k * hw: K * hw fits 31 bits
#pragma unroll
  for (int k = 0; k < K; ++k) {
    vec r;
    if constexpr (V == 4) r = rw_f32x4{acc[k][0], acc[k][1], acc[k][2], acc[k][3]};
    else r = acc[k][0];
    *reinterpret_cast<vec*>(dst + k * hw) = r;
  }
}

// peak[row] = max_p heat[row][p], one wave per row of hw responses (rows = images * K)
__global__ void __launch_bounds__(KR_BLOCK) key_response_peak_kernel(const float* __restrict__ heat, float* __restrict__ peak,
                                                                     int64_t rows, int hw) {
  const int64_t row = (int64_t)blockIdx.x * (KR_BLOCK / RW_WAVE) + (threadIdx.x >> 6);
  if (row >= rows) return;                                        // wave-uniform
  const float* src = heat + row * hw;
  float m = -INFINITY;
  for (int p = threadIdx.x & 63; p < hw; p += RW_WAVE) m = fmaxf(m, src[p]);
  m = rw_wave_max(m);
  if ((threadIdx.x & 63) == 0) peak[row] = m;
}

template <int K>
static void kr_launch(bool vec4, unsigned blocks, hipStream_t s, const float* a, const float* keys, float* heat,
                      int64_t groups, int channels, int hw, int gpi) {
  if (vec4)
    hipLaunchKernelGGL((key_response_kernel<K, 4>), dim3(blocks), dim3(KR_BLOCK), 0, s, a, keys, heat, groups, channels, hw, gpi);
  else
    hipLaunchKernelGGL((key_response_kernel<K, 1>), dim3(blocks), dim3(KR_BLOCK), 0, s, a, keys, heat, groups, channels, hw, gpi);
}

extern "C" int rw_key_response_f32(const float* a, const float* keys, float* heat, float* peak, int64_t images,
                                   int channels, int64_t hw, int n_keys, rw_stream_t stream) {
  RW_CHECK_ARG(a && keys && heat && images >= 1 && channels >= 1 && hw >= 1);
  RW_CHECK_ARG(n_keys >= 1 && n_keys <= RW_KEY_RESPONSE_MAX_KEYS);
  // offsets inside one image's key map / heat maps are 32-bit; image bases are 64-bit
  RW_CHECK_ARG(hw <= INT32_MAX && (int64_t)channels * hw <= INT32_MAX && (int64_t)n_keys * hw <= INT32_MAX);
  RW_CHECK_ARG(images <= INT32_MAX && (int64_t)n_keys * channels <= INT32_MAX);
  const bool vec4 = hw % 4 == 0 && ((uintptr_t)a % 16) == 0 && ((uintptr_t)heat % 16) == 0;
  const int gpi = (int)(vec4 ? hw / 4 : hw);
  const int64_t groups = images * gpi;
  const int64_t blocks = rw_cdiv(groups, KR_BLOCK);
  const int64_t rows = images * n_keys;
  const int64_t peak_blocks = rw_cdiv(rows, KR_BLOCK / RW_WAVE);
  RW_CHECK_ARG(blocks <= INT32_MAX && peak_blocks <= INT32_MAX);   // the grid's x extent
  hipStream_t s = rw_s(stream);
  const int ihw = (int)hw;
  switch (n_keys) {
    case 1: kr_launch<1>(vec4, (unsigned)blocks, s, a, keys, heat, groups, channels, ihw, gpi); break;
    case 2: kr_launch<2>(vec4, (unsigned)blocks, s, a, keys, heat, groups, channels, ihw, gpi); break;
    case 3: kr_launch<3>(vec4, (unsigned)blocks, s, a, keys, heat, groups, channels, ihw, gpi); break;
    case 4: kr_launch<4>(vec4, (unsigned)blocks, s, a, keys, heat, groups, channels, ihw, gpi); break;
    case 5: kr_launch<5>(vec4, (unsigned)blocks, s, a, keys, heat, groups, channels, ihw, gpi); break;
    case 6: kr_launch<6>(vec4, (unsigned)blocks, s, a, keys, heat, groups, channels, ihw, gpi); break;
    case 7: kr_launch<7>(vec4, (unsigned)blocks, s, a, keys, heat, groups, channels, ihw, gpi); break;
    default: kr_launch<8>(vec4, (unsigned)blocks, s, a, keys, heat, groups, channels, ihw, gpi); break;
  }
  const int rc = RW_LAUNCH_RESULT();
  if (rc || !peak) return rc;
  hipLaunchKernelGGL(key_response_peak_kernel, dim3((unsigned)peak_blocks), dim3(KR_BLOCK), 0, s, heat, peak, rows, ihw);
  return RW_LAUNCH_RESULT();
}
