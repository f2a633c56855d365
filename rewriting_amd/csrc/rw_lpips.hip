// LPIPS (v0.1, net-lin, vgg) behind the VGG16 taps, and the masked reductions of the edit distances -- what
// metrics/distances.py:18-59 (PerceptualLoss: lpips(spatial=True), sum(loss * w) / sum(w)) and :96-136 (compute_dl) run after the
// convolutions:
//
//   lpips_tap       d[b][p] = sum_c lin[c] (f0[b][c][p] / (|f0[b][:][p]| + 1e-10) - f1[..][c][p] / (|f1[..][:][p]| + 1e-10))^2 of one tap
//   lpips_combine   out[b][y][x] = sum_k bilinear(d_k)(y, x) (F.interpolate, align_corners=False, host tables) and / or, per image,
//                   (sum out w, sum w)
//   masked_l1_rgb   per image (sum_p mask sum_c |a - b|, sum_p mask): compute_dl's pixel mode (:131-133)
//
// float32 only.  Every sum runs in a fixed order, no atomics, nothing zeroed beforehand, nothing but launches on the caller's
// stream: two runs give the same bits.  The distance of a tap is formed from the normalised DIFFERENCE as written above, never
// from the expansion sum w a^2 / |a|^2 + sum w b^2 / |b|^2 - 2 sum w a b / (|a| |b|): before and after pictures are nearly equal
// outside the edit, and the expansion cancels there.
#include "rw_common.h"

static inline bool lp_aligned16(const void* p) { return ((uintptr_t)p & 15) == 0; }

// ---------------------------------------------------------------------------------------
// The tap kernel.  Memory-bound: at 1024^2 the first tap is 256 MB per image and input.  Every value comes from HBM ONCE: a
// workgroup owns a run of P = 2^p_log2 consecutive pixels of one image and stages both maps' ch x P values in LDS (rows
// [c][P], the loads coalesced along the run, 16 bytes per lane where hw % 4 == 0 and the pointers are aligned), then walks
// them twice -- the two norms, then the weighted squared difference.  Thread tid is pixel px = tid % P in channel group
// g = tid / P of G = 256 / P: it takes the channels g, g + G, ... in ascending order, the groups' partial sums meet in LDS
// and are added pairwise (group g takes group g + s for s = G / 2, G / 4, ... 1: log2 G additions on a term's way, not G --
// a 1 x 1 map of 256 channels is one channel per thread and the tree).
// P is the largest power of two with 2 ch P floats within the tile, and no larger than the map needs.  The tile is
// LP_TILE_FLOATS (32 KB, four workgroups per CU) where that leaves rows of 32 pixels = 128 bytes or more (up to 128 channels:
// 64 channels stage 64 pixels, 128 stage 32), LP_WIDE_TILE_FLOATS (64 KB, two per CU) above (256 channels: 32 pixels, 512: 16).
// Measured at 1024^2 (read rate in TB/s by tile, 64 / 128 / 256 / 512 channels): 32 KB 3.6 / 3.6 / 2.2 / 1.2, 64 KB 2.7 / 2.9 /
// 2.4 / 1.5, 128 KB 1.9 / 2.0 / 1.7 / 1.4 -- occupancy first, then the length of a row.  ch beyond half the wide tile (no single
// pixel fits): the same walk reads global memory twice (STAGED = false, P = 256).  RW_LPIPS_TILE: the tile in floats, for tuning.
// ---------------------------------------------------------------------------------------
#define LP_TILE_FLOATS 8192
#define LP_WIDE_TILE_FLOATS 16384
#define LP_MAX_TILE_FLOATS 32768             // what RW_LPIPS_TILE may ask for: 128 KB, one workgroup per CU
#define LP_RED_FLOATS 512                    // the groups' partial sums: [2][256]

struct LpTap {
  const float* f0; const float* f1; const float* lin; float* d;
  int ch, p_log2;
  int64_t hw, f1_stride, tiles_per_image;
};

template <bool STAGED, bool V4>
__global__ void __launch_bounds__(256) lpips_tap_kernel(const LpTap p) {
  extern __shared__ __attribute__((aligned(16))) float lp_lds[];
  const int tid = threadIdx.x;
  const int P = 1 << p.p_log2, G = 256 >> p.p_log2;
  float* t0 = lp_lds;
  float* t1 = t0 + (STAGED ? p.ch * P : 0);
  float* red = t1 + (STAGED ? p.ch * P : 0);
  const int64_t tile = blockIdx.x;
  const int64_t b = tile / p.tiles_per_image, p0 = (tile - b * p.tiles_per_image) * P;
  const float* g0 = p.f0 + b * p.ch * p.hw + p0;
  const float* g1 = p.f1 + b * p.f1_stride + p0;
  const int valid = (int)(p.hw - p0 < P ? p.hw - p0 : P);
  if (STAGED) {
    if (V4) {                                    // hw % 4 == 0 and P % 4 == 0: a quad is inside the map or outside it
      const int q_log2 = p.p_log2 - 2, quads = p.ch << q_log2;
      // four quads of each map per thread and step, all eight loads issued before the first LDS write: a full 64-channel
      // tile is two steps, and a CU's two workgroups keep 64 KB in flight
      for (int t4 = tid; t4 < quads; t4 += 1024) {
        float4 a[4], bq[4];
#pragma unroll
        for (int j = 0; j < 4; ++j) {
          const int t = t4 + 256 * j;
          const int c = t >> q_log2, q = t & ((1 << q_log2) - 1);
          a[j] = bq[j] = make_float4(0.f, 0.f, 0.f, 0.f);
          if (t < quads && 4 * q < valid) {
            a[j] = *reinterpret_cast<const float4*>(g0 + (int64_t)c * p.hw + 4 * q);
            bq[j] = *reinterpret_cast<const float4*>(g1 + (int64_t)c * p.hw + 4 * q);
          }
        }
#pragma unroll
        for (int j = 0; j < 4; ++j) {
          const int t = t4 + 256 * j;
          if (t < quads) {
            reinterpret_cast<float4*>(t0)[t] = a[j];
            reinterpret_cast<float4*>(t1)[t] = bq[j];
          }
        }
      }
    } else {
      const int n = p.ch << p.p_log2;
      for (int t = tid; t < n; t += 256) {
        const int c = t >> p.p_log2, q = t & (P - 1);
        const bool ok = q < valid;
        t0[t] = ok ? g0[(int64_t)c * p.hw + q] : 0.f;
        t1[t] = ok ? g1[(int64_t)c * p.hw + q] : 0.f;
      }
    }
    __syncthreads();
  }
  const int px = tid & (P - 1), g = tid >> p.p_log2;
  const bool ok = px < valid;
  auto a_of = [&](int c) __attribute__((always_inline)) {
    return STAGED ? t0[(c << p.p_log2) + px] : (ok ? g0[(int64_t)c * p.hw + px] : 0.f);
  };
  auto b_of = [&](int c) __attribute__((always_inline)) {
    return STAGED ? t1[(c << p.p_log2) + px] : (ok ? g1[(int64_t)c * p.hw + px] : 0.f);
  };
  float s0 = 0.f, s1 = 0.f;
  for (int c = g; c < p.ch; c += G) {
    const float a = a_of(c), bv = b_of(c);
    s0 = fmaf(a, a, s0);
    s1 = fmaf(bv, bv, s1);
  }
  red[tid] = s0;                                 // tid == g * P + px
  red[256 + tid] = s1;
  __syncthreads();
  for (int s = G >> 1; s > 0; s >>= 1) {
    if (g < s) {
      red[tid] += red[tid + (s << p.p_log2)];
      red[256 + tid] += red[256 + tid + (s << p.p_log2)];
    }
    __syncthreads();
  }
  const float den0 = sqrtf(red[px]) + 1e-10f, den1 = sqrtf(red[256 + px]) + 1e-10f;    // a zero vector: 0 / (0 + eps) = 0
  __syncthreads();
  float acc = 0.f;
  for (int c = g; c < p.ch; c += G) {
    const float t = a_of(c) / den0 - b_of(c) / den1;
    acc = fmaf(p.lin[c], t * t, acc);
  }
  red[tid] = acc;
  __syncthreads();
  for (int s = G >> 1; s > 0; s >>= 1) {
    if (g < s) red[tid] += red[tid + (s << p.p_log2)];
    __syncthreads();
  }
  if (g == 0 && ok) p.d[b * p.hw + p0 + px] = red[px];
}

template <bool STAGED, bool V4>
static int lp_launch_tap(const LpTap& p, int64_t tiles, size_t ldsb, hipStream_t s) {
  if (ldsb > 65536) {
    const hipError_t e = hipFuncSetAttribute((const void*)lpips_tap_kernel<STAGED, V4>, hipFuncAttributeMaxDynamicSharedMemorySize,
                                             (int)ldsb);
    if (e != hipSuccess) return (int)e;
  }
  hipLaunchKernelGGL((lpips_tap_kernel<STAGED, V4>), dim3((unsigned)tiles), dim3(256), ldsb, s, p);
  return RW_LAUNCH_RESULT();
}

extern "C" int rw_lpips_tap_f32(const float* f0, const float* f1, const float* lin, float* d, int batch, int f1_batch, int ch,
                                int64_t hw, rw_stream_t stream) {
  RW_CHECK_ARG(f0 && f1 && lin && d && batch > 0 && ch > 0 && hw > 0 && (f1_batch == batch || f1_batch == 1));
  const int dflt = 2 * (int64_t)ch * 32 <= LP_TILE_FLOATS ? LP_TILE_FLOATS : LP_WIDE_TILE_FLOATS;
  int tile = rw_env_int("RW_LPIPS_TILE", dflt);
  if (tile < 2 || tile > LP_MAX_TILE_FLOATS) tile = dflt;
  const bool staged = 2 * (int64_t)ch <= tile;
  int p_log2 = 8;
  while (staged && p_log2 > 0 && 2 * (int64_t)ch << p_log2 > tile) --p_log2;
  while (p_log2 > 0 && (1 << (p_log2 - 1)) >= hw) --p_log2;              // a small map: more channel groups, fewer idle pixels
  LpTap p;
  p.f0 = f0; p.f1 = f1; p.lin = lin; p.d = d; p.ch = ch; p.p_log2 = p_log2; p.hw = hw;
  p.f1_stride = f1_batch == 1 ? 0 : (int64_t)ch * hw;
  p.tiles_per_image = rw_cdiv(hw, 1 << p_log2);
  const int64_t tiles = p.tiles_per_image * batch;
  if (tiles > 0x7fffffff) return RW_ERR_UNSUPPORTED;
  const size_t ldsb = sizeof(float) * ((staged ? ((size_t)2 * ch << p_log2) : 0) + LP_RED_FLOATS);
  const bool v4 = staged && p_log2 >= 2 && hw % 4 == 0 && lp_aligned16(f0) && lp_aligned16(f1);
  if (!staged) return lp_launch_tap<false, false>(p, tiles, ldsb, rw_s(stream));
  if (v4) return lp_launch_tap<true, true>(p, tiles, ldsb, rw_s(stream));
  return lp_launch_tap<true, false>(p, tiles, ldsb, rw_s(stream));
}

// ---------------------------------------------------------------------------------------
// The per-image reductions (lpips_combine, masked_l1_rgb).  A thread adds its T <= LP_MAX_PER_THREAD terms in ascending pixel
// order, the workgroup's 256 threads meet in rw_block_sum_256 (6 additions across the wave, 3 across the waves), the
// workgroup stores its pair PLAINLY into its own slot of `scratch`, and lp_finish_kernel -- one workgroup per image --
// adds the nblk <= 256 LP_MAX_FINISH slots the same way: M = ceil(nblk / 256) <= LP_MAX_FINISH per thread, then 6 + 3.  A term
// passes through at most T + 9 + M + 9 <= 28 + 16 + 18 = 62 additions; there is no serial sum over an image.  T is the smallest
// count that keeps nblk within 256 LP_MAX_FINISH: 1 up to 1024^2 pixels; more than 28 (an image above 29.3 M pixels) is refused.
// ---------------------------------------------------------------------------------------
#define LP_MAX_PER_THREAD 28
#define LP_MAX_FINISH 16

// (T, nblk) for an image of hw pixels; false: refused
static bool lp_reduce_shape(int64_t hw, int* per_thread, int* nblk) {
  if (hw <= 0) return false;
  int t = 1;
  while (t <= LP_MAX_PER_THREAD && rw_cdiv(hw, 256LL * t) > 256 * LP_MAX_FINISH) ++t;
  if (t > LP_MAX_PER_THREAD) return false;
  *per_thread = t;
  *nblk = (int)rw_cdiv(hw, 256LL * t);
  return true;
}

extern "C" long long rw_lpips_reduce_scratch_elems(int batch, int64_t hw) {
  int t, nblk;
  if (batch <= 0 || !lp_reduce_shape(hw, &t, &nblk)) return -1;
  return 2LL * batch * nblk;
}

// the workgroup's pair into its slot
__device__ __forceinline__ void lp_store_partial(float* __restrict__ scratch, float s0, float s1, float* lds4) {
  s0 = rw_block_sum_256(s0, lds4);
  s1 = rw_block_sum_256(s1, lds4);
  if (threadIdx.x == 0) {
    float* slot = scratch + 2 * ((int64_t)blockIdx.y * gridDim.x + blockIdx.x);
    slot[0] = s0;
    slot[1] = s1;
  }
}

__global__ void __launch_bounds__(256) lp_finish_kernel(const float* __restrict__ scratch, float* __restrict__ sums, int nblk) {
  __shared__ float lds4[4];
  const float* slots = scratch + 2 * (int64_t)blockIdx.x * nblk;
  float s0 = 0.f, s1 = 0.f;
  for (int m = threadIdx.x; m < nblk; m += 256) {
    s0 += slots[2 * m];
    s1 += slots[2 * m + 1];
  }
  s0 = rw_block_sum_256(s0, lds4);
  s1 = rw_block_sum_256(s1, lds4);
  if (threadIdx.x == 0) {
    sums[2 * blockIdx.x] = s0;
    sums[2 * blockIdx.x + 1] = s1;
  }
}

// ---------------------------------------------------------------------------------------
// lpips_combine.  Tables of tap k (lpips.upsample_table, computed on the host in float64 and rounded once):
//   idx + k (2 h + 2 w): [row i0 (h)] [row i1 (h)] [column i0 (w)] [column i1 (w)]      lam + k (h + w): [row lambda (h)] [column lambda (w)]
// out(y, x) = sum_k  (1 - ly) ((1 - lx) d[y0][x0] + lx d[y0][x1]) + ly ((1 - lx) d[y1][x0] + lx d[y1][x1]), taps in ascending
// order -- upsample_bilinear2d's form.  Indices are clamped into the tap's map: a wrong table gives a wrong picture, never a
// read outside it.
// ---------------------------------------------------------------------------------------
struct LpCombine {
  rw_lpips_maps m;
  const int* idx; const float* lam; const float* weight;
  float* out; float* scratch;
  int64_t weight_stride;
  int h, w, per_thread;
};

__device__ __forceinline__ int lp_clamp(int i, int n) { return i < 0 ? 0 : (i >= n ? n - 1 : i); }

__global__ void __launch_bounds__(256) lpips_combine_kernel(const LpCombine p) {
  __shared__ float lds4[4];
  const int b = blockIdx.y;
  const int64_t hw = (int64_t)p.h * p.w, base = (int64_t)blockIdx.x * 256 * p.per_thread;
  float s0 = 0.f, s1 = 0.f;
  for (int r = 0; r < p.per_thread; ++r) {
    const int64_t at = base + (int64_t)r * 256 + threadIdx.x;
    if (at >= hw) break;
    const int y = (int)(at / p.w), x = (int)(at - (int64_t)y * p.w);
    float v = 0.f;
    for (int k = 0; k < p.m.n; ++k) {
      const int hk = p.m.h[k], wk = p.m.w[k];
      const int* ik = p.idx + (int64_t)k * (2 * p.h + 2 * p.w);
      const float* lk = p.lam + (int64_t)k * (p.h + p.w);
      const int y0 = lp_clamp(ik[y], hk), y1 = lp_clamp(ik[p.h + y], hk);
      const int x0 = lp_clamp(ik[2 * p.h + x], wk), x1 = lp_clamp(ik[2 * p.h + p.w + x], wk);
      const float ly = lk[y], lx = lk[p.h + x];
      const float* dk = p.m.d[k] + (int64_t)b * hk * wk;
      const float top = (1.f - lx) * dk[(int64_t)y0 * wk + x0] + lx * dk[(int64_t)y0 * wk + x1];
      const float bot = (1.f - lx) * dk[(int64_t)y1 * wk + x0] + lx * dk[(int64_t)y1 * wk + x1];
      v += (1.f - ly) * top + ly * bot;
    }
    if (p.out) p.out[b * hw + at] = v;
    const float wv = p.weight ? p.weight[b * p.weight_stride + at] : 1.f;
    s0 += v * wv;
    s1 += wv;
  }
  if (p.scratch) lp_store_partial(p.scratch, s0, s1, lds4);
}

extern "C" int rw_lpips_combine_f32(const rw_lpips_maps* taps, const int* idx, const float* lam, const float* weight,
                                    int weight_batch, float* out, float* sums, float* scratch, int batch, int h, int w,
                                    rw_stream_t stream) {
  RW_CHECK_ARG(taps && idx && lam && (out || sums) && batch > 0 && h > 0 && w > 0);
  RW_CHECK_ARG(taps->n >= 1 && taps->n <= RW_LPIPS_MAX_TAPS && (!sums || scratch));
  RW_CHECK_ARG(!weight || weight_batch == batch || weight_batch == 1);
  for (int k = 0; k < taps->n; ++k) RW_CHECK_ARG(taps->d[k] && taps->h[k] > 0 && taps->w[k] > 0);
  LpCombine p;
  int nblk;
  if (batch > 65535 || !lp_reduce_shape((int64_t)h * w, &p.per_thread, &nblk)) return RW_ERR_UNSUPPORTED;
  p.m = *taps; p.idx = idx; p.lam = lam; p.weight = weight; p.out = out; p.scratch = sums ? scratch : nullptr;
  p.weight_stride = weight && weight_batch == 1 ? 0 : (int64_t)h * w;
  p.h = h; p.w = w;
  hipLaunchKernelGGL(lpips_combine_kernel, dim3((unsigned)nblk, (unsigned)batch), dim3(256), 0, rw_s(stream), p);
  if (sums) hipLaunchKernelGGL(lp_finish_kernel, dim3((unsigned)batch), dim3(256), 0, rw_s(stream), scratch, sums, nblk);
  return RW_LAUNCH_RESULT();
}

// ---------------------------------------------------------------------------------------
// masked_l1_rgb: (sum_p mask[p] (|a0 - b0| + |a1 - b1| + |a2 - b2|)(p), sum_p mask[p]) per image, channels in ascending order.
// ---------------------------------------------------------------------------------------
__global__ void __launch_bounds__(256) masked_l1_rgb_kernel(const float* __restrict__ a, const float* __restrict__ bm,
                                                            const float* __restrict__ mask, int64_t mask_stride,
                                                            float* __restrict__ scratch, int64_t hw, int per_thread) {
  __shared__ float lds4[4];
  const int b = blockIdx.y;
  const int64_t base = (int64_t)blockIdx.x * 256 * per_thread;
  const float* ab = a + 3 * b * hw;
  const float* bb = bm + 3 * b * hw;
  float s0 = 0.f, s1 = 0.f;
  for (int r = 0; r < per_thread; ++r) {
    const int64_t at = base + (int64_t)r * 256 + threadIdx.x;
    if (at >= hw) break;
    float v = fabsf(ab[at] - bb[at]);
    v += fabsf(ab[hw + at] - bb[hw + at]);
    v += fabsf(ab[2 * hw + at] - bb[2 * hw + at]);
    const float mv = mask[b * mask_stride + at];
    s0 += mv * v;
    s1 += mv;
  }
  lp_store_partial(scratch, s0, s1, lds4);
}

extern "C" int rw_masked_l1_rgb_f32(const float* a, const float* b, const float* mask, int mask_batch, float* sums,
                                    float* scratch, int batch, int64_t hw, rw_stream_t stream) {
  RW_CHECK_ARG(a && b && mask && sums && scratch && batch > 0 && hw > 0 && (mask_batch == batch || mask_batch == 1));
  int per_thread, nblk;
  if (batch > 65535 || !lp_reduce_shape(hw, &per_thread, &nblk)) return RW_ERR_UNSUPPORTED;
  hipLaunchKernelGGL(masked_l1_rgb_kernel, dim3((unsigned)nblk, (unsigned)batch), dim3(256), 0, rw_s(stream), a, b, mask,
                     mask_batch == 1 ? (int64_t)0 : hw, scratch, hw, per_thread);
  hipLaunchKernelGGL(lp_finish_kernel, dim3((unsigned)batch), dim3(256), 0, rw_s(stream), scratch, sums, nblk);
  return RW_LAUNCH_RESULT();
}
