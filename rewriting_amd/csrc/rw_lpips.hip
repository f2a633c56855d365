// LPIPS (v0.1, net-lin, vgg) behind the VGG16 taps, and the masked reductions of the edit distances -- what
// metrics/distances.py:18-59 (PerceptualLoss: lpips(spatial=True), sum(loss * w) / sum(w)) and :96-136 (compute_dl) run after the
// convolutions:
//
//   lpips_tap       d[b][p] = sum_c lin[c] (f0[b][c][p] / (|f0[b][:][p]| + 1e-10) - f1[..][c][p] / (|f1[..][:][p]| + 1e-10))^2 of one tap
//   lpips_combine   out[b][y][x] = sum_k bilinear(d_k)(y, x) (F.interpolate, align_corners=False, host tables) and / or, per image,
//                   (sum out w, sum w)
//   masked_l1_rgb   per image (sum_p mask sum_c |a - b|, sum_p mask): compute_dl's pixel mode (:131-133)
//   lpips_tap_grad, lpips_combine_grad   the adjoints of the first two to f0 and to the tap maps: LPIPS as a loss (lpips.LPIPS.loss)
//
// float32 only.  Every sum runs in a fixed order, no atomics, nothing zeroed beforehand, nothing but launches on the caller's
// stream: two runs give the same bits.  The distance of a tap is formed from the normalised DIFFERENCE as written above, never
// from the expansion sum w a^2 / |a|^2 + sum w b^2 / |b|^2 - 2 sum w a b / (|a| |b|): before and after pictures are nearly equal
// outside the edit, and the expansion cancels there.
#include "rw_common.h"

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

// the tile of a workgroup, as both tap kernels read it
struct LpTile {
  const float* f0; const float* f1; const float* lin;
  int ch, p_log2;
  int64_t hw, f1_stride, tiles_per_image;
};

// The tile view: where this workgroup's tile lies in LDS and in the two maps, and which (pixel, channel group) this thread is.
template <bool STAGED> struct LpTileView {
  const LpTile& p;
  float* t0; float* t1; float* red;              // the two staged maps [c][P] (STAGED) and the reduction floats behind them
  const float* g0; const float* g1;              // the tile's first pixel in channel 0 of f0 and f1
  int64_t b, p0, at0;                            // image, first pixel, and g0's offset: that of acc and out as well
  int P, G, valid, px, g;                        // valid: the tile's pixels inside the map; tid == g * P + px
  bool ok;                                       // px is one of them
  __device__ __forceinline__ LpTileView(const LpTile& tile_of, float* lds) : p(tile_of) {
    const int tid = threadIdx.x;
    P = 1 << p.p_log2;
    G = 256 >> p.p_log2;
    t0 = lds;
    t1 = t0 + (STAGED ? p.ch * P : 0);
    red = t1 + (STAGED ? p.ch * P : 0);
    const int64_t tile = blockIdx.x;
    b = tile / p.tiles_per_image;
    p0 = (tile - b * p.tiles_per_image) * P;
    at0 = b * p.ch * p.hw + p0;
    g0 = p.f0 + at0;
    g1 = p.f1 + b * p.f1_stride + p0;
    valid = (int)(p.hw - p0 < P ? p.hw - p0 : P);
    px = tid & (P - 1);
    g = tid >> p.p_log2;
    ok = px < valid;
  }
  __device__ __forceinline__ float a_of(int c) const {
    return STAGED ? t0[(c << p.p_log2) + px] : (ok ? g0[(int64_t)c * p.hw + px] : 0.f);
  }
  __device__ __forceinline__ float b_of(int c) const {
    return STAGED ? t1[(c << p.p_log2) + px] : (ok ? g1[(int64_t)c * p.hw + px] : 0.f);
  }
};

// The staging: both maps' ch x P values into t0 and t1, zeros past the map's end; ends behind a barrier.
template <bool V4> __device__ __forceinline__ void lp_stage(const LpTileView<true>& v) {
  const LpTile& p = v.p;
  const int tid = threadIdx.x;
  if (V4) {                                      // hw % 4 == 0 and P % 4 == 0: a quad is inside the map or outside it
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
        if (t < quads && 4 * q < v.valid) {
          a[j] = *reinterpret_cast<const float4*>(v.g0 + (int64_t)c * p.hw + 4 * q);
          bq[j] = *reinterpret_cast<const float4*>(v.g1 + (int64_t)c * p.hw + 4 * q);
        }
      }
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        const int t = t4 + 256 * j;
        if (t < quads) {
          reinterpret_cast<float4*>(v.t0)[t] = a[j];
          reinterpret_cast<float4*>(v.t1)[t] = bq[j];
        }
      }
    }
  } else {
    const int n = p.ch << p.p_log2;
    for (int t = tid; t < n; t += 256) {
      const int c = t >> p.p_log2, q = t & (v.P - 1);
      const bool ok = q < v.valid;
      v.t0[t] = ok ? v.g0[(int64_t)c * p.hw + q] : 0.f;
      v.t1[t] = ok ? v.g1[(int64_t)c * p.hw + q] : 0.f;
    }
  }
  __syncthreads();
}

// The group tree: every thread's partial sum(s) -- ROWS = 1: s0, ROWS = 2: s0 and s1 -- meet in red[r][tid] and are added
// pairwise over the channel groups; then red[r][px] holds the pixel's sum, behind a barrier.
template <int ROWS, bool STAGED>
__device__ __forceinline__ void lp_group_sum(const LpTileView<STAGED>& v, float s0, float s1 = 0.f) {
  const int tid = threadIdx.x;
  v.red[tid] = s0;                               // tid == g * P + px
  if (ROWS == 2) v.red[256 + tid] = s1;
  __syncthreads();
  for (int s = v.G >> 1; s > 0; s >>= 1) {
    if (v.g < s) {
      v.red[tid] += v.red[tid + (s << v.p.p_log2)];
      if (ROWS == 2) v.red[256 + tid] += v.red[256 + tid + (s << v.p.p_log2)];
    }
    __syncthreads();
  }
}

// The norms walk: (|f0|, |f1|) over the channels of this thread's pixel; red is free again when it returns.  (The square roots
// are taken here, in front of the barrier, where the kernels had them.)
template <bool STAGED> __device__ __forceinline__ void lp_norms(const LpTileView<STAGED>& v, float& r0, float& r1) {
  float s0 = 0.f, s1 = 0.f;
  for (int c = v.g; c < v.p.ch; c += v.G) {
    const float a = v.a_of(c), bv = v.b_of(c);
    s0 = fmaf(a, a, s0);
    s1 = fmaf(bv, bv, s1);
  }
  lp_group_sum<2>(v, s0, s1);
  r0 = sqrtf(v.red[v.px]);
  r1 = sqrtf(v.red[256 + v.px]);
  __syncthreads();
}

struct LpTap {
  LpTile t;
  float* d;
};

template <bool STAGED, bool V4>
__global__ void __launch_bounds__(256) lpips_tap_kernel(const LpTap p) {
  extern __shared__ __attribute__((aligned(16))) float lp_lds[];
  const LpTileView<STAGED> v(p.t, lp_lds);
  if constexpr (STAGED) lp_stage<V4>(v);
  float r0, r1;
  lp_norms(v, r0, r1);
  const float den0 = r0 + 1e-10f, den1 = r1 + 1e-10f;                    // a zero vector: 0 / (0 + eps) = 0
  float acc = 0.f;
  for (int c = v.g; c < p.t.ch; c += v.G) {
    const float t = v.a_of(c) / den0 - v.b_of(c) / den1;
    acc = fmaf(p.t.lin[c], t * t, acc);
  }
  lp_group_sum<1>(v, acc);
  if (v.g == 0 && v.ok) p.d[v.b * p.t.hw + v.p0 + v.px] = v.red[v.px];
}

// The tile choice and everything else of a launch that depends on the shapes alone.
struct LpTapShape {
  int64_t tiles;
  size_t lds_bytes;                              // the staged maps and red_floats behind them
  bool staged, v4;                               // v4: 16-byte staging is possible as far as f0, f1 and hw go
};

// fills t and s; an error code where the launch is refused
static int lp_tap_shape(const float* f0, const float* f1, const float* lin, int batch, int f1_batch, int ch, int64_t hw,
                        int red_floats, LpTile* t, LpTapShape* s) {
  const int dflt = 2 * (int64_t)ch * 32 <= LP_TILE_FLOATS ? LP_TILE_FLOATS : LP_WIDE_TILE_FLOATS;
  int tile = rw_env_int("RW_LPIPS_TILE", dflt);
  if (tile < 2 || tile > LP_MAX_TILE_FLOATS) tile = dflt;
  s->staged = 2 * (int64_t)ch <= tile;
  int p_log2 = 8;
  while (s->staged && p_log2 > 0 && 2 * (int64_t)ch << p_log2 > tile) --p_log2;
  while (p_log2 > 0 && (1 << (p_log2 - 1)) >= hw) --p_log2;              // a small map: more channel groups, fewer idle pixels
  t->f0 = f0; t->f1 = f1; t->lin = lin; t->ch = ch; t->p_log2 = p_log2; t->hw = hw;
  t->f1_stride = f1_batch == 1 ? 0 : (int64_t)ch * hw;
  t->tiles_per_image = rw_cdiv(hw, 1 << p_log2);
  s->tiles = t->tiles_per_image * batch;
  if (s->tiles > 0x7fffffff) return RW_ERR_UNSUPPORTED;
  s->lds_bytes = sizeof(float) * ((s->staged ? ((size_t)2 * ch << p_log2) : 0) + red_floats);
  s->v4 = s->staged && p_log2 >= 2 && hw % 4 == 0 && rw_aligned16(f0) && rw_aligned16(f1);
  return 0;
}

// kernel = the <STAGED, V4> instance of either tap kernel that s and v4 ask for
template <class P> static int lp_launch_tap(void (*kernel)(P), const P& p, const LpTapShape& s, rw_stream_t stream) {
  if (s.lds_bytes > 65536) {
    const hipError_t e = hipFuncSetAttribute((const void*)kernel, hipFuncAttributeMaxDynamicSharedMemorySize, (int)s.lds_bytes);
    if (e != hipSuccess) return (int)e;
  }
  hipLaunchKernelGGL(kernel, dim3((unsigned)s.tiles), dim3(256), s.lds_bytes, rw_s(stream), p);
  return RW_LAUNCH_RESULT();
}
#define LP_TAP_KERNEL(kernel, s, v4) (!(s).staged ? kernel<false, false> : (v4) ? kernel<true, true> : kernel<true, false>)

extern "C" int rw_lpips_tap_f32(const float* f0, const float* f1, const float* lin, float* d, int batch, int f1_batch, int ch,
                                int64_t hw, rw_stream_t stream) {
  RW_CHECK_ARG(f0 && f1 && lin && d && batch > 0 && ch > 0 && hw > 0 && (f1_batch == batch || f1_batch == 1));
  LpTap p;
  LpTapShape s;
  if (const int rc = lp_tap_shape(f0, f1, lin, batch, f1_batch, ch, hw, LP_RED_FLOATS, &p.t, &s)) return rc;
  p.d = d;
  return lp_launch_tap(LP_TAP_KERNEL(lpips_tap_kernel, s, s.v4), p, s, stream);
}

// ---------------------------------------------------------------------------------------
// The tap kernel's adjoint to f0 (LPIPS as a loss: lpips.LPIPS.loss).  With r0 = |f0|, den0 = r0 + 1e-10 (r1, den1 likewise),
// t_c = f0_c / den0 - f1_c / den1 -- the normalised DIFFERENCE as in the forward -- and S = sum_c lin_c t_c f0_c:
//   out[b][j][p] = acc[b][j][p] + gd[b][p] (2 / den0) (lin_j t_j - f0_j S / (r0 den0))
// The forward's tile, by its own pieces: lp_tap_shape chooses it, LpTileView and lp_stage lay it out, then THREE walks -- lp_norms,
// S (lp_group_sum<1>), the outputs.  The third walk is elementwise, so with 16-byte staging (V4) it takes lp_stage's
// own mapping, a thread per (channel, quad of pixels): acc is read and out written 16 bytes per lane; each element is read
// and written by one thread, so out may be acc.  A pixel with r0 == 0 contributes exactly 0: the formula's derivative there is
// a 1 / eps spike (torch's autograd of the formula returns NaN, sqrt'(0) 0), and inside the module every element of such a
// pixel is masked by its ReLU anyway.  relu_mask: an element with f0 <= 0 gets exactly acc (or 0) -- the taps are ReLU outputs,
// and the mask pass is saved.  Per pixel the third walk reads (den0, den1, k = gd 2 / den0, m = S / (r0 den0)) from LDS.
// ---------------------------------------------------------------------------------------
#define LP_GRAD_RED_FLOATS 1024              // [4][256]: the partial sums, then the four per-pixel values

struct LpTapGrad {
  LpTile t;
  const float* gd; const float* acc; float* out;
  int relu_mask;
};

__device__ __forceinline__ float lp_tap_grad_value(float a, float bv, float lin, float acc, float den0, float den1, float k,
                                                   float m, int relu_mask) {
#pragma clang fp contract(off)                   // own is rounded before it meets acc: with acc the result is acc + (the result without)
  if ((k == 0.f && m == 0.f) || (relu_mask && !(a > 0.f))) return acc;      // a dead pixel has k = m = 0
  const float t = a / den0 - bv / den1;
  const float own = k * (lin * t - a * m);
  return acc + own;
}

template <bool STAGED, bool V4>
__global__ void __launch_bounds__(256) lpips_tap_grad_kernel(const LpTapGrad p) {
  extern __shared__ __attribute__((aligned(16))) float lp_lds[];
  const LpTile& tl = p.t;
  const LpTileView<STAGED> v(tl, lp_lds);
  if constexpr (STAGED) lp_stage<V4>(v);
  // walk 1: the norms
  float r0, r1;
  lp_norms(v, r0, r1);
  const float den0 = r0 + 1e-10f, den1 = r1 + 1e-10f;
  // walk 2: S
  float acc = 0.f;
  for (int c = v.g; c < tl.ch; c += v.G) {
    const float a = v.a_of(c);
    const float t = a / den0 - v.b_of(c) / den1;
    acc = fmaf(tl.lin[c] * t, a, acc);
  }
  lp_group_sum<1>(v, acc);
  const float big_s = v.red[v.px];
  const bool live = v.ok && r0 > 0.f;
  const float k = live ? p.gd[v.b * tl.hw + v.p0 + v.px] * (2.f / den0) : 0.f;
  const float m = live ? big_s / r0 / den0 : 0.f;
  // walk 3: the outputs
  if (V4) {
    float* red = v.red;
    __syncthreads();                                           // every thread has read its S
    if (v.g == 0) {
      red[v.px] = den0;
      red[256 + v.px] = den1;
      red[512 + v.px] = k;
      red[768 + v.px] = m;
    }
    __syncthreads();
    const int q_log2 = tl.p_log2 - 2, quads = tl.ch << q_log2;
    for (int t = threadIdx.x; t < quads; t += 256) {
      const int c = t >> q_log2, q = t & ((1 << q_log2) - 1);
      if (4 * q >= v.valid) continue;                          // hw % 4 == 0: a quad is inside the map or outside it
      const float4 a = reinterpret_cast<const float4*>(v.t0)[t], bq = reinterpret_cast<const float4*>(v.t1)[t];
      const float4 d0 = reinterpret_cast<const float4*>(red)[q], d1 = reinterpret_cast<const float4*>(red + 256)[q];
      const float4 kq = reinterpret_cast<const float4*>(red + 512)[q], mq = reinterpret_cast<const float4*>(red + 768)[q];
      const int64_t at = v.at0 + (int64_t)c * tl.hw + 4 * q;
      float4 ac = make_float4(0.f, 0.f, 0.f, 0.f);
      if (p.acc) ac = *reinterpret_cast<const float4*>(p.acc + at);
      const float lin = tl.lin[c];
      float4 o;
      o.x = lp_tap_grad_value(a.x, bq.x, lin, ac.x, d0.x, d1.x, kq.x, mq.x, p.relu_mask);
      o.y = lp_tap_grad_value(a.y, bq.y, lin, ac.y, d0.y, d1.y, kq.y, mq.y, p.relu_mask);
      o.z = lp_tap_grad_value(a.z, bq.z, lin, ac.z, d0.z, d1.z, kq.z, mq.z, p.relu_mask);
      o.w = lp_tap_grad_value(a.w, bq.w, lin, ac.w, d0.w, d1.w, kq.w, mq.w, p.relu_mask);
      *reinterpret_cast<float4*>(p.out + at) = o;
    }
  } else if (v.ok) {
    for (int c = v.g; c < tl.ch; c += v.G) {
      const int64_t at = v.at0 + (int64_t)c * tl.hw + v.px;
      const float ac = p.acc ? p.acc[at] : 0.f;
      p.out[at] = lp_tap_grad_value(v.a_of(c), v.b_of(c), tl.lin[c], ac, den0, den1, k, m, p.relu_mask);
    }
  }
}

extern "C" int rw_lpips_tap_grad_f32(const float* f0, const float* f1, const float* lin, const float* gd, const float* acc,
                                     float* out, int batch, int f1_batch, int ch, int64_t hw, int relu_mask,
                                     rw_stream_t stream) {
  RW_CHECK_ARG(f0 && f1 && lin && gd && out && batch > 0 && ch > 0 && hw > 0 && (f1_batch == batch || f1_batch == 1));
  LpTapGrad p;
  LpTapShape s;
  if (const int rc = lp_tap_shape(f0, f1, lin, batch, f1_batch, ch, hw, LP_GRAD_RED_FLOATS, &p.t, &s)) return rc;
  p.gd = gd; p.acc = acc; p.out = out; p.relu_mask = relu_mask != 0;
  const bool v4 = s.v4 && rw_aligned16(out) && (!acc || rw_aligned16(acc));      // the third walk's 16-byte loads and stores
  return lp_launch_tap(LP_TAP_KERNEL(lpips_tap_grad_kernel, s, v4), p, s, stream);
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
// lpips_combine's adjoint to every tap map: a GATHER per tap pixel, no scatter.
//   gd_k[b][i][j] = gscale[b] sum_{oy in R_y(i)} wy(oy, i) sum_{ox in R_x(j)} wx(ox, j) weight[b'][oy][ox]
// with w(o, i) = (1 - lam_o) [i0_o == i] + lam_o [i1_o == i] from the forward's tables (clamped as there; both indices equal
// i: exactly 1) and R(i) = [lo, hi) the outputs that touch input i -- i0 and i1 do not decrease, so those are one run;
// lpips.adjoint_table makes (lo, hi) on the host.  rng holds, tap after tap, [row lo (h_k)] [row hi (h_k)] [column lo (w_k)]
// [column hi (w_k)]; the kernel clamps them into the output: a wrong table gives a wrong picture, never a read outside a map.
// A row's columns are summed first (one fused multiply-add each), then the rows: a term passes through |R_x| + |R_y|
// additions, its two weights' roundings and the product with gscale.  One thread per tap pixel, blockIdx.z the tap.
// ---------------------------------------------------------------------------------------
struct LpCombineGrad {
  rw_lpips_grad_maps m;
  const int* idx; const float* lam; const int* rng; const float* weight; const float* gscale;
  int64_t weight_stride;
  int h, w;
};

__device__ __forceinline__ float lp_adjoint_weight(int i0, int i1, float lam, int i) {
  return i0 == i ? (i1 == i ? 1.f : 1.f - lam) : (i1 == i ? lam : 0.f);
}

__global__ void __launch_bounds__(256) lpips_combine_grad_kernel(const LpCombineGrad p) {
  const int k = blockIdx.z, b = blockIdx.y;
  const int hk = p.m.h[k], wk = p.m.w[k];
  const int64_t at = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (at >= (int64_t)hk * wk) return;
  const int i = (int)(at / wk), j = (int)(at - (int64_t)i * wk);
  int64_t off = 0;
  for (int t = 0; t < k; ++t) off += 2 * ((int64_t)p.m.h[t] + p.m.w[t]);
  const int* rk = p.rng + off;
  const int* ik = p.idx + (int64_t)k * (2 * p.h + 2 * p.w);
  const float* lk = p.lam + (int64_t)k * (p.h + p.w);
  const int y_lo = lp_clamp(rk[i], p.h + 1), y_hi = lp_clamp(rk[hk + i], p.h + 1);
  const int x_lo = lp_clamp(rk[2 * hk + j], p.w + 1), x_hi = lp_clamp(rk[2 * hk + wk + j], p.w + 1);
  const float* wt = p.weight ? p.weight + b * p.weight_stride : nullptr;
  float v = 0.f;
  for (int oy = y_lo; oy < y_hi; ++oy) {
    float row = 0.f;
    for (int ox = x_lo; ox < x_hi; ++ox) {
      const float wx = lp_adjoint_weight(lp_clamp(ik[2 * p.h + ox], wk), lp_clamp(ik[2 * p.h + p.w + ox], wk), lk[p.h + ox], j);
      row = fmaf(wx, wt ? wt[(int64_t)oy * p.w + ox] : 1.f, row);
    }
    v = fmaf(lp_adjoint_weight(lp_clamp(ik[oy], hk), lp_clamp(ik[p.h + oy], hk), lk[oy], i), row, v);
  }
  p.m.d[k][(int64_t)b * hk * wk + at] = p.gscale[b] * v;
}

extern "C" int rw_lpips_combine_grad_f32(const rw_lpips_grad_maps* grads, const int* idx, const float* lam, const int* rng,
                                         const float* weight, int weight_batch, const float* gscale, int batch, int h, int w,
                                         rw_stream_t stream) {
  RW_CHECK_ARG(grads && idx && lam && rng && gscale && batch > 0 && h > 0 && w > 0);
  RW_CHECK_ARG(grads->n >= 1 && grads->n <= RW_LPIPS_MAX_TAPS);
  RW_CHECK_ARG(!weight || weight_batch == batch || weight_batch == 1);
  int64_t most = 0;
  for (int k = 0; k < grads->n; ++k) {
    RW_CHECK_ARG(grads->d[k] && grads->h[k] > 0 && grads->w[k] > 0);
    const int64_t n = (int64_t)grads->h[k] * grads->w[k];
    most = n > most ? n : most;
  }
  if (batch > 65535 || h == 0x7fffffff || w == 0x7fffffff || rw_cdiv(most, 256) > 0x7fffffff) return RW_ERR_UNSUPPORTED;
  LpCombineGrad p;
  p.m = *grads; p.idx = idx; p.lam = lam; p.rng = rng; p.weight = weight; p.gscale = gscale;
  p.weight_stride = weight && weight_batch == 1 ? 0 : (int64_t)h * w;
  p.h = h; p.w = w;
  hipLaunchKernelGGL(lpips_combine_grad_kernel, dim3((unsigned)rw_cdiv(most, 256), (unsigned)batch, (unsigned)grads->n), dim3(256),
                     0, rw_s(stream), p);
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
