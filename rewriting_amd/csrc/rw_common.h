// Shared helpers for the gfx950 kernels of librewriting_hip.so.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <stdlib.h>
#include "../../include/rewriting_hip.h"

#define RW_WAVE 64

#define RW_CHECK_ARG(cond) do { if (!(cond)) return RW_ERR_BAD_ARGUMENT; } while (0)
#define RW_LAUNCH_RESULT() ((int)hipGetLastError())

static inline hipStream_t rw_s(rw_stream_t s) { return (hipStream_t)s; }

static inline int64_t rw_cdiv(int64_t a, int64_t b) { return (a + b - 1) / b; }

// what a launcher asks of a pointer before it takes the kernel form with 16-byte loads or stores
static inline bool rw_aligned16(const void* p) { return ((uintptr_t)p & 15) == 0; }

// Compute units of the CURRENT device (queried once per device; 256 on a whole MI355X, fewer on a partitioned one): the
// workgroup count of the persistent kernels, which own a CU each.
static inline int rw_cu_count(void) {
  static int cached[64];
  int dev = 0;
  if (hipGetDevice(&dev) != hipSuccess || dev < 0 || dev >= 64) return 256;
  if (cached[dev] == 0) {
    int n = 0;
    cached[dev] = (hipDeviceGetAttribute(&n, hipDeviceAttributeMultiprocessorCount, dev) == hipSuccess && n > 0) ? n : 256;
  }
  return cached[dev];
}

// Grid for a memory-bound grid-stride kernel: enough blocks to fill 256 CUs x 8, no more.
static inline int rw_stream_grid(int64_t work_items, int block) {
  int64_t g = rw_cdiv(work_items, block);
  if (g > 256 * 8) g = 256 * 8;
  if (g < 1) g = 1;
  return (int)g;
}

// one 4-byte index inside an image's maps: what a kernel that indexes with an int asks of its launcher
static inline bool rw_fits_31(int64_t n) { return n > 0 && n < (1LL << 31); }

// The 64-lane butterfly, for any type __shfl_xor takes (float, double, the 4- and 8-byte integers); every lane ends
// with the result.
template <typename T> __device__ __forceinline__ T rw_wave_sum(T v) {
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) v += __shfl_xor(v, off, 64);
  return v;
}

__device__ __forceinline__ float rw_max2(float a, float b) { return fmaxf(a, b); }
__device__ __forceinline__ double rw_max2(double a, double b) { return fmax(a, b); }
template <typename T> __device__ __forceinline__ T rw_wave_max(T v) {
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) v = rw_max2(v, __shfl_xor(v, off, 64));
  return v;
}

// Block-wide sum for 256-thread blocks (4 waves); result valid in every thread.
template <typename T> __device__ __forceinline__ T rw_block_sum_256(T v, T* lds4) {
  v = rw_wave_sum(v);
  const int wave = threadIdx.x >> 6;
  __syncthreads();
  if ((threadIdx.x & 63) == 0) lds4[wave] = v;
  __syncthreads();
  return lds4[0] + lds4[1] + lds4[2] + lds4[3];
}

typedef float rw_f32x16 __attribute__((ext_vector_type(16)));
typedef float rw_f32x4 __attribute__((ext_vector_type(4)));
typedef float rw_f32x2 __attribute__((ext_vector_type(2)));
typedef unsigned rw_u32x2 __attribute__((ext_vector_type(2)));
typedef unsigned rw_u32x4 __attribute__((ext_vector_type(4)));
typedef int rw_i32x4 __attribute__((ext_vector_type(4)));
typedef _Float16 rw_f16x2 __attribute__((ext_vector_type(2)));
typedef _Float16 rw_f16x4 __attribute__((ext_vector_type(4)));
typedef _Float16 rw_f16x8 __attribute__((ext_vector_type(8)));

// Row of the 32x32 C/D tile of v_mfma_f32_32x32x* that accumulator register r (0 .. 15) of a lane holds; frow = lane >> 5,
// the column is lane & 31.
__host__ __device__ __forceinline__ constexpr int rw_mfma32_row(int r, int frow = 0) {
  return 4 * frow + (r & 3) + 8 * (r >> 2);
}

// leaky ReLU (slope 0.2) times sqrt 2: the activation behind every styled convolution's bias
__device__ __forceinline__ float rw_lrelu_sqrt2(float v) { return ((v > 0.f) ? v : v * 0.2f) * 1.4142135623730951f; }

// ---- halo staging of the direct fp32 convolutions (rw_conv.hip).  The XH x XUSED patch of input rows y0 - 1 .., columns
// x0 - 1 .. lies in LDS at row pitch XW > XUSED; thread tid of 256 stages the positions pos = tid + 256 k, and the rule is
// branch-free: a position outside the h x w image loads a legal address (offset 0) and multiplies by mask 0, a slot past
// the patch does the same and writes the padding column XW - 1 of row 0, which no tap reads.
__host__ __device__ __forceinline__ void rw_halo_slot_of(int pos, int y0, int x0, int h, int w, int XH, int XW, int XUSED,
                                                         int& goff, float& mask, int& lds) {
  const int NPOS = XH * XUSED;
  const int r = pos / XUSED, c = pos - r * XUSED;
  const int iy = y0 - 1 + r, ix = x0 - 1 + c;
  const bool ok = pos < NPOS && iy >= 0 && iy < h && ix >= 0 && ix < w;
  goff = ok ? iy * w + ix : 0;
  mask = ok ? 1.0f : 0.0f;
  lds = pos < NPOS ? r * XW + c : XW - 1;
}

// ---- the 3x3 convolution as a GEMM over gathered columns (the solver's K1 / K3 in rw_solve.hip, conv_wgrad_kernel in
// rw_grad.hip).  Extent, along one axis of n input samples, of the map the convolution writes: n for the stride-1 layer,
// 2n + 1 -- the pre-blur map -- for an upsampling layer (conv_transpose2d stride 2, utils/stylegan2/models.py:315-316).
__host__ __device__ static inline int rw_conv_extent(int upsample, int n) { return upsample ? 2 * n + 1 : n; }
// xcol[k = (i, tap)][position]: the sample of the h x w plane of channel i that weight tap (ky, kx) multiplies at
// conv-output position (Y, X); zero outside the plane (zero padding, pad 1; the solver's crop: quirk Q2) and, for the
// transposed convolution, where the parity of (Y - ky, X - kx) does not land on an input sample.
// p = the kernel's problem struct (its upsample, h, w).
template <class P> __device__ __forceinline__ float rw_conv_gather(const P& p, const float* plane, int tap, int Y, int X) {
  const int ky = tap / 3, kx = tap - 3 * ky;
  int iy, ix;
  if (p.upsample) {
    const int ty = Y - ky, tx = X - kx;
    if ((ty | tx) < 0 || ((ty | tx) & 1)) return 0.f;
    iy = ty >> 1; ix = tx >> 1;
  } else {
    iy = Y + ky - 1; ix = X + kx - 1;
  }
  if (iy < 0 || iy >= p.h || ix < 0 || ix >= p.w) return 0.f;
  return plane[iy * p.w + ix];
}

// a compile-time integer as a function argument (generic lambdas unrolled by hand)
template <int N> struct rw_int { static constexpr int value = N; };

// Workgroup id -> work item such that the workgroups of one XCD (ids congruent mod 8) take a contiguous run of items:
// neighbours in the map share their halo and their weights in that XCD's L2.
__device__ __forceinline__ int rw_xcd_remap(int id, int total) {
  const int q = total >> 3, r = total & 7;
  const int xcd = id & 7, slot = id >> 3;
  const int base = (xcd < r) ? xcd * (q + 1) : r * (q + 1) + (xcd - r) * q;
  return base + slot;
}

// ---- tiles of the direct-sum kernels (rw_dconv.hip, rw_tconv.hip): tile id = ((ib * tiles_y + ty) * tiles_x + tx) * o_tiles + ot
// -- ot fastest, so that the out-channel tiles of one window run back to back.  p = the kernel's problem struct; I = int or
// unsigned, the division the body was written with.
template <class I, class P>
__device__ __forceinline__ void rw_tile_digits(const P& p, I tile, int& ot, int& tx, int& ty, int& ib) {
  ot = (int)(tile % (I)p.o_tiles);
  I pg = tile / (I)p.o_tiles;
  tx = (int)(pg % (I)p.tiles_x); pg /= (I)p.tiles_x;
  ty = (int)(pg % (I)p.tiles_y);
  ib = (int)(pg / (I)p.tiles_y);
}
// The walk of a persistent workgroup, tile bx + k * grid for k = 0, 1, ...: the digits of tile bx once, then + the grid's
// digits per step, with carries (64-bit divisions per tile cost the staging waves 1.7 k cycles per chunk on layer 17:
// profiles/r05p)
template <class P> struct rw_tile_walk {
  const P& p;
  int g_ot, g_tx, g_ty, g_ib;                       // the digits of the grid size
  __device__ __forceinline__ explicit rw_tile_walk(const P& problem) : p(problem) {
    rw_tile_digits(p, (unsigned)gridDim.x, g_ot, g_tx, g_ty, g_ib);
  }
  __device__ __forceinline__ void advance(int& ot, int& tx, int& ty, int& ib) const {
    ot += g_ot;
    int carry = ot >= p.o_tiles ? 1 : 0;
    ot -= carry ? p.o_tiles : 0;
    tx += g_tx + carry;
    carry = tx >= p.tiles_x ? 1 : 0;
    tx -= carry ? p.tiles_x : 0;
    ty += g_ty + carry;
    carry = ty >= p.tiles_y ? 1 : 0;
    ty -= carry ? p.tiles_y : 0;
    ib += g_ib + carry;
  }
};

// ---- f16-pair operands of the direct-sum kernels (rw_dconv.hip, rw_tconv.hip)
// position of channel quad g inside the 64 bytes of window column cc: g ^ rw_swz(cc).  ds_read_b128 is serviced in the
// lane groups {0-3, 12-15, 20-27}, {4-11, 16-19, 28-31} (+ 32): with this swizzle the 16 lanes of every group -- 16 pixels of
// one quad in the MFMA operand order, at any of the three tap columns -- hit 16 distinct 16-byte slots of the 256-byte bank
// row (searched exhaustively; (cc >> 2) & 3 is 2-way: SQ_LDS_BANK_CONFLICT was 48 % of the LDS cycles), and the eight
// consecutive pixels of a ds_write_b128 group hit eight distinct slots of its 128-byte row.
__device__ __forceinline__ int rw_swz(int cc) { return (cc >> 1) & 3; }
// the operand [u0 u1 u2 u3 u0 u1 u2 u3] of the four halves in w
__device__ __forceinline__ rw_f16x8 rw_expand(rw_f32x2 w) {
  const rw_f32x4 d = {w[0], w[1], w[0], w[1]};
  return __builtin_bit_cast(rw_f16x8, d);
}
// [a0 a1 a2 a3 b0 b1 b2 b3]: the first four halves of two operands (their Vh parts) / two 4-half weight pieces
__device__ __forceinline__ rw_f16x8 rw_pair(rw_f16x8 a, rw_f16x8 b) {
  return rw_f16x8{a[0], a[1], a[2], a[3], b[0], b[1], b[2], b[3]};
}
__device__ __forceinline__ rw_f16x8 rw_pair(rw_f32x2 a, rw_f32x2 b) {
  const rw_f32x4 d = {a[0], a[1], b[0], b[1]};
  return __builtin_bit_cast(rw_f16x8, d);
}
// the pixel operand [h0 h1 h2 h3 | l0 l1 l2 l3] of four values (four input channels of a pixel): the exact split v = h + l + an
// error below 2^-22 |v|, h = f16(v), l = f16(v - h), both rounded to nearest; v - (float)h is exact in fp32 and costs one
// v_fma_mix_f32 reading the half where the conversion left it
__device__ __forceinline__ rw_f16x8 rw_split4(float v0, float v1, float v2, float v3) {
  const rw_f16x2 h01 = __builtin_convertvector(rw_f32x2{v0, v1}, rw_f16x2);
  const rw_f16x2 h23 = __builtin_convertvector(rw_f32x2{v2, v3}, rw_f16x2);
  float r0, r1, r2, r3;                            // v - (float)h, exact
  asm("v_fma_mix_f32 %0, -%1, 1.0, %2 op_sel_hi:[1,0,0]" : "=v"(r0) : "v"(h01), "v"(v0));
  asm("v_fma_mix_f32 %0, -%1, 1.0, %2 op_sel:[1,0,0] op_sel_hi:[1,0,0]" : "=v"(r1) : "v"(h01), "v"(v1));
  asm("v_fma_mix_f32 %0, -%1, 1.0, %2 op_sel_hi:[1,0,0]" : "=v"(r2) : "v"(h23), "v"(v2));
  asm("v_fma_mix_f32 %0, -%1, 1.0, %2 op_sel:[1,0,0] op_sel_hi:[1,0,0]" : "=v"(r3) : "v"(h23), "v"(v3));
  const rw_f16x2 l01 = __builtin_convertvector(rw_f32x2{r0, r1}, rw_f16x2);
  const rw_f16x2 l23 = __builtin_convertvector(rw_f32x2{r2, r3}, rw_f16x2);
  return rw_f16x8{h01[0], h01[1], h23[0], h23[1], l01[0], l01[1], l23[0], l23[1]};
}

// ---- LDS-direct loads as inline assembly: M0 = LDS byte address of the wave's 64 x size destination, lane L lands at
// + L * size
__device__ __forceinline__ void rw_dma_buffer_b32(unsigned lds_addr, int voffset, rw_i32x4 rsrc, int soffset) {
  asm volatile("s_mov_b32 m0, %0\n\ts_nop 0\n\tbuffer_load_dword %1, %2, %3 offen lds"
               :: "s"(lds_addr), "v"(voffset), "s"(rsrc), "s"(soffset) : "memory");
}
// 16 bytes per lane; voffset + soffset and lds_addr are multiples of 16, an out-of-range lane writes four zeros
__device__ __forceinline__ void rw_dma_buffer_b128(unsigned lds_addr, int voffset, rw_i32x4 rsrc, int soffset) {
  asm volatile("s_mov_b32 m0, %0\n\ts_nop 0\n\tbuffer_load_dwordx4 %1, %2, %3 offen lds"
               :: "s"(lds_addr), "v"(voffset), "s"(rsrc), "s"(soffset) : "memory");
}
__device__ __forceinline__ void rw_dma_global_b32(unsigned lds_addr, const void* gptr) {
  asm volatile("s_mov_b32 m0, %0\n\ts_nop 0\n\tglobal_load_lds_dword %1, off" :: "s"(lds_addr), "v"(gptr) : "memory");
}
// 16 bytes per lane from a scalar base and a 32-bit lane offset: no 64-bit vector address arithmetic per piece
__device__ __forceinline__ void rw_dma_global_b128_s(unsigned lds_addr, int voffset, const void* sbase) {
  asm volatile("s_mov_b32 m0, %0\n\ts_nop 0\n\tglobal_load_lds_dwordx4 %1, %2" :: "s"(lds_addr), "v"(voffset), "s"(sbase)
               : "memory");
}

// ---- the barrier between the roles of a specialised workgroup: LDS traffic waited for (lgkmcnt(0)), nothing else --
// vector loads and stores stay in flight across the barrier
__device__ __forceinline__ void rw_lds_barrier() {
  asm volatile("" ::: "memory");
  __builtin_amdgcn_s_waitcnt(0xC07F);
  __builtin_amdgcn_s_barrier();
  asm volatile("" ::: "memory");
}

// ---- buffer descriptor of the feature maps of image ib: in_ch planes of hw floats, range checked -- a lane offset past the
// end reads 0, which is the convolutions' zero padding
__device__ __forceinline__ __amdgpu_buffer_rsrc_t rw_image_rsrc(const float* x, int ib, int in_ch, int64_t hw) {
  return __builtin_amdgcn_make_buffer_rsrc(const_cast<float*>(x + (int64_t)ib * in_ch * hw), 0,
                                           (int)((int64_t)in_ch * hw * 4), 0x00020000);
}

// ---------------------------------------------------------------------------------------
// Bounds (max |map|) handed from a launch to the next one -- see "a BOUND on a map" in include/rewriting_hip.h.
// Round 4 kept them in 4-byte device scalars: zeroed by a memset, raised by the producer's workgroups with (filtered,
// system-scope) atomics, read by the consumer with a system-scope load.  Occasionally a consumer read a stale value
// (images 0.01 - 0.05 off; GPUTEST_r04).  Nothing of that mechanism is left: a producer's wave (or workgroup) stores its
// maximum PLAINLY into ITS OWN slot, rw_bound_finish() reduces the slots of the launch into RW_BOUND_LANES floats with
// one small launch, and a consumer's wave loads those floats with an ordinary per-lane vector load.  No location is
// written by more than one workgroup, nothing is zeroed first, every slot that is read was written by the launch in
// front: what orders it is what orders every feature map -- the launch boundary.
// ---------------------------------------------------------------------------------------
// slots a producer may use for a result of n floats (rw_bound_floats(n) - RW_BOUND_LANES)
static inline int64_t rw_bound_slot_capacity(int64_t n_elems) { return 2048 + n_elems / 1024 + 1; }

// host: bound[0 .. RW_BOUND_LANES) <- the maxima of bound[RW_BOUND_LANES .. RW_BOUND_LANES + nslots)   (rw_bound.hip)
int rw_bound_finish(float* bound, int64_t nslots, hipStream_t stream);

// consumer: the bound (uniform over the wave).  ALL 64 lanes of the wave must be active.
__device__ __forceinline__ float rw_bound_load(const float* __restrict__ bound) {
  return rw_wave_max(bound[threadIdx.x & 63]);
}

// producer, one slot per WAVE: slot = workgroup * waves per workgroup + wave.  v = the wave's maximum (any lane's copy
// of the reduced value); every wave of the launch must call it exactly once.
__device__ __forceinline__ void rw_bound_store_wave(float* __restrict__ bound, float v) {
  if ((threadIdx.x & 63) == 0)
    bound[RW_BOUND_LANES + (int64_t)blockIdx.x * (blockDim.x >> 6) + (threadIdx.x >> 6)] = v;
}

// producer, one slot per WORKGROUP of 256 threads: v = this thread's maximum; every thread of the workgroup calls it.
__device__ __forceinline__ void rw_bound_store_block_256(float* __restrict__ bound, float v, float* lds4) {
  v = rw_wave_max(v);
  __syncthreads();
  if ((threadIdx.x & 63) == 0) lds4[threadIdx.x >> 6] = v;
  __syncthreads();
  if (threadIdx.x == 0) bound[RW_BOUND_LANES + blockIdx.x] = fmaxf(fmaxf(lds4[0], lds4[1]), fmaxf(lds4[2], lds4[3]));
}

// ---- max |style| of image ib, the factor that turns the bound on x into one on x style (no style: 1); p = the kernel's problem
// struct (its style and in_ch are read where they are used, as the bodies read them).  Thread `first` of STRIDE takes the
// channels first, first + STRIDE, ..., then the wave reduces: with the default every lane ends with the maximum, with
// <64 * WAVES>(p, ib, tid) with its wave's share of it -- rw_block_max() is the rest.
template <int STRIDE = 64, class P> __device__ __forceinline__ float rw_style_absmax_wave(const P& p, int ib, int first) {
  float smax = p.style ? 0.f : 1.f;
  if (p.style)
    for (int i = first; i < p.in_ch; i += STRIDE) smax = fmaxf(smax, fabsf(p.style[(int64_t)ib * p.in_ch + i]));
  return rw_wave_max(smax);
}
// The maximum over a workgroup of WAVES waves of v, a value every wave has reduced already; every thread ends with it
// (red: in LDS; one barrier).  lane and wave are the caller's own: its wave index is wave-uniform by readfirstlane, one
// derived here would not be.  (Called beside rw_style_absmax_wave, not from inside a helper that does both: nested, the
// compiler orders the bodies' instructions differently.)
template <int WAVES> __device__ __forceinline__ float rw_block_max(float v, int lane, int wave, float (&red)[WAVES]) {
  if (lane == 0) red[wave] = v;
  __syncthreads();
  v = red[0];
#pragma unroll
  for (int k = 1; k < WAVES; ++k) v = fmaxf(v, red[k]);
  return v;
}

// ---- the scale rule of the split-operand kernels, stated once for the host and every kernel body.
// e with x < 2^e, from the exponent field alone and clamped to +-100, so that 2^(+-(HEAD - e)) is a normal float whatever
// x is: zero and the denormals give -100, infinity and NaN 100.
__host__ __device__ __forceinline__ int rw_exp_above(float x) {
  const int e = (int)((__builtin_bit_cast(unsigned, x) >> 23) & 0xff) - 126;      // x < 2^e
  return e < -100 ? -100 : (e > 100 ? 100 : e);
}
// am >= max |x style| (a bound on x times the largest |style|), am < 2^e: in_scale = 2^(HEAD - e) rides in the style table,
// so that |V| = |x style in_scale| < 2^HEAD -- HEAD = 14 where V itself is split, less by the gain of the transform where
// one comes between (each site says which); out_scale = 2^(e - HEAD) / u_scale takes both scales off the result.
template <int HEAD>
__host__ __device__ __forceinline__ void rw_split_scales(float am, float u_inv, float& in_scale, float& out_scale) {
  const int e = rw_exp_above(am);
  in_scale = __builtin_bit_cast(float, (unsigned)(127 + HEAD - e) << 23);
  out_scale = __builtin_bit_cast(float, (unsigned)(127 + e - HEAD) << 23) * u_inv;
}
// u_scale = 2^(15 - e), max |U| < 2^e; 1 for all-zero weights  (rw_split_weight_scale in the header; one definition for
// host and tests)
static inline float rw_weight_scale_of(float u_absmax) {
  const int eu = u_absmax == 0.f ? 15 : rw_exp_above(u_absmax);
  return __builtin_bit_cast(float, (unsigned)(127 + 15 - eu) << 23);
}

// ---- the running RGB image upsampled where it is consumed (rgb_combine_up_kernel, the F(4x4) ToRGB epilogues).
// acc[e] = output (oy, ox + e), e = 0..3, ox % 4 == 0, of upfirdn2d(up 2, 4 x 4 kernel, pads 2 / 1) of the hh x hw plane xm --
// with the bits of upfirdn2d_up2k4_kernel (rw_ops.hip): from 0, kernel rows a ascending, then kernel columns c ascending,
// taps outside the plane skipped (not added as zeros), every step the one expression acc += x * k.  kf: the 4 x 4 kernel as
// stored; the taps are read flipped.  Output row oy takes the kernel rows a = (oy & 1), (oy & 1) + 2 at the input rows
// (oy + a - 2) >> 1; output column ox + e the kernel columns c = (e & 1), (e & 1) + 2 at the input columns
// (ox + e + c - 2) >> 1 = m - 1 + (e + c) / 2 with m = ox / 2: four input columns m - 1 .. m + 2 of two rows.
__device__ __forceinline__ void rw_up2k4_row4(const float* __restrict__ xm, int hh, int hw, int oy, int ox,
                                              const float* __restrict__ kf, float (&acc)[4]) {
  acc[0] = acc[1] = acc[2] = acc[3] = 0.f;
  const int m = ox >> 1;                          // m + 1 <= hw - 1: the output is 2 hw wide and ox + 4 <= 2 hw
  const bool okl = m >= 1, okr = m + 2 < hw;
#pragma unroll
  for (int j = 0; j < 2; ++j) {
    const int vy = oy + (oy & 1) + 2 * j - 2, iy = vy >> 1;
    const bool row = vy >= 0 && iy < hh;
    // no branches: a skipped tap is a step whose result is not taken, read from a clamped address
    const float* xr = xm + (int64_t)(row ? iy : 0) * hw + m;
    // flipped: tap (a, c) is kf[3 - a][3 - c], a = (oy & 1) + 2 j.  Read per lane where they are used (the row depends on
    // the lane): sixteen taps kept in scalar registers across an F(4x4) kernel's main loop cost it spills
    const float* kr = kf + 4 * (3 - (oy & 1) - 2 * j);
    const float k0 = kr[3], k1 = kr[2], k2 = kr[1], k3 = kr[0];
    const float xl = xr[okl ? -1 : 0], x0 = xr[0], x1 = xr[1], x2 = xr[okr ? 2 : 1];
    float t[4] = {acc[0], acc[1], acc[2], acc[3]};
    t[0] += xl * k0;
    t[0] = okl ? t[0] : acc[0];
    t[0] += x0 * k2;
    t[1] += x0 * k1;
    t[1] += x1 * k3;
    t[2] += x0 * k0;
    t[2] += x1 * k2;
    t[3] += x1 * k1;
    float u = t[3];
    u += x2 * k3;
    t[3] = okr ? u : t[3];
#pragma unroll
    for (int e = 0; e < 4; ++e) acc[e] = row ? t[e] : acc[e];
  }
}

// ---------------------------------------------------------------------------------------
// The host prologue of the convolution entries: what every launcher checks, copies and finishes with.
// ---------------------------------------------------------------------------------------
// noise needs its weight, the activation its bias
static inline bool rw_epilogue_ok(const rw_conv_epilogue* ep) {
  return !ep || ((!ep->noise || ep->noise_w) && (!ep->act || ep->bias));
}
// a ToRGB block needs its weight, its style and somewhere to write (bias and skip are optional)
static inline bool rw_rgb_ok(const rw_rgb_epilogue* rgb) { return rgb && rgb->weight && rgb->style && rgb->out; }

// the epilogue's fields into the same-named fields of a kernel's problem struct (ep == nullptr: none)
template <class P> static inline void rw_fill_epilogue(P& p, const rw_conv_epilogue* ep) {
  p.style = ep ? ep->style : nullptr; p.demod = ep ? ep->demod : nullptr; p.noise = ep ? ep->noise : nullptr;
  p.noise_w = ep ? ep->noise_w : nullptr; p.bias = ep ? ep->bias : nullptr; p.act = ep ? ep->act : 0;
}
template <class P> static inline void rw_fill_rgb(P& p, const rw_rgb_epilogue* rgb) {
  p.rgb_weight = rgb ? rgb->weight : nullptr; p.rgb_style = rgb ? rgb->style : nullptr;
  p.rgb_bias = rgb ? rgb->bias : nullptr; p.rgb_skip = rgb ? rgb->skip : nullptr; p.rgb_out = rgb ? rgb->out : nullptr;
  p.rgb_scale = rgb ? rgb->scale : 0.f;
}

// after a launch whose waves (or workgroups) stored their maxima into nslots slots: the launch's status, then the bound
// of the result where the caller wants one
static inline int rw_finish_bound(float* y_amax, int64_t nslots, rw_stream_t stream) {
  const int rc = RW_LAUNCH_RESULT();
  if (rc || !y_amax) return rc;
  return rw_bound_finish(y_amax, nslots, rw_s(stream));
}

// tuning switches of the environment, read where they are called (per launch: the tests flip them)
static inline int rw_env_int(const char* name, int dflt) { const char* e = getenv(name); return e ? atoi(e) : dflt; }
static inline bool rw_env_is(const char* name, char ch) { const char* e = getenv(name); return e && e[0] == ch; }

// Tile groups along x per workgroup: `wanted`, clamped to 1 .. groups_x, lowered until it divides groups_x, then lowered
// further while the launch -- other_work (batch x group rows x out-channel tiles) x groups_x / gpw -- has fewer than
// min_workgroups workgroups.
static inline int rw_groups_per_wg(int groups_x, int64_t other_work, int wanted, int64_t min_workgroups) {
  int gpw = wanted < 1 ? 1 : (wanted > groups_x ? groups_x : wanted);
  while (groups_x % gpw) --gpw;
  while (gpw > 1 && other_work * (groups_x / gpw) < min_workgroups) {
    --gpw;
    while (groups_x % gpw) --gpw;
  }
  return gpw;
}
