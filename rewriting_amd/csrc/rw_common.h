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

__device__ __forceinline__ float rw_wave_sum(float v) {
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) v += __shfl_xor(v, off, 64);
  return v;
}

__device__ __forceinline__ float rw_wave_max(float v) {
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) v = fmaxf(v, __shfl_xor(v, off, 64));
  return v;
}

// Block-wide sum for 256-thread blocks (4 waves); result valid in every thread.
__device__ __forceinline__ float rw_block_sum_256(float v, float* lds4) {
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

// ---- LDS-direct loads as inline assembly: M0 = LDS byte address of the wave's 64 x size destination, lane L lands at
// + L * size
__device__ __forceinline__ void rw_dma_buffer_b32(unsigned lds_addr, int voffset, rw_i32x4 rsrc, int soffset) {
  asm volatile("s_mov_b32 m0, %0\n\ts_nop 0\n\tbuffer_load_dword %1, %2, %3 offen lds"
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

// u_scale = 2^(15 - e), max |U| < 2^e  (rw_split_weight_scale in the header; one definition for host and tests)
static inline float rw_weight_scale_of(float u_absmax) {
  union { float f; unsigned u; } b;
  b.f = u_absmax;
  int eu = (int)((b.u >> 23) & 0xff) - 126;
  if ((b.u & 0x7fffffffu) == 0u) eu = 15;
  eu = eu < -100 ? -100 : (eu > 100 ? 100 : eu);
  b.u = (unsigned)(127 + 15 - eu) << 23;
  return b.f;
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
