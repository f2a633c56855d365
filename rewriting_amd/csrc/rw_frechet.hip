// hipcc-flags: -fno-slp-vectorize
// The Frechet distance on the device (metrics/fid.py:60-61,137-187): a float64 block one-sided (Hestenes) Jacobi
// eigensolver for symmetric PSD matrices, a small f64 GEMM, and the fixed-order sums that finish the distance.
//
//   Tr sqrt(S1 S2) = sum_i sqrt(mu_i(F^T S2 F)),  S1 = F F^T,  F = V diag(sqrt(lambda)),  S1 V = V diag(lambda)
//
// Storage: every working array is n x n row-major with ROW j = COLUMN j of the matrix the text speaks of (G, V): a
// workgroup that owns 2 B columns streams 2 B contiguous rows.  G starts as S (symmetric: its rows are its columns), V
// as I; at convergence the columns of G = S V are orthogonal, their norms are the eigenvalues and V holds the vectors.
//
// One launch of jacobi_step_f64_kernel is one step of the circle-method round robin over the n / B column blocks (every
// block meets every other once in blocks - 1 steps, blocks rounded up to even; the block that meets the dummy has a bye).
// Workgroup k of step r owns the pair rw_circle_pair(blocks, r, k) and
//   1. streams its 2 B columns once and forms their Gram matrix A = P P^T on v_mfma_f64_16x16x4_f64 (four waves take the
//      16-column chunks in turn; their partial sums are added in the order of the waves), refusing a non-finite value;
//   2. diagonalises A in LDS by at most RW_JACOBI_INNER_SWEEPS cyclic two-sided Jacobi sweeps (the same circle method
//      over the 2 B columns, B disjoint rotations per round), the rotations accumulated from the identity, so that Q is the
//      factor closest to I; then orders the columns of Q by decreasing diagonal of Q^T A Q (de Rijk: the large columns first);
//   3. applies P <- Q^T P to its rows of G and of V in a second pass on the same MFMA, in place (a wave reads all 2 B rows
//      of a 16-column chunk before it writes them, and no other wave touches that chunk).
// The rotation rule, the tolerance and the noise floor are RW_JACOBI_TOL / RW_JACOBI_FLOOR of the header.  No atomics,
// no workgroup waits for another; each writes its rotation count (-1: non-finite input) to its own slot with a plain
// store.  The sweep loop is the host's.
#include <float.h>
#include "rw_common.h"

typedef double rw_f64x4 __attribute__((ext_vector_type(4)));

#define RW_JACOBI_INNER_SWEEPS 10

// pair k of round r of the circle method over `count` players (count rounded up to even; hi >= count: a bye)
__host__ __device__ __forceinline__ void rw_circle_pair(int count, int r, int k, int& lo, int& hi) {
  const int m = count + (count & 1);
  int i, j;
  if (k == 0) { i = m - 1; j = r; } else { i = (r + k) % (m - 1); j = (r - k + (m - 1)) % (m - 1); }
  lo = i < j ? i : j;
  hi = i < j ? j : i;
}

// ---------------------------------------------------------------------------------------
// The block Jacobi step
// ---------------------------------------------------------------------------------------
template <int B>
__global__ void __launch_bounds__(256) jacobi_step_f64_kernel(double* __restrict__ g, double* __restrict__ v, int n,
                                                              int blocks, int step, const double* __restrict__ norms_sq,
                                                              double tol, double floor_sq, int* __restrict__ slots) {
  constexpr int W = 2 * B, T = W / 16, LD = W + 1, HALF = W / 2;
  __shared__ double part[4][W][W];         // the waves' partial Gram sums
  __shared__ double A[W][LD], Q[W][LD];
  __shared__ double rc[HALF], rs[HALF];
  __shared__ int rp[HALF], rq[HALF], inv[W];
  __shared__ double red[4];
  __shared__ int flags[4];                 // 0: non-finite input; 1: rotations of this inner sweep; 2: of this round; 3: order changed
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int r16 = lane & 15, q4 = lane >> 4;

  int bi, bj;
  rw_circle_pair(blocks, step, (int)blockIdx.x, bi, bj);
  if (bj >= blocks) {                      // the bye of an odd block count
    if (tid == 0) slots[blockIdx.x] = 0;
    return;
  }
  // local column 0 .. W-1 -> row of the arrays
  auto grow = [&](int r) -> int64_t { return r < B ? (int64_t)bi * B + r : (int64_t)bj * B + (r - B); };

  // the largest squared column norm of the input: what the noise floor is relative to
  double mx = 0.0;
  for (int j = tid; j < n; j += 256) mx = fmax(mx, norms_sq[j]);
  mx = rw_wave_max(mx);
  if (lane == 0) red[wave] = mx;
  if (tid < 4) flags[tid] = 0;
  __syncthreads();
  const double floor_abs = floor_sq * fmax(fmax(red[0], red[1]), fmax(red[2], red[3]));

  // ---- 1. the Gram matrix.  Lane (r16, q4) loads columns 16 c + 4 q4 .. + 3 of row r16 of each 16-row tile: k-step s of
  // the chunk sums over the columns 16 c + 4 q + s, q = 0 .. 3 -- the same four for both operands.
  rw_f64x4 acc[T][T];
#pragma unroll
  for (int i = 0; i < T; ++i)
#pragma unroll
    for (int j = 0; j < T; ++j) acc[i][j] = rw_f64x4{0.0, 0.0, 0.0, 0.0};
  bool finite = true;
  const int chunks = (n + 15) >> 4;
  for (int c = wave; c < chunks; c += 4) {
    const int col = 16 * c + 4 * q4;       // n % 4 == 0: a group of four is inside the row or past it
    rw_f64x4 x[T];
#pragma unroll
    for (int i = 0; i < T; ++i) {
      x[i] = rw_f64x4{0.0, 0.0, 0.0, 0.0};
      if (col < n) x[i] = *(const rw_f64x4*)(g + grow(16 * i + r16) * n + col);
#pragma unroll
      for (int e = 0; e < 4; ++e) finite = finite && (fabs(x[i][e]) <= DBL_MAX);     // false for NaN and for infinity
    }
#pragma unroll
    for (int s = 0; s < 4; ++s)
#pragma unroll
      for (int i = 0; i < T; ++i)
#pragma unroll
        for (int j = 0; j < T; ++j) acc[i][j] = __builtin_amdgcn_mfma_f64_16x16x4f64(x[i][s], x[j][s], acc[i][j], 0, 0, 0);
  }
  // result reg of a lane: row q4 + 4 reg, column r16 of the tile (the f64 map)
#pragma unroll
  for (int i = 0; i < T; ++i)
#pragma unroll
    for (int j = 0; j < T; ++j)
#pragma unroll
      for (int r = 0; r < 4; ++r) part[wave][16 * i + q4 + 4 * r][16 * j + r16] = acc[i][j][r];
  if (!finite) flags[0] = 1;               // every writer stores the same value
  __syncthreads();
  if (flags[0]) {
    if (tid == 0) slots[blockIdx.x] = -1;
    return;
  }
  for (int idx = tid; idx < W * W; idx += 256) {
    const int i = idx / W, j = idx % W;
    A[i][j] = ((part[0][i][j] + part[1][i][j]) + part[2][i][j]) + part[3][i][j];
    Q[i][j] = i == j ? 1.0 : 0.0;
  }
  __syncthreads();

  // ---- 2. the inner solve
  int total = 0;
  for (int sw = 0; sw < RW_JACOBI_INNER_SWEEPS; ++sw) {
    for (int r = 0; r < W - 1; ++r) {
      if (tid < HALF) {                    // all in wave 0
        int p, q;
        rw_circle_pair(W, r, tid, p, q);
        const double app = A[p][p], aqq = A[q][q], apq = A[p][q];
        // sqrt(a) sqrt(b), not sqrt(a b): the product of two squared norms of large inputs overflows
        const double thr = tol * sqrt(fmax(app, 0.0)) * sqrt(fmax(aqq, 0.0));
        const bool rotate = fabs(apq) > thr && fmax(app, aqq) > floor_abs;
        double c = 1.0, s = 0.0;
        if (rotate) {
          const double zeta = (aqq - app) / (2.0 * apq);
          const double t = copysign(1.0, zeta) / (fabs(zeta) + sqrt(1.0 + zeta * zeta));      // the smaller root: |t| <= 1
          c = 1.0 / sqrt(1.0 + t * t);
          s = c * t;
        }
        rc[tid] = c; rs[tid] = s; rp[tid] = p; rq[tid] = q;
        const int nrot = __popcll(__ballot(rotate));
        if (tid == 0) { flags[2] = nrot; flags[1] += nrot; }
      }
      __syncthreads();
      if (flags[2]) {                      // uniform over the workgroup
        // columns p, q of A and of Q
        for (int idx = tid; idx < W * HALF; idx += 256) {
          const int i = idx / HALF, t = idx % HALF;
          const int p = rp[t], q = rq[t];
          const double c = rc[t], s = rs[t];
          const double ap = A[i][p], aq = A[i][q];
          A[i][p] = c * ap - s * aq;
          A[i][q] = s * ap + c * aq;
          const double qp = Q[i][p], qq = Q[i][q];
          Q[i][p] = c * qp - s * qq;
          Q[i][q] = s * qp + c * qq;
        }
        __syncthreads();
        // rows p, q of A
        for (int idx = tid; idx < W * HALF; idx += 256) {
          const int t = idx / W, j = idx % W;
          const int p = rp[t], q = rq[t];
          const double c = rc[t], s = rs[t];
          const double ap = A[p][j], aq = A[q][j];
          A[p][j] = c * ap - s * aq;
          A[q][j] = s * ap + c * aq;
        }
      }
      __syncthreads();
    }
    const int live = flags[1];
    total += live;
    __syncthreads();
    if (tid == 0) flags[1] = 0;
    if (!live) break;
  }
  __syncthreads();

  // the order: column i goes to position rank(i) = how many diagonal entries are larger (ties: the lower index first)
  if (tid < W) {
    const double d = A[tid][tid];
    int rank = 0;
    for (int j = 0; j < W; ++j) {
      const double e = A[j][j];
      rank += (e > d || (e == d && j < tid)) ? 1 : 0;
    }
    inv[rank] = tid;
    const unsigned long long moved = __ballot(rank != tid);
    if (tid == 0) flags[3] = moved != 0ULL;
  }
  __syncthreads();
  if (tid == 0) slots[blockIdx.x] = total;
  if (total == 0 && !flags[3]) return;     // nothing to apply

  // ---- 3. P <- Qp^T P, Qp[k][i'] = Q[k][inv[i']]: A operand lane (r16, q4) = Qp[4 kk + q4][16 i + r16], B operand =
  // P[4 kk + q4][column r16 of the chunk]
  double qa[T][W / 4];
#pragma unroll
  for (int i = 0; i < T; ++i)
#pragma unroll
    for (int kk = 0; kk < W / 4; ++kk) qa[i][kk] = Q[4 * kk + q4][inv[16 * i + r16]];
  for (int m = 0; m < 2; ++m) {
    double* __restrict__ x = m ? v : g;
    if (!x) continue;
    for (int c = wave; c < chunks; c += 4) {
      const int col = 16 * c + r16;
      const bool ok = col < n;
      double xb[W / 4];
#pragma unroll
      for (int kk = 0; kk < W / 4; ++kk) xb[kk] = ok ? x[grow(4 * kk + q4) * n + col] : 0.0;
      rw_f64x4 d[T];
#pragma unroll
      for (int i = 0; i < T; ++i) {
        d[i] = rw_f64x4{0.0, 0.0, 0.0, 0.0};
#pragma unroll
        for (int kk = 0; kk < W / 4; ++kk) d[i] = __builtin_amdgcn_mfma_f64_16x16x4f64(qa[i][kk], xb[kk], d[i], 0, 0, 0);
      }
      if (ok) {
#pragma unroll
        for (int i = 0; i < T; ++i)
#pragma unroll
          for (int r = 0; r < 4; ++r) x[grow(16 * i + q4 + 4 * r) * n + col] = d[i][r];
      }
    }
  }
}

static inline bool rw_aligned32(const void* p) { return ((uintptr_t)p & 31) == 0; }

extern "C" int rw_jacobi_step_f64(double* g, double* v, int n, int block, int step, const double* norms_sq, int* slots,
                                  rw_stream_t stream) {
  RW_CHECK_ARG(g && norms_sq && slots && (block == 8 || block == 16) && n >= 2 * block && n % block == 0);
  const int blocks = n / block, m = blocks + (blocks & 1);
  RW_CHECK_ARG(step >= 0 && step < m - 1);
  if (!rw_aligned32(g) || (v && !rw_aligned32(v))) return RW_ERR_UNSUPPORTED;
  const double tol = RW_JACOBI_TOL(n), floor = RW_JACOBI_FLOOR(n);
  if (block == 8)
    hipLaunchKernelGGL(jacobi_step_f64_kernel<8>, dim3(m / 2), dim3(256), 0, rw_s(stream), g, v, n, blocks, step,
                       norms_sq, tol, floor * floor, slots);
  else
    hipLaunchKernelGGL(jacobi_step_f64_kernel<16>, dim3(m / 2), dim3(256), 0, rw_s(stream), g, v, n, blocks, step,
                       norms_sq, tol, floor * floor, slots);
  return RW_LAUNCH_RESULT();
}

// the rotation slots of a sweep: out[0] = their sum, out[1] = how many say "non-finite input"
__global__ void __launch_bounds__(256) jacobi_count_kernel(const int* __restrict__ slots, int64_t nslots,
                                                           long long* __restrict__ out) {
  __shared__ long long sum[256], bad[256];
  long long s = 0, b = 0;
  for (int64_t i = threadIdx.x; i < nslots; i += 256) {
    const int c = slots[i];
    if (c < 0) ++b; else s += c;
  }
  sum[threadIdx.x] = s; bad[threadIdx.x] = b;
  __syncthreads();
  if (threadIdx.x == 0) {
    for (int t = 1; t < 256; ++t) { s += sum[t]; b += bad[t]; }
    out[0] = s; out[1] = b;
  }
}

extern "C" int rw_jacobi_count_i32(const int* slots, int64_t nslots, long long* out, rw_stream_t stream) {
  RW_CHECK_ARG(slots && out && nslots > 0);
  hipLaunchKernelGGL(jacobi_count_kernel, dim3(1), dim3(256), 0, rw_s(stream), slots, nslots, out);
  return RW_LAUNCH_RESULT();
}

// ---------------------------------------------------------------------------------------
// Column norms (rows of the arrays): one wave per row, lane-strided partial sums, then the butterfly -- a fixed order.
// mode 0: the norm (the eigenvalue); 1: its square (what the noise floor is relative to); 2: its square root (the scale
// of F = V diag(sqrt(lambda)))
// ---------------------------------------------------------------------------------------
__global__ void __launch_bounds__(256) colnorm_f64_kernel(const double* __restrict__ g, double* __restrict__ out, int n,
                                                          int mode) {
  const int row = blockIdx.x * 4 + (threadIdx.x >> 6), lane = threadIdx.x & 63;
  if (row >= n) return;
  const double* gr = g + (int64_t)row * n;
  double acc = 0.0;
  for (int i = lane; i < n; i += 64) { const double x = gr[i]; acc += x * x; }
  acc = rw_wave_sum(acc);
  if (lane == 0) out[row] = mode == 1 ? acc : (mode == 2 ? sqrt(sqrt(acc)) : sqrt(acc));
}

extern "C" int rw_colnorm_f64(const double* g, double* out, int n, int mode, rw_stream_t stream) {
  RW_CHECK_ARG(g && out && n > 0 && mode >= 0 && mode <= 2);
  hipLaunchKernelGGL(colnorm_f64_kernel, dim3((n + 3) / 4), dim3(256), 0, rw_s(stream), g, out, n, mode);
  return RW_LAUNCH_RESULT();
}

// ---------------------------------------------------------------------------------------
// C = diag(row_scale) op(A) op(B) diag(col_scale), row-major, on v_mfma_f64_16x16x4_f64.  A workgroup takes a 64 x 64 tile
// (a wave 32 x 32 of it), K in chunks of 16 staged in LDS, edges zero-filled on load and masked on store; no split of K,
// so the order of every sum is fixed.
// ---------------------------------------------------------------------------------------
#define RW_GEMM64_PITCH 80      // rows of the four k of an operand start 32 banks apart

template <bool TA, bool TB>
__global__ void __launch_bounds__(256) gemm_f64_kernel(const double* __restrict__ a, const double* __restrict__ b,
                                                       double* __restrict__ c, int m, int n, int k,
                                                       const double* __restrict__ row_scale,
                                                       const double* __restrict__ col_scale) {
  __shared__ double as[16][RW_GEMM64_PITCH], bs[16][RW_GEMM64_PITCH];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int r16 = lane & 15, q4 = lane >> 4;
  const int bm = blockIdx.y * 64, bn = blockIdx.x * 64;
  const int wm = (wave >> 1) * 32, wn = (wave & 1) * 32;
  rw_f64x4 acc[2][2];
#pragma unroll
  for (int i = 0; i < 2; ++i)
#pragma unroll
    for (int j = 0; j < 2; ++j) acc[i][j] = rw_f64x4{0.0, 0.0, 0.0, 0.0};
  for (int k0 = 0; k0 < k; k0 += 16) {
    __syncthreads();
#pragma unroll
    for (int e = 0; e < 4; ++e) {
      const int idx = tid + 256 * e;
      {                                    // op(A)[i][kk]: consecutive threads along the stored rows
        const int i = TA ? idx % 64 : idx / 16, kk = TA ? idx / 64 : idx % 16;
        const int gi = bm + i, gk = k0 + kk;
        as[kk][i] = (gi < m && gk < k) ? (TA ? a[(int64_t)gk * m + gi] : a[(int64_t)gi * k + gk]) : 0.0;
      }
      {                                    // op(B)[kk][j]
        const int j = TB ? idx / 16 : idx % 64, kk = TB ? idx % 16 : idx / 64;
        const int gj = bn + j, gk = k0 + kk;
        bs[kk][j] = (gj < n && gk < k) ? (TB ? b[(int64_t)gj * k + gk] : b[(int64_t)gk * n + gj]) : 0.0;
      }
    }
    __syncthreads();
#pragma unroll
    for (int ks = 0; ks < 4; ++ks) {
      const int kk = 4 * ks + q4;
      const double a0 = as[kk][wm + r16], a1 = as[kk][wm + 16 + r16];
      const double b0 = bs[kk][wn + r16], b1 = bs[kk][wn + 16 + r16];
      acc[0][0] = __builtin_amdgcn_mfma_f64_16x16x4f64(a0, b0, acc[0][0], 0, 0, 0);
      acc[0][1] = __builtin_amdgcn_mfma_f64_16x16x4f64(a0, b1, acc[0][1], 0, 0, 0);
      acc[1][0] = __builtin_amdgcn_mfma_f64_16x16x4f64(a1, b0, acc[1][0], 0, 0, 0);
      acc[1][1] = __builtin_amdgcn_mfma_f64_16x16x4f64(a1, b1, acc[1][1], 0, 0, 0);
    }
  }
#pragma unroll
  for (int i = 0; i < 2; ++i)
#pragma unroll
    for (int j = 0; j < 2; ++j)
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const int row = bm + wm + 16 * i + q4 + 4 * r, col = bn + wn + 16 * j + r16;
        if (row < m && col < n) {
          double val = acc[i][j][r];
          if (row_scale) val *= row_scale[row];
          if (col_scale) val *= col_scale[col];
          c[(int64_t)row * n + col] = val;
        }
      }
}

extern "C" int rw_gemm_f64(const double* a, const double* b, double* c, int m, int n, int k, int trans_a, int trans_b,
                           const double* row_scale, const double* col_scale, rw_stream_t stream) {
  RW_CHECK_ARG(a && b && c && m > 0 && n > 0 && k > 0 && c != a && c != b);
  const dim3 grid((unsigned)rw_cdiv(n, 64), (unsigned)rw_cdiv(m, 64));
  if (grid.y > 65535) return RW_ERR_UNSUPPORTED;
#define RW_GEMM64_LAUNCH(TA, TB)                                                                                       \
  hipLaunchKernelGGL((gemm_f64_kernel<TA, TB>), grid, dim3(256), 0, rw_s(stream), a, b, c, m, n, k, row_scale, col_scale)
  if (trans_a && trans_b) RW_GEMM64_LAUNCH(true, true);
  else if (trans_a) RW_GEMM64_LAUNCH(true, false);
  else if (trans_b) RW_GEMM64_LAUNCH(false, true);
  else RW_GEMM64_LAUNCH(false, false);
#undef RW_GEMM64_LAUNCH
  return RW_LAUNCH_RESULT();
}

// ---------------------------------------------------------------------------------------
// The distance from its parts, one workgroup, every sum in a fixed order (thread-strided partial sums, the butterfly,
// then the four waves in turn): out = { d^2, |mu1 - mu2|^2, Tr S1, Tr S2, sum sqrt(ev) },
// d^2 = ((|mu1 - mu2|^2 + Tr S1) + Tr S2) - 2 sum sqrt(ev) -- the order of metrics/fid.py:186-187.
// ---------------------------------------------------------------------------------------
__global__ void __launch_bounds__(256) frechet_finish_f64_kernel(const double* __restrict__ mu1,
                                                                 const double* __restrict__ mu2,
                                                                 const double* __restrict__ s1,
                                                                 const double* __restrict__ s2,
                                                                 const double* __restrict__ ev, int n, int n_ev,
                                                                 double* __restrict__ out) {
  __shared__ double red[4][4];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  double acc[4] = {0.0, 0.0, 0.0, 0.0};
  for (int i = tid; i < n; i += 256) {
    const double d = mu1[i] - mu2[i];
    acc[0] += d * d;
    acc[1] += s1[(int64_t)i * n + i];
    acc[2] += s2[(int64_t)i * n + i];
  }
  for (int i = tid; i < n_ev; i += 256) acc[3] += sqrt(fmax(ev[i], 0.0));
#pragma unroll
  for (int q = 0; q < 4; ++q) {
    const double s = rw_wave_sum(acc[q]);
    if (lane == 0) red[q][wave] = s;
  }
  __syncthreads();
  if (tid == 0) {
    double t[4];
    for (int q = 0; q < 4; ++q) t[q] = ((red[q][0] + red[q][1]) + red[q][2]) + red[q][3];
    out[0] = ((t[0] + t[1]) + t[2]) - 2.0 * t[3];
    out[1] = t[0]; out[2] = t[1]; out[3] = t[2]; out[4] = t[3];
  }
}

extern "C" int rw_frechet_finish_f64(const double* mu1, const double* mu2, const double* s1, const double* s2,
                                     const double* ev, int n, int n_ev, double* out, rw_stream_t stream) {
  RW_CHECK_ARG(mu1 && mu2 && s1 && s2 && ev && out && n > 0 && n_ev > 0);
  hipLaunchKernelGGL(frechet_finish_f64_kernel, dim3(1), dim3(256), 0, rw_s(stream), mu1, mu2, s1, s2, ev, n, n_ev, out);
  return RW_LAUNCH_RESULT();
}
