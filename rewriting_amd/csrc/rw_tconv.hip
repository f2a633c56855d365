// Upsampling StyledConv in one pass WITHOUT the fourfold multiply count of the phase kernels (round 5):
// conv_transpose2d(stride 2) as a direct sum on the 16-bit matrix pipe, the 4x4 blur from LDS, noise + bias + leaky ReLU +
// the next layer's style in the same epilogue  (utils/stylegan2/models.py:313-316 F.conv_transpose2d(stride=2), :275-281
// Blur(pad 1,1), :539-546 NoiseInjection, :232-257 FusedLeakyReLU).
//
// Why another form.  The one-pass kernels of rw_wino4.hip / rw_dconv.hip compose the blur INTO the weights: four
// output-parity phases, each a dense 3x3 convolution -- 36 taps per 2x2 block of outputs where the transposed convolution
// itself has 9 (layer 17 of the 1024 generator: 38.6 GFLOP per image instead of 9.66; 10.2 ms per launch at batch 64, bound
// by MFMA issue).  The two-pass route (F(2,2) transposed convolution -> (2H+1)^2 map in HBM -> blur pass) multiplies less
// but writes and re-reads the largest map of the layer.  Here the transposed convolution is computed as it is defined,
//     z[o][2i + ky][2j + kx] += W[o][c][ky][kx] x[c][i][j]        (9 multiplies per input position and channel pair),
// its result stays in LDS, and the blur reads it there:
//     y[Y][X] = sum_{a,b} kf[a][b] z[Y - 1 + a][X - 1 + b]        (kf = the FIR as upfirdn2d applies it: flipped).
//
// Decomposition.  A POSITION (i, j) of the input grid owns the four z values (2i + py, 2j + px), py, px in {0, 1}:
//     z[2i + py][2j + px] = sum_{a,b in {0,1}, py + 2a <= 2, px + 2b <= 2}  W[py + 2a][px + 2b] . x[i - a][j - b]
// -- phase (0,0) has four taps, (0,1) and (1,0) two, (1,1) one: nine in all, on FOUR pixel operands x[i-a][j-b].  Positions
// are the M side of v_mfma_f32_16x16x32_f16 (16 consecutive positions of the flattened (TY + 2) x (TX + 2) position window:
// a shift in the flattened index is the same for every lane, so the four pixel operands are four LDS reads at fixed
// offsets), 16 out-channels the N side, a 16-channel chunk the K side with the exact f16 operand split of rw_dconv.hip
// ([Vh c0..3 | Vl c0..3] pixel words -- rw_split4, scaled by rw_split_scales<14>, both in rw_common.h -- against [Uh | Uh]
// and [Ul | Ul]: 18 MFMAs per block and chunk; the packed weights ARE
// rw_pack_dconv_weight_f32's -- the plain 3x3 kernel, no composition).  The blur needs z one row above and two below its
// output rows (one column left, two right): a workgroup computes the positions (TY + 2) x (TX + 2) around its TY x TX
// tile (halo factor 1.2 at 16 x 32) from an x window of (TY + 3) x (TX + 3) pixels staged as in rw_dconv.hip.
//
// Workgroup shapes (template): <TY = 8, 4 waves> two workgroups per CU (67 KB of LDS, <= 256 registers: a workgroup's
// epilogue runs beside the other one's MFMAs) -- the default; <TY = 16, 8 waves> one per CU (106 KB; halo factor 1.2 instead
// of 1.33).  Wave v owns the position blocks v, v + WAVES, ... x 4 phases (96 / 80 accumulator registers).  Per chunk: the
// chunk's 9 KB of weights and the next window are requested a chunk ahead (weights through LDS), the window converted and
// written behind the first / last blocks' MFMAs, one barrier per chunk.
// THREE piece products (rw_dconv.hip): the taps of a phase share the Vh Ul instruction in pairs --
// [Vh(P00) | Vh(P01)] x [Ul(t0) | Ul(t2)] and so on -- 14 MFMAs per block and chunk instead of 18, issued in three tap
// groups (the taps on x[i][j] alone, those that also need x[i][j-1], those on the row above: six operand reads per block
// where four would do, at most five weight operands live).
// Epilogue in two halves of 8 channels (the z tile of 8 channels, 2 (TY + 2) x 72 floats each, reuses the window buffers):
// accumulators -> LDS, barrier, blur, demodulation, noise, bias, leaky ReLU, post scale, max |y| for the bound, 16-byte
// stores.  The blur: when the FIR is an outer product kv x kh (the reference's always is: make_kernel([1,3,3,1])) a
// thread walks DOWN a strip of four output columns -- every z row is read once (two 16-byte LDS reads), filtered
// horizontally (16 multiply-adds), and the last four filtered rows give an output row (16 more): 9.5 multiply-adds per
// output where the direct 16-tap form spends 16, and a third of its LDS reads; any other FIR takes the 16-tap form.
#include "rw_common.h"
#include <stdio.h>
#include <mutex>

struct TconvProblem {
  const float* x; const unsigned char* wp; float* y; const float* k4;
  const float* style; const float* demod; const float* noise; const float* noise_w; const float* bias; int act;
  const float* post;
  int batch, in_ch, out_ch, h, w;
  int tiles_x, tiles_y, o_tiles;
  float w_scale, u_inv;
  const float* x_amax; float* y_amax;
};

#define TC_TX 32
#define TC_PC (TC_TX + 2)                 // position columns
#define TC_WC (TC_TX + 3)                 // window columns: J0 - 2 .. J0 + TX
#define TC_ZP 72                          // z row pitch (floats): columns 3 .. 70 are written, 4 .. 70 read
#define TC_WCH 9216                       // bytes of a chunk's weights of one 16-channel block: 9 taps x [Uh | Ul] x 512

// [h0 h1 h2 h3 q0 q1 q2 q3]: a Vh half-word and the Vh part of a pixel word
__device__ __forceinline__ rw_f16x8 tc_pair_hq(rw_f32x2 h, rw_f16x8 q) {
  const rw_f32x4 qq = __builtin_bit_cast(rw_f32x4, q);
  const rw_f32x4 d = {h[0], h[1], qq[0], qq[1]};
  return __builtin_bit_cast(rw_f16x8, d);
}
// a * b as ONE v_mul_f32: left to the vectoriser, products of values that sit in different 16-byte load results become
// v_pk_mul_f32 on register pairs assembled with two v_mov_b32 each
__device__ __forceinline__ float tc_mul(float a, float b) {
  float r;
  asm("v_mul_f32 %0, %1, %2" : "=v"(r) : "v"(a), "v"(b));
  return r;
}

// STAGED (round 12; p.x is then the map as operand words): the window and the weights arrive by LDS-direct copies of READY operand words -- split_map_kernel
// below has multiplied, split and laid out the whole map once -- where the other form loads fp32, converts and writes the
// window once per 16 NT out-channels.  See "staging by copies" in the body.
template <int TY, int WAVES, int NT, bool STAGED = false>
__device__ __forceinline__ void tconv_body(const TconvProblem& p) {
  constexpr int THREADS = 64 * WAVES;
  constexpr int PR = TY + 2;                        // position rows
  constexpr int NPOS = PR * TC_PC, NBLK = (NPOS + 15) / 16, BPW = (NBLK + WAVES - 1) / WAVES;
  constexpr int WR = TY + 3, NPIX = WR * TC_WC;    // window rows: input rows I0 - 2 .. I0 + TY
  constexpr int BUFB = NPIX * 64;                   // bytes of a window buffer: 16 channels x (2 + 2) bytes per pixel
  constexpr int ZR = 2 * PR, CHS = ZR * TC_ZP + 4;  // z rows of the tile; z channel stride (floats)
  static_assert(8 * CHS * 4 <= 2 * BUFB, "the z tile of eight channels fits the window buffers");
  constexpr int SR = 2 * TY * 128 / THREADS;        // output rows of a thread's strip in the epilogue
  static_assert(WAVES % 4 == 0 && THREADS % 128 == 0 && SR * (THREADS / 128) == 2 * TY && (SR == 4 || SR == 8),
                "four or eight output rows per strip segment");
  // NT blocks of 16 out-channels per workgroup (p.o_tiles = out_ch / OC): a pixel operand read from LDS multiplies into NT
  // accumulator blocks, the window is staged (requested, converted, written) once per OC out-channels
  constexpr int OC = 16 * NT, WCH = NT * TC_WCH;
  __shared__ __attribute__((aligned(16))) unsigned char Ls[2 * BUFB];
  __shared__ __attribute__((aligned(16))) unsigned char Wl[2 * WCH];
  __shared__ __attribute__((aligned(16))) float St[512];
  __shared__ float Sc[OC], Bs[OC], Po[OC], Kf[16], Red[WAVES];

  const int tid = threadIdx.x, lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int lk = lane >> 4, lt = lane & 15;

  int ot, tx, ty, ib;
  rw_tile_digits(p, rw_xcd_remap(blockIdx.x, gridDim.x), ot, tx, ty, ib);
  const int I0 = ty * TY, J0 = tx * TC_TX;
  const int64_t hw = (int64_t)p.h * p.w;
  const int NC = p.in_ch >> 4, T = 9 * NC;

  // ---- scales (rw_split_scales, rw_common.h); headroom 14: V itself is split
  float in_scale, out_scale;
  {
    const float smax = rw_block_max<WAVES>(rw_style_absmax_wave<64 * WAVES>(p, ib, tid), lane, wave, Red);
    rw_split_scales<14>(rw_bound_load(p.x_amax) * smax, p.u_inv, in_scale, out_scale);
  }
  const float gain = p.act ? 1.4142135623730951f : 1.f, slope = p.act ? 0.2f : 1.f;
  if constexpr (!STAGED)                            // (STAGED: the style and in_scale are in the words)
    for (int i = tid; i < p.in_ch; i += THREADS) St[i] = (p.style ? p.style[(int64_t)ib * p.in_ch + i] : 1.0f) * in_scale;
  if (tid < OC) {
    const int o = OC * ot + tid;
    Sc[tid] = (p.demod ? p.demod[(int64_t)ib * p.out_ch + o] * p.w_scale : p.w_scale) * out_scale * gain;
    Bs[tid] = p.act ? p.bias[o] * gain : 0.f;
    Po[tid] = p.post ? p.post[(int64_t)ib * p.out_ch + o] : 1.f;
  }
  if (tid < 16) {
    const int a = tid >> 2, c = tid & 3;
    Kf[tid] = p.k4[(3 - a) * 4 + (3 - c)];        // flipped, as upfirdn2d applies it
  }
  const float noise_wg = p.noise ? p.noise_w[0] * gain : 0.f;
  __syncthreads();                                  // the tables are read by other threads than their writers

  // ---- staging: wave v stages channel quad g = v & 3
  // A lane's ITEM is a 16-byte aligned run of four window columns (4 j - 2 .. 4 j + 1 of the window: input columns
  // J0 - 4 + 4 j ..) of one row: four 16-byte loads -- one per channel of the quad -- bring 4 pixels x 4 channels, i.e. four
  // LDS words.  (Round 5 staged one pixel per lane with 4-byte loads: the 24 loads a thread issued per chunk took ~20 cycles
  // EACH to issue -- cycle counters, profiles/r06q: the vector-memory address path, not latency or bandwidth, paced the
  // window; requesting both halves a whole chunk ahead made it slower.)  Items outside the image read 0 through the
  // descriptor's range check; the two columns left of the window (j = 0) and the three right of it (j = IPR - 1) are loaded
  // and dropped.  Piece s of wave v: item LPP (NSL s + (v >> 2)) + lane of the WR x IPR items, lanes < LPP -- every wave has
  // every piece (48 of 64 lanes each at TY = 16): no wave-dependent branch around a request, which would make hipcc's vmcnt
  // waits for the OLDER requests assume it absent (the software pipeline below keeps up to eleven in flight).
  constexpr int NSL = WAVES / 4;
  const int g = wave & 3, hsel = wave >> 2;
  const __amdgpu_buffer_rsrc_t xsrc = rw_image_rsrc(p.x, ib, p.in_ch, hw);
  const int hw4 = (int)hw * 4;
  constexpr int IPR = TC_TX / 4 + 2, NITEM = WR * IPR;
  constexpr int SI = (NITEM + 64 * NSL - 1) / (64 * NSL), LPP = ((NITEM + SI * NSL - 1) / (SI * NSL) + 3) & ~3;
  static_assert(SI <= 2 && LPP <= 64 && LPP * SI * NSL >= NITEM, "one or two pieces per wave cover the window");
  int xoff[SI], lofa[SI], lofb[SI], lok[SI];        // LDS byte offsets of the item's pixels 0 / 2 (1 / 3: + 64); bit e of lok: pixel e is a window pixel
#pragma unroll
  for (int s = 0; s < SI; ++s) {
    const int it = LPP * (NSL * s + hsel) + lane;
    const bool mine = lane < LPP && it < NITEM;
    const int r = it / IPR, j = it - r * IPR;
    const int iy = I0 - 2 + r, ix = J0 - 4 + 4 * j;                // the item lies inside the row or outside it as a whole
    const bool ok = mine && iy >= 0 && iy < p.h && ix >= 0 && ix < p.w;
    xoff[s] = ok ? (iy * p.w + ix) * 4 : 0x7ffffff0;
    const int cc0 = 4 * j - 2;                                      // window column of pixel 0
    lofa[s] = (r * TC_WC + cc0) * 64 + ((g ^ rw_swz(cc0 & 0x7ffffffe)) << 4);          // pixels 0, 1 share a swizzle ((cc >> 1) & 3) ...
    lofb[s] = (r * TC_WC + cc0 + 2) * 64 + ((g ^ rw_swz(cc0 + 2)) << 4);               // ... pixels 2, 3 the next one
    int m = 0;
#pragma unroll
    for (int e = 0; e < 4; ++e) m |= (mine && cc0 + e >= 0 && cc0 + e < TC_WC) ? (1 << e) : 0;
    lok[s] = m;
  }
  rw_f32x4 raw[SI][4];                              // [piece][channel]: four pixels
  // channels K0 .. K1 - 1 of piece s of chunk c requested
  auto stage_load_part = [&](int c, auto s_tag, auto k0_tag, auto k1_tag) __attribute__((always_inline)) {
    constexpr int s = decltype(s_tag)::value, K0 = decltype(k0_tag)::value, K1 = decltype(k1_tag)::value;
    const int s0 = (16 * c + 4 * g) * hw4;
#pragma unroll
    for (int k = K0; k < K1; ++k)
      raw[s][k] = __builtin_bit_cast(rw_f32x4, __builtin_amdgcn_raw_buffer_load_b128(xsrc, xoff[s], s0 + k * hw4, 0));
  };
  // pixels E0 .. E1 - 1 of piece s converted (style, exact f16 pair split) and written
  auto stage_store_part = [&](int c, int buf, auto s_tag, auto e0_tag, auto e1_tag) __attribute__((always_inline)) {
    constexpr int s = decltype(s_tag)::value, E0 = decltype(e0_tag)::value, E1 = decltype(e1_tag)::value;
    const rw_f32x4 sv = *reinterpret_cast<const rw_f32x4*>(&St[16 * c + 4 * g]);
    unsigned char* dst = Ls + buf * BUFB;
#pragma unroll
    for (int e = E0; e < E1; ++e) {
      const float v0 = tc_mul(raw[s][0][e], sv[0]), v1 = tc_mul(raw[s][1][e], sv[1]), v2 = tc_mul(raw[s][2][e], sv[2]),
                  v3 = tc_mul(raw[s][3][e], sv[3]);
      rw_f16x8 word = rw_split4(v0, v1, v2, v3);
      if (lok[s] & (1 << e)) *reinterpret_cast<rw_f16x8*>(dst + (e < 2 ? lofa[s] : lofb[s]) + (e & 1) * 64) = word;
    }
  };
  // the chunk's weights of this workgroup's NT out-channel blocks: NT x 9216 contiguous bytes of the packed array -> LDS
  const unsigned char* wsrc = p.wp + (int64_t)(NT * ot) * T * 1024;
  constexpr int NPC = NT * (TC_WCH / 16), NWP = (NPC + THREADS - 1) / THREADS;      // 16-byte pieces, per thread
  rw_f32x4 wraw[NWP];
  auto wstage_load = [&](int c) __attribute__((always_inline)) {
#pragma unroll
    for (int k = 0; k < NWP; ++k) {                 // (no branch around a request: the threads past the end read the last piece again)
      const int pc = tid + k * THREADS < NPC ? tid + k * THREADS : NPC - 1;
      const int n = pc / (TC_WCH / 16), r = pc - n * (TC_WCH / 16);
      wraw[k] = *reinterpret_cast<const rw_f32x4*>(wsrc + ((int64_t)n * T + 9 * c) * 1024 + r * 16);
    }
  };
  auto wstage_store = [&](int buf) __attribute__((always_inline)) {
    unsigned char* dst = Wl + buf * WCH;
#pragma unroll
    for (int k = 0; k < NWP; ++k)
      if ((k + 1) * THREADS <= NPC || tid + k * THREADS < NPC)
        *reinterpret_cast<rw_f32x4*>(dst + (tid + k * THREADS) * 16) = wraw[k];
  };

  // ---- staging by copies (STAGED).  p.x holds the map as the words the window buffer takes --
  // words[image][chunk][y][x][quad][8 halves], split_map_kernel -- so a window is copied, not converted: one
  // `buffer_load_dwordx4 ... lds` (rw_dma_buffer_b128) moves 64 lanes x 16 bytes into 1 KB of contiguous LDS = 16 consecutive
  // window pixels x their four 16-byte slots.  Lane (pixel, slot s) fetches quad s ^ rw_swz(column): the swizzle lives in the
  // lane's global offset, computed once; a pixel outside the image has the out-of-range offset and lands as zeros.  The
  // NPIX * 4 slots are NPC_S pieces, PPW per wave: piece wave + WAVES k, the ones past the end (and the last one, which would
  // overrun the buffer) start at slot NSLOT - 64 and write bytes a sibling writes too, with the same values -- no exec mask,
  // no wave-dependent branch.  The chunk advance is the scalar offset.  The weights come the same way
  // (rw_dma_global_b128_s): 9 NT pieces of 1 KB, NWS per wave, clamped to the last one.
  // Nothing but these copies and the epilogue's traffic is in the vector-memory queue of a STAGED workgroup, and the compiler
  // cannot count them (rw_dconv.hip): the waits are written by hand.  A chunk's copies are requested during the chunk before
  // it, behind its first position blocks, one request per block; the chunk ends with vmcnt(0) -- this wave issues nothing
  // behind them, so N = 0 -- lgkmcnt(0) and the raw barrier.  Two buffers as before; the noise loads and the stores come
  // after the loop, when no copy is in flight.
  constexpr int NSLOT = NPIX * 4, NPC_S = (NSLOT + 63) / 64, PPW = (NPC_S + WAVES - 1) / WAVES;
  constexpr int NWPC = 9 * NT, NWS = (NWPC + WAVES - 1) / WAVES;
  static_assert(NSLOT >= 64 && NWS + PPW <= 3 * BPW, "one request behind each position block of a chunk");
  typedef __attribute__((address_space(3))) unsigned char* lds_b;
  const unsigned ls_base = (unsigned)(size_t)(lds_b)Ls, wl_base = (unsigned)(size_t)(lds_b)Wl;
  // (the descriptor of rw_image_rsrc over the words of image ib, as the four integers the assembly takes)
  const unsigned long long xw_addr = (unsigned long long)(p.x + (int64_t)ib * p.in_ch * hw);
  const rw_i32x4 xsrc_w = {(int)(unsigned)xw_addr, (int)(unsigned)(xw_addr >> 32), (int)((int64_t)p.in_ch * hw * 4), 0x00020000};
  int voff[PPW], sslot[PPW];                        // the lane's global byte offset within (image, chunk); the piece's first slot
  if constexpr (STAGED) {
#pragma unroll
    for (int k = 0; k < PPW; ++k) {
      const int first = 64 * (wave + WAVES * k);
      sslot[k] = first < NSLOT - 64 ? first : NSLOT - 64;
      const int L = sslot[k] + lane, pix = L >> 2, s = L & 3;
      const int r = pix / TC_WC, c = pix - r * TC_WC;
      const int iy = I0 - 2 + r, ix = J0 - 2 + c;
      const bool ok = iy >= 0 && iy < p.h && ix >= 0 && ix < p.w;
      voff[k] = ok ? (iy * p.w + ix) * 64 + ((s ^ rw_swz(c)) << 4) : 0x7ffffff0;
    }
  }
  // request q of the copies of chunk c into buffer buf: the weight pieces first, then the window's
  // (q is a constant wherever the position-block loops are unrolled: the comparisons fold)
  auto copy_request = [&](int c, int buf, int q) __attribute__((always_inline)) {
#pragma unroll
    for (int k = 0; k < NWS; ++k)
      if (q == k) {
        const int first = wave + WAVES * k, wpc = first < NWPC ? first : NWPC - 1;
        const int n = wpc / 9, r = wpc - 9 * n;
        rw_dma_global_b128_s(wl_base + (unsigned)(buf * WCH + wpc * 1024), lane * 16,
                             wsrc + ((int64_t)n * T + 9 * c) * 1024 + r * 1024);
      }
#pragma unroll
    for (int k = 0; k < PPW; ++k)
      if (q == NWS + k)
        rw_dma_buffer_b128(ls_base + (unsigned)(buf * BUFB + sslot[k] * 16), voff[k], xsrc_w, c * hw4 * 16);
  };
  auto copy_wait = [&]() __attribute__((always_inline)) {
    asm volatile("" ::: "memory");
    __builtin_amdgcn_s_waitcnt(0x0070);             // vmcnt(0) lgkmcnt(0): this wave's copies have landed, its LDS reads are done
    __builtin_amdgcn_s_barrier();
    asm volatile("" ::: "memory");
  };

  // ---- this wave's position blocks: operand addresses of the lane's position q = 16 blk + lt (clamped), pixel offsets
  // (a, b) = x[i - a][j - b] at window pixel (r + 1 - a, c + 1 - b)
  // (the ROW ABOVE, a = 1; the position's own row is + TC_WC * 64: an immediate.  They include the window buffer's offset and
  // move by +- BUFB at the end of a chunk -- 2 BPW additions per chunk where `buffer base + offset` cost one per operand read)
  unsigned pb0[BPW], pb1[BPW];                     // column offset b = 0 / 1 at row offset a = 1
#pragma unroll
  for (int b = 0; b < BPW; ++b) {
    int q = 16 * (wave + WAVES * b) + lt;
    q = q < NPOS ? q : NPOS - 1;
    const int r = q / TC_PC, c = q - r * TC_PC;
    pb0[b] = (unsigned)((r * TC_WC + c + 1) * 64 + ((lk ^ rw_swz(c + 1)) << 4));
    pb1[b] = (unsigned)((r * TC_WC + c) * 64 + ((lk ^ rw_swz(c)) << 4));
  }

  rw_f32x4 acc[BPW][NT][4];
#pragma unroll
  for (int b = 0; b < BPW; ++b)
#pragma unroll
    for (int n = 0; n < NT; ++n)
#pragma unroll
      for (int ph = 0; ph < 4; ++ph) acc[b][n][ph] = rw_f32x4{0.f, 0.f, 0.f, 0.f};

  // One chunk in THREE tap groups, so that at most five weight operands per out-channel block (20 NT registers) are live
  // beside the accumulators: G0 = the taps on x[i][j] alone, G1 = those that also need x[i][j-1], G2 = those on the row above.
  // Tap t = 3 ky + kx of phase ph = 2 py + px sits on the operand (a, b) = x[i-a][j-b] with ky = py + 2a, kx = px + 2b.
  // Three piece products (rw_dconv.hip): Vh Uh + Vl Uh by [Vh | Vl] x [Uh | Uh]; the Vh Ul of two taps of one phase share an
  // instruction, [Vh(P) | Vh(Q)] x [Ul(tP) | Ul(tQ)]; tap (1, 1), alone in its phase, keeps all four ([Ul | Ul]).
#define TB_MFMA(PH, A, B) acc[b][n][PH] = __builtin_amdgcn_mfma_f32_16x16x32_f16(A, B, acc[b][n][PH], 0, 0, 0)
#define TB_UH(T_) rw_expand(*reinterpret_cast<const rw_f32x2*>(wb + n * TC_WCH + (T_) * 1024))
#define TB_UL(T_) (*reinterpret_cast<const rw_f32x2*>(wb + n * TC_WCH + (T_) * 1024 + 512))
#define TC_PIX(OFF) (*reinterpret_cast<const rw_f16x8*>(lb + (OFF)))
#define TC_VH(OFF) (*reinterpret_cast<const rw_f32x2*>(lb + (OFF)))
// (the persistent kernels below: one out-channel block per workgroup)
#define TC_MFMA(PH, A, B) acc[b][PH] = __builtin_amdgcn_mfma_f32_16x16x32_f16(A, B, acc[b][PH], 0, 0, 0)
#define TC_UH(T_) rw_expand(*reinterpret_cast<const rw_f32x2*>(wb + (T_) * 1024))
#define TC_UL(T_) (*reinterpret_cast<const rw_f32x2*>(wb + (T_) * 1024 + 512))
  auto chunk = [&](int c, auto last_tag) __attribute__((always_inline)) {
    constexpr bool LAST = decltype(last_tag)::value != 0;
    const int buf = c & 1;
    const unsigned char* lb = Ls;                   // (pb0 / pb1 carry the buffer's offset)
    const unsigned char* wb = Wl + buf * WCH + lane * 8;
    // The software pipeline: what is requested during chunk c (piece 0 behind the first tap group's blocks, piece 1 behind the
    // second group's, the weights behind the third's) belongs to chunk c + 2 and is converted / written during chunk c + 1
    // (behind the first blocks of the same groups, just before the registers are requested again): every load has a whole
    // chunk to arrive, the requests are spread (eight waves requesting a window at once stall at the issue of their loads and
    // the MFMAs behind them wait: profiles/r06s), the conversion sits between MFMAs.  The chunk barrier waits for LDS only.
    // No branches around the requests: past the end they read the last chunk again, into registers nobody converts -- with
    // them inside conditionals hipcc waits for vmcnt(0) at the first conversion of every chunk.
    constexpr bool st = !LAST;
    const int c2 = c + 2 < NC ? c + 2 : NC - 1;
    auto hook = [&](auto grp_tag, int b) __attribute__((always_inline)) {
      constexpr int grp = decltype(grp_tag)::value;
      if constexpr (STAGED) {
        if (st) copy_request(c + 1, buf ^ 1, grp * BPW + b);        // chunk c + 1, one request behind each block
      } else if constexpr (grp < SI) {
        if (b == 0 && st) stage_store_part(c + 1, buf ^ 1, rw_int<grp>(), rw_int<0>(), rw_int<2>());
        if (b == 1 && st) stage_store_part(c + 1, buf ^ 1, rw_int<grp>(), rw_int<2>(), rw_int<4>());
        if constexpr (BPW >= 4) {
          if (b == 2) stage_load_part(c2, rw_int<grp>(), rw_int<0>(), rw_int<2>());
          if (b == 3) stage_load_part(c2, rw_int<grp>(), rw_int<2>(), rw_int<4>());
        } else {
          if (b == 2) stage_load_part(c2, rw_int<grp>(), rw_int<0>(), rw_int<4>());
        }
      } else if constexpr (grp == 2) {
        if (b == 0 && st) wstage_store(buf ^ 1);
        if (b == 1) wstage_load(c2);
      }
    };
    // (operands one block ahead, the order pinned: left to itself the scheduler hoists every block's LDS reads to the top
    // of a group and spills; only the last block of a wave can be missing: NBLK > WAVES (BPW - 1))
    constexpr int LB = BPW - 1;
    const bool last_ok = wave + WAVES * LB < NBLK;  // wave-uniform
    {
      rw_f16x8 u0[NT], u1[NT], u3[NT], u4[NT], l4[NT];
#pragma unroll
      for (int n = 0; n < NT; ++n) { u0[n] = TB_UH(0); u1[n] = TB_UH(1); u3[n] = TB_UH(3); u4[n] = TB_UH(4); l4[n] = rw_expand(TB_UL(4)); }
      rw_f16x8 pc = TC_PIX(pb0[0] + TC_WC * 64);
#pragma unroll
      for (int b = 0; b < BPW; ++b) {
        rw_f16x8 pn = pc;
        if (b + 1 < BPW) pn = TC_PIX(pb0[b + 1] + TC_WC * 64);
        if (b < LB || last_ok) {
#pragma unroll
          for (int n = 0; n < NT; ++n) {
            TB_MFMA(3, pc, u4[n]); TB_MFMA(0, pc, u0[n]); TB_MFMA(1, pc, u1[n]); TB_MFMA(2, pc, u3[n]);
            TB_MFMA(3, pc, l4[n]);                  // (never two dependent MFMAs back to back)
          }
        }
        hook(rw_int<0>(), b);
        __builtin_amdgcn_sched_barrier(0);
        pc = pn;
      }
    }
    __builtin_amdgcn_sched_barrier(0);
    {
      rw_f16x8 u2[NT], u5[NT], m02[NT], m35[NT];
#pragma unroll
      for (int n = 0; n < NT; ++n) { u2[n] = TB_UH(2); u5[n] = TB_UH(5); m02[n] = rw_pair(TB_UL(0), TB_UL(2)); m35[n] = rw_pair(TB_UL(3), TB_UL(5)); }
      rw_f32x2 hc = TC_VH(pb0[0] + TC_WC * 64);             // Vh of x[i][j]: the first half of its word
      rw_f16x8 qc = TC_PIX(pb1[0] + TC_WC * 64);
#pragma unroll
      for (int b = 0; b < BPW; ++b) {
        rw_f32x2 hn = hc;
        rw_f16x8 qn = qc;
        if (b + 1 < BPW) { hn = TC_VH(pb0[b + 1] + TC_WC * 64); qn = TC_PIX(pb1[b + 1] + TC_WC * 64); }
        if (b < LB || last_ok) {
          const rw_f16x8 M = tc_pair_hq(hc, qc);
#pragma unroll
          for (int n = 0; n < NT; ++n) {
            TB_MFMA(0, qc, u2[n]); TB_MFMA(2, qc, u5[n]);                         // taps (0, 2), (1, 2)
            TB_MFMA(0, M, m02[n]); TB_MFMA(2, M, m35[n]);                         // Vh Ul of (0, 0) + (0, 2); (1, 0) + (1, 2)
          }
        }
        hook(rw_int<1>(), b);
        __builtin_amdgcn_sched_barrier(0);
        hc = hn; qc = qn;
      }
    }
    {
      rw_f16x8 u6[NT], u7[NT], u8[NT], m17[NT], m68[NT];
#pragma unroll
      for (int n = 0; n < NT; ++n) {
        u6[n] = TB_UH(6); u7[n] = TB_UH(7); u8[n] = TB_UH(8);
        m17[n] = rw_pair(TB_UL(1), TB_UL(7)); m68[n] = rw_pair(TB_UL(6), TB_UL(8));
      }
      rw_f32x2 hc = TC_VH(pb0[0] + TC_WC * 64);
      rw_f16x8 qc = TC_PIX(pb0[0]), rc = TC_PIX(pb1[0]);
#pragma unroll
      for (int b = 0; b < BPW; ++b) {
        rw_f32x2 hn = hc;
        rw_f16x8 qn = qc, rn = rc;
        if (b + 1 < BPW) { hn = TC_VH(pb0[b + 1] + TC_WC * 64); qn = TC_PIX(pb0[b + 1]); rn = TC_PIX(pb1[b + 1]); }
        if (b < LB || last_ok) {
          const rw_f16x8 M02 = tc_pair_hq(hc, qc), M23 = rw_pair(qc, rc);
#pragma unroll
          for (int n = 0; n < NT; ++n) {
            TB_MFMA(0, qc, u6[n]); TB_MFMA(1, qc, u7[n]);                         // taps (2, 0), (2, 1)
            TB_MFMA(0, rc, u8[n]); TB_MFMA(1, M02, m17[n]);                       // tap (2, 2); Vh Ul of (0, 1) + (2, 1)
            TB_MFMA(0, M23, m68[n]);                                              // Vh Ul of (2, 0) + (2, 2)
          }
        }
        hook(rw_int<2>(), b);
        __builtin_amdgcn_sched_barrier(0);
        hc = hn; qc = qn; rc = rn;
      }
    }
    if (!LAST) {
      const unsigned delta = buf ? (unsigned)-BUFB : (unsigned)BUFB;
#pragma unroll
      for (int b = 0; b < BPW; ++b) { pb0[b] += delta; pb1[b] += delta; }
      if constexpr (STAGED) copy_wait();            // the copies of chunk c + 1 have landed
      else {
        asm volatile("" ::: "memory");
        __builtin_amdgcn_s_waitcnt(0xC07F);         // lgkmcnt(0): the requests of chunk c + 2 stay in flight across the barrier
        __builtin_amdgcn_s_barrier();
        asm volatile("" ::: "memory");
      }
    }
  };

  // ---- prologue: chunk 0 requested, converted, written; chunk 1 (in_ch == 16: chunk 0 again, never converted) requested, in
  // the order of a chunk's requests, pinned -- the waits of the loop count the requests behind the one they need
  if constexpr (STAGED) {                           // chunk 0 copied; chunk 1 is requested inside chunk 0
#pragma unroll
    for (int q = 0; q < NWS + PPW; ++q) copy_request(0, 0, q);
    copy_wait();
  } else {
  wstage_load(0);
#pragma unroll
  for (int s = 0; s < SI; ++s) {
    if (s == 0) stage_load_part(0, rw_int<0>(), rw_int<0>(), rw_int<4>());
    else stage_load_part(0, rw_int<SI - 1>(), rw_int<0>(), rw_int<4>());
  }
  stage_store_part(0, 0, rw_int<0>(), rw_int<0>(), rw_int<4>());
  if constexpr (SI > 1) stage_store_part(0, 0, rw_int<SI - 1>(), rw_int<0>(), rw_int<4>());
  wstage_store(0);
  __syncthreads();
  {
    const int c1 = NC > 1 ? 1 : 0;
    __builtin_amdgcn_sched_barrier(0);
    stage_load_part(c1, rw_int<0>(), rw_int<0>(), rw_int<4>());
    __builtin_amdgcn_sched_barrier(0);
    if constexpr (SI > 1) stage_load_part(c1, rw_int<SI - 1>(), rw_int<0>(), rw_int<4>());
    __builtin_amdgcn_sched_barrier(0);
    wstage_load(c1);
    __builtin_amdgcn_sched_barrier(0);
  }
  }

  for (int c = 0; c + 1 < NC; ++c) chunk(c, rw_int<0>());
  chunk(NC - 1, rw_int<1>());
  __syncthreads();                                  // every wave has read its last operands: the windows become the z tile

  // ---- epilogue, eight channels at a time
  float* Z = reinterpret_cast<float*>(Ls);
  float ymax = 0.f;
  float kf[16];
#pragma unroll
  for (int t = 0; t < 16; ++t) kf[t] = Kf[t];
  // is the FIR an outer product kv x kh?  (kh = its first row, kv = its first column / its corner)
  bool sep = kf[0] != 0.f;
  float kv[4], kmax = 0.f;
#pragma unroll
  for (int t = 0; t < 16; ++t) kmax = fmaxf(kmax, fabsf(kf[t]));
#pragma unroll
  for (int a = 0; a < 4; ++a) kv[a] = sep ? kf[4 * a] / kf[0] : 0.f;
#pragma unroll
  for (int t = 0; t < 16; ++t) sep = sep && fabsf(kf[t] - kv[t >> 2] * kf[t & 3]) <= 1e-6f * kmax;
  const int W2 = 2 * p.w;
  const int64_t hw2 = 4 * hw;
  // strip of this thread (separable FIR): four output columns, SR output rows, one channel per pass.  Its SR noise
  // vectors are the same in every pass: requested here, ahead of the z writes and their barrier (one L2 round trip
  // instead of one per output row)
  const int strip = tid & 127, seg = tid >> 7;
  const int s_og = strip & 15, s_ch = strip >> 4, s_oy0 = SR * seg;
  const int64_t s_pix = (int64_t)(2 * I0 + s_oy0) * W2 + 2 * J0 + 4 * s_og;
  rw_f32x4 nzr[SR];
#pragma unroll
  for (int oy = 0; oy < SR; ++oy) {
    nzr[oy] = rw_f32x4{0.f, 0.f, 0.f, 0.f};
    if (sep && p.noise)
      nzr[oy] = *reinterpret_cast<const rw_f32x4*>(p.noise + (int64_t)ib * hw2 + s_pix + (int64_t)oy * W2);
  }
#pragma unroll
  for (int n = 0; n < NT; ++n) {
#pragma unroll 1
  for (int pass = 0; pass < 2; ++pass) {
    if ((lt >> 3) == pass) {
      float* zc = Z + (lt & 7) * CHS;
#pragma unroll
      for (int b = 0; b < BPW; ++b) {
        if (wave + WAVES * b >= NBLK) continue;
#pragma unroll
        for (int j = 0; j < 4; ++j) {
          const int q = 16 * (wave + WAVES * b) + 4 * lk + j;
          if (q < NPOS) {
            const int r = q / TC_PC, c = q - r * TC_PC;
            float* zp = zc + (2 * r) * TC_ZP + 2 * c + 3;
            zp[0] = acc[b][n][0][j];
            zp[1] = acc[b][n][1][j];
            zp[TC_ZP] = acc[b][n][2][j];
            zp[TC_ZP + 1] = acc[b][n][3][j];
          }
        }
      }
    }
    __syncthreads();
    if (sep) {
      // strip of four output columns, SR output rows: z rows oy0 + 1 .. oy0 + SR + 3, each read once
      const float* zb = Z + s_ch * CHS + (s_oy0 + 1) * TC_ZP + 4 * s_og + 4;
      const int cl = 16 * n + 8 * pass + s_ch;      // channel within the workgroup's OC
      const float sc = Sc[cl], bs = Bs[cl], post = Po[cl];
      float* yb = p.y + ((int64_t)ib * p.out_ch + OC * ot + cl) * hw2 + s_pix;
      rw_f32x4 hrow[4];                             // the last four horizontally filtered rows
      rw_f32x4 lo = *reinterpret_cast<const rw_f32x4*>(zb), hi = *reinterpret_cast<const rw_f32x4*>(zb + 4);
#pragma unroll
      for (int zr = 0; zr < SR + 3; ++zr) {
        rw_f32x4 lon = lo, hin = hi;                // the next z row, requested before this one is filtered
        if (zr + 1 < SR + 3) {
          lon = *reinterpret_cast<const rw_f32x4*>(zb + (zr + 1) * TC_ZP);
          hin = *reinterpret_cast<const rw_f32x4*>(zb + (zr + 1) * TC_ZP + 4);
        }
        rw_f32x4 hsum = lo * kf[0];
        hsum += rw_f32x4{lo[1], lo[2], lo[3], hi[0]} * kf[1];
        hsum += rw_f32x4{lo[2], lo[3], hi[0], hi[1]} * kf[2];
        hsum += rw_f32x4{lo[3], hi[0], hi[1], hi[2]} * kf[3];
        hrow[zr & 3] = hsum;
        if (zr >= 3) {
          const int oy = zr - 3;                    // output row oy0 + oy: filtered rows zr - 3 .. zr
          rw_f32x4 res = hrow[(zr - 3) & 3] * kv[0];
          res += hrow[(zr - 2) & 3] * kv[1];
          res += hrow[(zr - 1) & 3] * kv[2];
          res += hrow[zr & 3] * kv[3];
          const rw_f32x4 nz = nzr[oy] * noise_wg;
          rw_f32x4 v;
#pragma unroll
          for (int q = 0; q < 4; ++q) {
            const float u = res[q] * sc + nz[q] + bs;
            v[q] = fmaxf(u, u * slope) * post;
            ymax = fmaxf(ymax, fabsf(v[q]));
          }
          *reinterpret_cast<rw_f32x4*>(yb + (int64_t)oy * W2) = v;
        }
        __builtin_amdgcn_sched_barrier(0);
        lo = lon; hi = hin;
      }
    } else {
#pragma unroll 1
      for (int k = 0; k < 8 * 2 * TY * 16 / THREADS; ++k) {
        const int gid = tid + THREADS * k;          // 8 channels x 2 TY rows x 16 groups of four outputs
        const int og = gid & 15, oy = (gid >> 4) % (2 * TY), ch = gid / (32 * TY);
        const float* zb = Z + ch * CHS + (oy + 1) * TC_ZP + 4 * og + 4;
        float res[4] = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
        for (int a = 0; a < 4; ++a) {
          const rw_f32x4 lo = *reinterpret_cast<const rw_f32x4*>(zb + a * TC_ZP);
          const rw_f32x4 hi = *reinterpret_cast<const rw_f32x4*>(zb + a * TC_ZP + 4);
          const float rowv[7] = {lo[0], lo[1], lo[2], lo[3], hi[0], hi[1], hi[2]};
#pragma unroll
          for (int q = 0; q < 4; ++q)
#pragma unroll
            for (int cc = 0; cc < 4; ++cc) res[q] += rowv[q + cc] * kf[a * 4 + cc];
        }
        const int cl = 16 * n + 8 * pass + ch;
        const int64_t pix = (int64_t)(2 * I0 + oy) * W2 + 2 * J0 + 4 * og;
        rw_f32x4 nz = {0.f, 0.f, 0.f, 0.f};
        if (p.noise) nz = *reinterpret_cast<const rw_f32x4*>(p.noise + (int64_t)ib * hw2 + pix) * noise_wg;
        const float sc = Sc[cl], bs = Bs[cl], post = Po[cl];
        rw_f32x4 v;
#pragma unroll
        for (int q = 0; q < 4; ++q) {
          const float u = res[q] * sc + nz[q] + bs;
          v[q] = fmaxf(u, u * slope) * post;
          ymax = fmaxf(ymax, fabsf(v[q]));
        }
        *reinterpret_cast<rw_f32x4*>(p.y + ((int64_t)ib * p.out_ch + OC * ot + cl) * hw2 + pix) = v;
      }
    }
    __syncthreads();
  }
  }
  if (p.y_amax) rw_bound_store_wave(p.y_amax, rw_wave_max(ymax));
}

__global__ void __launch_bounds__(256, 2) tconv_blur_t8_kernel(const TconvProblem p) { tconv_body<8, 4, 1>(p); }
__global__ void __launch_bounds__(512, 1) tconv_blur_t16_kernel(const TconvProblem p) { tconv_body<16, 8, 1>(p); }
// 32 out-channels per workgroup (round 6): an 8 x 32 tile, eight waves of three position blocks x two out-channel blocks
__global__ void __launch_bounds__(512, 1) tconv_blur_n32_kernel(const TconvProblem p) { tconv_body<8, 8, 2>(p); }
// (four waves per SIMD -- <8, 8> twice per CU, <16, 16> once -- do not fit: 128 registers against 48 accumulators + ~125
// for the operands and the epilogue, 120 - 150 spilled)
// ---------------------------------------------------------------------------------------
// Third form: the waves of a workgroup SPECIALISE and the workgroup is PERSISTENT (rw_dconv.hip's dconv_ws_body, applied to
// the kernel above).  Measured on the forms above (profiles/r05g, layer 17): the window loads cost 2.2 ms of 7.8 (every
// half-chunk's HBM latency is exposed: four chunks, nothing else to run), the epilogue 3.9 (its noise loads alone 1.0), and
// nothing overlaps -- one wave does every job in turn.  Here ONE workgroup of eight waves owns a CU and walks every
// (grid)th tile:
//   waves 4..7 (one per SIMD) stage: one channel quad each, a lane's item = a 16-byte aligned run of four window columns x
//     four channels; piece s of chunk n + 1 is converted and written, then piece s of chunk n + 2 requested into the same
//     registers -- across tile boundaries and through the epilogue: loads are in flight all the time.  They carry the
//     chunk's 9 KB of weights (three 1-KB tap pieces per wave at most) and the tile's tables too;
//   waves 0..3 (one per SIMD) multiply: six position blocks each (96 accumulator registers), the tap groups of the kernel
//     above, pixel AND weight operands from LDS, and write the z tile (its own 46 KB of LDS: the window buffers belong to
//     the staging waves);
//   ALL eight run the blur: 512 strips of four output columns x four rows per pass of eight channels (noise requested a
//     chunk of MFMAs earlier), 16-byte stores.
// One raw s_barrier per chunk and two more per tile (z written -> blurred | the other eight channels written -> blurred).
// Tile: 8 x 32 positions (16 x 64 outputs) x 16 out-channels; in_ch >= 32 (the tables are double-buffered by tile parity).
// ---------------------------------------------------------------------------------------

// MW multiplying waves (4: the form of round 5, one per SIMD beside a staging wave; 8: two per SIMD beside a staging wave --
// twelve waves of at most 168 registers, which the kernel fits since the library is compiled without packed fp32 math: round 6)
template <int MW>
__device__ __forceinline__ void tconv_ws_body(const TconvProblem& p) {
  constexpr int TY = 8;
  constexpr int PR = TY + 2, NPOS = PR * TC_PC, NBLK = (NPOS + 15) / 16, BPW = (NBLK + MW - 1) / MW;
  constexpr int WR = TY + 3, NPIX = WR * TC_WC, BUFB = NPIX * 64;
  constexpr int IPR = TC_TX / 4 + 2, NITEM = WR * IPR, SI = (NITEM + 63) / 64;   // items: window columns 4 j - 2 .. 4 j + 1
  // z tile: rows 0 .. 2 PR - 1 + two spare rows (the last position block runs 12 positions past the window: written, never
  // read -- no per-position test in the write loop); position column c owns z columns 2 c + 4, 2 c + 5 (8-byte aligned
  // pairs; the blur reads the aligned 16-byte pieces 4 og + 4 .. 4 og + 11 and uses seven of them)
  constexpr int ZR = 2 * PR + 2, CHS = ZR * TC_ZP + 4;
  constexpr int SR = 4, CT = 512;                   // output rows of a strip; threads of the blur (all)
  static_assert(SI == 2 && BPW == 24 / MW && (MW == 4 || MW == 8) && SR * (CT / 128) == 2 * TY, "piece / block / strip counts the code below is written for");
  constexpr bool STAGERS_BLUR = MW == 4;            // (MW == 8: the 512 threads of the multiplying waves are the blur's)
  __shared__ __attribute__((aligned(16))) unsigned char Ls[2 * BUFB];
  __shared__ __attribute__((aligned(16))) unsigned char Wl[2 * TC_WCH];
  __shared__ __attribute__((aligned(16))) float Zs[8 * CHS];
  __shared__ float Sc[2][16], Bs[2][16], Po[2][16], Kf[16], Ks[12];   // Ks: kh[4], kv[4], [8] = 1 when the FIR is kv x kh

  const int tid = threadIdx.x, lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int64_t hw = (int64_t)p.h * p.w;
  const int NC = p.in_ch >> 4, T = 9 * NC;
  const float gain = p.act ? 1.4142135623730951f : 1.f, slope = p.act ? 0.2f : 1.f;

  // this workgroup's run: tile k * grid + bx (ot fastest, then x, y, image); those running at the same time are neighbours
  const int64_t total = (int64_t)p.batch * p.tiles_y * p.tiles_x * p.o_tiles;
  const int bx = rw_xcd_remap(blockIdx.x, gridDim.x);
  const int count = (int)((total - bx + gridDim.x - 1) / gridDim.x);
  if (count <= 0) {                                 // (every wave of the launch owns a slot of the bound: rw_common.h)
    if (p.y_amax) rw_bound_store_wave(p.y_amax, 0.f);
    return;
  }
  const int N = count * NC;                         // chunks of the run
  // tile coordinates: (ot, tx, ty, ib) of tile bx once, then + the grid's digits per step (rw_tile_walk, rw_common.h)
  const rw_tile_walk<TconvProblem> walk(p);
  if (tid < 16) {
    const int a = tid >> 2, c = tid & 3;
    Kf[tid] = p.k4[(3 - a) * 4 + (3 - c)];          // flipped, as upfirdn2d applies it (read after the first barrier)
  }

  // ---- the blur of one pass (every thread): strip = four output columns x SR rows of one channel
  const float noise_wg = p.noise ? p.noise_w[0] * gain : 0.f;
  const int W2 = 2 * p.w;
  const int64_t hw2 = 4 * hw;
  const int strip = tid & 127, seg = tid >> 7;
  const int s_og = strip & 15, s_ch = strip >> 4, s_oy0 = SR * seg;
  rw_f32x4 nzr[SR];
#pragma unroll
  for (int oy = 0; oy < SR; ++oy) nzr[oy] = rw_f32x4{0.f, 0.f, 0.f, 0.f};
  float ymax = 0.f;
  // is the FIR an outer product kv x kh?  (tconv_body; kh, kv and the answer live in LDS: every register counts beside the
  // multiplying waves' accumulators and operands.)  Thread 0 decides, before the first barrier.
  auto fir_setup = [&]() __attribute__((always_inline)) {
    if (tid == 0) {
      float kf[16], kvv[4], kmax = 0.f;
#pragma unroll
      for (int t = 0; t < 16; ++t) { kf[t] = p.k4[(3 - (t >> 2)) * 4 + (3 - (t & 3))]; kmax = fmaxf(kmax, fabsf(kf[t])); }
      bool ok = kf[0] != 0.f;
#pragma unroll
      for (int a = 0; a < 4; ++a) { kvv[a] = ok ? kf[4 * a] / kf[0] : 0.f; Ks[a] = kf[a]; Ks[4 + a] = kvv[a]; }
#pragma unroll
      for (int t = 0; t < 16; ++t) ok = ok && fabsf(kf[t] - kvv[t >> 2] * kf[t & 3]) <= 1e-6f * kmax;
      Ks[8] = ok ? 1.f : 0.f;
    }
  };
  fir_setup();
  // the strip's noise (the same in both passes), requested a chunk of MFMAs before the epilogue
  auto noise_request = [&](int ty, int tx, int ib) __attribute__((always_inline)) {
    if (Ks[8] != 0.f && p.noise) {
      const int64_t s_pix = (int64_t)(2 * ty * TY + s_oy0) * W2 + 2 * tx * TC_TX + 4 * s_og;
#pragma unroll
      for (int oy = 0; oy < SR; ++oy)
        nzr[oy] = *reinterpret_cast<const rw_f32x4*>(p.noise + (int64_t)ib * hw2 + s_pix + (int64_t)oy * W2);
    }
  };
  auto blur = [&](int pass, int par, int ot, int tx, int ty, int ib) __attribute__((always_inline)) {
    if (Ks[8] != 0.f) {
      const float kh[4] = {Ks[0], Ks[1], Ks[2], Ks[3]}, kv[4] = {Ks[4], Ks[5], Ks[6], Ks[7]};
      const int cl = 8 * pass + s_ch;               // channel within the workgroup's 16
      const int64_t s_pix = (int64_t)(2 * ty * TY + s_oy0) * W2 + 2 * tx * TC_TX + 4 * s_og;
      const float* zb = Zs + s_ch * CHS + (s_oy0 + 1) * TC_ZP + 4 * s_og + 4;
      const float sc = Sc[par][cl], bs = Bs[par][cl], post = Po[par][cl];
      float* yb = p.y + ((int64_t)ib * p.out_ch + 16 * ot + cl) * hw2 + s_pix;
      rw_f32x4 hrow[4];                             // the last four horizontally filtered rows
      rw_f32x4 lo = *reinterpret_cast<const rw_f32x4*>(zb), hi = *reinterpret_cast<const rw_f32x4*>(zb + 4);
#pragma unroll
      for (int zr = 0; zr < SR + 3; ++zr) {
        rw_f32x4 lon = lo, hin = hi;                // the next z row, requested before this one is filtered
        if (zr + 1 < SR + 3) {
          lon = *reinterpret_cast<const rw_f32x4*>(zb + (zr + 1) * TC_ZP);
          hin = *reinterpret_cast<const rw_f32x4*>(zb + (zr + 1) * TC_ZP + 4);
        }
        rw_f32x4 hsum = rw_f32x4{lo[1], lo[2], lo[3], hi[0]} * kh[0];
        hsum += rw_f32x4{lo[2], lo[3], hi[0], hi[1]} * kh[1];
        hsum += rw_f32x4{lo[3], hi[0], hi[1], hi[2]} * kh[2];
        hsum += hi * kh[3];
        hrow[zr & 3] = hsum;
        if (zr >= 3) {
          const int oy = zr - 3;                    // output row oy0 + oy: filtered rows zr - 3 .. zr
          rw_f32x4 res = hrow[(zr - 3) & 3] * kv[0];
          res += hrow[(zr - 2) & 3] * kv[1];
          res += hrow[(zr - 1) & 3] * kv[2];
          res += hrow[zr & 3] * kv[3];
          const rw_f32x4 nz = nzr[oy] * noise_wg;
          rw_f32x4 v;
#pragma unroll
          for (int q = 0; q < 4; ++q) {
            const float u = res[q] * sc + nz[q] + bs;
            v[q] = fmaxf(u, u * slope) * post;
            ymax = fmaxf(ymax, fabsf(v[q]));
          }
          *reinterpret_cast<rw_f32x4*>(yb + (int64_t)oy * W2) = v;
        }
        __builtin_amdgcn_sched_barrier(0);
        lo = lon; hi = hin;
      }
    } else {
#pragma unroll 1
      for (int k = 0; k < 8 * 2 * TY * 16 / CT; ++k) {
        const int gid = tid + CT * k;               // 8 channels x 2 TY rows x 16 groups of four outputs
        const int og = gid & 15, oy = (gid >> 4) % (2 * TY), ch = gid / (32 * TY);
        const float* zb = Zs + ch * CHS + (oy + 1) * TC_ZP + 4 * og + 4;
        float res[4] = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
        for (int a = 0; a < 4; ++a) {
          const rw_f32x4 lo = *reinterpret_cast<const rw_f32x4*>(zb + a * TC_ZP);
          const rw_f32x4 hi = *reinterpret_cast<const rw_f32x4*>(zb + a * TC_ZP + 4);
          const float rowv[7] = {lo[1], lo[2], lo[3], hi[0], hi[1], hi[2], hi[3]};
#pragma unroll
          for (int q = 0; q < 4; ++q)
#pragma unroll
            for (int cc = 0; cc < 4; ++cc) res[q] += rowv[q + cc] * Kf[a * 4 + cc];
        }
        const int cg = 8 * pass + ch;
        const int64_t pix = (int64_t)(2 * ty * TY + oy) * W2 + 2 * tx * TC_TX + 4 * og;
        rw_f32x4 nz = {0.f, 0.f, 0.f, 0.f};
        if (p.noise) nz = *reinterpret_cast<const rw_f32x4*>(p.noise + (int64_t)ib * hw2 + pix) * noise_wg;
        const float sc = Sc[par][cg], bs = Bs[par][cg], post = Po[par][cg];
        rw_f32x4 v;
#pragma unroll
        for (int q = 0; q < 4; ++q) {
          const float u = res[q] * sc + nz[q] + bs;
          v[q] = fmaxf(u, u * slope) * post;
          ymax = fmaxf(ymax, fabsf(v[q]));
        }
        *reinterpret_cast<rw_f32x4*>(p.y + ((int64_t)ib * p.out_ch + 16 * ot + cg) * hw2 + pix) = v;
      }
    }
  };

  if (wave >= MW) {
    // =========================== staging waves: channel quad g of every chunk ===========================
    const int g = wave - MW, lid = g * 64 + lane;
    const float xam = rw_bound_load(p.x_amax);
    const int hw4 = (int)hw * 4;
    int l_pos = 0, l_c = 0, l_ib = -1, l_ot, l_tx, l_ty, l_ibn;       // (l_ot, l_tx, l_ty, l_ibn): the tile being requested
    bool l_past = false;
    rw_tile_digits(p, (unsigned)bx, l_ot, l_tx, l_ty, l_ibn);
    float in_scale = 1.f, out_scale = 1.f;
    int xoff[SI];
    __amdgpu_buffer_rsrc_t xsrc = __builtin_amdgcn_make_buffer_rsrc(const_cast<float*>(p.x), 0, 0, 0x00020000);
    // Two chunks are in flight at any time (registers: slot n & 1 holds chunk n's window pieces, weight pieces and
    // scalars): chunk n + 3 is requested when chunk n + 1 has been written -- two intervals between a request and its use
    // (one left layer 17 waiting: 1.3 of 6.5 ms disappeared with the window loads, profiles/r05u)
    struct Flight {
      rw_f32x4 raw[SI][4];                          // [piece][channel]: four pixels
      float psv[4];
      float demod, bias, post, oscale, iscale;
      bool first;
      int par;
    };
    Flight fl[2];
    // (the weights come from the L2 and stay ONE interval ahead: tap pieces g, g + 4 and (g == 0) 8 of the chunk after the
    // one being written; w_next = where the chunk requested last finds its weights)
    rw_f32x4 wraw[3];
    float sv[4];
    int l_s0 = 0;
    const unsigned char* l_wsrc = p.wp;
    const unsigned char* w_next = p.wp;
    auto setup = [&](auto tag) __attribute__((always_inline)) {   // the chunk to REQUEST: (l_pos, l_c); loads only, none used here
      Flight& F = fl[decltype(tag)::value];
      F.first = l_c == 0 && !l_past;                              // (past the run: the last chunk again, never read)
      if (F.first) {
        const int ib = l_ibn;
        const int i0 = l_ty * TY, j0 = l_tx * TC_TX;
        if (ib != l_ib) {
          l_ib = ib;
          const float smax = rw_style_absmax_wave(p, ib, lane);
          rw_split_scales<14>(xam * smax, p.u_inv, in_scale, out_scale);      // headroom 14: V itself is split
          xsrc = rw_image_rsrc(p.x, ib, p.in_ch, hw);
        }
#pragma unroll
        for (int s = 0; s < SI; ++s) {
          const int it = 64 * s + lane;
          const int r = it / IPR, j = it - r * IPR;
          const int iy = i0 - 2 + r, ix = j0 - 4 + 4 * j;            // the item lies inside the row or outside it as a whole
          const bool ok = it < NITEM && iy >= 0 && iy < p.h && ix >= 0 && ix < p.w;
          xoff[s] = ok ? (iy * p.w + ix) * 4 : 0x7ffffff0;
        }
        F.par = l_pos & 1;
        F.oscale = out_scale;
        if (lid < 16) {
          const int o = 16 * l_ot + lid;
          F.demod = p.demod ? p.demod[(int64_t)l_ib * p.out_ch + o] : 1.f;
          F.bias = p.act ? p.bias[o] : 0.f;
          F.post = p.post ? p.post[(int64_t)l_ib * p.out_ch + o] : 1.f;
        }
      }
#pragma unroll
      for (int k = 0; k < 4; ++k) F.psv[k] = p.style ? p.style[(int64_t)l_ib * p.in_ch + 16 * l_c + 4 * g + k] : 1.f;
      F.iscale = in_scale;
      l_s0 = (16 * l_c + 4 * g) * hw4;
      l_wsrc = w_next;                              // the weights of the chunk set up ONE call ago
      w_next = p.wp + ((int64_t)l_ot * T + 9 * l_c) * 1024 + lane * 16;
      if (++l_c == NC) {
        if (l_pos + 1 < count) { l_c = 0; ++l_pos; walk.advance(l_ot, l_tx, l_ty, l_ibn); }
        else { l_c = NC - 1; l_past = true; }
      }
    };
    auto request_s = [&](auto tag, int s, bool with_w = true) __attribute__((always_inline)) {
      Flight& F = fl[decltype(tag)::value];
      // (the weights FIRST, all with piece 0: loads return in order -- the wait for them, an interval later, must not reach
      // past this interval's window requests)
      if (with_w && s == 0) {
        wraw[0] = *reinterpret_cast<const rw_f32x4*>(l_wsrc + g * 1024);
        wraw[1] = *reinterpret_cast<const rw_f32x4*>(l_wsrc + (g + 4) * 1024);
        if (g == 0) wraw[2] = *reinterpret_cast<const rw_f32x4*>(l_wsrc + 8 * 1024);
      }
#pragma unroll
      for (int k = 0; k < 4; ++k)
        F.raw[s][k] = __builtin_bit_cast(rw_f32x4, __builtin_amdgcn_raw_buffer_load_b128(xsrc, xoff[s], l_s0 + k * hw4, 0));
    };
    // what setup() requested beside the pixels -> registers / LDS (the first wait of an interval)
    auto tables = [&](auto tag) __attribute__((always_inline)) {
      Flight& F = fl[decltype(tag)::value];
#pragma unroll
      for (int k = 0; k < 4; ++k) sv[k] = F.psv[k] * F.iscale;
      if (F.first && lid < 16) {
        Sc[F.par][lid] = F.demod * p.w_scale * F.oscale * gain;
        Bs[F.par][lid] = F.bias * gain;
        Po[F.par][lid] = F.post;
      }
    };
    auto deliver_s = [&](auto tag, int buf, int s) __attribute__((always_inline)) {
      Flight& F = fl[decltype(tag)::value];
      unsigned char* dst = Ls + buf * BUFB;
      unsigned char* wdst = Wl + buf * TC_WCH + lane * 16;
      if (s == 0) {
        *reinterpret_cast<rw_f32x4*>(wdst + g * 1024) = wraw[0];
        *reinterpret_cast<rw_f32x4*>(wdst + (g + 4) * 1024) = wraw[1];
        if (g == 0) *reinterpret_cast<rw_f32x4*>(wdst + 8 * 1024) = wraw[2];
      }
      const int it = 64 * s + lane;
      const int r = it / IPR, j = it - r * IPR;
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        const float v0 = F.raw[s][0][e] * sv[0], v1 = F.raw[s][1][e] * sv[1], v2 = F.raw[s][2][e] * sv[2],
                    v3 = F.raw[s][3][e] * sv[3];
        const rw_f16x8 word = rw_split4(v0, v1, v2, v3);
        const int cc = 4 * j - 2 + e;                // window column of this pixel
        if (it < NITEM && cc >= 0 && cc < TC_WC)
          *reinterpret_cast<rw_f16x8*>(dst + (r * TC_WC + cc) * 64 + ((g ^ rw_swz(cc)) << 4)) = word;
      }
    };

    // chunks 0 and 1 requested (chunk 0's weights with chunk 1's window); chunk 0 written; chunk 2 requested
    setup(rw_int<0>());
#pragma unroll
    for (int s = 0; s < SI; ++s) request_s(rw_int<0>(), s, false);
    setup(rw_int<1>());
#pragma unroll
    for (int s = 0; s < SI; ++s) request_s(rw_int<1>(), s);
    tables(rw_int<0>());
    __builtin_amdgcn_sched_barrier(0);
    setup(rw_int<0>());
#pragma unroll
    for (int s = 0; s < SI; ++s) {
      deliver_s(rw_int<0>(), 0, s); __builtin_amdgcn_sched_barrier(0);
      request_s(rw_int<0>(), s); __builtin_amdgcn_sched_barrier(0);
    }
    rw_lds_barrier();
    int cn = 0, e_pos = 0;                          // the tile the multiplying waves are on (its epilogue is shared)
    int e_ot, e_tx, e_ty, e_ib;
    rw_tile_digits(p, (unsigned)bx, e_ot, e_tx, e_ty, e_ib);
    // interval n: chunk n + 1 (slot (n + 1) & 1, in flight for two intervals; its weights for one) -> LDS piece by piece, the
    // window of chunk n + 3 and the weights of chunk n + 2 requested behind it into the same registers (past the run:
    // harmless repeats)
    auto interval = [&](int n, auto tag) __attribute__((always_inline)) {
      tables(tag);
      __builtin_amdgcn_sched_barrier(0);
      // (the strip's noise BEFORE this interval's window requests: loads return in order, and the wait for the noise at the
      // blur must leave the younger window loads in flight)
      if (STAGERS_BLUR && cn == NC - 1) noise_request(e_ty, e_tx, e_ib);
      __builtin_amdgcn_sched_barrier(0);
      setup(tag);
#pragma unroll
      for (int s = 0; s < SI; ++s) {
        deliver_s(tag, (n + 1) & 1, s); __builtin_amdgcn_sched_barrier(0);
        request_s(tag, s); __builtin_amdgcn_sched_barrier(0);
      }
      rw_lds_barrier();
      if (++cn == NC) {                             // the tile's epilogue (the loads stay in flight)
        cn = 0;
        const int par = e_pos & 1;
        if (STAGERS_BLUR) blur(0, par, e_ot, e_tx, e_ty, e_ib);
        rw_lds_barrier();                           // z is free: the multiplying waves write the other eight channels
        rw_lds_barrier();
        if (STAGERS_BLUR) blur(1, par, e_ot, e_tx, e_ty, e_ib);
        ++e_pos;
        walk.advance(e_ot, e_tx, e_ty, e_ib);
      }
    };
    int n = 0;
    for (; n + 1 < N; n += 2) { interval(n, rw_int<1>()); interval(n + 1, rw_int<0>()); }
    if (n < N) interval(n, rw_int<1>());
    if (p.y_amax) rw_bound_store_wave(p.y_amax, rw_wave_max(ymax));
    return;
  }

  // =========================== multiplying waves ===========================
  const int lk = lane >> 4, lt = lane & 15;
  unsigned pb0[BPW], pb1[BPW];                     // operand addresses as in tconv_body
#pragma unroll
  for (int b = 0; b < BPW; ++b) {
    int q = 16 * (wave + MW * b) + lt;
    q = q < NPOS ? q : NPOS - 1;
    const int r = q / TC_PC, c = q - r * TC_PC;
    pb0[b] = (unsigned)(((r + 1) * TC_WC + c + 1) * 64 + ((lk ^ rw_swz(c + 1)) << 4));
    pb1[b] = (unsigned)(((r + 1) * TC_WC + c) * 64 + ((lk ^ rw_swz(c)) << 4));
  }
  rw_f32x4 acc[BPW][4];
#pragma unroll
  for (int b = 0; b < BPW; ++b)
#pragma unroll
    for (int ph = 0; ph < 4; ++ph) acc[b][ph] = rw_f32x4{0.f, 0.f, 0.f, 0.f};
  constexpr int LB = BPW - 1;
  const bool last_ok = wave + MW * LB < NBLK;       // wave-uniform: only the last block of a wave can be missing
  // One chunk: the three tap groups of tconv_body's chunk() (at most five weight operands live), the pixel operands of a
  // block requested TWO blocks ahead -- a group gives a block four or five MFMAs (90 - 110 cycles with one multiplying
  // wave per SIMD), less than an LDS round trip beside the staging waves' traffic: 36 cycles per MFMA with the operands one
  // block ahead (profiles/r05p).  (All fourteen weight operands live and fourteen MFMAs per block would cover it too: 35
  // registers more than there are.)
  auto mma = [&](const unsigned char* lb, const unsigned char* wb) __attribute__((always_inline)) {
    {
      const rw_f16x8 u0 = TC_UH(0), u1 = TC_UH(1), u3 = TC_UH(3), u4 = TC_UH(4), l4 = rw_expand(TC_UL(4));
      rw_f16x8 pc = TC_PIX(pb0[0]), pd = TC_PIX(pb0[1]);
#pragma unroll
      for (int b = 0; b < BPW; ++b) {
        rw_f16x8 pn = pd;
        if (b + 2 < BPW) pn = TC_PIX(pb0[b + 2]);
        if (b < LB || last_ok) {
          TC_MFMA(3, pc, u4); TC_MFMA(0, pc, u0); TC_MFMA(1, pc, u1); TC_MFMA(2, pc, u3);
          TC_MFMA(3, pc, l4);
        }
        __builtin_amdgcn_sched_barrier(0);
        pc = pd; pd = pn;
      }
    }
    {
      const rw_f16x8 u2 = TC_UH(2), u5 = TC_UH(5), m02 = rw_pair(TC_UL(0), TC_UL(2)), m35 = rw_pair(TC_UL(3), TC_UL(5));
      rw_f32x2 hc = TC_VH(pb0[0]), hd = TC_VH(pb0[1]);
      rw_f16x8 qc = TC_PIX(pb1[0]), qd = TC_PIX(pb1[1]);
#pragma unroll
      for (int b = 0; b < BPW; ++b) {
        rw_f32x2 hn = hd;
        rw_f16x8 qn = qd;
        if (b + 2 < BPW) { hn = TC_VH(pb0[b + 2]); qn = TC_PIX(pb1[b + 2]); }
        if (b < LB || last_ok) {
          const rw_f16x8 M = tc_pair_hq(hc, qc);
          TC_MFMA(0, qc, u2); TC_MFMA(2, qc, u5);
          TC_MFMA(0, M, m02); TC_MFMA(2, M, m35);
        }
        __builtin_amdgcn_sched_barrier(0);
        hc = hd; qc = qd; hd = hn; qd = qn;
      }
    }
    {
      const rw_f16x8 u6 = TC_UH(6), u7 = TC_UH(7), u8 = TC_UH(8), m17 = rw_pair(TC_UL(1), TC_UL(7)),
                     m68 = rw_pair(TC_UL(6), TC_UL(8));
      rw_f32x2 hc = TC_VH(pb0[0]), hd = TC_VH(pb0[1]);
      rw_f16x8 qc = TC_PIX(pb0[0] - TC_WC * 64), rc = TC_PIX(pb1[0] - TC_WC * 64);
      rw_f16x8 qd = TC_PIX(pb0[1] - TC_WC * 64), rd = TC_PIX(pb1[1] - TC_WC * 64);
#pragma unroll
      for (int b = 0; b < BPW; ++b) {
        rw_f32x2 hn = hd;
        rw_f16x8 qn = qd, rn = rd;
        if (b + 2 < BPW) { hn = TC_VH(pb0[b + 2]); qn = TC_PIX(pb0[b + 2] - TC_WC * 64); rn = TC_PIX(pb1[b + 2] - TC_WC * 64); }
        if (b < LB || last_ok) {
          const rw_f16x8 M02 = tc_pair_hq(hc, qc), M23 = rw_pair(qc, rc);
          TC_MFMA(0, qc, u6); TC_MFMA(1, qc, u7);
          TC_MFMA(0, rc, u8); TC_MFMA(1, M02, m17);
          TC_MFMA(0, M23, m68);
        }
        __builtin_amdgcn_sched_barrier(0);
        hc = hd; qc = qd; rc = rd; hd = hn; qd = qn; rd = rn;
      }
    }
  };
  // eight of the sixteen channels -> the z tile (lanes lt >> 3 == pass hold them).  A lane's four positions of a block are
  // consecutive: one division per block, then + 2 floats per position and + 76 (a z row pair is 144, a position row 68)
  // where the run crosses the end of a position row
  auto zwrite = [&](int pass) __attribute__((always_inline)) {
    if ((lt >> 3) == pass) {
      // (the addresses are loop invariants: left to itself the compiler keeps all of them in registers for the whole run;
      // an opaque zero keeps their few instructions inside the loop)
      int opaque;
      asm volatile("v_mov_b32 %0, 0" : "=v"(opaque));
      float* zc = Zs + (lt & 7) * CHS + 4;
#pragma unroll
      for (int b = 0; b < BPW; ++b) {
        if (wave + MW * b >= NBLK) continue;
        const int q0 = 16 * (wave + MW * b) + 4 * lk + opaque;         // < 352: the spare rows take what lies past the window
        const int r0 = (q0 * 1928) >> 16, c0 = q0 - r0 * TC_PC;        // q0 / 34 for q0 < 400
        float* z0 = zc + (2 * r0) * TC_ZP + 2 * c0;
#pragma unroll
        for (int j = 0; j < 4; ++j) {
          float* zp = z0 + 2 * j + (c0 + j >= TC_PC ? 2 * TC_ZP - 2 * TC_PC : 0);
          // (four dword stores: the compiler pairs them into ds_write2_b32 -- two separate source registers each; as 8-byte
          // vectors every pair cost two moves to bring accumulators of different blocks side by side)
          zp[0] = acc[b][0][j];
          zp[1] = acc[b][1][j];
          zp[TC_ZP] = acc[b][2][j];
          zp[TC_ZP + 1] = acc[b][3][j];
        }
      }
    }
  };

  int pos = 0, c = 0;
  int ot, tx, ty, ib;
  rw_tile_digits(p, (unsigned)bx, ot, tx, ty, ib);
  rw_lds_barrier();                                 // chunk 0 and the FIR are in LDS
  for (int n = 0; n < N; ++n) {
    const unsigned char* lb = Ls + (n & 1) * BUFB;
    const unsigned char* wb = Wl + (n & 1) * TC_WCH + lane * 8;
    mma(lb, wb);
    if (c + 1 < NC) { ++c; rw_lds_barrier(); continue; }
    // ---- epilogue of the tile, eight channels at a time
    c = 0;
    const int par = pos & 1;
    noise_request(ty, tx, ib);                      // (behind the MFMAs: sixteen registers they need; the z write and a barrier cover it)
    zwrite(0);
    rw_lds_barrier();                               // (the barrier of the tile's last chunk)
    blur(0, par, ot, tx, ty, ib);
    rw_lds_barrier();                               // every strip of the first eight channels is read: z is free again
    zwrite(1);
    rw_lds_barrier();
    blur(1, par, ot, tx, ty, ib);
#pragma unroll
    for (int b = 0; b < BPW; ++b)
#pragma unroll
      for (int ph = 0; ph < 4; ++ph) acc[b][ph] = rw_f32x4{0.f, 0.f, 0.f, 0.f};
    ++pos;
    walk.advance(ot, tx, ty, ib);
  }
  if (p.y_amax) rw_bound_store_wave(p.y_amax, rw_wave_max(ymax));
}
__global__ void __launch_bounds__(512, 2) tconv_blur_ws_kernel(const TconvProblem p) { tconv_ws_body<4>(p); }
__global__ void __launch_bounds__(768, 1) tconv_blur_ws12_kernel(const TconvProblem p) { tconv_ws_body<8>(p); }

// ---------------------------------------------------------------------------------------
// Fourth form (round 6): the persistent kernel above with its two halves PIPELINED across tiles.  There the phases of a
// tile take turns -- all eight waves wait while four multiply, the matrix pipe idles while all eight blur (27 - 29 k cycles
// per tile on layer 17: multiplies 10 k, z write 4 k in two half-lane passes, blur 8 k of vector issue per SIMD, waits).
// Here the z tile holds all SIXTEEN channels (20 rows: the last position block tests its positions instead of writing
// into spare rows -- 92 KB, 161 KB of LDS with the windows and the weights) and
//   waves 0..3 multiply tile t, then write ITS z tile in one pass with every lane active (one barrier before: z is free;
//     one behind: z is ready), and go on to tile t + 1;
//   waves 4..7 stage as before AND blur tile t - 1 meanwhile: four passes of four channels (256 strips of four columns x
//     four rows each), spread over the chunk intervals of tile t, the noise of the tile requested at the switch.
// The vector work of a tile (staging conversion + blur) runs beside the matrix work of the next one; NC + 1 barriers per
// tile.  The staging waves' LDS addresses are computed once (the window's geometry does not change from chunk to chunk).
// Tables (demodulation x scales, bias, post scale) are kept for FOUR tiles (tile index & 3): the tile being requested is two
// ahead of the one being blurred.
// ---------------------------------------------------------------------------------------
__global__ void __launch_bounds__(512, 2) tconv_blur_pp_kernel(const TconvProblem p) {
  constexpr int TY = 8, MW = 4;
  constexpr int PR = TY + 2, NPOS = PR * TC_PC, NBLK = (NPOS + 15) / 16, BPW = (NBLK + MW - 1) / MW;
  constexpr int WR = TY + 3, NPIX = WR * TC_WC, BUFB = NPIX * 64;
  constexpr int IPR = TC_TX / 4 + 2, NITEM = WR * IPR, SI = (NITEM + 63) / 64;   // items: window columns 4 j - 2 .. 4 j + 1
  constexpr int ZR = 2 * PR, CHS = ZR * TC_ZP + 4;  // z rows 0 .. 2 PR - 1; position column c owns z columns 2 c + 4, 2 c + 5
  constexpr int SR = 4;                             // output rows of a strip
  static_assert(SI == 2 && BPW == 6 && 4 * SR == 2 * TY, "piece / block / strip counts the code below is written for");
  static_assert(2 * BUFB + 2 * TC_WCH + 16 * CHS * 4 + 1024 <= 163840, "LDS of a compute unit");
  __shared__ __attribute__((aligned(16))) unsigned char Ls[2 * BUFB];
  __shared__ __attribute__((aligned(16))) unsigned char Wl[2 * TC_WCH];
  __shared__ __attribute__((aligned(16))) float Zs[16 * CHS];
  __shared__ float Sc[4][16], Bs[4][16], Po[4][16], Kf[16], Ks[12];   // Ks: kh[4], kv[4], [8] = 1 when the FIR is kv x kh

  const int tid = threadIdx.x, lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int64_t hw = (int64_t)p.h * p.w;
  const int NC = p.in_ch >> 4, T = 9 * NC;
  const float gain = p.act ? 1.4142135623730951f : 1.f, slope = p.act ? 0.2f : 1.f;

  const int64_t total = (int64_t)p.batch * p.tiles_y * p.tiles_x * p.o_tiles;
  const int bx = rw_xcd_remap(blockIdx.x, gridDim.x);
  const int count = (int)((total - bx + gridDim.x - 1) / gridDim.x);
  if (count <= 0) {                                 // (every wave of the launch owns a slot of the bound: rw_common.h)
    if (p.y_amax) rw_bound_store_wave(p.y_amax, 0.f);
    return;
  }
  const int N = count * NC;                         // chunks of the run
  const rw_tile_walk<TconvProblem> walk(p);
  if (tid < 16) {
    const int a = tid >> 2, c = tid & 3;
    Kf[tid] = p.k4[(3 - a) * 4 + (3 - c)];          // flipped, as upfirdn2d applies it (read after the first barrier)
  }
  if (tid == 0) {                                   // is the FIR an outer product kv x kh?  (tconv_body)
    float kf[16], kvv[4], kmax = 0.f;
#pragma unroll
    for (int t = 0; t < 16; ++t) { kf[t] = p.k4[(3 - (t >> 2)) * 4 + (3 - (t & 3))]; kmax = fmaxf(kmax, fabsf(kf[t])); }
    bool ok = kf[0] != 0.f;
#pragma unroll
    for (int a = 0; a < 4; ++a) { kvv[a] = ok ? kf[4 * a] / kf[0] : 0.f; Ks[a] = kf[a]; Ks[4 + a] = kvv[a]; }
#pragma unroll
    for (int t = 0; t < 16; ++t) ok = ok && fabsf(kf[t] - kvv[t >> 2] * kf[t & 3]) <= 1e-6f * kmax;
    Ks[8] = ok ? 1.f : 0.f;
  }

  // ---- the blur (both roles): strip = four output columns x SR rows of one channel; wave (w & 3) owns the rows SR (w & 3) ..,
  // a pass covers four channels with the 256 threads of a role
  const int bw = wave & 3, lid = bw * 64 + lane;
  const float noise_wg = p.noise ? p.noise_w[0] * gain : 0.f;
  const int W2 = 2 * p.w;
  const int64_t hw2 = 4 * hw;
  const int s_og = lane & 15, s_chl = lane >> 4, s_oy0 = SR * bw;
  rw_f32x4 nzr[SR];
#pragma unroll
  for (int oy = 0; oy < SR; ++oy) nzr[oy] = rw_f32x4{0.f, 0.f, 0.f, 0.f};
  float ymax = 0.f;
  auto noise_request = [&](int ty, int tx, int ib) __attribute__((always_inline)) {
    if (p.noise) {
      const int64_t s_pix = (int64_t)(2 * ty * TY + s_oy0) * W2 + 2 * tx * TC_TX + 4 * s_og;
#pragma unroll
      for (int oy = 0; oy < SR; ++oy)
        nzr[oy] = *reinterpret_cast<const rw_f32x4*>(p.noise + (int64_t)ib * hw2 + s_pix + (int64_t)oy * W2);
    }
  };
  auto blur = [&](int pass, int par, int ot, int tx, int ty, int ib) __attribute__((always_inline)) {
    if (Ks[8] != 0.f) {
      const float kh[4] = {Ks[0], Ks[1], Ks[2], Ks[3]}, kv[4] = {Ks[4], Ks[5], Ks[6], Ks[7]};
      const int cl = 4 * pass + s_chl;            // channel within the workgroup's 16
      const int64_t s_pix = (int64_t)(2 * ty * TY + s_oy0) * W2 + 2 * tx * TC_TX + 4 * s_og;
      const float* zb = Zs + cl * CHS + (s_oy0 + 1) * TC_ZP + 4 * s_og + 4;
      const float sc = Sc[par][cl], bs = Bs[par][cl], post = Po[par][cl];
      float* yb = p.y + ((int64_t)ib * p.out_ch + 16 * ot + cl) * hw2 + s_pix;
      rw_f32x4 hrow[4];                           // the last four horizontally filtered rows
      rw_f32x4 lo = *reinterpret_cast<const rw_f32x4*>(zb), hi = *reinterpret_cast<const rw_f32x4*>(zb + 4);
#pragma unroll
      for (int zr = 0; zr < SR + 3; ++zr) {
        rw_f32x4 lon = lo, hin = hi;              // the next z row, requested before this one is filtered
        if (zr + 1 < SR + 3) {
          lon = *reinterpret_cast<const rw_f32x4*>(zb + (zr + 1) * TC_ZP);
          hin = *reinterpret_cast<const rw_f32x4*>(zb + (zr + 1) * TC_ZP + 4);
        }
        rw_f32x4 hsum = rw_f32x4{lo[1], lo[2], lo[3], hi[0]} * kh[0];
        hsum += rw_f32x4{lo[2], lo[3], hi[0], hi[1]} * kh[1];
        hsum += rw_f32x4{lo[3], hi[0], hi[1], hi[2]} * kh[2];
        hsum += hi * kh[3];
        hrow[zr & 3] = hsum;
        if (zr >= 3) {
          const int oy = zr - 3;                  // output row oy0 + oy: filtered rows zr - 3 .. zr
          rw_f32x4 res = hrow[(zr - 3) & 3] * kv[0];
          res += hrow[(zr - 2) & 3] * kv[1];
          res += hrow[(zr - 1) & 3] * kv[2];
          res += hrow[zr & 3] * kv[3];
          const rw_f32x4 nz = nzr[oy] * noise_wg;
          rw_f32x4 v;
#pragma unroll
          for (int q = 0; q < 4; ++q) {
            const float u = res[q] * sc + nz[q] + bs;
            v[q] = fmaxf(u, u * slope) * post;
            ymax = fmaxf(ymax, fabsf(v[q]));
          }
          *reinterpret_cast<rw_f32x4*>(yb + (int64_t)oy * W2) = v;
        }
        __builtin_amdgcn_sched_barrier(0);
        lo = lon; hi = hin;
      }
    } else {
#pragma unroll 1
      for (int k = 0; k < 4; ++k) {
        const int gid = lid + 256 * k;            // 4 channels x 2 TY rows x 16 groups of four outputs
        const int og = gid & 15, oy = (gid >> 4) & (2 * TY - 1), ch = gid >> 8;
        const int cg = 4 * pass + ch;
        const float* zb = Zs + cg * CHS + (oy + 1) * TC_ZP + 4 * og + 4;
        float res[4] = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
        for (int a = 0; a < 4; ++a) {
          const rw_f32x4 lo = *reinterpret_cast<const rw_f32x4*>(zb + a * TC_ZP);
          const rw_f32x4 hi = *reinterpret_cast<const rw_f32x4*>(zb + a * TC_ZP + 4);
          const float rowv[7] = {lo[1], lo[2], lo[3], hi[0], hi[1], hi[2], hi[3]};
#pragma unroll
          for (int q = 0; q < 4; ++q)
#pragma unroll
            for (int cc = 0; cc < 4; ++cc) res[q] += rowv[q + cc] * Kf[a * 4 + cc];
        }
        const int64_t pix = (int64_t)(2 * ty * TY + oy) * W2 + 2 * tx * TC_TX + 4 * og;
        rw_f32x4 nz = {0.f, 0.f, 0.f, 0.f};
        if (p.noise) nz = *reinterpret_cast<const rw_f32x4*>(p.noise + (int64_t)ib * hw2 + pix) * noise_wg;
        const float sc = Sc[par][cg], bs = Bs[par][cg], post = Po[par][cg];
        rw_f32x4 v;
#pragma unroll
        for (int q = 0; q < 4; ++q) {
          const float u = res[q] * sc + nz[q] + bs;
          v[q] = fmaxf(u, u * slope) * post;
          ymax = fmaxf(ymax, fabsf(v[q]));
        }
        *reinterpret_cast<rw_f32x4*>(p.y + ((int64_t)ib * p.out_ch + 16 * ot + cg) * hw2 + pix) = v;
      }
    }
  };

  if (wave >= MW) {
    // =========================== staging + blurring waves ===========================
    const int g = wave - MW;
    const float xam = rw_bound_load(p.x_amax);
    const int hw4 = (int)hw * 4;
    int l_pos = 0, l_c = 0, l_ib = -1, l_ot, l_tx, l_ty, l_ibn;       // (l_ot, l_tx, l_ty, l_ibn): the tile being requested
    bool l_past = false;
    rw_tile_digits(p, (unsigned)bx, l_ot, l_tx, l_ty, l_ibn);
    float in_scale = 1.f, out_scale = 1.f;
    int xoff[SI];
    // where a lane's pixels go in a window buffer: the same for every chunk and tile (-1: outside the window)
    int ldst[SI][4];
#pragma unroll
    for (int s = 0; s < SI; ++s) {
      const int it = 64 * s + lane;
      const int r = it / IPR, j = it - r * IPR;
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        const int cc = 4 * j - 2 + e;               // window column of this pixel
        ldst[s][e] = (it < NITEM && cc >= 0 && cc < TC_WC) ? (r * TC_WC + cc) * 64 + ((g ^ rw_swz(cc)) << 4) : -1;
      }
    }
    __amdgpu_buffer_rsrc_t xsrc = __builtin_amdgcn_make_buffer_rsrc(const_cast<float*>(p.x), 0, 0, 0x00020000);
    struct Flight {
      rw_f32x4 raw[SI][4];                          // [piece][channel]: four pixels
      float psv[4];
      float demod, bias, post, oscale, iscale;
      bool first;
      int par;
    };
    Flight fl[2];
    rw_f32x4 wraw[3];
    float sv[4];
    int l_s0 = 0;
    const unsigned char* l_wsrc = p.wp;
    const unsigned char* w_next = p.wp;
    auto setup = [&](auto tag) __attribute__((always_inline)) {   // the chunk to REQUEST: (l_pos, l_c); loads only, none used here
      Flight& F = fl[decltype(tag)::value];
      F.first = l_c == 0 && !l_past;                              // (past the run: the last chunk again, never read)
      if (F.first) {
        const int ib = l_ibn;
        const int i0 = l_ty * TY, j0 = l_tx * TC_TX;
        if (ib != l_ib) {
          l_ib = ib;
          const float smax = rw_style_absmax_wave(p, ib, lane);
          rw_split_scales<14>(xam * smax, p.u_inv, in_scale, out_scale);      // headroom 14: V itself is split
          xsrc = rw_image_rsrc(p.x, ib, p.in_ch, hw);
        }
#pragma unroll
        for (int s = 0; s < SI; ++s) {
          const int it = 64 * s + lane;
          const int r = it / IPR, j = it - r * IPR;
          const int iy = i0 - 2 + r, ix = j0 - 4 + 4 * j;            // the item lies inside the row or outside it as a whole
          const bool ok = it < NITEM && iy >= 0 && iy < p.h && ix >= 0 && ix < p.w;
          xoff[s] = ok ? (iy * p.w + ix) * 4 : 0x7ffffff0;
        }
        F.par = l_pos & 3;
        F.oscale = out_scale;
        if (lid < 16) {
          const int o = 16 * l_ot + lid;
          F.demod = p.demod ? p.demod[(int64_t)l_ib * p.out_ch + o] : 1.f;
          F.bias = p.act ? p.bias[o] : 0.f;
          F.post = p.post ? p.post[(int64_t)l_ib * p.out_ch + o] : 1.f;
        }
      }
#pragma unroll
      for (int k = 0; k < 4; ++k) F.psv[k] = p.style ? p.style[(int64_t)l_ib * p.in_ch + 16 * l_c + 4 * g + k] : 1.f;
      F.iscale = in_scale;
      l_s0 = (16 * l_c + 4 * g) * hw4;
      l_wsrc = w_next;                              // the weights of the chunk set up ONE call ago
      w_next = p.wp + ((int64_t)l_ot * T + 9 * l_c) * 1024 + lane * 16;
      if (++l_c == NC) {
        if (l_pos + 1 < count) { l_c = 0; ++l_pos; walk.advance(l_ot, l_tx, l_ty, l_ibn); }
        else { l_c = NC - 1; l_past = true; }
      }
    };
    auto request_s = [&](auto tag, int s, bool with_w = true) __attribute__((always_inline)) {
      Flight& F = fl[decltype(tag)::value];
      if (with_w && s == 0) {                       // the weights FIRST (loads return in order)
        wraw[0] = *reinterpret_cast<const rw_f32x4*>(l_wsrc + g * 1024);
        wraw[1] = *reinterpret_cast<const rw_f32x4*>(l_wsrc + (g + 4) * 1024);
        if (g == 0) wraw[2] = *reinterpret_cast<const rw_f32x4*>(l_wsrc + 8 * 1024);
      }
#pragma unroll
      for (int k = 0; k < 4; ++k)
        F.raw[s][k] = __builtin_bit_cast(rw_f32x4, __builtin_amdgcn_raw_buffer_load_b128(xsrc, xoff[s], l_s0 + k * hw4, 0));
    };
    auto tables = [&](auto tag) __attribute__((always_inline)) {
      Flight& F = fl[decltype(tag)::value];
#pragma unroll
      for (int k = 0; k < 4; ++k) sv[k] = F.psv[k] * F.iscale;
      if (F.first && lid < 16) {
        Sc[F.par][lid] = F.demod * p.w_scale * F.oscale * gain;
        Bs[F.par][lid] = F.bias * gain;
        Po[F.par][lid] = F.post;
      }
    };
    auto deliver_s = [&](auto tag, int buf, int s) __attribute__((always_inline)) {
      Flight& F = fl[decltype(tag)::value];
      unsigned char* dst = Ls + buf * BUFB;
      unsigned char* wdst = Wl + buf * TC_WCH + lane * 16;
      if (s == 0) {
        *reinterpret_cast<rw_f32x4*>(wdst + g * 1024) = wraw[0];
        *reinterpret_cast<rw_f32x4*>(wdst + (g + 4) * 1024) = wraw[1];
        if (g == 0) *reinterpret_cast<rw_f32x4*>(wdst + 8 * 1024) = wraw[2];
      }
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        const float v0 = F.raw[s][0][e] * sv[0], v1 = F.raw[s][1][e] * sv[1], v2 = F.raw[s][2][e] * sv[2],
                    v3 = F.raw[s][3][e] * sv[3];
        // rw_split4 written out: through the helper the compiler orders this kernel's address additions differently
        const rw_f16x2 h01 = __builtin_convertvector(rw_f32x2{v0, v1}, rw_f16x2);
        const rw_f16x2 h23 = __builtin_convertvector(rw_f32x2{v2, v3}, rw_f16x2);
        float r0, r1, r2, r3;                        // v - (float)h, exact
        asm("v_fma_mix_f32 %0, -%1, 1.0, %2 op_sel_hi:[1,0,0]" : "=v"(r0) : "v"(h01), "v"(v0));
        asm("v_fma_mix_f32 %0, -%1, 1.0, %2 op_sel:[1,0,0] op_sel_hi:[1,0,0]" : "=v"(r1) : "v"(h01), "v"(v1));
        asm("v_fma_mix_f32 %0, -%1, 1.0, %2 op_sel_hi:[1,0,0]" : "=v"(r2) : "v"(h23), "v"(v2));
        asm("v_fma_mix_f32 %0, -%1, 1.0, %2 op_sel:[1,0,0] op_sel_hi:[1,0,0]" : "=v"(r3) : "v"(h23), "v"(v3));
        const rw_f16x2 l01 = __builtin_convertvector(rw_f32x2{r0, r1}, rw_f16x2);
        const rw_f16x2 l23 = __builtin_convertvector(rw_f32x2{r2, r3}, rw_f16x2);
        rw_f16x8 word = {h01[0], h01[1], h23[0], h23[1], l01[0], l01[1], l23[0], l23[1]};
        if (ldst[s][e] >= 0) *reinterpret_cast<rw_f16x8*>(dst + ldst[s][e]) = word;
      }
    };

    // chunks 0 and 1 requested (chunk 0's weights with chunk 1's window); chunk 0 written; chunk 2 requested
    setup(rw_int<0>());
#pragma unroll
    for (int s = 0; s < SI; ++s) request_s(rw_int<0>(), s, false);
    setup(rw_int<1>());
#pragma unroll
    for (int s = 0; s < SI; ++s) request_s(rw_int<1>(), s);
    tables(rw_int<0>());
    __builtin_amdgcn_sched_barrier(0);
    setup(rw_int<0>());
#pragma unroll
    for (int s = 0; s < SI; ++s) {
      deliver_s(rw_int<0>(), 0, s); __builtin_amdgcn_sched_barrier(0);
      request_s(rw_int<0>(), s); __builtin_amdgcn_sched_barrier(0);
    }
    rw_lds_barrier();
    int cn = 0, e_pos = 0;                          // the tile the multiplying waves are on
    int e_ot, e_tx, e_ty, e_ib;
    rw_tile_digits(p, (unsigned)bx, e_ot, e_tx, e_ty, e_ib);
    bool have_prev = false;                         // the tile whose z tile is in LDS, waiting to be blurred
    int b_ot = 0, b_tx = 0, b_ty = 0, b_ib = 0, b_par = 0;
    // interval n: chunk n + 1 -> LDS piece by piece, the window of chunk n + 3 and the weights of chunk n + 2 requested behind
    // it; then this interval's share of the previous tile's blur
    auto interval = [&](int n, auto tag) __attribute__((always_inline)) {
      tables(tag);
      __builtin_amdgcn_sched_barrier(0);
      setup(tag);
#pragma unroll
      for (int s = 0; s < SI; ++s) {
        deliver_s(tag, (n + 1) & 1, s); __builtin_amdgcn_sched_barrier(0);
        request_s(tag, s); __builtin_amdgcn_sched_barrier(0);
      }
      if (have_prev) {
        // the staging waves' passes 2 and 3 (the multiplying waves take 0 and 1), spread over the tile's intervals: pass
        // 2 + k in interval [k NC / NS]
        constexpr int NS = 2;
        const int p_lo = 2 + (NS * cn + NC - 1) / NC, p_hi = 2 + (NS * cn + NS + NC - 1) / NC;
#pragma unroll 1
        for (int ps = p_lo; ps < p_hi; ++ps) blur(ps, b_par, b_ot, b_tx, b_ty, b_ib);
      }
      rw_lds_barrier();
      if (++cn == NC) {                             // the multiplying waves write the z tile of THEIR tile now
        cn = 0;
        b_ot = e_ot; b_tx = e_tx; b_ty = e_ty; b_ib = e_ib; b_par = e_pos & 3;
        have_prev = true;
        noise_request(b_ty, b_tx, b_ib);                         // (ahead of the next interval's window requests: loads return in order)
        ++e_pos;
        walk.advance(e_ot, e_tx, e_ty, e_ib);
        rw_lds_barrier();                           // z is ready
      }
    };
    int n = 0;
    for (; n + 1 < N; n += 2) { interval(n, rw_int<1>()); interval(n + 1, rw_int<0>()); }
    if (n < N) interval(n, rw_int<1>());
    // the last tile's blur: nobody waits for it
#pragma unroll 1
    for (int ps = 2; ps < 4; ++ps) blur(ps, b_par, b_ot, b_tx, b_ty, b_ib);
    if (p.y_amax) rw_bound_store_wave(p.y_amax, rw_wave_max(ymax));
    return;
  }

  // =========================== multiplying waves ===========================
  const int lk = lane >> 4, lt = lane & 15;
  unsigned pb0[BPW], pb1[BPW];                     // operand addresses as in tconv_body
#pragma unroll
  for (int b = 0; b < BPW; ++b) {
    int q = 16 * (wave + MW * b) + lt;
    q = q < NPOS ? q : NPOS - 1;
    const int r = q / TC_PC, c = q - r * TC_PC;
    pb0[b] = (unsigned)(((r + 1) * TC_WC + c + 1) * 64 + ((lk ^ rw_swz(c + 1)) << 4));
    pb1[b] = (unsigned)(((r + 1) * TC_WC + c) * 64 + ((lk ^ rw_swz(c)) << 4));
  }
  rw_f32x4 acc[BPW][4];
#pragma unroll
  for (int b = 0; b < BPW; ++b)
#pragma unroll
    for (int ph = 0; ph < 4; ++ph) acc[b][ph] = rw_f32x4{0.f, 0.f, 0.f, 0.f};
  constexpr int LB = BPW - 1;
  const bool last_ok = wave + MW * LB < NBLK;       // wave-uniform: only the last block of a wave can be missing
  auto mma = [&](const unsigned char* lb, const unsigned char* wb) __attribute__((always_inline)) {
    {
      const rw_f16x8 u0 = TC_UH(0), u1 = TC_UH(1), u3 = TC_UH(3), u4 = TC_UH(4), l4 = rw_expand(TC_UL(4));
      rw_f16x8 pc = TC_PIX(pb0[0]), pd = TC_PIX(pb0[1]);
#pragma unroll
      for (int b = 0; b < BPW; ++b) {
        rw_f16x8 pn = pd;
        if (b + 2 < BPW) pn = TC_PIX(pb0[b + 2]);
        if (b < LB || last_ok) {
          TC_MFMA(3, pc, u4); TC_MFMA(0, pc, u0); TC_MFMA(1, pc, u1); TC_MFMA(2, pc, u3);
          TC_MFMA(3, pc, l4);
        }
        __builtin_amdgcn_sched_barrier(0);
        pc = pd; pd = pn;
      }
    }
    {
      const rw_f16x8 u2 = TC_UH(2), u5 = TC_UH(5), m02 = rw_pair(TC_UL(0), TC_UL(2)), m35 = rw_pair(TC_UL(3), TC_UL(5));
      rw_f32x2 hc = TC_VH(pb0[0]), hd = TC_VH(pb0[1]);
      rw_f16x8 qc = TC_PIX(pb1[0]), qd = TC_PIX(pb1[1]);
#pragma unroll
      for (int b = 0; b < BPW; ++b) {
        rw_f32x2 hn = hd;
        rw_f16x8 qn = qd;
        if (b + 2 < BPW) { hn = TC_VH(pb0[b + 2]); qn = TC_PIX(pb1[b + 2]); }
        if (b < LB || last_ok) {
          const rw_f16x8 M = tc_pair_hq(hc, qc);
          TC_MFMA(0, qc, u2); TC_MFMA(2, qc, u5);
          TC_MFMA(0, M, m02); TC_MFMA(2, M, m35);
        }
        __builtin_amdgcn_sched_barrier(0);
        hc = hd; qc = qd; hd = hn; qd = qn;
      }
    }
    {
      const rw_f16x8 u6 = TC_UH(6), u7 = TC_UH(7), u8 = TC_UH(8), m17 = rw_pair(TC_UL(1), TC_UL(7)),
                     m68 = rw_pair(TC_UL(6), TC_UL(8));
      rw_f32x2 hc = TC_VH(pb0[0]), hd = TC_VH(pb0[1]);
      rw_f16x8 qc = TC_PIX(pb0[0] - TC_WC * 64), rc = TC_PIX(pb1[0] - TC_WC * 64);
      rw_f16x8 qd = TC_PIX(pb0[1] - TC_WC * 64), rd = TC_PIX(pb1[1] - TC_WC * 64);
#pragma unroll
      for (int b = 0; b < BPW; ++b) {
        rw_f32x2 hn = hd;
        rw_f16x8 qn = qd, rn = rd;
        if (b + 2 < BPW) { hn = TC_VH(pb0[b + 2]); qn = TC_PIX(pb0[b + 2] - TC_WC * 64); rn = TC_PIX(pb1[b + 2] - TC_WC * 64); }
        if (b < LB || last_ok) {
          const rw_f16x8 M02 = tc_pair_hq(hc, qc), M23 = rw_pair(qc, rc);
          TC_MFMA(0, qc, u6); TC_MFMA(1, qc, u7);
          TC_MFMA(0, rc, u8); TC_MFMA(1, M02, m17);
          TC_MFMA(0, M23, m68);
        }
        __builtin_amdgcn_sched_barrier(0);
        hc = hd; qc = qd; rc = rd; hd = hn; qd = qn; rd = rn;
      }
    }
  };
  // all sixteen channels -> the z tile: lane (lk, lt) holds channel lt of the positions 4 lk .. 4 lk + 3 of each block
  auto zwrite = [&]() __attribute__((always_inline)) {
    int opaque;
    asm volatile("v_mov_b32 %0, 0" : "=v"(opaque));          // (keeps the address arithmetic inside the loop: tconv_blur_ws_kernel)
    float* zc = Zs + lt * CHS + 4;
#pragma unroll
    for (int b = 0; b < BPW; ++b) {
      if (wave + MW * b >= NBLK) continue;
      const int q0 = 16 * (wave + MW * b) + 4 * lk + opaque;
      const int r0 = (q0 * 1928) >> 16, c0 = q0 - r0 * TC_PC;          // q0 / 34 for q0 < 400
      float* z0 = zc + (2 * r0) * TC_ZP + 2 * c0;
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        if (b == BPW - 1 && q0 + j >= NPOS) continue;                  // (the last block runs past the window: no spare rows here)
        float* zp = z0 + 2 * j + (c0 + j >= TC_PC ? 2 * TC_ZP - 2 * TC_PC : 0);
        zp[0] = acc[b][0][j];
        zp[1] = acc[b][1][j];
        zp[TC_ZP] = acc[b][2][j];
        zp[TC_ZP + 1] = acc[b][3][j];
      }
    }
  };

  int c = 0, pos = 0;
  int ot, tx, ty, ib;
  rw_tile_digits(p, (unsigned)bx, ot, tx, ty, ib);
  rw_lds_barrier();                                 // chunk 0 and the FIR are in LDS
  for (int n = 0; n < N; ++n) {
    const unsigned char* lb = Ls + (n & 1) * BUFB;
    const unsigned char* wb = Wl + (n & 1) * TC_WCH + lane * 8;
    mma(lb, wb);
    rw_lds_barrier();                               // the chunk is consumed; at a tile's last chunk also: the previous tile is blurred, z is free
    if (c + 1 < NC) { ++c; continue; }
    c = 0;
    noise_request(ty, tx, ib);                      // (the z write and a barrier cover it)
    zwrite();
    rw_lds_barrier();                               // z is ready
    // this role's share of the tile's blur (passes 0 and 1 of the four), before the next tile's multiplies; the staging
    // waves take the rest beside them
#pragma unroll 1
    for (int ps = 0; ps < 2; ++ps) blur(ps, pos & 3, ot, tx, ty, ib);
    ++pos;
    walk.advance(ot, tx, ty, ib);
#pragma unroll
    for (int b = 0; b < BPW; ++b)
#pragma unroll
      for (int ph = 0; ph < 4; ++ph) acc[b][ph] = rw_f32x4{0.f, 0.f, 0.f, 0.f};
  }
  if (p.y_amax) rw_bound_store_wave(p.y_amax, rw_wave_max(ymax));
}

// ---------------------------------------------------------------------------------------
// tconv_body's three shapes (tconv_blur_t8 / t16 / n32_kernel) with the window copied from the words of split_map_kernel (STAGED).
__global__ void __launch_bounds__(256, 2) tconv_blur_t8s_kernel(const TconvProblem p) { tconv_body<8, 4, 1, true>(p); }
__global__ void __launch_bounds__(512, 1) tconv_blur_t16s_kernel(const TconvProblem p) { tconv_body<16, 8, 1, true>(p); }
__global__ void __launch_bounds__(512, 1) tconv_blur_n32s_kernel(const TconvProblem p) { tconv_body<8, 8, 2, true>(p); }

// ---- the pre-pass of the STAGED forms: the fp32 map (batch, in_ch, h, w) -> words[image][chunk = c / 16][y][x][quad g]
// [8 halves], word = [Vh c0..3 | Vl c0..3] of the channels 16 chunk + 4 g .. + 3 of a pixel: what stage_store_part writes into
// the window buffer, minus the swizzle, as many bytes as the map.  The same arithmetic on the same inputs -- the per-image
// smax, in_scale = rw_split_scales<14>(bound smax), the style times in_scale rounded first (St[]), one v_mul_f32 per value,
// rw_split4 -- so the MFMA operands are the bits the other form makes.  A thread takes four columns of a quad's four
// channels (four 16-byte loads) and writes four words; the four quads of a pixel sit in neighbouring lanes: 64-byte runs.
// Grid: (h w / (256 iters), in_ch / 16, batch), h w a multiple of 512: no tail.
struct SplitMapProblem {
  const float* x; unsigned char* words; const float* style; const float* x_amax;
  int batch, in_ch, h, w, iters;
  float u_inv;
};
__global__ void __launch_bounds__(256) split_map_kernel(const SplitMapProblem p) {
  __shared__ float Red[4];
  const int tid = threadIdx.x, lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int ib = blockIdx.z, ch = blockIdx.y;
  float in_scale, out_scale;
  {
    const float smax = rw_block_max<4>(rw_style_absmax_wave<256>(p, ib, tid), lane, wave, Red);
    rw_split_scales<14>(rw_bound_load(p.x_amax) * smax, p.u_inv, in_scale, out_scale);
  }
  const int g = tid & 3, c0 = 16 * ch + 4 * g;
  float sv[4];
#pragma unroll
  for (int k = 0; k < 4; ++k) sv[k] = (p.style ? p.style[(int64_t)ib * p.in_ch + c0 + k] : 1.0f) * in_scale;
  const int64_t hw = (int64_t)p.h * p.w;
  const float* xi = p.x + ((int64_t)ib * p.in_ch + c0) * hw;
  unsigned char* wo = p.words + ((int64_t)ib * p.in_ch + 16 * ch) * hw * 4 + g * 16;
  for (int it = 0; it < p.iters; ++it) {
    const int64_t pix = 4 * (((int64_t)blockIdx.x * p.iters + it) * 64 + (tid >> 2));       // four pixels of one row
    rw_f32x4 raw[4];
#pragma unroll
    for (int k = 0; k < 4; ++k) raw[k] = *reinterpret_cast<const rw_f32x4*>(xi + k * hw + pix);
#pragma unroll
    for (int e = 0; e < 4; ++e)
      *reinterpret_cast<rw_f16x8*>(wo + (pix + e) * 64) =
          rw_split4(tc_mul(raw[0][e], sv[0]), tc_mul(raw[1][e], sv[1]), tc_mul(raw[2][e], sv[2]), tc_mul(raw[3][e], sv[3]));
  }
}

static bool tconv_shape_ok(int out_ch, int in_ch, int h, int w) {
  return out_ch > 0 && out_ch % 16 == 0 && in_ch >= 16 && in_ch % 16 == 0 && in_ch <= 512 && w % TC_TX == 0 && h % 16 == 0;
}

extern "C" int rw_tconv_blur_supported(int out_ch, int in_ch, int h, int w) { return tconv_shape_ok(out_ch, in_ch, h, w) ? 1 : 0; }

// ---- the scratch of the STAGED forms: one buffer per (device, stream), registered by the caller, who owns it
// the form of a launch (what RW_TCONV_TY means), from the environment and the channels
static int tconv_form(int in_ch, int out_ch) {
  // the form: RW_TCONV_TY = 0 the specialised persistent kernel, 8 / 16 the two shapes of tconv_body; unset: by input channels -- the persistent kernel where a tile has few chunks (<= 128
  // channels: its staging waves run ahead through the epilogue), the one-workgroup-per-CU shape where the MFMAs dominate
  // (profiles/r05q: layer 17 6.4 against 7.1 ms, layer 15 4.6 / 4.9, layer 13 3.7 / 3.7, layer 11 3.3 / 3.2, layer 9 1.9 / 1.7)
  // (RW_TCONV_PERSISTENT = 0 / 2: which of the two persistent kernels the automatic choice means)
  const int persistent = rw_env_int("RW_TCONV_PERSISTENT", 0) == 2 ? 2 : 0;
  // (RW_TCONV_N32 = "lo:hi": the input-channel range the automatic choice gives to the 32-out-channel form.  Default: none --
  // stand-alone it ties the persistent form on layer 15 (4.2 against 4.3 ms), inside the forward the persistent form is ahead:
  // 1526 - 1528 against 1507 - 1518 img/s, same box, interleaved, profiles/r06ak)
  int n32_lo = 1, n32_hi = 0;
  if (const char* ne = getenv("RW_TCONV_N32")) { if (sscanf(ne, "%d:%d", &n32_lo, &n32_hi) != 2) { n32_lo = 1; n32_hi = 0; } }
  const int sel = rw_env_int("RW_TCONV_TY", out_ch % 32 == 0 && in_ch >= n32_lo && in_ch <= n32_hi ? 32
                                           : (in_ch >= 32 && in_ch <= 128 ? persistent : 16));
  return sel;
}
// does a launch of this form and these channels take the staged form when it finds a buffer?
static bool tconv_staged_wanted(int sel, int in_ch, int batch) {
  if ((sel == 0 || sel == 2 || sel == 12) && in_ch >= 32) return false;      // the persistent forms stage in their own waves
  // RW_TCONV_STAGED unset: the staged forms run where a buffer is registered; RW_TCONV_STAGED_MIN_IN unset: 256 is the
  // fewest input channels that take them
  return rw_env_int("RW_TCONV_STAGED", 1) != 0 && in_ch >= rw_env_int("RW_TCONV_STAGED_MIN_IN", 256) && batch <= 65535;
}
namespace {
struct StageBuffer { int dev; hipStream_t stream; void* ptr; long long bytes; };
constexpr int kStageBuffers = 64;
StageBuffer g_stage[kStageBuffers];          // ptr == nullptr: a free entry
std::mutex g_stage_lock;
}
// bytes of the scratch this launch would use: the map's own size, or 0 where no staged form runs (shape, form, environment)
extern "C" long long rw_tconv_stage_bytes(int batch, int in_ch, int out_ch, int h, int w) {
  if (batch <= 0 || !tconv_shape_ok(out_ch, in_ch, h, w) || (int64_t)in_ch * h * w * 4 > 0x7fffffffLL) return 0;
  if (!tconv_staged_wanted(tconv_form(in_ch, out_ch), in_ch, batch)) return 0;
  return (long long)batch * in_ch * h * w * 4;
}
extern "C" int rw_tconv_stage_buffer(rw_stream_t stream, void* ptr, long long bytes) {
  RW_CHECK_ARG((ptr == nullptr) == (bytes == 0) && bytes >= 0 && (reinterpret_cast<uintptr_t>(ptr) & 15) == 0);
  int dev = 0;
  if (hipGetDevice(&dev) != hipSuccess) return RW_ERR_UNSUPPORTED;
  std::lock_guard<std::mutex> hold(g_stage_lock);
  StageBuffer* slot = nullptr;
  for (StageBuffer& b : g_stage)
    if (b.ptr && b.dev == dev && b.stream == rw_s(stream)) slot = &b;
  if (!ptr) {
    if (slot) *slot = StageBuffer{};
    return 0;
  }
  for (StageBuffer& b : g_stage)
    if (!slot && !b.ptr) slot = &b;
  if (!slot) return RW_ERR_UNSUPPORTED;
  *slot = StageBuffer{dev, rw_s(stream), ptr, bytes};
  return 0;
}
static void* tconv_stage_lookup(rw_stream_t stream, long long need) {
  int dev = 0;
  if (hipGetDevice(&dev) != hipSuccess) return nullptr;
  std::lock_guard<std::mutex> hold(g_stage_lock);
  for (const StageBuffer& b : g_stage)
    if (b.ptr && b.dev == dev && b.stream == rw_s(stream)) return b.bytes >= need ? b.ptr : nullptr;
  return nullptr;
}

extern "C" int rw_tconv_blur_f32(const float* x, const float* wp, const float* k4, float* y, int batch, int in_ch,
                                 int out_ch, int h, int w, float w_scale, const rw_conv_epilogue* ep,
                                 const float* post_scale, float u_inv, const float* x_amax, float* y_amax,
                                 rw_stream_t stream) {
  RW_CHECK_ARG(x && wp && k4 && y && x_amax && u_inv > 0.f && batch > 0 && in_ch > 0 && out_ch > 0 && h > 0 && w > 0);
  RW_CHECK_ARG(rw_epilogue_ok(ep));
  if (!tconv_shape_ok(out_ch, in_ch, h, w)) return RW_ERR_UNSUPPORTED;
  if ((int64_t)in_ch * h * w * 4 > 0x7fffffffLL) return RW_ERR_UNSUPPORTED;
  TconvProblem p = {};
  p.x = x; p.wp = reinterpret_cast<const unsigned char*>(wp); p.y = y; p.k4 = k4;
  rw_fill_epilogue(p, ep);
  p.post = post_scale;
  p.batch = batch; p.in_ch = in_ch; p.out_ch = out_ch; p.h = h; p.w = w; p.w_scale = w_scale; p.u_inv = u_inv;
  p.x_amax = x_amax; p.y_amax = y_amax;
  const int sel = tconv_form(in_ch, out_ch);
  if ((sel == 0 || sel == 2 || sel == 12) && in_ch >= 32) {      // 0: the specialised persistent kernel (one workgroup of eight waves per CU); 2: its pipelined form; 12: twelve waves
    p.tiles_x = w / TC_TX; p.tiles_y = h / 8; p.o_tiles = out_ch / 16;
    const int64_t tiles = (int64_t)batch * p.tiles_y * p.tiles_x * p.o_tiles;
    if (tiles <= 0 || tiles > 0x7fffffff) return RW_ERR_UNSUPPORTED;
    int64_t grid = rw_env_int("RW_TCONV_GRID", rw_cu_count());      // one persistent workgroup per compute unit
    grid = grid < 1 ? 1 : (grid > tiles ? tiles : grid);
    const int wv = sel == 12 ? 12 : 8;
    if (y_amax && wv * grid > rw_bound_slot_capacity((int64_t)batch * out_ch * 4 * h * w)) return RW_ERR_UNSUPPORTED;
    if (sel == 2) hipLaunchKernelGGL(tconv_blur_pp_kernel, dim3((unsigned)grid), dim3(512), 0, rw_s(stream), p);
    else if (sel == 12) hipLaunchKernelGGL(tconv_blur_ws12_kernel, dim3((unsigned)grid), dim3(768), 0, rw_s(stream), p);
    else hipLaunchKernelGGL(tconv_blur_ws_kernel, dim3((unsigned)grid), dim3(512), 0, rw_s(stream), p);
    return rw_finish_bound(y_amax, wv * grid, stream);
  }
  const bool n32 = sel == 32 && out_ch % 32 == 0;   // 32 out-channels per workgroup (8 x 32 tile, eight waves)
  const int ty = sel == 16 ? 16 : 8;
  const int waves = ty == 16 || n32 ? 8 : 4;
  p.tiles_x = w / TC_TX; p.tiles_y = h / ty; p.o_tiles = out_ch / (n32 ? 32 : 16);
  const int64_t work = (int64_t)batch * p.tiles_y * p.tiles_x * p.o_tiles;
  if (work <= 0 || work > 0x7fffffff) return RW_ERR_UNSUPPORTED;
  if (y_amax && waves * work > rw_bound_slot_capacity((int64_t)batch * out_ch * 4 * h * w)) return RW_ERR_UNSUPPORTED;
  // the staged form of the same shape: a registered buffer of the stream that holds the map's words, enough input channels
  // for the pre-pass to pay (RW_TCONV_STAGED_MIN_IN; profiles/INDEX.md, round 12), RW_TCONV_STAGED = 0 turns it off
  void* words = nullptr;
  if (tconv_staged_wanted(sel, in_ch, batch)) words = tconv_stage_lookup(stream, (long long)batch * in_ch * h * w * 4);
  if (words) {
    SplitMapProblem sp = {};
    sp.x = x; sp.words = static_cast<unsigned char*>(words); sp.style = p.style; sp.x_amax = x_amax;
    sp.batch = batch; sp.in_ch = in_ch; sp.h = h; sp.w = w; sp.u_inv = u_inv;
    const int blocks = h * w / 256;                 // h % 16 == 0, w % 32 == 0: a multiple of 2
    sp.iters = blocks % 4 == 0 ? 4 : 2;
    hipLaunchKernelGGL(split_map_kernel, dim3((unsigned)(blocks / sp.iters), (unsigned)(in_ch / 16), (unsigned)batch), dim3(256),
                       0, rw_s(stream), sp);
    p.x = reinterpret_cast<const float*>(sp.words);      // the staged kernels read the words, never the map
    if (n32) hipLaunchKernelGGL(tconv_blur_n32s_kernel, dim3((unsigned)work), dim3(512), 0, rw_s(stream), p);
    else if (ty == 16) hipLaunchKernelGGL(tconv_blur_t16s_kernel, dim3((unsigned)work), dim3(512), 0, rw_s(stream), p);
    else hipLaunchKernelGGL(tconv_blur_t8s_kernel, dim3((unsigned)work), dim3(256), 0, rw_s(stream), p);
    return rw_finish_bound(y_amax, waves * work, stream);
  }
  if (n32) hipLaunchKernelGGL(tconv_blur_n32_kernel, dim3((unsigned)work), dim3(512), 0, rw_s(stream), p);
  else if (ty == 16) hipLaunchKernelGGL(tconv_blur_t16_kernel, dim3((unsigned)work), dim3(512), 0, rw_s(stream), p);
  else hipLaunchKernelGGL(tconv_blur_t8_kernel, dim3((unsigned)work), dim3(256), 0, rw_s(stream), p);
  return rw_finish_bound(y_amax, waves * work, stream);
}
