// Shared epilogue of the implicit-GEMM kernels (igemm.hip, igemm_pp.hip, conv_sw.hip): accumulators (+bias) -> half -> swizzled LDS
// tile E[m][n] -> 16-byte coalesced row stores with the residual add and ReLU applied on the way out.
// Call after a workgroup barrier that retires every read of the staging buffers (the tile reuses them).
// LDS layout of a kernel that uses it: [0, ig_lds_main) shared by the staging buffers of the main loop and, afterwards,
// the E tile + its two row-offset tables; then IG_BIAS_LDS bytes of per-channel vectors (ig_bias_to_lds).
#pragma once
#include <type_traits>
#include "igemm_common.h"

#ifdef FP_PROFILE_BUILD
// profiling build only: 100 MHz wall-clock time per epilogue phase, summed over the workgroups of a launch (one copy per translation
// unit; conv_sw.hip reports its own through fp_dbg_conv_sw): [0] row tables + barrier, [1] residual requests (layer-kind bodies of
// k_conv_sw: the residual row offsets read + barrier), [2] accumulators -> E tile + barrier (there: with the residual requests, issued
// in groups under the transposition), [3] E tile -> stores issued (waits for the residual rows), [4] calls; [5..7]: ig_epilogue_direct
static __device__ unsigned long long ig_epi_dbg[8];
#define IG_CLK(t) const unsigned long long t = wall_clock64()
#else
#define IG_CLK(t)
#endif

#define IG_VEC_FLOATS 256                       // per-channel epilogue vectors in LDS: bias | BatchNorm scale | BatchNorm shift
#define IG_BIAS_LDS (3 * IG_VEC_FLOATS * 4)

// FULL: every row of the tile exists (m0 + BM <= M) -- no per-row predicate, so the LDS reads and the stores of the
// 16 iterations are issued as batches instead of one LDS round trip after the other.
template <int BM, int BN>
constexpr int ig_lds_main(int stage_bytes) {
  return stage_bytes > BM * BN * 2 + BM * 16 ? stage_bytes : BM * BN * 2 + BM * 16;   // E tile + the two row-offset tables
}

// SLIM (k_conv_sw): the row tables take BM * 4 bytes behind the E tile instead of BM * 16, so that a workgroup leaves LDS for a light
// workgroup of another stream (ig_lds_main_slim; conv_sw.hip).  The output table holds 32-bit offsets relative to the tile's first
// row (the launcher checks that the buffers stay below 2^31 elements); the residual table is needed only until the residual rows are
// requested, so it borrows the first BM * 8 bytes of the E tile, and a barrier separates its last read from the first write of E.
// The addresses are the same 64-bit element offsets either way.
template <int BM, int BN>
constexpr int ig_lds_main_slim(int stage_bytes) {
  return stage_bytes > BM * BN * 2 + BM * 4 ? stage_bytes : BM * BN * 2 + BM * 4;
}
#define IG_ROW_NONE ((int)0x80000000)            // SLIM: a row past M

// Acc: float16_[2][TM], the accumulators of v_mfma_f32_32x32x16_f16 (2 x TM tiles of 32 channels x 32 pixels), or ig_float4[4][2 * TM],
// those of v_mfma_f32_16x16x32_f16 (4 x 2 TM tiles of 16 x 16, conv_sw.hip) -- the same 128 x 64 wave tile either way
typedef float ig_float4 __attribute__((ext_vector_type(4)));
typedef _Float16 ig_half2 __attribute__((ext_vector_type(2)));
// What a layer-kind body reads of IgemmParams, copied once in front of the dispatch.  Not for speed: the compiler forwards the reads of a by-value
// kernel argument to the constant kernel-argument segment only up to a bounded number of reads; past it the whole block is copied to private
// memory and every scalar of the main loop is read back from there (seen with the sixth body reading IgemmParams directly: an alloca and a memcpy
// of the block in the IR, and "illegal VGPR to SGPR copy" at the main loop's scalar operands).  tests/test_igemm_epilogue_resources_host.py
// holds every kernel of the family to a private segment of zero bytes.
struct IgEpiArgs {
  IgemmGeom out, res;
  const _Float16* R;
  _Float16* Y;
  const float* pe;
  _Float16* Ype;
  int pe_period;
  unsigned pe_mul, pe_shr;
  int N;
};
__device__ __forceinline__ IgEpiArgs ig_epi_args(const IgemmParams& p) {
  return {p.out, p.res, p.R, p.Y, p.pe, p.Ype, p.pe_period, p.pe_mul, p.pe_shr, p.N};
}

// a kernel-argument pointer as the compiler can prove it wave-uniform (a buffer descriptor has to live in scalar registers)
template <typename T>
__device__ __forceinline__ T* ig_uniform_ptr(const T* ptr) {
  const unsigned long long a = reinterpret_cast<unsigned long long>(ptr);
  const unsigned lo = __builtin_amdgcn_readfirstlane((unsigned)a), hi = __builtin_amdgcn_readfirstlane((unsigned)(a >> 32));
  return reinterpret_cast<T*>(((unsigned long long)hi << 32) | lo);
}

// max(v, 0) of four or eight halves (V: half4, half8), one packed fp16 max per pair.  __builtin_elementwise_max is maxnum, which has to
// quiet a signalling NaN first: for a value read back from LDS or from memory the compiler cannot know there is none and puts a packed
// max of v with itself in front of every max.  These epilogues hand it results of conversions, adds and FMAs only, which are never
// signalling, and for every other input the instruction alone returns maxnum's bits (a quiet NaN gives 0, -0 against +0 gives +0,
// whichever side it is on).
template <typename V>
__device__ __forceinline__ V ig_relu(const V& v) {
  V r;
#pragma unroll
  for (int e = 0; e < (int)(sizeof(V) / 4); ++e) {
    const ig_half2 x = {v[2 * e], v[2 * e + 1]};
    ig_half2 y;
    asm("v_pk_max_f16 %0, %1, 0" : "=v"(y) : "v"(x));
    r[2 * e] = y[0]; r[2 * e + 1] = y[1];
  }
  return r;
}

// The rounding policy of one accumulator quad -- four consecutive channels of one pixel -- and the ONLY text of it: every epilogue of the
// family (ig_epilogue_spec, ig_epilogue_direct, ig_epilogue_generic below; k_splitk_epilogue of igemm.hip) calls it, so they return the
// same bits given the same accumulators.  bv: the bias, b01 / b23: the same as fp16 pairs (ROUND_ACC only; the caller forms them once per
// channel quad), sc / sh: BatchNorm scale and shift (HAS_BN only).
//  * ROUND_ACC: the reference's autocast op sequence for conv (+ BatchNorm): every op rounds its result to fp16.  Packed fp16 math where it
//    is exact: v_cvt_pk_f16_f32 for the conv output, v_pk_add_f16 for the bias (an IEEE half add of two halves equals their fp32 sum rounded
//    to half: when the fp32 sum is inexact the smaller addend is below 1/8 ulp of the larger), fp32 FMA for BatchNorm (fp32 statistics).
//  * otherwise (nn.Linear): one rounding of acc + bias.
// A missing bias is a bias of +0 (which turns -0 into +0; dropping the add would not).
template <bool ROUND_ACC, bool HAS_BN>
__device__ __forceinline__ half4 ig_round4(float a0, float a1, float a2, float a3, const ig_float4& bv, const ig_half2& b01, const ig_half2& b23,
                                           const ig_float4& sc, const ig_float4& sh) {
  static_assert(ROUND_ACC || !HAS_BN, "BatchNorm follows the conv rounding");
  half4 v;
  if constexpr (ROUND_ACC) {
    ig_half2 t01 = {(_Float16)a0, (_Float16)a1};
    ig_half2 t23 = {(_Float16)a2, (_Float16)a3};
    t01 = t01 + b01;
    t23 = t23 + b23;
    if constexpr (HAS_BN) {
      const ig_half2 t[2] = {t01, t23};
#pragma unroll
      for (int e = 0; e < 4; ++e) v[e] = (_Float16)fmaf((float)t[e >> 1][e & 1], sc[e], sh[e]);
    } else {
      v[0] = t01[0]; v[1] = t01[1]; v[2] = t23[0]; v[3] = t23[1];
    }
  } else {
    v[0] = (_Float16)(a0 + bv[0]); v[1] = (_Float16)(a1 + bv[1]); v[2] = (_Float16)(a2 + bv[2]); v[3] = (_Float16)(a3 + bv[3]);
  }
  return v;
}

// The positional second output of four or eight channels (V: half4, half8): f16(f32(v) + pe), rounded for the in_proj GEMM
template <typename V>
__device__ __forceinline__ V ig_add_pe(const V& v, const float* pe) {
  constexpr int NQ = sizeof(V) / 8;
  ig_float4 t[NQ];
#pragma unroll
  for (int q = 0; q < NQ; ++q) t[q] = *reinterpret_cast<const ig_float4*>(pe + 4 * q);
  V w;
#pragma unroll
  for (int e = 0; e < 4; ++e)
#pragma unroll
    for (int q = 0; q < NQ; ++q) w[4 * q + e] = (_Float16)((float)v[4 * q + e] + t[q][e]);
  return w;
}

// ---- Layer-kind bodies (round 9): the epilogue of a WHOLE tile with the layer kind EPI (IG_EPI_* bits, igemm_common.h) fixed at compile
// time.  The arithmetic per element is the one copy above (ig_round4, then + residual as an IEEE half add, then ig_relu, then ig_add_pe),
// so a mode returns the generic body's bits; what goes is what the generic body executes per 4 values around that arithmetic: the tests
// of round_acc / has_bn, the bias converted to fp16 again for every accumulator group, residual add and ReLU computed and then selected,
// and addresses rebuilt that move by a compile-time constant:
//  * E-tile write: row (lane & 15 or & 31) and the swizzled chunk depend on (lane, wn, i) only, so there is one base per channel quad i and
//    the pixel tile j is a constant in the ds_write offset field (chunk = c0 ^ (m & 15), m & 15 == lane & 15 in every pixel tile);
//  * store loop: iteration `it` handles row tid / CPR + it * RPI and chunk tid % CPR: RPI is a multiple of 16, so the swizzle term is
//    the same in every iteration, and the E read and the row tables are one base + it * constant;
//  * SLIM (k_conv_sw, whose launcher holds the output and the residual buffer below 2^31 elements): rows are stored, and residual rows
//    loaded, through ONE buffer descriptor on the tensor's base with a 32-bit byte offset per lane, not through 64-bit lane addresses.
//    (The descriptor sits on the buffer's start, not on the tile: offsets relative to the tile's first row can be negative under bsplit.)
// A missing bias is not a mode (the generic body adds the +0 that ig_bias_to_lds leaves in LDS, which turns -0 into +0; dropping the add would not).
template <int BM, int BN, int TM, int THREADS, bool SLIM, int EPI, typename Acc>
__device__ __forceinline__ void ig_epilogue_spec(const IgEpiArgs& p, Acc& acc, unsigned char* smem, int m0, int n0,
                                                 int wm, int wn, int tid, int lane, const float* bias_lds) {
  constexpr bool S16 = std::is_same<Acc, ig_float4[4][2 * TM]>::value;
  static_assert(S16 || std::is_same<Acc, float16_[2][TM]>::value, "accumulator layout");
  static_assert((EPI & IG_EPI_SPEC) && (EPI & IG_EPI_BIAS), "a layer kind with a bias");
  constexpr bool ROUND_ACC = (EPI & IG_EPI_ROUND_ACC) != 0, HAS_BN = (EPI & IG_EPI_BN) != 0, RES = (EPI & IG_EPI_RES) != 0;
  constexpr bool RELU = (EPI & IG_EPI_RELU) != 0, PE = (EPI & IG_EPI_PE) != 0;
  constexpr int CPR = BN / 8;                      // 16-byte chunks per row of the epilogue tile
  constexpr int NIT = (BM * CPR) / THREADS;
  constexpr int RPI = THREADS / CPR;               // rows per iteration of the store loop
  static_assert(THREADS % CPR == 0 && RPI % 16 == 0 && NIT * RPI == BM, "the store loop's swizzle term must not depend on the iteration");
  constexpr int ROWB = 2 * BN;                     // bytes per row of E
  typedef unsigned uint4_ __attribute__((ext_vector_type(4)));
  unsigned char* E = smem;
  long long* rowY = reinterpret_cast<long long*>(smem + BM * ROWB);
  long long* rowR = SLIM ? reinterpret_cast<long long*>(smem) : rowY + BM;
  int* rowY32 = reinterpret_cast<int*>(smem + BM * ROWB);           // SLIM: in place of rowY
  const long long baseY = SLIM ? ig_row_off(p.out, m0) + n0 : 0;
  IG_CLK(te0);
  for (int r = tid; r < BM; r += THREADS) {
    const int m = m0 + r;                          // < M: a whole tile
    if constexpr (SLIM) rowY32[r] = (int)(ig_row_off(p.out, m) + n0 - baseY);
    else rowY[r] = ig_row_off(p.out, m) + n0;
    if constexpr (RES) rowR[r] = ig_row_off(p.res, m) + n0;
  }
  __syncthreads();
  IG_CLK(te1);
  const int ml0 = tid / CPR, ch = tid % CPR;       // iteration `it` of this thread: row ml0 + it * RPI, chunk ch
  // The residual rows are requested before the transposition: their HBM latency overlaps it
  half8 rv[RES ? NIT : 1];
  // SLIM: ... and UNDER it (round 10).  Sixteen 16-byte loads per lane issued back to back are 128 KB of requests per workgroup; the waves
  // then sit at the issue of their loads until the memory pipe has taken them, and the transposition starts when the rows have all but
  // arrived.  So the loads go out in NRG groups, one in front of each channel group of the transposition, and VALU and LDS transpose while
  // the memory pipe streams.  The lane's row offsets leave the E tile first (rowR borrows it), as 32-bit byte offsets in registers.
  constexpr int NRG = S16 ? 4 : 8;                 // channel groups of the transposition below: i, or (i, g)
  static_assert(NIT % NRG == 0, "residual loads per channel group");
  unsigned roff[RES && SLIM ? NIT : 1];
  const __amdgpu_buffer_rsrc_t rsR = __builtin_amdgcn_make_buffer_rsrc(ig_uniform_ptr(p.R), 0, -1, 0x00020000);   // RES && SLIM only
  auto res_group = [&](int g) {                    // SLIM: the residual rows of store iterations [g, g + 1) * NIT / NRG
    if constexpr (RES && SLIM) {
#pragma unroll
      for (int it = g * (NIT / NRG); it < (g + 1) * (NIT / NRG); ++it)
        rv[it] = __builtin_bit_cast(half8, __builtin_amdgcn_raw_buffer_load_b128(rsR, (int)roff[it], 0, 0));
      __builtin_amdgcn_sched_barrier(0);           // where it stands: not hoisted in front of, nor sunk behind, the groups around it
    }
  };
  if constexpr (RES) {
    if constexpr (SLIM) {
      const int* rR = reinterpret_cast<const int*>(rowR + ml0);    // the low words: offsets below 2^31 elements
#pragma unroll
      for (int it = 0; it < NIT; ++it) roff[it] = ((unsigned)rR[it * RPI * 2] + ch * 8) << 1;
      // rowR sits in the E tile: every wave has read it (the offsets are in its registers) before any wave writes E
      __builtin_amdgcn_sched_barrier(0);
      asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
      __builtin_amdgcn_s_barrier();
      __builtin_amdgcn_sched_barrier(0);
    } else {
      const long long* rR = rowR + ml0;
#pragma unroll
      for (int it = 0; it < NIT; ++it) rv[it] = *reinterpret_cast<const half8*>(p.R + rR[it * RPI] + ch * 8);
    }
  }
  IG_CLK(te2);
  // per-channel values of 4 consecutive channels nl .. nl + 3 (LDS broadcast reads), formed once per channel quad
  struct Vecs { ig_float4 bv, sc, sh; ig_half2 b01, b23; };
  auto vecs = [&](int nl) {
    Vecs c;
    c.bv = *reinterpret_cast<const ig_float4*>(bias_lds + nl);
    c.b01 = ig_half2{(_Float16)c.bv[0], (_Float16)c.bv[1]};
    c.b23 = ig_half2{(_Float16)c.bv[2], (_Float16)c.bv[3]};
    if constexpr (HAS_BN) {
      c.sc = *reinterpret_cast<const ig_float4*>(bias_lds + IG_VEC_FLOATS + nl);
      c.sh = *reinterpret_cast<const ig_float4*>(bias_lds + 2 * IG_VEC_FLOATS + nl);
    }
    return c;
  };
  // accumulators of those 4 channels of one pixel -> the policy's roundings (ig_round4) -> E tile
  auto put4 = [&](unsigned char* dst, float a0, float a1, float a2, float a3, const Vecs& c) {
    *reinterpret_cast<half4*>(dst) = ig_round4<ROUND_ACC, HAS_BN>(a0, a1, a2, a3, c.bv, c.b01, c.b23, c.sc, c.sh);
  };
  const int r15 = lane & 15;                       // == m & 15 of the lane's row in every pixel tile
  if constexpr (S16) {
    // 16x16x32: lane holds pixel (lane & 15) and channels 4 * sigma(lane >> 4) + {0..3} of a 16 x 16 tile, sigma = (0, 2, 3, 1)
    const int quad = (0x1320 >> (4 * (lane >> 4))) & 3;
    unsigned char* Erow = E + (wm * (32 * TM) + r15) * ROWB + ((quad & 1) << 3);
    const int cx = (wn * 8 + (quad >> 1)) ^ r15;   // chunk of channel quad i: (wn * 8 + 2 i + (quad >> 1)) ^ r15 = cx ^ 2 i
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      res_group(i);
      const Vecs c = vecs(wn * 64 + i * 16 + 4 * quad);
      unsigned char* Ei = Erow + ((cx ^ (2 * i)) << 4);
#pragma unroll
      for (int j = 0; j < 2 * TM; ++j) put4(Ei + j * (16 * ROWB), acc[i][j][0], acc[i][j][1], acc[i][j][2], acc[i][j][3], c);
    }
  } else {
    // 32x32x16: lane holds pixel (lane & 31), channels 8g + 4 * (lane >> 5) + {0..3} of a 32 x 32 tile, g = reg >> 2
    unsigned char* Erow = E + (wm * (32 * TM) + (lane & 31)) * ROWB + ((lane >> 5) << 3);
    const int cx = (wn * 8) ^ r15;                 // chunk of (i, g): (wn * 8 + 4 i + g) ^ r15 = cx ^ (4 i + g)
#pragma unroll
    for (int i = 0; i < 2; ++i) {
#pragma unroll
      for (int g = 0; g < 4; ++g) {
        res_group(i * 4 + g);
        const Vecs c = vecs(wn * 64 + i * 32 + 8 * g + 4 * (lane >> 5));
        unsigned char* Ei = Erow + ((cx ^ (4 * i + g)) << 4);
#pragma unroll
        for (int j = 0; j < TM; ++j)
          put4(Ei + j * (32 * ROWB), acc[i][j][g * 4 + 0], acc[i][j][g * 4 + 1], acc[i][j][g * 4 + 2], acc[i][j][g * 4 + 3], c);
      }
    }
  }
  __syncthreads();
  IG_CLK(te3);
  const unsigned char* Erd = E + ml0 * ROWB + ((ch ^ (ml0 & 15)) << 4);
  const __amdgpu_buffer_rsrc_t rsY = __builtin_amdgcn_make_buffer_rsrc(ig_uniform_ptr(p.Y), 0, -1, 0x00020000);   // SLIM only
  const unsigned cbY = ((unsigned)baseY + ch * 8) << 1;      // SLIM: byte offset of the lane's chunk in the tile's first row (below 2^32)
#pragma unroll
  for (int it = 0; it < NIT; ++it) {
    half8 v = *reinterpret_cast<const half8*>(Erd + it * (RPI * ROWB));
    if constexpr (RES) v = v + rv[it];             // IEEE half add == the fp32 add of two halves rounded once
    if constexpr (RELU) v = ig_relu(v);
    if constexpr (SLIM) __builtin_amdgcn_raw_buffer_store_b128(__builtin_bit_cast(uint4_, v), rsY, (int)(cbY + ((unsigned)rowY32[ml0 + it * RPI] << 1)), 0, 0);
    else *reinterpret_cast<half8*>(p.Y + rowY[ml0 + it * RPI] + ch * 8) = v;
    if constexpr (PE) {                            // tokens + positional table
      const int m = m0 + ml0 + it * RPI;
      const int mp = m - ig_fastdiv(m, p.pe_mul, p.pe_shr) * p.pe_period;   // m % pe_period
      *reinterpret_cast<half8*>(p.Ype + (size_t)m * p.N + n0 + ch * 8) = ig_add_pe(v, p.pe + (size_t)mp * p.N + n0 + ch * 8);
      // one row at a time: batched over the 16 iterations, the table rows (8 registers each) on top of the residual rows take k_conv_sw past
      // the 224 registers it is held to (tests/test_conv_sw_resources_host.py); one launch per network and step has this body
      __builtin_amdgcn_sched_barrier(0);
    }
  }
#ifdef FP_PROFILE_BUILD
  IG_CLK(te4);
  if (tid == 0) {
    atomicAdd(&ig_epi_dbg[0], te1 - te0); atomicAdd(&ig_epi_dbg[1], te2 - te1); atomicAdd(&ig_epi_dbg[2], te3 - te2);
    atomicAdd(&ig_epi_dbg[3], te4 - te3); atomicAdd(&ig_epi_dbg[4], 1ull);
  }
#endif
}
// ---- The direct epilogue (round 11, k_conv_sw_direct of conv_sw.hip): the 512 x 128 tile leaves straight from the accumulators.  That
// kernel issues its 16x16x32 MFMAs with pixels as A and weights as B and orders the weight rows so that lane l of wave (wm, wn) holds, in
// acc[t][j][e], pixel row wm * 128 + 16 j + 4 (l >> 4) + e and channel wn * 64 + 4 (l & 15) + t of the tile: four consecutive channels of a
// pixel per lane (8 bytes), the 64 channels of a pixel in 16 consecutive lanes (one 128-byte line), and the SAME four channels for the whole
// tile, so the per-channel vectors are read once.  No E tile and no barrier between conversion and store: a wave stores a pixel tile as
// soon as it is converted, and the eight waves are free to drift apart.
// Per element it calls what ig_epilogue_spec calls, in its order (ig_round4, then + residual, then ig_relu): the same bits given the same
// accumulators.  rowY32: the output row table the kernel built in its prologue (element offsets from the buffer's start, channel n0
// included; IG_ROW_NONE for a row past M).  The residual table goes over the operand stages (the caller's barrier retired their last read);
// residual rows are requested one group of two pixel tiles ahead of their use.  FULL: every row of the tile exists.
template <int EPI, bool FULL, typename Acc>
__device__ __forceinline__ void ig_epilogue_direct(const IgEpiArgs& p, Acc& acc, unsigned char* smem, const int* rowY32, int m0, int n0, int M,
                                                   int wm, int wn, int tid, int lane, const float* bias_lds) {
  constexpr int TM = 4;                            // the 512 x 128 tile: thread `tid` owns row `tid` of the tables
  static_assert(std::is_same<Acc, ig_float4[4][2 * TM]>::value, "accumulators of the 16x16x32 loop");
  static_assert((EPI & IG_EPI_CONV) == IG_EPI_CONV && !(EPI & IG_EPI_PE), "conv rounding + bias + ReLU, without the positional output");
  constexpr bool HAS_BN = (EPI & IG_EPI_BN) != 0, RES = (EPI & IG_EPI_RES) != 0;
  typedef int int4_ __attribute__((ext_vector_type(4)));
  typedef unsigned uint2_ __attribute__((ext_vector_type(2)));
  constexpr int JG = 2, NG = 2 * TM / JG;          // pixel tiles per residual group, groups
  const int nl = wn * 64 + 4 * (lane & 15);        // the lane's four channels, tile-local
  const int prow = wm * (32 * TM) + 4 * (lane >> 4);   // its four rows of pixel tile j: prow + 16 j + e
  int* rowR32 = reinterpret_cast<int*>(smem);
  IG_CLK(te0);
  if constexpr (RES) {
    // (a row past M: the offset of the last row, which is loaded and never stored)
    const int m = FULL || m0 + tid < M ? m0 + tid : M - 1;
    rowR32[tid] = (int)(ig_row_off(p.res, m) + n0);
    __syncthreads();
  }
  IG_CLK(te1);
  const ig_float4 bv = *reinterpret_cast<const ig_float4*>(bias_lds + nl);
  const ig_half2 b01 = {(_Float16)bv[0], (_Float16)bv[1]}, b23 = {(_Float16)bv[2], (_Float16)bv[3]};
  ig_float4 sc = {}, sh = {};                      // read by ig_round4 with BatchNorm only
  if constexpr (HAS_BN) {
    sc = *reinterpret_cast<const ig_float4*>(bias_lds + IG_VEC_FLOATS + nl);
    sh = *reinterpret_cast<const ig_float4*>(bias_lds + 2 * IG_VEC_FLOATS + nl);
  }
  const __amdgpu_buffer_rsrc_t rsY = __builtin_amdgcn_make_buffer_rsrc(ig_uniform_ptr(p.Y), 0, -1, 0x00020000);
  const __amdgpu_buffer_rsrc_t rsR = __builtin_amdgcn_make_buffer_rsrc(ig_uniform_ptr(p.R), 0, -1, 0x00020000);   // RES only
  half4 rv[RES ? 2 : 1][JG * 4];
  auto res_group = [&](int g) {                    // the residual rows of pixel tiles [g, g + 1) * JG: 8-byte loads
    if constexpr (RES) {
#pragma unroll
      for (int jj = 0; jj < JG; ++jj) {
        const int4_ ro = *reinterpret_cast<const int4_*>(rowR32 + prow + 16 * (g * JG + jj));
#pragma unroll
        for (int e = 0; e < 4; ++e)
          rv[g & 1][jj * 4 + e] = __builtin_bit_cast(half4, __builtin_amdgcn_raw_buffer_load_b64(rsR, (int)((unsigned)(ro[e] + nl) << 1), 0, 0));
      }
      __builtin_amdgcn_sched_barrier(0);           // where it stands: not hoisted in front of, nor sunk behind, the groups around it
    }
  };
  res_group(0);
#pragma unroll
  for (int g = 0; g < NG; ++g) {
    if (g + 1 < NG) res_group(g + 1);
#pragma unroll
    for (int jj = 0; jj < JG; ++jj) {
      const int j = g * JG + jj;
      const int4_ yo = *reinterpret_cast<const int4_*>(rowY32 + prow + 16 * j);
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        half4 v = ig_round4<true, HAS_BN>(acc[0][j][e], acc[1][j][e], acc[2][j][e], acc[3][j][e], bv, b01, b23, sc, sh);
        if constexpr (RES) v = v + rv[g & 1][jj * 4 + e];   // IEEE half add == the fp32 add of two halves rounded once
        v = ig_relu(v);
        if (FULL || yo[e] != IG_ROW_NONE)
          __builtin_amdgcn_raw_buffer_store_b64(__builtin_bit_cast(uint2_, v), rsY, (int)((unsigned)(yo[e] + nl) << 1), 0, 0);
      }
    }
    __builtin_amdgcn_sched_barrier(0);
  }
#ifdef FP_PROFILE_BUILD
  // slots of its own, so that a step that runs both kernels keeps them apart: [5] the residual table + its barrier (the output table is
  // built in the kernel's prologue and counts as cold start), [6] conversions + stores issued, [7] calls
  IG_CLK(te2);
  if (tid == 0) { atomicAdd(&ig_epi_dbg[5], te1 - te0); atomicAdd(&ig_epi_dbg[6], te2 - te1); atomicAdd(&ig_epi_dbg[7], 1ull); }
#endif
}

// ---- The generic body: reads the layer kind from IgemmParams at run time (any combination, partial tiles included; IgemmParams.epi == 0 and
// the A/B arm of FP_IGEMM_EPILOGUE_GENERIC).  The same per-element helpers as the layer-kind bodies, selected by the run-time flags.
template <int BM, int BN, int TM, int THREADS, bool FULL, bool SLIM, typename Acc>
__device__ __forceinline__ void ig_epilogue_generic(const IgemmParams& p, Acc& acc, unsigned char* smem, int m0, int n0,
                                                    int wm, int wn, int tid, int lane, const float* bias_lds) {
  constexpr bool S16 = std::is_same<Acc, ig_float4[4][2 * TM]>::value;
  static_assert(S16 || std::is_same<Acc, float16_[2][TM]>::value, "accumulator layout");
  constexpr int CPR = BN / 8;                      // 16-byte chunks per row of the epilogue tile
  constexpr int NIT = (BM * CPR) / THREADS;
  // ---- epilogue: accumulators (+bias) -> half -> swizzled LDS tile E[m][n] -> 16-B coalesced row stores
  // Row addressing first: ONE thread per tile row maps the row to its element offsets in the output (and residual)
  // buffer and parks them in LDS behind the E tile; the store loop then reads them back as broadcasts.  (Computing the
  // map per (row, 16-byte chunk), as the first version did, cost 16-32 emulated 64-bit address computations per thread
  // and made the epilogue 20-45 % of the kernel.)
  unsigned char* E = smem;   // BM rows x (2*BN) B, low 4 bits of the chunk index XORed with (m & 15)
  // bias: staged into LDS at kernel entry (ig_bias_to_lds) -- a global load issued here would be exposed in full, and
  // under the operand stream's load that is several thousand cycles
  const bool round_acc = p.round_acc != 0, has_bn = p.bn_scale != nullptr;
  long long* rowY = reinterpret_cast<long long*>(smem + BM * 2 * BN);
  long long* rowR = SLIM ? reinterpret_cast<long long*>(smem) : rowY + BM;
  int* rowY32 = reinterpret_cast<int*>(smem + BM * 2 * BN);        // SLIM: in place of rowY
  const long long baseY = SLIM ? ig_row_off(p.out, m0) + n0 : 0;   // m0 < M
  auto row_exists = [&](int ml) { return SLIM ? rowY32[ml] != IG_ROW_NONE : rowY[ml] >= 0; };
  IG_CLK(te0);
  for (int r = tid; r < BM; r += THREADS) {
    const int m = m0 + r;
    const bool in = m < p.M;
    if constexpr (SLIM) rowY32[r] = in ? (int)(ig_row_off(p.out, m) + n0 - baseY) : IG_ROW_NONE;
    else rowY[r] = in ? ig_row_off(p.out, m) + n0 : -1;
    if (p.R) rowR[r] = in ? ig_row_off(p.res, m) + n0 : 0;
  }
  __syncthreads();
  IG_CLK(te1);
  // The residual rows are requested before the transposition: their HBM latency overlaps it
  half8 rv[NIT];
  if (p.R) {
#pragma unroll
    for (int it = 0; it < NIT; ++it) {
      const int qd = tid + it * THREADS;
      const int ml = qd / CPR, ch = qd % CPR;
      if (FULL || row_exists(ml)) rv[it] = *reinterpret_cast<const half8*>(p.R + rowR[ml] + ch * 8);
    }
    if constexpr (SLIM) {
      // rowR sits in the E tile: every wave has read it (its loads are issued) before any wave writes E.  A bare barrier: __syncthreads()
      // would also wait for the residual rows themselves, whose latency the transposition is there to cover
      __builtin_amdgcn_sched_barrier(0);
      asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
      __builtin_amdgcn_s_barrier();
      __builtin_amdgcn_sched_barrier(0);
    }
  }
  IG_CLK(te2);
  // 4 consecutive channels nl .. nl + 3 (tile-local) of pixel row ml: accumulators -> the policy's roundings -> E tile
  auto put4 = [&](int nl, int ml, float a0, float a1, float a2, float a3, const ig_float4& bv, const ig_float4& sc, const ig_float4& sh) {
    half4 v;
    if (round_acc) {
      const ig_half2 b01 = {(_Float16)bv[0], (_Float16)bv[1]}, b23 = {(_Float16)bv[2], (_Float16)bv[3]};
      if (has_bn) v = ig_round4<true, true>(a0, a1, a2, a3, bv, b01, b23, sc, sh);
      else v = ig_round4<true, false>(a0, a1, a2, a3, bv, b01, b23, sc, sh);
    } else {
      v = ig_round4<false, false>(a0, a1, a2, a3, bv, ig_half2{}, ig_half2{}, sc, sh);
    }
    const int chunk = (nl >> 3) ^ (ml & 15);
    *reinterpret_cast<half4*>(E + ml * (2 * BN) + (chunk << 4) + ((nl & 4) << 1)) = v;
  };
  // per-channel vectors of 4 channels (LDS broadcast reads; kept out of registers until here)
  auto vecs = [&](int nl, ig_float4& bv, ig_float4& sc, ig_float4& sh) {
    bv = *reinterpret_cast<const ig_float4*>(bias_lds + nl);
    sc = ig_float4{1.f, 1.f, 1.f, 1.f}; sh = ig_float4{0.f, 0.f, 0.f, 0.f};
    if (has_bn) {
      sc = *reinterpret_cast<const ig_float4*>(bias_lds + IG_VEC_FLOATS + nl);
      sh = *reinterpret_cast<const ig_float4*>(bias_lds + 2 * IG_VEC_FLOATS + nl);
    }
  };
  if constexpr (S16) {
    // 16x16x32: D[channel][pixel] of a 16 x 16 tile: lane holds pixel (lane & 15) and the tile's channel quad (lane >> 4), which conv_sw.hip
    // maps to channels 4 * sigma(lane >> 4) + {0..3}, sigma = (0, 2, 3, 1): the order of the weight rows in its A fragments
    const int quad = (0x1320 >> (4 * (lane >> 4))) & 3;
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      const int nl = wn * 64 + i * 16 + 4 * quad;
      ig_float4 bv, sc, sh;
      vecs(nl, bv, sc, sh);
#pragma unroll
      for (int j = 0; j < 2 * TM; ++j) {
        const int ml = wm * (32 * TM) + j * 16 + (lane & 15);
        put4(nl, ml, acc[i][j][0], acc[i][j][1], acc[i][j][2], acc[i][j][3], bv, sc, sh);
      }
    }
  } else {
    // 32x32x16: D[i = channel][j = pixel]: lane holds pixel (lane & 31), channels 8g + 4*(lane>>5) + {0..3}, g = reg >> 2
#pragma unroll
    for (int i = 0; i < 2; ++i) {
#pragma unroll
      for (int g = 0; g < 4; ++g) {
        const int nl = wn * 64 + i * 32 + 8 * g + 4 * (lane >> 5);   // first of 4 consecutive channels (tile-local)
        ig_float4 bv, sc, sh;
        vecs(nl, bv, sc, sh);
#pragma unroll
        for (int j = 0; j < TM; ++j) {
          const int ml = wm * (32 * TM) + j * 32 + (lane & 31);
          put4(nl, ml, acc[i][j][g * 4 + 0], acc[i][j][g * 4 + 1], acc[i][j][g * 4 + 2], acc[i][j][g * 4 + 3], bv, sc, sh);
        }
      }
    }
  }
  __syncthreads();
  IG_CLK(te3);
  const half8 zero = {0, 0, 0, 0, 0, 0, 0, 0};
#pragma unroll
  for (int it = 0; it < NIT; ++it) {
    const int qd = tid + it * THREADS;
    const int ml = qd / CPR, ch = qd % CPR;
    if (!FULL && !row_exists(ml)) continue;
    const long long yo = SLIM ? baseY + rowY32[ml] : rowY[ml];
    half8 v = *reinterpret_cast<const half8*>(E + ml * (2 * BN) + ((ch ^ (ml & 15)) << 4));
    if (p.R) v = v + rv[it];                       // IEEE half add == the fp32 add of two halves rounded once
    if (p.relu) v = __builtin_elementwise_max(v, zero);
    *reinterpret_cast<half8*>(p.Y + yo + ch * 8) = v;
    if (p.Ype) {                                   // tokens + positional table
      const int m = m0 + ml;
      *reinterpret_cast<half8*>(p.Ype + (size_t)m * p.N + n0 + ch * 8) = ig_add_pe(v, p.pe + (size_t)(m % p.pe_period) * p.N + n0 + ch * 8);
    }
  }
#ifdef FP_PROFILE_BUILD
  IG_CLK(te4);
  if (tid == 0) {
    atomicAdd(&ig_epi_dbg[0], te1 - te0); atomicAdd(&ig_epi_dbg[1], te2 - te1); atomicAdd(&ig_epi_dbg[2], te3 - te2);
    atomicAdd(&ig_epi_dbg[3], te4 - te3); atomicAdd(&ig_epi_dbg[4], 1ull);
  }
#endif
}

// A whole tile of one of the six layer kinds the library compiles a body for runs ig_epilogue_spec (DBG == 0: the timing-only builds of
// k_igemm_pp keep to the generic body); everything else the generic body.
template <int BM, int BN, int TM, int THREADS, int DBG = 0, bool SLIM = false, typename Acc>
__device__ __forceinline__ void ig_epilogue(const IgemmParams& p, Acc& acc, unsigned char* smem, int m0, int n0,
                                            int wm, int wn, int tid, int lane, const float* bias_lds) {
  if (m0 + BM <= p.M) {
    if constexpr (DBG == 0) {
      // p.epi is a kernel argument: a scalar branch, the same for every wave of the launch (igemm.hip picks it: ig_epilogue_mode)
#define IG_EPI_CASE(E) case E: ig_epilogue_spec<BM, BN, TM, THREADS, SLIM, E>(q, acc, smem, m0, n0, wm, wn, tid, lane, bias_lds); return
      const IgEpiArgs q = ig_epi_args(p);
      switch (p.epi) {
        IG_EPI_CASE(IG_EPI_CONV);
        IG_EPI_CASE(IG_EPI_CONV | IG_EPI_RES);
        IG_EPI_CASE(IG_EPI_CONV | IG_EPI_RES | IG_EPI_PE);
        IG_EPI_CASE(IG_EPI_CONV | IG_EPI_BN);
        IG_EPI_CASE(IG_EPI_CONV | IG_EPI_BN | IG_EPI_RES);
        IG_EPI_CASE(IG_EPI_CONV | IG_EPI_BN | IG_EPI_RES | IG_EPI_PE);
        default: break;
      }
#undef IG_EPI_CASE
    }
    ig_epilogue_generic<BM, BN, TM, THREADS, true, SLIM>(p, acc, smem, m0, n0, wm, wn, tid, lane, bias_lds);
  }
  else ig_epilogue_generic<BM, BN, TM, THREADS, false, SLIM>(p, acc, smem, m0, n0, wm, wn, tid, lane, bias_lds);
}
// Kernel entry, BEFORE the first operand stage is requested: wave 0 sends the tile's bias straight to LDS with one
// LDS-DMA (1 KiB = 256 floats; reads past the end of the bias vector return 0 through the buffer descriptor's bound).
// Being the oldest vector-memory operation of the wave it is covered by every later counted vmcnt wait, and it is
// visible to the workgroup after the first barrier of the main loop.  The LDS area is always IG_BIAS_LDS bytes.
// Three vectors of IG_VEC_FLOATS floats: bias, BatchNorm scale, BatchNorm shift (waves 0, 1, 2 fetch one each).
// (The vectors and N as values: k_conv_sw passes the copies it reads at its top, conv_sw.hip.)
__device__ __forceinline__ void ig_bias_to_lds(const float* bias, const float* bn_scale, const float* bn_shift, int N, int n0, float* bias_lds,
                                               int wid, int lane) {
  if (wid > 2) return;
  const float* src = wid == 0 ? bias : (wid == 1 ? bn_scale : bn_shift);
  float* dst = bias_lds + wid * IG_VEC_FLOATS;
  if (src) {
    const __amdgpu_buffer_rsrc_t rs = __builtin_amdgcn_make_buffer_rsrc(const_cast<float*>(src), 0, N * 4, 0x00020000);
    __builtin_amdgcn_raw_ptr_buffer_load_lds(rs, (__attribute__((address_space(3))) void*)dst, 16, lane * 16, n0 * 4, 0, 0);
  } else if (wid == 0) {
    typedef float f4 __attribute__((ext_vector_type(4)));
    *reinterpret_cast<f4*>(dst + lane * 4) = f4{0.f, 0.f, 0.f, 0.f};
  }
}
__device__ __forceinline__ void ig_bias_to_lds(const IgemmParams& p, int n0, float* bias_lds, int wid, int lane) {
  ig_bias_to_lds(p.bias, p.bn_scale, p.bn_shift, p.N, n0, bias_lds, wid, lane);
}
