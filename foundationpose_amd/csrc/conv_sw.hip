// k_conv_sw -- shifted-window 3x3 convolution (stride 1, pad 1) on the ping-pong schedule of igemm_pp.hip: the kernel
// behind fp_igemm_f16_fwd for the twelve ResnetBasicBlock convolutions of each encoder (network_modules.py:73-111;
// refine_network.py:40-49, score_network.py:39-48), where input and output share one padded pixel grid.
//
// Why: as an implicit GEMM with k = (tap, ci) every workgroup fetches each of its activation rows nine times, once per
// tap (measured on the 256->256 layer: 1.33 GB moved for 0.43 GB of tensors, and an LDS-DMA issue rate that keeps the
// memory cluster of the ping-pong loop longer than its MFMA cluster).  Here the k order is (channel chunk,
// tap): per 32-channel chunk ONE patch of the padded input -- the tile's 256 output pixels plus a halo of Wp+1 pixels
// on either side, as one contiguous run of the padded NHWC grid -- is staged in LDS, and the nine taps read it at a row
// shift of ky*Wp + kx.  Rows of the GEMM stay the true output pixels (no border work, same epilogue): a lane's fragment
// row for tap (ky,kx) is its pixel's position in the patch + the shift.
//
// Operand traffic per k-step drops from (256 + BN) rows to BN rows + 1/9 patch; LDS-DMA instructions per wave and
// k-step from 4 to 2.4 (BN = 256) and from 3 to 1.4 (BN = 128).
//
// LDS: two patch buffers of 512 rows x 64 B (double buffered across chunks) + a ring of 4 weight stages of BN x 64 B;
// 64-byte rows XOR-swizzled as in igemm_pp.hip (chunk ^ ((row >> 2) & 3), a bijection of row mod 16, so 32 consecutive
// patch rows at ANY offset are conflict-free for ds_read_b128).  Schedule: two groups of 4 waves one cluster apart,
// a k-step = memory cluster (12 fragment reads + this step's LDS-DMA) | barrier | 16 MFMAs | barrier; weights are
// prefetched three k-steps ahead, the next chunk's patch is requested one piece per wave at taps 0-3 of the current chunk.
#include <hip/hip_fp16.h>
#include <stdlib.h>
#include <string.h>
#include <type_traits>
#include "igemm_common.h"
#include "igemm_epilogue.h"

#ifdef FP_PROFILE_BUILD
// profiling build only: 100 MHz wall-clock time per phase, summed over the workgroups of a launch (scripts/dbg_conv_sw.py):
// [0] cold start = kernel entry -> first operands landed, [1] main loop, [2] epilogue + drain, [3] workgroups, [4] the part of [0] up to
// "first operand DMAs issued", [5] the part of [2] and [3] that are k_conv_sw_direct's: [8] and [9] (fp_dbg_conv_sw_direct), [6] / [7] first entry / last exit
__device__ unsigned long long sw_dbg[10];
extern "C" int fp_dbg_conv_sw(unsigned long long* out, int reset) {
  if (reset) { unsigned long long z[10] = {0, 0, 0, 0, 0, 0, ~0ull, 0, 0, 0}; return (int)hipMemcpyToSymbol(HIP_SYMBOL(sw_dbg), z, sizeof(z)); }
  return (int)hipMemcpyFromSymbol(out, HIP_SYMBOL(sw_dbg), 8 * sizeof(unsigned long long));
}
// k_conv_sw_direct's share of [2] and [3]: out[0] epilogue + drain, out[1] workgroups (reset with fp_dbg_conv_sw)
extern "C" int fp_dbg_conv_sw_direct(unsigned long long* out) {
  return (int)hipMemcpyFromSymbol(out, HIP_SYMBOL(sw_dbg), 2 * sizeof(unsigned long long), 8 * sizeof(unsigned long long));
}
// the epilogue's own phase timers (igemm_epilogue.h, this translation unit's copy): out[0..7]
extern "C" int fp_dbg_conv_sw_epilogue(unsigned long long* out, int reset) {
  if (reset) { unsigned long long z[8] = {0, 0, 0, 0, 0, 0, 0, 0}; return (int)hipMemcpyToSymbol(HIP_SYMBOL(ig_epi_dbg), z, sizeof(z)); }
  return (int)hipMemcpyFromSymbol(out, HIP_SYMBOL(ig_epi_dbg), 8 * sizeof(unsigned long long));
}
#define SW_CLK(t) const unsigned long long t = wall_clock64()
#else
#define SW_CLK(t)
#endif

#ifndef SW_DEFAULT_VARIANT
#define SW_DEFAULT_VARIANT 0
#endif

namespace {

constexpr int SW_BK = 32, SW_NSTW = 4;
// patch rows per buffer (LDS-DMA instructions of 16 rows, a multiple of 8 of them): the tile's BM output pixels + halo,
// see fp_conv3x3_sw_applicable
constexpr int sw_prows(int BM) { return BM == 256 ? 512 : 768; }

template <int N>
__device__ __forceinline__ void sw_wait_vm() {
  static_assert(N >= 0 && N < 64, "vmcnt is a 6-bit field");
  asm volatile("s_waitcnt vmcnt(%0)" ::"n"(N) : "memory");
}

// acc += a * b on v_mfma_f32_16x16x32_f16 with the accumulator tied to its registers.  The builtin leaves destination and addend
// independent, and over the nine unrolled taps the register allocator then moves the 32 accumulator quads of a wave from k-step to
// k-step; the holes that leaves cost k_conv_sw<512,128,4,true> 256 VGPRs for 203 live values, the whole register file of a CU at two
// waves per SIMD.  Tied, it is 219, which leaves a third wave of up to 64 registers per SIMD to a light kernel of another stream
// (tests/test_conv_sw_resources_host.py holds it to 224).  The operands' waits are still the compiler's; each accumulator is used once
// per k-step, 31 MFMAs apart, and is read by other instructions only behind the barriers in front of the epilogue.
typedef float sw_float4 __attribute__((ext_vector_type(4)));
__device__ __forceinline__ void sw_mfma16(sw_float4& acc, const half8& a, const half8& b) {
  asm volatile("v_mfma_f32_16x16x32_f16 %0, %1, %2, %0" : "+v"(acc) : "v"(a), "v"(b));
}

// DIRECT: the same instruction with its two source operands exchanged.  For v_mfma_f32_16x16x32_f16 the A and B fragment layouts are the
// same (lane l: row or column l & 15, k chunk l >> 4), so D becomes [pixel][channel]: lane l holds channel column l & 15 of the pixels
// 4 (l >> 4) + e, e = 0..3, of a 16 x 16 tile.  The same products summed over the same k per element.
template <bool DIRECT>
__device__ __forceinline__ void sw_mfma16x(sw_float4& acc, const half8& w, const half8& a) {
  if constexpr (DIRECT) sw_mfma16(acc, a, w);
  else sw_mfma16(acc, w, a);
}

// DIRECT: which weight row of the 128-channel tile LDS row r of the weight image holds.  Lane frow of weight fragment t of wave column wn
// reads LDS row 64 wn + 16 t + 4 sigma(frow >> 2) + (frow & 3) (w_off, unchanged: it is what makes the read conflict-free), and that row has
// to be channel 64 wn + 4 frow + t: a lane's four fragments are then four CONSECUTIVE channels, and the 16 lanes of a pixel its 64.
// (sigma = (0, 2, 3, 1), its inverse (0, 3, 1, 2).)  tests/test_conv_sw_direct_model.py restates it.
__host__ __device__ constexpr int sw_direct_row(int r) {
  return (r & 64) + 4 * (4 * ((0x2130 >> (4 * ((r >> 2) & 3))) & 3) + (r & 3)) + ((r >> 4) & 3);
}

// n / d as umulhi(n, mul) >> shr, WITHOUT the select of ig_fastdiv for a divisor of 1 (mul == 0).  fp_conv3x3_sw_applicable refuses a
// geometry with Wo < 2 (and HoWo is a multiple of Wo), so the two divisors of this file are never 1; with the select, every one of the
// ~16 divisions in front of the first operand DMA was a branch whose taken side waited for its own scalar load of shr.
__device__ __forceinline__ int sw_div(int n, unsigned mul, unsigned shr) { return (int)(__umulhi((unsigned)n, mul) >> shr); }

// The input geometry as k_conv_sw holds it: values read once at the top of the kernel
struct SwGeom {
  int HoWo, Wo, Hp, Wp;
  unsigned mulP, shrP, mulW, shrW;
};

// padded-grid index of tap (0,0) of output pixel m: (b * Hp + oy) * Wp + ox.  G: SwGeom or IgemmGeom
template <typename G>
__device__ __forceinline__ int sw_q(const G& g, int m) {
  const int b = sw_div(m, g.mulP, g.shrP);
  const int r = m - b * g.HoWo;
  const int oy = sw_div(r, g.mulW, g.shrW);
  const int ox = r - oy * g.Wo;
  return (b * g.Hp + oy) * g.Wp + ox;
}

// Tile shapes: 512 x 128 (the product's, every layer since round 4: see SW_FORCE_512 below) and 256 x 256 (N % 256 == 0); each wave owns
// 128 x 64 outputs = 16 MFMAs per k-step either way.
// S16 (round 7): the main loop on v_mfma_f32_16x16x32_f16 instead of v_mfma_f32_32x32x16_f16.  The wave tile, the LDS image of the
// weights, the staging and the schedule are the same; what changes is the fragment map -- lane l holds row (l & 15) and the 16-byte chunk
// (l >> 4) of a 64-byte row, so ONE ds_read_b128 fetches a K = 32 fragment of 16 rows: 8 pixel + 4 weight fragments per k-step, 32 MFMAs:
//  * ds_read_b128 serves the lanes in four non-contiguous groups of 16 ({0-3, 12-15, 20-27}, {4-11, 16-19, 28-31}, + 32), i.e. 8 rows of
//    one chunk and the 8 other rows of its neighbour.  The patch is therefore swizzled chunk ^ 2 * ((row >> 2) & 1): conflict-free for 16
//    consecutive patch rows at ANY offset, 2-way across one image-row crossing (tests/test_conv_sw16_model.py; chunk ^ ((row >> 2) & 3)
//    is 2-way under this lane map: 1027 against 681 clocks per k-step for the fragment reads alone, scripts/conv_loop_probe).
//  * the weight rows keep their image (and the tile-packed copy its layout); a fragment's A rows take the tile's channel quads in the order
//    sigma = (0, 2, 3, 1), which makes the aligned 16-row read conflict-free on that image; the epilogue undoes sigma (igemm_epilogue.h).
//  * a 16x16x32 MFMA holds the SIMD's vector issue for half of its 16 cycles (a 32x32x16 for a quarter of its 32), so the tap addresses in
//    the MFMA shadow are cut to three instructions per fragment (add, shift, and-xor), 24 per k-step: with the five-instruction form of the
//    32x32x16 loop (64 per k-step) the partner group's fragment reads no longer found issue slots (scripts/conv_loop_probe,
//    profiles/r07_a_mfma_shape_probe.log: 1390 -> 1302 clocks per k-step).
// Sums of 32 products per MFMA instead of 2 x 16: by the ISA equal to S16 = false up to fp32 summation order only; measured on gfx950 the two
// loops return the same bits on every tested layer (profiles/r07_b_ab_mfma_shape.log), and the tests hold both to the policy's flip gates.
//
// DIRECT (round 11, k_conv_sw_direct below): the 16x16x32 MFMAs with their two source operands exchanged, pixels as A and weights as B, so that
// D is [pixel][channel] and the tile leaves from the accumulators (ig_epilogue_direct, igemm_epilogue.h).  Everything else of the main loop is
// the same text; what differs around it is the order of the weight rows in their LDS image (sw_direct_row) and the output row table, which
// is built in the prologue behind the first DMAs.
template <int BM, int BN, int TM, bool S16>
__global__ __launch_bounds__(512, 1) void k_conv_sw(IgemmParams p) {
  constexpr bool DIRECT = false;
#include "conv_sw_tile.inc"
}

// the tile on exchanged 16x16x32 MFMAs, stored straight from the accumulators: <512, 128, 4, true> only (the static_assert of the body)
template <int BM, int BN, int TM, bool S16>
__global__ __launch_bounds__(512, 1) void k_conv_sw_direct(IgemmParams p) {
  constexpr bool DIRECT = true;
#include "conv_sw_tile.inc"
}

// ---------------------------------------------------------------------------------------------------------------------
// k_conv_sw_ls -- the same shifted-window convolution as a LOCK-STEP kernel with TWO workgroups per CU (round 3).
// Why: k_conv_sw holds one 512-thread workgroup per CU, so nothing runs on the CU during a tile's cold start (first patch
// + weights: ~4 us) and epilogue (~8 us) -- 16 % of a 256->256 tile, 29 % of a 128-channel tile; making the
// kernel persistent serialised the same waves and was slower.  Here a workgroup is 4 waves (one per SIMD) on a 256 x 128
// tile -- each wave still owns 128 x 64 outputs = 16 MFMAs per k-step, the intensity of the ping-pong kernel -- and its
// LDS is exactly half of the CU's: two patch buffers of 448 rows x 64 B (double buffered across channel chunks) + a ring
// of 3 weight stages of 128 x 64 B = 80 KiB.  Two workgroups are then resident per CU, unsynchronised with each other:
// one's cold start / epilogue / fragment reads run under the other's MFMAs (the matrix pipe arbitrates by age, so two
// workgroups that start in phase drift apart).  One workgroup barrier per k-step: at the top of k-step s every wave has
// waited for its own pieces of W(s) (and of the chunk's patch), so past the barrier W(s) is visible to all and everyone
// is done reading the buffers of k-step s-1, which is where W(s+2) and the next patch piece are sent.
// The per-channel epilogue vectors do not fit beside the 80 KiB during the main loop; they are fetched into the (then
// free) staging area at the start of the epilogue, under the other workgroup's main loop.
constexpr int LS_PROWS = 448, LS_NSTW = 3;

template <int BM, int BN, int TM>
__global__ __launch_bounds__(256, 2) void k_conv_sw_ls(IgemmParams p) {
  constexpr int BK = SW_BK, NW = 4, THREADS = 256;
  constexpr int NWN = BN / 64;
  static_assert((BM / (32 * TM)) * NWN == NW, "4 waves");
  constexpr int ROWB = BK * 2;
  constexpr int W_BYTES = BN * ROWB;
  constexpr int PATCH_BYTES = LS_PROWS * ROWB;
  constexpr int WI = BN / 16 / NW;                  // weight LDS-DMA instructions per wave and k-step
  constexpr int PI = LS_PROWS / 16 / NW;            // patch instructions per wave and chunk: one at each of taps 0..PI-1
  static_assert(WI >= 1 && PI >= 1 && PI <= 8 && LS_PROWS == PI * 16 * NW, "tile shape");
  constexpr int STAGES_BYTES = 2 * PATCH_BYTES + LS_NSTW * W_BYTES;
  static_assert(STAGES_BYTES >= BM * BN * 2 + BM * 16 + IG_BIAS_LDS, "the epilogue tile, its tables and the vectors reuse the staging area");
  auto swz = [](int row) { return (row >> 2) & 3; };
  extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
  unsigned char* const patch = smem;
  unsigned char* const wring = smem + 2 * PATCH_BYTES;
  const int tid = threadIdx.x, lane = tid & 63;
  const int wid = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int wm = wid / NWN, wn = wid - wm * NWN;

  const int tiles_n = p.N / BN;
  const int nwg = gridDim.x;
  const int xcd = blockIdx.x & 7, loc = blockIdx.x >> 3;
  const int qd8 = nwg >> 3, r8 = nwg & 7;
  const int tile = (xcd < r8 ? xcd * (qd8 + 1) : r8 * (qd8 + 1) + (xcd - r8) * qd8) + loc;
  const int bm = tile / tiles_n, bn = tile - bm * tiles_n;
  const int m0 = bm * BM, n0 = bn * BN;
  const int Cin = p.Cin, Ktot = 9 * Cin, Wp = p.in.Wp;
  const int ncc = Cin / BK;

  const int q0 = sw_q(p.in, m0);
  const int qmax = (p.M / p.in.HoWo) * p.in.Hp * Wp - 1;
  unsigned poff32[PI], woff32[WI];
#pragma unroll
  for (int j = 0; j < PI; ++j) {
    const int row = (wid * PI + j) * 16 + (lane >> 2);
    const int c = (lane & 3) ^ swz(row);
    int q = q0 + row;
    q = q < qmax ? q : qmax;
    poff32[j] = (unsigned)(((long long)q * p.in.cstride + p.in.coff + c * 8) * 2);
  }
#pragma unroll
  for (int j = 0; j < WI; ++j) {
    const int row = (wid * WI + j) * 16 + (lane >> 2);
    const int c = (lane & 3) ^ swz(row);
    woff32[j] = (unsigned)((((size_t)(n0 + row) * Ktot) + c * 8) * 2);
  }
  const __amdgpu_buffer_rsrc_t rsA = __builtin_amdgcn_make_buffer_rsrc(const_cast<_Float16*>(p.A), 0, 0x7FFFFFFF, 0x00020000);
  const __amdgpu_buffer_rsrc_t rsW = __builtin_amdgcn_make_buffer_rsrc(const_cast<_Float16*>(p.Wt), 0, 0x7FFFFFFF, 0x00020000);

  auto stage_patch = [&](int cc, int j) {
    unsigned char* dst = patch + (cc & 1) * PATCH_BYTES + (wid * PI + j) * 1024;
    __builtin_amdgcn_raw_ptr_buffer_load_lds(rsA, (__attribute__((address_space(3))) void*)dst, 16, (int)poff32[j],
                                             cc * (BK * 2), 0, 0);
  };
  auto stage_w = [&](int cc, int tap, int slot) {
    const int wsoff = (tap * Cin + cc * BK) * 2;
    unsigned char* dst = wring + slot * W_BYTES + wid * (WI * 1024);
#pragma unroll
    for (int j = 0; j < WI; ++j)
      __builtin_amdgcn_raw_ptr_buffer_load_lds(rsW, (__attribute__((address_space(3))) void*)(dst + j * 1024), 16,
                                               (int)woff32[j], wsoff, 0, 0);
  };

  float16_ acc[2][TM];
#pragma unroll
  for (int i = 0; i < 2; ++i)
#pragma unroll
    for (int j = 0; j < TM; ++j)
#pragma unroll
      for (int e = 0; e < 16; ++e) acc[i][j][e] = 0.f;

  const int frow = lane & 31, fhalf = lane >> 5;
  int arow[TM], w_off[2][2];
#pragma unroll
  for (int t = 0; t < TM; ++t) {
    int m = m0 + wm * (32 * TM) + t * 32 + frow;
    m = m < p.M ? m : p.M - 1;
    arow[t] = sw_q(p.in, m) - q0;
  }
#pragma unroll
  for (int t = 0; t < 2; ++t) {
    const int rw = wn * 64 + t * 32 + frow;
#pragma unroll
    for (int kk = 0; kk < 2; ++kk) w_off[t][kk] = rw * ROWB + (((2 * kk + fhalf) ^ swz(rw)) << 4);
  }

  // ---- prologue: patch(0), W(0), W(1) requested
#pragma unroll
  for (int j = 0; j < PI; ++j) stage_patch(0, j);
  stage_w(0, 0, 0);
  stage_w(0, 1, 1);

  // k-step s = (chunk cc, tap T); weight slot s % 3 = T % 3.  vmcnt at the top (loads retire in order): this wave's pieces
  // of W(s) must have landed; younger and allowed in flight is what k-step s-1 sent: W(s+1) and its patch piece.
  auto kstep = [&](int cc, auto tap_c, auto last_c, auto first_c) {
    constexpr int T = decltype(tap_c)::value;
    constexpr bool LAST = decltype(last_c)::value;     // last chunk: no next patch, the weight prefetch runs dry
    constexpr bool FIRST = decltype(first_c)::value;   // k-step 0 of the tile: the prologue stands in for k-step -1
    constexpr int ky = T / 3, kx = T - 3 * ky;
    {
      // previous k-step: tap T-1 of this chunk, or tap 8 of the chunk before (never the last chunk, no patch piece at tap 8)
      constexpr bool prev_w = FIRST || T == 0 || !LAST || (T - 1) + 2 < 9;      // did k-step s-1 send W(s+1)?
      constexpr bool prev_p = !FIRST && T >= 1 && !LAST && (T - 1) < PI;        // ... and a patch piece?
      sw_wait_vm<(prev_w ? WI : 0) + (prev_p ? 1 : 0)>();
    }
    __builtin_amdgcn_sched_barrier(0);
    __builtin_amdgcn_s_barrier();
    __builtin_amdgcn_sched_barrier(0);
    if constexpr (!LAST) {
      // the patch piece BEFORE the weights: waiting for W(s+2) two k-steps later then also covers this piece
      if constexpr (T < PI) stage_patch(cc + 1, T);
      if constexpr (T + 2 < 9) stage_w(cc, T + 2, (T + 2) % LS_NSTW);
      else stage_w(cc + 1, T - 7, (T + 2) % LS_NSTW);
    } else {
      if constexpr (T + 2 < 9) stage_w(cc, T + 2, (T + 2) % LS_NSTW);
    }
    const unsigned char* pb = patch + (cc & 1) * PATCH_BYTES;
    const unsigned char* wb = wring + (T % LS_NSTW) * W_BYTES;
    const int shift = ky * Wp + kx;
    half8 fa[2][TM], fw[2][2];
    int a0[TM];
#pragma unroll
    for (int t = 0; t < TM; ++t) {
      int ar = arow[t];
      asm volatile("" : "+v"(ar));
      const int pr = ar + shift;
      a0[t] = (pr << 6) + ((fhalf ^ swz(pr)) << 4);
    }
#pragma unroll
    for (int t = 0; t < TM; ++t) fa[0][t] = *reinterpret_cast<const half8*>(pb + a0[t]);
#pragma unroll
    for (int t = 0; t < 2; ++t) fw[0][t] = *reinterpret_cast<const half8*>(wb + w_off[t][0]);
#pragma unroll
    for (int t = 0; t < TM; ++t) fa[1][t] = *reinterpret_cast<const half8*>(pb + (a0[t] ^ 32));
#pragma unroll
    for (int t = 0; t < 2; ++t) fw[1][t] = *reinterpret_cast<const half8*>(wb + w_off[t][1]);
    __builtin_amdgcn_sched_barrier(0);   // all twelve fragment reads are requested before the first MFMA
#pragma unroll
    for (int kk = 0; kk < 2; ++kk)
#pragma unroll
      for (int i = 0; i < 2; ++i)
#pragma unroll
        for (int j = 0; j < TM; ++j)
          acc[i][j] = __builtin_amdgcn_mfma_f32_32x32x16_f16(fw[kk][i], fa[kk][j], acc[i][j], 0, 0, 0);
    __builtin_amdgcn_sched_barrier(0);
  };
  auto chunk = [&](int cc, auto last_c, auto first_c) {
    kstep(cc, std::integral_constant<int, 0>{}, last_c, first_c);
    kstep(cc, std::integral_constant<int, 1>{}, last_c, std::false_type{});
    kstep(cc, std::integral_constant<int, 2>{}, last_c, std::false_type{});
    kstep(cc, std::integral_constant<int, 3>{}, last_c, std::false_type{});
    kstep(cc, std::integral_constant<int, 4>{}, last_c, std::false_type{});
    kstep(cc, std::integral_constant<int, 5>{}, last_c, std::false_type{});
    kstep(cc, std::integral_constant<int, 6>{}, last_c, std::false_type{});
    kstep(cc, std::integral_constant<int, 7>{}, last_c, std::false_type{});
    kstep(cc, std::integral_constant<int, 8>{}, last_c, std::false_type{});
  };
  chunk(0, std::false_type{}, std::true_type{});                 // ncc >= 2 (Cin % 64 == 0)
  for (int cc = 1; cc + 1 < ncc; ++cc) chunk(cc, std::false_type{}, std::false_type{});
  chunk(ncc - 1, std::true_type{}, std::false_type{});
  __syncthreads();                                               // every fragment read retired: the staging area is free
  float* bias_lds = reinterpret_cast<float*>(smem + BM * BN * 2 + BM * 16);
  ig_bias_to_lds(p, n0, bias_lds, wid, lane);
  asm volatile("s_waitcnt vmcnt(0)" ::: "memory");               // visible after the first barrier of the epilogue
  ig_epilogue<BM, BN, TM, THREADS, 0>(p, acc, smem, m0, n0, wm, wn, tid, lane, bias_lds);
}

template <int BM, int BN, int TM>
int sw_ls_launch(const IgemmParams& p, hipStream_t stream) {
  constexpr int LDS = 2 * LS_PROWS * SW_BK * 2 + LS_NSTW * BN * SW_BK * 2;
  static_assert(2 * LDS <= 160 * 1024, "two workgroups per CU");
  const long long tiles = (long long)fp_cdiv(p.M, BM) * (p.N / BN);
  FP_REQUIRE(tiles < (1ll << 31), "fp_igemm_f16_fwd: too many tiles");
  FP_SET_MAX_LDS((k_conv_sw_ls<BM, BN, TM>), LDS);
  hipLaunchKernelGGL((k_conv_sw_ls<BM, BN, TM>), dim3((unsigned)tiles), dim3(256), LDS, stream, p);
  FP_CHECK_LAUNCH("fp_igemm_f16_fwd(conv_sw_ls)");
  return FP_OK;
}

// LDS of a k_conv_sw workgroup.  512 x 128: 128 KiB of staging buffers = the E tile, 2 KiB of row table, 3 KiB of vectors = 136192 B,
// 107 allocation granules of 1280 B: with the 25872 B (21 granules) of a k_raster workgroup on 160-pixel crops that is the CU's 160 KiB
constexpr int sw_lds_bytes(int BM, int BN) {
  return (BM == 256 ? ig_lds_main_slim<256, 256>(2 * sw_prows(256) * SW_BK * 2 + SW_NSTW * 256 * SW_BK * 2)
                    : ig_lds_main_slim<512, 128>(2 * sw_prows(512) * SW_BK * 2 + SW_NSTW * 128 * SW_BK * 2)) + IG_BIAS_LDS;
}

template <int BM, int BN, int TM, bool S16>
int sw_launch(const IgemmParams& p, hipStream_t stream) {
  static_assert((BM == 256 && BN == 256) || (BM == 512 && BN == 128), "tile shapes of sw_lds_bytes");
  constexpr int LDS = sw_lds_bytes(BM, BN);
  static_assert(LDS <= 160 * 1024, "does not fit the 160 KiB LDS");
  const long long tiles = (long long)fp_cdiv(p.M, BM) * (p.N / BN);
  FP_REQUIRE(tiles < (1ll << 31), "fp_igemm_f16_fwd: too many tiles");
  FP_SET_MAX_LDS((k_conv_sw<BM, BN, TM, S16>), LDS);
  hipLaunchKernelGGL((k_conv_sw<BM, BN, TM, S16>), dim3((unsigned)tiles), dim3(512), LDS, stream, p);
  FP_CHECK_LAUNCH("fp_igemm_f16_fwd(conv_sw)");
  return FP_OK;
}

}  // namespace

// The patch of a tile is the run of padded pixels from tap (0,0) of its first output pixel to tap (2,2) of its last:
// BM - 1 + 2 per image-row crossing + 2 Wp + 2 per image crossing + 2 Wp + 3.  It has to fit the patch buffer.
static int sw_span(const IgemmGeom& g, int BM) {
  const int row_cross = (BM - 1) / g.Wo + 1, img_cross = (BM - 1) / g.HoWo + 1;
  return (BM - 1) + 2 * row_cross + (2 * g.Wp + 2) * img_cross + 2 * g.Wp + 3;
}

// which schedule: 1 = lock-step 256 x 128 tiles, two workgroups per CU (k_conv_sw_ls); 0 = ping-pong, one per CU
static int sw_variant(const IgemmParams& p) {
  int v = SW_DEFAULT_VARIANT;
#ifdef FP_PROFILE_BUILD
  static int forced = -2;
  if (forced == -2) {
    const char* e = getenv("FP_CONV_SW");          // profiling build only: ls | pp
    forced = e ? (!strcmp(e, "ls") ? 1 : (!strcmp(e, "pp") ? 0 : -1)) : -1;
  }
  if (forced >= 0) v = forced;
#endif
  // 2 / 3 (round 6 A/B builds): the two-per-CU lock-step kernel only where it measured ahead of the ping-pong kernel at sub-batch size
  // (DESIGN_HISTORY 3.2: 128 -> 128 +3-5 %, 256 -> 256 +2-3 %, 512 -> 512 -12 %): layers of up to 128 / 256 input channels
  if (v == 2) v = p.Cin <= 128 ? 1 : 0;
  if (v == 3) v = p.Cin <= 256 ? 1 : 0;
  if (v == 1 && sw_span(p.in, 256) > LS_PROWS) v = 0;
  return v;
}

// Round 4: 512 x 128 tiles for EVERY layer, also where N is a multiple of 256 (-DSW_FORCE_512=0 restores 256 x 256 there).  Per k-step a
// 256 x 256 tile stages 16 KB of weights + ~3.5 KB of patch for its 128 MFMAs, a 512 x 128 tile 8 KB + ~5 KB: a third fewer LDS-DMA
// pieces per MFMA, and the pieces' issue cost next to MFMAs is what the main loop is bound by; the activation rows are
// then fetched once per column tile (from L2 the second time).  Same k order per accumulator: the same bits.
#ifndef SW_FORCE_512
#define SW_FORCE_512 1
#endif
// (launches of fewer than two 512-row tiles keep the 256 x 256 shape where it exists, so that the smallest batches -- two hypotheses on
// the 20 x 20 layers -- stay on this kernel and on its summation order, as before the change)
static bool sw_use_256(const IgemmParams& p) { return (p.N % 256) == 0 && (!SW_FORCE_512 || p.M < 2 * 512); }
static int sw_tile_rows(const IgemmParams& p) { return sw_variant(p) == 1 ? 256 : (sw_use_256(p) ? 256 : 512); }

bool fp_conv3x3_sw_applicable(const IgemmParams& p) {
  const IgemmGeom& g = p.in;
  if (p.taps != 9 || g.stride != 1 || g.off != 0 || g.bsplit != 0) return false;
  if (g.HoWo % g.Wo != 0 || g.Wp != g.Wo + 2 || g.Hp != g.HoWo / g.Wo + 2) return false;
  // images one pixel wide: the kernels divide by Wo and HoWo without the divisor-1 case of ig_fastdiv (sw_div).  Nothing is lost: a patch
  // of such a tile (two border pixels per output pixel) fits no patch buffer, sw_span below
  if (g.Wo < 2) return false;
  const int BM = sw_tile_rows(p);
  if (p.M % g.HoWo != 0 || p.M < 2 * BM) return false;
  if (p.Cin % 64 != 0 || p.N % 128 != 0) return false;
  const long long bytes = (long long)(p.M / g.HoWo) * g.Hp * g.Wp * g.cstride * 2;
  if (bytes >= (1ll << 31)) return false;           // 32-bit byte offsets in the LDS-DMA source addresses
  if (g.cstride >= (1 << 19)) return false;         // ... formed BEFORE the clamp to the tensor's end: 1024 rows of a patch stay below 2^31 bytes
  // 32-bit tile-relative row offsets in the epilogue's output table (igemm_epilogue.h, SLIM): elements of the output buffer
  const IgemmGeom& o = p.out;
  const long long imgs = o.bsplit > 0 ? o.bsplit : p.M / g.HoWo, groups = o.bsplit > 0 ? (p.M / g.HoWo) / o.bsplit + 1 : 0;
  if (imgs * o.Hp * o.Wp * o.cstride + o.coff + groups * (long long)o.cgroup >= (1ll << 31)) return false;
  // ... and 32-bit byte offsets from the buffer's start for the output rows and for the residual rows (ig_epilogue_spec, SLIM)
  if (p.R) {
    const IgemmGeom& r = p.res;
    const long long rimgs = r.bsplit > 0 ? r.bsplit : p.M / g.HoWo, rgroups = r.bsplit > 0 ? (p.M / g.HoWo) / r.bsplit + 1 : 0;
    if (rimgs * r.Hp * r.Wp * r.cstride + r.coff + rgroups * (long long)r.cgroup >= (1ll << 31)) return false;
  }
  return sw_span(g, BM) <= (sw_variant(p) == 1 ? LS_PROWS : sw_prows(BM));
}

int fp_conv3x3_sw_tile_rows(const IgemmParams& p) { return sw_tile_rows(p); }

extern "C" int fp_conv3x3_sw_lds_bytes(void) { return sw_lds_bytes(512, 128); }

// FP_IGEMM_DIRECT_STORE reaches k_conv_sw_direct where that kernel exists: the 512 x 128 tile of the ping-pong schedule on 16x16x32 MFMAs,
// for the four layer kinds without the positional second output.  Every other launch stays on k_conv_sw.
static bool sw_direct(const IgemmParams& p) {
  if (!p.direct || !p.mfma16 || sw_variant(p) == 1 || sw_use_256(p)) return false;
  return p.epi == IG_EPI_CONV || p.epi == (IG_EPI_CONV | IG_EPI_RES) || p.epi == (IG_EPI_CONV | IG_EPI_BN) || p.epi == (IG_EPI_CONV | IG_EPI_BN | IG_EPI_RES);
}

static int sw_direct_launch(const IgemmParams& p, hipStream_t stream) {
  constexpr int LDS = sw_lds_bytes(512, 128);      // not a byte more than k_conv_sw<512,128>: the co-residency with k_raster (round 8)
  const long long tiles = (long long)fp_cdiv(p.M, 512) * (p.N / 128);
  FP_REQUIRE(tiles < (1ll << 31), "fp_igemm_f16_fwd: too many tiles");
  FP_SET_MAX_LDS((k_conv_sw_direct<512, 128, 4, true>), LDS);
  hipLaunchKernelGGL((k_conv_sw_direct<512, 128, 4, true>), dim3((unsigned)tiles), dim3(512), LDS, stream, p);
  FP_CHECK_LAUNCH("fp_igemm_f16_fwd(conv_sw_direct)");
  return FP_OK;
}

int fp_conv3x3_sw_launch(const IgemmParams& p, hipStream_t stream) {
  const bool direct = sw_direct(p);
  // the two tile-packed layouts differ in their row order only, so the wrong one would be a silently permuted convolution: refused where
  // the kernel of this launch reads the pack (the 512 x 128 tile of the ping-pong schedule; every other kernel stages the plain weights)
  if (p.Wpk && sw_variant(p) != 1 && !sw_use_256(p))
    FP_REQUIRE((p.wpk_direct != 0) == direct, "fp_igemm_f16_fwd: w_tiles is in the layout of %s but this launch runs %s (FP_IGEMM_W_TILES_DIRECT, FP_IGEMM_DIRECT_STORE)",
               p.wpk_direct ? "fp_pack_conv3x3_tiles_direct_f16" : "fp_pack_conv3x3_tiles_f16", direct ? "k_conv_sw_direct" : "k_conv_sw");
  if (direct) return sw_direct_launch(p, stream);
  if (sw_variant(p) == 1) return sw_ls_launch<256, 128, 4>(p, stream);
  // p.mfma16: the MFMA shape of the ping-pong kernel's main loop (FP_IGEMM_MFMA_* of the epilogue flags; include/fp_amd.h)
  if (sw_use_256(p)) return p.mfma16 ? sw_launch<256, 256, 4, true>(p, stream) : sw_launch<256, 256, 4, false>(p, stream);
  return p.mfma16 ? sw_launch<512, 128, 4, true>(p, stream) : sw_launch<512, 128, 4, false>(p, stream);
}

// ---------------------------------------------------------------------------------------------------------------------
// fp_pack_conv3x3_tiles_f16: one thread per 16-byte chunk of the packed matrix (include/fp_amd.h has the layout)
template <bool DIRECT>
__global__ __launch_bounds__(256) void k_pack_conv3x3_tiles(const _Float16* __restrict__ w, _Float16* __restrict__ out, int N, int Cin) {
  const int nk = 9 * (Cin / 32);
  const long long total = (long long)N * nk * 4;          // chunks: N rows x nk k-steps x 4 chunks of 8 halves
  const long long q = (long long)blockIdx.x * 256 + threadIdx.x;
  if (q >= total) return;
  const int pc = (int)(q & 3);
  const int r = (int)((q >> 2) & 127);
  const long long blk = q >> 9;                            // bn * nk + s
  const int s = (int)(blk % nk), bn = (int)(blk / nk);
  const int cc = s / 9, tap = s - 9 * cc;
  const int lc = pc ^ ((r >> 2) & 3);
  const int src = DIRECT ? sw_direct_row(r) : r;           // DIRECT: row r of the image holds another channel; its chunks stay where they were
  const half8 v = *reinterpret_cast<const half8*>(w + (size_t)(bn * 128 + src) * (9 * Cin) + tap * Cin + cc * 32 + lc * 8);
  *reinterpret_cast<half8*>(out + q * 8) = v;
}

template <bool DIRECT>
static int sw_pack_tiles(const void* w, void* w_tiles, int N, int Cin, void* stream, const char* who) {
  FP_REQUIRE(w && w_tiles && w != w_tiles, "%s: NULL tensor or in-place repack", who);
  FP_REQUIRE(N > 0 && N % 128 == 0 && Cin > 0 && Cin % 32 == 0, "%s: N=%d must be a multiple of 128, Cin=%d of 32", who, N, Cin);
  FP_REQUIRE((((size_t)w | (size_t)w_tiles) & 15) == 0, "%s: tensors must be 16-byte aligned", who);
  const long long total = (long long)N * 9 * (Cin / 32) * 4;
  hipLaunchKernelGGL(k_pack_conv3x3_tiles<DIRECT>, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, (hipStream_t)stream, (const _Float16*)w,
                     (_Float16*)w_tiles, N, Cin);
  FP_CHECK_LAUNCH(who);
  return FP_OK;
}

extern "C" int fp_pack_conv3x3_tiles_f16(const void* w, void* w_tiles, int N, int Cin, void* stream) {
  return sw_pack_tiles<false>(w, w_tiles, N, Cin, stream, "fp_pack_conv3x3_tiles_f16");
}

// ... with the rows of each 128-channel tile in the order of k_conv_sw_direct (sw_direct_row)
extern "C" int fp_pack_conv3x3_tiles_direct_f16(const void* w, void* w_tiles, int N, int Cin, void* stream) {
  return sw_pack_tiles<true>(w, w_tiles, N, Cin, stream, "fp_pack_conv3x3_tiles_direct_f16");
}
