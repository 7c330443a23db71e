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

// LDS of a k_conv_sw workgroup.  512 x 128: 128 KiB of staging buffers = the E tile, 2 KiB of row table, 3 KiB of vectors = 136192 B,
// 107 allocation granules of 1280 B: with the 25872 B (21 granules) of a k_raster workgroup on 160-pixel crops that is the CU's 160 KiB
constexpr int sw_lds_bytes(int BM, int BN) {
  return (BM == 256 ? ig_lds_main_slim<256, 256>(2 * sw_prows(256) * SW_BK * 2 + SW_NSTW * 256 * SW_BK * 2)
                    : ig_lds_main_slim<512, 128>(2 * sw_prows(512) * SW_BK * 2 + SW_NSTW * 128 * SW_BK * 2)) + IG_BIAS_LDS;
}

template <int BM, int BN, int TM, bool S16>
int sw_launch(const IgemmParams& p, hipStream_t stream) {
  static_assert((BM == 256 && BN == 256) || (BM == 512 && BN == 128), "tile shapes of sw_lds_bytes");
  return ig_launch_tiles<k_conv_sw<BM, BN, TM, S16>, BM, BN, 512, sw_lds_bytes(BM, BN)>(p, stream, "fp_igemm_f16_fwd(conv_sw)");
}

}  // namespace

// The patch of a tile is the run of padded pixels from tap (0,0) of its first output pixel to tap (2,2) of its last:
// BM - 1 + 2 per image-row crossing + 2 Wp + 2 per image crossing + 2 Wp + 3.  It has to fit the patch buffer.
static int sw_span(const IgemmGeom& g, int BM) {
  const int row_cross = (BM - 1) / g.Wo + 1, img_cross = (BM - 1) / g.HoWo + 1;
  return (BM - 1) + 2 * row_cross + (2 * g.Wp + 2) * img_cross + 2 * g.Wp + 3;
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
static int sw_tile_rows(const IgemmParams& p) { return sw_use_256(p) ? 256 : 512; }

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
  return sw_span(g, BM) <= sw_prows(BM);
}

extern "C" int fp_conv3x3_sw_lds_bytes(void) { return sw_lds_bytes(512, 128); }

// FP_IGEMM_DIRECT_STORE reaches k_conv_sw_direct where that kernel exists: the 512 x 128 tile of the ping-pong schedule on 16x16x32 MFMAs,
// for the four layer kinds without the positional second output.  Every other launch stays on k_conv_sw.
static bool sw_direct(const IgemmParams& p) {
  if (!p.direct || !p.mfma16 || sw_use_256(p)) return false;
  return p.epi == IG_EPI_CONV || p.epi == (IG_EPI_CONV | IG_EPI_RES) || p.epi == (IG_EPI_CONV | IG_EPI_BN) || p.epi == (IG_EPI_CONV | IG_EPI_BN | IG_EPI_RES);
}

static int sw_direct_launch(const IgemmParams& p, hipStream_t stream) {
  // LDS: not a byte more than k_conv_sw<512,128>: the co-residency with k_raster (round 8)
  return ig_launch_tiles<k_conv_sw_direct<512, 128, 4, true>, 512, 128, 512, sw_lds_bytes(512, 128)>(p, stream, "fp_igemm_f16_fwd(conv_sw_direct)");
}

int fp_conv3x3_sw_launch(const IgemmParams& p, hipStream_t stream) {
  const bool direct = sw_direct(p);
  // the two tile-packed layouts differ in their row order only, so the wrong one would be a silently permuted convolution: refused where
  // the kernel of this launch reads the pack (the 512 x 128 tile; the 256 x 256 tile stages the plain weights)
  if (p.Wpk && !sw_use_256(p))
    FP_REQUIRE((p.wpk_direct != 0) == direct, "fp_igemm_f16_fwd: w_tiles is in the layout of %s but this launch runs %s (FP_IGEMM_W_TILES_DIRECT, FP_IGEMM_DIRECT_STORE)",
               p.wpk_direct ? "fp_pack_conv3x3_tiles_direct_f16" : "fp_pack_conv3x3_tiles_f16", direct ? "k_conv_sw_direct" : "k_conv_sw");
  if (direct) return sw_direct_launch(p, stream);
  // p.mfma16: the MFMA shape of the main loop (FP_IGEMM_MFMA_* of the epilogue flags; include/fp_amd.h)
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
