// Shared by igemm.hip, igemm_pp.hip and conv_sw.hip: operand addressing, the kernel parameter block of fp_igemm_f16_fwd, the tile order
// and the launcher of the tile kernels.
#pragma once
#include <hip/hip_fp16.h>
#include <stddef.h>
#include "fp_common.h"

typedef _Float16 half8 __attribute__((ext_vector_type(8)));
typedef _Float16 half4 __attribute__((ext_vector_type(4)));
typedef float float16_ __attribute__((ext_vector_type(16)));

#define IG_BK 64
#ifndef SW_DEFAULT_MFMA16
#define SW_DEFAULT_MFMA16 1   // k_conv_sw without FP_IGEMM_MFMA_*: the 16x16x32 main loop (IgemmParams.mfma16)
#endif

struct IgemmGeom {      // row m -> element offset of pixel (b, y*stride + pad_off, x*stride + pad_off) in a padded NHWC buffer
  int HoWo, Wo;         // output pixels per image / per row (1,1 for a plain GEMM)
  int Hp, Wp;           // padded height / width of the buffer
  int stride;           // spatial stride applied to (oy, ox)
  int off;              // border offset added to the pixel position (0 for the conv input: tap (0,0) = top-left pad)
  int cstride;          // channels per pixel in the buffer
  int coff;             // first channel
  int bsplit;           // image b -> (b % bsplit), channel group (b / bsplit) * cgroup  (0 = off)
  int cgroup;
  unsigned mulP, shrP;  // n / HoWo, n / Wo, n / bsplit as umulhi(n, mul) >> shr (host-computed, exact for n < 2^31)
  unsigned mulW, shrW;
  unsigned mulB, shrB;
};

// division by a runtime constant without the ~40-instruction emulated divide (the row -> address maps run 20 times per
// thread and tile): mul == 0 encodes divisor 1
static inline void ig_fastdiv_init(int d, unsigned* mul, unsigned* shr) {
  if (d <= 1) { *mul = 0; *shr = 0; return; }
  int lg = 0;
  while ((1u << lg) < (unsigned)d) ++lg;              // ceil(log2 d)
  const int p = 31 + lg;
  *mul = (unsigned)(((1ull << p) + (unsigned)d - 1) / (unsigned)d);
  *shr = (unsigned)(p - 32);
}
__device__ __forceinline__ int ig_fastdiv(int n, unsigned mul, unsigned shr) {
  return mul ? (int)(__umulhi((unsigned)n, mul) >> shr) : n;
}

struct IgemmParams {
  // ---- the head: everything k_conv_sw reads in front of its first operand DMA (conv_sw.hip), as the first 128 bytes of the block, so
  // that the kernel fetches it with two wide scalar loads at its top instead of one load (and one wait) per field where the field is
  // first used.  Keep these members together and in front; the static_asserts below hold the layout.
  const _Float16* A;
  const _Float16* Wt;   // [N][taps*Cin]
  const _Float16* Wpk;  // the same weights tile-packed (fp_pack_conv3x3_tiles_f16) or null: read by k_conv_sw<512,128> only
  const float* bias;    // [N] or null
  const float* bn_scale;   // [N] or null: eval-mode BatchNorm as y = x * scale + shift, applied to the fp16-rounded conv + bias
  const float* bn_shift;
  int M, N, Cin, taps;
  IgemmGeom in;
  // ---- the rest: the epilogue's
  IgemmGeom out, res;
  const _Float16* R;    // residual or null
  _Float16* Y;
  const float* pe;      // optional second output (the positional-embedding add of network_modules.py:133-137 fused into the
  _Float16* Ype;        // last conv): Ype[m][n] = f16(f32(y[m][n]) + pe[m % pe_period][n]), a plain (M, N) matrix
  int pe_period;
  int relu;
  int round_acc;        // FP_IGEMM_ROUND_ACC: the accumulator is rounded to fp16 BEFORE the bias is added (nn.Conv2d under
                        // autocast: ATen adds the bias to the fp16 convolution output); 0: one rounding of acc + bias (nn.Linear)
  int mfma16;           // k_conv_sw: main loop on v_mfma_f32_16x16x32_f16 (1) or v_mfma_f32_32x32x16_f16 (0); FP_IGEMM_MFMA_*
  int epi;              // layer kind of the epilogue (IG_EPI_* below; igemm.hip ig_epilogue_mode): 0 = the generic body of igemm_epilogue.h
  unsigned pe_mul, pe_shr;   // m / pe_period as ig_fastdiv (the layer-kind bodies; the generic body divides)
  int direct;           // FP_IGEMM_DIRECT_STORE: the 512 x 128 tile of k_conv_sw leaves from its accumulators where k_conv_sw_direct applies (conv_sw.hip)
  float* slab;          // split-K only (fp_igemm_f16_splitk_fwd): fp32 partial accumulators in fragment order,
  int nsplit;           //   [split][tile][wave][(i, g, j)][lane] x float4; 0 = not split
  int wpk_direct;       // FP_IGEMM_W_TILES_DIRECT: Wpk has the row order of fp_pack_conv3x3_tiles_direct_f16
};
// (direct and wpk_direct, round 11, sit where the block had padding: its size, and with it every kernel's argument layout, is what it was)
static_assert(sizeof(IgemmParams) == 336, "IgemmParams grew: the hidden kernel arguments move");
static_assert(sizeof(IgemmGeom) == 64 && offsetof(IgemmParams, in) == 64 && offsetof(IgemmParams, out) == 128, "the head of IgemmParams is its first 128 bytes");

// IgemmParams.epi: what the epilogue of a launch consists of, as a bit set.  Bit 0 marks a body compiled for exactly that set
// (ig_epilogue_spec); the library compiles the six kinds of layer the two networks' plans launch -- IG_EPI_CONV, + BatchNorm, each
// plain / with a residual / with a residual and the positional second output -- and every other combination runs mode 0.
#define IG_EPI_SPEC 1
#define IG_EPI_ROUND_ACC 2
#define IG_EPI_BIAS 4
#define IG_EPI_BN 8
#define IG_EPI_RES 16
#define IG_EPI_RELU 32
#define IG_EPI_PE 64
#define IG_EPI_CONV (IG_EPI_SPEC | IG_EPI_ROUND_ACC | IG_EPI_BIAS | IG_EPI_RELU)   // nn.Conv2d rounding, bias, ReLU

__device__ __forceinline__ long long ig_row_off(const IgemmGeom& g, int m) {
  const int b = ig_fastdiv(m, g.mulP, g.shrP);
  const int r = m - b * g.HoWo;
  const int oy = ig_fastdiv(r, g.mulW, g.shrW);
  const int ox = r - oy * g.Wo;
  int bb = b, cg = 0;
  if (g.bsplit > 0) { cg = ig_fastdiv(b, g.mulB, g.shrB); bb = b - cg * g.bsplit; }
  return (((long long)bb * g.Hp + (oy * g.stride + g.off)) * g.Wp + (ox * g.stride + g.off)) * g.cstride + g.coff +
         (long long)cg * g.cgroup;
}

// XCD-aware tile order (bijective for any grid size): workgroup `block` of a grid of nwg runs on XCD block % 8, and the tiles of one XCD are
// consecutive -- the channel tiles of one pixel tile, and neighbouring pixel tiles, share that XCD's L2.
// (block as unsigned: the shift of blockIdx.x stays a logical one)
__device__ __forceinline__ int ig_xcd_tile(unsigned block, int nwg) {
  const int xcd = block & 7, loc = block >> 3;
  const int q = nwg >> 3, r8 = nwg & 7;
  return (xcd < r8 ? xcd * (q + 1) : r8 * (q + 1) + (xcd - r8) * q) + loc;
}

// The launch of a tile kernel of the family: one workgroup of THREADS threads and LDS bytes per BM x BN tile, times the k ranges of a
// split-K product (IgemmParams.nsplit; 0 = not split).  `name` is the launch's in the error text.
template <void (&KERNEL)(IgemmParams), int BM, int BN, int THREADS, int LDS>
static int ig_launch_tiles(const IgemmParams& p, hipStream_t stream, const char* name) {
  static_assert(LDS <= 160 * 1024, "tile does not fit the 160 KiB LDS");
  const long long tiles = (long long)fp_cdiv(p.M, BM) * (p.N / BN);
  const int ny = p.nsplit ? p.nsplit : 1;
  FP_REQUIRE(tiles * ny < (1ll << 31) && ny <= 65535, "%s: too many tiles", p.nsplit ? "fp_igemm_f16_splitk_fwd" : "fp_igemm_f16_fwd");
  FP_SET_MAX_LDS(KERNEL, LDS);
  hipLaunchKernelGGL(KERNEL, dim3((unsigned)tiles, (unsigned)ny), dim3(THREADS), LDS, stream, p);
  FP_CHECK_LAUNCH(name);
  return FP_OK;
}

