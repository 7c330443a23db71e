// fp_attention_f16_fwd -- softmax(q k^T / sqrt(d)) v for the self-attention blocks of the two networks
// (nn.MultiheadAttention(512, 4) inside nn.TransformerEncoderLayer, refine_network.py:56-70, and the MHA layers of
// score_network.py:52-53, :84-88), heads of 128, fp16 in / fp32 softmax and accumulation / fp16 out, as one flash-style
// MFMA kernel: the (B*H, S, S) probability tensor (161 M elements at N=252) never exists.
//
// Input is the in_proj output as it stands: rows of [q(H*128) | k(H*128) | v(H*128)]; output rows of H*128 (heads merged),
// the operand of out_proj.  One workgroup = 8 waves = 8 query tiles of 32 rows of one (sequence, head); K and V of that
// head stream through LDS in blocks of 64 keys (double buffered; while a block is multiplied the next K block is in
// flight as LDS-DMA and the next V block in registers).
//
// MFMA bookkeeping (v_mfma_f32_32x32x16_f16; A lane l = A[l&31][8(l>>5)+i], B lane l = B[8(l>>5)+i][l&31],
// D lane l reg r = D[(r&3) + 8(r>>2) + 4(l>>5)][l&31]):
//   * scores are computed TRANSPOSED, S^T = K Q^T (A = K rows, B = Q rows): a lane then owns one query (l&31) and 16 of
//     the 32 keys of a tile, so row max / row sum are 15 lane-local ops + one exchange with lane l^32;
//   * O^T = V^T P^T (A = V^T rows = one d per lane, B = P rows = one query per lane) keeps the output lane-local in the
//     query as well, so the online-softmax rescale is a plain per-lane multiply;
//   * the k index of that second product is a PERMUTATION of the keys: k-slot 8(l>>5)+i of k-step s stands for key
//     16s + 4(l>>5) + (i&3) + 8(i>>2), which is exactly the order in which a lane already holds its probabilities
//     (registers 8s..8s+7 of the score tile) -- no cross-lane movement between the two products; V^T is read from LDS
//     with the same permutation (two 8-byte reads of 4 consecutive keys each).
//   * V arrives [key][d] and is transposed while it is written to LDS (16-bit scatter, XOR-swizzled so that the
//     fragment reads are conflict-free and the scatter is 2-way).
#include <hip/hip_fp16.h>
#include <stdlib.h>
#include <type_traits>
#include "fp_common.h"

#ifdef FP_PROFILE_BUILD
// profiling build only: 100 MHz wall-clock time per phase of k_attention_f16 (thread 0 of every workgroup), summed over the workgroups of
// a launch (scripts/dbg_attention.py): [0] prologue (Q fragments, K(0), V(0) resident), [1] the block loop, [2] output, [3] workgroups,
// [6] / [7] first start / last end
__device__ unsigned long long at_dbg[8];
extern "C" int fp_dbg_attention(unsigned long long* out, int reset) {
  if (reset) { unsigned long long z[8] = {0, 0, 0, 0, 0, 0, ~0ull, 0}; return (int)hipMemcpyToSymbol(HIP_SYMBOL(at_dbg), z, sizeof(z)); }
  return (int)hipMemcpyFromSymbol(out, HIP_SYMBOL(at_dbg), 8 * sizeof(unsigned long long));
}
#define AT_CLK(t) const unsigned long long t = wall_clock64()
#else
#define AT_CLK(t)
#endif

namespace {

typedef _Float16 half8 __attribute__((ext_vector_type(8)));
typedef _Float16 half4 __attribute__((ext_vector_type(4)));
typedef float float16_ __attribute__((ext_vector_type(16)));
typedef unsigned uint4_ __attribute__((ext_vector_type(4)));

constexpr int AT_D = 128;            // head size
constexpr int AT_KB = 64;            // keys per LDS block
constexpr int AT_K_BYTES = AT_KB * AT_D * 2;      // 16 KiB, [key][d], 16-byte chunks XORed with key & 15
constexpr int AT_VROW = 136;                      // bytes per d row of the V^T image: 64 keys + 8 bytes of padding
constexpr int AT_V_BYTES = AT_D * AT_VROW;        // 17 KiB, [d][key position], key position = key ^ vswz(d)
constexpr int AT_BUF = AT_K_BYTES + AT_V_BYTES;
constexpr int AT_LDS = 2 * AT_BUF;                // 66 KiB: two workgroups per CU

// swizzle of the key position inside a V^T row: bits 3:2 only, so that the k-step (bits 5:4) stays an immediate offset of
// the fragment reads; with the 136-byte rows both the 8-byte fragment reads and the 16-bit transposing scatter are 2-way
__device__ __forceinline__ int vswz(int d) { return 4 * ((d >> 3) & 3); }

// LDS-DMA of 64 x 16 B, lane-linear destination.  A plain function on purpose: written inline in the kernel TEMPLATE the
// address-space cast + builtin made hipcc 7.2 drop the kernel's host stub without a diagnostic (the object then has no
// fat binary and the launch links against an undefined symbol).
__device__ __forceinline__ void at_dma16(__amdgpu_buffer_rsrc_t rs, unsigned char* lds_dst, int voff, int soff) {
  __builtin_amdgcn_raw_ptr_buffer_load_lds(rs, (__attribute__((address_space(3))) void*)lds_dst, 16, voff, soff, 0, 0);
}

// Two shapes of the same kernel (round 3):
//   QT = 1, 8 waves: one 32-query tile per wave, two waves per SIMD (rounds 1-2; 212 VGPRs)
//   QT = 2, 4 waves: TWO query tiles per wave, one wave per SIMD with the whole 512-register file: every K and V^T fragment
//       read from LDS feeds two MFMAs instead of one (the fragment reads were as long as the MFMAs they fed), the fragments
//       of a whole block are in flight ahead of their use, and K / V of a head are staged by half as many waves.
template <int QT, int WAVES>
struct AtShape {
  static constexpr int THREADS = WAVES * 64;
  static constexpr int ROWS = 32 * QT * WAVES;     // query rows per workgroup
};

// Where a sequence lies in qkv / out (the kernel's SEQ parameter):
//   AtUniform  (fp_attention_f16_fwd): B sequences of S rows each, sequence b = rows b S .. b S + S - 1;
//   AtSegments (fp_attention_segments_f16_fwd): sequence b = rows offs[b] .. offs[b + 1] - 1 (device table, ragged lengths); the
//       grid is sized for max_S rows per sequence, and a workgroup whose query group lies past its own sequence's end returns
//       as a whole before the first barrier.
// `grid_S` is the length that sizes the grid; `seq(b, S, row0)` gives the length and first row of sequence b.
struct AtUniform {
  int S;
  __device__ __forceinline__ int grid_S() const { return S; }
  __device__ __forceinline__ void seq(int b, int& S_b, size_t& row0) const { S_b = S; row0 = (size_t)b * S; }
};
struct AtSegments {
  const int32_t* offs;
  int max_S;
  __device__ __forceinline__ int grid_S() const { return max_S; }
  __device__ __forceinline__ void seq(int b, int& S_b, size_t& row0) const {
    const int r0 = offs[b];
    S_b = offs[b + 1] - r0;
    row0 = (size_t)r0;
  }
};

// qscale > 0 selects the fp16-score policy of the need_weights=True branch of F.multi_head_attention_forward under
// autocast (score_network.py:73,86): q is multiplied by qscale = sqrt(1/d) and rounded to fp16, the q.k products are
// rounded to fp16 before the fp32 softmax (c is then log2(e) alone).  qscale == 0: scaled_dot_product_attention.
template <int QT, int WAVES, typename SEQ>
__global__ __launch_bounds__(WAVES * 64, QT == 1 ? 2 : 1) void k_attention_f16(const _Float16* __restrict__ qkv, _Float16* __restrict__ out,
                                                                            SEQ seqs, int H, float c /* log2(e)/sqrt(d) | log2(e) */, float qscale) {
  constexpr int THREADS = WAVES * 64;
  extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
  const int tid = threadIdx.x, lane = tid & 63, wid = tid >> 6;
  const int lq = lane & 31, hi = lane >> 5;
  const int nqg = (seqs.grid_S() + 32 * QT * WAVES - 1) / (32 * QT * WAVES);   // query groups per (sequence, head)
  const int qg = blockIdx.x % nqg, bh = blockIdx.x / nqg;
  const int h = bh % H, b = bh / H;
  int S;
  size_t row0;
  seqs.seq(b, S, row0);
  if (!std::is_same<SEQ, AtUniform>::value && qg * (32 * QT * WAVES) >= S) return;   // past the end of this segment (or an empty one)
  const int ld = 3 * H * AT_D, ldo = H * AT_D;
  const _Float16* qp = qkv + row0 * ld + h * AT_D;
  const _Float16* kp = qp + H * AT_D;
  const _Float16* vp = kp + H * AT_D;
  const int q0 = (qg * WAVES + wid) * (32 * QT);   // first query row of this wave
  const bool wave_active = q0 < S;                 // idle waves still help staging and keep the barriers matched

  AT_CLK(t_start);
  // ---- Q fragments (B operand): row q0 + 32 t + lq, d = 16 kk + 8 hi + 0..7
  half8 qf[QT][8];
#pragma unroll
  for (int t = 0; t < QT; ++t) {
    int qr = q0 + 32 * t + lq;
    qr = qr < S ? qr : S - 1;
    const _Float16* src = qp + (size_t)qr * ld + 8 * hi;
#pragma unroll
    for (int kk = 0; kk < 8; ++kk) qf[t][kk] = *reinterpret_cast<const half8*>(src + 16 * kk);
    if (qscale > 0.f) {
#pragma unroll
      for (int kk = 0; kk < 8; ++kk)
#pragma unroll
        for (int e = 0; e < 8; ++e) qf[t][kk][e] = (_Float16)((float)qf[t][kk][e] * qscale);
    }
  }

  // ---- staging.  K: LDS-DMA (buffer_load ... lds), 1 KiB = 4 keys per wave-instruction, 16 / WAVES pieces per wave and
  // block; the destination is lane-linear, so the XOR swizzle is applied to the SOURCE chunk: LDS chunk position
  // (lane & 15) of key row k holds d-chunk (lane & 15) ^ (k & 15).  V: through registers (it has to be transposed), thread t
  // owns chunks c = t + THREADS i: key = c % 8 + 8 (c / 128), d-chunk = (c / 8) % 16 (8 lanes = 8 consecutive keys).
  const __amdgpu_buffer_rsrc_t rsK = __builtin_amdgcn_make_buffer_rsrc(const_cast<_Float16*>(kp), 0, 0x7FFFFFFF, 0x00020000);
  const __amdgpu_buffer_rsrc_t rsV = __builtin_amdgcn_make_buffer_rsrc(const_cast<_Float16*>(vp), 0, 0x7FFFFFFF, 0x00020000);
  constexpr int KPW = 16 / WAVES;                  // K pieces per wave and block
  constexpr int VCH = 1024 / THREADS;              // 16-byte V chunks per thread and block
  // per-lane byte offsets inside a block, computed once; the block adds a scalar (blk * 64 rows).  Only a block that
  // reaches past the end of the sequence recomputes them with the row clamped (rows past the end are masked below,
  // any finite data will do).
  int koff[KPW], kkey[KPW], voff[VCH], vkey[VCH];
#pragma unroll
  for (int i = 0; i < KPW; ++i) {
    const int piece = wid * KPW + i;
    kkey[i] = piece * 4 + (lane >> 4);
    koff[i] = kkey[i] * (ld * 2) + (((lane & 15) ^ (kkey[i] & 15)) << 4);
  }
#pragma unroll
  for (int i = 0; i < VCH; ++i) {
    const int cidx = tid + THREADS * i;
    vkey[i] = (cidx & 7) + 8 * (cidx >> 7);
    voff[i] = vkey[i] * (ld * 2) + ((cidx >> 3) & 15) * 16;
  }
  uint4_ rv[VCH];
  auto stage_next = [&](int blk, int buf) {        // K of block blk: LDS-DMA into buffer buf; V of block blk: into registers
    const int soff = blk * AT_KB * (ld * 2);
    if ((blk + 1) * AT_KB <= S) {
#pragma unroll
      for (int i = 0; i < KPW; ++i)
        at_dma16(rsK, smem + buf * AT_BUF + (wid * KPW + i) * 1024, koff[i], soff);
#pragma unroll
      for (int i = 0; i < VCH; ++i) rv[i] = __builtin_bit_cast(uint4_, __builtin_amdgcn_raw_buffer_load_b128(rsV, voff[i], soff, 0));
    } else {
#pragma unroll
      for (int i = 0; i < KPW; ++i) {
        const int back = max(blk * AT_KB + kkey[i] - (S - 1), 0) * (ld * 2);
        at_dma16(rsK, smem + buf * AT_BUF + (wid * KPW + i) * 1024, koff[i] - back, soff);
      }
#pragma unroll
      for (int i = 0; i < VCH; ++i) {
        const int back = max(blk * AT_KB + vkey[i] - (S - 1), 0) * (ld * 2);
        rv[i] = __builtin_bit_cast(uint4_, __builtin_amdgcn_raw_buffer_load_b128(rsV, voff[i] - back, soff, 0));
      }
    }
  };
  auto vstore = [&](int buf) {
    unsigned char* vb = smem + buf * AT_BUF + AT_K_BYTES;
#pragma unroll
    for (int i = 0; i < VCH; ++i) {
      const int cidx = tid + THREADS * i;
      const int key = (cidx & 7) + 8 * (cidx >> 7), dc = (cidx >> 3) & 15;
      const half8 v = __builtin_bit_cast(half8, rv[i]);
      unsigned char* dst = vb + (8 * dc) * AT_VROW + ((key ^ vswz(8 * dc)) << 1);   // vswz is constant over the 8 d of a chunk
#pragma unroll
      for (int e = 0; e < 8; ++e) *reinterpret_cast<_Float16*>(dst + e * AT_VROW) = v[e];
    }
  };

  float16_ o[QT][4];                               // O^T: d tile dt, lane = query
#pragma unroll
  for (int t = 0; t < QT; ++t)
#pragma unroll
    for (int dt = 0; dt < 4; ++dt)
#pragma unroll
      for (int r = 0; r < 16; ++r) o[t][dt][r] = 0.f;
  float m[QT], l[QT];                              // running row max (raw scores) and row sum, per query = per lane pair
#pragma unroll
  for (int t = 0; t < QT; ++t) { m[t] = -1e30f; l[t] = 0.f; }

  const int nblk = (S + AT_KB - 1) / AT_KB;
  stage_next(0, 0);
  vstore(0);
  asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
  __syncthreads();
  AT_CLK(t_pro);
  auto do_block = [&](int blk, auto half_c) {
    const int cur = blk & 1;
    if (blk + 1 < nblk) stage_next(blk + 1, cur ^ 1);   // in flight while this block is multiplied
    const unsigned char* kb = smem + cur * AT_BUF;
    const unsigned char* vb = kb + AT_K_BYTES;
    // HALF: only the first 32 keys of the block exist (last block of a sequence with S mod 64 in 1..32, e.g. S = 400):
    // the second score tile, its half of the softmax and k-steps 2-3 of the second product are skipped instead of
    // multiplied with masked zeros -- 1/14 of the kernel's arithmetic at S = 400 (round 3)
    auto block_compute = [&]() {
      constexpr bool HALF = decltype(half_c)::value;
      constexpr int NKT = HALF ? 1 : 2;           // 32-key score tiles of this block
      const int key0 = blk * AT_KB;
      // ---- S^T tiles = K (2 x 32 keys) x Q^T (QT x 32 queries): 2 QT independent accumulator chains
      float16_ s[QT][2];
#pragma unroll
      for (int t = 0; t < QT; ++t)
#pragma unroll
        for (int r = 0; r < 16; ++r) { s[t][0][r] = 0.f; s[t][1][r] = HALF ? -1e30f : 0.f; }
      const unsigned char* krp = kb + lq * 256;    // rows lq and 32 + lq share (row & 15)
      constexpr int KRING = 3;                     // fragment ring: the reads of the next KRING-1 k-steps are in flight
      half8 kf[KRING][2];
      auto kread = [&](int kk, int slot) {
        const int pos = ((2 * kk + hi) ^ (lq & 15)) << 4;
        kf[slot][0] = *reinterpret_cast<const half8*>(krp + pos);
        if (!HALF) kf[slot][1] = *reinterpret_cast<const half8*>(krp + 32 * 256 + pos);
      };
#pragma unroll
      for (int kk = 0; kk < KRING - 1; ++kk) kread(kk, kk);
      // the V^T fragments of the first k-step of the second product are requested ahead of the softmax
      const unsigned char* vr0[4];
      const unsigned char* vr1[4];
#pragma unroll
      for (int dt = 0; dt < 4; ++dt) {
        const int d = 32 * dt + lq;
        vr0[dt] = vb + d * AT_VROW + (((4 * hi) ^ vswz(d)) << 1);
        vr1[dt] = vb + d * AT_VROW + (((8 + 4 * hi) ^ vswz(d)) << 1);
      }
      constexpr int VRING = 2;
      half4 va[VRING][4], vc[VRING][4];
      auto vread = [&](int ks, int slot) {
#pragma unroll
        for (int dt = 0; dt < 4; ++dt) {
          va[slot][dt] = *reinterpret_cast<const half4*>(vr0[dt] + 32 * ks);
          vc[slot][dt] = *reinterpret_cast<const half4*>(vr1[dt] + 32 * ks);
        }
      };
#pragma unroll
      for (int kk = 0; kk < 8; ++kk) {
        if (kk + KRING - 1 < 8) kread(kk + KRING - 1, (kk + KRING - 1) % KRING);
        else if (kk + KRING - 1 - 8 < VRING - 1) vread(kk + KRING - 1 - 8, kk + KRING - 1 - 8);   // V^T k-steps 0 .. VRING-2
        __builtin_amdgcn_sched_barrier(0);
#pragma unroll
        for (int t = 0; t < QT; ++t) {
          s[t][0] = __builtin_amdgcn_mfma_f32_32x32x16_f16(kf[kk % KRING][0], qf[t][kk], s[t][0], 0, 0, 0);
          if (!HALF) s[t][1] = __builtin_amdgcn_mfma_f32_32x32x16_f16(kf[kk % KRING][1], qf[t][kk], s[t][1], 0, 0, 0);
        }
      }
      half8 pf[QT][4];                             // P fragments of the four k-steps (16 permuted keys each)
#pragma unroll
      for (int t = 0; t < QT; ++t) {
        float16_& s0 = s[t][0];
        float16_& s1 = s[t][1];
        if (qscale > 0.f) {                        // `bmm` under autocast returns fp16 scores
#pragma unroll
          for (int r = 0; r < 16; ++r) { s0[r] = (float)(_Float16)s0[r]; if (!HALF) s1[r] = (float)(_Float16)s1[r]; }
        }
        if (key0 + AT_KB > S) {                    // keys past the end of the sequence (last block only)
#pragma unroll
          for (int r = 0; r < 16; ++r) {
            const int k = key0 + (r & 3) + 8 * (r >> 2) + 4 * hi;
            if (k >= S) s0[r] = -1e30f;
            if (!HALF && k + 32 >= S) s1[r] = -1e30f;
          }
        }
        // ---- online softmax over the 64 keys (base 2, scores scaled by c inside the exponent)
        float mx = HALF ? s0[0] : fmaxf(s0[0], s1[0]);
#pragma unroll
        for (int r = 1; r < 16; ++r) mx = HALF ? fmaxf(mx, s0[r]) : fmaxf(mx, fmaxf(s0[r], s1[r]));
        mx = fmaxf(mx, __shfl_xor(mx, 32));
        const float mn = fmaxf(m[t], mx);
        if (__any(mn > m[t])) {                    // rescale what has been accumulated under the old maximum
          const float alpha = __builtin_amdgcn_exp2f((m[t] - mn) * c);
          l[t] *= alpha;
#pragma unroll
          for (int dt = 0; dt < 4; ++dt)
#pragma unroll
            for (int r = 0; r < 16; ++r) o[t][dt][r] *= alpha;
          m[t] = mn;
        }
        const float mc = m[t] * c;
        float rs = 0.f;
        {
          typedef _Float16 half2_ __attribute__((ext_vector_type(2)));
          unsigned pw[4][4];
#pragma unroll
          for (int r = 0; r < 16; r += 2) {
            const float a0 = __builtin_amdgcn_exp2f(fmaf(s0[r], c, -mc)), a1 = __builtin_amdgcn_exp2f(fmaf(s0[r + 1], c, -mc));
            const half2_ ha = {(_Float16)a0, (_Float16)a1};   // one v_cvt_pk_f16_f32
            pw[r >> 3][(r & 7) >> 1] = __builtin_bit_cast(unsigned, ha);
            if constexpr (!HALF) {
              const float b0 = __builtin_amdgcn_exp2f(fmaf(s1[r], c, -mc)), b1 = __builtin_amdgcn_exp2f(fmaf(s1[r + 1], c, -mc));
              rs += (a0 + a1) + (b0 + b1);
              const half2_ hb = {(_Float16)b0, (_Float16)b1};
              pw[2 + (r >> 3)][(r & 7) >> 1] = __builtin_bit_cast(unsigned, hb);
            } else {
              rs += (a0 + a1) + 0.f;        // the masked second tile contributes exp2(-inf) = 0: same sum, bit for bit
              pw[2 + (r >> 3)][(r & 7) >> 1] = 0u;
            }
          }
#pragma unroll
          for (int u = 0; u < 4; ++u) {
            const uint4_ w = {pw[u][0], pw[u][1], pw[u][2], pw[u][3]};
            pf[t][u] = __builtin_bit_cast(half8, w);
          }
        }
        rs += __shfl_xor(rs, 32);
        l[t] += rs;
      }
      // V of the next block goes to LDS HERE (its global loads were requested at the top of the block, two products ago),
      // so that the 16-bit transposing scatter -- LDS-write-bound -- runs under the MFMAs of the second product instead of
      // after them, in front of the barrier, with the matrix pipe idle (round 3)
      if (blk + 1 < nblk) vstore(cur ^ 1);
      // ---- O^T += V^T P^T: k-step outer, query tile and d tile inner (4 QT independent accumulators in rotation); the
      // fragments of the next VRING-1 k-steps are requested before the MFMAs of this one
#pragma unroll
      for (int ks = 0; ks < 2 * NKT; ++ks) {      // HALF: k-steps 2 and 3 would multiply V by zero probabilities
        if (ks + VRING - 1 < 2 * NKT) vread(ks + VRING - 1, (ks + VRING - 1) % VRING);
        __builtin_amdgcn_sched_barrier(0);
#pragma unroll
        for (int dt = 0; dt < 4; ++dt) {
          const half4 lo = va[ks % VRING][dt], hi4 = vc[ks % VRING][dt];
          const half8 vf = {lo[0], lo[1], lo[2], lo[3], hi4[0], hi4[1], hi4[2], hi4[3]};
#pragma unroll
          for (int t = 0; t < QT; ++t) o[t][dt] = __builtin_amdgcn_mfma_f32_32x32x16_f16(vf, pf[t][ks], o[t][dt], 0, 0, 0);
        }
      }
    };
    if (wave_active) block_compute();
    if (!wave_active && blk + 1 < nblk) vstore(cur ^ 1);   // waves without queries only help staging
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");   // the K pieces of the next block have landed
    __syncthreads();
  };
  // the main loop runs whole 64-key blocks; the last block is peeled so that its 32-key variant does not add to the
  // register pressure of the loop (both variants inlined in the loop body cost 42 more VGPRs and spills)
  for (int blk = 0; blk + 1 < nblk; ++blk) do_block(blk, std::false_type{});
  if ((nblk - 1) * AT_KB + 32 >= S) do_block(nblk - 1, std::true_type{});
  else do_block(nblk - 1, std::false_type{});

  AT_CLK(t_loop);
  // ---- normalise, transpose through a wave-private LDS tile [32 QT queries][128 d] (16-byte chunks XORed with q & 15),
  // store whole 256-byte rows
  unsigned char* tile = smem + wid * (32 * QT * 256);   // WAVES x 8 QT KiB = 64 KiB inside the two buffers (everyone is past the last barrier)
  if (wave_active) {
#pragma unroll
    for (int t = 0; t < QT; ++t) {
      const float inv = 1.0f / l[t];
#pragma unroll
      for (int dt = 0; dt < 4; ++dt)
#pragma unroll
        for (int g = 0; g < 4; ++g) {
          half4 v;
#pragma unroll
          for (int e = 0; e < 4; ++e) v[e] = (_Float16)(o[t][dt][4 * g + e] * inv);
          const int chunk = (4 * dt + g) ^ (lq & 15);
          *reinterpret_cast<half4*>(tile + (32 * t + lq) * 256 + (chunk << 4) + 8 * hi) = v;
        }
    }
    __builtin_amdgcn_s_waitcnt(0xc07f);            // lgkmcnt(0): the tile is wave-private, no barrier needed
    __builtin_amdgcn_wave_barrier();
#pragma unroll
    for (int it = 0; it < 8 * QT; ++it) {
      const int idx = lane + 64 * it;
      const int r = idx >> 4, ch = idx & 15;
      const int q = q0 + r;
      if (q < S) {
        const uint4_ v = *reinterpret_cast<const uint4_*>(tile + r * 256 + ((ch ^ (r & 15)) << 4));
        *reinterpret_cast<uint4_*>(out + (row0 + q) * ldo + h * AT_D + ch * 8) = v;
      }
    }
  }
#ifdef FP_PROFILE_BUILD
  asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
  AT_CLK(t_end);
  if (tid == 0) {
    atomicAdd(&at_dbg[0], t_pro - t_start); atomicAdd(&at_dbg[1], t_loop - t_pro); atomicAdd(&at_dbg[2], t_end - t_loop);
    atomicAdd(&at_dbg[3], 1ull); atomicMin(&at_dbg[6], t_start); atomicMax(&at_dbg[7], t_end);
  }
#endif
}

template <int QT, int WAVES, typename SEQ>
int at_launch(const char* name, const void* qkv, void* out, int B, SEQ seqs, int grid_S, int H, float c, float qscale, hipStream_t stream) {
  static_assert(WAVES * 32 * QT * 256 <= AT_LDS, "the output tiles reuse the K / V buffers");
  const long long wgs = (long long)B * H * ((grid_S + 32 * QT * WAVES - 1) / (32 * QT * WAVES));
  FP_REQUIRE(wgs < (1ll << 31), "%s: too many workgroups", name);
  FP_SET_MAX_LDS((k_attention_f16<QT, WAVES, SEQ>), AT_LDS);
  hipLaunchKernelGGL((k_attention_f16<QT, WAVES, SEQ>), dim3((unsigned)wgs), dim3(WAVES * 64), AT_LDS, stream,
                     (const _Float16*)qkv, (_Float16*)out, seqs, H, c, qscale);
  FP_CHECK_LAUNCH(name);
  return FP_OK;
}

// K and V of a sequence are read through buffer resources based at its first row, with 32-bit byte offsets (int arithmetic
// in the kernel, num_records 0x7FFFFFFF): every row of a sequence, and the 64 rows of a key block before the tail clamp,
// must lie within 2 GiB of that base, or the loads come back as zeros instead of failing
bool at_span_ok(int S, int H) { return (long long)(S > AT_KB ? S : AT_KB) * (3ll * H * AT_D * 2) <= 0x7FFFFFFFll; }

}  // namespace

#ifndef AT_DEFAULT_QT
#define AT_DEFAULT_QT 1
#endif

extern "C" int fp_attention_f16_fwd(const void* qkv, void* out, int B, int S, int H, int head_dim, int flags, void* stream) {
  FP_REQUIRE(B >= 0 && S >= 0, "fp_attention_f16_fwd: negative size");
  if (B == 0 || S == 0) return FP_OK;
  FP_REQUIRE(qkv && out, "fp_attention_f16_fwd: NULL tensor");
  FP_REQUIRE(head_dim == AT_D, "fp_attention_f16_fwd: head_dim=%d (only 128 is built)", head_dim);
  FP_REQUIRE(H > 0 && ((((size_t)qkv | (size_t)out) & 15) == 0), "fp_attention_f16_fwd: bad head count / unaligned tensors");
  FP_REQUIRE((flags & ~FP_ATT_FP16_SCORES) == 0, "fp_attention_f16_fwd: unknown flags 0x%x", flags);
  FP_REQUIRE(at_span_ok(S, H), "fp_attention_f16_fwd: a sequence of S=%d rows of H=%d heads spans more than 2 GiB of qkv", S, H);
  const bool f16s = (flags & FP_ATT_FP16_SCORES) != 0;
  const float qscale = f16s ? (float)sqrt(1.0 / (double)head_dim) : 0.f;
  const float c = f16s ? 1.4426950408889634f : 1.4426950408889634f / sqrtf((float)head_dim);
#ifdef FP_PROFILE_BUILD
  // profiling build only: FP_ATT_QT=2 selects the measured-and-rejected 64-queries-per-wave shape
  static int forced = -1;
  if (forced < 0) { const char* e = getenv("FP_ATT_QT"); forced = e ? atoi(e) : 0; }
  if ((forced == 2 || (forced == 0 && AT_DEFAULT_QT == 2)) && S > 32)
    return at_launch<2, 4>("fp_attention_f16_fwd", qkv, out, B, AtUniform{S}, S, H, c, qscale, (hipStream_t)stream);
#endif
  return at_launch<1, 8>("fp_attention_f16_fwd", qkv, out, B, AtUniform{S}, S, H, c, qscale, (hipStream_t)stream);
}

extern "C" int fp_attention_segments_f16_fwd(const void* qkv, void* out, const int32_t* seg_offsets, int B, int max_S, int H,
                                             int head_dim, int flags, void* stream) {
  FP_REQUIRE(B >= 0 && max_S >= 0, "fp_attention_segments_f16_fwd: negative size (B=%d, max_S=%d)", B, max_S);
  FP_REQUIRE(qkv && out && seg_offsets, "fp_attention_segments_f16_fwd: NULL tensor");
  FP_REQUIRE(head_dim == AT_D, "fp_attention_segments_f16_fwd: head_dim=%d (only 128 is built)", head_dim);
  FP_REQUIRE(H > 0 && ((((size_t)qkv | (size_t)out) & 15) == 0) && ((size_t)seg_offsets & 3) == 0,
             "fp_attention_segments_f16_fwd: bad head count / unaligned tensors");
  FP_REQUIRE((flags & ~FP_ATT_FP16_SCORES) == 0, "fp_attention_segments_f16_fwd: unknown flags 0x%x", flags);
  FP_REQUIRE(at_span_ok(max_S, H), "fp_attention_segments_f16_fwd: a sequence of max_S=%d rows of H=%d heads spans more than 2 GiB of qkv",
             max_S, H);
  if (B == 0 || max_S == 0) return FP_OK;
  const bool f16s = (flags & FP_ATT_FP16_SCORES) != 0;
  const float qscale = f16s ? (float)sqrt(1.0 / (double)head_dim) : 0.f;
  const float c = f16s ? 1.4426950408889634f : 1.4426950408889634f / sqrtf((float)head_dim);
  return at_launch<1, 8>("fp_attention_segments_f16_fwd", qkv, out, B, AtSegments{seg_offsets, max_S}, max_S, H, c, qscale,
                         (hipStream_t)stream);
}
