// The body of a k_conv_sw tile: included by conv_sw.hip inside each of its two kernels, k_conv_sw<BM, BN, TM, S16> (DIRECT = false) and
// k_conv_sw_direct (DIRECT = true), which define BM, BN, TM, S16 and DIRECT around it and take `IgemmParams p`.  One text for the main loop of
// both; as a device function behind two entries the compiler schedules the prologue of k_conv_sw differently than before.
  static_assert(!DIRECT || (S16 && BM == 512 && BN == 128 && TM == 4), "the direct epilogue is the 512 x 128 tile's, on 16x16x32 MFMAs");
  constexpr int BK = SW_BK, NW = 8, THREADS = 512;
  constexpr int NWN = BN / 64;
  static_assert((BM / (32 * TM)) * NWN == NW, "8 waves");
  constexpr int ROWB = BK * 2;                      // 64-byte LDS rows
  constexpr int W_BYTES = BN * ROWB;
  constexpr int SW_PROWS = sw_prows(BM);
  constexpr int SW_PATCH_BYTES = SW_PROWS * ROWB;
  constexpr int WI = BN / 16 / NW;                  // weight LDS-DMA instructions per wave and k-step (16 rows each)
  constexpr int PI = SW_PROWS / 16 / NW;            // patch instructions per wave and chunk: one at each of taps 0..PI-1
  static_assert(WI >= 1 && PI >= 1 && PI <= 7 && SW_PROWS == PI * 16 * NW, "tile shape");
  constexpr int STAGES_BYTES = 2 * SW_PATCH_BYTES + SW_NSTW * W_BYTES;
  constexpr int LDS_MAIN = ig_lds_main_slim<BM, BN>(STAGES_BYTES);
  auto swz = [](int row) { return (row >> 2) & 3; };                    // weight rows, and patch rows of the 32x32x16 loop
  auto swzp = [](int row) { return S16 ? (row >> 1) & 2 : (row >> 2) & 3; };   // patch rows
  extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
  SW_CLK(t_start);
  unsigned char* const patch = smem;                              // 2 x SW_PATCH_BYTES
  unsigned char* const wring = smem + 2 * SW_PATCH_BYTES;         // SW_NSTW x W_BYTES
  const int tid = threadIdx.x, lane = tid & 63;
  const int wid = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int grp = wid >> 2;
  const int wm = wid / NWN, wn = wid - wm * NWN;
  float* bias_lds = reinterpret_cast<float*>(smem + LDS_MAIN);

  // ---- Tile boundaries (round 10): the first operands leave as early as the wave can send them.  Everything in front of the first patch
  // and weight DMA reads the HEAD of IgemmParams (igemm_common.h), fetched here in one go -- adjacent kernel-argument dwords become wide
  // scalar loads behind ONE wait -- and pinned to scalar registers, so that no field is loaded (and waited for) where it is first used.
  const _Float16* A_ = p.A;
  const _Float16* W_ = p.Wt;
  const _Float16* Wpk_ = p.Wpk;
  const float* bias_ = p.bias;
  const float* bnsc_ = p.bn_scale;
  const float* bnsh_ = p.bn_shift;
  const int M = p.M, N = p.N, Cin = p.Cin, cstride = p.in.cstride, coff = p.in.coff;
  const SwGeom gi = {p.in.HoWo, p.in.Wo, p.in.Hp, p.in.Wp, p.in.mulP, p.in.shrP, p.in.mulW, p.in.shrW};
  // (inputs of an empty asm: the values exist here, in whatever registers they were loaded to -- tied outputs cost a move each)
  asm volatile("" ::"s"(A_), "s"(W_), "s"(Wpk_), "s"(bias_), "s"(bnsc_), "s"(bnsh_), "s"(M), "s"(N), "s"(Cin), "s"(cstride), "s"(coff),
               "s"(gi.HoWo), "s"(gi.Wo), "s"(gi.Hp), "s"(gi.Wp), "s"(gi.mulP), "s"(gi.shrP), "s"(gi.mulW), "s"(gi.shrW));
  __builtin_amdgcn_sched_barrier(0);               // nothing that needs a part of the head is scheduled in front of the loads of the rest

  // XCD-aware tile order (ig_xcd_tile): neighbouring pixel tiles (overlapping halos) and the channel tiles of one pixel
  // tile run on the same XCD
  const int tiles_n = N / BN;
  const int nwg = (int)(((unsigned)M + BM - 1) / BM) * tiles_n;   // == gridDim.x (ig_launch_tiles), without the round trip for a hidden argument
  const int tile = ig_xcd_tile(blockIdx.x, nwg);
  // (the emulated scalar division is ~35 instructions in front of the first DMA; every layer of the two networks has 1, 2 or 4 channel tiles)
  const int bm = __builtin_popcount(tiles_n) == 1 ? tile >> __builtin_ctz(tiles_n) : tile / tiles_n, bn = tile - bm * tiles_n;
  const int m0 = bm * BM, n0 = bn * BN;
  const int Ktot = 9 * Cin, Wp = gi.Wp;
  const int ncc = Cin / BK;
  ig_bias_to_lds(bias_, bnsc_, bnsh_, N, n0, bias_lds, wid, lane);

  // ---- DMA sources.  Patch row R <-> padded pixel q0 + R (clamped into the tensor: clamped rows are never read by a
  // row that is stored).  Wave w owns patch instructions 4w..4w+3 (16 rows each).
  const int q0 = sw_q(gi, m0);
  const int qmax = sw_div(M, gi.mulP, gi.shrP) * gi.Hp * Wp - 1;   // M / HoWo images
  unsigned poff32[PI], woff32[WI];
  {
    // byte offset of pixel min(q0 + row, qmax), channel chunk c: (q * cstride + coff + c * 8) * 2.  The product with the positive pixel
    // stride is monotonic, so the clamp is applied to the product: ONE vector multiplication for the wave's first piece, and an add and a
    // min per piece (pieces are 16 pixels apart, and the swizzle term of a row depends on row % 16 only).  Unsigned: the tensor ends below
    // 2^31 bytes and the unclamped rows of a patch lie less than 2^31 bytes behind it (fp_conv3x3_sw_applicable)
    const int row0 = wid * PI * 16 + (lane >> 2);
    const int c = (lane & 3) ^ swzp(row0);
    static_assert(((16 >> 1) & 2) == 0 && ((16 >> 2) & 3) == 0, "swzp(row0 + 16 j) == swzp(row0)");
    const unsigned ps2 = (unsigned)cstride * 2, omax = (unsigned)qmax * ps2, lane_off = (unsigned)(coff + c * 8) * 2;
    const unsigned o0 = (unsigned)(q0 + row0) * ps2;
#pragma unroll
    for (int j = 0; j < PI; ++j) {
      const unsigned o = o0 + j * 16 * ps2;
      poff32[j] = (o < omax ? o : omax) + lane_off;
    }
  }
#pragma unroll
  for (int j = 0; j < WI; ++j) {
    const int row = (wid * WI + j) * 16 + (lane >> 2);
    const int c = (lane & 3) ^ swz(row);
    const int src = DIRECT ? sw_direct_row(row) : row;              // DIRECT: LDS row `row` holds another channel's weights, the chunks where they were
    woff32[j] = (unsigned)((((size_t)(n0 + src) * Ktot) + c * 8) * 2);
  }
  // Tile-packed weights (round 5, fp_pack_conv3x3_tiles_f16; DIRECT: fp_pack_conv3x3_tiles_direct_f16, whose rows are permuted; BN = 128 only): the 8 KiB a k-step stages are one contiguous run that
  // already is the LDS image, so a piece is 1 KiB of consecutive addresses (8 whole 128-byte lines) instead of 16 half lines of 16 weight rows
  const bool wpk = (BN == 128) && Wpk_ != nullptr;
  if (wpk) {
#pragma unroll
    for (int j = 0; j < WI; ++j) woff32[j] = (unsigned)(((wid * WI + j) * 64 + lane) * 16);
  }
  const int wpk_base = wpk ? bn * (ncc * 9) * W_BYTES : 0;
  const __amdgpu_buffer_rsrc_t rsA = __builtin_amdgcn_make_buffer_rsrc(const_cast<_Float16*>(A_), 0, 0x7FFFFFFF, 0x00020000);
  const __amdgpu_buffer_rsrc_t rsW = __builtin_amdgcn_make_buffer_rsrc(const_cast<_Float16*>(wpk ? Wpk_ : W_), 0, 0x7FFFFFFF, 0x00020000);

  auto stage_patch = [&](int cc, int j) {          // piece j (0..3) of this wave of the patch of chunk cc
    unsigned char* dst = patch + (cc & 1) * SW_PATCH_BYTES + (wid * PI + j) * 1024;
    __builtin_amdgcn_raw_ptr_buffer_load_lds(rsA, (__attribute__((address_space(3))) void*)dst, 16, (int)poff32[j],
                                             cc * (BK * 2), 0, 0);
  };
  auto stage_w = [&](int cc, int tap, int slot) {  // weight columns [tap*Cin + cc*32, +32) of the tile's BN rows
    const int wsoff = wpk ? wpk_base + (cc * 9 + tap) * W_BYTES : (tap * Cin + cc * BK) * 2;
    unsigned char* dst = wring + slot * W_BYTES + wid * (WI * 1024);
#pragma unroll
    for (int j = 0; j < WI; ++j)
      __builtin_amdgcn_raw_ptr_buffer_load_lds(rsW, (__attribute__((address_space(3))) void*)(dst + j * 1024), 16,
                                               (int)woff32[j], wsoff, 0, 0);
  };

  // ---- prologue, first half: patch(0) + W of k-steps 0..2 requested.  Per wave the vector-memory operations keep their order and number
  // (bias oldest, the patch pieces, the three weight stages): the counted vmcnt waits of the k-steps rely on it.  What the first fragment
  // read needs and the DMAs do not -- accumulators, fragment rows, weight offsets -- is computed behind them, under their latency.
#pragma unroll
  for (int j = 0; j < PI; ++j) stage_patch(0, j);
  stage_w(0, 0, 0);
  stage_w(0, 1, 1);
  stage_w(0, 2, 2);
  __builtin_amdgcn_sched_barrier(0);
  SW_CLK(t_issue);

  // accumulators: 2 x TM tiles of 32 ch x 32 px (16 floats per lane), or 4 x 2 TM tiles of 16 x 16 (4 floats per lane)
  constexpr int NFA = S16 ? 2 * TM : TM, NFW = S16 ? 4 : 2;       // pixel / weight fragment rows of a wave (x 2 k halves for 32x32x16)
  constexpr int FR = S16 ? 16 : 32;                               // rows of a fragment
  typedef float float4_ __attribute__((ext_vector_type(4)));
  typedef typename std::conditional<S16, float4_, float16_>::type acc_t;
  acc_t acc[NFW][NFA];
#pragma unroll
  for (int i = 0; i < NFW; ++i)
#pragma unroll
    for (int j = 0; j < NFA; ++j)
#pragma unroll
      for (int e = 0; e < (S16 ? 4 : 16); ++e) acc[i][j][e] = 0.f;

  // fragment addressing: the lane's pixel rows (position in the patch at tap (0,0)) and its weight rows
  const int frow = lane & (FR - 1), fhalf = lane >> (S16 ? 4 : 5);     // fhalf: the lane's 16-byte chunk (S16) / chunk within a k half
  int arow[NFA], w_off[2][2];                                      // S16: w_off[t >> 1][t & 1] is weight fragment t
#pragma unroll
  for (int t = 0; t < NFA; ++t) {
    int m = m0 + wm * (32 * TM) + t * FR + frow;
    m = m < M ? m : M - 1;
    arow[t] = sw_q(gi, m) - q0;
    if constexpr (S16) arow[t] = (arow[t] << 6) + (fhalf << 4);    // as a byte address: a tap adds shift << 6, the swizzle flips bit 5
  }
  if constexpr (S16) {
    const int quad = (0x1320 >> (4 * (frow >> 2))) & 3;            // sigma
#pragma unroll
    for (int t = 0; t < 4; ++t) {
      const int rw = wn * 64 + t * 16 + 4 * quad + (frow & 3);
      w_off[t >> 1][t & 1] = rw * ROWB + ((fhalf ^ swz(rw)) << 4);
    }
  } else {
#pragma unroll
    for (int t = 0; t < 2; ++t) {
      const int rw = wn * 64 + t * 32 + frow;
#pragma unroll
      for (int kk = 0; kk < 2; ++kk) w_off[t][kk] = rw * ROWB + (((2 * kk + fhalf) ^ swz(rw)) << 4);
    }
  }
  static_assert(TM == 4, "the fragment addresses of the next tap are computed behind the MFMA groups of a k-step, one per group of four");
  int anext[NFA], aflip[NFA];                      // fragment addresses of the next k-step's tap, inside a patch buffer (S16: ^ aflip, the swizzle bit)
#pragma unroll
  for (int t = 0; t < NFA; ++t) {                  // tap (0,0) of the first k-step
    anext[t] = S16 ? arow[t] : (arow[t] << 6) + ((fhalf ^ swz(arow[t])) << 4);
    aflip[t] = S16 ? (arow[t] >> 3) & 32 : 0;
  }

  // ... and computed HERE: an empty asm per value keeps the compiler from sinking the computation behind the wait, where nothing covers it
#pragma unroll
  for (int t = 0; t < NFA; ++t) {
    asm volatile("" : "+v"(arow[t]), "+v"(anext[t]));
    if constexpr (S16) asm volatile("" : "+v"(aflip[t]));
  }
  asm volatile("" : "+v"(w_off[0][0]), "+v"(w_off[0][1]), "+v"(w_off[1][0]), "+v"(w_off[1][1]));
#pragma unroll
  for (int i = 0; i < NFW; ++i)
#pragma unroll
    for (int j = 0; j < NFA; ++j) asm volatile("" : "+v"(acc[i][j]));
  if constexpr (DIRECT) {
    // the output row table, one thread per row, in the 2 KiB behind the operand stages: under the latency of the first DMAs, and visible
    // long before the epilogue reads it (every k-step waits for its LDS operations in front of a barrier).  Element offsets from the
    // buffer's start, channel n0 included (below 2^31: fp_conv3x3_sw_applicable); IG_ROW_NONE for a row past M
    static_assert(THREADS == BM && STAGES_BYTES + BM * 4 <= LDS_MAIN, "one thread per row; the table lies behind the stages");
    const int m = m0 + tid;
    reinterpret_cast<int*>(smem + STAGES_BYTES)[tid] = m < M ? (int)(ig_row_off(p.out, m) + n0) : IG_ROW_NONE;
  }
  __builtin_amdgcn_sched_barrier(0);

  // ---- prologue, second half: patch(0) and W(0) landed and visible (W of k-steps 1 and 2 in flight)
  sw_wait_vm<2 * WI>();
  __builtin_amdgcn_s_barrier();
  SW_CLK(t_cold);
  if (grp) __builtin_amdgcn_s_barrier();           // group 1 sits out interval 0

  half8 fa[2][TM], fw[2][2];                       // S16: fa[t >> 2][t & 3] is pixel fragment t, fw[t >> 1][t & 1] weight fragment t
  // one k-step = (chunk cc, tap T).  LAST: cc is the last chunk (no next patch; the weight prefetch runs dry).
  // vmcnt bookkeeping (loads retire in order): this wave's pieces of W(s+1) must have landed when it leaves the memory
  // cluster; younger and allowed in flight are W(s+2), W(s+3) and the patch pieces issued in this and the previous step.
  auto kstep = [&](int cc, auto tap_c, auto last_c) {
    constexpr int T = decltype(tap_c)::value;
    constexpr bool LAST = decltype(last_c)::value;
    constexpr int ky = T / 3, kx = T - 3 * ky;
    const int s = cc * 9 + T;
    const unsigned char* pb = patch + (cc & 1) * SW_PATCH_BYTES;
    const unsigned char* wb = wring + (s & (SW_NSTW - 1)) * W_BYTES;
    const int shift = ky * Wp + kx;
    // ---- memory cluster.  Round 6: the tap's four fragment addresses (8 vector instructions each) are NOT computed here any more but
    // behind the MFMAs of the previous k-step (anext, below): the stand-alone probe of this loop (scripts/conv_loop_probe,
    // profiles/r06_i_conv_loop_probe.log) put the memory cluster at ~610 clk against the partner group's 512 clk of MFMAs, and without
    // the 32 address instructions at ~535 (matrix-pipe occupancy 0.84 -> 0.96); in the MFMA shadow they are free (<= 5 per MFMA hide)
    if constexpr (S16) {
#pragma unroll
      for (int t = 0; t < NFA; ++t) fa[t >> 2][t & 3] = *reinterpret_cast<const half8*>(pb + (anext[t] ^ aflip[t]));
#pragma unroll
      for (int t = 0; t < 4; ++t) fw[t >> 1][t & 1] = *reinterpret_cast<const half8*>(wb + w_off[t >> 1][t & 1]);
    } else {
#pragma unroll
      for (int t = 0; t < TM; ++t) {
        const int a0 = anext[t];
        fa[0][t] = *reinterpret_cast<const half8*>(pb + a0);
        fa[1][t] = *reinterpret_cast<const half8*>(pb + (a0 ^ 32));
      }
#pragma unroll
      for (int kk = 0; kk < 2; ++kk)
#pragma unroll
        for (int t = 0; t < 2; ++t) fw[kk][t] = *reinterpret_cast<const half8*>(wb + w_off[t][kk]);
    }
    (void)shift;
    if constexpr (!LAST) {
      if constexpr (T < PI) stage_patch(cc + 1, T);
      // k-step s+3 = (cc, T+3) or (cc+1, T-6)
      if constexpr (T + 3 < 9) stage_w(cc, T + 3, (s + 3) & (SW_NSTW - 1));
      else stage_w(cc + 1, T - 6, (s + 3) & (SW_NSTW - 1));
      // patch pieces are issued at taps 0..PI-1: in flight from this step and the previous one
      constexpr int NP = (T < PI ? 1 : 0) + ((T >= 1 && T - 1 < PI) ? 1 : 0);
      sw_wait_vm<2 * WI + NP>();
    } else {
      if constexpr (T + 3 < 9) stage_w(cc, T + 3, (s + 3) & (SW_NSTW - 1));
      // at T == 0 the previous step (tap 8 of the chunk before) issued no patch piece, and the last chunk issues none
      constexpr int NYOUNGER = T <= 5 ? 2 : (T == 6 ? 1 : 0);
      sw_wait_vm<NYOUNGER * WI>();
    }
    asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");   // fragment reads retired before the buffers can be refilled
    __builtin_amdgcn_sched_barrier(0);
    __builtin_amdgcn_s_barrier();
    __builtin_amdgcn_sched_barrier(0);
    // ---- compute cluster
    __builtin_amdgcn_s_setprio(1);
    {
      // the NEXT k-step's tap: (T + 1) % 9 -- the patch buffer (chunk parity) is added where the address is used
      constexpr int TN = (T + 1) % 9, kyn = TN / 3, kxn = TN - 3 * kyn;
      const int shift_n = kyn * Wp + kxn;
      if constexpr (S16) {
        int sh = shift_n << 6;
        asm volatile("" : "+s"(sh));               // keep the per-tap recomputation: 72 hoisted tap addresses would spill
#pragma unroll
        for (int i = 0; i < 4; ++i)
#pragma unroll
          for (int jh = 0; jh < 2; ++jh) {
            // one pixel fragment's address with each group of four MFMAs (8 fragments = the eight (i, jh) groups), one of its three
            // instructions behind each of the first three: a 16x16x32 MFMA leaves the vector issue port free for half of its cycles, which
            // takes one instruction and not three
            const int t = i * 2 + jh;
            int x, y;
            sw_mfma16x<DIRECT>(acc[i][jh * 4 + 0], fw[i >> 1][i & 1], fa[jh][0]);
            asm volatile("v_add_u32 %0, %1, %2" : "=v"(x) : "s"(sh), "v"(arow[t]));
            sw_mfma16x<DIRECT>(acc[i][jh * 4 + 1], fw[i >> 1][i & 1], fa[jh][1]);
            asm volatile("v_lshrrev_b32 %0, 3, %1" : "=v"(y) : "v"(x));
            sw_mfma16x<DIRECT>(acc[i][jh * 4 + 2], fw[i >> 1][i & 1], fa[jh][2]);
            asm volatile("v_and_b32 %0, 32, %0" : "+v"(y));
            sw_mfma16x<DIRECT>(acc[i][jh * 4 + 3], fw[i >> 1][i & 1], fa[jh][3]);
            anext[t] = x; aflip[t] = y;            // x ^ y where the address is used
          }
      } else {
#pragma unroll
      for (int kk = 0; kk < 2; ++kk)
#pragma unroll
        for (int i = 0; i < 2; ++i) {
#pragma unroll
          for (int j = 0; j < TM; ++j)
            acc[i][j] = __builtin_amdgcn_mfma_f32_32x32x16_f16(fw[kk][i], fa[kk][j], acc[i][j], 0, 0, 0);
          // one row tile's address behind each group of four MFMAs (TM == 4 row tiles = the four (kk, i) groups)
          const int t = kk * 2 + i;                // a constant after unrolling
          {
            int ar = arow[t];
            asm volatile("" : "+v"(ar));           // keep the per-tap recomputation: 36 hoisted tap addresses would spill
            const int pr = ar + shift_n;
            anext[t] = (pr << 6) + ((fhalf ^ swz(pr)) << 4);
          }
        }
      }
    }
    __builtin_amdgcn_s_setprio(0);
    __builtin_amdgcn_sched_barrier(0);
    __builtin_amdgcn_s_barrier();
    __builtin_amdgcn_sched_barrier(0);
  };
  auto chunk = [&](int cc, auto last_c) {
    kstep(cc, std::integral_constant<int, 0>{}, last_c);
    kstep(cc, std::integral_constant<int, 1>{}, last_c);
    kstep(cc, std::integral_constant<int, 2>{}, last_c);
    kstep(cc, std::integral_constant<int, 3>{}, last_c);
    kstep(cc, std::integral_constant<int, 4>{}, last_c);
    kstep(cc, std::integral_constant<int, 5>{}, last_c);
    kstep(cc, std::integral_constant<int, 6>{}, last_c);
    kstep(cc, std::integral_constant<int, 7>{}, last_c);
    kstep(cc, std::integral_constant<int, 8>{}, last_c);
  };
  for (int cc = 0; cc + 1 < ncc; ++cc) chunk(cc, std::false_type{});
  chunk(ncc - 1, std::true_type{});
  if (!grp) __builtin_amdgcn_s_barrier();          // group 0 waits out group 1's last compute cluster
  __syncthreads();
  SW_CLK(t_loop);
  if constexpr (DIRECT) {
    // p.epi is one of the four layer kinds without the positional output (sw_direct below): a scalar branch
    const IgEpiArgs q = ig_epi_args(p);
    const int* rowY32 = reinterpret_cast<const int*>(smem + STAGES_BYTES);
#define SW_DIRECT_CASE(E)                                                                                     \
    case E:                                                                                                   \
      if (m0 + BM <= M) ig_epilogue_direct<E, true>(q, acc, smem, rowY32, m0, n0, M, wm, wn, tid, lane, bias_lds);  \
      else ig_epilogue_direct<E, false>(q, acc, smem, rowY32, m0, n0, M, wm, wn, tid, lane, bias_lds);         \
      break
    switch (p.epi) {
      SW_DIRECT_CASE(IG_EPI_CONV);
      SW_DIRECT_CASE(IG_EPI_CONV | IG_EPI_RES);
      SW_DIRECT_CASE(IG_EPI_CONV | IG_EPI_BN);
      SW_DIRECT_CASE(IG_EPI_CONV | IG_EPI_BN | IG_EPI_RES);
      default: break;
    }
#undef SW_DIRECT_CASE
  } else {
    ig_epilogue<BM, BN, TM, THREADS, 0, true>(p, acc, smem, m0, n0, wm, wn, tid, lane, bias_lds);
  }
#ifdef FP_PROFILE_BUILD
  asm volatile("s_waitcnt vmcnt(0)" ::: "memory");   // stores drained: the workgroup's resources are free from here
  SW_CLK(t_end);
  if (tid == 0) {
    atomicAdd(&sw_dbg[0], t_cold - t_start); atomicAdd(&sw_dbg[1], t_loop - t_cold); atomicAdd(&sw_dbg[2], t_end - t_loop);
    atomicAdd(&sw_dbg[3], 1ull); atomicAdd(&sw_dbg[4], t_issue - t_start); atomicMin(&sw_dbg[6], t_start); atomicMax(&sw_dbg[7], t_end);
    if constexpr (DIRECT) { atomicAdd(&sw_dbg[8], t_end - t_loop); atomicAdd(&sw_dbg[9], 1ull); }
  }
#endif
