// The squeeze-excite-apply epilogues of conv3 (EPI_FWD_SE, EPI_FWD_SE_T), included TEXTUALLY into the SEK instances of
// k_conv_gemm: the 128 x 128 pointwise kernel with nothing but these two bodies (the IBK / GELU precedent: the other
// instances keep their text and with it their register allocation).  Names expected in scope: as conv_gemm_epilogue.inc,
// with MODE == 0.  What the separate elementwise kernel (k_se_apply_tiled) did after conv3 had written C3,
//     X' = C3 * (gate * ga) + SC ;  A' = beta * silu(X')         (and the same rule in Dual for the tangent pass),
// happens here on the accumulator tile: C3 is still stored (the backward gate gradient sums xbar * C3) and the value that
// enters the rule is C3 AS STORED (packed to the storage type and unpacked again), in the tiled kernel's expression order
// and with its multiply-adds (se_apply_primal / se_apply_tangent), so X' and A' keep the values they had.  The gate is a
// per-image vector: image = m / hw by the estimate-and-correct step of the per-image bias (ConvEpi::ib).
  static_assert(MODE == 0, "squeeze-excite epilogues: pointwise instances only");
  constexpr int WCOLS = TN * 32, PITCH = WCOLS + 4;
  constexpr int WROWS = TM * 32;
  constexpr int LPR = WCOLS / CE;      // lanes per output row
  constexpr int RPP = 64 / LPR;        // rows per pass
  constexpr int NP = 32 / RPP;
  float* stage = (float*)smem + wave * (32 * PITCH);   // one 32-row MFMA block at a time
  const ConvEpi& E = p.ep;
  AT* out_raw = (AT*)E.out_raw;
  AT* out_x = (AT*)E.out_x;
  AT* out_act = (AT*)E.out_act;
  const AT* Cst = (const AT*)E.c;
  const AT* Sc = (const AT*)E.add1;
  const AT* Sct = (const AT*)E.add2;
  const int lrow = lane / LPR, lcol = (lane % LPR) * CE;
  const int n = n0 + wn * WCOLS + lcol;
  const bool ncol_ok = n < G.nc;
  const int ch = grp * G.nc + n;
  float bias[CE];
#pragma unroll
  for (int e = 0; e < CE; ++e) bias[e] = 0.f;
  const float* bp = E.mode == EPI_FWD_SE ? E.bias : E.bias_t;
  if (bp && ncol_ok) {
#pragma unroll
    for (int e = 0; e < CE; e += 4) {
      float4 b4 = *(const float4*)(bp + ch + e);
      bias[e] = b4.x; bias[e + 1] = b4.y; bias[e + 2] = b4.z; bias[e + 3] = b4.w;
    }
  }
  const float beta = E.beta, ga = E.ib_mul;
  const float hw_inv = 1.f / (float)E.ib_hw;
  const bool do_act = out_act != nullptr;
  auto run = [&](auto TANc, auto FTc) __attribute__((always_inline)) {
    constexpr bool TAN = decltype(TANc)::value;
    constexpr bool FULLT = decltype(FTc)::value;   // every row of the block tile is a real output row
    // row passes whose global loads are in flight together (tangent: three 16-byte operands and two gate vectors per pass)
    constexpr int U0 = NP < MDD_EPI_UNROLL ? NP : MDD_EPI_UNROLL;
    constexpr int UU = (TAN && U0 > 2) ? U0 / 2 : U0;
#pragma unroll
    for (int hi = 0; hi < TM; ++hi) {
      // this wave's 32-row block hi of the accumulators -> its private LDS stage (aliases the K-loop
      // buffers: the loop's final barrier has retired every read of them)
      if (hi) { if constexpr (EPI_WAVE_SYNC) epi_wave_sync(); else __syncthreads(); }
#pragma unroll
      for (int j = 0; j < TN; ++j)
#pragma unroll
        for (int r = 0; r < 16; ++r)
          stage[((r & 3) + 8 * (r >> 2) + 4 * lh) * PITCH + j * 32 + l31] = acc[hi][j][r];
      if constexpr (EPI_WAVE_SYNC) epi_wave_sync(); else __syncthreads();
      if (!ncol_ok) continue;
#pragma unroll 1
      for (int ps0 = 0; ps0 < NP; ps0 += UU) {
        int idx[UU];
        bool ok[UU];
        uint4 q_c[TAN ? UU : 1], q_s[UU], q_st[TAN ? UU : 1];
        float4 q_g[UU][CE / 4], q_gt[TAN ? UU : 1][CE / 4];
#pragma unroll
        for (int u = 0; u < UU; ++u) {
          const int row = (ps0 + u) * RPP + lrow;
          const int m = m0 + wm * WROWS + hi * 32 + row;
          ok[u] = FULLT || m < e_M;
          idx[u] = m * G.co_tot + ch;          // < 2^31 elements for every tensor of the path
          if (ok[u]) {
            int img = (int)((float)m * hw_inv);              // estimate, then exact by one correction step
            const int rem = m - img * E.ib_hw;
            img += rem >= E.ib_hw ? 1 : (rem < 0 ? -1 : 0);
            const size_t gi = (size_t)img * G.co_tot + ch;
#pragma unroll
            for (int e = 0; e < CE / 4; ++e) q_g[u][e] = *(const float4*)(E.ib + gi + 4 * e);
            q_s[u] = *(const uint4*)(Sc + idx[u]);
            if constexpr (TAN) {
#pragma unroll
              for (int e = 0; e < CE / 4; ++e) q_gt[u][e] = *(const float4*)(E.ib_t + gi + 4 * e);
              q_c[u] = *(const uint4*)(Cst + idx[u]);
              q_st[u] = *(const uint4*)(Sct + idx[u]);
            }
          }
        }
#pragma unroll
        for (int u = 0; u < UU; ++u) {
          if (!ok[u]) continue;
          const int row = (ps0 + u) * RPP + lrow;
          float v[CE], s[CE], gv[CE], xo[CE], ao[CE];
#pragma unroll
          for (int e = 0; e < CE; e += 4) {
            float4 s4 = *(const float4*)(stage + row * PITCH + lcol + e);
            v[e] = s4.x + bias[e]; v[e + 1] = s4.y + bias[e + 1];
            v[e + 2] = s4.z + bias[e + 2]; v[e + 3] = s4.w + bias[e + 3];
          }
          const uint4 craw = Chunk<AT>::pack(v);
          *(uint4*)(out_raw + idx[u]) = craw;
          Chunk<AT>::unpack(craw, v);           // C3 (tangent pass: its tangent) as the stash holds it
          Chunk<AT>::unpack(q_s[u], s);
#pragma unroll
          for (int e = 0; e < CE / 4; ++e) {
            gv[4 * e] = q_g[u][e].x; gv[4 * e + 1] = q_g[u][e].y; gv[4 * e + 2] = q_g[u][e].z; gv[4 * e + 3] = q_g[u][e].w;
          }
          if constexpr (!TAN) {
#pragma unroll
            for (int e = 0; e < CE; ++e) se_apply_primal(v[e], gv[e] * ga, s[e], beta, xo[e], ao[e]);
          } else {
            float c0[CE], st[CE], gt[CE];
            Chunk<AT>::unpack(q_c[u], c0);
            Chunk<AT>::unpack(q_st[u], st);
#pragma unroll
            for (int e = 0; e < CE / 4; ++e) {
              gt[4 * e] = q_gt[u][e].x; gt[4 * e + 1] = q_gt[u][e].y; gt[4 * e + 2] = q_gt[u][e].z; gt[4 * e + 3] = q_gt[u][e].w;
            }
#pragma unroll
            for (int e = 0; e < CE; ++e)
              se_apply_tangent(c0[e], v[e], gv[e] * ga, gt[e] * ga, s[e], st[e], beta, xo[e], ao[e]);
          }
          *(uint4*)(out_x + idx[u]) = Chunk<AT>::pack(xo);
          if (do_act) *(uint4*)(out_act + idx[u]) = Chunk<AT>::pack(ao);
        }
      }
    }
  };
  const bool full_tile = m0 + BM <= e_M;
  if (E.mode == EPI_FWD_SE) {
    if (full_tile) run(std::false_type{}, std::true_type{}); else run(std::false_type{}, std::false_type{});
  } else {
    if (full_tile) run(std::true_type{}, std::true_type{}); else run(std::true_type{}, std::false_type{});
  }
