// NHWC elementwise / reduction kernels of the NF-RegNet image path (timm `nf_regnet_b1`) -- what the NFNet kernels of
// elementwise.hip do not cover.  Its squeeze-excite sits in the MIDDLE of the block, on the mid channels between conv2
// and conv3, and the activation follows it:
//     gate = sigmoid(fc2(relu(fc1(mean_hw c2)))) ;  u = ga * gate * c2 ;  a3 = silu(u) ;  c3 = conv3(a3)
//   * forward: a3 from (c2, gate) in one pass (c2 is stashed raw, u is recomputed wherever it is needed);
//   * backward: one pass over (c2, a3bar) writes the direct share of conv2's output gradient,
//     c2bar = ga * gate * dsilu(u) * a3bar, and reduces the gate gradient ga * sum_hw c2 * dsilu(u) * a3bar (with the
//     sigmoid backward applied: zbar); the pooled path's share, qbar / hw per (image, channel), is added by a second
//     small pass once the two small linears have produced it;
//   * the residual sum x' = alpha*conv3 + shortcut with the next block's pre-activation beta*silu(x').
// S = Dual gives the tangent of each (primal from the stash, tangents written only).
// Every access is a 16-byte chunk of consecutive channels per lane; channel counts are multiples of the chunk only
// (40, 88, 184, 360, 736), so every kernel guards its chunk column instead of assuming a tile of columns.
#include "kernels.h"

namespace {

template <class AT> DEVI void ldc(const AT* p, int64_t ci, float* f) { Chunk<AT>::unpack(((const uint4*)p)[ci], f); }
template <class AT> DEVI void stc(AT* p, int64_t ci, const float* f) { ((uint4*)p)[ci] = Chunk<AT>::pack(f); }
template <class S, class AT> DEVI void ldcS(const AT* pv, const AT* pt, int64_t ci, S* out) {
  constexpr int CE = Chunk<AT>::N;
  float a[CE], b[CE];
  ldc<AT>(pv, ci, a);
  if constexpr (IsDual<S>::v) {
    ldc<AT>(pt, ci, b);
#pragma unroll
    for (int i = 0; i < CE; ++i) out[i] = Dual(a[i], b[i]);
  } else {
#pragma unroll
    for (int i = 0; i < CE; ++i) out[i] = a[i];
  }
}
// Dual: the tangent goes to pt ; float: the value goes to pv
template <class S, class AT> DEVI void stcS(AT* pv, AT* pt, int64_t ci, const S* x) {
  constexpr int CE = Chunk<AT>::N;
  float a[CE];
#pragma unroll
  for (int i = 0; i < CE; ++i) a[i] = IsDual<S>::v ? tan_(x[i]) : val(x[i]);
  stc<AT>(IsDual<S>::v ? pt : pv, ci, a);
}

inline int grid_of(int64_t items, int block = 256) {
  int64_t g = (items + block - 1) / block;
  return (int)(g < 1 ? 1 : (g > 8192 ? 8192 : g));
}

// block = 256 threads = 8 chunk columns x 32 row lanes of ONE image; grid = (column groups, row splits, images).
// The per-(image, channel) operands are loaded once per thread, the row loop is 32-bit arithmetic.
struct ColTile { int ni, col, p0, p1; bool ok; };
DEVI ColTile col_tile(int hw, int cch, int rows_per_block) {
  ColTile t;
  t.ni = blockIdx.z;
  t.col = blockIdx.x * 8 + (threadIdx.x & 7);
  t.ok = t.col < cch;
  const int r0 = blockIdx.y * rows_per_block;
  t.p0 = r0 + (threadIdx.x >> 3);
  t.p1 = min(hw, r0 + rows_per_block);
  return t;
}

// a3 = silu(ga * gate * c2)
template <class S, class AT>
__global__ __launch_bounds__(256) void k_mid_se_apply(AT* __restrict__ a3, AT* __restrict__ a3_t, const AT* __restrict__ c2,
                                                      const AT* __restrict__ c2_t, const float* __restrict__ gate,
                                                      const float* __restrict__ gate_t, float ga, int hw, int c,
                                                      int rows_per_block) {
  constexpr int CE = Chunk<AT>::N;
  const int cch = c / CE;
  const ColTile t = col_tile(hw, cch, rows_per_block);
  if (!t.ok) return;
  S g[CE];
#pragma unroll
  for (int e = 0; e < CE; ++e) g[e] = ldS<S>(gate, gate_t, (size_t)t.ni * c + t.col * CE + e) * ga;
  const int64_t base = (int64_t)t.ni * hw * cch + t.col;
  for (int p = t.p0; p < t.p1; p += 32) {
    const int64_t i = base + (int64_t)p * cch;
    S x[CE], o[CE];
    ldcS<S, AT>(c2, c2_t, i, x);
#pragma unroll
    for (int e = 0; e < CE; ++e) o[e] = silu_(x[e] * g[e]);
    stcS<S, AT>(a3, a3_t, i, o);
  }
}

// c2bar = ga*gate*dsilu(u)*a3bar ; zbar[n,c] = (ga * sum_hw c2*dsilu(u)*a3bar) * gate*(1-gate).  One block per
// (image, 8 chunk columns): the 32 row lanes are reduced through LDS (no atomics, no zero-filled output).
template <class S, class AT>
__global__ __launch_bounds__(256) void k_mid_se_bwd(float* __restrict__ zbar, float* __restrict__ zbar_t,
                                                    AT* __restrict__ c2bar, AT* __restrict__ c2bar_t,
                                                    const AT* __restrict__ c2, const AT* __restrict__ c2_t,
                                                    const AT* __restrict__ a3bar, const AT* __restrict__ a3bar_t,
                                                    const float* __restrict__ gate, const float* __restrict__ gate_t,
                                                    float ga, int hw, int c) {
  constexpr int CE = Chunk<AT>::N;
  const int cch = c / CE;
  const int ni = blockIdx.y;
  const int cs = threadIdx.x & 7, lane = threadIdx.x >> 3;
  const int col = blockIdx.x * 8 + cs;
  S acc[CE];
#pragma unroll
  for (int e = 0; e < CE; ++e) acc[e] = mk<S>(0.f, 0.f);
  if (col < cch) {
    S g[CE];
#pragma unroll
    for (int e = 0; e < CE; ++e) g[e] = ldS<S>(gate, gate_t, (size_t)ni * c + col * CE + e) * ga;
    const int64_t base = (int64_t)ni * hw * cch + col;
    for (int p = lane; p < hw; p += 32) {
      const int64_t i = base + (int64_t)p * cch;
      S x[CE], ab[CE], o[CE];
      ldcS<S, AT>(c2, c2_t, i, x);
      ldcS<S, AT>(a3bar, a3bar_t, i, ab);
#pragma unroll
      for (int e = 0; e < CE; ++e) {
        const S d = dsilu_(x[e] * g[e]) * ab[e];
        o[e] = d * g[e];
        acc[e] = acc[e] + x[e] * d;
      }
      stcS<S, AT>(c2bar, c2bar_t, i, o);
    }
  }
  __shared__ float sh[32][8][CE * 2 + 1];
#pragma unroll
  for (int e = 0; e < CE; ++e) { sh[lane][cs][e] = val(acc[e]); sh[lane][cs][CE + e] = tan_(acc[e]); }
  __syncthreads();
  for (int o = threadIdx.x; o < 8 * CE; o += blockDim.x) {
    const int s_ = o / CE, e = o - s_ * CE;
    const int ccol = blockIdx.x * 8 + s_;
    if (ccol >= cch) continue;
    float sv = 0.f, stn = 0.f;
    for (int l = 0; l < 32; ++l) { sv += sh[l][s_][e]; stn += sh[l][s_][CE + e]; }
    const size_t oi = (size_t)ni * c + (size_t)ccol * CE + e;
    const S gt = ldS<S>(gate, gate_t, oi);
    const S r = mk<S>(sv * ga, stn * ga) * gt * (1.f - gt);
    stS<S>(zbar, zbar_t, oi, r);
  }
}

// x[n, p, c] += v[n, c] * mul   (linear: the tangent pass applies it to the tangent buffers)
template <class AT>
__global__ __launch_bounds__(256) void k_add_pooled(AT* __restrict__ x, const float* __restrict__ v, float mul, int hw, int c,
                                                    int rows_per_block) {
  constexpr int CE = Chunk<AT>::N;
  const int cch = c / CE;
  const ColTile t = col_tile(hw, cch, rows_per_block);
  if (!t.ok) return;
  float a[CE];
#pragma unroll
  for (int e = 0; e < CE; ++e) a[e] = v[(size_t)t.ni * c + t.col * CE + e] * mul;
  const int64_t base = (int64_t)t.ni * hw * cch + t.col;
  for (int p = t.p0; p < t.p1; p += 32) {
    const int64_t i = base + (int64_t)p * cch;
    float f[CE];
    ldc<AT>(x, i, f);
#pragma unroll
    for (int e = 0; e < CE; ++e) f[e] += a[e];
    stc<AT>(x, i, f);
  }
}

// X' = alpha*C3 + SC ; A' = beta*silu(X')      (timm NormFreeBlock: out*alpha + shortcut; beta = next block's
// 1/sqrt(expected var))
template <class S, class AT>
__global__ void k_resid_silu(const AT* __restrict__ c3, const AT* __restrict__ c3_t, const AT* __restrict__ sc,
                             const AT* __restrict__ sc_t, AT* __restrict__ xo, AT* __restrict__ xo_t,
                             AT* __restrict__ ao, AT* __restrict__ ao_t, float alpha, float beta, int64_t chunks) {
  constexpr int CE = Chunk<AT>::N;
  const bool act = ao || ao_t;
  for (int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; i < chunks; i += (int64_t)gridDim.x * blockDim.x) {
    S a[CE], b[CE], o[CE], r[CE];
    ldcS<S, AT>(c3, c3_t, i, a);
    ldcS<S, AT>(sc, sc_t, i, b);
#pragma unroll
    for (int e = 0; e < CE; ++e) {
      o[e] = a[e] * alpha + b[e];
      r[e] = silu_(o[e]) * beta;
    }
    stcS<S, AT>(xo, xo_t, i, o);
    if (act) stcS<S, AT>(ao, ao_t, i, r);
  }
}

// about 128 rows per block (four per thread), the row range split evenly and rounded up to the 32 row lanes
inline dim3 col_grid(int n, int hw, int cch, int* rows_per_block) {
  const int splits = (hw + 127) / 128;
  const int rpb = (((hw + splits - 1) / splits) + 31) & ~31;
  *rows_per_block = rpb;
  return dim3((unsigned)((cch + 7) / 8), (unsigned)((hw + rpb - 1) / rpb), (unsigned)n);
}

}  // namespace

// ====================================================================== launchers
template <class AT>
void launch_mid_se_apply(AT* a3, AT* a3_t, const AT* c2, const AT* c2_t, const float* gate, const float* gate_t, float ga,
                         int n, int hw, int c, hipStream_t st) {
  int rpb;
  const dim3 grid = col_grid(n, hw, c / Chunk<AT>::N, &rpb);
  if (c2_t) k_mid_se_apply<Dual, AT><<<grid, 256, 0, st>>>(a3, a3_t, c2, c2_t, gate, gate_t, ga, hw, c, rpb);
  else k_mid_se_apply<float, AT><<<grid, 256, 0, st>>>(a3, nullptr, c2, nullptr, gate, nullptr, ga, hw, c, rpb);
}
template <class AT>
void launch_mid_se_bwd(float* zbar, float* zbar_t, AT* c2bar, AT* c2bar_t, const AT* c2, const AT* c2_t, const AT* a3bar,
                       const AT* a3bar_t, const float* gate, const float* gate_t, float ga, int n, int hw, int c,
                       hipStream_t st) {
  const dim3 grid((unsigned)((c / Chunk<AT>::N + 7) / 8), (unsigned)n);
  if (c2_t)
    k_mid_se_bwd<Dual, AT><<<grid, 256, 0, st>>>(zbar, zbar_t, c2bar, c2bar_t, c2, c2_t, a3bar, a3bar_t, gate, gate_t, ga,
                                                 hw, c);
  else
    k_mid_se_bwd<float, AT><<<grid, 256, 0, st>>>(zbar, nullptr, c2bar, nullptr, c2, nullptr, a3bar, nullptr, gate,
                                                  nullptr, ga, hw, c);
}
template <class AT>
void launch_add_pooled(AT* x, const float* v, float mul, int n, int hw, int c, hipStream_t st) {
  int rpb;
  const dim3 grid = col_grid(n, hw, c / Chunk<AT>::N, &rpb);
  k_add_pooled<AT><<<grid, 256, 0, st>>>(x, v, mul, hw, c, rpb);
}
template <class AT>
void launch_resid_silu(const AT* c3, const AT* c3_t, const AT* sc, const AT* sc_t, AT* xo, AT* xo_t, AT* ao, AT* ao_t,
                       float alpha, float beta, int64_t elems, hipStream_t st) {
  const int64_t chunks = elems / Chunk<AT>::N;
  if (c3_t)
    k_resid_silu<Dual, AT><<<grid_of(chunks), 256, 0, st>>>(c3, c3_t, sc, sc_t, xo, xo_t, ao, ao_t, alpha, beta, chunks);
  else
    k_resid_silu<float, AT><<<grid_of(chunks), 256, 0, st>>>(c3, nullptr, sc, nullptr, xo, nullptr, ao, nullptr, alpha,
                                                             beta, chunks);
}
#define INST(AT)                                                                                                      \
  template void launch_mid_se_apply<AT>(AT*, AT*, const AT*, const AT*, const float*, const float*, float, int, int,  \
                                        int, hipStream_t);                                                            \
  template void launch_mid_se_bwd<AT>(float*, float*, AT*, AT*, const AT*, const AT*, const AT*, const AT*,           \
                                      const float*, const float*, float, int, int, int, hipStream_t);                 \
  template void launch_add_pooled<AT>(AT*, const float*, float, int, int, int, hipStream_t);                          \
  template void launch_resid_silu<AT>(const AT*, const AT*, const AT*, const AT*, AT*, AT*, AT*, AT*, float, float,   \
                                      int64_t, hipStream_t);
INST(float)
INST(bf16)
