// NHWC elementwise kernels of the NF-ResNet image path (timm `nf_resnet50`: ReLU, 7x7 stem + 3x3 max pool, residual
// blocks without squeeze-excite) -- what the NFNet kernels of elementwise.hip do not cover:
//   * MaxPool2d(3, stride 2, padding 1) after the stem: forward with a one-byte window index per element, its
//     tangent (a gather at the stored index), and its backward in gather form (no atomics), which is also the
//     tangent of the backward (the index is fixed: no second-order term);
//   * the residual sum x' = alpha*conv3 + shortcut with the next block's pre-activation beta*relu(x') (and tangent);
//   * a scaled copy (the gradient w.r.t. conv3's output, alpha * the gradient of the block output).
// Every access is a 16-byte chunk of consecutive channels per lane, except the tangent gather (one element per tap).
#include "kernels.h"

namespace {

template <class AT> DEVI void ldc(const AT* p, int64_t ci, float* f) { Chunk<AT>::unpack(((const uint4*)p)[ci], f); }
template <class AT> DEVI void stc(AT* p, int64_t ci, const float* f) { ((uint4*)p)[ci] = Chunk<AT>::pack(f); }

inline int grid_of(int64_t items, int block = 256) {
  int64_t g = (items + block - 1) / block;
  return (int)(g < 1 ? 1 : (g > 8192 ? 8192 : g));
}

// ------------------------------------------------------------------ max pool 3x3 / stride 2 / pad 1
// One block per (image, output row); threads walk the row's (ox, chunk column) pairs.  Window taps are visited in
// row-major order and a tap replaces the running maximum when `v > max` (or v is NaN): PyTorch's rule, so the FIRST
// maximum wins a tie; padding is -inf (skipped).  The index of element e is ky*3 + kx of its winning tap; it starts
// at the first tap inside the image (an all -inf window keeps it, as PyTorch does).
// act != null: act = beta * relu(pooled) as well (the first block's pre-activation).
template <class AT>
__global__ void k_maxpool3s2(AT* __restrict__ out, uint8_t* __restrict__ widx, AT* __restrict__ act,
                             const AT* __restrict__ in, float beta, int h, int w, int c, int ho, int wo) {
  constexpr int CE = Chunk<AT>::N;
  const int cch = c / CE;
  const int ni = blockIdx.x / ho, oy = blockIdx.x - ni * ho;
  const int iy0 = 2 * oy - 1;
  const int ky0 = iy0 < 0 ? 1 : 0;
  const int64_t orow = ((int64_t)ni * ho + oy) * wo * cch;
  const int items = wo * cch;
  for (int j = threadIdx.x; j < items; j += blockDim.x) {
    const int ox = j / cch, cc = j - ox * cch;
    const int ix0 = 2 * ox - 1;
    const int kx0 = ix0 < 0 ? 1 : 0;
    float m[CE];
    uint8_t id[CE];
#pragma unroll
    for (int e = 0; e < CE; ++e) { m[e] = -__builtin_huge_valf(); id[e] = (uint8_t)(ky0 * 3 + kx0); }
#pragma unroll
    for (int ky = 0; ky < 3; ++ky) {
      const int iy = iy0 + ky;
      if (iy < 0 || iy >= h) continue;
#pragma unroll
      for (int kx = 0; kx < 3; ++kx) {
        const int ix = ix0 + kx;
        if (ix < 0 || ix >= w) continue;
        float f[CE];
        ldc<AT>(in, (((int64_t)ni * h + iy) * w + ix) * cch + cc, f);
#pragma unroll
        for (int e = 0; e < CE; ++e)
          if (f[e] > m[e] || __builtin_isnan(f[e])) { m[e] = f[e]; id[e] = (uint8_t)(ky * 3 + kx); }
      }
    }
    stc<AT>(out, orow + j, m);
    if constexpr (CE == 8) {
      uint2 q;
      q.x = id[0] | (id[1] << 8) | (id[2] << 16) | ((unsigned)id[3] << 24);
      q.y = id[4] | (id[5] << 8) | (id[6] << 16) | ((unsigned)id[7] << 24);
      ((uint2*)widx)[orow + j] = q;
    } else {
      ((unsigned*)widx)[orow + j] = id[0] | (id[1] << 8) | (id[2] << 16) | ((unsigned)id[3] << 24);
    }
    if (act) {
      float a[CE];
#pragma unroll
      for (int e = 0; e < CE; ++e) a[e] = beta * relu_(m[e]);
      stc<AT>(act, orow + j, a);
    }
  }
}
template <int CE> DEVI void ld_idx(const uint8_t* widx, int64_t ci, int* id) {
  if constexpr (CE == 8) {
    const uint2 q = ((const uint2*)widx)[ci];
#pragma unroll
    for (int e = 0; e < 4; ++e) { id[e] = (q.x >> (8 * e)) & 255; id[4 + e] = (q.y >> (8 * e)) & 255; }
  } else {
    const unsigned q = ((const unsigned*)widx)[ci];
#pragma unroll
    for (int e = 0; e < 4; ++e) id[e] = (q >> (8 * e)) & 255;
  }
}
// tangent: out_t = in_t at the stored tap; act_t = beta * 1[pooled > 0] * out_t (pooled = the primal stash)
template <class AT>
__global__ void k_maxpool3s2_t(AT* __restrict__ out_t, AT* __restrict__ act_t, const AT* __restrict__ pooled,
                               const uint8_t* __restrict__ widx, const AT* __restrict__ in_t, float beta, int h, int w,
                               int c, int ho, int wo) {
  constexpr int CE = Chunk<AT>::N;
  const int cch = c / CE;
  const int ni = blockIdx.x / ho, oy = blockIdx.x - ni * ho;
  const int64_t orow = ((int64_t)ni * ho + oy) * wo * cch;
  const int items = wo * cch;
  for (int j = threadIdx.x; j < items; j += blockDim.x) {
    const int ox = j / cch, cc = j - ox * cch;
    int id[CE];
    ld_idx<CE>(widx, orow + j, id);
    float t[CE];
#pragma unroll
    for (int e = 0; e < CE; ++e) {
      const int ky = id[e] / 3, kx = id[e] - 3 * ky;
      const int iy = 2 * oy - 1 + ky, ix = 2 * ox - 1 + kx;   // inside the image by construction of the index
      const bool in_img = iy >= 0 && iy < h && ix >= 0 && ix < w;   // (never reads outside on a corrupt index)
      t[e] = in_img ? to_f(in_t[(((int64_t)ni * h + iy) * w + ix) * c + cc * CE + e]) : 0.f;
    }
    stc<AT>(out_t, orow + j, t);
    if (act_t) {
      float p[CE], a[CE];
      ldc<AT>(pooled, orow + j, p);
#pragma unroll
      for (int e = 0; e < CE; ++e) a[e] = p[e] > 0.f ? beta * t[e] : 0.f;
      stc<AT>(act_t, orow + j, a);
    }
  }
}
// backward in gather form: din[iy, ix] = sum over the (at most 2 x 2) windows that contain (iy, ix) of dout where
// that window's index points at (iy, ix).  Windows are visited in increasing (oy, ox) order, the order in which
// PyTorch's scatter adds them.  One block per (image, input row).
template <class AT>
__global__ void k_maxpool3s2_bwd(AT* __restrict__ din, const AT* __restrict__ dout, const uint8_t* __restrict__ widx,
                                 int h, int w, int c, int ho, int wo) {
  constexpr int CE = Chunk<AT>::N;
  const int cch = c / CE;
  const int ni = blockIdx.x / h, iy = blockIdx.x - ni * h;
  const int64_t irow = ((int64_t)ni * h + iy) * w * cch;
  const int items = w * cch;
  for (int j = threadIdx.x; j < items; j += blockDim.x) {
    const int ix = j / cch, cc = j - ix * cch;
    float acc[CE];
#pragma unroll
    for (int e = 0; e < CE; ++e) acc[e] = 0.f;
#pragma unroll
    for (int ky = 2; ky >= 0; --ky) {
      const int ty = iy + 1 - ky;
      if ((ty & 1) || ty < 0 || (ty >> 1) >= ho) continue;
      const int oy = ty >> 1;
#pragma unroll
      for (int kx = 2; kx >= 0; --kx) {
        const int tx = ix + 1 - kx;
        if ((tx & 1) || tx < 0 || (tx >> 1) >= wo) continue;
        const int64_t oc = (((int64_t)ni * ho + oy) * wo + (tx >> 1)) * cch + cc;
        int id[CE];
        float g[CE];
        ld_idx<CE>(widx, oc, id);
        ldc<AT>(dout, oc, g);
#pragma unroll
        for (int e = 0; e < CE; ++e)
          if (id[e] == ky * 3 + kx) acc[e] += g[e];
      }
    }
    stc<AT>(din, irow + j, acc);
  }
}

// ------------------------------------------------------------------ residual sum without squeeze-excite
// X' = alpha*C3 + SC ; A' = beta*relu(X')      (timm NormFreeBlock: out*alpha + shortcut; beta = next block's
// 1/sqrt(expected var)).  S = Dual: the tangent of both (primal from the stash), tangents written only.
template <class S, class AT>
__global__ void k_resid_relu(const AT* __restrict__ c3, const AT* __restrict__ c3_t, const AT* __restrict__ sc,
                             const AT* __restrict__ sc_t, AT* __restrict__ xo, AT* __restrict__ xo_t,
                             AT* __restrict__ ao, AT* __restrict__ ao_t, float alpha, float beta, int64_t chunks) {
  constexpr int CE = Chunk<AT>::N;
  const bool act = ao || ao_t;
  for (int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; i < chunks; i += (int64_t)gridDim.x * blockDim.x) {
    float a[CE], b[CE], at[CE], bt[CE], o[CE], ot[CE], r[CE], rt[CE];
    ldc<AT>(c3, i, a);
    ldc<AT>(sc, i, b);
    if constexpr (IsDual<S>::v) { ldc<AT>(c3_t, i, at); ldc<AT>(sc_t, i, bt); }
#pragma unroll
    for (int e = 0; e < CE; ++e) {
      o[e] = alpha * a[e] + b[e];
      r[e] = beta * relu_(o[e]);
      if constexpr (IsDual<S>::v) {
        ot[e] = alpha * at[e] + bt[e];
        rt[e] = o[e] > 0.f ? beta * ot[e] : 0.f;
      }
    }
    if constexpr (IsDual<S>::v) {
      stc<AT>(xo_t, i, ot);
      if (act) stc<AT>(ao_t, i, rt);
    } else {
      stc<AT>(xo, i, o);
      if (act) stc<AT>(ao, i, r);
    }
  }
}
template <class AT>
__global__ void k_scale(AT* __restrict__ out, const AT* __restrict__ in, float alpha, int64_t chunks) {
  constexpr int CE = Chunk<AT>::N;
  for (int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; i < chunks; i += (int64_t)gridDim.x * blockDim.x) {
    float f[CE];
    ldc<AT>(in, i, f);
#pragma unroll
    for (int e = 0; e < CE; ++e) f[e] *= alpha;
    stc<AT>(out, i, f);
  }
}

// ------------------------------------------------------------------ stem columns
// col[m, tap*cpad + c] = in[n, oy*stride - pad + ty, ox*stride - pad + tx, c] (0 outside), tap = ty*k + tx: the K layout
// of the packed forward weight [cout][k*k][cpad], so the 7x7 stem runs as a pointwise contraction over these columns
// (the implicit-GEMM kernels keep the valid taps of a row in a 32-bit mask: at most 5x5).  One block per (image, output
// row); threads walk the row's (ox, tap, 16-byte chunk) items with 32-bit index arithmetic.
template <class AT>
__global__ void k_im2col(AT* __restrict__ col, const AT* __restrict__ in, int h, int w, int cpad, int k, int stride,
                         int pad, int ho, int wo) {
  constexpr int CE = Chunk<AT>::N;
  const int cch = cpad / CE, kk = k * k, per_px = kk * cch;
  const int ni = blockIdx.x / ho, oy = blockIdx.x - ni * ho;
  const int64_t orow = ((int64_t)ni * ho + oy) * wo * per_px;
  const int64_t ibase = (int64_t)ni * h * w * cch;
  const int iy0 = oy * stride - pad;
  const int items = wo * per_px;
  for (int j = threadIdx.x; j < items; j += blockDim.x) {
    const int ox = j / per_px, r = j - ox * per_px;
    const int tap = r / cch, cc = r - tap * cch;
    const int ty = tap / k, tx = tap - ty * k;
    const int iy = iy0 + ty, ix = ox * stride - pad + tx;
    uint4 v = make_uint4(0u, 0u, 0u, 0u);
    if (iy >= 0 && iy < h && ix >= 0 && ix < w) v = ((const uint4*)in)[ibase + (iy * w + ix) * cch + cc];
    ((uint4*)col)[orow + j] = v;
  }
}

}  // namespace

// ====================================================================== launchers
template <class AT>
void launch_im2col(AT* col, const AT* in, int n, int h, int w, int cpad, int k, int stride, int pad, int ho, int wo,
                   hipStream_t st) {
  k_im2col<AT><<<n * ho, 256, 0, st>>>(col, in, h, w, cpad, k, stride, pad, ho, wo);
}
int maxpool3s2_out(int h) { return (h - 1) / 2 + 1; }
template <class AT>
void launch_maxpool3s2(AT* out, uint8_t* widx, AT* act, const AT* in, float beta, int n, int h, int w, int c,
                       hipStream_t st) {
  const int ho = maxpool3s2_out(h), wo = maxpool3s2_out(w);
  k_maxpool3s2<AT><<<n * ho, 256, 0, st>>>(out, widx, act, in, beta, h, w, c, ho, wo);
}
template <class AT>
void launch_maxpool3s2_t(AT* out_t, AT* act_t, const AT* pooled, const uint8_t* widx, const AT* in_t, float beta, int n,
                         int h, int w, int c, hipStream_t st) {
  const int ho = maxpool3s2_out(h), wo = maxpool3s2_out(w);
  k_maxpool3s2_t<AT><<<n * ho, 256, 0, st>>>(out_t, act_t, pooled, widx, in_t, beta, h, w, c, ho, wo);
}
template <class AT>
void launch_maxpool3s2_bwd(AT* din, const AT* dout, const uint8_t* widx, int n, int h, int w, int c, hipStream_t st) {
  const int ho = maxpool3s2_out(h), wo = maxpool3s2_out(w);
  k_maxpool3s2_bwd<AT><<<n * h, 256, 0, st>>>(din, dout, widx, h, w, c, ho, wo);
}
template <class AT>
void launch_resid_relu(const AT* c3, const AT* c3_t, const AT* sc, const AT* sc_t, AT* xo, AT* xo_t, AT* ao, AT* ao_t,
                       float alpha, float beta, int64_t elems, hipStream_t st) {
  const int64_t chunks = elems / Chunk<AT>::N;
  if (c3_t)
    k_resid_relu<Dual, AT><<<grid_of(chunks), 256, 0, st>>>(c3, c3_t, sc, sc_t, xo, xo_t, ao, ao_t, alpha, beta, chunks);
  else
    k_resid_relu<float, AT><<<grid_of(chunks), 256, 0, st>>>(c3, nullptr, sc, nullptr, xo, nullptr, ao, nullptr, alpha,
                                                             beta, chunks);
}
template <class AT>
void launch_scale_act(AT* out, const AT* in, float alpha, int64_t elems, hipStream_t st) {
  const int64_t chunks = elems / Chunk<AT>::N;
  k_scale<AT><<<grid_of(chunks), 256, 0, st>>>(out, in, alpha, chunks);
}
#define INST(AT)                                                                                                    \
  template void launch_maxpool3s2<AT>(AT*, uint8_t*, AT*, const AT*, float, int, int, int, int, hipStream_t);      \
  template void launch_maxpool3s2_t<AT>(AT*, AT*, const AT*, const uint8_t*, const AT*, float, int, int, int, int, \
                                        hipStream_t);                                                               \
  template void launch_maxpool3s2_bwd<AT>(AT*, const AT*, const uint8_t*, int, int, int, int, hipStream_t);        \
  template void launch_resid_relu<AT>(const AT*, const AT*, const AT*, const AT*, AT*, AT*, AT*, AT*, float, float, \
                                      int64_t, hipStream_t);                                                        \
  template void launch_scale_act<AT>(AT*, const AT*, float, int64_t, hipStream_t);                              \
  template void launch_im2col<AT>(AT*, const AT*, int, int, int, int, int, int, int, int, int, hipStream_t);
INST(float)
INST(bf16)
