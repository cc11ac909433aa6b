// Grouped 3x3 convolutions with EIGHT channels per group, bf16 storage (NF-RegNet's conv2: 5 ... 92 groups):
// forward (stride 1 and 2) and data gradient (stride 1 and 2), each with the optional second operand pair of the
// tangent passes, and the epilogues of csrc/conv_gemm_epilogue.inc that this topology puts on them.
//
// The general implicit-GEMM kernels run one block column per group: a 32-wide N tile of which 8 columns are real,
// K = 72 padded to 128, and 16-byte slivers of every activation row per block.  At 72 MAC per output element (about
// 36 FLOP per byte in bf16) these layers are bound by bytes, not by matrix-core density, so the kernel here is a plain
// fp32-FMA kernel laid out for the memory system: consecutive lanes own consecutive GROUPS of the same pixels, so a
// wave's 16-byte loads and stores cover whole contiguous activation rows, and one thread keeps a tap's 8 x 8 weight
// block in registers for a strip of pixels.
//   k_conv_g8: thread = (group, strip of 4 output pixels along x); out[m, g*8+n] = sum_{tap,kc} A[src(m,tap), g*8+kc] *
//   B[g][n][tap][kc], src by the forward or the transposed (data gradient) rule -- the packed layouts wf [cout][9][8]
//   and wt [groups][8][9][8] index the same way.
// Which geometry / pass is routed here is decided by g8_routes() from the timings of tools/bench_group8.py
// (profiles/nf_regnet_b1_group8_bench.json); mdd_set_group8_kernels(0) sends everything to the general kernels, (2)
// every geometry here.
// The WEIGHT gradient stays on the general kernel for every geometry: a dedicated one (a thread per (pixel chunk, tap,
// group) with 64 fp32 accumulators and a slab combine) measured 1.6 to 8.6 times SLOWER than k_conv_wgrad
// (0.60 against 0.07 ms at 5 groups, 112 / 2; 0.07 against 0.04 ms at 92 groups, 7 / 1:
// profiles/nf_regnet_b1_group8_wgrad_attempt.json) and was not kept.
#include <atomic>

#include "kernels.h"

namespace {

constexpr int PX = 4;   // output pixels per thread (a strip along x)

struct G8Args {
  const bf16 *A1, *B1, *A2, *B2;
  ConvEpi ep;
  int nimg, ha, wa, ho, wo, groups, stride, strips;
  int64_t items;
};

DEVI void unpack8(const uint4& q, float* f) { Chunk<bf16>::unpack(q, f); }

template <int TR>
__global__ __launch_bounds__(256) void k_conv_g8(G8Args a) {
  const int64_t item = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (item >= a.items) return;
  const int G = a.groups;
  const int g = (int)(item % G);
  int s = (int)(item / G);
  const int xs = s % a.strips; s /= a.strips;
  const int oy = s % a.ho, ni = s / a.ho;
  const int ox0 = xs * PX;
  float acc[PX][8];
#pragma unroll
  for (int j = 0; j < PX; ++j)
#pragma unroll
    for (int n = 0; n < 8; ++n) acc[j][n] = 0.f;
#pragma unroll 1
  for (int src = 0; src < 2; ++src) {
    const uint4* A = (const uint4*)(src ? a.A2 : a.A1);
    const uint4* B = (const uint4*)(src ? a.B2 : a.B1);
    if (A == nullptr) continue;
#pragma unroll 1
    for (int ty = 0; ty < 3; ++ty) {
      int iy;
      if (TR) {
        const int ny = oy + 1 - ty;
        if (ny < 0 || (ny % a.stride) != 0) continue;
        iy = ny / a.stride;
      } else {
        iy = oy * a.stride - 1 + ty;
      }
      if (iy < 0 || iy >= a.ha) continue;
      const int64_t arow = ((int64_t)ni * a.ha + iy) * a.wa;
#pragma unroll 1
      for (int tx = 0; tx < 3; ++tx) {
        int ix[PX];
        bool ok[PX], any = false;
#pragma unroll
        for (int j = 0; j < PX; ++j) {
          const int ox = ox0 + j;
          if (TR) {
            const int nx = ox + 1 - tx;
            ok[j] = nx >= 0 && (nx % a.stride) == 0;
            ix[j] = nx / a.stride;
          } else {
            ix[j] = ox * a.stride - 1 + tx;
            ok[j] = true;
          }
          ok[j] = ok[j] && ox < a.wo && ix[j] >= 0 && ix[j] < a.wa;
          any = any || ok[j];
        }
        if (!any) continue;
        uint4 qa[PX];
#pragma unroll
        for (int j = 0; j < PX; ++j)
          qa[j] = ok[j] ? A[(arow + ix[j]) * G + g] : make_uint4(0u, 0u, 0u, 0u);
        const uint4* wq = B + ((int64_t)g * 8 * 9 + ty * 3 + tx);   // + n * 9 chunks
        uint4 qw[8];
#pragma unroll
        for (int n = 0; n < 8; ++n) qw[n] = wq[n * 9];
        float x[PX][8];
#pragma unroll
        for (int j = 0; j < PX; ++j) unpack8(qa[j], x[j]);
#pragma unroll
        for (int n = 0; n < 8; ++n) {
          float w[8];
          unpack8(qw[n], w);
#pragma unroll
          for (int j = 0; j < PX; ++j)
#pragma unroll
            for (int k = 0; k < 8; ++k) acc[j][n] = fmaf(x[j][k], w[k], acc[j][n]);
        }
      }
    }
  }
  // ---- epilogue (csrc/conv_gemm_epilogue.inc, SiLU chain): v = acc + bias + add1 ; raw = v ; act by mode ; + add2
  const ConvEpi& E = a.ep;
  float bias[8];
#pragma unroll
  for (int n = 0; n < 8; ++n) bias[n] = 0.f;
  const float* bp = E.mode == EPI_FWD ? E.bias : (E.mode == EPI_FWD_T ? E.bias_t : nullptr);
  if (bp) {
#pragma unroll
    for (int n = 0; n < 8; ++n) bias[n] = bp[g * 8 + n];
  }
  const bool do_act = E.mode != EPI_BWD_LIN && E.out_act != nullptr;
#pragma unroll
  for (int j = 0; j < PX; ++j) {
    const int ox = ox0 + j;
    if (ox >= a.wo) break;
    const int64_t ci = (((int64_t)ni * a.ho + oy) * a.wo + ox) * G + g;
    float v[8], t0[8], t1[8], t2[8], o[8];
#pragma unroll
    for (int n = 0; n < 8; ++n) v[n] = acc[j][n] + bias[n];
    if (E.add1 != nullptr && E.mode != EPI_FWD) {
      unpack8(((const uint4*)E.add1)[ci], t0);
#pragma unroll
      for (int n = 0; n < 8; ++n) v[n] += t0[n];
    }
    if (E.out_raw) ((uint4*)E.out_raw)[ci] = Chunk<bf16>::pack(v);
    if (!do_act) continue;
    if (E.mode == EPI_FWD) {
#pragma unroll
      for (int n = 0; n < 8; ++n) o[n] = E.beta * silu_(v[n]);
    } else if (E.mode == EPI_BWD_T) {
      unpack8(((const uint4*)E.c)[ci], t0); unpack8(((const uint4*)E.c_t)[ci], t1); unpack8(((const uint4*)E.abar)[ci], t2);
#pragma unroll
      for (int n = 0; n < 8; ++n) o[n] = E.beta * (dsilu_(Dual(t0[n], t1[n])) * Dual(t2[n], v[n])).t;
    } else {   // EPI_FWD_T, EPI_BWD
      unpack8(((const uint4*)E.c)[ci], t0);
#pragma unroll
      for (int n = 0; n < 8; ++n) o[n] = E.beta * dsilu_(t0[n]) * v[n];
    }
    if (E.add2 != nullptr) {
      unpack8(((const uint4*)E.add2)[ci], t0);
#pragma unroll
      for (int n = 0; n < 8; ++n) o[n] += t0[n];
    }
    ((uint4*)E.out_act)[ci] = Chunk<bf16>::pack(o);
  }
}

std::atomic<int> g_g8_on{1};

bool g8_geom(const ConvGeom& g) {
  return g.k == 3 && g.pad == 1 && (g.stride == 1 || g.stride == 2) && g.kc == 8 && g.nc == 8 && g.groups >= 1 &&
         g.ca_tot == g.groups * 8 && g.co_tot == g.groups * 8 && g.prec == 0;
}
// Routed here: what tools/bench_group8.py measured faster than the general kernel by more than the run-to-run spread of
// the call (profiles/nf_regnet_b1_group8_bench.json; N = 100, bf16, microseconds dedicated / general), by the
// convolution's input side and stride, and only what did so in each of three calls of the tool:
//   forward        112 / 2 (72 / 82)
//   data gradient  112 / 2 (157 / 234), 56 / 2 (92 / 133), 28 / 2 (55 / 75), 56 / 1 (136 / 153)
// Left on the general kernels: sides 14 and 7 with stride 1 and 14 / 2 forward, where they are faster (62 / 47, 42 / 29,
// 21 / 18), and the wins that were inside the spread in at least one call -- forward 56 / 1 (141 / 153), 56 / 2, 28 / 1,
// 28 / 2 (27 / 30), data gradient 28 / 1 and 14 / 2 (37 / 43).
bool g8_routes(const ConvGeom& g) {
  const int side = g.transposed ? g.ho : g.ha;     // input side of the forward convolution
  if (g.transposed) return g.stride == 2 ? side >= 28 : side >= 56;
  return g.stride == 2 && side >= 112;
}

}  // namespace

int group8_kernels_mode() { return g_g8_on.load(std::memory_order_relaxed); }
void set_group8_kernels(int mode) { g_g8_on.store(mode < 0 ? 0 : (mode > 2 ? 2 : mode), std::memory_order_relaxed); }

bool launch_conv_g8(const ConvGeom& g, const bf16* A1, const bf16* B1, const bf16* A2, const bf16* B2, const ConvEpi& ep,
                    hipStream_t st) {
  const int mode = group8_kernels_mode();       // 0 off, 1 the measured routes, 2 every geometry (tests, timing)
  if (mode == 0 || !g8_geom(g) || (mode == 1 && !g8_routes(g))) return false;
  // epilogues of this topology only: SiLU chain, no per-image bias
  if (ep.ib != nullptr || (ep.out_act != nullptr && ep.act != 0)) return false;
  if (ep.mode < EPI_FWD || ep.mode > EPI_BWD_LIN) return false;
  G8Args a;
  a.A1 = A1; a.B1 = B1; a.A2 = A2; a.B2 = A2 ? B2 : nullptr; a.ep = ep;
  a.nimg = g.nimg; a.ha = g.ha; a.wa = g.wa; a.ho = g.ho; a.wo = g.wo; a.groups = g.groups; a.stride = g.stride;
  a.strips = (g.wo + PX - 1) / PX;
  a.items = (int64_t)g.nimg * g.ho * a.strips * g.groups;
  const unsigned blocks = (unsigned)((a.items + 255) / 256);
  if (g.transposed) k_conv_g8<1><<<blocks, 256, 0, st>>>(a);
  else k_conv_g8<0><<<blocks, 256, 0, st>>>(a);
  return true;
}
