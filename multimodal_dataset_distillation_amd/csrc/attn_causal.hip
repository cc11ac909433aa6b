// Causal multi-head attention of the frozen CLIP text tower (clip/model.py: nn.MultiheadAttention with the additive -inf
// upper-triangular mask), forward only: head dimension 64, 1 <= tokens <= 128 (CLIP's context is 77).
//
//   out[i, :] = softmax(scale * q_i . K[0..i]) V[0..i]
//
// A workgroup handles one (sequence, head); nothing of size tokens x tokens leaves the CU.  Keys after the query take no
// part in anything: not in the row maximum (a masked score must not set the exponent's reference point), not in the
// denominator, and their probabilities are exact zeros, so whatever stands in K behind the diagonal cannot change a bit of
// the rows in front of it.
//
// bf16: the structure of attn.hip's forward mode.  Wave w owns the 32 query rows 32 w .. 32 w + 31 and walks the key tiles
// 0 .. w only -- the tiles wholly above the diagonal are skipped, tile w is masked per element.  A score tile is
// v_mfma_f32_32x32x16_bf16(K rows from LDS, Q rows from registers): the accumulator holds S[key (registers), query (lane)],
// which is the A-operand layout of the second product O[query, :] = sum_key P[query, key] V[key, :], so the probabilities
// go from the accumulator registers to the matrix cores without touching LDS; V is staged transposed so that a lane's
// eight keys of one column are two 8-byte reads.  The scores are computed twice (maximum, then exponentials): with at most
// four key tiles that is cheaper than rescaling the output accumulators.
//
// fp32 (the parity dtype): one thread per query row, K and V of the head in LDS (every lane reads the same key: broadcast
// reads), plain FMA in a fixed order.
#include <cstdint>

#include "host.h"
#include "mdd_hip.h"

namespace {

constexpr int HD = 64;                 // head dimension
constexpr int TPC = 128;               // tokens padded to whole 32-row tiles
constexpr int RTP = 132;               // pitch (elements) of the transposed V: 66 dwords, conflict-free 8-byte reads
constexpr int KB = TPC * 128;          // bytes of the row-major K [TPC x 64] bf16
constexpr int VB = HD * RTP * 2;       // bytes of the transposed V

DEVI int lds_row_off(int row, int chunk) { return row * 128 + ((chunk ^ ((row >> 1) & 7)) << 4); }
DEVI int rowmap(int r, int lh) { return (r & 3) + 8 * (r >> 2) + 4 * lh; }

typedef unsigned __attribute__((ext_vector_type(4))) u32x4;

struct CausalArgs {
  const void* qkv;                     // [n, tok, 3, heads, 64]
  void* out;                           // [n, tok, heads, 64]
  int tok, heads;
  float scale;
};

__global__ __launch_bounds__(256) void k_attn_causal_bf16(const CausalArgs p) {
  __shared__ __attribute__((aligned(16))) char smem[KB + VB];
  char* const Ks = smem;
  char* const Vt = smem + KB;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, l31 = lane & 31, lh = lane >> 5;
  const int T = p.tok, H = p.heads, Dm = H * HD;
  const int head = blockIdx.x % H;
  const size_t seq = blockIdx.x / H;
  const size_t qrow = (size_t)3 * Dm;
  const bf16* qkv = (const bf16*)p.qkv + seq * T * qrow + (size_t)head * HD;
  const bf16 *gq = qkv, *gk = qkv + Dm, *gv = qkv + 2 * Dm;
  const int nt = (T + 31) >> 5;        // tiles that hold tokens

  // ---- LDS fill: K row-major (16-byte chunks, swizzled), V transposed (a 32-bit store holds [row 2 j | row 2 j + 1] of a
  // column); rows beyond the tokens are zeros (their probabilities are zeros too: 0 * 0)
  for (int c = tid; c < nt * 32 * 8; c += 256) {
    const int row = c >> 3, ch = c & 7;
    u32x4 v = {0u, 0u, 0u, 0u};
    if (row < T) v = *(const u32x4*)(gk + (size_t)row * qrow + ch * 8);
    *(u32x4*)(Ks + lds_row_off(row, ch)) = v;
  }
  for (int c = tid; c < nt * 16 * 8; c += 256) {
    const int rp = c >> 3, ch = c & 7;
    u32x4 a = {0u, 0u, 0u, 0u}, b = {0u, 0u, 0u, 0u};
    if (2 * rp < T) a = *(const u32x4*)(gv + (size_t)(2 * rp) * qrow + ch * 8);
    if (2 * rp + 1 < T) b = *(const u32x4*)(gv + (size_t)(2 * rp + 1) * qrow + ch * 8);
    unsigned* d = (unsigned*)Vt;
#pragma unroll
    for (int e = 0; e < 8; ++e) {
      const unsigned lo = (a[e >> 1] >> ((e & 1) * 16)) & 0xffffu, hi = (b[e >> 1] >> ((e & 1) * 16)) & 0xffffu;
      d[((ch * 8 + e) * RTP + 2 * rp) >> 1] = lo | (hi << 16);
    }
  }
  // ---- the owner's query row: lane (row 32 w + l31, half lh) holds elements 16 s + 8 lh .. + 8, s = 0 .. 3
  const int own = wave * 32 + l31;
  const bool own_ok = own < T;
  u32x4 fQ[4];
#pragma unroll
  for (int s = 0; s < 4; ++s) {
    u32x4 v = {0u, 0u, 0u, 0u};
    if (own_ok) v = *(const u32x4*)(gq + (size_t)own * qrow + 16 * s + 8 * lh);
    fQ[s] = v;
  }
  __syncthreads();

  auto mm = [&](const u32x4& a, const u32x4& b, f32x16& acc) {
    acc = __builtin_amdgcn_mfma_f32_32x32x16_bf16(__builtin_bit_cast(bf16x8, a), __builtin_bit_cast(bf16x8, b), acc, 0, 0, 0);
  };
  // score tile t: acc[r] = sum_d K[32 t + rowmap(r, lh)][d] * Q[own][d]
  auto tile = [&](int t, f32x16& acc) {
#pragma unroll
    for (int r = 0; r < 16; ++r) acc[r] = 0.f;
#pragma unroll
    for (int s = 0; s < 4; ++s) mm(*(const u32x4*)(Ks + lds_row_off(32 * t + l31, 2 * s + lh)), fQ[s], acc);
  };
  f32x16 o[2];
#pragma unroll
  for (int r = 0; r < 16; ++r) { o[0][r] = 0.f; o[1][r] = 0.f; }
  if (wave < nt) {                     // (wave-uniform) the other waves own no token
    const float c1 = p.scale * 1.4426950408889634f;    // exp(s x) = exp2(c1 x)
    // pass A: the maximum over the keys 0 .. own.  Tiles t < wave lie wholly below the diagonal
    float mx = -3.0e38f;
    for (int t = 0; t <= wave; ++t) {
      f32x16 S; tile(t, S);
      if (t == wave) {
#pragma unroll
        for (int r = 0; r < 16; ++r) if (32 * t + rowmap(r, lh) <= own) mx = fmaxf(mx, S[r]);
      } else {
#pragma unroll
        for (int r = 0; r < 16; ++r) mx = fmaxf(mx, S[r]);
      }
    }
    mx = fmaxf(mx, __shfl_xor(mx, 32, 64));
    const float nm = -mx * c1;
    // pass B: probabilities -> second product, the denominator on the way
    float l_run = 0.f;
    for (int t = 0; t <= wave; ++t) {
      f32x16 S; tile(t, S);
      const bool diag = t == wave;
#pragma unroll
      for (int h = 0; h < 2; ++h) {
        float w[8];
#pragma unroll
        for (int i = 0; i < 8; ++i) {
          const int r = 8 * h + i;
          float P = __builtin_amdgcn_exp2f(fmaf(S[r], c1, nm));
          if (diag && 32 * t + rowmap(r, lh) > own) P = 0.f;     // a select: whatever S holds there (inf, NaN) is dropped
          l_run += P;
          w[i] = P;
        }
        u32x4 pa;
#pragma unroll
        for (int e = 0; e < 4; ++e) pa[e] = Chunk<bf16>::pk(w[2 * e], w[2 * e + 1]);
        const int base = 32 * t + 16 * h + 4 * lh;
#pragma unroll
        for (int dt = 0; dt < 2; ++dt) {
          const unsigned short* row = (const unsigned short*)Vt + (size_t)(32 * dt + l31) * RTP;
          const uint2 a = *(const uint2*)(row + base), b = *(const uint2*)(row + base + 8);
          u32x4 vb; vb[0] = a.x; vb[1] = a.y; vb[2] = b.x; vb[3] = b.y;
          mm(pa, vb, o[dt]);
        }
      }
    }
    // normalise: row rho of the output belongs to the lane with l31 = rho (key `own` is never masked: l_run >= 1 there)
    l_run += __shfl_xor(l_run, 32, 64);
    const float linv = 1.f / l_run;
#pragma unroll
    for (int r = 0; r < 16; ++r) {
      const float f = __shfl(linv, rowmap(r, lh), 64);
      o[0][r] *= f; o[1][r] *= f;
    }
  }
  // ---- store through this wave's 4 KB of the K region (free once every wave has left the tile loops): global memory sees
  // 16-byte chunks of whole rows
  __syncthreads();
  if (wave >= nt) return;
  unsigned short* stg16 = (unsigned short*)(Ks + wave * 4096);
#pragma unroll
  for (int dt = 0; dt < 2; ++dt)
#pragma unroll
    for (int r = 0; r < 16; ++r) {
      const bf16 v = (bf16)o[dt][r];
      stg16[rowmap(r, lh) * 64 + 32 * dt + l31] = __builtin_bit_cast(unsigned short, v);
    }
  __builtin_amdgcn_s_waitcnt(0xc07f);                   // lgkmcnt(0): this wave's LDS stores have landed
  __builtin_amdgcn_wave_barrier();
  bf16* dst = (bf16*)p.out + seq * T * Dm + (size_t)head * HD;
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    const int c = lane + 64 * j, row = c >> 3, ch = c & 7, grow = wave * 32 + row;
    if (grow < T) *(uint4*)(dst + (size_t)grow * Dm + ch * 8) = *(const uint4*)((const char*)stg16 + row * 128 + ch * 16);
  }
}

// exact fp32: thread i owns query row i; dynamic LDS = K [tok][64] | V [tok][64] floats
__global__ __launch_bounds__(128) void k_attn_causal_f32(const CausalArgs p) {
  extern __shared__ __attribute__((aligned(16))) float smf[];
  const int T = p.tok, H = p.heads, Dm = H * HD, tid = threadIdx.x;
  float* const Ks = smf;
  float* const Vs = smf + (size_t)T * HD;
  const int head = blockIdx.x % H;
  const size_t seq = blockIdx.x / H;
  const size_t qrow = (size_t)3 * Dm;
  const float* qkv = (const float*)p.qkv + seq * T * qrow + (size_t)head * HD;
  for (int c = tid; c < T * 16; c += 128) {
    const int row = c >> 4, ch = c & 15;
    *(float4*)(Ks + row * HD + 4 * ch) = *(const float4*)(qkv + (size_t)row * qrow + Dm + 4 * ch);
    *(float4*)(Vs + row * HD + 4 * ch) = *(const float4*)(qkv + (size_t)row * qrow + 2 * Dm + 4 * ch);
  }
  __syncthreads();
  const int i = tid;
  if (i >= T) return;
  float q[HD];
#pragma unroll
  for (int d = 0; d < HD; d += 4) {
    const float4 v = *(const float4*)(qkv + (size_t)i * qrow + d);
    q[d] = v.x; q[d + 1] = v.y; q[d + 2] = v.z; q[d + 3] = v.w;
  }
  // the same instruction sequence in both passes: a key's score is the same number in both
  auto score = [&](int j) __attribute__((always_inline)) {
    const float* k = Ks + j * HD;
    float s0 = 0.f, s1 = 0.f, s2 = 0.f, s3 = 0.f;
#pragma unroll
    for (int d = 0; d < HD; d += 4) {
      const float4 v = *(const float4*)(k + d);
      s0 = fmaf(q[d], v.x, s0); s1 = fmaf(q[d + 1], v.y, s1); s2 = fmaf(q[d + 2], v.z, s2); s3 = fmaf(q[d + 3], v.w, s3);
    }
    return (s0 + s1) + (s2 + s3);
  };
  float mx = -3.0e38f;
  for (int j = 0; j <= i; ++j) mx = fmaxf(mx, score(j));
  float o[HD];
#pragma unroll
  for (int d = 0; d < HD; ++d) o[d] = 0.f;
  float l = 0.f;
  for (int j = 0; j <= i; ++j) {
    const float P = __expf(p.scale * (score(j) - mx));
    l += P;
    const float* v = Vs + j * HD;
#pragma unroll
    for (int d = 0; d < HD; d += 4) {
      const float4 u = *(const float4*)(v + d);
      o[d] = fmaf(P, u.x, o[d]); o[d + 1] = fmaf(P, u.y, o[d + 1]); o[d + 2] = fmaf(P, u.z, o[d + 2]); o[d + 3] = fmaf(P, u.w, o[d + 3]);
    }
  }
  const float linv = 1.f / l;
  float* dst = (float*)p.out + seq * T * Dm + (size_t)i * Dm + (size_t)head * HD;
#pragma unroll
  for (int d = 0; d < HD; d += 4) *(float4*)(dst + d) = make_float4(o[d] * linv, o[d + 1] * linv, o[d + 2] * linv, o[d + 3] * linv);
}

}  // namespace

extern "C" int mdd_op_attention_causal(int dtype, int n, int tokens, int heads, float scale, const void* qkv, void* out,
                                       void* stream) {
  CHECK_STORAGE(dtype);
  CHECK_ARG(qkv && out && n >= 1 && heads >= 1, "causal attention operands");
  CHECK_ARG(tokens >= 1 && tokens <= TPC, "causal attention needs 1 <= tokens <= 128");
  CHECK_ARG((int64_t)n * heads <= 2147483647ll, "causal attention: n * heads overflows the grid");
  CausalArgs a; a.qkv = qkv; a.out = out; a.tok = tokens; a.heads = heads; a.scale = scale;
  const unsigned grid = (unsigned)((int64_t)n * heads);
  hipStream_t st = (hipStream_t)stream;
  if (dtype == MDD_DTYPE_BF16) k_attn_causal_bf16<<<grid, 256, 0, st>>>(a);
  else k_attn_causal_f32<<<grid, 128, (size_t)2 * tokens * HD * sizeof(float), st>>>(a);   // <= 64 KiB: no attribute needed
  POST_LAUNCH("op_attention_causal");
  return 0;
}
