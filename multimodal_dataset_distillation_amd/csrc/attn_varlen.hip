// Bidirectional multi-head attention over PACKED sequences of different lengths (BERT's key-padding mask without the
// padding), forward only: head dimension 64, 1 <= len_r <= max_len <= 512.
//
//   out[cu[r] + i, :] = softmax(scale * q_i . K_r) V_r          K_r, V_r: the len_r = cu[r + 1] - cu[r] rows of sequence r
//
// qkv is [total, 3, heads, 64], out [total, heads, 64]; there is no padding row anywhere.  A workgroup handles 128 query
// rows of one (sequence, head): grid (n * heads, ceil(max_len / 128)), and a chunk that starts at or beyond len_r exits at
// once.  The keys of another sequence are never loaded, so they cannot reach a bit of this one; the LDS rows beyond len_r
// (the last 32-row tile is filled up with zeros) take no part in the row maximum or the denominator and their
// probabilities are exact zeros -- the standard attn_causal.hip sets for its masked keys.
//
// K and V are STREAMED through LDS in stages of 128 keys (DESIGN.md section 14 has the arithmetic): the workgroup needs
// the 33,280 B of attn_causal.hip's kernel whatever max_len is, so four workgroups share a CU at 512 tokens as at 20,
// where K and V resident for 512 keys (130 KB) would leave one workgroup -- one wave per SIMD -- on a CU for every
// sequence of a call that holds a single long one.  There is no running maximum: as in attn_causal.hip the scores are
// computed twice, a first sweep over the stages for the row maximum and a second one for the probabilities, so the output
// accumulators are never rescaled and a probability is exp(scale * (s - max)) with the row's final maximum.  A sequence of
// at most 128 tokens (every caption but a handful) is one stage: K and V are loaded once and the flow is the causal
// kernel's.  Longer ones load K twice; the second read comes from L2.
//
// bf16: attn_causal.hip's structure (wave w owns 32 query rows, S[key (registers), query (lane)] from
// v_mfma_f32_32x32x16_bf16 is the A operand of the second product, V staged transposed).  fp32 (the parity dtype): one
// thread per query row, K and V of a stage in LDS, plain FMA in a fixed order (keys ascending).
//
// cu_seqlens is device data the host cannot inspect without a synchronisation: the kernels clamp what they read from it so
// that no row outside [0, total) is read or written whatever it holds.
#include <cstdint>

#include "host.h"
#include "mdd_hip.h"

namespace {

constexpr int HD = 64;                 // head dimension
constexpr int STG = 128;               // keys per stage; also the query rows of a workgroup
constexpr int RTP = 132;               // pitch (elements) of the transposed V: 66 dwords, conflict-free 8-byte reads
constexpr int KB = STG * 128;          // bytes of the row-major K stage [128 x 64] bf16
constexpr int VB = HD * RTP * 2;       // bytes of the transposed V stage
constexpr int MAXLEN = 512;

DEVI int lds_row_off(int row, int chunk) { return row * 128 + ((chunk ^ ((row >> 1) & 7)) << 4); }
DEVI int rowmap(int r, int lh) { return (r & 3) + 8 * (r >> 2) + 4 * lh; }

typedef unsigned __attribute__((ext_vector_type(4))) u32x4;

struct VarlenArgs {
  const void* qkv;                     // [total, 3, heads, 64]
  void* out;                           // [total, heads, 64]
  const int32_t* cu;                   // [n + 1]
  int total, heads, max_len;
  float scale;
};

// first row and length of sequence `seq`, clamped so that [start, start + len) lies in [0, total) and len <= max_len
DEVI void seq_span(const VarlenArgs& p, int seq, int& start, int& len) {
  int s = p.cu[seq], e = p.cu[seq + 1];
  s = s < 0 ? 0 : (s > p.total ? p.total : s);
  e = e < s ? s : (e > p.total ? p.total : e);
  start = s;
  len = e - s > p.max_len ? p.max_len : e - s;
}

__global__ __launch_bounds__(256) void k_attn_varlen_bf16(const VarlenArgs p) {
  __shared__ __attribute__((aligned(16))) char smem[KB + VB];
  char* const Ks = smem;
  char* const Vt = smem + KB;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, l31 = lane & 31, lh = lane >> 5;
  const int H = p.heads, Dm = H * HD;
  const int head = blockIdx.x % H, seq = blockIdx.x / H;
  int start, T;
  seq_span(p, seq, start, T);
  const int q0 = blockIdx.y * STG;     // first query row of this workgroup
  if (q0 >= T) return;                 // (uniform) nothing of this chunk belongs to the sequence
  const size_t qrow = (size_t)3 * Dm;
  const bf16* qkv = (const bf16*)p.qkv + (size_t)start * qrow + (size_t)head * HD;
  const bf16 *gq = qkv, *gk = qkv + Dm, *gv = qkv + 2 * Dm;
  const int ns = (T + STG - 1) / STG;  // stages that hold keys

  // ---- LDS fill of stage st: K row-major (16-byte chunks, swizzled), V transposed (a 32-bit store holds [row 2 j | row
  // 2 j + 1] of a column); rows beyond the sequence are zeros up to the end of their 32-row tile
  auto fill_k = [&](int st) {
    const int k0 = st * STG, rows = T - k0 < STG ? T - k0 : STG, nt = (rows + 31) >> 5;
    for (int c = tid; c < nt * 32 * 8; c += 256) {
      const int row = c >> 3, ch = c & 7;
      u32x4 v = {0u, 0u, 0u, 0u};
      if (row < rows) v = *(const u32x4*)(gk + (size_t)(k0 + row) * qrow + ch * 8);
      *(u32x4*)(Ks + lds_row_off(row, ch)) = v;
    }
  };
  auto fill_v = [&](int st) {
    const int k0 = st * STG, rows = T - k0 < STG ? T - k0 : STG, nt = (rows + 31) >> 5;
    for (int c = tid; c < nt * 16 * 8; c += 256) {
      const int rp = c >> 3, ch = c & 7;
      u32x4 a = {0u, 0u, 0u, 0u}, b = {0u, 0u, 0u, 0u};
      if (2 * rp < rows) a = *(const u32x4*)(gv + (size_t)(k0 + 2 * rp) * qrow + ch * 8);
      if (2 * rp + 1 < rows) b = *(const u32x4*)(gv + (size_t)(k0 + 2 * rp + 1) * qrow + ch * 8);
      unsigned* d = (unsigned*)Vt;
#pragma unroll
      for (int e = 0; e < 8; ++e) {
        const unsigned lo = (a[e >> 1] >> ((e & 1) * 16)) & 0xffffu, hi = (b[e >> 1] >> ((e & 1) * 16)) & 0xffffu;
        d[((ch * 8 + e) * RTP + 2 * rp) >> 1] = lo | (hi << 16);
      }
    }
  };
  // ---- the owner's query row: lane (row q0 + 32 w + l31, half lh) holds elements 16 s + 8 lh .. + 8, s = 0 .. 3
  const int own = q0 + wave * 32 + l31;
  const bool active = q0 + wave * 32 < T;          // (wave-uniform) this wave owns at least one token
  u32x4 fQ[4];
#pragma unroll
  for (int s = 0; s < 4; ++s) {
    u32x4 v = {0u, 0u, 0u, 0u};
    if (own < T) v = *(const u32x4*)(gq + (size_t)own * qrow + 16 * s + 8 * lh);
    fQ[s] = v;
  }

  auto mm = [&](const u32x4& a, const u32x4& b, f32x16& acc) {
    acc = __builtin_amdgcn_mfma_f32_32x32x16_bf16(__builtin_bit_cast(bf16x8, a), __builtin_bit_cast(bf16x8, b), acc, 0, 0, 0);
  };
  // score tile t of the stage in LDS: acc[r] = sum_d K[32 t + rowmap(r, lh)][d] * Q[own][d]
  auto tile = [&](int t, f32x16& acc) {
#pragma unroll
    for (int r = 0; r < 16; ++r) acc[r] = 0.f;
#pragma unroll
    for (int s = 0; s < 4; ++s) mm(*(const u32x4*)(Ks + lds_row_off(32 * t + l31, 2 * s + lh)), fQ[s], acc);
  };
  const float c1 = p.scale * 1.4426950408889634f;  // exp(s x) = exp2(c1 x)

  // ---- sweep A: the row maximum over the keys 0 .. T - 1
  float mx = -3.0e38f;
  for (int st = 0; st < ns; ++st) {
    if (st > 0) __syncthreads();       // every wave has left the previous stage
    fill_k(st);
    if (ns == 1) fill_v(0);            // one stage: both operands stay for sweep B
    __syncthreads();
    if (active) {
      const int rows = T - st * STG < STG ? T - st * STG : STG, nt = (rows + 31) >> 5;
      for (int t = 0; t < nt; ++t) {
        f32x16 S; tile(t, S);
        if (32 * t + 32 > rows) {      // the tile the sequence ends in: per element
#pragma unroll
          for (int r = 0; r < 16; ++r) if (32 * t + rowmap(r, lh) < rows) mx = fmaxf(mx, S[r]);
        } else {
#pragma unroll
          for (int r = 0; r < 16; ++r) mx = fmaxf(mx, S[r]);
        }
      }
    }
  }
  mx = fmaxf(mx, __shfl_xor(mx, 32, 64));
  const float nm = -mx * c1;

  // ---- sweep B: probabilities -> second product, the denominator on the way
  f32x16 o[2];
#pragma unroll
  for (int r = 0; r < 16; ++r) { o[0][r] = 0.f; o[1][r] = 0.f; }
  float l_run = 0.f;
  for (int st = 0; st < ns; ++st) {
    if (ns > 1) {
      __syncthreads();
      fill_k(st); fill_v(st);
      __syncthreads();
    }
    if (active) {
      const int rows = T - st * STG < STG ? T - st * STG : STG, nt = (rows + 31) >> 5;
      for (int t = 0; t < nt; ++t) {
        f32x16 S; tile(t, S);
        const bool edge = 32 * t + 32 > rows;
#pragma unroll
        for (int h = 0; h < 2; ++h) {
          float w[8];
#pragma unroll
          for (int i = 0; i < 8; ++i) {
            const int r = 8 * h + i;
            float P = __builtin_amdgcn_exp2f(fmaf(S[r], c1, nm));
            if (edge && 32 * t + rowmap(r, lh) >= rows) P = 0.f;   // a select: whatever S holds there is dropped
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
    }
  }
  if (active) {
    // normalise: row rho of the output belongs to the lane with l31 = rho (the key of the maximum has probability 1:
    // l_run >= 1)
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
  if (!active) return;
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
  bf16* dst = (bf16*)p.out + (size_t)start * Dm + (size_t)head * HD;
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    const int c = lane + 64 * j, row = c >> 3, ch = c & 7, grow = q0 + wave * 32 + row;
    if (grow < T) *(uint4*)(dst + (size_t)grow * Dm + ch * 8) = *(const uint4*)((const char*)stg16 + row * 128 + ch * 16);
  }
}

// exact fp32: thread i owns query row q0 + i; dynamic LDS = K [kt][64] | V [kt][64] floats, kt = min(max_len, 128)
__global__ __launch_bounds__(128) void k_attn_varlen_f32(const VarlenArgs p, const int kt) {
  extern __shared__ __attribute__((aligned(16))) float smf[];
  const int H = p.heads, Dm = H * HD, tid = threadIdx.x;
  float* const Ks = smf;
  float* const Vs = smf + (size_t)kt * HD;
  const int head = blockIdx.x % H, seq = blockIdx.x / H;
  int start, T;
  seq_span(p, seq, start, T);
  const int q0 = blockIdx.y * STG;
  if (q0 >= T) return;
  const size_t qrow = (size_t)3 * Dm;
  const float* qkv = (const float*)p.qkv + (size_t)start * qrow + (size_t)head * HD;
  const int ns = (T + STG - 1) / STG;
  // rows of stage st are keys st * 128 ..; T <= max_len, so a stage never holds more than kt rows
  auto fill = [&](int st, bool with_v) {
    const int k0 = st * STG, rows = T - k0 < STG ? T - k0 : STG;
    for (int c = tid; c < rows * 16; c += 128) {
      const int row = c >> 4, ch = c & 15;
      const float* src = qkv + (size_t)(k0 + row) * qrow;
      *(float4*)(Ks + row * HD + 4 * ch) = *(const float4*)(src + Dm + 4 * ch);
      if (with_v) *(float4*)(Vs + row * HD + 4 * ch) = *(const float4*)(src + 2 * Dm + 4 * ch);
    }
  };
  const int i = q0 + tid;
  const bool own_ok = i < T;
  float q[HD];
#pragma unroll
  for (int d = 0; d < HD; d += 4) {
    float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
    if (own_ok) v = *(const float4*)(qkv + (size_t)i * qrow + d);
    q[d] = v.x; q[d + 1] = v.y; q[d + 2] = v.z; q[d + 3] = v.w;
  }
  // the same instruction sequence in both sweeps: a key's score is the same number in both
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
  for (int st = 0; st < ns; ++st) {
    if (st > 0) __syncthreads();
    fill(st, ns == 1);
    __syncthreads();
    const int rows = T - st * STG < STG ? T - st * STG : STG;
    if (own_ok)
      for (int j = 0; j < rows; ++j) mx = fmaxf(mx, score(j));
  }
  float o[HD];
#pragma unroll
  for (int d = 0; d < HD; ++d) o[d] = 0.f;
  float l = 0.f;
  for (int st = 0; st < ns; ++st) {
    if (ns > 1) {
      __syncthreads();
      fill(st, true);
      __syncthreads();
    }
    const int rows = T - st * STG < STG ? T - st * STG : STG;
    if (own_ok)
      for (int j = 0; j < rows; ++j) {
        const float P = __expf(p.scale * (score(j) - mx));
        l += P;
        const float* v = Vs + j * HD;
#pragma unroll
        for (int d = 0; d < HD; d += 4) {
          const float4 u = *(const float4*)(v + d);
          o[d] = fmaf(P, u.x, o[d]); o[d + 1] = fmaf(P, u.y, o[d + 1]); o[d + 2] = fmaf(P, u.z, o[d + 2]); o[d + 3] = fmaf(P, u.w, o[d + 3]);
        }
      }
  }
  if (!own_ok) return;
  const float linv = 1.f / l;
  float* dst = (float*)p.out + ((size_t)start + i) * Dm + (size_t)head * HD;
#pragma unroll
  for (int d = 0; d < HD; d += 4) *(float4*)(dst + d) = make_float4(o[d] * linv, o[d + 1] * linv, o[d + 2] * linv, o[d + 3] * linv);
}

}  // namespace

extern "C" int mdd_op_attention_varlen(int dtype, int n, int total, int heads, float scale, const void* qkv,
                                       const int32_t* cu_seqlens, int max_len, void* out, void* stream) {
  CHECK_STORAGE(dtype);
  CHECK_ARG(qkv && out && cu_seqlens, "varlen attention: null pointer");
  CHECK_ARG(n >= 1 && heads >= 1 && total >= n, "varlen attention: n, heads >= 1 and total >= n (no sequence is empty)");
  CHECK_ARG(max_len >= 1 && max_len <= MAXLEN, "varlen attention needs 1 <= max_len <= 512");
  CHECK_ARG((int64_t)n * heads <= 2147483647ll, "varlen attention: n * heads overflows the grid");
  VarlenArgs a; a.qkv = qkv; a.out = out; a.cu = cu_seqlens; a.total = total; a.heads = heads; a.max_len = max_len;
  a.scale = scale;
  const dim3 grid((unsigned)((int64_t)n * heads), (unsigned)((max_len + STG - 1) / STG));
  hipStream_t st = (hipStream_t)stream;
  if (dtype == MDD_DTYPE_BF16) k_attn_varlen_bf16<<<grid, 256, 0, st>>>(a);
  else {
    const int kt = max_len < STG ? max_len : STG;       // <= 64 KiB of LDS: no attribute needed
    k_attn_varlen_f32<<<grid, 128, (size_t)2 * kt * HD * sizeof(float), st>>>(a, kt);
  }
  POST_LAUNCH("op_attention_varlen");
  return 0;
}
