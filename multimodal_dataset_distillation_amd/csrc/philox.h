// Counter-based dropout masks of the text head (reference networks.py:636,643: Dropout(0.1) in train mode).  Nothing is
// stored: every pass that needs the mask of (seed, iteration, step, sample, column) draws it again with Philox4x32-10
// (Salmon et al., "Parallel random numbers: as easy as 1, 2, 3", SC'11).
//   key     = (seed low 32 bits, seed high 32 bits)
//   counter = (column / 4, sample, step, iteration);  output word column % 4 belongs to `column`
//   sample  = (uint32_t)idx[row] when the pass has a row index vector, else row: a shard that holds some rows of a
//             minibatch draws exactly those rows of the unsharded mask
//   u = float(word >> 8) * 2^-24;  keep iff u >= p (the torch.rand(...) >= p convention);  value = keep ? 1/(1-p) : 0
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

struct DropSpec {
  float p;                   // drop probability in [0, 1); 0 = no dropout
  float scale;               // 1.0f / (1.0f - p), formed in fp32
  uint32_t key0, key1;       // seed low / high word
  uint32_t step, iteration;  // counter words 2 and 3
  const int64_t* idx;        // device: sample id of each row, or null (= the row number)
};

inline DropSpec drop_spec_none() { return DropSpec{0.f, 1.f, 0u, 0u, 0u, 0u, nullptr}; }
inline DropSpec drop_spec(float p, uint64_t seed, uint32_t step, uint32_t iteration, const int64_t* idx) {
  return DropSpec{p, 1.0f / (1.0f - p), (uint32_t)seed, (uint32_t)(seed >> 32), step, iteration, idx};
}
// p in [0, 1); false for NaN as well
inline bool drop_p_valid(float p) { return p >= 0.f && p < 1.f; }

struct Philox4 { uint32_t w0, w1, w2, w3; };

__device__ __forceinline__ Philox4 philox4x32_10(uint32_t c0, uint32_t c1, uint32_t c2, uint32_t c3, uint32_t k0,
                                                 uint32_t k1) {
#pragma unroll
  for (int r = 0; r < 10; ++r) {
    const uint32_t hi0 = __umulhi(0xD2511F53u, c0), lo0 = 0xD2511F53u * c0;
    const uint32_t hi1 = __umulhi(0xCD9E8D57u, c2), lo1 = 0xCD9E8D57u * c2;
    const uint32_t n0 = hi1 ^ c1 ^ k0, n2 = hi0 ^ c3 ^ k1;
    c0 = n0; c1 = lo1; c2 = n2; c3 = lo0;
    k0 += 0x9E3779B9u; k1 += 0xBB67AE85u;   // the key is bumped between rounds (the bump after the last is unused)
  }
  return Philox4{c0, c1, c2, c3};
}

__device__ __forceinline__ float drop_word_value(const DropSpec& s, uint32_t word) {
  const float u = (float)(word >> 8) * 5.9604644775390625e-08f;   // 2^-24: u is exact, in [0, 1)
  return u >= s.p ? s.scale : 0.f;
}
__device__ __forceinline__ uint32_t drop_sample(const DropSpec& s, int row) {
  return s.idx ? (uint32_t)s.idx[row] : (uint32_t)row;
}
// the four words of the quad of columns 4q .. 4q + 3 of `row`
__device__ __forceinline__ Philox4 drop_quad(const DropSpec& s, int row, uint32_t q) {
  return philox4x32_10(q, drop_sample(s, row), s.step, s.iteration, s.key0, s.key1);
}
// mask value of (row, col)
__device__ __forceinline__ float drop_mask_value(const DropSpec& s, int row, int col) {
  const Philox4 w = drop_quad(s, row, (uint32_t)col >> 2);
  const int j = col & 3;
  const uint32_t word = j == 0 ? w.w0 : (j == 1 ? w.w1 : (j == 2 ? w.w2 : w.w3));
  return drop_word_value(s, word);
}
