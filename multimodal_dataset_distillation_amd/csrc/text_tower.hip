// The frozen text towers that write the caption caches, which the reference reaches through textprocess /
// textprocess_train (networks.py:700-735, distill.py:107-144).
//
// --text_encoder clip: OpenAI CLIP's encode_text (clip/model.py).
//
//   x = token_embedding[ids] + positional_embedding                     k_token_embed
//   per block:  x += out_proj(causal_attention(in_proj(ln_1(x))))        k_conv_gemm MODE 0, attn_causal.hip, vit.hip LayerNorm
//               x += c_proj(QuickGELU(c_fc(ln_2(x))))                    k_conv_gemm with the QuickGELU epilogue
//   features = ln_final(x[r, argmax ids[r]]) @ text_projection           k_eot_gather, fp32 LayerNorm, small-batch linear
//
// --text_encoder bert (the reference's default): transformers' BertModel("bert-base-uncased"), last_hidden_state[:, 0].
// The tokens stay PACKED -- total = sum(len) rows and cu_seqlens, no padding row anywhere (the reference pads a chunk to
// its longest caption and computes every padded row):
//
//   x = LN_emb(word[id] + position[t] + token_type[0])                   k_bert_embed (t = row - cu[r]), vit.hip LayerNorm
//   per layer:  x1 = LN(x + dense(attention_varlen(x Wqkv + b)))         one fused [3 D, D] contraction, attn_varlen.hip
//               x  = LN(x1 + dense(GELU(x1 Wi + b)))                     exact GELU in fc1's epilogue where that instance exists
//   features[r] = x[cu[r]]                                               k_cls_gather + fp32 LayerNorm on the n [CLS] rows only
//
// Forward only, its own handle (mdd_text_tower): no theta tangent, no stash, no backward.  The linears run over n * context
// token rows on the engine's contraction kernel; a residual sum is formed by the LayerNorm kernel that reads it (and the
// last one by the gather, in fp32).  The weights are frozen, so they are cast and packed ONCE (mdd_text_tower_load) and every
// other parameter is copied into the workspace beside them; encode only enqueues kernels.
#include <cmath>
#include <cstring>
#include <string>
#include <vector>

#include "kernels.h"
#include "mdd_hip.h"

namespace {

// ---------------------------------------------------------------------------------------------- kernels
// one thread per 16-byte chunk of the output: out[row, c ..] = table[id, c ..] + pos[t, c ..] (fp32 sum, one rounding)
template <class AT>
__global__ __launch_bounds__(256) void k_token_embed(AT* __restrict__ out, const int32_t* __restrict__ ids,
                                                     const float* __restrict__ table, const float* __restrict__ pos,
                                                     int64_t chunks, int ctx, int width, int vocab) {
  constexpr int CE = Chunk<AT>::N;
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (i >= chunks) return;
  const int cpr = width / CE;
  const int64_t row = i / cpr;
  const int c = (int)(i - row * cpr) * CE, t = (int)(row % ctx);
  int id = ids[row];
  id = id < 0 ? 0 : (id >= vocab ? vocab - 1 : id);        // no id reads outside the table
  const float* a = table + (size_t)id * width + c;
  const float* b = pos + (size_t)t * width + c;
  float v[CE];
#pragma unroll
  for (int e = 0; e < CE; e += 4) {
    const float4 x = *(const float4*)(a + e), y = *(const float4*)(b + e);
    v[e] = x.x + y.x; v[e + 1] = x.y + y.y; v[e + 2] = x.z + y.z; v[e + 3] = x.w + y.w;
  }
  *(uint4*)(out + row * width + c) = Chunk<AT>::pack(v);
}

// one wave per sequence: the first position of the largest id, then that row of x (+ b) in fp32
template <class AT>
__global__ __launch_bounds__(64) void k_eot_gather(float* __restrict__ out, const int32_t* __restrict__ ids,
                                                   const AT* __restrict__ x, const AT* __restrict__ b, int ctx, int width) {
  const int r = blockIdx.x, lane = threadIdx.x;
  const int32_t* row = ids + (size_t)r * ctx;
  int best = INT32_MIN, at = 0x7fffffff;
  for (int t = lane; t < ctx; t += 64) {                   // ascending t: a later equal id does not replace an earlier one
    const int v = row[t];
    if (at == 0x7fffffff || v > best) { best = v; at = t; }
  }
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    const int ob = __shfl_xor(best, o, 64), oa = __shfl_xor(at, o, 64);
    if (oa != 0x7fffffff && (at == 0x7fffffff || ob > best || (ob == best && oa < at))) { best = ob; at = oa; }
  }
  const AT* src = x + ((size_t)r * ctx + at) * width;
  const AT* src2 = b ? b + ((size_t)r * ctx + at) * width : nullptr;
  for (int c = lane; c < width; c += 64) out[(size_t)r * width + c] = to_f(src[c]) + (src2 ? to_f(src2[c]) : 0.f);
}

// BERT's embedding sum, packed rows: one thread per 16-byte chunk of the output,
//   out[row, c ..] = (word[id, c ..] + pos[t, c ..]) + type0[c ..]     fp32, one rounding; t = row - cu[r], cu[r] <= row < cu[r + 1]
// r is found by bisection in cu_seqlens (n + 1 cached ints); id and t are clamped into their tables
template <class AT>
__global__ __launch_bounds__(256) void k_bert_embed(AT* __restrict__ out, const int32_t* __restrict__ ids,
                                                    const int32_t* __restrict__ cu, const float* __restrict__ word,
                                                    const float* __restrict__ pos, const float* __restrict__ type0,
                                                    int64_t chunks, int n, int width, int vocab, int positions) {
  constexpr int CE = Chunk<AT>::N;
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (i >= chunks) return;
  const int cpr = width / CE;
  const int64_t row = i / cpr;
  const int c = (int)(i - row * cpr) * CE;
  int lo = 0, hi = n;                                        // the last r in [0, n) with cu[r] <= row
  while (hi - lo > 1) {
    const int mid = (lo + hi) >> 1;
    if (cu[mid] <= row) lo = mid; else hi = mid;
  }
  int64_t t = row - cu[lo];
  t = t < 0 ? 0 : (t >= positions ? positions - 1 : t);     // no position reads outside the table
  int id = ids[row];
  id = id < 0 ? 0 : (id >= vocab ? vocab - 1 : id);
  const float* a = word + (size_t)id * width + c;
  const float* b = pos + (size_t)t * width + c;
  float v[CE];
#pragma unroll
  for (int e = 0; e < CE; e += 4) {
    const float4 x = *(const float4*)(a + e), y = *(const float4*)(b + e), z = *(const float4*)(type0 + c + e);
    v[e] = (x.x + y.x) + z.x; v[e + 1] = (x.y + y.y) + z.y; v[e + 2] = (x.z + y.z) + z.z; v[e + 3] = (x.w + y.w) + z.w;
  }
  *(uint4*)(out + row * width + c) = Chunk<AT>::pack(v);
}

// one wave per sequence: the [CLS] row cu[r] of x (+ b) in fp32; the row is clamped into [0, total)
template <class AT>
__global__ __launch_bounds__(64) void k_cls_gather(float* __restrict__ out, const int32_t* __restrict__ cu,
                                                   const AT* __restrict__ x, const AT* __restrict__ b, int total, int width) {
  const int r = blockIdx.x, lane = threadIdx.x;
  int at = cu[r];
  at = at < 0 ? 0 : (at >= total ? total - 1 : at);
  const AT* src = x + (size_t)at * width;
  const AT* src2 = b ? b + (size_t)at * width : nullptr;
  for (int c = lane; c < width; c += 64) out[(size_t)r * width + c] = to_f(src[c]) + (src2 ? to_f(src2[c]) : 0.f);
}

// ---------------------------------------------------------------------------------------------- spec
struct TextCfg {
  int vocab, ctx, width, heads, layers, embed;
  float eps = 1e-5f;
  int act = 4;        // MLP activation (ConvEpi::act): 4 QuickGELU (CLIP), 1 exact GELU (BERT)
  int causal = 1;     // attention mask: 1 causal over whole contexts (CLIP); 0 BERT's key-padding mask, as packed sequences
  int post_ln = 0;    // 0: pre-LN residual block (CLIP); 1: post-LN (BERT)
  int type_vocab = 0; // rows of BERT's token-type table (row 0 is the only one used: the reference passes no token_type_ids)
};
bool bert_cfg(TextCfg& c, int vocab, int ctx, int width, int heads, int layers) {
  c = {vocab, ctx, width, heads, layers, width};            // the feature is the [CLS] row itself
  c.eps = 1e-12f; c.act = 1; c.causal = 0; c.post_ln = 1; c.type_vocab = 2;
  return true;
}
bool get_text_cfg(const char* v, TextCfg& c) {
  if (!strcmp(v, "clip_text_b32")) { c = {49408, 77, 512, 8, 12, 512}; return true; }   // clip/model.py CLIP(512, ..., 77, 49408, 512, 8, 12)
  // build-defined miniatures (tests): the real context; one row past a 32-row tile with a single head
  if (!strcmp(v, "clip_text_micro")) { c = {512, 77, 128, 2, 2, 24}; return true; }
  if (!strcmp(v, "clip_text_nano")) { c = {64, 33, 64, 1, 2, 8}; return true; }
  if (!strcmp(v, "bert_base_uncased")) return bert_cfg(c, 30522, 512, 768, 12, 12);        // transformers BertConfig()
  // build-defined miniatures (tests): the real position table with two heads; 40 positions with a single head
  if (!strcmp(v, "bert_micro")) return bert_cfg(c, 512, 512, 128, 2, 2);
  if (!strcmp(v, "bert_nano")) return bert_cfg(c, 64, 40, 64, 1, 2);
  return false;
}

struct TParam { std::string name; int64_t shape[4]; int ndim; int64_t offset, numel, res; };   // res: offset in the resident copy, -1 = a packed linear
struct TLin { int cin, cout; int64_t off_w, off_p; const float* bias = nullptr; int64_t res_b; };
struct TBlk { int qkv, proj, fc1, fc2; int64_t ln1_w, ln1_b, ln2_w, ln2_b; };
struct TArena {
  int64_t cur = 0;
  int64_t take(int64_t bytes) { int64_t o = cur; cur += (bytes + 255) / 256 * 256; return o; }
};

}  // namespace

struct mdd_text_tower {
  TextCfg c;
  int max_batch = 0, dtype = 0;
  int64_t max_tokens = 0;            // token rows the workspace is planned for
  std::vector<TParam> params;
  int64_t P = 0;
  virtual ~mdd_text_tower() {}
  virtual int64_t workspace_bytes() const = 0;
  virtual int bind(void* ws, int64_t bytes, hipStream_t st) = 0;
  virtual int load(const float* theta, hipStream_t st) = 0;
  virtual int encode(const int32_t* ids, int n, float* out, hipStream_t st) = 0;
  virtual int encode_varlen(const int32_t* ids, const int32_t* cu, int n, int total, int max_len, float* out,
                            hipStream_t st) = 0;
};

namespace {

template <class AT>
struct Tower : mdd_text_tower {
  static constexpr int DT = sizeof(AT) == 4 ? MDD_DTYPE_F32 : MDD_DTYPE_BF16;
  std::vector<TLin> lins;
  std::vector<TBlk> blks;
  std::vector<LinPackDesc> lpd;
  int lpd_tiles = 0;
  int64_t packed_total = 0, res_total = 0;
  int64_t r_pos = 0, r_proj = 0, r_tok = 0, r_lnf_w = 0, r_lnf_b = 0, r_type = 0;
  bool fused_act = false;
  // workspace
  int64_t ws_bytes = 0, o_res = 0, o_wf = 0, o_lpd = 0, o_un = 0, o_eot = 0, o_hin = 0;
  int64_t o_X = 0, o_X2 = 0, o_N = 0, o_O = 0, o_TMP = 0, o_QKV = 0, o_A = 0, o_C = 0;
  char* base = nullptr;
  bool loaded = false;
  float* res = nullptr; AT* wf = nullptr; LinPackDesc* d_lpd = nullptr;
  AT *X = nullptr, *X2 = nullptr, *Nn = nullptr, *O = nullptr, *TMP = nullptr, *QKV = nullptr, *A = nullptr, *C = nullptr;
  float *eot = nullptr, *hin = nullptr;

  int64_t add_param(const std::string& name, std::initializer_list<int64_t> shape, bool resident) {
    TParam p; p.name = name; p.ndim = (int)shape.size(); p.numel = 1;
    int i = 0;
    for (auto s : shape) { p.shape[i++] = s; p.numel *= s; }
    for (; i < 4; ++i) p.shape[i] = 1;
    p.offset = P; P += p.numel;
    p.res = -1;
    if (resident) { p.res = res_total; res_total += (p.numel + 63) / 64 * 64; }    // 256-byte rows: float4 loads of any of them
    params.push_back(p);
    return resident ? p.res : p.offset;
  }
  int add_lin(const std::string& wname, const std::string& bname, int cin, int cout) {
    TLin L; L.cin = cin; L.cout = cout;
    L.off_w = add_param(wname, {cout, cin}, false);
    L.res_b = add_param(bname, {cout}, true);
    L.off_p = packed_total; packed_total += (int64_t)cin * cout;
    lins.push_back(L);
    return (int)lins.size() - 1;
  }
  // BERT's query, key and value linears as ONE [3 D, D] contraction: the three weights lie next to each other in the flat
  // vector (one pack descriptor), and so do the three biases in the resident copy (D is a multiple of its 64-float rows)
  int add_qkv(const std::string& pre, int D) {
    TLin L; L.cin = D; L.cout = 3 * D;
    L.off_w = add_param(pre + "query.weight", {D, D}, false);
    add_param(pre + "key.weight", {D, D}, false); add_param(pre + "value.weight", {D, D}, false);
    L.res_b = add_param(pre + "query.bias", {D}, true);
    add_param(pre + "key.bias", {D}, true); add_param(pre + "value.bias", {D}, true);
    L.off_p = packed_total; packed_total += (int64_t)3 * D * D;
    lins.push_back(L);
    return (int)lins.size() - 1;
  }
  int build(const mdd_text_tower_config& cfg) {
    CHECK_ARG(get_text_cfg(cfg.variant, c), "unknown text tower variant (clip_text_b32 | clip_text_micro | clip_text_nano | "
                                            "bert_base_uncased | bert_micro | bert_nano)");
    CHECK_ARG(cfg.max_batch >= 1, "max_batch must be at least 1");
    CHECK_ARG(cfg.max_tokens >= 0, "max_tokens must not be negative (0 = max_batch * context)");
    CHECK_ARG((c.causal == 1 && c.post_ln == 0 && c.act == 4) || (c.causal == 0 && c.post_ln == 1 && c.act == 1),
              "internal: the pre-LN causal QuickGELU tower (CLIP) and the post-LN packed GELU tower (BERT) are built");
    max_batch = cfg.max_batch; dtype = cfg.dtype;
    // CLIP computes whole contexts: its rows are max_batch * context whatever max_tokens says
    max_tokens = c.post_ln && cfg.max_tokens > 0 ? cfg.max_tokens : (int64_t)max_batch * c.ctx;
    const int D = c.width, ce = 16 / (int)sizeof(AT);
    CHECK_ARG(D == c.heads * 64, "internal: the attention kernels take head dimension 64");
    CHECK_ARG(c.ctx >= 1 && c.ctx <= (c.causal ? 128 : 512), "internal: the causal attention takes at most 128 tokens, the packed one 512");
    CHECK_ARG(D % ce == 0 && D / ce <= 256, "internal: width must be whole 16-byte chunks, at most 256 of them");
    // the contraction kernel indexes its output with 32-bit element offsets
    if (c.post_ln) CHECK_ARG(max_tokens * 4 * D < (1ll << 31), "max_tokens * 4 * width must stay below 2^31 elements");
    else CHECK_ARG((int64_t)max_batch * c.ctx * 4 * D < (1ll << 31), "max_batch * context * 4 * width must stay below 2^31 elements");
    if (c.post_ln) build_bert_table(); else {
    // the `clip` package's names (CLIP.named_parameters order, the text tower's entries of it), under "model."
    const std::string m = "model.";
    r_pos = add_param(m + "positional_embedding", {c.ctx, D}, true);
    r_proj = add_param(m + "text_projection", {D, c.embed}, true);
    for (int l = 0; l < c.layers; ++l) {
      const std::string pre = m + "transformer.resblocks." + std::to_string(l);
      TBlk B;
      B.qkv = add_lin(pre + ".attn.in_proj_weight", pre + ".attn.in_proj_bias", D, 3 * D);
      B.proj = add_lin(pre + ".attn.out_proj.weight", pre + ".attn.out_proj.bias", D, D);
      B.ln1_w = add_param(pre + ".ln_1.weight", {D}, true); B.ln1_b = add_param(pre + ".ln_1.bias", {D}, true);
      B.fc1 = add_lin(pre + ".mlp.c_fc.weight", pre + ".mlp.c_fc.bias", D, 4 * D);
      B.fc2 = add_lin(pre + ".mlp.c_proj.weight", pre + ".mlp.c_proj.bias", 4 * D, D);
      B.ln2_w = add_param(pre + ".ln_2.weight", {D}, true); B.ln2_b = add_param(pre + ".ln_2.bias", {D}, true);
      blks.push_back(B);
    }
    r_tok = add_param(m + "token_embedding.weight", {c.vocab, D}, true);
    r_lnf_w = add_param(m + "ln_final.weight", {D}, true); r_lnf_b = add_param(m + "ln_final.bias", {D}, true);
    }
    int64_t tiles = 0;
    for (auto& L : lins) lpd.push_back(lin_pack_desc(L.cout, L.cin, L.off_w, L.off_p, tiles));
    CHECK_ARG(tiles <= 2147483647ll, "too many tiles");
    lpd_tiles = (int)tiles;
    fused_act = conv_gemm_supports_gelu(geom(lins[blks[0].fc1], 1));
    // ---- workspace plan
    TArena a;
    const int64_t M = max_tokens, es = sizeof(AT);
    o_res = a.take(res_total * 4);
    o_wf = a.take(packed_total * es);
    o_lpd = a.take((int64_t)lpd.size() * sizeof(LinPackDesc));
    o_eot = a.take((int64_t)max_batch * D * 4);
    o_hin = a.take((int64_t)max_batch * D * 4);
    // the transposed pack k_lin_pack_all also writes is used by no forward contraction: it shares the activations' memory
    o_un = a.cur;
    o_X = a.take(M * D * es); o_X2 = a.take(M * D * es); o_N = a.take(M * D * es); o_O = a.take(M * D * es);
    o_TMP = a.take(M * D * es); o_QKV = a.take(M * 3 * D * es); o_A = a.take(M * 4 * D * es);
    o_C = fused_act ? -1 : a.take(M * 4 * D * es);
    if (a.cur - o_un < packed_total * es) { a.cur = o_un; a.take(packed_total * es); }
    ws_bytes = a.cur;
    return 0;
  }
  // transformers' names (BertModel.named_parameters, bare), every parameter but pooler.*; query / key / value adjacent
  void build_bert_table() {
    const int D = c.width;
    const std::string e = "embeddings.";
    r_tok = add_param(e + "word_embeddings.weight", {c.vocab, D}, true);
    r_pos = add_param(e + "position_embeddings.weight", {c.ctx, D}, true);
    r_type = add_param(e + "token_type_embeddings.weight", {c.type_vocab, D}, true);
    r_lnf_w = add_param(e + "LayerNorm.weight", {D}, true); r_lnf_b = add_param(e + "LayerNorm.bias", {D}, true);   // LN_emb
    for (int l = 0; l < c.layers; ++l) {
      const std::string pre = "encoder.layer." + std::to_string(l) + ".";
      TBlk B;
      B.qkv = add_qkv(pre + "attention.self.", D);
      B.proj = add_lin(pre + "attention.output.dense.weight", pre + "attention.output.dense.bias", D, D);
      B.ln1_w = add_param(pre + "attention.output.LayerNorm.weight", {D}, true);
      B.ln1_b = add_param(pre + "attention.output.LayerNorm.bias", {D}, true);
      B.fc1 = add_lin(pre + "intermediate.dense.weight", pre + "intermediate.dense.bias", D, 4 * D);
      B.fc2 = add_lin(pre + "output.dense.weight", pre + "output.dense.bias", 4 * D, D);
      B.ln2_w = add_param(pre + "output.LayerNorm.weight", {D}, true);
      B.ln2_b = add_param(pre + "output.LayerNorm.bias", {D}, true);
      blks.push_back(B);
    }
  }
  ConvGeom geom(const TLin& L, int rows) const {
    ConvGeom g; g.nimg = rows; g.ha = 1; g.wa = 1; g.ca_tot = L.cin; g.ho = 1; g.wo = 1; g.co_tot = L.cout; g.kc = L.cin;
    g.nc = L.cout; g.groups = 1; g.k = 1; g.stride = 1; g.pad = 0; g.transposed = 0; g.prec = 0; return g;
  }
  int64_t workspace_bytes() const override { return ws_bytes; }
  int bind(void* ws, int64_t bytes, hipStream_t st) override {
    CHECK_ARG(ws && bytes >= ws_bytes, "workspace too small");
    CHECK_ARG(((uintptr_t)ws & 255) == 0, "workspace must be 256-byte aligned");
    base = (char*)ws; loaded = false;
    res = (float*)(base + o_res); wf = (AT*)(base + o_wf); d_lpd = (LinPackDesc*)(base + o_lpd);
    eot = (float*)(base + o_eot); hin = (float*)(base + o_hin);
    X = (AT*)(base + o_X); X2 = (AT*)(base + o_X2); Nn = (AT*)(base + o_N); O = (AT*)(base + o_O); TMP = (AT*)(base + o_TMP);
    QKV = (AT*)(base + o_QKV); A = (AT*)(base + o_A); C = o_C >= 0 ? (AT*)(base + o_C) : nullptr;
    for (auto& L : lins) L.bias = res + L.res_b;
    HIP_CHECK_RET(hipMemcpyAsync(d_lpd, lpd.data(), lpd.size() * sizeof(LinPackDesc), hipMemcpyHostToDevice, st));
    HIP_CHECK_RET(hipStreamSynchronize(st));   // lpd.data() is host memory
    return 0;
  }
  int load(const float* theta, hipStream_t st) override {
    CHECK_ARG(base, "no workspace bound");
    CHECK_ARG(theta, "null theta");
    // the padding between two resident parameters is never read
    for (auto& p : params)
      if (p.res >= 0)
        HIP_CHECK_RET(hipMemcpyAsync(res + p.res, theta + p.offset, (size_t)p.numel * 4, hipMemcpyDeviceToDevice, st));
    launch_lin_pack_all<AT>(d_lpd, (int)lpd.size(), lpd_tiles, theta, nullptr, wf, (AT*)(base + o_un), nullptr, nullptr, st);
    POST_LAUNCH("text_tower_load");
    loaded = true;
    return 0;
  }
  void lin(const TLin& L, int rows, const AT* in, AT* raw, AT* act_out, int act, hipStream_t st) {
    ConvEpi e; memset(&e, 0, sizeof e);
    e.mode = EPI_FWD; e.bias = L.bias; e.out_raw = raw; e.out_act = act_out; e.beta = 1.f; e.act = act;
    launch_conv_gemm<AT>(geom(L, rows), in, wf + L.off_p, nullptr, nullptr, e, st);
  }
#define TT_RC(expr) do { int rc_ = (expr); if (rc_) return rc_; } while (0)
  int encode(const int32_t* ids, int n, float* out, hipStream_t st) override {
    CHECK_ARG(!c.post_ln, "a BERT tower takes packed sequences: mdd_text_tower_encode_varlen");
    CHECK_ARG(loaded, "mdd_text_tower_load has not run on this workspace");
    CHECK_ARG(ids && out, "null pointer");
    CHECK_ARG(n >= 1 && n <= max_batch, "n must be in [1, max_batch]");
    const int D = c.width, M = n * c.ctx;
    const float scale = 1.f / std::sqrt(64.f);
    TT_RC(mdd_op_token_embed(DT, n, c.ctx, D, c.vocab, ids, res + r_tok, res + r_pos, X, st));
    for (int l = 0; l < c.layers; ++l) {
      const TBlk& B = blks[l];
      // x_l = x2_{l-1} + c_proj's output (still in TMP) is formed by the kernel that normalises it
      if (l == 0) TT_RC(mdd_op_layernorm(DT, M, D, c.eps, X, nullptr, res + B.ln1_w, nullptr, res + B.ln1_b, nullptr, Nn, nullptr, st));
      else TT_RC(mdd_op_add_layernorm(DT, M, D, c.eps, X2, nullptr, TMP, nullptr, X, nullptr, res + B.ln1_w, nullptr,
                                      res + B.ln1_b, nullptr, Nn, nullptr, st));
      lin(lins[B.qkv], M, Nn, QKV, nullptr, 0, st);
      TT_RC(mdd_op_attention_causal(DT, n, c.ctx, c.heads, scale, QKV, O, st));
      lin(lins[B.proj], M, O, TMP, nullptr, 0, st);
      TT_RC(mdd_op_add_layernorm(DT, M, D, c.eps, X, nullptr, TMP, nullptr, X2, nullptr, res + B.ln2_w, nullptr,
                                 res + B.ln2_b, nullptr, Nn, nullptr, st));
      // c_fc with QuickGELU in its epilogue wherever that instance of the kernel exists for the width (the pre-activation is
      // not kept: nothing differentiates this tower)
      if (fused_act) lin(lins[B.fc1], M, Nn, nullptr, A, c.act, st);
      else {
        lin(lins[B.fc1], M, Nn, C, nullptr, 0, st);
        TT_RC(mdd_op_quick_gelu(DT, (int64_t)M * 4 * D, C, nullptr, A, nullptr, st));
      }
      lin(lins[B.fc2], M, A, TMP, nullptr, 0, st);
    }
    // the last residual sum is formed in fp32 on the gathered rows only; LayerNorm is per row, so normalising those rows
    // equals normalising every row first
    TT_RC(mdd_op_eot_gather(DT, n, c.ctx, D, ids, X2, TMP, eot, st));
    TT_RC(mdd_op_layernorm(MDD_DTYPE_F32, n, D, c.eps, eot, nullptr, res + r_lnf_w, nullptr, res + r_lnf_b, nullptr, hin,
                           nullptr, st));
    // @ text_projection, stored [width, embed]: the data-gradient form A W of the small-batch linears (the image tower's
    // output projection is done the same way)
    LinScratch ls; ls.mfma = true;
    launch_linear_dgrad(out, nullptr, hin, nullptr, res + r_proj, nullptr, nullptr, n, c.embed, D, ls, st);
    POST_LAUNCH("text_tower_encode");
    return 0;
  }
  int encode_varlen(const int32_t* ids, const int32_t* cu, int n, int total, int max_len, float* out,
                    hipStream_t st) override {
    CHECK_ARG(c.post_ln, "a CLIP tower takes whole contexts: mdd_text_tower_encode");
    CHECK_ARG(loaded, "mdd_text_tower_load has not run on this workspace");
    CHECK_ARG(ids && cu && out, "null pointer");
    CHECK_ARG(n >= 1 && n <= max_batch, "n must be in [1, max_batch]");
    CHECK_ARG(total >= n && total <= max_tokens, "total must be in [n, max_tokens]");
    CHECK_ARG(max_len >= 1 && max_len <= c.ctx, "max_len must be in [1, positions]");
    const int D = c.width, M = total;
    const float scale = 1.f / std::sqrt(64.f);
    TT_RC(mdd_op_bert_embed(DT, n, M, D, c.vocab, c.ctx, ids, cu, res + r_tok, res + r_pos, res + r_type, TMP, st));
    TT_RC(mdd_op_layernorm(DT, M, D, c.eps, TMP, nullptr, res + r_lnf_w, nullptr, res + r_lnf_b, nullptr, X, nullptr, st));
    for (int l = 0; l < c.layers; ++l) {
      const TBlk& B = blks[l];
      lin(lins[B.qkv], M, X, QKV, nullptr, 0, st);
      TT_RC(mdd_op_attention_varlen(DT, n, M, c.heads, scale, QKV, cu, max_len, O, st));
      lin(lins[B.proj], M, O, TMP, nullptr, 0, st);
      // post-LN: the residual sum is normalised in place of being carried (the sum itself, written to Nn, is not read again)
      TT_RC(mdd_op_add_layernorm(DT, M, D, c.eps, X, nullptr, TMP, nullptr, Nn, nullptr, res + B.ln1_w, nullptr,
                                 res + B.ln1_b, nullptr, X2, nullptr, st));
      if (fused_act) lin(lins[B.fc1], M, X2, nullptr, A, c.act, st);
      else {
        lin(lins[B.fc1], M, X2, C, nullptr, 0, st);
        TT_RC(mdd_op_gelu(DT, (int64_t)M * 4 * D, C, nullptr, A, nullptr, st));
      }
      lin(lins[B.fc2], M, A, TMP, nullptr, 0, st);
      if (l + 1 < c.layers)
        TT_RC(mdd_op_add_layernorm(DT, M, D, c.eps, X2, nullptr, TMP, nullptr, Nn, nullptr, res + B.ln2_w, nullptr,
                                   res + B.ln2_b, nullptr, X, nullptr, st));
    }
    // the last layer's residual sum and LayerNorm in fp32 on the n [CLS] rows only (LayerNorm is per row)
    const TBlk& L = blks[c.layers - 1];
    k_cls_gather<AT><<<(unsigned)n, 64, 0, st>>>(eot, cu, X2, TMP, M, D);
    TT_RC(mdd_op_layernorm(MDD_DTYPE_F32, n, D, c.eps, eot, nullptr, res + L.ln2_w, nullptr, res + L.ln2_b, nullptr, out,
                           nullptr, st));
    POST_LAUNCH("text_tower_encode_varlen");
    return 0;
  }
#undef TT_RC
};

}  // namespace

extern "C" {

int mdd_op_token_embed(int dtype, int n, int ctx, int width, int vocab, const int32_t* ids, const float* table,
                       const float* pos, void* out, void* stream) {
  CHECK_STORAGE(dtype);
  CHECK_ARG(n >= 1 && ctx >= 1 && width >= 1 && vocab >= 1 && ids && table && pos && out, "null pointer / empty problem");
  const int ce = dtype == MDD_DTYPE_F32 ? 4 : 8;
  CHECK_ARG(width % ce == 0, "width must be a multiple of the 16-byte chunk");
  const int64_t chunks = (int64_t)n * ctx * (width / ce);
  CHECK_ARG((chunks + 255) / 256 <= 2147483647ll, "too many rows");
  with_storage(dtype, [&](auto* tag) {
    using AT = tag_t<decltype(tag)>;
    k_token_embed<AT><<<(unsigned)((chunks + 255) / 256), 256, 0, (hipStream_t)stream>>>((AT*)out, ids, table, pos, chunks, ctx,
                                                                                         width, vocab);
  });
  POST_LAUNCH("op_token_embed");
  return 0;
}

int mdd_op_bert_embed(int dtype, int n, int total, int width, int vocab, int positions, const int32_t* ids,
                      const int32_t* cu_seqlens, const float* word, const float* pos, const float* type0, void* out,
                      void* stream) {
  CHECK_STORAGE(dtype);
  CHECK_ARG(n >= 1 && total >= n && width >= 1 && vocab >= 1 && positions >= 1, "empty problem");
  CHECK_ARG(ids && cu_seqlens && word && pos && type0 && out, "null pointer");
  const int ce = dtype == MDD_DTYPE_F32 ? 4 : 8;
  CHECK_ARG(width % ce == 0, "width must be a multiple of the 16-byte chunk");
  const int64_t chunks = (int64_t)total * (width / ce);
  CHECK_ARG((chunks + 255) / 256 <= 2147483647ll, "too many rows");
  with_storage(dtype, [&](auto* tag) {
    using AT = tag_t<decltype(tag)>;
    k_bert_embed<AT><<<(unsigned)((chunks + 255) / 256), 256, 0, (hipStream_t)stream>>>((AT*)out, ids, cu_seqlens, word, pos,
                                                                                        type0, chunks, n, width, vocab, positions);
  });
  POST_LAUNCH("op_bert_embed");
  return 0;
}

int mdd_op_eot_gather(int dtype, int n, int ctx, int width, const int32_t* ids, const void* x, const void* b, float* out,
                      void* stream) {
  CHECK_STORAGE(dtype);
  CHECK_ARG(n >= 1 && ctx >= 1 && width >= 1 && ids && x && out, "null pointer / empty problem");
  with_storage(dtype, [&](auto* tag) {
    using AT = tag_t<decltype(tag)>;
    k_eot_gather<AT><<<(unsigned)n, 64, 0, (hipStream_t)stream>>>(out, ids, (const AT*)x, (const AT*)b, ctx, width);
  });
  POST_LAUNCH("op_eot_gather");
  return 0;
}

size_t mdd_sizeof_text_tower_config(void) { return sizeof(mdd_text_tower_config); }
int mdd_text_tower_create(const mdd_text_tower_config* cfg, mdd_text_tower** out) {
  CHECK_ARG(cfg && out && cfg->variant, "null config");
  *out = nullptr;
  CHECK_STORAGE(cfg->dtype);
  int rc = 0;
  with_storage(cfg->dtype, [&](auto* tag) {
    auto* t = new Tower<tag_t<decltype(tag)>>();
    rc = t->build(*cfg);
    if (rc) delete t; else *out = t;
  });
  return rc;
}
void mdd_text_tower_destroy(mdd_text_tower* t) { delete t; }
int64_t mdd_text_tower_param_numel(const mdd_text_tower* t) { return t ? t->P : -1; }
int mdd_text_tower_param_count(const mdd_text_tower* t) { return t ? (int)t->params.size() : -1; }
int mdd_text_tower_param_info(const mdd_text_tower* t, int index, char* name, int name_cap, int64_t* shape4, int* ndim,
                              int64_t* offset) {
  CHECK_ARG(t, "null tower");
  CHECK_ARG(index >= 0 && index < (int)t->params.size(), "param index");
  const TParam& p = t->params[index];
  if (name && name_cap > 0) { strncpy(name, p.name.c_str(), name_cap - 1); name[name_cap - 1] = 0; }
  if (shape4) memcpy(shape4, p.shape, sizeof p.shape);
  if (ndim) *ndim = p.ndim;
  if (offset) *offset = p.offset;
  return 0;
}
int mdd_text_tower_feature_dim(const mdd_text_tower* t) { return t ? t->c.embed : -1; }
int mdd_text_tower_context(const mdd_text_tower* t) { return t ? t->c.ctx : -1; }
int mdd_text_tower_vocab(const mdd_text_tower* t) { return t ? t->c.vocab : -1; }
int64_t mdd_text_tower_workspace_bytes(const mdd_text_tower* t) { return t ? t->workspace_bytes() : -1; }
int mdd_text_tower_bind_workspace(mdd_text_tower* t, void* ws_dev, int64_t bytes, void* stream) {
  CHECK_ARG(t, "null tower");
  return t->bind(ws_dev, bytes, (hipStream_t)stream);
}
int mdd_text_tower_load(mdd_text_tower* t, const float* theta_dev, void* stream) {
  CHECK_ARG(t, "null tower");
  return t->load(theta_dev, (hipStream_t)stream);
}
int mdd_text_tower_encode(mdd_text_tower* t, const int32_t* ids_dev, int n, float* out_dev, void* stream) {
  CHECK_ARG(t, "null tower");
  return t->encode(ids_dev, n, out_dev, (hipStream_t)stream);
}

int mdd_text_tower_encode_varlen(mdd_text_tower* t, const int32_t* ids_packed_dev, const int32_t* cu_seqlens_dev, int n,
                                 int total, int max_len, float* out_dev, void* stream) {
  CHECK_ARG(t, "null tower");
  return t->encode_varlen(ids_packed_dev, cu_seqlens_dev, n, total, max_len, out_dev, (hipStream_t)stream);
}

}  // extern "C"
