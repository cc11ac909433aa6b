// The stateless entry points of libmdd_hip.so: `mdd_op_*` (one kernel family each, what the parity tests drive),
// `mdd_flat_*` (the fp32 theta-vector kernels), the evaluation kernels and the run-time kernel switches.  None of them
// takes an mdd_engine: each checks its arguments and calls the launchers the engine (engine.hip) itself calls.  The
// transformer operators' entries sit beside their kernels in vit.hip and attn.hip.
#include <hip/hip_runtime.h>

#include <cstring>
#include <vector>

#include "kernels.h"
#include "philox.h"
#include "mdd_hip.h"

extern "C" {

int mdd_set_pipe_kernels(int enable) {
  const int prev = pipe_kernels_enabled() ? 1 : 0;
  set_pipe_kernels(enable != 0);
  return prev;
}

int mdd_set_group8_kernels(int enable) {
  const int prev = group8_kernels_mode();
  set_group8_kernels(enable);
  return prev;
}

int mdd_op_dropout_mask(float p, uint64_t seed, uint32_t step, uint32_t iteration, int n, int d, const int64_t* idx,
                        float* out, void* stream) {
  CHECK_ARG(out && n >= 1 && d >= 1, "null pointer or empty shape");
  CHECK_ARG(drop_p_valid(p), "p must lie in [0, 1)");
  launch_dropout_mask(out, drop_spec(p, seed, step, iteration, idx), n, d, (hipStream_t)stream);
  POST_LAUNCH("op_dropout_mask");
  return 0;
}
int64_t mdd_op_contrastive_workspace_floats(int n, int d) { return loss_work_floats(n, d); }
int mdd_op_contrastive(int n, int d, const float* x, const float* y, const float* xd, const float* yd,
                       const float* scale_dev, float scale_const, float* work, float* loss, float* xbar,
                       float* ybar, float* sbar, void* stream) {
  CHECK_ARG(n > 0 && d > 0 && x && y && work && xbar && ybar && sbar, "null pointer / empty problem");
  CHECK_ARG((xd == nullptr) == (yd == nullptr), "x_dot and y_dot come together");
  CHECK_ARG(xd || loss, "loss output is null");
  CHECK_CONTRASTIVE(n, d);
  LossWork w = loss_work_carve(work, n, d);
  if (!xd) launch_contrastive(w, loss, xbar, ybar, sbar, nullptr, nullptr, nullptr, x, y, nullptr, nullptr,
                              scale_dev, scale_const, n, d, (hipStream_t)stream);
  else launch_contrastive(w, nullptr, nullptr, nullptr, nullptr, xbar, ybar, sbar, x, y, xd, yd, scale_dev,
                          scale_const, n, d, (hipStream_t)stream);
  POST_LAUNCH("op_contrastive");
  return 0;
}

// ---- the fp32 theta-vector kernels (flat_ops.hip)
int mdd_flat_axpy(float* out, const float* x, const float* g, const float* lr, float sign,
                  int64_t n, void* stream) {
  CHECK_ARG(out && x && g && lr && n >= 0, "null pointer");
  launch_axpy_out(out, x, g, lr, sign, n, (hipStream_t)stream);
  POST_LAUNCH("axpy");
  return 0;
}
int mdd_flat_sqdist(const float* a, const float* b, double* out, int64_t n, void* stream) {
  CHECK_ARG(a && b && out && n >= 0, "null pointer");
  launch_sqdist(a, b, out, n, (hipStream_t)stream);
  POST_LAUNCH("sqdist");
  return 0;
}
int mdd_flat_sgd_momentum(float* p, const float* g, float* buf, float lr, float mom, int first,
                          int64_t n, void* stream) {
  CHECK_ARG(p && g && buf && n >= 0, "null pointer");
  launch_sgd_momentum(p, g, buf, lr, mom, first, n, nullptr, (hipStream_t)stream);
  POST_LAUNCH("sgd");
  return 0;
}
int mdd_flat_sgd_momentum_guarded(float* p, const float* g, float* buf, float lr, float mom, int first,
                                  int64_t n, const float* skip_flag, void* stream) {
  CHECK_ARG(p && g && buf && skip_flag && n >= 0, "null pointer");
  launch_sgd_momentum(p, g, buf, lr, mom, first, n, skip_flag, (hipStream_t)stream);
  POST_LAUNCH("sgd_guarded");
  return 0;
}
int mdd_flat_dot(const float* a, const float* b, double* out, double sign, int64_t n, void* stream) {
  CHECK_ARG(a && b && out && n >= 0, "null pointer");
  launch_dot(a, b, out, sign, n, (hipStream_t)stream);
  POST_LAUNCH("dot");
  return 0;
}
int mdd_flat_scale_out(float* y, const float* x, const float* coef, float mul, int64_t n, void* stream) {
  CHECK_ARG(y && x && n >= 0, "null pointer");
  launch_scale_out(y, x, coef, mul, n, (hipStream_t)stream);
  POST_LAUNCH("scale_out");
  return 0;
}
int mdd_flat_sub_inplace(float* y, const float* x, int64_t n, void* stream) {
  CHECK_ARG(y && x && n >= 0, "null pointer");
  launch_sub_inplace(y, x, n, (hipStream_t)stream);
  POST_LAUNCH("sub_inplace");
  return 0;
}
int mdd_flat_lambda_init(float* lam, const float* thK, const float* tgt, const double* dist0, int64_t n, void* stream) {
  CHECK_ARG(lam && thK && tgt && dist0 && n >= 0, "null pointer");
  launch_lambda_init(lam, thK, tgt, dist0, n, (hipStream_t)stream);
  POST_LAUNCH("lambda_init");
  return 0;
}
int mdd_flat_match_finalize(const double* s4, float* out3, void* stream) {
  CHECK_ARG(s4 && out3, "null pointer");
  launch_match_finalize(s4, out3, (hipStream_t)stream);
  POST_LAUNCH("match_finalize");
  return 0;
}
int mdd_flat_d2f(float* out, const double* in, float mul, int accum, int n, void* stream) {
  CHECK_ARG(out && in, "null pointer");
  CHECK_ARG(n >= 1 && n <= 64, "d2f hands over at most 64 scalars (one wave)");
  launch_d2f(out, in, mul, accum, n, (hipStream_t)stream);
  POST_LAUNCH("d2f");
  return 0;
}
int mdd_flat_accum_f2d(double* out, const float* in, double sign, void* stream) {
  CHECK_ARG(out && in, "null pointer");
  launch_accum_f2d(out, in, sign, (hipStream_t)stream);
  POST_LAUNCH("accum_f2d");
  return 0;
}

// ---- convolutions
static ConvGeom op_geom(int dtype, int transposed, int nimg, int hin, int win, int cin, int cout, int k,
                        int stride, int pad, int groups) {
  int hout = (hin + 2 * pad - k) / stride + 1, wout = (win + 2 * pad - k) / stride + 1;
  ConvGeom g;
  g.nimg = nimg; g.groups = groups; g.k = k; g.stride = stride; g.pad = pad; g.transposed = transposed;
  g.prec = op_prec(dtype);
  if (!transposed) {
    g.ha = hin; g.wa = win; g.ca_tot = cin; g.ho = hout; g.wo = wout; g.co_tot = cout;
    g.kc = cin / groups; g.nc = cout / groups;
  } else {
    g.ha = hout; g.wa = wout; g.ca_tot = cout; g.ho = hin; g.wo = win; g.co_tot = cin;
    g.kc = cout / groups; g.nc = cin / groups;
  }
  return g;
}
int mdd_op_conv2d(int dtype, int transposed, int nimg, int hin, int win, int cin, int cout, int k,
                  int stride, int pad, int groups, const void* a, const void* w, const float* bias,
                  void* out, void* stream) {
  CHECK_ARG(a && w && out, "null pointer");
  CHECK_ARG(dtype >= 0 && dtype <= 3, "dtype");
  CHECK_ARG(stride == 1 || stride == 2, "stride must be 1 or 2");
  const ConvGeom g = op_geom(dtype, transposed, nimg, hin, win, cin, cout, k, stride, pad, groups);
  ConvEpi e; memset(&e, 0, sizeof e);
  e.mode = transposed ? EPI_BWD_LIN : EPI_FWD; e.bias = bias; e.out_raw = out; e.beta = 1.f;
  with_storage(dtype, [&](auto* tag) {
    using AT = tag_t<decltype(tag)>;
    launch_conv_gemm<AT>(g, (const AT*)a, (const AT*)w, nullptr, nullptr, e, (hipStream_t)stream);
  });
  POST_LAUNCH("op_conv2d");
  return 0;
}
int mdd_op_conv2d_wgrad(int dtype, int nimg, int hin, int win, int cin, int cout, int k, int stride,
                        int pad, int groups, const void* dy, const void* x, float* dw, float* db,
                        void* stream) {
  CHECK_ARG(dy && x && dw, "null pointer");
  CHECK_ARG(dtype >= 0 && dtype <= 3, "dtype");
  const ConvGeom g = op_geom(dtype, 0, nimg, hin, win, cin, cout, k, stride, pad, groups);
  with_storage(dtype, [&](auto* tag) {
    using AT = tag_t<decltype(tag)>;
    launch_conv_wgrad<AT>(g, (const AT*)dy, (const AT*)x, nullptr, nullptr, dw, db, nullptr, 0, nullptr, (hipStream_t)stream);
  });
  POST_LAUNCH("op_conv2d_wgrad");
  return 0;
}
int mdd_op_conv2d_wgrad2(int dtype, int nimg, int hin, int win, int cin, int cout, int k, int stride,
                         int pad, int groups, const void* dy1, const void* x1, const void* dy2, const void* x2,
                         float* dw, float* db, float* ws, long long ws_floats, void* stream) {
  CHECK_ARG(dy1 && x1 && dw, "null pointer");
  CHECK_ARG((dy2 == nullptr) == (x2 == nullptr), "the second pair is given whole or not at all");
  CHECK_ARG(dtype >= 0 && dtype <= 3, "dtype");
  CHECK_ARG(ws_floats >= 0 && (ws != nullptr || ws_floats == 0), "workspace");
  const ConvGeom g = op_geom(dtype, 0, nimg, hin, win, cin, cout, k, stride, pad, groups);
  with_storage(dtype, [&](auto* tag) {
    using AT = tag_t<decltype(tag)>;
    launch_conv_wgrad<AT>(g, (const AT*)dy1, (const AT*)x1, (const AT*)dy2, (const AT*)x2, dw, db, ws, (int64_t)ws_floats,
                          nullptr, (hipStream_t)stream);
  });
  POST_LAUNCH("op_conv2d_wgrad2");
  return 0;
}

// ---- NF-ResNet / NF-RegNet / NFNet block kernels
int mdd_op_maxpool2d_3s2(int dtype, int mode, int n, int h, int w, int c, const void* x, void* y, void* idx,
                         void* stream) {
  CHECK_ARG(x && y && idx, "null pointer");
  CHECK_ARG(n > 0 && h > 0 && w > 0 && c > 0, "empty problem");
  CHECK_STORAGE(dtype);
  CHECK_ARG(mode >= 0 && mode <= 2, "mode must be 0 (forward), 1 (tangent) or 2 (backward)");
  CHECK_ARG(c % (dtype == MDD_DTYPE_F32 ? 4 : 8) == 0, "channels must be a multiple of the 16-byte chunk");
  hipStream_t st = (hipStream_t)stream;
  uint8_t* ix = (uint8_t*)idx;
  with_storage(dtype, [&](auto* tag) {
    using AT = tag_t<decltype(tag)>;
    if (mode == 0) launch_maxpool3s2<AT>((AT*)y, ix, nullptr, (const AT*)x, 1.f, n, h, w, c, st);
    else if (mode == 1) launch_maxpool3s2_t<AT>((AT*)y, nullptr, nullptr, ix, (const AT*)x, 1.f, n, h, w, c, st);
    else launch_maxpool3s2_bwd<AT>((AT*)y, (const AT*)x, ix, n, h, w, c, st);
  });
  POST_LAUNCH("op_maxpool2d_3s2");
  return 0;
}

int mdd_op_mid_se(int dtype, int mode, int n, int hw, int c, float ga, const void* c2, const void* c2_t, const float* gate,
                  const float* gate_t, const void* a3bar, const void* a3bar_t, const float* qbar, void* out, void* out_t,
                  float* zbar, float* zbar_t, void* stream) {
  CHECK_ARG(c2 && gate && out, "null pointer");
  CHECK_ARG(n > 0 && hw > 0 && c > 0, "empty problem");
  CHECK_STORAGE(dtype);
  CHECK_ARG(mode == 0 || mode == 1, "mode must be 0 (forward) or 1 (backward)");
  CHECK_ARG(c % (dtype == MDD_DTYPE_F32 ? 4 : 8) == 0, "channels must be a multiple of the 16-byte chunk");
  const bool T = c2_t != nullptr;
  CHECK_ARG(T == (gate_t != nullptr) && T == (out_t != nullptr), "tangent operands come together");
  CHECK_ARG(mode == 0 || (a3bar && zbar && T == (a3bar_t != nullptr) && T == (zbar_t != nullptr)), "backward operands");
  hipStream_t st = (hipStream_t)stream;
  with_storage(dtype, [&](auto* tag) {
    using AT = tag_t<decltype(tag)>;
    if (mode == 0) {
      launch_mid_se_apply<AT>((AT*)out, (AT*)out_t, (const AT*)c2, (const AT*)c2_t, gate, gate_t, ga, n, hw, c, st);
    } else {
      launch_mid_se_bwd<AT>(zbar, zbar_t, (AT*)out, (AT*)out_t, (const AT*)c2, (const AT*)c2_t, (const AT*)a3bar,
                            (const AT*)a3bar_t, gate, gate_t, ga, n, hw, c, st);
      if (qbar) launch_add_pooled<AT>(T ? (AT*)out_t : (AT*)out, qbar, 1.f / (float)hw, n, hw, c, st);
    }
  });
  POST_LAUNCH("op_mid_se");
  return 0;
}

int mdd_op_pool_se(int dtype, int op, int n, int h, int w, int c, float ga, float beta, const void* a, const void* a_t,
                   const void* b, const void* b_t, const float* v, const float* v_t, void* out, void* out_t, void* out2,
                   void* out2_t, void* stream) {
  CHECK_ARG(a && out, "null pointer");
  CHECK_ARG(n > 0 && h > 0 && w > 0 && c > 0, "empty problem");
  CHECK_STORAGE(dtype);
  CHECK_ARG(op >= 0 && op <= 8, "op");
  CHECK_ARG(c % (dtype == MDD_DTYPE_F32 ? 4 : 8) == 0, "channels must be a multiple of the 16-byte chunk");
  const bool T = a_t != nullptr;
  const bool lin = op == 0 || op >= 7;           // linear in a: the tangent is the same call on a_t
  CHECK_ARG(!lin || !(T || out_t), "ops 0, 7 and 8 have no tangent form");
  CHECK_ARG(lin || T == (out_t != nullptr), "tangent operands come together");
  CHECK_ARG(op < 3 || op > 6 || (v && T == (v_t != nullptr)), "the [n, c] operand");
  CHECK_ARG(op < 5 || op > 6 || (b && T == (b_t != nullptr)), "the second activation operand");
  CHECK_ARG(op != 5 || T || !out2_t, "se_apply: ao_t belongs to the tangent form");
  CHECK_ARG(op != 6 || (out2 && T == (out2_t != nullptr)), "gate_grad: c3bar");
  const int hw = h * w;
  hipStream_t st = (hipStream_t)stream;
  with_storage(dtype, [&](auto* tag) {
    using AT = tag_t<decltype(tag)>;
    const AT *A = (const AT*)a, *A_t = (const AT*)a_t, *B = (const AT*)b, *B_t = (const AT*)b_t;
    switch (op) {
      case 0: launch_pool_mean<AT>((float*)out, A, n, hw, c, st); break;
      case 1: case 2: launch_final_pool<AT>((float*)out, (float*)out_t, A, A_t, n, hw, c, st, op == 2); break;
      case 3: case 4: launch_final_pool_bwd<AT>((AT*)out, (AT*)out_t, v, v_t, A, A_t, n, hw, c, st, op == 4); break;
      case 5:   // the tangent form stores through ao_t alone: without it there is no activation output at all
        launch_se_apply<AT>(A, A_t, v, v_t, B, B_t, (AT*)out, (AT*)out_t, (AT*)(T && !out2_t ? nullptr : out2),
                            (AT*)out2_t, ga, beta, n, hw, c, st);
        break;
      case 6: launch_se_gate_grad_c3b<AT>((float*)out, (float*)out_t, (AT*)out2, (AT*)out2_t, A, A_t, B, B_t, v, v_t, ga, n, hw, c, st); break;
      case 7: launch_avgpool2<AT>((AT*)out, A, n, h, w, c, 2, st); break;
      default: launch_avgpool2_bwd<AT>((AT*)out, A, n, h, w, c, 2, st); break;
    }
  });
  POST_LAUNCH("op_pool_se");
  return 0;
}

int mdd_op_resid(int dtype, int op, int64_t elems, float alpha, float beta, const void* c3, const void* c3_t, const void* sc,
                 const void* sc_t, void* xo, void* xo_t, void* ao, void* ao_t, void* stream) {
  CHECK_STORAGE(dtype);
  CHECK_ARG(op >= 0 && op <= 2, "op must be 0 (ReLU), 1 (SiLU) or 2 (scale)");
  CHECK_ARG(elems > 0 && elems % (dtype == MDD_DTYPE_F32 ? 4 : 8) == 0, "elems must be a positive multiple of the 16-byte chunk");
  CHECK_ARG(c3 && xo, "null pointer");
  const bool T = c3_t != nullptr;
  if (op == 2) CHECK_ARG(!T && !sc && !sc_t && !xo_t && !ao && !ao_t, "scale: in, out");
  else {
    CHECK_ARG(sc && T == (sc_t != nullptr) && T == (xo_t != nullptr), "tangent operands come together");
    CHECK_ARG(T ? (!ao_t || ao) : !ao_t, "ao_t belongs to the tangent form, with the stashed ao");
  }
  hipStream_t st = (hipStream_t)stream;
  with_storage(dtype, [&](auto* tag) {
    using AT = tag_t<decltype(tag)>;
    // the tangent form stores through ao_t alone: without it there is no activation output at all
    AT* AO = (AT*)(T && !ao_t ? nullptr : ao);
    if (op == 0) launch_resid_relu<AT>((const AT*)c3, (const AT*)c3_t, (const AT*)sc, (const AT*)sc_t, (AT*)xo, (AT*)xo_t, AO, (AT*)ao_t, alpha, beta, elems, st);
    else if (op == 1) launch_resid_silu<AT>((const AT*)c3, (const AT*)c3_t, (const AT*)sc, (const AT*)sc_t, (AT*)xo, (AT*)xo_t, AO, (AT*)ao_t, alpha, beta, elems, st);
    else launch_scale_act<AT>((AT*)xo, (const AT*)c3, alpha, elems, st);
  });
  POST_LAUNCH("op_resid");
  return 0;
}

// ---- small-batch linears
int mdd_op_linear(int form, int route, int wdtype, int n, int k, int j, int act, float alpha, const float* x,
                  const float* x_t, const void* W, const void* W_t, const float* b, const float* b_t, const float* dy,
                  const float* dy_t, const float* relu_of, float* out, float* out_t, float* db, void* stream) {
  CHECK_ARG(form >= 0 && form <= 4, "form must be 0 (forward), 1 (dgrad), 2 (wgrad), 3 (typed forward) or 4 (wgrad, accumulating)");
  CHECK_ARG(route == 0 || route == 1, "route must be 0 (engine) or 1 (retrieval)");
  CHECK_ARG(n > 0 && k > 0 && j > 0, "empty problem");
  CHECK_ARG(out, "null output");
  CHECK_ARG(wdtype == MDD_DTYPE_F32 || (form == 3 && wdtype == MDD_DTYPE_BF16), "weights are fp32 (form 3: fp32 or bf16)");
  CHECK_ARG(act >= 0 && act <= 2 && (form == 0 || act == 0), "act is 0, 1 or 2, and belongs to form 0");
  CHECK_ARG(route == 0 || (form == 0 && act == 0 && !b && !out_t), "route 1 is the plain primal forward");
  hipStream_t st = (hipStream_t)stream;
  LinScratch ws;           // route 1: no scratch, as retrieval.hip passes it
  if (route == 0) ws.mfma = true;   // what lin_scratch_carve gives the engine (the matrix-core kernel uses no scratch)
  const float* Wf = (const float*)W;
  const float* Wf_t = (const float*)W_t;
  if (form == 0 || form == 3) {
    CHECK_ARG(x && W, "forward operands");
    CHECK_ARG(out_t || !(x_t || W_t || b_t), "tangent operands without a tangent output");
    if (form == 0) launch_linear_fwd(out, out_t, x, x_t, Wf, Wf_t, b, b_t, n, k, j, act, ws, st);
    else with_storage(wdtype, [&](auto* tag) {
      using TW = tag_t<decltype(tag)>;
      launch_linear_fwd_w<TW>(out, out_t, x, x_t, (const TW*)W, (const TW*)W_t, b, b_t, n, k, j, alpha, st);
    });
  } else if (form == 1) {
    CHECK_ARG(dy && W, "dgrad operands");
    CHECK_ARG(out_t || !(dy_t || W_t), "tangent operands without a tangent output");
    launch_linear_dgrad(out, out_t, dy, dy_t, Wf, Wf_t, relu_of, n, k, j, ws, st);
  } else {
    CHECK_ARG(dy && x && !out_t, "wgrad operands (the tangent is written to out / db)");
    if (form == 2) launch_linear_wgrad(out, db, dy, dy_t, x, x_t, n, k, j, ws, st);
    else launch_linear_wgrad_accum(out, db, dy, dy_t, x, x_t, n, k, j, st);
  }
  POST_LAUNCH("op_linear");
  return 0;
}

// ---- packed weights: the descriptors come from the builders Eng::build fills its own tables with (ws_desc_fill,
// lin_pack_desc); what differs is the parameter layout, which is the caller's
int mdd_op_weight_std(int dtype, int mode, int nconv, const mdd_ws_conv* convs, float gamma, float eps, const float* theta,
                      const float* theta_t, void* wf, void* wt, void* wf_t, void* wt_t, const float* dwf,
                      const float* dwf_t, float* gtheta, void* stream) {
  CHECK_STORAGE(dtype);
  CHECK_ARG(mode == 0 || mode == 1, "mode must be 0 (forward) or 1 (backward)");
  CHECK_ARG(nconv > 0 && convs && theta, "null pointer / empty problem");
  const bool T = theta_t != nullptr;
  if (mode == 0) {
    CHECK_ARG(T ? (wf_t && wt_t && (wf != nullptr) == (wt != nullptr)) : (wf && wt && !wf_t && !wt_t),
              "forward: wf and wt (tangent: wf_t and wt_t, the primal pair both or neither)");
    CHECK_ARG(!dwf && !dwf_t && !gtheta, "forward takes no gradient operands");
  } else {
    CHECK_ARG(dwf && gtheta && T == (dwf_t != nullptr), "backward: dwf and gtheta (tangent: dwf_t with theta_t)");
    CHECK_ARG(!wf && !wt && !wf_t && !wt_t, "backward takes no packed weights");
  }
  // theta holds {weight, gain} per conv, back to back; no bias (weight standardisation never reads it)
  std::vector<WsDesc> descs(nconv);
  int64_t off = 0, off_p = 0, row = 0, tile = 0;
  for (int i = 0; i < nconv; ++i) {
    const mdd_ws_conv& L = convs[i];
    CHECK_ARG(L.cout > 0 && L.cin > 0 && L.k > 0 && L.groups > 0 && L.cin_pad >= L.cin, "conv geometry");
    CHECK_ARG(L.cout % L.groups == 0 && L.cin % L.groups == 0 && L.cin_pad % L.groups == 0, "groups must divide the channel counts");
    const int64_t wnum = (int64_t)L.cout * (L.cin / L.groups) * L.k * L.k, off_g = off + wnum;
    const bool chunks = ws_desc_fill(descs[i], L.cout, L.cin, L.k, L.groups, L.cin_pad, off, off_g, off_g, off_p, gamma, eps,
                                     row, tile, dtype == MDD_DTYPE_F32 ? 4 : 2);
    CHECK_ARG(row <= 2147483647ll && tile <= 2147483647ll, "too many rows");
    CHECK_ARG(chunks, "channel counts must be multiples of the 16-byte chunk");
    off = off_g + L.cout; off_p += (int64_t)L.cout * L.k * L.k * (L.cin_pad / L.groups);
  }
  hipStream_t st = (hipStream_t)stream;
  return with_device_descs(descs, st, [&](const WsDesc* d_descs) {
    if (mode == 1) launch_ws_backward(d_descs, nconv, (int)row, theta, theta_t, dwf, dwf_t, gtheta, st);
    else with_storage(dtype, [&](auto* tag) {
      using AT = tag_t<decltype(tag)>;
      launch_ws_forward<AT>(d_descs, nconv, (int)row, (int)tile, theta, theta_t, (AT*)wf, (AT*)wt, (AT*)wf_t, (AT*)wt_t, st);
    });
  });
}

int mdd_op_lin_pack(int dtype, int nlin, const int32_t* shapes, const float* theta, const float* theta_t, void* wf, void* wt,
                    void* wf_t, void* wt_t, void* stream) {
  CHECK_STORAGE(dtype);
  CHECK_ARG(nlin > 0 && shapes && theta && wf && wt, "null pointer / empty problem");
  CHECK_ARG(theta_t ? (wf_t && wt_t) : (!wf_t && !wt_t), "wf_t and wt_t come with theta_t");
  // theta holds {weight, bias} per linear, back to back
  std::vector<LinPackDesc> lpd;
  int64_t off = 0, off_p = 0, tiles = 0;
  for (int i = 0; i < nlin; ++i) {
    const int out = shapes[2 * i], in = shapes[2 * i + 1];
    CHECK_ARG(out > 0 && in > 0, "linear geometry");
    lpd.push_back(lin_pack_desc(out, in, off, off_p, tiles));
    CHECK_ARG(tiles <= 2147483647ll, "too many tiles");
    off += (int64_t)out * in + out; off_p += (int64_t)out * in;
  }
  hipStream_t st = (hipStream_t)stream;
  return with_device_descs(lpd, st, [&](const LinPackDesc* d_lpd) {
    with_storage(dtype, [&](auto* tag) {
      using AT = tag_t<decltype(tag)>;
      launch_lin_pack_all<AT>(d_lpd, nlin, (int)tiles, theta, theta_t, (AT*)wf, (AT*)wt, (AT*)wf_t, (AT*)wt_t, st);
    });
  });
}

// ---- text head
int mdd_op_text_head(int op, int n, int d, float eps, float mul, const float* a, const float* a_t, const float* b,
                     const float* b_t, const float* c, const float* c_t, const float* mask, const float* gamma,
                     const float* gamma_t, const float* beta, const float* beta_t, const int64_t* idx, const float* coef,
                     float* out, float* out_t, float* out2, float* out2_t, float* dgamma, float* dbeta, float* stats,
                     void* stream) {
  CHECK_ARG(op >= 0 && op <= 5, "op must be 0 (gelu), 1 (gelu_bwd), 2 (ln_fwd), 3 (ln_bwd), 4 (gather_rows) or 5 (scatter_rows_axpy)");
  CHECK_ARG(n > 0 && d > 0, "empty problem");
  CHECK_ARG(a && out, "null pointer");
  const bool T = out_t != nullptr;
  CHECK_ARG(T == (a_t != nullptr), "tangent operands come together");
  CHECK_ARG(op == 2 || op == 3 || !(mask || gamma || gamma_t || beta || beta_t || out2 || out2_t || dgamma || dbeta || stats),
            "LayerNorm operands belong to ops 2 and 3");
  CHECK_ARG(op >= 4 || !(idx || coef), "idx and coef belong to ops 4 and 5");
  CHECK_ARG(T || !(b_t || c_t || gamma_t || beta_t || out2_t), "tangent operands without a tangent output");
  hipStream_t st = (hipStream_t)stream;
  const int64_t nd = (int64_t)n * d;
  switch (op) {
    case 0:   // a = p -> out = g
      CHECK_ARG(!b && !b_t && !c && !c_t, "gelu takes one operand");
      launch_gelu(out, out_t, a, a_t, nd, st);
      break;
    case 1:   // a = p, b = rbar, c = gbar -> out = pbar = rbar + gbar * gelu'(p)
      CHECK_ARG(b && c && T == (b_t != nullptr) && T == (c_t != nullptr), "gelu_bwd: p, rbar, gbar (tangent: all three)");
      launch_gelu_bwd(out, out_t, b, b_t, c, c_t, a, a_t, nd, st);
      break;
    case 2:   // a = f, b = p -> out2 = r = f * mask + p, out = y = LN(r) * gamma + beta
      CHECK_ARG(b && gamma && beta && out2 && !c && !c_t, "ln_fwd: f, p, gamma, beta, y, r");
      CHECK_ARG(T == (b_t != nullptr) && T == (out2_t != nullptr), "ln_fwd tangent: f_t, p_t, y_t, r_t");
      CHECK_ARG(!dgamma && !dbeta && !stats, "ln_fwd has no parameter gradients");
      launch_ln_fwd(out, out_t, out2, out2_t, a, a_t, mask, drop_spec_none(), b, b_t, gamma, gamma_t, beta, beta_t, n, d, eps, st);
      break;
    case 3:   // a = ybar, b = r -> out = rbar, out2 = fbar = rbar * mask, dgamma, dbeta (tangent: their tangents)
      CHECK_ARG(b && gamma && out2 && dgamma && dbeta && stats && !c && !c_t && !beta && !beta_t,
                "ln_bwd: ybar, r, gamma, rbar, fbar, dgamma, dbeta, stats [4 n]");
      CHECK_ARG(T == (b_t != nullptr) && T == (out2_t != nullptr), "ln_bwd tangent: ybar_t, r_t, rbar_t, fbar_t");
      launch_ln_bwd(out, out_t, out2, out2_t, dgamma, dbeta, stats, a, a_t, b, b_t, mask, drop_spec_none(), gamma, gamma_t, n, d, eps, st);
      break;
    case 4:   // out [n, d] = a[idx]
      CHECK_ARG(!T && !b && !c && !coef, "gather_rows: in, idx");
      launch_gather_rows(out, a, idx, n, d, st);
      break;
    default:  // out[idx] += coef * mul * a [n, d]
      CHECK_ARG(!T && !b && !c, "scatter_rows_axpy: in, idx, coef");
      launch_scatter_rows_axpy(out, a, idx, coef, mul, n, d, st);
      break;
  }
  POST_LAUNCH("op_text_head");
  return 0;
}

// ---- evaluation
int mdd_retrieval_ranks(const float* img_feat, const float* txt_feat, const int* img2txt_off,
                        const int* img2txt_idx, const int* txt2img, int n_img, int n_txt, int dim,
                        float scale, float* scores_ws, float* norm_ws, int* rank_i2t, int* rank_t2i,
                        void* stream) {
  CHECK_ARG(img_feat && txt_feat && img2txt_off && img2txt_idx && txt2img, "null input pointer");
  CHECK_ARG(scores_ws && norm_ws && rank_i2t && rank_t2i, "null output / workspace pointer");
  CHECK_ARG(n_img > 0 && n_txt > 0 && dim > 0, "empty problem");
  launch_retrieval_ranks(rank_i2t, rank_t2i, scores_ws, norm_ws, img_feat, txt_feat, img2txt_off,
                         img2txt_idx, txt2img, n_img, n_txt, dim, scale, (hipStream_t)stream);
  POST_LAUNCH("retrieval_ranks");
  return 0;
}

int mdd_nearest_neighbor(const float* query, const float* bank, int n_query, int n_bank, int dim,
                         float* scores_ws, float* norm_ws, int* idx_out, void* stream) {
  CHECK_ARG(query && bank && scores_ws && norm_ws && idx_out, "null pointer");
  CHECK_ARG(n_query > 0 && n_bank > 0 && dim > 0, "empty problem");
  launch_nearest_neighbor(idx_out, scores_ws, norm_ws, query, bank, n_query, n_bank, dim, (hipStream_t)stream);
  POST_LAUNCH("nearest_neighbor");
  return 0;
}

// ---- the kernels at the edges of every pass
int mdd_op_image_edge(int dtype, int op, int n, int h, int w, int c, int k, int stride, int pad, float mul,
                      const float* image, const int64_t* idx, const float* coef, const void* a, const void* wt1,
                      const void* a2, const void* wt2, void* out, float* dimage, void* stream) {
  CHECK_STORAGE(dtype);
  CHECK_ARG(op >= 0 && op <= 5, "op must be 0 (gather), 1 (scatter), 2 (stem dgrad), 3 (patchify), 4 (unpatchify_accum) or 5 (im2col)");
  CHECK_ARG(n > 0 && h > 0 && w > 0 && c > 0, "empty problem");
  CHECK_ARG((int64_t)n * h * w <= 2147483647ll / 64, "problem too large");
  const int ce = dtype == MDD_DTYPE_F32 ? 4 : 8;
  const bool reads_image = op == 0 || op == 3, accumulates = op == 1 || op == 2 || op == 4;
  CHECK_ARG(reads_image ? (image && out && !a && !dimage) : (a && !image), "gather / patchify: image -> out; the others read a");
  CHECK_ARG(accumulates ? (dimage && !out) : (out && !dimage && !coef), "scatter / stem dgrad / unpatchify_accum: dimage (+ coef); the others: out");
  CHECK_ARG(op != 5 || !idx, "im2col takes no idx");
  CHECK_ARG(op == 2 ? (wt1 && (a2 == nullptr) == (wt2 == nullptr)) : (!wt1 && !a2 && !wt2), "stem dgrad: dy1, wt1 and the second pair whole or not at all; the others take no weights");
  CHECK_ARG(op == 3 || op == 4 || op == 5 || (k == 0 && stride == 0 && pad == 0), "k, stride, pad belong to patchify / unpatchify_accum (k) and im2col");
  if (op <= 1) CHECK_ARG(c >= 3, "cpad must hold the 3 image channels");
  if (op == 2) CHECK_ARG(h == w, "stem dgrad: square images");
  if (op == 3 || op == 4) CHECK_ARG(h == w && k > 0 && stride == 0 && pad == 0 && h % k == 0 && c == 3, "patches: square images, s % p == 0, c = 3");
  if (op == 5) {
    CHECK_ARG(k > 0 && stride > 0 && pad >= 0 && h + 2 * pad >= k && w + 2 * pad >= k, "im2col: conv geometry");
    CHECK_ARG(c % ce == 0, "im2col: cpad must be a multiple of the 16-byte chunk");
    CHECK_ARG((int64_t)((w + 2 * pad - k) / stride + 1) * k * k * (c / ce) <= 2147483647ll, "im2col: row too long");
  }
  hipStream_t st = (hipStream_t)stream;
  bool taken = true;
  with_storage(dtype, [&](auto* tag) {
    using AT = tag_t<decltype(tag)>;
    switch (op) {
      case 0: launch_img_gather_nhwc<AT>((AT*)out, image, idx, n, 3, h, w, c, st); break;
      case 1: launch_img_scatter_grad<AT>(dimage, (const AT*)a, idx, coef, mul, n, 3, h, w, c, st); break;
      case 2: taken = launch_stem_dgrad_image<AT>(dimage, (const AT*)a, (const AT*)wt1, (const AT*)a2, (const AT*)wt2, idx, coef, mul, n, h, c, 8, st); break;
      case 3: launch_patchify<AT>((AT*)out, image, idx, n, h, k, st); break;
      case 4: launch_unpatchify_accum<AT>(dimage, (const AT*)a, idx, coef, mul, n, h, k, st); break;
      default: launch_im2col<AT>((AT*)out, (const AT*)a, n, h, w, c, k, stride, pad, (h + 2 * pad - k) / stride + 1, (w + 2 * pad - k) / stride + 1, st); break;
    }
  });
  CHECK_ARG(taken, "stem dgrad: s must be a multiple of 8 and cout 8 or 16");
  POST_LAUNCH("op_image_edge");
  return 0;
}

int mdd_op_vit_glue(int dtype, int op, int n, int tok, int dim, const void* a, const void* a_t, const void* b, const void* b_t,
                    const float* cls, const float* cls_t, const float* pos, const float* pos_t, void* out, void* out_t,
                    float* dcls, float* dpos, void* stream) {
  CHECK_STORAGE(dtype);
  CHECK_ARG(op >= 0 && op <= 6, "op must be 0 (embed), 1 (embed_bwd), 2 (cls_gather), 3 (cls_scatter), 4 (add2), 5 (act_to_f32) or 6 (f32_to_act)");
  CHECK_ARG(n > 0 && tok > 0 && dim > 0, "empty problem");
  CHECK_ARG(a, "null pointer");
  const bool T = a_t != nullptr;
  CHECK_ARG(T == (out_t != nullptr), "tangent operands come together");
  CHECK_ARG(T || out, "null output");
  CHECK_ARG(!T || op == 0 || op == 1 || op == 4, "only embed, embed_bwd and add2 have a tangent form");
  CHECK_ARG(op == 0 ? (cls && pos && T == (cls_t != nullptr) && T == (pos_t != nullptr)) : (!cls && !cls_t && !pos && !pos_t),
            "embed: cls and pos (tangent: cls_t and pos_t); the others take neither");
  CHECK_ARG(op == 1 ? (dcls && dpos) : (!dcls && !dpos), "embed_bwd: dcls and dpos; the others take neither");
  CHECK_ARG(op == 4 ? (b && T == (b_t != nullptr)) : (!b && !b_t), "add2: b (tangent: b_t); the others take one operand");
  CHECK_ARG(op > 1 || tok >= 2, "embed: the class token and at least one patch");
  const int64_t elems = (int64_t)n * tok * dim;
  CHECK_ARG(op != 4 || elems % (dtype == MDD_DTYPE_F32 ? 4 : 8) == 0, "add2: n * tok * dim must be a multiple of the 16-byte chunk");
  hipStream_t st = (hipStream_t)stream;
  with_storage(dtype, [&](auto* tag) {
    using AT = tag_t<decltype(tag)>;
    const AT *A = (const AT*)a, *A_t = (const AT*)a_t;
    switch (op) {
      case 0: launch_vit_embed<AT>((AT*)out, (AT*)out_t, A, A_t, cls, cls_t, pos, pos_t, n, tok, dim, st); break;
      case 1: launch_vit_embed_bwd<AT>(A, A_t, (AT*)out, (AT*)out_t, dcls, dpos, n, tok, dim, st); break;
      case 2: launch_cls_gather<AT>((AT*)out, A, n, tok, dim, st); break;
      case 3: launch_cls_scatter<AT>((AT*)out, A, n, tok, dim, st); break;
      case 4: launch_add2<AT>((AT*)out, (AT*)out_t, A, A_t, (const AT*)b, (const AT*)b_t, elems, st); break;
      case 5: launch_act_to_f32<AT>((float*)out, A, elems, st); break;
      default: launch_f32_to_act<AT>((AT*)out, (const float*)a, elems, st); break;
    }
  });
  POST_LAUNCH("op_vit_glue");
  return 0;
}

}  // extern "C"
