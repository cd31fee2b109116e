// Operator-level C ABI (include/pfhip_ops.h): thin wrappers over the kernel launchers.
#include "../../include/pfhip_ops.h"

#include "ctx_graph.h"
#include "lm_graph.h"
#include "internal.h"      // build_frontend_tables, DevMem; brings kernels.h
#include "beam_front.h"

#include <algorithm>
#include <cmath>
#include <vector>

namespace {
inline hipStream_t S(void* s) { return static_cast<hipStream_t>(s); }
inline int done() { return (int)hipGetLastError(); }
// The entries of kernels that read device descriptors (StreamSeg, VadSeg) take plain host arrays: the descriptors are built here,
// uploaded with a synchronous copy, and freed after the stream has drained.  Test entries: the sync costs nothing that matters.
template <class Seg, class Launch>
int with_device_segs(const std::vector<Seg>& host, hipStream_t s, Launch launch) {
  Seg* d = nullptr;
  hipError_t e = hipMalloc(reinterpret_cast<void**>(&d), host.size() * sizeof(Seg));
  if (e != hipSuccess) return (int)e;
  e = hipMemcpy(d, host.data(), host.size() * sizeof(Seg), hipMemcpyHostToDevice);
  if (e == hipSuccess) {
    launch(d);
    e = hipGetLastError();
    const hipError_t e2 = hipStreamSynchronize(s);
    if (e == hipSuccess) e = e2;
  }
  (void)hipFree(d);
  return (int)e;
}
// The ABI's integer `kind` (pfhip_ops.h) as the launchers' enum — the one place the numbers appear; false for 6 and outside 0..10
constexpr int kKindBySize = 0;
bool kernel_of_kind(int kind, pfhip::GemmKernel* kernel) {
  using G = pfhip::GemmKernel;
  static const G table[11] = {G::BySize,   G::Tiled128, G::Streaming, G::Tiled64, G::Bf16_256, G::Bf16_128,
                              G::BySize /* 6: none */, G::Bf16_64,  G::F16_256,   G::F16_128, G::F16_64};
  if (kind < 0 || kind > 10 || kind == 6) return false;
  *kernel = table[kind];
  return true;
}
// the rows and K that pfhip_op_fused_ln_gemm and its route entry take
inline bool ln_gemm_shape_ok(int M, int K) { return M >= 1 && M <= 32 && K % 8 == 0; }
}  // namespace

extern "C" {

int pfhip_op_gemm_f32(const float* A, int lda, const float* W, int ldw, float* C, int ldc, const float* bias,
                      const float* R1, int ldr1, const float* R2, int ldr2, int M, int N, int K, int relu,
                      int guard, void* stream) {
  return pfhip_op_gemm_f32_scaled(A, lda, W, ldw, C, ldc, bias, R1, ldr1, R2, ldr2, M, N, K, relu, guard, kKindBySize, 1.0f, stream);
}
int pfhip_op_gemm_f32_kind(const float* A, int lda, const float* W, int ldw, float* C, int ldc, const float* bias,
                           const float* R1, int ldr1, const float* R2, int ldr2, int M, int N, int K, int relu,
                           int guard, int kind, void* stream) {
  return pfhip_op_gemm_f32_scaled(A, lda, W, ldw, C, ldc, bias, R1, ldr1, R2, ldr2, M, N, K, relu, guard, kind, 1.0f, stream);
}
int pfhip_op_fused_ln_gemm(const float* X, int ldx, int D, const float* g, const float* b, float eps, const float* W, int ldw,
                           float* C, int ldc, const float* bias, const float* R1, int ldr1, const float* R2, int ldr2,
                           const float* fsmn_v, int ldv, const float* fsmn_w, int M, int N, int K, int relu, void* stream) {
  if (!ln_gemm_shape_ok(M, K) || (g && (D % 4 || D > K || D > 2048))) return (int)hipErrorInvalidValue;
  pfhip::launch_fused_ln_gemm({.X = X, .ldx = ldx, .W = W, .ldw = ldw, .C = C, .ldc = ldc, .M = M, .N = N, .K = K, .bias = bias, .R1 = R1,
                               .ldr1 = ldr1, .R2 = R2, .ldr2 = ldr2, .relu = relu != 0, .eps = eps, .fsmn_v = fsmn_v, .ldv = ldv,
                               .fsmn_w = fsmn_w, .ln_g = g, .ln_b = b, .D = D},
                              S(stream));
  return done();
}
// dev hook (tools/fused_gemv_bench.py): n launches back to back over a ring of weight copies, so the host loop is not Python
int pfhip_dev_fused_ln_gemm_bench(const float* X, int ldx, int D, const float* g, const float* b, const float* W, int ldw,
                                  size_t w_stride_floats, int n_copies, float* C, int ldc, const float* bias, const float* R1, int ldr1,
                                  int M, int N, int K, int relu, int n_launch, void* stream) {
  for (int i = 0; i < n_launch; ++i)
    pfhip::launch_fused_ln_gemm({.X = X, .ldx = ldx, .W = W + (size_t)(i % n_copies) * w_stride_floats, .ldw = ldw, .C = C, .ldc = ldc,
                                 .M = M, .N = N, .K = K, .bias = bias, .R1 = R1, .ldr1 = ldr1, .relu = relu != 0, .ln_g = g, .ln_b = b, .D = D},
                                S(stream));
  return done();
}
int pfhip_op_fused_gemv_1trip(const float* X, int ldx, const float* W, int ldw, float* C, int ldc, const float* bias,
                              const float* ln_colsum, float eps, const float* R1, int ldr1, const float* fsmn_v, int ldv,
                              const float* fsmn_w, int M, int N, int K, int relu, void* stream) {
  if (!pfhip::launch_fused_gemv_1trip({.X = X, .ldx = ldx, .W = W, .ldw = ldw, .C = C, .ldc = ldc, .M = M, .N = N, .K = K, .bias = bias, .R1 = R1,
                                       .ldr1 = ldr1, .relu = relu != 0, .eps = eps, .fsmn_v = fsmn_v, .ldv = ldv, .fsmn_w = fsmn_w,
                                       .ln_colsum = ln_colsum},
                                      S(stream)))
    return (int)hipErrorInvalidValue;
  return done();
}
// what the two entries above would launch (kernels.h: the launchers' own choice; nothing is launched, no device is touched)
int pfhip_op_fused_gemv_1trip_route(int M, int N, int K, int has_ln, int has_fsmn, int* out) {
  if (!out) return (int)hipErrorInvalidValue;
  const pfhip::Gemv1tRoute r = pfhip::fused_gemv_1trip_route(M, N, K, has_ln != 0, has_fsmn != 0);
  const int v[8] = {r.ok, r.ln, r.fs, r.cw, r.cpl, r.rpl, r.nf, r.waves};
  for (int i = 0; i < 8; ++i) out[i] = v[i];
  return 0;
}
int pfhip_op_fused_ln_gemm_route(int M, int N, int K, int has_ln, int* out) {
  if (!out || !ln_gemm_shape_ok(M, K)) return (int)hipErrorInvalidValue;
  const pfhip::LnGemmRoute r = pfhip::fused_ln_gemm_route(M, N, K, has_ln != 0);
  const int v[6] = {(int)r.kernel, r.ln, r.cw, r.mr, r.waves, r.k_blocks};
  for (int i = 0; i < 6; ++i) out[i] = v[i];
  return 0;
}
// dev hook (tools/fused_gemv_bench.py): the one-trip form over the same ring of weight copies
int pfhip_dev_fused_gemv_1trip_bench(const float* X, int ldx, const float* W, int ldw, size_t w_stride_floats, int n_copies, float* C, int ldc,
                                     const float* bias, const float* ln_colsum, const float* R1, int ldr1, int M, int N, int K, int relu,
                                     int n_launch, void* stream) {
  for (int i = 0; i < n_launch; ++i)
    if (!pfhip::launch_fused_gemv_1trip({.X = X, .ldx = ldx, .W = W + (size_t)(i % n_copies) * w_stride_floats, .ldw = ldw, .C = C, .ldc = ldc,
                                         .M = M, .N = N, .K = K, .bias = bias, .R1 = R1, .ldr1 = ldr1, .relu = relu != 0, .ln_colsum = ln_colsum},
                                        S(stream)))
      return (int)hipErrorInvalidValue;
  return done();
}
int pfhip_op_window_attention(const float* Q, int ldq, const float* K, int ldk, const float* V, int ldv, float* O, int ldo, int Lq, int Lk,
                              int H, float scale, void* stream) {
  return pfhip_op_window_attention_hd(Q, ldq, K, ldk, V, ldv, O, ldo, Lq, Lk, H, scale, pfhip::kHeadDim, stream);
}
int pfhip_op_window_attention_hd(const float* Q, int ldq, const float* K, int ldk, const float* V, int ldv, float* O, int ldo, int Lq, int Lk,
                                 int H, float scale, int head_dim, void* stream) {
  if (head_dim != 128 && head_dim != 80) return (int)hipErrorInvalidValue;      // before anything is launched
  if (!pfhip::launch_window_attention({.Q = Q, .ldq = ldq, .K = K, .ldk = ldk, .V = V, .ldv = ldv, .O = O, .ldo = ldo, .H = H, .max_q_len = Lq,
                                       .scale = scale, .head_dim = head_dim},
                                      Lk, S(stream)))
    return (int)hipErrorInvalidValue;
  return done();
}
int pfhip_op_window_attention_segments(const float* Q, int ldq, const float* K, int ldk, const float* V, int ldv, float* O, int ldo,
                                       const int* q_off, const int* q_len, const int* kv_off, const int* kv_len, int B, int H, int max_q_len,
                                       int max_kv_len, float scale, const float* fsmn_w, float* mem, int ldmem, int head_dim, void* stream) {
  // before anything is launched: the kernel reads float4s of H * head_dim columns of every Q / K row and stores as many of O / mem
  if ((head_dim != 128 && head_dim != 80) || B < 1 || H < 1 || max_q_len < 1 || max_q_len > 32 || max_kv_len < 1 || max_kv_len > 32 ||
      !Q || !K || !V || !O || !q_off || !q_len || !kv_off || !kv_len)
    return (int)hipErrorInvalidValue;
  const long long w = (long long)H * head_dim;
  if ((ldq | ldk | ldv | ldo) % 4 || ldq < w || ldk < w || ldv < w || ldo < w || (fsmn_w && (!mem || ldmem < w || ldmem % 4)))
    return (int)hipErrorInvalidValue;
  if (!pfhip::launch_window_attention({.Q = Q, .ldq = ldq, .K = K, .ldk = ldk, .V = V, .ldv = ldv, .O = O, .ldo = ldo, .q_off = q_off, .q_len = q_len,
                                       .kv_off = kv_off, .kv_len = kv_len, .B = B, .H = H, .max_q_len = max_q_len, .scale = scale,
                                       .head_dim = head_dim, .fsmn_w = fsmn_w, .mem = mem, .ldmem = ldmem},
                                      max_kv_len, S(stream)))
    return (int)hipErrorInvalidValue;
  return done();
}
int pfhip_op_fused_att_out(const float* Q, int ldq, const float* K, int ldk, const float* V, int ldv, int Lq, int Lk, int H, float scale,
                           const float* W, int ldw, float* C, int ldc, const float* bias, const float* R1, int ldr1, const float* fsmn_v,
                           int ldfv, const float* fsmn_w, int N, void* stream) {
  if (!pfhip::launch_fused_att_out({.Q = Q, .ldq = ldq, .K = K, .ldk = ldk, .V = V, .ldv = ldv, .H = H, .max_q_len = Lq, .scale = scale}, Lk,
                                   {.W = W, .ldw = ldw, .C = C, .ldc = ldc, .N = N, .bias = bias, .R1 = R1, .ldr1 = ldr1, .fsmn_v = fsmn_v,
                                    .ldv = ldfv, .fsmn_w = fsmn_w},
                                   S(stream)))
    return (int)hipErrorInvalidValue;
  return done();
}
int pfhip_op_gemm_f32_scaled(const float* A, int lda, const float* W, int ldw, float* C, int ldc, const float* bias, const float* R1,
                             int ldr1, const float* R2, int ldr2, int M, int N, int K, int relu, int guard, int kind, float w_scale,
                             void* stream) {
  pfhip::GemmKernel kernel;
  if (K % pfhip::kTileK || !kernel_of_kind(kind, &kernel) || !(w_scale > 0.f)) return (int)hipErrorInvalidValue;
  pfhip::launch_gemm({.A = A, .lda = lda, .W = W, .ldw = ldw, .C = C, .ldc = ldc, .M = M, .N = N, .K = K, .bias = bias, .R1 = R1, .ldr1 = ldr1,
                      .R2 = R2, .ldr2 = ldr2, .relu = relu != 0, .w_scale = w_scale},
                     kernel, guard != 0, S(stream));
  return (int)hipGetLastError();
}
float pfhip_op_best_w_scale(float max_abs) { return pfhip::best_w_scale(max_abs); }
int pfhip_op_set_launch_ctx(int* range_flag, int exact) {
  pfhip::launch_ctx().range_flag = range_flag;
  pfhip::launch_ctx().exact = exact != 0;
  return 0;
}
int pfhip_op_gemm_f32_ln(const float* A, int lda, const float* W, int ldw, float* C, int ldc, const float* bias, const float* R1, int ldr1,
                         const float* R2, int ldr2, int M, int N, int K, int relu, const float* ln_stats, int ln_tiles,
                         const float* ln_colsum, float* stats_out, float w_scale, void* stream) {
  // the kernels clamp operand rows to M - 1 / N - 1 and bounds-check every store; what they assume beyond that is checked here
  if (M <= 0 || N <= 0 || K < pfhip::kTileK || K % pfhip::kTileK || !A || !W || !C || lda < K || ldw < K || ldc < N || (R1 && ldr1 < N) ||
      (R2 && ldr2 < N) || (lda | ldw | ldc | ldr1 | ldr2) % 4 || !(w_scale > 0.f) || (ln_stats && (!ln_colsum || ln_tiles <= 0 || N % 4)) || (!ln_stats && ln_colsum) ||
      (stats_out && N % 128))
    return (int)hipErrorInvalidValue;
  pfhip::launch_gemm({.A = A, .lda = lda, .W = W, .ldw = ldw, .C = C, .ldc = ldc, .M = M, .N = N, .K = K, .bias = bias, .R1 = R1, .ldr1 = ldr1,
                      .R2 = R2, .ldr2 = ldr2, .relu = relu != 0, .w_scale = w_scale, .ln_stats = ln_stats, .ln_tiles = ln_tiles,
                      .ln_colsum = ln_colsum, .stats_out = stats_out},
                     pfhip::GemmKernel::SplitBySize, false, S(stream));
  return (int)hipGetLastError();
}

size_t pfhip_op_plane_image_bytes(int rows, int K) { return pfhip::plane_image_bytes(rows, K); }
int pfhip_op_split_planes(const float* X, int ld, int rows_valid, int rows, int K, float scale, void* hi, void* lo, void* stream) {
  if (K < 16 || K % 16 || rows <= 0 || rows % 128 || rows_valid < 0 || rows_valid > rows || !hi || !lo || (rows_valid > 0 && (!X || ld < K)))
    return (int)hipErrorInvalidValue;
  pfhip::launch_split_planes(X, ld, rows_valid, rows, K, scale, hi, lo, S(stream));
  return (int)hipGetLastError();
}
int pfhip_op_gemm_p3(const void* Ah, const void* Al, int rows_a, const void* Wh, const void* Wl, int rows_w, float w_scale, float* C, int ldc,
                     void* Ph, void* Pl, int rows_p, const float* bias, const float* R1, int ldr1, int M, int N, int K, int relu,
                     const float* ln_stats, int ln_tiles, const float* ln_colsum, float* stats_out, int tile_rows, void* stream) {
  // everything the kernel and its grid assume, checked here: a wrong image size would be an out-of-bounds DMA on the device
  const int mp = (M + 127) / 128 * 128;
  if (M <= 0 || N <= 0 || K < 16 || K % 16 || N % 128 || rows_a % 128 || rows_w % 128 || rows_a < mp || rows_w < N || !Ah || !Al || !Wh ||
      !Wl || (!C && !Ph) || (Ph && (!Pl || rows_p % 128 || rows_p < mp)) || (C && ldc < N) || (R1 && ldr1 < N) || !(w_scale > 0.f) ||
      (ln_stats && (!ln_colsum || ln_tiles <= 0)) || (stats_out && !C) /* the statistics come out of the fp32 epilogue */ ||
      (tile_rows != 0 && tile_rows != 64 && tile_rows != 128 && tile_rows != 256))
    return (int)hipErrorInvalidValue;
  pfhip::launch_gemm_p3({.Ah = Ah, .Al = Al, .rows_a = rows_a, .Wh = Wh, .Wl = Wl, .rows_w = rows_w, .w_scale = w_scale, .C = C, .ldc = ldc,
                         .Ph = Ph, .Pl = Pl, .rows_p = rows_p, .M = M, .N = N, .K = K, .bias = bias, .R1 = R1, .ldr1 = ldr1,
                         .relu = relu != 0, .ln_stats = ln_stats, .ln_tiles = ln_tiles, .ln_colsum = ln_colsum, .stats_out = stats_out},
                        S(stream), tile_rows);
  return (int)hipGetLastError();
}
// The same with a tile-width selector: tile_cols 0 = as pfhip_op_gemm_p3, 256 = the 256 x 256 tile (tile_rows must be 0), refused for the
// forms and shapes that kernel does not serve.
int pfhip_op_gemm_p3_cols(const void* Ah, const void* Al, int rows_a, const void* Wh, const void* Wl, int rows_w, float w_scale, float* C, int ldc,
                          void* Ph, void* Pl, int rows_p, const float* bias, const float* R1, int ldr1, int M, int N, int K, int relu,
                          const float* ln_stats, int ln_tiles, const float* ln_colsum, float* stats_out, int tile_rows, int tile_cols, void* stream) {
  if (tile_cols == 0)
    return pfhip_op_gemm_p3(Ah, Al, rows_a, Wh, Wl, rows_w, w_scale, C, ldc, Ph, Pl, rows_p, bias, R1, ldr1, M, N, K, relu, ln_stats, ln_tiles, ln_colsum,
                            stats_out, tile_rows, stream);
  const int mp = (M + 127) / 128 * 128;
  if (tile_cols != 256 || tile_rows != 0 || M <= 0 || N <= 0 || K < 16 || K % 16 || N % 256 || rows_a % 128 || rows_w % 128 || rows_a < mp ||
      rows_w < N || !Ah || !Al || !Wh || !Wl || (Ph && (!Pl || rows_p % 128 || rows_p < mp)) || (C && ldc < N) || !(w_scale > 0.f) ||
      (ln_stats && (!ln_colsum || ln_tiles <= 0)) ||
      !pfhip::gemm_p3_wide_serves(C != nullptr, Ph != nullptr, R1 != nullptr, ln_stats != nullptr, stats_out != nullptr, 0, N, K))
    return (int)hipErrorInvalidValue;
  pfhip::launch_gemm_p3({.Ah = Ah, .Al = Al, .rows_a = rows_a, .Wh = Wh, .Wl = Wl, .rows_w = rows_w, .w_scale = w_scale, .C = C, .ldc = ldc,
                         .Ph = Ph, .Pl = Pl, .rows_p = rows_p, .M = M, .N = N, .K = K, .bias = bias, .relu = relu != 0,
                         .ln_stats = ln_stats, .ln_tiles = ln_tiles, .ln_colsum = ln_colsum},
                        S(stream), 0, 256);
  return (int)hipGetLastError();
}
long pfhip_op_gemm_p3_wide_launches(void) { return pfhip::gemm_p3_wide_launches(); }

int pfhip_op_layernorm(const float* x, int ldx, float* y, int ldy, const float* g, const float* b, int M, int D,
                       int Dout, float eps, void* stream) {
  if (D % 4 || Dout % 4 || Dout > 2048 || D > Dout) return (int)hipErrorInvalidValue;
  pfhip::launch_layernorm(x, ldx, y, ldy, g, b, M, D, Dout, eps, S(stream));
  return done();
}
int pfhip_op_fsmn(const float* v, int ldv, const float* w, const float* res, int ldres, float* out, int ldo,
                  const int* off, const int* len, int B, int max_len, int C, void* stream) {
  if (C % 4) return (int)hipErrorInvalidValue;
  pfhip::launch_fsmn(v, ldv, w, res, ldres, out, ldo, off, len, B, max_len, C, S(stream));
  return done();
}
int pfhip_op_fsmn_shift(const float* v, int ldv, const float* w, const float* res, int ldres, float* out, int ldo,
                        const int* off, const int* len, int B, int max_len, int C, int shift, void* stream) {
  // before anything is launched: one float4 of four channels per thread and row
  if ((shift != 0 && shift != 5) || C <= 0 || C % 4 || !v || !w || !out || !off || !len || (ldv | ldo) % 4 || ldv < C || ldo < C ||
      (res && (ldres % 4 || ldres < C)))
    return (int)hipErrorInvalidValue;
  pfhip::launch_fsmn_shift(v, ldv, w, res, ldres, out, ldo, off, len, B, max_len, C, shift, S(stream));
  return done();
}
int pfhip_op_attention_limit(const float* Q, int ldq, const float* K, int ldk, const float* V, int ldv, float* O, int ldo,
                             const int* q_off, const int* q_len, const int* kv_off, const int* kv_len, int B, int H,
                             int max_q_len, float scale, int head_dim, const int* q_kv_limit, void* stream) {
  // before anything is launched: the fp32-MFMA kernel reads and writes float4s of H * head_dim columns of every row
  if ((head_dim != 32 && head_dim != 80 && head_dim != 128) || H < 1 || !Q || !K || !V || !O || !q_off || !q_len || !kv_off || !kv_len ||
      !q_kv_limit)
    return (int)hipErrorInvalidValue;
  const long long w = (long long)H * head_dim;
  if ((ldq | ldk | ldv | ldo) % 4 || ldq < w || ldk < w || ldv < w || ldo < w) return (int)hipErrorInvalidValue;
  pfhip::launch_attention({.Q = Q, .ldq = ldq, .K = K, .ldk = ldk, .V = V, .ldv = ldv, .O = O, .ldo = ldo, .q_off = q_off, .q_len = q_len, .kv_off = kv_off, .kv_len = kv_len, .B = B, .H = H,
                           .max_q_len = max_q_len, .scale = scale, .head_dim = head_dim, .q_kv_limit = q_kv_limit},
                          S(stream));
  return done();
}
int pfhip_op_attention(const float* Q, int ldq, const float* K, int ldk, const float* V, int ldv, float* O, int ldo,
                       const int* q_off, const int* q_len, const int* kv_off, const int* kv_len, int B, int H,
                       int max_q_len, float scale, void* stream) {
  return pfhip_op_attention_hd(Q, ldq, K, ldk, V, ldv, O, ldo, q_off, q_len, kv_off, kv_len, B, H, max_q_len, scale, pfhip::kHeadDim, stream);
}
int pfhip_op_attention_hd(const float* Q, int ldq, const float* K, int ldk, const float* V, int ldv, float* O, int ldo,
                          const int* q_off, const int* q_len, const int* kv_off, const int* kv_len, int B, int H,
                          int max_q_len, float scale, int head_dim, void* stream) {
  if (head_dim != 32 && head_dim != 80 && head_dim != 128) return (int)hipErrorInvalidValue;      // before anything is launched
  pfhip::launch_attention({.Q = Q, .ldq = ldq, .K = K, .ldk = ldk, .V = V, .ldv = ldv, .O = O, .ldo = ldo, .q_off = q_off, .q_len = q_len, .kv_off = kv_off, .kv_len = kv_len, .B = B, .H = H,
                           .max_q_len = max_q_len, .scale = scale, .head_dim = head_dim},
                          S(stream));
  return done();
}
int pfhip_op_attention_dk(const float* Q, int ldq, const float* K, int ldk, const float* V, int ldv, float* O, int ldo,
                          const int* q_off, const int* q_len, const int* kv_off, const int* kv_len, int B, int H,
                          int max_q_len, float scale, int d_k, const int* q_kv_limit, void* stream) {
  // before anything is launched: the kernel reads and writes H * d_k columns of every row
  if (d_k < 1 || d_k > 64 || H < 1 || !Q || !K || !V || !O || !q_off || !q_len || !kv_off || !kv_len) return (int)hipErrorInvalidValue;
  const long long w = (long long)H * d_k;
  if (ldq < w || ldk < w || ldv < w || ldo < w) return (int)hipErrorInvalidValue;
  pfhip::launch_attention_dk({.Q = Q, .ldq = ldq, .K = K, .ldk = ldk, .V = V, .ldv = ldv, .O = O, .ldo = ldo, .q_off = q_off, .q_len = q_len, .kv_off = kv_off, .kv_len = kv_len, .B = B, .H = H,
                              .max_q_len = max_q_len, .scale = scale, .head_dim = d_k, .q_kv_limit = q_kv_limit},
                             S(stream));
  return done();
}
int pfhip_op_attention_fsmn(const float* Q, int ldq, const float* K, int ldk, const float* V, int ldv, float* O, int ldo, const int* off,
                            const int* len, int B, int H, int max_len, float scale, const float* fsmn_w, float* mem, int ldmem,
                            int mem_accumulate, int head_dim, void* stream) {
  if ((head_dim != 80 && head_dim != 128) || !fsmn_w || !mem || !O || H <= 0 || ldmem < H * head_dim) return (int)hipErrorInvalidValue;
  pfhip::launch_attention_fsmn({.Q = Q, .ldq = ldq, .K = K, .ldk = ldk, .V = V, .ldv = ldv, .O = O, .ldo = ldo, .q_off = off, .q_len = len, .kv_off = off, .kv_len = len, .B = B, .H = H, .max_q_len = max_len,
                                .scale = scale, .head_dim = head_dim, .fsmn_w = fsmn_w, .mem = mem, .ldmem = ldmem,
                                .mem_accumulate = mem_accumulate != 0},
                               S(stream));
  return done();
}
int pfhip_op_attention_fsmn_is_fused(int max_len, int head_dim) { return pfhip::attention_fsmn_is_fused(max_len, head_dim) ? 1 : 0; }
int pfhip_op_attention_planes(const float* Q, int ldq, const float* K, int ldk, const float* V, int ldv, void* planes_hi, void* planes_lo,
                              int plane_rows, const int* q_off, const int* q_len, const int* kv_off, const int* kv_len, int B, int H,
                              int max_q_len, int total_q_rows, float scale, void* stream) {
  // the image must hold every query row the launch writes (rows are global: q_off[b] + t), in whole 128-row tiles
  if (!planes_hi || !planes_lo || plane_rows % 128 || total_q_rows > plane_rows || B <= 0 || H <= 0) return (int)hipErrorInvalidValue;
  pfhip::launch_attention_x3({.Q = Q, .ldq = ldq, .K = K, .ldk = ldk, .V = V, .ldv = ldv, .q_off = q_off, .q_len = q_len, .kv_off = kv_off,
                              .kv_len = kv_len, .B = B, .H = H, .max_q_len = max_q_len, .scale = scale, .planes_hi = planes_hi,
                              .planes_lo = planes_lo, .plane_rows = plane_rows},
                             S(stream));
  return done();
}
int pfhip_op_split_rows(const float* X, int ld, int rows, int cols, void* hi, void* lo, int ldp, void* stream) {
  if (!X || !hi || !lo || rows <= 0 || cols <= 0 || cols % 8 || ld < cols || ldp < cols || ldp % 8) return (int)hipErrorInvalidValue;
  pfhip::launch_split_rows(X, ld, rows, cols, hi, lo, ldp, S(stream));
  return (int)hipGetLastError();
}
int pfhip_op_gemm_p3_qkv(const void* Ah, const void* Al, int rows_a, const void* Wh, const void* Wl, int rows_w, float w_scale, float* C, int ldc,
                         void* kv_hi, void* kv_lo, int ldkv, int q_cols, const float* bias, int M, int N, int K, const float* ln_stats,
                         int ln_tiles, const float* ln_colsum, int tile_rows, void* stream) {
  const int mp = (M + 127) / 128 * 128;
  if (M <= 0 || N <= 0 || K < 16 || K % 16 || N % 128 || rows_a % 128 || rows_w % 128 || rows_a < mp || rows_w < N || !Ah || !Al || !Wh ||
      !Wl || !C || !kv_hi || !kv_lo || q_cols <= 0 || q_cols % 128 || q_cols >= N || ldc < q_cols || ldkv < N - q_cols || ldkv % 8 ||
      !(w_scale > 0.f) || (ln_stats && (!ln_colsum || ln_tiles <= 0)) || (tile_rows != 0 && tile_rows != 64 && tile_rows != 128))
    return (int)hipErrorInvalidValue;
  pfhip::launch_gemm_p3({.Ah = Ah, .Al = Al, .rows_a = rows_a, .Wh = Wh, .Wl = Wl, .rows_w = rows_w, .w_scale = w_scale, .C = C, .ldc = ldc,
                         .Ph = kv_hi, .Pl = kv_lo, .rows_p = ldkv, .row_planes_from = q_cols, .M = M, .N = N, .K = K,
                         .bias = bias, .ln_stats = ln_stats, .ln_tiles = ln_tiles, .ln_colsum = ln_colsum},
                        S(stream), tile_rows);
  return (int)hipGetLastError();
}
int pfhip_op_attention_kvplanes(const float* Q, int ldq, const void* kv_hi, const void* kv_lo, int ldkv, int v_col, int total_kv_rows, float* O,
                                int ldo, void* planes_hi, void* planes_lo, int plane_rows, const int* q_off, const int* q_len,
                                const int* kv_off, const int* kv_len, int B, int H, int max_q_len, int total_q_rows, float scale,
                                const float* fsmn_w, float* mem, int ldmem, int mem_accumulate, void* stream) {
  // shapes the kernel's DMA and stores assume: 16-byte chunks of whole heads inside a plane row, both operands inside one row
  if (!Q || !kv_hi || !kv_lo || B <= 0 || H <= 0 || ldkv % 8 || v_col % 8 || v_col < H * 128 || ldkv < v_col + H * 128 || total_kv_rows <= 0 ||
      (!O && !planes_hi) || (planes_hi && (!planes_lo || plane_rows % 128 || total_q_rows > plane_rows)) || (O && ldo < H * 128) ||
      (fsmn_w && (!mem || ldmem < H * 128)))
    return (int)hipErrorInvalidValue;
  pfhip::launch_attention_p3({.Q = Q, .ldq = ldq, .O = O, .ldo = ldo, .q_off = q_off, .q_len = q_len, .kv_off = kv_off, .kv_len = kv_len, .B = B,
                              .H = H, .max_q_len = max_q_len, .scale = scale, .fsmn_w = fsmn_w, .mem = mem, .ldmem = ldmem,
                              .mem_accumulate = mem_accumulate != 0, .planes_hi = planes_hi, .planes_lo = planes_lo,
                              .plane_rows = plane_rows, .kv_hi = kv_hi, .kv_lo = kv_lo, .ldkv = ldkv, .v_col = v_col},
                             S(stream));
  return done();
}
int pfhip_op_cif(const float* hidden, int ldh, const float* alphas, const int* row_off, const int* len, int B, int D,
                 float threshold, float tail, float* stage, int* n_fires, int* token_num, void* stream) {
  if (D > 1024) return (int)hipErrorInvalidValue;
  pfhip::launch_cif(hidden, ldh, alphas, row_off, len, B, D, threshold, tail, stage, n_fires, token_num, S(stream));
  return done();
}
int pfhip_op_cif_fires(const float* hidden, int ldh, const float* alphas, const int* row_off, const int* len, int B, int D,
                       float threshold, float tail, float* stage, int* n_fires, int* token_num, int* fire_frame, void* stream) {
  if (D > 1024 || !fire_frame) return (int)hipErrorInvalidValue;
  pfhip::launch_cif(hidden, ldh, alphas, row_off, len, B, D, threshold, tail, stage, n_fires, token_num, S(stream), fire_frame);
  return done();
}
int pfhip_op_logsoftmax_argmax(const float* logits, int ldl, int ML, int V, float* logp, int32_t* ids, void* stream) {
  pfhip::launch_logsoftmax_argmax(logits, ldl, ML, V, logp, ids, S(stream));
  return done();
}
int pfhip_op_logsoftmax_topk(const float* logits, int ldl, int M, int V, int k, float* logp, int32_t* ids, int32_t* topk_ids,
                             float* topk_logp, void* stream) {
  // the launcher checks k, V >= k, ldl >= V and the buffers before it launches anything
  if (!pfhip::launch_logsoftmax_topk(logits, ldl, M, V, k, logp, ids, topk_ids, topk_logp, S(stream))) return (int)hipErrorInvalidValue;
  return done();
}
size_t pfhip_op_ctc_head_workspace_bytes(int M, int V) { return M > 0 && V > 0 ? pfhip::ctc_head_workspace_bytes(M, V) : 0; }
int pfhip_op_ctc_head(const float* X, int ldx, const float* W, int ldw, const float* bias, float w_scale, int M, int V, int K,
                      int32_t* ids, float* logp_best, float* lse, void* workspace, size_t workspace_bytes, void* stream) {
  // the launcher checks shapes, strides, buffers and the workspace size before it launches anything
  if (!pfhip::launch_ctc_head(X, ldx, W, ldw, bias, w_scale, M, V, K, ids, logp_best, lse, workspace, workspace_bytes, S(stream)))
    return (int)hipErrorInvalidValue;
  return done();
}
int pfhip_op_ctc_collapse(const int32_t* frame_ids, const float* frame_logp, const int* row_off, const int* len, int B, int blank,
                          int max_tokens, int32_t* ids, int32_t* tok_frame, float* tok_logp, int32_t* token_num, void* stream) {
  if (!pfhip::launch_ctc_collapse(frame_ids, frame_logp, row_off, len, B, blank, max_tokens, ids, tok_frame, tok_logp, token_num, S(stream)))
    return (int)hipErrorInvalidValue;
  return done();
}
int pfhip_op_ctc_collapse_chunk(void) { return pfhip::ctc_collapse_chunk(); }
int pfhip_op_ctc_emissions(const float* X, int ldx, const float* W, int ldw, const float* bias, const float* lse, const int* row_off,
                           const int* len, const int* lab_off, const int* n_lab, const int32_t* labels, const long long* e_off, int B,
                           int K, int V, int blank, float* E, void* stream) {
  if (!pfhip::launch_ctc_emissions(X, ldx, W, ldw, bias, lse, row_off, len, lab_off, n_lab, labels, e_off, B, K, V, blank, E, S(stream)))
    return (int)hipErrorInvalidValue;
  return done();
}
int pfhip_op_ctc_greedy_plan(const int32_t* token_num, const int* speech_len, int B, int maxT, long long cap_floats, int* n_lab, int* lab_off,
                             long long* e_off, long long* total, void* stream) {
  if (!pfhip::launch_ctc_greedy_plan(token_num, speech_len, B, maxT, cap_floats, n_lab, lab_off, e_off, total, S(stream)))
    return (int)hipErrorInvalidValue;
  return done();
}
size_t pfhip_op_ctc_head_topk_workspace_bytes(int M, int V, int k) {
  return M > 0 && V > 0 && k >= 1 && k <= pfhip::kCtcTopkMax ? pfhip::ctc_head_topk_workspace_bytes(M, V, k) : 0;
}
int pfhip_op_ctc_head_topk(const float* X, int ldx, const float* W, int ldw, const float* bias, float w_scale, int M, int V, int K, int k,
                           int32_t* ids, float* logp_best, float* lse, int32_t* topk_ids, float* topk_logp, void* workspace,
                           size_t workspace_bytes, void* stream) {
  // the launcher checks k, V >= k, shapes, strides, buffers and the workspace size before it launches anything
  if (!pfhip::launch_ctc_head_topk(X, ldx, W, ldw, bias, w_scale, M, V, K, k, ids, logp_best, lse, topk_ids, topk_logp, workspace,
                                   workspace_bytes, S(stream)))
    return (int)hipErrorInvalidValue;
  return done();
}
// the graph's packed image goes in front of the trie nodes, 16-byte aligned
static size_t beam_graph_bytes(const pfhip_ctx_graph* g) { return g ? (g->packed.size() * 4 + 15) / 16 * 16 : 0; }
size_t pfhip_op_ctc_prefix_beam_workspace_bytes(long long rows, int B, int second_beam, const pfhip_ctx_graph* graph) {
  const size_t nodes = pfhip::ctc_prefix_beam_workspace_bytes(rows, B, second_beam);
  return nodes ? nodes + beam_graph_bytes(graph) : 0;
}
int pfhip_op_ctc_prefix_beam(const int32_t* topk_ids, const float* topk_logp, int k, long long rows, const int* row_off, const int* len, int B,
                             int V, int blank, int first_beam, int second_beam, const pfhip_ctx_graph* graph, int nbest, int max_tokens,
                             int32_t* n_hyp, int32_t* ids, int32_t* n_tokens, float* score, float* ctc_score, float* ctx_score,
                             void* workspace, size_t workspace_bytes, void* stream) {
  const size_t gbytes = beam_graph_bytes(graph);
  if ((graph && graph->vocab != V) || !workspace || workspace_bytes < gbytes) return (int)hipErrorInvalidValue;
  pfhip::CtxGraphDev dev;
  if (graph) {
    const int S_ = graph->n_states(), A = graph->n_arcs();
    const int32_t* w = static_cast<const int32_t*>(workspace);
    dev.n_states = S_; dev.n_arcs = A;
    dev.arc_begin = w;
    dev.escape = reinterpret_cast<const float*>(w + S_ + 1);
    dev.arc_label = w + 2 * S_ + 1;
    dev.arc_next = w + 2 * S_ + 1 + A;
    dev.arc_weight = reinterpret_cast<const float*>(w + 2 * S_ + 1 + 2 * A);
  }
  // nothing is copied for a call the launcher refuses: its checks first, on a launcher call that launches nothing (B = 0)
  if (!pfhip::launch_ctc_prefix_beam(topk_ids, topk_logp, k, rows, row_off, len, 0, V, blank, first_beam, second_beam, dev, nbest, max_tokens,
                                     n_hyp, ids, n_tokens, score, ctc_score, ctx_score, nullptr, 0, S(stream)))
    return (int)hipErrorInvalidValue;
  if (B < 0 || B > 65535 || workspace_bytes - gbytes < pfhip::ctc_prefix_beam_workspace_bytes(rows, B, second_beam))
    return (int)hipErrorInvalidValue;
  // ... and the buffers the launcher would refuse at B > 0, before the graph is copied
  if (B > 0 && (!row_off || !len || !n_hyp || !n_tokens || !score || !ctc_score || !ctx_score || (max_tokens > 0 && !ids) ||
                (rows > 0 && (!topk_ids || !topk_logp))))
    return (int)hipErrorInvalidValue;
  if (graph && B > 0) {
    // the graph's memory is the handle's and pageable: the copy has left it when the call returns
    const hipError_t e = hipMemcpyAsync(workspace, graph->packed.data(), graph->packed.size() * 4, hipMemcpyHostToDevice, S(stream));
    if (e != hipSuccess) return (int)e;
  }
  if (!pfhip::launch_ctc_prefix_beam(topk_ids, topk_logp, k, rows, row_off, len, B, V, blank, first_beam, second_beam, dev, nbest, max_tokens,
                                     n_hyp, ids, n_tokens, score, ctc_score, ctx_score, static_cast<char*>(workspace) + gbytes,
                                     workspace_bytes - gbytes, S(stream)))
    return (int)hipErrorInvalidValue;
  return done();
}
// every utterance on its own beams and graph: the descriptors are HOST arrays, checked here before anything is copied or launched,
// then taken to the front of the workspace with the graphs' images in one copy (beam_front.h)
static bool beam_multi_args(const int* first_beam, const int* second_beam, const int* nbest, const int* graph_of, int B, int k,
                            const pfhip_ctx_graph* const* graphs, int n_graphs, int V, std::vector<pfhip::BeamUtt>* utt, int* sb_max, int* nb_max) {
  if (B < 0 || B > 65535 || n_graphs < 0 || (n_graphs > 0 && !graphs) || (B > 0 && (!first_beam || !second_beam || !nbest || !graph_of)))
    return false;
  for (int g = 0; g < n_graphs; ++g)
    if (!graphs[g] || graphs[g]->vocab != V) return false;
  utt->resize((size_t)B);
  for (int b = 0; b < B; ++b) (*utt)[b] = pfhip::BeamUtt{first_beam[b], second_beam[b], nbest[b], graph_of[b]};
  return pfhip::ctc_prefix_beam_multi_check(utt->data(), B, k, n_graphs, sb_max, nb_max);
}
size_t pfhip_op_ctc_prefix_beam_multi_workspace_bytes(long long rows, int B, int k, const int* first_beam, const int* second_beam, const int* nbest,
                                                      const int* graph_of, const pfhip_ctx_graph* const* graphs, int n_graphs) {
  std::vector<pfhip::BeamUtt> utt;
  int sb_max = 1, nb_max = 1;
  if (n_graphs < 0 || (n_graphs > 0 && !graphs)) return 0;
  for (int g = 0; g < n_graphs; ++g)
    if (!graphs[g]) return 0;
  if (!beam_multi_args(first_beam, second_beam, nbest, graph_of, B, k, graphs, n_graphs, n_graphs ? graphs[0]->vocab : 1, &utt, &sb_max, &nb_max))
    return 0;
  const size_t nodes = pfhip::ctc_prefix_beam_workspace_bytes(rows, B, sb_max);
  return nodes ? nodes + pfhip::beam_front_bytes(B, graphs, n_graphs) : 0;
}
int pfhip_op_ctc_prefix_beam_multi(const int32_t* topk_ids, const float* topk_logp, int k, long long rows, const int* row_off, const int* len,
                                   int B, int V, int blank, const int* first_beam, const int* second_beam, const int* nbest,
                                   const int* graph_of, const pfhip_ctx_graph* const* graphs, int n_graphs, int max_tokens, int32_t* n_hyp,
                                   int32_t* ids, int32_t* n_tokens, float* score, float* ctc_score, float* ctx_score, void* workspace,
                                   size_t workspace_bytes, void* stream) {
  std::vector<pfhip::BeamUtt> utt;
  int sb_max = 1, nb_max = 1;
  if (!beam_multi_args(first_beam, second_beam, nbest, graph_of, B, k, graphs, n_graphs, V, &utt, &sb_max, &nb_max)) return (int)hipErrorInvalidValue;
  // the launcher's own checks, on a call that launches nothing (B = 0), then the buffers it would refuse at B > 0
  if (!pfhip::launch_ctc_prefix_beam_multi(topk_ids, topk_logp, k, rows, row_off, len, 0, V, blank, nullptr, nullptr, n_graphs, sb_max, nb_max,
                                           max_tokens, n_hyp, ids, n_tokens, score, ctc_score, ctx_score, nullptr, 0, S(stream)))
    return (int)hipErrorInvalidValue;
  const size_t front = pfhip::beam_front_bytes(B, graphs, n_graphs), nodes = pfhip::ctc_prefix_beam_workspace_bytes(rows, B, sb_max);
  if (!workspace || workspace_bytes < front || workspace_bytes - front < nodes) return (int)hipErrorInvalidValue;
  if (B > 0 && (!row_off || !len || !n_hyp || !n_tokens || !score || !ctc_score || !ctx_score || (max_tokens > 0 && !ids) ||
                (rows > 0 && (!topk_ids || !topk_logp))))
    return (int)hipErrorInvalidValue;
  if (B == 0) return done();
  char* const dev = static_cast<char*>(workspace);
  std::vector<char> host(front, 0);
  pfhip::beam_front_fill(host.data(), dev, utt.data(), B, graphs, n_graphs);
  {
    // pageable memory: the copy has left it when the call returns
    const hipError_t e = hipMemcpyAsync(dev, host.data(), front, hipMemcpyHostToDevice, S(stream));
    if (e != hipSuccess) return (int)e;
  }
  if (!pfhip::launch_ctc_prefix_beam_multi(topk_ids, topk_logp, k, rows, row_off, len, B, V, blank, reinterpret_cast<const pfhip::BeamUtt*>(dev),
                                           reinterpret_cast<const pfhip::CtxGraphDev*>(dev + pfhip::beam_front_table_off(B)), n_graphs, sb_max,
                                           nb_max, max_tokens, n_hyp, ids, n_tokens, score, ctc_score, ctx_score, dev + front,
                                           workspace_bytes - front, S(stream)))
    return (int)hipErrorInvalidValue;
  return done();
}
// the search over a non-autoregressive head's candidates (nar_beam.hip): the same shape of entry, width >= 1 for every utterance
static bool nar_beam_args(const int* width, const int* beam, const int* nbest, const int* graph_of, int B, int k,
                          const pfhip_ctx_graph* const* graphs, int n_graphs, int V, std::vector<pfhip::BeamUtt>* utt, int* beam_max, int* nb_max) {
  if (B < 0 || B > 65535 || n_graphs < 0 || (n_graphs > 0 && !graphs) || (B > 0 && (!width || !beam || !nbest || !graph_of))) return false;
  for (int g = 0; g < n_graphs; ++g)
    if (!graphs[g] || graphs[g]->vocab != V) return false;
  utt->resize((size_t)B);
  for (int b = 0; b < B; ++b) (*utt)[b] = pfhip::BeamUtt{width[b], beam[b], nbest[b], graph_of[b]};
  return pfhip::nbest_ctx_beam_check(utt->data(), B, k, n_graphs, false, beam_max, nb_max);
}
size_t pfhip_op_nbest_ctx_beam_workspace_bytes(long long rows, int B, int k, const int* width, const int* beam, const int* nbest,
                                               const int* graph_of, const pfhip_ctx_graph* const* graphs, int n_graphs) {
  std::vector<pfhip::BeamUtt> utt;
  int beam_max = 1, nb_max = 1;
  if (n_graphs < 0 || (n_graphs > 0 && !graphs)) return 0;
  for (int g = 0; g < n_graphs; ++g)
    if (!graphs[g]) return 0;
  if (!nar_beam_args(width, beam, nbest, graph_of, B, k, graphs, n_graphs, n_graphs ? graphs[0]->vocab : 1, &utt, &beam_max, &nb_max)) return 0;
  const size_t nodes = pfhip::nbest_ctx_beam_workspace_bytes(rows, B, beam_max);
  return nodes ? nodes + pfhip::beam_front_bytes(B, graphs, n_graphs) : 0;
}
int pfhip_op_nbest_ctx_beam(const int32_t* cand_ids, const float* cand_logp, int k, long long rows, const int* row_off, const int* len, int B,
                            int V, const int* width, const int* beam, const int* nbest, const int* graph_of,
                            const pfhip_ctx_graph* const* graphs, int n_graphs, int max_tokens, int32_t* n_hyp, int32_t* ids,
                            int32_t* n_tokens, float* score, float* am_score, float* ctx_score, void* workspace, size_t workspace_bytes,
                            void* stream) {
  std::vector<pfhip::BeamUtt> utt;
  int beam_max = 1, nb_max = 1;
  if (!nar_beam_args(width, beam, nbest, graph_of, B, k, graphs, n_graphs, V, &utt, &beam_max, &nb_max)) return (int)hipErrorInvalidValue;
  // the launcher's own checks, on a call that launches nothing (B = 0), then the buffers it would refuse at B > 0
  if (!pfhip::launch_nbest_ctx_beam(cand_ids, cand_logp, k, rows, row_off, len, nullptr, 0, V, nullptr, nullptr, n_graphs, beam_max, nb_max, max_tokens,
                                    n_hyp, ids, n_tokens, score, am_score, ctx_score, nullptr, 0, S(stream)))
    return (int)hipErrorInvalidValue;
  const size_t front = pfhip::beam_front_bytes(B, graphs, n_graphs), nodes = pfhip::nbest_ctx_beam_workspace_bytes(rows, B, beam_max);
  if (!workspace || workspace_bytes < front || workspace_bytes - front < nodes) return (int)hipErrorInvalidValue;
  if (B > 0 && (!row_off || !len || !n_hyp || !n_tokens || !score || !am_score || !ctx_score || (max_tokens > 0 && !ids) ||
                (rows > 0 && (!cand_ids || !cand_logp))))
    return (int)hipErrorInvalidValue;
  if (B == 0) return done();
  char* const dev = static_cast<char*>(workspace);
  std::vector<char> host(front, 0);
  pfhip::beam_front_fill(host.data(), dev, utt.data(), B, graphs, n_graphs);
  {
    // pageable memory: the copy has left it when the call returns
    const hipError_t e = hipMemcpyAsync(dev, host.data(), front, hipMemcpyHostToDevice, S(stream));
    if (e != hipSuccess) return (int)e;
  }
  if (!pfhip::launch_nbest_ctx_beam(cand_ids, cand_logp, k, rows, row_off, len, nullptr, B, V, reinterpret_cast<const pfhip::BeamUtt*>(dev),
                                    reinterpret_cast<const pfhip::CtxGraphDev*>(dev + pfhip::beam_front_table_off(B)), n_graphs, beam_max,
                                    nb_max, max_tokens, n_hyp, ids, n_tokens, score, am_score, ctx_score, dev + front,
                                    workspace_bytes - front, S(stream)))
    return (int)hipErrorInvalidValue;
  return done();
}
// the CTC search with a token n-gram language model: its image follows the front block in the call's one copy.  lm == NULL is the
// sibling entry, argument for argument.
size_t pfhip_op_ctc_prefix_beam_multi_lm_workspace_bytes(long long rows, int B, int k, const int* first_beam, const int* second_beam,
                                                         const int* nbest, const int* graph_of, const pfhip_ctx_graph* const* graphs,
                                                         int n_graphs, const pfhip_lm_graph* lm) {
  const size_t plain = pfhip_op_ctc_prefix_beam_multi_workspace_bytes(rows, B, k, first_beam, second_beam, nbest, graph_of, graphs, n_graphs);
  return plain ? plain + pfhip::lm_graph_image_bytes(lm) : 0;
}
int pfhip_op_ctc_prefix_beam_multi_lm(const int32_t* topk_ids, const float* topk_logp, int k, long long rows, const int* row_off, const int* len,
                                      int B, int V, int blank, const int* first_beam, const int* second_beam, const int* nbest,
                                      const int* graph_of, const pfhip_ctx_graph* const* graphs, int n_graphs, const pfhip_lm_graph* lm,
                                      int max_tokens, int32_t* n_hyp, int32_t* ids, int32_t* n_tokens, float* score, float* ctc_score,
                                      float* ctx_score, float* lm_score, void* workspace, size_t workspace_bytes, void* stream) {
  if (!lm_score) return (int)hipErrorInvalidValue;
  std::vector<pfhip::BeamUtt> utt;
  int sb_max = 1, nb_max = 1;
  if (!lm) {
    const int e = pfhip_op_ctc_prefix_beam_multi(topk_ids, topk_logp, k, rows, row_off, len, B, V, blank, first_beam, second_beam, nbest, graph_of,
                                                 graphs, n_graphs, max_tokens, n_hyp, ids, n_tokens, score, ctc_score, ctx_score, workspace,
                                                 workspace_bytes, stream);
    if (e != 0 || B == 0) return e;
    beam_multi_args(first_beam, second_beam, nbest, graph_of, B, k, graphs, n_graphs, V, &utt, &sb_max, &nb_max);      // passed above
    const hipError_t z = hipMemsetAsync(lm_score, 0, sizeof(float) * (size_t)B * nb_max, S(stream));
    return z != hipSuccess ? (int)z : done();
  }
  if (lm->vocab != V) return (int)hipErrorInvalidValue;
  if (!beam_multi_args(first_beam, second_beam, nbest, graph_of, B, k, graphs, n_graphs, V, &utt, &sb_max, &nb_max)) return (int)hipErrorInvalidValue;
  // the launcher's own checks, on a call that launches nothing (B = 0), then the buffers it would refuse at B > 0
  if (!pfhip::launch_ctc_prefix_beam_multi_lm(topk_ids, topk_logp, k, rows, row_off, len, 0, V, blank, nullptr, nullptr, n_graphs,
                                              pfhip::lm_graph_dev(lm, nullptr), sb_max, nb_max, max_tokens, n_hyp, ids, n_tokens, score,
                                              ctc_score, ctx_score, lm_score, nullptr, 0, S(stream)))
    return (int)hipErrorInvalidValue;
  const size_t front = pfhip::beam_front_bytes(B, graphs, n_graphs), image = pfhip::lm_graph_image_bytes(lm),
               nodes = pfhip::ctc_prefix_beam_workspace_bytes(rows, B, sb_max);
  if (!workspace || workspace_bytes < front + image || workspace_bytes - front - image < nodes) return (int)hipErrorInvalidValue;
  if (B > 0 && (!row_off || !len || !n_hyp || !n_tokens || !score || !ctc_score || !ctx_score || (max_tokens > 0 && !ids) ||
                (rows > 0 && (!topk_ids || !topk_logp))))
    return (int)hipErrorInvalidValue;
  if (B == 0) return done();
  char* const dev = static_cast<char*>(workspace);
  std::vector<char> host(front + image, 0);
  pfhip::beam_front_fill(host.data(), dev, utt.data(), B, graphs, n_graphs);
  std::memcpy(host.data() + front, lm->packed.data(), lm->packed.size() * 4);
  {
    // pageable memory: the copy has left it when the call returns
    const hipError_t e = hipMemcpyAsync(dev, host.data(), front + image, hipMemcpyHostToDevice, S(stream));
    if (e != hipSuccess) return (int)e;
  }
  if (!pfhip::launch_ctc_prefix_beam_multi_lm(topk_ids, topk_logp, k, rows, row_off, len, B, V, blank, reinterpret_cast<const pfhip::BeamUtt*>(dev),
                                              reinterpret_cast<const pfhip::CtxGraphDev*>(dev + pfhip::beam_front_table_off(B)), n_graphs,
                                              pfhip::lm_graph_dev(lm, dev + front), sb_max, nb_max, max_tokens, n_hyp, ids, n_tokens, score,
                                              ctc_score, ctx_score, lm_score, dev + front + image, workspace_bytes - front - image, S(stream)))
    return (int)hipErrorInvalidValue;
  return done();
}
// the search over a non-autoregressive head's candidates the same way
size_t pfhip_op_nbest_ctx_beam_lm_workspace_bytes(long long rows, int B, int k, const int* width, const int* beam, const int* nbest,
                                                  const int* graph_of, const pfhip_ctx_graph* const* graphs, int n_graphs,
                                                  const pfhip_lm_graph* lm) {
  const size_t plain = pfhip_op_nbest_ctx_beam_workspace_bytes(rows, B, k, width, beam, nbest, graph_of, graphs, n_graphs);
  return plain ? plain + pfhip::lm_graph_image_bytes(lm) : 0;
}
int pfhip_op_nbest_ctx_beam_lm(const int32_t* cand_ids, const float* cand_logp, int k, long long rows, const int* row_off, const int* len, int B,
                               int V, const int* width, const int* beam, const int* nbest, const int* graph_of,
                               const pfhip_ctx_graph* const* graphs, int n_graphs, const pfhip_lm_graph* lm, int max_tokens, int32_t* n_hyp,
                               int32_t* ids, int32_t* n_tokens, float* score, float* am_score, float* ctx_score, float* lm_score,
                               void* workspace, size_t workspace_bytes, void* stream) {
  if (!lm_score) return (int)hipErrorInvalidValue;
  if (!lm) {
    const int e = pfhip_op_nbest_ctx_beam(cand_ids, cand_logp, k, rows, row_off, len, B, V, width, beam, nbest, graph_of, graphs, n_graphs,
                                          max_tokens, n_hyp, ids, n_tokens, score, am_score, ctx_score, workspace, workspace_bytes, stream);
    if (e != 0 || B == 0) return e;
    int nb_max = 1;
    for (int b = 0; b < B; ++b) nb_max = std::max(nb_max, nbest[b]);
    const hipError_t z = hipMemsetAsync(lm_score, 0, sizeof(float) * (size_t)B * nb_max, S(stream));
    return z != hipSuccess ? (int)z : done();
  }
  if (lm->vocab != V) return (int)hipErrorInvalidValue;
  std::vector<pfhip::BeamUtt> utt;
  int beam_max = 1, nb_max = 1;
  if (!nar_beam_args(width, beam, nbest, graph_of, B, k, graphs, n_graphs, V, &utt, &beam_max, &nb_max)) return (int)hipErrorInvalidValue;
  // the launcher's own checks, on a call that launches nothing (B = 0), then the buffers it would refuse at B > 0
  const pfhip::LmGraphDev probe = pfhip::lm_graph_dev(lm, nullptr);
  if (!pfhip::launch_nbest_ctx_beam_lm(cand_ids, cand_logp, k, rows, row_off, len, nullptr, 0, V, nullptr, nullptr, n_graphs, probe, beam_max, nb_max,
                                       max_tokens, n_hyp, ids, n_tokens, score, am_score, ctx_score, lm_score, nullptr, 0, S(stream)))
    return (int)hipErrorInvalidValue;
  const size_t front = pfhip::beam_front_bytes(B, graphs, n_graphs), image = pfhip::lm_graph_image_bytes(lm),
               nodes = pfhip::nbest_ctx_beam_workspace_bytes(rows, B, beam_max);
  if (!workspace || workspace_bytes < front + image || workspace_bytes - front - image < nodes) return (int)hipErrorInvalidValue;
  if (B > 0 && (!row_off || !len || !n_hyp || !n_tokens || !score || !am_score || !ctx_score || (max_tokens > 0 && !ids) ||
                (rows > 0 && (!cand_ids || !cand_logp))))
    return (int)hipErrorInvalidValue;
  if (B == 0) return done();
  char* const dev = static_cast<char*>(workspace);
  std::vector<char> host(front + image, 0);
  pfhip::beam_front_fill(host.data(), dev, utt.data(), B, graphs, n_graphs);
  std::memcpy(host.data() + front, lm->packed.data(), lm->packed.size() * 4);
  {
    // pageable memory: the copy has left it when the call returns
    const hipError_t e = hipMemcpyAsync(dev, host.data(), front + image, hipMemcpyHostToDevice, S(stream));
    if (e != hipSuccess) return (int)e;
  }
  if (!pfhip::launch_nbest_ctx_beam_lm(cand_ids, cand_logp, k, rows, row_off, len, nullptr, B, V, reinterpret_cast<const pfhip::BeamUtt*>(dev),
                                       reinterpret_cast<const pfhip::CtxGraphDev*>(dev + pfhip::beam_front_table_off(B)), n_graphs,
                                       pfhip::lm_graph_dev(lm, dev + front), beam_max, nb_max, max_tokens, n_hyp, ids, n_tokens, score, am_score,
                                       ctx_score, lm_score, dev + front + image, workspace_bytes - front - image, S(stream)))
    return (int)hipErrorInvalidValue;
  return done();
}
// sentences scored by the model (lm_score.hip): the image goes to the workspace first
size_t pfhip_op_lm_score_workspace_bytes(const pfhip_lm_graph* lm) { return pfhip::lm_graph_image_bytes(lm); }
int pfhip_op_lm_score(const int32_t* ids, const int* len, int B, int max_len, const pfhip_lm_graph* lm, float* tok_w, float* eos_w, float* total,
                      void* workspace, size_t workspace_bytes, void* stream) {
  static_assert(pfhip::kLmOrderMax == PFHIP_LM_ORDER_MAX, "one cap for the builder and the device loop");
  if (!lm || B < 0 || max_len < 0) return (int)hipErrorInvalidValue;
  const size_t image = pfhip::lm_graph_image_bytes(lm);
  if (!workspace || workspace_bytes < image) return (int)hipErrorInvalidValue;
  if (!pfhip::launch_lm_score(ids, len, 0, max_len, pfhip::lm_graph_dev(lm, nullptr), tok_w, eos_w, total, S(stream)) ||
      (long long)B * max_len > 0x7fffffffLL)
    return (int)hipErrorInvalidValue;
  if (B > 0 && (!len || !eos_w || !total || (max_len > 0 && (!ids || !tok_w)))) return (int)hipErrorInvalidValue;
  if (B == 0) return done();
  {
    // the graph's memory is the handle's and pageable: the copy has left it when the call returns
    const hipError_t e = hipMemcpyAsync(workspace, lm->packed.data(), lm->packed.size() * 4, hipMemcpyHostToDevice, S(stream));
    if (e != hipSuccess) return (int)e;
  }
  if (!pfhip::launch_lm_score(ids, len, B, max_len, pfhip::lm_graph_dev(lm, workspace), tok_w, eos_w, total, S(stream)))
    return (int)hipErrorInvalidValue;
  return done();
}
size_t pfhip_op_ctc_align_workspace_bytes(size_t e_floats) { return pfhip::ctc_align_workspace_bytes(e_floats); }
int pfhip_op_ctc_align_max_tokens(void) { return pfhip::ctc_align_max_tokens(); }
int pfhip_op_ctc_align(const float* E, const long long* e_off, size_t e_floats, const int* len, const int* n_lab, const int32_t* labels,
                       const int* lab_off, int B, int max_tokens, int32_t* tok_begin, int32_t* tok_end, float* tok_logp, float* score,
                       void* workspace, size_t workspace_bytes, void* stream) {
  if (!pfhip::launch_ctc_align(E, e_off, e_floats, len, n_lab, labels, lab_off, B, max_tokens, tok_begin, tok_end, tok_logp, score, workspace,
                               workspace_bytes, S(stream)))
    return (int)hipErrorInvalidValue;
  return done();
}

// ---- the scan, cache and row kernels (tests only: the descriptor-taking ones upload their descriptors synchronously) ----------------
static int cif_stream_op(const float* enc, int lde, const float* alphas, const int* row_off, const int* n, const int* is_last,
                        const int* pre, const int* suf, float* carry, long long carry_stride, int B, int D, float threshold,
                        float tail, float* emb, int emb_rows, int* n_fire, int* fire_step, void* stream) {
  if (B <= 0 || D <= 0 || D > 1024 || lde < D || emb_rows < 0 || carry_stride < D + 1 || !enc || !alphas || !row_off || !n || !is_last ||
      !pre || !suf || !carry || !emb || !n_fire)
    return (int)hipErrorInvalidValue;
  std::vector<pfhip::StreamSeg> segs((size_t)B);
  for (int b = 0; b < B; ++b) {
    if (row_off[b] < 0 || n[b] < 0) return (int)hipErrorInvalidValue;
    pfhip::StreamSeg sg{};
    sg.carry = carry + (size_t)b * carry_stride;
    sg.row_off = row_off[b]; sg.n = n[b];
    sg.is_last = is_last[b]; sg.pre = pre[b]; sg.suf = suf[b];
    segs[b] = sg;
  }
  return with_device_segs(segs, S(stream), [&](const pfhip::StreamSeg* d) {
    pfhip::launch_cif_stream(enc, lde, alphas, d, B, threshold, tail, emb, emb_rows, n_fire, D, S(stream), fire_step);
  });
}
int pfhip_op_cif_stream(const float* enc, int lde, const float* alphas, const int* row_off, const int* n, const int* is_last,
                        const int* pre, const int* suf, float* carry, long long carry_stride, int B, int D, float threshold,
                        float tail, float* emb, int emb_rows, int* n_fire, void* stream) {
  return cif_stream_op(enc, lde, alphas, row_off, n, is_last, pre, suf, carry, carry_stride, B, D, threshold, tail, emb, emb_rows, n_fire,
                       nullptr, stream);
}
int pfhip_op_cif_stream_fires(const float* enc, int lde, const float* alphas, const int* row_off, const int* n, const int* is_last,
                              const int* pre, const int* suf, float* carry, long long carry_stride, int B, int D, float threshold,
                              float tail, float* emb, int emb_rows, int* n_fire, int* fire_step, void* stream) {
  if (!fire_step) return (int)hipErrorInvalidValue;
  return cif_stream_op(enc, lde, alphas, row_off, n, is_last, pre, suf, carry, carry_stride, B, D, threshold, tail, emb, emb_rows, n_fire,
                       fire_step, stream);
}
int pfhip_op_fsmn_cached(const float* t2, const float* w, const float* res, float* out, const int* tok_off, const int* n_tok, float* dcache,
                         long long dcache_stride, int B, int layer, int C, void* stream) {
  if (B <= 0 || C <= 0 || C % 4 || layer < 0 || dcache_stride < (long long)(layer + 1) * 10 * C || dcache_stride % 4 || !t2 || !w || !res ||
      !out || !tok_off || !n_tok || !dcache)
    return (int)hipErrorInvalidValue;
  std::vector<pfhip::StreamSeg> segs((size_t)B);
  for (int b = 0; b < B; ++b) {
    if (tok_off[b] < 0) return (int)hipErrorInvalidValue;
    pfhip::StreamSeg sg{};
    sg.dcache = dcache + (size_t)b * dcache_stride;
    sg.tok_off = tok_off[b]; sg.n_tok = n_tok[b];
    segs[b] = sg;
  }
  return with_device_segs(segs, S(stream), [&](const pfhip::StreamSeg* d) {
    pfhip::launch_fsmn_cached(t2, w, res, out, d, B, layer, C, S(stream));
  });
}
int pfhip_op_fsmn_causal20(const float* p, int ldp, const float* w, const int* row_off, const int* T, const int* final,
                           const float* cache_in, float* cache_out, long long cache_stride, int B, int layer, float* out, int ldo, int C,
                           void* stream) {
  if (B <= 0 || C <= 0 || C % 4 || ldp % 4 || ldo % 4 || ldp < C || ldo < C || layer < 0 || cache_stride < (long long)(layer + 1) * 19 * C ||
      cache_stride % 4 || !p || !w || !row_off || !T || !final || !cache_in || !cache_out || cache_in == cache_out || !out)
    return (int)hipErrorInvalidValue;
  std::vector<pfhip::VadSeg> segs((size_t)B);
  int max_T = 0;
  for (int b = 0; b < B; ++b) {
    if (row_off[b] < 0 || T[b] < 0) return (int)hipErrorInvalidValue;
    segs[b] = pfhip::VadSeg{cache_in + (size_t)b * cache_stride, final[b] ? nullptr : cache_out + (size_t)b * cache_stride, row_off[b], T[b]};
    if (T[b] > max_T) max_T = T[b];
  }
  return with_device_segs(segs, S(stream), [&](const pfhip::VadSeg* d) {
    pfhip::launch_fsmn_causal20(p, ldp, w, d, B, max_T, layer, out, ldo, C, S(stream));
  });
}
int pfhip_op_softmax_rows(const float* x, int ldx, int M, int N, float* y, float* col0, void* stream) {
  if (M < 0 || N <= 0 || ldx < N || !x || !y) return (int)hipErrorInvalidValue;
  pfhip::launch_softmax_rows(x, ldx, M, N, y, col0, S(stream));
  return done();
}
int pfhip_op_frame_energy(const float* pcm, const int64_t* sample_off, const int* frame_off, const int* nframes, int B, int total_frames,
                          int flen, int fshift, float* e, void* stream) {
  if (B < 0 || total_frames < 0 || !sample_off || !frame_off || !nframes || (total_frames && (!pcm || !e))) return (int)hipErrorInvalidValue;
  if (!pfhip::launch_frame_energy(pcm, sample_off, frame_off, nframes, B, total_frames, flen, fshift, e, S(stream))) return (int)hipErrorInvalidValue;
  return done();
}
int pfhip_op_frame_energy_s16(const int16_t* pcm, const int64_t* sample_off, const int* frame_off, const int* nframes, int B,
                              int total_frames, int flen, int fshift, float* e, void* stream) {
  if (B < 0 || total_frames < 0 || !sample_off || !frame_off || !nframes || (total_frames && (!pcm || !e))) return (int)hipErrorInvalidValue;
  if (!pfhip::launch_frame_energy(pcm, sample_off, frame_off, nframes, B, total_frames, flen, fshift, e, S(stream))) return (int)hipErrorInvalidValue;
  return done();
}
int pfhip_op_im2col3(const float* h, int ldh, float* col, int ldc, const int* row_pos, const int* row_len, int M, int D, void* stream) {
  if (M < 0 || D <= 0 || D % 4 || ldh % 4 || ldc % 4 || ldh < D || ldc < 3 * D || !h || !col || !row_pos || !row_len) return (int)hipErrorInvalidValue;
  pfhip::launch_im2col3(h, ldh, col, ldc, row_pos, row_len, M, D, S(stream));
  return done();
}
int pfhip_op_alpha(const float* o, int ldo, const float* w, const float* b, float smooth, float noise, float* alphas, int M, int D,
                   void* stream) {
  if (M < 0 || D <= 0 || D % 4 || ldo % 4 || ldo < D || !o || !w || !b || !alphas) return (int)hipErrorInvalidValue;
  pfhip::launch_alpha(o, ldo, w, b, smooth, noise, alphas, M, D, S(stream));
  return done();
}
int pfhip_op_alpha2(const float* y, int ldy, const float* w, float b, float smooth, float noise, float* a2, int rows, int D, void* stream) {
  if (rows < 0 || D <= 0 || D % 4 || ldy % 4 || ldy < D || !y || !w || !a2) return (int)hipErrorInvalidValue;
  pfhip::launch_alpha2(y, ldy, w, b, smooth, noise, a2, rows, D, S(stream));
  return done();
}
int pfhip_op_us_cif(const float* a2, const int* off, const int* len, const int* token_num, int B, int max_len, float threshold,
                    float* us_alphas, float* us_peaks, void* stream) {
  if (B < 0 || max_len < 0 || !a2 || !off || !len || !token_num || !us_alphas || !us_peaks) return (int)hipErrorInvalidValue;
  pfhip::launch_us_cif(a2, off, len, token_num, B, max_len, threshold, us_alphas, us_peaks, S(stream));
  return done();
}
int pfhip_op_blstm_scratch_floats(void) { return pfhip::kBlstmScratchFloats; }
int pfhip_op_blstm_flag_word(void) { return pfhip::kBlstmFlagWord; }
int pfhip_op_blstm(const float* gx, const float* whh, float* y, const int* off, const int* len, int B, int Lmax, int stepwise, float* hx,
                   float* cst, void* stream) {
  if (B < 0 || B > 32 || Lmax < 0 || !gx || !whh || !y || !off || !len || !hx || (stepwise && !cst)) return (int)hipErrorInvalidValue;
  if (B == 0 || Lmax == 0) return 0;
  const hipError_t e = stepwise ? pfhip::launch_blstm_stepwise(gx, whh, y, hx, cst, off, len, B, Lmax, S(stream))
                                : pfhip::launch_blstm(gx, whh, y, hx, off, len, B, Lmax, S(stream));
  return (int)e;
}
int pfhip_op_lstm_cell(const float* G, float* c, float* h, const int32_t* lens, int t, float* sel, int H, int D, void* stream) {
  if (H < 0 || D <= 0 || !G || !c || !h || !lens || !sel) return (int)hipErrorInvalidValue;
  pfhip::launch_lstm_cell(G, c, h, lens, t, sel, H, D, S(stream));
  return done();
}

}  // extern "C"

// ---- the front-end kernels, the LFR/CMVN family, the PE kernels, the row gathers and small reductions (tests only) -------------------
namespace {
constexpr int kInvalid = (int)hipErrorInvalidValue;
// launch, then wait: the entries below free what they uploaded when they return
template <class Launch>
int launch_and_drain(hipStream_t s, Launch launch) {
  launch();
  hipError_t e = hipGetLastError();
  const hipError_t e2 = hipStreamSynchronize(s);
  return (int)(e == hipSuccess ? e2 : e);
}
// The fbank kernel in either launch form from HOST index arrays.  Everything the kernel assumes is checked here: every frame it reads
// lies inside pcm (pcm_samples samples), every row it writes inside feats (feats_rows rows of 560) or fb_out (total_frames rows of 80).
template <typename Sample>
int fbank_op(const Sample* pcm, long long pcm_samples, const int64_t* sample_off, const int* frame_off, const int* nframes, int B,
             int total_frames, float* fb_out, float* feats, long long feats_rows, const int* row_off, const float* cmvn_mean,
             const float* cmvn_istd, void* stream) {
  const bool raw = fb_out != nullptr;
  if (!pcm || !sample_off || !frame_off || !nframes || B < 1 || total_frames < 0 || pcm_samples < 0 || raw == (feats != nullptr))
    return kInvalid;
  if (!raw && (!row_off || !cmvn_mean || !cmvn_istd || feats_rows < 0)) return kInvalid;
  if (frame_off[0] != 0 || frame_off[B] != total_frames) return kInvalid;
  for (int b = 0; b < B; ++b) {
    const int nf = nframes[b];
    if (nf < 0 || frame_off[b + 1] - frame_off[b] != nf) return kInvalid;
    if (nf == 0) continue;
    if (sample_off[b] < 0 || sample_off[b] + 400 + 160LL * (nf - 1) > pcm_samples) return kInvalid;
    if (!raw && (row_off[b] < 0 || row_off[b] + (nf + 5) / 6 > feats_rows)) return kInvalid;
  }
  if (total_frames == 0) return 0;
  pfhip_impl::FrontendTables ft;
  if (pfhip_impl::build_frontend_tables(80, 16000, &ft) != PFHIP_OK) return (int)hipErrorUnknown;
  pfhip_impl::DevMem d_so, d_fo, d_nf, d_ro;
  hipError_t e = d_so.upload(sample_off, sizeof(int64_t) * B);
  if (e == hipSuccess) e = d_fo.upload(frame_off, sizeof(int) * (B + 1));
  if (e == hipSuccess) e = d_nf.upload(nframes, sizeof(int) * B);
  if (e == hipSuccess && !raw) e = d_ro.upload(row_off, sizeof(int) * B);
  if (e != hipSuccess) return (int)e;
  const pfhip::FbankTables tb = ft.fbank(cmvn_mean, cmvn_istd);
  return launch_and_drain(S(stream), [&] {
    if (!raw)
      pfhip::launch_fbank_lfr_cmvn(pcm, d_so.as<int64_t>(), d_fo.as<int>(), d_nf.as<int>(), d_ro.as<int>(), B, total_frames, tb, feats, S(stream));
    else if (B == 1)
      pfhip::launch_fbank_frames(pcm, d_so.as<int64_t>(), d_fo.as<int>(), d_nf.as<int>(), total_frames, tb, fb_out, S(stream));
    else
      pfhip::launch_fbank_frames_batch(pcm, d_so.as<int64_t>(), d_fo.as<int>(), d_nf.as<int>(), B, total_frames, tb, fb_out, S(stream));
  });
}
inline bool lfr_shape_ok(int m, int n, int n_mels, int ldo) {
  return m >= 1 && n >= 1 && n_mels >= 1 && (long long)m * n_mels <= ldo;
}
}  // namespace

extern "C" {

int pfhip_op_fbank(const float* pcm, long long pcm_samples, const int64_t* sample_off, const int* frame_off, const int* nframes, int B,
                   int total_frames, float* fb_out, float* feats, long long feats_rows, const int* row_off, const float* cmvn_mean,
                   const float* cmvn_istd, void* stream) {
  return fbank_op(pcm, pcm_samples, sample_off, frame_off, nframes, B, total_frames, fb_out, feats, feats_rows, row_off, cmvn_mean, cmvn_istd,
                  stream);
}
int pfhip_op_fbank_s16(const int16_t* pcm, long long pcm_samples, const int64_t* sample_off, const int* frame_off, const int* nframes, int B,
                       int total_frames, float* fb_out, float* feats, long long feats_rows, const int* row_off, const float* cmvn_mean,
                       const float* cmvn_istd, void* stream) {
  return fbank_op(pcm, pcm_samples, sample_off, frame_off, nframes, B, total_frames, fb_out, feats, feats_rows, row_off, cmvn_mean, cmvn_istd,
                  stream);
}

int pfhip_op_lfr_cmvn(const float* fb, int F, int m, int n, int n_mels, const float* mean, const float* istd, float* out, int ldo,
                      void* stream) {
  if (!fb || !mean || !istd || !out || F < 0 || !lfr_shape_ok(m, n, n_mels, ldo)) return kInvalid;
  pfhip::launch_lfr_cmvn(fb, F, (F + n - 1) / n, m, n, n_mels, mean, istd, out, ldo, S(stream));
  return done();
}
int pfhip_op_lfr_cmvn_packed(const float* fb, long long fb_frames, const int* frame_off, const int* nframes, const int* row_off, int B,
                             int m, int n, int n_mels, const float* mean, const float* istd, float* out, int ldo, long long out_rows,
                             void* stream) {
  if (!fb || !frame_off || !nframes || !row_off || !mean || !istd || !out || B < 1 || fb_frames < 0 || out_rows < 0 ||
      !lfr_shape_ok(m, n, n_mels, ldo))
    return kInvalid;
  int max_T = 0;
  for (int b = 0; b < B; ++b) {
    const int T = nframes[b] < 0 ? -1 : (nframes[b] + n - 1) / n;
    if (T < 0 || frame_off[b] < 0 || (long long)frame_off[b] + nframes[b] > fb_frames || row_off[b] < 0 || (long long)row_off[b] + T > out_rows)
      return kInvalid;
    if (T > max_T) max_T = T;
  }
  pfhip_impl::DevMem d_fo, d_nf, d_ro;
  hipError_t e = d_fo.upload(frame_off, sizeof(int) * B);
  if (e == hipSuccess) e = d_nf.upload(nframes, sizeof(int) * B);
  if (e == hipSuccess) e = d_ro.upload(row_off, sizeof(int) * B);
  if (e != hipSuccess) return (int)e;
  return launch_and_drain(S(stream), [&] {
    pfhip::launch_lfr_cmvn_packed(fb, d_fo.as<int>(), d_nf.as<int>(), d_ro.as<int>(), B, max_T, m, n, n_mels, mean, istd, out, ldo, S(stream));
  });
}
int pfhip_op_lfr_cmvn_online_batch(const float* fb, long long fb_frames, const int* fb_off, const int* Tin, const int* n_out,
                                   const int* row_off, int n_ops, int m, int n, int n_mels, const float* mean, const float* istd,
                                   float* out, int ldo, long long out_rows, void* stream) {
  if (!fb || !fb_off || !Tin || !n_out || !row_off || !mean || !istd || !out || n_ops < 1 || fb_frames < 0 || out_rows < 0 ||
      !lfr_shape_ok(m, n, n_mels, ldo))
    return kInvalid;
  std::vector<pfhip::VadLfrOp> ops((size_t)n_ops);
  int max_rows = 0;
  for (int k = 0; k < n_ops; ++k) {
    // an operation with rows reads frame min(i n + j, Tin - 1): it needs one frame at least
    if (n_out[k] < 0 || Tin[k] < 0 || (n_out[k] > 0 && Tin[k] < 1) || fb_off[k] < 0 || (long long)fb_off[k] + Tin[k] > fb_frames ||
        row_off[k] < 0 || (long long)row_off[k] + n_out[k] > out_rows)
      return kInvalid;
    ops[k] = pfhip::VadLfrOp{fb + (size_t)fb_off[k] * n_mels, Tin[k], n_out[k], row_off[k], 0};
    if (n_out[k] > max_rows) max_rows = n_out[k];
  }
  return with_device_segs(ops, S(stream), [&](const pfhip::VadLfrOp* d) {
    pfhip::launch_lfr_cmvn_online_batch(d, n_ops, max_rows, m, n, n_mels, mean, istd, out, ldo, S(stream));
  });
}
int pfhip_op_stream_lfr_batch(const float* fb, long long fb_frames, const int* fb_off, const int* T, const int* n_rows, const int* pos0,
                              const int* row_off, int n_ops, const float* mean, const float* istd, float scale, const float* inv_ts,
                              float* out, int ldo, long long out_rows, void* stream) {
  if (!fb || !fb_off || !T || !n_rows || !pos0 || !row_off || !mean || !istd || !inv_ts || !out || n_ops < 1 || fb_frames < 0 ||
      out_rows < 0 || ldo < 560)
    return kInvalid;
  std::vector<pfhip::StreamLfrOp> ops((size_t)n_ops);
  int max_rows = 0;
  for (int k = 0; k < n_ops; ++k) {
    if (n_rows[k] < 0 || T[k] < 0 || (n_rows[k] > 0 && T[k] < 1) || fb_off[k] < 0 || (long long)fb_off[k] + T[k] > fb_frames ||
        row_off[k] < 0 || (long long)row_off[k] + n_rows[k] > out_rows || pos0[k] < 0)
      return kInvalid;
    ops[k] = pfhip::StreamLfrOp{fb + (size_t)fb_off[k] * 80, out + (size_t)row_off[k] * ldo, T[k], n_rows[k], pos0[k], 0};
    if (n_rows[k] > max_rows) max_rows = n_rows[k];
  }
  return with_device_segs(ops, S(stream), [&](const pfhip::StreamLfrOp* d) {
    pfhip::launch_stream_lfr_batch(d, n_ops, max_rows, mean, istd, scale, inv_ts, ldo, S(stream));
  });
}
int pfhip_op_rows_copy_batch(float* dst, long long dst_floats, const long long* dst_off, const float* src, long long src_floats,
                             const long long* src_off, const int* ldd, const int* lds, const int* nrows, const int* ncols, int n_ops,
                             void* stream) {
  if (!dst || !dst_off || !src_off || !ldd || !lds || !nrows || !ncols || n_ops < 1 || dst_floats < 0 || src_floats < 0) return kInvalid;
  std::vector<pfhip::RowsCopyOp> ops((size_t)n_ops);
  int max_rows = 0;
  for (int k = 0; k < n_ops; ++k) {
    const bool has_src = src_off[k] >= 0;      // a negative source offset: no source, the rows are zeroed
    if (nrows[k] < 0 || ldd[k] < 0 || ncols[k] < 0 || ncols[k] > ldd[k] || dst_off[k] < 0 ||
        dst_off[k] + (long long)nrows[k] * ldd[k] > dst_floats)
      return kInvalid;
    if (has_src && nrows[k] > 0 &&
        (!src || lds[k] < 0 || (lds[k] != 0 && lds[k] < ncols[k]) || src_off[k] + (long long)(nrows[k] - 1) * lds[k] + ncols[k] > src_floats))
      return kInvalid;
    ops[k] = pfhip::RowsCopyOp{dst + dst_off[k], has_src ? src + src_off[k] : nullptr, ldd[k], lds[k], nrows[k], ncols[k]};
    if (nrows[k] > max_rows) max_rows = nrows[k];
  }
  return with_device_segs(ops, S(stream), [&](const pfhip::RowsCopyOp* d) { pfhip::launch_rows_copy_batch(d, n_ops, max_rows, S(stream)); });
}

int pfhip_op_embed(const float* feats, int D, float* x0, int ldx, const int* row_pos, int M, const float* inv_ts, float scale, void* stream) {
  // inv_ts holds D / 2 entries: column c reads entry c or c - D / 2
  if (!feats || !x0 || !row_pos || !inv_ts || M < 0 || D < 2 || D % 2 || ldx < D) return kInvalid;
  pfhip::launch_embed(feats, D, x0, ldx, row_pos, M, inv_ts, scale, S(stream));
  return done();
}
int pfhip_op_embed_gather(const int32_t* ids, const float* table, int vocab, int D, int Dout, float* out, int ldo, int N,
                          const float* inv_ts, float scale, const int* pos_of_row, void* stream) {
  if (!ids || !table || !out || !inv_ts || N < 0 || vocab < 1 || D < 2 || D % 2 || Dout < D || ldo < Dout) return kInvalid;
  pfhip::launch_embed_gather(ids, table, vocab, D, Dout, out, ldo, N, inv_ts, scale, pos_of_row, S(stream));
  return done();
}
int pfhip_op_argmax_first(const float* logits, int ldl, int N, int ncls, int32_t* out, void* stream) {
  if (!logits || !out || N < 0 || ncls < 1 || ldl < ncls) return kInvalid;
  pfhip::launch_argmax_first(logits, ldl, N, ncls, out, S(stream));
  return done();
}
int pfhip_op_compact(const float* stage, float* emb, const int* tok_row_src, int ML, int D, void* stream) {
  if (!stage || !emb || !tok_row_src || ML < 0 || D <= 0 || D % 4) return kInvalid;      // rows move as float4s
  pfhip::launch_compact(stage, emb, tok_row_src, ML, D, S(stream));
  return done();
}
int pfhip_op_gather_rows(const int32_t* ids, const float* table, int D, float* out, int R, void* stream) {
  if (!ids || !table || !out || R < 0 || D <= 0 || D % 4) return kInvalid;               // rows move as float4s
  pfhip::launch_gather_rows(ids, table, D, out, R, S(stream));
  return done();
}
int pfhip_op_svs_prompt_rows(const float* E, int D, const int* prompt, const int* row_off, const int* len, int B, float* feats, int ld,
                             void* stream) {
  if (!E || !prompt || !row_off || !len || !feats || B < 0 || D <= 0 || D % 4 || ld < D) return kInvalid;
  pfhip::launch_svs_prompt_rows(E, D, prompt, row_off, len, B, feats, ld, S(stream));
  return done();
}
int pfhip_op_gather_best(const float* logp, int ld, const int32_t* ids, int M, float* best, void* stream) {
  if (!logp || !ids || !best || M < 0 || ld < 1) return kInvalid;
  pfhip::launch_gather_best(logp, ld, ids, M, best, S(stream));
  return done();
}
int pfhip_op_row_lse(const float* logits, int ld, int M, int V, float* lse, void* stream) {
  if (!logits || !lse || M < 0 || V < 1 || ld < V) return kInvalid;
  pfhip::launch_row_lse(logits, ld, M, V, lse, S(stream));
  return done();
}

}  // extern "C"

// ---- the DNSMOS networks' kernels (conv3x3.hip, dnsmos.hip), one entry each ----------------------------------------------------------
namespace {
// window offsets from a HOST array: every window's samples must lie inside pcm
bool windows_inside(const int64_t* win_off, int n_win, long long need, long long pcm_samples) {
  for (int i = 0; i < n_win; ++i)
    if (win_off[i] < 0 || win_off[i] + need > pcm_samples) return false;
  return true;
}
template <typename Sample>
int logpow_op(const Sample* pcm, long long pcm_samples, const int64_t* win_off, int n_win, int n_frames, const float* stft_real,
              const float* stft_imag, float floor_v, float power, float denom, float* out, void* stream) {
  // the graph's Pow exponent is the initialiser 2.0: the kernel squares
  if (!pcm || !win_off || !stft_real || !stft_imag || !out || n_win < 0 || n_win > 65535 || n_frames < 1 || n_frames > 1 << 20 ||
      power != 2.0f || !(denom != 0.f) || !windows_inside(win_off, n_win, 160LL * (n_frames + 1), pcm_samples))
    return kInvalid;
  if (n_win == 0) return 0;
  std::vector<float> wr(161 * 320), wi(161 * 320), tab((size_t)320 * 2 * pfhip::kDnsmosBinStride);
  hipError_t e = hipMemcpy(wr.data(), stft_real, wr.size() * sizeof(float), hipMemcpyDeviceToHost);
  if (e == hipSuccess) e = hipMemcpy(wi.data(), stft_imag, wi.size() * sizeof(float), hipMemcpyDeviceToHost);
  if (e != hipSuccess) return (int)e;
  pfhip::dnsmos_stft_table(wr.data(), wi.data(), tab.data());
  pfhip_impl::DevMem d_tab, d_off;
  e = d_tab.upload(tab);
  if (e == hipSuccess) e = d_off.upload(win_off, sizeof(int64_t) * n_win);
  if (e != hipSuccess) return (int)e;
  bool ok = true;
  const int rc = launch_and_drain(S(stream), [&] {
    ok = pfhip::launch_dnsmos_logpow(pcm, d_off.as<int64_t>(), n_win, d_tab.f(), n_frames, floor_v, denom, out, S(stream));
  });
  return ok ? rc : kInvalid;
}
template <typename Sample>
int melspec_op(const Sample* pcm, long long pcm_samples, const int64_t* win_off, int n_win, float* out, void* stream) {
  if (!pcm || !win_off || !out || n_win < 0 || n_win > 65535 || !windows_inside(win_off, n_win, 144000, pcm_samples)) return kInvalid;
  if (n_win == 0) return 0;
  std::vector<float> tab((size_t)pfhip::kDnsmosFft * 2 * pfhip::kDnsmosBinStride), melT((size_t)161 * pfhip::kDnsmosMels);
  pfhip::dnsmos_mel_tables(tab.data(), melT.data());
  pfhip_impl::DevMem d_tab, d_mel, d_off, d_max;
  hipError_t e = d_tab.upload(tab);
  if (e == hipSuccess) e = d_mel.upload(melT);
  if (e == hipSuccess) e = d_off.upload(win_off, sizeof(int64_t) * n_win);
  if (e == hipSuccess) e = d_max.alloc(sizeof(unsigned) * n_win);
  if (e != hipSuccess) return (int)e;
  bool ok = true;
  const int rc = launch_and_drain(S(stream), [&] {
    ok = pfhip::launch_dnsmos_melspec(pcm, d_off.as<int64_t>(), n_win, d_tab.f(), d_mel.f(), out, d_max.as<unsigned>(), S(stream));
  });
  return ok ? rc : kInvalid;
}
}  // namespace

extern "C" {

int pfhip_op_conv3x3_relu(const float* x, const float* w, const float* bias, float* y, int N, int H, int W, int Cin, int Cout, int pool,
                          void* stream) {
  if (!x || !w || !bias || !y || N < 0 || H < 1 || W < 1) return kInvalid;
  if (Cin == 1) {
    if (!pfhip::launch_conv3x3_c1_relu(x, w, bias, y, N, H, W, Cout, pool != 0, S(stream))) return kInvalid;
    return done();
  }
  if (!(Cin == 32 || (Cin >= 64 && Cin % 64 == 0 && Cin <= 4096)) || (Cout != 32 && Cout != 64)) return kInvalid;
  // what a model does once at load: the weights' largest magnitude fixes the power-of-two scale of their plane images; a weight
  // that is not finite has no place in the fp16 two-plane domain and is refused
  std::vector<float> hw((size_t)Cout * Cin * 9);
  hipError_t e = hipMemcpy(hw.data(), w, hw.size() * sizeof(float), hipMemcpyDeviceToHost);
  if (e != hipSuccess) return (int)e;
  float mx = 0.f;
  for (float v : hw) {
    if (!std::isfinite(v)) return kInvalid;
    mx = std::max(mx, std::fabs(v));
  }
  const float scale = pfhip::best_w_scale(mx);
  if (!(mx * scale <= 32768.0f)) return kInvalid;
  pfhip_impl::DevMem hi, lo;
  e = hi.alloc(pfhip::conv3x3_plane_bytes(Cin, Cout));
  if (e == hipSuccess) e = lo.alloc(pfhip::conv3x3_plane_bytes(Cin, Cout));
  if (e != hipSuccess) return (int)e;
  bool ok = true;
  const int rc = launch_and_drain(S(stream), [&] {
    ok = pfhip::launch_conv3x3_pack(w, Cin, Cout, scale, hi.p, lo.p, S(stream)) &&
         pfhip::launch_conv3x3_relu(x, hi.p, lo.p, scale, bias, y, N, H, W, Cin, Cout, pool != 0, S(stream));
  });
  return ok ? rc : kInvalid;
}
int pfhip_op_dnsmos_logpow(const float* pcm, long long pcm_samples, const int64_t* win_off, int n_win, int n_frames, const float* stft_real,
                           const float* stft_imag, float floor_v, float power, float denom, float* out, void* stream) {
  return logpow_op(pcm, pcm_samples, win_off, n_win, n_frames, stft_real, stft_imag, floor_v, power, denom, out, stream);
}
int pfhip_op_dnsmos_logpow_s16(const int16_t* pcm, long long pcm_samples, const int64_t* win_off, int n_win, int n_frames,
                               const float* stft_real, const float* stft_imag, float floor_v, float power, float denom, float* out,
                               void* stream) {
  return logpow_op(pcm, pcm_samples, win_off, n_win, n_frames, stft_real, stft_imag, floor_v, power, denom, out, stream);
}
int pfhip_op_dnsmos_melspec(const float* pcm, long long pcm_samples, const int64_t* win_off, int n_win, float* out, void* stream) {
  return melspec_op(pcm, pcm_samples, win_off, n_win, out, stream);
}
int pfhip_op_dnsmos_melspec_s16(const int16_t* pcm, long long pcm_samples, const int64_t* win_off, int n_win, float* out, void* stream) {
  return melspec_op(pcm, pcm_samples, win_off, n_win, out, stream);
}
int pfhip_op_globalmax_mlp(const float* x, int N, int HW, int C, const float* w1, const float* b1, int D1, const float* w2, const float* b2,
                           int D2, const float* w3, const float* b3, int D3, float* out, void* stream) {
  if (!pfhip::launch_globalmax_mlp(x, N, HW, C, w1, b1, D1, w2, b2, D2, w3, b3, D3, out, S(stream))) return kInvalid;
  return done();
}

}  // extern "C"
