// The C ABI between the HIP translation units (csrc/{kernels,comm,blas}/*.hip, compiled by hipcc
// without torch) and the Python bindings (csrc/bindings/*.cpp, compiled by g++ against torch): the
// one declaration of every dpfs_* function that is defined in one translation unit and called
// from another.  Every .hip file and every binding file includes it, so a definition or a call
// that disagrees with a prototype here is a compile error and not a corrupted argument at run time.
// A new kernel's launcher gets its prototype here, under its defining file; what the parameters
// mean (units, layouts, "may be null") is documented at the definition.
#pragma once

#include <hip/hip_runtime_api.h>

#include <cstddef>
#include <cstdint>

extern "C" {

// kernels/adam.hip
void dpfs_adam_patch_grads(void* desc, const long long* ptrs, int n, hipStream_t s);
int dpfs_adam_chunk();
int dpfs_adam_desc_bytes();
void dpfs_adam_step(const void* desc, const int* chunks, int n_chunks, float lr, float b1, float b2, float eps,
                    float wd, float bc1, float bc2_sqrt, float gscale, const float* dscale, hipStream_t s);
void dpfs_grad_sumsq(const void* desc, const int* chunks, int n_chunks, float* partial, hipStream_t s);

// kernels/attention.hip
int dpfs_attn_supported_hd(int hd);
void dpfs_attn_diag(void* p);
void dpfs_attn_prefetch(int v);
void dpfs_attn_stagger(int v);
void dpfs_attn_fwd(const void* q, const void* k, const void* v, void* o, float* lse, int B, int T, int H, int hd,
                   long long ldq, long long ldk, long long ldv, long long ldo, float scale, int causal, int impl_req,
                   hipStream_t s);
int dpfs_attn_bwd(const void* dout, const void* q, const void* k, const void* v, const void* o, const float* lse,
                  float* delta, void* dq, void* dk, void* dv, int B, int T, int H, int hd, long long lddo,
                  long long ldq, long long ldk, long long ldv, long long ldo, long long lddq, long long lddk,
                  long long lddv, float scale, int causal, const int64_t* rope_pos, const float* rope_tab,
                  hipStream_t s, float* dbias, float* bws, int impl_req);
long long dpfs_attn_bias_ws(int B, int T, int H, int hd);

// kernels/attn_extend.hip
void dpfs_attn_extend(const void* q, long long ldq, const void* kc, const void* vc, const int* len, int len_rows,
                      const int* n, void* o, int B, int T, int H, int HD, int Tmax, float scale, hipStream_t s);
void dpfs_kv_append_chunk(const void* ksrc, const void* vsrc, long long ld, void* kc, void* vc, const int* len,
                          int len_rows, const int* n, int B, int T, int H, int HD, int Tmax, hipStream_t s);
// fp8 KV cache: e4m3 codes k8 / v8 (B, Tmax, H, HD) with fp32 row scales ks / vs (B, Tmax, H)
void dpfs_attn_extend_q8(const void* q, long long ldq, const void* k8, const void* v8, const float* ks,
                         const float* vs, const int* len, int len_rows, const int* n, void* o, int B, int T, int H,
                         int HD, int Tmax, float scale, hipStream_t s);
// paged KV cache (kernels/kv_page.h): pools kp / vp (P, PS, H, HD), tbl (B, MP) int32, PS = 1 << lg, len[B];
// ks / vs null: bf16 pools, else e4m3 pools with fp32 scale pools (P, PS, H)
void dpfs_attn_extend_paged(const void* q, long long ldq, const void* kp, const void* vp, const float* ks,
                            const float* vs, const int* tbl, int MP, int P, int lg, const int* len, const int* n,
                            void* o, int B, int T, int H, int HD, int Tmax, float scale, hipStream_t s);
void dpfs_kv_append_chunk_paged(const void* ksrc, const void* vsrc, long long ld, void* kp, void* vp, const int* tbl,
                                int MP, int P, int lg, const int* len, const int* n, int B, int T, int H, int HD,
                                int Tmax, hipStream_t s);

// kernels/attention_fused.hip
void dpfs_attn_bwd_dkdv4(int items, const void* q, const void* k, const void* v, const void* dout, const float* lsn,
                         const float* ndel, void* dk, void* dv, int T, int H, int BH, long long ldq, long long ldk,
                         long long ldv, long long lddo, long long lddk, long long lddv, float scale, int causal,
                         const int64_t* rope_pos, const float* rope_tab, float* pk, float* pv, int prefetch,
                         hipStream_t s);
long long dpfs_attn_fused_ws(int B, int T, int H, int hd);
long long dpfs_attn_fused_bias_ws(int B, int T, int H, int hd);
int dpfs_attn_bwd_fused(const void* dout, const void* q, const void* k, const void* v, const void* o,
                        const float* lse, float* delta, float* dqp, void* dq, void* dk, void* dv, int B, int T, int H,
                        int hd, long long lddo, long long ldq, long long ldk, long long ldv, long long ldo,
                        long long lddq, long long lddk, long long lddv, float scale, int causal,
                        const int64_t* rope_pos, const float* rope_tab, hipStream_t s, float* dbias, float* bws);

// kernels/decode.hip
int dpfs_decode_nsplit(int Tmax);
void dpfs_attn_decode(const void* q, long long ldq, const void* kc, const void* vc, const int* len_ptr, void* o,
                      long long ldo, float* part, int B, int H, int HD, int Tmax, float scale, hipStream_t s);
void dpfs_kv_append(const void* ksrc, const void* vsrc, long long ld, void* kc, void* vc, const int* len_ptr, int B,
                    int H, int HD, int Tmax, hipStream_t s);
void dpfs_step_advance(int* len_ptr, int64_t* pos, int B, hipStream_t s);
int dpfs_gemv16_ok(int M, int N, int K, long long lda, long long ldw);
void dpfs_gemv16(const void* A, long long lda, const void* W, long long ldw, const float* bias, void* Y,
                 long long ldy, int M, int N, int K, int swiglu, hipStream_t s);
void dpfs_rope_append(void* qkv, long long ld, const int64_t* pos, const float* tab, void* kc, void* vc,
                      const int* len_ptr, int B, int H, int HD, int Tmax, hipStream_t s);
// per-row lengths (ragged batches): len[B], sequence b uses len[b]; step_advance_rows clamps at t_max
void dpfs_attn_decode_rows(const void* q, long long ldq, const void* kc, const void* vc, const int* len, void* o,
                           long long ldo, float* part, int B, int H, int HD, int Tmax, float scale, hipStream_t s);
void dpfs_kv_append_rows(const void* ksrc, const void* vsrc, long long ld, void* kc, void* vc, const int* len, int B,
                         int H, int HD, int Tmax, hipStream_t s);
void dpfs_rope_append_rows(void* qkv, long long ld, const int64_t* pos, const float* tab, void* kc, void* vc,
                           const int* len, int B, int H, int HD, int Tmax, hipStream_t s);
void dpfs_step_advance_rows(int* len, int64_t* pos, int B, int t_max, hipStream_t s);
// fp8 KV cache: e4m3 codes k8 / v8 (B, Tmax, H, HD) with fp32 row scales ks / vs (B, Tmax, H)
void dpfs_attn_decode_q8(const void* q, long long ldq, const void* k8, const void* v8, const float* ks,
                         const float* vs, const int* len, int len_rows, void* o, long long ldo, float* part, int B,
                         int H, int HD, int Tmax, float scale, hipStream_t s);
// paged KV cache (kernels/kv_page.h): pools kp / vp (P, PS, H, HD), tbl (B, MP) int32, PS = 1 << lg, len[B];
// ks / vs null: bf16 pools, else e4m3 pools with fp32 scale pools (P, PS, H)
void dpfs_attn_decode_paged(const void* q, long long ldq, const void* kp, const void* vp, const float* ks,
                            const float* vs, const int* tbl, int MP, int P, int lg, const int* len, void* o,
                            long long ldo, float* part, int B, int H, int HD, int Tmax, float scale, hipStream_t s);
void dpfs_rope_append_paged(void* qkv, long long ld, const int64_t* pos, const float* tab, void* kp, void* vp,
                            const int* tbl, int MP, int P, int lg, const int* len, int B, int H, int HD, int Tmax,
                            hipStream_t s);

// kernels/elementwise.hip
void dpfs_swiglu_fwd(int dtype, const void* gu, void* h, int M, int F, int perm, hipStream_t s);
void dpfs_swiglu_bwd(int dtype, const void* dh, const void* gu, void* dgu, int M, int F, int perm, hipStream_t s);
long long dpfs_swiglu_bwd_dbias_ws(int M, int F);
void dpfs_swiglu_bwd_dbias(int dtype, const void* dh, const void* gu, void* dgu, float* dbias, float* ws, int M,
                           int F, int perm, hipStream_t s);
void dpfs_colsum_rows_small(const float* part, float* out, int rows, int N, hipStream_t s);
void dpfs_colsum_rows_split(const float* part, float* out, float* out2, int split, int rows, int N, hipStream_t s);
int dpfs_colsum_plan(int M, int cblocks, int target_blocks, int* rpc);
void dpfs_rope(int dtype, void* qkv, const int64_t* pos, const float* table, int M, int ld, int n_heads, int hd,
               int inverse, hipStream_t s);
void dpfs_bias_residual(int dtype, const void* y, const float* bias, const void* res, void* out, int M, int N,
                        hipStream_t s);
long long dpfs_colsum_ws(int M, int N);
void dpfs_bias_grad(int dtype, const void* dy, float* out, float* ws, int M, int N, hipStream_t s);
void dpfs_colsum_f32(const float* x, float* out, float* ws, int M, int N, hipStream_t s);
void dpfs_colsum_f32_split(const float* x, float* out, float* out2, int split, float* ws, int M, int N,
                           hipStream_t s);
void dpfs_occupy(int blocks, double us, hipStream_t s);

// kernels/embedding_ce.hip
long long dpfs_ce_bwd_dbias_ws(int dtype, int M, int V);
void dpfs_ce_bwd_dbias(int dtype, const void* logits, const int64_t* tgt, const float* lse, const float* gscale,
                       void* out, float* dbias, float* ws, int M, int V, long long vstart, int vvalid, hipStream_t s);
void dpfs_embedding_fwd(int out_dtype, const int64_t* ids, const float* w, void* out, int M, int D, long long vstart,
                        int vlocal, hipStream_t s);
void dpfs_embedding_bwd_seg(int in_dtype, const void* dout, const int64_t* perm, const int64_t* seg, float* dw, int D,
                            int vlocal, int accumulate, hipStream_t s);
void dpfs_embedding_bwd(int in_dtype, const void* dout, const int64_t* ids, float* dw, int M, int D, long long vstart,
                        int vlocal, hipStream_t s);
long long dpfs_ce_fused_ws(int M, int V);
int dpfs_ce_fused(int dtype, void* logits, const int64_t* tgt, const float* gscale, float* stats, float* dbias,
                  float* part, int M, int V, long long vstart, int vvalid, hipStream_t s);
void dpfs_ce_stats(int dtype, const void* logits, const int64_t* tgt, float* stats, int M, int V, long long vstart,
                   int vvalid, hipStream_t s);
void dpfs_ce_bwd(int dtype, const void* logits, const int64_t* tgt, const float* lse, const float* gscale, void* out,
                 int M, int V, long long vstart, int vvalid, hipStream_t s);
int dpfs_ce_part_floats();
void dpfs_ce_finalize(const float* stats, const int64_t* tgt, long long ignore, float* lse, float* valid, float* acc,
                      float* loss, float* part, int M, int nsh, int first, int last, hipStream_t s);
void dpfs_ce_valid_scale(const int64_t* tgt, long long ignore, float* gs, float* n_valid, float* part, int M,
                         hipStream_t s);
void dpfs_ce_grad_scale(const float* valid, const void* gloss, int gloss_bf16, const float* n_valid, float* gs, int M,
                        hipStream_t s);
long long dpfs_emb_sort_ws(int M);
void dpfs_emb_sort(const int64_t* ids, int M, long long vstart, int vlocal, int* ws, int64_t* perm, int64_t* seg,
                   hipStream_t s);

// kernels/fp32.hip
int dpfs_gemm_f32_splits(int M, int N, int K);
void dpfs_gemm_f32(int layout, const void* A, const void* B, void* C, const float* bias, int M, int N, int K,
                   long long lda, long long ldb, long long ldc, int accumulate, float* ws, int in_bf16, int out_bf16,
                   hipStream_t s);
int dpfs_attn_f32_supported_hd(int hd);
void dpfs_attn_fwd_f32(const float* q, const float* k, const float* v, float* o, float* lse, int B, int T, int H,
                       int hd, long long ldq, long long ldk, long long ldv, long long ldo, float scale, int causal,
                       hipStream_t s);
long long dpfs_attn_bwd_f32_ws(int B, int T, int H, int hd, int bias);
int dpfs_attn_bwd_f32(const float* dout, const float* q, const float* k, const float* v, const float* o,
                      const float* lse, float* ws, float* dq, float* dk, float* dv, int B, int T, int H, int hd,
                      long long lddo, long long ldq, long long ldk, long long ldv, long long ldo, long long lddq,
                      long long lddk, long long lddv, float scale, int causal, const int64_t* rpos, const float* rtab,
                      float* dbias, hipStream_t s);

// kernels/fp8.hip
int dpfs_fp8_work_floats();
void dpfs_fp8_quant(const void* x, long long n, int fmt, void* out, float* inv, float* work, hipStream_t s);

// kernels/gemm.hip
void dpfs_gemm_v2_sched(int v);
void dpfs_gemm_force(int cfg, int splits);
void dpfs_gemm_set_impl(int v);
void dpfs_gemm_set_workspace(float* ws, long long n);
long long dpfs_gemm_bf16_ws(int M, int N, int K);
int dpfs_gemm_rope_fusable(int M, int N, int K, int hd, int variant);
void dpfs_gemm_nt_rope(const void* A, const void* B, void* C, const float* bias, int M, int N, int K, int lda,
                       int ldb, int ldc, const int64_t* pos, const float* tab, int rope_cols, int rope_hd,
                       int variant, hipStream_t s);
void dpfs_gemm_nt(const void* A, const void* B, void* C, const float* bias, int M, int N, int K, int lda, int ldb,
                  int ldc, int variant, hipStream_t s);
void dpfs_gemm_nn(const void* A, const void* B, void* C, int M, int N, int K, int lda, int ldb, int ldc, int variant,
                  hipStream_t s);
int dpfs_gemm_tn_splits(int M, int N, int K);
long long dpfs_gemm_tn_ws(int M, int N, int K, int accumulate);
void dpfs_gemm_tn(const void* A, const void* B, float* C, float* ws, int M, int N, int K, int lda, int ldb,
                  int accumulate, int variant, hipStream_t s);
long long dpfs_gemm_tn2_ws(int M, int N, int K0, int K1);
int dpfs_gemm_tn2(const void* A0, const void* B0, const void* A1, const void* B1, float* C, float* ws, int M, int N,
                  int K0, int K1, int lda0, int ldb0, int lda1, int ldb1, int accumulate, int variant, hipStream_t s);

// kernels/gemm4.hip
void dpfs_gemm4_br_tn(int v);
void dpfs_gemm4_ablate(int v);
void dpfs_gemm4_diag(void* p);
void dpfs_gemm4_sched(int v);
void dpfs_gemm4_br(int v);
void dpfs_gemm4_group_m(int g);
void dpfs_gemm4_m32(int v);
void dpfs_gemm4_m32k(int v);
bool dpfs_gemm4_nt_swiglu(const void* A, const void* B, void* C, const float* bias, void* H, int M, int N, int K,
                          int lda, int ldb, int ldc, int ldh, unsigned a_bytes, unsigned b_bytes, hipStream_t s);
void dpfs_gemm4_swb_depth(int d);
bool dpfs_gemm4_nn_swiglu_bwd(const void* A, const void* B, const void* gu, void* dgu, float* part, int M, int F,
                              int K, int lda, int ldb, int ldgu, int lddgu, int perm, unsigned a_bytes,
                              unsigned b_bytes, hipStream_t s);
long long dpfs_gemm4_sk_ws(int M, int N, int K);
int dpfs_gemm4_sk_error(int reset);
void dpfs_gemm4_sk_starve(int on);
// One v4 GEMM.  Zero-initialised (`dpfs_gemm4_args a{}`) means: no RoPE, no second buffer, tile
// width chosen per shape, plain stores, no stream-K; a caller sets the fields it uses by name.
struct dpfs_gemm4_args {
  int layout;    // 0 = NT, 1 = NN, 2 = TN
  int out_f32;   // C: 0 = bf16, 1 = fp32 (split-K slabs)
  const void* A;
  const void* B;
  void* C;
  const float* bias;
  int M, N, K, lda, ldb, ldc;
  int kps, splits;         // rows of K per split (a multiple of 32), number of splits
  long long slab_stride;   // elements between the splits' slabs
  unsigned a_bytes, b_bytes;
  const int64_t* rope_pos;   // RoPE in the epilogue where rope_cols > 0 (bf16 NT)
  const float* rope_tab;
  int rope_cols, rope_hd;
  const void* A2;   // rows of K from k_switch on come from second buffers (null: one buffer)
  const void* B2;
  int k_switch, lda2, ldb2;
  unsigned a2_bytes, b2_bytes;
  int width;           // tile width of a non-split bf16 GEMM: 0 = per shape, 256 / 192 forced
  int stream_stores;   // the bf16 output written with non-temporal stores (plain NT / NN)
  int stream_k;        // the stream-K kernel where it applies (dpfs_gemm4_sk_ws)
  float* sk_ws;        // stream-K partials / flags: dpfs_gemm4_sk_ws floats
  long long sk_ws_floats;
};
bool dpfs_gemm4_launch(const dpfs_gemm4_args* args, hipStream_t s);
long long dpfs_gemm_tn_group_ws(int n, const int* M, const int* N, const int* lda, const int* ldb, int K,
                                const int* acc, const int* lda2, const int* ldb2, int K1);
int dpfs_gemm_tn_group(int n, const void* const* A, const void* const* B, float* const* C, const int* M, const int* N,
                       const int* lda, const int* ldb, const int* acc, int K, float* ws, long long ws_floats,
                       const void* const* A2, const void* const* B2, const int* lda2, const int* ldb2, int K1,
                       hipStream_t s);

// kernels/kv8.hip
void dpfs_kv_append_chunk_q8(const void* ksrc, const void* vsrc, long long ld, void* k8, void* v8, float* ks,
                             float* vs, const int* len, int len_rows, const int* n, int B, int T, int H, int HD,
                             int Tmax, hipStream_t s);
void dpfs_rope_append_q8(void* qkv, long long ld, const int64_t* pos, const float* tab, void* k8, void* v8, float* ks,
                         float* vs, const int* len, int len_rows, int B, int H, int HD, int Tmax, hipStream_t s);
// paged KV cache (kernels/kv_page.h): e4m3 pools kp / vp (P, PS, H, HD) with fp32 scale pools ks / vs (P, PS, H)
void dpfs_kv_append_chunk_q8_paged(const void* ksrc, const void* vsrc, long long ld, void* kp, void* vp, float* ks,
                                   float* vs, const int* tbl, int MP, int P, int lg, const int* len, const int* n,
                                   int B, int T, int H, int HD, int Tmax, hipStream_t s);
void dpfs_rope_append_q8_paged(void* qkv, long long ld, const int64_t* pos, const float* tab, void* kp, void* vp,
                               float* ks, float* vs, const int* tbl, int MP, int P, int lg, const int* len, int B,
                               int H, int HD, int Tmax, hipStream_t s);

// kernels/norm.hip
int dpfs_norm_bwd_grid(int M);
long long dpfs_norm_bwd_ws(int mode, int M, int D);
void dpfs_rmsnorm_fwd(int dtype, const void* x, const float* w, void* y, float* rstd, int M, int D, float eps,
                      hipStream_t s);
void dpfs_add_rmsnorm_fwd(int dtype, const void* yin, const float* bias, const void* res, const float* w, void* xo,
                          void* y, float* rstd, int M, int D, float eps, hipStream_t s);
void dpfs_layernorm_fwd(int dtype, const void* x, const float* w, const float* b, void* y, float* mean, float* rstd,
                        int M, int D, float eps, hipStream_t s);
void dpfs_norm_bwd(int mode, int dtype, const void* dy, const void* x, const float* w, const float* mean,
                   const float* rstd, const void* dres, void* dx, float* dw, float* db, float* partial_w,
                   float* partial_b, int M, int D, hipStream_t s);

// kernels/sample.hip
void dpfs_sample_logits(const void* logits, int dtype, long long ld, int B, int vocab, int vec_ok, float inv_t,
                        int top_k, double top_p, unsigned long long seed, const int64_t* pos, const float* u_in,
                        int64_t* ids, int* kept, float* thresh, float* u_out, hipStream_t s);
void dpfs_sample_logits_rows(const void* logits, int dtype, long long ld, int B, int vocab, int vec_ok,
                             const float* inv_t, const int* top_k, const double* top_p, const int64_t* seed,
                             const int* rid, const int64_t* pos, const float* u_in, int64_t* ids, int* kept,
                             float* thresh, float* u_out, hipStream_t s);
void dpfs_sample_logits_pen(const void* logits, int dtype, long long ld, int B, int vocab, int vec_ok,
                            const float* inv_t, const int* top_k, const double* top_p, const int64_t* seed,
                            const int* rid, const float* rep, const float* inv_rep, const float* pres,
                            const float* freq, int* hist, long long ld_h, int hist_vec_ok, int update,
                            const int64_t* pos, const float* u_in, int64_t* ids, int* kept, float* thresh,
                            float* u_out, float* logp, hipStream_t s);

// comm/rccl_comm.hip
const char* dpfs_rccl_last_error();
int dpfs_rccl_id_bytes();
int dpfs_rccl_unique_id(void* out);
int dpfs_rccl_init(const void* id_bytes, int nranks, int rank, void** comm_out);
int dpfs_rccl_destroy(void* comm);
int dpfs_rccl_async_error(void* comm);
int dpfs_rccl_all_reduce(void* comm, const void* send, void* recv, size_t count, int dtype, int op, hipStream_t s);
int dpfs_rccl_reduce_scatter(void* comm, const void* send, void* recv, size_t recvcount, int dtype, int op,
                             hipStream_t s);
int dpfs_rccl_all_gather(void* comm, const void* send, void* recv, size_t sendcount, int dtype, hipStream_t s);
int dpfs_rccl_broadcast(void* comm, const void* send, void* recv, size_t count, int dtype, int root, hipStream_t s);
int dpfs_rccl_group_start();
int dpfs_rccl_group_end();

// comm/xgmi.hip
const char* dpfs_xgmi_last_error();
long long dpfs_xgmi_handle_bytes();
void* dpfs_xgmi_create(int rank, int world, long long cap_bytes, int nslots, void* handles_out);
int dpfs_xgmi_open(void* h, const void* handles);
void dpfs_xgmi_set_blocks(void* h, int blocks);
long long dpfs_xgmi_capacity(void* h);
long long dpfs_xgmi_one_shot_capacity(void* h);
void* dpfs_xgmi_slot(void* h, int slot);
int dpfs_xgmi_error(void* h);
void dpfs_xgmi_clear_error(void* h);
int dpfs_xgmi_run(void* h, int op, int dtype, const void* x, void* out, long long n, long long part, double timeout_s,
                  int slot, hipStream_t stream);
void dpfs_xgmi_destroy(void* h);

// blas/blaslt.hip
const char* dpfs_lt_last_error();
int dpfs_lt_algos(int layout, long long M, long long N, long long K, int bias);
long long dpfs_lt_workspace(int layout, long long M, long long N, long long K, int bias, int i);
int dpfs_lt_run(int layout, long long M, long long N, long long K, const float* bias, int i, const void* op_a,
                const void* op_b, void* d, float beta, void* ws, long long ws_bytes, hipStream_t s);

}  // extern "C"
