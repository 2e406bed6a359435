// What the encoder's translation units (gemm.hip, vit_ops.hip, attention.hip, tower.hip) call across files: the GEMM
// epilogue codes and every launcher's prototype, declared once.  A signature or an enum value that differs between two
// files would link and misbehave at run time; included by the definer and the caller, it fails to compile instead.
#pragma once
#include "mmr_common.h"

namespace mmr {

// GEMM epilogues (gemm.hip)
enum { EPI_BIAS_BF16 = 0, EPI_BIAS_GELU_BF16 = 1, EPI_BIAS_RESID_F32 = 2, EPI_STORE_F32 = 3,
       EPI_BIAS_F32 = 4, EPI_BIAS_GELU_ERF_BF16 = 5, EPI_BIAS_TANH_BF16 = 6,
       // LayerNorm folded into the GEMM that consumes it (A = bf16 of the UN-normalised residual, W' = W*gamma):
       //   LN(h) . W^T + b  =  rstd * (h . W'^T - mean * colsum(W')) + (beta . W^T + b)
       EPI_LNFOLD_BF16 = 7, EPI_LNFOLD_GELU_BF16 = 8,
       // residual update that also emits what the NEXT folded GEMM needs: bf16(h_new) and per-row (sum, sumsq)
       EPI_RESID_STATS_F32 = 9, EPI_COUNT = 10 };

// gemm.hip
int launch_gemm(int epi, const bf16_t *A, const bf16_t *W, int M, int N, int K, const float *bias, void *out, hipStream_t st);
int launch_gemm_patch32(const bf16_t *pix, int B, int S, const bf16_t *W, int M, int N, float *out, hipStream_t st);
int launch_gemm_aux(int epi, const bf16_t *A, const bf16_t *W, int M, int N, int K, const float *bias, void *out, const GemmAux &aux, hipStream_t st);
void gemm_set_shared_chip_hint(bool on);
// vit_ops.hip
int launch_im2col(const void *px, mmr_dtype dt, bf16_t *ap, int B, int S, int P, int G, int K, int Kpad, hipStream_t st);
int launch_embed_vision(const float *pe, const float *cls, const float *pos, const float *lw, const float *lb, float *h, int B, int T, int d, float eps, bf16_t *xb, float2 *stats, int32_t *status, hipStream_t st);
int launch_embed_text(const int32_t *ids, const bf16_t *tok, const float *pos, float *h, int Nb, int T, int d, int vocab, bf16_t *xb, float2 *stats, int32_t *status, hipStream_t st);
int launch_layernorm(const float *h, const float *w, const float *b, bf16_t *x, int64_t rows, int d, float eps, hipStream_t st);
int launch_pool_ln(const float *h, const int32_t *ids, const float *w, const float *b, bf16_t *xc, int Nb, int T, int d, float eps, hipStream_t st);
int launch_finish(const float *feat, void *out, mmr_dtype odt, int Nb, int E, int normalize, hipStream_t st);
int launch_embed_bert(const int32_t *ids, const bf16_t *tok, const float *pos, const float *type0, const float *lw, const float *lb, float *h, bf16_t *x, int Nb, int T, int d, int vocab, float eps, const int32_t *types, int32_t *status, hipStream_t st);
int launch_layernorm_inplace(float *h, const float *w, const float *b, bf16_t *x, int64_t rows, int d, float eps, hipStream_t st);
int launch_gather_first_rows(const bf16_t *x, bf16_t *xc, int Nb, int T, int d, hipStream_t st);
int launch_pick_gather(const int32_t *ids, const bf16_t *x, const float *h, bf16_t *xg, float *hc, int32_t *picks, int Nb, int T, int d, hipStream_t st);
// attention.hip
int launch_attention(const bf16_t *qkv, bf16_t *o, int Bn, int T, int heads, int d, int causal, const int32_t *kmask, hipStream_t st);
int launch_attention_pooled(const bf16_t *q, int ldq, const bf16_t *k, const bf16_t *v, int ldkv, const int32_t *picks, bf16_t *o, int Bn, int T, int heads, int d, int causal, hipStream_t st);

}  // namespace mmr
