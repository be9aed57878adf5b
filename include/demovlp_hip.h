/* demovlp_hip.h -- C ABI of libdemovlp_hip.so: the MI355X (gfx950) kernels behind DemoVLP's cross-modal
 * forward/backward hot path.
 *
 * Conventions
 *   - Every pointer is a DEVICE pointer borrowed from the caller (PyTorch-ROCm allocates; nothing here allocates,
 *     frees or synchronises except dvlp_prof_collect).  Workspaces are passed in; their sizes come from the
 *     *_bytes / *_blocks / *_chunks helpers below.
 *   - `stream` is a hipStream_t; every call is asynchronous on it and re-entrant per stream.
 *   - `dtype` selects the COMPUTE/STORAGE dtype of activations: DVLP_F32 (exact-fp32 MFMA, the 1e-4 parity path)
 *     or DVLP_BF16 (bf16 MFMA, fp32 accumulate, the throughput path).  Biases, LayerNorm parameters, statistics,
 *     masks, losses and optimizer state are always fp32.
 *   - Return value: 0 on success, negative DVLP_ERR_* otherwise (the Python binding raises).
 *
 * The reference (showlab/DemoVLP) has no native code: each entry point below replaces the PyTorch op sequence
 * cited next to it (paths relative to the reference repo root).
 */
#ifndef DEMOVLP_HIP_H
#define DEMOVLP_HIP_H
#include <stdint.h>
#ifdef __cplusplus
extern "C" {
#endif

enum { DVLP_F32 = 0, DVLP_BF16 = 1 };
enum { DVLP_OK = 0, DVLP_ERR_DTYPE = -1, DVLP_ERR_SHAPE = -2, DVLP_ERR_LAUNCH = -3, DVLP_ERR_UNSUPPORTED = -4 };
/* ---- Every entry point here is stateless apart from caller-registered scratch (dvlp_set_workspace*, dvlp_reduce_*); optional per-call
 *      extras travel in the `dvlp_*_ext` structs of the `*_ex` calls, never through "next call" setters.  The developer switches
 *      (`dvlp_dev_*`: A/B measurements, timing ablations, forced code paths) are NOT in this library: they exist only in the -DDVLP_DEV
 *      build (libdemovlp_hip_dev.so, declared in demovlp_hip_dev.h); here each of them is a compile-time constant at its default. ---- */
/* dvlp_gemm epilogue flags */
enum { DVLP_EPI_GELU = 1, DVLP_EPI_GELU_BWD = 2, DVLP_EPI_RELU_BWD = 4, DVLP_EPI_ACCUM = 8, DVLP_EPI_LEAKY = 16,
       DVLP_EPI_OUT_F32 = 32 /* C is fp32 whatever the compute dtype (weight gradients) */ };

/* ---- K1 region select: data_loader/WebVid_dataset.py:134-283 (read_all_object_from_disk + object_select_random) ---- */
int dvlp_region_select(int64_t BF, int64_t F, int64_t Nraw, int64_t R, const float* feats, const float* bbox, const float* conf,
                       const float* wh, const int* nvalid, float* obj, float* mask, int* order, int* lens, void* stream);

/* ---- GEMM: nn.Linear forward/backward everywhere on the path (model/object_transformer.py:116-122, 155, 194,
 *      404-408, 451; DistilBERT q/k/v/out/ffn; model/model.py:40-43) and the contractions of model/loss.py:235,267.
 *      C[M,N] = epi(alpha * op(A) op(B)^T); transX=0: X[r*ld+k], transX=1: X[k*ld+r].                              ---- */
int dvlp_gemm(int dtype, int transA, int transB, int64_t M, int64_t N, int64_t K, const void* A, int64_t lda, const void* B,
              int64_t ldb, void* C, int64_t ldc, const float* bias, const void* res, int64_t ldres, void* aux, int64_t ldaux,
              int flags, float alpha, void* stream);
int dvlp_gemm_batched(int dtype, int transA, int transB, int64_t M, int64_t N, int64_t K, const void* A, int64_t lda,
                      const void* B, int64_t ldb, void* C, int64_t ldc, const float* bias, const void* res, int64_t ldres,
                      void* aux, int64_t ldaux, int flags, float alpha, int64_t batch, int64_t strideA, int64_t strideB,
                      int64_t strideC, int64_t strideRes, int64_t strideAux, void* stream);
/* The weight gradients of `count` linears at once: dW_p[M_p, N_p] (fp32, contiguous) (+)= dY_p[K_p, M_p]^T X_p[K_p, N_p], i.e.
   count calls of dvlp_gemm(transA=1, transB=1, fp32 out) -- the K = batch*tokens reductions of one transformer layer
   (reference: autograd of the nn.Linear modules in object_transformer.py:100-196 and DistilBERT's TransformerBlock).  Arguments are
   host arrays of length `count`.  bf16 problems that suit the 256 x 256 kernel run as one grouped launch. */
int dvlp_wgrad_grouped(int dtype, int count, const int64_t* M, const int64_t* N, const int64_t* K, const void* const* dY,
                       const int64_t* ld_dy, const void* const* X, const int64_t* ld_x, void* const* dW, int accumulate, void* stream);
/* The same with an optimizer update riding along (round 6): `ext` describes one dvlp_adamw_range_dev call -- the fused HF-AdamW pass over a
   contiguous range of the flat parameter / gradient / moment buffers, typically the PREVIOUS layer's weights, whose gradients are final -- that
   is executed by the workgroups this launch would leave idle (a ViT layer's group is 216 workgroups on 256 CUs) instead of as a launch of its
   own between two GEMM launches; when the group has fewer than 16 spare workgroups (or does not take the grouped path) the update is launched
   right behind it.  ext->fused (out) says which.  NULL ext = dvlp_wgrad_grouped. */
typedef struct dvlp_wgrad_ext {
    int64_t n;
    float* p; const float* g; float* m; float* v; const float* hyper; void* bf16_shadow;
    int fused;
} dvlp_wgrad_ext;
int dvlp_wgrad_grouped_ex(int dtype, int count, const int64_t* M, const int64_t* N, const int64_t* K, const void* const* dY,
                          const int64_t* ld_dy, const void* const* X, const int64_t* ld_x, void* const* dW, int accumulate,
                          dvlp_wgrad_ext* ext, void* stream);
/* Per-stream hint, caller-registered like the workspaces: co_running != 0 says that launches on `stream` share the chip with kernels of another
   stream (the text tower beside the object tower, model.ObjectRelation.parallel_towers); the bf16 GEMM dispatch then favours CU-time per FLOP
   (tall tiles) over the latency of its own grid.  0 removes the hint. */
int dvlp_stream_hint(void* stream, int co_running);
/* dvlp_gemm with optional extras, handed to the call that consumes them (NULL = none).  `colsum`: fp32 dst[N] = column sums of the stored
   output C -- e.g. the bias gradient of the Linear whose output gradient this product is (batch 1, not for fp32 outputs).  Fused into the
   256-row kernel's epilogue through the deferred-reduction queue where possible (final after dvlp_reduce_flush; colsum_fused = 1),
   otherwise a plain column-sum pass runs behind the product (colsum_fused = 0; final when the call's work is). */
typedef struct dvlp_gemm_ext {
    float* colsum;
    int colsum_fused;      /* out */
} dvlp_gemm_ext;
int dvlp_gemm_ex(int dtype, int transA, int transB, int64_t M, int64_t N, int64_t K, const void* A, int64_t lda, const void* B,
                 int64_t ldb, void* C, int64_t ldc, const float* bias, const void* res, int64_t ldres, void* aux, int64_t ldaux,
                 int flags, float alpha, dvlp_gemm_ext* ext, void* stream);
/* scratch for split-K partial sums (weight-gradient GEMMs); caller-owned device memory, NULL disables splitting */
int dvlp_set_workspace(void* ptr, int64_t bytes);
/* same, for one stream only (GEMMs running concurrently on two streams need separate slabs) */
int dvlp_set_workspace_stream(void* stream, void* ptr, int64_t bytes);
/* per-launch HIP-event timing of the GEMM kernels (bench.py roofline figure) */
int dvlp_prof_enable(int on);
int dvlp_prof_collect(double* total_ms, double* total_flops, int64_t* count);

/* ---- LayerNorm: norm1/norm2 (object_transformer.py:261,271, eps 1e-6) and DistilBERT's post-LNs (eps 1e-12) ---- */
int dvlp_layernorm_fwd(int dtype, int64_t M, int64_t D, const void* x, const float* gamma, const float* beta, float eps, void* y,
                       void* y_relu, float* mean, float* rstd, void* stream);
int64_t dvlp_layernorm_bwd_blocks(int64_t M);
/* dx_colsum (optional): fp32 [D] <- column sums of dx, i.e. the bias gradient of the Linear that dx feeds (nn.Linear backward
   after the LayerNorm's); produced by the same kernel on the deferred path, by a dvlp_colsum pass otherwise */
int dvlp_layernorm_bwd(int dtype, int64_t M, int64_t D, const void* dy, const void* x, const float* gamma, const float* mean,
                       const float* rstd, const void* dres, void* dx, float* dgamma, float* dbeta, float* workspace, int accumulate,
                       float* dx_colsum, void* stream);
/* Deferred second stages.  dvlp_layernorm_bwd / dvlp_colsum called with (accumulate | 2) -- "nobody reads the result before
   the flush" -- park their partial sums in `workspace` and queue the final column reduction; dvlp_reduce_flush runs every
   queued reduction as ONE launch (a training step otherwise pays ~125 ten-microsecond launches for them).  The table is
   device memory for the queue (48 bytes per queued reduction).  NULL workspace disables deferral (the default): such calls
   then reduce immediately.  The trainer flushes before the optimizer step / before reducing the tail gradient bucket. */
int dvlp_reduce_defer(void* workspace, int64_t workspace_bytes, void* table, int64_t table_bytes);
int dvlp_reduce_flush(void* stream);
/* bias / table gradients: out[g][n] (+)= sum_m x_g[m][n] */
int64_t dvlp_colsum_chunks(int64_t M);
/* optional: `count` zeroed uint32 counters enabling the single-launch (last-workgroup-reduces) form of dvlp_colsum */
int dvlp_colsum_counters(void* ptr, int64_t count);
int dvlp_colsum(int dtype, int64_t M, int64_t N, const void* x, int64_t ld, int64_t inner, int64_t ostride, int64_t groups,
                int64_t gstride, float* out, float* workspace, int accumulate, void* stream);

/* ---- attention: VarAttention.forward + attn_mask (object_transformer.py:152-196, 91-97) [mode 0] and DistilBERT
 *      multi-head self-attention [mode 1]                                                                          ---- */
/* `workspace` (B*H*F*66 floats) and `cls_stats` (B*H*4 floats), both optional (mode 0, bf16): the CLS query -- the one query that
   attends to every key of the clip (object_transformer.py:162-167) -- is folded into the per-frame waves, merged flash-style by a
   64-thread launch, and its softmax statistics stay in `cls_stats` for dvlp_attention_bwd (`fwd_out` = this call's `out`), which
   then needs no statistics pass.  Backward workspace (mode 0): B*H*(F*192 + 4) floats.
   The two PLAIN calls below never fold: dvlp_attention_fwd leaves `cls_stats` untouched and dvlp_attention_bwd ignores `fwd_out` /
   `cls_stats` (it recomputes the statistics) -- pairing them is always safe; the fold is a contract of the `_ex` pair (ext->folded). */
int dvlp_attention_fwd(int dtype, int mode, int64_t B, int64_t N, int64_t H, int64_t F, int64_t R, const void* q, const void* k,
                       const void* v, int64_t ld, const float* addmask, void* out, int64_t ldo, float scale, float* workspace,
                       float* cls_stats, void* stream);
int dvlp_attention_bwd(int dtype, int mode, int64_t B, int64_t N, int64_t H, int64_t F, int64_t R, const void* q, const void* k,
                       const void* v, int64_t ld, const float* addmask, const void* dout, int64_t ldo, void* dq, void* dk, void* dv,
                       int64_t ldd, float* workspace, float scale, const void* fwd_out, int64_t ld_fwd_out, const float* cls_stats,
                       void* stream);
/* The same two calls with optional extras, handed to the call that consumes them (ext may be NULL):
     keep / keepT / keep_scale  (mode 1) dropout of the attention probabilities: keep bytes in both orientations from dvlp_dropout_attn_mask and
                                1 / (1 - p) -- HF MultiHeadSelfAttention's `weights = dropout(softmax(scores))`
     colsum                     (backward, mode 0) fp32 [3*H*64]: column sums of dq | dk | dv = the gradient of the packed qkv bias
                                (object_transformer.py:310 qkv_bias=True), queued through the deferred-reduction queue when the call can
                                (bf16 one-pass form with the forward's statistics): colsum_fused = 1; else the caller sums the columns itself
     folded                     (forward, out) 1 if the CLS query was folded and `cls_stats` filled -- only then hand them to the backward.
   The CLS fold needs `ext` (the caller must be able to learn whether `cls_stats` were written): the plain dvlp_attention_fwd never folds. */
typedef struct dvlp_attn_ext {
    const void* keep; const void* keepT; float keep_scale;
    float* colsum;
    int colsum_fused;      /* out */
    int folded;            /* out */
} dvlp_attn_ext;
int dvlp_attention_fwd_ex(int dtype, int mode, int64_t B, int64_t N, int64_t H, int64_t F, int64_t R, const void* q, const void* k,
                          const void* v, int64_t ld, const float* addmask, void* out, int64_t ldo, float scale, float* workspace,
                          float* cls_stats, dvlp_attn_ext* ext, void* stream);
int dvlp_attention_bwd_ex(int dtype, int mode, int64_t B, int64_t N, int64_t H, int64_t F, int64_t R, const void* q, const void* k,
                          const void* v, int64_t ld, const float* addmask, const void* dout, int64_t ldo, void* dq, void* dk, void* dv,
                          int64_t ldd, float* workspace, float scale, const void* fwd_out, int64_t ld_fwd_out, const float* cls_stats,
                          dvlp_attn_ext* ext, void* stream);

/* ---- tower prologues: ObjectTransformer.forward_features (object_transformer.py:400-433); DistilBERT embeddings ---- */
int dvlp_obj_split(int dtype, int64_t M, const float* obj, void* feat, float* box, void* stream);
int dvlp_embed_assemble(int dtype, int64_t B, int64_t F, int64_t R, const void* tok, const float* box, const float* Wp,
                        const float* bp, const float* temporal, const float* cls, const float* pos0, const float* mask01, void* x,
                        float* addmask, void* stream);
/* time attention of SpaceTimeBlock (object_transformer.py:252-258, 'b (f n) d -> (b n) f d'): dst[b][1 + n F + f] = src[b][1 + f R + n]
   (+ res at the destination index when non-NULL), CLS row in place; dvlp_attention_* mode 0 on the transposed order with (F, R)
   swapped IS the time attention; the same call with F and R swapped transposes back.  F = 1 is the identity (a plain add). */
int dvlp_token_transpose(int dtype, int64_t B, int64_t F, int64_t R, int64_t D, const void* src, const void* res, void* dst, void* stream);
int dvlp_embed_unassemble(int dtype, int64_t B, int64_t F, int64_t R, const void* dx, void* dtok, void* stream);

/* ---- the heads' view of a tower output (model/model.py:70-96: `[:, 0]` / `[:, 1:]` + .contiguous()): x [B][N][row_bytes] -> g [B][row_bytes]
 *      (row 0 of each sample) and l [B][N-1][row_bytes] in one launch, and its backward (dx from dg / dl, NULL = zeros) in one launch.
 *      Raw bytes, any dtype; row_bytes a multiple of 16, pointers 16-byte aligned.                                                    ---- */
int dvlp_split_cls(int64_t B, int64_t N, int64_t row_bytes, const void* x, void* g, void* l, void* stream);
int dvlp_merge_cls(int64_t B, int64_t N, int64_t row_bytes, const void* dg, const void* dl, void* dx, void* stream);
int64_t dvlp_box_wgrad_chunks(int64_t M);
int dvlp_box_wgrad(int dtype, int64_t M, const void* dtok, const float* box, float* dWp, float* workspace, int accumulate,
                   void* stream);
int dvlp_text_embed_fwd(int dtype, int64_t B, int64_t L, const int64_t* ids, const float* word, const float* pos,
                        const float* gamma, const float* beta, float eps, void* e_out, void* y, float* mean, float* rstd,
                        void* stream);
int dvlp_text_embed_bwd(int dtype, int64_t M, const int64_t* ids, const void* de, float* dword, void* stream);
int dvlp_cast(int src_dtype, int dst_dtype, int64_t n, const void* src, void* dst, void* stream);
/* the loss' caption-side inputs from the attention mask in one launch (trainer/trainer_dist.py:152-159): text_length[b] = sum_w att[b][w] (int64)
   and text_mask[b][w - 1] = (att[b][w] - 1) * 100, w = 1 .. L - 1 (fp32 [B, L - 1]); att int64 [B, L] */
int dvlp_text_mask_len(int64_t B, int64_t L, const int64_t* att, int64_t* text_length, float* text_mask, void* stream);
/* DistilBERT's additive key mask (HF: scores.masked_fill(attention_mask == 0, -inf); call site model/model.py:87): key_mask[B][L] fp32 = 0 where
   att != 0, -inf elsewhere -- one launch instead of a fill, a comparison and a masked fill */
int dvlp_text_key_mask(int64_t B, int64_t L, const int64_t* att, float* key_mask, void* stream);

/* ---- dropout of the text tower: the reference keeps DistilBERT in train mode (model/model.py:29-30), so HuggingFace's three
 *      dropouts (embeddings, attention probabilities, feed-forward output; p = 0.1) are part of every training step.  Masks are
 *      Philox4x32-10 streams keyed by (seed, step offset, site, element); `state` is DEVICE memory uint32[4] =
 *      {seed_lo, seed_hi, offset, -}; dvlp_dropout_advance bumps the offset (once per forward; replayable inside a hipGraph). ---- */
int dvlp_dropout_advance(void* state, void* stream);
/* y = x * keep / (1 - p) (+ res); keep (uint8 [n], 0/1) is stored for the backward.  n % 4 == 0. */
int dvlp_dropout_fwd(int dtype, int64_t n, const void* x, const void* res, void* y, void* keep, float p, const void* state, int site, void* stream);
int dvlp_dropout_bwd(int dtype, int64_t n, const void* dy, const void* keep, float p, void* dx, void* stream);
/* keep bytes of the attention probabilities of BH = batch * heads [N x N] maps in both orientations: keep[bh][q][key] and
   keepT[bh][key][q], row stride N rounded up to 16 (pads 0) */
int dvlp_dropout_attn_mask(int64_t BH, int64_t N, float p, const void* state, int site, void* keep, void* keepT, void* stream);
/* (the masks reach the attention kernels through dvlp_attn_ext of dvlp_attention_fwd_ex / dvlp_attention_bwd_ex) */
/* out[4] = Philox4x32-10(ctr_key[0..3], key = ctr_key[4..5]) computed on the device (known-answer test) */
int dvlp_philox_kat(const void* ctr_key, void* out, void* stream);

/* ---- local loss: xattn_score_fast / func_attention_fast / focal_equal / cosine_similarity (model/loss.py:209-330) ---- */
/* `gate`: bit 0 = focal_equal gate on (model/loss.py:274-283); bit 1 (DVLP_XATTN_ONE_STREAM) = issue everything on the caller's stream --
   by default the text->image half of the multi-kernel path (its contractions and cosine passes) runs on an internal side stream beside
   the image->text half between the softmax stages (fork / join by events, capturable into a hipGraph; its split-K slabs are a region of
   `workspace` of their own).  A per-call option, not process state: bench.py's per-launch timing pass sets it so that an event pair
   brackets one launch. */
enum { DVLP_XATTN_GATE = 1, DVLP_XATTN_ONE_STREAM = 2 };
int64_t dvlp_xattn_workspace_bytes(int dtype, int64_t Bi, int64_t Bj, int64_t G, int64_t W, int bwd);
int dvlp_xattn_fwd(int dtype, int64_t Bi, int64_t Bj, int64_t G, int64_t W, int64_t d, const void* Craw, const void* Qraw,
                   const float* mimg, const float* mcap, float lam, int gate, float* scores, void* workspace, int bwd, void* stream);
int dvlp_xattn_bwd(int dtype, int64_t Bi, int64_t Bj, int64_t G, int64_t W, int64_t d, const void* Craw, const void* Qraw,
                   const float* mimg, const float* mcap, float lam, int gate, const float* dscores, void* workspace, void* dC,
                   void* dQ, void* stream);
/* Pair list (forward only): scores[i][k] = the local similarity above of video i (Craw [Bi][G][d], mimg [Bi][G]) and caption cand[i K + k] of
   the pool Qraw [Bj][W][d] / mcap [Bj][W]; cand is an int32 [Bi][K] device array, NULL meaning caption i K + k (the multiple-choice layout,
   trainer/trainer_dist.py:820-829, without its K x K grid).  A cand entry outside [0, Bj) reads nothing and scores NaN.  bf16 within the
   fused kernel's range (G <= 288, W <= 112): one prep of the Bi videos and Bj captions, then one workgroup per pair -- the per-pair code of
   the full-grid fused kernel, so scores[i][k] equals its entry [i][cand[i K + k]] bit for bit.  Otherwise the multi-kernel path scores each
   video against its K gathered captions.  Workspace sizes return a negative DVLP_ERR_* for a bad dtype / shape. */
int64_t dvlp_xattn_pairs_workspace_bytes(int dtype, int64_t Bi, int64_t Bj, int64_t K, int64_t G, int64_t W);
int dvlp_xattn_pairs_fwd(int dtype, int64_t Bi, int64_t Bj, int64_t K, int64_t G, int64_t W, int64_t d, const void* Craw, const void* Qraw,
                         const float* mimg, const float* mcap, const int* cand, float lam, int gate, float* scores, void* workspace,
                         void* stream);

/* Resident video index + query-major pair list (text-to-video search, demovlp_amd/search.py): the local similarity above
   (model/loss.py:209-330) of caption j against the videos cand[j K + k] of a collection whose video side was prepared ONCE.
   The index is caller-owned device memory of dvlp_xattn_index_bytes(capacity, G) bytes holding, per video, what the fused kernel's prep
   writes per call (normalised regions in both orientations, bf16, and the region norms, fp32: ~296 KB at G = 288).  bf16 only and only inside
   the fused kernel's range (G <= 288, W <= 112): anything else returns DVLP_ERR_UNSUPPORTED (size helpers: as a negative value).
     dvlp_xattn_index_add        preps videos Craw (bf16 [n][G][256]) into rows row0 .. row0 + n; a row's bytes do not depend on the call
                                 that wrote it (several adds == one add).  No reference counterpart.
     dvlp_xattn_index_pairs_fwd  preps the Bj captions Qraw (bf16 [Bj][W][256]) into `workspace` (dvlp_xattn_index_query_workspace_bytes(Bj, W):
                                 independent of the capacity), then one workgroup per (k, j) runs the per-pair code of the full-grid fused
                                 kernel: scores[j][k] (fp32 [Bj][K]) equals entry [cand[j K + k]][j] of dvlp_xattn_fwd's grid bit for bit.  cand is
                                 int32 [Bj][K] on the device; an entry outside [0, capacity) reads nothing and scores NaN (the -1 of a short
                                 dvlp_topk_rows list).  mimg is the additive region mask of the whole index, fp32 [capacity][G].  Bj <= 65535. */
int64_t dvlp_xattn_index_bytes(int64_t capacity, int64_t G);
int dvlp_xattn_index_add(int64_t capacity, int64_t G, int64_t row0, int64_t n, const void* Craw, void* index, void* stream);
int64_t dvlp_xattn_index_query_workspace_bytes(int64_t Bj, int64_t W);
int dvlp_xattn_index_pairs_fwd(int64_t capacity, int64_t G, const void* index, const float* mimg, int64_t Bj, int64_t W, int64_t d,
                               const void* Qraw, const float* mcap, int64_t K, const int* cand, float lam, int gate, float* scores,
                               void* workspace, void* stream);

/* Grounding of the same pairs (no reference counterpart beyond an HTML visualiser every shipped config switches off): the local similarity
   above (model/loss.py:209-330) of caption j and video cand[j K + k], and where it came from.  One launch on the (K, Bj) grid of
   dvlp_xattn_index_pairs_fwd running the same per-pair code; in the notation of that score (A = S / |S_row|, A2 = S / |S_col|, P / P2 the
   two focal softmaxes), per pair o = j K + k:
     score              fp32 [Bj][K]     equal to dvlp_xattn_index_pairs_fwd's scores[j][k] bit for bit
     word_scores        fp32 [Bj][K][W]  cos(Q_w, (P C^)_w) for every word, padded ones included; mean over w = the image->text half of score
     region_scores      fp32 [Bj][K][G]  cos(C_g, (P2 Q^)_g) for every region, masked ones included; mean over g = the other half
     word_region        int32 [Bj][K][W] argmax over g of lam (A[g][w] + mimg[g]) (ties: smaller g): the region word w attends to most
     word_region_weight fp32 [Bj][K][W]  P[w][word_region[w]] after the focal gate and renormalisation (the bf16 value the kernel multiplies with)
     region_word        int32 [Bj][K][G] argmax over w of lam (A2[g][w] + mcap[w]) (ties: smaller w)
     frame_scores       fp32 [Bj][K][frames]  mean of region_scores over the frame's regions (G / frames consecutive ones) with mimg == 0;
                                         -inf for a frame without one.  frames = 0 and frame_scores = NULL: not computed.
   The argmaxes are taken from the fp32 logits and do not depend on scheduling.  A cand entry outside [0, capacity) reads nothing: NaN in the
   float rows, -1 in the int rows.  Argument errors -- d != 256, frames not dividing G (or frames != 0 without frame_scores and the reverse),
   K < 1, a null required pointer, a shape outside the fused range (G <= 288, W <= 112) -- return DVLP_ERR_SHAPE and launch nothing.  bf16
   only.  workspace: dvlp_xattn_index_ground_workspace_bytes(Bj, W, K, G) bytes (host arithmetic; a negative DVLP_ERR_* outside that range). */
int64_t dvlp_xattn_index_ground_workspace_bytes(int64_t Bj, int64_t W, int64_t K, int64_t G);
int dvlp_xattn_index_pairs_ground(int64_t capacity, int64_t G, const void* index, const float* mimg, int64_t Bj, int64_t W, int64_t d,
                                  const void* Qraw, const float* mcap, const int* cand, int64_t K, int64_t frames, float lam, int gate,
                                  float* score, float* word_scores, float* region_scores, int* word_region, float* word_region_weight,
                                  int* region_word, float* frame_scores, void* workspace, void* stream);

/* Long videos (no reference counterpart): the resident video index, pair list and grounding above for 1 <= G <= 1152 regions (32 frames x 36)
   and W <= 112 words, bf16, on a region-tiled pair kernel (csrc/xfused.hip): one workgroup per pair walks the regions twice in
   tiles of 128 with O(tile) LDS, instead of keeping both attention matrices resident.  The index layout, the query workspace, the argument
   lists, the outputs and the error rules are those of dvlp_xattn_index_* (a row of the index at G <= 288 has the same bytes in both
   families; ~1.18 MB per video at G = 1152); only the range differs -- the size helpers return a negative DVLP_ERR_* outside it, the calls
   DVLP_ERR_UNSUPPORTED (pairs_ground: DVLP_ERR_SHAPE, as its sibling).  A cand entry outside [0, capacity) reads nothing: NaN scores, -1
   indices.  Scores agree with dvlp_xattn_index_pairs_fwd to rounding (2e-3), not bit for bit: the softmax numerators are summed per tile
   and the image->text context is scaled after its product.  dvlp_xattn_long_index_pairs_ground's score equals
   dvlp_xattn_long_index_pairs_fwd's bit for bit, and
     word_region_weight = gated softmax numerator at word_region[w] (the bf16 value the kernel multiplies with) / gated sum over all regions,
                          in fp32 -- this kernel multiplies by UNNORMALISED numerators, so there is no bf16 quotient to report.
   No float atomics; results do not depend on scheduling. */
int64_t dvlp_xattn_long_index_bytes(int64_t capacity, int64_t G);
int dvlp_xattn_long_index_add(int64_t capacity, int64_t G, int64_t row0, int64_t n, const void* Craw, void* index, void* stream);
int64_t dvlp_xattn_long_index_query_workspace_bytes(int64_t Bj, int64_t W);
int dvlp_xattn_long_index_pairs_fwd(int64_t capacity, int64_t G, const void* index, const float* mimg, int64_t Bj, int64_t W, int64_t d,
                                    const void* Qraw, const float* mcap, int64_t K, const int* cand, float lam, int gate, float* scores,
                                    void* workspace, void* stream);
int64_t dvlp_xattn_long_index_ground_workspace_bytes(int64_t Bj, int64_t W, int64_t K, int64_t G);
int dvlp_xattn_long_index_pairs_ground(int64_t capacity, int64_t G, const void* index, const float* mimg, int64_t Bj, int64_t W, int64_t d,
                                       const void* Qraw, const float* mcap, const int* cand, int64_t K, int64_t frames, float lam, int gate,
                                       float* score, float* word_scores, float* region_scores, int* word_region, float* word_region_weight,
                                       int* region_word, float* frame_scores, void* workspace, void* stream);

/* Moments of a long video (no reference counterpart): the pairs of dvlp_xattn_long_index_pairs_fwd scored on every window of
   `win` consecutive frames instead of the whole video.  A video of G regions has `frames` frames of R = G / frames regions, frame-major;
   window m covers the frames [m stride, m stride + win), i.e. the regions [g0, g1) = [m stride R, (m stride + win) R), and
     scores[j][k][m] = the local similarity of (video cand[j K + k] restricted to the regions [g0, g1), caption j)
   -- the pair score of the family above with C[g0:g1], m_img[g0:g1] as the video side: the means run over the win R regions of the window
   and all W words, the focal gate of image->text compares against 1 / (win R).  The global cosine is not part of it.  A window without an
   unmasked region (m_img != 0 on all of it) scores -inf.  The index is read in place -- a window is rows g0 .. g1 of chat, columns g0 .. g1
   of chatT and entries g0 .. g1 of nc -- by one workgroup per (window, pair), all M windows of all pairs in one launch; nothing is resident
   beyond the index of dvlp_xattn_long_index_bytes / _add, and the workspace is dvlp_xattn_long_index_query_workspace_bytes(Bj, W).
     dvlp_xattn_long_index_moments_count  host arithmetic: M = (frames - win) / stride + 1, or a negative DVLP_ERR_* when frames does not
                                          divide G, win is outside [1, frames], stride < 1 or G is out of range.
     dvlp_xattn_long_index_moments_fwd    scores fp32 [Bj][K][M].  Argument rules of dvlp_xattn_long_index_pairs_fwd (DVLP_ERR_SHAPE /
                                          DVLP_ERR_UNSUPPORTED before anything is launched, null pointers refused; K M <= 2^31 - 1); what
                                          _moments_count refuses is refused here with its code.  A cand entry outside [0, capacity) reads
                                          nothing: NaN in all M scores of that pair.
   With win = frames (M = 1) the score equals dvlp_xattn_long_index_pairs_fwd's bit for bit.  No float atomics; every cross-wave sum is taken
   in a fixed order: two runs give equal bytes. */
int64_t dvlp_xattn_long_index_moments_count(int64_t G, int64_t frames, int64_t win, int64_t stride);
int dvlp_xattn_long_index_moments_fwd(int64_t capacity, int64_t G, const void* index, const float* mimg, int64_t Bj, int64_t W, int64_t d,
                                      const void* Qraw, const float* mcap, int64_t K, const int* cand, int64_t frames, int64_t win,
                                      int64_t stride, float lam, int gate, float* scores, void* workspace, void* stream);

/* Resident caption index + video-major pair list (video-to-text search, demovlp_amd/search.py): the family above with the roles swapped.
   The index is caller-owned device memory of dvlp_xattn_caption_index_bytes(capacity, W) bytes holding, per caption of W words, what the
   fused kernel's prep writes per call: qhat [Wp][256] and qhatT [256][Wk] in bf16 (Wp = W rounded up to 16, Wk = to 32) and the word norms
   nq [W] in fp32, each section rounded up to 256 bytes (123 392 bytes at capacity 1, W = 99).  bf16 only, W <= 112, and a query's G inside the
   fused range (G <= 288): anything else returns DVLP_ERR_UNSUPPORTED (size helpers: a negative value; Bi > 65535 is DVLP_ERR_SHAPE).
     dvlp_xattn_caption_index_add        preps captions Qraw (bf16 [n][W][256]) into rows row0 .. row0 + n; a row's bytes do not depend on
                                         the call that wrote it (several adds == one add).
     dvlp_xattn_caption_index_pairs_fwd  preps the Bi videos Craw (bf16 [Bi][G][256]) into `workspace`
                                         (dvlp_xattn_caption_index_query_workspace_bytes(Bi, G, W): independent of the capacity), then one
                                         workgroup per (k, i) runs the per-pair code of the full-grid fused kernel: scores[i][k] (fp32 [Bi][K])
                                         equals entry [i][cand[i K + k]] of dvlp_xattn_fwd's grid bit for bit.  cand is int32 [Bi][K] on the
                                         device; an entry outside [0, capacity) reads nothing and scores NaN.  mcap is the additive word mask
                                         of the whole index, fp32 [capacity][W]; mimg is fp32 [Bi][G].  Bi <= 65535.
     dvlp_xattn_caption_index_pairs_ground  the same grid with the outputs of dvlp_xattn_index_pairs_ground, laid out [Bi][K][...] (score
                                         [Bi][K], word rows [Bi][K][W], region rows [Bi][K][G], frame_scores [Bi][K][frames]); the same
                                         argument rules (every error DVLP_ERR_SHAPE), NaN / -1 rows for a cand entry outside the index.
                                         workspace: dvlp_xattn_caption_index_ground_workspace_bytes(Bi, G, K, W) bytes. */
int64_t dvlp_xattn_caption_index_bytes(int64_t capacity, int64_t W);
int dvlp_xattn_caption_index_add(int64_t capacity, int64_t W, int64_t row0, int64_t n, const void* Qraw, void* index, void* stream);
int64_t dvlp_xattn_caption_index_query_workspace_bytes(int64_t Bi, int64_t G, int64_t W);
int dvlp_xattn_caption_index_pairs_fwd(int64_t capacity, int64_t W, const void* index, const float* mcap, int64_t Bi, int64_t G, int64_t d,
                                       const void* Craw, const float* mimg, int64_t K, const int* cand, float lam, int gate, float* scores,
                                       void* workspace, void* stream);
int64_t dvlp_xattn_caption_index_ground_workspace_bytes(int64_t Bi, int64_t G, int64_t K, int64_t W);
int dvlp_xattn_caption_index_pairs_ground(int64_t capacity, int64_t W, const void* index, const float* mcap, int64_t Bi, int64_t G, int64_t d,
                                          const void* Craw, const float* mimg, const int* cand, int64_t K, int64_t frames, float lam, int gate,
                                          float* score, float* word_scores, float* region_scores, int* word_region, float* word_region_weight,
                                          int* region_word, float* frame_scores, void* workspace, void* stream);

/* Long QUERY videos over the resident caption index (no reference counterpart): dvlp_xattn_caption_index_pairs_fwd / _pairs_ground
   for 1 <= G <= 1152 regions, W <= 112 words, bf16, on the region-tiled pair kernel of dvlp_xattn_long_index_* with the video-major (K, Bi)
   grid.  The resident side is the index dvlp_xattn_caption_index_bytes / _add define, byte for byte: there is no add or bytes entry of this
   family.  The argument lists, the [Bi][K][...] outputs, the NaN / -1 rows of a cand entry outside [0, capacity) and the argument rules are
   those of dvlp_xattn_caption_index_*; only the range of G differs -- the size helpers return a negative DVLP_ERR_* outside it, _pairs_fwd
   DVLP_ERR_UNSUPPORTED, _pairs_ground DVLP_ERR_SHAPE.  workspace (the video-side prep): _query_workspace_bytes(Bi, G, W) resp.
   _ground_workspace_bytes(Bi, G, K, W) bytes, at G <= 288 the sizes of the short family.  scores[i][k] equals, bit for bit, what
   dvlp_xattn_long_index_pairs_fwd gives for the pair (video i, caption cand[i K + k]) from a video index of the same videos, every grounding
   row likewise, and _pairs_ground's score equals _pairs_fwd's: the per-pair code is shared and a prepared row's bytes do not depend on the
   call that wrote it.  word_region_weight is the fp32 quotient of dvlp_xattn_long_index_pairs_ground.  No float atomics. */
int64_t dvlp_xattn_long_caption_index_query_workspace_bytes(int64_t Bi, int64_t G, int64_t W);
int dvlp_xattn_long_caption_index_pairs_fwd(int64_t capacity, int64_t W, const void* index, const float* mcap, int64_t Bi, int64_t G, int64_t d,
                                            const void* Craw, const float* mimg, int64_t K, const int* cand, float lam, int gate, float* scores,
                                            void* workspace, void* stream);
int64_t dvlp_xattn_long_caption_index_ground_workspace_bytes(int64_t Bi, int64_t G, int64_t K, int64_t W);
int dvlp_xattn_long_caption_index_pairs_ground(int64_t capacity, int64_t W, const void* index, const float* mcap, int64_t Bi, int64_t G, int64_t d,
                                               const void* Craw, const float* mimg, const int* cand, int64_t K, int64_t frames, float lam,
                                               int gate, float* score, float* word_scores, float* region_scores, int* word_region,
                                               float* word_region_weight, int* region_word, float* frame_scores, void* workspace, void* stream);

/* Moments of a long QUERY video against the resident caption index (no reference counterpart): the windows of
   dvlp_xattn_long_index_moments_fwd on the pairs of dvlp_xattn_long_caption_index_pairs_fwd.  Window m of video i covers the frames
   [m stride, m stride + win), i.e. the regions [m stride R, (m stride + win) R) with R = G / frames, and its score is the local similarity
   of (video i restricted to those regions, caption cand[i K + k]) -- bit for bit what dvlp_xattn_long_index_moments_fwd gives for that
   pair and window from a video index of the same videos.  M = dvlp_xattn_long_index_moments_count(G, frames, win, stride).
     windows_per_group  0: the host planner chooses (arithmetic on Bi, K, M alone); n >= 1: each workgroup stages its caption once and scores
                        up to n consecutive windows of one pair in turn; negative: DVLP_ERR_SHAPE.  Every window's arithmetic is independent
                        of the chunking: the scores are byte-identical for every value.
     window_major       0: scores fp32 [Bi][K][M]; 1: scores fp32 [Bi][M][K] (rows for a per-window top-k over the captions).
   The argument lists and rules are those of the two parent entries: DVLP_ERR_SHAPE / DVLP_ERR_UNSUPPORTED before anything is launched, null
   pointers refused, Bi <= 65535, Bi K M <= 2^31 - 1, and what _moments_count refuses is refused with its code.  A cand entry outside
   [0, capacity) reads nothing: NaN in all M scores of that pair, in either layout.  A window without an unmasked region scores -inf.
   Nothing new is resident; workspace: dvlp_xattn_long_caption_index_query_workspace_bytes(Bi, G, W).  With win = frames the score equals
   dvlp_xattn_long_caption_index_pairs_fwd's bit for bit.  No float atomics: two runs give equal bytes. */
int dvlp_xattn_long_caption_index_moments_fwd(int64_t capacity, int64_t W, const void* index, const float* mcap, int64_t Bi, int64_t G, int64_t d,
                                              const void* Craw, const float* mimg, int64_t K, const int* cand, int64_t frames, int64_t win,
                                              int64_t stride, int64_t windows_per_group, int window_major, float lam, int gate, float* scores,
                                              void* workspace, void* stream);

/* ---- row top-k (csrc/topk.hip; no reference counterpart: the reference ranks on the host, model/metric.py) ----
   Per row m of the fp32 matrix x [M][ld] (first N columns): val[m][0..K) = the K largest values, descending, idx[m][..] = their column numbers
   + index_base (int32).  Total order: larger value first, equal values by smaller index -- np.argsort(-x, kind="stable")[:K]; -0.0 == +0.0; a NaN
   sorts after every number.  N < K: the tail is val = -inf, idx = -1.  merge = 1: the K entries already in val / idx take part as further
   candidates (idx as they are; idx < 0 = filler), so a caller can stream over column chunks (index_base = c * chunk, merge = c > 0) and gets
   the one-shot result bit for bit.  Values come back with the bits they had.  No float atomics; the result does not depend on scheduling.
   1 <= K <= 1024, N < 2^31, ld >= N, index_base + N < 2^31; workspace: dvlp_topk_workspace_bytes(M, N, K) (negative DVLP_ERR_* for a bad shape). */
int64_t dvlp_topk_workspace_bytes(int64_t M, int64_t N, int K);
int dvlp_topk_rows(int64_t M, int64_t N, const float* x, int64_t ld, int K, int64_t index_base, float* val, int* idx, int merge,
                   void* workspace, void* stream);
/* dvlp_topk_rows with a per-column allow mask: by definition dvlp_topk_rows applied to each row with its disallowed columns DELETED -- the
   same total order, the same raw value bits, the same (-inf, -1) tail when fewer than K columns are allowed (a row with none is all tail); an
   allowed column holding -inf is listed with its index, a disallowed column never is, whatever it holds.
     allow     device memory of 32-bit words, addressed by GLOBAL column number: column c of row m takes part iff bit (index_base + c) & 31 of
               allow[m * allow_ld + ((index_base + c) >> 5)] is set, so a caller streaming over column chunks passes the same mask with a moving
               index_base (any value, not only multiples of 32).
     allow_ld  words between the mask rows of consecutive matrix rows; 0 = one mask row shared by all M rows; otherwise at least
               ceil((index_base + N) / 32).
   Words the kernel may load: of each mask row, words index_base >> 5 .. (index_base + N - 1) >> 5, nothing before or after; in the last of
   them the bits at or beyond index_base + N are never read as columns.  merge = 1 as above: the entries already in val / idx take part
   unconditionally (they passed the mask when they were selected), so chunked calls equal the one-shot call bit for bit.  The scan is the
   kernel of dvlp_topk_rows with the mask as a template parameter (one or two more word loads per 16-byte load); dvlp_topk_rows itself runs the
   unmasked instantiation.  Shape limits, workspace and error codes of dvlp_topk_rows; DVLP_ERR_SHAPE also for a null or misaligned allow, a
   negative allow_ld and a positive one below ceil((index_base + N) / 32).  No float atomics; the result does not depend on scheduling. */
int dvlp_topk_rows_masked(int64_t M, int64_t N, const float* x, int64_t ld, int K, int64_t index_base, const uint32_t* allow, int64_t allow_ld,
                          float* val, int* idx, int merge, void* workspace, void* stream);

/* ---- moment selection (csrc/moments.hip; no reference counterpart) ----
   Greedy temporal non-maximum suppression over window scores, per row.  scores is fp32 [P][ld]; the first M columns of a row are the window
   scores of one (query, video) pair, window c covering the frames [start[c], start[c] + length[c]) (start / length int32 [M] on the device,
   start >= 0, length >= 1, start + length < 2^30: not checked).  val is fp32 [P][T], pos int32 [P][T].  For each row independently: a window
   is selectable while it is alive and its score is neither NaN nor -inf; T times, the selectable window that is largest in the order of
   dvlp_topk_rows (by value, -0.0 == +0.0, then by smaller position) is written -- the bits its value had, and its position -- and killed,
   and with it every alive window c' with  float(inter) > float(union) * iou,  where inter = max(0, min(e, e') - max(s, s')) and
   union = len + len' - inter are integers and the right-hand side is ONE fp32 multiply.  When nothing selectable is left the remaining
   entries are pos = -1 with val = NaN (0x7fc00000) if the row holds a NaN anywhere in its M columns, -inf otherwise.  iou = 0: any temporal
   overlap suppresses; iou = 1: nothing but the selected window is suppressed -- dvlp_topk_rows without its NaN / -inf entries.
   1 <= T <= 32, 1 <= M <= 4096, ld >= M, P >= 0 (0: nothing is launched), P max(ld, T) < 2^31, 0 <= iou <= 1; a null or misaligned pointer
   or a shape violation is DVLP_ERR_SHAPE, M > 4096 or T > 32 DVLP_ERR_UNSUPPORTED, before anything is launched.  No workspace, no atomics:
   two runs give equal bytes.  Columns [M, ld) are never read; nothing outside [P][T] of val / pos is written.  stream: a hipStream_t. */
int dvlp_moment_select(int64_t P, int64_t M, const float* scores, int64_t ld, const int* start, const int* length, int T, float iou,
                       float* val, int* pos, void* stream);

/* ---- loss heads: sim_matrix (model/model.py:582-590) + NormSoftmaxLoss (model/loss.py:126-138) + RWALoss tail
 *      (model/loss.py:105-116) + GlobalLocalLoss sum (:29-45); forward and analytic gradients in one launch        ---- */
int dvlp_global_local_loss(int dtype, int64_t B, int64_t d, const void* gt, const void* go, const float* xs, float temperature,
                           float lam, int use_global, int use_local, int stages, float* sim, float* dsim, void* dgt, void* dgo,
                           float* dxs, float* losses, void* stream);

/* rectangular sim_matrix (model/model.py:582-590 on [N,256] x [M,256], e.g. the whole eval set at trainer/trainer_dist.py:369):
   xn (fp32) = x / max(|x|, 1e-8) row-wise and norm = |x|; the [N,M] product and its two gradient products are dvlp_gemm calls in
   DVLP_F32; dvlp_rownorm_bwd takes d loss / d xn back through the normalisation */
int dvlp_rownorm_fwd(int dtype, int64_t M, int64_t d, const void* x, float* xn, float* norm, void* stream);
int dvlp_rownorm_bwd(int dtype, int64_t M, int64_t d, const void* x, const float* norm, const float* dxn, void* dx, void* stream);

/* ---- video-QA answer head (csrc/qahead.hip): BUTDQAHead (model/video_qa_mdoel.py:56-97) on the embeddings ObjectQARelation.compute_fusion
 *      hands over (model/model.py:281-289), and the QA loss (model/loss.py:180-187).  Every sum inside adds its partials in a fixed order. ---- */
/* torch.nn.utils.weight_norm(nn.Linear, dim=None) (model/video_qa_mdoel.py:16-22, 63): W = g V / |V|_F with a scalar g, for `count` (<= 8)
   tensors in one launch.  V, g, numel, W, Wb, dW, dV, dg are HOST arrays of `count` device pointers / element counts; everything they point to
   is fp32 except Wb (optional bf16 copy of W; the table or single entries may be NULL).  norms [count] fp32 is written by _fwd and read by
   _bwd, which turns the gradient dW of the folded weight into dV = (g / |V|) (dW - <dW, V> / |V|^2 V) and dg = <dW, V> / |V|. */
int dvlp_wn_fold_fwd(int count, const void* const* V, const void* const* g, const int64_t* numel, void* const* W, void* const* Wb,
                     float* norms, void* stream);
int dvlp_wn_fold_bwd(int count, const void* const* V, const void* const* g, const int64_t* numel, const void* const* dW, const float* norms,
                     void* const* dV, void* const* dg, void* stream);
/* torch.max(text_embeddings, dim=1) (model/model.py:285): x [B][T][d] (dtype) -> out [B][d] fp32 and idx [B][d] int32, the FIRST maximal
   token (padded tokens take part, as in the reference; unlike torch.max a NaN never wins the comparison, it is skipped); _bwd scatters dout [B][d] back into dx [B][T][d] (dtype), zero elsewhere */
int dvlp_token_max_fwd(int dtype, int64_t B, int64_t T, int64_t d, const void* x, float* out, void* idx, void* stream);
int dvlp_token_max_bwd(int dtype, int64_t B, int64_t T, int64_t d, const float* dout, const void* idx, void* dx, void* stream);
/* Attention.forward + the weighted region sum of BUTDQAHead.forward (model/video_qa_mdoel.py:56-75, 94-97), widths fixed at 256.  Per sample b:
     qp = relu(Wq q_b + bq);  H = v_b Wv^T + bv [G][256];  logit_g = ((relu(H_g) . qp . keep_g / (1 - drop_p)) . wl + bl) mask[b][g]
     att = softmax_g(logit)  (the mask MULTIPLIES, so padded regions keep logit 0 and take part);  pooled = sum_g att_g v_g
   v (dtype) is read in place: region g of sample b starts at v + b v_sample_stride + g v_row_stride (elements; 16-byte aligned, 256 contiguous
   channels).  mask [B][G], q [B][256], Wq [256][256], bq, bv, wl [256], bl [1] are fp32 (the FOLDED weights).
   Route: H == NULL is the fused one (dvlp_qa_attend_fused(dtype, G) != 0: bf16, G <= 288; anything else returns DVLP_ERR_UNSUPPORTED) -- Wv_bf16
   [256][256] is staged in LDS, H is formed by v_mfma_f32_16x16x32_bf16 on a (64-row tile, sample) grid and consumed in registers.  Otherwise H
   (dtype, row b hrows + g, 256 channels, bias added, before the ReLU) is the caller's dvlp_gemm product and Wv_bf16 is not read.
   Dropout (drop_p > 0): keep bits are Philox words of drop_state at `site`, element (b G + g) 256 + n in the numbering of dvlp_dropout_fwd;
   _fwd copies the four state words to state_snapshot, which is what _bwd takes.
   Outputs: qp [B][256], att [B][G], pooled [B][256] fp32.
   _bwd: from d_pooled [B][256] fp32 it writes dv (dtype, row b hrows + g: the direct part att_g d_pooled ONLY), dH (dtype, same rows: the
   gradient of H before the ReLU; rows g >= G of a sample are not written), dq [B][256], dWq [256][256], dbq, dbv, dwl [256], dbl [1] fp32.  The
   two large products are the caller's: dv += dH Wv (DVLP_EPI_ACCUM) and dWv = dH^T v.  The fused route recomputes H.  workspace: fp32,
   dvlp_qa_attend_workspace_floats(B, G) elements. */
int64_t dvlp_qa_attend_fused(int dtype, int64_t G);
int64_t dvlp_qa_attend_workspace_floats(int64_t B, int64_t G);
int dvlp_qa_attend_fwd(int dtype, int64_t B, int64_t G, const void* v, int64_t v_sample_stride, int64_t v_row_stride, const float* mask,
                       const float* q, const float* Wq, const float* bq, const void* Wv_bf16, const float* bv, const float* wl, const float* bl,
                       const void* H, int64_t hrows, float drop_p, const void* drop_state, int site, void* state_snapshot, float* qp, float* att,
                       float* pooled, void* stream);
int dvlp_qa_attend_bwd(int dtype, int64_t B, int64_t G, const void* v, int64_t v_sample_stride, int64_t v_row_stride, const float* mask,
                       const float* q, const float* Wq, const void* Wv_bf16, const float* bv, const float* wl, const void* H, int64_t hrows,
                       float drop_p, const void* state_snapshot, int site, const float* qp, const float* att, const float* d_pooled, void* dv,
                       void* dH, float* dq, float* dWq, float* dbq, float* dbv, float* dwl, float* dbl, float* workspace, void* stream);
/* nn.CrossEntropyLoss (model/loss.py:180-187) and the trainer's `logits.max(dim=-1)[1]` (trainer/trainer_dist.py:545) in one pass over fp32
   logits [B][C] with int64 labels [B]: loss_rows [B], loss [1] = their mean (summed in row order), dlogits [B][C] = (softmax - onehot) / B
   (NULL: not wanted), pred [B] int32 = first maximal class (a NaN logit never wins the arg-max, unlike torch.max).  A label outside [0, C) makes its row's loss NaN. */
int dvlp_softmax_xent(int64_t B, int64_t C, const float* logits, const void* labels, float* loss_rows, float* dlogits, void* pred, float* loss,
                      void* stream);

/* ---- optimizer: transformers.AdamW as constructed at train_dist_multi.py:64 ---- */
int dvlp_adamw_step(int64_t n, float* p, const float* g, float* m, float* v, float lr, float beta1, float beta2, float eps,
                    float weight_decay, int64_t step, float grad_scale, void* bf16_shadow, void* stream);
/* same update with the hyper-parameters in DEVICE memory: hyper[8] fp32 = {lr, beta1, beta2, eps, weight_decay, grad_scale, step,
   step_size}; each call first advances hyper[6] (the step counter) and recomputes hyper[7] on the device, so one captured hipGraph of
   a training step replays with the right bias correction, and lr / grad_scale change by writing the buffer */
int dvlp_adamw_step_dev(int64_t n, float* p, const float* g, float* m, float* v, float* hyper, void* bf16_shadow, void* stream);
/* the two halves of dvlp_adamw_step_dev, for a step whose update is spread over the backward pass: _prep advances the device step
   counter / step size once per step, _range updates n elements at the given (16-byte aligned) pointers with the hyper-parameters as
   they stand */
int dvlp_adamw_prep_dev(float* hyper, void* stream);
int dvlp_adamw_range_dev(int64_t n, float* p, const float* g, float* m, float* v, const float* hyper, void* bf16_shadow, void* stream);

#ifdef __cplusplus
}
#endif
#endif
