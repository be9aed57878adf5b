// Fused per-pair local-loss kernels (K11 "xattn_pair_fused" of SURVEY.md section 2.2; model/loss.py:209-330 restated per
// section 8(a) row A10), bf16 MFMA path.  ONE workgroup per (video i, caption j) pair keeps everything on chip:
//
//   S = LeakyReLU(C^ Q^T)            MFMA, rows of S owned by waves (accumulators never leave registers)
//   both focal softmaxes               VALU on the accumulators; the column direction exchanges 3 x [8][W] floats through LDS
//   P1' [W][G], P2' [G][W]             written ONCE to LDS as bf16 -- the B operands of the two context products
//   wc^T = C^^T P1'^T, wc2^T = Q^^T P2'^T   MFMA, waves own 32-channel slices of d; only |wc|^2, |wc2|^2 are kept
//   cosines                            <raw, ctx> = (|raw| + eps) * sum P' S_pre  comes straight from the softmax pass
//                                      (C = C^ (|C| + eps)), so the raw embeddings are never re-read
//
// and writes one scalar.  The round-1 structure (xattn.hip; still used for fp32 parity runs and for F*R > 288) streamed
// S, P1, P2, wc, wc2 (+ their gradients) through HBM between 9 batched GEMMs and 6 VALU kernels: ~2 GB of workspace and
// ~4.5 ms per step at B = 64; this keeps O(B (G + W) d) operands + O(B^2) results.
//
// The backward recomputes S and the softmaxes from the same operands (nothing but the inputs is saved), then runs the six
// gradient products per pair on chip; the per-image / per-caption accumulations go through fp32 atomics in HBM
// (dC^_i: 64 adders per address, dQ^_j: 64 adders).
//
// MFMA layouts (v_mfma_f32_16x16x32_bf16): lane l holds A[row l&15][k = 8 (l>>4) + t], B[k = 8 (l>>4) + t][col l&15], t < 8;
// D[row 4 (l>>4) + r][col l&15], r < 4.
#include "common.h"

constexpr int FD = 256;          // projection_dim
constexpr int FW_MAXB = 7;       // word blocks of 16 (W <= 112)
constexpr int FG_SLOTS = 3;      // region blocks of 16 per wave (8 waves: G <= 384 by registers, <= 288 by LDS)
constexpr int FQS = FD + 8;      // LDS row stride of the staged Q^ (elements): 528 B rows -> conflict-free 16-byte fragment reads

struct FusedArgs {
    const bf16 *chat, *chatT, *qhat, *qhatT;   // [Bi][Gr][256], [Bi][256][Gk], [Bj][Wp][256], [Bj][256][Wk]
    const float *nc, *nq;                      // |C_raw| [Bi][G], |Q_raw| [Bj][W]
    const float *mimg, *mcap;                  // additive masks [Bi][G], [Bj][W]
    float* scores;                             // [Bi][Bj]; pair form: [Bi][K]
    const int* cand;                           // pair form: caption of pair (i, k) = cand[i K + k] (NULL: i K + k); index form: video of pair (j, k) = cand[j K + k]
    int Bi, Bj, G, W, Gr, Gk, Wp, Wk, K;
    float lam;
    int gate;
    int stop;                                  // TIMING-ONLY ablation: stop after phase n (0 = run everything)
};

typedef bf16 bf16x2 __attribute__((ext_vector_type(2)));
// two fp32 values as one register of bf16 (round to nearest even: v_cvt_pk_bf16_f32) and back
__device__ __forceinline__ unsigned pk2(float lo, float hi) { bf16x2 p; p[0] = (bf16)lo; p[1] = (bf16)hi; return __builtin_bit_cast(unsigned, p); }
__device__ __forceinline__ float pk_lo(unsigned u) { return __uint_as_float(u << 16); }
__device__ __forceinline__ float pk_hi(unsigned u) { return __uint_as_float(u & 0xffff0000u); }

__device__ __forceinline__ f32x4 mfma16(bf16x8 a, bf16x8 b, f32x4 c) { return __builtin_amdgcn_mfma_f32_16x16x32_bf16(a, b, c, 0, 0, 0); }

// hat rows (x / (|x| + 1e-8), loss.py:333-338) in both orientations + |x|.  One wave per padded row; pad rows / pad
// columns are written as zeros so the MFMA operands can be read without bounds checks.
__global__ __launch_bounds__(256) void xf_prep_kernel(int outer, int inner, int rows_p, int cols_p, const bf16* __restrict__ raw,
                                                      bf16* __restrict__ hat, bf16* __restrict__ hatT, float* __restrict__ nrm) {
    const int lane = threadIdx.x & 63;
    const int rmax = rows_p > cols_p ? rows_p : cols_p;
    const int64_t idx = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (idx >= (int64_t)outer * rmax) return;
    const int o = (int)(idx / rmax), r = (int)(idx % rmax);
    float v[4] = {0.f, 0.f, 0.f, 0.f};
    if (r < inner) {
        const bf16x4 x = *(const bf16x4*)(raw + ((int64_t)o * inner + r) * FD + lane * 4);
#pragma unroll
        for (int t = 0; t < 4; ++t) v[t] = (float)x[t];
        const float n = sqrtf(wave_sum(v[0] * v[0] + v[1] * v[1] + v[2] * v[2] + v[3] * v[3]));
        if (lane == 0) nrm[(int64_t)o * inner + r] = n;
        const float inv = 1.f / (n + 1e-8f);
#pragma unroll
        for (int t = 0; t < 4; ++t) v[t] *= inv;
    }
    bf16x4 h;
#pragma unroll
    for (int t = 0; t < 4; ++t) h[t] = (bf16)v[t];
    if (r < rows_p) *(bf16x4*)(hat + ((int64_t)o * rows_p + r) * FD + lane * 4) = h;
    if (r < cols_p) {
#pragma unroll
        for (int t = 0; t < 4; ++t) hatT[((int64_t)o * FD + lane * 4 + t) * cols_p + r] = h[t];
    }
}

// LDS map of the forward kernel (bytes)
struct FLds { int qs, p2, p1, xa, xb, xc, xd, dotg, dotw, nw1, nw2, total; };
static __host__ __device__ inline FLds flds(int Gr, int Gk, int Wp, int Wk) {
    FLds L;
    const int p2b = Gr * (Wk + 8) * 2, qsb = Wp * FQS * 2, p1b = Wp * (Gk + 8) * 2;
    L.qs = 0; L.p2 = 0;                                   // Q^ is dead (barrier) before P2' is written over it
    L.p1 = (p2b > qsb ? p2b : qsb);
    L.p1 = (L.p1 + 255) & ~255;
    int o = L.p1 + ((p1b + 255) & ~255);
    L.xa = o; o += 8 * 112 * 4; L.xb = o; o += 8 * 112 * 4; L.xc = o; o += 8 * 112 * 4; L.xd = o; o += 8 * 112 * 4;
    L.dotg = o; o += 384 * 4; L.dotw = o; o += 112 * 4; L.nw1 = o; o += 112 * 4; L.nw2 = o; o += 384 * 4;
    L.total = o;
    return L;
}

// sum over the 8 waves' partials of column c (c = 16 nb + (lane & 15)) for every word block
__device__ __forceinline__ void xch_put(float* x, int wid, int lane, const float (&v)[FW_MAXB], int nwb) {
    if ((lane >> 4) == 0) {
#pragma unroll
        for (int nb = 0; nb < FW_MAXB; ++nb) if (nb < nwb) x[wid * 112 + nb * 16 + lane] = v[nb];
    }
}
__device__ __forceinline__ void xch_get(const float* x, int lane, float (&v)[FW_MAXB], int nwb) {
#pragma unroll
    for (int nb = 0; nb < FW_MAXB; ++nb) {
        float t = 0.f;
        if (nb < nwb) {
#pragma unroll
            for (int w = 0; w < 8; ++w) t += x[w * 112 + nb * 16 + (lane & 15)];
        }
        v[nb] = t;
    }
}

// S tiles of this wave's region blocks and both focal softmaxes.
// On return: P1' is in LDS [w][g] (row stride Gk + 8), P2' in LDS [g][w] (row stride Wk + 8), dotg[g] = sum_w P2' S_pre,
// dotw[w] = sum_g P1' S_pre.  S (post-LeakyReLU), rn, cn stay in R for the caller.
struct PairRegs {
    f32x4 S[FG_SLOTS][FW_MAXB];     // LeakyReLU(S_pre)
    float rn[FG_SLOTS][4];          // 1 / (|S_row| + eps)
    float cn[FW_MAXB];              // 1 / (|S_col| + eps)   (column 16 nb + (lane & 15))
};

__device__ __forceinline__ void pair_forward(const FusedArgs& a, char* smem, int i, int j, PairRegs& R) {
    unsigned E[FG_SLOTS][FW_MAXB][2];   // softmax numerators of the pass in flight as packed bf16 pairs (they end as bf16 MFMA operands)
    const int tid = threadIdx.x, lane = tid & 63, lq = lane >> 4, lc = lane & 15;
    const int wid = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int nbg = a.Gr >> 4, nwb = a.Wp >> 4;
    const FLds L = flds(a.Gr, a.Gk, a.Wp, a.Wk);
    bf16* Qs = (bf16*)(smem + L.qs);
    bf16* P1s = (bf16*)(smem + L.p1);
    bf16* P2s = (bf16*)(smem + L.p2);
    float *xa = (float*)(smem + L.xa), *xb = (float*)(smem + L.xb), *xc = (float*)(smem + L.xc), *xd = (float*)(smem + L.xd);
    float *dotg = (float*)(smem + L.dotg), *dotw = (float*)(smem + L.dotw);
    const int p1s = a.Gk + 8, p2s = a.Wk + 8;

    // ---- C^ fragments of this wave's region blocks (wid, wid + 8, wid + 16) are requested first: their L2 latency runs under the
    //      staging of Q^_j [Wp][256] into LDS (16-byte pieces, padded rows)
    const bf16* ch = a.chat + (int64_t)i * a.Gr * FD;
    const float* mimg = a.mimg + (int64_t)i * a.G;
    const float* mcap = a.mcap + (int64_t)j * a.W;
    bf16x8 af[FG_SLOTS][8];
    float mi[FG_SLOTS][4];               // additive region mask; -1e4 for pad rows (exp -> 0)
#pragma unroll
    for (int s = 0; s < FG_SLOTS; ++s) {
        const int rb = wid + 8 * s;
        const bf16* ap = ch + (int64_t)((rb < nbg ? rb : 0) * 16 + lc) * FD + 8 * lq;
#pragma unroll
        for (int ks = 0; ks < 8; ++ks) af[s][ks] = *(const bf16x8*)(ap + ks * 32);
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            const int g = rb * 16 + lq * 4 + r;
            mi[s][r] = (rb < nbg && g < a.G) ? mimg[g] : -1e4f;
        }
    }
    {
        const bf16* q = a.qhat + (int64_t)j * a.Wp * FD;
        for (int p = tid; p < a.Wp * 32; p += blockDim.x) {
            const int r = p >> 5, c = (p & 31) * 8;
            *(bf16x8*)(Qs + r * FQS + c) = *(const bf16x8*)(q + r * FD + c);
        }
    }
    __syncthreads();

    // ---- S = LeakyReLU(C^ Q^T)
#pragma unroll
    for (int s = 0; s < FG_SLOTS; ++s) {
        const int rb = wid + 8 * s;
#pragma unroll
        for (int nb = 0; nb < FW_MAXB; ++nb) R.S[s][nb] = (f32x4){0.f, 0.f, 0.f, 0.f};
        if (rb < nbg) {
#pragma unroll
            for (int nb = 0; nb < FW_MAXB; ++nb) {
                if (nb < nwb) {
                    f32x4 c = (f32x4){0.f, 0.f, 0.f, 0.f};
                    const bf16* bp = Qs + (nb * 16 + lc) * FQS + 8 * lq;
#pragma unroll
                    for (int ks = 0; ks < 8; ++ks) c = mfma16(af[s][ks], *(const bf16x8*)(bp + ks * 32), c);
#pragma unroll
                    for (int r = 0; r < 4; ++r) c[r] = fmaxf(c[r], 0.1f * c[r]);             // LeakyReLU(0.1), loss.py:236
                    R.S[s][nb] = c;
                }
            }
        }
    }
    if (a.stop == 1) return;
    // validity of this lane's columns, caption mask
    float mc[FW_MAXB];                   // additive word mask; -1e4 for pad columns
#pragma unroll
    for (int nb = 0; nb < FW_MAXB; ++nb) {
        const int w = nb * 16 + lc;
        mc[nb] = (nb < nwb && w < a.W) ? mcap[w] : -1e4f;
    }

    // ---- reciprocal row / column norms of S (loss.py:238 in both directions); pad rows / columns of S are exact zeros
    float csq[FW_MAXB];
#pragma unroll
    for (int nb = 0; nb < FW_MAXB; ++nb) csq[nb] = 0.f;
    const float L2E = 1.4426950408889634f * a.lam;        // exp(lam x) = exp2(L2E x)
    float k1[FG_SLOTS][4];                                // per region: exponent scale lam log2(e) / (|S_row| + eps)
#pragma unroll
    for (int s = 0; s < FG_SLOTS; ++s) {
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            float q = 0.f;
#pragma unroll
            // (q += v * v; csq[nb] += v * v, with the contraction written out -- a product at the head of each sum, fused multiply-adds after it --
            //  so that every instantiation of this code rounds alike: left to the optimiser, the grounding kernel got packed products and separate adds)
            for (int nb = 0; nb < FW_MAXB; ++nb) {
                const float v = R.S[s][nb][r];
                q = nb == 0 ? v * v : fmaf(v, v, q);
                csq[nb] = (s == 0 && r == 0) ? v * v : fmaf(v, v, csq[nb]);
            }
            R.rn[s][r] = 1.f / (sqrtf(row16_sum(q)) + 1e-8f);
            k1[s][r] = L2E * R.rn[s][r];
            mi[s][r] = L2E * (mi[s][r] - 1.f);            // exponent offset: lam log2(e) (m_img - 1); z <= lam, so no max pass is needed
        }
    }
#pragma unroll
    for (int nb = 0; nb < FW_MAXB; ++nb) csq[nb] = col4_sum(csq[nb]);
    xch_put(xa, wid, lane, csq, nwb);
    __syncthreads();                                   // (also: every wave is done reading Q^ from LDS)
    xch_get(xa, lane, csq, nwb);
#pragma unroll
    for (int nb = 0; nb < FW_MAXB; ++nb) R.cn[nb] = 1.f / (sqrtf(csq[nb]) + 1e-8f);
    if (a.stop == 2) return;

    // ---- image -> text: for each word, softmax over regions of lam (S rn + m_img) (loss.py:241-259), in exp2 form
    float cs[FW_MAXB];
#pragma unroll
    for (int nb = 0; nb < FW_MAXB; ++nb) cs[nb] = 0.f;
#pragma unroll
    for (int s = 0; s < FG_SLOTS; ++s)
#pragma unroll
        for (int nb = 0; nb < FW_MAXB; ++nb) {
#pragma unroll
            for (int h = 0; h < 2; ++h) {
                const unsigned u = pk2(__builtin_amdgcn_exp2f(fmaf(R.S[s][nb][2 * h], k1[s][2 * h], mi[s][2 * h])),
                                       __builtin_amdgcn_exp2f(fmaf(R.S[s][nb][2 * h + 1], k1[s][2 * h + 1], mi[s][2 * h + 1])));
                E[s][nb][h] = u; cs[nb] += pk_lo(u) + pk_hi(u);
            }
            __builtin_amdgcn_sched_barrier(0);            // keep the unrolled tiles from being interleaved (register pressure)
        }
#pragma unroll
    for (int nb = 0; nb < FW_MAXB; ++nb) cs[nb] = col4_sum(cs[nb]);
    xch_put(xb, wid, lane, cs, nwb);
    __syncthreads();
    xch_get(xb, lane, cs, nwb);
    // focal gate (loss.py:274-283): H = [P G - sum P > 0], P = e / sum e.  sum P is sum e * (1 / sum e) (1 within an ulp), so the
    // gate is a per-word threshold on e:  e > sum P / (G / sum e)
    float thr[FW_MAXB], gs[FW_MAXB], gd[FW_MAXB];
    const float fG = (float)a.G, fW = (float)a.W;
#pragma unroll
    for (int nb = 0; nb < FW_MAXB; ++nb) {
        const float inv = cs[nb] > 0.f ? 1.f / cs[nb] : 0.f;
        thr[nb] = a.gate ? (cs[nb] * inv) / (inv * fG) : -1.f;
        gs[nb] = 0.f; gd[nb] = 0.f;
    }
#pragma unroll
    for (int s = 0; s < FG_SLOTS; ++s)
#pragma unroll
        for (int nb = 0; nb < FW_MAXB; ++nb) {
#pragma unroll
            for (int h = 0; h < 2; ++h) {
                const unsigned u = E[s][nb][h];
                const float e0 = pk_lo(u), e1 = pk_hi(u);
                const unsigned keep = (e0 > thr[nb] ? 0x0000ffffu : 0u) | (e1 > thr[nb] ? 0xffff0000u : 0u);
                const unsigned v = u & keep;
                const float s0 = R.S[s][nb][2 * h], s1 = R.S[s][nb][2 * h + 1];
                E[s][nb][h] = v;
                gs[nb] += pk_lo(v) + pk_hi(v);
                gd[nb] = fmaf(pk_lo(v), fminf(s0, 10.f * s0), fmaf(pk_hi(v), fminf(s1, 10.f * s1), gd[nb]));     // S_pre: undo LeakyReLU(0.1)
            }
            __builtin_amdgcn_sched_barrier(0);
        }
#pragma unroll
    for (int nb = 0; nb < FW_MAXB; ++nb) { gs[nb] = col4_sum(gs[nb]); gd[nb] = col4_sum(gd[nb]); }
    xch_put(xc, wid, lane, gs, nwb);
    xch_put(xd, wid, lane, gd, nwb);
    __syncthreads();
    xch_get(xc, lane, gs, nwb);
    xch_get(xd, lane, gd, nwb);
#pragma unroll
    for (int nb = 0; nb < FW_MAXB; ++nb) {
        gs[nb] = gs[nb] > 0.f ? 1.f / gs[nb] : 0.f;        // P1' = H e / sum(H e)
        if (wid == 0 && lq == 0 && nb < nwb) dotw[nb * 16 + lc] = gd[nb] * gs[nb];
    }
    // P1' -> LDS [w][g], 4 consecutive regions per 8-byte write
#pragma unroll
    for (int s = 0; s < FG_SLOTS; ++s) {
        const int rb = wid + 8 * s;
        if (rb < nbg) {
#pragma unroll
            for (int nb = 0; nb < FW_MAXB; ++nb) {
                if (nb < nwb) {
                    uint2 o;
                    o.x = pk2(pk_lo(E[s][nb][0]) * gs[nb], pk_hi(E[s][nb][0]) * gs[nb]);
                    o.y = pk2(pk_lo(E[s][nb][1]) * gs[nb], pk_hi(E[s][nb][1]) * gs[nb]);
                    *(uint2*)(P1s + (nb * 16 + lc) * p1s + rb * 16 + lq * 4) = o;
                }
            }
        }
    }
    // zero the k padding of P1' (regions Gr .. Gk-1), if any
    if (a.Gk > a.Gr) {
        for (int p = tid; p < a.Wp * (a.Gk - a.Gr); p += blockDim.x) P1s[(p / (a.Gk - a.Gr)) * p1s + a.Gr + p % (a.Gk - a.Gr)] = (bf16)0.f;
    }
    if (a.stop == 3) return;

    // ---- text -> image: for each region, softmax over words of lam (S cn + m_cap); rows live inside the wave
    float kc[FW_MAXB];
#pragma unroll
    for (int nb = 0; nb < FW_MAXB; ++nb) { kc[nb] = L2E * R.cn[nb]; mc[nb] = L2E * (mc[nb] - 1.f); }
#pragma unroll
    for (int s = 0; s < FG_SLOTS; ++s) {
        const int rb = wid + 8 * s;
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            float sum = 0.f;
            float e[FW_MAXB];
#pragma unroll
            for (int nb = 0; nb < FW_MAXB; ++nb) {
                e[nb] = __builtin_amdgcn_exp2f(fmaf(R.S[s][nb][r], kc[nb], mc[nb]));
                sum += e[nb];
            }
            sum = row16_sum(sum);
            const float inv = sum > 0.f ? 1.f / sum : 0.f;
            const float th = a.gate ? (sum * inv) / (inv * fW) : -1.f;
            float g1 = 0.f, g2 = 0.f;
#pragma unroll
            for (int nb = 0; nb < FW_MAXB; ++nb) {
                const float he = e[nb] > th ? e[nb] : 0.f;
                float sv = R.S[s][nb][r];
                asm volatile("" : "+v"(sv));                 // opaque copy: without it S_pre is shared with the image->text pass and 84 more registers stay live
                const float spre = fminf(sv, 10.f * sv);
                e[nb] = he;
                g1 += he; g2 = fmaf(he, spre, g2);
            }
            g1 = row16_sum(g1); g2 = row16_sum(g2);
            const float is = g1 > 0.f ? 1.f / g1 : 0.f;
            const int g = rb * 16 + lq * 4 + r;
            if (rb < nbg) {
                if (lc == 0) dotg[g] = g2 * is;
#pragma unroll
                for (int nb = 0; nb < FW_MAXB; ++nb)
                    if (nb < nwb) P2s[g * p2s + nb * 16 + lc] = (bf16)(e[nb] * is);
            }
            __builtin_amdgcn_sched_barrier(0);
        }
    }
    // zero the k padding of P2' (words Wp .. Wk-1)
    if (a.Wk > a.Wp) {
        for (int p = tid; p < a.Gr * (a.Wk - a.Wp); p += blockDim.x) P2s[(p / (a.Wk - a.Wp)) * p2s + a.Wp + p % (a.Wk - a.Wp)] = (bf16)0.f;
    }
}

// ---- grounding (xf_index_pairs_ground_kernel): where one pair's score came from.  Rows of ONE pair; see DESIGN.md 6e.
struct GroundOut {
    float *word_scores, *region_scores;        // [W], [G]: the cosines whose means are the score
    int *word_region, *region_word;            // [W], [G]: argmax of the image->text logit over regions / of the text->image logit over words
    float *word_weight;                        // [W]: P1'[w][word_region[w]]
    float* frame_scores;                       // [frames] or NULL
    int frames;
};
// "larger logit, then smaller index" as ONE unsigned comparison (the order of csrc/topk.hip): the float mapped to an unsigned that sorts like
// it in the high word, ~index in the low word.  0 is below every key of a real entry and stands for "no entry" (padding).
typedef unsigned long long u64;
__device__ __forceinline__ u64 gr_key(float v, int index) {
    const unsigned u = __float_as_uint(v);
    return ((u64)(u ^ ((u >> 31) ? 0xffffffffu : 0x80000000u)) << 32) | (u64)(0xffffffffu - (unsigned)index);
}
// lam (s n + m).  Written as instructions, not as C++ arithmetic: the optimiser packs and contracts floating-point expressions by what else
// the function holds (see the squared norms in pair_forward), and the score must not depend on that.  Through here the grounding adds no
// floating-point expression for it to weigh against the shared per-pair code.
__device__ __forceinline__ float gr_logit(float lam, float s, float n, float m) {
    float x;
    asm("v_fma_f32 %0, %1, %2, %3\n\tv_mul_f32 %0, %0, %4" : "=&v"(x) : "v"(s), "v"(n), "v"(m), "v"(lam));
    return x;
}
__device__ __forceinline__ int gr_index(u64 k) { return (int)(0xffffffffu - (unsigned)k); }
__device__ __forceinline__ u64 gr_max(u64 a, u64 b) { return a > b ? a : b; }
template <int CTRL>
__device__ __forceinline__ u64 gr_dpp_max(u64 x) {
    const unsigned lo = (unsigned)__builtin_amdgcn_update_dpp(0, (int)(unsigned)x, CTRL, 0xf, 0xf, true);
    const unsigned hi = (unsigned)__builtin_amdgcn_update_dpp(0, (int)(unsigned)(x >> 32), CTRL, 0xf, 0xf, true);
    return gr_max(x, ((u64)hi << 32) | lo);
}
// all-reduce inside each 16-lane row / over the four lanes that share lane & 15 (row16_sum / col4_sum of common.h, for keys)
__device__ __forceinline__ u64 gr_row16_max(u64 k) {
    k = gr_dpp_max<0xB1>(k); k = gr_dpp_max<0x4E>(k); k = gr_dpp_max<0x141>(k); k = gr_dpp_max<0x140>(k);
    return k;
}
__device__ __forceinline__ u64 gr_col4_max(u64 k) {
    {
        auto lo = __builtin_amdgcn_permlane16_swap((unsigned)k, (unsigned)k, false, false);
        auto hi = __builtin_amdgcn_permlane16_swap((unsigned)(k >> 32), (unsigned)(k >> 32), false, false);
        k = gr_max(((u64)hi[0] << 32) | lo[0], ((u64)hi[1] << 32) | lo[1]);
    }
    auto lo = __builtin_amdgcn_permlane32_swap((unsigned)k, (unsigned)k, false, false);
    auto hi = __builtin_amdgcn_permlane32_swap((unsigned)(k >> 32), (unsigned)(k >> 32), false, false);
    return gr_max(((u64)hi[0] << 32) | lo[0], ((u64)hi[1] << 32) | lo[1]);
}

// Both argmaxes of one pair from the fp32 accumulators pair_forward leaves in R (not from the bf16 P1' / P2' tiles, whose rounding makes
// ties the reference does not have).  region_word[g]: row g lives in one 16-lane row of one wave -> written here.  word_region[w]: column w
// is spread over the eight waves -> this wave's best key per word goes to keys [8][112] (u64) over the exchange rows xa, xb, both dead once a
// wave is past the last barrier of pair_forward (xa and xb are last read before that barrier, by every wave); xf_pair_score finishes them.
__device__ __forceinline__ void ground_argmax(const FusedArgs& a, char* smem, int i, int j, const PairRegs& R, const GroundOut& go) {
    const int tid = threadIdx.x, lane = tid & 63, lq = lane >> 4, lc = lane & 15;
    const int wid = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int nbg = a.Gr >> 4, nwb = a.Wp >> 4;
    const float* mimg = a.mimg + (int64_t)i * a.G;
    const float* mcap = a.mcap + (int64_t)j * a.W;
    u64* keys = (u64*)(smem + flds(a.Gr, a.Gk, a.Wp, a.Wk).xa);
    float mc[FW_MAXB];
    bool okw[FW_MAXB];
    u64 kw[FW_MAXB];
#pragma unroll
    for (int nb = 0; nb < FW_MAXB; ++nb) {
        const int w = nb * 16 + lc;
        okw[nb] = nb < nwb && w < a.W;
        mc[nb] = okw[nb] ? mcap[w] : 0.f;
        kw[nb] = 0ull;
    }
#pragma unroll
    for (int s = 0; s < FG_SLOTS; ++s) {
        const int rb = wid + 8 * s;
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            const int g = rb * 16 + lq * 4 + r;
            const bool okg = rb < nbg && g < a.G;
            const float mi = okg ? mimg[g] : 0.f;
            u64 kg = 0ull;
#pragma unroll
            for (int nb = 0; nb < FW_MAXB; ++nb) {
                const float sv = R.S[s][nb][r];
                if (okg) kw[nb] = gr_max(kw[nb], gr_key(gr_logit(a.lam, sv, R.rn[s][r], mi), g));                // lam (A[g][w] + m_img[g])
                if (okw[nb]) kg = gr_max(kg, gr_key(gr_logit(a.lam, sv, R.cn[nb], mc[nb]), nb * 16 + lc));       // lam (A2[g][w] + m_cap[w])
            }
            kg = gr_row16_max(kg);
            if (okg && lc == 0) go.region_word[g] = gr_index(kg);
        }
    }
#pragma unroll
    for (int nb = 0; nb < FW_MAXB; ++nb) {
        const u64 k = gr_col4_max(kw[nb]);
        if (lq == 0 && nb < nwb) keys[wid * 112 + nb * 16 + lc] = k;
    }
}

// The score of one (video i, caption j) pair -> *out: the whole forward of every launch shape below (full grid, pair lists), so that a
// pair's arithmetic -- and its result, bit for bit -- does not depend on which of them computed it.  GROUND adds the rows of `go` and one
// barrier; it changes no operand and no order of the arithmetic that ends in *out.
template <bool GROUND>
__device__ __forceinline__ void xf_pair_score(const FusedArgs& a, char* smem, int i, int j, float* out, const GroundOut& go) {
    const int tid = threadIdx.x, lane = tid & 63, lq = lane >> 4, lc = lane & 15;
    const int wid = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int nbg = a.Gr >> 4, nwb = a.Wp >> 4;
    const FLds L = flds(a.Gr, a.Gk, a.Wp, a.Wk);
    float *dotg = (float*)(smem + L.dotg), *dotw = (float*)(smem + L.dotw), *nw1 = (float*)(smem + L.nw1), *nw2 = (float*)(smem + L.nw2);
    const bf16* P1s = (const bf16*)(smem + L.p1);
    const bf16* P2s = (const bf16*)(smem + L.p2);
    const int p1s = a.Gk + 8, p2s = a.Wk + 8;
    // per-wave partials of |wc_w|^2 [8][112] (the exchange rows xa, dead once P1' / P2' are published) and of |wc2_g|^2 [8][p1s] (over P1',
    // dead once every wave is past the wc product): summed in wave order below, so the result does not depend on which wave finished first
    float* nw1p = (float*)(smem + L.xa);
    float* nw2p = (float*)(smem + L.p1);
    {
        PairRegs R;
        pair_forward(a, smem, i, j, R);
        if constexpr (GROUND) ground_argmax(a, smem, i, j, R, go);
    }
    // A operands of the two context products (this wave's 32 channels of C^^T and Q^^T) are requested BEFORE the barrier that
    // publishes P1' / P2': their L2 latency runs under the wait for the slowest wave
    constexpr int MAXKS = 9;                               // Gk <= 288
    const int nks1 = a.Gk >> 5, nks2 = a.Wk >> 5;
    bf16x8 ca[2][MAXKS], qa[2][4];
    {
        const bf16* ct = a.chatT + ((int64_t)i * FD + wid * 32 + lc) * a.Gk + 8 * lq;
        const bf16* qt = a.qhatT + ((int64_t)j * FD + wid * 32 + lc) * a.Wk + 8 * lq;
#pragma unroll
        for (int ks = 0; ks < MAXKS; ++ks) {
            const int k = ks < nks1 ? ks : 0;
            ca[0][ks] = *(const bf16x8*)(ct + k * 32); ca[1][ks] = *(const bf16x8*)(ct + (int64_t)16 * a.Gk + k * 32);
        }
#pragma unroll
        for (int ks = 0; ks < 4; ++ks) {
            const int k = ks < nks2 ? ks : 0;
            qa[0][ks] = *(const bf16x8*)(qt + k * 32); qa[1][ks] = *(const bf16x8*)(qt + (int64_t)16 * a.Wk + k * 32);
        }
    }
    __syncthreads();
    if (a.stop >= 1 && a.stop <= 4) { if (tid == 0) *out = dotg[0] + dotw[0]; return; }
    if constexpr (GROUND) {
        // word w: the best of the eight waves' keys, and its weight from the published P1' tile (P1' is overwritten after the next product)
        if (tid < a.W) {
            const u64* keys = (const u64*)(smem + L.xa);
            u64 k = 0ull;
#pragma unroll
            for (int w = 0; w < 8; ++w) k = gr_max(k, keys[w * 112 + tid]);
            const int g = gr_index(k);
            go.word_region[tid] = g;
            go.word_weight[tid] = (float)P1s[tid * p1s + g];
        }
        __syncthreads();                                   // the keys are read: xa takes the |wc|^2 partials below
    }

    // ---- |wc_w|^2: wc^T [d][w] = C^^T [d][g] P1'^T; wave wid owns channels 32 wid .. 32 wid + 31
    {
        f32x4 acc[2][FW_MAXB];
#pragma unroll
        for (int db = 0; db < 2; ++db)
#pragma unroll
            for (int nb = 0; nb < FW_MAXB; ++nb) acc[db][nb] = (f32x4){0.f, 0.f, 0.f, 0.f};
#pragma unroll
        for (int ks = 0; ks < MAXKS; ++ks) {
            if (ks < nks1) {
#pragma unroll
                for (int nb = 0; nb < FW_MAXB; ++nb) {
                    if (nb < nwb) {
                        const bf16x8 b = *(const bf16x8*)(P1s + (nb * 16 + lc) * p1s + ks * 32 + 8 * lq);
                        acc[0][nb] = mfma16(ca[0][ks], b, acc[0][nb]);
                        acc[1][nb] = mfma16(ca[1][ks], b, acc[1][nb]);
                    }
                }
            }
        }
#pragma unroll
        for (int nb = 0; nb < FW_MAXB; ++nb) {
            float q = 0.f;
#pragma unroll
            for (int db = 0; db < 2; ++db)
#pragma unroll
                for (int r = 0; r < 4; ++r) q += acc[db][nb][r] * acc[db][nb][r];
            q = col4_sum(q);
            if (nb < nwb && lq == 0) nw1p[wid * 112 + nb * 16 + lc] = q;
        }
    }
    __syncthreads();                                       // every wave is done reading P1': its space takes the |wc2|^2 partials
    // ---- |wc2_g|^2: wc2^T [d][g] = Q^^T [d][w] P2'^T, two region blocks per iteration (independent accumulator chains)
    if (a.stop != 5) {
        for (int gb = 0; gb < nbg; gb += 2) {
            const int gb1 = gb + 1 < nbg ? gb + 1 : gb;
            f32x4 c00 = (f32x4){0.f, 0.f, 0.f, 0.f}, c01 = c00, c10 = c00, c11 = c00;
#pragma unroll
            for (int ks = 0; ks < 4; ++ks) {
                if (ks < nks2) {
                    const bf16x8 b0 = *(const bf16x8*)(P2s + (gb * 16 + lc) * p2s + ks * 32 + 8 * lq);
                    const bf16x8 b1 = *(const bf16x8*)(P2s + (gb1 * 16 + lc) * p2s + ks * 32 + 8 * lq);
                    c00 = mfma16(qa[0][ks], b0, c00); c01 = mfma16(qa[1][ks], b0, c01);
                    c10 = mfma16(qa[0][ks], b1, c10); c11 = mfma16(qa[1][ks], b1, c11);
                }
            }
            float q0 = 0.f, q1 = 0.f;
#pragma unroll
            for (int r = 0; r < 4; ++r) { q0 += c00[r] * c00[r] + c01[r] * c01[r]; q1 += c10[r] * c10[r] + c11[r] * c11[r]; }
            q0 = col4_sum(q0); q1 = col4_sum(q1);
            if (lq == 0) { nw2p[wid * p1s + gb * 16 + lc] = q0; if (gb + 1 < nbg) nw2p[wid * p1s + gb1 * 16 + lc] = q1; }
        }
    }
    __syncthreads();
    for (int t = tid; t < a.Wp; t += blockDim.x) {
        float q = 0.f;
#pragma unroll
        for (int w = 0; w < 8; ++w) q += nw1p[w * 112 + t];
        nw1[t] = q;
    }
    for (int t = tid; t < a.Gr; t += blockDim.x) {
        float q = 0.f;
        if (a.stop != 5) {
#pragma unroll
            for (int w = 0; w < 8; ++w) q += nw2p[w * p1s + t];
        }
        nw2[t] = q;
    }
    __syncthreads();
    // ---- cosines (loss.py:286-291, 317-327): means over ALL W words / G regions (padded ones included, as the reference)
    float part = 0.f;
    const float* nq = a.nq + (int64_t)j * a.W;
    const float* nc = a.nc + (int64_t)i * a.G;
    for (int w = tid; w < a.W; w += blockDim.x) {
        const float n = nq[w];
        const float c = dotw[w] * (n + 1e-8f) / fmaxf(n * sqrtf(nw1[w]), 1e-8f);
        if constexpr (GROUND) go.word_scores[w] = c;
        part += c / (float)a.W;
    }
    for (int g = tid; g < a.G; g += blockDim.x) {
        const float n = nc[g];
        const float c = dotg[g] * (n + 1e-8f) / fmaxf(n * sqrtf(nw2[g]), 1e-8f);
        if constexpr (GROUND) { go.region_scores[g] = c; nw2[g] = c; }      // (nw2[g] is this thread's own entry: kept for the frame means)
        part += c / (float)a.G;
    }
    part = wave_sum(part);
    float* red = (float*)(smem + L.xb);
    if (lane == 0) red[wid] = part;
    __syncthreads();
    if (tid == 0) {
        float t = 0.f;
        for (int w = 0; w < 8; ++w) t += red[w];
        *out = t;
    }
    if constexpr (GROUND) {
        // frame f: mean of the region cosines (nw2, published by the barrier above) over its unmasked regions, summed in region order
        if (go.frame_scores && tid < go.frames) {
            const float* mimg = a.mimg + (int64_t)i * a.G;
            const int rf = a.G / go.frames;
            float t = 0.f;
            int n = 0;
            for (int g = tid * rf; g < (tid + 1) * rf; ++g)
                if (mimg[g] == 0.f) { t += nw2[g]; ++n; }
            go.frame_scores[tid] = n ? t / (float)n : -__builtin_inff();
        }
    }
}

// full grid: workgroup (j, i) -> scores[i][j]
__global__ __launch_bounds__(512) void xf_fwd_kernel(FusedArgs a) {
    extern __shared__ __attribute__((aligned(16))) char smem[];
    const int j = blockIdx.x, i = blockIdx.y;
    xf_pair_score<false>(a, smem, i, j, a.scores + (int64_t)i * a.Bj + j, GroundOut{});
}

// pair list: workgroup (k, i) -> scores[i][k], caption cand[i K + k]; an index outside [0, Bj) reads nothing and scores NaN
__global__ __launch_bounds__(512) void xf_pairs_fwd_kernel(FusedArgs a) {
    extern __shared__ __attribute__((aligned(16))) char smem[];
    const int i = blockIdx.y;
    const int64_t o = (int64_t)i * a.K + blockIdx.x;
    const int j = a.cand ? a.cand[o] : (int)o;
    if (j < 0 || j >= a.Bj) {
        if (threadIdx.x == 0) a.scores[o] = __builtin_nanf("");
        return;
    }
    xf_pair_score<false>(a, smem, i, j, a.scores + o, GroundOut{});
}

// resident index, query-major pair list: workgroup (k, j) -> scores[j][k], video cand[j K + k] of the index (a.Bi = its capacity); an index
// outside [0, capacity) reads nothing and scores NaN (the -1 of a short top-k list lands here)
__global__ __launch_bounds__(512) void xf_index_pairs_kernel(FusedArgs a) {
    extern __shared__ __attribute__((aligned(16))) char smem[];
    const int j = blockIdx.y;
    const int64_t o = (int64_t)j * a.K + blockIdx.x;
    const int i = a.cand[o];
    if (i < 0 || i >= a.Bi) {
        if (threadIdx.x == 0) a.scores[o] = __builtin_nanf("");
        return;
    }
    xf_pair_score<false>(a, smem, i, j, a.scores + o, GroundOut{});
}

// the same grid with grounding: `go` holds the bases of the [Bj][K][...] output arrays; pair o = j K + k writes row o of each.  An index
// outside [0, capacity) reads nothing: NaN in the float rows, -1 in the int rows.
__global__ __launch_bounds__(512) void xf_index_pairs_ground_kernel(FusedArgs a, GroundOut go) {
    extern __shared__ __attribute__((aligned(16))) char smem[];
    const int j = blockIdx.y;
    const int64_t o = (int64_t)j * a.K + blockIdx.x;
    const int i = a.cand[o];
    go.word_scores += o * a.W; go.word_region += o * a.W; go.word_weight += o * a.W;
    go.region_scores += o * a.G; go.region_word += o * a.G;
    if (go.frame_scores) go.frame_scores += o * go.frames;
    if (i < 0 || i >= a.Bi) {
        const float nan = __builtin_nanf("");
        if (threadIdx.x == 0) a.scores[o] = nan;
        for (int t = threadIdx.x; t < a.W; t += blockDim.x) { go.word_scores[t] = nan; go.word_weight[t] = nan; go.word_region[t] = -1; }
        for (int t = threadIdx.x; t < a.G; t += blockDim.x) { go.region_scores[t] = nan; go.region_word[t] = -1; }
        if (go.frame_scores)
            for (int t = threadIdx.x; t < go.frames; t += blockDim.x) go.frame_scores[t] = nan;
        return;
    }
    xf_pair_score<true>(a, smem, i, j, a.scores + o, go);
}

// resident CAPTION index, video-major pair list (the roles of xf_index_pairs_kernel swapped): workgroup (k, i) -> scores[i][k], caption
// cand[i K + k] of the index (a.Bj = its capacity), video i of the per-call workspace; an index outside [0, capacity) reads nothing and
// scores NaN
__global__ __launch_bounds__(512) void xf_caption_index_pairs_kernel(FusedArgs a) {
    extern __shared__ __attribute__((aligned(16))) char smem[];
    const int i = blockIdx.y;
    const int64_t o = (int64_t)i * a.K + blockIdx.x;
    const int j = a.cand[o];
    if (j < 0 || j >= a.Bj) {
        if (threadIdx.x == 0) a.scores[o] = __builtin_nanf("");
        return;
    }
    xf_pair_score<false>(a, smem, i, j, a.scores + o, GroundOut{});
}

// the same grid with grounding: `go` holds the bases of the [Bi][K][...] output arrays; pair o = i K + k writes row o of each.  An index
// outside [0, capacity) reads nothing: NaN in the float rows, -1 in the int rows.
__global__ __launch_bounds__(512) void xf_caption_index_pairs_ground_kernel(FusedArgs a, GroundOut go) {
    extern __shared__ __attribute__((aligned(16))) char smem[];
    const int i = blockIdx.y;
    const int64_t o = (int64_t)i * a.K + blockIdx.x;
    const int j = a.cand[o];
    go.word_scores += o * a.W; go.word_region += o * a.W; go.word_weight += o * a.W;
    go.region_scores += o * a.G; go.region_word += o * a.G;
    if (go.frame_scores) go.frame_scores += o * go.frames;
    if (j < 0 || j >= a.Bj) {
        const float nan = __builtin_nanf("");
        if (threadIdx.x == 0) a.scores[o] = nan;
        for (int t = threadIdx.x; t < a.W; t += blockDim.x) { go.word_scores[t] = nan; go.word_weight[t] = nan; go.word_region[t] = -1; }
        for (int t = threadIdx.x; t < a.G; t += blockDim.x) { go.region_scores[t] = nan; go.region_word[t] = -1; }
        if (go.frame_scores)
            for (int t = threadIdx.x; t < go.frames; t += blockDim.x) go.frame_scores[t] = nan;
        return;
    }
    xf_pair_score<true>(a, smem, i, j, a.scores + o, go);
}

// ------------------------------------------------------------------------------------------------------------------
// host side (called from dvlp_xattn_fwd / dvlp_xattn_bwd in xattn.hip)
// ------------------------------------------------------------------------------------------------------------------
static inline int64_t frup(int64_t a, int64_t m) { return (a + m - 1) / m * m; }

struct FusedLayout { int64_t Gr, Gk, Wp, Wk, off_chat, off_chatT, off_qhat, off_qhatT, off_nc, off_nq, total; };
static FusedLayout fused_layout(int64_t Bi, int64_t Bj, int64_t G, int64_t W) {
    FusedLayout F{};
    F.Gr = frup(G, 16); F.Gk = frup(G, 32); F.Wp = frup(W, 16); F.Wk = frup(W, 32);
    int64_t o = 0;
    auto take = [&](int64_t bytes) { int64_t r = o; o += frup(bytes, 256); return r; };
    F.off_chat = take(Bi * F.Gr * FD * 2); F.off_chatT = take(Bi * FD * F.Gk * 2);
    F.off_qhat = take(Bj * F.Wp * FD * 2); F.off_qhatT = take(Bj * FD * F.Wk * 2);
    F.off_nc = take(Bi * G * 4); F.off_nq = take(Bj * W * 4);
    F.total = o;
    return F;
}

static int g_xf_stop = 0;
DVLP_DEV_API int dvlp_dev_xfused_ablate(int stop) { g_xf_stop = stop; return 0; }

bool dvlp_xfused_ok(int64_t G, int64_t W) {
    if (G < 1 || W < 1 || W > 16 * FW_MAXB || G > 16 * 8 * FG_SLOTS) return false;
    const FLds L = flds((int)frup(G, 16), (int)frup(G, 32), (int)frup(W, 16), (int)frup(W, 32));
    return L.total <= 160 * 1024;
}
int64_t dvlp_xfused_workspace_bytes(int64_t Bi, int64_t Bj, int64_t G, int64_t W) { return fused_layout(Bi, Bj, G, W).total; }

// prep of the Bi videos and the Bj captions into the workspace; the kernel arguments of the pair kernels
static FusedArgs xf_prep(int64_t Bi, int64_t Bj, int64_t G, int64_t W, const void* Craw, const void* Qraw, const float* mimg, const float* mcap,
                         float lam, int gate, float* scores, void* workspace, hipStream_t st) {
    const FusedLayout F = fused_layout(Bi, Bj, G, W);
    char* ws = (char*)workspace;
    FusedArgs a{};
    a.chat = (const bf16*)(ws + F.off_chat); a.chatT = (const bf16*)(ws + F.off_chatT);
    a.qhat = (const bf16*)(ws + F.off_qhat); a.qhatT = (const bf16*)(ws + F.off_qhatT);
    a.nc = (const float*)(ws + F.off_nc); a.nq = (const float*)(ws + F.off_nq);
    a.mimg = mimg; a.mcap = mcap; a.scores = scores;
    a.Bi = (int)Bi; a.Bj = (int)Bj; a.G = (int)G; a.W = (int)W; a.Gr = (int)F.Gr; a.Gk = (int)F.Gk; a.Wp = (int)F.Wp; a.Wk = (int)F.Wk;
    a.lam = lam; a.gate = gate; a.stop = g_xf_stop;
    const int64_t rc = F.Gr > F.Gk ? F.Gr : F.Gk, rq = F.Wp > F.Wk ? F.Wp : F.Wk;
    hipLaunchKernelGGL(xf_prep_kernel, dim3((unsigned)cdiv(Bi * rc, 4)), dim3(256), 0, st, (int)Bi, (int)G, (int)F.Gr, (int)F.Gk, (const bf16*)Craw,
                       (bf16*)(ws + F.off_chat), (bf16*)(ws + F.off_chatT), (float*)(ws + F.off_nc));
    hipLaunchKernelGGL(xf_prep_kernel, dim3((unsigned)cdiv(Bj * rq, 4)), dim3(256), 0, st, (int)Bj, (int)W, (int)F.Wp, (int)F.Wk, (const bf16*)Qraw,
                       (bf16*)(ws + F.off_qhat), (bf16*)(ws + F.off_qhatT), (float*)(ws + F.off_nq));
    return a;
}

int dvlp_xfused_fwd(int64_t Bi, int64_t Bj, int64_t G, int64_t W, const void* Craw, const void* Qraw, const float* mimg, const float* mcap,
                    float lam, int gate, float* scores, void* workspace, hipStream_t st) {
    const FusedArgs a = xf_prep(Bi, Bj, G, W, Craw, Qraw, mimg, mcap, lam, gate, scores, workspace, st);
    const FLds L = flds(a.Gr, a.Gk, a.Wp, a.Wk);
    { static bool once = false; if (!once) { once = true;
        (void)hipFuncSetAttribute((const void*)xf_fwd_kernel, hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024); } }
    hipLaunchKernelGGL(xf_fwd_kernel, dim3((unsigned)Bj, (unsigned)Bi), dim3(512), (size_t)L.total, st, a);
    return 0;
}

// pair list (dvlp_xattn_pairs_fwd): the same prep over the Bi videos and the Bj pool captions, then one workgroup per (i, k)
int dvlp_xfused_pairs_fwd(int64_t Bi, int64_t Bj, int64_t K, int64_t G, int64_t W, const void* Craw, const void* Qraw, const float* mimg,
                          const float* mcap, const int* cand, float lam, int gate, float* scores, void* workspace, hipStream_t st) {
    FusedArgs a = xf_prep(Bi, Bj, G, W, Craw, Qraw, mimg, mcap, lam, gate, scores, workspace, st);
    a.cand = cand; a.K = (int)K;
    const FLds L = flds(a.Gr, a.Gk, a.Wp, a.Wk);
    { static bool once = false; if (!once) { once = true;
        (void)hipFuncSetAttribute((const void*)xf_pairs_fwd_kernel, hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024); } }
    hipLaunchKernelGGL(xf_pairs_fwd_kernel, dim3((unsigned)K, (unsigned)Bi), dim3(512), (size_t)L.total, st, a);
    return 0;
}

// ------------------------------------------------------------------------------------------------------------------
// resident video side (dvlp_xattn_index_*): the prepared form xf_prep writes per call -- chat [Gr][256], chatT [256][Gk] (bf16), nc [G]
// (fp32) per video -- in caller-owned memory for `capacity` videos, filled `n` rows at a time by the same prep kernel (a row's bytes do not
// depend on which call wrote it); a query call then preps its Bj captions only.
// ------------------------------------------------------------------------------------------------------------------
struct IndexLayout { int64_t Gr, Gk, off_chat, off_chatT, off_nc, total; };
static IndexLayout index_layout(int64_t capacity, int64_t G) {
    IndexLayout I{};
    I.Gr = frup(G, 16); I.Gk = frup(G, 32);
    I.off_chat = 0;
    I.off_chatT = frup(capacity * I.Gr * FD * 2, 256);
    I.off_nc = I.off_chatT + frup(capacity * FD * I.Gk * 2, 256);
    I.total = I.off_nc + frup(capacity * G * 4, 256);
    return I;
}
struct QueryLayout { int64_t Wp, Wk, off_qhat, off_qhatT, off_nq, total; };
static QueryLayout query_layout(int64_t Bj, int64_t W) {
    QueryLayout Q{};
    Q.Wp = frup(W, 16); Q.Wk = frup(W, 32);
    Q.off_qhat = 0;
    Q.off_qhatT = frup(Bj * Q.Wp * FD * 2, 256);
    Q.off_nq = Q.off_qhatT + frup(Bj * FD * Q.Wk * 2, 256);
    Q.total = Q.off_nq + frup(Bj * W * 4, 256);
    return Q;
}

int64_t dvlp_xfused_index_bytes(int64_t capacity, int64_t G) { return index_layout(capacity, G).total; }
int64_t dvlp_xfused_query_bytes(int64_t Bj, int64_t W) { return query_layout(Bj, W).total; }

int dvlp_xfused_index_add(int64_t capacity, int64_t G, int64_t row0, int64_t n, const void* Craw, void* index, hipStream_t st) {
    const IndexLayout I = index_layout(capacity, G);
    char* ix = (char*)index;
    const int64_t rc = I.Gr > I.Gk ? I.Gr : I.Gk;
    hipLaunchKernelGGL(xf_prep_kernel, dim3((unsigned)cdiv(n * rc, 4)), dim3(256), 0, st, (int)n, (int)G, (int)I.Gr, (int)I.Gk, (const bf16*)Craw,
                       (bf16*)(ix + I.off_chat) + row0 * I.Gr * FD, (bf16*)(ix + I.off_chatT) + row0 * FD * I.Gk, (float*)(ix + I.off_nc) + row0 * G);
    return 0;
}

// prep of the Bj captions into the workspace; the kernel arguments of the index pair kernels
static FusedArgs xf_index_prep(int64_t capacity, int64_t G, const void* index, const float* mimg, int64_t Bj, int64_t W, const void* Qraw,
                               const float* mcap, int64_t K, const int* cand, float lam, int gate, float* scores, void* workspace, hipStream_t st) {
    const IndexLayout I = index_layout(capacity, G);
    const QueryLayout Q = query_layout(Bj, W);
    const char* ix = (const char*)index;
    char* ws = (char*)workspace;
    FusedArgs a{};
    a.chat = (const bf16*)(ix + I.off_chat); a.chatT = (const bf16*)(ix + I.off_chatT); a.nc = (const float*)(ix + I.off_nc);
    a.qhat = (const bf16*)(ws + Q.off_qhat); a.qhatT = (const bf16*)(ws + Q.off_qhatT); a.nq = (const float*)(ws + Q.off_nq);
    a.mimg = mimg; a.mcap = mcap; a.scores = scores; a.cand = cand; a.K = (int)K;
    a.Bi = (int)capacity; a.Bj = (int)Bj; a.G = (int)G; a.W = (int)W; a.Gr = (int)I.Gr; a.Gk = (int)I.Gk; a.Wp = (int)Q.Wp; a.Wk = (int)Q.Wk;
    a.lam = lam; a.gate = gate; a.stop = g_xf_stop;
    const int64_t rq = Q.Wp > Q.Wk ? Q.Wp : Q.Wk;
    hipLaunchKernelGGL(xf_prep_kernel, dim3((unsigned)cdiv(Bj * rq, 4)), dim3(256), 0, st, (int)Bj, (int)W, (int)Q.Wp, (int)Q.Wk, (const bf16*)Qraw,
                       (bf16*)(ws + Q.off_qhat), (bf16*)(ws + Q.off_qhatT), (float*)(ws + Q.off_nq));
    return a;
}

int dvlp_xfused_index_pairs_fwd(int64_t capacity, int64_t G, const void* index, const float* mimg, int64_t Bj, int64_t W, const void* Qraw,
                                const float* mcap, int64_t K, const int* cand, float lam, int gate, float* scores, void* workspace, hipStream_t st) {
    const FusedArgs a = xf_index_prep(capacity, G, index, mimg, Bj, W, Qraw, mcap, K, cand, lam, gate, scores, workspace, st);
    const FLds L = flds(a.Gr, a.Gk, a.Wp, a.Wk);
    { static bool once = false; if (!once) { once = true;
        (void)hipFuncSetAttribute((const void*)xf_index_pairs_kernel, hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024); } }
    hipLaunchKernelGGL(xf_index_pairs_kernel, dim3((unsigned)K, (unsigned)Bj), dim3(512), (size_t)L.total, st, a);
    return 0;
}

// grounding of the same pairs (dvlp_xattn_index_pairs_ground): the same prep and grid; no ablation switch reaches it
int dvlp_xfused_index_pairs_ground(int64_t capacity, int64_t G, const void* index, const float* mimg, int64_t Bj, int64_t W, const void* Qraw,
                                   const float* mcap, int64_t K, const int* cand, int frames, float lam, int gate, float* scores, float* word_scores,
                                   float* region_scores, int* word_region, float* word_weight, int* region_word, float* frame_scores,
                                   void* workspace, hipStream_t st) {
    FusedArgs a = xf_index_prep(capacity, G, index, mimg, Bj, W, Qraw, mcap, K, cand, lam, gate, scores, workspace, st);
    a.stop = 0;
    GroundOut go{};
    go.word_scores = word_scores; go.region_scores = region_scores; go.word_region = word_region; go.region_word = region_word;
    go.word_weight = word_weight; go.frame_scores = frame_scores; go.frames = frames;
    const FLds L = flds(a.Gr, a.Gk, a.Wp, a.Wk);
    { static bool once = false; if (!once) { once = true;
        (void)hipFuncSetAttribute((const void*)xf_index_pairs_ground_kernel, hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024); } }
    hipLaunchKernelGGL(xf_index_pairs_ground_kernel, dim3((unsigned)K, (unsigned)Bj), dim3(512), (size_t)L.total, st, a, go);
    return 0;
}

// ------------------------------------------------------------------------------------------------------------------
// resident caption side (dvlp_xattn_caption_index_*): the roles of the family above swapped.  Per caption the index holds what xf_prep
// writes per call -- qhat [Wp][256], qhatT [256][Wk] (bf16), nq [W] (fp32) -- for `capacity` captions of W words, filled `n` rows at a
// time by the same prep kernel; a query call then preps its Bi videos only (chat, chatT, nc: the sections of IndexLayout at capacity Bi).
// ------------------------------------------------------------------------------------------------------------------
int64_t dvlp_xfused_caption_index_bytes(int64_t capacity, int64_t W) { return query_layout(capacity, W).total; }
int64_t dvlp_xfused_video_query_bytes(int64_t Bi, int64_t G) { return index_layout(Bi, G).total; }

int dvlp_xfused_caption_index_add(int64_t capacity, int64_t W, int64_t row0, int64_t n, const void* Qraw, void* index, hipStream_t st) {
    const QueryLayout Q = query_layout(capacity, W);
    char* ix = (char*)index;
    const int64_t rq = Q.Wp > Q.Wk ? Q.Wp : Q.Wk;
    hipLaunchKernelGGL(xf_prep_kernel, dim3((unsigned)cdiv(n * rq, 4)), dim3(256), 0, st, (int)n, (int)W, (int)Q.Wp, (int)Q.Wk, (const bf16*)Qraw,
                       (bf16*)(ix + Q.off_qhat) + row0 * Q.Wp * FD, (bf16*)(ix + Q.off_qhatT) + row0 * FD * Q.Wk, (float*)(ix + Q.off_nq) + row0 * W);
    return 0;
}

// prep of the Bi videos into the workspace; the kernel arguments of the caption-index pair kernels
static FusedArgs xf_caption_index_prep(int64_t capacity, int64_t W, const void* index, const float* mcap, int64_t Bi, int64_t G, const void* Craw,
                                       const float* mimg, int64_t K, const int* cand, float lam, int gate, float* scores, void* workspace,
                                       hipStream_t st) {
    const QueryLayout Q = query_layout(capacity, W);
    const IndexLayout I = index_layout(Bi, G);
    const char* ix = (const char*)index;
    char* ws = (char*)workspace;
    FusedArgs a{};
    a.qhat = (const bf16*)(ix + Q.off_qhat); a.qhatT = (const bf16*)(ix + Q.off_qhatT); a.nq = (const float*)(ix + Q.off_nq);
    a.chat = (const bf16*)(ws + I.off_chat); a.chatT = (const bf16*)(ws + I.off_chatT); a.nc = (const float*)(ws + I.off_nc);
    a.mimg = mimg; a.mcap = mcap; a.scores = scores; a.cand = cand; a.K = (int)K;
    a.Bi = (int)Bi; a.Bj = (int)capacity; a.G = (int)G; a.W = (int)W; a.Gr = (int)I.Gr; a.Gk = (int)I.Gk; a.Wp = (int)Q.Wp; a.Wk = (int)Q.Wk;
    a.lam = lam; a.gate = gate; a.stop = g_xf_stop;
    const int64_t rc = I.Gr > I.Gk ? I.Gr : I.Gk;
    hipLaunchKernelGGL(xf_prep_kernel, dim3((unsigned)cdiv(Bi * rc, 4)), dim3(256), 0, st, (int)Bi, (int)G, (int)I.Gr, (int)I.Gk, (const bf16*)Craw,
                       (bf16*)(ws + I.off_chat), (bf16*)(ws + I.off_chatT), (float*)(ws + I.off_nc));
    return a;
}

int dvlp_xfused_caption_index_pairs_fwd(int64_t capacity, int64_t W, const void* index, const float* mcap, int64_t Bi, int64_t G, const void* Craw,
                                        const float* mimg, int64_t K, const int* cand, float lam, int gate, float* scores, void* workspace,
                                        hipStream_t st) {
    const FusedArgs a = xf_caption_index_prep(capacity, W, index, mcap, Bi, G, Craw, mimg, K, cand, lam, gate, scores, workspace, st);
    const FLds L = flds(a.Gr, a.Gk, a.Wp, a.Wk);
    { static bool once = false; if (!once) { once = true;
        (void)hipFuncSetAttribute((const void*)xf_caption_index_pairs_kernel, hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024); } }
    hipLaunchKernelGGL(xf_caption_index_pairs_kernel, dim3((unsigned)K, (unsigned)Bi), dim3(512), (size_t)L.total, st, a);
    return 0;
}

// grounding of the same pairs (dvlp_xattn_caption_index_pairs_ground): the same prep and grid; no ablation switch reaches it
int dvlp_xfused_caption_index_pairs_ground(int64_t capacity, int64_t W, const void* index, const float* mcap, int64_t Bi, int64_t G,
                                           const void* Craw, const float* mimg, int64_t K, const int* cand, int frames, float lam, int gate,
                                           float* scores, float* word_scores, float* region_scores, int* word_region, float* word_weight,
                                           int* region_word, float* frame_scores, void* workspace, hipStream_t st) {
    FusedArgs a = xf_caption_index_prep(capacity, W, index, mcap, Bi, G, Craw, mimg, K, cand, lam, gate, scores, workspace, st);
    a.stop = 0;
    GroundOut go{};
    go.word_scores = word_scores; go.region_scores = region_scores; go.word_region = word_region; go.region_word = region_word;
    go.word_weight = word_weight; go.frame_scores = frame_scores; go.frames = frames;
    const FLds L = flds(a.Gr, a.Gk, a.Wp, a.Wk);
    { static bool once = false; if (!once) { once = true;
        (void)hipFuncSetAttribute((const void*)xf_caption_index_pairs_ground_kernel, hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024); } }
    hipLaunchKernelGGL(xf_caption_index_pairs_ground_kernel, dim3((unsigned)K, (unsigned)Bi), dim3(512), (size_t)L.total, st, a, go);
    return 0;
}

// ------------------------------------------------------------------------------------------------------------------
// Region-tiled pair kernel (dvlp_xattn_long_index_*): the pair score above for long videos, 1 <= G <= 1152 regions and
// W <= 112 words, bf16.  The fused kernel keeps P1' [W][G] and P2' [G][W] resident, which is what stops it at G = 288; the score splits
// along the region axis, so here one workgroup per pair walks the regions in tiles of 128 (one 16-row block per wave) twice, recomputing
// S = LeakyReLU(C^ Q^T) per tile with Q^ staged once:
//
//   sweep 1   per tile: S, its row norms (region-local), and into per-lane accumulators the column sums of squares (-> cn[w]) and
//             cs[w] = sum_g e, e = exp(lam (S rn + m_img - 1)) rounded to bf16.  No running maximum: z <= lam (see pair_forward).
//   sweep 2   per tile, on the recomputed S (same code, same operands: same bits):
//             image -> text   the gate is a per-word threshold on e; the gated, UNNORMALISED numerators go to LDS as bf16 [w][128] and
//                             feed wc^T += C^^T_tile P1u_tile^T, accumulated in registers over all tiles (waves own 32-channel slices);
//                             gs[w] = sum_g H e and gd[w] = sum_g H e S_pre accumulate beside it.  The per-word scale 1 / gs is applied
//                             once at the end (to the accumulators, before they are squared).
//             text -> image   tile-local throughout: softmax over words, gate, renormalise, P2' tile [128][w] to LDS, wc2 product,
//                             |wc2_g|^2, cos(C_g, wc2_g) -> rc[g].
//   end       |wc_w|^2, the word cosines, and the sum of all cosines in a fixed order.
//
// The cosines use <raw, ctx> = (|raw| + eps) sum P' S_pre as above.  No float atomics; every cross-wave sum is taken in wave order, so
// the result does not depend on scheduling.  Pad rows / columns are zeros in the operands and -1e4 in the masks, as in pair_forward.
//
// GROUND adds the rows of dvlp_xattn_index_pairs_ground: word_region is a running "larger logit, then smaller index" key per lane and word,
// carried across the tiles (with the gated numerator at that entry beside it); region_word / region_scores are tile-local; word_scores come
// at the end.  word_region_weight = gated numerator (the bf16 value the kernel multiplies with) / gated sum, in fp32 -- the fused kernel
// reports the bf16-rounded quotient instead, because that is what IT multiplies with.
//
// The score of the GROUND instantiation equals the other's bit for bit: floating-point contraction is switched off for everything below
// (a fused multiply-add appears only where fmaf is written), no fast-math reassociation is in force, and GROUND touches no operand of the
// arithmetic that ends in the score.
// ------------------------------------------------------------------------------------------------------------------
#pragma clang fp contract(off)

constexpr int LT = 128;              // regions per tile: one 16-row block per wave
constexpr int LPS = LT + 8;          // row stride (elements) of the P1u tile [w][128] and of the P2' tile [128][Wk <= 128]
constexpr int LG_MAX = 1152;         // 32 frames x 36 regions
// LDS map (bytes; fixed, whatever the shape)
constexpr int LL_QS = 0;                                    // Q^ [Wp][FQS] bf16, staged once                       59 136
constexpr int LL_P1 = LL_QS + 16 * FW_MAXB * FQS * 2;       // P1u tile [Wp][LPS] bf16                              30 464
constexpr int LL_P2 = LL_P1 + 16 * FW_MAXB * LPS * 2;       // P2' tile [LT][LPS] bf16 (GROUND, at the end: weights) 34 816
constexpr int LL_XA = LL_P2 + LT * LPS * 2;                 // four cross-wave exchanges [8][112] fp32               4 x 3 584
constexpr int LL_XB = LL_XA + 8 * 112 * 4;                  //   (GROUND, at the end: xa + xb hold the keys [8][112] u64)
constexpr int LL_XC = LL_XB + 8 * 112 * 4;
constexpr int LL_XD = LL_XC + 8 * 112 * 4;
constexpr int LL_NW2P = LL_XD + 8 * 112 * 4;                // per-wave partials of |wc2_g|^2 [8][LT] (at the end: of |wc_w|^2)  4 096
constexpr int LL_DOTG = LL_NW2P + 8 * LT * 4;               // sum_w P2' S_pre per region [1152]                     4 608
constexpr int LL_RC = LL_DOTG + LG_MAX * 4;                 // region cosines [1152]                                 4 608
constexpr int LL_DOTW = LL_RC + LG_MAX * 4;                 // sum_g P1' S_pre per word [112]                          448
constexpr int LL_GINV = LL_DOTW + 112 * 4;                  // 1 / gated sum per word [112]                            448
constexpr int LL_RED = LL_GINV + 112 * 4;                   // the eight waves' shares of the score                     32
constexpr int LL_TOTAL = LL_RED + 8 * 4;                    // 152 992
static_assert(LL_TOTAL <= 160 * 1024 && LL_XA % 8 == 0 && 8 * 112 * 4 <= LT * LPS * 2 && 8 * 112 * 4 <= 8 * LT * 4, "LDS map of the tiled kernel");

// S of region block rb (16 rows) against all words, with what is local to its rows
struct TileRegs {
    f32x4 S[FW_MAXB];      // LeakyReLU(S_pre); zeros for a block past the video and for pad words
    float rn[4];           // 1 / (|S_row| + eps)
    float k1[4], mi[4];    // exponent scale lam log2(e) rn and offset lam log2(e) (m_img - 1); m_img = -1e4 for pad rows
    float mraw[4];         // m_img (0 for pad rows)
    bool okg[4];           // a region of the video
};
// RANGE (moments): the video side is the regions [g0, g1) only.  Blocks are still the video's own (absolute) 16-row blocks, so every
// operand keeps its alignment; a row outside the range is a neighbouring frame's, not zeros, and its S is forced to zero here -- from there
// on it behaves like a pad row (e = 0, nothing in the column sums, zeros in the P1u tile).
template <bool RANGE>
__device__ __forceinline__ void xl_tile_s(const FusedArgs& a, const bf16* ch, const float* mimg, const bf16* Qs, int rb, int g0, int g1, float L2E,
                                          TileRegs& T) {
    const int lane = threadIdx.x & 63, lq = lane >> 4, lc = lane & 15;
    const int nbg = a.Gr >> 4, nwb = a.Wp >> 4;
    const bool live = RANGE ? rb * 16 < g1 && rb * 16 + 16 > g0 : rb < nbg;      // wave-uniform
    bf16x8 af[8];
    const bf16* ap = ch + (int64_t)((live ? rb : 0) * 16 + lc) * FD + 8 * lq;
#pragma unroll
    for (int ks = 0; ks < 8; ++ks) af[ks] = *(const bf16x8*)(ap + ks * 32);
#pragma unroll
    for (int r = 0; r < 4; ++r) {
        const int g = rb * 16 + lq * 4 + r;
        T.okg[r] = RANGE ? live && g >= g0 && g < g1 : live && g < a.G;
        T.mraw[r] = T.okg[r] ? mimg[g] : 0.f;
    }
#pragma unroll
    for (int nb = 0; nb < FW_MAXB; ++nb) {
        f32x4 c = (f32x4){0.f, 0.f, 0.f, 0.f};
        if (live && nb < nwb) {
            const bf16* bp = Qs + (nb * 16 + lc) * FQS + 8 * lq;
#pragma unroll
            for (int ks = 0; ks < 8; ++ks) c = mfma16(af[ks], *(const bf16x8*)(bp + ks * 32), c);
#pragma unroll
            for (int r = 0; r < 4; ++r) c[r] = fmaxf(c[r], 0.1f * c[r]);             // LeakyReLU(0.1), loss.py:236
            if constexpr (RANGE) {
#pragma unroll
                for (int r = 0; r < 4; ++r) c[r] = T.okg[r] ? c[r] : 0.f;
            }
        }
        T.S[nb] = c;
    }
#pragma unroll
    for (int r = 0; r < 4; ++r) {
        float q = 0.f;
#pragma unroll
        for (int nb = 0; nb < FW_MAXB; ++nb) q = fmaf(T.S[nb][r], T.S[nb][r], q);
        T.rn[r] = 1.f / (sqrtf(row16_sum(q)) + 1e-8f);
        T.k1[r] = L2E * T.rn[r];
        T.mi[r] = L2E * ((T.okg[r] ? T.mraw[r] : -1e4f) - 1.f);
    }
}

// Q^_j [Wp][256] -> LDS, kept for the whole pair; the k padding of the P2' tile (words Wp .. Wk-1) is zeroed once.  Published by the first
// barrier of xl_pair_score.
__device__ __forceinline__ void xl_stage_q(const FusedArgs& a, char* smem, int j) {
    const int tid = threadIdx.x;
    bf16* Qs = (bf16*)(smem + LL_QS);
    bf16* P2s = (bf16*)(smem + LL_P2);
    const bf16* q = a.qhat + (int64_t)j * a.Wp * FD;
    for (int p = tid; p < a.Wp * 32; p += blockDim.x) {
        const int r = p >> 5, c = (p & 31) * 8;
        *(bf16x8*)(Qs + r * FQS + c) = *(const bf16x8*)(q + r * FD + c);
    }
    if (a.Wk > a.Wp)
        for (int p = tid; p < LT * (a.Wk - a.Wp); p += blockDim.x) P2s[(p / (a.Wk - a.Wp)) * LPS + a.Wp + p % (a.Wk - a.Wp)] = (bf16)0.f;
}

// STAGED (xl_caption_index_moments_kernel): the caller has run xl_stage_q for caption j and calls this once per window of its
// chunk.  Nothing else differs: the barrier below publishes the staging for the first window and, for every later one, separates the
// previous window's last LDS reads (thread 0: red and the flags in xa) from this window's first writes.  What a window reads of LDS it has
// written itself -- the P1u / P2' tiles whole per tile (a block outside the range writes zeros), the exchange slots, nw2p, dotw, ginv, red
// whole, dotg / rc at the regions of its own range -- except Q^ and the k padding of the P2' tile, which no window writes.
template <bool GROUND, bool RANGE = false, bool STAGED = false>
__device__ __forceinline__ void xl_pair_score(const FusedArgs& a, char* smem, int i, int j, float* out, const GroundOut& go, int g0 = 0, int g1 = 0) {
    const int tid = threadIdx.x, lane = tid & 63, lq = lane >> 4, lc = lane & 15;
    const int wid = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int nbg = a.Gr >> 4, nwb = a.Wp >> 4, nks2 = a.Wk >> 5;
    const int t0 = RANGE ? g0 / LT : 0, nt = RANGE ? (g1 - 1) / LT + 1 : (nbg + 7) >> 3;        // the tiles [t0, nt) hold the regions scored
    bf16* Qs = (bf16*)(smem + LL_QS);
    bf16* P1s = (bf16*)(smem + LL_P1);
    bf16* P2s = (bf16*)(smem + LL_P2);
    float *xa = (float*)(smem + LL_XA), *xb = (float*)(smem + LL_XB), *xc = (float*)(smem + LL_XC), *xd = (float*)(smem + LL_XD);
    float *nw2p = (float*)(smem + LL_NW2P), *dotg = (float*)(smem + LL_DOTG), *rc = (float*)(smem + LL_RC);
    float *dotw = (float*)(smem + LL_DOTW), *ginv = (float*)(smem + LL_GINV), *red = (float*)(smem + LL_RED);
    const bf16* ch = a.chat + (int64_t)i * a.Gr * FD;
    const bf16* ct = a.chatT + ((int64_t)i * FD + wid * 32 + lc) * a.Gk + 8 * lq;      // this wave's 32 channels of C^^T
    const bf16* qt = a.qhatT + ((int64_t)j * FD + wid * 32 + lc) * a.Wk + 8 * lq;      // ... and of Q^^T
    const float* mimg = a.mimg + (int64_t)i * a.G;
    const float* mcap = a.mcap + (int64_t)j * a.W;
    const float* nc = a.nc + (int64_t)i * a.G;
    const float L2E = 1.4426950408889634f * a.lam;        // exp(lam x) = exp2(L2E x)
    const float fG = RANGE ? (float)(g1 - g0) : (float)a.G, fW = (float)a.W;

    if constexpr (!STAGED) xl_stage_q(a, smem, j);
    float mc[FW_MAXB], mcraw[FW_MAXB];       // exponent offset lam log2(e) (m_cap - 1), m_cap = -1e4 for pad columns; m_cap itself
    bool okw[FW_MAXB];
#pragma unroll
    for (int nb = 0; nb < FW_MAXB; ++nb) {
        const int w = nb * 16 + lc;
        okw[nb] = nb < nwb && w < a.W;
        mcraw[nb] = okw[nb] ? mcap[w] : 0.f;
        mc[nb] = L2E * ((okw[nb] ? mcraw[nb] : -1e4f) - 1.f);
    }
    __syncthreads();

    // ---- sweep 1: column sums of squares of S and cs[w] = sum_g e
    float csq[FW_MAXB], cs[FW_MAXB];
#pragma unroll
    for (int nb = 0; nb < FW_MAXB; ++nb) { csq[nb] = 0.f; cs[nb] = 0.f; }
    for (int t = t0; t < nt; ++t) {
        TileRegs T;
        xl_tile_s<RANGE>(a, ch, mimg, Qs, t * 8 + wid, g0, g1, L2E, T);
#pragma unroll
        for (int nb = 0; nb < FW_MAXB; ++nb) {
#pragma unroll
            for (int r = 0; r < 4; ++r) csq[nb] = fmaf(T.S[nb][r], T.S[nb][r], csq[nb]);
#pragma unroll
            for (int h = 0; h < 2; ++h) {
                const unsigned u = pk2(__builtin_amdgcn_exp2f(fmaf(T.S[nb][2 * h], T.k1[2 * h], T.mi[2 * h])),
                                       __builtin_amdgcn_exp2f(fmaf(T.S[nb][2 * h + 1], T.k1[2 * h + 1], T.mi[2 * h + 1])));
                cs[nb] += pk_lo(u) + pk_hi(u);
            }
        }
    }
#pragma unroll
    for (int nb = 0; nb < FW_MAXB; ++nb) { csq[nb] = col4_sum(csq[nb]); cs[nb] = col4_sum(cs[nb]); }
    xch_put(xa, wid, lane, csq, nwb);
    xch_put(xb, wid, lane, cs, nwb);
    __syncthreads();
    xch_get(xa, lane, csq, nwb);
    xch_get(xb, lane, cs, nwb);
    // text -> image exponent scale lam log2(e) / (|S_col| + eps); focal gate of image -> text as a per-word threshold on e (see pair_forward)
    float cn[FW_MAXB], kc[FW_MAXB], thr[FW_MAXB], gs[FW_MAXB], gd[FW_MAXB];
#pragma unroll
    for (int nb = 0; nb < FW_MAXB; ++nb) {
        cn[nb] = 1.f / (sqrtf(csq[nb]) + 1e-8f);
        kc[nb] = L2E * cn[nb];
        const float inv = cs[nb] > 0.f ? 1.f / cs[nb] : 0.f;
        thr[nb] = a.gate ? (cs[nb] * inv) / (inv * fG) : -1.f;
        gs[nb] = 0.f; gd[nb] = 0.f;
    }

    // ---- sweep 2
    f32x4 acc[2][FW_MAXB];               // wc^T [d][w] times the gated sum: channels 32 wid + 16 db + 4 lq + r, word 16 nb + lc
#pragma unroll
    for (int db = 0; db < 2; ++db)
#pragma unroll
        for (int nb = 0; nb < FW_MAXB; ++nb) acc[db][nb] = (f32x4){0.f, 0.f, 0.f, 0.f};
    u64 kw[FW_MAXB];                     // GROUND: best image->text key of this lane's rows so far, per word, and the gated numerator there
    float ew[FW_MAXB];
#pragma unroll
    for (int nb = 0; nb < FW_MAXB; ++nb) { kw[nb] = 0ull; ew[nb] = 0.f; }

    for (int t = t0; t < nt; ++t) {
        const int rb = t * 8 + wid, row0 = wid * 16 + lq * 4;       // this lane's four rows of the tile: row0 .. row0 + 3
        TileRegs T;
        xl_tile_s<RANGE>(a, ch, mimg, Qs, rb, g0, g1, L2E, T);
        // image -> text: gated numerators of this block -> P1u tile [w][row], four consecutive regions per 8-byte write
#pragma unroll
        for (int nb = 0; nb < FW_MAXB; ++nb) {
            unsigned v[2];
#pragma unroll
            for (int h = 0; h < 2; ++h) {
                const unsigned u = pk2(__builtin_amdgcn_exp2f(fmaf(T.S[nb][2 * h], T.k1[2 * h], T.mi[2 * h])),
                                       __builtin_amdgcn_exp2f(fmaf(T.S[nb][2 * h + 1], T.k1[2 * h + 1], T.mi[2 * h + 1])));
                const unsigned keep = (pk_lo(u) > thr[nb] ? 0x0000ffffu : 0u) | (pk_hi(u) > thr[nb] ? 0xffff0000u : 0u);
                v[h] = u & keep;
                const float s0 = T.S[nb][2 * h], s1 = T.S[nb][2 * h + 1];
                gs[nb] += pk_lo(v[h]) + pk_hi(v[h]);
                gd[nb] = fmaf(pk_lo(v[h]), fminf(s0, 10.f * s0), fmaf(pk_hi(v[h]), fminf(s1, 10.f * s1), gd[nb]));     // S_pre: undo LeakyReLU(0.1)
            }
            if (nb < nwb) *(uint2*)(P1s + (nb * 16 + lc) * LPS + row0) = make_uint2(v[0], v[1]);
            if constexpr (GROUND) {
#pragma unroll
                for (int r = 0; r < 4; ++r) {
                    const u64 k = gr_key(gr_logit(a.lam, T.S[nb][r], T.rn[r], T.mraw[r]), rb * 16 + lq * 4 + r);       // lam (A[g][w] + m_img[g])
                    if (T.okg[r] && k > kw[nb]) { kw[nb] = k; ew[nb] = (r & 1) ? pk_hi(v[r >> 1]) : pk_lo(v[r >> 1]); }
                }
            }
            __builtin_amdgcn_sched_barrier(0);            // keep the unrolled word blocks from being interleaved (register pressure)
        }
        // text -> image: softmax over words of lam (S cn + m_cap) per region, gate, renormalise -> P2' tile [row][w]
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            float e[FW_MAXB], sum = 0.f;
#pragma unroll
            for (int nb = 0; nb < FW_MAXB; ++nb) {
                e[nb] = __builtin_amdgcn_exp2f(fmaf(T.S[nb][r], kc[nb], mc[nb]));
                sum += e[nb];
            }
            sum = row16_sum(sum);
            const float inv = sum > 0.f ? 1.f / sum : 0.f;
            const float th = a.gate ? (sum * inv) / (inv * fW) : -1.f;
            float g1 = 0.f, g2 = 0.f;
#pragma unroll
            for (int nb = 0; nb < FW_MAXB; ++nb) {
                const float sv = T.S[nb][r];
                e[nb] = e[nb] > th ? e[nb] : 0.f;
                g1 += e[nb]; g2 = fmaf(e[nb], fminf(sv, 10.f * sv), g2);
            }
            g1 = row16_sum(g1); g2 = row16_sum(g2);
            const float is = g1 > 0.f ? 1.f / g1 : 0.f;
#pragma unroll
            for (int nb = 0; nb < FW_MAXB; ++nb)
                if (nb < nwb) P2s[(row0 + r) * LPS + nb * 16 + lc] = (bf16)(e[nb] * is);
            const int g = rb * 16 + lq * 4 + r;
            if (rb < nbg && lc == 0) dotg[g] = g2 * is;
            if constexpr (GROUND) {
                u64 kg = 0ull;
#pragma unroll
                for (int nb = 0; nb < FW_MAXB; ++nb)
                    if (okw[nb]) kg = gr_max(kg, gr_key(gr_logit(a.lam, T.S[nb][r], cn[nb], mcraw[nb]), nb * 16 + lc));  // lam (A2[g][w] + m_cap[w])
                kg = gr_row16_max(kg);
                if (T.okg[r] && lc == 0) go.region_word[g] = gr_index(kg);
            }
            __builtin_amdgcn_sched_barrier(0);
        }
        __syncthreads();                                   // both tiles are published
        // A operands of the two products: this tile's (at most four) 32-region steps of C^^T, and Q^^T (L2 hits after the first tile);
        // requested after the barrier: 64 registers that the softmax passes above have no room for
        const int k0 = t * LT;
        const int nks1 = (a.Gk - k0) >> 5 < 4 ? (a.Gk - k0) >> 5 : 4;
        // RANGE: a 32-region step wholly outside [g0, g1) has zeros in the P1u tile and is skipped (g1 <= Gk: a step inside is below nks1)
        const auto ks1 = [&](int ks) {
            if constexpr (RANGE) return k0 + ks * 32 < g1 && k0 + ks * 32 + 32 > g0;
            else return ks < nks1;
        };
        bf16x8 ca[2][4], qa[2][4];
#pragma unroll
        for (int ks = 0; ks < 4; ++ks) {
            const int k = ks1(ks) ? k0 + ks * 32 : 0;
            ca[0][ks] = *(const bf16x8*)(ct + k); ca[1][ks] = *(const bf16x8*)(ct + (int64_t)16 * a.Gk + k);
            const int kq = ks < nks2 ? ks * 32 : 0;
            qa[0][ks] = *(const bf16x8*)(qt + kq); qa[1][ks] = *(const bf16x8*)(qt + (int64_t)16 * a.Wk + kq);
        }
        // wc^T += C^^T_tile P1u_tile^T
#pragma unroll
        for (int ks = 0; ks < 4; ++ks) {
            if (ks1(ks)) {
#pragma unroll
                for (int nb = 0; nb < FW_MAXB; ++nb) {
                    if (nb < nwb) {
                        const bf16x8 b = *(const bf16x8*)(P1s + (nb * 16 + lc) * LPS + ks * 32 + 8 * lq);
                        acc[0][nb] = mfma16(ca[0][ks], b, acc[0][nb]);
                        acc[1][nb] = mfma16(ca[1][ks], b, acc[1][nb]);
                    }
                }
            }
        }
        // |wc2_g|^2 of the tile's regions: wc2^T [d][g] = Q^^T [d][w] P2'^T, per-wave partials over this wave's 32 channels
        for (int gb = 0; gb < 8 && t * 8 + gb < nbg; ++gb) {
            if constexpr (RANGE) {
                if ((t * 8 + gb) * 16 >= g1 || (t * 8 + gb) * 16 + 16 <= g0) continue;      // no region of the range in this block
            }
            f32x4 c0 = (f32x4){0.f, 0.f, 0.f, 0.f}, c1 = c0;
#pragma unroll
            for (int ks = 0; ks < 4; ++ks) {
                if (ks < nks2) {
                    const bf16x8 b = *(const bf16x8*)(P2s + (gb * 16 + lc) * LPS + ks * 32 + 8 * lq);
                    c0 = mfma16(qa[0][ks], b, c0); c1 = mfma16(qa[1][ks], b, c1);
                }
            }
            float q = 0.f;
#pragma unroll
            for (int r = 0; r < 4; ++r) q = fmaf(c0[r], c0[r], fmaf(c1[r], c1[r], q));
            q = col4_sum(q);
            if (lq == 0) nw2p[wid * LT + gb * 16 + lc] = q;
        }
        __syncthreads();                                   // the tiles are read; the partials are published
        // region cosines of the tile (loss.py:320-327), the eight partials summed in wave order
        if (tid < LT && (RANGE ? k0 + tid >= g0 && k0 + tid < g1 : k0 + tid < a.G)) {
            const int g = k0 + tid;
            float q = 0.f;
#pragma unroll
            for (int w = 0; w < 8; ++w) q += nw2p[w * LT + tid];
            const float n = nc[g];
            const float c = dotg[g] * (n + 1e-8f) / fmaxf(n * sqrtf(q), 1e-8f);
            rc[g] = c;
            if constexpr (GROUND) go.region_scores[g] = c;
        }
        // (the next tile writes P1u / P2' before its first barrier and nw2p after it; rc and dotg entries are written once)
    }

    // ---- end: gated sums over all regions, |wc_w|^2, the word cosines
#pragma unroll
    for (int nb = 0; nb < FW_MAXB; ++nb) { gs[nb] = col4_sum(gs[nb]); gd[nb] = col4_sum(gd[nb]); }
    xch_put(xc, wid, lane, gs, nwb);
    xch_put(xd, wid, lane, gd, nwb);
    if constexpr (GROUND) {
        // this wave's best key per word, and the numerator of the lane that holds it (keys of real entries are distinct)
        u64* keys = (u64*)(smem + LL_XA);
        float* wts = (float*)(smem + LL_P2);
#pragma unroll
        for (int nb = 0; nb < FW_MAXB; ++nb) {
            const u64 k = gr_col4_max(kw[nb]);
            if (nb < nwb) {
                if (lq == 0) keys[wid * 112 + nb * 16 + lc] = k;
                if (k != 0ull && kw[nb] == k) wts[wid * 112 + nb * 16 + lc] = ew[nb];
            }
        }
    }
    __syncthreads();
    xch_get(xc, lane, gs, nwb);
    xch_get(xd, lane, gd, nwb);
    float* nw1p = nw2p;                  // per-wave partials of |wc_w|^2 [8][112]
#pragma unroll
    for (int nb = 0; nb < FW_MAXB; ++nb) {
        const float is = gs[nb] > 0.f ? 1.f / gs[nb] : 0.f;          // P1' = H e / sum(H e): the scale the accumulators still lack
        if (wid == 0 && lq == 0 && nb < nwb) { dotw[nb * 16 + lc] = gd[nb] * is; ginv[nb * 16 + lc] = is; }
        float q = 0.f;
#pragma unroll
        for (int db = 0; db < 2; ++db)
#pragma unroll
            for (int r = 0; r < 4; ++r) { const float x = acc[db][nb][r] * is; q = fmaf(x, x, q); }
        q = col4_sum(q);
        if (nb < nwb && lq == 0) nw1p[wid * 112 + nb * 16 + lc] = q;
    }
    __syncthreads();
    // ---- cosines (loss.py:286-291, 317-327): means over ALL W words / G regions (padded ones included, as the reference)
    float part = 0.f;
    const float* nq = a.nq + (int64_t)j * a.W;
    for (int w = tid; w < a.W; w += blockDim.x) {
        float q = 0.f;
#pragma unroll
        for (int v = 0; v < 8; ++v) q += nw1p[v * 112 + w];
        const float n = nq[w];
        const float c = dotw[w] * (n + 1e-8f) / fmaxf(n * sqrtf(q), 1e-8f);
        part += c / fW;
        if constexpr (GROUND) {
            const u64* keys = (const u64*)(smem + LL_XA);
            const float* wts = (const float*)(smem + LL_P2);
            u64 k = 0ull;
            int best = 0;
#pragma unroll
            for (int v = 0; v < 8; ++v) { const u64 kv = keys[v * 112 + w]; if (kv > k) { k = kv; best = v; } }
            go.word_scores[w] = c;
            go.word_region[w] = gr_index(k);
            go.word_weight[w] = wts[best * 112 + w] * ginv[w];
        }
    }
    if constexpr (RANGE) {
        // the regions of the range (with g0 = 0, g1 = G: the loop below); a range without an unmasked region scores -inf, as an empty frame does
        bool seen = false;
        for (int g = g0 + tid; g < g1; g += blockDim.x) { part += rc[g] / fG; seen |= mimg[g] == 0.f; }
        const int wseen = __ballot(seen) != 0ull;           // by the whole wave: inside the lane-0 branch it would see lane 0 alone
        if (lane == 0) ((int*)xa)[wid] = wseen;
    } else {
        for (int g = tid; g < a.G; g += blockDim.x) part += rc[g] / fG;
    }
    part = wave_sum(part);
    if (lane == 0) red[wid] = part;
    __syncthreads();
    if (tid == 0) {
        float t = 0.f;
        for (int w = 0; w < 8; ++w) t += red[w];
        if constexpr (RANGE) {
            int any = 0;
            for (int w = 0; w < 8; ++w) any |= ((const int*)xa)[w];
            if (!any) t = -__builtin_inff();
        }
        *out = t;
    }
    if constexpr (GROUND) {
        // frame f: mean of the region cosines over its unmasked regions, summed in region order
        for (int f = tid; f < go.frames; f += blockDim.x) {
            if (!go.frame_scores) break;
            const int rf = a.G / go.frames;
            float t = 0.f;
            int n = 0;
            for (int g = f * rf; g < (f + 1) * rf; ++g)
                if (mimg[g] == 0.f) { t += rc[g]; ++n; }
            go.frame_scores[f] = n ? t / (float)n : -__builtin_inff();
        }
    }
}

// resident index, query-major pair list (the grid of xf_index_pairs_kernel): workgroup (k, j) -> scores[j][k], video cand[j K + k]
__global__ __launch_bounds__(512) void xl_index_pairs_kernel(FusedArgs a) {
    extern __shared__ __attribute__((aligned(16))) char smem[];
    const int j = blockIdx.y;
    const int64_t o = (int64_t)j * a.K + blockIdx.x;
    const int i = a.cand[o];
    if (i < 0 || i >= a.Bi) {
        if (threadIdx.x == 0) a.scores[o] = __builtin_nanf("");
        return;
    }
    xl_pair_score<false>(a, smem, i, j, a.scores + o, GroundOut{});
}

// the same grid with grounding; an index outside [0, capacity) reads nothing: NaN in the float rows, -1 in the int rows
__global__ __launch_bounds__(512) void xl_index_pairs_ground_kernel(FusedArgs a, GroundOut go) {
    extern __shared__ __attribute__((aligned(16))) char smem[];
    const int j = blockIdx.y;
    const int64_t o = (int64_t)j * a.K + blockIdx.x;
    const int i = a.cand[o];
    go.word_scores += o * a.W; go.word_region += o * a.W; go.word_weight += o * a.W;
    go.region_scores += o * a.G; go.region_word += o * a.G;
    if (go.frame_scores) go.frame_scores += o * go.frames;
    if (i < 0 || i >= a.Bi) {
        const float nan = __builtin_nanf("");
        if (threadIdx.x == 0) a.scores[o] = nan;
        for (int t = threadIdx.x; t < a.W; t += blockDim.x) { go.word_scores[t] = nan; go.word_weight[t] = nan; go.word_region[t] = -1; }
        for (int t = threadIdx.x; t < a.G; t += blockDim.x) { go.region_scores[t] = nan; go.region_word[t] = -1; }
        if (go.frame_scores)
            for (int t = threadIdx.x; t < go.frames; t += blockDim.x) go.frame_scores[t] = nan;
        return;
    }
    xl_pair_score<true>(a, smem, i, j, a.scores + o, go);
}

// moments: workgroup (k M + m, j) -> scores[j][k][m], the frames [m stride, m stride + win) of video cand[j K + k] as a video
// side of their own, read in place.  m is the fast grid axis: the windows of a pair run together and share its video in L2.
__global__ __launch_bounds__(512) void xl_index_moments_kernel(FusedArgs a, int R, int win, int stride, int M) {
    extern __shared__ __attribute__((aligned(16))) char smem[];
    const int j = blockIdx.y, k = blockIdx.x / M, m = blockIdx.x - k * M;
    const int64_t o = (int64_t)j * a.K + k;
    const int i = a.cand[o];
    float* out = a.scores + o * M + m;
    if (i < 0 || i >= a.Bi) {
        if (threadIdx.x == 0) *out = __builtin_nanf("");
        return;
    }
    const int g0 = m * stride * R;
    xl_pair_score<false, true>(a, smem, i, j, out, GroundOut{}, g0, g0 + win * R);
}

// resident CAPTION index, video-major pair list (the grid and hole rule of xf_caption_index_pairs_kernel, the body of xl_index_pairs_kernel):
// workgroup (k, i) -> scores[i][k], caption cand[i K + k] of the index (a.Bj = its capacity), video i of the per-call workspace.  k is the
// fast grid axis, so the workgroups in flight together share video i (1.18 MB at G = 1152) in L2 and stream one caption each.
__global__ __launch_bounds__(512) void xl_caption_index_pairs_kernel(FusedArgs a) {
    extern __shared__ __attribute__((aligned(16))) char smem[];
    const int i = blockIdx.y;
    const int64_t o = (int64_t)i * a.K + blockIdx.x;
    const int j = a.cand[o];
    if (j < 0 || j >= a.Bj) {
        if (threadIdx.x == 0) a.scores[o] = __builtin_nanf("");
        return;
    }
    xl_pair_score<false>(a, smem, i, j, a.scores + o, GroundOut{});
}

// moments of a query video against the resident captions: workgroup (k nch + c, i) -> the windows [c wpg, min(M, (c + 1) wpg))
// of the pair (video i, caption cand[i K + k]).  The caption is staged once and the windows of the chunk are scored in turn, each by the
// code of xl_index_moments_kernel (xl_pair_score<false, true>) on the regions [m stride R, (m stride + win) R) of video i in the per-call
// workspace.  scores[(i K + k) M + m], window-major: scores[(i M + m) K + k].  The chunks of a pair are neighbours on the fast grid axis and
// blockIdx.y is the video, so the workgroups in flight together share video i in L2, as in xl_caption_index_pairs_kernel.
__global__ __launch_bounds__(512) void xl_caption_index_moments_kernel(FusedArgs a, int R, int win, int stride, int M, int wpg, int nch, int wmajor) {
    extern __shared__ __attribute__((aligned(16))) char smem[];
    const int i = blockIdx.y, k = blockIdx.x / nch, c = blockIdx.x - k * nch;
    const int64_t o = (int64_t)i * a.K + k;
    const int j = a.cand[o];
    const int m0 = c * wpg, m1 = m0 + wpg < M ? m0 + wpg : M;
    float* out = a.scores + (wmajor ? (int64_t)i * M * a.K + k : o * M);
    const int64_t sm = wmajor ? a.K : 1;
    if (j < 0 || j >= a.Bj) {
        for (int m = m0 + threadIdx.x; m < m1; m += blockDim.x) out[m * sm] = __builtin_nanf("");
        return;
    }
    xl_stage_q(a, smem, j);
    for (int m = m0; m < m1; ++m) {
        // the pair is made opaque per window: what xl_pair_score derives from (i, j) alone -- operand pointers, the caption's mask
        // registers -- is then derived inside the loop, as in the one-window kernel, instead of being hoisted and held live across it
        int iw = i, jw = j;
        asm volatile("" : "+s"(iw), "+s"(jw));
        const int g0 = m * stride * R;
        xl_pair_score<false, true, true>(a, smem, iw, jw, out + m * sm, GroundOut{}, g0, g0 + win * R);
    }
}

// the same grid with grounding: rows laid out [Bi][K][...]; an index outside [0, capacity) reads nothing: NaN in the float rows, -1 in the
// int rows
__global__ __launch_bounds__(512) void xl_caption_index_pairs_ground_kernel(FusedArgs a, GroundOut go) {
    extern __shared__ __attribute__((aligned(16))) char smem[];
    const int i = blockIdx.y;
    const int64_t o = (int64_t)i * a.K + blockIdx.x;
    const int j = a.cand[o];
    go.word_scores += o * a.W; go.word_region += o * a.W; go.word_weight += o * a.W;
    go.region_scores += o * a.G; go.region_word += o * a.G;
    if (go.frame_scores) go.frame_scores += o * go.frames;
    if (j < 0 || j >= a.Bj) {
        const float nan = __builtin_nanf("");
        if (threadIdx.x == 0) a.scores[o] = nan;
        for (int t = threadIdx.x; t < a.W; t += blockDim.x) { go.word_scores[t] = nan; go.word_weight[t] = nan; go.word_region[t] = -1; }
        for (int t = threadIdx.x; t < a.G; t += blockDim.x) { go.region_scores[t] = nan; go.region_word[t] = -1; }
        if (go.frame_scores)
            for (int t = threadIdx.x; t < go.frames; t += blockDim.x) go.frame_scores[t] = nan;
        return;
    }
    xl_pair_score<true>(a, smem, i, j, a.scores + o, go);
}

// ---- C ABI of the tiled family (include/demovlp_hip.h: dvlp_xattn_long_index_*).  The resident layout, the prep kernel and the query
//      workspace are those of dvlp_xattn_index_* (index_layout / query_layout are generic in G and W); only the range and the pair kernel differ.
static bool xlong_ok(int64_t G, int64_t W) { return G >= 1 && G <= LG_MAX && W >= 1 && W <= 16 * FW_MAXB; }

extern "C" int64_t dvlp_xattn_long_index_bytes(int64_t capacity, int64_t G) {
    if (capacity <= 0 || capacity > INT32_MAX || G <= 0) return DVLP_ERR_SHAPE;
    if (!xlong_ok(G, 1)) return DVLP_ERR_UNSUPPORTED;
    return index_layout(capacity, G).total;
}

extern "C" int dvlp_xattn_long_index_add(int64_t capacity, int64_t G, int64_t row0, int64_t n, const void* Craw, void* index, void* stream) {
    dvlp_clear_status();
    if (capacity <= 0 || capacity > INT32_MAX || G <= 0 || row0 < 0 || n <= 0 || row0 + n > capacity) return DVLP_ERR_SHAPE;
    if (!Craw || !index) return DVLP_ERR_SHAPE;
    if (!xlong_ok(G, 1)) return DVLP_ERR_UNSUPPORTED;
    dvlp_xfused_index_add(capacity, G, row0, n, Craw, index, (hipStream_t)stream);
    return dvlp_launch_status();
}

extern "C" int64_t dvlp_xattn_long_index_query_workspace_bytes(int64_t Bj, int64_t W) {
    if (Bj <= 0 || W <= 0) return DVLP_ERR_SHAPE;
    if (!xlong_ok(1, W)) return DVLP_ERR_UNSUPPORTED;
    return query_layout(Bj, W).total;
}

extern "C" int dvlp_xattn_long_index_pairs_fwd(int64_t capacity, int64_t G, const void* index, const float* mimg, int64_t Bj, int64_t W, int64_t d,
                                               const void* Qraw, const float* mcap, int64_t K, const int* cand, float lam, int gate, float* scores,
                                               void* workspace, void* stream) {
    dvlp_clear_status();
    if (d != FD || capacity <= 0 || capacity > INT32_MAX || G <= 0 || Bj <= 0 || W <= 0 || K <= 0) return DVLP_ERR_SHAPE;
    if (Bj > 65535 || Bj * K > INT32_MAX) return DVLP_ERR_SHAPE;
    if (!index || !mimg || !Qraw || !mcap || !cand || !scores || !workspace) return DVLP_ERR_SHAPE;
    if (!xlong_ok(G, W)) return DVLP_ERR_UNSUPPORTED;
    FusedArgs a = xf_index_prep(capacity, G, index, mimg, Bj, W, Qraw, mcap, K, cand, lam, gate & 1, scores, workspace, (hipStream_t)stream);
    a.stop = 0;
    { static bool once = false; if (!once) { once = true;
        (void)hipFuncSetAttribute((const void*)xl_index_pairs_kernel, hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024); } }
    hipLaunchKernelGGL(xl_index_pairs_kernel, dim3((unsigned)K, (unsigned)Bj), dim3(512), (size_t)LL_TOTAL, (hipStream_t)stream, a);
    return dvlp_launch_status();
}

extern "C" int64_t dvlp_xattn_long_index_ground_workspace_bytes(int64_t Bj, int64_t W, int64_t K, int64_t G) {
    if (Bj <= 0 || W <= 0 || K <= 0 || G <= 0 || Bj > 65535 || Bj * K > INT32_MAX) return DVLP_ERR_SHAPE;
    if (!xlong_ok(G, W)) return DVLP_ERR_UNSUPPORTED;
    return query_layout(Bj, W).total;                               // the caption-side prep; every exchange lives in LDS
}

// anything wrong with the arguments, a shape beyond the range included, is DVLP_ERR_SHAPE (as dvlp_xattn_index_pairs_ground); nothing is launched then
extern "C" int dvlp_xattn_long_index_pairs_ground(int64_t capacity, int64_t G, const void* index, const float* mimg, int64_t Bj, int64_t W, int64_t d,
                                                  const void* Qraw, const float* mcap, const int* cand, int64_t K, int64_t frames, float lam, int gate,
                                                  float* score, float* word_scores, float* region_scores, int* word_region,
                                                  float* word_region_weight, int* region_word, float* frame_scores, void* workspace, void* stream) {
    dvlp_clear_status();
    if (d != FD || capacity <= 0 || capacity > INT32_MAX || G <= 0 || Bj <= 0 || W <= 0 || K < 1) return DVLP_ERR_SHAPE;
    if (Bj > 65535 || Bj * K > INT32_MAX) return DVLP_ERR_SHAPE;
    if (!index || !mimg || !Qraw || !mcap || !cand || !score || !word_scores || !region_scores || !word_region || !word_region_weight ||
        !region_word || !workspace)
        return DVLP_ERR_SHAPE;
    // frames = 0 <=> no frame_scores; otherwise frames must divide G
    if (frames < 0 || frames > G || (frames == 0) != (frame_scores == nullptr) || (frames > 0 && G % frames != 0)) return DVLP_ERR_SHAPE;
    if (!xlong_ok(G, W)) return DVLP_ERR_SHAPE;
    FusedArgs a = xf_index_prep(capacity, G, index, mimg, Bj, W, Qraw, mcap, K, cand, lam, gate & 1, score, workspace, (hipStream_t)stream);
    a.stop = 0;
    GroundOut go{};
    go.word_scores = word_scores; go.region_scores = region_scores; go.word_region = word_region; go.region_word = region_word;
    go.word_weight = word_region_weight; go.frame_scores = frame_scores; go.frames = (int)frames;
    { static bool once = false; if (!once) { once = true;
        (void)hipFuncSetAttribute((const void*)xl_index_pairs_ground_kernel, hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024); } }
    hipLaunchKernelGGL(xl_index_pairs_ground_kernel, dim3((unsigned)K, (unsigned)Bj), dim3(512), (size_t)LL_TOTAL, (hipStream_t)stream, a, go);
    return dvlp_launch_status();
}

// ---- moments: every window of `win` frames at starts 0, stride, 2 stride, ... of the pairs of dvlp_xattn_long_index_pairs_fwd
extern "C" int64_t dvlp_xattn_long_index_moments_count(int64_t G, int64_t frames, int64_t win, int64_t stride) {
    if (G <= 0 || frames < 1 || frames > G || G % frames != 0 || win < 1 || win > frames || stride < 1) return DVLP_ERR_SHAPE;
    if (!xlong_ok(G, 1)) return DVLP_ERR_UNSUPPORTED;
    return (frames - win) / stride + 1;
}

extern "C" int dvlp_xattn_long_index_moments_fwd(int64_t capacity, int64_t G, const void* index, const float* mimg, int64_t Bj, int64_t W, int64_t d,
                                                 const void* Qraw, const float* mcap, int64_t K, const int* cand, int64_t frames, int64_t win,
                                                 int64_t stride, float lam, int gate, float* scores, void* workspace, void* stream) {
    dvlp_clear_status();
    if (d != FD || capacity <= 0 || capacity > INT32_MAX || G <= 0 || Bj <= 0 || W <= 0 || K <= 0) return DVLP_ERR_SHAPE;
    if (Bj > 65535 || Bj * K > INT32_MAX) return DVLP_ERR_SHAPE;
    if (!index || !mimg || !Qraw || !mcap || !cand || !scores || !workspace) return DVLP_ERR_SHAPE;
    if (!xlong_ok(G, W)) return DVLP_ERR_UNSUPPORTED;
    const int64_t M = dvlp_xattn_long_index_moments_count(G, frames, win, stride);
    if (M < 0) return (int)M;
    if (K * M > INT32_MAX || Bj * K * M > INT32_MAX) return DVLP_ERR_SHAPE;      // the (window, candidate) grid axis; the score offsets
    FusedArgs a = xf_index_prep(capacity, G, index, mimg, Bj, W, Qraw, mcap, K, cand, lam, gate & 1, scores, workspace, (hipStream_t)stream);
    a.stop = 0;
    { static bool once = false; if (!once) { once = true;
        (void)hipFuncSetAttribute((const void*)xl_index_moments_kernel, hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024); } }
    hipLaunchKernelGGL(xl_index_moments_kernel, dim3((unsigned)(K * M), (unsigned)Bj), dim3(512), (size_t)LL_TOTAL, (hipStream_t)stream, a,
                       (int)(G / frames), (int)win, (int)stride, (int)M);
    return dvlp_launch_status();
}

// ---- C ABI of the video-major tiled family (dvlp_xattn_long_caption_index_*): the resident caption side is the one
//      dvlp_xattn_caption_index_bytes / _add define (query_layout is generic in W, and W <= 112 in both families), the video-side prep and
//      workspace are those of dvlp_xattn_caption_index_* (index_layout at capacity Bi); only the range of G and the pair kernel differ.
extern "C" int64_t dvlp_xattn_long_caption_index_query_workspace_bytes(int64_t Bi, int64_t G, int64_t W) {
    if (Bi <= 0 || G <= 0 || W <= 0 || Bi > 65535) return DVLP_ERR_SHAPE;
    if (!xlong_ok(G, W)) return DVLP_ERR_UNSUPPORTED;
    return index_layout(Bi, G).total;
}

extern "C" int dvlp_xattn_long_caption_index_pairs_fwd(int64_t capacity, int64_t W, const void* index, const float* mcap, int64_t Bi, int64_t G,
                                                       int64_t d, const void* Craw, const float* mimg, int64_t K, const int* cand, float lam,
                                                       int gate, float* scores, void* workspace, void* stream) {
    dvlp_clear_status();
    if (d != FD || capacity <= 0 || capacity > INT32_MAX || W <= 0 || Bi <= 0 || G <= 0 || K <= 0) return DVLP_ERR_SHAPE;
    if (Bi > 65535 || Bi * K > INT32_MAX) return DVLP_ERR_SHAPE;
    if (!index || !mcap || !Craw || !mimg || !cand || !scores || !workspace) return DVLP_ERR_SHAPE;
    if (!xlong_ok(G, W)) return DVLP_ERR_UNSUPPORTED;
    FusedArgs a = xf_caption_index_prep(capacity, W, index, mcap, Bi, G, Craw, mimg, K, cand, lam, gate & 1, scores, workspace, (hipStream_t)stream);
    a.stop = 0;
    { static bool once = false; if (!once) { once = true;
        (void)hipFuncSetAttribute((const void*)xl_caption_index_pairs_kernel, hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024); } }
    hipLaunchKernelGGL(xl_caption_index_pairs_kernel, dim3((unsigned)K, (unsigned)Bi), dim3(512), (size_t)LL_TOTAL, (hipStream_t)stream, a);
    return dvlp_launch_status();
}

extern "C" int64_t dvlp_xattn_long_caption_index_ground_workspace_bytes(int64_t Bi, int64_t G, int64_t K, int64_t W) {
    if (Bi <= 0 || G <= 0 || K <= 0 || W <= 0 || Bi > 65535 || Bi * K > INT32_MAX) return DVLP_ERR_SHAPE;
    if (!xlong_ok(G, W)) return DVLP_ERR_UNSUPPORTED;
    return index_layout(Bi, G).total;                               // the video-side prep; every exchange lives in LDS
}

// anything wrong with the arguments, a shape beyond the range included, is DVLP_ERR_SHAPE (as dvlp_xattn_long_index_pairs_ground); nothing is
// launched then
extern "C" int dvlp_xattn_long_caption_index_pairs_ground(int64_t capacity, int64_t W, const void* index, const float* mcap, int64_t Bi, int64_t G,
                                                          int64_t d, const void* Craw, const float* mimg, const int* cand, int64_t K,
                                                          int64_t frames, float lam, int gate, float* score, float* word_scores,
                                                          float* region_scores, int* word_region, float* word_region_weight, int* region_word,
                                                          float* frame_scores, void* workspace, void* stream) {
    dvlp_clear_status();
    if (d != FD || capacity <= 0 || capacity > INT32_MAX || W <= 0 || Bi <= 0 || G <= 0 || K < 1) return DVLP_ERR_SHAPE;
    if (Bi > 65535 || Bi * K > INT32_MAX) return DVLP_ERR_SHAPE;
    if (!index || !mcap || !Craw || !mimg || !cand || !score || !word_scores || !region_scores || !word_region || !word_region_weight ||
        !region_word || !workspace)
        return DVLP_ERR_SHAPE;
    // frames = 0 <=> no frame_scores; otherwise frames must divide G
    if (frames < 0 || frames > G || (frames == 0) != (frame_scores == nullptr) || (frames > 0 && G % frames != 0)) return DVLP_ERR_SHAPE;
    if (!xlong_ok(G, W)) return DVLP_ERR_SHAPE;
    FusedArgs a = xf_caption_index_prep(capacity, W, index, mcap, Bi, G, Craw, mimg, K, cand, lam, gate & 1, score, workspace, (hipStream_t)stream);
    a.stop = 0;
    GroundOut go{};
    go.word_scores = word_scores; go.region_scores = region_scores; go.word_region = word_region; go.region_word = region_word;
    go.word_weight = word_region_weight; go.frame_scores = frame_scores; go.frames = (int)frames;
    { static bool once = false; if (!once) { once = true;
        (void)hipFuncSetAttribute((const void*)xl_caption_index_pairs_ground_kernel, hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024); } }
    hipLaunchKernelGGL(xl_caption_index_pairs_ground_kernel, dim3((unsigned)K, (unsigned)Bi), dim3(512), (size_t)LL_TOTAL, (hipStream_t)stream, a,
                       go);
    return dvlp_launch_status();
}

// ---- moments of a query video against the resident captions: the windows of dvlp_xattn_long_index_moments_fwd on the pairs of
//      dvlp_xattn_long_caption_index_pairs_fwd, up to windows_per_group consecutive windows of a pair per workgroup
// windows per workgroup when the caller leaves it open: host arithmetic on (Bi, K, M) alone.  One workgroup fits a CU (150 KB of LDS) and
// the chip has 256 of them: when the pairs alone fill it, a workgroup walks all M windows of its pair and the caption is staged once per
// pair; below that the windows are cut into just enough chunks to give every CU a workgroup.
static int64_t xl_moments_plan(int64_t Bi, int64_t K, int64_t M) {
    const int64_t pairs = Bi * K, cus = 256;
    if (pairs >= cus) return M;
    const int64_t want = (cus + pairs - 1) / pairs;             // chunks per pair that fill the chip
    const int64_t n = M / want;                                 // (floor: at least `want` chunks)
    return n < 1 ? 1 : n;
}

extern "C" int dvlp_xattn_long_caption_index_moments_fwd(int64_t capacity, int64_t W, const void* index, const float* mcap, int64_t Bi, int64_t G,
                                                         int64_t d, const void* Craw, const float* mimg, int64_t K, const int* cand, int64_t frames,
                                                         int64_t win, int64_t stride, int64_t windows_per_group, int window_major, float lam,
                                                         int gate, float* scores, void* workspace, void* stream) {
    dvlp_clear_status();
    if (d != FD || capacity <= 0 || capacity > INT32_MAX || W <= 0 || Bi <= 0 || G <= 0 || K <= 0 || windows_per_group < 0) return DVLP_ERR_SHAPE;
    if (Bi > 65535 || Bi * K > INT32_MAX) return DVLP_ERR_SHAPE;
    if (!index || !mcap || !Craw || !mimg || !cand || !scores || !workspace) return DVLP_ERR_SHAPE;
    if (!xlong_ok(G, W)) return DVLP_ERR_UNSUPPORTED;
    const int64_t M = dvlp_xattn_long_index_moments_count(G, frames, win, stride);
    if (M < 0) return (int)M;
    if (K * M > INT32_MAX || Bi * K * M > INT32_MAX) return DVLP_ERR_SHAPE;      // the (chunk, candidate) grid axis; the score offsets
    int64_t wpg = windows_per_group ? windows_per_group : xl_moments_plan(Bi, K, M);
    if (wpg > M) wpg = M;
    const int64_t nch = (M + wpg - 1) / wpg;
    FusedArgs a = xf_caption_index_prep(capacity, W, index, mcap, Bi, G, Craw, mimg, K, cand, lam, gate & 1, scores, workspace, (hipStream_t)stream);
    a.stop = 0;
    { static bool once = false; if (!once) { once = true;
        (void)hipFuncSetAttribute((const void*)xl_caption_index_moments_kernel, hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024); } }
    hipLaunchKernelGGL(xl_caption_index_moments_kernel, dim3((unsigned)(K * nch), (unsigned)Bi), dim3(512), (size_t)LL_TOTAL, (hipStream_t)stream,
                       a, (int)(G / frames), (int)win, (int)stride, (int)M, (int)wpg, (int)nch, window_major ? 1 : 0);
    return dvlp_launch_status();
}
