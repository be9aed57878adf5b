// Video-QA answer head (BUTDQAHead, model/video_qa_mdoel.py:56-97, on the embeddings of ObjectQARelation.compute_fusion, model/model.py:281-289)
// and its loss (CrossEntropy, model/loss.py:180-187).
//
//   wn_fold_*          weight_norm(dim=None) of the head's five linears, W = g V / |V|_F, all tensors in ONE launch (one workgroup per tensor)
//   token_max_*        max over the 100 token projections, first index on ties (torch.max on the CPU reference)
//   qa_attend_*        Attention.forward + the weighted region sum: per sample  qp = relu(W_q q + b_q),  H = relu(v W_v^T + b_v),
//                      logit_g = ((H_g . qp . keep_g / (1-p)) . w_l + b_l) mask_g,  att = softmax_g,  pooled = sum_g att_g v_g
//   softmax_xent       mean cross-entropy, d logits and the arg-max prediction in one pass over the logits
//
// Cut of the attention (DESIGN.md "QA head"): a (64-row tile, sample) grid -- B = 64, G = 240 gives 256 workgroups, one per CU, where one
// workgroup per sample would leave 192 CUs idle.  bf16, G <= 288: each workgroup stages W_v (bf16, 128 KB) in LDS once; each of its four waves
// holds 16 rows of v in registers as the B operand of v_mfma_f32_16x16x32_bf16 and walks the 16 column tiles of H^T.  In that orientation a
// lane holds ONE region g = lane & 15 and four consecutive output channels n, so bias, ReLU, the qp . w_l factor, the dropout (one Philox call
// yields exactly those four channels' words) and the dot with w_l are lane-local; H never leaves the registers.  The [B, G] logits go to a second,
// small launch (softmax + pool, one workgroup per sample).  The backward recomputes H the same way and emits the pre-ReLU gradient dH.
// fp32 embeddings and G > 288 take the general route: H comes from dvlp_gemm (the caller's launch) and qa_rows_kernel is its epilogue.
//
// Every cross-lane / cross-wave / cross-workgroup sum adds its partials in a fixed order: no float atomics, results are bit-reproducible.
#include "common.h"
#include <atomic>

namespace {

constexpr int QA_D = 256;          // every width inside the head (v_dim = q_dim = hid_dim)
constexpr int QA_TILE = 64;        // rows of one workgroup (4 waves x 16)
constexpr int QA_WROW = QA_D + 8;  // LDS row pitch of W_v in bf16 elements: 528 B = 4 banks past a multiple of 64 banks, so the 16 rows of a ds_read_b128 spread
constexpr int WN_MAX = 8;

inline uint32_t qa_drop_threshold(float p) {
    const double t = (double)p * 4294967296.0;
    return t >= 4294967295.0 ? 0xffffffffu : (uint32_t)t;
}

// block-wide sum in a fixed order: strided per-thread partials (the caller's), DPP butterfly inside a wave, then the waves' values in index order
template <int NW>
__device__ __forceinline__ float block_sum(float v, float* red) {
    v = wave_sum(v);
    __syncthreads();
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = v;
    __syncthreads();
    float t = 0.f;
#pragma unroll
    for (int w = 0; w < NW; ++w) t += red[w];
    return t;
}
template <int NW>
__device__ __forceinline__ float block_max(float v, float* red) {
    v = wave_max(v);
    __syncthreads();
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = v;
    __syncthreads();
    float t = red[0];
#pragma unroll
    for (int w = 1; w < NW; ++w) t = fmaxf(t, red[w]);
    return t;
}

// ---------------------------------------------------------------------------------------------------------------------------------
// weight-norm fold
// ---------------------------------------------------------------------------------------------------------------------------------
struct WnArgs {
    const float* V[WN_MAX];
    const float* g[WN_MAX];
    const float* dW[WN_MAX];
    float* W[WN_MAX];        // fwd: folded weight   bwd: dV
    bf16* Wb[WN_MAX];        // fwd: optional bf16 copy of the folded weight
    float* dg[WN_MAX];
    int64_t n[WN_MAX];
    float* norms;
};

__global__ __launch_bounds__(1024) void wn_fold_fwd_kernel(WnArgs a) {
    __shared__ float red[16];
    const int t = blockIdx.x;
    const float* __restrict__ V = a.V[t];
    const int64_t n = a.n[t];
    float s = 0.f;
    for (int64_t i = threadIdx.x; i < n; i += 1024) s += V[i] * V[i];
    const float nrm = sqrtf(block_sum<16>(s, red));
    const float sc = a.g[t][0] / nrm;
    if (threadIdx.x == 0) a.norms[t] = nrm;
    float* __restrict__ W = a.W[t];
    bf16* __restrict__ Wb = a.Wb[t];
    for (int64_t i = threadIdx.x; i < n; i += 1024) {
        const float w = V[i] * sc;
        W[i] = w;
        if (Wb) Wb[i] = (bf16)w;
    }
}

// dg = <dW, V> / |V|,  dV = (g / |V|) (dW - <dW, V> / |V|^2  V)
__global__ __launch_bounds__(1024) void wn_fold_bwd_kernel(WnArgs a) {
    __shared__ float red[16];
    const int t = blockIdx.x;
    const float* __restrict__ V = a.V[t];
    const float* __restrict__ dW = a.dW[t];
    const int64_t n = a.n[t];
    float s = 0.f;
    for (int64_t i = threadIdx.x; i < n; i += 1024) s += dW[i] * V[i];
    const float dot = block_sum<16>(s, red);
    const float nrm = a.norms[t], g = a.g[t][0];
    if (threadIdx.x == 0) a.dg[t][0] = dot / nrm;
    const float sc = g / nrm, k = dot / (nrm * nrm);
    float* __restrict__ dV = a.W[t];
    for (int64_t i = threadIdx.x; i < n; i += 1024) dV[i] = sc * (dW[i] - k * V[i]);
}

// ---------------------------------------------------------------------------------------------------------------------------------
// token max
// ---------------------------------------------------------------------------------------------------------------------------------
// block (256, 4): thread (c, s) scans tokens t = s, s + 4, ... of column c; the four candidates merge by (value, then smaller index)
template <typename T>
__global__ __launch_bounds__(1024) void token_max_fwd_kernel(int T_, int d, const T* __restrict__ x, float* __restrict__ out, int* __restrict__ idx) {
    __shared__ float sv[4][256];
    __shared__ int si[4][256];
    const int b = blockIdx.x, tx = threadIdx.x, ty = threadIdx.y;
    for (int c0 = 0; c0 < d; c0 += 256) {
        const int c = c0 + tx;
        float best = -INFINITY;
        int bi = -1;
        if (c < d)
            for (int t = ty; t < T_; t += 4) {
                const float v = to_f(x[((int64_t)b * T_ + t) * d + c]);
                if (bi < 0 || v > best) { best = v; bi = t; }
            }
        sv[ty][tx] = best; si[ty][tx] = bi;
        __syncthreads();
        if (ty == 0 && c < d) {
#pragma unroll
            for (int s = 1; s < 4; ++s) {
                const float v = sv[s][tx];
                const int i = si[s][tx];
                if (i >= 0 && (bi < 0 || v > best || (v == best && i < bi))) { best = v; bi = i; }
            }
            out[(int64_t)b * d + c] = best;
            idx[(int64_t)b * d + c] = bi;
        }
        __syncthreads();
    }
}

template <typename T>
__global__ __launch_bounds__(256) void token_max_bwd_kernel(int64_t rows, int T_, int d, const float* __restrict__ dout, const int* __restrict__ idx, T* __restrict__ dx) {
    const int64_t r = blockIdx.x;              // = b T + t
    if (r >= rows) return;
    const int64_t b = r / T_;
    const int t = (int)(r - b * T_);
    for (int c = threadIdx.x; c < d; c += 256) dx[r * d + c] = from_f<T>(idx[b * d + c] == t ? dout[b * d + c] : 0.f);
}

// ---------------------------------------------------------------------------------------------------------------------------------
// region attention
// ---------------------------------------------------------------------------------------------------------------------------------
struct QaArgs {
    int B, G, tiles;
    int64_t vss, vrs;              // element strides of v between samples / regions (channels are contiguous)
    int64_t hrows;                 // rows per sample in H / dH / dv (row b hrows + g, 256 channels)
    const void* v;
    const float* mask;             // [B, G] 0/1
    const float* q;                // [B, 256]
    const float *Wq, *bq, *bv, *wl, *bl;
    const bf16* Wvb;               // bf16 W_v [256 out, 256 in] (fused route)
    const void* H;                 // pre-ReLU v W_v^T + b_v (general route)
    float* qp;                     // [B, 256]
    float* att;                    // [B, G]: logits, then the softmax
    float* pooled;                 // [B, 256]
    uint32_t thr; float scale;     // dropout: keep iff word >= thr, scale 1 / (1 - p); thr = 0 <=> no dropout
    const uint32_t* state;         // {seed_lo, seed_hi, offset, -}
    uint32_t* snap;                // fwd: copy of the state for the backward
    uint32_t site;
    // backward
    const float* dpooled;          // [B, 256]
    void *dv, *dH;
    float *dlog, *dblp, *pS, *pBv, *dqpre;      // workspace
    float *dq, *dWq, *dbq, *dbv, *dwl, *dbl;
};

// qp = relu(W_q q + b_q): one workgroup per sample, a wave per output channel (lanes split the 256 inputs)
__global__ __launch_bounds__(256) void qa_qproj_kernel(QaArgs a) {
    const int b = blockIdx.x, lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    const float4 qv = *(const float4*)(a.q + (int64_t)b * QA_D + 4 * lane);
    for (int n = w; n < QA_D; n += 4) {
        const float4 wv = *(const float4*)(a.Wq + (int64_t)n * QA_D + 4 * lane);
        const float s = wave_sum(wv.x * qv.x + wv.y * qv.y + wv.z * qv.z + wv.w * qv.w);
        if (lane == 0) a.qp[(int64_t)b * QA_D + n] = fmaxf(s + a.bq[n], 0.f);
    }
    if (b == 0 && threadIdx.x < 4 && a.snap && a.state) a.snap[threadIdx.x] = a.state[threadIdx.x];
}

// keep / (1 - p) of the four channels 4 c4 .. 4 c4 + 3 of region row `row` (= b G + g): flat element (row 256 + n) of a [B, G, 256] tensor in the
// numbering of dropout_fwd_kernel (word e % 4 of counter e / 4)
__device__ __forceinline__ void qa_keep4(const QaArgs& a, const uint32_t* st, int64_t row, int c4, float (&ks)[4]) {
    if (a.thr == 0u) { ks[0] = ks[1] = ks[2] = ks[3] = 1.f; return; }
    const uint64_t i = (uint64_t)row * (QA_D / 4) + (uint64_t)c4;
    uint32_t u[4];
    philox4x32_10((uint32_t)i, (uint32_t)(i >> 32), a.site, st[2], st[0], st[1], u);
#pragma unroll
    for (int t = 0; t < 4; ++t) ks[t] = u[t] >= a.thr ? a.scale : 0.f;
}

// Fused route.  grid (tiles, B), 256 threads, dynamic LDS: W_v bf16 [256][QA_WROW] + 2 x [4 waves][256] floats (backward partials).
template <bool BWD>
__global__ __launch_bounds__(256) void qa_tile_kernel(QaArgs a) {
    extern __shared__ __attribute__((aligned(16))) char smem[];
    bf16* Ws = (bf16*)smem;
    float* part = (float*)(smem + (size_t)QA_D * QA_WROW * sizeof(bf16));          // [2][4][256]
    const int tile = blockIdx.x, b = blockIdx.y, tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
    const int col = lane & 15, quad = lane >> 4;
    // stage W_v: 256 rows x 32 chunks of 16 bytes
    for (int i = tid; i < QA_D * (QA_D / 8); i += 256) {
        const int r = i >> 5, c = i & 31;
        *(bf16x8*)(Ws + r * QA_WROW + 8 * c) = *(const bf16x8*)(a.Wvb + (int64_t)r * QA_D + 8 * c);
    }
    const uint32_t* st = BWD ? a.snap : a.state;
    // this lane's region and its eight B fragments (rows past G read as zero and are never stored)
    const int g = tile * QA_TILE + 16 * w + col;
    const bool live = g < a.G;
    bf16x8 vf[8];
    {
        const bf16* vp = (const bf16*)a.v + (int64_t)b * a.vss + (int64_t)(live ? g : 0) * a.vrs + 8 * quad;
#pragma unroll
        for (int ks = 0; ks < 8; ++ks) {
            vf[ks] = *(const bf16x8*)(vp + 32 * ks);
            if (!live)
#pragma unroll
                for (int t = 0; t < 8; ++t) vf[ks][t] = (bf16)0.f;
        }
    }
    const float dl = (BWD && live) ? a.dlog[(int64_t)b * a.G + g] : 0.f;
    const float* qp = a.qp + (int64_t)b * QA_D;
    const int64_t row = (int64_t)b * a.G + g;
    float logit = 0.f;
    __syncthreads();
#pragma unroll 1
    for (int nt = 0; nt < 16; ++nt) {
        f32x4 c = {0.f, 0.f, 0.f, 0.f};
        const bf16* ap = Ws + (nt * 16 + col) * QA_WROW + 8 * quad;
#pragma unroll
        for (int ks = 0; ks < 8; ++ks) c = __builtin_amdgcn_mfma_f32_16x16x32_bf16(*(const bf16x8*)(ap + 32 * ks), vf[ks], c, 0, 0, 0);
        const int n0 = nt * 16 + 4 * quad;                    // c[i] = H[g][n0 + i]
        float ks4[4];
        qa_keep4(a, st, live ? row : 0, nt * 4 + quad, ks4);
        const float4 bv = *(const float4*)(a.bv + n0), wl = *(const float4*)(a.wl + n0), qv = *(const float4*)(qp + n0);
        const float bvv[4] = {bv.x, bv.y, bv.z, bv.w}, wlv[4] = {wl.x, wl.y, wl.z, wl.w}, qvv[4] = {qv.x, qv.y, qv.z, qv.w};
        if (!BWD) {
#pragma unroll
            for (int i = 0; i < 4; ++i) logit += fmaxf(c[i] + bvv[i], 0.f) * (qvv[i] * ks4[i]) * wlv[i];
        } else {
            float s4[4], d4[4];
            bf16x4 o;
#pragma unroll
            for (int i = 0; i < 4; ++i) {
                const float h = c[i] + bvv[i];
                const float dh = h > 0.f ? dl * wlv[i] * (qvv[i] * ks4[i]) : 0.f;
                o[i] = (bf16)dh;
                s4[i] = row16_sum(dl * fmaxf(h, 0.f) * ks4[i]);      // S[n] = sum_g dl_g relu(H_gn) keep_gn: d qp = S w_l, d w_l = S qp
                d4[i] = row16_sum(dh);                               // d b_v
            }
            if (live) *(bf16x4*)((bf16*)a.dH + ((int64_t)b * a.hrows + g) * QA_D + n0) = o;
            if (col == 0) {
#pragma unroll
                for (int i = 0; i < 4; ++i) { part[w * QA_D + n0 + i] = s4[i]; part[(4 + w) * QA_D + n0 + i] = d4[i]; }
            }
        }
    }
    if (!BWD) {
        logit = col4_sum(logit);
        if (quad == 0 && live) a.att[row] = (logit + a.bl[0]) * a.mask[row];
    } else {
        __syncthreads();
        const int64_t o = ((int64_t)b * a.tiles + tile) * QA_D + tid;
        a.pS[o] = ((part[tid] + part[QA_D + tid]) + part[2 * QA_D + tid]) + part[3 * QA_D + tid];
        a.pBv[o] = ((part[4 * QA_D + tid] + part[5 * QA_D + tid]) + part[6 * QA_D + tid]) + part[7 * QA_D + tid];
    }
}

// General route: H (pre-ReLU, bias added) comes from memory.  grid (tiles, B), 256 threads; wave w takes rows w, w + 4, ... of the tile, a lane
// four consecutive channels (one Philox call), so the backward's channel sums stay in the lane until the waves meet in LDS.
template <typename T, bool BWD>
__global__ __launch_bounds__(256) void qa_rows_kernel(QaArgs a) {
    __shared__ float part[8 * QA_D];
    const int tile = blockIdx.x, b = blockIdx.y, tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
    const int n0 = 4 * lane;
    const uint32_t* st = BWD ? a.snap : a.state;
    const float4 bq = *(const float4*)(a.qp + (int64_t)b * QA_D + n0), wl = *(const float4*)(a.wl + n0);
    const float qvv[4] = {bq.x, bq.y, bq.z, bq.w}, wlv[4] = {wl.x, wl.y, wl.z, wl.w};
    float s4[4] = {0.f, 0.f, 0.f, 0.f}, d4[4] = {0.f, 0.f, 0.f, 0.f};
    const int gend = min(a.G, (tile + 1) * QA_TILE);
    for (int g = tile * QA_TILE + w; g < gend; g += 4) {
        const int64_t row = (int64_t)b * a.G + g, hrow = (int64_t)b * a.hrows + g;
        float ks4[4], h[4];
        qa_keep4(a, st, row, lane, ks4);
        const T* hp = (const T*)a.H + hrow * QA_D + n0;
#pragma unroll
        for (int i = 0; i < 4; ++i) h[i] = to_f(hp[i]);
        if (!BWD) {
            float z = 0.f;
#pragma unroll
            for (int i = 0; i < 4; ++i) z += fmaxf(h[i], 0.f) * (qvv[i] * ks4[i]) * wlv[i];
            z = wave_sum(z);
            if (lane == 0) a.att[row] = (z + a.bl[0]) * a.mask[row];
        } else {
            const float dl = a.dlog[row];
            T* op = (T*)a.dH + hrow * QA_D + n0;
#pragma unroll
            for (int i = 0; i < 4; ++i) {
                const float dh = h[i] > 0.f ? dl * wlv[i] * (qvv[i] * ks4[i]) : 0.f;
                op[i] = from_f<T>(dh);
                s4[i] += dl * fmaxf(h[i], 0.f) * ks4[i];
                d4[i] += dh;
            }
        }
    }
    if (BWD) {
#pragma unroll
        for (int i = 0; i < 4; ++i) { part[w * QA_D + n0 + i] = s4[i]; part[(4 + w) * QA_D + n0 + i] = d4[i]; }
        __syncthreads();
        const int64_t o = ((int64_t)b * a.tiles + tile) * QA_D + tid;
        a.pS[o] = ((part[tid] + part[QA_D + tid]) + part[2 * QA_D + tid]) + part[3 * QA_D + tid];
        a.pBv[o] = ((part[4 * QA_D + tid] + part[5 * QA_D + tid]) + part[6 * QA_D + tid]) + part[7 * QA_D + tid];
    }
}

// softmax over the G logits of a sample (in place in att) and pooled = sum_g att_g v_g.  One workgroup of 16 waves per sample: wave w takes regions
// w, w + 16, ..., a lane four channels; the 16 partial rows are added in wave order.
template <typename T>
__global__ __launch_bounds__(1024) void qa_softmax_pool_kernel(QaArgs a) {
    __shared__ float red[16];
    __shared__ float part[16 * QA_D];
    const int b = blockIdx.x, tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
    float* att = a.att + (int64_t)b * a.G;
    float m = -INFINITY;
    for (int g = tid; g < a.G; g += 1024) m = fmaxf(m, att[g]);
    m = block_max<16>(m, red);
    float s = 0.f;
    for (int g = tid; g < a.G; g += 1024) s += expf(att[g] - m);
    s = block_sum<16>(s, red);
    const float inv = 1.f / s;
    for (int g = tid; g < a.G; g += 1024) att[g] = expf(att[g] - m) * inv;
    __syncthreads();
    float acc[4] = {0.f, 0.f, 0.f, 0.f};
    const T* vb = (const T*)a.v + (int64_t)b * a.vss + 4 * lane;
#pragma unroll 4
    for (int g = w; g < a.G; g += 16) {
        const float p = att[g];
        const T* vp = vb + (int64_t)g * a.vrs;
#pragma unroll
        for (int i = 0; i < 4; ++i) acc[i] += p * to_f(vp[i]);
    }
#pragma unroll
    for (int i = 0; i < 4; ++i) part[w * QA_D + 4 * lane + i] = acc[i];
    __syncthreads();
    if (tid < QA_D) {
        float t = 0.f;
#pragma unroll
        for (int k = 0; k < 16; ++k) t += part[k * QA_D + tid];
        a.pooled[(int64_t)b * QA_D + tid] = t;
    }
}

// backward of pool + softmax + mask: d att_g = d pooled . v_g,  d logit_g = att_g (d att_g - sum_g' att_g' d att_g') mask_g,  dv_g = att_g d pooled
// (the direct part; dH W_v is accumulated onto it by the caller's GEMM).  One workgroup of 16 waves per sample.
template <typename T>
__global__ __launch_bounds__(1024) void qa_pool_bwd_kernel(QaArgs a) {
    __shared__ float red[16];
    const int b = blockIdx.x, tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
    const float* att = a.att + (int64_t)b * a.G;
    float* dlog = a.dlog + (int64_t)b * a.G;
    const float4 dp4 = *(const float4*)(a.dpooled + (int64_t)b * QA_D + 4 * lane);
    const float dp[4] = {dp4.x, dp4.y, dp4.z, dp4.w};
    const T* vb = (const T*)a.v + (int64_t)b * a.vss + 4 * lane;
    T* dvb = (T*)a.dv + (int64_t)b * a.hrows * QA_D + 4 * lane;
    for (int g = w; g < a.G; g += 16) {
        const T* vp = vb + (int64_t)g * a.vrs;
        const float p = att[g];
        float d = 0.f;
#pragma unroll
        for (int i = 0; i < 4; ++i) { d += dp[i] * to_f(vp[i]); dvb[(int64_t)g * QA_D + i] = from_f<T>(p * dp[i]); }
        d = wave_sum(d);
        if (lane == 0) dlog[g] = d;
    }
    __syncthreads();
    float s = 0.f;
    for (int g = tid; g < a.G; g += 1024) s += att[g] * dlog[g];
    s = block_sum<16>(s, red);
    float t = 0.f;
    for (int g = tid; g < a.G; g += 1024) {
        const float dl = att[g] * (dlog[g] - s) * a.mask[(int64_t)b * a.G + g];
        dlog[g] = dl;
        t += dl;
    }
    t = block_sum<16>(t, red);
    if (tid == 0) a.dblp[b] = t;
}

// per sample: S = sum of the tiles' partials, d qpre = S w_l [qp > 0], dq = d qpre W_q
__global__ __launch_bounds__(256) void qa_finish_sample_kernel(QaArgs a) {
    __shared__ float dqs[QA_D];
    const int b = blockIdx.x, n = threadIdx.x;
    float s = 0.f;
    for (int t = 0; t < a.tiles; ++t) s += a.pS[((int64_t)b * a.tiles + t) * QA_D + n];
    const float d = a.qp[(int64_t)b * QA_D + n] > 0.f ? s * a.wl[n] : 0.f;
    a.dqpre[(int64_t)b * QA_D + n] = d;
    dqs[n] = d;
    __syncthreads();
    float acc = 0.f;
    for (int k = 0; k < QA_D; ++k) acc += dqs[k] * a.Wq[(int64_t)k * QA_D + n];
    a.dq[(int64_t)b * QA_D + n] = acc;
}

// across samples, in sample order: block n < 256: dW_q[n][:] = sum_b d qpre[b][n] q[b][:];  block 256: d w_l, d b_v, d b_q, d b_l
__global__ __launch_bounds__(256) void qa_finish_params_kernel(QaArgs a) {
    const int n = blockIdx.x, k = threadIdx.x;
    if (n < QA_D) {
        float acc = 0.f;
        for (int b = 0; b < a.B; ++b) acc += a.dqpre[(int64_t)b * QA_D + n] * a.q[(int64_t)b * QA_D + k];
        a.dWq[(int64_t)n * QA_D + k] = acc;
        return;
    }
    float dwl = 0.f, dbv = 0.f, dbq = 0.f;
    for (int b = 0; b < a.B; ++b) {
        float s = 0.f, v = 0.f;
        for (int t = 0; t < a.tiles; ++t) {
            s += a.pS[((int64_t)b * a.tiles + t) * QA_D + k];
            v += a.pBv[((int64_t)b * a.tiles + t) * QA_D + k];
        }
        dwl += s * a.qp[(int64_t)b * QA_D + k];
        dbv += v;
        dbq += a.dqpre[(int64_t)b * QA_D + k];
    }
    a.dwl[k] = dwl; a.dbv[k] = dbv; a.dbq[k] = dbq;
    if (k == 0) {
        float t = 0.f;
        for (int b = 0; b < a.B; ++b) t += a.dblp[b];
        a.dbl[0] = t;
    }
}

// ---------------------------------------------------------------------------------------------------------------------------------
// softmax cross-entropy: one workgroup per row
// ---------------------------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void softmax_xent_kernel(int64_t C, float invB, const float* __restrict__ logits, const int64_t* __restrict__ labels,
                                                           float* __restrict__ loss_rows, float* __restrict__ dlogits, int* __restrict__ pred) {
    __shared__ float sv[256];
    __shared__ int si[256];
    __shared__ float red[4];
    const int64_t r = blockIdx.x;
    const int tid = threadIdx.x;
    const float* x = logits + r * C;
    float best = -INFINITY;
    int bi = -1;
    for (int64_t c = tid; c < C; c += 256) {
        const float v = x[c];
        if (bi < 0 || v > best) { best = v; bi = (int)c; }
    }
    sv[tid] = best; si[tid] = bi;
    __syncthreads();
    for (int s = 128; s > 0; s >>= 1) {
        if (tid < s) {
            const float v = sv[tid + s];
            const int i = si[tid + s];
            if (i >= 0 && (si[tid] < 0 || v > sv[tid] || (v == sv[tid] && i < si[tid]))) { sv[tid] = v; si[tid] = i; }
        }
        __syncthreads();
    }
    const float m = sv[0];
    float s = 0.f;
    for (int64_t c = tid; c < C; c += 256) s += expf(x[c] - m);
    s = block_sum<4>(s, red);
    const int64_t y = labels[r];
    const bool ok = y >= 0 && y < C;
    if (tid == 0) {
        pred[r] = si[0];
        loss_rows[r] = ok ? (logf(s) + m) - x[y] : __builtin_nanf("");
    }
    if (dlogits) {
        const float inv = 1.f / s;
        for (int64_t c = tid; c < C; c += 256) dlogits[r * C + c] = (expf(x[c] - m) * inv - (c == y ? 1.f : 0.f)) * invB;
    }
}

__global__ __launch_bounds__(64) void xent_mean_kernel(int64_t B, const float* __restrict__ loss_rows, float* __restrict__ loss) {
    if (threadIdx.x != 0) return;
    float t = 0.f;
    for (int64_t r = 0; r < B; ++r) t += loss_rows[r];
    loss[0] = t / (float)B;
}

constexpr size_t QA_TILE_LDS = (size_t)QA_D * QA_WROW * sizeof(bf16) + 8 * QA_D * sizeof(float);

}  // namespace

// ---------------------------------------------------------------------------------------------------------------------------------
// C entries
// ---------------------------------------------------------------------------------------------------------------------------------
extern "C" int dvlp_wn_fold_fwd(int count, const void* const* V, const void* const* g, const int64_t* numel, void* const* W, void* const* Wb,
                                float* norms, void* stream) {
    if (count <= 0 || count > WN_MAX || !V || !g || !numel || !W || !norms) return DVLP_ERR_SHAPE;
    WnArgs a{};
    for (int i = 0; i < count; ++i) {
        if (!V[i] || !g[i] || !W[i] || numel[i] <= 0) return DVLP_ERR_SHAPE;
        a.V[i] = (const float*)V[i]; a.g[i] = (const float*)g[i]; a.W[i] = (float*)W[i]; a.Wb[i] = Wb ? (bf16*)Wb[i] : nullptr; a.n[i] = numel[i];
    }
    a.norms = norms;
    dvlp_clear_status();
    hipLaunchKernelGGL(wn_fold_fwd_kernel, dim3((unsigned)count), dim3(1024), 0, (hipStream_t)stream, a);
    return dvlp_launch_status();
}

extern "C" int dvlp_wn_fold_bwd(int count, const void* const* V, const void* const* g, const int64_t* numel, const void* const* dW,
                                const float* norms, void* const* dV, void* const* dg, void* stream) {
    if (count <= 0 || count > WN_MAX || !V || !g || !numel || !dW || !norms || !dV || !dg) return DVLP_ERR_SHAPE;
    WnArgs a{};
    for (int i = 0; i < count; ++i) {
        if (!V[i] || !g[i] || !dW[i] || !dV[i] || !dg[i] || numel[i] <= 0) return DVLP_ERR_SHAPE;
        a.V[i] = (const float*)V[i]; a.g[i] = (const float*)g[i]; a.dW[i] = (const float*)dW[i]; a.W[i] = (float*)dV[i]; a.dg[i] = (float*)dg[i];
        a.n[i] = numel[i];
    }
    a.norms = const_cast<float*>(norms);
    dvlp_clear_status();
    hipLaunchKernelGGL(wn_fold_bwd_kernel, dim3((unsigned)count), dim3(1024), 0, (hipStream_t)stream, a);
    return dvlp_launch_status();
}

extern "C" int dvlp_token_max_fwd(int dtype, int64_t B, int64_t T, int64_t d, const void* x, float* out, void* idx, void* stream) {
    if (dtype != DVLP_F32 && dtype != DVLP_BF16) return DVLP_ERR_DTYPE;
    if (B <= 0 || T <= 0 || d <= 0 || B > 0x7fffffff || T > 0x7fffffff || d > 0x7fffffff || !x || !out || !idx) return DVLP_ERR_SHAPE;
    dvlp_clear_status();
    if (dtype == DVLP_F32)
        hipLaunchKernelGGL(token_max_fwd_kernel<float>, dim3((unsigned)B), dim3(256, 4), 0, (hipStream_t)stream, (int)T, (int)d, (const float*)x, out, (int*)idx);
    else
        hipLaunchKernelGGL(token_max_fwd_kernel<bf16>, dim3((unsigned)B), dim3(256, 4), 0, (hipStream_t)stream, (int)T, (int)d, (const bf16*)x, out, (int*)idx);
    return dvlp_launch_status();
}

extern "C" int dvlp_token_max_bwd(int dtype, int64_t B, int64_t T, int64_t d, const float* dout, const void* idx, void* dx, void* stream) {
    if (dtype != DVLP_F32 && dtype != DVLP_BF16) return DVLP_ERR_DTYPE;
    if (B <= 0 || T <= 0 || d <= 0 || B * T > 0x7fffffff || d > 0x7fffffff || !dout || !idx || !dx) return DVLP_ERR_SHAPE;
    dvlp_clear_status();
    if (dtype == DVLP_F32)
        hipLaunchKernelGGL(token_max_bwd_kernel<float>, dim3((unsigned)(B * T)), dim3(256), 0, (hipStream_t)stream, B * T, (int)T, (int)d, dout, (const int*)idx, (float*)dx);
    else
        hipLaunchKernelGGL(token_max_bwd_kernel<bf16>, dim3((unsigned)(B * T)), dim3(256), 0, (hipStream_t)stream, B * T, (int)T, (int)d, dout, (const int*)idx, (bf16*)dx);
    return dvlp_launch_status();
}

extern "C" int64_t dvlp_qa_attend_fused(int dtype, int64_t G) { return dtype == DVLP_BF16 && G >= 1 && G <= 288 ? 1 : 0; }

extern "C" int64_t dvlp_qa_attend_workspace_floats(int64_t B, int64_t G) {
    if (B <= 0 || G <= 0) return 0;
    const int64_t tiles = cdiv(G, QA_TILE);
    return B * G + B + 2 * B * tiles * QA_D + B * QA_D;
}

static int qa_common(QaArgs& a, int dtype, int64_t B, int64_t G, const void* v, int64_t vss, int64_t vrs, const float* mask, const void* Wvb, const void* H,
                     int64_t hrows, float drop_p, const void* state) {
    if (dtype != DVLP_F32 && dtype != DVLP_BF16) return DVLP_ERR_DTYPE;
    if (B <= 0 || G <= 0 || B > 65535 || G > (1 << 24) || !v || !mask || vrs < QA_D || vss < 0 || hrows < G) return DVLP_ERR_SHAPE;
    if (!(drop_p >= 0.f && drop_p < 1.f) || (drop_p > 0.f && !state)) return DVLP_ERR_SHAPE;
    const int64_t esz = dtype == DVLP_BF16 ? 2 : 4;
    if (((uintptr_t)v % 16) || (vss * esz) % 16 || (vrs * esz) % 16) return DVLP_ERR_SHAPE;
    if (!H) {        // fused route
        if (!dvlp_qa_attend_fused(dtype, G)) return DVLP_ERR_UNSUPPORTED;
        if (!Wvb || ((uintptr_t)Wvb % 16)) return DVLP_ERR_SHAPE;
    } else if ((uintptr_t)H % 16) return DVLP_ERR_SHAPE;
    a.B = (int)B; a.G = (int)G; a.tiles = (int)cdiv(G, QA_TILE); a.vss = vss; a.vrs = vrs; a.hrows = hrows; a.v = v; a.mask = mask;
    a.Wvb = (const bf16*)Wvb; a.H = H;
    a.thr = drop_p > 0.f ? qa_drop_threshold(drop_p) : 0u;
    a.scale = 1.f / (1.f - drop_p);
    a.state = (const uint32_t*)state;
    return DVLP_OK;
}

// the tile kernels take 140 KB of dynamic LDS: raise the limit once per DEVICE (the attribute belongs to the device's copy of the kernel); two
// threads meeting here both set it, which is harmless.  A failure is reported by the caller as a launch error.
static int qa_tile_attr() {
    static std::atomic<bool> done[64];
    int dev = 0;
    if (hipGetDevice(&dev) != hipSuccess) return DVLP_ERR_LAUNCH;
    const bool track = dev >= 0 && dev < 64;
    if (track && done[dev].load(std::memory_order_acquire)) return DVLP_OK;
    if (hipFuncSetAttribute((const void*)qa_tile_kernel<false>, hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024) != hipSuccess ||
        hipFuncSetAttribute((const void*)qa_tile_kernel<true>, hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024) != hipSuccess)
        { (void)dvlp_launch_status(); return DVLP_ERR_LAUNCH; }
    if (track) done[dev].store(true, std::memory_order_release);
    return DVLP_OK;
}

extern "C" int dvlp_qa_attend_fwd(int dtype, int64_t B, int64_t G, const void* v, int64_t v_sample_stride, int64_t v_row_stride, const float* mask,
                                  const float* q, const float* Wq, const float* bq, const void* Wv_bf16, const float* bv, const float* wl, const float* bl,
                                  const void* H, int64_t hrows, float drop_p, const void* drop_state, int site, void* state_snapshot, float* qp, float* att,
                                  float* pooled, void* stream) {
    QaArgs a{};
    const int rc = qa_common(a, dtype, B, G, v, v_sample_stride, v_row_stride, mask, Wv_bf16, H, hrows, drop_p, drop_state);
    if (rc != DVLP_OK) return rc;
    if (!q || !Wq || !bq || !bv || !wl || !bl || !qp || !att || !pooled || (drop_p > 0.f && !state_snapshot)) return DVLP_ERR_SHAPE;
    if (((uintptr_t)q | (uintptr_t)Wq | (uintptr_t)bv | (uintptr_t)wl | (uintptr_t)qp) % 16) return DVLP_ERR_SHAPE;
    a.q = q; a.Wq = Wq; a.bq = bq; a.bv = bv; a.wl = wl; a.bl = bl; a.qp = qp; a.att = att; a.pooled = pooled;
    a.snap = (uint32_t*)state_snapshot; a.site = (uint32_t)site;
    hipStream_t st = (hipStream_t)stream;
    dvlp_clear_status();
    hipLaunchKernelGGL(qa_qproj_kernel, dim3((unsigned)B), dim3(256), 0, st, a);
    const dim3 grid((unsigned)a.tiles, (unsigned)B);
    if (!H) {
        if (qa_tile_attr() != DVLP_OK) return DVLP_ERR_LAUNCH;
        hipLaunchKernelGGL(qa_tile_kernel<false>, grid, dim3(256), QA_TILE_LDS, st, a);
    } else if (dtype == DVLP_BF16) {
        hipLaunchKernelGGL((qa_rows_kernel<bf16, false>), grid, dim3(256), 0, st, a);
    } else {
        hipLaunchKernelGGL((qa_rows_kernel<float, false>), grid, dim3(256), 0, st, a);
    }
    if (dtype == DVLP_BF16) hipLaunchKernelGGL(qa_softmax_pool_kernel<bf16>, dim3((unsigned)B), dim3(1024), 0, st, a);
    else hipLaunchKernelGGL(qa_softmax_pool_kernel<float>, dim3((unsigned)B), dim3(1024), 0, st, a);
    return dvlp_launch_status();
}

extern "C" int dvlp_qa_attend_bwd(int dtype, int64_t B, int64_t G, const void* v, int64_t v_sample_stride, int64_t v_row_stride, const float* mask,
                                  const float* q, const float* Wq, const void* Wv_bf16, const float* bv, const float* wl, const void* H, int64_t hrows,
                                  float drop_p, const void* state_snapshot, int site, const float* qp, const float* att, const float* d_pooled, void* dv,
                                  void* dH, float* dq, float* dWq, float* dbq, float* dbv, float* dwl, float* dbl, float* workspace, void* stream) {
    QaArgs a{};
    const int rc = qa_common(a, dtype, B, G, v, v_sample_stride, v_row_stride, mask, Wv_bf16, H, hrows, drop_p, state_snapshot);
    if (rc != DVLP_OK) return rc;
    if (!q || !Wq || !bv || !wl || !qp || !att || !d_pooled || !dv || !dH || !dq || !dWq || !dbq || !dbv || !dwl || !dbl || !workspace) return DVLP_ERR_SHAPE;
    if (((uintptr_t)q | (uintptr_t)Wq | (uintptr_t)bv | (uintptr_t)wl | (uintptr_t)qp | (uintptr_t)d_pooled | (uintptr_t)dv | (uintptr_t)dH | (uintptr_t)workspace) % 16)
        return DVLP_ERR_SHAPE;
    a.q = q; a.Wq = Wq; a.bv = bv; a.wl = wl; a.qp = const_cast<float*>(qp); a.att = const_cast<float*>(att); a.dpooled = d_pooled;
    a.snap = (uint32_t*)const_cast<void*>(state_snapshot); a.site = (uint32_t)site;
    a.dv = dv; a.dH = dH; a.dq = dq; a.dWq = dWq; a.dbq = dbq; a.dbv = dbv; a.dwl = dwl; a.dbl = dbl;
    const int64_t pt = B * a.tiles * QA_D;
    a.dlog = workspace; a.dblp = a.dlog + B * G; a.pS = a.dblp + B; a.pBv = a.pS + pt; a.dqpre = a.pBv + pt;
    hipStream_t st = (hipStream_t)stream;
    dvlp_clear_status();
    if (dtype == DVLP_BF16) hipLaunchKernelGGL(qa_pool_bwd_kernel<bf16>, dim3((unsigned)B), dim3(1024), 0, st, a);
    else hipLaunchKernelGGL(qa_pool_bwd_kernel<float>, dim3((unsigned)B), dim3(1024), 0, st, a);
    const dim3 grid((unsigned)a.tiles, (unsigned)B);
    if (!H) {
        if (qa_tile_attr() != DVLP_OK) return DVLP_ERR_LAUNCH;
        hipLaunchKernelGGL(qa_tile_kernel<true>, grid, dim3(256), QA_TILE_LDS, st, a);
    } else if (dtype == DVLP_BF16) {
        hipLaunchKernelGGL((qa_rows_kernel<bf16, true>), grid, dim3(256), 0, st, a);
    } else {
        hipLaunchKernelGGL((qa_rows_kernel<float, true>), grid, dim3(256), 0, st, a);
    }
    hipLaunchKernelGGL(qa_finish_sample_kernel, dim3((unsigned)B), dim3(256), 0, st, a);
    hipLaunchKernelGGL(qa_finish_params_kernel, dim3(QA_D + 1), dim3(256), 0, st, a);
    return dvlp_launch_status();
}

extern "C" int dvlp_softmax_xent(int64_t B, int64_t C, const float* logits, const void* labels, float* loss_rows, float* dlogits, void* pred,
                                 float* loss, void* stream) {
    if (B <= 0 || C <= 0 || B > 0x7fffffff || C > 0x7fffffff || !logits || !labels || !loss_rows || !pred || !loss) return DVLP_ERR_SHAPE;
    dvlp_clear_status();
    hipLaunchKernelGGL(softmax_xent_kernel, dim3((unsigned)B), dim3(256), 0, (hipStream_t)stream, C, 1.f / (float)B, logits, (const int64_t*)labels, loss_rows,
                       dlogits, (int*)pred);
    hipLaunchKernelGGL(xent_mean_kernel, dim3(1), dim3(64), 0, (hipStream_t)stream, B, loss_rows, loss);
    return dvlp_launch_status();
}
