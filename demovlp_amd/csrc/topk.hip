// Row top-k (no reference counterpart: the reference ranks on the host, in numpy): per row of an fp32 matrix the K largest values in
// descending order with their column numbers -- the device half of text-to-video search (demovlp_amd/search.py): the shortlist of the
// global stage and the final cut after the re-rank.
//
// Order.  Every candidate becomes one 64-bit word  (key << 32) | ~index : `key` is the float mapped to an unsigned that sorts like it
// (-0.0 folded onto +0.0, NaN = 1: below -inf, above nothing but a filler), `index` the column number + index_base, so a LARGER word is
// "larger value, then smaller index": np.argsort(-x, kind="stable").  Indices are unique, hence words are: the top K of a set of words is
// one well-defined list whatever order the set was visited in.  That is the whole determinism argument -- no float atomics, and the only
// order that varies from run to run (which wave appended to the LDS buffer first) permutes a set that is sorted before anyone reads it.
// The raw bits of the value ride along as a payload (the key forgets a zero's sign and a NaN's payload; `val` returns them untouched).
//
// Scan.  A workgroup (256 threads) walks its column segment 1024 columns a round, one 16-byte load per thread with the next round's load
// in flight.  Words above the running threshold (the K-th best so far; 0 = nothing yet) are appended to an LDS buffer of 2048 entries;
// when another round might not fit, the buffer is sorted (bitonic, in LDS) and cut to K, which raises the threshold.  After the first cut
// a survivor is rare (K / columns seen), so most rounds cost their loads, a compare and two barriers.
//
// Small M.  Below ~512 rows each row is split into column segments (TopkPlan) so that the launch fills the chip: workgroup (m, s) writes its
// sorted K-list to the workspace and topk_merge_kernel -- one workgroup per row, the same selector fed from lists instead of columns --
// picks the row's K out of the S lists.  merge = 1 adds the K entries already in val / idx as one more list: the same pass, so chunked
// calls equal the one-shot call bit for bit.
//
// Mask.  dvlp_topk_rows_masked is the same scan with an allow bit per GLOBAL column (index_base + column): a disallowed column offers word 0,
// so it is deleted, not merely ranked last -- it can neither be listed nor raise the threshold.  The merge pass is unchanged.
#include "common.h"

constexpr int TK_THREADS = 256, TK_ROUND = 4 * TK_THREADS, TK_MAXK = 1024, TK_CAP = TK_MAXK + TK_ROUND, TK_MAXSEG = 256;
constexpr unsigned TK_NEG_INF = 0xff800000u;

typedef unsigned long long u64;

struct TopkSel {
    u64 word[TK_CAP];
    unsigned raw[TK_CAP];
    int cnt;
    u64 thr;
};

__device__ __forceinline__ unsigned tk_key(unsigned u) {
    if ((u & 0x7fffffffu) > 0x7f800000u) return 1u;            // NaN: after every number
    if (u == 0x80000000u) u = 0u;                               // -0.0 == +0.0
    return (u & 0x80000000u) ? ~u : (u | 0x80000000u);          // -inf -> 0x007fffff ... +inf -> 0xff800000
}
__device__ __forceinline__ u64 tk_word(unsigned rawbits, int index) { return ((u64)tk_key(rawbits) << 32) | (u64)(0xffffffffu - (unsigned)index); }

// descending bitonic sort of the first n2 (power of two >= cnt) entries, then the cut to K
__device__ __forceinline__ void tk_sort_cut(TopkSel& s, int K) {
    const int tid = threadIdx.x;
    const int cnt = s.cnt;                                      // (uniform: read between two barriers)
    int n2 = 2;
    while (n2 < cnt) n2 <<= 1;
    for (int t = cnt + tid; t < n2; t += TK_THREADS) { s.word[t] = 0ull; s.raw[t] = TK_NEG_INF; }
    __syncthreads();
    for (int k = 2; k <= n2; k <<= 1) {
        for (int j = k >> 1; j > 0; j >>= 1) {
            for (int t = tid; t < (n2 >> 1); t += TK_THREADS) {
                const int i = ((t & ~(j - 1)) << 1) | (t & (j - 1)), p = i | j;
                const u64 a = s.word[i], b = s.word[p];
                const bool desc = (i & k) == 0;
                if (desc ? a < b : a > b) {
                    s.word[i] = b; s.word[p] = a;
                    const unsigned ra = s.raw[i]; s.raw[i] = s.raw[p]; s.raw[p] = ra;
                }
            }
            __syncthreads();
        }
    }
    if (tid == 0) {
        if (cnt >= K) { s.cnt = K; s.thr = s.word[K - 1]; }
    }
    __syncthreads();
}

// One round: every thread offers up to 4 (word, raw) candidates (word 0 = none).  Uniform control flow; two barriers.
__device__ __forceinline__ void tk_offer(TopkSel& s, int K, const u64 (&w)[4], const unsigned (&r)[4]) {
    const u64 thr = s.thr;
    int n = 0;
#pragma unroll
    for (int e = 0; e < 4; ++e) n += w[e] > thr;
    if (n) {
        int pos = atomicAdd(&s.cnt, n);                         // integer, in LDS: places entries, never decides which survive
#pragma unroll
        for (int e = 0; e < 4; ++e)
            if (w[e] > thr) { s.word[pos] = w[e]; s.raw[pos] = r[e]; ++pos; }
    }
    __syncthreads();
    const bool full = s.cnt > TK_CAP - TK_ROUND;
    __syncthreads();
    if (full) tk_sort_cut(s, K);
}

__device__ __forceinline__ void tk_init(TopkSel& s) {
    if (threadIdx.x == 0) { s.cnt = 0; s.thr = 0ull; }
    __syncthreads();
}

// final sort, then K entries out (raw value bits, index); short lists end in (-inf, -1)
__device__ __forceinline__ void tk_emit(TopkSel& s, int K, unsigned* __restrict__ oval, int* __restrict__ oidx) {
    tk_sort_cut(s, K);
    const int cnt = s.cnt < K ? s.cnt : K;
    for (int t = threadIdx.x; t < K; t += TK_THREADS) {
        const u64 w = t < cnt ? s.word[t] : 0ull;
        oval[t] = w ? s.raw[t] : TK_NEG_INF;
        oidx[t] = w ? (int)(0xffffffffu - (unsigned)(w & 0xffffffffull)) : -1;
    }
}

// workgroup (m, s): columns [s seg, min(N, (s + 1) seg)) of row m -> list (m, s).  MASKED: column c takes part iff bit (index_base + c) & 31 of
// word (index_base + c) >> 5 of the row's allow mask is set; a disallowed column offers word 0 ("none"), like a column beyond N.  A thread's
// four columns are consecutive, so their bits sit in one or two words: those of its first and last column inside [lo, hi), fetched with the
// 16-byte load (the next round's are in flight with it) and read as one 64-bit field.  Only words (index_base + lo) >> 5 ..
// (index_base + hi - 1) >> 5 are loaded.  The unmasked instantiation is the kernel as it was: every masked line is under `if constexpr`.
struct TopkLoad { f32x4 v; u64 bits; };

template <bool MASKED>
__global__ __launch_bounds__(TK_THREADS) void topk_scan_kernel(int64_t N, const float* __restrict__ x, int64_t ld, int K, int64_t index_base, int S, int64_t seg,
                                                               const unsigned* __restrict__ allow, int64_t allow_ld,
                                                               unsigned* __restrict__ oval, int* __restrict__ oidx) {
    __shared__ TopkSel s;
    const int tid = threadIdx.x;
    const int64_t m = blockIdx.x / S;
    const int sg = (int)(blockIdx.x % S);
    const float* xr = x + m * ld;
    const int64_t lo = (int64_t)sg * seg, hi = lo + seg < N ? lo + seg : N;
    // 16-byte loads: columns c with (c + off) % 4 == 0 sit on 16-byte addresses; the walk starts at the aligned column at or below lo
    const int64_t off = (int64_t)(((uintptr_t)xr >> 2) & 3);
    const int64_t base = lo - ((lo + off) & 3);
    const int64_t rounds = (hi - base + TK_ROUND - 1) / TK_ROUND;
    tk_init(s);
    auto load = [&](int64_t rd) -> TopkLoad {
        const int64_t q = base + rd * TK_ROUND + tid * 4;
        TopkLoad L;
        L.v = f32x4{0.f, 0.f, 0.f, 0.f};
        L.bits = 0ull;
        if (q >= lo && q + 3 < hi) L.v = __builtin_nontemporal_load((const f32x4*)(xr + q));
        else {
#pragma unroll
            for (int e = 0; e < 4; ++e) if (q + e >= lo && q + e < hi) L.v[e] = xr[q + e];
        }
        if constexpr (MASKED) {
            const int64_t c0 = q > lo ? q : lo, c1 = q + 3 < hi ? q + 3 : hi - 1;      // the thread's columns inside [lo, hi)
            if (c0 <= c1) {
                const unsigned* ar = allow + m * allow_ld;
                const int64_t w0 = (index_base + c0) >> 5, w1 = (index_base + c1) >> 5;
                const unsigned a0 = ar[w0];
                L.bits = (u64)a0 | ((u64)(w1 != w0 ? ar[w1] : a0) << 32);
            }
        }
        return L;
    };
    TopkLoad cur = load(0);
    for (int64_t rd = 0; rd < rounds; ++rd) {
        TopkLoad nxt;
        nxt.v = f32x4{0.f, 0.f, 0.f, 0.f};
        nxt.bits = 0ull;
        if (rd + 1 < rounds) nxt = load(rd + 1);
        const int64_t q = base + rd * TK_ROUND + tid * 4;
        u64 w[4]; unsigned r[4];
        [[maybe_unused]] const int64_t bit0 = ((index_base + (q > lo ? q : lo)) >> 5) << 5;      // global column of bit 0 of cur.bits
#pragma unroll
        for (int e = 0; e < 4; ++e) {
            r[e] = __float_as_uint(cur.v[e]);
            bool in = q + e >= lo && q + e < hi;
            if constexpr (MASKED) in = in && ((cur.bits >> (int)((index_base + q + e - bit0) & 63)) & 1ull);      // (in range: 0 .. 34)
            w[e] = in ? tk_word(r[e], (int)(index_base + q + e)) : 0ull;
        }
        tk_offer(s, K, w, r);
        cur = nxt;
    }
    const int64_t o = (int64_t)blockIdx.x * K;
    tk_emit(s, K, oval + o, oidx + o);
}

// workgroup m: the S lists of row m (+ the K entries already in val / idx when merge) -> val / idx of row m
__global__ __launch_bounds__(TK_THREADS) void topk_merge_kernel(int K, int S, int merge, const unsigned* __restrict__ lval, const int* __restrict__ lidx,
                                                                unsigned* __restrict__ val, int* __restrict__ idx) {
    __shared__ TopkSel s;
    const int tid = threadIdx.x;
    const int64_t m = blockIdx.x;
    const unsigned* lv = lval + m * S * K;
    const int* li = lidx + m * S * K;
    unsigned* ov = val + m * K;
    int* oi = idx + m * K;
    const int n_list = S * K, total = n_list + (merge ? K : 0);
    tk_init(s);
    for (int t0 = 0; t0 < total; t0 += TK_ROUND) {
        u64 w[4]; unsigned r[4];
#pragma unroll
        for (int e = 0; e < 4; ++e) {
            const int t = t0 + e * TK_THREADS + tid;
            int ix = -1; unsigned rv = TK_NEG_INF;
            if (t < n_list) { ix = li[t]; rv = lv[t]; }
            else if (t < total) { ix = oi[t - n_list]; rv = ov[t - n_list]; }
            r[e] = rv;
            w[e] = ix >= 0 ? tk_word(rv, ix) : 0ull;               // fillers of short lists (index -1) take no part
        }
        tk_offer(s, K, w, r);                                       // (the barriers inside order the reads of val / idx before tk_emit's writes)
    }
    tk_emit(s, K, ov, oi);
}

// rows below ~2 workgroups per CU are split into S <= 256 column segments of `seg` columns (a multiple of the round)
struct TopkPlan { int S; int64_t seg; };
static TopkPlan topk_plan(int64_t M, int64_t N, int K) {
    int64_t want = cdiv(512, M);
    const int64_t most = cdiv(N, 4 * TK_ROUND);                     // at least four rounds per segment
    int64_t cap = 32768 / K;                                        // the merge pass is one workgroup per row: bound its S K candidates
    cap = cap < 16 ? 16 : (cap > TK_MAXSEG ? TK_MAXSEG : cap);
    if (want > most) want = most;
    if (want > cap) want = cap;
    if (want < 1) want = 1;
    TopkPlan P;
    P.seg = cdiv(cdiv(N, want), TK_ROUND) * TK_ROUND;
    P.S = (int)cdiv(N, P.seg);
    return P;
}

static int topk_check(int64_t M, int64_t N, int K) {
    if (M < 1 || N < 1 || N >= (1ll << 31) || K < 1 || K > TK_MAXK) return DVLP_ERR_SHAPE;
    if (M * (int64_t)topk_plan(M, N, K).S > INT32_MAX) return DVLP_ERR_SHAPE;
    return DVLP_OK;
}

extern "C" int64_t dvlp_topk_workspace_bytes(int64_t M, int64_t N, int K) {
    const int rc = topk_check(M, N, K);
    if (rc != DVLP_OK) return rc;
    return M * topk_plan(M, N, K).S * K * 8;
}

static int topk_launch(int64_t M, int64_t N, const float* x, int64_t ld, int K, int64_t index_base, const unsigned* allow, int64_t allow_ld, bool masked,
                       float* val, int* idx, int merge, void* workspace, void* stream) {
    dvlp_clear_status();
    const int rc = topk_check(M, N, K);
    if (rc != DVLP_OK) return rc;
    if (ld < N || index_base < 0 || index_base + N > INT32_MAX || (merge != 0 && merge != 1)) return DVLP_ERR_SHAPE;
    if (!x || !val || !idx || !workspace || ((uintptr_t)x & 3)) return DVLP_ERR_SHAPE;
    // a mask row holds the bits of global columns 0 .. index_base + N - 1: allow_ld = 0 (one row for all) or at least that many words
    if (masked && (!allow || ((uintptr_t)allow & 3) || allow_ld < 0 || (allow_ld != 0 && allow_ld < (index_base + N + 31) / 32))) return DVLP_ERR_SHAPE;
    const TopkPlan P = topk_plan(M, N, K);
    hipStream_t st = (hipStream_t)stream;
    const bool direct = P.S == 1 && !merge;
    unsigned* lval = (unsigned*)workspace;
    int* lidx = (int*)((char*)workspace + M * P.S * K * 4);
    const dim3 grid((unsigned)(M * P.S)), block(TK_THREADS);
    if (masked)
        hipLaunchKernelGGL(topk_scan_kernel<true>, grid, block, 0, st, N, x, ld, K, index_base, P.S, P.seg, allow, allow_ld,
                           direct ? (unsigned*)val : lval, direct ? idx : lidx);
    else
        hipLaunchKernelGGL(topk_scan_kernel<false>, grid, block, 0, st, N, x, ld, K, index_base, P.S, P.seg, (const unsigned*)nullptr, (int64_t)0,
                           direct ? (unsigned*)val : lval, direct ? idx : lidx);
    if (!direct)
        hipLaunchKernelGGL(topk_merge_kernel, dim3((unsigned)M), dim3(TK_THREADS), 0, st, K, P.S, merge, lval, lidx, (unsigned*)val, idx);
    return dvlp_launch_status();
}

// x [M][ld] fp32 (first N columns) -> val [M][K] fp32, idx [M][K] int32; workspace: dvlp_topk_workspace_bytes(M, N, K)
extern "C" int dvlp_topk_rows(int64_t M, int64_t N, const float* x, int64_t ld, int K, int64_t index_base, float* val, int* idx, int merge,
                              void* workspace, void* stream) {
    return topk_launch(M, N, x, ld, K, index_base, nullptr, 0, false, val, idx, merge, workspace, stream);
}

// the same with disallowed columns deleted: column c of row m takes part iff bit (index_base + c) & 31 of allow[m allow_ld + ((index_base + c) >> 5)]
// is set (allow_ld = 0: one mask row for all M rows).  Entries merged in from val / idx passed the mask when they were selected.
extern "C" int dvlp_topk_rows_masked(int64_t M, int64_t N, const float* x, int64_t ld, int K, int64_t index_base, const uint32_t* allow, int64_t allow_ld,
                                     float* val, int* idx, int merge, void* workspace, void* stream) {
    return topk_launch(M, N, x, ld, K, index_base, allow, allow_ld, true, val, idx, merge, workspace, stream);
}
