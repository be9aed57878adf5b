// Moment selection (no reference counterpart: moment search has none): greedy temporal non-maximum suppression over the window scores of a
// (query, video) pair -- the device half of "where, in which video, does this happen" (demovlp_amd/search.py).  It sits beside
// the row top-k of topk.hip: that one ranks columns that are independent of each other, this one ranks windows that overlap in time, where
// the runner-up of a row is almost always the winner shifted by a frame.
//
// Definition, per row of scores [P][ld] (first M columns; window c covers the frames [start[c], start[c] + length[c])).  A window is
// selectable while it is alive and its score is neither NaN nor -inf.  T times: take the selectable window that is largest in the order of
// topk.hip (by value with -0.0 folded onto +0.0, then by smaller position), write its raw value bits and its position, kill it, and kill every
// alive window c' with  float(inter) > float(union) * iou,  inter = max(0, min(e, e') - max(s, s')), union = len + len' - inter in integers
// and the right-hand side ONE fp32 multiply.  When nothing selectable is left the remaining entries are (pad, -1): pad = the quiet NaN
// 0x7fc00000 if the row holds a NaN anywhere in its M columns, -inf otherwise.  iou = 0: any overlap suppresses; iou = 1: nothing but the
// selected window is suppressed (inter <= union), which is plain top-T.
//
// Layout.  One wavefront per row, four rows per 256-thread workgroup; start / length are staged in LDS once per workgroup (2 M ints, dynamic).
// Lane l keeps the candidates c = 64 j + l, j < NC = ceil(M / 64) rounded up to a power of two, as raw bits in registers with an alive bit
// each, so the row is loaded once, coalesced.  A round is: the lane-local maximum over the alive candidates (ascending j is ascending
// position, so a strict compare on the key keeps the smaller position), a wave-wide maximum of the 64-bit word (key << 32) | ~position by
// six xor-shuffles -- words are unique, so the maximum is one well-defined candidate whatever the order of the reduction -- a broadcast of the
// winner's raw bits, its (start, length) read from LDS at one address, and the per-lane suppression.  Lane t keeps the t-th result and the
// wave writes val / pos [T] with one store each at the end.  No workspace, no atomics of any kind: two runs give equal bytes.
#include "common.h"

#include <type_traits>

constexpr int MS_WAVES = 4, MS_THREADS = 64 * MS_WAVES, MS_MAXM = 4096, MS_MAXT = 32;
constexpr unsigned MS_NEG_INF = 0xff800000u, MS_NAN = 0x7fc00000u;

typedef unsigned long long u64;

// the key of topk.hip (tk_key): the float as an unsigned that sorts like it, -0.0 folded onto +0.0.  A NaN or -inf never gets here.
__device__ __forceinline__ unsigned ms_key(unsigned u) {
    if (u == 0x80000000u) u = 0u;
    return (u & 0x80000000u) ? ~u : (u | 0x80000000u);          // -FLT_MAX -> 0x00800000 ... +inf -> 0xff800000: never 0
}

template <int NC>
__global__ __launch_bounds__(MS_THREADS) void moment_select_kernel(int64_t P, int M, const float* __restrict__ scores, int64_t ld, const int* __restrict__ start,
                                                                   const int* __restrict__ length, int T, float iou, unsigned* __restrict__ val,
                                                                   int* __restrict__ pos) {
    using mask_t = typename std::conditional<(NC <= 32), unsigned, u64>::type;
    extern __shared__ int ms_win[];                             // start [M], length [M]
    int* ws = ms_win;
    int* wl = ms_win + M;
    const int lane = threadIdx.x & 63;
    const int64_t row = (int64_t)blockIdx.x * MS_WAVES + (threadIdx.x >> 6);
    const bool live = row < P;                                  // (whole waves of the ragged last workgroup are not)
    const float* x = scores + (live ? row : 0) * ld;
    unsigned raw[NC];
#pragma unroll
    for (int j = 0; j < NC; ++j) {                              // the row's loads are in flight while the windows are staged
        const int c = j * 64 + lane;
        raw[j] = (live && c < M) ? __float_as_uint(x[c]) : MS_NEG_INF;      // columns [M, ld) are never read
    }
    for (int c = threadIdx.x; c < M; c += MS_THREADS) { ws[c] = start[c]; wl[c] = length[c]; }
    __syncthreads();
    if (!live) return;                                          // (no barrier follows)
    mask_t alive = 0;
    bool nan = false;
#pragma unroll
    for (int j = 0; j < NC; ++j) {
        const unsigned u = raw[j];
        const bool isnan = (u & 0x7fffffffu) > 0x7f800000u;
        nan |= isnan;
        if (!isnan && u != MS_NEG_INF) alive |= (mask_t)1 << j;
    }
    unsigned oval = __any(nan) ? MS_NAN : MS_NEG_INF;           // lane t holds entry t: the padding until a round fills it
    int opos = -1;
    for (int t = 0; t < T; ++t) {
        unsigned bk = 0u, br = 0u;                              // key 0: none
        int bc = 0;
#pragma unroll
        for (int j = 0; j < NC; ++j) {
            if ((alive >> j) & 1) {
                const unsigned k = ms_key(raw[j]);
                if (k > bk) { bk = k; br = raw[j]; bc = j * 64 + lane; }
            }
        }
        u64 w = bk ? (((u64)bk << 32) | (u64)(0xffffffffu - (unsigned)bc)) : 0ull;
#pragma unroll
        for (int off = 32; off > 0; off >>= 1) {
            const u64 o = __shfl_xor(w, off);
            w = o > w ? o : w;
        }
        if (w == 0ull) break;                                   // (uniform: every lane holds the wave's maximum)
        const int p = (int)(0xffffffffu - (unsigned)(w & 0xffffffffull));
        const unsigned r = __shfl(br, p & 63);
        if (lane == t) { oval = r; opos = p; }
        const int s = ws[p], l = wl[p], e = s + l;
#pragma unroll
        for (int j = 0; j < NC; ++j) {
            if ((alive >> j) & 1) {
                const int c = j * 64 + lane;                    // (alive: c < M)
                const int s2 = ws[c], l2 = wl[c], e2 = s2 + l2;
                const int hi = e < e2 ? e : e2, lo = s > s2 ? s : s2;
                const int inter = hi > lo ? hi - lo : 0, uni = l + l2 - inter;
                if (c == p || (float)inter > (float)uni * iou) alive &= ~((mask_t)1 << j);
            }
        }
    }
    if (lane < T) {
        val[row * T + lane] = oval;
        pos[row * T + lane] = opos;
    }
}

// scores fp32 [P][ld] (first M columns), start / length int32 [M] on the device (length >= 1, start >= 0, start + length < 2^30: not checked,
// they live on the device) -> val fp32 [P][T], pos int32 [P][T]
extern "C" int dvlp_moment_select(int64_t P, int64_t M, const float* scores, int64_t ld, const int* start, const int* length, int T, float iou,
                                  float* val, int* pos, void* stream) {
    dvlp_clear_status();
    if (P < 0 || M < 1 || T < 1 || ld < M || !(iou >= 0.f && iou <= 1.f)) return DVLP_ERR_SHAPE;
    if (M > MS_MAXM || T > MS_MAXT) return DVLP_ERR_UNSUPPORTED;
    if (P * (ld > T ? ld : (int64_t)T) >= (1ll << 31)) return DVLP_ERR_SHAPE;
    if (!scores || !start || !length || !val || !pos) return DVLP_ERR_SHAPE;
    if (((uintptr_t)scores | (uintptr_t)start | (uintptr_t)length | (uintptr_t)val | (uintptr_t)pos) & 3) return DVLP_ERR_SHAPE;
    if (P == 0) return DVLP_OK;
    const dim3 grid((unsigned)cdiv(P, MS_WAVES)), block(MS_THREADS);
    const size_t lds = (size_t)M * 2 * sizeof(int);
    hipStream_t st = (hipStream_t)stream;
    const int nc = (int)cdiv(M, 64);
#define MS_LAUNCH(NC) hipLaunchKernelGGL(moment_select_kernel<NC>, grid, block, lds, st, P, (int)M, scores, ld, start, length, T, iou, (unsigned*)val, pos)
    if (nc <= 1) MS_LAUNCH(1);
    else if (nc <= 2) MS_LAUNCH(2);
    else if (nc <= 4) MS_LAUNCH(4);
    else if (nc <= 8) MS_LAUNCH(8);
    else if (nc <= 16) MS_LAUNCH(16);
    else if (nc <= 32) MS_LAUNCH(32);
    else MS_LAUNCH(64);
#undef MS_LAUNCH
    return dvlp_launch_status();
}
