// What dvlp_gemm launches, decided as a pure function of the problem, the developer switches, the registered split-K workspace, the CU count
// and the stream hint.  Plain C++17 host arithmetic: no HIP header, no global, no static, no environment read -- gemm.hip looks the inputs up,
// asks gemm_plan() and launches from the answer; dvlp_dev_gemm_plan() (developer library) hands the same answer to tests without a GPU.
#pragma once
#include <cstdint>

namespace gp {
// (mirrors of common.h / gemm.hip constants, pinned there by static_assert: this header must not include a HIP header)
constexpr int F32 = 0, BF16 = 1, ERR_DTYPE = -1, ERR_SHAPE = -2;
constexpr int GELU = 1, GELU_BWD = 2, RELU_BWD = 4, ACCUM = 8, OUT_F32 = 32;
constexpr int BM = 128, BN = 128, BK = 64;                                        // tile of the fp32 and the 128-row bf16 kernels; K tile
constexpr int EK_ANY = 4;                                                         // epilogue kind "run-time flags" of the 256-column kernel
constexpr int LDS_128 = 69632, LDS_WIDE = 3 * (256 + 128) * 128, LDS_P8 = 139264; // dynamic LDS bytes per family
static inline int64_t cdiv(int64_t a, int64_t b) { return (a + b - 1) / b; }
}

// Developer switches of the GEMM path (include/demovlp_hip_dev.h; defaults = what the product library runs with, nothing can write them there).
struct GemmKnobs {
    int ablate = 0;                // tools/gemm_bench.py --ablate: 1 skip LDS-DMA issue, 2 skip LDS fragment reads, 4 skip MFMAs (TIMING ONLY)
    bool use_glds = true;          // A/B switch between the LDS-DMA kernel (default) and the register-staged one (tools/gemm_bench.py --variant)
    int wide_mode = 0;             // 0: never use the 256-row tile (default: measured no faster on this path's shapes), 1: heuristic, 2: always
    int p8_mode = 1;               // 256 x 256 ping-pong kernel: 0 never, 1 where the grid suits it, 2 whenever the operands allow
    int p8_short = 1;              // 224-row tiles of the 256-row kernel: 0 never, 1 where they save CU-rounds (default), 2 whenever allowed
    int p8_persist = 1;            // persistent form of the 256-row kernel on multi-round outputs: 0 off, 1 on (default; A/B: tools/p8p_bench.py)
    int rb = 1;                    // resident-B streaming kernel (csrc/gemm_rb.hip) for batched skinny products: 0 never, 1 where its shapes fit (default)
    int force_split = 0;           // dvlp_gemm: 0 = automatic K split, > 0 = forced (A/B measurements: tools/gemm_sweep.py)
    int64_t splitk_target = 768;   // workgroups a split-K launch aims for (tools/gemm_bench.py --splitk-target)
    int corun_split = 0;           // 1 = a launch on a co-running stream is K-split like any other (A/B runs); 0 (default) = it is not split
    int wgrad_ride = 1;            // grouped weight gradients: 1 = an optimizer update handed to dvlp_wgrad_grouped_ex rides on the launch's spare workgroups, 0 = its own launch
    int wgrad_patch = 1;           // grouped weight gradients: 1 = 3 x 3 tile patches pinned to XCDs (operand panels shared through L2), 0 = per-problem tile order
    int wgrad_split = 0;           // grouped weight gradients: 0 = automatic uniform K split, > 0 = forced
    int corun_wgrad_split = 0;     // 1 = a co-running weight-gradient group keeps its K split (A/B runs); 0 (default) = it runs unsplit
};

// What the decision depends on.  Operand pointers enter only as the alignment facts the code derives from them.
struct GemmProblem {
    int dtype, transA, transB;
    int64_t M, N, K, lda, ldb, ldc, ldres, ldaux, batch, strideA, strideB, strideC, strideRes, strideAux;
    int flags;
    float alpha;
    bool has_bias, has_res, has_aux, want_csum;            // want_csum: column sums of the stored output requested (dvlp_gemm_ext::colsum)
    bool a16, b16, c16, res16, aux16, bias16;              // operand base address is a multiple of 16 bytes
};

enum GemmFamily { GEMM_F32 = 0, GEMM_RB = 1, GEMM_REG = 2, GEMM_DMA128 = 3, GEMM_WIDE = 4, GEMM_P8 = 5 };

struct GemmPlan {
    int err;                   // 0, or the status dvlp_gemm returns without launching
    int family;                // GemmFamily; GEMM_P8 with `p8p` is the persistent form
    bool safe;                 // register-staged kernel with bounds-checked loads (ragged operands)
    int mih8;                  // 256-column kernel: tile height 128 + 32 mih8 rows
    int64_t S, kchunk;         // K slices (S > 1: fp32 slabs + splitk_reduce_kernel) and the K range of one slice
    int ek8;                   // epilogue kind of the 256-column kernel (0 plain / split, 1 residual, 2 GELU, 3 GELU backward, EK_ANY run-time flags)
    bool p8p;                  // persistent form
    bool csum_fuse;            // column sums come out of the product's epilogue, through csum_rows partial rows of the deferred-reduction queue
    int64_t csum_rows;
    bool vec, a_vec, b_vec;    // 16-byte epilogue accesses (Epi::vec); fp32 kernel: 16-byte operand loads
    unsigned grid[3], block;   // of the product launch
    int lds;                   // its dynamic LDS bytes
    int64_t ntm, ntn;          // row / column tiles of the chosen family (the kernels take the column count, the persistent form both)
    unsigned reduce_grid;      // S > 1: x dimension of the slab reduction's grid (y = batch)
};

// Shapes the resident-B streaming kernel (csrc/gemm_rb.hip) takes: batched skinny products, B operand resident in LDS.
static inline bool gemm_rb_fits(int transA, int transB, int64_t M, int64_t N, int64_t K, int64_t lda, int64_t ldb, int64_t ldc, int64_t batch,
                                int64_t sA, int64_t sB, int64_t sC, bool aligned16) {
    if (transA || batch < 8 || M < 2048 || N % 8 || K % 8 || N > 288 || K > 288 || lda % 8 || ldb % 8 || ldc % 8 || sA % 8 || sB % 8 || sC % 8) return false;
    if (!aligned16 || M * lda * 2 >= 0x7fffffffll) return false;
    return transB ? N <= 256 : K <= 256;          // (the tile shapes rb_launch is instantiated for)
}

// Tile height x K split of the 256-column kernel for an under-filled or round-quantised output (round 6).  What a block costs is not
// proportional to its rows: per 64-deep K tile ~ (0.55 + 0.0016 rows) us on a lightly filled chip, up to ~1.35x that when every CU streams
// (clock and L2 share), plus a prologue + epilogue of ~ (6 + 0.028 rows) us; a K split adds the slab round trip and the reduction launch
// (~2.5 us + 1.08 us per million output elements and slice).  Constants fitted to tools/tile_sweep.py on MI355X (profiles/r6_tile_sweep.txt:
// M = 6400 / 7712 / 18496 tokens x the eight forward / dX shapes of a layer); the model only has to RANK the candidates.
struct P8Plan { int mih; int64_t S; };
static inline P8Plan p8_plan(int64_t M, int64_t N, int64_t K, int64_t ntn8, int ncu, bool may_split, int64_t ws_bytes) {
    using gp::cdiv;
    const int64_t nk = K / 64;
    P8Plan best{4, 1};
    double best_c = 1e30;
    for (int h = 4; h >= 1; --h) {
        const int64_t rows = 128 + 32 * h, nb1 = cdiv(M, rows) * ntn8;
        for (int64_t S = 1; S <= (may_split ? 4 : 1); ++S) {
            if (S > 1 && (nk < 8 * S || nb1 >= 200 || S * M * N * 4 > ws_bytes)) break;
            const int64_t nb = nb1 * S, rounds = cdiv(nb, ncu);
            const double fill = (double)nb / (double)(rounds * ncu);
            const double crowd = 1.0 + 0.35 * (fill > 0.3 ? (fill - 0.3) / 0.7 : 0.0);
            const double tk = (0.55 + 0.0016 * rows) * crowd, fixed = 6.0 + 0.028 * rows;
            const double c = rounds * ((double)cdiv(nk, S) * tk + fixed) + (S > 1 ? 2.5 + 1.08e-6 * (double)S * (double)M * (double)N : 0.0);
            if (c < best_c * 0.995) { best_c = c; best = P8Plan{h, S}; }        // (ties go to the taller tile / the smaller split: tried first)
        }
    }
    return best;
}

// ws_bytes: size of the split-K workspace registered for the stream (<= 0: none, no K split); ncu: compute units of the device;
// co_running: the stream shares the chip with another stream's kernels (dvlp_stream_hint); rd_queue: the deferred-reduction queue has room for
// fused column sums (the caller plans with true, tries to reserve csum_rows and plans again with false if that fails).
static inline GemmPlan gemm_plan(const GemmProblem& p, const GemmKnobs& kn, int64_t ws_bytes, int ncu, bool co_running, bool rd_queue = true) {
    using gp::cdiv;
    const int64_t M = p.M, N = p.N, K = p.K, batch = p.batch;
    const int flags = p.flags;
    const auto fail = [](int err) { GemmPlan f{}; f.err = err; return f; };      // (nothing but the status is meaningful)
    GemmPlan pl{};
    if (M <= 0 || N <= 0 || K <= 0 || batch <= 0 || batch > 65535) return fail(gp::ERR_SHAPE);
    if ((flags & (gp::GELU | gp::GELU_BWD | gp::RELU_BWD)) && !p.has_aux) return fail(gp::ERR_SHAPE);
    {
        const int64_t cal = (flags & gp::OUT_F32) ? 4 : 8;      // elements per 16 bytes of C
        bool v = (p.ldc % cal == 0) && p.c16 && (p.strideC % cal == 0);
        if (p.has_res) v = v && (p.ldres % 8 == 0) && p.res16 && (p.strideRes % 8 == 0);
        if (p.has_aux) v = v && (p.ldaux % 8 == 0) && p.aux16 && (p.strideAux % 8 == 0);
        if (p.has_bias) v = v && p.bias16;
        pl.vec = v;
    }
    const int64_t ntm = cdiv(M, gp::BM), ntn = cdiv(N, gp::BN);
    if (p.dtype == gp::F32) {
        pl.family = GEMM_F32;
        pl.ntm = ntm; pl.ntn = ntn; pl.block = 256;
        pl.grid[0] = (unsigned)(ntm * ntn); pl.grid[1] = (unsigned)batch; pl.grid[2] = 1;
        pl.a_vec = (p.lda % 4 == 0) && p.a16 && (p.strideA % 4 == 0);
        pl.b_vec = (p.ldb % 4 == 0) && p.b16 && (p.strideB % 4 == 0);
        return pl;
    }
    if (p.dtype != gp::BF16) return fail(gp::ERR_DTYPE);
    // batched skinny product with its B operand resident in LDS (the local loss' per-video / per-caption contractions)
    if (kn.rb && !p.has_bias && !p.has_res && !p.has_aux && flags == 0 && p.alpha == 1.0f && !p.want_csum && !kn.ablate &&
        gemm_rb_fits(p.transA, p.transB, M, N, K, p.lda, p.ldb, p.ldc, batch, p.strideA, p.strideB, p.strideC, p.a16 && p.b16 && p.c16)) {
        pl.family = GEMM_RB;          // (its grid is gemm_rb.hip's business)
        return pl;
    }
    // 16-byte vector loads need 8-element-aligned leading dims and base pointers
    if (p.lda % 8 || p.ldb % 8 || !p.a16 || !p.b16 || p.strideA % 8 || p.strideB % 8) return fail(gp::ERR_SHAPE);
    // the branch-free loader clamps rows: form-K operands need >= 1 row, form-R operands a row count that is a multiple of 8
    const bool safe = (p.transA ? (M % 8 != 0 || M < 8) : false) || (p.transB ? (N % 8 != 0 || N < 8) : false) || K < 8 || K % 8 != 0;
    const bool dma = !safe && kn.use_glds;                // (!safe implies K % 8 == 0; a ragged last K tile is zero-filled)
    // 256 x 256 ping-pong kernel: one workgroup per CU, so it wants >= ~a quarter chip of tiles (or a K long enough to split)
    const int64_t ntm8 = cdiv(M, 256), ntn8 = cdiv(N, 256), tiles8 = ntm8 * ntn8 * batch;
    // ... and outputs that fill its tiles: 288 columns would leave the second 256-wide tile 7/8 empty
    const bool fills8 = 10 * M * N >= 8 * (ntm8 * 256) * (ntn8 * 256);
    // (measured per shape with tools/gemm_sweep.py: a 3-tile weight gradient -- the two 256-wide projections -- runs faster on 384 128-row
    //  blocks than on 96 256-row ones; in the step, with the text tower beside the object tower, its 75 / 300-tile products on the 256-row
    //  kernel -- any round count -- take 1 % off the step although alone they measured slower)
    // (round 6: batched long-K reductions whose output half-fills its tiles -- the local loss' dC^_i [288 x 256] and dQ^_j [104 x 256] products
    //  over K = 6 656 / 18 432, batch 64 -- also run faster here with a 2- / 4-way K split than on the 128-row kernel: 181 -> 132, 162 -> 122,
    //  197 -> 160 us (profiles/r6_loss_reductions_on_p8.txt); a [104 x 104] output does not: 108 -> 132)
    const bool longk8 = batch >= 8 && K >= 4096 && N % 256 == 0 && 10 * M >= 4 * ntm8 * 256;
    const bool p8 = dma && K % gp::BK == 0 && kn.p8_mode != 0 &&
                    (kn.p8_mode == 2 || longk8 || (M >= 256 && N >= 256 && fills8 && (tiles8 >= 64 || (tiles8 >= 8 && K >= 4096))));
    // Under-filled grids with a long reduction (weight gradients: 36-144 output tiles, K = B*N tokens) are split along
    // K so that ~3 workgroups (128-row kernel) or 1 workgroup (256-row kernel) land on every CU; partials go through fp32
    // slabs (deterministic, no float atomics).
    int64_t S = 1;
    const int64_t tiles = p8 ? tiles8 : ntm * ntn * batch;
    const bool has_ws = ws_bytes > 0;
    // tile height (p8_tile_rows) and K split of the 256-column kernel, chosen TOGETHER where every tile takes a whole-tile store (row-major
    // A, whole 256-column tiles, aligned outputs; a split launch writes slabs, which any height can): p8_plan above.  M = 18496: 224-row
    // tiles (83 x {3, 9, 12} = 249 / 747 / 996 blocks fill 1 / 3 / 4 rounds of 256 CUs that 256-row tiles leave 14 % empty); M = 6400
    // (the text tower): 160-row tiles (120 / 480 blocks instead of 75 / 300), K >= 2304 as 160 rows x 2 slices instead of 256 x 3.
    int mih8 = 4;
    const bool plan8 = p8 && kn.p8_short != 0 && !p.transA && batch == 1 && N % 256 == 0 && pl.vec && (N & 3) == 0;
    // A co-running launch is not helped by finishing its own grid in fewer rounds (the other stream fills the CUs it leaves idle); what counts
    // is CU-time per FLOP, i.e. the tallest tiles: round 5's rule (256 / 224 rows) instead of the latency planner, and no K split -- slabs and a
    // reduction launch buy latency it does not need with CU-time the other stream does (kn.corun_split restores the split for A/B runs)
    const bool co_run = plan8 && kn.p8_short == 1 && co_running;
    if (plan8 && kn.p8_short == 1 && kn.force_split == 0 && !co_run) {
        const P8Plan pp = p8_plan(M, N, K, ntn8, ncu, has_ws && K >= 1024, ws_bytes);
        mih8 = pp.mih; S = pp.S;
    } else {
        if (has_ws && tiles < (p8 ? 129 : 200) && K >= 1024 && !(co_run && !kn.corun_split)) {
            S = p8 ? 256 / tiles : (kn.splitk_target + tiles - 1) / tiles;
            if (S > K / 256) S = K / 256;
            if (S > 32) S = 32;
            while (S > 1 && S * batch * M * N * 4 > ws_bytes) --S;
        }
        if (kn.force_split > 0 && has_ws) { S = kn.force_split; while (S > 1 && S * batch * M * N * 4 > ws_bytes) --S; }
        if (plan8) {           // developer switches: a forced height (10 + MIH), "224 wherever allowed" (2), round 5's rule (3)
            if (kn.p8_short >= 10) mih8 = kn.p8_short - 10 >= 1 && kn.p8_short - 10 <= 4 ? kn.p8_short - 10 : 4;
            else if (kn.p8_short == 2) mih8 = 3;
            else if ((kn.p8_short == 3 || co_run) && S == 1 && cdiv(cdiv(M, 224) * ntn8, ncu) * 224 < cdiv(tiles8, ncu) * 256) mih8 = 3;
        }
    }
    const int64_t kchunk = cdiv(cdiv(K, S), gp::BK) * gp::BK;
    S = cdiv(K, kchunk);
    // wide (256 x 128) tiles when they still give every CU at least ~2 workgroups; A form R needs M % 8 (guaranteed by !safe)
    const int64_t ntm_w = cdiv(M, 256);
    const bool wide = dma && !p8 && kn.wide_mode != 0 && (kn.wide_mode == 2 || ntm_w * ntn * batch * S >= 512);
    // epilogue kind of the 256-row kernel (see p8_tile)
    const int fmask8 = flags & (gp::GELU | gp::GELU_BWD | gp::RELU_BWD | gp::ACCUM | gp::OUT_F32);
    // (a specialised kind only where every tile is whole: N a multiple of 256 and, unless the launch writes split-K slabs, 16-byte aligned outputs)
    const bool whole8 = N % 256 == 0 && (S > 1 ? N % 4 == 0 : pl.vec);
    const int ek8 = (kn.ablate || !whole8) ? gp::EK_ANY
                    : (S > 1 || fmask8 == 0) ? ((p.has_res && S == 1) ? 1 : 0)
                    : (fmask8 == gp::GELU && !p.has_res) ? 2 : (fmask8 == gp::GELU_BWD && !p.has_res) ? 3 : gp::EK_ANY;
    if (ek8 == gp::EK_ANY && S == 1) mih8 = 4;        // run-time-flag epilogues exist at 256 rows only
    // a many-round product with a very short K (the local loss' S = C^ Q^^T: 1 872 tiles of 4 K tiles each) is all prologue and epilogue: the
    // persistent form (224-row tiles only) hides them behind the neighbouring tiles' K loops -- 105 -> 91.5 us -- whatever the planner's height
    const int64_t nk = K / gp::BK;
    if (plan8 && kn.p8_short == 1 && kn.p8_persist != 0 && S == 1 && (ek8 == 0 || ek8 == 2) && nk >= 4 && nk <= 8 && nk % 2 == 0 &&
        cdiv(M, 224) * ntn8 > 2 * ncu) mih8 = 3;
    const int64_t ntm8h = cdiv(M, 128 + 32 * mih8);
    // column sums from the epilogue: partial rows per (row tile, upper / lower wave group)
    pl.csum_fuse = p.want_csum && p8 && batch == 1 && S == 1 && pl.vec && N % 256 == 0 && !(flags & gp::OUT_F32) && rd_queue;
    pl.csum_rows = 2 * ntm8h;
    // persistent form: more than one round of whole tiles, an even number (>= 4) of K tiles, a specialised epilogue, no fused column sums
    // (residual / aux-in epilogues: the compiler closes their loads with vmcnt(0) inside the tile loop)
    pl.p8p = p8 && kn.p8_persist != 0 && mih8 == 3 && M * p.lda < (1ll << 31) && N * p.ldb < (1ll << 31) && K * p.ldb < (1ll << 31) && !p.transA && S == 1 &&
             batch == 1 && ntm8h * ntn8 > ncu && N % 256 == 0 && pl.vec && p.alpha == 1.0f && nk % 2 == 0 && nk >= 4 && (ek8 == 0 || ek8 == 2) && !pl.csum_fuse;
    pl.family = p8 ? GEMM_P8 : wide ? GEMM_WIDE : dma ? GEMM_DMA128 : GEMM_REG;
    pl.safe = safe; pl.mih8 = mih8; pl.S = S; pl.kchunk = kchunk; pl.ek8 = ek8;
    pl.ntm = ntm; pl.ntn = ntn; pl.block = 256; pl.lds = gp::LDS_128;
    pl.grid[0] = (unsigned)(ntm * ntn); pl.grid[1] = (unsigned)batch; pl.grid[2] = (unsigned)S;
    if (p8) {
        pl.ntm = ntm8h; pl.ntn = ntn8; pl.block = 512; pl.lds = gp::LDS_P8;
        pl.grid[0] = pl.p8p ? (unsigned)ncu : (unsigned)(ntm8h * ntn8);
    } else if (wide) {
        pl.ntm = ntm_w; pl.block = 512; pl.lds = gp::LDS_WIDE;
        pl.grid[0] = (unsigned)(ntm_w * ntn);
    }
    if (S > 1) pl.reduce_grid = (unsigned)cdiv(M * cdiv(N, 8), 256);
    return pl;
}
