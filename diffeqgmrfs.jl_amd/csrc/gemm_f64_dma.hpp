// fp64 MFMA GEMM whose operand tiles go global -> LDS WITHOUT passing through registers
// (global_load_lds_dwordx4), round 3.  Same contract as gemm_f64_mfma (gemm_f64.hpp):
//
//   C[m][n] = beta * D[m][n] + alpha * sum_k A[m*lda + k] * b(k,n),   b(k,n) = B_N ? B[k*ldb + n] : B[n*ldb + k]
//
// Why: every instruction that RETURNS data into VGPRs beside the fp64 MFMA stream costs matrix-pipe issue time
// (tools/mb5.hip: ds_read_b128 and global_load_dwordx4 -> VGPR alike), and the register-staged kernel pays, per 32
// MFMAs of a wave, 8 global loads + 8 ds_write_b128 + 16 ds_read_b128.  Here the staging costs no VGPR traffic at
// all (the loads write LDS directly, 1 KiB per wave instruction), and the BM x BN workgroup tile is a template
// parameter: 128 x 64 / 64 x 128 (a wave owns 64 x 32 / 32 x 64 = 8 MFMA tiles: 6 fragment reads per 16 MFMAs instead of
// 4 per 8) for launches whose M / N allow it, 64 x 64 otherwise.
//
// LDS images (K step BK = 16, DMA_STAGES buffers of (BM + BN) * 128 bytes):
//   [row][16] for an operand stored [row][k]: a row is 128 bytes = 8 chunks of 16 bytes; chunk c of row r sits at
//       chunk position c ^ ((r >> 1) & 7).  A wave's ds_read_b128 of one k pair from 16 consecutive rows then touches
//       every bank once (unswizzled, rows 128 bytes apart put every second row on the same banks: 4-way conflicts).
//       global_load_lds writes LDS linearly (wave-uniform base + lane * 16), so the swizzle is applied on the SOURCE
//       side: lane l of the instruction that fills rows 8q .. 8q+7 fetches chunk (l & 7) ^ ((row >> 1) & 7) of row 8q + (l >> 3).
//   [16][BN] as it lies in memory for B stored [k][n] (a 16-lane group reads 256 contiguous bytes: conflict free).
// Pipeline: DMA_STAGES - 1 = one tile is in flight (LDS-DMA) while one is multiplied; a wave waits for ITS OWN requests of tile
// kt with s_waitcnt vmcnt(0), and ONE raw s_barrier per K step both makes
// every wave's part of tile kt visible and frees the buffer of tile kt - 1 for the next request (no __syncthreads: its
// fence would drain the DMA queue).  All LDS is ONE dynamic array (cdna_hip_programming.md: a second __shared__ object makes hipcc
// wait vmcnt(0) before every fragment read).
// Summation order per output element = gemm_f64_mfma's (k ascending in steps of 8, even k then odd k inside a step
// pair ... identical MFMA k-slot assignment), so results are bitwise those of the register-staged kernel.
#pragma once
#include <type_traits>
#include "gemm_f64.hpp"

namespace gmrf {

constexpr int DMA_BK = 16;
constexpr int DMA_STAGES = 2;                // LDS ring: one tile in flight while one is multiplied
constexpr int DMA_ROWS_ASCENDING = 1024;     // GemmArgs::tri bit set by the launcher: triangular grid walked from row tile 0 on

template <int BM, int BN>
constexpr size_t gemm_dma_lds_bytes() { return (size_t)DMA_STAGES * (BM + BN) * DMA_BK * sizeof(double); }

#define GMRF_LDS_PTR(p) ((__attribute__((address_space(3))) void*)(p))
#define GMRF_GLB_PTR(p) ((const __attribute__((address_space(1))) void*)(p))

// Tile order over the 1-D grid: XCD-grouped problems (blockIdx % 8 = group), inside a group longest K first.
// lower_only == 1: triangular grid of BM x BN tiles that touch the lower triangle (M == N).
template <int BM, int BN>
__device__ __forceinline__ void gemm_dma_tile_order(const GemmArgs& g, int bid, int gdim, int& bm, int& bn, int& z) {
    const int nx = g.N / BN, ny = g.M / BM;
    int tpp;
    if (g.lower_only == 1) {
        // row tile bm covers rows [bm BM, (bm + 1) BM): column tiles 0 .. ((bm + 1) BM - 1) / BN
        if (BM >= BN) tpp = (BM / BN) * ny * (ny + 1) / 2;
        else tpp = 0;                                           // (not launched: see launch_gemm_dma)
    } else tpp = nx * ny;
    const int nz = gdim / tpp;
    const int groups = (nz % 8 == 0) ? 8 : 1;
    const int xg = bid % groups, q = bid / groups, nzg = nz / groups;
    int zq;
    if (g.lower_only == 1) {
        constexpr int R = BM / BN > 0 ? BM / BN : 1;            // column tiles per diagonal step
        const int tile = q % tpp;
        zq = q / tpp;
        // tiles of row bm: R (bm + 1); before it: R bm (bm + 1) / 2.  Longest rows first does not matter here (K is
        // the same for all tiles of a rank-k update; G2's staircase bounds grow with bm): rows in descending order.
        // (round 4) with staircase bounds K shrinks as bm grows -- K(bm, bn) = W - kst[bm] for bn <= bm -- so ascending rows ARE
        // longest first, and the descending order used to leave every problem group's longest tile, (0, 0), for the very end
        const int tr = (g.tri & DMA_ROWS_ASCENDING) ? tile : tpp - 1 - tile;
        int b = (int)((sqrtf(8.0f * (float)(tr / R) + 1.0f) - 1.0f) * 0.5f);
        while (R * b * (b + 1) / 2 > tr) --b;
        while (R * (b + 1) * (b + 2) / 2 <= tr) ++b;
        bm = b;
        bn = tr - R * b * (b + 1) / 2;
    } else {
        const bool cls_n = (g.tri & (TRI_B_LOWER | TRI_B_UPPER)) || !(g.tri & (TRI_A_LOWER | TRI_A_UPPER));
        const bool desc = cls_n ? ((g.tri & TRI_B_UPPER) != 0 || (g.ke_n && !g.kb_n)) : (g.tri & TRI_A_LOWER) != 0;
        const int ncls = cls_n ? nx : ny, other = cls_n ? ny : nx;
        int c = q / (other * nzg);
        const int rem = q % (other * nzg);
        const int o = rem % other;
        zq = rem / other;
        if (desc) c = ncls - 1 - c;
        bn = cls_n ? c : o;
        bm = cls_n ? o : c;
    }
    z = xg + groups * zq;
}

// A_T (round 4): A stored [k][m] -- the product A^T B of two operands that both lie [k][.] in memory (selected inversion:
// M = T1^T C_w, S = X^T Y) without a transposing pass before it.  Its LDS image is the [16][BM] image of a B stored [k][n], its
// fragments pair neighbouring ROW tiles the way that image pairs column tiles: MFMA tile i = 2 ip + q of a wave holds the rows
// wm + 32 ip + 2 li + q (li = MFMA row index), which only moves where the epilogue puts a register.  Same k slots, same
// summation order: bitwise the result of transposing A first.
//
// TAIL (round 6, 64 x 64 tiles, B stored [k][n]): ONE more output row, row M of A / C / D (the operands hold M + 1 rows), summed on
// the VALU from the B tile the MFMAs already read.  The workgroups of the last row tile stage A's row M beside the tile (16 doubles
// per K step, lanes 0 .. 7 of wave 0: one more LDS-DMA request); wave w takes k pair group w >> 1 of a K step for its 32 columns --
// the B fragments it holds anyway -- with 4 fp64 FMAs per lane, and the 8 partial sums of a column are added in a fixed order at
// the end.  The M rows of the MFMA tile are untouched: bitwise those of the kernel without the tail.  (The batched posterior runs
// the mean's backward sweep as this row of the samples' sweep: gmrf_hip.hip, posterior_fused.)
// (round 7) The same for B stored [n][k] -- wave w then holds columns wn + li and wn + 16 + li of k pair group w >> 1 -- for
// triangular grids (lower_only == 1) and TRI_B_UPPER products, and with operands of its own (GemmArgs::tA / tC / tD, the
// factorisation's forward solve: gmrf_hip.hip, factor_blocks_range).  The tile that carries the tail of column tile bn is the one
// whose K range is the tail's: the diagonal tile (bn, bn) of a triangular grid (with staircase bounds K starts at kst[bn] there,
// as the tail's column does), else the last row tile.
//
// DOUT (round 13, TAIL with B stored [k][n] and the tail in row M): the product that finishes x_i of the fused posterior's backward
// sweep also writes the caller's arrays -- samples[(p k + r) ld + j] = tile row r + tail row for r < k, mean[p n + j] = tail row --
// which used to be a pass of its own over the whole result panel (unpack_panel_mean).  Every row tile then sums the tail row
// (the same sums in the same order: the same bits), the last one stores it; the tail's sum moves in front of the tile's stores.
// Where the caller's arrays are (GemmDirectOut) is read from device memory: a captured sweep graph holds no pointer of a call.
//
// The body is a function of (descriptor, workgroup index, workgroups of the descriptor) so that one launch can run two
// descriptors (gemm_f64_dma_grouped below); gemm_f64_dma itself is the body at (g, blockIdx.x, gridDim.x).
template <int BM, int BN, bool B_N, bool A_T, bool TAIL, bool DOUT>
__device__ __forceinline__ void gemm_dma_body(const GemmArgs& g, const int bid, const int gdim) {
    constexpr int BK = DMA_BK, STAGES = DMA_STAGES;
    constexpr int MI = BM / 32, NJ = BN / 32;                    // 16 x 16 MFMA tiles of a wave: MI x NJ
    constexpr int NA = BM / 32, NB = BN / 32;                    // LDS-DMA instructions per wave and K step (A, B)
    constexpr int A_ST = BM * BK, B_ST = BN * BK, T_ST = TAIL ? BK : 0, ST = A_ST + B_ST + T_ST;   // doubles per stage
    static_assert(NJ % 2 == 0 || !B_N, "the [k][n] image pairs neighbouring column tiles");
    static_assert(MI % 2 == 0 || !A_T, "the [k][m] image pairs neighbouring row tiles");
    static_assert(!TAIL || (BM == 64 && BN == 64 && !A_T), "the tail row: 64 x 64 tiles");
    static_assert(!DOUT || (TAIL && B_N), "direct output: the tail-row product on B [k][n]");
    int bm, bn, z;
    gemm_dma_tile_order<BM, BN>(g, bid, gdim, bm, bn, z);
    const bool tail_owner = TAIL && (g.lower_only == 1 ? bm == bn : bm == g.M / BM - 1);     // (workgroup-uniform)
    const bool tail = DOUT || tail_owner;               // (DOUT: every row tile sums the tail row, its owner stores it)
    const int m0 = bm * BM, n0 = bn * BN;
    if (g.lower_only == 2 && n0 > m0 + BM - 1) return;
    const int zi = z % g.nb1, zp = z / g.nb1;
    const double* __restrict__ A = g.A + (int64_t)zi * g.strideA + (int64_t)zp * g.pA;
    const double* __restrict__ B = g.B + (int64_t)zi * g.strideB + (int64_t)zp * g.pB;
    double* C = g.C + (int64_t)zi * g.strideC + (int64_t)zp * g.pC;
    const double* Dm = g.D ? g.D + (int64_t)zp * g.pD : C;
    const int64_t ldd = g.D ? g.ldd : g.ldc;

    int kb = 0, ke = g.K;
    if (g.tri & TRI_A_LOWER) ke = min(ke, m0 + BM);
    if (g.tri & TRI_A_UPPER) kb = max(kb, m0);
    if (g.tri & TRI_B_LOWER) kb = max(kb, n0);
    if (g.tri & TRI_B_UPPER) ke = min(ke, n0 + BN);
    // staircase bounds are kept per 64-wide tile and are monotone: a wider tile starts at its first part's bound and
    // ends at its last part's (the parts' own zero ranges hold real zeros)
    // (round 19: the envelope bounds of potrf_block need not be monotone -- a wider tile takes the smallest start of its parts,
    // which is the first part's for a staircase, and the largest ke_m)
    if (g.kb_m) kb = max(kb, BM > 64 ? min(g.kb_m[bm * (BM / 64)], g.kb_m[bm * (BM / 64) + BM / 64 - 1]) : g.kb_m[bm]);
    if (g.kb_n) kb = max(kb, BN > 64 ? min(g.kb_n[bn * (BN / 64)], g.kb_n[bn * (BN / 64) + BN / 64 - 1]) : g.kb_n[bn]);
    if (g.ke_n) ke = min(ke, g.ke_n[bn * (BN / 64) + BN / 64 - 1]);
    if (g.ke_m) ke = min(ke, BM > 64 ? max(g.ke_m[bm * (BM / 64)], g.ke_m[bm * (BM / 64) + BM / 64 - 1]) : g.ke_m[bm]);
    const int nkt = (ke > kb) ? (ke - kb) / BK : 0;

    extern __shared__ __attribute__((aligned(16))) double gsm[];
    const int t = threadIdx.x;
    const int lane = t & 63, w = __builtin_amdgcn_readfirstlane(t >> 6);
    const int wm = (w >> 1) * (BM / 2), wn = (w & 1) * (BN / 2);
    const int li = lane & 15, lq = lane >> 4;
    // waves whose whole quadrant lies strictly above the block diagonal of a lower-only product only help with staging
    // (inside a 64 x 64 tile on the diagonal everything is computed, as gemm_f64_mfma does)
    bool idle = g.lower_only != 0 && ((n0 + wn) / 64 > (m0 + wm + BM / 2 - 1) / 64);
    // (round 29) GemmArgs::strict_lower, 64 x 64 tiles, on a diagonal tile of a triangular grid (workgroup-uniform; per wave
    // everything below is wave-uniform: scalar branches).
    //   B stored [k][n]: wave 1 (rows 0 .. 31, columns 32 .. 63) owns only elements strictly above the ELEMENT diagonal.  It is
    //   idle as above -- its share of the requests, the waits and the barrier of every K step, nothing else -- unless the tile
    //   carries the tail row (TAIL: the diagonal tiles are the tail's owners): then it still reads the two B fragments of its k
    //   pair group and the tail row and does its four FMAs per step.
    //   B stored [n][k] (the symmetric products of the factor): 16 x 16 granularity.  Six of the tile's sixteen MFMA blocks are
    //   strictly upper; the ten others are dealt 3 / 2 / 2 / 3 over the waves -- an idle wave 1 alone would leave the tile as
    //   long as it was, its three sisters' SIMDs as loaded as before -- by giving wave 1 the lower half of wave 2's quadrant:
    //       wave 0: (0,0) (1,0) (1,1)    wave 1: (3,0) (3,1)    wave 2: (2,0) (2,1)    wave 3: (2,2) (3,2) (3,3)
    //   A block's sum is the same MFMA sequence whichever wave runs it (k ascending, the same k slots): the same bits.  The
    //   tail's partial sums stay with their waves (wave 1: columns 32 .. 63 of k pair group 0, from two fragment reads of its own).
    bool strict_diag = false;
    if constexpr (BM == 64 && BN == 64 && !A_T && !DOUT) strict_diag = g.strict_lower != 0 && g.lower_only == 1 && bm == bn;
    const bool skipq = B_N && strict_diag && w == 1;
    const bool diag16 = !B_N && strict_diag;
    const bool tail_only = TAIL && skipq;
    if (!TAIL) idle = idle || skipq;
    // the wave's MFMA blocks (bit 2 i + j) and where they lie: wave 1's at rows 32 .., columns 0 .. instead of its quadrant's
    const int omask = !diag16 ? 15 : (w == 1 ? 12 : (w == 2 ? 3 : 13));
    const int dwm = (diag16 && w == 1) ? BM / 2 : wm, dwn = (diag16 && w == 1) ? 0 : wn;

    // ---- staging plan: per-lane byte offsets (relative to the operand's k0 column / row), one per DMA instruction
    uint32_t offa[NA], offb[NB];
#pragma unroll
    for (int i = 0; i < NA; ++i) {
        const int q = w + 4 * i;
        if (A_T) {
            constexpr int LPR = BM / 2;                          // lanes per k row
            const int k = q * (64 / LPR) + lane / LPR, col = (lane % LPR) * 2;
            offa[i] = (uint32_t)(((int64_t)k * g.lda + m0 + col) * 8);
        } else {
            const int row = 8 * q + (lane >> 3), ch = (lane & 7) ^ ((row >> 1) & 7);
            offa[i] = (uint32_t)(((int64_t)(m0 + row) * g.lda + 2 * ch) * 8);
        }
    }
#pragma unroll
    for (int i = 0; i < NB; ++i) {
        const int q = w + 4 * i;
        if (B_N) {
            // [k][n]: BN * 8 bytes per k row; an instruction covers 1024 / (BN * 8) rows
            constexpr int LPR = BN / 2;                          // lanes per k row
            const int k = q * (64 / LPR) + lane / LPR, col = (lane % LPR) * 2;
            offb[i] = (uint32_t)(((int64_t)k * g.ldb + n0 + col) * 8);
        } else {
            const int row = 8 * q + (lane >> 3), ch = (lane & 7) ^ ((row >> 1) & 7);
            offb[i] = (uint32_t)(((int64_t)(n0 + row) * g.ldb + 2 * ch) * 8);
        }
    }
    const double* arow = g.tC ? g.tA + (int64_t)zp * g.ptA : A + (int64_t)g.M * g.lda;      // (TAIL) the tail row of A
    auto issue = [&](int kt, int stage) {
        const int k0 = kb + kt * BK;
        const char* abase = reinterpret_cast<const char*>(A_T ? A + (int64_t)k0 * g.lda : A + k0);
        const char* bbase = reinterpret_cast<const char*>(B_N ? B + (int64_t)k0 * g.ldb : B + k0);
        double* as = gsm + stage * ST;
        double* bs = as + A_ST;
        // (the one more request of wave 0 needs no count of its own: every wait is vmcnt(0))
        if constexpr (TAIL)
            if (tail && w == 0 && lane < 8)
                __builtin_amdgcn_global_load_lds(GMRF_GLB_PTR(arow + k0 + 2 * lane), GMRF_LDS_PTR(bs + B_ST), 16, 0, 0);
#pragma unroll
        for (int i = 0; i < NA; ++i) {
            asm volatile("" : "+v"(offa[i]));                    // keep base + zext(offset) visible to instruction selection
            __builtin_amdgcn_global_load_lds(GMRF_GLB_PTR(abase + offa[i]), GMRF_LDS_PTR(as + (w + 4 * i) * 128), 16, 0, 0);
        }
#pragma unroll
        for (int i = 0; i < NB; ++i) {
            asm volatile("" : "+v"(offb[i]));
            __builtin_amdgcn_global_load_lds(GMRF_GLB_PTR(bbase + offb[i]), GMRF_LDS_PTR(bs + (w + 4 * i) * 128), 16, 0, 0);
        }
    };

    v4d acc[MI][NJ];
#pragma unroll
    for (int i = 0; i < MI; ++i)
#pragma unroll
        for (int j = 0; j < NJ; ++j) acc[i][j] = (v4d){0.0, 0.0, 0.0, 0.0};
    v2d tacc = (v2d){0.0, 0.0};                                  // (TAIL) columns wn + 2 li, + 1 ([k][n]) / wn + li, + 16 ([n][k]): k pairs 2 lq of group w >> 1
    const int tkg = w >> 1;

    // fragment addresses inside a stage (doubles): A rows wm + 16 i + li, chunk kg * 4 + lq swizzled by the row
    int fa[MI], fb[NJ];
#pragma unroll
    for (int i = 0; i < MI; ++i) {
        const int row = wm + 16 * i + li;
        fa[i] = A_T ? (2 * lq + (i & 1)) * BM + wm + 32 * (i >> 1) + 2 * li : row * 16 + 2 * (lq ^ ((row >> 1) & 3));
    }
    // (chunk = kg * 4 + lq; swizzle key (row >> 1) & 7 = 4 * s2 + s01: chunk ^ key = (kg ^ s2) * 4 + (lq ^ s01))
    int sa2[MI], sb2[NJ];
#pragma unroll
    for (int i = 0; i < MI; ++i) { const int row = wm + 16 * i + li; sa2[i] = (!A_T && ((row >> 1) & 4)) ? 8 : 0; }   // doubles: chunk bit 2 = 4 chunks = 8 doubles
    if (!B_N) {
#pragma unroll
        for (int j = 0; j < NJ; ++j) {
            const int row = wn + 16 * j + li;
            fb[j] = A_ST + row * 16 + 2 * (lq ^ ((row >> 1) & 3));
            sb2[j] = ((row >> 1) & 4) ? 8 : 0;
        }
    } else {
#pragma unroll
        for (int j = 0; j < NJ; ++j) { fb[j] = A_ST + (2 * lq + (j & 1)) * BN + wn + 32 * (j >> 1) + 2 * li; sb2[j] = 0; }
        // fb[2 jp + p]: row k = kg * 8 + 2 lq + p, columns (2 li, 2 li + 1) of column group jp
    }

    // Pipeline: DEPTH = STAGES - 1 = 1 tile is in flight while one is multiplied.  Per K step: wait for this wave's own
    // requests of tile kt (all it has made: nothing is requested behind tile kt), barrier (every wave's part of tile kt has
    // landed, and every wave has finished reading tile kt - 1), request tile kt + DEPTH into the buffer tile kt - 1 occupied,
    // multiply tile kt.  ONE barrier per step.
    constexpr int DEPTH = STAGES - 1;
#pragma unroll
    for (int s = 0; s < DEPTH; ++s)
        if (s < nkt) issue(s, s);
    int kt_first = 0;
    if constexpr (TAIL) {
        if (tail_only) {
            // (round 29) the wave of the skipped quadrant of a diagonal tile that carries the tail: a K loop of its own with the
            // same requests, waits and barrier per step, the tail's operands and its four FMAs as in the loop below, no A
            // fragments and no MFMA
            for (int kt = 0; kt < nkt; ++kt) {
                asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
                __builtin_amdgcn_s_barrier();
                __builtin_amdgcn_sched_barrier(0);
                if (kt + DEPTH < nkt) issue(kt + DEPTH, (kt + DEPTH) % STAGES);
                const double* sm = gsm + (kt % STAGES) * ST;
                const v2d b0 = *reinterpret_cast<const v2d*>(sm + fb[0] + (B_N ? tkg * 8 * BN : ((tkg * 8) ^ sb2[0])));
                const v2d b1 = *reinterpret_cast<const v2d*>(sm + fb[1] + (B_N ? tkg * 8 * BN : ((tkg * 8) ^ sb2[1])));
                const v2d ta = *reinterpret_cast<const v2d*>(sm + A_ST + B_ST + tkg * 8 + 2 * lq);
                if (B_N) {
                    tacc.x = fma(ta.x, b0.x, tacc.x); tacc.x = fma(ta.y, b1.x, tacc.x);
                    tacc.y = fma(ta.x, b0.y, tacc.y); tacc.y = fma(ta.y, b1.y, tacc.y);
                } else {
                    tacc.x = fma(ta.x, b0.x, tacc.x); tacc.x = fma(ta.y, b0.y, tacc.x);
                    tacc.y = fma(ta.x, b1.x, tacc.y); tacc.y = fma(ta.y, b1.y, tacc.y);
                }
                __builtin_amdgcn_sched_barrier(0);
            }
            kt_first = nkt;
        }
    }
    if constexpr (BM == 64 && BN == 64 && !B_N && !A_T && !DOUT) {
        if (diag16) {
            // (round 29) the K loop of a strict-lower diagonal tile: the loop below with the wave's blocks (MASK, bit 2 i + j)
            // chosen at compile time -- the same requests, waits and barrier per step, the fragments its blocks need, their
            // MFMAs in the order of the loop below, the tail as there (TX: wave 1, whose tail columns are not its blocks')
            auto run = [&](auto mask_c, auto tx_c) {
                constexpr int MASK = decltype(mask_c)::value;
                constexpr bool TX = decltype(tx_c)::value;
                // (TX: wave 1) its blocks' rows lie 32 rows of the A image behind its quadrant's, their columns 32 rows of the B
                // image in front of it: the same swizzle (it depends on the row's low four bits), 32 * 16 doubles away.  The
                // tail's columns are the quadrant's.
                constexpr int ash = TX ? 32 * 16 : 0, bsh = TX ? -32 * 16 : 0;
                for (int kt = 0; kt < nkt; ++kt) {
                    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
                    __builtin_amdgcn_s_barrier();
                    __builtin_amdgcn_sched_barrier(0);
                    if (kt + DEPTH < nkt) issue(kt + DEPTH, (kt + DEPTH) % STAGES);
                    const double* sm = gsm + (kt % STAGES) * ST;
                    v2d a[BK / 8][2], b[BK / 8][2];
#pragma unroll
                    for (int kg = 0; kg < BK / 8; ++kg) {
#pragma unroll
                        for (int i = 0; i < 2; ++i) {
                            a[kg][i] = (v2d){0.0, 0.0};
                            if ((MASK >> (2 * i)) & 3) a[kg][i] = *reinterpret_cast<const v2d*>(sm + ash + fa[i] + ((kg * 8) ^ sa2[i]));
                        }
#pragma unroll
                        for (int j = 0; j < 2; ++j) b[kg][j] = *reinterpret_cast<const v2d*>(sm + bsh + fb[j] + ((kg * 8) ^ sb2[j]));
                    }
                    v2d ta = (v2d){0.0, 0.0}, tb0 = ta, tb1 = ta;
                    if constexpr (TAIL) {
                        ta = *reinterpret_cast<const v2d*>(sm + A_ST + B_ST + tkg * 8 + 2 * lq);
                        if constexpr (TX) {
                            tb0 = *reinterpret_cast<const v2d*>(sm + fb[0] + ((tkg * 8) ^ sb2[0]));
                            tb1 = *reinterpret_cast<const v2d*>(sm + fb[1] + ((tkg * 8) ^ sb2[1]));
                        }
                    }
                    __builtin_amdgcn_sched_barrier(0);
#pragma unroll
                    for (int kg = 0; kg < BK / 8; ++kg)
#pragma unroll
                        for (int p = 0; p < 2; ++p)
#pragma unroll
                            for (int i = 0; i < 2; ++i)
#pragma unroll
                                for (int j = 0; j < 2; ++j)
                                    if ((MASK >> (2 * i + j)) & 1)
                                        acc[i][j] = __builtin_amdgcn_mfma_f64_16x16x4f64(p ? a[kg][i].y : a[kg][i].x, p ? b[kg][j].y : b[kg][j].x,
                                                                                         acc[i][j], 0, 0, 0);
                    if constexpr (TAIL) {
                        if constexpr (!TX) { tb0 = tkg ? b[1][0] : b[0][0]; tb1 = tkg ? b[1][1] : b[0][1]; }
                        tacc.x = fma(ta.x, tb0.x, tacc.x); tacc.x = fma(ta.y, tb0.y, tacc.x);
                        tacc.y = fma(ta.x, tb1.x, tacc.y); tacc.y = fma(ta.y, tb1.y, tacc.y);
                    }
                    __builtin_amdgcn_sched_barrier(0);
                }
            };
            if (w == 1) run(std::integral_constant<int, 12>{}, std::true_type{});
            else if (w == 2) run(std::integral_constant<int, 3>{}, std::false_type{});
            else run(std::integral_constant<int, 13>{}, std::false_type{});
            kt_first = nkt;
        }
    }
    for (int kt = kt_first; kt < nkt; ++kt) {
        static_assert(DEPTH == 1, "no tile is requested behind tile kt: the wait is for all of the wave's requests");
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        __builtin_amdgcn_s_barrier();
        __builtin_amdgcn_sched_barrier(0);
        if (kt + DEPTH < nkt) issue(kt + DEPTH, (kt + DEPTH) % STAGES);
        if (!idle) {
            const double* sm = gsm + (kt % STAGES) * ST;
            v2d a[BK / 8][MI], b[BK / 8][NJ];
#pragma unroll
            for (int kg = 0; kg < BK / 8; ++kg) {
#pragma unroll
                for (int i = 0; i < MI; ++i) a[kg][i] = *reinterpret_cast<const v2d*>(sm + fa[i] + (A_T ? kg * 8 * BM : ((kg * 8) ^ sa2[i])));
#pragma unroll
                for (int j = 0; j < NJ; ++j)
                    b[kg][j] = *reinterpret_cast<const v2d*>(sm + fb[j] + (B_N ? kg * 8 * BN : ((kg * 8) ^ sb2[j])));
            }
            v2d ta = (v2d){0.0, 0.0};
            if constexpr (TAIL)
                if (tail) ta = *reinterpret_cast<const v2d*>(sm + A_ST + B_ST + tkg * 8 + 2 * lq);     // a(k), a(k + 1), k = 8 tkg + 2 lq
            __builtin_amdgcn_sched_barrier(0);
#pragma unroll
            for (int kg = 0; kg < BK / 8; ++kg)
#pragma unroll
                for (int p = 0; p < 2; ++p)
#pragma unroll
                    for (int i = 0; i < MI; ++i)
#pragma unroll
                        for (int j = 0; j < NJ; ++j) {
                            double av;                             // ([k][m] image: a[2 ip + p] = row k + p, .x / .y = rows 2 li / 2 li + 1 = tiles 2 ip / 2 ip + 1)
                            if (A_T) av = (i & 1) ? a[kg][2 * (i >> 1) + p].y : a[kg][2 * (i >> 1) + p].x;
                            else av = p ? a[kg][i].y : a[kg][i].x;
                            // [n][k] image: tile j = b[j], k slot = .x / .y.  [k][n] image: b[2 jp + p] = row k + p,
                            // .x / .y = even / odd columns = output tiles 2 jp / 2 jp + 1
                            double bv;
                            if (B_N) bv = (j & 1) ? b[kg][2 * (j >> 1) + p].y : b[kg][2 * (j >> 1) + p].x;
                            else bv = p ? b[kg][j].y : b[kg][j].x;
                            acc[i][j] = __builtin_amdgcn_mfma_f64_16x16x4f64(av, bv, acc[i][j], 0, 0, 0);
                        }
            if constexpr (TAIL) {
                if (tail) {
                    const v2d b0 = tkg ? b[1][0] : b[0][0], b1 = tkg ? b[1][1] : b[0][1];
                    if (B_N) {
                        // b[kg][p] = B(8 kg + 2 lq + p, wn + 2 li .. + 1)
                        tacc.x = fma(ta.x, b0.x, tacc.x); tacc.x = fma(ta.y, b1.x, tacc.x);
                        tacc.y = fma(ta.x, b0.y, tacc.y); tacc.y = fma(ta.y, b1.y, tacc.y);
                    } else {
                        // b[kg][j] = b(8 kg + 2 lq .. + 1, wn + 16 j + li)
                        tacc.x = fma(ta.x, b0.x, tacc.x); tacc.x = fma(ta.y, b0.y, tacc.x);
                        tacc.y = fma(ta.x, b1.x, tacc.y); tacc.y = fma(ta.y, b1.y, tacc.y);
                    }
                }
            }
            __builtin_amdgcn_sched_barrier(0);
        }
    }
    if (idle) return;

    // f64 MFMA C/D map: col = lane & 15, row = (lane >> 4) + 4 * reg.  With an addend (beta != 0) all of its loads are
    // issued before the first is used (one wait instead of one per element).
    const double alpha = g.alpha, beta = g.beta;
    auto orow = [&](int i, int r) -> int64_t {          // row of register r of the wave's MFMA tile i
        return A_T ? m0 + wm + 32 * (i >> 1) + 2 * (lq + 4 * r) + (i & 1) : m0 + wm + i * 16 + lq + 4 * r;
    };
    // (DOUT) the tail row first: its 8 partial sums per column through LDS as below, the finished row kept in LDS for every wave
    v2d mu[NJ / 2 > 0 ? NJ / 2 : 1];
    double* o_s = nullptr;
    int64_t o_ld = 0;
    int o_k = 0;
    if constexpr (DOUT) {
        const GemmDirectOut o = *g.dout;                         // (uniform: scalar loads)
        o_ld = o.ld; o_k = (int)o.k;
        o_s = o.samples + (int64_t)zp * o.k * o.ld + g.o_j0;
        __syncthreads();                                         // every wave is done with the stages
        *reinterpret_cast<v2d*>(gsm + (tkg * 4 + lq) * BN + wn + 2 * li) = tacc;
        __syncthreads();
        if (w == 0) {
            double s = 0.0;
#pragma unroll
            for (int q = 0; q < 8; ++q) s += gsm[q * BN + lane];
            double v = alpha * s;
            if (beta != 0.0) v += beta * Dm[(int64_t)g.M * ldd + n0 + lane];
            if (tail_owner) {
                C[(int64_t)g.M * g.ldc + n0 + lane] = v;
                if (n0 + lane < g.o_cols) o.mean[(int64_t)zp * g.o_n + g.o_j0 + n0 + lane] = v;
            }
            gsm[8 * BN + lane] = v;
        }
        __syncthreads();
#pragma unroll
        for (int jp = 0; jp < NJ / 2; ++jp) mu[jp] = *reinterpret_cast<const v2d*>(gsm + 8 * BN + wn + jp * 32 + 2 * li);
    }
    if (tail_only) {
        // (the skipped quadrant: no addend loads, no stores -- C keeps what it held there; the tail's sums follow below)
    } else if (diag16) {
        // the wave's blocks of a strict-lower diagonal tile; the six blocks strictly above the diagonal keep what C held
#pragma unroll
        for (int i = 0; i < 2; ++i)
#pragma unroll
            for (int j = 0; j < 2; ++j)
                if (omask & (1 << (2 * i + j))) {
                    double d[4] = {0.0, 0.0, 0.0, 0.0};
                    if (beta != 0.0) {
#pragma unroll
                        for (int r = 0; r < 4; ++r) d[r] = Dm[(int64_t)(m0 + dwm + i * 16 + lq + 4 * r) * ldd + n0 + dwn + j * 16 + li];
                    }
#pragma unroll
                    for (int r = 0; r < 4; ++r) {
                        double v = alpha * acc[i][j][r];
                        if (beta != 0.0) v += beta * d[r];
                        C[(int64_t)(m0 + dwm + i * 16 + lq + 4 * r) * g.ldc + n0 + dwn + j * 16 + li] = v;
                    }
                }
    } else if (B_N) {
        v2d d[MI][4][NJ / 2 > 0 ? NJ / 2 : 1];
        if (beta != 0.0) {
#pragma unroll
            for (int i = 0; i < MI; ++i)
#pragma unroll
                for (int r = 0; r < 4; ++r)
#pragma unroll
                    for (int jp = 0; jp < NJ / 2; ++jp)
                        d[i][r][jp] = *reinterpret_cast<const v2d*>(Dm + orow(i, r) * ldd + n0 + wn + jp * 32 + 2 * li);
        }
#pragma unroll
        for (int i = 0; i < MI; ++i)
#pragma unroll
            for (int r = 0; r < 4; ++r)
#pragma unroll
                for (int jp = 0; jp < NJ / 2; ++jp) {
                    v2d v = (v2d){alpha * acc[i][2 * jp][r], alpha * acc[i][2 * jp + 1][r]};
                    if (beta != 0.0) { v.x += beta * d[i][r][jp].x; v.y += beta * d[i][r][jp].y; }
                    *reinterpret_cast<v2d*>(C + orow(i, r) * g.ldc + n0 + wn + jp * 32 + 2 * li) = v;
                    if constexpr (DOUT) {
                        // the caller's layout: sample row r of the problem is a column of ld doubles (8-byte stores: j0 may be odd)
                        const int c = n0 + wn + jp * 32 + 2 * li;
                        if (orow(i, r) < o_k) {
                            double* sp = o_s + orow(i, r) * o_ld + c;
                            if (c < g.o_cols) sp[0] = __dadd_rn(v.x, mu[jp].x);
                            if (c + 1 < g.o_cols) sp[1] = __dadd_rn(v.y, mu[jp].y);
                        }
                    }
                }
    } else {
        double d[MI][4][NJ];
        if (beta != 0.0) {
#pragma unroll
            for (int i = 0; i < MI; ++i)
#pragma unroll
                for (int r = 0; r < 4; ++r)
#pragma unroll
                    for (int j = 0; j < NJ; ++j)
                        d[i][r][j] = Dm[orow(i, r) * ldd + n0 + wn + j * 16 + li];
        }
#pragma unroll
        for (int i = 0; i < MI; ++i)
#pragma unroll
            for (int r = 0; r < 4; ++r)
#pragma unroll
                for (int j = 0; j < NJ; ++j) {
                    double v = alpha * acc[i][j][r];
                    if (beta != 0.0) v += beta * d[i][r][j];
                    C[orow(i, r) * g.ldc + n0 + wn + j * 16 + li] = v;
                }
    }
    if constexpr (TAIL && !DOUT) {
        if (tail) {
            // the 8 partial sums of a column (k pair groups x lq) through LDS, added by wave 0 in a fixed order
            __syncthreads();                                     // every wave is done with the stages
            if (B_N) *reinterpret_cast<v2d*>(gsm + (tkg * 4 + lq) * BN + wn + 2 * li) = tacc;
            else { gsm[(tkg * 4 + lq) * BN + wn + li] = tacc.x; gsm[(tkg * 4 + lq) * BN + wn + 16 + li] = tacc.y; }
            __syncthreads();
            if (w == 0) {
                double s = 0.0;
#pragma unroll
                for (int q = 0; q < 8; ++q) s += gsm[q * BN + lane];
                double v = alpha * s;
                if (g.tC) {
                    double* tc = g.tC + (int64_t)zp * g.ptC;
                    const double* td = g.tD ? g.tD + (int64_t)zp * g.ptD : tc;
                    if (g.tbeta != 0.0) v += g.tbeta * td[n0 + lane];
                    tc[n0 + lane] = v;
                } else {
                    if (beta != 0.0) v += beta * Dm[(int64_t)g.M * ldd + n0 + lane];
                    C[(int64_t)g.M * g.ldc + n0 + lane] = v;
                }
            }
        }
    }
}

__global__ void set_direct_out(GemmDirectOut* o, double* samples, double* mean, int64_t ld, int64_t k) {
    o->samples = samples; o->mean = mean; o->ld = ld; o->k = k;
}

template <int BM, int BN, bool B_N, bool A_T = false, bool TAIL = false, bool DOUT = false>
__global__ __launch_bounds__(256, (BM + BN > 128) ? 3 : 4) void gemm_f64_dma(GemmArgs g) {
    gemm_dma_body<BM, BN, B_N, A_T, TAIL, DOUT>(g, (int)blockIdx.x, (int)gridDim.x);
}

// Two independent products in ONE launch (round 13, 64 x 64 tiles): workgroups [0, wg0) run descriptor g0, [wg0, wg0 + wg1) run g1,
// each exactly as its own launch of wg0 / wg1 workgroups would (same body, same tile order inside the descriptor, same sums: the
// same bits).  The descriptor and its B layout (bit 0 / bit 1 of b_n: g0 / g1 stored [k][n]) are chosen once per workgroup from
// blockIdx.x -- wave-uniform -- in front of the K loop; the K loops themselves are the two bodies unchanged.  A multiple of 8 for
// wg0 keeps g1's problems on the XCDs a launch of its own would put them on (a matter of locality only).
__global__ __launch_bounds__(256, 4) void gemm_f64_dma_grouped(GemmArgs g0, GemmArgs g1, int wg0, int wg1, int b_n) {
    const bool second = (int)blockIdx.x >= wg0;
    const GemmArgs g = second ? g1 : g0;
    const int bid = second ? (int)blockIdx.x - wg0 : (int)blockIdx.x, gdim = second ? wg1 : wg0;
    if ((b_n >> (second ? 1 : 0)) & 1) gemm_dma_body<64, 64, true, false, false, false>(g, bid, gdim);
    else gemm_dma_body<64, 64, false, false, false, false>(g, bid, gdim);
}

// ---------------------------------------------------------------------------------------------
// Kernel choice.  The policy (moved by the test hooks only): 0 = never, 1 = only the 64 x 64 tile, 2 (default) = 128 x 64 /
// 64 x 128 on full products of many tiles, 64 x 64 otherwise.
inline int& gemm_dma_policy() {
    static int v = 2;
    return v;
}
inline int& gemm_dma_force() {          // tests: 0 = by policy, 1 / 2 / 3 = this tile shape wherever the sizes divide
    static int v = 0;
    return v;
}

// (round 29, moved by a test hook only) non-zero: the launchers below drop GemmArgs::strict_lower -- every diagonal tile is
// computed whole, as before round 29.  Read when a launch is issued, so when a factor graph is CAPTURED: a graph replays what
// it was captured with.
inline int& gemm_strict_lower_off() {
    static int v = 0;
    return v;
}

// 0: not a DMA launch; 1: 64 x 64; 2: 128 x 64; 3: 64 x 128
inline int gemm_dma_shape(bool a_t, const GemmArgs& g, int batch) {
    const int policy = gemm_dma_force() ? 2 : gemm_dma_policy();
    if (policy == 0 || g.stamps || (g.tri & ~15) || g.K % DMA_BK || g.M % 64 || g.N % 64) return 0;
    if ((g.lda & 1) || (g.ldb & 1) || ((uintptr_t)g.A & 15) || ((uintptr_t)g.B & 15) || ((g.strideA | g.strideB | g.pA | g.pB) & 1)) return 0;
    // the B [k][n] epilogue loads the addend and stores the result as 16-byte pieces
    if (((uintptr_t)g.C & 15) || (g.ldc & 1) || ((g.strideC | g.pC) & 1)) return 0;
    if (g.D && (((uintptr_t)g.D & 15) || (g.ldd & 1) || (g.pD & 1))) return 0;
    if ((int64_t)g.M * g.ldc * 8 >= ((int64_t)1 << 32) || (g.D && (int64_t)g.M * g.ldd * 8 >= ((int64_t)1 << 32))) return 0;
    // 32-bit byte offsets inside a problem's operand
    if ((int64_t)(a_t ? g.K : g.M) * g.lda * 8 >= ((int64_t)1 << 32) || (int64_t)std::max(g.N, g.K) * g.ldb * 8 >= ((int64_t)1 << 32)) return 0;
    if (a_t) return 1;                                  // A stored [k][m]: the 64 x 64 tile
    const int force = gemm_dma_force();
    if (force == 2 && g.M % 128 == 0) return 2;
    if (force == 3 && g.N % 128 == 0 && !g.lower_only) return 3;
    if (force) return 1;
    if (policy == 1) return 1;
    // The wide tiles pay on full products only (1024^3 x 16: 65 - 69 TF/s against 61 - 64 with 64 x 64 tiles); on the factor's
    // triangular / lower-only / staircase launches their idle quadrants and longer tails lose what the fewer fragment reads gain
    // (tools/gemm_dma_rate.py: G2 304 us against 280 us, rank-256 update of 768^2 101 against 88 us).
    const bool plain = !g.lower_only && !g.tri && !g.kb_m && !g.kb_n && !g.ke_n && !g.ke_m;
    const int64_t t64 = (int64_t)(g.M / 64) * (g.N / 64) * batch;
    if (plain && t64 >= 2048) {
        if (g.M % 128 == 0) return 2;
        if (g.N % 128 == 0 && !g.lower_only) return 3;
    }
    return 1;
}
inline bool gemm_uses_dma(bool a_t, const GemmArgs& g, int batch) { return gemm_dma_shape(a_t, g, batch) != 0; }

inline hipError_t gemm_dma_init() {
    hipError_t e = hipSuccess;
#define GMRF_DMA_ATTR(BM, BN, BNAT)                                                                              \
    if (e == hipSuccess)                                                                                          \
        e = hipFuncSetAttribute((const void*)gemm_f64_dma<BM, BN, BNAT>, hipFuncAttributeMaxDynamicSharedMemorySize, \
                                (int)gemm_dma_lds_bytes<BM, BN>() + 64 * 1024);
    GMRF_DMA_ATTR(64, 64, false) GMRF_DMA_ATTR(64, 64, true)
    GMRF_DMA_ATTR(128, 64, false) GMRF_DMA_ATTR(128, 64, true)
    GMRF_DMA_ATTR(64, 128, false) GMRF_DMA_ATTR(64, 128, true)
#undef GMRF_DMA_ATTR
    return e;
}

// A triangular grid whose tiles have K begins of their own (kb_m / kb_n: staircase or envelope bounds) walks its rows ascending --
// longest tiles first (see gemm_dma_tile_order).  Returns the GemmArgs::tri bit to set, for the descriptor as the caller gave it.
inline int gemm_dma_row_order(const GemmArgs& g) {
    return (g.lower_only && g.M == g.N && (g.kb_m || g.kb_n)) ? DMA_ROWS_ASCENDING : 0;
}

// The product plus its tail row M (see TAIL above) on the 64 x 64 tile -- the kernel launch_gemm picks for the M rows when
// gemm_dma_shape says 1 and gemm_uses_ll does not take the launch; nothing else qualifies.  Returns false (nothing launched) if
// the product does not.
inline bool gemm_tail_ok(bool a_t, bool b_n, const GemmArgs& g, int batch) {
    if (a_t || gemm_uses_ll(g, batch) || gemm_dma_shape(false, g, batch) != 1) return false;
    if (g.lower_only && g.M != g.N) return false;                // (a triangular grid: the diagonal tiles carry the tail)
    if (g.tC && g.dout) return false;
    if (g.tC) {
        // operands of its own: one problem per z, 16-byte aligned tail A (LDS-DMA of 16 bytes), even problem stride
        return g.nb1 == 1 && g.tA && ((uintptr_t)g.tA & 15) == 0 && (g.ptA & 1) == 0;
    }
    if (!b_n || g.lower_only) return false;                      // (so a direct output, g.dout, is on B [k][n] with the tail in row M)
    if (g.dout && g.nb1 != 1) return false;
    // (a direct output: EVERY row tile sums the tail row, so the tail must not read C and must share every tile's K range)
    // (TRI_A_* give the row tiles of one column tile different K ranges; TRI_B_* do not)
    if (g.dout && (g.beta != 0.0 || g.kb_m || g.kb_n || g.ke_n || g.ke_m || (g.tri & (TRI_A_LOWER | TRI_A_UPPER)))) return false;
    // 32-bit byte offsets inside a problem's operand for the M + 1 rows (A: row M read with 64-bit addressing)
    return (int64_t)(g.M + 1) * g.ldc * 8 < ((int64_t)1 << 32) && (!g.D || (int64_t)(g.M + 1) * g.ldd * 8 < ((int64_t)1 << 32));
}
inline bool gemm_try_dma_tail(hipStream_t st, bool a_t, bool b_n, const GemmArgs& g, int batch, hipEvent_t ev_start, hipEvent_t ev_stop,
                              hipError_t* err) {
    if (!gemm_tail_ok(a_t, b_n, g, batch)) return false;
    // (grid and tile order as gemm_try_dma sets them up for the 64 x 64 tile)
    const bool tri_grid = g.lower_only && g.M == g.N;
    GemmArgs gs = g;
    gs.lower_only = tri_grid ? 1 : 0;
    gs.tri |= gemm_dma_row_order(g);
    if (gemm_strict_lower_off()) gs.strict_lower = 0;
    const int64_t nx = g.N / 64, ny = g.M / 64;
    const dim3 grid((unsigned)((tri_grid ? ny * (ny + 1) / 2 : nx * ny) * batch)), block(256);
    const size_t lds = (size_t)DMA_STAGES * (64 + 64 + DMA_BK) * DMA_BK * sizeof(double);
#define GMRF_DMA_TK(...)                                                                                                   \
    do {                                                                                                                   \
        if (ev_start) hipExtLaunchKernelGGL((gemm_f64_dma<64, 64, __VA_ARGS__>), grid, block, lds, st, ev_start, ev_stop, 0, gs); \
        else hipLaunchKernelGGL((gemm_f64_dma<64, 64, __VA_ARGS__>), grid, block, lds, st, gs);                          \
    } while (0)
    if (g.dout) GMRF_DMA_TK(true, false, true, true);
    else if (b_n) GMRF_DMA_TK(true, false, true);
    else GMRF_DMA_TK(false, false, true);
#undef GMRF_DMA_TK
    *err = hipGetLastError();
    return true;
}

// Launches the product on a DMA kernel if it qualifies (returns true), else leaves it to launch_gemm's other kernels.
inline bool gemm_try_dma(hipStream_t st, bool a_t, bool b_n, const GemmArgs& g, int batch, hipEvent_t ev_start, hipEvent_t ev_stop,
                         hipError_t* err) {
    const int shape = gemm_dma_shape(a_t, g, batch);
    if (shape == 0) return false;
    const bool tri_grid = g.lower_only && g.M == g.N;
    GemmArgs gs = g;
    gs.lower_only = tri_grid ? 1 : (g.lower_only ? 2 : 0);
    gs.tri |= gemm_dma_row_order(g);
    if (gemm_strict_lower_off()) gs.strict_lower = 0;
    const dim3 block(256);
#define GMRF_DMA_GO(BM, BN)                                                                                       \
    do {                                                                                                          \
        const int64_t nx = g.N / BN, ny = g.M / BM;                                                               \
        const int64_t tiles = tri_grid ? (int64_t)(BM / BN > 0 ? BM / BN : 1) * ny * (ny + 1) / 2 : nx * ny;      \
        const dim3 grid((unsigned)(tiles * batch));                                                               \
        const size_t lds = gemm_dma_lds_bytes<BM, BN>();                                                          \
        if (a_t && BM == 64 && BN == 64) {                                                                        \
            if (b_n) GMRF_DMA_K((gemm_f64_dma<64, 64, true, true>)); else GMRF_DMA_K((gemm_f64_dma<64, 64, false, true>)); \
        } else {                                                                                                  \
            if (b_n) GMRF_DMA_K((gemm_f64_dma<BM, BN, true>)); else GMRF_DMA_K((gemm_f64_dma<BM, BN, false>));    \
        }                                                                                                         \
    } while (0)
#define GMRF_DMA_K(KERNEL)                                                                                        \
    do {                                                                                                          \
        if (ev_start) hipExtLaunchKernelGGL(KERNEL, grid, block, lds, st, ev_start, ev_stop, 0, gs);              \
        else hipLaunchKernelGGL(KERNEL, grid, block, lds, st, gs);                                                \
    } while (0)
    if (shape == 2) GMRF_DMA_GO(128, 64);
    else if (shape == 3) GMRF_DMA_GO(64, 128);
    else GMRF_DMA_GO(64, 64);
#undef GMRF_DMA_K
#undef GMRF_DMA_GO
    *err = hipGetLastError();
    return true;
}

// Two products as ONE launch of gemm_f64_dma_grouped (64 x 64 tiles): may they?  Both on A [m][k], without a tail, each a launch
// the 64 x 64 LDS-DMA kernel takes on its own.  (The kernels launch_gemm would pick for either -- the 32 x 32 one for a handful of
// problems, the wide tiles -- sum every output element in the same order: grouping changes no bit.)
inline bool gemm_grouped_ok(const GemmArgs& g0, const GemmArgs& g1, int batch) {
    if (gemm_dma_policy() == 0 || g0.tC || g1.tC || g0.dout || g1.dout) return false;
    if (g0.lower_only && g0.M != g0.N) return false;             // (an early-exit grid: not needed here)
    if (g1.lower_only && g1.M != g1.N) return false;
    return gemm_dma_shape(false, g0, batch) != 0 && gemm_dma_shape(false, g1, batch) != 0;
}
inline int64_t gemm_dma_grid64(const GemmArgs& g, int batch) {
    const int64_t nx = g.N / 64, ny = g.M / 64;
    return ((g.lower_only && g.M == g.N) ? ny * (ny + 1) / 2 : nx * ny) * batch;
}
inline bool gemm_try_dma_grouped(hipStream_t st, bool b_n0, const GemmArgs& g0, bool b_n1, const GemmArgs& g1, int batch,
                                 hipEvent_t ev_start, hipEvent_t ev_stop, hipError_t* err) {
    if (!gemm_grouped_ok(g0, g1, batch)) return false;
    GemmArgs gs[2] = {g0, g1};
    for (GemmArgs& g : gs) {                                     // (as gemm_try_dma sets a launch of its own up)
        g.tri |= gemm_dma_row_order(g);
        g.lower_only = (g.lower_only && g.M == g.N) ? 1 : 0;
        if (gemm_strict_lower_off()) g.strict_lower = 0;
    }
    const int wg0 = (int)gemm_dma_grid64(g0, batch), wg1 = (int)gemm_dma_grid64(g1, batch);
    const int bn = (b_n0 ? 1 : 0) | (b_n1 ? 2 : 0);
    const dim3 grid((unsigned)(wg0 + wg1)), block(256);
    const size_t lds = gemm_dma_lds_bytes<64, 64>();
    if (ev_start) hipExtLaunchKernelGGL(gemm_f64_dma_grouped, grid, block, lds, st, ev_start, ev_stop, 0, gs[0], gs[1], wg0, wg1, bn);
    else hipLaunchKernelGGL(gemm_f64_dma_grouped, grid, block, lds, st, gs[0], gs[1], wg0, wg1, bn);
    *err = hipGetLastError();
    return true;
}

}  // namespace gmrf
