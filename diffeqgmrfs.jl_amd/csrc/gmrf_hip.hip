// libgmrf_hip.so -- C ABI (include/gmrf_hip.h) over the gfx950 kernels of this directory.
//
// Host orchestration of the block-tridiagonal Cholesky path of DiffEqGMRFs.jl
// (/root/reference/src/tridiagonal_cholesky.jl): symbolic analysis of the CSC matrix into
// per-block entry lists, then per block  scatter -> C = B Linv^T -> S = D - C C^T ->
// potrf(S) by 64-wide panels -> Linv by recursive doubling;  sweeps as chains of
// matrix-panel products.  Launch sequences are captured once into HIP graphs and replayed
// (the chains are launch-latency bound: ~60 dependent launches per block).
#include <hip/hip_runtime.h>
#include <dlfcn.h>
#include <stdint.h>
#include <stdlib.h>
#include <string.h>
#include <time.h>

#include <algorithm>
#include <atomic>
#include <iterator>
#include <cmath>
#include <map>
#include <memory>
#include <chrono>
#include <functional>
#include <initializer_list>
#include <mutex>
#include <string>
#include <type_traits>
#include <vector>

#include "../../include/gmrf_hip.h"
#include "assemble.hpp"
#include "fem_assemble.hpp"
#include "burgers_line.hpp"
#include "burgers_colloc.hpp"
#include "gemm_f64.hpp"
#include "gemm_f64_dma.hpp"
#include "microbench.hpp"
#include "misc_kernels.hpp"
#include "potrf_step.hpp"
#include "potrf_persist.hpp"
#include "sweep.hpp"
#include "sweep_persist.hpp"
#include "swe_assemble.hpp"
#include "elliptic_assemble.hpp"
#include "elliptic_assemble_p2.hpp"
#include "fem_assemble_p2.hpp"
#include "selinv.hpp"
#include "gauss_newton.hpp"
#include "darcy_cond.hpp"
#include "gn_posterior.hpp"
#include "burgers_prior.hpp"
#include "burgers_line_prior.hpp"
#include "field_eval.hpp"

using namespace gmrf;

#include "host_util.hpp"      // g_last_error, HIPCHK / GCHK, bad_shape, is_device_ptr, DevBuf / DevArr, DevCtx, Staging, Carve

static double g_tile_us = 0.0;
static unsigned long long g_tile_stamps[64];
static unsigned long long g_persist_stamps[128];    // chain workgroup of the last gmrf_test_potrf_block (potrf_persist.hpp)

// Do the byte ranges [p, p + pb) and [q, q + qb) meet?  Addresses only: host and device pointers alike.
static bool ranges_overlap(const void* p, int64_t pb, const void* q, int64_t qb) {
    if (!p || !q || pb <= 0 || qb <= 0) return false;
    const uintptr_t a = reinterpret_cast<uintptr_t>(p), b = reinterpret_cast<uintptr_t>(q);
    return a < b + (uintptr_t)qb && b < a + (uintptr_t)pb;
}

// bytes spanned by `cols` column-major columns of n doubles with leading dimension ld
static int64_t cols_bytes(int64_t n, int64_t cols, int64_t ld) {
    return cols <= 0 ? 0 : ((cols - 1) * ld + n) * (int64_t)sizeof(double);
}

static int64_t next_pow2(int64_t v) {
    int64_t p = 1;
    while (p < v) p <<= 1;
    return p;
}

// ------------------------------------------------------------------------------------ csr
struct gmrf_csr : DevCtx {
    int64_t n_rows = 0, n_cols = 0, nnz = 0;
    DevArr<int64_t> d_rowptr;
    DevArr<int32_t> d_colidx;
    DevArr<double> d_vals;
    DevArr<float> d_vals32;
    DevArr<double> d_diag;
    bool tiles_ok = false;             // every SPMV_ROWS-row tile has at most SPMV_CAP entries (csr_spmv_tiles)
    DevBuf stage_x, stage_y;           // host operands of gmrf_spmm / gmrf_spmm_rows
    // tile plan of csr_spmm_tiles (node-major right-hand sides), built on first use
    int plan_state = 0;                // 0: not built, 1: usable, -1: a tile exceeds the LDS image
    DevArr<int64_t> d_tile_uptr;       // [tiles + 1] ranges into d_ucols
    DevArr<int32_t> d_ucols;           // distinct columns of every tile, ascending
    DevArr<uint16_t> d_lidx;           // per entry: index of its column in the tile's list
    int64_t n_ucols = 0;
    int plan_rows = 0, plan_ucap = 0, plan_ecap = 0, plan_ecap_pad = 0, plan_umax = 0;   // rows per tile, LDS capacities (distinct columns, entries)
    uint64_t id = 0;                   // unique per created matrix (the selected-inverse plan of a handle is keyed by it)
    // the routes of the last products launched on this matrix (gmrf_test_spmm_route): node-major kind (SpmmRowsRoute) and NG,
    // column-major lane group (0: csr_spmv_tiles); -1: none yet
    int last_rows_kind = -1, last_rows_ng = -1, last_cols_g = -1;
};
static std::atomic<uint64_t> g_csr_ids{0};

// ------------------------------------------------------------------------------------ handle
struct EvPair {
    hipEvent_t a, b;
    int kind;       // kernel class, see gmrf_stats
    double work;    // flops or bytes
    int shape = -1; // GEMM launches: index into gmrf_handle::gemm_shapes
};

// one distinct GEMM launch shape of a profiled run (gmrf_test_gemm_shapes): the roofline table by shape
struct GemmShapeStat {
    int64_t key[8];     // class, M, N, K, tri, lower_only, problems, per-tile K bounds?
    double launches = 0, ms = 0, work = 0;
};

struct TwistState;

struct gmrf_handle : DevCtx {
    int64_t n = 0, N = 0, bs = 0, bsp = 0, n_pad = 0;
    int64_t B = 1;                     // independent problems factored / solved in lock step
    int64_t sel = 0;                   // problem the accessors (get_block, logdet, ...) address
    int64_t alloc_B = 0, vals_B = 0;
    // symbolic
    int64_t nnz_in = 0, n_entries = 0;
    DevArr<uint64_t> d_keys;
    DevArr<double> d_vals;
    DevArr<int64_t> d_src;             // entry -> index into the caller's nzval
    DevArr<double> d_nz_stage;         // staging for host nzval
    std::vector<int64_t> diag_first, diag_count, low_first, low_count;
    bool analyzed = false;
    // Layout of the coupling blocks C_i of the CURRENT factor (set by the symbolic phase, by
    // gmrf_bt_adopt_layout for a factor received by broadcast, "dense" for an imported image): C_i is
    // zero left of column cmin and below row rmax (64-aligned), and inside that window row tile t
    // (64 rows) is zero left of column cmin + kst[t] -- the staircase a FEM coupling block has
    // (kst: monotone envelope over all blocks).  C is STORED as the window only: [rmax][bsp - cmin].
    int64_t cmin = 0, rmax = 0;
    std::vector<int> kst, mend;        // mend[u]: column tile u (64 columns from cmin) is zero below row mend[u]
    DevArr<int> d_kst;                 // device copies: [bsp / 64] each
    DevArr<int> d_mend;
    DevArr<int> d_kbx;                 // [bsp / 64]: max(0, 64 u - cmin): first non-zero row of column tile u of Linv_i[cmin:, :] (selected inversion)
    double c_streamed = 0.0;           // doubles of one C_i inside the staircase (what a k = 1 sweep reads)
    double g2_tile_k = 0.0;            // sum over lower tiles of the K extent of S = -C C^T (flop accounting)
    bool c_dirty = false;              // C must be re-zeroed (new pattern)
    // (round 19) Envelope of the rows of a Schur block that S = D_i - C C^T leaves as D_i's (build_symbolic: env_lo / env_hi, in-block
    // columns per block and 64-row tile) and what potrf_block passes of it per block i and 256-column panel p, relative to the panel:
    // env_host / d_env[((i np + p) 4 + a) nt + bm], bm = row tile below the panel; a = 0: kb (row tile bm of L[below, P] is zero left
    // of it), 1: ke (row tile bm of S[below, P] is zero from it on), 2 / 3: kb / ke with the LAST row tile's trivial (it carries a tail
    // row of operands of its own).  env_has[i np + p]: bit 0 some kb > 0, bit 1 some kb > 0 or ke < 256, bit 2 the same for a = 2 / 3.
    // d_env_ken[4 i + bn]: row tiles of L[256:, 0:256] that column tile bn meets, as a K end (the backward sweep's L_ba^T product).
    std::vector<int> env_lo, env_hi, env_host, env_ken;
    std::vector<unsigned char> env_has, env_ken_has;
    DevArr<int> d_env;
    DevArr<int> d_env_ken;
    bool env_ok = false;               // the arrays above describe the analysed pattern and the current layout
    bool tw_half = false;              // a half of a twisted handle: never takes the envelope bounds
    DevArr<int> d_lo_rowptr;
    DevArr<int> d_dg_rowptr;          // [N][bsp + 1]: the diagonal blocks' entries row by row (absolute positions in d_keys)
    // tile plan of the sparse C = B X^T (spmm_bxt_tiles): per lower block and 64-row tile the distinct columns, per entry its index into them
    DevArr<int> d_bxt_uptr, d_bxt_ucols; DevArr<uint16_t> d_bxt_lidx; DevArr<int> d_bxt_gtiles;
    std::vector<int> bxt_ng;           // groups of row tiles per lower block (host copy: the launch's grid)
    int group_tiles_force = -1;        // test hook (gmrf_test_coupling_group_tiles): the next analysis groups tiles (1) / keeps every tile alone (0); -1: by the batch
    int bxt_ecap = 0; int bxt_nrt = 0; bool bxt_plan_ok = false;        // [N][bsp + 1] row-wise view of the lower blocks' entry lists
    int64_t lo_row_max = 0;            // most entries in one row of a lower block
    bool sparse_b = false;             // lower blocks are sparse enough for C = B X^T by spmm_bxt
    // factor storage
    DevArr<double> d_L, d_C, d_Linv;   // ours, or the caller's (gmrf_bt_set_storage: borrowed, never freed)
    bool external_storage = false;
    bool keep_l = true;                // false: L_i lives in a one-block work buffer (sweeps need Linv and C only)
    bool l_valid = false;              // d_L holds the blocks of the current factor (get_block / export / logdet from L)
    bool logdet_valid = false;         // d_logdet holds every block's log-determinant part of the current factor
    std::vector<char> got_block;       // blocks received through gmrf_bt_unpack_blocks_async since the last adopt / commit
    int64_t alloc_rm = 0, alloc_wc = 0;
    bool alloc_keep_l = true;
    DevArr<double> d_S, d_B, d_T, d_W;
    DevArr<double> d_V;                // two more work blocks per problem, allocated by the first exact-variance call (var_exact)
    // selected inverse on a pattern (gmrf_bt_selinv / gmrf_bt_trace_inv): the plan of the last pattern, built on the host once per
    // (layout, pattern); a new layout or shape (layout_gen) drops it, new values of the same pattern keep it
    uint64_t layout_gen = 0;
    uint64_t sel_csr = 0, sel_gen = ~0ull;            // plan of matrix id sel_csr under layout_gen sel_gen
    int64_t sel_nnz = 0;
    std::vector<int64_t> sel_off, sel_nd;             // [N + 1] block step i's entries; [N] how many of them read S_ii
    DevArr<int64_t> d_sel_src;                        // [entries] element offset inside the block (row * bsp + col)
    DevArr<int64_t> d_sel_slot;                       // [2][sel_cap] output slot, mirrored slot (-1: none)
    int64_t sel_cap = 0;                              // stride between the two halves of d_sel_slot
    DevArr<double> d_sig;                             // [B][nnz] Sigma on the pattern (gmrf_bt_trace_inv, host output)
    DevArr<double> d_dv;                              // staged host dvals / trace output
    DevArr<int> d_info;
    DevArr<double> d_logdet;
    int64_t alloc_N = 0, alloc_bsp = 0;
    bool factored = false;
    // right-hand-side panels
    DevArr<double> d_P, d_Y, d_Tp;
    DevArr<double> d_stage;
    DevBuf mean_arena;                 // a host `mean` of gmrf_bt_sample, a host `out` of gmrf_bt_logdet_batch (Staging)
    DevArr<double> d_acc;              // variance accumulator / output ([problems][n])
    int32_t var_group = 0, var_groups = 0;   // the last batched sampled estimator: problems per group of the stage, groups per chunk (gmrf_test_var_groups)
    // route switches: the last gmrf_bt_set_eager word, GMRF_SW_* of gmrf_hip.h (a half of a twisted handle beside another half
    // also carries GMRF_SW_NO_SWEEP_PERSIST)
    int32_t switches = 0;
    bool sw(int32_t bit) const { return (switches & bit) != 0; }
    // graphs
    bool tail_probe = false;           // gemm(tail): only check whether the product qualifies (posterior_fused_ok)
    bool tail_refused = false;         // ... one did not
    // The forward solve inside a batch's factorisation (round 7, gmrf_bt_set_factor_rhs): with the registered right-hand side b the
    // factor's own products also leave y = L^-1 b (tail rows of G2, the panel products and the rank-256 updates; factor_blocks_range)
    const double* frhs = nullptr;      // registered b (device, n x B, read at factor time)
    const double* fy_for = nullptr;    // the current factor left y = L^-1 fy_for in d_fy (nullptr: none)
    bool fwd_run = false;              // the factorisation being enqueued carries the forward solve (factor_fwd_ok)
    DevArr<GemmDirectOut> d_dout;      // where the fused posterior's last products write the caller's mean / samples (posterior_fused_ok allocates)
    DevArr<double> d_ft;               // [B][bsp]: t = b_i - C_i y_{i-1} of the block being factored, updated panel by panel
    DevArr<double> d_fy;               // [B][n_pad]: y, laid out as a k = 1 panel (what fill_normals_panel reads row kp from)
    const double* factor_graph_rhs = nullptr;   // b the captured factor graph reads (nullptr: it does not solve)
    unsigned long long* dbg_stamps = nullptr;   // test hook: phase stamps of the fused panel step
    // Split representation of the block inverses (batches whose coupling blocks are zero left of column cmin >= 256):
    // with p = xsplit, a = [0, p), b = [p, bsp), the storage of Linv_i holds X_aa, X_bb and -- in the place of
    // X_ba = -X_bb L_ba X_aa -- the factor's own L_ba.  C_i = B_i Linv_{i-1}^T reads X_bb only; the sweeps apply
    // y_a = X_aa t_a, y_b = X_bb (t_b - L_ba y_a) (and the transposed order backward).  0: the full inverse.
    int xsplit = 0;                    // state of the stored factor
    int adopt_xsplit = 0;              // what the layout record of an adopted factor said (committed by gmrf_bt_adopt_commit)
    // One problem: the in-block Cholesky as ONE persistent launch per block / per 256-column panel (potrf_persist.hpp) instead of a
    // launch per 64-column step.  Needs every workgroup resident (1 + tiles <= CUs); a wait that gives up sets d_info[1], and
    // factor_finish then repeats the factorisation with the launch-per-step form and keeps it for this handle.
    bool persist_gave_up = false;      // a bounded wait inside a persistent launch gave up: this handle keeps the launch-per-step forms for good (set_eager cannot clear it)
    bool persist_launched = false;     // a persistent launch was enqueued since the abort word was last looked at
    int persist_cus = 0;               // CUs held of the device's budget (persist_plan); 0: no persistent launches
    int info_checked = 0;              // d_info[0] as the host last saw it (restored when an aborted range is repeated)
    int factor_graph_route = 0;        // stats.persist_route of the captured factor graph
    int persist_aborts = 0;
    int cu_count = 0;
    DevArr<unsigned> d_pflags;         // flag words of the persistent launches (zero between launches: potrf_persist cleans up after itself)
    // One problem: a whole sweep as ONE persistent launch (sweep_persist.hpp) instead of two dependent launches per block.  Every
    // workgroup must be resident: the handle then claims the whole chip (persist_plan).  A wait that gives up sets the mapped host
    // word; gmrf_bt_solve / gmrf_bt_sample see it at their synchronisation and repeat the call with the launch-per-product form.
    bool sweep_persist_planned = false;   // the claim covers the whole chip (persist_plan)
    bool sweep_persist_launched = false;  // such a launch was enqueued since the abort word was last looked at
    DevArr<unsigned> d_sweep_flags;       // [0] the device's abort word
    DevArr<double> d_Tsw;                 // intermediate panel of the persistent sweeps (right-hand side minus coupling product)
    HostWord h_sweep_abort;               // mapped host word
    int sweep_nw = 0;
    DevArr<double> d_P2, d_Y2, d_T2;      // gmrf_bt_posterior: the samples' panels (their sweep runs beside the mean's)
    bool sweep_persist_hold = false;      // this call must not use it (an input overlaps an output: a launch that gave up could not be repeated)
    // second branch of the captured factor graph: the inverse assembly of a block's first half runs
    // beside the panel chain of its second half (see potrf_block)
    hipStream_t aux = nullptr;
    bool aux_distinct = false;         // `aux` was chosen on a hardware queue of its own (gmrf_bt_posterior)
    hipStream_t gemm_stream = nullptr; // stream gemm() launches on (h->stream unless inside the aux branch)
    bool capturing = false;
    std::vector<hipEvent_t> fork_events;
    size_t fork_next = 0;
    hipGraphExec_t factor_graph = nullptr;
    int64_t factor_graph_i0 = -1, factor_graph_i1 = -1;
    std::map<int64_t, hipGraphExec_t> sweep_graphs;   // key = mode * 4096 + kp
    // profiling
    int profiling = 0;
    std::vector<EvPair> events;
    std::vector<hipEvent_t> ev_pool;
    std::vector<GemmShapeStat> gemm_shapes;
    gmrf_stats stats;
    hipEvent_t ev0 = nullptr, ev1 = nullptr;
    // elimination order (gmrf_bt_set_order): GMRF_ORDER_TWISTED runs the factorisation as two chains that meet in block m, on two
    // one-problem sub-handles (TwistState); meet_req = -1: automatic
    int order = GMRF_ORDER_REFERENCE;
    int64_t meet_req = -1;
    TwistState* tw = nullptr;
    // the top half of a twisted handle: block tw_blk is the meeting block, its Schur block also takes -HJ HJ^T (HJ = H_m J) and
    // its factorisation leaves W = L_m^-1 HJ (the meeting corrections of the sweeps).  -1: a plain handle.
    int64_t tw_blk = -1;
    const double* tw_hj = nullptr;
    double* tw_w = nullptr;
};

// --------------------------------------------------------------------------------- twisted (two-ended) order
// Q = T T^T with T's diagonal blocks L_0 .. L_m (lower) and U_{m+1} .. U_{N-1} (upper), couplings G_i = T[i, i-1] (1 <= i <= m)
// and H_i = T[i, i+1] (m <= i < N-1): two chains of about N / 2 blocks that run at the same time and meet in block m.  The handle
// owns two one-problem sub-handles.  `top` factors blocks 0 .. m with the existing code; its meeting block also takes -H_m H_m^T
// (the hook tw_blk / tw_hj of factor_blocks_range).  `bot` factors the FULLY index-reversed trailing matrix, x'_k = x_{n-1-k}
// over blocks N-1 .. m+1: a plain block-tridiagonal matrix whose couplings keep the window / staircase shape (reversing the
// block order alone would transpose them), so U_i = J L'_i J with J the flip inside a block.  The meeting coupling is kept as
// HJ = H_m J = J C', where C' = B' L'^-T is the coupling the reversed chain would form for one more block; B-hat = J B' is
// scattered straight from the caller's entries of Q[m+1, m].  W = L_m^-1 HJ is the one matrix both sweeps' meeting corrections
// need:  forward  y_m -= W y'_last  (= L_m^-1 H_m y_{m+1}),  backward  y'_last -= W^T y_m  (= J H_m^T x_m with x_m = L_m^-T y_m).
// Each half keeps its own single-stream captured graphs; the halves run on the handle's stream and on `aux`, forked and joined
// with events.  m = N - 1: no bottom half, the handle IS its top half (the reference order, bitwise).
struct TwistState {
    gmrf_handle* top = nullptr;
    gmrf_handle* bot = nullptr;
    int64_t m = -1, N = 0, n = 0, bs = 0, bsp = 0, nnz = 0;
    DevArr<uint64_t> d_mkeys;          // entries of Q[m+1, m] as entries of B-hat: (row gamma, column bs-1-rho) for Q[rho, gamma]
    DevArr<int64_t> d_msrc;
    DevArr<double> d_mvals;
    int64_t m_count = 0;
    DevArr<double> d_Bm, d_HJ, d_W, d_Smm;       // bsp x bsp, row-major
    DevArr<double> d_nz;               // staged host nzval (both halves gather from it)
    const double* d_nz_cur = nullptr;  // the nzval of the current factorisation (device)
    DevArr<double> d_z;                // column-major n x 64 samples (sampled variances)
    DevArr<double> d_var;              // the bottom half's variances in its own (reversed) order
    hipEvent_t ev_fork = nullptr, ev_join = nullptr;
};


static bool tw_on(const gmrf_handle* h) { return h && h->tw && h->tw->bot; }
// A twisted handle whose meeting block is the last one IS its top half: the calls go there.
static gmrf_handle* tw_route(gmrf_handle* h) {
    return (h && h->order == GMRF_ORDER_TWISTED && h->tw && h->tw->top && !h->tw->bot && h->factored) ? h->tw->top : h;
}
static gmrf_status tw_refuse(const gmrf_handle* h, const char* what) {
    if (!h || h->order != GMRF_ORDER_TWISTED) return GMRF_OK;
    g_last_error = std::string(what) + ": not supported on a handle in the twisted elimination order (gmrf_bt_set_order)";
    return GMRF_ERR_BAD_SHAPE;
}

static void destroy_graphs(gmrf_handle* h) {
    if (h->factor_graph) { (void)hipGraphExecDestroy(h->factor_graph); h->factor_graph = nullptr; }
    for (auto& kv : h->sweep_graphs) (void)hipGraphExecDestroy(kv.second);
    h->sweep_graphs.clear();
}

static hipEvent_t ev_get(gmrf_handle* h) {
    if (!h->ev_pool.empty()) {
        hipEvent_t e = h->ev_pool.back();
        h->ev_pool.pop_back();
        return e;
    }
    hipEvent_t e;
    (void)hipEventCreate(&e);
    return e;
}

struct ProfScope {
    gmrf_handle* h;
    EvPair p;
    bool on;
    ProfScope(gmrf_handle* hh, int kind, double work) : h(hh), on(hh->profiling > 0) {
        if (on) {
            p.kind = kind; p.work = work;
            p.a = ev_get(h); p.b = ev_get(h);
            (void)hipEventRecord(p.a, h->stream);
        }
    }
    ~ProfScope() {
        if (on) {
            (void)hipEventRecord(p.b, h->stream);
            h->events.push_back(p);
        }
    }
};

static void prof_collect(gmrf_handle* h) {
    for (auto& p : h->events) {
        float ms = 0.f;
        (void)hipEventElapsedTime(&ms, p.a, p.b);
        h->stats.kernel_ms[p.kind] += ms; h->stats.kernel_work[p.kind] += p.work; h->stats.kernel_launches[p.kind]++;
        if (p.shape >= 0) { auto& g = h->gemm_shapes[(size_t)p.shape]; g.launches += 1; g.ms += ms; g.work += p.work; }
        h->ev_pool.push_back(p.a);
        h->ev_pool.push_back(p.b);
    }
    h->events.clear();
}

// ------------------------------------------------------------------------------------ helpers
// A tail row on operands of its own (GemmArgs::tA / tC / tD): tC = beta tD + alpha tA b, per problem strides pA / pC / pD
// C == nullptr: the tail is row M of the product's own operands.  out (then; B [k][n]): the product also writes the caller's mean and
// samples (gemm_f64_dma's DOUT) -- its columns are the dofs j0 .. of a problem, the first `cols` of them real
struct GemmTail {
    const double* A = nullptr; int64_t pA = 0;
    double* C = nullptr; int64_t pC = 0;
    const double* D = nullptr; int64_t pD = 0;
    double beta = 0.0;
    const GemmDirectOut* out = nullptr;
    int64_t j0 = 0;
    int cols = 0;
};

// the flops gemm() books for one product of `nprob` problems (a triangular grid and a triangular operand by their 64-wide tiles)
static inline double gemm_flops(int M, int N, int K, int tri, int lower_only, double nprob) {
    double flops = 2.0 * M * N * (double)K * nprob;
    if (lower_only) flops *= 0.5 * (1.0 + 64.0 / std::max(M, 64));
    if (tri) flops *= 0.5 * (1.0 + 64.0 / std::max(K, 64));
    return flops;
}
// the row of gemm_by_shape with this key (added at its first launch)
static int gemm_shape_row(gmrf_handle* h, const int64_t (&key)[8]) {
    for (size_t i = 0; i < h->gemm_shapes.size(); ++i)
        if (!memcmp(h->gemm_shapes[i].key, key, sizeof(key))) return (int)i;
    GemmShapeStat st; memcpy(st.key, key, sizeof(key));
    h->gemm_shapes.push_back(st);
    return (int)h->gemm_shapes.size() - 1;
}

// One dense product as gemm() takes it:  C = beta (D or C) + alpha op(A) op(B)  for every problem of the handle's batch, operand
// P of problem z at P + z pP.  The constructor and a() / b() / c() give what every product has; everything below them is OPTIONAL
// and absent unless the call site names it.  A new option is a new named field with its setter, absent by default.
struct GemmCall {
    bool a_t, b_n;                     // A stored [k][m] (else [m][k]); B stored [k][n] (else [n][k])
    int M, N, K;
    double alpha, beta;
    const double* A = nullptr; int64_t lda = 0, pA = 0;
    const double* B = nullptr; int64_t ldb = 0, pB = 0;
    double* C = nullptr; int64_t ldc = 0, pC = 0;
    int tri = 0, lower_only = 0;       // TRI_* of the operands; only the tiles on and below the block diagonal
    bool strict = false;               // with lower(): nothing strictly above the ELEMENT diagonal is needed (GemmArgs::strict_lower)
    int batch = 1; int64_t sA = 0, sB = 0, sC = 0;                 // products per problem, and their strides
    const double* D = nullptr; int64_t ldd = 0, pD = 0;            // addend (null: C, in place)
    int pclass = 0; double pwork = -1.0;                           // statistics class (0: by kernel) and work (< 0: the product's flops)
    // K bounds per 64-wide tile (GemmArgs): from max(kb_m[bm], kb_n[bn]) to min(ke_m[bm], ke_n[bn]).  ke_m is for the LDS-DMA
    // kernels only.  hints: the bounds are optional (the operands hold real zeros outside them) -- a launch that another kernel
    // family takes gets none of them and books its flops; ke_m is such a hint always
    const int* kb_m = nullptr; const int* kb_n = nullptr; const int* ke_m = nullptr; const int* ke_n = nullptr;
    bool hints = false;
    bool tail = false, tail_own = false;                           // one more row: row M of A / C, or (tail_own) on gt's operands
    GemmTail gt;

    GemmCall(bool a_t_, bool b_n_, int M_, int N_, int K_, double alpha_, double beta_)
        : a_t(a_t_), b_n(b_n_), M(M_), N(N_), K(K_), alpha(alpha_), beta(beta_) {}
    GemmCall& a(const double* p, int64_t ld, int64_t pp) { A = p; lda = ld; pA = pp; return *this; }
    GemmCall& b(const double* p, int64_t ld, int64_t pp) { B = p; ldb = ld; pB = pp; return *this; }
    GemmCall& c(double* p, int64_t ld, int64_t pp) { C = p; ldc = ld; pC = pp; return *this; }
    GemmCall& triangular(int flags) { tri = flags; return *this; }
    GemmCall& lower() { lower_only = 1; return *this; }
    GemmCall& strict_lower(bool on = true) { strict = on; return *this; }
    GemmCall& batched(int n, int64_t sa, int64_t sb, int64_t sc) { batch = n; sA = sa; sB = sb; sC = sc; return *this; }
    GemmCall& addend(const double* p, int64_t ld, int64_t pp) { D = p; ldd = ld; pD = pp; return *this; }
    GemmCall& work(double w, int cls = 0) { pwork = w; pclass = cls; return *this; }
    GemmCall& k_begin(const int* m, const int* n) { kb_m = m; kb_n = n; return *this; }
    GemmCall& k_end(const int* m, const int* n) { ke_m = m; ke_n = n; return *this; }
    GemmCall& k_hints(bool on = true) { hints = on; return *this; }
    GemmCall& tail_row(bool on = true) { tail = on; return *this; }
    GemmCall& tail_ops(const GemmTail* t) { if (t) { tail = tail_own = true; gt = *t; } return *this; }   // (null: none)
};

static void gemm_fill(const gmrf_handle* h, const GemmCall& c, GemmArgs& g) {
    if (c.tail_own) {
        const GemmTail& t = c.gt;
        if (t.C) { g.tA = t.A; g.ptA = t.pA; g.tC = t.C; g.ptC = t.pC; g.tD = t.D; g.ptD = t.pD; g.tbeta = t.beta; }
        g.dout = t.out; g.o_j0 = t.j0; g.o_cols = t.cols; g.o_n = h->n;
    }
    g.A = c.A; g.B = c.B; g.C = c.C; g.lda = c.lda; g.ldb = c.ldb; g.ldc = c.ldc; g.pA = c.pA; g.pB = c.pB; g.pC = c.pC;
    g.nb1 = c.batch; g.strideA = c.sA; g.strideB = c.sB; g.strideC = c.sC;
    g.D = c.D; g.ldd = c.ldd; g.pD = c.pD;
    g.M = c.M; g.N = c.N; g.K = c.K; g.tri = c.tri; g.lower_only = c.lower_only; g.alpha = c.alpha; g.beta = c.beta; g.stamps = nullptr;
    g.kb_m = c.kb_m; g.kb_n = c.kb_n; g.ke_n = c.ke_n; g.ke_m = c.ke_m;
    g.strict_lower = (c.strict && c.lower_only && c.M == c.N) ? 1 : 0;
}

// Runs one GEMM launch on the handle's GEMM stream -- run(stream, begin, end) -> hipError_t; when profiling, with an event pair
// for the dispatch's own begin / end time stamps (see launch_gemm) booked as {kind, work, gemm_by_shape row of `key`}
template <class Run>
static gmrf_status gemm_run(gmrf_handle* h, int kind, double work, const int64_t (&key)[8], Run&& run) {
    hipStream_t st = h->gemm_stream ? h->gemm_stream : h->stream;
    if (h->profiling <= 0) { HIPCHK(run(st, nullptr, nullptr)); return GMRF_OK; }
    EvPair p;
    p.kind = kind; p.work = work;
    p.a = ev_get(h); p.b = ev_get(h);
    p.shape = gemm_shape_row(h, key);
    HIPCHK(run(st, p.a, p.b));
    h->events.push_back(p);
    return GMRF_OK;
}

static gmrf_status gemm(gmrf_handle* h, const GemmCall& c) {
    GemmArgs g;
    gemm_fill(h, c, g);
    const bool a_t = c.a_t, b_n = c.b_n;
    const int M = c.M, nz = c.batch * (int)h->B;
    int pclass = c.pclass;
    double pwork = c.pwork;
    if ((g.ke_m || c.hints) && (gemm_uses_big(a_t, g, nz) || gemm_uses_ll(g, nz) || !gemm_uses_dma(a_t, g, nz))) {
        g.ke_m = nullptr;
        if (c.hints) { g.kb_m = g.kb_n = g.ke_n = nullptr; pwork = -1.0; }
    }
    double flops = gemm_flops(M, c.N, c.K, c.tri, c.lower_only, c.batch * (double)h->B);
    const int64_t bounded = (g.kb_m || g.kb_n || g.ke_n || g.ke_m) ? 1 : 0;
    if (c.tail) {
        // one more row, row M of A / C (gemm_f64_dma's TAIL): the kernel the M rows alone would get, or not at all.  A dry run
        // (tail_probe) only asks whether every product of a sweep qualifies.
        if (!gemm_tail_ok(a_t, b_n, g, nz)) {
            h->tail_refused = true;
            return h->tail_probe ? GMRF_OK : bad_shape("internal: a product does not qualify for the tail-row GEMM");
        }
        if (h->tail_probe) return GMRF_OK;
        flops *= (M + 1.0) / M;
        if (pwork >= 0.0) pwork *= (M + 1.0) / M;
        pclass = b_n ? 15 : 14;
    } else if (gemm_uses_big(a_t, g, nz)) {
        // statistics: launches of the 128 x 128 kernel are their own classes (6: B stored [n][k],
        // 7: B stored [k][n]) whoever calls, so that a class is one kernel symbol of a rocprof trace
        pclass = b_n ? 7 : 6; pwork = -1.0;
    } else if (pclass == 0) {
        if (gemm_uses_ll(g, nz)) pclass = 13;
        else if (gemm_uses_dma(a_t, g, nz)) pclass = a_t ? 18 : (b_n ? 15 : 14);   // gemm_f64_dma<.., B [n][k]> / <.., B [k][n]> / <.., A [k][m]>
        else pclass = a_t ? 12 : (b_n ? 11 : 0);
    }
    const int64_t key[8] = {pclass, c.tail ? M + 1 : M, c.N, c.K, c.tri, c.lower_only, c.batch * h->B, bounded};
    return gemm_run(h, pclass, pwork >= 0.0 ? pwork : flops, key, [&](hipStream_t st, hipEvent_t ea, hipEvent_t eb) {
        if (!c.tail) return launch_gemm(st, a_t, b_n, g, nz, ea, eb);
        hipError_t e = hipSuccess;
        (void)gemm_try_dma_tail(st, a_t, b_n, g, nz, ea, eb, &e);
        return e;
    });
}

// Two products neither of which reads what the other writes, as one launch of gemm_f64_dma_grouped where both qualify (and set_eager
// bit 20 does not keep them apart), else one after the other.  Both on A [m][k], one per problem, with no addend, K bounds or tail.
// Statistics: ONE launch of class 14 (the LDS-DMA kernel; the grouped symbol has no class of its own) with both products' work, and
// one gemm_by_shape row: M = both products' rows, tri / lower_only = the first product's flags | the second's << 8.
static gmrf_status gemm_pair(gmrf_handle* h, const GemmCall& q0, const GemmCall& q1) {
    GemmArgs g[2];
    const GemmCall* q[2] = {&q0, &q1};
    double work[2];
    for (int i = 0; i < 2; ++i) {
        const GemmCall& c = *q[i];
        if (c.a_t || c.batch != 1 || c.D || c.kb_m || c.kb_n || c.ke_m || c.ke_n || c.hints || c.tail || c.pclass)
            return bad_shape("internal: a product of a GEMM pair is on A [m][k], one per problem, with no addend, K bounds or tail");
        gemm_fill(h, c, g[i]);
        work[i] = c.pwork >= 0.0 ? c.pwork : gemm_flops(c.M, c.N, c.K, c.tri, c.lower_only, (double)h->B);
    }
    if (h->sw(GMRF_SW_NO_GROUPED_GEMM) || !gemm_grouped_ok(g[0], g[1], (int)h->B)) {
        GCHK(gemm(h, q0));
        return gemm(h, q1);
    }
    const int64_t key[8] = {14, q0.M + q1.M, q0.N, q0.K, q0.tri | (q1.tri << 8), q0.lower_only | (q1.lower_only << 8), h->B, 0};
    return gemm_run(h, 14, work[0] + work[1], key, [&](hipStream_t st, hipEvent_t ea, hipEvent_t eb) {
        hipError_t e = hipSuccess;
        (void)gemm_try_dma_grouped(st, q0.b_n, g[0], q1.b_n, g[1], (int)h->B, ea, eb, &e);
        return e;
    });
}

// element counts / strides of the factor arrays (doubles)
static inline int64_t blk_elems(const gmrf_handle* h) { return h->bsp * h->bsp; }
static inline int64_t c_ld(const gmrf_handle* h) { return h->bsp - h->cmin; }                      // row stride of a stored C_i
static inline int64_t c_blk(const gmrf_handle* h) { return h->rmax * (h->bsp - h->cmin); }         // one stored C_i
static inline int64_t stride_pL(const gmrf_handle* h) { return blk_elems(h) * (h->keep_l ? h->N : 1); }
static inline int64_t stride_pX(const gmrf_handle* h) { return blk_elems(h) * h->N; }
static inline int64_t stride_pC(const gmrf_handle* h) { return c_blk(h) * std::max<int64_t>(h->N - 1, 1); }
static inline double* l_block(const gmrf_handle* h, int64_t i) { return h->d_L + (h->keep_l ? i * blk_elems(h) : 0); }

// Layout of the coupling blocks (see gmrf_handle): validates, derives mend / the accounting sums and
// uploads the per-tile bounds.  kst_abs[t]: first non-zero column of row tile t (absolute, any value;
// it is rounded down to 64 and replaced by its monotone envelope).  Needs set_shape first.
// (host only: gmrf_test_coupling_plan reaches it without a device)
static void layout_kst(int64_t bsp, int64_t cmin, int64_t rmax, const std::vector<int64_t>& kst_abs, std::vector<int>& kst) {
    const int nrt = (int)(rmax / 64), ntile = (int)(bsp / 64);
    kst.assign((size_t)ntile, 0);
    int64_t run = bsp - 64;                                   // envelope from the bottom: kst[t] = min over t' >= t
    for (int t = nrt - 1; t >= 0; --t) {
        int64_t v = std::min(std::max(kst_abs[t], cmin), bsp - 64);
        run = std::min(run, (v / 64) * 64);
        kst[t] = (int)(run - cmin);
    }
    if (nrt > 0) kst[0] = 0;                                  // cmin is the smallest start by definition
    for (int t = nrt; t < ntile; ++t) kst[t] = (int)(bsp - cmin);         // rows below rmax: empty
}
static gmrf_status set_layout(gmrf_handle* h, int64_t cmin, int64_t rmax, const std::vector<int64_t>& kst_abs) {
    const int64_t bsp = h->bsp;
    if (cmin < 0 || cmin >= bsp || cmin % 64 || rmax <= 0 || rmax > bsp || rmax % 64) return bad_shape("bad coupling-block layout");
    const int nrt = (int)(rmax / 64), nct = (int)((bsp - cmin) / 64), ntile = (int)(bsp / 64);
    if ((int)kst_abs.size() != nrt) return bad_shape("bad coupling-block layout (row tiles)");
    (void)hipStreamSynchronize(h->stream);
    destroy_graphs(h);
    h->cmin = cmin; h->rmax = rmax;
    h->layout_gen++;
    h->env_ok = false;                                        // (the envelope bounds belong to the analysed pattern's layout: upload_envelope)
    layout_kst(bsp, cmin, rmax, kst_abs, h->kst);
    h->mend.assign((size_t)ntile, (int)rmax);
    for (int u = 0; u < nct; ++u) {
        int m = 0;
        for (int t = 0; t < nrt; ++t) if (h->kst[t] <= 64 * u) m = 64 * (t + 1);
        h->mend[u] = m;
    }
    h->c_streamed = 0.0; h->g2_tile_k = 0.0;
    for (int t = 0; t < nrt; ++t) {
        h->c_streamed += 64.0 * (double)(bsp - cmin - h->kst[t]);
        h->g2_tile_k += (double)(t + 1) * (double)(bsp - cmin - h->kst[t]);    // tiles (t, 0..t) start at kst[t]
    }
    GCHK(reserve_group(h->stream, {h->d_kst.want((size_t)ntile), h->d_mend.want((size_t)ntile), h->d_kbx.want((size_t)ntile)}));
    {
        std::vector<int> kbx((size_t)ntile);
        for (int u = 0; u < ntile; ++u) kbx[(size_t)u] = (int)std::max<int64_t>(0, 64 * (int64_t)u - cmin);
        HIPCHK(hipMemcpyAsync(h->d_kbx, kbx.data(), sizeof(int) * ntile, hipMemcpyHostToDevice, h->stream));
        HIPCHK(hipStreamSynchronize(h->stream));        // (kbx is a local)
    }
    HIPCHK(hipMemcpyAsync(h->d_kst, h->kst.data(), sizeof(int) * ntile, hipMemcpyHostToDevice, h->stream));
    HIPCHK(hipMemcpyAsync(h->d_mend, h->mend.data(), sizeof(int) * ntile, hipMemcpyHostToDevice, h->stream));
    HIPCHK(hipStreamSynchronize(h->stream));
    h->c_dirty = true;
    return GMRF_OK;
}

static gmrf_status set_layout_dense(gmrf_handle* h) {
    return set_layout(h, 0, h->bsp, std::vector<int64_t>((size_t)(h->bsp / 64), 0));
}

static gmrf_status alloc_work(gmrf_handle* h);
// The factor and the work blocks that follow its shape.  Caller-owned storage is let go of, not freed.
static void release_factor(gmrf_handle* h) {
    for (auto* a : {&h->d_L, &h->d_C, &h->d_Linv, &h->d_S, &h->d_B, &h->d_T, &h->d_W, &h->d_logdet}) a->release();
}
static gmrf_status alloc_factor(gmrf_handle* h) {
    if (h->alloc_N == h->N && h->alloc_bsp == h->bsp && h->alloc_B == h->B && h->alloc_rm == h->rmax &&
        h->alloc_wc == c_ld(h) && h->alloc_keep_l == h->keep_l && h->d_L && h->d_C && h->d_Linv && h->d_S && h->d_B && h->d_T &&
        h->d_W && h->d_logdet && h->d_pflags)
        return GMRF_OK;
    destroy_graphs(h);
    h->logdet_valid = false;
    if (h->external_storage) {
        // caller-owned L / C / Linv (sized by gmrf_bt_storage_bytes for this shape and batch): only the
        // work buffers follow the layout
        if (h->alloc_N != h->N || h->alloc_bsp != h->bsp || h->alloc_B != h->B || h->alloc_keep_l != h->keep_l) {
            g_last_error = "external factor storage does not match the shape / batch";
            return GMRF_ERR_BAD_SHAPE;
        }
        h->alloc_rm = h->rmax; h->alloc_wc = c_ld(h);
        h->l_valid = false;
        return GMRF_OK;
    }
    release_factor(h);
    h->l_valid = false;
    const size_t blk = (size_t)blk_elems(h) * sizeof(double) * (size_t)h->B;
    GCHK(reserve_group(h->stream, {h->d_L.want((size_t)blk_elems(h) * (size_t)h->B * (size_t)(h->keep_l ? h->N : 1)),
                                   h->d_Linv.want((size_t)stride_pX(h) * (size_t)h->B), h->d_C.want((size_t)stride_pC(h) * (size_t)h->B)}));
    // tiles strictly above the block diagonal of L / Linv are never written: keep them zero
    HIPCHK(hipMemsetAsync(h->d_L, 0, blk * (h->keep_l ? h->N : 1), h->stream));
    HIPCHK(hipMemsetAsync(h->d_Linv, 0, blk * h->N, h->stream));
    HIPCHK(hipMemsetAsync(h->d_C, 0, (size_t)stride_pC(h) * sizeof(double) * (size_t)h->B, h->stream));
    h->c_dirty = false;
    GCHK(alloc_work(h));
    h->alloc_rm = h->rmax; h->alloc_wc = c_ld(h); h->alloc_keep_l = h->keep_l;
    return GMRF_OK;
}

static gmrf_status alloc_work(gmrf_handle* h) {
    const size_t blk = (size_t)blk_elems(h) * sizeof(double) * (size_t)h->B;
    const size_t be = (size_t)blk_elems(h) * (size_t)h->B;
    GCHK(reserve_group(h->stream, {h->d_S.want(be), h->d_B.want(be), h->d_T.want(be), h->d_W.want(be), h->d_logdet.want((size_t)(h->N * h->B))}));
    {   // flag words of the persistent in-block launches (potrf_persist.hpp), one set per problem
        const size_t words = (size_t)persist_flag_words((int)(h->bsp / 64)) * (size_t)h->B;
        if (!h->d_pflags.fits(words)) {
            GCHK(h->d_pflags.reserve(h->stream, words));
            HIPCHK(hipMemsetAsync(h->d_pflags, 0, sizeof(unsigned) * words, h->stream));
            HIPCHK(hipStreamSynchronize(h->stream));     // (whatever stream the first launch is on later sees the zeros)
        }
    }
    h->alloc_N = h->N; h->alloc_bsp = h->bsp; h->alloc_B = h->B;
    h->stats.factor_bytes = (int64_t)(blk * ((h->keep_l ? 2 : 1) * h->N) + (size_t)stride_pC(h) * sizeof(double) * (size_t)h->B);
    return GMRF_OK;
}

// Buffers sized by n / n_pad / the batch: dropped whenever the shape or the batch changes
// (they are re-created on demand with the new sizes).
static void release_shape_buffers(gmrf_handle* h) {
    for (auto& kv : h->sweep_graphs) (void)hipGraphExecDestroy(kv.second);
    h->sweep_graphs.clear();
    for (auto* a : {&h->d_P, &h->d_Y, &h->d_Tp, &h->d_acc, &h->d_stage, &h->d_ft, &h->d_fy}) a->release();
    h->mean_arena.release();
    h->fy_for = nullptr;
}

static gmrf_status set_shape(gmrf_handle* h, int64_t n, int64_t N) {
    if (n <= 0 || N <= 0 || n % N != 0) return bad_shape("n must be a positive multiple of N_blocks");
    const int64_t bs = n / N;
    if (bs > (1 << 20)) return bad_shape("block size too large");
    if (h->n != n || h->N != N) {
        (void)hipStreamSynchronize(h->stream);
        destroy_graphs(h);
        release_shape_buffers(h);
        h->factored = false;
        h->analyzed = false;
    }
    h->n = n; h->N = N; h->bs = bs;
    h->layout_gen++;
    h->bsp = 64 * next_pow2((bs + 63) / 64);
    h->n_pad = h->bsp * N;
    h->stats.n = n; h->stats.n_blocks = N; h->stats.block_size = bs; h->stats.block_size_padded = h->bsp;
    h->stats.factor_flops = ((double)N * bs * bs * bs / 3.0 + (double)(N - 1) * 2.0 * bs * bs * bs) * (double)h->B;
    return GMRF_OK;
}

static gmrf_status ensure_panels(gmrf_handle* h, int64_t kp) {
    const size_t pe = (size_t)(kp * h->n_pad * h->B), te = (size_t)(kp * h->bsp * h->B);
    if (h->d_P.fits(pe) && h->d_Y.fits(pe) && h->d_Tp.fits(te)) return GMRF_OK;
    for (auto& kv : h->sweep_graphs) (void)hipGraphExecDestroy(kv.second);
    h->sweep_graphs.clear();
    return reserve_group(h->stream, {h->d_P.want(pe), h->d_Y.want(pe), h->d_Tp.want(te)});
}

static gmrf_status ensure_stage(gmrf_handle* h, int64_t elems) {
    return h->d_stage.reserve(h->stream, (size_t)elems);
}

// ------------------------------------------------------------------------------------ symbolic
struct HostEntry { uint64_t key; int64_t src; };

// Everything the symbolic phase derives on the HOST from the blocks' entry lists (no HIP call: the sanitizer build of the
// host side reaches it without a GPU through gmrf_test_symbolic_csc): the flat key / source arrays in block order (lower
// blocks row by row), the zero structure shared by all lower blocks (first non-zero column, last non-zero row, per 64-row
// tile the first non-zero column: the staircase), the row pointers into the lower blocks' entry lists, and the tile plan
// of the sparse C = B X^T (spmm_bxt_tiles: per lower block and 64-row tile the distinct columns, per entry its index).
struct SymbolicPlan {
    std::vector<int64_t> diag_first, diag_count, low_first, low_count;
    std::vector<uint64_t> keys;
    std::vector<int64_t> src;
    int64_t cmin = 0, rmax = 0;
    std::vector<int64_t> first;            // per 64-row tile of the window: first non-zero column (absolute)
    std::vector<int> rowptr;               // [N][bsp + 1]
    int64_t max_row = 0;
    bool sparse_b = false, bxt_ok = false;
    // tile plan of spmm_bxt_tiles, by GROUPS of up to three 64-row tiles of a lower block whose entries meet (mostly) the same
    // columns of X (round 4): per block the groups' tiles gtiles[N][nrt][3] (-1: none) and their count ng[N]; per group the
    // distinct columns (uptr[N][nrt + 1] into ucols), per entry its index into its group's list
    std::vector<int> uptr, ucols, gtiles, ng;
    std::vector<uint16_t> lidx;
    int ecap = 0, nrt = 0;
    std::vector<int> drowptr;          // [N][bsp + 1]: a diagonal block's entries row by row
    // (round 19) [N][bsp / 64], in-block columns: the rows of S_i = D_i - C C^T that the product does not write (all of block 0, rows
    // >= rmax otherwise) keep D_i's sparsity until a panel they meet has been eliminated.  env_lo: the smallest column of D_i in the
    // tile's rows (the diagonal counts), rounded down to 64 -- L is zero left of it (envelope theorem).  env_hi: the largest column
    // + 1 of D_i in those rows INSIDE the 256-column panel of env_lo, rounded up to 64 (no earlier panel has touched the rows, so
    // S[rows, panel] is still D_i's); the panel's end where the tile lies in that panel itself.  Other tiles: 0 and bsp.
    std::vector<int> env_lo, env_hi;
};

static void build_envelope(int64_t N, int64_t bsp, const std::vector<std::vector<HostEntry>>& dg, int64_t rmax, SymbolicPlan& sp) {
    const int nt = (int)(bsp / 64);
    sp.env_lo.assign((size_t)(N * nt), 0);
    sp.env_hi.assign((size_t)(N * nt), (int)bsp);
    std::vector<int64_t> lo((size_t)nt), hi((size_t)nt);
    for (int64_t i = 0; i < N; ++i) {
        const int64_t rm = i > 0 ? rmax : 0;
        for (int t = 0; t < nt; ++t) lo[(size_t)t] = 64 * (int64_t)t;
        for (auto& e : dg[(size_t)i]) {
            const int64_t r = (int64_t)(e.key >> 32), c = (int64_t)(e.key & 0xffffffffu);
            lo[(size_t)(r / 64)] = std::min(lo[(size_t)(r / 64)], c);
        }
        for (int t = 0; t < nt; ++t) { lo[(size_t)t] = lo[(size_t)t] / 64 * 64; hi[(size_t)t] = 0; }
        for (auto& e : dg[(size_t)i]) {
            const int64_t r = (int64_t)(e.key >> 32), c = (int64_t)(e.key & 0xffffffffu);
            const int64_t p0 = lo[(size_t)(r / 64)] / 256 * 256;
            if (c >= p0 && c < p0 + 256) hi[(size_t)(r / 64)] = std::max(hi[(size_t)(r / 64)], c + 1);
        }
        for (int t = 0; t < nt; ++t) {
            if (64 * (int64_t)t < rm) continue;
            const int64_t p0 = lo[(size_t)t] / 256 * 256;
            sp.env_lo[(size_t)(i * nt + t)] = (int)lo[(size_t)t];
            sp.env_hi[(size_t)(i * nt + t)] = (int)((64 * (int64_t)t < p0 + 256) ? std::min(p0 + 256, bsp) : (hi[(size_t)t] + 63) / 64 * 64);
        }
    }
}

static void build_symbolic(int64_t N, int64_t bsp, const std::vector<std::vector<HostEntry>>& dg,
                           const std::vector<std::vector<HostEntry>>& lo, bool no_staircase, SymbolicPlan& sp, bool group_tiles = true) {
    sp.diag_first.assign((size_t)N, 0); sp.diag_count.assign((size_t)N, 0);
    sp.low_first.assign((size_t)N, 0); sp.low_count.assign((size_t)N, 0);
    auto& keys = sp.keys; auto& src = sp.src;
    keys.clear(); src.clear();
    for (int64_t i = 0; i < N; ++i) {
        sp.diag_first[i] = (int64_t)keys.size(); sp.diag_count[i] = (int64_t)dg[i].size();
        {   // row by row too (round 5): the workgroups of spmm_bxt_tiles that zero rows of the next Schur block scatter D_i's rows into them
            std::vector<HostEntry> drow(dg[i]);
            std::stable_sort(drow.begin(), drow.end(), [](const HostEntry& x, const HostEntry& y) { return x.key < y.key; });
            for (auto& e : drow) { keys.push_back(e.key); src.push_back(e.src); }
        }
        sp.low_first[i] = (int64_t)keys.size(); sp.low_count[i] = (int64_t)lo[i].size();
        std::vector<HostEntry> byrow(lo[i]);           // row by row (key = row << 32 | col): spmm_bxt walks rows
        std::stable_sort(byrow.begin(), byrow.end(), [](const HostEntry& x, const HostEntry& y) { return x.key < y.key; });
        for (auto& e : byrow) { keys.push_back(e.key); src.push_back(e.src); }
    }
    // zero structure shared by all lower blocks (set_layout takes the monotone envelope of `first`)
    {
        int64_t cmin = bsp, rmax = 0;
        std::vector<int64_t> first((size_t)(bsp / 64), bsp);
        for (int64_t i = 1; i < N; ++i)
            for (auto& e : lo[i]) {
                const int64_t r = (int64_t)(e.key >> 32), c = (int64_t)(e.key & 0xffffffffu);
                cmin = std::min(cmin, c); rmax = std::max(rmax, r + 1);
                first[(size_t)(r / 64)] = std::min(first[(size_t)(r / 64)], c);
            }
        if (rmax == 0) { cmin = 0; rmax = 64; first[0] = 0; }
        cmin = (cmin / 64) * 64;
        rmax = std::min<int64_t>(bsp, (rmax + 63) / 64 * 64);
        first.resize((size_t)(rmax / 64));
        if (no_staircase) std::fill(first.begin(), first.end(), cmin);
        sp.cmin = cmin; sp.rmax = rmax; sp.first = first;
    }
    build_envelope(N, bsp, dg, sp.rmax, sp);
    // row pointers into the lower blocks' entry lists for the sparse C = B X^T (spmm_bxt)
    sp.rowptr.assign((size_t)(N * (bsp + 1)), 0);
    int64_t max_row = 0;
    for (int64_t i = 1; i < N; ++i) {
        int* rp = sp.rowptr.data() + i * (bsp + 1);
        const int64_t first = sp.low_first[i], cnt = sp.low_count[i];
        for (int64_t k = 0; k < cnt; ++k) rp[(keys[first + k] >> 32) + 1]++;
        for (int64_t r = 0; r < bsp; ++r) max_row = std::max<int64_t>(max_row, rp[r + 1]);
        rp[0] = (int)first;
        for (int64_t r = 0; r < bsp; ++r) rp[r + 1] += rp[r];
    }
    // row pointers into the diagonal blocks' entry lists (absolute positions in `keys`)
    sp.drowptr.assign((size_t)(N * (bsp + 1)), 0);
    if (keys.size() < ((size_t)1 << 31)) {
        for (int64_t i = 0; i < N; ++i) {
            int* rp = sp.drowptr.data() + i * (bsp + 1);
            const int64_t first = sp.diag_first[i], cnt = sp.diag_count[i];
            for (int64_t k = 0; k < cnt; ++k) rp[(keys[first + k] >> 32) + 1]++;
            rp[0] = (int)first;
            for (int64_t r = 0; r < bsp; ++r) rp[r + 1] += rp[r];
        }
    }
    // dense GEMM: 2 bs^3 flop at ~50 TF/s; sparse: one pass over C.  Rows of up to 32 entries go the sparse way,
    // anything denser keeps the GEMM.
    sp.max_row = max_row;
    sp.sparse_b = keys.size() < ((size_t)1 << 31) && max_row <= 32 && bsp >= 64;
    // tile plan for spmm_bxt_tiles (rows of the lower blocks are sorted by (row, column): a 64-row tile is a contiguous
    // range of entries)
    sp.bxt_ok = false; sp.uptr.clear(); sp.ucols.clear(); sp.lidx.clear(); sp.gtiles.clear(); sp.ng.clear();
    if (sp.sparse_b && N > 1) {
        // Row tiles whose entries meet the same columns share ONE gathered chunk of X inside a workgroup (a stencil block: the
        // tiles of mesh rows 2 and 3 of a block meet subsets of the columns the tile of mesh row 1 above them meets -- darcy256:
        // 195 + 129 + 64 gathered columns become 195).  Greedy: a tile joins the group of an earlier tile when at least half of
        // its columns are already there and the union still fits one thread per column.
        static const bool no_groups = env_int("GMRF_BXT_GROUPS", 1) == 0;   // every tile alone (the tests' bitwise reference)
        const int nrt = (int)(sp.rmax / 64);
        sp.uptr.assign((size_t)(N * (nrt + 1)), 0);
        sp.gtiles.assign((size_t)(N * nrt * 3), -1);
        sp.ng.assign((size_t)N, 0);
        sp.lidx.assign(std::max<size_t>(keys.size(), 1), 0);
        std::vector<std::vector<int>> cols((size_t)nrt);
        std::vector<int> uni, tmp;
        bool ok = true;
        int64_t pmax = 0;
        for (int64_t i = 1; i < N && ok; ++i) {
            const int* rp = sp.rowptr.data() + i * (bsp + 1);
            for (int rt = 0; rt < nrt; ++rt) {
                auto& c = cols[(size_t)rt];
                c.clear();
                for (int e = rp[rt * 64]; e < rp[rt * 64 + 64]; ++e) c.push_back((int)(keys[(size_t)e] & 0xffffffffu));
                std::sort(c.begin(), c.end());
                c.erase(std::unique(c.begin(), c.end()), c.end());
                if ((int)c.size() > BXT_UCAP) ok = false;
            }
            if (!ok) break;
            std::vector<char> taken((size_t)nrt, 0);
            int g = 0;
            for (int rt = 0; rt < nrt; ++rt) {
                if (taken[(size_t)rt]) continue;
                int* gt = sp.gtiles.data() + ((size_t)i * nrt + g) * 3;
                int cnt = 0;
                gt[cnt++] = rt; taken[(size_t)rt] = 1;
                uni = cols[(size_t)rt];
                for (int u = rt + 1; u < nrt && cnt < 3 && !no_groups && group_tiles; ++u) {
                    if (taken[(size_t)u] || cols[(size_t)u].empty()) continue;
                    tmp.clear();
                    std::set_union(uni.begin(), uni.end(), cols[(size_t)u].begin(), cols[(size_t)u].end(), std::back_inserter(tmp));
                    const size_t common = uni.size() + cols[(size_t)u].size() - tmp.size();
                    if (2 * common >= cols[(size_t)u].size() && tmp.size() <= (size_t)BXT_UCAP) {
                        gt[cnt++] = u; taken[(size_t)u] = 1;
                        uni.swap(tmp);
                    }
                }
                int64_t padded = 0;
                for (int q = 0; q < cnt; ++q) {
                    const int t = gt[q];
                    for (int e = rp[t * 64]; e < rp[t * 64 + 64]; ++e)
                        sp.lidx[(size_t)e] = (uint16_t)(std::lower_bound(uni.begin(), uni.end(), (int)(keys[(size_t)e] & 0xffffffffu)) - uni.begin());
                    for (int r = t * 64; r < t * 64 + 64; ++r) padded += (rp[r + 1] - rp[r] + 3) / 4 * 4;     // (the kernel pads a row to turns of 4 entries)
                }
                pmax = std::max(pmax, padded);
                sp.uptr[(size_t)(i * (nrt + 1) + g)] = (int)sp.ucols.size();
                sp.ucols.insert(sp.ucols.end(), uni.begin(), uni.end());
                ++g;
            }
            sp.uptr[(size_t)(i * (nrt + 1) + g)] = (int)sp.ucols.size();
            for (int q = g + 1; q <= nrt; ++q) sp.uptr[(size_t)(i * (nrt + 1) + q)] = (int)sp.ucols.size();
            sp.ng[(size_t)i] = g;
        }
        const int ecap = (int)std::max<int64_t>(64, (pmax + 63) / 64 * 64);
        if (ok && bxt_tile_lds_bytes(ecap) <= 53 * 1024) { sp.bxt_ok = true; sp.ecap = ecap; sp.nrt = nrt; }
    }
}

// (round 19) What potrf_block and the backward sweep pass of the envelope (gmrf_handle::env_host), per block and 256-column panel
// (gmrf_handle::env_host / env_ken / env_has / env_ken_has; any: some panel of some block has a non-trivial bound)
struct EnvHost { std::vector<int> host, ken; std::vector<unsigned char> has, ken_has; bool any = false; };
// (host only: gmrf_test_envelope_csc reaches it without a device)
static void derive_envelope(int64_t N, int64_t bsp, const SymbolicPlan& sp, EnvHost& o) {
    const int nt = (int)(bsp / 64), np = nt / 4;
    auto& env_host = o.host; auto& env_has = o.has; auto& env_ken = o.ken; auto& env_ken_has = o.ken_has;
    env_host.assign((size_t)(N * np * 4 * nt), 0);
    env_has.assign((size_t)(N * np), 0);
    env_ken.assign((size_t)(N * 4), 0);
    env_ken_has.assign((size_t)N, 0);
    bool any = false;
    for (int64_t i = 0; i < N; ++i)
        for (int p = 0; p < np; ++p) {
            const int oa = 256 * p, m3 = nt - 4 * p - 4;
            int* a = env_host.data() + (size_t)((i * np + p) * 4) * nt;
            unsigned char has = 0;
            for (int bm = 0; bm < m3; ++bm) {
                const int t = 4 * p + 4 + bm, lo = sp.env_lo[(size_t)(i * nt + t)], hi = sp.env_hi[(size_t)(i * nt + t)];
                const int kb = std::min(std::max(lo - oa, 0), 256);
                const int ke = (lo >= oa && lo < oa + 256) ? std::min(std::max(hi - oa, kb), 256) : 256;
                a[bm] = kb; a[nt + bm] = ke;
                const bool last = bm == m3 - 1;
                a[2 * nt + bm] = last ? 0 : kb; a[3 * nt + bm] = last ? 256 : ke;
                if (kb > 0) has |= 1;
                if (kb > 0 || ke < 256) has |= 2;
                if (!last && (kb > 0 || ke < 256)) has |= 4;
            }
            for (int bm = m3; bm < nt; ++bm) { a[bm] = a[2 * nt + bm] = 0; a[nt + bm] = a[3 * nt + bm] = 256; }
            env_has[(size_t)(i * np + p)] = has;
            any = any || has;
            if (p == 0 && m3 > 0) {
                // column tile bn of L[256:, 0:256] is non-zero in row tile bm only where kb[bm] <= 64 bn
                for (int bn = 0; bn < 4; ++bn) {
                    int end = 0;
                    for (int bm = 0; bm < m3; ++bm) if (a[bm] <= 64 * bn) end = 64 * (bm + 1);
                    env_ken[(size_t)(i * 4 + bn)] = end;
                    if (end < 64 * m3) env_ken_has[(size_t)i] = 1;
                }
            }
        }
    o.any = any;
}
static gmrf_status upload_envelope(gmrf_handle* h, const SymbolicPlan& sp) {
    h->env_ok = false;
    const int64_t N = h->N, bsp = h->bsp;
    const int nt = (int)(bsp / 64);
    if (N <= 0 || bsp % 256 != 0 || (int64_t)sp.env_lo.size() != N * nt) return GMRF_OK;
    h->env_lo = sp.env_lo; h->env_hi = sp.env_hi;
    EnvHost eh;
    derive_envelope(N, bsp, sp, eh);
    h->env_host.swap(eh.host); h->env_has.swap(eh.has); h->env_ken.swap(eh.ken); h->env_ken_has.swap(eh.ken_has);
    const bool any = eh.any;
    h->d_env.release(); h->d_env_ken.release();
    if (!any) return GMRF_OK;                                  // (no such structure: every launch as without the bounds)
    GCHK(reserve_group(h->stream, {h->d_env.want(h->env_host.size()), h->d_env_ken.want(h->env_ken.size())}));
    GCHK(h->d_env.upload(h->stream, h->env_host));
    GCHK(h->d_env_ken.upload(h->stream, h->env_ken));
    HIPCHK(hipStreamSynchronize(h->stream));
    h->env_ok = true;
    return GMRF_OK;
}

static gmrf_status upload_entries(gmrf_handle* h, const std::vector<std::vector<HostEntry>>& dg,
                                  const std::vector<std::vector<HostEntry>>& lo, int64_t nnz_in) {
    const int64_t N = h->N;
    SymbolicPlan sp;
    // (tile groups for batches: one problem alone has too few workgroups as it is -- 48 chunks x 12 tiles = 576 of 768 slots -- and
    //  a third of them doing three tiles' rows each is slower: 7.1 -> 9.7 us per block on darcy256)
    build_symbolic(N, h->bsp, dg, lo, h->sw(GMRF_SW_NO_STAIRCASE), sp, h->group_tiles_force >= 0 ? h->group_tiles_force != 0 : h->B >= 8);
    h->diag_first = sp.diag_first; h->diag_count = sp.diag_count; h->low_first = sp.low_first; h->low_count = sp.low_count;
    const auto& keys = sp.keys; const auto& src = sp.src;
    GCHK(set_layout(h, sp.cmin, sp.rmax, sp.first));
    GCHK(upload_envelope(h, sp));
    h->n_entries = (int64_t)keys.size();
    h->nnz_in = nnz_in;
    GCHK(reserve_group(h->stream, {h->d_keys.want(keys.size()), h->d_vals.want(keys.size() * (size_t)h->B), h->d_src.want(keys.size()),
                                   h->d_nz_stage.want((size_t)nnz_in * (size_t)h->B)}));
    h->vals_B = h->B;
    if (!keys.empty()) {
        // (stream-ordered copies + a stream wait: a synchronous hipMemcpy goes through the legacy stream,
        //  which HIP refuses while another host thread is capturing a graph)
        GCHK(h->d_keys.upload(h->stream, keys));
        GCHK(h->d_src.upload(h->stream, src));
        HIPCHK(hipStreamSynchronize(h->stream));
    }
    GCHK(h->d_lo_rowptr.upload(h->stream, sp.rowptr));
    GCHK(h->d_dg_rowptr.upload(h->stream, sp.drowptr));
    HIPCHK(hipStreamSynchronize(h->stream));
    h->lo_row_max = sp.max_row;
    h->sparse_b = sp.sparse_b;
    h->bxt_plan_ok = false;
    if (sp.bxt_ok) {
        GCHK(reserve_group(h->stream, {h->d_bxt_gtiles.want(sp.gtiles.size()), h->d_bxt_uptr.want(sp.uptr.size()),
                                       h->d_bxt_ucols.want(sp.ucols.size()), h->d_bxt_lidx.want(sp.lidx.size())}));
        GCHK(h->d_bxt_gtiles.upload(h->stream, sp.gtiles));
        h->bxt_ng = sp.ng;
        GCHK(h->d_bxt_uptr.upload(h->stream, sp.uptr));
        GCHK(h->d_bxt_ucols.upload(h->stream, sp.ucols));
        GCHK(h->d_bxt_lidx.upload(h->stream, sp.lidx));
        HIPCHK(hipStreamSynchronize(h->stream));
        h->bxt_ecap = sp.ecap; h->bxt_nrt = sp.nrt; h->bxt_plan_ok = true;
    }
    h->analyzed = true;
    h->factored = false;
    return GMRF_OK;
}

// The CSC walk of the symbolic phase (host only): which stored entries belong to which block; band check.
static gmrf_status split_csc(int64_t n, int64_t N, int64_t bs, const int64_t* colptr, const int64_t* rowval, int32_t base,
                             std::vector<std::vector<HostEntry>>& dg, std::vector<std::vector<HostEntry>>& lo) {
    dg.assign((size_t)N, {}); lo.assign((size_t)N, {});
    if (colptr[0] != base) return bad_shape("colptr must start at the index base");
    for (int64_t c = 0; c < n; ++c) {
        const int64_t bj = c / bs;
        if (colptr[c + 1] < colptr[c]) return bad_shape("colptr must be non-decreasing");
        for (int64_t p = colptr[c] - base; p < colptr[c + 1] - base; ++p) {
            const int64_t r = rowval[p] - base;
            if (r < 0 || r >= n) return bad_shape("row index out of range");
            const int64_t bi = r / bs;
            if (bi == bj) {
                if (r >= c) dg[bi].push_back({((uint64_t)(r - bi * bs) << 32) | (uint64_t)(c - bj * bs), p});
            } else if (bi == bj + 1) {
                lo[bi].push_back({((uint64_t)(r - bi * bs) << 32) | (uint64_t)(c - bj * bs), p});
            } else if (bi + 1 == bj) {
                // upper block: never read by the reference (src/tridiagonal_cholesky.jl:73,76)
            } else {
                g_last_error = "entry outside the block tri-band of the partition";
                return GMRF_ERR_BAND;
            }
        }
    }
    return GMRF_OK;
}

static gmrf_status analyze_csc(gmrf_handle* h, int64_t n, int64_t N, const int64_t* colptr,
                               const int64_t* rowval, int32_t base) {
    if (!colptr || !rowval) return bad_shape("null CSC arrays");
    GCHK(set_shape(h, n, N));
    std::vector<std::vector<HostEntry>> dg, lo;
    GCHK(split_csc(n, N, h->bs, colptr, rowval, base, dg, lo));
    return upload_entries(h, dg, lo, colptr[n] - base);
}

// blockIdx.y = problem: nzval of problem p starts at nz + p * nnz
__global__ void gather_values(const double* __restrict__ nz, const int64_t* __restrict__ src,
                              int64_t count, double* __restrict__ vals, int64_t nnz) {
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i < count) vals[(int64_t)blockIdx.y * count + i] = nz[(int64_t)blockIdx.y * nnz + src[i]];
}

static gmrf_status load_values(gmrf_handle* h, const double* nzval) {
    if (!nzval) return bad_shape("null nzval");
    const double* d_nz = nzval;
    if (h->vals_B != h->B) {            // batch size changed after the analysis: resize the value buffers
        GCHK(reserve_group(h->stream, {h->d_vals.want((size_t)(h->n_entries * h->B)), h->d_nz_stage.want((size_t)(h->nnz_in * h->B))}));
        h->vals_B = h->B;
    }
    if (!is_device_ptr(nzval)) {
        HIPCHK(hipMemcpyAsync(h->d_nz_stage, nzval, sizeof(double) * h->nnz_in * h->B, hipMemcpyHostToDevice, h->stream));
        d_nz = h->d_nz_stage;
    }
    if (h->n_entries > 0) {
        const int bl = 256;
        hipLaunchKernelGGL(gather_values, dim3((unsigned)((h->n_entries + bl - 1) / bl), (unsigned)h->B), dim3(bl), 0,
                           h->stream, d_nz, h->d_src, h->n_entries, h->d_vals, h->nnz_in);
        HIPCHK(hipGetLastError());
    }
    return GMRF_OK;
}

// ------------------------------------------------------------------------------------ numeric factor
// One doubling pair  T21 = L21 X11,  X21 = -X22 T21  on the m x n block at rows r .., columns c .. of L (problem stride pL), X and
// T:  X11 = X[c:c+n, c:c+n] and X22 = X[r:r+m, r:r+m], both lower triangular.  `pairs` such blocks, `st` elements apart, in one
// launch each.  which: bit 0 the first product, bit 1 the second.
static gmrf_status doubling_pair(gmrf_handle* h, const double* L, int64_t pL, double* X, double* T, int r, int c, int m, int n,
                                 int pairs, int64_t st, int which = 3) {
    const int64_t ld = h->bsp, pX = stride_pX(h), pW = ld * ld, o21 = r * ld + c;
    if (which & 1)
        GCHK(gemm(h, GemmCall(false, true, m, n, n, 1.0, 0.0).a(L + o21, ld, pL).b(X + c * ld + c, ld, pX).c(T + o21, ld, pW)
                         .triangular(TRI_B_LOWER).batched(pairs, st, st, st)));
    if (which & 2)
        GCHK(gemm(h, GemmCall(false, true, m, n, m, -1.0, 0.0).a(X + r * ld + r, ld, pX).b(T + o21, ld, pW).c(X + o21, ld, pX)
                         .triangular(TRI_A_LOWER).batched(pairs, st, st, st)));
    return GMRF_OK;
}

// Recursive doubling  X21 = -X22 (L21 X11)  over pairs of hh-wide diagonal blocks, levels hh = lo .. hi.
// half: -1 all pairs, 0 / 1 only the pairs inside the first / second half of the block.
static gmrf_status doubling_levels(gmrf_handle* h, double* L, double* X, double* T, int lo, int hi, int half, int split = 0) {
    const int bsp = (int)h->bsp;
    if (split > 0 && half >= 0) return bad_shape("internal: the split inverse is not assembled half by half");
    for (int hh = lo; hh <= hi && hh < bsp; hh *= 2) {
        int pairs = bsp / (2 * hh), first = 0;
        if (half >= 0) { pairs /= 2; first = half * pairs; }
        if (split > 0 && hh >= split) {
            // split representation (split = p, a power of two): the first block column [0, p) of the rows >= p is not
            // assembled.  Level p: the first pair IS that part; above: the first pair keeps its columns [p, hh) --
            // T[:, p:hh] = L21[:, p:hh] X11[p:hh, p:hh],  X21[:, p:hh] = -X22 T[:, p:hh]
            if (hh > split) GCHK(doubling_pair(h, L, stride_pL(h), X, T, hh, split, hh, hh - split, 1, 0));
            first = 1; pairs -= 1;
        }
        if (pairs <= 0) continue;
        GCHK(doubling_pair(h, L, stride_pL(h), X, T, first * 2 * hh + hh, first * 2 * hh, hh, hh, pairs, (int64_t)2 * hh * bsp + 2 * hh));
    }
    return GMRF_OK;
}

// The top level (hh = bsp / 2, one pair) in its two halves: T21 = L21 X11, then X21 = -X22 T21.
static gmrf_status doubling_top(gmrf_handle* h, double* L, double* X, double* T, bool first_product, bool second_product) {
    const int hh = (int)h->bsp / 2;
    return doubling_pair(h, L, stride_pL(h), X, T, hh, 0, hh, hh, 1, 0, (first_product ? 1 : 0) | (second_product ? 2 : 0));
}

static gmrf_status fork_event(gmrf_handle* h, hipEvent_t* out) {
    if (h->fork_next == h->fork_events.size()) {
        hipEvent_t e;
        HIPCHK(hipEventCreateWithFlags(&e, hipEventDisableTiming));
        h->fork_events.push_back(e);
    }
    *out = h->fork_events[h->fork_next++];
    return GMRF_OK;
}

// Which in-block Cholesky the next factorisation of this handle takes: the ONE route predicate (potrf_block follows it,
// planned_xsplit asks it; round 5 -- the comparison routes that lost twice, left-looking panels, rank-64 panel steps of batches,
// 128-column panels and the one-workgroup potrf_panel256, are gone, and with them four flags both places had to agree on by hand).
enum PotrfRoute {
    ROUTE_FUSED = 1,       // one problem, blocks of up to 16 tiles: ONE persistent launch per block, else one launch per 64-column step
    ROUTE_BIG_ONE = 2,     // one problem, larger blocks: 256-column panels, each a persistent launch (or fused steps) + a rank-256 GEMM
    ROUTE_PANELS256 = 3,   // batches: 256-column panels -- potrf_diag128 x 2 + 128^3 GEMMs, or one persistent launch per diagonal block -- + GEMM
    ROUTE_STEPS = 4        // what is left (blocks of fewer than 4 tiles, tile counts not divisible by 4, the forked graph): tile, panel, update
};
static int potrf_route(const gmrf_handle* h) {
    const int nt = (int)(h->bsp / 64);
    if (h->B == 1 && !h->sw(GMRF_SW_BATCH_ROUTES)) return nt <= 16 ? ROUTE_FUSED : ROUTE_BIG_ONE;
    if (h->sw(GMRF_SW_FORK_GRAPH) && nt >= 8) return ROUTE_STEPS;
    return (nt >= 4 && nt % 4 == 0) ? ROUTE_PANELS256 : ROUTE_STEPS;
}

// (round 29) May the symmetric products into the Schur block S -- G2, the rank-256 updates, the 128^2 S_BB update -- leave the
// 16 x 16 blocks strictly above the diagonal of S's diagonal tiles unwritten (GemmCall::strict_lower)?  Only where every reader
// of a diagonal tile of S has been read for it ([r29]: the 256-column panel route of batches, whose readers are
// potrf_diag128 / potrf_diag128_slim and the persistent diagonal-block launch); one problem, the twisted order and the
// launch-per-step route keep whole tiles.
static bool strict_lower_route(const gmrf_handle* h) {
    return h->B > 1 && potrf_route(h) == ROUTE_PANELS256 && !h->tw && !h->tw_half && h->tw_blk < 0;
}

// The split the next factorisation of this handle will use (0: none): only the 256-column panel route of batches
// assembles the inverse level by level, and only a coupling window that starts at cmin >= 256 leaves a first block
// column nobody multiplies with.  p = the largest power of two <= cmin (the doubling tree splits at powers of two).
static int planned_xsplit(const gmrf_handle* h) {
    const int bsp = (int)h->bsp, nt = bsp / 64;
    if (h->sw(GMRF_SW_NO_XSPLIT) || h->N <= 0 || nt < 8 || potrf_route(h) != ROUTE_PANELS256) return 0;
    int p = 256;
    while (2 * p <= (int)h->cmin) p *= 2;
    return (h->cmin >= 256 && p < bsp) ? p : 0;
}

// ---- the device's budget of CUs for persistent launches (round 5) --------------------------------------------------------
// Every workgroup of a potrf_persist launch must be resident at once (140 KB of LDS: one per CU).  One handle alone checks its
// launch against the CU count; several handles' launches in flight together -- a StreamSet of batched handles, two one-problem
// handles on two threads -- can together ask for more than the chip has, end up partially resident and starve each other until
// their bounded waits give up (0.2 - 2 s each).  So a handle CLAIMS the CUs its widest persistent launch needs when it plans a
// factorisation, the claims of a device never exceed its CU count, and a handle whose claim does not fit takes the launch-per-
// step routes up front (stats: persist_refused).  A claim is held until the handle is destroyed, gives a launch up, or
// re-plans with another shape: the route of a handle does not depend on what other handles happen to be doing at the moment.
static std::mutex g_persist_mu;
static std::map<int, std::map<const void*, int>> g_persist_claims;     // device -> handle -> CUs

// `who` asks for `want` CUs of a device with `cus`: true and recorded when it fits beside the others' claims (want = 0 releases)
static bool persist_budget_claim(std::map<const void*, int>& claims, const void* who, int want, int cus) {
    int others = 0;
    for (const auto& kv : claims) if (kv.first != who) others += kv.second;
    if (want <= 0 || others + want > cus) { claims.erase(who); return false; }
    claims[who] = want;
    return true;
}

// persistent launches are open to this handle: not switched off, and no launch of its own has given up
static bool persist_allowed(const gmrf_handle* h) { return !h->sw(GMRF_SW_NO_PERSIST) && !h->persist_gave_up; }
// CUs the widest persistent launch of this handle's next factorisation needs at once (0: its route launches none)
static int persist_demand(const gmrf_handle* h) {
    if (!persist_allowed(h) || h->cu_count <= 0 || h->bsp < 128 || h->sw(GMRF_SW_FORK_GRAPH)) return 0;
    const int nt = (int)(h->bsp / 64);
    int64_t wgs = 0;
    switch (potrf_route(h)) {
        case ROUTE_FUSED: if (!h->sw(GMRF_SW_NO_LOOKAHEAD) && !h->sw(GMRF_SW_DOUBLING_INVERSE)) wgs = 1 + persist_tiles(nt, 0, nt, 1); break;
        case ROUTE_BIG_ONE: if (!h->sw(GMRF_SW_NO_LOOKAHEAD)) wgs = 1 + persist_tiles(nt, 0, std::min(nt, 4), 0); break;      // (the first panel is the widest)
        case ROUTE_PANELS256: if (!h->sw(GMRF_SW_NO_PERSIST_PANELS)) wgs = 1 + persist_tiles(4, 0, 4, 2); break;
        default: break;
    }
    wgs *= h->B;
    return wgs > 0 && wgs <= h->cu_count ? (int)wgs : 0;
}
// One problem with blocks of 512 .. 1024: its sweeps run as one persistent launch each (sweep_persist.hpp), whose workgroups --
// one per CU, up to 256 -- must all be resident: the handle then asks for the whole chip.  0: the sweeps keep a launch per product.
static int sweep_persist_demand(const gmrf_handle* h) {
    if (!persist_allowed(h) || h->sw(GMRF_SW_NO_SWEEP_PERSIST) || h->cu_count < 64 || h->B != 1) return 0;
    if (!h->d_kst || !h->d_mend) return 0;             // (a handle that adopted a factor without analysing a pattern)
    if (h->bsp < 512 || h->bsp > SWEEP_PERSIST_XMAX || h->bsp % 64 != 0 || h->cmin % 16 != 0 || h->rmax % 16 != 0) return 0;      // (the bodies' tilings: 16 rows, 8 / 16 columns)
    return h->cu_count;
}
// plan the persistent launches of the next factorisation: claim (or release) this handle's CUs
static void persist_plan(gmrf_handle* h) {
    const int want_f = persist_demand(h), want_s = sweep_persist_demand(h);
    int want = std::max(want_f, want_s);
    bool ok;
    {
        std::lock_guard<std::mutex> lock(g_persist_mu);
        ok = persist_budget_claim(g_persist_claims[h->device], h, want, h->cu_count);
        if (!ok && want_f > 0 && want_f < want) {          // (the whole chip is not free: the factorisation's launches alone)
            want = want_f;
            ok = persist_budget_claim(g_persist_claims[h->device], h, want, h->cu_count);
        }
    }
    h->sweep_persist_planned = ok && want_s > 0 && want >= want_s;
    const int got = ok ? want : 0;
    if (got != h->persist_cus) destroy_graphs(h);              // (a captured factor graph holds the launches of the old plan)
    h->persist_cus = got;
    h->stats.persist_cus = got;
    h->stats.persist_refused = (want > 0 && !ok) ? 1 : 0;
}
static void persist_release(gmrf_handle* h) {
    std::lock_guard<std::mutex> lock(g_persist_mu);
    auto it = g_persist_claims.find(h->device);
    if (it != g_persist_claims.end()) it->second.erase(h);
    h->persist_cus = 0;
    h->stats.persist_cus = 0;
    h->sweep_persist_planned = false;
}

// A bounded wait inside a persistent launch gave up: this handle keeps the launch-per-step / per-product forms for good, lets go
// of its claim and drops the captured graphs that hold such launches.  (The caller resets its abort word and repeats its work.)
static void persist_give_up(gmrf_handle* h) {
    h->persist_gave_up = true; h->persist_aborts++;
    h->stats.persist_aborts = h->persist_aborts;
    persist_release(h);
    destroy_graphs(h);
}

// One persistent launch (potrf_persist.hpp) over the column tiles [j0, j1) of a block of nt tiles (its flag words are zero
// between launches: the last workgroup out of a launch leaves them so).  false: the handle holds no claim that covers this
// shape (it does not fit the chip beside the other handles' launches, or the form is switched off).
static bool persist_fits(const gmrf_handle* h, int nt, int j0, int j1, int xrows) {
    if (!persist_allowed(h) || h->persist_cus <= 0) return false;
    // (a batch: every problem brings its own set of workgroups and flag words; all of them must fit the claim at once)
    return (int64_t)(1 + persist_tiles(nt, j0, j1, xrows)) * h->B <= h->persist_cus;
}

static gmrf_status launch_persist(gmrf_handle* h, double* S, double* L, double* X, int nt, int j0, int j1, int xrows, int blk_id,
                                  double flops) {
    const int words = persist_flag_words(nt);
    if (!h->d_pflags.fits((size_t)((int64_t)words * h->B))) return bad_shape("internal: flag words of the persistent launches not allocated");
    // (no memset node: the words are zero -- zeroed when allocated, left zero by the last workgroup out of every launch)
    PersistArgs pa;
    pa.S = S; pa.L = L; pa.X = X; pa.ld = h->bsp; pa.nt = nt; pa.j0 = j0; pa.j1 = j1; pa.xrows = xrows;
    pa.tail_panel = (!xrows && j1 < nt) ? 1 : 0;
    pa.info = h->d_info; pa.blk = blk_id;
    pa.pS = h->bsp * h->bsp; pa.pL = stride_pL(h); pa.pX = stride_pX(h); pa.blk_per_problem = (int)h->N;
    pa.flags = h->d_pflags; pa.flag_stride = words;
    pa.abort_word = reinterpret_cast<unsigned*>(h->d_info + 1);
    // Bound of every wait, in ticks of the 100 MHz clock: 2 s for one problem; 200 ms for a batch -- several handles' launches
    // can ask for more workgroups than the chip has CUs (each must be resident as a whole), and if they ever hold each other's
    // CUs the handles should learn it soon, drain, and go on with the other route (a launch lasts 60 us; a wait that is
    // honest ends within a few GEMM launches of another stream).
    static const int limit_ms = env_int("GMRF_PERSIST_SPIN_MS", -1);
    pa.spin_limit = (unsigned)(limit_ms >= 0 ? limit_ms : (h->B > 1 ? 200 : 2000)) * 100000u;
    pa.stamps = h->dbg_stamps;
    h->persist_launched = true;
    h->stats.persist_route = xrows == 1 ? 1 : (xrows == 0 ? 2 : 3);
    ProfScope ps(h, 17, flops);                        // (its own class: the rocprof symbol is potrf_persist, not potrf_step)
    hipLaunchKernelGGL(potrf_persist<false>, dim3(1 + persist_tiles(nt, j0, j1, xrows), (unsigned)h->B), dim3(POTRF_PERSIST_THREADS), POTRF_PERSIST_LDS,
                       h->stream, pa);
    HIPCHK(hipGetLastError());
    return GMRF_OK;
}

// (round 19) The envelope bounds of block i's panel p for the panel product (pp_kb / pp_ke: GemmArgs::kb_m / ke_m) and the rank-256
// update (upd_kb: kb_m and kb_n), null where the panel has none (or set_eager bit 21, one problem, a twisted order: the launches of
// before), and the 64-wide K units the two launches then execute -- what their ProfScope books, as G2's g2_tile_k does.
struct EnvPanel { const int* pp_kb; const int* pp_ke; const int* upd_kb; double units_pp, units_upd; };
// 64-wide K units the panel product (rows a / a + 1 of a panel's four bound arrays: kb / ke) and the update (kb) execute
static double env_units_pp(const int* host, int nt, int m3, int a) {
    double u = 0.0;
    for (int bm = 0; bm < m3; ++bm)
        for (int bn = 0; bn < 4; ++bn) u += std::max(0, std::min(64 * (bn + 1), host[(a + 1) * nt + bm]) - host[a * nt + bm]) / 64;
    return u;
}
static double env_units_upd(const int* host, int m3) {
    double u = 0.0;
    for (int bm = 0; bm < m3; ++bm)
        for (int bn = 0; bn <= bm; ++bn) u += (256 - std::max(host[bm], host[bn])) / 64;
    return u;
}
static EnvPanel env_panel(const gmrf_handle* h, int64_t i, int p, bool tail_rides) {
    const int nt = (int)(h->bsp / 64), np = nt / 4, m3 = nt - 4 * p - 4;
    EnvPanel e{nullptr, nullptr, nullptr, 10.0 * m3, 4.0 * (m3 * (m3 + 1) / 2)};
    if (!h->env_ok || h->sw(GMRF_SW_NO_ENVELOPE) || h->B <= 1 || h->tw || h->tw_half || h->tw_blk >= 0 || i < 0 || i >= h->N || p < 0 || p >= np || m3 <= 0) return e;
    const size_t at = (size_t)((i * np + p) * 4) * nt;
    const unsigned char has = h->env_has[(size_t)(i * np + p)];
    const int* host = h->env_host.data() + at;
    if (has & (tail_rides ? 4 : 2)) {
        const int a = tail_rides ? 2 : 0;
        e.pp_kb = h->d_env + at + (size_t)a * nt; e.pp_ke = h->d_env + at + (size_t)(a + 1) * nt;
        e.units_pp = env_units_pp(host, nt, m3, a);
    }
    if (has & 1) {
        e.upd_kb = h->d_env + at;
        e.units_upd = env_units_upd(host, m3);
    }
    return e;
}

// The factor's three tail-carrying products, one builder each: factor_blocks_range / potrf_block launch what they return, and
// factor_fwd_ok asks gemm() about the same descriptions in a dry run.
// G2 of block i >= 1,  S = D - C C^T  (src/tridiagonal_cholesky.jl:77): the product part.  Tile (R, R') sums over the columns from
// max(kst[R], kst[R']) on -- the rest of the two row tiles is structurally zero.  accumulate: D_i is in S already.
// (tail: the forward solve's row, y_{i-1}'s window against C^T, gives t = b_i - C y_{i-1} for the rows below rmax)
static GemmCall g2_product(const gmrf_handle* h, int64_t i, bool accumulate, bool tail) {
    const int bsp = (int)h->bsp, cm = (int)h->cmin, rm = (int)h->rmax;
    const double* C = h->d_C + (i - 1) * c_blk(h);
    const GemmTail tg{h->d_fy + (i - 1) * bsp + cm, h->n_pad, h->d_ft, bsp, nullptr, 0, 1.0};
    return GemmCall(false, false, rm, rm, bsp - cm, -1.0, accumulate ? 1.0 : 0.0).a(C, c_ld(h), stride_pC(h)).b(C, c_ld(h), stride_pC(h))
        .c(h->d_S, bsp, (int64_t)bsp * bsp).lower().strict_lower(strict_lower_route(h)).work(2.0 * 64.0 * 64.0 * h->g2_tile_k * (double)h->B)
        .k_begin(h->d_kst, h->d_kst).tail_ops(tail ? &tg : nullptr);
}
// The 256-column panel at column tile j of a block (S, L, X) with rows below it, and the bounds `ev` of its envelope (env_panel):
// where L[below, P] lies.  Split representation with p = the panel width and no L blocks kept: L[p:, 0:p] is read by this panel's
// own update only, so it is formed directly in the place it takes in Linv's storage (see gmrf_handle::xsplit)
struct PanelBelow { double* Lb; int64_t pLb; };
static PanelBelow panel_below(const gmrf_handle* h, double* L, double* X, int j) {
    const int64_t at = ((int64_t)j * 64 + 256) * h->bsp + (int64_t)j * 64;
    const bool in_slot = (j == 0 && h->xsplit == 256 && !h->keep_l);
    return in_slot ? PanelBelow{X + at, stride_pX(h)} : PanelBelow{L + at, stride_pL(h)};
}
// L[below, P] = S[below, P] X_P^T: b(k, n) = X_P[n][k], zero for k > n (tile-K units: 1 + 2 + 3 + 4 of 16).
// fy (this block's part of the forward solve, or null): y_P = X_P t_P is the product's tail row
static GemmCall panel_product(const gmrf_handle* h, double* S, double* L, double* X, int j, const EnvPanel& ev, double* fy) {
    const int64_t ld = h->bsp, oa = (int64_t)j * 64, oc = oa + 256;
    const int m3 = (int)(ld / 64) - j - 4;
    const PanelBelow lb = panel_below(h, L, X, j);
    const GemmTail tp{h->d_ft + oa, ld, fy + oa, h->n_pad, nullptr, 0, 0.0};
    return GemmCall(false, false, 64 * m3, 256, 256, 1.0, 0.0).a(S + oc * ld + oa, ld, ld * ld).b(X + oa * ld + oa, ld, stride_pX(h))
        .c(lb.Lb, ld, lb.pLb).triangular(TRI_B_UPPER).work(2.0 * 64.0 * 64.0 * 64.0 * ev.units_pp * (double)h->B)
        .k_begin(ev.pp_kb, nullptr).k_end(ev.pp_ke, nullptr).k_hints().tail_ops(fy ? &tp : nullptr);
}
// S[r,c] -= L[r,P] L[c,P]^T for the tiles right of / below the panel.  fy: t[below] -= L[below, P] y_P is the update's tail row
static GemmCall panel_update(const gmrf_handle* h, double* S, double* L, double* X, int j, const EnvPanel& ev, double* fy) {
    const int64_t ld = h->bsp, oa = (int64_t)j * 64, oc = oa + 256;
    const int m3 = (int)(ld / 64) - j - 4;
    const PanelBelow lb = panel_below(h, L, X, j);
    const GemmTail tu{fy + oa, h->n_pad, h->d_ft + oc, ld, nullptr, 0, 1.0};
    return GemmCall(false, false, m3 * 64, m3 * 64, 256, -1.0, 1.0).a(lb.Lb, ld, lb.pLb).b(lb.Lb, ld, lb.pLb).c(S + oc * ld + oc, ld, ld * ld)
        .lower().strict_lower(strict_lower_route(h)).work(2.0 * 64.0 * 64.0 * 64.0 * ev.units_upd * (double)h->B).k_begin(ev.upd_kb, ev.upd_kb).k_hints()
        .tail_ops(fy ? &tu : nullptr);
}

// fy (batches on the 256-column panel route, factor_fwd_ok): also y_i = L_i^-1 t into fy ([B][n_pad]: this block's part), t = d_ft
static gmrf_status potrf_block(gmrf_handle* h, double* S, double* L, double* X, double* T, int blk_id, double* fy = nullptr) {
    const int bsp = (int)h->bsp;
    const int64_t ld = bsp;
    const int nt = bsp / 64;
    // Batches: two-level blocking.  Inside a 256-column panel the 64-column steps update only the
    // panel's own columns; the rest of the trailing block gets ONE rank-256 update per panel from
    // the GEMM kernel (a quarter of the read-modify-write traffic of four rank-64 updates, and
    // one rounding at |S| instead of four).  A lone problem with blocks up to 1024 keeps the fused
    // one-launch step (43 ms against 48 ms on darcy256); beyond that the fused step's redundant
    // tile factorisations lose (bs = 4096: 4.45 s fused, 2.93 s two-level).
    const int route = potrf_route(h);
    const bool fused = route == ROUTE_FUSED;
    if (h->xsplit > 0 && route != ROUTE_PANELS256) return bad_shape("internal: split inverse planned off the 256-column panel route");
    static const int pw_env = env_int("GMRF_PANEL_TILES", 4);      // (tests pin the widths 2 and 8)
    const int pw = (!fused && nt >= 8) ? ((pw_env == 2 || pw_env == 8) ? pw_env : 4) : nt;           // panel width in tiles
    // a lone problem with larger blocks: two-level, with the fused kernel restricted to the panel's
    // own columns as the in-panel step (one launch instead of three where the panel has columns left)
    const bool fused_in_panel = route == ROUTE_BIG_ONE;
    // Opt-in (set_eager bit 4): inside a captured graph the block forks once its first half is
    // factored: a second branch assembles the inverse of that half and the top-level product
    // T21 = L21 X11 (everything they read is final) while this branch runs the latency-bound panel
    // chain of the second half.  Measured on darcy256: the branches do overlap (3.4 ms of a 42 ms
    // factor) but the two cross-queue dependencies per block cost as much, and with several handles
    // the extra streams share hardware queues (3 x 32: 22.6 k -> 19.3 k solves/s).  Off by default.
    const bool overlap = h->capturing && h->sw(GMRF_SW_FORK_GRAPH) && nt >= 8;
    if (overlap && !h->aux) HIPCHK(hipStreamCreateWithFlags(&h->aux, hipStreamNonBlocking));
    hipEvent_t ev_fork = nullptr, ev_join = nullptr;
    if (overlap) { GCHK(fork_event(h, &ev_fork)); GCHK(fork_event(h, &ev_join)); }
    if (fused && !h->sw(GMRF_SW_NO_LOOKAHEAD) && !h->sw(GMRF_SW_DOUBLING_INVERSE) && !overlap && nt >= 2 && persist_fits(h, nt, 0, nt, 1)) {
        // One problem, ONE launch per block: the look-ahead chain below with flags in place of its launch boundaries
        // (potrf_persist.hpp)
        const double t3 = 64.0 * 64.0 * 64.0;
        double fl = t3 / 3.0 * nt;
        for (int j = 0; j + 1 < nt; ++j) {
            const int m = nt - j - 1;
            fl += (double)m * t3 + 2.0 * t3 * (m * (m + 1) / 2) + 2.0 * t3 * (0.5 * (double)(j + 1) * (j + 2) + 0.625 * (j + 1));
        }
        return launch_persist(h, S, L, X, nt, 0, nt, 1, blk_id, fl);
    }
    if (fused && !h->sw(GMRF_SW_NO_LOOKAHEAD) && !h->sw(GMRF_SW_DOUBLING_INVERSE) && !overlap && nt >= 2) {
        // One problem, look-ahead chain (potrf_step, `lookahead`): tile 0 alone, then per step j ONE launch in which
        // workgroup 0 forms L[j+1,j], updates tile (j+1,j+1) in LDS and factors it for the next launch while the other
        // workgroups do panel + update of their tiles with the X_jj the previous launch left; the tiles of row j of
        // the inverse ride along (xrow_strip), its last row gets the launch at the end.
        StepArgs sa;
        sa.S = S; sa.L = L; sa.X = X; sa.ld = ld; sa.nt = nt; sa.cend = nt;
        sa.info = h->d_info; sa.blk = blk_id; sa.dbg = nullptr;
        sa.pS = (int64_t)bsp * bsp; sa.pL = stride_pL(h); sa.pX = stride_pX(h); sa.blk_per_problem = (int)h->N;
        const double t3 = 64.0 * 64.0 * 64.0;
        {
            sa.j = 0; sa.lookahead = 0; sa.xrow = -1;
            ProfScope ps(h, 1, t3 / 3.0);
            hipLaunchKernelGGL(potrf_step<false>, dim3(1, 1), dim3(256), POTRF_TILE_LDS, h->stream, sa);
        }
        for (int j = 0; j + 1 < nt; ++j) {
            const int m = nt - j - 1, ntile_wg = m * (m + 1) / 2;
            sa.j = j; sa.lookahead = 1;
            sa.xrow = (j >= 1) ? j : -1; sa.xrow_first = ntile_wg;
            const int nx_wg = (j >= 1) ? 4 * j : 0;
            const double f_x = (j >= 1) ? 2.0 * t3 * (0.5 * (double)j * (j + 1) + 0.625 * j) : 0.0;
            ProfScope ps(h, 1, t3 / 3.0 + (double)m * t3 + 2.0 * t3 * ntile_wg + f_x);
            hipLaunchKernelGGL(potrf_step<false>, dim3(ntile_wg + nx_wg, 1), dim3(256), POTRF_STEP_LDS, h->stream, sa);
        }
        {
            sa.j = nt - 1; sa.lookahead = 0; sa.xrow = nt - 1; sa.xrow_first = 0;
            ProfScope ps(h, 1, 2.0 * t3 * (0.5 * (double)(nt - 1) * nt + 0.625 * (nt - 1)));
            hipLaunchKernelGGL(potrf_step<false>, dim3(4 * (nt - 1), 1), dim3(256), 64 * 18 * sizeof(double), h->stream, sa);
        }
        HIPCHK(hipGetLastError());
        return GMRF_OK;
    }
    // Batches (round 3): 256-column panels whose diagonal block is two potrf_diag128 launches (see potrf_step.hpp); the
    // rows below a panel meet the 256 x 256 inverse of its diagonal block in ONE product on the GEMM kernel (K = 256):
    //   potrf_diag128(A)                              A, B: the panel's two 128 x 128 diagonal blocks
    //   L_BA = S_BA X_A^T,  S_BB -= L_BA L_BA^T       (two 128^3 products)
    //   potrf_diag128(B)
    //   X_BA = -X_B (L_BA X_A)                        (the level-128 doubling step of this pair: X_P = [X_A 0; X_BA X_B])
    //   L[below, P] = S[below, P] X_P^T               (K = 256, X_P lower triangular)
    //   S[below, below] -= L[below, P] L[below, P]^T  (rank-256 update)
    if (fy && (route != ROUTE_PANELS256 || overlap)) return bad_shape("internal: forward solve planned off the 256-column panel route");
    if (route == ROUTE_PANELS256 && !overlap) {
        StepArgs sa;
        sa.S = S; sa.L = L; sa.X = X; sa.ld = ld; sa.nt = nt; sa.cend = nt;
        sa.info = h->d_info; sa.blk = blk_id; sa.dbg = nullptr;
        sa.pS = (int64_t)bsp * bsp; sa.pL = stride_pL(h); sa.pX = stride_pX(h); sa.blk_per_problem = (int)h->N;
        const int64_t pW = (int64_t)bsp * bsp;
        const double t3 = 64.0 * 64.0 * 64.0, nb = (double)h->B;
        auto diag128 = [&](int j) -> gmrf_status {
            sa.j = j;
            // two tile Choleskys + four triangular 64^3 products (L10, S11 update, L10 X00, X11 W)
            ProfScope ps(h, 16, (2.0 * t3 / 3.0 + 4.0 * 2.0 * t3 * 0.625) * nb);
            static const bool fat = env_int("GMRF_DIAG128_FAT", 0) != 0;      // the three-tile form (tests: bitwise the slim one)
            if (fat) hipLaunchKernelGGL(potrf_diag128, dim3(1, (unsigned)h->B), dim3(256), POTRF_DIAG128_LDS, h->stream, sa);
            else hipLaunchKernelGGL(potrf_diag128_slim, dim3(1, (unsigned)h->B), dim3(256), POTRF_DIAG128_SLIM_LDS, h->stream, sa);
            HIPCHK(hipGetLastError());
            return GMRF_OK;
        };
        // Small batches (round 4): 7 workgroups per problem fit the chip up to a batch of 36, and then the panel's whole
        // 256 x 256 diagonal block -- two potrf_diag128 launches and the four 128^3 products -- is ONE persistent launch
        // (potrf_persist on the 4 x 4 tiles of the block, inverse rows included): 62 us instead of ~100 us per panel, on
        // 7 B CUs instead of B (C4 elliptic512 at batch 8: 8 of 256 CUs were busy in the diagonal chain).  Larger batches keep
        // the one-workgroup kernels: their chain hides behind the other problems, and 7 B workgroups of 140 KB would not fit.
        const bool persist_panels = !h->sw(GMRF_SW_NO_PERSIST_PANELS) && persist_fits(h, 4, 0, 4, 2);
        for (int j = 0; j < nt; j += 4) {
            const int64_t oa = (int64_t)j * 64, ob = oa + 128;
            if (persist_panels) {
                const double fl = (4.0 * t3 / 3.0 + 2.0 * t3 * (6.0 * 0.625 + 10.0 + 10.0 + 6.0 * 0.625)) * nb;
                GCHK(launch_persist(h, S + oa * ld + oa, L + oa * ld + oa, X + oa * ld + oa, 4, 0, 4, 2, blk_id, fl));
            } else {
                GCHK(diag128(j));
                // The four 128^3 products of the panel are three GEMM launches: L_BA = S_BA X_A^T (256 workgroups at batch 64); then
                // S_BB -= L_BA L_BA^T and T = L_BA X_A together (192 + 256), both in front of the second diagonal block; and
                // X_BA = -X_B T (256) after it.  Until round 13 they were four launches, T behind the second diagonal block
                // (13 % of a step's GEMM time at 20.7 TF/s).
                // (Round 4 built and measured the alternative, ONE workgroup per problem in two launches, bitwise the same results:
                //  the time-weighted GEMM fraction rose to 0.66 and the job got SLOWER, 45.6 k against 48.1 k solves/s -- twelve
                //  dependent 64^3 products take one CU 57 us, the four launches of then 39 us.  Removed in round 5.)
                // L_BA = S_BA X_A^T (X_A lower triangular, stored [n][k])
                GCHK(gemm(h, GemmCall(false, false, 128, 128, 128, 1.0, 0.0).a(S + ob * ld + oa, ld, sa.pS).b(X + oa * ld + oa, ld, sa.pX)
                                 .c(L + ob * ld + oa, ld, sa.pL).triangular(TRI_B_UPPER).work(2.0 * t3 * 3.0 * 2.0 * nb)));
                // S_BB -= L_BA L_BA^T (lower tiles), and T = L_BA X_A -- the first half of X_BA = -X_B (L_BA X_A), the level-128 doubling step of this pair (T is the
                // work block doubling_levels uses) -- reads L_BA and X_A only, as the update of S_BB reads L_BA only: ONE launch of
                // 192 + 256 workgroups per 64 problems in front of the second diagonal block instead of a launch on either side of it
                GCHK(gemm_pair(h,
                               GemmCall(false, false, 128, 128, 128, -1.0, 1.0).a(L + ob * ld + oa, ld, sa.pL).b(L + ob * ld + oa, ld, sa.pL)
                                   .c(S + ob * ld + ob, ld, sa.pS).lower().strict_lower(strict_lower_route(h)).work(2.0 * t3 * 2.0 * 3.0 * nb),
                               GemmCall(false, true, 128, 128, 128, 1.0, 0.0).a(L + ob * ld + oa, ld, sa.pL).b(X + oa * ld + oa, ld, sa.pX)
                                   .c(T + ob * ld + oa, ld, pW).triangular(TRI_B_LOWER)));
                GCHK(diag128(j + 2));
                GCHK(gemm(h, GemmCall(false, true, 128, 128, 128, -1.0, 0.0).a(X + ob * ld + ob, ld, sa.pX).b(T + ob * ld + oa, ld, pW)
                                 .c(X + ob * ld + oa, ld, sa.pX).triangular(TRI_A_LOWER)));
            }
            const int m3 = nt - j - 4;                             // row tiles below the panel
            // forward solve (fy): y_P = X_P t_P is the tail row of the panel product, t[below] -= L[below, P] y_P the tail row of the
            // rank-256 update; the last panel has no rows below it and takes the 256^2 product on its own
            const int64_t pT = bsp, pY = h->n_pad;
            if (m3 <= 0) {
                if (fy) {
                    // y_P = X_P t_P on the forward sweep's k = 1 kernel (X_P lower triangular, 256 x 256)
                    SweepArgs sw;
                    sw.Mat = X + oa * ld + oa; sw.ld = ld; sw.Xin = h->d_ft + oa; sw.ldx = pT; sw.Bin = nullptr; sw.ldb = 0;
                    sw.Out = fy + oa; sw.ldo = pY; sw.rows = 256; sw.kdim = 256; sw.sub = 0;
                    sw.pMat = sa.pX; sw.pXin = pT; sw.pBin = 0; sw.pOut = pY;
                    ProfScope ps(h, 3, 4.0 * 256.0 * 257.0 * nb);
                    HIPCHK(launch_sweep(h->stream, false, true, 1, sw, (int)h->B));
                }
                continue;
            }
            // (round 19) Envelope bounds, relative to the panel (gmrf_handle::env_host): the rows below the panel that S = D_i - C C^T did
            // not write and no earlier panel has met are still D_i's -- row tile bm of S[below, P] is zero outside [kb, ke), of
            // L[below, P] left of kb.  The products skip those K ranges (sums of 0 x: the same bits); a panel product whose last row
            // tile carries the forward solve's tail row keeps that tile's full range (the tail's own).
            const EnvPanel ev = env_panel(h, blk_id - 1, j / 4, fy != nullptr);
            GCHK(gemm(h, panel_product(h, S, L, X, j, ev, fy)));
            GCHK(gemm(h, panel_update(h, S, L, X, j, ev, fy)));
        }
        // X = L^-1 by recursive doubling over the 256-wide diagonal inverses -- or, split representation, everything
        // but its first block column below row p, whose place L[p:, 0:p] takes (see gmrf_handle::xsplit)
        const int p = h->xsplit;
        GCHK(doubling_levels(h, L, X, T, 256, bsp / 2, -1, p));
        if (p > 0 && !(p == 256 && !h->keep_l)) {
            hipLaunchKernelGGL(copy_rect, dim3((unsigned)((bsp - p) / 4), (unsigned)h->B), dim3(256), 0, h->stream,
                               L + (int64_t)p * ld, ld, sa.pL, X + (int64_t)p * ld, ld, sa.pX, bsp - p, p);
            HIPCHK(hipGetLastError());
        }
        return GMRF_OK;
    }
    // (only the 256-column panel route above leaves the split form: planned_xsplit asks the same predicate)
    if (h->xsplit > 0) return bad_shape("internal: split inverse planned off the 256-column panel route");
    for (int j = 0; j < nt; ++j) {
        StepArgs sa;
        sa.S = S; sa.L = L; sa.X = X; sa.ld = ld; sa.j = j; sa.nt = nt;
        sa.info = h->d_info; sa.blk = blk_id; sa.dbg = h->dbg_stamps;
        sa.pS = (int64_t)bsp * bsp; sa.pL = stride_pL(h); sa.pX = stride_pX(h); sa.blk_per_problem = (int)h->N;
        const int m = nt - j - 1;
        const int cend = std::min(nt, (j / pw + 1) * pw);  // first column tile outside this panel
        sa.cend = cend;
        int utiles = 0;
        for (int c = j + 1; c < cend; ++c) utiles += nt - c;
        const double rem = 64.0 * m, nb = (double)h->B;
        const double f_tile = 64.0 * 64.0 * 64.0 / 3.0 * nb, f_panel = rem * 64.0 * 64.0 * nb;
        const double f_upd = 2.0 * 64.0 * 64.0 * 64.0 * utiles * nb;
        if (fused_in_panel && !h->sw(GMRF_SW_NO_LOOKAHEAD) && !overlap && j % pw == 0 && cend - j >= 2 && persist_fits(h, nt, j, cend, 0)) {
            // One problem, larger blocks: the panel's column tiles [j, cend) as ONE persistent launch (potrf_persist.hpp): the
            // look-ahead chain over the panel's own columns, the last column's rows below included (the launch's last-column
            // workgroups form them: `tail_panel`); the rank-256 update of the rest of the block (GEMM) follows as before
            const int npc = cend - j;
            double fl = 64.0 * 64.0 * 64.0 / 3.0 * npc;
            for (int jj = j; jj + 1 < cend; ++jj) {
                int ut = 0;
                for (int c = jj + 1; c < cend; ++c) ut += nt - c;
                fl += 64.0 * (nt - jj - 1) * 64.0 * 64.0 + 2.0 * 64.0 * 64.0 * 64.0 * ut;
            }
            fl += 64.0 * (nt - cend) * 64.0 * 64.0;          // (the last column's rows below the panel: formed inside the launch too)
            GCHK(launch_persist(h, S, L, X, nt, j, cend, 0, blk_id, fl));
            j = cend - 1;                                     // the loop continues behind the panel's last column
            sa.j = j;
        } else if (fused || m == 0) {
            // one problem, fused steps: the tiles of row j - 1 of the inverse ride in the launch of step j (4 workgroups
            // per tile on CUs the step leaves idle; see xrow_strip), the last row gets a launch of its own below
            const bool xrows = fused && !h->sw(GMRF_SW_DOUBLING_INVERSE) && !overlap && j >= 2;
            const int ntile_wg = 1 + m * (m + 1) / 2;
            sa.xrow = xrows ? j - 1 : -1; sa.xrow_first = ntile_wg;
            const int nx_wg = xrows ? 4 * (j - 1) : 0;
            const double f_x = xrows ? 2.0 * 64.0 * 64.0 * 64.0 * (0.5 * (double)(j - 1) * j + 0.625 * (j - 1)) : 0.0;
            ProfScope ps(h, 1, f_tile + f_panel + f_upd + f_x);
            hipLaunchKernelGGL(potrf_step<false>, dim3(ntile_wg + nx_wg, (unsigned)h->B), dim3(256),
                               m == 0 ? POTRF_TILE_LDS : POTRF_STEP_LDS, h->stream, sa);
            sa.xrow = -1;
        } else if (fused_in_panel && utiles > 0) {
            // the workgroups of column j+1 write the whole panel L[j+1.., j]
            ProfScope ps(h, 1, f_tile + f_panel + f_upd);
            hipLaunchKernelGGL(potrf_step<false>, dim3(1 + utiles, 1), dim3(256), POTRF_STEP_LDS, h->stream, sa);
        } else {
            // factor the B diagonal tiles once, then panel and update without the redundant tile work
            {
                ProfScope ps(h, 1, f_tile);
                hipLaunchKernelGGL(potrf_step<false>, dim3(1, (unsigned)h->B), dim3(256), POTRF_TILE_LDS, h->stream, sa);
            }
            {
                ProfScope ps(h, 8, f_panel);
                hipLaunchKernelGGL(potrf_panel, dim3(m, (unsigned)h->B), dim3(256), 0, h->stream, sa);
            }
            if (utiles > 0) {
                ProfScope ps(h, 9, f_upd);
                hipLaunchKernelGGL(potrf_update, dim3(utiles, (unsigned)h->B), dim3(256), 0, h->stream, sa);
            }
        }
        HIPCHK(hipGetLastError());
        if (j + 1 == cend && cend < nt) {
            // S[r,c] -= L[r,P] L[c,P]^T for the tiles right of / below the finished panel P
            const int j0 = cend - pw, mr = nt - cend;
            const double* Lp = L + (int64_t)cend * 64 * ld + (int64_t)j0 * 64;
            double* Sr = S + (int64_t)cend * 64 * ld + (int64_t)cend * 64;
            GCHK(gemm(h, GemmCall(false, false, mr * 64, mr * 64, pw * 64, -1.0, 1.0).a(Lp, ld, sa.pL).b(Lp, ld, sa.pL).c(Sr, ld, sa.pS).lower()
                             .work(2.0 * 64.0 * 64.0 * (pw * 64.0) * (mr * (mr + 1) / 2) * (double)h->B)));
        }
        if (overlap && j + 1 == nt / 2) {
            HIPCHK(hipEventRecord(ev_fork, h->stream));
            HIPCHK(hipStreamWaitEvent(h->aux, ev_fork, 0));
            h->gemm_stream = h->aux;
            gmrf_status st = doubling_levels(h, L, X, T, 64, bsp / 4, 0);
            if (st == GMRF_OK) st = doubling_top(h, L, X, T, true, false);
            h->gemm_stream = nullptr;
            GCHK(st);
        }
    }
    if (fused && !h->sw(GMRF_SW_DOUBLING_INVERSE) && !overlap) {
        // the inverse was assembled row by row inside the step launches; its last row is what is left
        if (nt >= 2) {
            StepArgs sa;
            sa.S = S; sa.L = L; sa.X = X; sa.ld = ld; sa.j = nt - 1; sa.nt = nt;
            sa.info = h->d_info; sa.blk = blk_id; sa.dbg = nullptr;
            sa.pS = (int64_t)bsp * bsp; sa.pL = stride_pL(h); sa.pX = stride_pX(h); sa.blk_per_problem = (int)h->N;
            sa.cend = nt; sa.xrow = nt - 1; sa.xrow_first = 0;
            ProfScope ps(h, 1, 2.0 * 64.0 * 64.0 * 64.0 * (0.5 * (double)(nt - 1) * nt + 0.625 * (nt - 1)));
            hipLaunchKernelGGL(potrf_step<false>, dim3(4 * (nt - 1), 1), dim3(256), 64 * 18 * sizeof(double), h->stream, sa);
            HIPCHK(hipGetLastError());
        }
        return GMRF_OK;
    }
    // X = L^-1 by recursive doubling over the 64-wide diagonal inverses (the part not done beside
    // the panel chain above)
    if (overlap) {
        GCHK(doubling_levels(h, L, X, T, 64, bsp / 4, 1));       // second half, levels below the top
        HIPCHK(hipEventRecord(ev_join, h->aux));
        HIPCHK(hipStreamWaitEvent(h->stream, ev_join, 0));       // T21 of the top level is ready
        GCHK(doubling_top(h, L, X, T, false, true));
    } else {
        GCHK(doubling_levels(h, L, X, T, 64, bsp / 2, -1));
    }
    return GMRF_OK;
}

// ---- The coupling step of block i > 0 as a value: C_i = B_i Linv_{i-1}^T and whoever clears the Schur block S before S = D_i - C C^T.
// coupling_route decides (host only: gmrf_test_coupling_plan asks it without a device), launch_coupling issues what it says and
// nothing else; factor_blocks_range calls the two, gmrf_test_coupling_product the second with a forced or overridden route.
enum CouplingKind { COUPLING_DENSE = 0, COUPLING_BXT = 1, COUPLING_TILES = 2 };
// who clears S: nobody (rm == bsp: the product writes every row), zero_rows (a launch of its own, rows >= rm), the zero role of
// spmm_bxt_tiles (rows >= rm), its scatter role (one problem: the whole block, then D_i's entries)
enum CouplingFill { FILL_NONE = 0, FILL_ZERO_ROWS = 1, FILL_ZERO_ROLE = 2, FILL_SCATTER_ROLE = 3 };
struct CouplingShape {
    int bsp = 0, bs = 0, cm = 0, rm = 0, nb = 1, cus = 0;
    bool sparse_b = false;      // rows of at most 32 entries (build_symbolic)
    bool plan_ok = false;       // a tile plan that covers the coupling rows
    bool has_drow = false;      // D_i's entries row by row are on the device (the scatter role reads them)
    int max_row = 0, ng = 0;    // longest row of a lower block; groups of row tiles of THIS block
    int32_t switches = 0;
};
struct CouplingRoute {
    int kind = COUPLING_DENSE;
    int km = 0, cw = 0;                     // spmm_bxt<km>, columns per workgroup
    int nch = 0, ncg = 0, ng = 0;           // spmm_bxt_tiles: 16-column chunks per workgroup, column groups, tile groups
    int grid = 0;                           // workgroups of the product's launch (0: the GEMM's own)
    int fill = FILL_NONE, zwgs = 0;
    int skip_dead = 0;
};
static const int kBxtNch[] = {1, 2, 3, 4, 6, 8, 12, 16, 24, 48};

// workgroups of the product's launch for the fields as they stand
static void coupling_grid(const CouplingShape& s, CouplingRoute& r) {
    const int W = s.bsp - s.cm, rch = (s.rm + 255) / 256;
    if (r.kind == COUPLING_BXT) r.grid = (W / r.cw) * rch * s.nb;
    else if (r.kind == COUPLING_TILES) { r.ncg = (W / 16 + r.nch - 1) / r.nch; r.grid = (r.ncg * r.ng + r.zwgs) * s.nb; }
    else r.grid = 0;
}
static int coupling_zero_wgs(const CouplingShape& s) {        // the zero role: >= 128 KB per workgroup
    const int64_t zcount = (int64_t)(s.bsp - s.rm) * s.bsp;
    return (int)std::min<int64_t>(32, std::max<int64_t>(1, zcount / 16384));
}
// every field of the route once the kernel family is chosen (its preconditions are the caller's to check)
static CouplingRoute coupling_route_of(const CouplingShape& s, int kind) {
    CouplingRoute r;
    r.kind = kind;
    const int W = s.bsp - s.cm, rch = (s.rm + 255) / 256, nb = s.nb;
    if (kind == COUPLING_TILES) {
        static const bool live_skip = env_int("GMRF_BXT_LIVE", 0) != 0;      // tuning aid (measured: 4.1 vs 3.9 ms per step, off)
        r.skip_dead = live_skip ? 1 : 0;
        const int chunks = W / 16;
        r.ng = s.ng;
        // 16-column chunks per workgroup: the launch should be a whole number of rounds over the 3 workgroups a CU
        // holds (measured, darcy256 x 64, 4 groups x 48 chunks: 16 chunks = 768 workgroups = one round 85 us; 8 =
        // two rounds 96 us; 12 = 1.33 rounds 108 us; 24 = 2/3 round 99 us): rounds x (chunks + ~2 for the prologue)
        const int64_t slots = 3 * (int64_t)std::max(s.cus, 1);
        int best = 1; int64_t best_cost = INT64_MAX;
        for (int c : kBxtNch) {
            if (c > chunks) break;
            const int64_t wgs = (int64_t)((chunks + c - 1) / c) * r.ng * nb;
            const int64_t cost = ((wgs + slots - 1) / slots) * (c + 2);
            if (cost < best_cost || (cost == best_cost && c < best)) { best = c; best_cost = cost; }
        }
        r.nch = best;
        // (round 5: the launch clears the Schur block as well) one problem: the WHOLE block, and D_i scattered into it
        if (nb == 1 && s.has_drow && s.bsp == s.bs && !(s.switches & GMRF_SW_NO_SCATTER_FOLD)) { r.fill = FILL_SCATTER_ROLE; r.zwgs = 64; }
        else if (s.rm < s.bsp && ((int64_t)(s.bsp - s.rm) * s.bsp) % 2 == 0) { r.fill = FILL_ZERO_ROLE; r.zwgs = coupling_zero_wgs(s); }
        else if (s.rm < s.bsp) r.fill = FILL_ZERO_ROWS;
    } else {
        if (kind == COUPLING_BXT) {
            r.km = s.max_row <= 8 ? 8 : (s.max_row <= 16 ? 16 : 32);
            r.cw = ((int64_t)(W / 64) * rch * nb >= 512) ? 64 : (((int64_t)(W / 32) * rch * nb >= 512) ? 32 : 16);
        }
        if (s.rm < s.bsp) r.fill = FILL_ZERO_ROWS;
    }
    coupling_grid(s, r);
    return r;
}
// The route rule: sparse lower blocks, not forced onto the dense GEMM, go to spmm_bxt_tiles where a tile plan covers the coupling
// rows, else to spmm_bxt.  (GMRF_BXT_TILES=0 keeps spmm_bxt: the tests' bitwise reference.)
static CouplingRoute coupling_route(const CouplingShape& s) {
    static const bool no_tiles = env_int("GMRF_BXT_TILES", 1) == 0;
    const bool sparse_g1 = s.sparse_b && !(s.switches & GMRF_SW_DENSE_COUPLING);
    return coupling_route_of(s, !sparse_g1 ? COUPLING_DENSE : (s.plan_ok && !no_tiles ? COUPLING_TILES : COUPLING_BXT));
}
static CouplingShape coupling_shape(const gmrf_handle* h, int64_t i) {
    CouplingShape s;
    s.bsp = (int)h->bsp; s.bs = (int)h->bs; s.cm = (int)h->cmin; s.rm = (int)h->rmax; s.nb = (int)h->B; s.cus = h->cu_count;
    s.sparse_b = h->sparse_b;
    s.plan_ok = h->bxt_plan_ok && h->bxt_nrt == (int)h->rmax / 64;
    s.has_drow = (bool)h->d_dg_rowptr;
    s.max_row = (int)h->lo_row_max;
    s.ng = (s.plan_ok && i >= 0 && (size_t)i < h->bxt_ng.size()) ? h->bxt_ng[(size_t)i] : 0;
    s.switches = h->switches;
    return s;
}
static CouplingRoute coupling_route(const gmrf_handle* h, int64_t i) { return coupling_route(coupling_shape(h, i)); }

// Block i > 0, everything up to (not including) S = -C C^T: the Schur block's zero fill, whoever does it; the dense image of B_i
// for the GEMM route; the product C_i = B_i Linv_{i-1}^T into the stored window of d_C.
static gmrf_status launch_coupling(gmrf_handle* h, int64_t i, const CouplingRoute& r) {
    const int bsp = (int)h->bsp;
    const int64_t ld = bsp;
    const size_t blk_bytes = (size_t)bsp * bsp * sizeof(double) * (size_t)h->B;
    const int64_t bstride = (int64_t)bsp * bsp;
    const int64_t pX = stride_pX(h), pC = stride_pC(h);
    const int64_t ldc = c_ld(h), cstride = c_blk(h);
    const unsigned nb = (unsigned)h->B;
    const int cm = (int)h->cmin, rm = (int)h->rmax;
    const int W = bsp - cm;
    if (r.fill == FILL_ZERO_ROWS) {
        const int64_t cnt = (int64_t)(bsp - rm) * bsp;
        hipLaunchKernelGGL(zero_rows, dim3((unsigned)((cnt / 2 + 255) / 256), nb), dim3(256), 0, h->stream,
                           h->d_S + (int64_t)rm * ld, cnt, bstride);
        HIPCHK(hipGetLastError());
    }
    double* C = h->d_C + (i - 1) * cstride;              // stored window: rows 0 .. rm, columns cm ..
    const double* Xp = h->d_Linv + (i - 1) * bstride;
    if (r.kind == COUPLING_DENSE) {          // dense image of B for the GEMM route
        HIPCHK(hipMemsetAsync(h->d_B, 0, blk_bytes, h->stream));
        if (h->low_count[i] > 0) {
            hipLaunchKernelGGL(scatter_block, dim3((unsigned)((h->low_count[i] + 255) / 256), nb), dim3(256), 0,
                               h->stream, h->d_keys, h->d_vals, h->low_first[i], h->low_count[i], h->d_B, ld,
                               h->n_entries, bstride, 0);
            HIPCHK(hipGetLastError());
        }
        // C = B * Linv_{i-1}^T      (src/tridiagonal_cholesky.jl:74).  B is zero left of column
        // cmin and below row rmax, hence C is zero there too and only the rest is computed; inside that
        // window row tile t of B -- and of C, Linv being lower triangular -- is zero left of kst[t].
        return gemm(h, GemmCall(false, false, rm, W, W, 1.0, 0.0).a(h->d_B + cm, ld, bstride).b(Xp + (int64_t)cm * ld + cm, ld, pX)
                           .c(C, ldc, pC).triangular(TRI_B_UPPER).k_begin(h->d_kst, nullptr));
    }
    // streamed bytes: C inside the staircase (written) + the rows of Linv from the first gathered column on (read)
    ProfScope ps(h, 10, 8.0 * (h->c_streamed + 0.5 * (double)W * W) * (double)h->B);
    if (r.kind == COUPLING_TILES) {
        BxtTileArgs ta;
        ta.rowptr = h->d_lo_rowptr + i * (h->bsp + 1); ta.lidx = h->d_bxt_lidx; ta.vals = h->d_vals; ta.n_entries = h->n_entries;
        ta.uptr = h->d_bxt_uptr + i * (h->bxt_nrt + 1); ta.ucols = h->d_bxt_ucols;
        ta.gtiles = h->d_bxt_gtiles + i * h->bxt_nrt * 3; ta.ng = r.ng;
        ta.X = Xp; ta.C = C; ta.ld = ld; ta.ldc = ldc; ta.pX = pX; ta.pC = pC; ta.kst = h->d_kst;
        ta.cm = cm; ta.rm = rm; ta.bsp = bsp; ta.ecap = h->bxt_ecap;
        ta.skip_dead = r.skip_dead;
        ta.nch = r.nch;
        ta.nprob = (int)nb;
        ta.zdst = nullptr; ta.zcount = 0; ta.zpdst = 0; ta.zwgs = 0;
        ta.srowptr = nullptr; ta.skeys = nullptr; ta.svals = nullptr;
        if (r.fill == FILL_SCATTER_ROLE) {
            // one problem: the launch zeroes the WHOLE Schur block and scatters D_i into it row range by row range; the
            // product then accumulates, S = 1.0 * S - C C^T -- the same single rounding fl(D - acc) as "S := -C C^T, then
            // S += D_i", without the scatter launch (4.9 us + a boundary) between the product and the block's Cholesky
            ta.zdst = h->d_S; ta.zcount = (int64_t)bsp * bsp; ta.zpdst = bstride; ta.zwgs = r.zwgs;
            ta.srowptr = h->d_dg_rowptr + i * (h->bsp + 1); ta.skeys = h->d_keys; ta.svals = h->d_vals;
        } else if (r.fill == FILL_ZERO_ROLE) {
            ta.zdst = h->d_S + (int64_t)rm * ld; ta.zcount = (int64_t)(bsp - rm) * bsp; ta.zpdst = bstride; ta.zwgs = r.zwgs;
        }
        hipLaunchKernelGGL(spmm_bxt_tiles, dim3((unsigned)r.grid), dim3(256), bxt_tile_lds_bytes(h->bxt_ecap), h->stream, ta);
    } else {
        BxtArgs ba;
        ba.rowptr = h->d_lo_rowptr + i * (h->bsp + 1); ba.keys = h->d_keys;
        ba.vals = h->d_vals; ba.n_entries = h->n_entries;
        ba.X = Xp; ba.C = C; ba.ld = ld; ba.ldc = ldc; ba.pX = pX; ba.pC = pC; ba.cm = cm; ba.rm = rm;
        ba.kst = h->d_kst;
        ba.cw = r.cw;
        ba.bsp = bsp;
        const dim3 grid((unsigned)r.grid);
        if (r.km == 8) hipLaunchKernelGGL(spmm_bxt<8>, grid, dim3(256), 0, h->stream, ba);
        else if (r.km == 16) hipLaunchKernelGGL(spmm_bxt<16>, grid, dim3(256), 0, h->stream, ba);
        else hipLaunchKernelGGL(spmm_bxt<32>, grid, dim3(256), 0, h->stream, ba);
    }
    HIPCHK(hipGetLastError());
    return GMRF_OK;
}

static gmrf_status factor_blocks_range(gmrf_handle* h, int64_t i0, int64_t i1) {
    const int bsp = (int)h->bsp;
    h->xsplit = planned_xsplit(h);                     // representation of the inverses this factorisation leaves
    const int64_t ld = bsp;
    const int64_t bstride = (int64_t)bsp * bsp;
    const unsigned nb = (unsigned)h->B;
    for (int64_t i = i0; i < i1; ++i) {
        double* L = l_block(h, i);
        double* X = h->d_Linv + i * bstride;
        // S = D_i - C C^T is built as  S := -C C^T (GEMM, beta = 0)  then  S += D_i (scatter): same
        // single rounding as D - acc, and only the rows the product does not write (>= rmax) need
        // zeroing -- a quarter of the block on darcy instead of all of it.  The first block has no product.
        if (h->fwd_run) {
            // t = b_i (the rows G2's tail does not write stay so)
            hipLaunchKernelGGL(factor_rhs_block, dim3((unsigned)((bsp + 255) / 256), nb), dim3(256), 0, h->stream, h->frhs, h->n, (int)h->bs,
                               bsp, i, h->d_ft);
            HIPCHK(hipGetLastError());
        }
        // (round 5: where the coupling product of this block runs on spmm_bxt_tiles, that launch zeroes the rows as well)
        const CouplingRoute route = i > 0 ? coupling_route(h, i) : CouplingRoute();
        const bool scatter_in_bxt = i > 0 && route.fill == FILL_SCATTER_ROLE;
        if (i == 0) {
            const int64_t cnt = (int64_t)bsp * bsp;
            hipLaunchKernelGGL(zero_rows, dim3((unsigned)((cnt / 2 + 255) / 256), nb), dim3(256), 0, h->stream, h->d_S, cnt, bstride);
            HIPCHK(hipGetLastError());
        } else {
            GCHK(launch_coupling(h, i, route));
            // S = D - C C^T: the product part (with the forward solve's tail row)
            GCHK(gemm(h, g2_product(h, i, scatter_in_bxt, h->fwd_run)));
        }
        if (h->diag_count[i] > 0 && !scatter_in_bxt) {
            hipLaunchKernelGGL(scatter_block, dim3((unsigned)((h->diag_count[i] + 255) / 256), nb), dim3(256), 0,
                               h->stream, h->d_keys, h->d_vals, h->diag_first[i], h->diag_count[i], h->d_S, ld,
                               h->n_entries, bstride, 1);
            HIPCHK(hipGetLastError());
        }
        if (i == h->tw_blk && h->tw_hj)      // twisted order, meeting block: S -= H_m H_m^T = HJ HJ^T (J is an orthogonal flip)
            GCHK(gemm(h, GemmCall(false, false, bsp, bsp, bsp, -1.0, 1.0).a(h->tw_hj, ld, 0).b(h->tw_hj, ld, 0).c(h->d_S, ld, 0).lower()));
        if (h->bsp > h->bs) {
            hipLaunchKernelGGL(pad_identity, dim3((unsigned)((h->bsp - h->bs + 255) / 256), nb), dim3(256), 0,
                               h->stream, h->d_S, ld, (int)h->bs, bsp, bstride);
            HIPCHK(hipGetLastError());
        }
        GCHK(potrf_block(h, h->d_S, L, X, h->d_T, (int)(i + 1), h->fwd_run ? h->d_fy + i * bsp : nullptr));
        if (i == h->tw_blk && h->tw_w)       // W = L_m^-1 HJ: the coupling of the twisted sweeps' meeting corrections
            GCHK(gemm(h, GemmCall(false, true, bsp, bsp, bsp, 1.0, 0.0).a(X, ld, 0).b(h->tw_hj, ld, 0).c(h->tw_w, ld, 0)));
        if (!h->keep_l) {
            // L_i lives in a work buffer that the next block overwrites: its log-determinant part is taken now
            hipLaunchKernelGGL(logdet_blocks, dim3(1, nb), dim3(256), 0, h->stream, L, bstride, ld, (int)h->bs,
                               h->d_logdet + i, stride_pL(h), h->N);
            HIPCHK(hipGetLastError());
        }
    }
    return GMRF_OK;
}

// Split representation -> full inverse, in place, every block and problem: X_ba = -X_bb (L_ba X_aa) takes L_ba's place.
// Needed by whoever reads Linv_i as a matrix (selected inversion, gmrf_bt_get_block / export); the sweeps and the
// coupling products never are.  The factor stays full until the next factorisation.
static gmrf_status ensure_full_inverse(gmrf_handle* h) {
    if (h->xsplit <= 0) return GMRF_OK;
    const int bsp = (int)h->bsp, p = h->xsplit;
    for (int64_t i = 0; i < h->N; ++i) {
        double* X = h->d_Linv + i * blk_elems(h);
        GCHK(doubling_pair(h, X, stride_pX(h), X, h->d_T, p, 0, bsp - p, p, 1, 0));
    }
    h->xsplit = 0;
    return GMRF_OK;
}

// Stream captures of different handles (host threads) are taken one at a time: capture + instantiate is a
// once-per-shape set-up step, and concurrent captures are the one place where handles would meet inside the runtime.
// A PRECAUTION, not a diagnosed fix: no fault of the runtime under concurrent thread-local captures was ever reproduced or
// traced to a cause here (round 2 saw one unexplained profiler-side crash and kept no log of it); the mutex costs nothing
// in steady state (graphs are replayed, not re-captured) and can go once concurrent captures have been shown to be safe.
static std::mutex g_capture_mu;

// Decided once per factorisation, before anything is enqueued: may this one carry the forward solve of the registered right-hand
// side?  Batches on the 256-column panel route, not twisted, and EVERY product that would carry a tail row -- G2, the panel
// products, the rank-256 updates -- on the 64 x 64 LDS-DMA tile that takes it (a dry run of gemm() with the tails asks).  Else the
// handle leaves no y, and gmrf_bt_posterior runs its forward sweep.  Allocates d_ft / d_fy.
static gmrf_status factor_fwd_ok(gmrf_handle* h, bool* ok) {
    *ok = false;
    if (!h->frhs || h->sw(GMRF_SW_NO_FACTOR_FWD) || h->B <= 1 || tw_on(h) || h->tw_blk >= 0 || h->sw(GMRF_SW_FORK_GRAPH) || h->rmax <= 0) return GMRF_OK;
    const int bsp = (int)h->bsp, nt = bsp / 64;
    if (potrf_route(h) != ROUTE_PANELS256 || bsp % 256 != 0) return GMRF_OK;
    const size_t ye = (size_t)(h->B * h->n_pad), te = (size_t)(h->B * h->bsp);
    if (!h->d_fy.fits(ye) || !h->d_ft.fits(te)) {
        h->fy_for = nullptr;
        GCHK(reserve_group(h->stream, {h->d_fy.want(ye), h->d_ft.want(te)}));
    }
    h->tail_probe = true; h->tail_refused = false;
    gmrf_status st = GMRF_OK;
    if (h->N > 1) st = gemm(h, g2_product(h, 1, false, true));
    for (int j = 0; j + 4 < nt && st == GMRF_OK; j += 4) {         // (the panels with rows below them)
        // (the envelope bounds potrf_block passes -- those of a block behind the first, as good as any: what qualifies does not
        // depend on their values, nor on where L[below, P] lies)
        const EnvPanel ev = env_panel(h, std::min<int64_t>(1, h->N - 1), j / 4, true);
        st = gemm(h, panel_product(h, h->d_S, h->d_L, h->d_Linv, j, ev, h->d_fy));
        if (st == GMRF_OK) st = gemm(h, panel_update(h, h->d_S, h->d_L, h->d_Linv, j, ev, h->d_fy));
    }
    h->tail_probe = false;
    *ok = st == GMRF_OK && !h->tail_refused;
    return GMRF_OK;
}

static gmrf_status run_factor(gmrf_handle* h, int64_t i0, int64_t i1) {
    if (h->sw(GMRF_SW_EAGER) || h->profiling) { h->stats.persist_route = 0; return factor_blocks_range(h, i0, i1); }
    const double* grhs = h->fwd_run ? h->frhs : nullptr;          // (the graph reads b, and the choice of launches depends on it)
    if (!h->factor_graph || h->factor_graph_i0 != i0 || h->factor_graph_i1 != i1 || h->factor_graph_rhs != grhs) {
        std::lock_guard<std::mutex> capture_lock(g_capture_mu);
        if (h->factor_graph) { (void)hipGraphExecDestroy(h->factor_graph); h->factor_graph = nullptr; }
        hipGraph_t graph = nullptr;
        HIPCHK(hipStreamBeginCapture(h->stream, hipStreamCaptureModeThreadLocal));
        h->capturing = true; h->fork_next = 0;
        h->stats.persist_route = 0;
        gmrf_status s = factor_blocks_range(h, i0, i1);
        h->capturing = false;
        h->factor_graph_route = h->stats.persist_route;
        hipError_t e = hipStreamEndCapture(h->stream, &graph);
        if (s != GMRF_OK) { if (graph) (void)hipGraphDestroy(graph); return s; }
        HIPCHK(e);
        HIPCHK(hipGraphInstantiate(&h->factor_graph, graph, nullptr, nullptr, 0));
        (void)hipGraphDestroy(graph);
        h->factor_graph_i0 = i0; h->factor_graph_i1 = i1; h->factor_graph_rhs = grhs;
    }
    h->xsplit = planned_xsplit(h);                     // (what the captured launches produce)
    h->stats.persist_route = h->factor_graph_route;
    if (h->factor_graph_route) h->persist_launched = true;
    HIPCHK(hipGraphLaunch(h->factor_graph, h->stream));
    return GMRF_OK;
}

// The blocks [i0, i1) have been enqueued; if a persistent launch was among them, wait for the range and look at the abort word:
// a bounded wait inside such a launch gave up (its workgroups were not all resident, or starved) -- every such launch has drained
// and left garbage.  The range is then repeated at once with the launch-per-step forms (its inputs, the value lists and the
// previous block's inverse, are untouched), which the handle keeps for good; the event is counted in stats.persist_aborts.
// Called per range by gmrf_bt_factor_step_async, BEFORE the caller packs / shares the range (a range shared before
// gmrf_bt_factor_end looked at the word carried garbage to the other ranks), and for the whole chain by factor_finish.
static gmrf_status persist_check_range(gmrf_handle* h, int64_t i0, int64_t i1, int* hinfo_out) {
    int hinfo2[2] = {0, 0};
    HIPCHK(hipMemcpyAsync(hinfo2, h->d_info, 2 * sizeof(int), hipMemcpyDeviceToHost, h->stream));
    HIPCHK(hipStreamSynchronize(h->stream));
    h->persist_launched = false;
    if (hinfo2[1] != 0) {
        persist_give_up(h);
        const int restore[4] = {h->info_checked, 0, 0, 0};     // (what the aborted range wrote into the info word means nothing)
        HIPCHK(hipMemcpyAsync(h->d_info, restore, 4 * sizeof(int), hipMemcpyHostToDevice, h->stream));
        if (h->d_pflags) HIPCHK(hipMemsetAsync(h->d_pflags, 0, sizeof(unsigned) * h->d_pflags.size(), h->stream));   // (belt and braces: the drained launches cleaned up themselves)
        h->stats.persist_route = 0;
        GCHK(factor_blocks_range(h, i0, i1));
        HIPCHK(hipMemcpyAsync(hinfo2, h->d_info, 2 * sizeof(int), hipMemcpyDeviceToHost, h->stream));
        HIPCHK(hipStreamSynchronize(h->stream));
        h->persist_launched = false;
    }
    h->info_checked = hinfo2[0];
    if (hinfo_out) *hinfo_out = hinfo2[0];
    return GMRF_OK;
}

static gmrf_status factor_finish(gmrf_handle* h, int32_t* info) {
    // (stepwise factorisations have looked at every range that held a persistent launch already; the monolithic one is one range)
    int hinfo = 0;
    GCHK(persist_check_range(h, 0, h->N, &hinfo));
    if (info) *info = hinfo;
    if (hinfo != 0) {
        h->factored = false;
        g_last_error = "matrix is not positive definite; failed block " + std::to_string((hinfo - 1) % h->N + 1) +
                       " of problem " + std::to_string((hinfo - 1) / h->N);
        if (info) *info = (hinfo - 1) % (int)h->N + 1;
        return GMRF_ERR_NOT_SPD;
    }
    h->factored = true;
    h->l_valid = h->keep_l;
    h->logdet_valid = !h->keep_l;      // without the L blocks the factorisation left every block's part in d_logdet
    return GMRF_OK;
}

static gmrf_status numeric_factor(gmrf_handle* h, const double* nzval, int32_t* info) {
    if (!h->analyzed) { g_last_error = "no sparsity pattern analysed"; return GMRF_ERR_NO_FACTOR; }
    GCHK(alloc_factor(h));
    if (h->c_dirty) {
        HIPCHK(hipMemsetAsync(h->d_C, 0, sizeof(double) * stride_pC(h) * h->B, h->stream));
        h->c_dirty = false;
    }
    persist_plan(h);
    HIPCHK(hipEventRecord(h->ev0, h->stream));
    GCHK(load_values(h, nzval));
    HIPCHK(hipMemsetAsync(h->d_info, 0, 4 * sizeof(int), h->stream));
    h->info_checked = 0; h->persist_launched = false;
    h->fy_for = nullptr;
    bool fwd = false;
    GCHK(factor_fwd_ok(h, &fwd));
    // (an abort-and-repeat inside factor_finish re-runs the blocks' launches, the forward solve's included: t is set per block)
    h->fwd_run = fwd;
    gmrf_status s = run_factor(h, 0, h->N);
    if (s == GMRF_OK) {
        (void)hipEventRecord(h->ev1, h->stream);
        s = factor_finish(h, info);
    }
    h->fwd_run = false;
    if (s == GMRF_OK && fwd) h->fy_for = h->frhs;
    float ms = 0.f;
    (void)hipEventElapsedTime(&ms, h->ev0, h->ev1);
    h->stats.factor_ms = ms;
    if (h->profiling) prof_collect(h);
    return s;
}

// ------------------------------------------------------------------------------------ streams on distinct hardware queues
// spins for `ticks` of the constant 100 MHz clock (always terminates: the clock advances)
__global__ void gmrf_spin_kernel(unsigned long long ticks) {
    const unsigned long long t0 = __builtin_amdgcn_s_memrealtime();
    while (__builtin_amdgcn_s_memrealtime() - t0 < ticks) {}
}

static double spin_pair_ms(hipStream_t a, hipStream_t b, unsigned long long ticks) {
    (void)hipDeviceSynchronize();
    const auto t0 = std::chrono::steady_clock::now();
    hipLaunchKernelGGL(gmrf_spin_kernel, dim3(1), dim3(64), 0, a, ticks);
    if (b) hipLaunchKernelGGL(gmrf_spin_kernel, dim3(1), dim3(64), 0, b, ticks);
    (void)hipStreamSynchronize(a);
    if (b) (void)hipStreamSynchronize(b);
    return std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
}

gmrf_status gmrf_streams_create(int32_t device, int32_t n, void** streams, int32_t* n_distinct) {
    if (n <= 0 || n > 32 || !streams) return bad_shape("gmrf_streams_create: 1 <= n <= 32 streams");
    HIPCHK(hipSetDevice(device));
    const int ncand = std::min(3 * n + 4, 48);
    std::vector<hipStream_t> cand((size_t)ncand, nullptr);
    for (int i = 0; i < ncand; ++i) {
        if (hipStreamCreateWithFlags(&cand[(size_t)i], hipStreamNonBlocking) != hipSuccess) {
            for (int j = 0; j < i; ++j) (void)hipStreamDestroy(cand[(size_t)j]);
            g_last_error = "hipStreamCreateWithFlags failed"; return GMRF_ERR_HIP;
        }
        // first use binds the stream to its hardware queue
        hipLaunchKernelGGL(gmrf_spin_kernel, dim3(1), dim3(64), 0, cand[(size_t)i], 1ull);
    }
    HIPCHK(hipDeviceSynchronize());
    const unsigned long long ticks = 100000ull;                       // 1 ms at 100 MHz
    double one = 1e30;
    for (int r = 0; r < 3; ++r) one = std::min(one, spin_pair_ms(cand[0], nullptr, ticks));
    std::vector<int> chosen;
    for (int i = 0; i < ncand && (int)chosen.size() < n; ++i) {
        bool ok = true;
        for (int c : chosen) {
            // serialised pairs take 2 x one, overlapped ones ~1 x one (best of two tries against host jitter)
            const double t = std::min(spin_pair_ms(cand[(size_t)c], cand[(size_t)i], ticks), spin_pair_ms(cand[(size_t)c], cand[(size_t)i], ticks));
            if (t > 1.5 * one) { ok = false; break; }
        }
        if (ok) chosen.push_back(i);
    }
    const int nd = (int)chosen.size();
    std::vector<char> used((size_t)ncand, 0);
    for (int c : chosen) used[(size_t)c] = 1;
    for (int i = 0; i < ncand && (int)chosen.size() < n; ++i)         // not enough distinct queues: fill up with the others
        if (!used[(size_t)i]) { chosen.push_back(i); used[(size_t)i] = 1; }
    for (int k = 0; k < n; ++k) streams[k] = (void*)cand[(size_t)chosen[(size_t)k]];
    for (int i = 0; i < ncand; ++i)
        if (!used[(size_t)i]) (void)hipStreamDestroy(cand[(size_t)i]);
    if (n_distinct) *n_distinct = nd;
    return GMRF_OK;
}

gmrf_status gmrf_streams_destroy(int32_t device, int32_t n, void** streams) {
    if (n < 0 || (n > 0 && !streams)) return bad_shape("gmrf_streams_destroy");
    HIPCHK(hipSetDevice(device));
    for (int k = 0; k < n; ++k)
        if (streams[k]) { (void)hipStreamSynchronize((hipStream_t)streams[k]); (void)hipStreamDestroy((hipStream_t)streams[k]); streams[k] = nullptr; }
    return GMRF_OK;
}

// ------------------------------------------------------------------------------------ sweeps
static double sweep_bytes(const gmrf_handle* h, int64_t k) {
    const double bs = (double)h->bs, N = (double)h->N;
    return 8.0 * (N * bs * (bs + 1) / 2.0 + (N - 1) * bs * bs) + 16.0 * (double)h->n * (double)k;
}

// One problem: may this sweep run as one persistent launch?  (the claim is planned with the factorisation: persist_plan)
static bool sweep_persist_ok(const gmrf_handle* h, int kp) {
    if (!h->sweep_persist_planned || h->sweep_persist_hold || h->sw(GMRF_SW_NO_SWEEP_PERSIST) || !persist_allowed(h) || h->B != 1 || h->xsplit != 0) return false;
    if (h->persist_cus < h->cu_count || sweep_persist_demand(h) <= 0) return false;
    if (kp != 1 && (kp % 16 != 0 || (int64_t)kp * h->n_pad * 8 >= ((int64_t)1 << 31))) return false;
    if (h->n_pad * 8 >= ((int64_t)1 << 31)) return false;
    const bool via_gemm = (kp % 64 == 0) && !h->sw(GMRF_SW_SWEEP_NO_GEMM) && (int64_t)(h->bsp / 64) * (kp / 64) >= 128;
    return !via_gemm;
}

// the words and the intermediate panel of the persistent sweeps (before any capture: allocations are not allowed inside one)
static gmrf_status sweep_persist_prepare(gmrf_handle* h, int kp) {
    if (!h->d_sweep_flags) {
        GCHK(h->d_sweep_flags.reserve(h->stream, 16));
        HIPCHK(hipMemsetAsync(h->d_sweep_flags, 0, sizeof(unsigned) * 16, h->stream));
    }
    h->sweep_nw = std::min(256, h->cu_count);
    HIPCHK(h->h_sweep_abort.open());
    const size_t need = (size_t)((int64_t)kp * h->n_pad);
    if (!h->d_Tsw.fits(need)) {
        HIPCHK(hipStreamSynchronize(h->stream));
        destroy_graphs(h);                                  // (captured sweeps hold the old pointer)
        GCHK(h->d_Tsw.reserve(h->stream, need));
    }
    return GMRF_OK;
}

static gmrf_status launch_sweep_persist(gmrf_handle* h, bool backward, int kp, double* Pin, double* Yout, hipStream_t st_over = nullptr,
                                        double* T_over = nullptr) {
    const int nw = h->sweep_nw;
    const int64_t elems = (int64_t)kp * h->n_pad;
    hipStream_t st = st_over ? st_over : h->stream;
    double* Tp = T_over ? T_over : h->d_Tsw;
    if (!h->d_sweep_flags || !h->h_sweep_abort || nw <= 0 || !Tp || (!T_over && !h->d_Tsw.fits((size_t)elems)))
        return bad_shape("internal: words / panel of the persistent sweeps not allocated");
    if (elems % 2 != 0) return bad_shape("internal: the persistent sweeps' panels need an even element count (sweep_fill_sentinel)");
    SweepPersistArgs a;
    a.C = h->d_C; a.Linv = h->d_Linv; a.Pin = Pin; a.T = Tp; a.Yout = Yout;
    a.N = (int)h->N; a.bsp = (int)h->bsp; a.cm = (int)h->cmin; a.rm = (int)h->rmax; a.kp = kp; a.backward = backward ? 1 : 0; a.nw = nw;
    a.npad = h->n_pad; a.ldc = c_ld(h); a.cstride = c_blk(h); a.bstride = (int64_t)h->bsp * h->bsp;
    a.kst = h->d_kst; a.mend = h->d_mend;
    a.abort_w = h->d_sweep_flags;
    void* dev_abort = nullptr;
    HIPCHK(hipHostGetDevicePointer(&dev_abort, h->h_sweep_abort, 0));
    a.host_abort = reinterpret_cast<unsigned*>(dev_abort);
    // (tests: the sweeps' own bound, so that the factorisation's launches pass)
    static const int limit_ms = env_int("GMRF_SWEEP_SPIN_MS", env_int("GMRF_PERSIST_SPIN_MS", -1));
    a.spin_limit = (unsigned)(limit_ms >= 0 ? limit_ms : 2000) * 100000u;
    static const int dbg = env_int("GMRF_SWEEP_DBG", 0);      // tuning aid
    a.dbg = dbg;
    // Pause between two looks at an input that has not arrived: k = 1 looks again at once (8 units = 0.2 us; a longer pause only
    // adds to every product: +0.28 us per 0.43 us measured).  The k >= 16 bodies look with 4 waves x 16 KB per workgroup, and
    // their looks load the fabric the OTHER workgroups' stores and looks travel on: 64 units (1.7 us) -- darcy256's 64-sample
    // sweep 0.96 -> 0.91 ms, and beside the mean's two sweeps (gmrf_bt_posterior) 1.52 -> 1.39 ms for the three; 128 units: 1.05 / 1.35.
    a.pause = (kp == 1) ? 8 : 64;
    const double N = (double)h->N, bsp = (double)h->bsp;
    const double work = (kp == 1) ? 8.0 * ((N - 1) * h->c_streamed + N * 0.5 * bsp * (bsp + 1))
                                  : kp * (2.0 * (N - 1) * h->c_streamed + N * bsp * (bsp + 1));
    {
        // the panels the products read from each other: sentinel everywhere (two elements per thread: elems is even, checked above)
        ProfScope ps(h, 5, 16.0 * (double)elems);
        hipLaunchKernelGGL(sweep_fill_sentinel, dim3((unsigned)((elems / 2 + 255) / 256)), dim3(256), 0, st, Tp, Yout, elems);
        HIPCHK(hipGetLastError());
    }
    ProfScope ps(h, kp == 1 ? 19 : 20, work);
    if (kp == 1) hipLaunchKernelGGL(sweep_persist<true>, dim3((unsigned)nw), dim3(256), 0, st, a);
    else hipLaunchKernelGGL(sweep_persist<false>, dim3((unsigned)nw), dim3(256), 0, st, a);
    HIPCHK(hipGetLastError());
    return GMRF_OK;
}

// behind a synchronisation of the stream: did a persistent sweep give up?  Then its panels hold garbage: the words are zeroed,
// the handle keeps the launch-per-product form for good (stats.persist_aborts), and the caller repeats its call.
static gmrf_status sweep_persist_check(gmrf_handle* h, bool* repeat) {
    *repeat = false;
    if (!h->sweep_persist_launched) return GMRF_OK;
    h->sweep_persist_launched = false;
    if (!h->h_sweep_abort || *static_cast<volatile unsigned*>(h->h_sweep_abort.p) == 0u) return GMRF_OK;
    *h->h_sweep_abort = 0u;
    persist_give_up(h);
    HIPCHK(hipMemsetAsync(h->d_sweep_flags, 0, sizeof(unsigned) * 16, h->stream));
    h->stats.sweep_persist = 0;
    *repeat = true;
    return GMRF_OK;
}

// (input, output) byte ranges of a call that runs sweeps
struct SweepIo { const void* in; int64_t in_bytes; const void* out; int64_t out_bytes; };

// Every public call that runs sweeps goes through here.  A persistent sweep whose wait gave up leaves garbage in its panels and
// raises the abort words (the call's later persistent launches drain at once and add more garbage); the call sees the word behind
// the synchronisation that ends it -- none per chunk -- and is repeated from its inputs with a launch per product (the handle has
// left the persistent form for good).  So the persistent form is held off for a call whose inputs overlap its outputs (`io`: the
// repeat would read what the first pass wrote).  `body` enqueues the call and ends in its synchronisation; `restore`, if given,
// puts back before the repeat an input that the body changes in place.
static gmrf_status sweep_guarded(gmrf_handle* h, std::initializer_list<SweepIo> io, const std::function<gmrf_status()>& body,
                                 const std::function<gmrf_status()>& restore = nullptr) {
    h->stats.sweep_persist = 0;
    h->sweep_persist_hold = std::any_of(io.begin(), io.end(), [](const SweepIo& r) { return ranges_overlap(r.in, r.in_bytes, r.out, r.out_bytes); });
    GCHK(body());
    bool repeat = false;
    GCHK(sweep_persist_check(h, &repeat));
    if (!repeat) return GMRF_OK;
    if (restore) GCHK(restore());
    return body();
}

// tail (backward, via the GEMM only): the panels hold kp + 1 rows per problem and row kp -- the mean's right-hand side -- is swept
// as the tail row of every product (gemm_f64_dma's TAIL): the mean's backward sweep and the samples' in one pass over the factor.
// dout (with tail): the products that finish x_i also write the caller's mean and samples (gemm_f64_dma's DOUT)
static gmrf_status sweep_launches(gmrf_handle* h, bool backward, int kp, double* Pin, double* Yout, bool tail = false,
                                  const GemmDirectOut* dout = nullptr) {
    if (!tail && sweep_persist_ok(h, kp)) return launch_sweep_persist(h, backward, kp, Pin, Yout);
    const int bsp = (int)h->bsp;
    const int64_t ld = bsp, bstride = (int64_t)bsp * bsp, npad = h->n_pad;
    const int64_t N = h->N;
    SweepArgs s;
    s.ld = ld;
    const int nprob = (int)h->B;
    s.narrow = (nprob < 8 && bsp >= 512 && bsp <= SWEEP_PERSIST_XMAX) ? 1 : 0;      // (what sweep_persist's k = 1 bodies sum: 8-column blocks)
    const int64_t pPanel = (int64_t)(kp + (tail ? 1 : 0)) * npad;
    const int64_t pX = stride_pX(h), pCm = stride_pC(h);
    const int64_t ldc = c_ld(h), cstride = c_blk(h);
    // C_i is stored as its non-zero window (rows 0 .. rm, columns cm ..); inside it row tile t is zero
    // left of kst[t] (staircase).  forward: rows m < rm take sums over k >= cm + kst; backward (C^T):
    // outputs k >= cm take sums over the rows m < mend.
    const int cm = (int)h->cmin, rm = (int)h->rmax, wc = bsp - cm;
    // class 3 (k = 1): bytes the kernels stream (C inside the staircase, the lower triangle of Linv);
    // class 2: flops of the panel product
    const int pclass = (kp == 1) ? 3 : 2;
    const double blk_work_c = ((kp == 1) ? 8.0 * h->c_streamed : 2.0 * h->c_streamed * kp) * nprob;
    const double blk_work_t = ((kp == 1) ? 4.0 * bsp * (double)(bsp + 1) : 1.0 * bsp * (double)(bsp + 1) * kp) * nprob;
    // 64-multiples of right-hand sides go through the GEMM kernel (panel = the [m][k] operand) when
    // the batch gives it enough 64 x 64 tiles; a lone problem stays on sweep_mm (256 workgroups)
    const bool via_gemm = (kp % 64 == 0) && !h->sw(GMRF_SW_SWEEP_NO_GEMM) && (int64_t)nprob * (bsp / 64) * (kp / 64) >= 128;
    if (tail && (!via_gemm || !backward)) return bad_shape("internal: the tail row needs the backward sweep on the GEMM");
    if (dout && !tail) return bad_shape("internal: direct output needs the tail-row sweep");
    for (int64_t step = 0; step < N; ++step) {
        const int64_t i = backward ? (N - 1 - step) : step;
        double* rhs = Pin + i * bsp;               // the input panel is consumed: P_i becomes P_i - C y_prev
        if (step > 0) {
            // forward: P_i -= C_{i-1} y_{i-1};  backward: P_i -= C_i^T x_{i+1}      (in place)
            const int64_t ci = backward ? i : (i - 1);
            const int64_t prev = backward ? (i + 1) : (i - 1);
            const double* Cs = h->d_C + ci * cstride;
            const double* xin = Yout + prev * bsp + (backward ? 0 : cm);
            double* out = rhs + (backward ? cm : 0);
            const int rows = backward ? wc : rm, kdim = backward ? rm : wc;
            if (via_gemm) {
                // T[r][m] = P[r][m] - sum_k y[r][k] c(k,m): the panel is the [m][k] operand, the block the other
                GCHK(gemm(h, GemmCall(false, backward, kp, rows, kdim, -1.0, 1.0).a(xin, npad, pPanel).b(Cs, ldc, pCm).c(out, npad, pPanel)
                                 .work(2.0 * h->c_streamed * kp * nprob).k_begin(nullptr, backward ? nullptr : h->d_kst)
                                 .k_end(nullptr, backward ? h->d_mend : nullptr).tail_row(tail)));
            } else {
                s.Mat = Cs; s.ld = ldc; s.Xin = xin; s.ldx = npad; s.Bin = out; s.ldb = npad; s.Out = out; s.ldo = npad;
                s.rows = rows; s.kdim = kdim; s.sub = 1;
                s.pMat = pCm; s.pXin = pPanel; s.pBin = pPanel; s.pOut = pPanel;
                s.kst = h->d_kst; s.mend = h->d_mend;
                ProfScope ps(h, pclass, blk_work_c);
                HIPCHK(launch_sweep(h->stream, backward, false, kp, s, nprob));
            }
        }
        // y_i = Linv_i T   /   x_i = Linv_i^T T
        const double* X = h->d_Linv + i * bstride;
        double* yout = Yout + i * bsp;
        // On the GEMM, for the n columns from `first` on with the diagonal block Xd of the inverse -- forward: Linv stored [m][k], zero
        // for k > m; backward: Linv^T, stored [k][m], zero for k < m.  (dout) column c of the product is the dof i bs + first + c, real
        // while first + c < bs
        auto tri_product = [&](int first, int n, const double* Xd) {
            const GemmTail d{nullptr, 0, nullptr, 0, nullptr, 0, 0.0, dout, i * h->bs + first, (int)h->bs - first};
            return gemm(h, GemmCall(false, backward, kp, n, n, 1.0, 0.0).a(rhs + first, npad, pPanel).b(Xd, ld, pX).c(yout + first, npad, pPanel)
                               .triangular(backward ? TRI_B_LOWER : TRI_B_UPPER).tail_row(tail).tail_ops(dout ? &d : nullptr));
        };
        if (h->xsplit > 0) {
            // split representation: [X_aa 0; L_ba X_bb] in the block's storage.  forward: y_a = X_aa t_a, t_b -= L_ba y_a,
            // y_b = X_bb t_b;  backward: x_b = X_bb^T t_b, t_a -= L_ba^T x_b, x_a = X_aa^T t_a.  Same bytes, same flops.
            const int p = h->xsplit, q = bsp - p;
            const double* Xbb = X + (int64_t)p * ld + p;
            const double* Lba = X + (int64_t)p * ld;
            for (int part = 0; part < 3; ++part) {
                const int which = backward ? 2 - part : part;          // 0: aa, 1: ba, 2: bb
                if (via_gemm) {
                    if (which == 0) GCHK(tri_product(0, p, X));
                    else if (which == 2) GCHK(tri_product(p, q, Xbb));
                    else if (!backward)
                        GCHK(gemm(h, GemmCall(false, false, kp, q, p, -1.0, 1.0).a(yout, npad, pPanel).b(Lba, ld, pX).c(rhs + p, npad, pPanel)));
                    else {
                        // (round 19) envelope: column tile bn of L_ba = L[256:, 0:256] is zero below row env_ken[bn] (gmrf_handle)
                        const bool env = p == 256 && h->env_ok && !h->sw(GMRF_SW_NO_ENVELOPE) && !h->tw && !h->tw_half && h->tw_blk < 0 && h->env_ken_has[(size_t)i];
                        double units = 0.0;
                        for (int bn = 0; env && bn < 4; ++bn) units += h->env_ken[(size_t)(i * 4 + bn)] / 64;
                        GCHK(gemm(h, GemmCall(false, true, kp, p, q, -1.0, 1.0).a(yout + p, npad, pPanel).b(Lba, ld, pX).c(rhs, npad, pPanel)
                                         .work(env ? 2.0 * kp * 64.0 * 64.0 * units * nprob : -1.0)
                                         .k_end(nullptr, env ? h->d_env_ken + i * 4 : nullptr).k_hints(env).tail_row(tail)));
                    }
                } else {
                    s.ld = ld; s.ldx = npad; s.ldo = npad; s.pMat = pX; s.pXin = pPanel; s.pOut = pPanel; s.kst = nullptr; s.mend = nullptr;
                    if (which == 0) { s.Mat = X; s.Xin = rhs; s.Bin = nullptr; s.ldb = 0; s.Out = yout; s.rows = p; s.kdim = p; s.sub = 0; s.pBin = 0; }
                    else if (which == 2) { s.Mat = Xbb; s.Xin = rhs + p; s.Bin = nullptr; s.ldb = 0; s.Out = yout + p; s.rows = q; s.kdim = q; s.sub = 0; s.pBin = 0; }
                    else if (!backward) { s.Mat = Lba; s.Xin = yout; s.Bin = rhs + p; s.ldb = npad; s.Out = rhs + p; s.rows = q; s.kdim = p; s.sub = 1; s.pBin = pPanel; }
                    else { s.Mat = Lba; s.Xin = yout + p; s.Bin = rhs; s.ldb = npad; s.Out = rhs; s.rows = p; s.kdim = q; s.sub = 1; s.pBin = pPanel; }
                    const double frac = which == 0 ? (double)p * (p + 1) : (which == 2 ? (double)q * (q + 1) : 2.0 * p * q);
                    ProfScope ps(h, pclass, blk_work_t * frac / ((double)bsp * (bsp + 1)));
                    HIPCHK(launch_sweep(h->stream, backward, which != 1, kp, s, nprob));
                }
            }
        } else if (via_gemm) {
            GCHK(tri_product(0, bsp, X));
        } else {
            s.Mat = X; s.ld = ld; s.Xin = rhs; s.ldx = npad; s.Bin = nullptr; s.ldb = 0; s.Out = yout; s.ldo = npad;
            s.rows = bsp; s.kdim = bsp; s.sub = 0;
            s.pMat = pX; s.pXin = pPanel; s.pBin = 0; s.pOut = pPanel;
            s.kst = nullptr; s.mend = nullptr;
            ProfScope ps(h, pclass, blk_work_t);
            HIPCHK(launch_sweep(h->stream, backward, true, kp, s, nprob));
        }
    }
    return GMRF_OK;
}

// mode: 1 forward P->Y, 2 backward P->Y, 0 full P->Y->P (result in P); 3 backward Y->P (the second half of a twisted solve);
// 4 backward P->Y of kp + 1 rows per problem, row kp the tail row (posterior_fused)
constexpr int SWEEP_BACKWARD_YP = 3, SWEEP_BACKWARD_TAIL = 4;
static gmrf_status run_sweeps(gmrf_handle* h, int mode, int kp) {
    auto body = [&]() -> gmrf_status {
        if (mode == GMRF_SOLVE_FORWARD) return sweep_launches(h, false, kp, h->d_P, h->d_Y);
        if (mode == SWEEP_BACKWARD_TAIL) return sweep_launches(h, true, kp, h->d_P, h->d_Y, true, h->d_dout);
        if (mode == SWEEP_BACKWARD_YP) return sweep_launches(h, true, kp, h->d_Y, h->d_P);
        if (mode == GMRF_SOLVE_BACKWARD) return sweep_launches(h, true, kp, h->d_P, h->d_Y);
        GCHK(sweep_launches(h, false, kp, h->d_P, h->d_Y));
        return sweep_launches(h, true, kp, h->d_Y, h->d_P);
    };
    const bool persistent = mode != SWEEP_BACKWARD_TAIL && sweep_persist_ok(h, kp);
    if (persistent) {
        GCHK(sweep_persist_prepare(h, kp));
        h->sweep_persist_launched = true;                  // (here, not at the launch: a graph replay launches it too)
        h->stats.sweep_persist = 1;
        h->stats.sweep_persist_launches += (mode == GMRF_SOLVE_FULL) ? 2 : 1;
    }
    if (h->sw(GMRF_SW_EAGER) || h->profiling) return body();
    const int64_t key = ((int64_t)h->xsplit << 32) | ((int64_t)mode * 4096 + kp) |       // (the representation decides the launches)
                        (persistent ? ((int64_t)1 << 60) : 0);
    auto it = h->sweep_graphs.find(key);
    if (it == h->sweep_graphs.end()) {
        std::lock_guard<std::mutex> capture_lock(g_capture_mu);
        hipGraph_t graph = nullptr;
        hipGraphExec_t exec = nullptr;
        HIPCHK(hipStreamBeginCapture(h->stream, hipStreamCaptureModeThreadLocal));
        gmrf_status s = body();
        hipError_t e = hipStreamEndCapture(h->stream, &graph);
        if (s != GMRF_OK) { if (graph) (void)hipGraphDestroy(graph); return s; }
        HIPCHK(e);
        HIPCHK(hipGraphInstantiate(&exec, graph, nullptr, nullptr, 0));
        (void)hipGraphDestroy(graph);
        it = h->sweep_graphs.emplace(key, exec).first;
    }
    HIPCHK(hipGraphLaunch(it->second, h->stream));
    return GMRF_OK;
}

static int pad_k(int64_t k) { return k == 1 ? 1 : (int)((k + 15) / 16 * 16); }

static gmrf_status launch_pack(gmrf_handle* h, const double* d_src, int64_t ld, int k, int kp) {
    const int64_t total = (int64_t)kp * h->n_pad;
    hipLaunchKernelGGL(pack_panel, dim3((unsigned)((total + 255) / 256), (unsigned)h->B), dim3(256), 0, h->stream, d_src, ld,
                       h->d_P, h->n_pad, (int)h->bs, (int)h->bsp, (int)h->N, k, kp);
    HIPCHK(hipGetLastError());
    return GMRF_OK;
}

static gmrf_status launch_unpack(gmrf_handle* h, const double* panel, double* d_dst, int64_t ld, int k,
                                 const double* d_mean) {
    const int64_t total = h->n * (int64_t)k;
    hipLaunchKernelGGL(unpack_panel, dim3((unsigned)((total + 255) / 256), (unsigned)h->B), dim3(256), 0, h->stream, panel,
                       h->n_pad, d_dst, ld, (int)h->bs, (int)h->bsp, h->n, k, pad_k(k), d_mean);
    HIPCHK(hipGetLastError());
    return GMRF_OK;
}

// k columns per problem of the caller's (src, ld) as the pack reads them: where they lie in device memory, else copied into
// d_stage (leading dimension n)
static gmrf_status cols_in(gmrf_handle* h, const double* src, int64_t ld, bool src_dev, int k, const double** d_src, int64_t* d_ld) {
    *d_src = src; *d_ld = ld;
    if (src_dev) return GMRF_OK;
    GCHK(ensure_stage(h, (int64_t)k * h->n * h->B));
    HIPCHK(hipMemcpy2DAsync(h->d_stage, h->n * sizeof(double), src, ld * sizeof(double),
                            h->n * sizeof(double), k * h->B, hipMemcpyHostToDevice, h->stream));
    *d_src = h->d_stage; *d_ld = h->n;
    return GMRF_OK;
}

// k columns per problem of a panel (plus d_mean, if given) out to the caller's (dst, ld): unpacked there if it is device memory,
// else into d_stage and copied to the host from there (the caller synchronises)
static gmrf_status cols_out(gmrf_handle* h, const double* panel, int k, const double* d_mean, double* dst, int64_t ld, bool dst_dev) {
    if (dst_dev) return launch_unpack(h, panel, dst, ld, k, d_mean);
    GCHK(ensure_stage(h, (int64_t)k * h->n * h->B));
    GCHK(launch_unpack(h, panel, h->d_stage, h->n, k, d_mean));
    HIPCHK(hipMemcpy2DAsync(dst, ld * sizeof(double), h->d_stage, h->n * sizeof(double),
                            h->n * sizeof(double), k * h->B, hipMemcpyDeviceToHost, h->stream));
    return GMRF_OK;
}

constexpr int64_t KP_CHUNK = 128;

// the twisted order (implemented with the variances, below)
static void tw_free(gmrf_handle* h);
static gmrf_status tw_analyze(gmrf_handle* h, int64_t n, int64_t N, const int64_t* colptr, const int64_t* rowval, int32_t base);
static gmrf_status tw_numeric(gmrf_handle* h, const double* nzval, int32_t* info);
static gmrf_status tw_solve(gmrf_handle* h, const double* b, double* y, int64_t k, int64_t ldb, int64_t ldy, int mode);
static gmrf_status tw_sample(gmrf_handle* h, uint64_t seed, int64_t first_id, int64_t k, const double* mean, const double* z,
                             double* out, int64_t ld);
static gmrf_status tw_logdet(gmrf_handle* h, double* out);
static gmrf_status tw_get_block(gmrf_handle* h, int32_t kind, int64_t i, double* out, int64_t ld);
static gmrf_status tw_var_exact(gmrf_handle* h, double* d_out);
static gmrf_status tw_var_accumulate_dev(gmrf_handle* h, int method, int64_t first_id, int64_t k, uint64_t seed, const gmrf_csr* Q,
                                         double* d_acc);

// ------------------------------------------------------------------------------------ C ABI
extern "C" {

int32_t gmrf_version(void) { return 100; }
const char* gmrf_last_error(void) { return g_last_error.c_str(); }

gmrf_status gmrf_bt_create(int32_t device, void* stream, gmrf_handle** out) {
    if (!out) return bad_shape("null out pointer");
    int count = 0;
    if (hipGetDeviceCount(&count) != hipSuccess || count <= 0 || device < 0 || device >= count) {
        (void)hipGetLastError();
        g_last_error = "no HIP device visible (libgmrf_hip needs an MI355X / gfx950 GPU)";
        return GMRF_ERR_NO_DEVICE;
    }
    HIPCHK(hipSetDevice(device));
    std::unique_ptr<gmrf_handle, gmrf_status (*)(gmrf_handle*)> guard(new gmrf_handle(), gmrf_bt_destroy);
    gmrf_handle* h = guard.get();
    memset(&h->stats, 0, sizeof(h->stats));
    h->device = device;
    if (stream) { h->stream = (hipStream_t)stream; h->own_stream = false; }
    else { HIPCHK(hipStreamCreateWithFlags(&h->stream, hipStreamNonBlocking)); h->own_stream = true; }
    GCHK(h->d_info.reserve(h->stream, 4));                    // [0] info, [1] abort word of the persistent kernel
    HIPCHK(hipMemsetAsync(h->d_info, 0, 4 * sizeof(int), h->stream));
    HIPCHK(hipStreamSynchronize(h->stream));
    HIPCHK(hipEventCreate(&h->ev0));
    HIPCHK(hipEventCreate(&h->ev1));
    HIPCHK(hipFuncSetAttribute((const void*)potrf_step<false>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)POTRF_STEP_LDS));
    HIPCHK(hipFuncSetAttribute((const void*)potrf_diag128, hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024));
    HIPCHK(hipFuncSetAttribute((const void*)potrf_persist<false>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)POTRF_PERSIST_LDS));
    HIPCHK(hipDeviceGetAttribute(&h->cu_count, hipDeviceAttributeMultiprocessorCount, device));
    HIPCHK(hipFuncSetAttribute((const void*)potrf_diag128_slim, hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024));
    HIPCHK(gemm_init());
    HIPCHK(gemm_dma_init());
    *out = guard.release();
    return GMRF_OK;
}

gmrf_status gmrf_bt_destroy(gmrf_handle* h) {
    if (!h) return GMRF_OK;
    (void)hipSetDevice(h->device);
    tw_free(h);
    (void)hipStreamSynchronize(h->stream);
    persist_release(h);
    destroy_graphs(h);
    for (auto e : h->ev_pool) (void)hipEventDestroy(e);
    if (h->ev0) (void)hipEventDestroy(h->ev0);
    if (h->ev1) (void)hipEventDestroy(h->ev1);
    for (auto e : h->fork_events) (void)hipEventDestroy(e);
    if (h->aux) (void)hipStreamDestroy(h->aux);
    h->close();
    delete h;
    return GMRF_OK;
}

gmrf_status gmrf_bt_set_batch(gmrf_handle* h, int64_t batch) {
    if (!h || batch < 1 || batch > 4096) return bad_shape("batch must be in [1, 4096]");
    if (batch != 1) GCHK(tw_refuse(h, "gmrf_bt_set_batch (batch > 1)"));
    if (batch != h->B) {
        HIPCHK(hipSetDevice(h->device));
        HIPCHK(hipStreamSynchronize(h->stream));
        destroy_graphs(h);
        h->B = batch;
        h->sel = 0;
        h->factored = false;
        release_shape_buffers(h);
        if (h->n > 0) (void)set_shape(h, h->n, h->N);      // flop accounting follows the batch
    }
    return GMRF_OK;
}

gmrf_status gmrf_bt_select_problem(gmrf_handle* h, int64_t p) {
    if (!h || p < 0 || p >= h->B) return bad_shape("problem index out of range");
    h->sel = p;
    return GMRF_OK;
}

gmrf_status gmrf_bt_set_profiling(gmrf_handle* h, int32_t level) {
    if (!h) return bad_shape("null handle");
    h->profiling = level;
    if (h->tw)
        for (gmrf_handle* s : {h->tw->top, h->tw->bot}) if (s) GCHK(gmrf_bt_set_profiling(s, level));
    if (level > 0 && h->events.empty()) h->gemm_shapes.clear();
    for (int i = 0; i < GMRF_KERNEL_CLASSES; ++i) { h->stats.kernel_ms[i] = h->stats.kernel_work[i] = 0; h->stats.kernel_launches[i] = 0; }
    return GMRF_OK;
}

// The switches whose change leaves the captured graphs holding other launches than the next capture would record: every live one
// but GMRF_SW_EAGER (the graphs stay good, they are just not replayed), GMRF_SW_NO_STAIRCASE (takes effect at the next analysis,
// which drops them itself), GMRF_SW_TWO_CALL_POSTERIOR (chooses which calls a posterior makes, outside any graph) and
// GMRF_SW_NO_FACTOR_FWD (the factor graph is kept per right-hand side: factor_graph_rhs).
static const int32_t SW_DROP_GRAPHS =
    GMRF_SW_BATCH_ROUTES | GMRF_SW_SWEEP_NO_GEMM | GMRF_SW_DENSE_COUPLING | GMRF_SW_FORK_GRAPH | GMRF_SW_DOUBLING_INVERSE | GMRF_SW_NO_LOOKAHEAD
    | GMRF_SW_NO_XSPLIT | GMRF_SW_NO_PERSIST | GMRF_SW_NO_PERSIST_PANELS | GMRF_SW_NO_SWEEP_PERSIST | GMRF_SW_NO_SCATTER_FOLD
    | GMRF_SW_NO_GROUPED_GEMM | GMRF_SW_NO_ENVELOPE;

gmrf_status gmrf_bt_set_eager(gmrf_handle* h, int32_t eager) {
    if (!h) return bad_shape("null handle");
    if ((eager ^ h->switches) & SW_DROP_GRAPHS) destroy_graphs(h);
    if (eager != h->switches) h->fy_for = nullptr;         // (a factor of other settings: no y taken for granted)
    h->switches = eager;
    if (h->tw)
        for (gmrf_handle* s : {h->tw->top, h->tw->bot})
            if (s) {
                GCHK(gmrf_bt_set_eager(s, eager));
                if (h->tw->bot) s->switches |= GMRF_SW_NO_SWEEP_PERSIST;       // (two halves never take the persistent sweep)
            }
    return GMRF_OK;
}

gmrf_status gmrf_bt_synchronize(gmrf_handle* h) {
    if (!h) return bad_shape("null handle");
    HIPCHK(hipStreamSynchronize(h->stream));
    if (tw_on(h)) HIPCHK(hipStreamSynchronize(h->tw->bot->stream));
    return GMRF_OK;
}

gmrf_status gmrf_bt_stats(gmrf_handle* h, gmrf_stats* out) {
    if (!h || !out) return bad_shape("null pointer");
    if (tw_on(h)) {
        // a twisted handle: its own timings, the halves' persistent launches (aborts summed)
        const gmrf_stats &a = h->tw->top->stats, &b = h->tw->bot->stats;
        *out = h->stats;
        out->persist_route = a.persist_route;
        out->persist_aborts = a.persist_aborts + b.persist_aborts;
        out->persist_cus = a.persist_cus + b.persist_cus;
        out->persist_refused = a.persist_refused | b.persist_refused;
        out->factor_bytes = a.factor_bytes + b.factor_bytes;
        return GMRF_OK;
    }
    h = tw_route(h);
    *out = h->stats;
    return GMRF_OK;
}

gmrf_status gmrf_bt_factor_csc(gmrf_handle* h, int64_t n, int64_t n_blocks, const int64_t* colptr,
                               const int64_t* rowval, const double* nzval, int32_t index_base,
                               int32_t* info) {
    if (!h) return bad_shape("null handle");
    HIPCHK(hipSetDevice(h->device));
    if (info) *info = 0;
    if (h->order == GMRF_ORDER_TWISTED) {
        GCHK(tw_analyze(h, n, n_blocks, colptr, rowval, index_base));
        return tw_numeric(h, nzval, info);
    }
    GCHK(analyze_csc(h, n, n_blocks, colptr, rowval, index_base));
    return numeric_factor(h, nzval, info);
}

gmrf_status gmrf_bt_factor_begin_csc(gmrf_handle* h, int64_t n, int64_t n_blocks, const int64_t* colptr,
                                     const int64_t* rowval, const double* nzval, int32_t index_base) {
    GCHK(tw_refuse(h, "gmrf_bt_factor_begin_csc"));
    if (!h) return bad_shape("null handle");
    HIPCHK(hipSetDevice(h->device));
    if (colptr) GCHK(analyze_csc(h, n, n_blocks, colptr, rowval, index_base));
    if (!h->analyzed) { g_last_error = "no sparsity pattern analysed"; return GMRF_ERR_NO_FACTOR; }
    GCHK(alloc_factor(h));
    if (h->c_dirty) {
        HIPCHK(hipMemsetAsync(h->d_C, 0, sizeof(double) * stride_pC(h) * h->B, h->stream));
        h->c_dirty = false;
    }
    persist_plan(h);
    GCHK(load_values(h, nzval));
    HIPCHK(hipMemsetAsync(h->d_info, 0, 4 * sizeof(int), h->stream));
    h->info_checked = 0; h->persist_launched = false; h->stats.persist_route = 0;
    h->factored = false; h->fy_for = nullptr;
    return GMRF_OK;
}

gmrf_status gmrf_bt_factor_step_async(gmrf_handle* h, int64_t i0, int64_t i1) {
    GCHK(tw_refuse(h, "gmrf_bt_factor_step_async"));
    if (!h) return bad_shape("null handle");
    if (i0 < 0 || i1 > h->N || i0 > i1) return bad_shape("bad block range");
    HIPCHK(hipSetDevice(h->device));
    // block ranges are launched directly (a graph per range would have to be re-captured)
    GCHK(factor_blocks_range(h, i0, i1));
    // A range that holds persistent launches is waited for here and repeated launch-per-step if one of them gave up, so that
    // what the caller packs / broadcasts next is the factor (the call is asynchronous only for handles without such launches)
    if (h->persist_launched) GCHK(persist_check_range(h, i0, i1, nullptr));
    return GMRF_OK;
}

gmrf_status gmrf_bt_factor_end(gmrf_handle* h, int32_t* info) {
    GCHK(tw_refuse(h, "gmrf_bt_factor_end"));
    if (!h) return bad_shape("null handle");
    HIPCHK(hipSetDevice(h->device));
    gmrf_status s = factor_finish(h, info);
    if (h->profiling) prof_collect(h);
    return s;
}

gmrf_status gmrf_bt_refactor_values(gmrf_handle* h, const double* nzval, int32_t* info) {
    if (!h) return bad_shape("null handle");
    HIPCHK(hipSetDevice(h->device));
    if (info) *info = 0;
    if (h->order == GMRF_ORDER_TWISTED) return tw_numeric(h, nzval, info);
    return numeric_factor(h, nzval, info);
}

gmrf_status gmrf_bt_factor_blocks(gmrf_handle* h, int64_t n, int64_t n_blocks, const gmrf_sparse_block* diag,
                                  const gmrf_sparse_block* lower, int32_t index_base,
                                  int32_t compressed_by_column, int32_t* info) {
    GCHK(tw_refuse(h, "gmrf_bt_factor_blocks"));
    if (!h || !diag || (n_blocks > 1 && !lower)) return bad_shape("null pointer");
    HIPCHK(hipSetDevice(h->device));
    if (info) *info = 0;
    GCHK(set_shape(h, n, n_blocks));
    const int64_t bs = h->bs;
    std::vector<std::vector<HostEntry>> dg(n_blocks), lo(n_blocks);
    std::vector<double> vals;
    auto add_block = [&](const gmrf_sparse_block& b, std::vector<HostEntry>& dst, bool lower_tri_only) -> bool {
        for (int64_t o = 0; o < bs; ++o) {
            for (int64_t p = b.ptr[o] - index_base; p < b.ptr[o + 1] - index_base; ++p) {
                const int64_t in = b.idx[p] - index_base;
                if (in < 0 || in >= bs) return false;
                const int64_t r = compressed_by_column ? in : o, c = compressed_by_column ? o : in;
                if (lower_tri_only && r < c) continue;
                dst.push_back({((uint64_t)r << 32) | (uint64_t)c, (int64_t)vals.size()});
                vals.push_back(b.val[p]);
            }
        }
        return true;
    };
    for (int64_t i = 0; i < n_blocks; ++i) {
        if (!add_block(diag[i], dg[i], true)) return bad_shape("block index out of range");
        if (i > 0 && !add_block(lower[i - 1], lo[i], false)) return bad_shape("block index out of range");
    }
    GCHK(upload_entries(h, dg, lo, (int64_t)vals.size()));
    return numeric_factor(h, vals.data(), info);
}


gmrf_status gmrf_bt_storage_bytes(int64_t n, int64_t n_blocks, int64_t batch, int64_t* bytes_L, int64_t* bytes_C,
                                  int64_t* bytes_Linv) {
    if (n <= 0 || n_blocks <= 0 || n % n_blocks != 0 || batch < 1 || !bytes_L || !bytes_C || !bytes_Linv)
        return bad_shape("n must be a positive multiple of N_blocks, batch >= 1");
    const int64_t bs = n / n_blocks, bsp = 64 * next_pow2((bs + 63) / 64);
    const int64_t blk = bsp * bsp * (int64_t)sizeof(double) * batch;
    *bytes_L = blk * n_blocks; *bytes_Linv = blk * n_blocks; *bytes_C = blk * std::max<int64_t>(n_blocks - 1, 1);
    return GMRF_OK;
}

gmrf_status gmrf_bt_set_storage(gmrf_handle* h, int64_t n, int64_t n_blocks, int64_t batch, void* dev_L, void* dev_C,
                                void* dev_Linv) {
    GCHK(tw_refuse(h, "gmrf_bt_set_storage"));
    if (!h || !dev_C || !dev_Linv) return bad_shape("null pointer");
    if (batch != h->B) return bad_shape("storage batch differs from the handle's batch (gmrf_bt_set_batch first)");
    if (!dev_L && h->keep_l) return bad_shape("dev_L may be NULL only after gmrf_bt_set_keep_l(h, 0)");
    HIPCHK(hipSetDevice(h->device));
    GCHK(set_shape(h, n, n_blocks));
    HIPCHK(hipStreamSynchronize(h->stream));
    destroy_graphs(h);
    release_factor(h);                                 // (frees what is ours: an earlier call's storage stays the caller's)
    const size_t be = (size_t)blk_elems(h) * (size_t)h->B;
    h->d_C.borrow((double*)dev_C, be * (size_t)std::max<int64_t>(h->N - 1, 1));
    h->d_Linv.borrow((double*)dev_Linv, be * (size_t)h->N);
    h->external_storage = true;
    h->factored = false; h->l_valid = false; h->logdet_valid = false;   // whatever was factored lived in the old buffers
    if (h->keep_l) h->d_L.borrow((double*)dev_L, be * (size_t)h->N);
    else {                                             // one-block work buffer for L_i: ours
        GCHK(h->d_L.reserve(h->stream, be));
        HIPCHK(hipMemsetAsync(h->d_L, 0, (size_t)blk_elems(h) * sizeof(double) * (size_t)h->B, h->stream));
    }
    if (!h->analyzed) GCHK(set_layout_dense(h));      // until a pattern is analysed / a layout adopted
    // tiles strictly above the block diagonal of L / Linv are never written: keep them zero
    const size_t blk = (size_t)blk_elems(h) * sizeof(double) * (size_t)h->B;
    if (h->keep_l) HIPCHK(hipMemsetAsync(h->d_L, 0, blk * h->N, h->stream));
    HIPCHK(hipMemsetAsync(h->d_Linv, 0, blk * h->N, h->stream));
    HIPCHK(hipMemsetAsync(h->d_C, 0, blk * std::max<int64_t>(h->N - 1, 1), h->stream));
    h->c_dirty = false;
    GCHK(alloc_work(h));
    h->alloc_rm = h->rmax; h->alloc_wc = c_ld(h); h->alloc_keep_l = h->keep_l;
    HIPCHK(hipStreamSynchronize(h->stream));
    return GMRF_OK;
}

gmrf_status gmrf_bt_set_keep_l(gmrf_handle* h, int32_t keep) {
    GCHK(tw_refuse(h, "gmrf_bt_set_keep_l"));
    if (!h) return bad_shape("null handle");
    if ((keep != 0) == h->keep_l) return GMRF_OK;
    if (h->external_storage) return bad_shape("choose gmrf_bt_set_keep_l before gmrf_bt_set_storage");
    HIPCHK(hipSetDevice(h->device));
    HIPCHK(hipStreamSynchronize(h->stream));
    destroy_graphs(h);
    h->keep_l = keep != 0;
    h->factored = false; h->l_valid = false; h->logdet_valid = false;
    return GMRF_OK;
}

// Layout of the stored coupling blocks: out = {cmin, rmax, n_row_tiles, kst[0 .. n_row_tiles)} (kst relative to cmin).
gmrf_status gmrf_bt_get_layout(gmrf_handle* h, int64_t* out, int64_t cap, int64_t* count) {
    GCHK(tw_refuse(h, "gmrf_bt_get_layout"));
    if (!h || !count) return bad_shape("null pointer");
    if (h->N <= 0 || h->kst.empty()) { g_last_error = "no shape"; return GMRF_ERR_NO_FACTOR; }
    const int64_t nrt = h->rmax / 64;
    *count = 4 + nrt;
    if (!out) return GMRF_OK;
    if (cap < 4 + nrt) return bad_shape("layout buffer too small");
    out[0] = h->cmin; out[1] = h->rmax; out[2] = nrt;
    for (int64_t t = 0; t < nrt; ++t) out[3 + t] = h->kst[(size_t)t];
    // representation of the block inverses (gmrf_handle::xsplit): of the stored factor, or what the next factorisation will leave
    out[3 + nrt] = h->factored ? h->xsplit : planned_xsplit(h);
    return GMRF_OK;
}

// A rank that receives the factor by broadcast: shape + the root's layout (NULL: dense coupling blocks),
// storage allocated (or the caller's, gmrf_bt_set_storage), nothing factored yet.
gmrf_status gmrf_bt_adopt_layout(gmrf_handle* h, int64_t n, int64_t n_blocks, const int64_t* layout, int64_t count) {
    GCHK(tw_refuse(h, "gmrf_bt_adopt_layout"));
    if (!h) return bad_shape("null handle");
    HIPCHK(hipSetDevice(h->device));
    GCHK(set_shape(h, n, n_blocks));
    h->analyzed = false;                               // whatever pattern was analysed does not describe this factor
    if (layout) {
        if (count < 3 || layout[2] < 1 || count < 3 + layout[2] || layout[1] != 64 * layout[2]) return bad_shape("bad layout record");
        std::vector<int64_t> first((size_t)layout[2]);
        for (int64_t t = 0; t < layout[2]; ++t) first[(size_t)t] = layout[0] + layout[3 + t];
        GCHK(set_layout(h, layout[0], layout[1], first));
        h->adopt_xsplit = 0;
        if (count >= 4 + layout[2]) {
            const int64_t xs = layout[3 + layout[2]];
            if (xs < 0 || xs >= h->bsp || xs % 64) return bad_shape("bad layout record (split)");
            h->adopt_xsplit = (int)xs;
        }
    } else {
        GCHK(set_layout_dense(h));
        h->adopt_xsplit = 0;
    }
    GCHK(alloc_factor(h));
    if (h->c_dirty) {
        HIPCHK(hipMemsetAsync(h->d_C, 0, sizeof(double) * stride_pC(h) * h->B, h->stream));
        h->c_dirty = false;
    }
    h->factored = false; h->l_valid = false; h->logdet_valid = false;
    h->got_block.assign((size_t)h->N, 0);
    HIPCHK(hipStreamSynchronize(h->stream));
    return GMRF_OK;
}

gmrf_status gmrf_bt_adopt_shape(gmrf_handle* h, int64_t n, int64_t n_blocks) {
    GCHK(tw_refuse(h, "gmrf_bt_adopt_shape"));
    return gmrf_bt_adopt_layout(h, n, n_blocks, nullptr, 0);
}

// l_blocks_valid != 0: the caller also filled the L buffer (gmrf_bt_factor_buffer kind L), so F.chos / logdet work
gmrf_status gmrf_bt_adopt_commit(gmrf_handle* h, int32_t l_blocks_valid) {
    GCHK(tw_refuse(h, "gmrf_bt_adopt_commit"));
    if (!h || !h->d_Linv) return bad_shape("no factor storage");
    HIPCHK(hipSetDevice(h->device));
    // Representation of the block inverses: a packed image says which form ITS sender was in when it packed (the layout record
    // may be older than that: the sender converts to the full form for get_block / export / exact variances and goes back to the
    // split form at its next factorisation); raw buffer transfers carry no tag and follow the record.
    int seen = 0;
    HIPCHK(hipMemcpyAsync(&seen, h->d_info + 2, sizeof(int), hipMemcpyDeviceToHost, h->stream));
    HIPCHK(hipStreamSynchronize(h->stream));
    if (seen != 0) HIPCHK(hipMemsetAsync(h->d_info + 2, 0, sizeof(int), h->stream));
    if (seen < 0) { g_last_error = "the packed ranges of this factor carry different (or no) representation tags"; return GMRF_ERR_BAD_SHAPE; }
    const int xs = seen > 0 ? seen - 1 : h->adopt_xsplit;
    if (xs < 0 || xs >= h->bsp || xs % 64) { g_last_error = "bad representation tag in the packed image"; return GMRF_ERR_BAD_SHAPE; }
    h->factored = true; h->fy_for = nullptr;
    h->xsplit = xs;
    h->l_valid = l_blocks_valid != 0 && h->keep_l;
    // the log-determinant parts travel inside the packed transport image (gmrf_bt_unpack_blocks_async): valid once
    // every block of this factor came that way; a factor moved as raw buffers has none (logdet then needs the L blocks)
    bool all = !h->got_block.empty();
    for (char g : h->got_block) all = all && g;
    h->logdet_valid = all;
    h->got_block.assign((size_t)h->N, 0);
    persist_plan(h);                   // (a receiver's sweeps may be persistent launches too: the claim is planned where a factor becomes usable)
    return GMRF_OK;
}

gmrf_status gmrf_bt_factor_buffer(gmrf_handle* h, int32_t kind, void** dev_ptr, int64_t* bytes) {
    GCHK(tw_refuse(h, "gmrf_bt_factor_buffer"));
    if (!h || !dev_ptr || !bytes) return bad_shape("null pointer");
    if (!h->d_Linv) { g_last_error = "no factor storage"; return GMRF_ERR_NO_FACTOR; }
    const int64_t blk = blk_elems(h) * (int64_t)sizeof(double) * h->B;
    if (kind == GMRF_BLOCK_L) {
        if (!h->keep_l) { g_last_error = "L blocks are not kept (gmrf_bt_set_keep_l)"; return GMRF_ERR_NO_FACTOR; }
        *dev_ptr = h->d_L; *bytes = blk * h->N;
    }
    else if (kind == GMRF_BLOCK_C) { *dev_ptr = h->d_C; *bytes = stride_pC(h) * (int64_t)sizeof(double) * h->B; }
    else if (kind == GMRF_BLOCK_LINV) { *dev_ptr = h->d_Linv; *bytes = blk * h->N; }
    else return bad_shape("bad block kind");
    return GMRF_OK;
}

// Element ranges (in doubles, per problem) of blocks [i0, i1) inside the three factor buffers: what a
// block-range broadcast moves.  C holds the coupling blocks i0-1 .. i1-2 (C_i couples blocks i and i+1).
gmrf_status gmrf_bt_block_range(gmrf_handle* h, int32_t kind, int64_t i0, int64_t i1, int64_t* first_elem,
                                int64_t* n_elems, int64_t* problem_stride) {
    GCHK(tw_refuse(h, "gmrf_bt_block_range"));
    if (!h || !first_elem || !n_elems || !problem_stride) return bad_shape("null pointer");
    if (h->N <= 0 || i0 < 0 || i1 > h->N || i0 > i1) return bad_shape("bad block range");
    if (kind == GMRF_BLOCK_C) {
        const int64_t c0 = std::max<int64_t>(i0 - 1, 0), c1 = std::max<int64_t>(i1 - 1, 0);
        *first_elem = c0 * c_blk(h); *n_elems = (c1 - c0) * c_blk(h); *problem_stride = stride_pC(h);
    } else if (kind == GMRF_BLOCK_LINV || kind == GMRF_BLOCK_L) {
        if (kind == GMRF_BLOCK_L && !h->keep_l) { g_last_error = "L blocks are not kept"; return GMRF_ERR_NO_FACTOR; }
        *first_elem = i0 * blk_elems(h); *n_elems = (i1 - i0) * blk_elems(h);
        *problem_stride = kind == GMRF_BLOCK_L ? stride_pL(h) : stride_pX(h);
    } else return bad_shape("bad block kind");
    return GMRF_OK;
}

// Packed transport image of the blocks [i0, i1) of every problem of the batch: per problem one segment of
//   (i1 - i0) * ntri * 4096   lower-triangular 64 x 64 tiles of Linv_i0 .. Linv_{i1-1} (linv_tiles_copy),
//   (c1 - c0) * c_blk          stored windows of the coupling blocks C_{i0-1} .. C_{i1-2},
//   2                          representation tag {xsplit of the sender, magic} (pack_tag_write: the receiver's commit follows it)
//   (i1 - i0) rounded to even  log-determinant parts of the blocks
// doubles: darcy256 0.56 GB per posterior instead of the 0.83 GB of the raw Linv / C buffers.
static void packed_counts(const gmrf_handle* h, int64_t i0, int64_t i1, int64_t* x_elems, int64_t* c_elems, int64_t* ld_elems,
                          int64_t* c0_out) {
    const int64_t nt = h->bsp / 64, ntri = nt * (nt + 1) / 2;
    const int64_t c0 = std::max<int64_t>(i0 - 1, 0), c1 = std::max<int64_t>(i1 - 1, 0);
    *x_elems = (i1 - i0) * ntri * 4096;
    *c_elems = (c1 - c0) * c_blk(h);
    *ld_elems = 2 + ((i1 - i0) + 1) / 2 * 2;
    if (c0_out) *c0_out = c0;
}

gmrf_status gmrf_bt_packed_size(gmrf_handle* h, int64_t i0, int64_t i1, int64_t* elems_per_problem) {
    GCHK(tw_refuse(h, "gmrf_bt_packed_size"));
    if (!h || !elems_per_problem) return bad_shape("null pointer");
    if (h->N <= 0 || i0 < 0 || i1 > h->N || i0 >= i1) return bad_shape("bad block range");
    int64_t xe, ce, le;
    packed_counts(h, i0, i1, &xe, &ce, &le, nullptr);
    *elems_per_problem = xe + ce + le;
    return GMRF_OK;
}

static gmrf_status pack_blocks_on(gmrf_handle* h, hipStream_t st, int64_t i0, int64_t i1, double* buf, bool pack) {
    if (!h->d_Linv || h->N <= 0) { g_last_error = "no factor storage"; return GMRF_ERR_NO_FACTOR; }
    if (i0 < 0 || i1 > h->N || i0 >= i1) return bad_shape("bad block range");
    if (!buf || !is_device_ptr(buf)) return bad_shape("the transport image lives in device memory");
    int64_t xe, ce, le, c0;
    packed_counts(h, i0, i1, &xe, &ce, &le, &c0);
    const int64_t seg = xe + ce + le;
    const int nt = (int)(h->bsp / 64), ntri = nt * (nt + 1) / 2;
    const dim3 grid((unsigned)(ntri * (i1 - i0)), (unsigned)h->B);
    double* X = h->d_Linv + i0 * blk_elems(h);
    if (pack) hipLaunchKernelGGL(linv_tiles_copy<true>, grid, dim3(256), 0, st, X, h->bsp, blk_elems(h), stride_pX(h), buf, seg, ntri);
    else hipLaunchKernelGGL(linv_tiles_copy<false>, grid, dim3(256), 0, st, X, h->bsp, blk_elems(h), stride_pX(h), buf, seg, ntri);
    HIPCHK(hipGetLastError());
    if (ce > 0) {
        double* Cw = h->d_C + c0 * c_blk(h);
        if (pack) HIPCHK(hipMemcpy2DAsync(buf + xe, seg * sizeof(double), Cw, stride_pC(h) * sizeof(double), ce * sizeof(double),
                                          (size_t)h->B, hipMemcpyDeviceToDevice, st));
        else HIPCHK(hipMemcpy2DAsync(Cw, stride_pC(h) * sizeof(double), buf + xe, seg * sizeof(double), ce * sizeof(double),
                                     (size_t)h->B, hipMemcpyDeviceToDevice, st));
    }
    if (pack && h->keep_l) {
        // with the L blocks resident nobody has taken their log-determinant parts yet
        hipLaunchKernelGGL(logdet_blocks, dim3((unsigned)(i1 - i0), (unsigned)h->B), dim3(256), 0, st, h->d_L + i0 * blk_elems(h),
                           blk_elems(h), h->bsp, (int)h->bs, h->d_logdet + i0, stride_pL(h), h->N);
        HIPCHK(hipGetLastError());
    }
    if (pack) {
        if (h->B > 1024) return bad_shape("batch too large for the transport tag");
        hipLaunchKernelGGL(pack_tag_write, dim3(1), dim3((unsigned)h->B), 0, st, buf + xe + ce, seg, (double)h->xsplit);
        HIPCHK(hipGetLastError());
        HIPCHK(hipMemcpy2DAsync(buf + xe + ce + 2, seg * sizeof(double), h->d_logdet + i0, h->N * sizeof(double),
                                (i1 - i0) * sizeof(double), (size_t)h->B, hipMemcpyDeviceToDevice, st));
    } else {
        hipLaunchKernelGGL(pack_tag_read, dim3(1), dim3(1), 0, st, buf + xe + ce, seg, (int)h->B, h->d_info + 2);
        HIPCHK(hipGetLastError());
        HIPCHK(hipMemcpy2DAsync(h->d_logdet + i0, h->N * sizeof(double), buf + xe + ce + 2, seg * sizeof(double),
                                (i1 - i0) * sizeof(double), (size_t)h->B, hipMemcpyDeviceToDevice, st));
        if (h->got_block.size() != (size_t)h->N) h->got_block.assign((size_t)h->N, 0);
        for (int64_t i = i0; i < i1; ++i) h->got_block[(size_t)i] = 1;
    }
    return GMRF_OK;
}

gmrf_status gmrf_bt_pack_blocks_async(gmrf_handle* h, int64_t i0, int64_t i1, double* dev_buf) {
    GCHK(tw_refuse(h, "gmrf_bt_pack_blocks_async"));
    if (!h) return bad_shape("null handle");
    HIPCHK(hipSetDevice(h->device));
    return pack_blocks_on(h, h->stream, i0, i1, dev_buf, true);
}

gmrf_status gmrf_bt_unpack_blocks_async(gmrf_handle* h, int64_t i0, int64_t i1, const double* dev_buf) {
    GCHK(tw_refuse(h, "gmrf_bt_unpack_blocks_async"));
    if (!h) return bad_shape("null handle");
    HIPCHK(hipSetDevice(h->device));
    return pack_blocks_on(h, h->stream, i0, i1, const_cast<double*>(dev_buf), false);
}

gmrf_status gmrf_bt_get_block(gmrf_handle* h, int32_t kind, int64_t i, double* out, int64_t ld) {
    h = tw_route(h);
    if (!h || !out) return bad_shape("null pointer");
    if (!h->factored) { g_last_error = "no factor"; return GMRF_ERR_NO_FACTOR; }
    HIPCHK(hipSetDevice(h->device));
    if (tw_on(h)) return tw_get_block(h, kind, i, out, ld);
    const int64_t bs = h->bs, bsp = h->bsp;
    if (ld < bs) return bad_shape("ld < block_size");
    // source window [rows][cols] with row stride lds, placed at (0, c0) of the logical block
    const double* src;
    int64_t rows = bsp, cols = bsp, lds = bsp, c0 = 0;
    if (kind == GMRF_BLOCK_L) {
        if (i < 0 || i >= h->N) return bad_shape("block index");
        if (!h->l_valid) { g_last_error = "the L blocks of this factor are not resident (gmrf_bt_set_keep_l(h, 0), or a factor adopted without them)"; return GMRF_ERR_NO_FACTOR; }
        src = h->d_L + h->sel * stride_pL(h) + i * blk_elems(h);
    } else if (kind == GMRF_BLOCK_LINV) {
        if (i < 0 || i >= h->N) return bad_shape("block index");
        GCHK(ensure_full_inverse(h));
        src = h->d_Linv + h->sel * stride_pX(h) + i * blk_elems(h);
    } else if (kind == GMRF_BLOCK_C) {
        if (i < 0 || i >= h->N - 1) return bad_shape("block index");
        src = h->d_C + h->sel * stride_pC(h) + i * c_blk(h);
        rows = h->rmax; cols = c_ld(h); lds = cols; c0 = h->cmin;
    } else return bad_shape("bad block kind");
    std::vector<double> tmp((size_t)rows * cols);
    HIPCHK(hipMemcpyAsync(tmp.data(), src, tmp.size() * sizeof(double), hipMemcpyDeviceToHost, h->stream));
    HIPCHK(hipStreamSynchronize(h->stream));
    const bool dev_out = is_device_ptr(out);
    std::vector<double> cm;
    double* dst = out;
    int64_t ldd = ld;
    if (dev_out) { cm.resize((size_t)bs * bs); dst = cm.data(); ldd = bs; }
    for (int64_t c = 0; c < bs; ++c)
        for (int64_t r = 0; r < bs; ++r) {                 // row-major window -> column-major block
            const bool in = r < rows && c >= c0 && c - c0 < cols;
            dst[c * ldd + r] = in ? tmp[(size_t)r * lds + (c - c0)] : 0.0;
        }
    if (dev_out) {
        HIPCHK(hipMemcpy2DAsync(out, ld * sizeof(double), cm.data(), bs * sizeof(double), bs * sizeof(double), bs, hipMemcpyHostToDevice, h->stream));
        HIPCHK(hipStreamSynchronize(h->stream));
    }
    return GMRF_OK;
}

// Flat image of one problem's factor: int64 header[8] = {magic, version, n, N, bs, 1, 0, 0}, then
// column-major bs x bs blocks: L_1..L_N, C_1..C_{N-1}, Linv_1..Linv_N  (SURVEY 8b export/import).
static const int64_t EXPORT_MAGIC = 0x46524d47;   // "GMRF"

gmrf_status gmrf_bt_export_size(gmrf_handle* h, int64_t* bytes) {
    GCHK(tw_refuse(h, "gmrf_bt_export_size"));
    if (!h || !bytes) return bad_shape("null pointer");
    if (h->N <= 0) { g_last_error = "no shape"; return GMRF_ERR_NO_FACTOR; }
    *bytes = 64 + (int64_t)sizeof(double) * h->bs * h->bs * (3 * h->N - 1);
    return GMRF_OK;
}

gmrf_status gmrf_bt_export_factor(gmrf_handle* h, void* buf, int64_t bytes) {
    GCHK(tw_refuse(h, "gmrf_bt_export_factor"));
    if (!h || !buf) return bad_shape("null pointer");
    if (!h->factored) { g_last_error = "no factor"; return GMRF_ERR_NO_FACTOR; }
    if (is_device_ptr(buf)) return bad_shape("export buffer must be host memory");
    int64_t need = 0;
    GCHK(gmrf_bt_export_size(h, &need));
    if (bytes < need) return bad_shape("export buffer too small");
    int64_t* hdr = (int64_t*)buf;
    hdr[0] = EXPORT_MAGIC; hdr[1] = 1; hdr[2] = h->n; hdr[3] = h->N; hdr[4] = h->bs; hdr[5] = 1; hdr[6] = hdr[7] = 0;
    double* out = (double*)((char*)buf + 64);
    const int64_t be = h->bs * h->bs;
    for (int64_t i = 0; i < h->N; ++i) GCHK(gmrf_bt_get_block(h, GMRF_BLOCK_L, i, out + i * be, h->bs));
    out += h->N * be;
    for (int64_t i = 0; i + 1 < h->N; ++i) GCHK(gmrf_bt_get_block(h, GMRF_BLOCK_C, i, out + i * be, h->bs));
    out += (h->N - 1) * be;
    for (int64_t i = 0; i < h->N; ++i) GCHK(gmrf_bt_get_block(h, GMRF_BLOCK_LINV, i, out + i * be, h->bs));
    return GMRF_OK;
}

gmrf_status gmrf_bt_import_factor(gmrf_handle* h, const void* buf, int64_t bytes) {
    GCHK(tw_refuse(h, "gmrf_bt_import_factor"));
    if (!h || !buf) return bad_shape("null pointer");
    if (is_device_ptr(buf)) return bad_shape("import buffer must be host memory");
    if (bytes < 64) return bad_shape("import buffer too small");
    const int64_t* hdr = (const int64_t*)buf;
    if (hdr[0] != EXPORT_MAGIC || hdr[1] != 1 || hdr[5] != 1) return bad_shape("not a factor image");
    const int64_t n = hdr[2], N = hdr[3], bs = hdr[4];
    if (N <= 0 || bs <= 0 || n != N * bs) return bad_shape("bad shape in factor image");
    if (bytes < 64 + (int64_t)sizeof(double) * bs * bs * (3 * N - 1)) return bad_shape("factor image truncated");
    HIPCHK(hipSetDevice(h->device));
    if (!h->keep_l) return bad_shape("import needs the L blocks kept (gmrf_bt_set_keep_l(h, 1))");
    if ((h->n != n || h->N != N) && h->B != 1) return bad_shape("a batched handle imports into an existing shape only");
    // The image holds dense blocks and says nothing about the coupling blocks' zero structure: the handle
    // takes the dense layout (a pattern analysed earlier no longer describes the factor) and every
    // problem's stored C window is re-laid out accordingly.
    const bool relayout = (h->n != n || h->N != N || h->cmin != 0 || h->rmax != 64 * next_pow2((bs + 63) / 64) || !h->d_Linv);
    if (relayout && h->B != 1 && h->factored) return bad_shape("a batched handle imports only into a dense-layout factor");
    GCHK(set_shape(h, n, N));
    h->analyzed = false;
    if (relayout) {
        GCHK(set_layout_dense(h));
        GCHK(alloc_factor(h));
        if (h->c_dirty) {
            HIPCHK(hipMemsetAsync(h->d_C, 0, sizeof(double) * stride_pC(h) * h->B, h->stream));
            h->c_dirty = false;
        }
    } else {
        std::vector<int64_t> z((size_t)(h->bsp / 64), 0);
        bool dense_ks = true;
        for (int v : h->kst) if (v != 0) dense_ks = false;
        if (!dense_ks) GCHK(set_layout(h, 0, h->bsp, z));      // same window, staircase dropped
        h->c_dirty = false;
    }
    const int64_t bsp = h->bsp, be = bs * bs;
    std::vector<double> tmp((size_t)bsp * bsp);
    auto put = [&](const double* src, double* dst, bool unit_pad) -> gmrf_status {
        std::fill(tmp.begin(), tmp.end(), 0.0);
        for (int64_t r = 0; r < bs; ++r)
            for (int64_t c = 0; c < bs; ++c) tmp[(size_t)r * bsp + c] = src[c * bs + r];   // column-major -> row-major
        if (unit_pad)
            for (int64_t r = bs; r < bsp; ++r) tmp[(size_t)r * bsp + r] = 1.0;
        HIPCHK(hipMemcpyAsync(dst, tmp.data(), tmp.size() * sizeof(double), hipMemcpyHostToDevice, h->stream));
        HIPCHK(hipStreamSynchronize(h->stream));
        return GMRF_OK;
    };
    const double* in = (const double*)((const char*)buf + 64);
    for (int64_t i = 0; i < N; ++i) GCHK(put(in + i * be, h->d_L + h->sel * stride_pL(h) + i * blk_elems(h), true));
    in += N * be;
    for (int64_t i = 0; i + 1 < N; ++i) GCHK(put(in + i * be, h->d_C + h->sel * stride_pC(h) + i * c_blk(h), false));
    in += (N - 1) * be;
    for (int64_t i = 0; i < N; ++i) GCHK(put(in + i * be, h->d_Linv + h->sel * stride_pX(h) + i * blk_elems(h), true));
    h->factored = true; h->fy_for = nullptr; h->l_valid = true;
    persist_plan(h);
    h->xsplit = 0;                                     // the image holds the full inverses
    return GMRF_OK;
}

// ------------------------------------------------------------------------------------ RCCL (xGMI)
// One communicator per process and GPU.  librccl is opened at run time (dlopen) the first time a
// communicator is asked for: a host that never shares a factor never loads it, and inside a PyTorch
// process the copy PyTorch already mapped is the one that gets used (two RCCL images in one process
// would both export the nccl* symbols).
struct NcclUid { char b[128]; };
struct RcclApi {
    void* lib = nullptr;
    int (*GetUniqueId)(NcclUid*) = nullptr;
    int (*CommInitRank)(void**, int, NcclUid, int) = nullptr;
    int (*CommDestroy)(void*) = nullptr;
    int (*Broadcast)(const void*, void*, size_t, int, int, void*, hipStream_t) = nullptr;
    int (*AllReduce)(const void*, void*, size_t, int, int, void*, hipStream_t) = nullptr;
    int (*AllGather)(const void*, void*, size_t, int, void*, hipStream_t) = nullptr;
    int (*GroupStart)() = nullptr;
    int (*GroupEnd)() = nullptr;
    const char* (*GetErrorString)(int) = nullptr;
};
static RcclApi g_rccl;
static std::mutex g_rccl_mu;

static gmrf_status rccl_load() {
    std::lock_guard<std::mutex> lock(g_rccl_mu);
    if (g_rccl.lib) return GMRF_OK;
    const char* env = getenv("GMRF_RCCL_PATH");
    const char* names[] = {env, "librccl.so.1", "librccl.so", "/opt/rocm/lib/librccl.so.1", "/opt/rocm/lib/librccl.so"};
    void* lib = nullptr;
    for (int pass = 0; pass < 2 && !lib; ++pass)          // pass 0: an image that is already mapped (PyTorch's)
        for (const char* nm : names) {
            if (!nm) continue;
            lib = dlopen(nm, RTLD_NOW | RTLD_LOCAL | (pass == 0 ? RTLD_NOLOAD : 0));
            if (lib) break;
        }
    if (!lib) { g_last_error = std::string("librccl not found (set GMRF_RCCL_PATH): ") + (dlerror() ? dlerror() : ""); return GMRF_ERR_RCCL; }
#define GMRF_RCCL_SYM(field, name)                                                           \
    g_rccl.field = reinterpret_cast<decltype(g_rccl.field)>(dlsym(lib, name));               \
    if (!g_rccl.field) { g_last_error = std::string("librccl lacks ") + name; return GMRF_ERR_RCCL; }
    GMRF_RCCL_SYM(GetUniqueId, "ncclGetUniqueId") GMRF_RCCL_SYM(CommInitRank, "ncclCommInitRank")
    GMRF_RCCL_SYM(CommDestroy, "ncclCommDestroy") GMRF_RCCL_SYM(Broadcast, "ncclBroadcast")
    GMRF_RCCL_SYM(AllReduce, "ncclAllReduce") GMRF_RCCL_SYM(AllGather, "ncclAllGather") GMRF_RCCL_SYM(GroupStart, "ncclGroupStart")
    GMRF_RCCL_SYM(GroupEnd, "ncclGroupEnd") GMRF_RCCL_SYM(GetErrorString, "ncclGetErrorString")
#undef GMRF_RCCL_SYM
    g_rccl.lib = lib;
    return GMRF_OK;
}

#define NCCLCHK(expr)                                                                       \
    do {                                                                                    \
        int _r = (expr);                                                                    \
        if (_r != 0) {                                                                      \
            g_last_error = std::string(#expr) + ": " + g_rccl.GetErrorString(_r);           \
            return GMRF_ERR_RCCL;                                                           \
        }                                                                                   \
    } while (0)

struct gmrf_comm {
    int device = 0, rank = 0, world = 1;
    void* comm = nullptr;
    hipStream_t stream = nullptr;          // collectives run here, beside the handle's compute stream
    hipEvent_t ev_in = nullptr, ev_out = nullptr;
    DevBuf small;                          // staging of small host records (layout, scalars)
    DevBuf pack;                           // staging of the packed transport image of a block range
    double bytes_moved = 0.0;              // factor bytes broadcast so far (gmrf_comm_bytes)
};

gmrf_status gmrf_comm_unique_id(void* id128) {
    if (!id128) return bad_shape("null pointer");
    GCHK(rccl_load());
    NcclUid u;
    NCCLCHK(g_rccl.GetUniqueId(&u));
    memcpy(id128, u.b, 128);
    return GMRF_OK;
}

gmrf_status gmrf_comm_create(int32_t device, int32_t rank, int32_t world, const void* id128, gmrf_comm** out) {
    if (!out || !id128 || world < 1 || rank < 0 || rank >= world) return bad_shape("bad communicator arguments");
    int count = 0;
    if (hipGetDeviceCount(&count) != hipSuccess || count <= 0 || device < 0 || device >= count) {
        (void)hipGetLastError();
        g_last_error = "no HIP device visible";
        return GMRF_ERR_NO_DEVICE;
    }
    GCHK(rccl_load());
    HIPCHK(hipSetDevice(device));
    std::unique_ptr<gmrf_comm, gmrf_status (*)(gmrf_comm*)> guard(new gmrf_comm(), gmrf_comm_destroy);
    gmrf_comm* c = guard.get();
    c->device = device; c->rank = rank; c->world = world;
    NcclUid u;
    memcpy(u.b, id128, 128);
    int r = g_rccl.CommInitRank(&c->comm, world, u, rank);
    if (r != 0) { g_last_error = std::string("ncclCommInitRank: ") + g_rccl.GetErrorString(r); return GMRF_ERR_RCCL; }
    HIPCHK(hipStreamCreateWithFlags(&c->stream, hipStreamNonBlocking));
    HIPCHK(hipEventCreateWithFlags(&c->ev_in, hipEventDisableTiming));
    HIPCHK(hipEventCreateWithFlags(&c->ev_out, hipEventDisableTiming));
    *out = guard.release();
    return GMRF_OK;
}

gmrf_status gmrf_comm_destroy(gmrf_comm* c) {
    if (!c) return GMRF_OK;
    (void)hipSetDevice(c->device);
    if (c->stream) (void)hipStreamSynchronize(c->stream);
    if (c->comm) (void)g_rccl.CommDestroy(c->comm);
    if (c->ev_in) (void)hipEventDestroy(c->ev_in);
    if (c->ev_out) (void)hipEventDestroy(c->ev_out);
    if (c->stream) (void)hipStreamDestroy(c->stream);
    delete c;
    return GMRF_OK;
}

// Broadcast a small HOST record (layout, log-determinants ...) from `root`; synchronous.
gmrf_status gmrf_comm_bcast_host(gmrf_comm* c, void* host_buf, int64_t bytes, int32_t root) {
    if (!c || !host_buf || bytes <= 0 || root < 0 || root >= c->world) return bad_shape("bad broadcast arguments");
    HIPCHK(hipSetDevice(c->device));
    GCHK(c->small.reserve(c->stream, (size_t)bytes));
    if (c->rank == root) HIPCHK(hipMemcpyAsync(c->small.p, host_buf, (size_t)bytes, hipMemcpyHostToDevice, c->stream));
    NCCLCHK(g_rccl.Broadcast(c->small.p, c->small.p, (size_t)bytes, /*ncclInt8*/ 0, root, c->comm, c->stream));
    if (c->rank != root) HIPCHK(hipMemcpyAsync(host_buf, c->small.p, (size_t)bytes, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(hipStreamSynchronize(c->stream));
    return GMRF_OK;
}

// R2 of SURVEY 8e: sum of the ranks' variance accumulators (device buffer of `count` doubles), in place.
// `stream_of`: a handle whose stream produced the buffer and consumes the result (may be NULL: synchronous).
gmrf_status gmrf_comm_allreduce_sum(gmrf_comm* c, gmrf_handle* stream_of, double* dev_buf, int64_t count) {
    if (!c || !dev_buf || count <= 0) return bad_shape("bad all-reduce arguments");
    if (!is_device_ptr(dev_buf)) return bad_shape("all-reduce needs a device buffer");
    HIPCHK(hipSetDevice(c->device));
    if (stream_of) {
        HIPCHK(hipEventRecord(c->ev_in, stream_of->stream));
        HIPCHK(hipStreamWaitEvent(c->stream, c->ev_in, 0));
    }
    NCCLCHK(g_rccl.AllReduce(dev_buf, dev_buf, (size_t)count, /*ncclFloat64*/ 8, /*ncclSum*/ 0, c->comm, c->stream));
    if (stream_of) {
        HIPCHK(hipEventRecord(c->ev_out, c->stream));
        HIPCHK(hipStreamWaitEvent(stream_of->stream, c->ev_out, 0));
    } else {
        HIPCHK(hipStreamSynchronize(c->stream));
    }
    return GMRF_OK;
}

// R1 of SURVEY 8e: broadcast of the factor blocks [i0, i1) of every problem of the batch from `root` to all ranks
// as ONE packed transport image (pack_blocks_on: lower-triangular tiles of Linv_i, the stored windows of the coupling
// blocks C_{i0-1} .. C_{i1-2}, the blocks' log-determinant parts): the root packs into the communicator's staging
// buffer, one ncclBroadcast moves it, the receivers unpack into their factor storage -- all three on the
// communicator's stream, behind whatever the handle's stream holds at the time of the call (root: the factorisation
// of these blocks; receivers: the sweeps of the previous job that still read the buffers).  The root goes on
// factoring the next range meanwhile.  with_l != 0: the raw L_i blocks follow (full squares).
gmrf_status gmrf_bt_bcast_blocks_async(gmrf_handle* h, gmrf_comm* c, int32_t root, int64_t i0, int64_t i1, int32_t with_l) {
    GCHK(tw_refuse(h, "gmrf_bt_bcast_blocks_async"));
    if (!h || !c) return bad_shape("null pointer");
    if (!h->d_Linv || h->N <= 0) { g_last_error = "no factor storage"; return GMRF_ERR_NO_FACTOR; }
    if (i0 < 0 || i1 > h->N || i0 >= i1 || root < 0 || root >= c->world) return bad_shape("bad block range / root");
    if (with_l && !h->keep_l) return bad_shape("the L blocks are not kept on this handle");
    if (c->device != h->device) return bad_shape("communicator and handle live on different devices");
    HIPCHK(hipSetDevice(h->device));
    int64_t seg = 0;
    GCHK(gmrf_bt_packed_size(h, i0, i1, &seg));
    const size_t need = (size_t)seg * (size_t)h->B * sizeof(double);
    GCHK(c->pack.reserve(c->stream, need));
    double* d_pack = c->pack.as<double>();
    HIPCHK(hipEventRecord(c->ev_in, h->stream));
    HIPCHK(hipStreamWaitEvent(c->stream, c->ev_in, 0));
    if (c->rank == root) GCHK(pack_blocks_on(h, c->stream, i0, i1, d_pack, true));
    NCCLCHK(g_rccl.Broadcast(d_pack, d_pack, (size_t)seg * (size_t)h->B, /*ncclFloat64*/ 8, root, c->comm, c->stream));
    c->bytes_moved += (double)need;
    if (c->rank != root) GCHK(pack_blocks_on(h, c->stream, i0, i1, d_pack, false));
    if (with_l) {
        int64_t first = 0, cnt = 0, pstride = 0;
        GCHK(gmrf_bt_block_range(h, GMRF_BLOCK_L, i0, i1, &first, &cnt, &pstride));
        NCCLCHK(g_rccl.GroupStart());
        int rc = 0;
        for (int64_t p = 0; p < h->B && rc == 0; ++p) {
            double* ptr = h->d_L + p * pstride + first;
            rc = g_rccl.Broadcast(ptr, ptr, (size_t)cnt, /*ncclFloat64*/ 8, root, c->comm, c->stream);
        }
        const int rg = g_rccl.GroupEnd();                  // the group is closed on the error path too
        if (rc != 0 || rg != 0) { g_last_error = std::string("ncclBroadcast: ") + g_rccl.GetErrorString(rc ? rc : rg); return GMRF_ERR_RCCL; }
        c->bytes_moved += (double)cnt * (double)h->B * sizeof(double);
    }
    return GMRF_OK;
}

// The other way to share a batch of factors (round 4): EVERY rank factors its own share of the batch -- `src`, src->B
// posteriors -- and the packed images of the blocks [i0, i1) are all-gathered into `dst`, a handle of the same shape and layout
// with a batch of world * src->B: problem r * src->B + p of dst is problem p of rank r.  Against the root broadcast every link
// of the fabric carries a share of the traffic (per rank (world - 1) / world of the batch comes in over all its links, instead of
// the whole batch leaving the root over each of ITS links) and the factorisation itself is spread over the ranks.
// Enqueued on the communicator's stream behind src's stream; gmrf_comm_wait(dst, c) orders dst's stream behind the unpack.
gmrf_status gmrf_bt_allgather_blocks_async(gmrf_handle* src, gmrf_handle* dst, gmrf_comm* c, int64_t i0, int64_t i1) {
    GCHK(tw_refuse(src, "gmrf_bt_allgather_blocks_async"));
    GCHK(tw_refuse(dst, "gmrf_bt_allgather_blocks_async"));
    if (!src || !dst || !c) return bad_shape("null pointer");
    if (!src->d_Linv || !dst->d_Linv || src->N <= 0) { g_last_error = "no factor storage"; return GMRF_ERR_NO_FACTOR; }
    if (src->n != dst->n || src->N != dst->N || src->bsp != dst->bsp || src->cmin != dst->cmin || src->rmax != dst->rmax || src->kst != dst->kst)
        return bad_shape("the two handles differ in shape or coupling-block layout (gmrf_bt_adopt_layout the gathering handle with the factoring handle's record)");
    if (dst->B != src->B * (int64_t)c->world) return bad_shape("the gathering handle's batch must be world x the factoring handle's");
    if (i0 < 0 || i1 > src->N || i0 >= i1) return bad_shape("bad block range");
    if (c->device != src->device || c->device != dst->device) return bad_shape("communicator and handles live on different devices");
    HIPCHK(hipSetDevice(src->device));
    int64_t seg = 0;
    GCHK(gmrf_bt_packed_size(src, i0, i1, &seg));
    const size_t own = (size_t)seg * (size_t)src->B, all = own * (size_t)c->world;
    const size_t need = (own + all) * sizeof(double);          // [own image | gathered images]
    GCHK(c->pack.reserve(c->stream, need));
    double* d_pack = c->pack.as<double>();
    HIPCHK(hipEventRecord(c->ev_in, src->stream));
    HIPCHK(hipStreamWaitEvent(c->stream, c->ev_in, 0));
    HIPCHK(hipEventRecord(c->ev_in, dst->stream));            // dst's earlier sweeps still read the blocks the unpack overwrites
    HIPCHK(hipStreamWaitEvent(c->stream, c->ev_in, 0));
    GCHK(pack_blocks_on(src, c->stream, i0, i1, d_pack, true));
    NCCLCHK(g_rccl.AllGather(d_pack, d_pack + own, own, /*ncclFloat64*/ 8, c->comm, c->stream));
    c->bytes_moved += (double)(all - own) * sizeof(double);    // what came in over this rank's links
    GCHK(pack_blocks_on(dst, c->stream, i0, i1, d_pack + own, false));
    return GMRF_OK;
}

// Bytes this communicator has broadcast so far (factor transport; reset = 1 clears the counter).
gmrf_status gmrf_comm_bytes(gmrf_comm* c, int32_t reset, double* bytes) {
    if (!c || !bytes) return bad_shape("null pointer");
    *bytes = c->bytes_moved;
    if (reset) c->bytes_moved = 0.0;
    return GMRF_OK;
}

// The handle's stream waits for every transfer enqueued so far on the communicator's stream.
gmrf_status gmrf_comm_wait(gmrf_handle* h, gmrf_comm* c) {
    if (!h || !c) return bad_shape("null pointer");
    HIPCHK(hipSetDevice(h->device));
    HIPCHK(hipEventRecord(c->ev_out, c->stream));
    HIPCHK(hipStreamWaitEvent(h->stream, c->ev_out, 0));
    return GMRF_OK;
}

gmrf_status gmrf_bt_solve(gmrf_handle* h, const double* b, double* y, int64_t k, int64_t ldb, int64_t ldy, int32_t mode) {
    h = tw_route(h);
    if (!h || !b || !y) return bad_shape("null pointer");
    if (!h->factored) { g_last_error = "solve before factor"; return GMRF_ERR_NO_FACTOR; }
    if (k <= 0 || ldb < h->n || ldy < h->n || mode < 0 || mode > 2) return bad_shape("bad k / ldb / ldy / mode");
    if (b == y && ldb != ldy) return bad_shape("in place (y == b) needs ldb == ldy");
    HIPCHK(hipSetDevice(h->device));
    if (tw_on(h)) return tw_solve(h, b, y, k, ldb, ldy, mode);
    if (h->B > 1 && k > KP_CHUNK) return bad_shape("with a batch of problems k is limited to 128 per call");
    const bool b_dev = is_device_ptr(b), y_dev = is_device_ptr(y);
    const int64_t nb = h->B;            // b / y hold nb consecutive groups of k columns (problem-major)
    // b and y overlap (in place, or y a column further on): a persistent sweep that gave up could not be repeated from b
    return sweep_guarded(h, {{b, cols_bytes(h->n, k * nb, ldb), y, cols_bytes(h->n, k * nb, ldy)}}, [&]() -> gmrf_status {
        h->stats.solve_ms = 0.0;
        for (int64_t c0 = 0; c0 < k; c0 += KP_CHUNK) {
            const int kc = (int)std::min<int64_t>(KP_CHUNK, k - c0);
            const int kp = pad_k(kc);
            GCHK(ensure_panels(h, kp));
            const double* d_b = nullptr;
            int64_t ld_b = 0;
            GCHK(cols_in(h, b + c0 * ldb, ldb, b_dev, kc, &d_b, &ld_b));
            GCHK(launch_pack(h, d_b, ld_b, kc, kp));
            HIPCHK(hipEventRecord(h->ev0, h->stream));
            GCHK(run_sweeps(h, mode, kp));
            HIPCHK(hipEventRecord(h->ev1, h->stream));
            GCHK(cols_out(h, (mode == GMRF_SOLVE_FULL) ? h->d_P : h->d_Y, kc, nullptr, y + c0 * ldy, ldy, y_dev));
            HIPCHK(hipStreamSynchronize(h->stream));
            float ms = 0.f;
            (void)hipEventElapsedTime(&ms, h->ev0, h->ev1);
            h->stats.solve_ms += ms;
            const int nsweeps = (mode == GMRF_SOLVE_FULL) ? 2 : 1;
            h->stats.sweep_ms = ms / nsweeps;
            h->stats.sweep_bytes = sweep_bytes(h, kc) * (double)nb;
            h->stats.sweep_bytes_streamed = (8.0 * ((double)h->N * 0.5 * (double)h->bsp * (double)(h->bsp + 1) +
                                                    (double)(h->N - 1) * h->c_streamed) + 16.0 * (double)h->n_pad * kc) * (double)nb;
            if (h->profiling) prof_collect(h);
        }
        return GMRF_OK;
    });
}

// draws (or loads) z for samples [first_id + c0, +kc) into panel P and runs the backward sweep -> panel Y
static gmrf_status sample_chunk(gmrf_handle* h, uint64_t seed, int64_t first_id, int kc, const double* z,
                                int64_t ldz, int64_t id_stride) {
    const int kp = pad_k(kc);
    GCHK(ensure_panels(h, kp));
    if (z) {
        const double* d_z = nullptr;
        int64_t ldd = 0;
        GCHK(cols_in(h, z, ldz, is_device_ptr(z), kc, &d_z, &ldd));
        GCHK(launch_pack(h, d_z, ldd, kc, kp));
    } else {
        const int64_t total = (int64_t)kp * h->n_pad;
        hipLaunchKernelGGL(fill_normals_panel, dim3((unsigned)((total + 255) / 256), (unsigned)h->B), dim3(256), 0,
                           h->stream, h->d_P, h->n_pad, (int)h->bs, (int)h->bsp, kc, kp, seed, first_id, id_stride, nullptr, (int64_t)0);
        HIPCHK(hipGetLastError());
    }
    return run_sweeps(h, GMRF_SOLVE_BACKWARD, kp);
}

gmrf_status gmrf_bt_sample(gmrf_handle* h, uint64_t seed, int64_t first_id, int64_t k, const double* mean,
                           const double* z, double* out, int64_t ld) {
    h = tw_route(h);
    if (!h || !out) return bad_shape("null pointer");
    if (!h->factored) { g_last_error = "sample before factor"; return GMRF_ERR_NO_FACTOR; }
    if (k <= 0 || ld < h->n) return bad_shape("bad k / ld");
    if (h->B > 1 && k > KP_CHUNK) return bad_shape("with a batch of problems k is limited to 128 per call");
    HIPCHK(hipSetDevice(h->device));
    if (tw_on(h)) return tw_sample(h, seed, first_id, k, mean, z, out, ld);
    const double* d_mean = nullptr;
    Staging args(h->mean_arena);
    args.in(mean, sizeof(double) * h->n * h->B, &d_mean);
    GCHK(args.commit(h->stream));
    const bool out_dev = is_device_ptr(out);
    // z or the mean overlaps the output: the repeat after a persistent sweep that gave up would read what the first pass wrote
    const int64_t smp_bytes = cols_bytes(h->n, k * h->B, ld);      // z and out alike
    GCHK(sweep_guarded(h, {{z, smp_bytes, out, smp_bytes}, {mean, h->n * h->B * (int64_t)sizeof(double), out, smp_bytes}},
                       [&]() -> gmrf_status {
        HIPCHK(hipEventRecord(h->ev0, h->stream));
        for (int64_t c0 = 0; c0 < k; c0 += KP_CHUNK) {
            const int kc = (int)std::min<int64_t>(KP_CHUNK, k - c0);
            GCHK(sample_chunk(h, seed, first_id + c0, kc, z ? z + c0 * ld : nullptr, ld, k));
            GCHK(cols_out(h, h->d_Y, kc, d_mean, out + c0 * ld, ld, out_dev));
            if (!out_dev) HIPCHK(hipStreamSynchronize(h->stream));
        }
        HIPCHK(hipEventRecord(h->ev1, h->stream));
        HIPCHK(hipStreamSynchronize(h->stream));
        return GMRF_OK;
    }));
    float ms = 0.f;
    (void)hipEventElapsedTime(&ms, h->ev0, h->ev1);
    h->stats.sample_ms = ms;
    if (h->profiling) prof_collect(h);
    return GMRF_OK;
}

// The handle's second stream `aux` on a hardware queue of its own (two streams on one queue serialise: gmrf_streams_create):
// candidates are timed against this handle's stream with the 1 ms spin kernel, the first that overlaps is kept.  Used by
// gmrf_bt_posterior (the samples' sweep beside the mean's) and by a twisted handle (the stream of its bottom half).
static gmrf_status ensure_aux(gmrf_handle* h) {
    if (h->aux_distinct) return GMRF_OK;
    HIPCHK(hipStreamSynchronize(h->stream));
    if (h->aux) { (void)hipStreamSynchronize(h->aux); (void)hipStreamDestroy(h->aux); h->aux = nullptr; }
    const unsigned long long ticks = 100000ull;
    double one = 1e30;
    for (int r = 0; r < 2; ++r) one = std::min(one, spin_pair_ms(h->stream, nullptr, ticks));
    std::vector<hipStream_t> cand;
    for (int c = 0; c < 12 && !h->aux; ++c) {
        hipStream_t st = nullptr;
        HIPCHK(hipStreamCreateWithFlags(&st, hipStreamNonBlocking));
        hipLaunchKernelGGL(gmrf_spin_kernel, dim3(1), dim3(64), 0, st, 1ull);      // (first use binds the stream to its queue)
        (void)hipStreamSynchronize(st);
        const double t = std::min(spin_pair_ms(h->stream, st, ticks), spin_pair_ms(h->stream, st, ticks));
        if (t < 1.5 * one) h->aux = st; else cand.push_back(st);
    }
    if (!h->aux && !cand.empty()) { h->aux = cand.back(); cand.pop_back(); }       // (none overlaps: any will do, serialised)
    for (hipStream_t st : cand) (void)hipStreamDestroy(st);
    if (!h->aux) return bad_shape("internal: no second stream");
    h->aux_distinct = true;
    return GMRF_OK;
}

// The samples' backward sweep of gmrf_bt_posterior beside the mean's two (persistent launches, device pointers, no two of b, mean,
// samples overlapping); ends in the synchronisation of the handle's stream.
static gmrf_status posterior_beside(gmrf_handle* h, const double* b, uint64_t seed, int64_t first_id, int64_t k, double* mean,
                                    double* samples, int64_t ld) {
    const int kp = pad_k(k);
    GCHK(ensure_panels(h, 1));
    GCHK(sweep_persist_prepare(h, 1));
    const size_t elems = (size_t)((int64_t)kp * h->n_pad);
    GCHK(reserve_group(h->stream, {h->d_P2.want(elems), h->d_Y2.want(elems), h->d_T2.want(elems)}));
    GCHK(ensure_aux(h));
    h->fork_next = 0;
    hipEvent_t ev_fork = nullptr, ev_join = nullptr;
    GCHK(fork_event(h, &ev_fork)); GCHK(fork_event(h, &ev_join));
    h->sweep_persist_launched = true;
    h->stats.sweep_persist = 1;
    h->stats.sweep_persist_launches += 3;
    HIPCHK(hipEventRecord(h->ev0, h->stream));
    HIPCHK(hipEventRecord(ev_fork, h->stream));
    HIPCHK(hipStreamWaitEvent(h->aux, ev_fork, 0));
    // second stream: z -> P2, backward sweep P2 -> Y2
    {
        const int64_t total = (int64_t)kp * h->n_pad;
        hipLaunchKernelGGL(fill_normals_panel, dim3((unsigned)((total + 255) / 256), 1), dim3(256), 0, h->aux, h->d_P2, h->n_pad,
                           (int)h->bs, (int)h->bsp, (int)k, kp, seed, first_id, k, nullptr, (int64_t)0);
        HIPCHK(hipGetLastError());
        GCHK(launch_sweep_persist(h, true, kp, h->d_P2, h->d_Y2, h->aux, h->d_T2));
        HIPCHK(hipEventRecord(ev_join, h->aux));
    }
    // this stream: b -> P, forward P -> Y, backward Y -> P, mean out
    GCHK(launch_pack(h, b, h->n, 1, 1));
    GCHK(launch_sweep_persist(h, false, 1, h->d_P, h->d_Y));
    GCHK(launch_sweep_persist(h, true, 1, h->d_Y, h->d_P));
    GCHK(launch_unpack(h, h->d_P, mean, h->n, 1, nullptr));
    HIPCHK(hipStreamWaitEvent(h->stream, ev_join, 0));
    GCHK(launch_unpack(h, h->d_Y2, samples, ld, (int)k, mean));
    HIPCHK(hipEventRecord(h->ev1, h->stream));
    HIPCHK(hipStreamSynchronize(h->stream));
    return GMRF_OK;
}

// A batch's posterior with the mean's backward sweep carried in the samples' (round 6): may it run fused?  Batches only (B > 1),
// k <= 128 with kp = pad_k(k) a multiple of 64 on the GEMM route of the sweeps, device pointers, not switched off (GMRF_SW_TWO_CALL_POSTERIOR),
// and every product of the backward sweep on the 64 x 64 LDS-DMA tile that takes the tail row (a dry run of the sweep asks).
// Needs the panels of kp + 1 rows (ensure_panels).
static bool posterior_fused_ok(gmrf_handle* h, int64_t k, bool dev_all) {
    if (tw_on(h) || h->B <= 1 || !dev_all || h->sw(GMRF_SW_TWO_CALL_POSTERIOR) || h->sw(GMRF_SW_SWEEP_NO_GEMM) || k <= 0 || k > KP_CHUNK) return false;
    const int kp = pad_k(k);
    if (kp % 64 != 0 || (int64_t)h->B * (h->bsp / 64) * (kp / 64) < 128) return false;
    if ((int64_t)(kp + 1) * h->n_pad * 8 >= ((int64_t)1 << 32)) return false;
    if (ensure_panels(h, kp + 1) != GMRF_OK) return false;
    if (!h->d_dout && h->d_dout.reserve(h->stream, 1) != GMRF_OK) { (void)hipGetLastError(); return false; }
    h->tail_probe = true; h->tail_refused = false;
    const gmrf_status st = sweep_launches(h, true, kp, h->d_P, h->d_Y, true, h->d_dout);
    h->tail_probe = false;
    return st == GMRF_OK && !h->tail_refused;
}

// The fused posterior of a batch (posterior_fused_ok): b -> P, forward k = 1 sweep P -> Y (the mean's, as gmrf_bt_solve runs it);
// P <- normals in rows 0 .. kp - 1 and y in row kp; ONE backward sweep P -> Y over kp + 1 rows, the mean's being every product's
// tail row (gemm_f64_dma TAIL): the factor is streamed once for both instead of once each.  Rows 0 .. k - 1 are bitwise the
// samples' sweep of gmrf_bt_sample (same kernel, same sums); the mean is summed by the tail row instead of the k = 1 kernels (rounding
// level).  Out: mean = row kp, samples = rows + mean.  Ends in the synchronisation of the handle's stream.
static gmrf_status posterior_fused(gmrf_handle* h, const double* b, uint64_t seed, int64_t first_id, int64_t k, double* mean,
                                   double* samples, int64_t ld) {
    const int kp = pad_k(k);
    GCHK(ensure_panels(h, kp + 1));
    HIPCHK(hipEventRecord(h->ev0, h->stream));
    // (round 7) the factorisation of b, the registered right-hand side, left y = L^-1 b beside the factor: no forward sweep
    const bool have_y = h->fy_for && b == h->fy_for;
    if (!have_y) {
        GCHK(launch_pack(h, b, h->n, 1, 1));
        GCHK(run_sweeps(h, GMRF_SOLVE_FORWARD, 1));
    }
    {
        const int64_t total = (int64_t)(kp + 1) * h->n_pad;
        hipLaunchKernelGGL(fill_normals_panel, dim3((unsigned)((total + 255) / 256), (unsigned)h->B), dim3(256), 0,
                           h->stream, h->d_P, h->n_pad, (int)h->bs, (int)h->bsp, (int)k, kp, seed, first_id, k,
                           have_y ? h->d_fy : h->d_Y, h->n_pad);
        HIPCHK(hipGetLastError());
    }
    // (round 13) the products that finish x_i write mean and samples themselves: where to is handed over in device memory (the
    // sweep's captured graph holds no pointer of a call), by a one-thread launch in front of the sweep
    hipLaunchKernelGGL(set_direct_out, dim3(1), dim3(1), 0, h->stream, h->d_dout, samples, mean, ld, k);
    HIPCHK(hipGetLastError());
    GCHK(run_sweeps(h, SWEEP_BACKWARD_TAIL, kp));
    HIPCHK(hipEventRecord(h->ev1, h->stream));
    HIPCHK(hipStreamSynchronize(h->stream));
    if (h->profiling) prof_collect(h);
    return GMRF_OK;
}

// mean = A^-1 b and k samples mean + L^-T z in ONE call (scripts/darcy/solve_darcy_gmrf-fem.jl:190-191 calls `mean` and `rand` on one
// factor, one after the other).  The samples' backward sweep needs nothing of the mean -- only their last step, adding it, does --
// so where the sweeps are persistent launches (one problem, blocks of 512 .. 1024) it runs BESIDE the mean's two sweeps, on a second
// stream with panels of its own: both are bound by their chains of hand-offs, not by the chip, and two resident workgroups per
// CU (97 + 189 VGPRs, 13 + 33 KB of LDS) take turns in the same time one takes alone.  The same kernels and the same sums as
// gmrf_bt_solve + gmrf_bt_sample: bitwise their results.  A batch (B > 1) whose samples' sweep runs on the GEMM and whose inputs
// and outputs do not overlap runs posterior_fused: the mean's backward sweep as the tail row of the samples'.  Anywhere else the call
// IS those two calls.
gmrf_status gmrf_bt_posterior(gmrf_handle* h, const double* b, uint64_t seed, int64_t first_id, int64_t k, double* mean,
                              double* samples, int64_t ld) {
    h = tw_route(h);
    if (!h || !b || !mean || !samples) return bad_shape("null pointer");
    if (!h->factored) { g_last_error = "posterior before factor"; return GMRF_ERR_NO_FACTOR; }
    if (k <= 0 || ld < h->n) return bad_shape("bad k / ld");
    HIPCHK(hipSetDevice(h->device));
    const bool dev_all = is_device_ptr(b) && is_device_ptr(mean) && is_device_ptr(samples);
    // beside only when no two of b, mean, samples overlap (else the two calls, each with its own guard)
    const int64_t vec_bytes = h->n * h->B * (int64_t)sizeof(double), smp_bytes = cols_bytes(h->n, k * h->B, ld);
    bool beside = false, fused = false;
    GCHK(sweep_guarded(h, {{b, vec_bytes, mean, vec_bytes}, {b, vec_bytes, samples, smp_bytes}, {mean, vec_bytes, samples, smp_bytes}},
                       [&]() -> gmrf_status {
        // (decided behind the hold, which sweep_persist_ok reads; the repeat after an abort finds the handle off the persistent form)
        beside = !tw_on(h) && h->B == 1 && k <= KP_CHUNK && k >= 2 && dev_all && !h->profiling && sweep_persist_ok(h, 1) &&
                 sweep_persist_ok(h, pad_k(k));      // (a twisted handle: its mean, then its samples)
        if (beside) return posterior_beside(h, b, seed, first_id, k, mean, samples, ld);
        // (the hold also marks inputs that overlap outputs: the fused pass would write the mean before the samples read b's sweep)
        fused = !h->sweep_persist_hold && posterior_fused_ok(h, k, dev_all);
        return fused ? posterior_fused(h, b, seed, first_id, k, mean, samples, ld) : GMRF_OK;
    }, [&]() -> gmrf_status {
        if (h->aux) HIPCHK(hipStreamSynchronize(h->aux));
        return GMRF_OK;
    }));
    if (!beside && !fused) {
        GCHK(gmrf_bt_solve(h, b, mean, 1, h->n, h->n, GMRF_SOLVE_FULL));
        return gmrf_bt_sample(h, seed, first_id, k, mean, nullptr, samples, ld);
    }
    float ms = 0.f;
    (void)hipEventElapsedTime(&ms, h->ev0, h->ev1);
    h->stats.solve_ms = ms;                            // (mean and samples together)
    h->stats.sample_ms = 0.0;
    return GMRF_OK;
}

gmrf_status gmrf_bt_set_factor_rhs(gmrf_handle* h, const double* b) {
    if (!h) return bad_shape("null handle");
    if (b && !is_device_ptr(b)) return bad_shape("the factor's right-hand side must be device memory");
    h->frhs = b;
    h->fy_for = nullptr;
    return GMRF_OK;
}

gmrf_status gmrf_bt_normals(gmrf_handle* h, uint64_t seed, int64_t first_id, int64_t k, double* z, int64_t ld) {
    if (!h || !z) return bad_shape("null pointer");
    if (h->n <= 0) return bad_shape("no shape set");
    if (k <= 0 || ld < h->n) return bad_shape("bad k / ld");
    if (h->B > 1 && k > KP_CHUNK) return bad_shape("with a batch of problems k is limited to 128 per call");
    HIPCHK(hipSetDevice(h->device));
    const bool z_dev = is_device_ptr(z);
    for (int64_t c0 = 0; c0 < k; c0 += KP_CHUNK) {
        const int kc = (int)std::min<int64_t>(KP_CHUNK, k - c0);
        const int kp = pad_k(kc);
        GCHK(ensure_panels(h, kp));
        const int64_t total = (int64_t)kp * h->n_pad;
        hipLaunchKernelGGL(fill_normals_panel, dim3((unsigned)((total + 255) / 256), (unsigned)h->B), dim3(256), 0,
                           h->stream, h->d_P, h->n_pad, (int)h->bs, (int)h->bsp, kc, kp, seed, first_id + c0, k, nullptr, (int64_t)0);
        HIPCHK(hipGetLastError());
        GCHK(cols_out(h, h->d_P, kc, nullptr, z + c0 * ld, ld, z_dev));
        HIPCHK(hipStreamSynchronize(h->stream));
    }
    return GMRF_OK;
}

gmrf_status gmrf_bt_logdet(gmrf_handle* h, double* out) {
    h = tw_route(h);
    if (!h || !out) return bad_shape("null pointer");
    if (!h->factored) { g_last_error = "logdet before factor"; return GMRF_ERR_NO_FACTOR; }
    HIPCHK(hipSetDevice(h->device));
    if (tw_on(h)) return tw_logdet(h, out);
    if (h->keep_l && h->l_valid) {
        hipLaunchKernelGGL(logdet_blocks, dim3((unsigned)h->N, 1), dim3(256), 0, h->stream,
                           h->d_L + h->sel * stride_pL(h), blk_elems(h), h->bsp, (int)h->bs, h->d_logdet + h->sel * h->N,
                           (int64_t)0, (int64_t)0);
        HIPCHK(hipGetLastError());
    } else if (!h->logdet_valid) {
        // (a factor adopted as raw buffers without its L blocks: nothing ever filled d_logdet)
        g_last_error = "neither the L blocks nor the log-determinant parts of this factor are resident (adopted as raw buffers without L)";
        return GMRF_ERR_NO_FACTOR;
    }   // else: the factorisation (or the transport image) left every block's part in d_logdet
    std::vector<double> part((size_t)h->N);
    HIPCHK(hipMemcpyAsync(part.data(), h->d_logdet + h->sel * h->N, sizeof(double) * h->N, hipMemcpyDeviceToHost, h->stream));
    HIPCHK(hipStreamSynchronize(h->stream));
    double s = 0.0;
    for (double v : part) s += v;
    *out = 2.0 * s;
    return GMRF_OK;
}

// logdet of every problem -> d_out[B] (device), enqueued on the handle's stream: the parts as gmrf_bt_logdet takes them (from the
// resident L blocks, else what the factorisation left), then one thread per problem adds them in its order
static gmrf_status logdet_batch_enqueue(gmrf_handle* h, double* d_out) {
    if (h->keep_l && h->l_valid) {
        hipLaunchKernelGGL(logdet_blocks, dim3((unsigned)h->N, (unsigned)h->B), dim3(256), 0, h->stream, h->d_L, blk_elems(h), h->bsp,
                           (int)h->bs, h->d_logdet, stride_pL(h), h->N);
    } else if (!h->logdet_valid) {
        g_last_error = "neither the L blocks nor the log-determinant parts of this factor are resident (adopted as raw buffers without L)";
        return GMRF_ERR_NO_FACTOR;
    }
    hipLaunchKernelGGL(logdet_sum_batch, dim3((unsigned)((h->B + 255) / 256)), dim3(256), 0, h->stream, h->d_logdet, h->N, h->B, d_out);
    HIPCHK(hipGetLastError());
    return GMRF_OK;
}

gmrf_status gmrf_bt_logdet_batch(gmrf_handle* h, double* out) {
    if (!h || !out) return bad_shape("null pointer");
    GCHK(tw_refuse(h, "gmrf_bt_logdet_batch"));
    if (!h->factored) { g_last_error = "logdet before factor"; return GMRF_ERR_NO_FACTOR; }
    HIPCHK(hipSetDevice(h->device));
    double* d_out;
    Staging args(h->mean_arena);
    args.out(out, sizeof(double) * h->B, &d_out);
    GCHK(args.commit(h->stream));
    GCHK(logdet_batch_enqueue(h, d_out));
    GCHK(args.flush(h->stream));
    HIPCHK(hipStreamSynchronize(h->stream));
    return GMRF_OK;
}

// --------------------------------------------------------------------------------- CSR / SpMM
// The routes of Y = S X as values: what the launchers below branch on, and what gmrf_test_spmm_plan / gmrf_test_spmm_route report
// (host only, no device state).

// csr_spmv_tiles can take the matrix: no SPMV_ROWS-row tile has more than SPMV_CAP entries (rp: 0-based row pointers)
static bool spmv_tiles_ok(int64_t n_rows, const int64_t* rp) {
    for (int64_t r = 0; r < n_rows; r += SPMV_ROWS)
        if (rp[std::min(n_rows, r + SPMV_ROWS)] - rp[r] > SPMV_CAP) return false;
    return true;
}

// Column-major operands: 0 = csr_spmv_tiles (one right-hand side, tiles_ok), else the lane group G of csr_spmm<VT, G>, by entries per row
static int spmm_cols_route(int64_t nnz, int64_t n_rows, int k, bool tiles_ok) {
    if (k == 1 && tiles_ok) return 0;
    const double avg = (double)nnz / (double)n_rows;
    return avg > 40 ? 64 : avg > 20 ? 32 : avg > 10 ? 16 : 8;
}

// Tile plan of csr_spmm_tiles: per R-row tile the ascending list of distinct columns and, per entry, the 16-bit index of its
// column in that list; the LDS capacities of the two tiled kernels.
struct SpmmPlan {
    int state = -1;                    // 1: usable, -1: no tile height fits the LDS image
    int R = 0, ucap = 0, ecap = 0;     // rows per tile; distinct columns (rounded to 32) and entries (rounded to 256) of the largest tile
    int ecap_pad = 0;                  // entries of the largest tile with rows padded to 8, rounded to 64; 0: the padded image does not fit
    int umax = 0;                      // most distinct columns of a tile
    std::vector<int64_t> tile_uptr;    // [tiles + 1] ranges into ucols
    std::vector<int32_t> ucols;
    std::vector<uint16_t> lidx;        // [nnz]
};

static void spmm_plan_host(int64_t n_rows, const int64_t* rp, const int32_t* ci, SpmmPlan& pl) {
    const int64_t nnz = rp[n_rows];
    std::vector<int64_t>& uptr = pl.tile_uptr;
    std::vector<int32_t>& ucols = pl.ucols;
    std::vector<uint16_t>& lidx = pl.lidx;
    lidx.assign((size_t)std::max<int64_t>(nnz, 1), 0);
    std::vector<int32_t> tmp;
    // the tallest tile whose LDS image (distinct rows of X for 16 right-hand sides + the entries) lets three
    // workgroups share a CU; a matrix whose 16-row tiles do not fit keeps the plain kernel
    constexpr size_t lds_budget = 52 * 1024;
    pl.state = -1;
    for (int R : {64, 32, 16}) {
        const int64_t T = (n_rows + R - 1) / R;
        uptr.assign((size_t)T + 1, 0);
        ucols.clear();
        ucols.reserve((size_t)(nnz / 3 + 16));
        int64_t umax = 0, emax = 0, pmax = 0;
        bool ok = true;
        for (int64_t tix = 0; tix < T && ok; ++tix) {
            const int64_t r0 = tix * R, r1 = std::min(n_rows, r0 + R);
            const int64_t a = rp[r0], b = rp[r1];
            tmp.assign(ci + a, ci + b);
            std::sort(tmp.begin(), tmp.end());
            tmp.erase(std::unique(tmp.begin(), tmp.end()), tmp.end());
            umax = std::max<int64_t>(umax, (int64_t)tmp.size()); emax = std::max(emax, b - a);
            int64_t padded = 0;                                  // rows padded to multiples of 8 entries (csr_spmm_tiles_pad)
            for (int64_t r = r0; r < r1; ++r) padded += (rp[r + 1] - rp[r] + 7) / 8 * 8;
            pmax = std::max(pmax, padded);
            if ((int64_t)tmp.size() > 32 * SPMM_NG || b - a > 8192) { ok = false; break; }
            for (int64_t e = a; e < b; ++e)
                lidx[(size_t)e] = (uint16_t)(std::lower_bound(tmp.begin(), tmp.end(), ci[e]) - tmp.begin());
            ucols.insert(ucols.end(), tmp.begin(), tmp.end());
            uptr[(size_t)tix + 1] = (int64_t)ucols.size();
        }
        if (!ok) continue;
        const int ucap = (int)std::max<int64_t>(32, (umax + 31) / 32 * 32), ecap = (int)std::max<int64_t>(256, (emax + 255) / 256 * 256);
        if (spmm_tile_lds_bytes(R, ucap, ecap) > lds_budget) continue;
        pl.R = R; pl.ucap = ucap; pl.ecap = ecap; pl.umax = (int)umax;
        // (the padded kernel sizes its LDS image by the distinct columns rounded to 8, the entries to 64: 39.3 KB on the
        //  burgers4096x512 matrix -- four workgroups per CU)
        const int ecap_pad64 = (int)std::max<int64_t>(64, (pmax + 63) / 64 * 64);
        pl.ecap_pad = (spmm_tile_pad_lds_bytes(R, (int)((umax + 7) / 8 * 8), ecap_pad64) <= lds_budget + 1024) ? ecap_pad64 : 0;
        pl.state = 1;
        return;
    }
    uptr.clear(); ucols.clear();
}

// Node-major operands: which kernel takes one call.  The tiled kernels read X and write Y as 16-byte pieces and keep a gathered row's
// offset in 32 bits of 16-byte units: even k, ld and batch strides, 16-byte aligned bases, n_cols * ldx < 2^32 -- else the plain kernel.
enum { SPMM_ROWS_PLAIN = 0, SPMM_ROWS_TILES = 1, SPMM_ROWS_PAD = 2 };
struct SpmmRowsRoute { int kind, ng; };                  // ng: gather loads per thread and chunk (7: up to 224 distinct columns, else SPMM_NG)
static SpmmRowsRoute spmm_rows_route(int plan_state, int ucap, int ecap_pad, int64_t n_cols, int k, int64_t ldx, int64_t ldy,
                                     bool x_aligned, bool y_aligned, int64_t x_stride, int64_t y_stride, bool no_pad) {
    const bool aligned = (k % 2 == 0) && (ldx % 2 == 0) && (ldy % 2 == 0) && x_aligned && y_aligned && (x_stride % 2 == 0) &&
                         (y_stride % 2 == 0) && (n_cols * ldx < ((int64_t)1 << 32));
    if (plan_state != 1 || !aligned) return {SPMM_ROWS_PLAIN, 0};
    // 7 gather loads per thread and chunk serve up to 224 distinct columns per tile, 10 up to 320
    return {ecap_pad > 0 && !no_pad ? SPMM_ROWS_PAD : SPMM_ROWS_TILES, ucap <= 224 ? 7 : SPMM_NG};
}
static bool ptr_aligned16(const void* p) { return ((uintptr_t)p) % 16 == 0; }

gmrf_status gmrf_csr_create(int32_t device, void* stream, int64_t n_rows, int64_t n_cols, const int64_t* rowptr,
                            const int64_t* colidx, const double* vals, int32_t index_base, int32_t values_f32,
                            gmrf_csr** out) {
    if (!out || !rowptr || !colidx || !vals || n_rows <= 0 || n_cols <= 0) return bad_shape("bad CSR arguments");
    // (whatever fails from here on, the guard's gmrf_csr_destroy releases what has been allocated so far)
    std::unique_ptr<gmrf_csr, gmrf_status (*)(gmrf_csr*)> guard(new gmrf_csr(), gmrf_csr_destroy);
    gmrf_csr* m = guard.get();
    GCHK(m->open(device, stream, hipStreamNonBlocking, "gmrf_csr_create", /*pattern_only_ok=*/false));
    const int64_t nnz = rowptr[n_rows] - index_base;
    if (nnz < 0 || rowptr[0] != index_base) return bad_shape("bad CSR row pointers");
    std::vector<int64_t> rp((size_t)n_rows + 1);
    for (int64_t i = 0; i <= n_rows; ++i) {
        rp[i] = rowptr[i] - index_base;
        if (i > 0 && rp[i] < rp[i - 1]) return bad_shape("CSR row pointers must be non-decreasing");
    }
    std::vector<int32_t> ci((size_t)nnz);
    for (int64_t p = 0; p < nnz; ++p) {
        const int64_t c = colidx[p] - index_base;
        if (c < 0 || c >= n_cols) return bad_shape("column index out of range");
        ci[p] = (int32_t)c;
    }
    m->id = ++g_csr_ids;
    m->tiles_ok = spmv_tiles_ok(n_rows, rp.data());
    m->n_rows = n_rows; m->n_cols = n_cols; m->nnz = nnz;
    GCHK(m->d_rowptr.upload(m->stream, rp));
    GCHK(m->d_colidx.upload(m->stream, ci));
    HIPCHK(hipStreamSynchronize(m->stream));
    if (values_f32) {
        std::vector<float> vf((size_t)nnz);
        for (int64_t p = 0; p < nnz; ++p) vf[p] = (float)vals[p];
        GCHK(m->d_vals32.upload(m->stream, vf));
        HIPCHK(hipStreamSynchronize(m->stream));
    } else {
        GCHK(m->d_vals.upload(m->stream, vals, (size_t)nnz));
        HIPCHK(hipStreamSynchronize(m->stream));
    }
    if (n_rows == n_cols) {
        GCHK(m->d_diag.reserve(m->stream, (size_t)n_rows));
        hipLaunchKernelGGL(csr_extract_diag, dim3((unsigned)((n_rows + 255) / 256)), dim3(256), 0, m->stream,
                           m->d_rowptr, m->d_colidx, m->d_vals, m->d_vals32, n_rows, m->d_diag);
        HIPCHK(hipGetLastError());
        HIPCHK(hipStreamSynchronize(m->stream));
    }
    *out = guard.release();
    return GMRF_OK;
}

gmrf_status gmrf_csr_destroy(gmrf_csr* m) {
    if (!m) return GMRF_OK;
    m->close();
    delete m;
    return GMRF_OK;
}

static gmrf_status spmm_device(const gmrf_csr* S, hipStream_t st, const double* d_X, int64_t ldx, double* d_Y,
                               int64_t ldy, int k, const double* vals_override = nullptr) {
    const int lg = spmm_cols_route(S->nnz, S->n_rows, k, S->tiles_ok);      // 0: csr_spmv_tiles, else the lane group
    const_cast<gmrf_csr*>(S)->last_cols_g = lg;
    const int bl = 256;
    if (lg == 0) {
        // SpMV: LDS-staged row tiles (with 3+ right-hand sides the lane-group kernel, which reuses the
        // entries for four of them, is faster than one pass per right-hand side)
        // (at most 256 * 8 workgroups -- what the chip holds at once -- each walking several tiles)
        const dim3 grid((unsigned)std::min<int64_t>((S->n_rows + SPMV_ROWS - 1) / SPMV_ROWS, 256 * 8));
#define GMRF_SPMV(VT, VP)                                                                                                   \
        hipLaunchKernelGGL(csr_spmv_tiles<VT>, grid, dim3(bl), 0, st, S->d_rowptr, S->d_colidx, VP, S->n_rows, d_X + r * ldx, d_Y + r * ldy)
        for (int r = 0; r < k; ++r) {
            if (vals_override) GMRF_SPMV(double, vals_override);
            else if (S->d_vals32) GMRF_SPMV(float, S->d_vals32);
            else GMRF_SPMV(double, S->d_vals);
        }
#undef GMRF_SPMV
        HIPCHK(hipGetLastError());
        return GMRF_OK;
    }
    auto grid_for = [&](int G) { return dim3((unsigned)((S->n_rows * G + bl - 1) / bl)); };
#define SPMM_LAUNCH(VT, G, VP)                                                                               \
    hipLaunchKernelGGL((csr_spmm<VT, G>), grid_for(G), dim3(bl), 0, st, S->d_rowptr, S->d_colidx, VP,        \
                       S->n_rows, d_X, ldx, d_Y, ldy, k)
#define SPMM_LAUNCH_G(VT, VP)                                                                                \
    do {                                                                                                     \
        if (lg == 64) SPMM_LAUNCH(VT, 64, VP);                                                               \
        else if (lg == 32) SPMM_LAUNCH(VT, 32, VP);                                                          \
        else if (lg == 16) SPMM_LAUNCH(VT, 16, VP);                                                          \
        else SPMM_LAUNCH(VT, 8, VP);                                                                         \
    } while (0)
    if (vals_override) SPMM_LAUNCH_G(double, vals_override);      // same pattern, another problem's values (fp64)
    else if (S->d_vals32) SPMM_LAUNCH_G(float, S->d_vals32);
    else SPMM_LAUNCH_G(double, S->d_vals);
#undef SPMM_LAUNCH_G
#undef SPMM_LAUNCH
    HIPCHK(hipGetLastError());
    return GMRF_OK;
}

// The tile plan of a matrix, built once (spmm_plan_host over the pattern read back from the device, like the symbolic phase
// of the factor) and uploaded.
static gmrf_status spmm_plan(gmrf_csr* m) {
    if (m->plan_state != 0) return GMRF_OK;
    std::vector<int64_t> rp((size_t)m->n_rows + 1);
    std::vector<int32_t> ci((size_t)std::max<int64_t>(m->nnz, 1));
    HIPCHK(hipMemcpyAsync(rp.data(), m->d_rowptr, sizeof(int64_t) * (m->n_rows + 1), hipMemcpyDeviceToHost, m->stream));
    if (m->nnz > 0) HIPCHK(hipMemcpyAsync(ci.data(), m->d_colidx, sizeof(int32_t) * m->nnz, hipMemcpyDeviceToHost, m->stream));
    HIPCHK(hipStreamSynchronize(m->stream));
    SpmmPlan pl;
    spmm_plan_host(m->n_rows, rp.data(), ci.data(), pl);
    m->plan_state = -1;
    if (pl.state != 1) return GMRF_OK;
    m->plan_rows = pl.R; m->plan_ucap = pl.ucap; m->plan_ecap = pl.ecap; m->plan_umax = pl.umax; m->plan_ecap_pad = pl.ecap_pad;
    m->n_ucols = (int64_t)pl.ucols.size();
    GCHK(m->d_tile_uptr.upload(m->stream, pl.tile_uptr));
    GCHK(m->d_ucols.upload(m->stream, pl.ucols));
    GCHK(m->d_lidx.upload(m->stream, pl.lidx.data(), (size_t)m->nnz));
    HIPCHK(hipStreamSynchronize(m->stream));
    m->plan_state = 1;
    return GMRF_OK;
}

// Launch geometry of the tiled kernels on S's plan: the padded kernel sizes its LDS image by the distinct columns rounded to 8
struct SpmmTileGeom { int R, uc, ec; size_t lds; };
static SpmmTileGeom spmm_tile_geom(const gmrf_csr* m, bool pad) {
    SpmmTileGeom g;
    g.R = m->plan_rows;
    g.uc = pad ? (m->plan_umax + 7) / 8 * 8 : m->plan_ucap;            // LDS rows of the staged X image
    g.ec = pad ? m->plan_ecap_pad : m->plan_ecap;
    g.lds = pad ? spmm_tile_pad_lds_bytes(g.R, g.uc, g.ec) : spmm_tile_lds_bytes(g.R, g.uc, g.ec);
    return g;
}

// Y = S X with node-major device operands (X[col][rhs], Y[row][rhs]); vals_override: same pattern,
// another problem's fp64 values.
static gmrf_status spmm_rows_device(const gmrf_csr* S, hipStream_t st, const double* d_X, int64_t ldx, double* d_Y,
                                    int64_t ldy, int k, const double* vals_override = nullptr) {
    gmrf_csr* m = const_cast<gmrf_csr*>(S);
    GCHK(spmm_plan(m));
    const SpmmRowsRoute rt = spmm_rows_route(m->plan_state, m->plan_ucap, m->plan_ecap_pad, S->n_cols, k, ldx, ldy, ptr_aligned16(d_X),
                                             ptr_aligned16(d_Y), 0, 0, false);
    m->last_rows_kind = rt.kind; m->last_rows_ng = rt.ng;
    if (rt.kind != SPMM_ROWS_PLAIN) {
        const bool pad = rt.kind == SPMM_ROWS_PAD;
        const SpmmTileGeom tg = spmm_tile_geom(m, pad);
        const dim3 grid((unsigned)((S->n_rows + tg.R - 1) / tg.R));
#define GMRF_SPMM_TILES_K(KERNEL, VT, NGV, VP)                                                                           \
        hipLaunchKernelGGL((KERNEL<VT, NGV>), grid, dim3(SPMM_THREADS), tg.lds, st, S->d_rowptr, S->d_lidx, VP, S->d_tile_uptr, \
                           S->d_ucols, S->n_rows, d_X, ldx, d_Y, ldy, k, tg.R, tg.uc, tg.ec, SpmmBatch())
#define GMRF_SPMM_TILES(VT, VP)                                                                                          \
        do {                                                                                                             \
            if (pad && rt.ng == 7) GMRF_SPMM_TILES_K(csr_spmm_tiles_pad, VT, 7, VP);                                     \
            else if (pad) GMRF_SPMM_TILES_K(csr_spmm_tiles_pad, VT, SPMM_NG, VP);                                        \
            else if (rt.ng == 7) GMRF_SPMM_TILES_K(csr_spmm_tiles, VT, 7, VP);                                           \
            else GMRF_SPMM_TILES_K(csr_spmm_tiles, VT, SPMM_NG, VP);                                                     \
        } while (0)
        if (vals_override) GMRF_SPMM_TILES(double, vals_override);
        else if (S->d_vals32) GMRF_SPMM_TILES(float, S->d_vals32);
        else GMRF_SPMM_TILES(double, S->d_vals);
#undef GMRF_SPMM_TILES
#undef GMRF_SPMM_TILES_K
    } else {
        const dim3 grid((unsigned)((S->n_rows + 15) / 16));
        if (vals_override) hipLaunchKernelGGL(csr_spmm_rows<double>, grid, dim3(256), 0, st, S->d_rowptr, S->d_colidx, vals_override, S->n_rows, d_X, ldx, d_Y, ldy, k);
        else if (S->d_vals32) hipLaunchKernelGGL(csr_spmm_rows<float>, grid, dim3(256), 0, st, S->d_rowptr, S->d_colidx, S->d_vals32, S->n_rows, d_X, ldx, d_Y, ldy, k);
        else hipLaunchKernelGGL(csr_spmm_rows<double>, grid, dim3(256), 0, st, S->d_rowptr, S->d_colidx, S->d_vals, S->n_rows, d_X, ldx, d_Y, ldy, k);
    }
    HIPCHK(hipGetLastError());
    return GMRF_OK;
}

// The same product for `batch` problems on S's pattern in one launch: problem p has the fp64 values vals + p nnz and the
// node-major operands d_X + p x_stride, d_Y + p y_stride.  The route (tiled, padded, plain) is the one spmm_rows_route gives
// one problem -- the strides keep the operands 16-byte aligned or the plain kernel runs.  no_pad withholds the padded plan
// for this call (gmrf_test_spmm_rows_batch: the unpadded kernels on a matrix whose padded image fits).
static gmrf_status spmm_rows_device_batch(const gmrf_csr* S, hipStream_t st, int64_t batch, const double* vals, const double* d_X,
                                          int64_t ldx, int64_t x_stride, double* d_Y, int64_t ldy, int64_t y_stride, int k,
                                          bool no_pad = false) {
    gmrf_csr* m = const_cast<gmrf_csr*>(S);
    GCHK(spmm_plan(m));
    const SpmmRowsRoute rt = spmm_rows_route(m->plan_state, m->plan_ucap, m->plan_ecap_pad, S->n_cols, k, ldx, ldy, ptr_aligned16(d_X),
                                             ptr_aligned16(d_Y), x_stride, y_stride, no_pad);
    m->last_rows_kind = rt.kind; m->last_rows_ng = rt.ng;
    if (rt.kind != SPMM_ROWS_PLAIN) {
        const bool pad = rt.kind == SPMM_ROWS_PAD;
        const SpmmTileGeom tg = spmm_tile_geom(m, pad);
        const dim3 grid((unsigned)((S->n_rows + tg.R - 1) / tg.R), (unsigned)batch);
#define GMRF_SPMM_TILES_B(KERNEL, NGV)                                                                                        \
        hipLaunchKernelGGL((KERNEL<double, NGV, true>), grid, dim3(SPMM_THREADS), tg.lds, st, S->d_rowptr, S->d_lidx, vals, S->d_tile_uptr, \
                           S->d_ucols, S->n_rows, d_X, ldx, d_Y, ldy, k, tg.R, tg.uc, tg.ec, sb)
        const SpmmBatch sb{S->nnz, x_stride, y_stride};
        if (pad && rt.ng == 7) GMRF_SPMM_TILES_B(csr_spmm_tiles_pad, 7);
        else if (pad) GMRF_SPMM_TILES_B(csr_spmm_tiles_pad, SPMM_NG);
        else if (rt.ng == 7) GMRF_SPMM_TILES_B(csr_spmm_tiles, 7);
        else GMRF_SPMM_TILES_B(csr_spmm_tiles, SPMM_NG);
#undef GMRF_SPMM_TILES_B
    } else {
        hipLaunchKernelGGL(csr_spmm_rows_batch<double>, dim3((unsigned)((S->n_rows + 15) / 16), (unsigned)batch), dim3(256), 0, st,
                           S->d_rowptr, S->d_colidx, vals, S->n_rows, d_X, ldx, d_Y, ldy, k, S->nnz, x_stride, y_stride);
    }
    HIPCHK(hipGetLastError());
    return GMRF_OK;
}

// Y = S X with NODE-MAJOR operands: X is n_cols x k with the k values of a column index contiguous
// (row stride ldx >= k), Y likewise (ldy >= k) -- in Julia terms the k x n matrices permutedims(X),
// permutedims(Y).  This is the layout the LDS-tiled kernel wants (one gathered column index fetches
// k contiguous doubles); host pointers are staged.
gmrf_status gmrf_spmm_rows(const gmrf_csr* S, const double* X, double* Y, int64_t k, int64_t ldx, int64_t ldy) {
    if (!S || !X || !Y) return bad_shape("null pointer");
    if (k <= 0 || k > (1 << 20) || ldx < k || ldy < k) return bad_shape("bad k / ld");
    HIPCHK(hipSetDevice(S->device));
    gmrf_csr* m = const_cast<gmrf_csr*>(S);
    const bool x_dev = is_device_ptr(X), y_dev = is_device_ptr(Y);
    const double* d_X = X;
    double* d_Y = Y;
    int64_t lx = ldx, ly = ldy;
    const int64_t kk = k + (k & 1);                       // staging keeps rows 16-byte aligned
    if (!x_dev) {
        GCHK(m->stage_x.reserve(S->stream, sizeof(double) * kk * S->n_cols));
        HIPCHK(hipMemcpy2DAsync(m->stage_x.p, kk * sizeof(double), X, ldx * sizeof(double), k * sizeof(double), S->n_cols,
                                hipMemcpyHostToDevice, S->stream));
        d_X = m->stage_x.as<double>(); lx = kk;
    }
    if (!y_dev) {
        GCHK(m->stage_y.reserve(S->stream, sizeof(double) * kk * S->n_rows));
        d_Y = m->stage_y.as<double>(); ly = kk;
    }
    GCHK(spmm_rows_device(S, S->stream, d_X, lx, d_Y, ly, (int)k));
    if (!y_dev)
        HIPCHK(hipMemcpy2DAsync(Y, ldy * sizeof(double), d_Y, kk * sizeof(double), k * sizeof(double), S->n_rows,
                                hipMemcpyDeviceToHost, S->stream));
    HIPCHK(hipStreamSynchronize(S->stream));
    return GMRF_OK;
}

gmrf_status gmrf_spmm(const gmrf_csr* S, const double* X, double* Y, int64_t k, int64_t ldx, int64_t ldy) {
    if (!S || !X || !Y) return bad_shape("null pointer");
    if (k <= 0 || ldx < S->n_cols || ldy < S->n_rows) return bad_shape("bad k / ld");
    HIPCHK(hipSetDevice(S->device));
    gmrf_csr* m = const_cast<gmrf_csr*>(S);
    const bool x_dev = is_device_ptr(X), y_dev = is_device_ptr(Y);
    const double* d_X = X;
    double* d_Y = Y;
    int64_t lx = ldx, ly = ldy;
    if (!x_dev) {
        GCHK(m->stage_x.reserve(S->stream, sizeof(double) * k * S->n_cols));
        HIPCHK(hipMemcpy2DAsync(m->stage_x.p, S->n_cols * sizeof(double), X, ldx * sizeof(double),
                                S->n_cols * sizeof(double), k, hipMemcpyHostToDevice, S->stream));
        d_X = m->stage_x.as<double>(); lx = S->n_cols;
    }
    if (!y_dev) {
        GCHK(m->stage_y.reserve(S->stream, sizeof(double) * k * S->n_rows));
        d_Y = m->stage_y.as<double>(); ly = S->n_rows;
    }
    GCHK(spmm_device(S, S->stream, d_X, lx, d_Y, ly, (int)k));
    if (!y_dev)
        HIPCHK(hipMemcpy2DAsync(Y, ldy * sizeof(double), d_Y, S->n_rows * sizeof(double),
                                S->n_rows * sizeof(double), k, hipMemcpyDeviceToHost, S->stream));
    HIPCHK(hipStreamSynchronize(S->stream));
    return GMRF_OK;
}

// Stream-ordered variants for device-resident operands: no staging, no synchronisation -- the product is enqueued on
// the matrix's stream and the call returns (pipelines of `Q * x` on the device: Gauss-Newton loops, estimators).
gmrf_status gmrf_spmm_async(const gmrf_csr* S, const double* X, double* Y, int64_t k, int64_t ldx, int64_t ldy) {
    if (!S || !X || !Y) return bad_shape("null pointer");
    if (k <= 0 || ldx < S->n_cols || ldy < S->n_rows) return bad_shape("bad k / ld");
    HIPCHK(hipSetDevice(S->device));
    if (!is_device_ptr(X) || !is_device_ptr(Y)) return bad_shape("gmrf_spmm_async takes device pointers");
    return spmm_device(S, S->stream, X, ldx, Y, ldy, (int)k);
}

gmrf_status gmrf_spmm_rows_async(const gmrf_csr* S, const double* X, double* Y, int64_t k, int64_t ldx, int64_t ldy) {
    if (!S || !X || !Y) return bad_shape("null pointer");
    if (k <= 0 || k > (1 << 20) || ldx < k || ldy < k) return bad_shape("bad k / ld");
    HIPCHK(hipSetDevice(S->device));
    if (!is_device_ptr(X) || !is_device_ptr(Y)) return bad_shape("gmrf_spmm_rows_async takes device pointers");
    return spmm_rows_device(S, S->stream, X, ldx, Y, ldy, (int)k);
}

// --------------------------------------------------------------------------------- posterior assembly
struct gmrf_assembler : DevCtx {        // device -1: symbolic only (pattern queries; no numeric phase)
    int64_t n = 0, m = 0, nnz_q = 0, nnz_j = 0, nnz_out = 0, n_pairs = 0;
    std::vector<int64_t> colptr, rowval;            // result pattern (CSC, 0-based, rows ascending)
    DevArr<int64_t> d_pptr, d_qmap, d_jt_ptr, d_j_rptr;
    DevArr<int32_t> d_pa, d_pb, d_jt_row, d_jt_src, d_j_col;
    DevBuf arena;                       // host arguments of the current call (Staging)
    // the batch calls: Q's own pattern (0-based; symmetric, so its CSC arrays are read by rows), uploaded by the first objective
    std::vector<int64_t> q_ptr;
    std::vector<int32_t> q_row;
    DevArr<int64_t> d_q_ptr;
    DevArr<int32_t> d_q_row;
    // ... and the result pattern the same way (colptr / rowval with 32-bit rows), uploaded by the first quadratic form
    DevArr<int64_t> d_o_ptr;
    DevArr<int32_t> d_o_row;
    DevBuf bpart;                       // work arrays: [batch][m] (J x + obs_diff) of the rhs, the partial sums of the objective / quadratic form
};

gmrf_status gmrf_assemble_create(int32_t device, void* stream, int64_t n, const int64_t* q_colptr, const int64_t* q_rowval,
                                 int64_t m, const int64_t* j_rowptr, const int64_t* j_colidx, int32_t index_base,
                                 gmrf_assembler** out) {
    if (!out || !q_colptr || !q_rowval || !j_rowptr || !j_colidx || n <= 0 || m <= 0) return bad_shape("bad assembler arguments");
    if (index_base != 0 && index_base != 1) return bad_shape("index_base must be 0 or 1");
    const int64_t b = index_base;
    const int64_t nnz_q = q_colptr[n] - b, nnz_j = j_rowptr[m] - b;
    if (nnz_q < 0 || nnz_j < 0 || nnz_j >= ((int64_t)1 << 31)) return bad_shape("bad pattern sizes");
    // J by columns: for column j the (row k, position in the CSR value array)
    std::vector<int64_t> jt_ptr((size_t)n + 1, 0);
    for (int64_t p = 0; p < nnz_j; ++p) {
        const int64_t c = j_colidx[p] - b;
        if (c < 0 || c >= n) return bad_shape("J column index out of range");
        jt_ptr[c + 1]++;
    }
    for (int64_t i = 0; i < n; ++i) jt_ptr[i + 1] += jt_ptr[i];
    std::vector<int32_t> jt_row((size_t)nnz_j), jt_src((size_t)nnz_j), j_col((size_t)nnz_j);
    {
        std::vector<int64_t> fill(jt_ptr.begin(), jt_ptr.end() - 1);
        for (int64_t k = 0; k < m; ++k)
            for (int64_t p = j_rowptr[k] - b; p < j_rowptr[k + 1] - b; ++p) {
                const int64_t c = j_colidx[p] - b;
                jt_row[fill[c]] = (int32_t)k; jt_src[fill[c]] = (int32_t)p; fill[c]++;
                j_col[p] = (int32_t)c;
            }
    }
    // result column j = rows of Q's column j  U  { i : J[k,i] != 0 and J[k,j] != 0 for some k }
    struct Prod { int64_t i; int32_t k, a, b; };
    // (whatever fails from here on, the guard's gmrf_assemble_destroy releases what has been built so far)
    std::unique_ptr<gmrf_assembler, gmrf_status (*)(gmrf_assembler*)> guard(new gmrf_assembler(), gmrf_assemble_destroy);
    gmrf_assembler* as = guard.get();
    as->n = n; as->m = m; as->nnz_q = nnz_q; as->nnz_j = nnz_j;
    as->colptr.assign((size_t)n + 1, 0);
    std::vector<int64_t> pptr(1, 0), qmap;
    std::vector<int32_t> pa, pb;
    std::vector<Prod> prods;
    for (int64_t j = 0; j < n; ++j) {
        prods.clear();
        for (int64_t t = jt_ptr[j]; t < jt_ptr[j + 1]; ++t) {
            const int64_t k = jt_row[t];
            for (int64_t p = j_rowptr[k] - b; p < j_rowptr[k + 1] - b; ++p)
                prods.push_back({j_colidx[p] - b, (int32_t)k, (int32_t)p, jt_src[t]});
        }
        std::sort(prods.begin(), prods.end(), [](const Prod& x, const Prod& y) { return x.i != y.i ? x.i < y.i : x.k < y.k; });
        size_t pi = 0;
        int64_t qp = q_colptr[j] - b;
        const int64_t qe = q_colptr[j + 1] - b;
        int64_t last_row = -1;
        while (pi < prods.size() || qp < qe) {
            const int64_t rq = qp < qe ? q_rowval[qp] - b : INT64_MAX, rp = pi < prods.size() ? prods[pi].i : INT64_MAX;
            const int64_t r = std::min(rq, rp);
            if (r < 0 || r >= n || r <= last_row) return bad_shape("Q rows must be ascending within a column and in range");
            last_row = r;
            as->rowval.push_back(r);
            qmap.push_back(rq == r ? qp++ : -1);
            while (pi < prods.size() && prods[pi].i == r) { pa.push_back(prods[pi].a); pb.push_back(prods[pi].b); ++pi; }
            pptr.push_back((int64_t)pa.size());
        }
        as->colptr[j + 1] = (int64_t)as->rowval.size();
    }
    as->nnz_out = (int64_t)as->rowval.size();
    as->n_pairs = (int64_t)pa.size();
    if (n < ((int64_t)1 << 31)) {
        as->q_ptr.resize((size_t)n + 1); as->q_row.resize((size_t)nnz_q);
        for (int64_t j = 0; j <= n; ++j) as->q_ptr[(size_t)j] = q_colptr[j] - b;
        for (int64_t e = 0; e < nnz_q; ++e) as->q_row[(size_t)e] = (int32_t)(q_rowval[e] - b);
    }
    GCHK(as->open(device, stream, hipStreamDefault, "gmrf_assemble_create"));      // (a blocking stream: inherited, not chosen)
    if (as->device >= 0) {
        auto up = [&](auto& d, const auto& v) -> gmrf_status {
            GCHK(d.upload(as->stream, v));
            HIPCHK(hipStreamSynchronize(as->stream));
            return GMRF_OK;
        };
        std::vector<int64_t> j_rptr((size_t)m + 1);
        for (int64_t k = 0; k <= m; ++k) j_rptr[k] = j_rowptr[k] - b;
        GCHK(up(as->d_pptr, pptr)); GCHK(up(as->d_qmap, qmap)); GCHK(up(as->d_pa, pa)); GCHK(up(as->d_pb, pb));
        GCHK(up(as->d_jt_ptr, jt_ptr)); GCHK(up(as->d_jt_row, jt_row)); GCHK(up(as->d_jt_src, jt_src));
        GCHK(up(as->d_j_rptr, j_rptr)); GCHK(up(as->d_j_col, j_col));
    }
    *out = guard.release();
    return GMRF_OK;
}

gmrf_status gmrf_assemble_destroy(gmrf_assembler* as) {
    if (!as) return GMRF_OK;
    as->close();
    delete as;
    return GMRF_OK;
}

gmrf_status gmrf_assemble_pattern(const gmrf_assembler* as, int64_t* nnz_out, int64_t* n_products, int64_t* colptr,
                                  int64_t* rowval, int32_t index_base) {
    if (!as) return bad_shape("null assembler");
    if (nnz_out) *nnz_out = as->nnz_out;
    if (n_products) *n_products = as->n_pairs;
    if (colptr) for (int64_t j = 0; j <= as->n; ++j) colptr[j] = as->colptr[j] + index_base;
    if (rowval) for (int64_t e = 0; e < as->nnz_out; ++e) rowval[e] = as->rowval[e] + index_base;
    return GMRF_OK;
}

static const char* const AS_PATTERN_ONLY = "symbolic-only assembler";

// (defined with the batch forms below: a one-problem call is a batch of 1)
static gmrf_status assemble_precision_staged(gmrf_assembler* as, int64_t batch, const double* q_nzval, int64_t q_stride,
                                             const double* j_vals, double noise, double* out_nzval);
static gmrf_status assemble_rhs_staged(gmrf_assembler* as, int64_t batch, const double* base, const double* j_vals, const double* x,
                                       const double* obs_diff, double noise, double* out);

gmrf_status gmrf_assemble_precision(gmrf_assembler* as, const double* q_nzval, const double* j_vals, double noise,
                                    double* out_nzval) {
    if (!as) return bad_shape("null assembler");
    GCHK(as->ready(AS_PATTERN_ONLY));
    if (!q_nzval || !j_vals || !out_nzval) return bad_shape("null pointer");
    return assemble_precision_staged(as, 1, q_nzval, 0, j_vals, noise, out_nzval);
}

gmrf_status gmrf_assemble_rhs(gmrf_assembler* as, const double* base, const double* j_vals, const double* x,
                              const double* obs_diff, double noise, double* out) {
    if (!as) return bad_shape("null assembler");
    GCHK(as->ready(AS_PATTERN_ONLY));
    if (!j_vals || !x || !out) return bad_shape("null pointer");
    return assemble_rhs_staged(as, 1, base, j_vals, x, obs_diff, noise, out);
}

// --------------------------------------------------------------------------------- FEM block assembly (Darcy, P1)
struct gmrf_darcy_p1 : DevCtx {         // device -1: pattern only
    int64_t nx = 0, ny = 0, n = 0, nnz = 0;
    int order = 1;                      // 1: P1 triangles on the nx x ny nodes; 2: quadratic triangles, dofs = the (2 nx - 1) x (2 ny - 1) lattice
    std::vector<int64_t> rowptr, colidx;            // 0-based
    DevArr<int64_t> d_rowptr;
    DevArr<int32_t> d_colidx;           // order 2: the pattern's columns and the Dirichlet mask for darcy_p2_constrain_batch
    DevArr<uint8_t> d_pres;
    DevBuf arena;                       // host arguments of the current call (Staging)
    DevBuf bwork;                       // work of an assembly: [batch][n] |diagonal|, [batch] means
};

// Pattern of the quadratic-triangle lattice: row (I, J) couples with every node of every cell it belongs to (the same
// enumeration as darcy_p2_row: 5 x 5 window of lattice offsets, touched entries in ascending column order).
static void p2_lattice_pattern(int64_t nx, int64_t ny, std::vector<int64_t>& rowptr, std::vector<int64_t>& colidx) {
    const int64_t W = 2 * nx - 1, H = 2 * ny - 1;
    rowptr.assign((size_t)(W * H) + 1, 0);
    colidx.clear();
    colidx.reserve((size_t)(W * H) * 12);
    for (int64_t J = 0; J < H; ++J)
        for (int64_t I = 0; I < W; ++I) {
            unsigned present = 0u;
            int cand[6][3], nc;
            if (!(I & 1) && !(J & 1)) { const int t[6][3] = {{-1, -1, 0}, {-1, 0, 0}, {0, 0, 0}, {-1, -1, 1}, {0, -1, 1}, {0, 0, 1}}; nc = 6; memcpy(cand, t, sizeof(t)); }
            else if ((I & 1) && !(J & 1)) { const int t[2][3] = {{0, 0, 0}, {0, -1, 1}}; nc = 2; memcpy(cand, t, sizeof(t)); }
            else if (!(I & 1) && (J & 1)) { const int t[2][3] = {{-1, 0, 0}, {0, 0, 1}}; nc = 2; memcpy(cand, t, sizeof(t)); }
            else { const int t[2][3] = {{0, 0, 0}, {0, 0, 1}}; nc = 2; memcpy(cand, t, sizeof(t)); }
            for (int e = 0; e < nc; ++e) {
                const int64_t qx = I / 2 + cand[e][0], qy = J / 2 + cand[e][1];
                if (qx < 0 || qy < 0 || qx >= nx - 1 || qy >= ny - 1) continue;
                const bool upper = cand[e][2] != 0;
                const int64_t I0 = 2 * qx, J0 = 2 * qy;
                int64_t nI[6], nJ[6];
                nI[0] = I0; nJ[0] = J0;
                if (!upper) { nI[1] = I0 + 2; nJ[1] = J0; nI[2] = I0 + 2; nJ[2] = J0 + 2; }
                else { nI[1] = I0 + 2; nJ[1] = J0 + 2; nI[2] = I0; nJ[2] = J0 + 2; }
                nI[3] = (nI[0] + nI[1]) / 2; nJ[3] = (nJ[0] + nJ[1]) / 2;
                nI[4] = (nI[1] + nI[2]) / 2; nJ[4] = (nJ[1] + nJ[2]) / 2;
                nI[5] = (nI[2] + nI[0]) / 2; nJ[5] = (nJ[2] + nJ[0]) / 2;
                for (int j = 0; j < 6; ++j) present |= 1u << (unsigned)((nJ[j] - J + 2) * 5 + (nI[j] - I + 2));
            }
            for (int s5 = 0; s5 < 25; ++s5)
                if (present & (1u << s5)) colidx.push_back((J + s5 / 5 - 2) * W + (I + s5 % 5 - 2));
            rowptr[(size_t)(J * W + I) + 1] = (int64_t)colidx.size();
        }
}

static void darcy_p2_pattern(gmrf_darcy_p1* d) {
    d->n = (2 * d->nx - 1) * (2 * d->ny - 1);
    p2_lattice_pattern(d->nx, d->ny, d->rowptr, d->colidx);
}

// CSR pattern of the P1 triangle mesh (nx x ny nodes, x fastest, quads cut by the diagonal n00 - n11): the 7-point stencil
// -nx-1, -nx, -1, 0, +1, +nx, +nx+1 clipped at the border, ascending columns (Darcy P1 and the elliptic tangent)
static void p1_stencil_pattern(int64_t nx, int64_t ny, std::vector<int64_t>& rowptr, std::vector<int64_t>& colidx) {
    rowptr.assign((size_t)(nx * ny) + 1, 0);
    colidx.clear();
    colidx.reserve((size_t)(nx * ny) * 7);
    const int dxs[7] = {-1, 0, -1, 0, 1, 0, 1}, dys[7] = {-1, -1, 0, 0, 0, 1, 1};
    for (int64_t iy = 0; iy < ny; ++iy)
        for (int64_t ix = 0; ix < nx; ++ix) {
            for (int s7 = 0; s7 < 7; ++s7) {
                const int64_t jx = ix + dxs[s7], jy = iy + dys[s7];
                if (jx < 0 || jy < 0 || jx >= nx || jy >= ny) continue;
                colidx.push_back(jy * nx + jx);
            }
            rowptr[(size_t)(iy * nx + ix) + 1] = (int64_t)colidx.size();
        }
}

static gmrf_status darcy_create(int32_t device, void* stream, int64_t nx, int64_t ny, int order, gmrf_darcy_p1** out) {
    if (!out || nx < 2 || ny < 2 || nx > 32768 || ny > 32768 || (order == 2 && (nx > 16384 || ny > 16384))) return bad_shape("bad Darcy mesh size");
    std::unique_ptr<gmrf_darcy_p1, gmrf_status (*)(gmrf_darcy_p1*)> guard(new gmrf_darcy_p1(), gmrf_darcy_p1_destroy);
    gmrf_darcy_p1* d = guard.get();
    d->nx = nx; d->ny = ny; d->n = nx * ny; d->order = order;
    if (order == 2) darcy_p2_pattern(d);
    else p1_stencil_pattern(nx, ny, d->rowptr, d->colidx);
    d->nnz = (int64_t)d->colidx.size();
    GCHK(d->open(device, stream, hipStreamNonBlocking, "gmrf_darcy_p1_create"));
    if (d->device >= 0) {
        GCHK(d->d_rowptr.upload(d->stream, d->rowptr.data(), (size_t)(d->n + 1)));
        std::vector<int32_t> col32;
        std::vector<uint8_t> pres;
        if (order == 2) {
            const int64_t W = 2 * nx - 1, H = 2 * ny - 1;
            col32.assign(d->colidx.begin(), d->colidx.end());
            pres.resize((size_t)d->n);
            for (int64_t r = 0; r < d->n; ++r) { const int64_t I = r % W, J = r / W; pres[(size_t)r] = (I == 0 || J == 0 || I == W - 1 || J == H - 1) ? 1 : 0; }
            GCHK(d->d_colidx.upload(d->stream, col32));
            GCHK(d->d_pres.upload(d->stream, pres));
        }
        HIPCHK(hipStreamSynchronize(d->stream));
    }
    *out = guard.release();
    return GMRF_OK;
}

gmrf_status gmrf_darcy_p1_create(int32_t device, void* stream, int64_t nx, int64_t ny, gmrf_darcy_p1** out) {
    return darcy_create(device, stream, nx, ny, 1, out);
}

gmrf_status gmrf_darcy_p2_create(int32_t device, void* stream, int64_t nx, int64_t ny, gmrf_darcy_p1** out) {
    return darcy_create(device, stream, nx, ny, 2, out);
}

gmrf_status gmrf_darcy_p1_destroy(gmrf_darcy_p1* d) {
    if (!d) return GMRF_OK;
    d->close();
    delete d;
    return GMRF_OK;
}

gmrf_status gmrf_darcy_p1_pattern(const gmrf_darcy_p1* d, int64_t* nnz_out, int64_t* rowptr, int64_t* colidx, int32_t index_base) {
    if (!d) return bad_shape("null handle");
    if (nnz_out) *nnz_out = d->nnz;
    if (rowptr) for (int64_t i = 0; i <= d->n; ++i) rowptr[i] = d->rowptr[(size_t)i] + index_base;
    if (colidx) for (int64_t e = 0; e < d->nnz; ++e) colidx[e] = d->colidx[(size_t)e] + index_base;
    return GMRF_OK;
}

static bool darcy_ng_ok(int64_t ng) { return ng >= 2 && ng <= 46340; }
// (defined with the batch form below: a one-problem call is a batch of 1)
static gmrf_status darcy_assemble_staged(gmrf_darcy_p1* d, int64_t batch, const double* coeff_tables, int64_t ng, double beta,
                                         double* vals_out, double* f_out);

gmrf_status gmrf_darcy_p1_assemble(gmrf_darcy_p1* d, const double* coeff_table, int64_t ng, double beta, double* vals_out,
                                   double* f_out) {
    if (!d || !coeff_table || !vals_out || !f_out || !darcy_ng_ok(ng)) return bad_shape("bad Darcy assembly arguments");
    return darcy_assemble_staged(d, 1, coeff_table, ng, beta, vals_out, f_out);
}

// --------------------------------------------------------------------------------- Burgers tangent (8f rank 4)
struct gmrf_burgers_p1 : DevCtx {       // device -1: pattern only
    int64_t ns = 0, nt = 0, rows = 0, nnz = 0;
    int order = 1;                      // 1: P1 line, 2: quadratic line
    int scheme = GMRF_BURGERS_EULER, bc = GMRF_BURGERS_PERIODIC;
    double dt = 0.0, nu = 0.0, h = 0.0; // h: cell length
    std::vector<int64_t> rowptr;        // 0-based row pointer of J
    DevArr<int64_t> d_rowptr;           // dirichlet only: the periodic rows have a closed form
    int64_t npts = 0;                   // GMRF_BURGERS_COLLOCATION (gmrf_burgers_colloc_create): the points of a slice, their
    std::vector<int32_t> cell;          // cells, and the device table of burgers_colloc.hpp: cells, then a and d as [3][npts]
    DevArr<int32_t> d_cell;
    DevArr<double> d_shape;             // a at 0, d at 3 npts
    DevBuf arena;                       // host arguments of the current call (Staging)
};

// The in-slice columns of row i, ascending: the window {i-1, i, i+1} (P1, quadratic midpoint) or {i-2 .. i+2} (quadratic
// vertex), wrapped on the periodic line, clipped to [0, ns) on the Dirichlet interval.  Returns their number.
static int burgers_line_row_cols(const gmrf_burgers_p1* b, int64_t i, int64_t (&c)[5]) {
    const int64_t r = (b->order == 2 && !(i & 1)) ? 2 : 1;
    int cnt = 0;
    for (int64_t j = i - r; j <= i + r; ++j) {
        if (b->bc == GMRF_BURGERS_PERIODIC) c[cnt++] = (j + b->ns) % b->ns;
        else if (j >= 0 && j < b->ns) c[cnt++] = j;
    }
    std::sort(c, c + cnt);
    return cnt;
}

gmrf_status gmrf_burgers_line_create(int32_t device, void* stream, int64_t nc, int64_t nt, double dt, double nu, int32_t order,
                                     int32_t scheme, int32_t bc, double length, gmrf_burgers_p1** out) {
    const bool dirichlet = bc == GMRF_BURGERS_DIRICHLET;
    if (!out || (order != 1 && order != 2) || (scheme != GMRF_BURGERS_EULER && scheme != GMRF_BURGERS_CN) ||
        (bc != GMRF_BURGERS_PERIODIC && !dirichlet))
        return bad_shape("bad Burgers line (order 1 or 2, scheme euler or cn, bc periodic or dirichlet)");
    if (nc < (dirichlet ? 2 : 3) || nt < 2 || nc > (1 << 24) || order * nc + (dirichlet ? 1 : 0) > (1 << 24) || nt > (1 << 20) ||
        !(dt > 0.0) || !(nu >= 0.0) || !(length > 0.0) || !std::isfinite(length))
        return bad_shape("bad Burgers mesh (>= 3 cells, >= 2 on the Dirichlet interval; nt >= 2 slices, dt > 0, nu >= 0, length > 0)");
    std::unique_ptr<gmrf_burgers_p1, gmrf_status (*)(gmrf_burgers_p1*)> guard(new gmrf_burgers_p1(), gmrf_burgers_p1_destroy);
    gmrf_burgers_p1* b = guard.get();
    b->ns = order * nc + (dirichlet ? 1 : 0); b->nt = nt; b->rows = (nt - 1) * b->ns; b->dt = dt; b->nu = nu; b->order = order;
    b->scheme = scheme; b->bc = bc; b->h = length / (double)nc;
    b->rowptr.resize((size_t)b->rows + 1);
    b->rowptr[0] = 0;
    for (int64_t r = 0; r < b->rows; ++r) {
        int64_t c[5];
        b->rowptr[(size_t)r + 1] = b->rowptr[(size_t)r] + 2 * burgers_line_row_cols(b, r % b->ns, c);
    }
    b->nnz = b->rowptr[(size_t)b->rows];
    GCHK(b->open(device, stream, hipStreamNonBlocking, "gmrf_burgers_line_create"));
    if (b->device >= 0 && dirichlet) {
        GCHK(b->d_rowptr.upload(b->stream, b->rowptr.data(), (size_t)(b->rows + 1)));
        HIPCHK(hipStreamSynchronize(b->stream));
    }
    *out = guard.release();
    return GMRF_OK;
}

gmrf_status gmrf_burgers_p1_create(int32_t device, void* stream, int64_t ns, int64_t nt, double dt, double nu, gmrf_burgers_p1** out) {
    return gmrf_burgers_line_create(device, stream, ns, nt, dt, nu, 1, GMRF_BURGERS_EULER, GMRF_BURGERS_PERIODIC, 1.0, out);
}
gmrf_status gmrf_burgers_p2_create(int32_t device, void* stream, int64_t ns, int64_t nt, double dt, double nu, gmrf_burgers_p1** out) {
    if (ns % 2) return bad_shape("the quadratic line has an even number of dofs (>= 6): two per cell");
    return gmrf_burgers_line_create(device, stream, ns / 2, nt, dt, nu, 2, GMRF_BURGERS_EULER, GMRF_BURGERS_PERIODIC, 1.0, out);
}

// The collocation tangent of burgers_colloc.hpp on the periodic quadratic line.  The per-point table is computed here, once, in
// double precision; the pattern reads the same cells.
gmrf_status gmrf_burgers_colloc_create(int32_t device, void* stream, int64_t nc, int64_t nt, double dt, double nu, double length,
                                       int64_t npts, const double* points, gmrf_burgers_p1** out) {
    if (!out || !points) return bad_shape("null pointer");
    if (nc < 3 || nt < 2 || nc > (1 << 23) || nt > (1 << 20) || npts < 1 || npts > (1 << 24) || !(dt > 0.0) || !(nu >= 0.0) ||
        !(length > 0.0) || !std::isfinite(length) || ((nt - 1) * npts + 255) / 256 > 0x7fffffffLL)
        return bad_shape("bad Burgers collocation mesh (>= 3 cells, nt >= 2 slices, >= 1 point, dt > 0, nu >= 0, length > 0)");
    const double h = length / (double)nc;
    for (int64_t c = 0; c < npts; ++c)
        if (!std::isfinite(points[c]) || points[c] < 0.0 || !(points[c] < length)) {
            g_last_error = "collocation point " + std::to_string(c) + " = " + std::to_string(points[c]) + " is not in [0, length = " +
                           std::to_string(length) + ")";
            return GMRF_ERR_BAD_SHAPE;
        }
    std::unique_ptr<gmrf_burgers_p1, gmrf_status (*)(gmrf_burgers_p1*)> guard(new gmrf_burgers_p1(), gmrf_burgers_p1_destroy);
    gmrf_burgers_p1* b = guard.get();
    b->ns = 2 * nc; b->nt = nt; b->npts = npts; b->rows = (nt - 1) * npts; b->nnz = 6 * b->rows; b->dt = dt; b->nu = nu; b->order = 2;
    b->scheme = GMRF_BURGERS_COLLOCATION; b->bc = GMRF_BURGERS_PERIODIC; b->h = h;
    b->cell.resize((size_t)npts);
    std::vector<double> shape((size_t)(6 * npts));
    for (int64_t c = 0; c < npts; ++c) {
        const int64_t e = std::min((int64_t)std::floor(points[c] / h), nc - 1);
        const double xi = 2.0 * (points[c] - (double)e * h) / h - 1.0;
        const double a[3] = {0.5 * xi * (xi - 1.0), 0.5 * xi * (xi + 1.0), 1.0 - xi * xi};
        const double d[3] = {(xi - 0.5) * (2.0 / h), (xi + 0.5) * (2.0 / h), (-2.0 * xi) * (2.0 / h)};
        b->cell[(size_t)c] = (int32_t)e;
        for (int k = 0; k < 3; ++k) { shape[(size_t)(k * npts + c)] = a[k]; shape[(size_t)((3 + k) * npts + c)] = d[k]; }
    }
    b->rowptr.resize((size_t)b->rows + 1);
    for (int64_t r = 0; r <= b->rows; ++r) b->rowptr[(size_t)r] = 6 * r;
    GCHK(b->open(device, stream, hipStreamNonBlocking, "gmrf_burgers_colloc_create"));
    if (b->device >= 0) {
        GCHK(b->d_cell.upload(b->stream, b->cell.data(), (size_t)npts));
        GCHK(b->d_shape.upload(b->stream, shape.data(), 6 * (size_t)npts));
        HIPCHK(hipStreamSynchronize(b->stream));
    }
    *out = guard.release();
    return GMRF_OK;
}

gmrf_status gmrf_burgers_p1_destroy(gmrf_burgers_p1* b) {
    if (!b) return GMRF_OK;
    b->close();
    delete b;
    return GMRF_OK;
}

// CSR pattern of J: row (t, i), t = 1 .. nt-1 (0-based slices), holds the columns of burgers_line_row_cols of slices t-1 and t,
// ascending
gmrf_status gmrf_burgers_p1_pattern(const gmrf_burgers_p1* b, int64_t* nnz_out, int64_t* rowptr, int64_t* colidx,
                                    int32_t index_base) {
    if (!b) return bad_shape("null handle");
    if (nnz_out) *nnz_out = b->nnz;
    if (rowptr) for (int64_t r = 0; r <= b->rows; ++r) rowptr[r] = b->rowptr[(size_t)r] + index_base;
    if (colidx && b->scheme == GMRF_BURGERS_COLLOCATION) {
        // row (t, c): the three dofs of the point's cell, ascending -- the wrap cell's right dof is column 0
        for (int64_t r = 0; r < b->rows; ++r) {
            const int64_t t = r / b->npts + 1, e = b->cell[(size_t)(r % b->npts)];
            const bool wrap = 2 * e + 2 == b->ns;
            const int64_t c[3] = {wrap ? 0 : 2 * e, wrap ? 2 * e : 2 * e + 1, wrap ? 2 * e + 1 : 2 * e + 2};
            int64_t* out = colidx + 6 * r;
            for (int k = 0; k < 3; ++k) { out[k] = (t - 1) * b->ns + c[k] + index_base; out[3 + k] = t * b->ns + c[k] + index_base; }
        }
    } else if (colidx)
        for (int64_t r = 0; r < b->rows; ++r) {
            const int64_t t = r / b->ns + 1;
            int64_t c[5];
            const int cnt = burgers_line_row_cols(b, r % b->ns, c);
            int64_t* out = colidx + b->rowptr[(size_t)r];
            for (int k = 0; k < cnt; ++k) { out[k] = (t - 1) * b->ns + c[k] + index_base; out[cnt + k] = t * b->ns + c[k] + index_base; }
        }
    return GMRF_OK;
}

// --------------------------------------------------------------------------------- batch forms of the Gauss-Newton glue
// Problem-major arrays ([batch][...]), host or device pointers; the one-problem calls are these at batch 1.
static bool batch_ok(int64_t batch) { return batch >= 1 && batch <= 4096; }

// Implicit Euler on the periodic unit line keeps the kernels of fem_assemble.hpp (and their bits), which know the cell length
// 1 / cells only; every other variant, another length included, is a burgers_line_rows instance.
static bool burgers_unit_euler_periodic(const gmrf_burgers_p1* b) {
    return b->scheme == GMRF_BURGERS_EULER && b->bc == GMRF_BURGERS_PERIODIC && b->h == 1.0 / (double)(b->ns / b->order);
}

static gmrf_status launch_tangent_batch(const gmrf_burgers_p1* b, hipStream_t st, int64_t batch, const double* d_w, double* d_vals,
                                        double* d_f) {
    const bool cn = b->scheme == GMRF_BURGERS_CN, dir = b->bc == GMRF_BURGERS_DIRICHLET, p2 = b->order == 2;
    const dim3 grid((unsigned)((b->rows + 255) / 256), (unsigned)batch);
    if (b->scheme == GMRF_BURGERS_COLLOCATION) {
        BurgersCollocArgs a;
        const double s = 4.0 / (b->h * b->h);
        a.ns = (int)b->ns; a.nt = (int)b->nt; a.npts = (int)b->npts; a.dt = b->dt; a.nu = b->nu;
        a.s[0] = s; a.s[1] = s; a.s[2] = -2.0 * s;
        a.cell = b->d_cell; a.a = b->d_shape; a.d = b->d_shape + 3 * b->npts; a.w = d_w; a.vals = d_vals; a.f = d_f;
        hipLaunchKernelGGL(burgers_colloc_rows, grid, dim3(256), 0, st, a);
    } else if (burgers_unit_euler_periodic(b)) {
        BurgersP1Args a;
        a.ns = (int)b->ns; a.nt = (int)b->nt; a.dt = b->dt; a.nu = b->nu; a.w = d_w; a.vals = d_vals; a.f = d_f;
        if (p2) hipLaunchKernelGGL(burgers_p2_rows_batch, grid, dim3(256), 0, st, a, b->nnz);
        else hipLaunchKernelGGL(burgers_p1_rows_batch, grid, dim3(256), 0, st, a, b->nnz);
    } else {
        BurgersLineArgs a;
        a.ns = (int)b->ns; a.nt = (int)b->nt; a.dt = b->dt; a.nu = b->nu; a.h = b->h; a.rowptr = b->d_rowptr; a.w = d_w; a.vals = d_vals; a.f = d_f;
        void (*kern)(BurgersLineArgs, int64_t) =
            p2 ? (cn ? (dir ? burgers_line_rows<2, true, true> : burgers_line_rows<2, true, false>)
                     : (dir ? burgers_line_rows<2, false, true> : burgers_line_rows<2, false, false>))
               : (cn ? (dir ? burgers_line_rows<1, true, true> : burgers_line_rows<1, true, false>)
                     : (dir ? burgers_line_rows<1, false, true> : burgers_line_rows<1, false, false>));
        hipLaunchKernelGGL(kern, grid, dim3(256), 0, st, a, b->nnz);
    }
    HIPCHK(hipGetLastError());
    return GMRF_OK;
}

// The body of gmrf_burgers_p1_tangent and its batch form after their argument checks; a one-problem call is a batch of 1.
static gmrf_status burgers_tangent_staged(gmrf_burgers_p1* b, int64_t batch, const double* w, double* vals_out, double* f_out) {
    GCHK(b->ready("pattern-only Burgers assembler"));
    const double* d_w;
    double *d_vals, *d_f;
    Staging args(b->arena);
    args.in(w, sizeof(double) * batch * b->ns * b->nt, &d_w);
    args.out(vals_out, sizeof(double) * batch * b->nnz, &d_vals);
    args.out(f_out, sizeof(double) * batch * b->rows, &d_f);
    GCHK(args.commit(b->stream));
    GCHK(launch_tangent_batch(b, b->stream, batch, d_w, d_vals, d_f));
    GCHK(args.flush(b->stream));
    HIPCHK(hipStreamSynchronize(b->stream));
    return GMRF_OK;
}

gmrf_status gmrf_burgers_p1_tangent(gmrf_burgers_p1* b, const double* w, double* vals_out, double* f_out) {
    if (!b || !w || !vals_out || !f_out) return bad_shape("bad Burgers tangent arguments");
    return burgers_tangent_staged(b, 1, w, vals_out, f_out);
}

gmrf_status gmrf_burgers_p1_tangent_batch(gmrf_burgers_p1* b, int64_t batch, const double* w, double* vals_out, double* f_out) {
    if (!b || !w || !vals_out || !f_out || !batch_ok(batch)) return bad_shape("bad Burgers tangent arguments (batch in [1, 4096])");
    return burgers_tangent_staged(b, batch, w, vals_out, f_out);
}

// --------------------------------------------------------------------------------- Burgers prior ("Prior" / "Initial condition" stages)
struct gmrf_burgers_prior : DevCtx {    // device -1: pattern only
    int64_t ns = 0, nt = 0, n = 0, nnz = 0;
    double dt = 0.0, nu = 0.0, ic_noise = 0.0;
    bool general = false;               // gmrf_burgers_line_prior_create's: `line` states it, burgers_line_prior.hpp evaluates it
    BurgersLinePriorArgs line{};
    DevBuf arena;                       // host arguments of the current call (Staging)
    DevBuf bulk;                        // [batch] means of a call that does not ask for them
};

// the pattern by its one statement: the P1 periodic prior's or the general line's
static int64_t prior_colptr(const gmrf_burgers_prior* p, int64_t j) {
    if (p->general) return burgers_line_prior_colptr(p->line, j / p->ns, j % p->ns);
    return burgers_prior_colptr(p->ns, p->nt, j / p->ns, j % p->ns);
}

static void prior_entry(const gmrf_burgers_prior* p, int64_t e, int64_t* row, int64_t* col) {
    if (p->general) burgers_line_prior_entry(p->line, e, row, col);
    else burgers_prior_entry(p->ns, p->nt, e, row, col);
}

gmrf_status gmrf_burgers_prior_create(int32_t device, void* stream, int64_t ns, int64_t nt, double dt, double nu, double ic_noise,
                                      gmrf_burgers_prior** out) {
    if (!out || nt < 2 || ns > (1 << 24) || nt > (1 << 20) || !(dt > 0.0) || !(nu > 0.0) || !(ic_noise >= 0.0) || !std::isfinite(ic_noise))
        return bad_shape("bad Burgers prior (nt >= 2 slices, dt > 0, nu > 0, ic_noise >= 0)");
    if (ns < 5) return bad_shape("the Burgers prior needs ns >= 5 nodes: fewer fold the periodic offsets 0, +-1, +-2 onto each other");
    std::unique_ptr<gmrf_burgers_prior, gmrf_status (*)(gmrf_burgers_prior*)> guard(new gmrf_burgers_prior(), gmrf_burgers_prior_destroy);
    gmrf_burgers_prior* p = guard.get();
    p->ns = ns; p->nt = nt; p->n = ns * nt; p->nnz = burgers_prior_nnz(ns, nt); p->dt = dt; p->nu = nu; p->ic_noise = ic_noise;
    GCHK(p->open(device, stream, hipStreamNonBlocking, "gmrf_burgers_prior_create"));
    *out = guard.release();
    return GMRF_OK;
}

gmrf_status gmrf_burgers_line_prior_create(int32_t device, void* stream, int64_t nc, int64_t nt, double dt, double nu, double ic_noise,
                                           int32_t order, int32_t bc, double length, double pin, int32_t ic_obs, gmrf_burgers_prior** out) {
    if (!out) return bad_shape("null pointer");
    if (order != 1 && order != 2) return bad_shape("Burgers line prior: order must be 1 or 2");
    if (bc != GMRF_BURGERS_PERIODIC && bc != GMRF_BURGERS_DIRICHLET) return bad_shape("Burgers line prior: bc must be GMRF_BURGERS_PERIODIC or GMRF_BURGERS_DIRICHLET");
    if (ic_obs != GMRF_BURGERS_IC_ALL && ic_obs != GMRF_BURGERS_IC_VERTICES) return bad_shape("Burgers line prior: ic_obs must be GMRF_BURGERS_IC_ALL or GMRF_BURGERS_IC_VERTICES");
    if (ic_obs == GMRF_BURGERS_IC_VERTICES && order != 2) return bad_shape("Burgers line prior: ic_obs = vertices needs order 2 (every dof of the P1 line is a vertex)");
    if (!(length > 0.0) || !std::isfinite(length)) return bad_shape("Burgers line prior: length must be > 0");
    if (!(nu > 0.0) || !std::isfinite(nu)) return bad_shape("Burgers line prior: nu must be > 0");
    if (!(dt > 0.0) || !std::isfinite(dt)) return bad_shape("Burgers line prior: dt must be > 0");
    if (!(pin >= 0.0) || !std::isfinite(pin)) return bad_shape("Burgers line prior: pin must be >= 0");
    if (!(ic_noise >= 0.0) || !std::isfinite(ic_noise)) return bad_shape("Burgers line prior: ic_noise must be >= 0");
    if (nt < 2 || nt > (1 << 20)) return bad_shape("Burgers line prior: nt must be >= 2 slices (and <= 2^20)");
    if (nc > (1 << 23)) return bad_shape("Burgers line prior: nc must be <= 2^23 cells");
    if (bc == GMRF_BURGERS_PERIODIC && order * nc < 4 * order + 1)
        return bad_shape("Burgers line prior: the periodic line needs order * nc >= 4 * order + 1 dofs: fewer fold the offsets 0 .. +-2 order onto each other");
    if (bc == GMRF_BURGERS_DIRICHLET && nc < 2) return bad_shape("Burgers line prior: the dirichlet line needs nc >= 2 cells");
    std::unique_ptr<gmrf_burgers_prior, gmrf_status (*)(gmrf_burgers_prior*)> guard(new gmrf_burgers_prior(), gmrf_burgers_prior_destroy);
    gmrf_burgers_prior* p = guard.get();
    BurgersLinePriorArgs& a = p->line;
    a.nc = nc; a.nt = nt; a.order = order; a.periodic = bc == GMRF_BURGERS_PERIODIC ? 1 : 0; a.vertices = ic_obs == GMRF_BURGERS_IC_VERTICES ? 1 : 0;
    a.ns = order * nc + (a.periodic ? 0 : 1);
    a.dt = dt; a.nu = nu; a.ic_noise = ic_noise; a.h = length / (double)nc; a.pin = a.periodic ? 0.0 : pin;
    p->general = true;
    p->ns = a.ns; p->nt = nt; p->n = a.ns * nt; p->nnz = burgers_line_prior_nnz(a); p->dt = dt; p->nu = nu; p->ic_noise = ic_noise;
    GCHK(p->open(device, stream, hipStreamNonBlocking, "gmrf_burgers_line_prior_create"));
    *out = guard.release();
    return GMRF_OK;
}

gmrf_status gmrf_burgers_prior_destroy(gmrf_burgers_prior* p) {
    if (!p) return GMRF_OK;
    p->close();
    delete p;
    return GMRF_OK;
}

// CSC pattern of Q_ic (symmetric, both triangles, rows ascending): burgers_prior_entry is its one statement
gmrf_status gmrf_burgers_prior_pattern(const gmrf_burgers_prior* p, int64_t* nnz_out, int64_t* colptr, int64_t* rowval, int32_t index_base) {
    if (!p) return bad_shape("null handle");
    if (index_base != 0 && index_base != 1) return bad_shape("index_base must be 0 or 1");
    if (nnz_out) *nnz_out = p->nnz;
    if (colptr) {
        for (int64_t j = 0; j < p->n; ++j) colptr[j] = prior_colptr(p, j) + index_base;
        colptr[p->n] = p->nnz + index_base;
    }
    if (rowval)
        for (int64_t e = 0; e < p->nnz; ++e) {
            int64_t row, col;
            prior_entry(p, e, &row, &col);
            rowval[e] = row + index_base;
        }
    return GMRF_OK;
}

static BurgersPriorArgs prior_args(const gmrf_burgers_prior* p) {
    BurgersPriorArgs a;
    a.ns = p->ns; a.nt = p->nt; a.dt = p->dt; a.nu = p->nu; a.ic_noise = p->ic_noise;
    return a;
}

// d_q / d_qx: nullptr = not wanted
static gmrf_status launch_prior_batch(const gmrf_burgers_prior* p, hipStream_t st, int64_t batch, const double* d_ic, double* d_bulk,
                                      double* d_q, double* d_qx) {
    if (p->general) {
        const BurgersLinePriorArgs& l = p->line;
        hipLaunchKernelGGL(burgers_line_bulk_batch, dim3(1, (unsigned)batch), dim3(256), 0, st, l, d_ic, d_bulk);
        if (d_q)
            hipLaunchKernelGGL(burgers_line_prior_values_batch, dim3((unsigned)((p->nnz + 255) / 256), (unsigned)batch), dim3(256), 0, st, l,
                               d_bulk, p->nnz, d_q);
        if (d_qx)
            hipLaunchKernelGGL(burgers_line_prior_rhs_batch, dim3((unsigned)((p->n + 255) / 256), (unsigned)batch), dim3(256), 0, st, l, d_bulk,
                               d_ic, d_qx);
        HIPCHK(hipGetLastError());
        return GMRF_OK;
    }
    const BurgersPriorArgs a = prior_args(p);
    hipLaunchKernelGGL(burgers_bulk_batch, dim3(1, (unsigned)batch), dim3(256), 0, st, d_ic, p->ns, d_bulk);
    if (d_q)
        hipLaunchKernelGGL(burgers_prior_values_batch, dim3((unsigned)((p->nnz + 255) / 256), (unsigned)batch), dim3(256), 0, st, a, d_bulk,
                           p->nnz, d_q);
    if (d_qx)
        hipLaunchKernelGGL(burgers_prior_rhs_batch, dim3((unsigned)((p->n + 255) / 256), (unsigned)batch), dim3(256), 0, st, a, d_bulk, d_ic,
                           d_qx);
    HIPCHK(hipGetLastError());
    return GMRF_OK;
}

gmrf_status gmrf_burgers_prior_values_batch(gmrf_burgers_prior* p, int64_t batch, const double* ic, double* bulk_out, double* q_values_out,
                                            double* qx_out) {
    if (!p || !ic || !batch_ok(batch)) return bad_shape("bad Burgers prior arguments (batch in [1, 4096])");
    GCHK(p->ready("pattern-only Burgers prior"));
    const double* d_ic;
    double *d_bulk, *d_q, *d_qx;
    Staging args(p->arena);
    args.in(ic, sizeof(double) * batch * p->ns, &d_ic);
    args.out(bulk_out, sizeof(double) * batch, &d_bulk);
    args.out(q_values_out, sizeof(double) * batch * p->nnz, &d_q);
    args.out(qx_out, sizeof(double) * batch * p->n, &d_qx);
    GCHK(args.commit(p->stream));
    if (!d_bulk) {
        GCHK(p->bulk.reserve(p->stream, sizeof(double) * batch));
        d_bulk = p->bulk.as<double>();
    }
    GCHK(launch_prior_batch(p, p->stream, batch, d_ic, d_bulk, d_q, d_qx));
    GCHK(args.flush(p->stream));
    HIPCHK(hipStreamSynchronize(p->stream));
    return GMRF_OK;
}

// --------------------------------------------------------------------------------- nonlinear elliptic tangent
struct gmrf_elliptic_p1 : DevCtx {      // device -1: pattern and quadrature points only
    int64_t nx = 0, ny = 0, n = 0, nnz = 0, cells = 0;
    int order = 1, nq = 3;              // element order and quadrature points per cell (order 2: the lattice of gmrf_darcy_p2_create, 4)
    std::vector<int64_t> rowptr, colidx;            // 0-based: the pattern of gmrf_darcy_p1_create / _p2_create(nx, ny)
    DevArr<int64_t> d_rowptr;
    DevBuf arena;                       // host arguments of the current call (Staging)
};

static gmrf_status elliptic_create(int32_t device, void* stream, int64_t nx, int64_t ny, int order, gmrf_elliptic_p1** out) {
    if (!out || nx < 2 || ny < 2 || nx > 32768 || ny > 32768 || (order == 2 && (nx > 16384 || ny > 16384))) return bad_shape("bad elliptic mesh size");
    std::unique_ptr<gmrf_elliptic_p1, gmrf_status (*)(gmrf_elliptic_p1*)> guard(new gmrf_elliptic_p1(), gmrf_elliptic_p1_destroy);
    gmrf_elliptic_p1* e = guard.get();
    e->nx = nx; e->ny = ny; e->cells = 2 * (nx - 1) * (ny - 1); e->order = order;
    if (order == 2) { e->n = (2 * nx - 1) * (2 * ny - 1); e->nq = 4; p2_lattice_pattern(nx, ny, e->rowptr, e->colidx); }
    else { e->n = nx * ny; e->nq = 3; p1_stencil_pattern(nx, ny, e->rowptr, e->colidx); }
    e->nnz = (int64_t)e->colidx.size();
    GCHK(e->open(device, stream, hipStreamNonBlocking, "gmrf_elliptic_p1_create"));
    if (e->device >= 0) {
        GCHK(e->d_rowptr.upload(e->stream, e->rowptr.data(), (size_t)(e->n + 1)));
        HIPCHK(hipStreamSynchronize(e->stream));
    }
    *out = guard.release();
    return GMRF_OK;
}

gmrf_status gmrf_elliptic_p1_create(int32_t device, void* stream, int64_t nx, int64_t ny, gmrf_elliptic_p1** out) {
    return elliptic_create(device, stream, nx, ny, 1, out);
}

gmrf_status gmrf_elliptic_p2_create(int32_t device, void* stream, int64_t nx, int64_t ny, gmrf_elliptic_p1** out) {
    return elliptic_create(device, stream, nx, ny, 2, out);
}

gmrf_status gmrf_elliptic_p1_destroy(gmrf_elliptic_p1* e) {
    if (!e) return GMRF_OK;
    e->close();
    delete e;
    return GMRF_OK;
}

gmrf_status gmrf_elliptic_p1_pattern(const gmrf_elliptic_p1* e, int64_t* nnz_out, int64_t* rowptr, int64_t* colidx, int32_t index_base) {
    if (!e) return bad_shape("null handle");
    if (nnz_out) *nnz_out = e->nnz;
    if (rowptr) for (int64_t i = 0; i <= e->n; ++i) rowptr[i] = e->rowptr[(size_t)i] + index_base;
    if (colidx) for (int64_t k = 0; k < e->nnz; ++k) colidx[k] = e->colidx[(size_t)k] + index_base;
    return GMRF_OK;
}

// spatial_coordinate(cellvalues, q_point, cell_coords) of every cell of the P1 triangle mesh under the symmetric 3-point rule:
// xy[cell][q][2] (shallow water :52, elliptic :206)
static void p1_triangle_qpoints(int64_t nx, int64_t ny, double* xy) {
    const int64_t nlow = (nx - 1) * (ny - 1);
    auto lin = [](int64_t i, int64_t n) { return (i == n - 1) ? 1.0 : (double)i * (1.0 / (double)(n - 1)); };
    const double bary[3][3] = {{1.0 / 6, 1.0 / 6, 2.0 / 3}, {1.0 / 6, 2.0 / 3, 1.0 / 6}, {2.0 / 3, 1.0 / 6, 1.0 / 6}};
    for (int up = 0; up < 2; ++up)
        for (int64_t qy = 0; qy < ny - 1; ++qy)
            for (int64_t qx = 0; qx < nx - 1; ++qx) {
                const int64_t cell = up * nlow + qy * (nx - 1) + qx;
                const int64_t nxs[3] = {qx, qx + 1, up ? qx : qx + 1}, nys[3] = {qy, up ? qy + 1 : qy, qy + 1};
                for (int q = 0; q < 3; ++q) {
                    xy[(cell * 3 + q) * 2 + 0] = (bary[q][0] * lin(nxs[0], nx) + bary[q][1] * lin(nxs[1], nx)) + bary[q][2] * lin(nxs[2], nx);
                    xy[(cell * 3 + q) * 2 + 1] = (bary[q][0] * lin(nys[0], ny) + bary[q][1] * lin(nys[1], ny)) + bary[q][2] * lin(nys[2], ny);
                }
            }
}

// The same for the quadratic triangles under the 4-point rule of fem_assemble_p2.hpp: xy[cell][q][2], the straight-sided cell's
// xi_x x_1 + xi_y x_2 + gamma x_3 in the unfused order of darcy_p2_row
static void p2_triangle_qpoints(int64_t nx, int64_t ny, double* xy) {
#pragma clang fp contract(off)
    const int64_t nlow = (nx - 1) * (ny - 1);
    auto lin = [](int64_t i, int64_t n) { return (i == n - 1) ? 1.0 : (double)i * (1.0 / (double)(n - 1)); };
    for (int up = 0; up < 2; ++up)
        for (int64_t qy = 0; qy < ny - 1; ++qy)
            for (int64_t qx = 0; qx < nx - 1; ++qx) {
                const int64_t cell = up * nlow + qy * (nx - 1) + qx;
                const int64_t vx[3] = {qx, qx + 1, up ? qx : qx + 1}, vy[3] = {qy, up ? qy + 1 : qy, qy + 1};
                const double x1 = lin(vx[0], nx), x2 = lin(vx[1], nx), x3 = lin(vx[2], nx);
                const double y1 = lin(vy[0], ny), y2 = lin(vy[1], ny), y3 = lin(vy[2], ny);
                for (int q = 0; q < 4; ++q) {
                    const double xx = p2_tri_qpoint(q).xi, xe = p2_tri_qpoint(q).eta, g = 1.0 - xx - xe;
                    const double t0 = xx * x1, t1 = xe * x2, t2 = g * x3, u0 = xx * y1, u1 = xe * y2, u2 = g * y3;      // (products first: no contraction)
                    xy[(cell * 4 + q) * 2 + 0] = (t0 + t1) + t2;
                    xy[(cell * 4 + q) * 2 + 1] = (u0 + u1) + u2;
                }
            }
}

gmrf_status gmrf_elliptic_p1_qpoints(const gmrf_elliptic_p1* e, double* xy) {
    if (!e || !xy) return bad_shape("null pointer");
    if (is_device_ptr(xy)) return bad_shape("quadrature points are written to host memory");
    if (e->order == 2) p2_triangle_qpoints(e->nx, e->ny, xy);
    else p1_triangle_qpoints(e->nx, e->ny, xy);
    return GMRF_OK;
}

static gmrf_status launch_elliptic_batch(const gmrf_elliptic_p1* e, hipStream_t st, int64_t batch, const double* d_w, double* d_vals,
                                         double* d_f) {
    const dim3 grid((unsigned)((e->n + 255) / 256), (unsigned)batch);
    auto launch = [&](auto kern, auto a) {
        a.nx = (int)e->nx; a.ny = (int)e->ny; a.rowptr = e->d_rowptr; a.w = d_w; a.vals = d_vals; a.f = d_f;
        hipLaunchKernelGGL(kern, grid, dim3(256), 0, st, a, e->nnz);
    };
    if (e->order == 2) launch(elliptic_p2_rows_batch, EllipticP2Args{});
    else launch(elliptic_p1_rows_batch, EllipticP1Args{});
    HIPCHK(hipGetLastError());
    return GMRF_OK;
}

// The body of gmrf_elliptic_p1_tangent and its batch form after their argument checks; a one-problem call is a batch of 1.
static gmrf_status elliptic_tangent_staged(gmrf_elliptic_p1* e, int64_t batch, const double* w, double* vals_out, double* f_out) {
    GCHK(e->ready("pattern-only elliptic tangent"));
    const double* d_w;
    double *d_vals, *d_f;
    Staging args(e->arena);
    args.in(w, sizeof(double) * batch * e->n, &d_w);
    args.out(vals_out, sizeof(double) * batch * e->nnz, &d_vals);
    args.out(f_out, sizeof(double) * batch * e->n, &d_f);
    GCHK(args.commit(e->stream));
    GCHK(launch_elliptic_batch(e, e->stream, batch, d_w, d_vals, d_f));
    GCHK(args.flush(e->stream));
    HIPCHK(hipStreamSynchronize(e->stream));
    return GMRF_OK;
}

gmrf_status gmrf_elliptic_p1_tangent(gmrf_elliptic_p1* e, const double* w, double* vals_out, double* f_out) {
    if (!e || !w || !vals_out || !f_out) return bad_shape("bad elliptic tangent arguments");
    return elliptic_tangent_staged(e, 1, w, vals_out, f_out);
}

gmrf_status gmrf_elliptic_p1_tangent_batch(gmrf_elliptic_p1* e, int64_t batch, const double* w, double* vals_out, double* f_out) {
    if (!e || !w || !vals_out || !f_out || !batch_ok(batch)) return bad_shape("bad elliptic tangent arguments (batch in [1, 4096])");
    return elliptic_tangent_staged(e, batch, w, vals_out, f_out);
}

// src_q [batch][cells][nq] -> b_out [batch][n]
gmrf_status gmrf_elliptic_p1_load(gmrf_elliptic_p1* e, int64_t batch, const double* src_q, double* b_out) {
    if (!e || !src_q || !b_out || !batch_ok(batch)) return bad_shape("bad elliptic load arguments (batch in [1, 4096])");
    GCHK(e->ready("pattern-only elliptic tangent"));
    const double* d_src;
    double* d_b;
    Staging args(e->arena);
    args.in(src_q, sizeof(double) * batch * e->cells * e->nq, &d_src);
    args.out(b_out, sizeof(double) * batch * e->n, &d_b);
    GCHK(args.commit(e->stream));
    const dim3 grid((unsigned)((e->n + 255) / 256), (unsigned)batch);
    auto launch = [&](auto kern, auto a) {
        a.nx = (int)e->nx; a.ny = (int)e->ny; a.src = d_src; a.b = d_b;
        hipLaunchKernelGGL(kern, grid, dim3(256), 0, e->stream, a);
    };
    if (e->order == 2) launch(elliptic_p2_load_batch, EllipticP2LoadArgs{});
    else launch(elliptic_p1_load_batch, EllipticLoadArgs{});
    HIPCHK(hipGetLastError());
    GCHK(args.flush(e->stream));
    HIPCHK(hipStreamSynchronize(e->stream));
    return GMRF_OK;
}

// Darcy element kernels for a batch of coefficient tables (problem-major); d_work: [batch][n] |diagonal| then [batch] means
static int64_t darcy_batch_work_elems(const gmrf_darcy_p1* d, int64_t batch) { return batch * d->n + batch; }

static gmrf_status launch_darcy_batch(const gmrf_darcy_p1* d, hipStream_t st, int64_t batch, const double* d_tab, int64_t ng, double beta,
                                      double* d_vals, double* d_f, double* d_work) {
    double* d_diag = d_work;
    double* d_mean = d_work + batch * d->n;
    const dim3 grid((unsigned)((d->n + 255) / 256), (unsigned)batch);
    auto fill = [&](auto a) {
        a.nx = (int)d->nx; a.ny = (int)d->ny; a.ng = (int)ng; a.table = d_tab; a.rowptr = d->d_rowptr; a.beta = beta;
        a.vals = d_vals; a.f = d_f; a.diag = d_diag;
        return a;
    };
    if (d->order == 2) {
        hipLaunchKernelGGL(darcy_p2_rows_batch, grid, dim3(256), 0, st, fill(DarcyP2Args{}), d->nnz);
        hipLaunchKernelGGL(darcy_meandiag_batch, dim3((unsigned)batch), dim3(256), 0, st, d_diag, d->n, d_mean);
        hipLaunchKernelGGL(darcy_p2_constrain_batch, grid, dim3(256), 0, st, d->d_rowptr, d->d_colidx, d->d_pres, d->n, d->nnz, d_mean,
                           d_vals, d_f);
    } else {
        const DarcyP1Args a = fill(DarcyP1Args{});
        hipLaunchKernelGGL(darcy_p1_rows_batch, grid, dim3(256), 0, st, a, d->nnz);
        hipLaunchKernelGGL(darcy_meandiag_batch, dim3((unsigned)batch), dim3(256), 0, st, d_diag, d->n, d_mean);
        hipLaunchKernelGGL(darcy_p1_constrain_batch, grid, dim3(256), 0, st, a, d->nnz, d_mean);
    }
    HIPCHK(hipGetLastError());
    return GMRF_OK;
}

// The body of gmrf_darcy_p1_assemble and its batch form after their argument checks; a one-problem call is a batch of 1.
static gmrf_status darcy_assemble_staged(gmrf_darcy_p1* d, int64_t batch, const double* coeff_tables, int64_t ng, double beta,
                                         double* vals_out, double* f_out) {
    GCHK(d->ready("pattern-only Darcy assembler"));
    const double* d_tab;
    double *d_vals, *d_f;
    Staging args(d->arena);
    args.in(coeff_tables, sizeof(double) * batch * ng * ng, &d_tab);
    args.out(vals_out, sizeof(double) * batch * d->nnz, &d_vals);
    args.out(f_out, sizeof(double) * batch * d->n, &d_f);
    GCHK(args.commit(d->stream));
    GCHK(d->bwork.reserve(d->stream, sizeof(double) * darcy_batch_work_elems(d, batch)));
    GCHK(launch_darcy_batch(d, d->stream, batch, d_tab, ng, beta, d_vals, d_f, d->bwork.as<double>()));
    GCHK(args.flush(d->stream));
    HIPCHK(hipStreamSynchronize(d->stream));
    return GMRF_OK;
}

gmrf_status gmrf_darcy_p1_assemble_batch(gmrf_darcy_p1* d, int64_t batch, const double* coeff_tables, int64_t ng, double beta,
                                         double* vals_out, double* f_out) {
    if (!d || !coeff_tables || !vals_out || !f_out || !batch_ok(batch) || !darcy_ng_ok(ng))
        return bad_shape("bad Darcy assembly arguments (batch in [1, 4096], ng in [2, 46340])");
    return darcy_assemble_staged(d, batch, coeff_tables, ng, beta, vals_out, f_out);
}

static gmrf_status launch_precision_batch(const gmrf_assembler* as, hipStream_t st, int64_t batch, const double* d_q, int64_t q_stride,
                                          const double* d_jv, double noise, double* d_out) {
    hipLaunchKernelGGL(assemble_precision_batch, dim3((unsigned)((as->nnz_out + 255) / 256), (unsigned)batch), dim3(256), 0, st,
                       as->d_pptr, as->d_pa, as->d_pb, as->d_qmap, d_q, q_stride, d_jv, as->nnz_j, noise, as->nnz_out, d_out);
    HIPCHK(hipGetLastError());
    return GMRF_OK;
}

// d_v: [batch][m] work array (J x + obs_diff)
static gmrf_status launch_rhs_batch(const gmrf_assembler* as, hipStream_t st, int64_t batch, const double* d_base, const double* d_jv,
                                    const double* d_x, const double* d_add, double noise, double* d_v, double* d_out) {
    hipLaunchKernelGGL(assemble_j_apply_batch, dim3((unsigned)((as->m + 255) / 256), (unsigned)batch), dim3(256), 0, st, as->d_j_rptr,
                       as->d_j_col, d_jv, as->nnz_j, d_x, as->n, d_add, as->m, d_v);
    hipLaunchKernelGGL(assemble_jt_apply_batch, dim3((unsigned)((as->n + 255) / 256), (unsigned)batch), dim3(256), 0, st, as->d_jt_ptr,
                       as->d_jt_row, as->d_jt_src, d_jv, as->nnz_j, d_v, as->m, d_base, noise, as->n, d_out);
    HIPCHK(hipGetLastError());
    return GMRF_OK;
}

// chunks of the objective's fixed partition: a function of n and m only
static int64_t objective_chunks(const gmrf_assembler* as) {
    return std::min<int64_t>(1024, std::max<int64_t>(1, (std::max(as->n, as->m) + 2047) / 2048));
}

static gmrf_status objective_ready(gmrf_assembler* as) {
    if (as->d_q_ptr && as->d_q_row) return GMRF_OK;
    if (as->q_ptr.empty()) return bad_shape("the objective needs n < 2^31");
    GCHK(reserve_group(as->stream, {as->d_q_ptr.want(as->q_ptr.size()), as->d_q_row.want(as->q_row.size())}));
    GCHK(as->d_q_ptr.upload(as->stream, as->q_ptr));
    GCHK(as->d_q_row.upload(as->stream, as->q_row));
    HIPCHK(hipStreamSynchronize(as->stream));
    return GMRF_OK;
}

// d_part: [batch][objective_chunks] work array
static gmrf_status launch_objective_batch(const gmrf_assembler* as, hipStream_t st, int64_t batch, const double* d_q, int64_t q_stride,
                                          const double* d_xp, const double* d_x, const double* d_o, double noise, double* d_part,
                                          double* d_obj) {
    const int64_t nch = objective_chunks(as), len_n = (as->n + nch - 1) / nch, len_m = (as->m + nch - 1) / nch;
    hipLaunchKernelGGL(gn_objective_part, dim3((unsigned)nch, (unsigned)batch), dim3(256), 0, st, as->d_q_ptr, as->d_q_row, d_q, q_stride,
                       d_xp, d_x, as->n, d_o, as->m, noise, len_n, len_m, d_part);
    hipLaunchKernelGGL(pattern_dot_sum, dim3(1, (unsigned)batch), dim3(256), 0, st, d_part, nch, (int64_t)1, d_obj);
    HIPCHK(hipGetLastError());
    return GMRF_OK;
}

static gmrf_status q_stride_ok(const gmrf_assembler* as, int64_t q_stride) {
    if (q_stride != 0 && q_stride != as->nnz_q) return bad_shape("q_stride must be 0 (one Q for all problems) or nnz(Q)");
    return GMRF_OK;
}

// The bodies of the assembly calls after their argument checks; a one-problem call is a batch of 1.
static gmrf_status assemble_precision_staged(gmrf_assembler* as, int64_t batch, const double* q_nzval, int64_t q_stride,
                                             const double* j_vals, double noise, double* out_nzval) {
    const double *d_q, *d_jv;
    double* d_out;
    Staging args(as->arena);
    args.in(q_nzval, sizeof(double) * (q_stride ? batch * as->nnz_q : as->nnz_q), &d_q);
    args.in(j_vals, sizeof(double) * batch * as->nnz_j, &d_jv);
    args.out(out_nzval, sizeof(double) * batch * as->nnz_out, &d_out);
    GCHK(args.commit(as->stream));
    GCHK(launch_precision_batch(as, as->stream, batch, d_q, q_stride, d_jv, noise, d_out));
    GCHK(args.flush(as->stream));
    HIPCHK(hipStreamSynchronize(as->stream));
    return GMRF_OK;
}

static gmrf_status assemble_rhs_staged(gmrf_assembler* as, int64_t batch, const double* base, const double* j_vals, const double* x,
                                       const double* obs_diff, double noise, double* out) {
    const double *d_base, *d_jv, *d_x, *d_add;
    double* d_out;
    Staging args(as->arena);
    args.in(base, sizeof(double) * batch * as->n, &d_base);
    args.in(j_vals, sizeof(double) * batch * as->nnz_j, &d_jv);
    args.in(x, sizeof(double) * batch * as->n, &d_x);
    args.in(obs_diff, sizeof(double) * batch * as->m, &d_add);
    args.out(out, sizeof(double) * batch * as->n, &d_out);
    GCHK(args.commit(as->stream));
    GCHK(as->bpart.reserve(as->stream, sizeof(double) * batch * as->m));
    GCHK(launch_rhs_batch(as, as->stream, batch, d_base, d_jv, d_x, d_add, noise, as->bpart.as<double>(), d_out));
    GCHK(args.flush(as->stream));
    HIPCHK(hipStreamSynchronize(as->stream));
    return GMRF_OK;
}

gmrf_status gmrf_assemble_precision_batch(gmrf_assembler* as, int64_t batch, const double* q_nzval, int64_t q_stride,
                                          const double* j_vals, double noise, double* out_nzval) {
    if (!as || !q_nzval || !j_vals || !out_nzval || !batch_ok(batch)) return bad_shape("null pointer or batch outside [1, 4096]");
    GCHK(q_stride_ok(as, q_stride));
    GCHK(as->ready(AS_PATTERN_ONLY));
    return assemble_precision_staged(as, batch, q_nzval, q_stride, j_vals, noise, out_nzval);
}

gmrf_status gmrf_assemble_rhs_batch(gmrf_assembler* as, int64_t batch, const double* base, const double* j_vals, const double* x,
                                    const double* obs_diff, double noise, double* out) {
    if (!as || !j_vals || !x || !out || !batch_ok(batch)) return bad_shape("null pointer or batch outside [1, 4096]");
    GCHK(as->ready(AS_PATTERN_ONLY));
    return assemble_rhs_staged(as, batch, base, j_vals, x, obs_diff, noise, out);
}

gmrf_status gmrf_assemble_objective_batch(gmrf_assembler* as, int64_t batch, const double* q_nzval, int64_t q_stride,
                                          const double* x_prior, const double* x, const double* obs_diff, double noise,
                                          double* obj_out) {
    if (!as || !q_nzval || !x_prior || !x || !obs_diff || !obj_out || !batch_ok(batch)) return bad_shape("null pointer or batch outside [1, 4096]");
    GCHK(q_stride_ok(as, q_stride));
    GCHK(as->ready(AS_PATTERN_ONLY));
    GCHK(objective_ready(as));
    const double *d_q, *d_xp, *d_x, *d_o;
    double* d_obj;
    Staging args(as->arena);
    args.in(q_nzval, sizeof(double) * (q_stride ? batch * as->nnz_q : as->nnz_q), &d_q);
    args.in(x_prior, sizeof(double) * batch * as->n, &d_xp);
    args.in(x, sizeof(double) * batch * as->n, &d_x);
    args.in(obs_diff, sizeof(double) * batch * as->m, &d_o);
    args.out(obj_out, sizeof(double) * batch, &d_obj);
    GCHK(args.commit(as->stream));
    GCHK(as->bpart.reserve(as->stream, sizeof(double) * batch * objective_chunks(as)));
    GCHK(launch_objective_batch(as, as->stream, batch, d_q, q_stride, d_xp, d_x, d_o, noise, as->bpart.as<double>(), d_obj));
    GCHK(args.flush(as->stream));
    HIPCHK(hipStreamSynchronize(as->stream));
    return GMRF_OK;
}

// chunks of the fixed partition of a sum over n elements (std_norm_part, quadform_part): a function of n only
static int64_t std_norm_chunks(int64_t n) { return std::min<int64_t>(1024, std::max<int64_t>(1, (n + 2047) / 2048)); }

static gmrf_status quadform_ready(gmrf_assembler* as) {
    if (as->d_o_ptr && as->d_o_row) return GMRF_OK;
    if (as->n >= ((int64_t)1 << 31)) return bad_shape("the quadratic form needs n < 2^31");
    const std::vector<int32_t> row(as->rowval.begin(), as->rowval.end());
    GCHK(reserve_group(as->stream, {as->d_o_ptr.want(as->colptr.size()), as->d_o_row.want(row.size())}));
    GCHK(as->d_o_ptr.upload(as->stream, as->colptr));
    GCHK(as->d_o_row.upload(as->stream, row));
    HIPCHK(hipStreamSynchronize(as->stream));        // (`row` goes with this scope)
    return GMRF_OK;
}

// d_part: [batch][std_norm_chunks(n)] work array; quadform_ready(as) has run
static gmrf_status launch_quadform_batch(const gmrf_assembler* as, hipStream_t st, int64_t batch, const double* d_a, int64_t a_stride,
                                         const double* d_x, const double* d_z, double* d_part, double* d_out) {
    const int64_t nch = std_norm_chunks(as->n), len = (as->n + nch - 1) / nch;
    hipLaunchKernelGGL(quadform_part, dim3((unsigned)nch, (unsigned)batch), dim3(256), 0, st, as->d_o_ptr, as->d_o_row, d_a, a_stride, d_x,
                       d_z, as->n, len, d_part);
    hipLaunchKernelGGL(pattern_dot_sum, dim3(1, (unsigned)batch), dim3(256), 0, st, d_part, nch, (int64_t)1, d_out);
    HIPCHK(hipGetLastError());
    return GMRF_OK;
}

gmrf_status gmrf_assemble_quadform_batch(gmrf_assembler* as, int64_t batch, const double* a_nzval, int64_t a_stride, const double* x,
                                         const double* z, double* out) {
    if (!as || !a_nzval || !x || !z || !out || !batch_ok(batch)) return bad_shape("null pointer or batch outside [1, 4096]");
    if (a_stride != 0 && a_stride != as->nnz_out) return bad_shape("a_stride must be 0 (one A for all problems) or nnz of the assembled pattern");
    GCHK(as->ready(AS_PATTERN_ONLY));
    GCHK(quadform_ready(as));
    const double *d_a, *d_x, *d_z;
    double* d_out;
    Staging args(as->arena);
    args.in(a_nzval, sizeof(double) * (a_stride ? batch * as->nnz_out : as->nnz_out), &d_a);
    args.in(x, sizeof(double) * batch * as->n, &d_x);
    args.in(z, sizeof(double) * batch * as->n, &d_z);
    args.out(out, sizeof(double) * batch, &d_out);
    GCHK(args.commit(as->stream));
    GCHK(as->bpart.reserve(as->stream, sizeof(double) * batch * std_norm_chunks(as->n)));
    GCHK(launch_quadform_batch(as, as->stream, batch, d_a, a_stride, d_x, d_z, as->bpart.as<double>(), d_out));
    GCHK(args.flush(as->stream));
    HIPCHK(hipStreamSynchronize(as->stream));
    return GMRF_OK;
}

// --------------------------------------------------------------------------------- what the batched drivers share
// gmrf_gn, gmrf_dc and gmrf_bic bind a handle and an assembler (and one more object of their own) that live on one device and
// stream, keep their device buffers in one carved allocation, and run with a buffer of theirs registered as the factor's rhs.
struct DriverBase {
    gmrf_handle* h = nullptr;
    gmrf_assembler* as = nullptr;
    int device = 0;                      // (copies: a destroy does not reach into the handle)
    hipStream_t stream = nullptr;
    DevBuf in;                           // arena of a run's host arguments (Staging)
    DevBuf work;                         // every device buffer of the driver, carved up by its *_alloc
    int64_t B = 0;                       // the batch `work` is carved for
    gmrf_csr* Qp = nullptr;              // the posterior pattern as a CSR matrix (tile plan of the RBMC product), made by the first RBMC run

    void bind(gmrf_handle* handle, gmrf_assembler* assembler) { h = handle; as = assembler; device = handle->device; stream = handle->stream; }
    void close() {
        (void)hipSetDevice(device);
        (void)hipStreamSynchronize(stream);
        if (Qp) (void)gmrf_csr_destroy(Qp);
        Qp = nullptr;
    }
};

// The driver's `rhs` is the factor's registered right-hand side (gmrf_bt_set_factor_rhs) while this lives: where that route
// qualifies the factorisation leaves y = L^-1 rhs.  The caller's registration comes back on every way out.
struct FactorRhsScope {
    gmrf_handle* h;
    const double* saved;
    FactorRhsScope(gmrf_handle* handle, const double* rhs) : h(handle), saved(handle->frhs) { h->frhs = rhs; h->fy_for = nullptr; }
    ~FactorRhsScope() { h->frhs = saved; h->fy_for = nullptr; }
    FactorRhsScope(const FactorRhsScope&) = delete;
    FactorRhsScope& operator=(const FactorRhsScope&) = delete;
};

// a driver's result to the caller's host or device array; null: not wanted
static gmrf_status copy_out(hipStream_t st, void* dst, const void* src, size_t bytes) {
    if (!dst) return GMRF_OK;
    HIPCHK(hipMemcpyAsync(dst, src, bytes, is_device_ptr(dst) ? hipMemcpyDeviceToDevice : hipMemcpyDeviceToHost, st));
    return GMRF_OK;
}

// The binding checks every driver makes.  `peer` names the driver's third object, which lives on (peer_device, peer_stream).
static gmrf_status driver_same_device_stream(const DriverBase* g, int peer_device, hipStream_t peer_stream, const char* peer) {
    const gmrf_handle* h = g->h;
    if (g->as->device != h->device || peer_device != h->device)
        return bad_shape((std::string("handle, assembler and ") + peer + " must live on one device").c_str());
    if (g->as->stream != h->stream || peer_stream != h->stream)
        return bad_shape((std::string("handle, assembler and ") + peer + " must share one stream").c_str());
    return GMRF_OK;
}
// ... and, after its own pattern comparison: a handle that has analysed a pattern has analysed the assembler's
static gmrf_status driver_analysis_ok(const DriverBase* g) {
    if (g->h->analyzed && (g->h->n != g->as->n || g->h->nnz_in != g->as->nnz_out)) return bad_shape("the handle has not analysed the assembler's pattern");
    return GMRF_OK;
}

// the posterior pattern (symmetric: the assembler's CSC arrays read by rows) as the matrix whose tile plan the RBMC product uses
static gmrf_status driver_pattern_csr(DriverBase* g) {
    if (g->Qp) return GMRF_OK;
    const gmrf_assembler* as = g->as;
    const std::vector<double> ones((size_t)std::max<int64_t>(as->nnz_out, 1), 1.0);
    return gmrf_csr_create(g->h->device, (void*)g->h->stream, as->n, as->n, as->colptr.data(), as->rowval.data(), ones.data(), 0, 0, &g->Qp);
}

static gmrf_status var_batch_enqueue(gmrf_handle* h, int method, int64_t k, uint64_t seed, const gmrf_csr* Q, const double* qv,
                                     double* d_diag, double* d_var);

// The variance tail of a driver's stage on the factor its handle holds: d_var [B][n] <- the marginal variances by var_method
// (-1: nothing is done), the sampled estimators on the posterior values d_nz [B][nnz] just assembled, with d_diag [B][n] as work
// and driver_pattern_csr made for RBMC.  Behind the public calls' own abort-and-repeat guard.
static gmrf_status driver_variances(DriverBase* g, int32_t var_method, int64_t k_var, uint64_t var_seed, const double* d_nz,
                                    double* d_diag, double* d_var) {
    gmrf_handle* h = g->h;
    if (var_method == GMRF_VAR_EXACT) return gmrf_bt_marginal_var(h, GMRF_VAR_EXACT, 0, 0, nullptr, d_var);
    if (var_method != GMRF_VAR_RBMC && var_method != GMRF_VAR_MC) return GMRF_OK;
    return sweep_guarded(h, {}, [&]() -> gmrf_status {     // (a batch of one: its sweeps may be persistent launches)
        GCHK(var_batch_enqueue(h, var_method, k_var, var_seed, g->Qp, d_nz, d_diag, d_var));
        HIPCHK(hipStreamSynchronize(h->stream));
        return GMRF_OK;
    });
}

// ... and its last line: std = sqrt(var) in place, d_norm [B] <- |std_p|_2; d_part: [B][std_norm_chunks(n)] work
static gmrf_status driver_std_norm(const DriverBase* g, double* d_var, double* d_part, double* d_norm) {
    const int64_t n = g->as->n, B = g->h->B, nch = std_norm_chunks(n), len = (n + nch - 1) / nch;
    hipLaunchKernelGGL(std_norm_part, dim3((unsigned)nch, (unsigned)B), dim3(256), 0, g->h->stream, d_var, n, len, d_part);
    hipLaunchKernelGGL(std_norm_finish, dim3(1, (unsigned)B), dim3(256), 0, g->h->stream, d_part, nch, d_norm);
    HIPCHK(hipGetLastError());
    return GMRF_OK;
}

// --------------------------------------------------------------------------------- the batched Gauss-Newton driver
// B = batch of the handle Burgers problems on one mesh in lock step (scripts/solve_burger.jl:151-180 per problem).  One iteration
// on the handle's stream:
//     tangent(x) -> A = Q + noise J'J, rhs -> gmrf_bt_refactor_values -> solve -> tangent(candidate) -> objective -> stop rule
// The rhs buffer is registered as the factor's right-hand side (gmrf_bt_set_factor_rhs) for the run: where that route
// qualifies the factorisation leaves y = L^-1 rhs and the solve is the backward sweep alone.  Problems that have stopped stay in
// the batch, frozen: their x does not change, so they are re-factored with the same values.
struct gmrf_gn : DriverBase {
    gmrf_burgers_p1* b = nullptr;        // the bound tangent: Burgers (gmrf_gn_create) ...
    gmrf_elliptic_p1* e = nullptr;       // ... or nonlinear elliptic (gmrf_gn_create_elliptic); exactly one is set
    int32_t hist_steps = -1;             // the steps `work` is carved for
    double *d_x = nullptr, *d_xn = nullptr, *d_od = nullptr, *d_on = nullptr, *d_f = nullptr, *d_v = nullptr, *d_jv = nullptr;
    double *d_a = nullptr, *d_rhs = nullptr, *d_q = nullptr, *d_part = nullptr, *d_obj = nullptr;
    double *d_last = nullptr, *d_cur = nullptr, *d_hist = nullptr;
    int32_t *d_steps = nullptr, *d_active = nullptr, *d_take = nullptr;
    HostWord h_active;                   // mapped host word the stop rule writes
    unsigned* dev_active = nullptr;      // ... as the device addresses it
    int64_t q_stride = 0;
    double noise = 0.0;
    bool have_x = false;                 // a run has left its iterate in d_x (gmrf_gn_finalize)
    int32_t iterations = 0, fwd_iterations = 0;      // of the last run: iterations, and those whose solve was the backward sweep alone
    // the posterior stage (gmrf_gn_posterior): buffers of its own, carved for (post_B, post_ks); the run's layout is not touched
    DevBuf post;
    int64_t post_B = 0, post_ks = -1;
    double *d_smp = nullptr, *d_var = nullptr, *d_diag = nullptr, *d_spart = nullptr, *d_norm = nullptr;
    double *d_ld = nullptr, *d_sq = nullptr, *d_nll = nullptr, *d_err = nullptr, *d_epart = nullptr;
};

// The one place that knows which tangent is bound: its device, stream and the shape of its J, and its batch launch.
struct GnTangent { int device; hipStream_t stream; int64_t n, m, nnz; };
static GnTangent gn_tangent(const gmrf_gn* g) {
    if (g->e) return {g->e->device, g->e->stream, g->e->n, g->e->n, g->e->nnz};
    return {g->b->device, g->b->stream, g->b->ns * g->b->nt, g->b->rows, g->b->nnz};
}
static gmrf_status gn_launch_tangent(const gmrf_gn* g, hipStream_t st, int64_t batch, const double* d_w, double* d_vals, double* d_f) {
    return g->e ? launch_elliptic_batch(g->e, st, batch, d_w, d_vals, d_f) : launch_tangent_batch(g->b, st, batch, d_w, d_vals, d_f);
}

static gmrf_status gn_bound_ok(const gmrf_gn* g) {
    const gmrf_handle* h = g->h;
    const GnTangent t = gn_tangent(g);
    if (h->order == GMRF_ORDER_TWISTED) return bad_shape("the Gauss-Newton driver takes a reference-order handle");
    GCHK(driver_same_device_stream(g, t.device, t.stream, "tangent"));
    if (g->as->n != t.n || g->as->m != t.m || g->as->nnz_j != t.nnz)
        return bad_shape("the assembler's J is not the tangent's pattern");
    return GMRF_OK;
}

static gmrf_status gn_create(gmrf_handle* h, gmrf_assembler* as, gmrf_burgers_p1* b, gmrf_elliptic_p1* el, gmrf_gn** out) {
    if (!h || !as || (!b && !el) || !out) return bad_shape("null pointer");
    if (as->device < 0 || (b ? b->device : el->device) < 0) return bad_shape("the Gauss-Newton driver needs an assembler and a tangent with a device");
    auto g = std::make_unique<gmrf_gn>();
    g->bind(h, as); g->b = b; g->e = el;
    GCHK(gn_bound_ok(g.get()));
    HIPCHK(hipSetDevice(h->device));
    void* dev_word = nullptr;
    hipError_t e = g->h_active.open();
    if (e == hipSuccess) e = hipHostGetDevicePointer(&dev_word, g->h_active, 0);
    if (e != hipSuccess) { g_last_error = std::string("gmrf_gn_create: ") + hipGetErrorString(e); return GMRF_ERR_HIP; }
    g->dev_active = static_cast<unsigned*>(dev_word);
    *out = g.release();
    return GMRF_OK;
}

gmrf_status gmrf_gn_create(gmrf_handle* h, gmrf_assembler* as, gmrf_burgers_p1* b, gmrf_gn** out) {
    return gn_create(h, as, b, nullptr, out);
}
gmrf_status gmrf_gn_create_elliptic(gmrf_handle* h, gmrf_assembler* as, gmrf_elliptic_p1* e, gmrf_gn** out) {
    return gn_create(h, as, nullptr, e, out);
}

gmrf_status gmrf_gn_destroy(gmrf_gn* g) {
    if (!g) return GMRF_OK;
    g->close();
    delete g;
    return GMRF_OK;
}

static gmrf_status gn_alloc(gmrf_gn* g, int64_t B, int32_t max_steps) {
    const gmrf_assembler* as = g->as;
    if (g->B == B && g->hist_steps >= max_steps) return GMRF_OK;
    g->B = 0; g->hist_steps = -1; g->have_x = false;     // (the iterate of an earlier run goes with its layout)
    const int64_t n = as->n, m = as->m;
    auto lay = [&](char* base) {
        Carve c{base};
        c(&g->d_x, B * n); c(&g->d_xn, B * n); c(&g->d_rhs, B * n);
        c(&g->d_od, B * m); c(&g->d_on, B * m); c(&g->d_f, B * m); c(&g->d_v, B * m);
        c(&g->d_jv, B * as->nnz_j); c(&g->d_a, B * as->nnz_out); c(&g->d_q, B * as->nnz_q);
        c(&g->d_part, B * objective_chunks(as)); c(&g->d_obj, B);
        c(&g->d_last, B); c(&g->d_cur, B); c(&g->d_hist, B * ((int64_t)max_steps + 1));
        c(&g->d_steps, B); c(&g->d_active, B); c(&g->d_take, B);
        return c.used;
    };
    GCHK(g->work.reserve(g->h->stream, lay(nullptr)));
    lay(g->work.as<char>());
    GCHK(g->in.reserve(g->h->stream, 2 * Staging::padded(sizeof(double) * B * n) + Staging::padded(sizeof(double) * B * m)));      // qx_prior, x_prior, y
    g->B = B; g->hist_steps = max_steps;
    return GMRF_OK;
}

// A^-1 d_rhs -> d_out on the handle's stream.  The factorisation of the registered rhs left y = L^-1 rhs (fy_for): the backward sweep
// of a copy of y is the whole solve; else both sweeps.  A batch's sweeps are never persistent launches, so nothing is waited for;
// one problem goes through the guard of the persistent sweeps and ends in the stream's synchronisation.  *took_y: which it was.
static gmrf_status solve_registered(gmrf_handle* h, const double* d_rhs, double* d_out, bool* took_y) {
    const int64_t vec_bytes = h->n * h->B * (int64_t)sizeof(double);
    return sweep_guarded(h, {{d_rhs, vec_bytes, d_out, vec_bytes}}, [&]() -> gmrf_status {
        GCHK(ensure_panels(h, 1));
        const bool have_y = h->fy_for && h->fy_for == d_rhs;
        *took_y = have_y;
        if (have_y) {
            HIPCHK(hipMemcpyAsync(h->d_P, h->d_fy, sizeof(double) * (size_t)(h->B * h->n_pad), hipMemcpyDeviceToDevice, h->stream));
            GCHK(run_sweeps(h, GMRF_SOLVE_BACKWARD, 1));
            GCHK(launch_unpack(h, h->d_Y, d_out, h->n, 1, nullptr));
        } else {
            GCHK(launch_pack(h, d_rhs, h->n, 1, 1));
            GCHK(run_sweeps(h, GMRF_SOLVE_FULL, 1));
            GCHK(launch_unpack(h, h->d_P, d_out, h->n, 1, nullptr));
        }
        if (h->B == 1) HIPCHK(hipStreamSynchronize(h->stream));
        return GMRF_OK;
    });
}

static gmrf_status gn_solve(gmrf_gn* g) {
    bool took_y = false;
    GCHK(solve_registered(g->h, g->d_rhs, g->d_xn, &took_y));
    if (took_y) g->fwd_iterations += 1;
    return GMRF_OK;
}

static GnState gn_state(const gmrf_gn* g) {
    GnState s;
    s.last = g->d_last; s.cur = g->d_cur; s.steps = g->d_steps; s.active = g->d_active; s.take = g->d_take; s.hist = g->d_hist;
    s.host_active = g->dev_active;
    return s;
}

gmrf_status gmrf_gn_run(gmrf_gn* g, const double* q_nzval, int64_t q_stride, const double* qx_prior, const double* x_prior, double* x,
                        const double* y, double noise, double rtol, int32_t max_steps, int32_t* steps_out, double* obj_hist_out,
                        int32_t* info) {
    if (!g || !q_nzval || !qx_prior || !x_prior || !x) return bad_shape("null pointer");
    if (info) *info = 0;
    gmrf_handle* h = g->h;
    gmrf_assembler* as = g->as;
    GCHK(gn_bound_ok(g));
    GCHK(q_stride_ok(as, q_stride));
    if (max_steps < 0 || max_steps > (1 << 20) || !(rtol >= 0.0)) return bad_shape("max_steps in [0, 2^20], rtol >= 0");
    if (!h->analyzed) { g_last_error = "gmrf_gn_run: factor the assembler's pattern once on this handle first"; return GMRF_ERR_NO_FACTOR; }
    GCHK(driver_analysis_ok(g));
    HIPCHK(hipSetDevice(h->device));
    GCHK(objective_ready(as));
    const int64_t B = h->B, n = as->n, m = as->m, wide = std::max(n, m);
    GCHK(gn_alloc(g, B, max_steps));
    hipStream_t st = h->stream;
    // inputs: Q's values and the start point are copied (gmrf_gn_finalize reads them later), the rest is read where it lies
    const int64_t q_count = q_stride ? B * as->nnz_q : as->nnz_q;
    HIPCHK(hipMemcpyAsync(g->d_q, q_nzval, sizeof(double) * q_count, is_device_ptr(q_nzval) ? hipMemcpyDeviceToDevice : hipMemcpyHostToDevice, st));
    HIPCHK(hipMemcpyAsync(g->d_x, x, sizeof(double) * B * n, is_device_ptr(x) ? hipMemcpyDeviceToDevice : hipMemcpyHostToDevice, st));
    const double *d_qxp, *d_xp, *d_y;
    Staging args(g->in);
    args.in(qx_prior, sizeof(double) * B * n, &d_qxp);
    args.in(x_prior, sizeof(double) * B * n, &d_xp);
    args.in(y, sizeof(double) * B * m, &d_y);
    GCHK(args.commit(st));
    g->q_stride = q_stride; g->noise = noise; g->have_x = true;
    const GnState s = gn_state(g);
    // (slots of the history that no step reaches read NaN: all bits set)
    HIPCHK(hipMemsetAsync(g->d_hist, 0xFF, sizeof(double) * B * ((size_t)max_steps + 1), st));
    const dim3 grid_m((unsigned)((m + 255) / 256), (unsigned)B), grid_w((unsigned)((wide + 255) / 256), (unsigned)B);
    // the start: obs_diff = y - f(x), objective, every problem active (the first `last` is +Inf)
    GCHK(gn_launch_tangent(g, st, B, g->d_x, g->d_jv, g->d_f));
    hipLaunchKernelGGL(gn_obs_diff, grid_m, dim3(256), 0, st, d_y, g->d_f, m, g->d_od);
    GCHK(launch_objective_batch(as, st, B, g->d_q, q_stride, d_xp, g->d_x, g->d_od, noise, g->d_part, g->d_obj));
    hipLaunchKernelGGL(gn_decide, dim3(1), dim3(256), 0, st, s, g->d_obj, B, rtol, max_steps, 1);
    HIPCHK(hipGetLastError());
    HIPCHK(hipStreamSynchronize(st));
    const FactorRhsScope registered(h, g->d_rhs);         // the rhs buffer rides in the factorisations of this run
    gmrf_status status = GMRF_OK;
    g->iterations = g->fwd_iterations = 0;
    auto iteration = [&]() -> gmrf_status {
        GCHK(gn_launch_tangent(g, st, B, g->d_x, g->d_jv, g->d_f));
        GCHK(launch_precision_batch(as, st, B, g->d_q, q_stride, g->d_jv, noise, g->d_a));
        GCHK(launch_rhs_batch(as, st, B, d_qxp, g->d_jv, g->d_x, g->d_od, noise, g->d_v, g->d_rhs));
        GCHK(numeric_factor(h, g->d_a, info));
        GCHK(gn_solve(g));
        // the candidate's residual and objective; J's values are not needed any more this iteration and are overwritten
        GCHK(gn_launch_tangent(g, st, B, g->d_xn, g->d_jv, g->d_f));
        hipLaunchKernelGGL(gn_obs_diff, grid_m, dim3(256), 0, st, d_y, g->d_f, m, g->d_on);
        GCHK(launch_objective_batch(as, st, B, g->d_q, q_stride, d_xp, g->d_xn, g->d_on, noise, g->d_part, g->d_obj));
        hipLaunchKernelGGL(gn_decide, dim3(1), dim3(256), 0, st, s, g->d_obj, B, rtol, max_steps, 0);
        hipLaunchKernelGGL(gn_apply, grid_w, dim3(256), 0, st, g->d_take, g->d_xn, g->d_x, n, g->d_on, g->d_od, m);
        HIPCHK(hipGetLastError());
        HIPCHK(hipStreamSynchronize(st));
        return GMRF_OK;
    };
    for (int32_t it = 0; it < max_steps && status == GMRF_OK; ++it) {
        if (*static_cast<volatile unsigned*>(g->h_active.p) == 0u) break;
        status = iteration();
        if (status == GMRF_OK) g->iterations += 1;
    }
    // x holds the last complete iterate of every problem, also after a failed factorisation
    gmrf_status out_status = copy_out(st, x, g->d_x, sizeof(double) * B * n);
    if (out_status == GMRF_OK) out_status = copy_out(st, steps_out, g->d_steps, sizeof(int32_t) * B);
    if (out_status == GMRF_OK) out_status = copy_out(st, obj_hist_out, g->d_hist, sizeof(double) * B * ((size_t)max_steps + 1));
    HIPCHK(hipStreamSynchronize(st));
    return status != GMRF_OK ? status : out_status;
}

// tangent at the run's final x, A = Q + noise J'J into d_a, factor (a run on this batch has been checked for)
static gmrf_status gn_factor_final(gmrf_gn* g, int32_t* info) {
    gmrf_handle* h = g->h;
    GCHK(gn_launch_tangent(g, h->stream, g->B, g->d_x, g->d_jv, g->d_f));
    GCHK(launch_precision_batch(g->as, h->stream, g->B, g->d_q, g->q_stride, g->d_jv, g->noise, g->d_a));
    return numeric_factor(h, g->d_a, info);
}

gmrf_status gmrf_gn_finalize(gmrf_gn* g, int32_t* info) {
    if (!g) return bad_shape("null pointer");
    if (info) *info = 0;
    if (!g->have_x || g->B != g->h->B) { g_last_error = "gmrf_gn_finalize: no run on this batch"; return GMRF_ERR_NO_FACTOR; }
    GCHK(gn_bound_ok(g));
    HIPCHK(hipSetDevice(g->h->device));
    return gn_factor_final(g, info);
}

// --------------------------------------------------------------------------------- the batched Darcy conditioning driver
// B = batch of the handle Darcy data-set problems on one mesh (scripts/darcy/solve_darcy_gmrf-fem.jl:176-198 per problem) in ONE
// call on the handle's stream:
//     coefficient tables -> A, y -> Q + q_eps A'A, information vector -> gmrf_bt_refactor_values -> mean, samples -> variances -> std, |std|
// The information vector is registered as the factor's right-hand side (gmrf_bt_set_factor_rhs) for the run, as gmrf_gn_run
// does.  Mean / samples and the variances go through the public calls' own abort-and-repeat guards (sweep_guarded); every
// intermediate -- A's values, the posterior values the RBMC product reads -- stays in the driver's buffers on the device.
struct gmrf_dc : DriverBase {
    gmrf_darcy_p1* d = nullptr;
    int64_t ks = -1;                     // the samples `work` is carved for
    double *d_av = nullptr, *d_y = nullptr, *d_dw = nullptr, *d_nz = nullptr, *d_rhs = nullptr, *d_mean = nullptr, *d_smp = nullptr;
    double *d_var = nullptr, *d_diag = nullptr, *d_part = nullptr, *d_norm = nullptr;
    int32_t fwd_in_factor = 0;           // the last run's factorisation left y = L^-1 rhs (gmrf_test_dc_route)
};

static gmrf_status dc_bound_ok(const gmrf_dc* g) {
    const gmrf_handle* h = g->h;
    GCHK(tw_refuse(h, "the Darcy conditioning driver"));
    GCHK(driver_same_device_stream(g, g->d->device, g->d->stream, "Darcy assembler"));
    if (g->as->n != g->d->n || g->as->m != g->d->n || g->as->nnz_j != g->d->nnz)
        return bad_shape("the assembler's J is not the Darcy assembler's pattern");
    return driver_analysis_ok(g);
}

gmrf_status gmrf_dc_create(gmrf_handle* h, gmrf_assembler* as, gmrf_darcy_p1* d, gmrf_dc** out) {
    if (!out || !as || !d) return bad_shape("null pointer");
    if (as->device < 0 || d->device < 0) {
        g_last_error = "the Darcy conditioning driver needs an assembler and a Darcy assembler with a device (created with device -1)";
        return GMRF_ERR_NO_DEVICE;
    }
    if (!h) return bad_shape("null handle");
    auto g = std::make_unique<gmrf_dc>();
    g->bind(h, as); g->d = d;
    GCHK(dc_bound_ok(g.get()));
    *out = g.release();
    return GMRF_OK;
}

gmrf_status gmrf_dc_destroy(gmrf_dc* g) {
    if (!g) return GMRF_OK;
    g->close();
    delete g;
    return GMRF_OK;
}

static gmrf_status dc_alloc(gmrf_dc* g, int64_t B, int64_t ks) {
    if (g->B == B && g->ks == ks && g->work.p) return GMRF_OK;
    const gmrf_assembler* as = g->as;
    const int64_t n = as->n;
    auto lay = [&](char* base) {
        Carve c{base};
        c(&g->d_av, B * as->nnz_j); c(&g->d_y, B * n); c(&g->d_dw, darcy_batch_work_elems(g->d, B)); c(&g->d_nz, B * as->nnz_out);
        c(&g->d_rhs, B * n); c(&g->d_mean, B * n); c(&g->d_smp, B * ks * n); c(&g->d_var, B * n); c(&g->d_diag, B * n);
        c(&g->d_part, B * std_norm_chunks(n)); c(&g->d_norm, B);
        return c.used;
    };
    GCHK(g->work.reserve(g->h->stream, lay(nullptr)));
    lay(g->work.as<char>());
    g->B = B; g->ks = ks;
    return GMRF_OK;
}

gmrf_status gmrf_dc_run(gmrf_dc* g, const double* coeff_tables, int64_t ng, double beta, const double* q_nzval, int64_t q_stride,
                        const double* q_mu, double q_eps, int64_t k_samples, uint64_t sample_seed, int32_t var_method, int64_t k_var,
                        uint64_t var_seed, double* mean_out, double* samples_out, double* std_out, double* std_norm_out, int32_t* info) {
    // (the checks of the plain arguments come before anything of *g is read: tests/test_darcy_batch_cpu.py drives them without a
    //  device, with a driver pointer that must never be followed -- keep them above the first g->)
    if (!g || !coeff_tables || !q_nzval) return bad_shape("null pointer");
    if (info) *info = 0;
    if (!darcy_ng_ok(ng)) return bad_shape("ng in [2, 46340]");
    if (k_samples < 0 || k_samples > KP_CHUNK) return bad_shape("k_samples in [0, 128]");
    if (samples_out && k_samples == 0) return bad_shape("samples_out with k_samples = 0");
    const bool sampled = var_method == GMRF_VAR_RBMC || var_method == GMRF_VAR_MC;
    if (var_method != -1 && var_method != GMRF_VAR_EXACT && !sampled) return bad_shape("var_method: -1 (none), exact, RBMC or MC");
    if (sampled && k_var <= 0) return bad_shape("k_var <= 0");
    if (var_method == -1 && (std_out || std_norm_out)) return bad_shape("std_out / std_norm_out without a variance method");
    gmrf_handle* h = g->h;
    gmrf_assembler* as = g->as;
    GCHK(dc_bound_ok(g));
    GCHK(q_stride_ok(as, q_stride));
    if (!h->analyzed) { g_last_error = "gmrf_dc_run: factor the assembler's pattern once on this handle first"; return GMRF_ERR_NO_FACTOR; }
    const int64_t B = h->B, n = as->n;
    if (!batch_ok(B)) return bad_shape("batch outside [1, 4096]");
    HIPCHK(hipSetDevice(h->device));
    hipStream_t st = h->stream;
    GCHK(dc_alloc(g, B, k_samples));
    if (var_method == GMRF_VAR_RBMC) GCHK(driver_pattern_csr(g));
    const double *d_tab, *d_q, *d_qmu;
    Staging args(g->in);
    args.in(coeff_tables, sizeof(double) * B * ng * ng, &d_tab);
    args.in(q_nzval, sizeof(double) * (q_stride ? B * as->nnz_q : as->nnz_q), &d_q);
    args.in(q_mu, sizeof(double) * B * n, &d_qmu);
    GCHK(args.commit(st));
    // 1 - 3: A's values and y, the posterior values, the information vector q_mu + q_eps A' y (x = 0: A x + y is y itself)
    GCHK(launch_darcy_batch(g->d, st, B, d_tab, ng, beta, g->d_av, g->d_y, g->d_dw));
    GCHK(launch_precision_batch(as, st, B, d_q, q_stride, g->d_av, q_eps, g->d_nz));
    hipLaunchKernelGGL(assemble_jt_apply_batch, dim3((unsigned)((n + 255) / 256), (unsigned)B), dim3(256), 0, st, as->d_jt_ptr, as->d_jt_row,
                       as->d_jt_src, g->d_av, as->nnz_j, g->d_y, as->m, d_qmu, q_eps, n, g->d_rhs);
    HIPCHK(hipGetLastError());
    // 4 - 6 behind the registration; the caller's comes back afterwards
    g->fwd_in_factor = 0;
    auto solve = [&]() -> gmrf_status {
        const FactorRhsScope registered(h, g->d_rhs);
        GCHK(numeric_factor(h, g->d_nz, info));
        g->fwd_in_factor = (h->fy_for && h->fy_for == g->d_rhs) ? 1 : 0;
        if (k_samples > 0) GCHK(gmrf_bt_posterior(h, g->d_rhs, sample_seed, 0, k_samples, g->d_mean, g->d_smp, n));
        else GCHK(gmrf_bt_solve(h, g->d_rhs, g->d_mean, 1, n, n, GMRF_SOLVE_FULL));
        return driver_variances(g, var_method, k_var, var_seed, g->d_nz, g->d_diag, g->d_var);
    };
    const gmrf_status status = solve();
    if (status != GMRF_OK) { (void)hipStreamSynchronize(st); return status; }      // (the outputs are untouched)
    // 7: std = sqrt(var) in place, |std| per problem
    if (var_method != -1) GCHK(driver_std_norm(g, g->d_var, g->d_part, g->d_norm));
    GCHK(copy_out(st, mean_out, g->d_mean, sizeof(double) * B * n));
    GCHK(copy_out(st, samples_out, g->d_smp, sizeof(double) * B * k_samples * n));
    GCHK(copy_out(st, std_out, g->d_var, sizeof(double) * B * n));
    GCHK(copy_out(st, std_norm_out, g->d_norm, sizeof(double) * B));
    HIPCHK(hipStreamSynchronize(st));
    return GMRF_OK;
}

// --------------------------------------------------------------------------------- the batched Burgers initial-condition stage
// B = batch of the handle problems of the Burgers data-set loop (scripts/burgers/solve_burgers_gmrf-fem.jl:154-208), its "Prior"
// and "Initial condition" stages in ONE call on the handle's stream:
//     ic -> bulk, Q_ic's values, Qx_prior (burgers_prior.hpp) -> Q_ic in the order of the assembler's pattern -> gmrf_bt_refactor_values
//     -> x_ic = Q_ic^-1 Qx_prior = mean(x_ic)
// on the handle and the analysis the Gauss-Newton driver uses afterwards: the assembler's pattern, that of Q + J'J, filled by the
// assembler's own kernel with noise 0 and J = 0.  Qx_prior is registered as the factor's right-hand side (gmrf_bt_set_factor_rhs)
// for the run, as gmrf_dc_run does; the caller's registration comes back afterwards.
struct gmrf_bic : DriverBase {
    gmrf_burgers_prior* pr = nullptr;
    double *d_bulk = nullptr, *d_q = nullptr, *d_qx = nullptr, *d_jz = nullptr, *d_a = nullptr, *d_x = nullptr;
    int32_t fwd_in_factor = 0;           // the last run's factorisation left y = L^-1 Qx_prior (gmrf_test_bic_route)
};

static gmrf_status bic_bound_ok(const gmrf_bic* g) {
    const gmrf_handle* h = g->h;
    GCHK(tw_refuse(h, "the Burgers initial-condition driver"));
    GCHK(driver_same_device_stream(g, g->pr->device, g->pr->stream, "Burgers prior"));
    if (g->as->n != g->pr->n || g->as->nnz_q != g->pr->nnz) return bad_shape("the assembler's Q is not the Burgers prior's pattern");
    return driver_analysis_ok(g);
}

gmrf_status gmrf_bic_create(gmrf_handle* h, gmrf_assembler* as, gmrf_burgers_prior* prior, gmrf_bic** out) {
    if (!out || !as || !prior) return bad_shape("null pointer");
    if (as->device < 0 || prior->device < 0) {
        g_last_error = "the Burgers initial-condition driver needs an assembler and a Burgers prior with a device (created with device -1)";
        return GMRF_ERR_NO_DEVICE;
    }
    if (!h) return bad_shape("null handle");
    auto g = std::make_unique<gmrf_bic>();
    g->bind(h, as); g->pr = prior;
    GCHK(bic_bound_ok(g.get()));
    // the same sizes are not yet the same pattern: entry by entry against the prior's statement of it
    if (as->q_ptr.empty()) return bad_shape("the Burgers initial-condition driver needs n < 2^31");
    for (int64_t j = 0; j <= as->n; ++j) {
        const int64_t at = j < as->n ? prior_colptr(prior, j) : prior->nnz;
        if (as->q_ptr[(size_t)j] != at) return bad_shape("the assembler's Q is not the Burgers prior's pattern");
    }
    for (int64_t e = 0; e < prior->nnz; ++e) {
        int64_t row, col;
        prior_entry(prior, e, &row, &col);
        if (as->q_row[(size_t)e] != row) return bad_shape("the assembler's Q is not the Burgers prior's pattern");
    }
    *out = g.release();
    return GMRF_OK;
}

gmrf_status gmrf_bic_destroy(gmrf_bic* g) {
    if (!g) return GMRF_OK;
    g->close();
    delete g;
    return GMRF_OK;
}

static gmrf_status bic_alloc(gmrf_bic* g, int64_t B) {
    if (g->B == B && g->work.p) return GMRF_OK;
    const gmrf_assembler* as = g->as;
    auto lay = [&](char* base) {
        Carve c{base};
        c(&g->d_bulk, B); c(&g->d_q, B * as->nnz_q); c(&g->d_qx, B * as->n); c(&g->d_jz, as->nnz_j); c(&g->d_a, B * as->nnz_out);
        c(&g->d_x, B * as->n);
        return c.used;
    };
    GCHK(g->work.reserve(g->h->stream, lay(nullptr)));
    lay(g->work.as<char>());
    // J = 0, once: one array serves every problem (a stride of 0), and nothing writes it
    HIPCHK(hipMemsetAsync(g->d_jz, 0, sizeof(double) * (size_t)std::max<int64_t>(as->nnz_j, 1), g->h->stream));
    g->B = B;
    return GMRF_OK;
}

gmrf_status gmrf_bic_run(gmrf_bic* g, const double* ic, double* x_ic_out, double* q_values_out, double* qx_out, double* bulk_out,
                         int32_t* info) {
    if (!g || !ic || !x_ic_out) return bad_shape("null pointer");
    if (info) *info = 0;
    gmrf_handle* h = g->h;
    gmrf_assembler* as = g->as;
    GCHK(bic_bound_ok(g));
    if (!h->analyzed) { g_last_error = "gmrf_bic_run: factor the assembler's pattern once on this handle first"; return GMRF_ERR_NO_FACTOR; }
    const int64_t B = h->B, n = as->n;
    if (!batch_ok(B)) return bad_shape("batch outside [1, 4096]");
    HIPCHK(hipSetDevice(h->device));
    hipStream_t st = h->stream;
    GCHK(bic_alloc(g, B));
    const double* d_ic;
    Staging args(g->in);
    args.in(ic, sizeof(double) * B * g->pr->ns, &d_ic);
    GCHK(args.commit(st));
    // 1 - 2: the prior's values and information vector, Q_ic in the order of the handle's analysis (noise 0, J = 0 at stride 0)
    GCHK(launch_prior_batch(g->pr, st, B, d_ic, g->d_bulk, g->d_q, g->d_qx));
    hipLaunchKernelGGL(assemble_precision_batch, dim3((unsigned)((as->nnz_out + 255) / 256), (unsigned)B), dim3(256), 0, st, as->d_pptr,
                       as->d_pa, as->d_pb, as->d_qmap, g->d_q, as->nnz_q, g->d_jz, (int64_t)0, 0.0, as->nnz_out, g->d_a);
    HIPCHK(hipGetLastError());
    // 3 - 4 behind the registration; the caller's comes back afterwards
    g->fwd_in_factor = 0;
    auto solve = [&]() -> gmrf_status {
        const FactorRhsScope registered(h, g->d_qx);
        GCHK(numeric_factor(h, g->d_a, info));
        bool took_y = false;
        GCHK(solve_registered(h, g->d_qx, g->d_x, &took_y));
        g->fwd_in_factor = took_y ? 1 : 0;
        return GMRF_OK;
    };
    const gmrf_status status = solve();
    if (status != GMRF_OK) { (void)hipStreamSynchronize(st); return status; }      // (the outputs are untouched)
    GCHK(copy_out(st, x_ic_out, g->d_x, sizeof(double) * B * n));
    GCHK(copy_out(st, q_values_out, g->d_q, sizeof(double) * B * as->nnz_q));
    GCHK(copy_out(st, qx_out, g->d_qx, sizeof(double) * B * n));
    GCHK(copy_out(st, bulk_out, g->d_bulk, sizeof(double) * B));
    HIPCHK(hipStreamSynchronize(st));
    return GMRF_OK;
}

// --------------------------------------------------------------------------------- batched error metrics (src/metrics.jl)
static int64_t field_errors_chunks(int64_t count) { return std::min<int64_t>(1024, std::max<int64_t>(1, (count + 2047) / 2048)); }

// d_part: [batch][field_errors_chunks(n - first)][3] work array; d_out: [batch][3]
static gmrf_status launch_field_errors_batch(hipStream_t st, int64_t batch, int64_t n, int64_t first, const double* d_pred,
                                             const double* d_soln, double* d_part, double* d_out) {
    const int64_t count = n - first, nch = field_errors_chunks(count), len = (count + nch - 1) / nch;
    hipLaunchKernelGGL(field_errors_part, dim3((unsigned)nch, (unsigned)batch), dim3(256), 0, st, d_pred, d_soln, n, first, len, d_part);
    hipLaunchKernelGGL(field_errors_finish, dim3(1, (unsigned)batch), dim3(256), 0, st, d_part, nch, count, d_out);
    HIPCHK(hipGetLastError());
    return GMRF_OK;
}

gmrf_status gmrf_field_errors_batch(int32_t device, void* stream, int64_t batch, int64_t n, int64_t first, const double* pred,
                                    const double* soln, double* out) {
    if (!pred || !soln || !out || !batch_ok(batch)) return bad_shape("null pointer or batch outside [1, 4096]");
    if (n <= 0 || first < 0 || first >= n) return bad_shape("the elements [first, n) must not be empty");
    DevCtx ctx;
    GCHK(ctx.open(device, stream, hipStreamNonBlocking, "gmrf_field_errors_batch", false));
    DevBuf arena, part;
    const double *d_pred, *d_soln;
    double* d_out;
    Staging args(arena);
    args.in(pred, sizeof(double) * batch * n, &d_pred);
    args.in(soln, sizeof(double) * batch * n, &d_soln);
    args.out(out, sizeof(double) * batch * 3, &d_out);
    auto run = [&]() -> gmrf_status {
        GCHK(args.commit(ctx.stream));
        GCHK(part.reserve(ctx.stream, sizeof(double) * (size_t)(batch * field_errors_chunks(n - first) * 3)));
        GCHK(launch_field_errors_batch(ctx.stream, batch, n, first, d_pred, d_soln, part.as<double>(), d_out));
        GCHK(args.flush(ctx.stream));
        HIPCHK(hipStreamSynchronize(ctx.stream));
        return GMRF_OK;
    };
    const gmrf_status status = run();
    ctx.close();                        // (drains the stream before the buffers go)
    arena.release(); part.release();
    return status;
}

// --------------------------------------------------------------------------------- fields at data-grid points (field_eval.hpp)
// E = evaluation_matrix(disc, pred_coords) of the data-set loops (solve_darcy_gmrf-fem.jl:82-89, solve_burgers_gmrf-fem.jl:75-83) as
// a table of `width` (dof, weight) pairs per point, built here once in double precision; `pred = E f` and the metrics against a
// truth on the device.
struct gmrf_eval : DevCtx {             // device -1: the rows only
    int64_t ns = 0, npts = 0;
    int width = 0;
    std::vector<int64_t> idx;           // [npts][width], ascending within a row
    std::vector<double> w;
    DevArr<int32_t> d_idx;              // [width][npts]
    DevArr<double> d_w;
    DevBuf arena, part;                 // host arguments of the current call (Staging); the chunk sums of the metrics
    // pair table of the pointwise variance (field_eval_pairs): the spatial pattern P and the pairs' positions in it
    std::vector<int64_t> p_rowptr, p_colidx;
    std::vector<int32_t> pos;           // [width (width + 1) / 2][npts]
    DevArr<int32_t> d_pos;
    gmrf_csr* var_csr = nullptr;        // I_nt (x) P on the device, the pattern gmrf_bt_selinv is asked for; rebuilt when nt changes
    int64_t var_nt = 0;
    DevArr<double> d_var;               // [batch][nt][npts] of a calibration call that does not return the variances
};

gmrf_status gmrf_eval_destroy(gmrf_eval* e) {
    if (!e) return GMRF_OK;
    if (e->var_csr) (void)gmrf_csr_destroy(e->var_csr);
    e->close();
    delete e;
    return GMRF_OK;
}

static gmrf_status eval_bad_point(int64_t c, const std::string& what, const char* domain) {
    g_last_error = "evaluation point " + std::to_string(c) + " = " + what + " is not in " + domain;
    return GMRF_ERR_BAD_SHAPE;
}

// Opens the device side of a handle whose rows are complete and uploads the table point-minor.
static gmrf_status eval_finish(std::unique_ptr<gmrf_eval, gmrf_status (*)(gmrf_eval*)>& guard, int32_t device, void* stream,
                               const char* who, gmrf_eval** out) {
    gmrf_eval* e = guard.get();
    if (!field_eval_pairs(e->width, e->npts, e->ns, e->idx.data(), e->p_rowptr, e->p_colidx, e->pos))
        return bad_shape((std::string(who) + ": the pair pattern of the points has 2^31 entries or more").c_str());
    GCHK(e->open(device, stream, hipStreamNonBlocking, who));
    if (e->device >= 0) {
        GCHK(e->d_pos.upload(e->stream, e->pos));
        const int64_t W = e->width, np = e->npts;
        std::vector<int32_t> ti((size_t)(W * np));
        std::vector<double> tw((size_t)(W * np));
        for (int64_t c = 0; c < np; ++c)
            for (int64_t k = 0; k < W; ++k) {
                ti[(size_t)(k * np + c)] = (int32_t)e->idx[(size_t)(c * W + k)];
                tw[(size_t)(k * np + c)] = e->w[(size_t)(c * W + k)];
            }
        GCHK(e->d_idx.upload(e->stream, ti));
        GCHK(e->d_w.upload(e->stream, tw));
        HIPCHK(hipStreamSynchronize(e->stream));
    }
    *out = guard.release();
    return GMRF_OK;
}

static bool eval_npts_ok(int64_t npts) { return npts >= 1 && npts <= (1 << 28); }

gmrf_status gmrf_eval_line_create(int32_t device, void* stream, int64_t nc, int32_t order, int32_t bc, double length, int64_t npts,
                                  const double* points, gmrf_eval** out) {
    const bool dirichlet = bc == GMRF_BURGERS_DIRICHLET;
    if (!out) return bad_shape("null pointer");
    if (order != 1 && order != 2) return bad_shape("order must be 1 or 2");
    if (bc != GMRF_BURGERS_PERIODIC && !dirichlet) return bad_shape("bc must be periodic or dirichlet");
    if (!(length > 0.0) || !std::isfinite(length)) return bad_shape("length must be positive");
    if (nc < (dirichlet ? 2 : 3) || nc > (1 << 24)) return bad_shape("nc: >= 3 cells, >= 2 on the Dirichlet interval (<= 2^24)");
    if (!eval_npts_ok(npts)) return bad_shape("npts must lie in [1, 2^28]");
    if (!points) return bad_shape("null pointer");
    for (int64_t c = 0; c < npts; ++c) {
        const double x = points[c];
        if (!std::isfinite(x) || x < 0.0 || !(dirichlet ? x <= length : x < length))
            return eval_bad_point(c, std::to_string(x), dirichlet ? "[0, length]" : "[0, length)");
    }
    std::unique_ptr<gmrf_eval, gmrf_status (*)(gmrf_eval*)> guard(new gmrf_eval(), gmrf_eval_destroy);
    gmrf_eval* e = guard.get();
    e->ns = order * nc + (dirichlet ? 1 : 0); e->npts = npts; e->width = order + 1;
    e->idx.resize((size_t)(npts * e->width)); e->w.resize((size_t)(npts * e->width));
    const double h = length / (double)nc;
    for (int64_t c = 0; c < npts; ++c)
        field_eval_line_row(order, nc, e->ns, h, points[c], &e->idx[(size_t)(c * e->width)], &e->w[(size_t)(c * e->width)]);
    return eval_finish(guard, device, stream, "gmrf_eval_line_create", out);
}

gmrf_status gmrf_eval_tri_create(int32_t device, void* stream, int64_t nx, int64_t ny, int32_t order, int64_t npts, const double* xy,
                                 gmrf_eval** out) {
    if (!out) return bad_shape("null pointer");
    if (order != 1 && order != 2) return bad_shape("order must be 1 or 2");
    if (nx < 2 || ny < 2 || nx > 16384 || ny > 16384) return bad_shape("nx, ny must lie in [2, 16384]");
    if (!eval_npts_ok(npts)) return bad_shape("npts must lie in [1, 2^28]");
    if (!xy) return bad_shape("null pointer");
    for (int64_t c = 0; c < npts; ++c) {
        const double x = xy[2 * c], y = xy[2 * c + 1];
        if (!std::isfinite(x) || !std::isfinite(y) || x < 0.0 || x > 1.0 || y < 0.0 || y > 1.0)
            return eval_bad_point(c, "(" + std::to_string(x) + ", " + std::to_string(y) + ")", "[0, 1]^2");
    }
    std::unique_ptr<gmrf_eval, gmrf_status (*)(gmrf_eval*)> guard(new gmrf_eval(), gmrf_eval_destroy);
    gmrf_eval* e = guard.get();
    e->ns = order == 1 ? nx * ny : (2 * nx - 1) * (2 * ny - 1); e->npts = npts; e->width = order == 1 ? 3 : 6;
    e->idx.resize((size_t)(npts * e->width)); e->w.resize((size_t)(npts * e->width));
    for (int64_t c = 0; c < npts; ++c)
        field_eval_tri_row(order, nx, ny, xy[2 * c], xy[2 * c + 1], &e->idx[(size_t)(c * e->width)], &e->w[(size_t)(c * e->width)]);
    return eval_finish(guard, device, stream, "gmrf_eval_tri_create", out);
}

gmrf_status gmrf_eval_rows(const gmrf_eval* e, int64_t* ns_out, int64_t* width_out, int64_t* idx, double* w) {
    if (!e) return bad_shape("null handle");
    if (ns_out) *ns_out = e->ns;
    if (width_out) *width_out = e->width;
    if (idx) std::copy(e->idx.begin(), e->idx.end(), idx);
    if (w) std::copy(e->w.begin(), e->w.end(), w);
    return GMRF_OK;
}

gmrf_status gmrf_eval_pairs(const gmrf_eval* e, int64_t* nnz_out, int64_t* rowptr, int64_t* colidx, int32_t* pos) {
    if (!e) return bad_shape("null handle");
    if (nnz_out) *nnz_out = (int64_t)e->p_colidx.size();
    if (rowptr) std::copy(e->p_rowptr.begin(), e->p_rowptr.end(), rowptr);
    if (colidx) std::copy(e->p_colidx.begin(), e->p_colidx.end(), colidx);
    if (pos) std::copy(e->pos.begin(), e->pos.end(), pos);
    return GMRF_OK;
}

// rows is looped over inside the kernel: grid.y stays under its cap of 65 535
static gmrf_status launch_eval_apply(const gmrf_eval* e, int64_t rows, const double* d_fields, double* d_pred) {
    const dim3 grid((unsigned)((e->npts + 255) / 256), (unsigned)std::min<int64_t>(rows, 65535));
    auto go = [&](auto kernel) {
        hipLaunchKernelGGL(kernel, grid, dim3(256), 0, e->stream, e->d_idx.get(), e->d_w.get(), e->npts, e->ns, rows, d_fields, d_pred);
    };
    if (e->width == 2) go(field_eval_apply<2>);
    else if (e->width == 3) go(field_eval_apply<3>);
    else go(field_eval_apply<6>);
    HIPCHK(hipGetLastError());
    return GMRF_OK;
}

gmrf_status gmrf_eval_apply_batch(gmrf_eval* e, int64_t rows, const double* fields, double* pred_out) {
    if (!e) return bad_shape("null handle");
    if (!fields || !pred_out) return bad_shape("null pointer");
    if (rows < 1 || rows > (1 << 24)) return bad_shape("rows outside [1, 2^24]");
    GCHK(e->ready("gmrf_eval_apply_batch needs the device"));
    const double* d_fields;
    double* d_pred;
    Staging args(e->arena);
    args.in(fields, sizeof(double) * rows * e->ns, &d_fields);
    args.out(pred_out, sizeof(double) * rows * e->npts, &d_pred);
    GCHK(args.commit(e->stream));
    GCHK(launch_eval_apply(e, rows, d_fields, d_pred));
    GCHK(args.flush(e->stream));
    HIPCHK(hipStreamSynchronize(e->stream));
    return GMRF_OK;
}

gmrf_status gmrf_eval_errors_batch(gmrf_eval* e, int64_t batch, int64_t nt, int64_t first_slice, const double* fields,
                                   const double* truth, double* errors_out, double* pred_out) {
    if (!e) return bad_shape("null handle");
    if (!fields || !truth || !errors_out) return bad_shape("null pointer");
    if (!batch_ok(batch)) return bad_shape("batch outside [1, 4096]");
    if (nt < 1 || first_slice < 0 || first_slice >= nt || nt > (int64_t)0x7fffffff / e->npts)
        return bad_shape("the slices [first_slice, nt) must not be empty (nt npts < 2^31)");
    GCHK(e->ready("gmrf_eval_errors_batch needs the device"));
    const hipStream_t st = e->stream;
    const int64_t n = nt * e->npts, first = first_slice * e->npts, count = n - first, nch = field_errors_chunks(count),
                  len = (count + nch - 1) / nch;
    const double *d_fields, *d_truth;
    double *d_err, *d_pred;
    Staging args(e->arena);
    args.in(fields, sizeof(double) * batch * nt * e->ns, &d_fields);
    args.in(truth, sizeof(double) * batch * n, &d_truth);
    args.out(errors_out, sizeof(double) * batch * 3, &d_err);
    args.out(pred_out, sizeof(double) * batch * n, &d_pred);
    GCHK(args.commit(st));
    GCHK(e->part.reserve(st, sizeof(double) * (size_t)(batch * nch * 3)));
    if (d_pred) {
        // the caller wants pred: it is written once by the apply kernel and the metrics read it
        GCHK(launch_eval_apply(e, batch * nt, d_fields, d_pred));
        GCHK(launch_field_errors_batch(st, batch, n, first, d_pred, d_truth, e->part.as<double>(), d_err));
    } else {
        const dim3 grid((unsigned)nch, (unsigned)batch);
        auto go = [&](auto kernel) {
            hipLaunchKernelGGL(kernel, grid, dim3(256), 0, st, e->d_idx.get(), e->d_w.get(), e->npts, e->ns, nt, d_fields, d_truth, first,
                               len, e->part.as<double>());
        };
        if (e->width == 2) go(field_eval_errors_part<2>);
        else if (e->width == 3) go(field_eval_errors_part<3>);
        else go(field_eval_errors_part<6>);
        hipLaunchKernelGGL(field_errors_finish, dim3(1, (unsigned)batch), dim3(256), 0, st, e->part.as<double>(), nch, count, d_err);
        HIPCHK(hipGetLastError());
    }
    GCHK(args.flush(st));
    HIPCHK(hipStreamSynchronize(st));
    return GMRF_OK;
}

// --------------------------------------------------------------------------------- the posterior stage of the Gauss-Newton driver
// What the data-set loops do with the final iterate (solve_burgers_gmrf-fem.jl:184-208, -collocation.jl:248-263, the final GMRF of
// _research/elliptic_chen24.jl) for the batch of the last gmrf_gn_run, in ONE call on the handle's stream:
//     gmrf_gn_finalize's tangent, A = Q + noise J'J and factor -> samples x + L^-T z -> variances -> std, |std| -> logdet, sqmahal, nll
//     -> errors of x against z
// Samples and variances go through the public calls' own abort-and-repeat guards; A's values, which the RBMC product and the
// quadratic form read, the samples' mean x and every score stay in the driver's buffers on the device.
static gmrf_status gn_post_alloc(gmrf_gn* g, int64_t B, int64_t ks) {
    if (g->post_B == B && g->post_ks == ks && g->post.p) return GMRF_OK;
    const int64_t n = g->as->n;
    auto lay = [&](char* base) {
        Carve c{base};
        c(&g->d_smp, B * ks * n); c(&g->d_var, B * n); c(&g->d_diag, B * n); c(&g->d_spart, B * std_norm_chunks(n)); c(&g->d_norm, B);
        c(&g->d_ld, B); c(&g->d_sq, B); c(&g->d_nll, B); c(&g->d_err, B * 3); c(&g->d_epart, B * field_errors_chunks(n) * 3);
        return c.used;
    };
    GCHK(g->post.reserve(g->h->stream, lay(nullptr)));
    lay(g->post.as<char>());
    g->post_B = B; g->post_ks = ks;
    return GMRF_OK;
}

gmrf_status gmrf_gn_posterior(gmrf_gn* g, const double* z, int64_t first, int64_t k_samples, uint64_t sample_seed, int32_t var_method,
                              int64_t k_var, uint64_t var_seed, double* samples_out, double* std_out, double* std_norm_out,
                              double* logdet_out, double* sqmahal_out, double* nll_out, double* errors_out, int32_t* info) {
    // (the checks of the plain arguments come before anything of *g is read, as in gmrf_dc_run: tests/test_gn_posterior_cpu.py
    //  drives them without a device, with a driver pointer that must never be followed -- keep them above the first g->)
    if (!g) return bad_shape("null pointer");
    if (info) *info = 0;
    if (k_samples < 0 || k_samples > KP_CHUNK) return bad_shape("k_samples in [0, 128]");
    if (samples_out && k_samples == 0) return bad_shape("samples_out with k_samples = 0");
    const bool sampled = var_method == GMRF_VAR_RBMC || var_method == GMRF_VAR_MC;
    if (var_method != -1 && var_method != GMRF_VAR_EXACT && !sampled) return bad_shape("var_method: -1 (none), exact, RBMC or MC");
    if (sampled && k_var <= 0) return bad_shape("k_var <= 0");
    if (var_method == -1 && (std_out || std_norm_out)) return bad_shape("std_out / std_norm_out without a variance method");
    if (!z && (sqmahal_out || nll_out || errors_out)) return bad_shape("sqmahal_out / nll_out / errors_out without z");
    if (first < 0) return bad_shape("first < 0");
    if (!g->have_x || g->B != g->h->B) { g_last_error = "gmrf_gn_posterior: no run on this batch"; return GMRF_ERR_NO_FACTOR; }
    GCHK(gn_bound_ok(g));
    gmrf_handle* h = g->h;
    gmrf_assembler* as = g->as;
    const int64_t B = g->B, n = as->n;
    if (errors_out && first >= n) return bad_shape("the elements [first, n) must not be empty");
    HIPCHK(hipSetDevice(h->device));
    hipStream_t st = h->stream;
    const bool want_sq = sqmahal_out || nll_out, want_ld = logdet_out || nll_out;
    GCHK(gn_post_alloc(g, B, k_samples));
    if (var_method == GMRF_VAR_RBMC) GCHK(driver_pattern_csr(g));
    if (want_sq) GCHK(quadform_ready(as));
    const double* d_z;
    Staging args(g->in);
    args.in(z, sizeof(double) * B * n, &d_z);
    GCHK(args.commit(st));
    // 1: the factor at the final iterate
    const gmrf_status status = gn_factor_final(g, info);
    if (status != GMRF_OK) { (void)hipStreamSynchronize(st); return status; }      // (the outputs are untouched)
    // 2 - 3: samples around the iterate (nothing is solved for the mean), variances on the values just assembled, std and |std|
    if (k_samples > 0) GCHK(gmrf_bt_sample(h, sample_seed, 0, k_samples, g->d_x, nullptr, g->d_smp, n));
    GCHK(driver_variances(g, var_method, k_var, var_seed, g->d_a, g->d_diag, g->d_var));
    if (var_method != -1) GCHK(driver_std_norm(g, g->d_var, g->d_spart, g->d_norm));
    // 4: scores
    if (want_ld) GCHK(logdet_batch_enqueue(h, g->d_ld));
    if (want_sq) GCHK(launch_quadform_batch(as, st, B, g->d_a, as->nnz_out, g->d_x, d_z, g->d_spart, g->d_sq));
    if (nll_out) {
        hipLaunchKernelGGL(nll_batch, dim3((unsigned)((B + 255) / 256)), dim3(256), 0, st, (double)n, std::log(2.0 * M_PI), g->d_sq, g->d_ld, B,
                           g->d_nll);
        HIPCHK(hipGetLastError());
    }
    // 5: errors of the iterate against z over [first, n)
    if (errors_out) GCHK(launch_field_errors_batch(st, B, n, first, g->d_x, d_z, g->d_epart, g->d_err));
    // 6
    GCHK(copy_out(st, samples_out, g->d_smp, sizeof(double) * B * k_samples * n));
    GCHK(copy_out(st, std_out, g->d_var, sizeof(double) * B * n));
    GCHK(copy_out(st, std_norm_out, g->d_norm, sizeof(double) * B));
    GCHK(copy_out(st, logdet_out, g->d_ld, sizeof(double) * B));
    GCHK(copy_out(st, sqmahal_out, g->d_sq, sizeof(double) * B));
    GCHK(copy_out(st, nll_out, g->d_nll, sizeof(double) * B));
    GCHK(copy_out(st, errors_out, g->d_err, sizeof(double) * B * 3));
    HIPCHK(hipStreamSynchronize(st));
    return GMRF_OK;
}

// --------------------------------------------------------------------------------- shallow-water element kernels
struct gmrf_swe_p1 : DevCtx {           // device -1: patterns / quadrature points only
    int64_t nx = 0, ny = 0, nn = 0, n = 0, cells = 0, nnz_k = 0, nnz_s = 0;
    std::vector<int64_t> rowptr_k, col_k, rowptr_s, col_s;     // 0-based
    DevArr<int64_t> d_rowptr_k, d_rowptr_s;
    DevArr<int32_t> d_col_k, d_col_s;
    DevArr<double> d_dk, d_ds, d_mean;                            // |diagonals|, three meandiag scalars
    DevBuf arena;                       // host arguments of the current call (Staging)
};

gmrf_status gmrf_shallow_water_p1_destroy(gmrf_swe_p1* w) {
    if (!w) return GMRF_OK;
    w->close();
    delete w;
    return GMRF_OK;
}

gmrf_status gmrf_shallow_water_p1_create(int32_t device, void* stream, int64_t nx, int64_t ny, gmrf_swe_p1** out) {
    if (!out || nx < 2 || ny < 2 || nx > 16384 || ny > 16384) return bad_shape("bad shallow-water mesh size");
    std::unique_ptr<gmrf_swe_p1, gmrf_status (*)(gmrf_swe_p1*)> guard(new gmrf_swe_p1(), gmrf_shallow_water_p1_destroy);
    gmrf_swe_p1* w = guard.get();
    w->nx = nx; w->ny = ny; w->nn = nx * ny; w->n = 3 * w->nn; w->cells = 2 * (nx - 1) * (ny - 1);
    w->rowptr_k.assign((size_t)w->n + 1, 0); w->rowptr_s.assign((size_t)w->n + 1, 0);
    w->col_k.reserve((size_t)w->n * 21); w->col_s.reserve((size_t)w->n * 7);
    const int dxs[7] = {-1, 0, -1, 0, 1, 0, 1}, dys[7] = {-1, -1, 0, 0, 0, 1, 1};
    for (int64_t node = 0; node < w->nn; ++node) {
        const int64_t ix = node % nx, iy = node / nx;
        for (int fa = 0; fa < 3; ++fa) {
            const int64_t row = 3 * node + fa;
            for (int s7 = 0; s7 < 7; ++s7) {
                const int64_t jx = ix + dxs[s7], jy = iy + dys[s7];
                if (jx < 0 || jy < 0 || jx >= nx || jy >= ny) continue;
                const int64_t nj = jy * nx + jx;
                for (int fb = 0; fb < 3; ++fb) w->col_k.push_back(3 * nj + fb);      // full field coupling (:140)
                w->col_s.push_back(3 * nj + fa);                                     // block-diagonal coupling (:141-150)
            }
            w->rowptr_k[(size_t)row + 1] = (int64_t)w->col_k.size();
            w->rowptr_s[(size_t)row + 1] = (int64_t)w->col_s.size();
        }
    }
    w->nnz_k = (int64_t)w->col_k.size(); w->nnz_s = (int64_t)w->col_s.size();
    GCHK(w->open(device, stream, hipStreamNonBlocking, "gmrf_shallow_water_p1_create"));
    if (w->device >= 0) {
        std::vector<int32_t> ck(w->col_k.begin(), w->col_k.end()), cs(w->col_s.begin(), w->col_s.end());
        GCHK(reserve_group(w->stream, {w->d_dk.want((size_t)w->n), w->d_ds.want((size_t)w->n), w->d_mean.want(4)}));
        GCHK(w->d_rowptr_k.upload(w->stream, w->rowptr_k));
        GCHK(w->d_rowptr_s.upload(w->stream, w->rowptr_s));
        GCHK(w->d_col_k.upload(w->stream, ck));
        GCHK(w->d_col_s.upload(w->stream, cs));
        HIPCHK(hipStreamSynchronize(w->stream));
    }
    *out = guard.release();
    return GMRF_OK;
}

gmrf_status gmrf_shallow_water_p1_pattern(const gmrf_swe_p1* w, int32_t which, int64_t* nnz_out, int64_t* rowptr, int64_t* colidx,
                                          int32_t index_base) {
    if (!w || (which != 0 && which != 1)) return bad_shape("pattern: 0 = K (coupling), 1 = S / M (block diagonal)");
    const auto& rp = which == 0 ? w->rowptr_k : w->rowptr_s;
    const auto& ci = which == 0 ? w->col_k : w->col_s;
    if (nnz_out) *nnz_out = (int64_t)ci.size();
    if (rowptr) for (int64_t i = 0; i <= w->n; ++i) rowptr[i] = rp[(size_t)i] + index_base;
    if (colidx) for (size_t p = 0; p < ci.size(); ++p) colidx[p] = ci[p] + index_base;
    return GMRF_OK;
}

// spatial_coordinate(cvh, qp, cell_coords) (:52) of every cell: xy[cell][q][2]
gmrf_status gmrf_shallow_water_p1_qpoints(const gmrf_swe_p1* w, double* xy) {
    if (!w || !xy) return bad_shape("null pointer");
    if (is_device_ptr(xy)) return bad_shape("quadrature points are written to host memory");
    p1_triangle_qpoints(w->nx, w->ny, xy);
    return GMRF_OK;
}

// meandiag of a vector of |diagonal| values + apply! on CSR values
static gmrf_status swe_constrain(gmrf_swe_p1* w, const int64_t* d_rowptr, const int32_t* d_col, const uint8_t* d_pres, const double* d_absdiag,
                                 double* d_mean, double* d_vals) {
    hipLaunchKernelGGL(darcy_meandiag, dim3(1), dim3(256), 0, w->stream, d_absdiag, w->n, d_mean);
    hipLaunchKernelGGL(csr_apply_constraints, dim3((unsigned)((w->n + 255) / 256)), dim3(256), 0, w->stream, d_rowptr, d_col, d_pres, w->n,
                       d_mean, d_vals);
    HIPCHK(hipGetLastError());
    return GMRF_OK;
}

gmrf_status gmrf_shallow_water_p1_assemble(gmrf_swe_p1* w, const double* H_q, double k, double f, double g, const uint8_t* prescribed,
                                           double* K_vals, double* M_lumped, double* S_vals) {
    if (!w) return bad_shape("null handle");
    GCHK(w->ready("pattern-only shallow-water handle"));
    if (!H_q || !K_vals || !M_lumped || !S_vals) return bad_shape("null pointer");
    const double* d_hq; const uint8_t* d_pres;
    double *d_kv, *d_sv, *d_ml;
    Staging args(w->arena);
    args.in(H_q, sizeof(double) * w->cells * 3, &d_hq);
    args.in(prescribed, (size_t)w->n, &d_pres);
    args.out(K_vals, sizeof(double) * w->nnz_k, &d_kv);
    args.out(S_vals, sizeof(double) * w->nnz_s, &d_sv);
    args.out(M_lumped, sizeof(double) * w->n, &d_ml);
    GCHK(args.commit(w->stream));
    SweP1Args a;
    a.nx = (int)w->nx; a.ny = (int)w->ny; a.Hq = d_hq; a.k = k; a.f = f; a.g = g;
    a.rowptr_k = w->d_rowptr_k; a.rowptr_s = w->d_rowptr_s; a.kv = d_kv; a.sv = d_sv; a.ml = d_ml; a.dk = w->d_dk; a.ds = w->d_ds;
    hipLaunchKernelGGL(swe_p1_rows, dim3((unsigned)((w->n + 255) / 256)), dim3(256), 0, w->stream, a);
    HIPCHK(hipGetLastError());
    if (d_pres) {
        // apply!(K, ..), apply!(M, ..), apply!(S, ..)  (:119-121)
        GCHK(swe_constrain(w, w->d_rowptr_k, w->d_col_k, d_pres, w->d_dk, w->d_mean, d_kv));
        GCHK(swe_constrain(w, w->d_rowptr_s, w->d_col_s, d_pres, w->d_ds, w->d_mean + 1, d_sv));
        hipLaunchKernelGGL(darcy_meandiag, dim3(1), dim3(256), 0, w->stream, d_ml, w->n, w->d_mean + 2);      // M >= 0: |M_ii| = M_ii
        hipLaunchKernelGGL(vec_set_prescribed, dim3((unsigned)((w->n + 255) / 256)), dim3(256), 0, w->stream, d_pres, w->n,
                           (const double*)(w->d_mean + 2), 0.0, d_ml);
        HIPCHK(hipGetLastError());
    }
    GCHK(args.flush(w->stream));
    HIPCHK(hipStreamSynchronize(w->stream));
    return GMRF_OK;
}

gmrf_status gmrf_shallow_water_p1_operators(gmrf_swe_p1* w, const double* K_vals, const double* M_lumped, const double* S_vals,
                                            const uint8_t* prescribed, double kappa_matern, double tau, double dt, double* G_vals,
                                            double* J_vals, double* M_tilde, double* beta) {
    if (!w) return bad_shape("null handle");
    GCHK(w->ready("pattern-only shallow-water handle"));
    if (!K_vals || !M_lumped || !S_vals || !G_vals || !J_vals || !M_tilde || !beta) return bad_shape("null pointer");
    if (!(kappa_matern > 0.0) || !(dt > 0.0)) return bad_shape("kappa_matern and dt must be positive");
    SweOpArgs a;
    const uint8_t* d_pres;
    Staging args(w->arena);
    args.in(K_vals, sizeof(double) * w->nnz_k, &a.kv);
    args.in(S_vals, sizeof(double) * w->nnz_s, &a.sv);
    args.in(M_lumped, sizeof(double) * w->n, &a.ml);
    args.in(prescribed, (size_t)w->n, &d_pres);
    args.out(G_vals, sizeof(double) * w->nnz_k, &a.Gd);
    args.out(J_vals, sizeof(double) * w->nnz_s, &a.J);
    args.out(M_tilde, sizeof(double) * w->n, &a.Mt);
    args.out(beta, sizeof(double) * w->n, &a.beta);
    GCHK(args.commit(w->stream));
    a.n = w->n; a.rowptr_k = w->d_rowptr_k; a.col_k = w->d_col_k; a.rowptr_s = w->d_rowptr_s; a.col_s = w->d_col_s;
    a.pres = d_pres; a.kappa2 = kappa_matern * kappa_matern; a.tau = tau; a.dt = dt; a.dg = w->d_dk;
    const double nu = 2.0;                                     // :180
    a.sqrt_ratio = std::sqrt(std::tgamma(nu) / (std::tgamma(nu + 1.0) * (4.0 * M_PI) * std::pow(kappa_matern, 2.0 * nu)));
    hipLaunchKernelGGL(swe_p1_operators, dim3((unsigned)((w->n + 255) / 256)), dim3(256), 0, w->stream, a);
    HIPCHK(hipGetLastError());
    if (d_pres) GCHK(swe_constrain(w, w->d_rowptr_k, w->d_col_k, d_pres, w->d_dk, w->d_mean + 3, a.Gd));      // apply!(S_tmp, f, ch) :213
    GCHK(args.flush(w->stream));
    HIPCHK(hipStreamSynchronize(w->stream));
    return GMRF_OK;
}

// --------------------------------------------------------------------------------- variances
static gmrf_status need_single(gmrf_handle* h) {
    if (h->B != 1) return bad_shape("marginal variances are computed per handle with batch 1");
    return GMRF_OK;
}

// The Takahashi block step that var_exact and selinv_pattern share (see var_exact for the recurrence).  Its work block d_V holds
// T1 (tk_t1) and behind it M (tk_m), one bsp x bsp block per problem each; Y is d_T.
static double* tk_t1(const gmrf_handle* h) { return h->d_V; }
static double* tk_m(const gmrf_handle* h) { return h->d_V + blk_elems(h) * h->B; }
static gmrf_status tk_alloc(gmrf_handle* h) {
    return h->d_V.reserve(h->stream, 2 * (size_t)blk_elems(h) * (size_t)h->B);
}
// Block i < N - 1, Sg = the leading block of Sigma_{i+1,i+1} (full, mirrored):  T1 = S' C_w,  M = T1^T C_w,  Y[cmin:] = (I + M) X[cmin:]
static gmrf_status tk_coupled_y(gmrf_handle* h, int64_t i, const double* Sg) {
    const int bsp = (int)h->bsp, cm = (int)h->cmin, rm = (int)h->rmax, wc = bsp - cm, twc = wc / 64;
    const int64_t ld = bsp, pX = stride_pX(h), pCm = stride_pC(h), pW = blk_elems(h);
    const double* Xw = h->d_Linv + i * pW + (int64_t)cm * ld;      // X[cmin:, :]
    const double* C = h->d_C + i * c_blk(h);
    double* V1 = tk_t1(h); double* V2 = tk_m(h); double* Yw = h->d_T + (int64_t)cm * ld;
    // T1 = S' C_w
    GCHK(gemm(h, GemmCall(false, true, rm, wc, rm, 1.0, 0.0).a(Sg, ld, pW).b(C, c_ld(h), pCm).c(V1, ld, pW)
                     .work(2.0 * rm * h->c_streamed * (double)h->B).k_end(nullptr, h->d_mend)));
    // M = T1^T C_w (lower tiles; T1 taken as it lies, [k][m]), mirrored
    GCHK(gemm(h, GemmCall(true, true, wc, wc, rm, 1.0, 0.0).a(V1, ld, pW).b(C, c_ld(h), pCm).c(V2, ld, pW).lower().k_end(nullptr, h->d_mend)));
    hipLaunchKernelGGL(transpose_tiles, dim3((unsigned)(twc * (twc + 1) / 2), (unsigned)h->B), dim3(256), 0, h->stream, V2, ld, V2, ld, pW, pW, twc, twc, 2);
    HIPCHK(hipGetLastError());
    // Y[cmin:, :] = M X[cmin:, :] + X[cmin:, :]   (column tile u of X[cmin:, :] starts at row max(0, 64 u - cmin))
    return gemm(h, GemmCall(false, true, wc, bsp, wc, 1.0, 1.0).a(V2, ld, pW).b(Xw, ld, pX).c(Yw, ld, pW).addend(Xw, ld, pX)
                       .k_begin(nullptr, h->d_kbx));
}
// S_ii[0:ms, 0:ms] = X^T Y on its lower tiles into Sn (X taken as it lies, [k][m]; the rows below cmin of Y are X's; uncoupled: Y = X)
static gmrf_status tk_xty(gmrf_handle* h, int64_t i, bool coupled, int ms, double* Sn) {
    const int bsp = (int)h->bsp, cm = (int)h->cmin;
    const int64_t ld = bsp, pX = stride_pX(h), pW = blk_elems(h);
    const double* X = h->d_Linv + i * pW;
    if (!coupled || cm > 0)
        GCHK(gemm(h, GemmCall(true, true, ms, ms, coupled ? cm : bsp, 1.0, 0.0).a(X, ld, pX).b(X, ld, pX).c(Sn, ld, pW)
                         .triangular(TRI_A_UPPER | TRI_B_LOWER).lower()));
    if (coupled)
        GCHK(gemm(h, GemmCall(true, true, ms, ms, bsp - cm, 1.0, cm > 0 ? 1.0 : 0.0).a(X + (int64_t)cm * ld, ld, pX)
                         .b(h->d_T + (int64_t)cm * ld, ld, pW).c(Sn, ld, pW).lower().k_begin(h->d_kbx, nullptr)));
    return GMRF_OK;
}

// seeded: the twisted order's bottom half -- the caller has put the whole Sigma of the last block (its start, seeded by the
// meeting block) into d_S; the recurrence goes on from there.
static gmrf_status var_exact(gmrf_handle* h, double* d_out, bool seeded = false) {
    // Selected inversion (Takahashi recurrence on the block-tridiagonal factor), all problems of a batch in lock step:
    //   S_NN = X_N^T X_N,   S_ii = X_i^T (I + C_i^T S_{i+1,i+1} C_i) X_i,      X_i = Linv_i, C_i = L_{i+1,i};  d_out[B][n] = diag.
    // Round 4: what the recurrence NEEDS of S_ii is its diagonal and its leading rmax x rmax block (C_i is zero below row rmax
    // and left of column cmin), and both follow from  S_ii = X^T Y,  Y = X with its rows >= cmin replaced by
    // (I + M) X[cmin:, :],  M = C_w^T S' C_w  (C_w: the stored window of C_i, S' = S_{i+1,i+1}[0:rmax, 0:rmax]):
    //   T1 = S' C_w                 rmax x wc,   K = rmax, column tile u of C_w ends at row mend[u]
    //   M  = T1^T C_w               wc x wc, lower tiles, same K bound (T1 as it lies: gemm_f64_dma's A [k][m] form), mirrored
    //   Y[cmin:, :] = M X[cmin:, :] + X[cmin:, :]          K = wc from the first non-zero row of each column tile of X
    //   S[0:rmax, 0:rmax] = X^T[0:rmax, :] Y[:, 0:rmax]    lower tiles, K from each row tile's diagonal (X as it lies, [k][m])
    //   diag(S)[n] = sum_k X[k][n] Y[k][n]                  (coldot_lower)
    // 1.9 GF per 1024-block instead of 5.7 (two full 1024^3 products, two of them on the register-staged kernel that the
    // [k][m] operand forced), every product on gemm_f64_dma.
    const int bsp = (int)h->bsp;
    const int64_t ld = bsp, bstride = (int64_t)bsp * bsp;
    const int64_t pX = stride_pX(h), pW = bstride;
    const int cm = (int)h->cmin, rm = (int)h->rmax;
    const unsigned nb = (unsigned)h->B;
    GCHK(ensure_full_inverse(h));
    GCHK(tk_alloc(h));
    double* Sg = h->d_S;     // leading block of Sigma_{i+1,i+1} (full, mirrored)
    double* Sn = h->d_W;
    double* Y = h->d_T;
    const int nt = bsp / 64, trm = rm / 64;
    for (int64_t i = h->N - 1; i >= 0; --i) {
        if (seeded && i == h->N - 1) {
            hipLaunchKernelGGL(extract_diag_dense, dim3((unsigned)((h->bs + 255) / 256), nb), dim3(256), 0, h->stream, Sg, ld, (int)h->bs,
                               d_out + i * h->bs, bstride, h->n);
            HIPCHK(hipGetLastError());
            continue;
        }
        const double* X = h->d_Linv + i * bstride;
        const bool coupled = i < h->N - 1;
        if (coupled) GCHK(tk_coupled_y(h, i, Sg));
        // diag(S_ii): of the last block processed (i = 0) and of the columns >= rmax by column dot products; the columns below
        // rmax of the other blocks are the diagonal of the leading block formed below (saves reading X and Y once more)
        const int u0 = (i == 0) ? 0 : trm;
        if (u0 < nt) {
            hipLaunchKernelGGL(coldot_lower, dim3((unsigned)(nt - u0), nb), dim3(256), 0, h->stream, X, coupled ? Y : nullptr, ld, bsp, cm, (int)h->bs,
                               d_out + i * h->bs, pX, pW, h->n, u0);
            HIPCHK(hipGetLastError());
        }
        if (i == 0) break;                               // nobody needs the leading block of S_00
        // leading block of S_ii for the next step: the product X^T Y on its lower tiles (X taken as it lies, [k][m]), mirrored
        GCHK(tk_xty(h, i, coupled, rm, Sn));
        hipLaunchKernelGGL(transpose_tiles, dim3((unsigned)(trm * (trm + 1) / 2), nb), dim3(256), 0, h->stream, Sn, ld, Sn, ld, pW, pW, trm, trm, 2);
        HIPCHK(hipGetLastError());
        {
            const int cnt = (int)std::min<int64_t>(rm, h->bs);
            hipLaunchKernelGGL(extract_diag_dense, dim3((unsigned)((cnt + 255) / 256), nb), dim3(256), 0, h->stream, Sn, ld, cnt,
                               d_out + i * h->bs, bstride, h->n);
            HIPCHK(hipGetLastError());
        }
        std::swap(Sg, Sn);
    }
    return GMRF_OK;
}

// ------------------------------------------------------------------------ selected inverse on a pattern
// Plan of a pattern S (gmrf_bt_selinv): every stored entry (r, c) is read from the block step that forms it -- S_ii for
// blk(r) = blk(c) = i, Sigma_{i+1,i}[0:rmax, :] for an entry between blocks i and i+1 -- at its canonical place (the lower
// triangle of S_ii; row in block i+1, column in block i).  Entries that share that place (the two triangles of a symmetric
// pattern) share one plan entry with two output slots.  Built on the host from S's index arrays, uploaded once.
static gmrf_status selinv_plan(gmrf_handle* h, const gmrf_csr* S, const char* who) {
    if (h->sel_csr == S->id && h->sel_gen == h->layout_gen && h->d_sel_src) return GMRF_OK;
    const int64_t n = h->n, bs = h->bs, bsp = h->bsp, rm = h->rmax, N = h->N, nnz = S->nnz;
    std::vector<int64_t> rp((size_t)n + 1);
    std::vector<int32_t> ci((size_t)std::max<int64_t>(nnz, 1));
    HIPCHK(hipMemcpyAsync(rp.data(), S->d_rowptr, sizeof(int64_t) * (n + 1), hipMemcpyDeviceToHost, S->stream));
    if (nnz > 0) HIPCHK(hipMemcpyAsync(ci.data(), S->d_colidx, sizeof(int32_t) * nnz, hipMemcpyDeviceToHost, S->stream));
    HIPCHK(hipStreamSynchronize(S->stream));
    struct Ent { int64_t key, src, slot; };            // key = 2 * step + (coupling ? 1 : 0)
    std::vector<Ent> ents((size_t)nnz);
    for (int64_t r = 0; r < n; ++r) {
        for (int64_t e = rp[r]; e < rp[r + 1]; ++e) {
            const int64_t c = ci[e], br = r / bs, bc = c / bs, lr = r % bs, lc = c % bs;
            if (br == bc) {
                ents[e] = {2 * br, std::max(lr, lc) * bsp + std::min(lr, lc), e};
                continue;
            }
            const int64_t late = br > bc ? lr : lc, early = br > bc ? lc : lr;
            if (std::abs(br - bc) > 1 || late >= rm) {
                g_last_error = std::string(who) + ": pattern entry (" + std::to_string(r) + ", " + std::to_string(c) + ") " +
                               (std::abs(br - bc) > 1 ? "lies " + std::to_string(std::abs(br - bc)) + " blocks off the diagonal"
                                                      : "is a coupling entry whose index in the later block (" + std::to_string(late) +
                                                        ") is not below rmax = " + std::to_string(rm)) +
                               " (block size " + std::to_string(bs) + ")";
                return GMRF_ERR_BAD_SHAPE;
            }
            ents[e] = {2 * std::min(br, bc) + 1, late * bsp + early, e};
        }
    }
    std::sort(ents.begin(), ents.end(), [](const Ent& a, const Ent& b) {
        return a.key != b.key ? a.key < b.key : (a.src != b.src ? a.src < b.src : a.slot < b.slot);
    });
    std::vector<int64_t> src, slot, slot2;
    src.reserve((size_t)nnz); slot.reserve((size_t)nnz); slot2.reserve((size_t)nnz);
    std::vector<int64_t> off((size_t)N + 1, 0), nd((size_t)N, 0);
    for (size_t a = 0; a < ents.size();) {
        size_t b = a + 1;
        const bool pair = b < ents.size() && ents[b].key == ents[a].key && ents[b].src == ents[a].src;
        src.push_back(ents[a].src); slot.push_back(ents[a].slot); slot2.push_back(pair ? ents[b].slot : -1);
        const int64_t step = ents[a].key / 2;
        off[(size_t)step + 1]++;
        if (!(ents[a].key & 1)) nd[(size_t)step]++;
        a = pair ? b + 1 : b;
    }
    for (int64_t i = 0; i < N; ++i) off[(size_t)i + 1] += off[(size_t)i];
    const int64_t cnt = (int64_t)src.size();
    HIPCHK(hipStreamSynchronize(h->stream));
    if (!h->d_sel_src || !h->d_sel_slot || h->sel_cap < cnt) {
        h->sel_cap = std::max<int64_t>(cnt, 1);           // (the stride between the two halves of d_sel_slot)
        GCHK(reserve_group(h->stream, {h->d_sel_src.want((size_t)h->sel_cap), h->d_sel_slot.want(2 * (size_t)h->sel_cap)}));
    }
    if (cnt > 0) {
        HIPCHK(hipMemcpyAsync(h->d_sel_src, src.data(), sizeof(int64_t) * cnt, hipMemcpyHostToDevice, h->stream));
        HIPCHK(hipMemcpyAsync(h->d_sel_slot, slot.data(), sizeof(int64_t) * cnt, hipMemcpyHostToDevice, h->stream));
        HIPCHK(hipMemcpyAsync(h->d_sel_slot + h->sel_cap, slot2.data(), sizeof(int64_t) * cnt, hipMemcpyHostToDevice, h->stream));
        HIPCHK(hipStreamSynchronize(h->stream));       // (the vectors are locals)
    }
    h->sel_off = std::move(off); h->sel_nd = std::move(nd);
    h->sel_nnz = nnz; h->sel_csr = S->id; h->sel_gen = h->layout_gen;
    return GMRF_OK;
}

// Sigma = A^-1 on the plan's pattern into d_out[B][nnz].  The recurrence of var_exact with the same products, plus per block step
//   Sigma_{i+1,i}[0:rmax, :] = -T1 X[cmin:, :]        rmax x bsp, K = wc from the first non-zero row of each column tile (d_kbx)
//                                                     (Sigma L = L^-T, block row i+1 of block column i; T1 = S' C_w as formed)
//   S_ii = X[:cmin]^T X[:cmin] + X[cmin:]^T Y[cmin:]  the whole block on its lower tiles, the two K ranges of the leading block
// and a scatter of the step's pattern entries to their slots.  The coupling block goes to the M buffer once Y is formed, S_ii to
// the buffer the leading block goes to (its leading rmax x rmax block is then mirrored for the next step, as var_exact does).
static gmrf_status selinv_pattern(gmrf_handle* h, double* d_out) {
    const int bsp = (int)h->bsp;
    const int64_t ld = bsp, bstride = (int64_t)bsp * bsp;
    const int64_t pX = stride_pX(h), pW = bstride;
    const int cm = (int)h->cmin, rm = (int)h->rmax, wc = bsp - cm;
    const unsigned nb = (unsigned)h->B;
    GCHK(ensure_full_inverse(h));
    GCHK(tk_alloc(h));
    double* Sg = h->d_S;
    double* Sn = h->d_W;
    double* V2 = tk_m(h);                                // M, then Sigma_{i+1,i}[0:rmax, :]
    const int trm = rm / 64;
    const int64_t* slot2 = h->d_sel_slot + h->sel_cap;
    for (int64_t i = h->N - 1; i >= 0; --i) {
        const double* X = h->d_Linv + i * bstride;
        const bool coupled = i < h->N - 1;
        const int64_t e0 = h->sel_off[(size_t)i], ne = h->sel_off[(size_t)i + 1] - e0, nd = h->sel_nd[(size_t)i];
        if (coupled) {
            GCHK(tk_coupled_y(h, i, Sg));
            if (ne > nd)
                GCHK(gemm(h, GemmCall(false, true, rm, bsp, wc, -1.0, 0.0).a(tk_t1(h), ld, pW).b(X + (int64_t)cm * ld, ld, pX).c(V2, ld, pW)
                                 .k_begin(nullptr, h->d_kbx)));
        }
        // S_ii on its lower tiles: the whole block if this step has entries there, else its leading block for the next step
        if (nd > 0 || i > 0) GCHK(tk_xty(h, i, coupled, nd > 0 ? bsp : rm, Sn));
        if (ne > 0) {
            hipLaunchKernelGGL(selinv_scatter, dim3((unsigned)((ne + 255) / 256), nb), dim3(256), 0, h->stream, Sn, V2, pW,
                               h->d_sel_src, h->d_sel_slot, slot2, e0, nd, ne, d_out, h->sel_nnz);
            HIPCHK(hipGetLastError());
        }
        if (i == 0) break;
        hipLaunchKernelGGL(transpose_tiles, dim3((unsigned)(trm * (trm + 1) / 2), nb), dim3(256), 0, h->stream, Sn, ld, Sn, ld, pW, pW, trm, trm, 2);
        HIPCHK(hipGetLastError());
        std::swap(Sg, Sn);
    }
    return GMRF_OK;
}

static gmrf_status selinv_ready(gmrf_handle* h, const gmrf_csr* S, const char* who) {
    GCHK(tw_refuse(h, who));
    if (!h->factored) { g_last_error = std::string(who) + " before factor"; return GMRF_ERR_NO_FACTOR; }
    if (S->n_rows != h->n || S->n_cols != h->n)
        return bad_shape((std::string(who) + ": the pattern must be n x n with the factored n").c_str());
    HIPCHK(hipSetDevice(h->device));
    GCHK(selinv_plan(h, S, who));
    return GMRF_OK;
}

static gmrf_status ensure_sig(gmrf_handle* h) {
    return h->d_sig.reserve(h->stream, (size_t)(std::max<int64_t>(h->sel_nnz, 1) * h->B));
}

gmrf_status gmrf_bt_selinv(gmrf_handle* h, const gmrf_csr* S, double* vals_out) {
    if (!h || !S || !vals_out) return bad_shape("null pointer");
    GCHK(selinv_ready(h, S, "gmrf_bt_selinv"));
    const bool dev = is_device_ptr(vals_out);
    if (!dev) GCHK(ensure_sig(h));
    double* d_out = dev ? vals_out : h->d_sig;          // every slot of the pattern is written
    GCHK(selinv_pattern(h, d_out));
    if (!dev) HIPCHK(hipMemcpyAsync(vals_out, d_out, sizeof(double) * h->sel_nnz * h->B, hipMemcpyDeviceToHost, h->stream));
    HIPCHK(hipStreamSynchronize(h->stream));
    if (h->profiling) prof_collect(h);
    return GMRF_OK;
}

gmrf_status gmrf_bt_trace_inv(gmrf_handle* h, const gmrf_csr* S, const double* dvals, int64_t m, double* out) {
    if (!h || !S || !dvals || !out) return bad_shape("null pointer");
    if (m <= 0 || m > 65535) return bad_shape("gmrf_bt_trace_inv: m must be in [1, 65535]");
    GCHK(selinv_ready(h, S, "gmrf_bt_trace_inv"));
    GCHK(ensure_sig(h));
    const int64_t nnz = h->sel_nnz, dv_count = h->B * m * nnz;
    const int64_t nch = std::min<int64_t>(256, std::max<int64_t>(1, (nnz + 8191) / 8192)), len = (nnz + nch - 1) / nch;
    const bool dv_dev = is_device_ptr(dvals), out_dev = is_device_ptr(out);
    const int64_t need = (dv_dev ? 0 : dv_count) + h->B * m * nch + (out_dev ? 0 : h->B * m);
    if (need > 0) GCHK(h->d_dv.reserve(h->stream, (size_t)need));
    const double* d_dv = dvals;
    if (!dv_dev) {
        HIPCHK(hipMemcpyAsync(h->d_dv, dvals, sizeof(double) * dv_count, hipMemcpyHostToDevice, h->stream));
        d_dv = h->d_dv;
    }
    double* d_part = h->d_dv + (dv_dev ? 0 : dv_count);                 // [B][m][nch] partial sums
    double* d_res = out_dev ? out : d_part + h->B * m * nch;
    GCHK(selinv_pattern(h, h->d_sig));
    hipLaunchKernelGGL(pattern_dot_part, dim3((unsigned)nch, (unsigned)m, (unsigned)h->B), dim3(256), 0, h->stream, h->d_sig, d_dv, nnz, m,
                       len, d_part);
    HIPCHK(hipGetLastError());
    hipLaunchKernelGGL(pattern_dot_sum, dim3((unsigned)m, (unsigned)h->B), dim3(256), 0, h->stream, d_part, nch, m, d_res);
    HIPCHK(hipGetLastError());
    if (!out_dev) HIPCHK(hipMemcpyAsync(out, d_res, sizeof(double) * h->B * m, hipMemcpyDeviceToHost, h->stream));
    HIPCHK(hipStreamSynchronize(h->stream));
    if (h->profiling) prof_collect(h);
    return GMRF_OK;
}

// ------------------------------------------------------------- pointwise predictive variance at data-grid points (field_eval.hpp)
// var = diag(E Sigma E^T): the selected inverse of the handle's factor on I_nt (x) P, P the evaluator's pair pattern, into the
// handle's own Sigma buffer, then one quadratic form per (problem, slice, point) on the evaluator's stream.  The pattern matrix is
// the evaluator's, so the handle's plan (keyed by the matrix id) holds across refactor_values and is rebuilt only after another
// pattern was asked of the handle in between.
static gmrf_status eval_var_sigma(gmrf_eval* e, gmrf_handle* h, int64_t nt, int64_t batch, const char* who) {
    GCHK(tw_refuse(h, who));
    if (!h->factored) { g_last_error = std::string(who) + " before factor"; return GMRF_ERR_NO_FACTOR; }
    const int64_t nnzp = (int64_t)e->p_colidx.size(), ns = e->ns;
    if (nt < 1 || h->n != nt * ns)
        return bad_shape((std::string(who) + ": the factored n = " + std::to_string(h->n) + " is not nt * ns = " + std::to_string(nt) + " * " +
                          std::to_string(ns)).c_str());
    if (nt > (int64_t)0x7fffffff / std::max(nnzp, e->npts))
        return bad_shape((std::string(who) + ": nt npts and nt nnz(P) must stay below 2^31").c_str());
    if (h->device != e->device) return bad_shape((std::string(who) + ": the factor handle and the evaluator live on different devices").c_str());
    if (batch >= 0 && batch != h->B)
        return bad_shape((std::string(who) + ": batch = " + std::to_string(batch) + " but the handle factors " + std::to_string(h->B) +
                          " problems").c_str());
    if (!e->var_csr || e->var_nt != nt) {
        std::vector<int64_t> rp((size_t)(nt * ns) + 1), ci((size_t)(nt * nnzp));
        for (int64_t t = 0; t < nt; ++t) {
            for (int64_t r = 0; r < ns; ++r) rp[(size_t)(t * ns + r)] = t * nnzp + e->p_rowptr[(size_t)r];
            for (int64_t k = 0; k < nnzp; ++k) ci[(size_t)(t * nnzp + k)] = t * ns + e->p_colidx[(size_t)k];
        }
        rp[(size_t)(nt * ns)] = nt * nnzp;
        const std::vector<double> zeros((size_t)(nt * nnzp), 0.0);          // (the values of a pattern matrix are never read)
        if (e->var_csr) { (void)gmrf_csr_destroy(e->var_csr); e->var_csr = nullptr; }
        GCHK(gmrf_csr_create(e->device, e->stream, nt * ns, nt * ns, rp.data(), ci.data(), zeros.data(), 0, 0, &e->var_csr));
        e->var_nt = nt;
    }
    GCHK(selinv_ready(h, e->var_csr, who));
    GCHK(ensure_sig(h));
    GCHK(selinv_pattern(h, h->d_sig));
    HIPCHK(hipStreamSynchronize(h->stream));            // (the evaluator's stream reads Sigma after this)
    if (h->profiling) prof_collect(h);
    return GMRF_OK;
}

static gmrf_status launch_eval_var(const gmrf_eval* e, const gmrf_handle* h, int64_t nt, double* d_var) {
    const int64_t rows = h->B * nt, nnzp = (int64_t)e->p_colidx.size();
    const dim3 grid((unsigned)((e->npts + 255) / 256), (unsigned)std::min<int64_t>(rows, 65535));
    auto go = [&](auto kernel) {
        hipLaunchKernelGGL(kernel, grid, dim3(256), 0, e->stream, e->d_pos.get(), e->d_w.get(), e->npts, nnzp, rows, h->d_sig.get(), d_var);
    };
    if (e->width == 2) go(field_eval_var<2>);
    else if (e->width == 3) go(field_eval_var<3>);
    else go(field_eval_var<6>);
    HIPCHK(hipGetLastError());
    return GMRF_OK;
}

gmrf_status gmrf_eval_var_batch(gmrf_eval* e, gmrf_handle* h, int64_t nt, double* var_out) {
    if (!e || !h) return bad_shape("null handle");
    if (!var_out) return bad_shape("null pointer");
    GCHK(e->ready("gmrf_eval_var_batch needs the device"));
    GCHK(eval_var_sigma(e, h, nt, -1, "gmrf_eval_var_batch"));
    double* d_var;
    Staging args(e->arena);
    args.out(var_out, sizeof(double) * h->B * nt * e->npts, &d_var);
    GCHK(args.commit(e->stream));
    GCHK(launch_eval_var(e, h, nt, d_var));
    GCHK(args.flush(e->stream));
    HIPCHK(hipStreamSynchronize(e->stream));
    return GMRF_OK;
}

gmrf_status gmrf_eval_calibration_batch(gmrf_eval* e, gmrf_handle* h, int64_t batch, int64_t nt, int64_t first_slice, double zcrit,
                                        const double* fields, const double* truth, double* out, double* pred_out, double* var_out) {
    if (!e || !h) return bad_shape("null handle");
    if (!fields || !truth || !out) return bad_shape("null pointer");
    if (!batch_ok(batch)) return bad_shape("batch outside [1, 4096]");
    if (nt < 1 || first_slice < 0 || first_slice >= nt || nt > (int64_t)0x7fffffff / e->npts)
        return bad_shape("the slices [first_slice, nt) must not be empty (nt npts < 2^31)");
    if (!(zcrit >= 0.0)) return bad_shape("zcrit must not be negative");
    GCHK(e->ready("gmrf_eval_calibration_batch needs the device"));
    GCHK(eval_var_sigma(e, h, nt, batch, "gmrf_eval_calibration_batch"));
    const hipStream_t st = e->stream;
    const int64_t n = nt * e->npts, first = first_slice * e->npts, count = n - first, nch = field_errors_chunks(count),
                  len = (count + nch - 1) / nch;
    const double *d_fields, *d_truth;
    double *d_out, *d_pred, *d_var;
    Staging args(e->arena);
    args.in(fields, sizeof(double) * batch * nt * e->ns, &d_fields);
    args.in(truth, sizeof(double) * batch * n, &d_truth);
    args.out(out, sizeof(double) * batch * 4, &d_out);
    args.out(pred_out, sizeof(double) * batch * n, &d_pred);
    args.out(var_out, sizeof(double) * batch * n, &d_var);
    GCHK(args.commit(st));
    GCHK(e->part.reserve(st, sizeof(double) * (size_t)(batch * nch * 4)));
    if (!d_var) {
        GCHK(e->d_var.reserve(st, (size_t)(batch * n)));
        d_var = e->d_var;
    }
    GCHK(launch_eval_var(e, h, nt, d_var));
    if (d_pred) GCHK(launch_eval_apply(e, batch * nt, d_fields, d_pred));       // (the caller's copy; the sums form pred themselves)
    auto go = [&](auto kernel) {
        hipLaunchKernelGGL(kernel, dim3((unsigned)nch, (unsigned)batch), dim3(256), 0, st, e->d_idx.get(), e->d_w.get(), e->npts, e->ns, nt,
                           d_fields, d_truth, (const double*)d_var, zcrit, first, len, e->part.as<double>());
    };
    if (e->width == 2) go(field_eval_calibration_part<2>);
    else if (e->width == 3) go(field_eval_calibration_part<3>);
    else go(field_eval_calibration_part<6>);
    hipLaunchKernelGGL(field_eval_calibration_finish, dim3(1, (unsigned)batch), dim3(256), 0, st, e->part.as<double>(), nch, count, d_out);
    HIPCHK(hipGetLastError());
    GCHK(args.flush(st));
    HIPCHK(hipStreamSynchronize(st));
    return GMRF_OK;
}

// One chunk of samples (panel p of d_Y, kc right-hand sides) -> node-major X[n][kcp] -> the RBMC / MC
// accumulator: the samples leave the sweep as a panel (each right-hand side contiguous); the
// transposing unpack puts the kc values of a node side by side, which is the layout the LDS-tiled
// SpMM and the accumulator read with full 128-byte lines.
// (panel != nullptr: the samples come from that panel, leading dimension panel_ld, blocks of pbs rows padded to pbsp -- a twisted
//  handle passes its samples column-major, pbs = pbsp = n)
static gmrf_status var_chunk(gmrf_handle* h, int method, int64_t p, int kc, const gmrf_csr* Q, const double* q_vals,
                             const double* d_diag, double* d_acc, const double* panel = nullptr, int64_t panel_ld = 0,
                             int64_t pbs = 0, int64_t pbsp = 0) {
    const int64_t n = h->n;
    const int kp = pad_k(kc), kcp = kc + (kc & 1);
    GCHK(ensure_stage(h, 2 * (int64_t)kcp * n));
    double* Xr = h->d_stage;
    double* QX = h->d_stage + (int64_t)kcp * n;
    if (!panel) { panel = h->d_Y + p * kp * h->n_pad; panel_ld = h->n_pad; pbs = h->bs; pbsp = h->bsp; }
    hipLaunchKernelGGL(unpack_panel_rows, dim3((unsigned)((n + 63) / 64), (unsigned)((kc + 63) / 64)), dim3(256), 0, h->stream,
                       panel, panel_ld, Xr, (int64_t)kcp, (int)pbs, (int)pbsp, n, kc);
    HIPCHK(hipGetLastError());
    if (method == GMRF_VAR_RBMC) GCHK(spmm_rows_device(Q, h->stream, Xr, kcp, QX, kcp, kc, q_vals));
    hipLaunchKernelGGL(rbmc_accumulate_rows, dim3((unsigned)((n + 15) / 16)), dim3(256), 0, h->stream, QX, Xr, (int64_t)kcp,
                       d_diag, n, kc, d_acc, method == GMRF_VAR_RBMC ? 0 : 1);
    HIPCHK(hipGetLastError());
    return GMRF_OK;
}

// Most bytes the node-major stage of the batched estimators may take (GMRF_VAR_STAGE_MB, read at every call; default 512):
// a problem's stage is 2 kcp n doubles (67 MB at darcy256), so a batch goes through it in groups.
static int64_t var_stage_cap_bytes() {
    const char* e = getenv("GMRF_VAR_STAGE_MB");
    const int64_t mb = e ? atoll(e) : 512;
    return std::max<int64_t>(mb, 1) << 20;
}

// The sampled estimator of every problem of a batch, enqueued on the handle's stream (no synchronisation): d_var[B][n] <- the
// variances.  Per chunk of 64 samples one sweep serves all problems (sample_chunk); then, per group of problems that fits the
// stage, ONE transposing unpack, ONE SpMM (RBMC; qv[B][nnz]: the problems' values on Q's pattern, device) and ONE accumulate
// with the problem as a grid dimension -- the kernels of var_chunk with the same sums per row and entry, so problem p gets the
// bits of var_chunk(h, method, p, ...).  d_diag[B][n]: work (RBMC).
static gmrf_status var_batch_enqueue(gmrf_handle* h, int method, int64_t k, uint64_t seed, const gmrf_csr* Q, const double* qv,
                                     double* d_diag, double* d_var) {
    const int64_t n = h->n, B = h->B;
    const bool rb = method == GMRF_VAR_RBMC;
    const dim3 grid_n((unsigned)((n + 255) / 256), (unsigned)B);
    HIPCHK(hipMemsetAsync(d_var, 0, sizeof(double) * n * B, h->stream));
    if (rb) {
        hipLaunchKernelGGL(csr_extract_diag_batch, grid_n, dim3(256), 0, h->stream, Q->d_rowptr, Q->d_colidx, qv, Q->nnz, n, d_diag);
        HIPCHK(hipGetLastError());
    }
    // groups sized by the widest chunk of the call, the same for every chunk (MC has no Q X half)
    const int64_t halves = rb ? 2 : 1;
    const int64_t kc_max = std::min<int64_t>(64, k), per_max = halves * (kc_max + (kc_max & 1)) * n;
    const int64_t G = std::max<int64_t>(1, std::min<int64_t>(B, var_stage_cap_bytes() / (per_max * (int64_t)sizeof(double))));
    GCHK(ensure_stage(h, G * per_max));
    h->var_group = (int32_t)G; h->var_groups = (int32_t)((B + G - 1) / G);
    for (int64_t c0 = 0; c0 < k; c0 += 64) {
        const int kc = (int)std::min<int64_t>(64, k - c0);
        GCHK(sample_chunk(h, seed, c0, kc, nullptr, 0, k));          // every problem's chunk in one sweep
        const int kp = pad_k(kc), kcp = kc + (kc & 1);
        const int64_t per = halves * (int64_t)kcp * n;
        for (int64_t g0 = 0; g0 < B; g0 += G) {
            const int64_t gb = std::min(G, B - g0);
            double* Xr = h->d_stage;
            double* QX = rb ? h->d_stage + (int64_t)kcp * n : Xr;      // (MC: not read)
            hipLaunchKernelGGL(unpack_panel_rows_batch, dim3((unsigned)((n + 63) / 64), (unsigned)((kc + 63) / 64), (unsigned)gb), dim3(256), 0,
                               h->stream, h->d_Y + g0 * kp * h->n_pad, h->n_pad, (int64_t)kp * h->n_pad, Xr, (int64_t)kcp, per, (int)h->bs,
                               (int)h->bsp, n, kc);
            HIPCHK(hipGetLastError());
            if (rb) GCHK(spmm_rows_device_batch(Q, h->stream, gb, qv + g0 * Q->nnz, Xr, kcp, per, QX, kcp, per, kc));
            hipLaunchKernelGGL(rbmc_accumulate_rows_batch, dim3((unsigned)((n + 15) / 16), (unsigned)gb), dim3(256), 0, h->stream, QX, Xr,
                               (int64_t)kcp, per, rb ? d_diag + g0 * n : (const double*)nullptr, n, kc, d_var + g0 * n, rb ? 0 : 1);
            HIPCHK(hipGetLastError());
        }
    }
    // finish in place: var = base + acc / k
    hipLaunchKernelGGL(var_finish_batch, grid_n, dim3(256), 0, h->stream, d_var, rb ? d_diag : (const double*)nullptr, 1.0 / (double)k, n, d_var);
    HIPCHK(hipGetLastError());
    return GMRF_OK;
}

static gmrf_status var_accumulate_dev(gmrf_handle* h, int method, int64_t first_id, int64_t k, uint64_t seed,
                                      const gmrf_csr* Q, double* d_acc) {
    for (int64_t c0 = 0; c0 < k; c0 += 64) {
        const int kc = (int)std::min<int64_t>(64, k - c0);
        GCHK(sample_chunk(h, seed, first_id + c0, kc, nullptr, 0, 0));
        GCHK(var_chunk(h, method, 0, kc, Q, nullptr, Q ? Q->d_diag : nullptr, d_acc));
    }
    return GMRF_OK;
}

// h->d_acc: room for the variances of B problems
static gmrf_status ensure_acc(gmrf_handle* h, int64_t B) {
    return h->d_acc.reserve(h->stream, (size_t)(h->n * B));
}

gmrf_status gmrf_bt_var_accumulate(gmrf_handle* h, int32_t method, int64_t first_id, int64_t k, uint64_t seed,
                                   const gmrf_csr* Q, double* acc) {
    h = tw_route(h);
    if (!h || !acc) return bad_shape("null pointer");
    if (!h->factored) { g_last_error = "variance before factor"; return GMRF_ERR_NO_FACTOR; }
    if (method != GMRF_VAR_RBMC && method != GMRF_VAR_MC) return bad_shape("accumulate needs RBMC or MC");
    if (method == GMRF_VAR_RBMC && (!Q || Q->n_rows != h->n || !Q->d_diag)) return bad_shape("RBMC needs the square matrix Q");
    if (k <= 0) return bad_shape("k <= 0");
    GCHK(need_single(h));
    HIPCHK(hipSetDevice(h->device));
    const bool dev = is_device_ptr(acc);
    GCHK(ensure_acc(h, 1));
    // h->d_acc: the accumulator a host acc is summed in, or the copy of a device acc as it came in (for the repeat)
    double* d_acc = dev ? acc : h->d_acc;
    GCHK(sweep_guarded(h, {}, [&]() -> gmrf_status {
        HIPCHK(hipMemcpyAsync(h->d_acc, acc, sizeof(double) * h->n, dev ? hipMemcpyDeviceToDevice : hipMemcpyHostToDevice, h->stream));
        GCHK(tw_on(h) ? tw_var_accumulate_dev(h, method, first_id, k, seed, Q, d_acc) : var_accumulate_dev(h, method, first_id, k, seed, Q, d_acc));
        HIPCHK(hipStreamSynchronize(h->stream));
        return GMRF_OK;
    }, [&]() -> gmrf_status {
        if (dev) HIPCHK(hipMemcpyAsync(acc, h->d_acc, sizeof(double) * h->n, hipMemcpyDeviceToDevice, h->stream));
        return GMRF_OK;
    }));
    if (!dev) {
        HIPCHK(hipMemcpyAsync(acc, d_acc, sizeof(double) * h->n, hipMemcpyDeviceToHost, h->stream));
        HIPCHK(hipStreamSynchronize(h->stream));
    }
    return GMRF_OK;
}

gmrf_status gmrf_bt_marginal_var(gmrf_handle* h, int32_t method, int64_t k, uint64_t seed, const gmrf_csr* Q,
                                 double* var_out) {
    h = tw_route(h);
    if (!h || !var_out) return bad_shape("null pointer");
    if (!h->factored) { g_last_error = "variance before factor"; return GMRF_ERR_NO_FACTOR; }
    if (method != GMRF_VAR_EXACT) {
        GCHK(need_single(h));                          // sampled estimators: one problem per handle
        if (method != GMRF_VAR_RBMC && method != GMRF_VAR_MC) return bad_shape("bad variance method");
        if (method == GMRF_VAR_RBMC && (!Q || Q->n_rows != h->n || !Q->d_diag)) return bad_shape("RBMC needs the square matrix Q");
        if (k <= 0) return bad_shape("k <= 0");
    }
    HIPCHK(hipSetDevice(h->device));
    GCHK(ensure_acc(h, h->B));
    const hipMemcpyKind kind = is_device_ptr(var_out) ? hipMemcpyDeviceToDevice : hipMemcpyDeviceToHost;
    GCHK(sweep_guarded(h, {}, [&]() -> gmrf_status {
        if (method == GMRF_VAR_EXACT) {
            GCHK(tw_on(h) ? tw_var_exact(h, h->d_acc) : var_exact(h, h->d_acc));      // selected inversion; var_out is [batch][n]
        } else {
            HIPCHK(hipMemsetAsync(h->d_acc, 0, sizeof(double) * h->n, h->stream));
            GCHK(tw_on(h) ? tw_var_accumulate_dev(h, method, 0, k, seed, Q, h->d_acc) : var_accumulate_dev(h, method, 0, k, seed, Q, h->d_acc));
            // finish in place: var = base + acc / k
            hipLaunchKernelGGL(var_finish, dim3((unsigned)((h->n + 255) / 256)), dim3(256), 0, h->stream, h->d_acc,
                               method == GMRF_VAR_RBMC ? Q->d_diag : (const double*)nullptr, 1.0 / (double)k, h->n, h->d_acc);
            HIPCHK(hipGetLastError());
        }
        HIPCHK(hipMemcpyAsync(var_out, h->d_acc, sizeof(double) * h->n * h->B, kind, h->stream));
        HIPCHK(hipStreamSynchronize(h->stream));
        return GMRF_OK;
    }));
    if (h->profiling) prof_collect(h);
    return GMRF_OK;
}

// Sampled marginal variances of every problem of a batch (the reference's per-problem
// `std(x_cond)` with RBMCStrategy(k), scripts/darcy/solve_darcy_gmrf-fem.jl:174,192).  Q gives the
// sparsity pattern (its values are not used); q_vals[p] are problem p's values in Q's CSR order --
// for a symmetric matrix the nzval array the factor was given.  Problem p draws the sample ids
// p * k .. p * k + k - 1, so problem 0 equals what a one-problem handle computes.
gmrf_status gmrf_bt_marginal_var_batch(gmrf_handle* h, int32_t method, int64_t k, uint64_t seed, const gmrf_csr* Q,
                                       const double* q_vals, double* var_out) {
    GCHK(tw_refuse(h, "gmrf_bt_marginal_var_batch"));
    if (!h || !var_out) return bad_shape("null pointer");
    if (!h->factored) { g_last_error = "variance before factor"; return GMRF_ERR_NO_FACTOR; }
    if (method != GMRF_VAR_RBMC && method != GMRF_VAR_MC) return bad_shape("batch variances: RBMC or MC (exact: gmrf_bt_marginal_var)");
    if (method == GMRF_VAR_RBMC && (!Q || Q->n_rows != h->n || Q->n_cols != h->n || !q_vals)) return bad_shape("RBMC needs the pattern of Q and its values per problem");
    if (k <= 0) return bad_shape("k <= 0");
    HIPCHK(hipSetDevice(h->device));
    const int64_t n = h->n, B = h->B;
    GCHK(ensure_acc(h, B));
    GCHK(sweep_guarded(h, {}, [&]() -> gmrf_status {     // (a batch of one: its sweeps may be persistent launches)
        DevArr<double> d_qv, d_diag;                     // (freed on every way out)
        const double* qv = q_vals;
        if (method == GMRF_VAR_RBMC) {
            if (!is_device_ptr(q_vals)) {
                GCHK(d_qv.upload(h->stream, q_vals, (size_t)(Q->nnz * B)));
                qv = d_qv;
            }
            GCHK(d_diag.reserve(h->stream, (size_t)(n * B)));
        }
        GCHK(var_batch_enqueue(h, method, k, seed, Q, qv, d_diag.get(), h->d_acc));
        const hipMemcpyKind kind = is_device_ptr(var_out) ? hipMemcpyDeviceToDevice : hipMemcpyDeviceToHost;
        HIPCHK(hipMemcpyAsync(var_out, h->d_acc, sizeof(double) * n * B, kind, h->stream));
        HIPCHK(hipStreamSynchronize(h->stream));
        return GMRF_OK;
    }));
    return GMRF_OK;
}

// the meeting block when the two halves' forms cost a and b per block: m a = (N - 1 - m) b.  Launch-per-step over persistent
// in-block form, per block: 1.51 measured on MI355X (darcy256 reference order: 20.22 ms with set_eager bit 13 -- persistent
// launches off -- against 13.38 ms, tools/twisted_latency.py), used as 1.5.
constexpr double TW_STEP_RATIO = 1.5;
static int64_t tw_auto_meet(int64_t N, bool top_persist, bool bot_persist) {
    if (N < 3) return N - 1;
    const double a = top_persist ? 1.0 : TW_STEP_RATIO, b = bot_persist ? 1.0 : TW_STEP_RATIO;
    const int64_t m = (int64_t)std::llround((double)(N - 1) * b / (a + b));
    return std::min<int64_t>(std::max<int64_t>(m, 1), N - 2);
}

// The handle's OWN factor (a reference-order one) is dropped: its claim on the device's persistent-launch budget (else the halves
// of a twisted factorisation would be refused it, and sweep_persist_ok would still let a call run persistent sweeps over the old
// buffers), its captured graphs, and its factor storage (re-allocated by the next reference-order factorisation; caller-owned
// storage is left to the caller).
static void tw_drop_own_factor(gmrf_handle* h) {
    (void)hipStreamSynchronize(h->stream);
    persist_release(h);
    destroy_graphs(h);
    h->factored = false;
    h->xsplit = 0;
    h->l_valid = h->logdet_valid = false;
    if (h->external_storage) return;
    release_factor(h);
    h->d_V.release();
    h->alloc_N = h->alloc_bsp = h->alloc_B = 0;
    h->stats.factor_bytes = 0;
}

static void tw_free(gmrf_handle* h) {
    TwistState* t = h->tw;
    if (!t) return;
    if (t->bot) (void)hipStreamSynchronize(t->bot->stream);
    (void)hipStreamSynchronize(h->stream);
    if (t->top) (void)gmrf_bt_destroy(t->top);
    if (t->bot) (void)gmrf_bt_destroy(t->bot);
    if (t->ev_fork) (void)hipEventDestroy(t->ev_fork);
    if (t->ev_join) (void)hipEventDestroy(t->ev_join);
    delete t;
    h->tw = nullptr;
}

static gmrf_status tw_new_half(gmrf_handle* h, hipStream_t st, gmrf_handle** out) {
    GCHK(gmrf_bt_create(h->device, (void*)st, out));
    GCHK(gmrf_bt_set_eager(*out, h->switches));
    (*out)->profiling = h->profiling;
    (*out)->tw_half = true;
    return GMRF_OK;
}

static gmrf_status tw_fork(gmrf_handle* h) {
    HIPCHK(hipEventRecord(h->tw->ev_fork, h->stream));
    HIPCHK(hipStreamWaitEvent(h->tw->bot->stream, h->tw->ev_fork, 0));
    return GMRF_OK;
}
static gmrf_status tw_join(gmrf_handle* h) {
    HIPCHK(hipEventRecord(h->tw->ev_join, h->tw->bot->stream));
    HIPCHK(hipStreamWaitEvent(h->stream, h->tw->ev_join, 0));
    return GMRF_OK;
}

// symbolic phase: the meeting block, both halves' entry lists (the bottom's fully reversed) and the meeting coupling's
static gmrf_status tw_analyze(gmrf_handle* h, int64_t n, int64_t N, const int64_t* colptr, const int64_t* rowval, int32_t base) {
    if (!colptr || !rowval) return bad_shape("null CSC arrays");
    if (h->B != 1) return bad_shape("the twisted order needs batch 1");
    tw_drop_own_factor(h);                     // (a reference-order factor of this handle, whatever way it came)
    GCHK(set_shape(h, n, N));                  // the handle's own shape: staging of host columns, normals
    h->analyzed = false;                       // (the handle's own pattern, if it had one, is not this factor's)
    if (h->meet_req > N - 1) return bad_shape("twisted order: meet must lie in [0, N_blocks - 1] (or -1: automatic)");
    const int64_t bs = h->bs;
    std::vector<std::vector<HostEntry>> dg, lo;
    GCHK(split_csc(n, N, bs, colptr, rowval, base, dg, lo));
    if (!h->tw) {
        h->tw = new TwistState();
        HIPCHK(hipEventCreateWithFlags(&h->tw->ev_fork, hipEventDisableTiming));
        HIPCHK(hipEventCreateWithFlags(&h->tw->ev_join, hipEventDisableTiming));
    }
    TwistState* t = h->tw;
    if (!t->top) GCHK(tw_new_half(h, h->stream, &t->top));
    int64_t m = h->meet_req;
    if (m < 0 && N < 3) m = N - 1;
    if (m < 0 || m < N - 1) {
        if (!t->bot) { GCHK(ensure_aux(h)); GCHK(tw_new_half(h, h->aux, &t->bot)); }
        // the halves never take the persistent sweep: it needs every CU while the other half runs
        for (gmrf_handle* s : {t->top, t->bot}) s->switches |= GMRF_SW_NO_SWEEP_PERSIST;
    }
    if (m < 0) {
        // automatic: which half's in-block Cholesky is the persistent form decides the balance (the CU budget holds one
        // 1024-block launch, not two); the routes depend on the block size, not on the number of blocks
        // (planned at the halves' block size without reshaping them: a new shape would drop their panels and graphs)
        const int64_t bsp = 64 * next_pow2((bs + 63) / 64);
        for (gmrf_handle* s : {t->top, t->bot}) {
            const int64_t keep = s->bsp;
            s->bsp = bsp;
            persist_plan(s);
            s->bsp = keep;
        }
        m = tw_auto_meet(N, t->top->persist_cus > 0, t->bot->persist_cus > 0);
    }
    if (m == N - 1 && t->bot) { (void)gmrf_bt_destroy(t->bot); t->bot = nullptr; }
    if (!t->bot) t->top->switches = h->switches;       // (the handle IS its top half: its own GMRF_SW_NO_SWEEP_PERSIST again)
    t->m = m; t->N = N; t->n = n; t->bs = bs; t->nnz = colptr[n] - base;
    const int64_t nnz = t->nnz;
    {   // top: blocks 0 .. m as they are
        std::vector<std::vector<HostEntry>> dgt(dg.begin(), dg.begin() + m + 1), lot(lo.begin(), lo.begin() + m + 1);
        GCHK(set_shape(t->top, (m + 1) * bs, m + 1));
        GCHK(upload_entries(t->top, dgt, lot, nnz));
    }
    t->top->tw_blk = -1; t->top->tw_hj = nullptr; t->top->tw_w = nullptr;
    t->bsp = t->top->bsp;
    if (!t->bot) return GMRF_OK;
    const int64_t Nb = N - 1 - m;
    {   // bottom: block j is block N-1-j, entry (r, c) of a block -> (bs-1-r, bs-1-c); diagonal entries transposed back to the
        // lower triangle, the coupling of bottom blocks j, j-1 is Q[N-1-j, N-j] = lo[N-j]^T
        std::vector<std::vector<HostEntry>> dgb((size_t)Nb), lob((size_t)Nb);
        for (int64_t j = 0; j < Nb; ++j) {
            for (const auto& e : dg[(size_t)(N - 1 - j)]) {
                const uint64_t r = e.key >> 32, c = e.key & 0xffffffffu;
                dgb[(size_t)j].push_back({((uint64_t)(bs - 1 - c) << 32) | (uint64_t)(bs - 1 - r), e.src});
            }
            if (j >= 1)
                for (const auto& e : lo[(size_t)(N - j)]) {
                    const uint64_t rho = e.key >> 32, gam = e.key & 0xffffffffu;
                    lob[(size_t)j].push_back({((uint64_t)(bs - 1 - gam) << 32) | (uint64_t)(bs - 1 - rho), e.src});
                }
        }
        GCHK(set_shape(t->bot, Nb * bs, Nb));
        GCHK(upload_entries(t->bot, dgb, lob, nnz));
    }
    {   // the meeting coupling: Q[rho, gamma] of lo[m+1] is B-hat[gamma][bs-1-rho]
        std::vector<uint64_t> keys;
        std::vector<int64_t> src;
        for (const auto& e : lo[(size_t)(m + 1)]) {
            const uint64_t rho = e.key >> 32, gam = e.key & 0xffffffffu;
            keys.push_back((gam << 32) | (uint64_t)(bs - 1 - rho));
            src.push_back(e.src);
        }
        t->m_count = (int64_t)keys.size();
        GCHK(reserve_group(h->stream, {t->d_mkeys.want(keys.size()), t->d_msrc.want(keys.size()), t->d_mvals.want(keys.size())}));
        if (!keys.empty()) {
            GCHK(t->d_mkeys.upload(h->stream, keys));
            GCHK(t->d_msrc.upload(h->stream, src));
            HIPCHK(hipStreamSynchronize(h->stream));
        }
    }
    const size_t be = (size_t)(t->bsp * t->bsp);
    GCHK(reserve_group(h->stream, {t->d_Bm.want(be), t->d_HJ.want(be), t->d_W.want(be), t->d_Smm.want(be)}));
    return t->d_var.reserve(h->stream, (size_t)(Nb * bs));        // (d_z and d_nz follow n / nnz at their first use)
}

// HJ = B-hat L'^-T of the bottom half's last block (= J C'), on the bottom half's stream
static gmrf_status tw_meeting_coupling(gmrf_handle* h) {
    TwistState* t = h->tw;
    gmrf_handle* bot = t->bot;
    const int bsp = (int)t->bsp;
    HIPCHK(hipMemsetAsync(t->d_Bm, 0, sizeof(double) * (size_t)bsp * bsp, bot->stream));
    if (t->m_count > 0) {
        hipLaunchKernelGGL(gather_values, dim3((unsigned)((t->m_count + 255) / 256), 1), dim3(256), 0, bot->stream, t->d_nz_cur, t->d_msrc,
                           t->m_count, t->d_mvals, t->nnz);
        HIPCHK(hipGetLastError());
        hipLaunchKernelGGL(scatter_block, dim3((unsigned)((t->m_count + 255) / 256), 1), dim3(256), 0, bot->stream, t->d_mkeys, t->d_mvals,
                           (int64_t)0, t->m_count, t->d_Bm, (int64_t)bsp, t->m_count, (int64_t)0, 0);
        HIPCHK(hipGetLastError());
    }
    const double* X = bot->d_Linv + (bot->N - 1) * (int64_t)bsp * bsp;
    GCHK(gemm(bot, GemmCall(false, false, bsp, bsp, bsp, 1.0, 0.0).a(t->d_Bm, bsp, 0).b(X, bsp, 0).c(t->d_HJ, bsp, 0)));
    return GMRF_OK;
}

// numeric phase: bottom chain + meeting coupling on the second stream, top chain up to the meeting block on this one, then the
// meeting block; a persistent launch that gave up goes through each half's own repeat
static gmrf_status tw_numeric(gmrf_handle* h, const double* nzval, int32_t* info) {
    TwistState* t = h->tw;
    if (!t || !t->top || !t->top->analyzed) { g_last_error = "no sparsity pattern analysed"; return GMRF_ERR_NO_FACTOR; }
    if (!nzval) return bad_shape("null nzval");
    h->factored = false;
    gmrf_handle *top = t->top, *bot = t->bot;
    if (!bot) {
        gmrf_status s = numeric_factor(top, nzval, info);
        h->factored = top->factored;
        h->stats.factor_ms = top->stats.factor_ms;
        return s;
    }
    const int64_t m = t->m, Nb = bot->N, N = t->N;
    const double* d_nz = nzval;
    if (!is_device_ptr(nzval)) {
        GCHK(t->d_nz.upload(h->stream, nzval, (size_t)t->nnz));
        d_nz = t->d_nz;
    }
    t->d_nz_cur = d_nz;
    for (gmrf_handle* s : {top, bot}) {
        GCHK(alloc_factor(s));
        if (s->c_dirty) {
            HIPCHK(hipMemsetAsync(s->d_C, 0, sizeof(double) * stride_pC(s) * s->B, s->stream));
            s->c_dirty = false;
        }
        persist_plan(s);
        s->factored = false;
    }
    top->tw_blk = m; top->tw_hj = t->d_HJ; top->tw_w = t->d_W;
    HIPCHK(hipEventRecord(h->ev0, h->stream));
    GCHK(tw_fork(h));
    // second stream: the bottom chain, then the meeting coupling
    GCHK(load_values(bot, d_nz));
    HIPCHK(hipMemsetAsync(bot->d_info, 0, 4 * sizeof(int), bot->stream));
    bot->info_checked = 0; bot->persist_launched = false;
    GCHK(run_factor(bot, 0, Nb));
    GCHK(tw_meeting_coupling(h));
    // this stream: the top chain up to the meeting block, which waits for the coupling
    GCHK(load_values(top, d_nz));
    HIPCHK(hipMemsetAsync(top->d_info, 0, 4 * sizeof(int), top->stream));
    top->info_checked = 0; top->persist_launched = false;
    if (m > 0) GCHK(run_factor(top, 0, m));
    GCHK(tw_join(h));
    GCHK(factor_blocks_range(top, m, m + 1));
    HIPCHK(hipEventRecord(h->ev1, h->stream));
    int ib = 0, it = 0;
    const int aborts_bot = bot->persist_aborts;
    GCHK(persist_check_range(bot, 0, Nb, &ib));
    if (bot->persist_aborts != aborts_bot) {
        // the bottom chain was repeated: its coupling and the whole top half (whose meeting block read the old one) again
        HIPCHK(hipStreamSynchronize(h->stream));
        GCHK(tw_meeting_coupling(h));
        HIPCHK(hipStreamSynchronize(bot->stream));
        HIPCHK(hipMemsetAsync(top->d_info, 0, 4 * sizeof(int), top->stream));
        top->info_checked = 0;
        GCHK(factor_blocks_range(top, 0, m + 1));
    }
    GCHK(persist_check_range(top, 0, m + 1, &it));
    float ms = 0.f;
    (void)hipEventElapsedTime(&ms, h->ev0, h->ev1);
    h->stats.factor_ms = ms;
    top->stats.factor_ms = ms; bot->stats.factor_ms = ms;
    if (top->profiling) prof_collect(top);
    if (bot->profiling) prof_collect(bot);
    int64_t fail = 0;
    if (it >= 1 && it <= m) fail = it;                 // the top chain (its numbering is the original one)
    else if (ib != 0) fail = N + 1 - ib;               // the bottom chain: its block j is block N-1-j
    else if (it == m + 1) fail = m + 1;                // the meeting block
    if (info) *info = (int32_t)fail;
    if (fail) {
        g_last_error = "matrix is not positive definite; failed block " + std::to_string(fail) + " (twisted order, meeting block " +
                       std::to_string(m + 1) + ")";
        return GMRF_ERR_NOT_SPD;
    }
    for (gmrf_handle* s : {top, bot}) { s->factored = true; s->l_valid = s->keep_l; s->logdet_valid = !s->keep_l; }
    h->factored = true;
    return GMRF_OK;
}

// the caller's columns (device, leading dimension ld) -> both panels; src == nullptr: Philox normals of samples first_id + r
static gmrf_status tw_fill(gmrf_handle* h, const double* d_src, int64_t ld, int k, int kp, uint64_t seed, int64_t first_id) {
    TwistState* t = h->tw;
    const int64_t total = (int64_t)kp * (t->top->n_pad + t->bot->n_pad);
    hipLaunchKernelGGL(tw_fill_panels, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, h->stream, d_src, ld, t->top->d_P,
                       t->top->n_pad, t->bot->d_P, t->bot->n_pad, (int)t->bs, (int)t->bsp, t->n, k, kp, seed, first_id);
    HIPCHK(hipGetLastError());
    return GMRF_OK;
}

// both halves' panels (P: full solve, Y: otherwise) -> the caller's (dst, ld), plus d_mean; host dst through d_stage
static gmrf_status tw_cols_out(gmrf_handle* h, bool from_p, int k, const double* d_mean, double* dst, int64_t ld, bool dst_dev) {
    TwistState* t = h->tw;
    const double* pt = from_p ? t->top->d_P : t->top->d_Y;
    const double* pb = from_p ? t->bot->d_P : t->bot->d_Y;
    double* d = dst;
    int64_t ldd = ld;
    if (!dst_dev) { GCHK(ensure_stage(h, (int64_t)k * h->n)); d = h->d_stage; ldd = h->n; }
    const int64_t total = t->n * (int64_t)k;
    hipLaunchKernelGGL(tw_unpack_panels, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, h->stream, pt, t->top->n_pad, pb,
                       t->bot->n_pad, d, ldd, (int)t->bs, (int)t->bsp, t->n, (t->m + 1) * t->bs, k, d_mean);
    HIPCHK(hipGetLastError());
    if (!dst_dev)
        HIPCHK(hipMemcpy2DAsync(dst, ld * sizeof(double), h->d_stage, h->n * sizeof(double), h->n * sizeof(double), k,
                                hipMemcpyDeviceToHost, h->stream));
    return GMRF_OK;
}

static gmrf_status tw_couple_launch(gmrf_handle* h, bool trans, int kp, const double* src, int64_t lds, double* dst, int64_t ldd) {
    const int bsp = (int)h->tw->bsp;
    const dim3 grid((unsigned)(bsp / 64), (unsigned)((kp + 15) / 16));
    if (trans) hipLaunchKernelGGL(tw_couple<true>, grid, dim3(256), 0, h->stream, h->tw->d_W, bsp, src, lds, dst, ldd, kp);
    else hipLaunchKernelGGL(tw_couple<false>, grid, dim3(256), 0, h->stream, h->tw->d_W, bsp, src, lds, dst, ldd, kp);
    HIPCHK(hipGetLastError());
    return GMRF_OK;
}

// mode FORWARD: P -> Y (T^-1), BACKWARD: P -> Y (T^-T), FULL: P -> Y -> P; both halves' sweeps run at the same time
static gmrf_status tw_sweeps(gmrf_handle* h, int mode, int kp) {
    TwistState* t = h->tw;
    gmrf_handle *top = t->top, *bot = t->bot;
    const int64_t om = t->m * t->bsp, ol = (bot->N - 1) * t->bsp;
    if (mode == GMRF_SOLVE_BACKWARD) {
        GCHK(tw_couple_launch(h, true, kp, top->d_P + om, top->n_pad, bot->d_P + ol, bot->n_pad));
        GCHK(tw_fork(h));
        GCHK(run_sweeps(top, GMRF_SOLVE_BACKWARD, kp));
        GCHK(run_sweeps(bot, GMRF_SOLVE_BACKWARD, kp));
        return tw_join(h);
    }
    GCHK(tw_fork(h));
    GCHK(run_sweeps(top, GMRF_SOLVE_FORWARD, kp));
    GCHK(run_sweeps(bot, GMRF_SOLVE_FORWARD, kp));
    GCHK(tw_join(h));
    GCHK(tw_couple_launch(h, false, kp, bot->d_Y + ol, bot->n_pad, top->d_Y + om, top->n_pad));
    if (mode == GMRF_SOLVE_FORWARD) return GMRF_OK;
    GCHK(tw_couple_launch(h, true, kp, top->d_Y + om, top->n_pad, bot->d_Y + ol, bot->n_pad));
    GCHK(tw_fork(h));
    GCHK(run_sweeps(top, SWEEP_BACKWARD_YP, kp));
    GCHK(run_sweeps(bot, SWEEP_BACKWARD_YP, kp));
    return tw_join(h);
}

static gmrf_status tw_panels(gmrf_handle* h, int kp) {
    GCHK(ensure_panels(h->tw->top, kp));
    GCHK(ensure_panels(h->tw->bot, kp));
    return GMRF_OK;
}

static gmrf_status tw_solve(gmrf_handle* h, const double* b, double* y, int64_t k, int64_t ldb, int64_t ldy, int mode) {
    const bool b_dev = is_device_ptr(b), y_dev = is_device_ptr(y);
    h->stats.solve_ms = 0.0;
    for (int64_t c0 = 0; c0 < k; c0 += KP_CHUNK) {
        const int kc = (int)std::min<int64_t>(KP_CHUNK, k - c0);
        const int kp = pad_k(kc);
        GCHK(tw_panels(h, kp));
        const double* d_b = nullptr;
        int64_t ld_b = 0;
        GCHK(cols_in(h, b + c0 * ldb, ldb, b_dev, kc, &d_b, &ld_b));
        GCHK(tw_fill(h, d_b, ld_b, kc, kp, 0, 0));
        HIPCHK(hipEventRecord(h->ev0, h->stream));
        GCHK(tw_sweeps(h, mode, kp));
        HIPCHK(hipEventRecord(h->ev1, h->stream));
        GCHK(tw_cols_out(h, mode == GMRF_SOLVE_FULL, kc, nullptr, y + c0 * ldy, ldy, y_dev));
        HIPCHK(hipStreamSynchronize(h->stream));
        float ms = 0.f;
        (void)hipEventElapsedTime(&ms, h->ev0, h->ev1);
        h->stats.solve_ms += ms;
        h->stats.sweep_ms = ms / ((mode == GMRF_SOLVE_FULL) ? 2 : 1);
        h->stats.sweep_bytes = sweep_bytes(h, kc);
    }
    return GMRF_OK;
}

// samples [first_id, first_id + kc) (or the caller's z) -> both panels -> T^-T z in the Y panels
static gmrf_status tw_sample_chunk(gmrf_handle* h, uint64_t seed, int64_t first_id, int kc, const double* z, int64_t ldz) {
    const int kp = pad_k(kc);
    GCHK(tw_panels(h, kp));
    const double* d_z = nullptr;
    int64_t ldd = 0;
    if (z) GCHK(cols_in(h, z, ldz, is_device_ptr(z), kc, &d_z, &ldd));
    GCHK(tw_fill(h, d_z, ldd, kc, kp, seed, first_id));
    return tw_sweeps(h, GMRF_SOLVE_BACKWARD, kp);
}

static gmrf_status tw_sample(gmrf_handle* h, uint64_t seed, int64_t first_id, int64_t k, const double* mean, const double* z,
                             double* out, int64_t ld) {
    const double* d_mean = nullptr;
    Staging args(h->mean_arena);
    args.in(mean, sizeof(double) * h->n * h->B, &d_mean);
    GCHK(args.commit(h->stream));
    const bool out_dev = is_device_ptr(out);
    HIPCHK(hipEventRecord(h->ev0, h->stream));
    for (int64_t c0 = 0; c0 < k; c0 += KP_CHUNK) {
        const int kc = (int)std::min<int64_t>(KP_CHUNK, k - c0);
        GCHK(tw_sample_chunk(h, seed, first_id + c0, kc, z ? z + c0 * ld : nullptr, ld));
        GCHK(tw_cols_out(h, false, kc, d_mean, out + c0 * ld, ld, out_dev));
        if (!out_dev) HIPCHK(hipStreamSynchronize(h->stream));
    }
    HIPCHK(hipEventRecord(h->ev1, h->stream));
    HIPCHK(hipStreamSynchronize(h->stream));
    float ms = 0.f;
    (void)hipEventElapsedTime(&ms, h->ev0, h->ev1);
    h->stats.sample_ms = ms;
    return GMRF_OK;
}

// exact variances: the top half's own recurrence (it starts at Sigma_mm = L_m^-T L_m^-1) on this stream; on the second stream the
// bottom half's, seeded with  Sigma' = L'^-T (I + HJ^T Sigma_mm HJ) L'^-1  for its last block (block m+1, reversed)
static gmrf_status tw_var_exact(gmrf_handle* h, double* d_out) {
    TwistState* t = h->tw;
    gmrf_handle *top = t->top, *bot = t->bot;
    const int bsp = (int)t->bsp;
    const int64_t bstride = (int64_t)bsp * bsp;
    GCHK(ensure_full_inverse(top)); GCHK(ensure_full_inverse(bot));
    GCHK(tw_fork(h));
    {
        const double* Xm = top->d_Linv + t->m * bstride;
        const double* Xl = bot->d_Linv + (bot->N - 1) * bstride;
        GCHK(gemm(bot, GemmCall(true, true, bsp, bsp, bsp, 1.0, 0.0).a(Xm, bsp, 0).b(Xm, bsp, 0).c(t->d_Smm, bsp, 0)));           // Sigma_mm
        GCHK(gemm(bot, GemmCall(false, true, bsp, bsp, bsp, 1.0, 0.0).a(t->d_Smm, bsp, 0).b(t->d_HJ, bsp, 0).c(bot->d_W, bsp, 0)));  // Sigma_mm HJ
        GCHK(gemm(bot, GemmCall(true, true, bsp, bsp, bsp, 1.0, 0.0).a(t->d_HJ, bsp, 0).b(bot->d_W, bsp, 0).c(bot->d_B, bsp, 0)));  // HJ^T Sigma_mm HJ
        hipLaunchKernelGGL(add_identity, dim3((unsigned)((bsp + 255) / 256)), dim3(256), 0, bot->stream, bot->d_B, (int64_t)bsp, bsp);
        HIPCHK(hipGetLastError());
        GCHK(gemm(bot, GemmCall(false, true, bsp, bsp, bsp, 1.0, 0.0).a(bot->d_B, bsp, 0).b(Xl, bsp, 0).c(bot->d_T, bsp, 0)));       // (I + M) L'^-1
        GCHK(gemm(bot, GemmCall(true, true, bsp, bsp, bsp, 1.0, 0.0).a(Xl, bsp, 0).b(bot->d_T, bsp, 0).c(bot->d_S, bsp, 0)));        // Sigma'
        GCHK(var_exact(bot, t->d_var, true));
        const int64_t cnt = bot->N * t->bs;
        hipLaunchKernelGGL(tw_reverse, dim3((unsigned)((cnt + 255) / 256)), dim3(256), 0, bot->stream, t->d_var, d_out + (t->m + 1) * t->bs, cnt);
        HIPCHK(hipGetLastError());
    }
    GCHK(var_exact(top, d_out));
    return tw_join(h);
}

// sampled variances: chunks of 64 twisted samples (no mean), column-major in d_z, into the accumulator (var_chunk)
static gmrf_status tw_var_accumulate_dev(gmrf_handle* h, int method, int64_t first_id, int64_t k, uint64_t seed, const gmrf_csr* Q,
                                         double* d_acc) {
    TwistState* t = h->tw;
    GCHK(t->d_z.reserve(h->stream, (size_t)(64 * t->n)));
    for (int64_t c0 = 0; c0 < k; c0 += 64) {
        const int kc = (int)std::min<int64_t>(64, k - c0);
        GCHK(tw_sample_chunk(h, seed, first_id + c0, kc, nullptr, 0));
        GCHK(tw_cols_out(h, false, kc, nullptr, t->d_z, t->n, true));
        GCHK(var_chunk(h, method, 0, kc, Q, nullptr, Q ? Q->d_diag : nullptr, d_acc, t->d_z, t->n, t->n, t->n));
    }
    return GMRF_OK;
}

static gmrf_status tw_logdet(gmrf_handle* h, double* out) {
    double a = 0.0, b = 0.0;
    GCHK(gmrf_bt_logdet(h->tw->top, &a));
    GCHK(gmrf_bt_logdet(h->tw->bot, &b));
    *out = a + b;
    return GMRF_OK;
}

// blocks of T in original coordinates: a bottom block is J (block of the reversed chain) J
static gmrf_status tw_get_block(gmrf_handle* h, int32_t kind, int64_t i, double* out, int64_t ld) {
    TwistState* t = h->tw;
    const int64_t N = t->N, m = t->m, bs = t->bs, bsp = t->bsp;
    if (ld < bs) return bad_shape("ld < block_size");
    std::vector<double> tmp((size_t)(bs * bs)), res((size_t)(bs * bs));     // column-major, leading dimension bs
    bool flip = false;
    if (kind == GMRF_BLOCK_L || kind == GMRF_BLOCK_LINV) {
        if (i < 0 || i >= N) return bad_shape("block index");
        if (i <= m) GCHK(gmrf_bt_get_block(t->top, kind, i, tmp.data(), bs));
        else { GCHK(gmrf_bt_get_block(t->bot, kind, N - 1 - i, tmp.data(), bs)); flip = true; }
    } else if (kind == GMRF_BLOCK_C) {
        if (i < 0 || i >= N - 1) return bad_shape("block index");
        if (i < m) GCHK(gmrf_bt_get_block(t->top, kind, i, tmp.data(), bs));                  // G_{i+1}
        else if (i > m) { GCHK(gmrf_bt_get_block(t->bot, kind, N - 2 - i, tmp.data(), bs)); flip = true; }   // H_i
        else {                                                                                 // H_m = HJ J
            std::vector<double> hj((size_t)(bsp * bsp));
            HIPCHK(hipMemcpyAsync(hj.data(), t->d_HJ, hj.size() * sizeof(double), hipMemcpyDeviceToHost, h->stream));
            HIPCHK(hipStreamSynchronize(h->stream));
            for (int64_t c = 0; c < bs; ++c)
                for (int64_t r = 0; r < bs; ++r) tmp[(size_t)(c * bs + r)] = hj[(size_t)(r * bsp + (bs - 1 - c))];
        }
    } else return bad_shape("bad block kind");
    for (int64_t c = 0; c < bs; ++c)
        for (int64_t r = 0; r < bs; ++r)
            res[(size_t)(c * bs + r)] = flip ? tmp[(size_t)((bs - 1 - c) * bs + (bs - 1 - r))] : tmp[(size_t)(c * bs + r)];
    HIPCHK(hipMemcpy2DAsync(out, ld * sizeof(double), res.data(), bs * sizeof(double), bs * sizeof(double), bs, hipMemcpyDefault, h->stream));
    HIPCHK(hipStreamSynchronize(h->stream));
    return GMRF_OK;
}

gmrf_status gmrf_bt_set_order(gmrf_handle* h, int32_t order, int64_t meet) {
    if (!h) return bad_shape("null handle");
    if (order != GMRF_ORDER_REFERENCE && order != GMRF_ORDER_TWISTED) return bad_shape("unknown elimination order");
    if (meet < -1) return bad_shape("twisted order: meet must be -1 (automatic) or a block index");
    if (order == GMRF_ORDER_TWISTED && h->B != 1) return bad_shape("the twisted order needs batch 1");
    HIPCHK(hipSetDevice(h->device));
    HIPCHK(hipStreamSynchronize(h->stream));
    tw_free(h);
    tw_drop_own_factor(h);
    h->order = order;
    h->meet_req = meet;
    return GMRF_OK;
}

gmrf_status gmrf_bt_get_order(gmrf_handle* h, int32_t* order, int64_t* meet) {
    if (!h || !order || !meet) return bad_shape("null pointer");
    *order = h->order;
    if (h->order == GMRF_ORDER_TWISTED) *meet = (h->tw && h->tw->m >= 0) ? h->tw->m : h->meet_req;
    else *meet = h->N > 0 ? h->N - 1 : -1;
    return GMRF_OK;
}

gmrf_status gmrf_bt_half_stats(gmrf_handle* h, int32_t half, gmrf_stats* out) {
    if (!h || !out) return bad_shape("null pointer");
    if (h->order != GMRF_ORDER_TWISTED || !h->tw || !h->tw->top) return bad_shape("gmrf_bt_half_stats: not a factored twisted handle");
    if (half != 0 && half != 1) return bad_shape("half must be 0 (top) or 1 (bottom)");
    if (half == 1 && !h->tw->bot) { memset(out, 0, sizeof(*out)); return GMRF_OK; }
    *out = (half == 0 ? h->tw->top : h->tw->bot)->stats;
    return GMRF_OK;
}

// --------------------------------------------------------------------------------- test hooks
gmrf_status gmrf_test_gemm(int32_t device, int64_t M, int64_t N, int64_t K, int32_t transA, int32_t transB,
                           int32_t tri_flags, int32_t lower_only, double alpha, const double* A, int64_t lda,
                           const double* B, int64_t ldb, double beta, double* C, int64_t ldc) {
    if (M % 64 || N % 64 || K % 16 || (lda & 1) || (ldb & 1)) return bad_shape("gemm test sizes");
    // bit 65536: the 64 x 64 LDS-DMA kernel with the tail row (gemm_f64_dma TAIL): A and C hold M + 1 rows, row M summed on the VALU
    const bool tail = (tri_flags & 65536) != 0;
    if (tail && (transA || transB)) return bad_shape("gemm test: the tail row needs A [m][k] and B [k][n]");
    HIPCHK(hipSetDevice(device));
    const int64_t a_rows = transA ? K : M + (tail ? 1 : 0), b_rows = transB ? N : K, c_rows = M + (tail ? 1 : 0);
    double *dA, *dB, *dC;
    HIPCHK(hipMalloc(&dA, sizeof(double) * a_rows * lda));
    HIPCHK(hipMalloc(&dB, sizeof(double) * b_rows * ldb));
    HIPCHK(hipMalloc(&dC, sizeof(double) * c_rows * ldc));
    HIPCHK(hipMemcpy(dA, A, sizeof(double) * a_rows * lda, hipMemcpyHostToDevice));
    HIPCHK(hipMemcpy(dB, B, sizeof(double) * b_rows * ldb, hipMemcpyHostToDevice));
    HIPCHK(hipMemcpy(dC, C, sizeof(double) * c_rows * ldc, hipMemcpyHostToDevice));
    GemmArgs g;
    g.A = dA; g.B = dB; g.C = dC; g.lda = lda; g.ldb = ldb; g.ldc = ldc;
    g.strideA = g.strideB = g.strideC = 0;
    g.pA = g.pB = g.pC = 0; g.nb1 = 1;
    g.D = nullptr; g.ldd = 0; g.pD = 0;
    // tri_flags bit 2048: take the 128 x 128 kernel whatever the tile count
    // bit 4096: the 32 x 32 low-latency kernel (taken by launches of <= 128 tiles of 64 x 64)
    // bits 8192 / 16384 / 32768: the LDS-DMA kernel with 64 x 64 / 128 x 64 / 64 x 128 tiles (gemm_f64_dma.hpp); none of
    // them: the register-staged kernels only
    const bool force_big = (tri_flags & 2048) != 0, use_ll = (tri_flags & 4096) != 0;
    const int dma_shape = (tri_flags & 8192) ? 1 : ((tri_flags & 16384) ? 2 : ((tri_flags & 32768) ? 3 : 0));
    g.M = (int)M; g.N = (int)N; g.K = (int)K; g.tri = tri_flags & ~(2048 | 4096 | 8192 | 16384 | 32768 | 65536); g.lower_only = lower_only;
    g.alpha = alpha; g.beta = beta;
    unsigned long long* dst = nullptr;
    HIPCHK(hipMalloc(&dst, 16));
    HIPCHK(hipMemset(dst, 0, 16));
    g.stamps = (force_big || use_ll || dma_shape || tail) ? nullptr : dst;
    HIPCHK(gemm_init());
    HIPCHK(gemm_dma_init());
    if (tail) {
        const int saved_dma = gemm_dma_policy(), saved_ll = gemm_ll_policy();
        gemm_dma_policy() = 1; gemm_ll_policy() = 2;
        hipError_t le = hipSuccess;
        const bool ok = gemm_try_dma_tail(nullptr, false, true, g, 1, nullptr, nullptr, &le);
        gemm_dma_policy() = saved_dma; gemm_ll_policy() = saved_ll;
        if (!ok) { hipFree(dst); hipFree(dA); hipFree(dB); hipFree(dC); return bad_shape("gemm test: not a tail-row product"); }
        HIPCHK(le);
        HIPCHK(hipDeviceSynchronize());
        HIPCHK(hipMemcpy(C, dC, sizeof(double) * c_rows * ldc, hipMemcpyDeviceToHost));
        hipFree(dst); hipFree(dA); hipFree(dB); hipFree(dC);
        return GMRF_OK;
    }
    const int saved = gemm_big_policy(), saved_ll = gemm_ll_policy(), saved_dma = gemm_dma_policy(), saved_force = gemm_dma_force();
    gemm_big_policy() = force_big ? 1 : 2;
    gemm_ll_policy() = use_ll ? 0 : 2;
    gemm_dma_policy() = dma_shape ? 2 : 0;
    gemm_dma_force() = dma_shape;
    // BLAS-style flags: op(A) is M x K, op(B) is K x N; B "not transposed" is stored K x N
    hipError_t le = launch_gemm(nullptr, transA != 0, transB == 0, g, 1);
    gemm_big_policy() = saved; gemm_ll_policy() = saved_ll; gemm_dma_policy() = saved_dma; gemm_dma_force() = saved_force;
    HIPCHK(le);
    HIPCHK(hipDeviceSynchronize());
    HIPCHK(hipMemcpy(C, dC, sizeof(double) * M * ldc, hipMemcpyDeviceToHost));
    HIPCHK(hipMemcpy(g_tile_stamps, dst, 16, hipMemcpyDeviceToHost));
    hipFree(dst);
    hipFree(dA); hipFree(dB); hipFree(dC);
    return GMRF_OK;
}

// Two products C_i = beta_i C_i + alpha_i A_i b_i of `batch` problems each (host arrays, contiguous per problem: A [M][K], B [K][N] if
// b_n else [N][K], C [M][N]) on the 64 x 64 LDS-DMA kernel: grouped != 0 as ONE launch of gemm_f64_dma_grouped, else as two launches.
// desc: M, N, K, b_n, tri, lower_only of product 0, then of product 1; ab: alpha_0, beta_0, alpha_1, beta_1.
gmrf_status gmrf_test_gemm_pair(int32_t device, int32_t batch, int32_t grouped, const int64_t* desc, const double* ab,
                                const double* A0, const double* B0, double* C0, const double* A1, const double* B1, double* C1) {
    if (!desc || !ab || !A0 || !B0 || !C0 || !A1 || !B1 || !C1 || batch < 1) return bad_shape("gemm pair test: null pointer / batch");
    HIPCHK(hipSetDevice(device));
    HIPCHK(gemm_init());
    HIPCHK(gemm_dma_init());
    const double* hA[2] = {A0, A1};
    const double* hB[2] = {B0, B1};
    double* hC[2] = {C0, C1};
    double *dA[2] = {nullptr, nullptr}, *dB[2] = {nullptr, nullptr}, *dC[2] = {nullptr, nullptr};
    GemmArgs g[2];
    bool b_n[2];
    auto drop = [&]() { for (int i = 0; i < 2; ++i) { (void)hipFree(dA[i]); (void)hipFree(dB[i]); (void)hipFree(dC[i]); } };
    for (int i = 0; i < 2; ++i) {
        const int64_t M = desc[6 * i], N = desc[6 * i + 1], K = desc[6 * i + 2];
        b_n[i] = desc[6 * i + 3] != 0;
        if (M <= 0 || N <= 0 || K <= 0 || M % 64 || N % 64 || K % 16) { drop(); return bad_shape("gemm pair test sizes"); }
        const size_t na = sizeof(double) * M * K * batch, nb = sizeof(double) * K * N * batch, nc = sizeof(double) * M * N * batch;
        hipError_t e = hipMalloc(&dA[i], na);
        if (e == hipSuccess) e = hipMalloc(&dB[i], nb);
        if (e == hipSuccess) e = hipMalloc(&dC[i], nc);
        if (e == hipSuccess) e = hipMemcpy(dA[i], hA[i], na, hipMemcpyHostToDevice);
        if (e == hipSuccess) e = hipMemcpy(dB[i], hB[i], nb, hipMemcpyHostToDevice);
        if (e == hipSuccess) e = hipMemcpy(dC[i], hC[i], nc, hipMemcpyHostToDevice);
        if (e != hipSuccess) { drop(); HIPCHK(e); }
        GemmArgs& a = g[i];
        a.A = dA[i]; a.B = dB[i]; a.C = dC[i]; a.lda = K; a.ldb = b_n[i] ? N : K; a.ldc = N;
        a.strideA = a.strideB = a.strideC = 0;
        a.pA = M * K; a.pB = K * N; a.pC = M * N; a.nb1 = 1;
        a.M = (int)M; a.N = (int)N; a.K = (int)K; a.tri = (int)desc[6 * i + 4]; a.lower_only = (int)desc[6 * i + 5];
        a.alpha = ab[2 * i]; a.beta = ab[2 * i + 1]; a.D = nullptr; a.ldd = 0; a.pD = 0; a.stamps = nullptr;
    }
    const int saved = gemm_big_policy(), saved_ll = gemm_ll_policy(), saved_dma = gemm_dma_policy(), saved_force = gemm_dma_force();
    gemm_big_policy() = 2; gemm_ll_policy() = 2; gemm_dma_policy() = 2; gemm_dma_force() = 1;
    hipError_t le = hipSuccess;
    bool ok = true;
    if (grouped) ok = gemm_try_dma_grouped(nullptr, b_n[0], g[0], b_n[1], g[1], batch, nullptr, nullptr, &le);
    else {
        for (int i = 0; i < 2 && ok && le == hipSuccess; ++i) ok = gemm_try_dma(nullptr, false, b_n[i], g[i], batch, nullptr, nullptr, &le);
    }
    gemm_big_policy() = saved; gemm_ll_policy() = saved_ll; gemm_dma_policy() = saved_dma; gemm_dma_force() = saved_force;
    if (!ok) { drop(); return bad_shape("gemm pair test: not a pair of LDS-DMA products"); }
    if (le == hipSuccess) le = hipDeviceSynchronize();
    for (int i = 0; i < 2 && le == hipSuccess; ++i)
        le = hipMemcpy(hC[i], dC[i], sizeof(double) * g[i].M * g[i].N * batch, hipMemcpyDeviceToHost);
    drop();
    HIPCHK(le);
    return GMRF_OK;
}

// One launch of a fully general GemmArgs on ONE chosen route (tests/test_gpu_gemm_desc.py).  Host buffers are copied whole, the
// descriptor is checked against their sizes before anything is launched (furthest element addressed per operand), C / tC / the
// direct-out arrays come back whole.  desc (28 x int64): M, N, K, transA, b_n, tri, lower_only, batch, nb1, lda, ldb, ldc, ldd,
// strideA, strideB, strideC, pA, pB, pC, pD, ptA, ptC, ptD, o_j0, o_n, o_cols, o_ld, o_k.  abt: alpha, beta, tbeta.
// route: 0 register-staged 64 x 64, 1 the 128 x 128 kernel, 2 the 32 x 32 one, 3 / 4 / 5 LDS-DMA 64 x 64 / 128 x 64 / 64 x 128,
// 6 the tail-row product (row M of A / C / D unless tC is given; samples != nullptr: with the direct output), 7 launch_gemm's
// own choice with every policy at its default.  *family: 1 / 2 register-staged at BK 16 / 32 (+ 256: single stage), 3 the
// 128 x 128 kernel, 4 the 32 x 32 one, 5 / 6 / 7 LDS-DMA by tile shape, 8 tail row, 9 tail row with direct output.  A forced
// route the descriptor does not qualify for is GMRF_ERR_BAD_SHAPE and launches nothing.  The family is this hook's statement of
// launch_gemm's order of questions (gemm_uses_big, gemm_dma_shape, gemm_uses_ll, K % 32, grid.x > 768).
// (ke_m, grouped: gmrf_test_gemm_env below)
static gmrf_status gemm_desc_run(int32_t device, int32_t route, const int64_t* desc, const double* abt,
                                 const double* A, int64_t nA, const double* B, int64_t nB, double* C, int64_t nC,
                                 const double* D, int64_t nD, const double* tA, int64_t ntA, double* tC, int64_t ntC,
                                 const double* tD, int64_t ntD, const int32_t* kb_m, int64_t n_kb_m, const int32_t* kb_n,
                                 int64_t n_kb_n, const int32_t* ke_n, int64_t n_ke_n, double* samples, int64_t n_samples,
                                 double* mean, int64_t n_mean, int32_t* family, const int32_t* ke_m, int64_t n_ke_m, int32_t grouped,
                                 int32_t strict_lower = 0) {
    if (!desc || !abt || !A || !B || !C || !family) return bad_shape("gemm desc test: null pointer");
    if (strict_lower != 0 && strict_lower != 1) return bad_shape("gemm desc test: strict_lower is 0 or 1");
    if (strict_lower && (desc[6] != 1 || desc[0] != desc[1])) return bad_shape("gemm desc test: strict_lower needs a square lower-only product");
    *family = 0;
    const int64_t M = desc[0], N = desc[1], K = desc[2];
    const bool a_t = desc[3] != 0, b_n = desc[4] != 0;
    const int64_t tri = desc[5], lower_only = desc[6], batch = desc[7], nb1 = desc[8];
    const int64_t lda = desc[9], ldb = desc[10], ldc = desc[11], ldd = desc[12];
    const int64_t sA = desc[13], sB = desc[14], sC = desc[15], pA = desc[16], pB = desc[17], pC = desc[18], pD = desc[19];
    const int64_t ptA = desc[20], ptC = desc[21], ptD = desc[22], o_j0 = desc[23], o_n = desc[24], o_cols = desc[25];
    const int64_t o_ld = desc[26], o_k = desc[27];
    if (route < 0 || route > 7) return bad_shape("gemm desc test: unknown route");
    if (M <= 0 || N <= 0 || K <= 0 || M % 64 || N % 64 || K % 16 || M > 16384 || N > 16384 || K > 16384)
        return bad_shape("gemm desc test: sizes");
    if (tri < 0 || tri > 15 || (lower_only != 0 && lower_only != 1)) return bad_shape("gemm desc test: tri / lower_only");
    if (batch < 1 || nb1 < 1 || batch % nb1 || batch > 4096) return bad_shape("gemm desc test: batch is not a multiple of nb1");
    const int64_t strides[] = {sA, sB, sC, pA, pB, pC, pD, ptA, ptC, ptD};
    for (int64_t s : strides)
        if (s < 0 || s > ((int64_t)1 << 40)) return bad_shape("gemm desc test: negative stride");
    const bool tail = route == 6, own_tail = tail && tC != nullptr, dout = tail && samples != nullptr;
    if (!tail && (tA || tC || tD || samples || mean)) return bad_shape("gemm desc test: tail operands without the tail route");
    if (dout && (!mean || own_tail)) return bad_shape("gemm desc test: direct output");
    if (!dout && mean) return bad_shape("gemm desc test: mean without samples");
    if (own_tail && !tA) return bad_shape("gemm desc test: tC without tA");
    if (!own_tail && (tA || tD)) return bad_shape("gemm desc test: tA / tD without tC");
    const int64_t rows = M + ((tail && !own_tail) ? 1 : 0);      // rows of A (stored [m][k]) / C / D
    if (lda < (a_t ? M : K) || ldb < (b_n ? N : K) || ldc < N || (D && ldd < N) || lda > ((int64_t)1 << 24) || ldb > ((int64_t)1 << 24) ||
        ldc > ((int64_t)1 << 24) || ldd > ((int64_t)1 << 24))
        return bad_shape("gemm desc test: leading dimension");
    // the furthest element each operand is addressed at (all strides >= 0) must lie inside its buffer
    const int64_t np = batch / nb1, zin = (nb1 - 1), zout = (np - 1);
    const int64_t needA = zin * sA + zout * pA + (a_t ? (K - 1) * lda + M : (rows - 1) * lda + K);
    const int64_t needB = zin * sB + zout * pB + (b_n ? (K - 1) * ldb + N : (N - 1) * ldb + K);
    const int64_t needC = zin * sC + zout * pC + (rows - 1) * ldc + N;
    const int64_t needD = zout * pD + (rows - 1) * ldd + N;
    if (needA > nA || needB > nB || needC > nC || (D && needD > nD)) return bad_shape("gemm desc test: operand buffer too small");
    if (own_tail && (zout * ptA + K > ntA || zout * ptC + N > ntC || (tD && zout * ptD + N > ntD)))
        return bad_shape("gemm desc test: tail buffer too small");
    if ((kb_m && n_kb_m < M / 64) || (kb_n && n_kb_n < N / 64) || (ke_n && n_ke_n < N / 64) || (ke_m && n_ke_m < M / 64))
        return bad_shape("gemm desc test: K bounds too short");
    if (grouped < 0 || grouped > 2 || (grouped && route != 3)) return bad_shape("gemm desc test: grouped launches are of the 64 x 64 LDS-DMA kernel");
    const int32_t* kbs[4] = {kb_m, kb_n, ke_n, ke_m};
    const int64_t nkb[4] = {M / 64, N / 64, N / 64, M / 64};
    for (int a = 0; a < 4; ++a)
        for (int64_t i = 0; kbs[a] && i < nkb[a]; ++i)
            if (kbs[a][i] < 0 || kbs[a][i] > K || kbs[a][i] % 64) return bad_shape("gemm desc test: K bound value");
    if (dout) {
        if (o_k < 0 || o_k > M || o_cols < 0 || o_cols > N || o_j0 < 0 || o_ld < 0 || o_n < 0 || o_ld > ((int64_t)1 << 24) || o_n > ((int64_t)1 << 30))
            return bad_shape("gemm desc test: direct-out fields");
        if (o_cols > 0 && o_k > 0 && (zout * o_k + o_k - 1) * o_ld + o_j0 + o_cols > n_samples) return bad_shape("gemm desc test: samples too small");
        if (o_cols > 0 && zout * o_n + o_j0 + o_cols > n_mean) return bad_shape("gemm desc test: mean too small");
    }
    HIPCHK(hipSetDevice(device));
    HIPCHK(gemm_init());
    HIPCHK(gemm_dma_init());

    std::vector<void*> owned;
    auto drop = [&]() { for (void* p : owned) (void)hipFree(p); owned.clear(); };
    hipError_t e = hipSuccess;
    auto up = [&](const void* host, int64_t count, size_t elem) -> void* {
        if (!host || e != hipSuccess) return nullptr;
        void* d = nullptr;
        e = hipMalloc(&d, std::max<size_t>((size_t)count * elem, 16));
        if (e != hipSuccess) return nullptr;
        owned.push_back(d);
        if (count > 0) e = hipMemcpy(d, host, (size_t)count * elem, hipMemcpyHostToDevice);
        return d;
    };
    GemmArgs g;
    g.A = (const double*)up(A, nA, 8); g.B = (const double*)up(B, nB, 8); g.C = (double*)up(C, nC, 8);
    g.D = (const double*)up(D, nD, 8);
    g.tA = (const double*)up(tA, ntA, 8); g.tC = (double*)up(tC, ntC, 8); g.tD = (const double*)up(tD, ntD, 8);
    g.kb_m = (const int*)up(kb_m, n_kb_m, 4); g.kb_n = (const int*)up(kb_n, n_kb_n, 4); g.ke_n = (const int*)up(ke_n, n_ke_n, 4);
    g.ke_m = (const int*)up(ke_m, n_ke_m, 4);
    double* d_samples = (double*)up(samples, n_samples, 8);
    double* d_mean = (double*)up(mean, n_mean, 8);
    GemmDirectOut* d_out = nullptr;
    if (dout && e == hipSuccess) {
        e = hipMalloc(&d_out, sizeof(GemmDirectOut));
        if (e == hipSuccess) {
            owned.push_back(d_out);
            hipLaunchKernelGGL(set_direct_out, dim3(1), dim3(1), 0, nullptr, d_out, d_samples, d_mean, o_ld, o_k);
            e = hipGetLastError();
        }
    }
    if (e != hipSuccess) { drop(); HIPCHK(e); }
    g.lda = lda; g.ldb = ldb; g.ldc = ldc; g.ldd = D ? ldd : 0;
    g.strideA = sA; g.strideB = sB; g.strideC = sC; g.pA = pA; g.pB = pB; g.pC = pC; g.pD = D ? pD : 0;
    g.nb1 = (int)nb1; g.M = (int)M; g.N = (int)N; g.K = (int)K; g.tri = (int)tri; g.lower_only = (int)lower_only;
    g.alpha = abt[0]; g.beta = abt[1]; g.tbeta = abt[2];
    g.ptA = ptA; g.ptC = ptC; g.ptD = ptD;
    g.stamps = nullptr;
    g.dout = d_out; g.o_j0 = o_j0; g.o_n = o_n; g.o_cols = (int)o_cols;
    g.strict_lower = strict_lower;

    const int saved_big = gemm_big_policy(), saved_ll = gemm_ll_policy(), saved_dma = gemm_dma_policy(), saved_force = gemm_dma_force();
    auto restore = [&]() { gemm_big_policy() = saved_big; gemm_ll_policy() = saved_ll; gemm_dma_policy() = saved_dma; gemm_dma_force() = saved_force; };
    // route:                   0  1  2  3  4  5  6  7
    static const int big_p[] = {2, 1, 2, 2, 2, 2, 2, 0};
    static const int ll_p[] = {2, 2, 0, 2, 2, 2, 2, 0};
    static const int dma_p[] = {0, 0, 0, 2, 2, 2, 1, 2};
    static const int force_p[] = {0, 0, 0, 1, 2, 3, 0, 0};
    gemm_big_policy() = big_p[route]; gemm_ll_policy() = ll_p[route]; gemm_dma_policy() = dma_p[route]; gemm_dma_force() = force_p[route];
    const int nz = (int)batch;
    int fam;
    hipError_t le = hipSuccess;
    if (tail) {
        fam = gemm_try_dma_tail(nullptr, a_t, b_n, g, nz, nullptr, nullptr, &le) ? (dout ? 9 : 8) : 0;     // (false: nothing launched)
    } else {
        // (the order launch_gemm asks in)
        if (gemm_uses_big(a_t, g, nz)) fam = 3;
        else if (!gemm_uses_ll(g, nz) && gemm_dma_shape(a_t, g, nz) != 0) fam = 4 + gemm_dma_shape(a_t, g, nz);
        else if (gemm_uses_ll(g, nz)) fam = 4;
        else {
            const bool tri_grid = lower_only && M == N;
            const int64_t sx = N / GEMM_BN, sy = M / GEMM_BM;
            fam = (K % 32 == 0 ? 2 : 1) + ((tri_grid ? sx * (sx + 1) / 2 : sx * sy) * batch > 768 ? 256 : 0);
        }
        static const int want[] = {0, 3, 4, 5, 6, 7};
        if (route == 0 ? (fam & 255) > 2 : (route < 6 && fam != want[route])) fam = 0;
        if (fam && grouped) {
            // the descriptor as the first / second product of a grouped launch; the other is its copy on an output buffer of its own
            GemmArgs g2 = g;
            g2.C = (double*)up(C, nC, 8);
            le = e;
            if (le == hipSuccess && !gemm_try_dma_grouped(nullptr, b_n, grouped == 1 ? g : g2, b_n, grouped == 1 ? g2 : g, nz, nullptr, nullptr, &le)) fam = 0;
        } else if (fam) le = launch_gemm(nullptr, a_t, b_n, g, nz);
    }
    restore();
    if (!fam) { drop(); return bad_shape("gemm desc test: the descriptor does not qualify for the route"); }
    if (le == hipSuccess) le = hipDeviceSynchronize();
    if (le == hipSuccess) le = hipMemcpy(C, g.C, sizeof(double) * nC, hipMemcpyDeviceToHost);
    if (le == hipSuccess && own_tail) le = hipMemcpy(tC, g.tC, sizeof(double) * ntC, hipMemcpyDeviceToHost);
    if (le == hipSuccess && dout && n_samples > 0) le = hipMemcpy(samples, d_samples, sizeof(double) * n_samples, hipMemcpyDeviceToHost);
    if (le == hipSuccess && dout && n_mean > 0) le = hipMemcpy(mean, d_mean, sizeof(double) * n_mean, hipMemcpyDeviceToHost);
    drop();
    HIPCHK(le);
    *family = fam;
    return GMRF_OK;
}

gmrf_status gmrf_test_gemm_desc(int32_t device, int32_t route, const int64_t* desc, const double* abt,
                                const double* A, int64_t nA, const double* B, int64_t nB, double* C, int64_t nC,
                                const double* D, int64_t nD, const double* tA, int64_t ntA, double* tC, int64_t ntC,
                                const double* tD, int64_t ntD, const int32_t* kb_m, int64_t n_kb_m, const int32_t* kb_n,
                                int64_t n_kb_n, const int32_t* ke_n, int64_t n_ke_n, double* samples, int64_t n_samples,
                                double* mean, int64_t n_mean, int32_t* family) {
    return gemm_desc_run(device, route, desc, abt, A, nA, B, nB, C, nC, D, nD, tA, ntA, tC, ntC, tD, ntD, kb_m, n_kb_m, kb_n, n_kb_n,
                         ke_n, n_ke_n, samples, n_samples, mean, n_mean, family, nullptr, 0, 0);
}
// gmrf_test_gemm_desc with GemmArgs::ke_m (upper K bound per 64-row tile of A: M / 64 values, multiples of 64) and, grouped = 1 / 2
// (route 3 only), the descriptor as the first / second product of ONE gemm_f64_dma_grouped launch beside a copy of itself.
gmrf_status gmrf_test_gemm_env(int32_t device, int32_t route, const int64_t* desc, const double* abt,
                               const double* A, int64_t nA, const double* B, int64_t nB, double* C, int64_t nC,
                               const double* D, int64_t nD, const double* tA, int64_t ntA, double* tC, int64_t ntC,
                               const double* tD, int64_t ntD, const int32_t* kb_m, int64_t n_kb_m, const int32_t* kb_n,
                               int64_t n_kb_n, const int32_t* ke_n, int64_t n_ke_n, const int32_t* ke_m, int64_t n_ke_m,
                               int32_t grouped, int32_t* family) {
    return gemm_desc_run(device, route, desc, abt, A, nA, B, nB, C, nC, D, nD, tA, ntA, tC, ntC, tD, ntD, kb_m, n_kb_m, kb_n, n_kb_n,
                         ke_n, n_ke_n, nullptr, 0, nullptr, 0, family, ke_m, n_ke_m, grouped);
}
// gmrf_test_gemm_env with GemmArgs::strict_lower (0 / 1; 1 needs lower_only = 1 and M == N).  The 64 x 64 LDS-DMA launches --
// route 3, its grouped forms and the tail route 6 -- then leave, in every diagonal tile, the six 16 x 16 blocks above its block
// diagonal (B stored [n][k]) or the quadrant rows 0 .. 31 x columns 32 .. 63 (B stored [k][n]) as C held them; the other routes
// take the field and write whole tiles.
gmrf_status gmrf_test_gemm_sym(int32_t device, int32_t route, const int64_t* desc, const double* abt,
                               const double* A, int64_t nA, const double* B, int64_t nB, double* C, int64_t nC,
                               const double* D, int64_t nD, const double* tA, int64_t ntA, double* tC, int64_t ntC,
                               const double* tD, int64_t ntD, const int32_t* kb_m, int64_t n_kb_m, const int32_t* kb_n,
                               int64_t n_kb_n, const int32_t* ke_n, int64_t n_ke_n, const int32_t* ke_m, int64_t n_ke_m,
                               int32_t grouped, int32_t strict_lower, int32_t* family) {
    return gemm_desc_run(device, route, desc, abt, A, nA, B, nB, C, nC, D, nD, tA, ntA, tC, ntC, tD, ntD, kb_m, n_kb_m, kb_n, n_kb_n,
                         ke_n, n_ke_n, nullptr, 0, nullptr, 0, family, ke_m, n_ke_m, grouped, strict_lower);
}
// Process-wide: enabled = 0 makes every launcher drop GemmArgs::strict_lower (whole diagonal tiles, the launches of before round
// 29), 1 (the default) honours it.  Read when a launch is issued -- for a handle, when its factor graph is captured.
gmrf_status gmrf_test_strict_lower(int32_t enabled) {
    if (enabled != 0 && enabled != 1) return bad_shape("gmrf_test_strict_lower: 0 or 1");
    gemm_strict_lower_off() = enabled ? 0 : 1;
    return GMRF_OK;
}
// The envelope bounds of the analysed pattern (gmrf_handle::env_lo / env_hi: [n_blocks][bsp / 64], in-block columns) and what the
// factorisation does with them: *state = 0 none computed (blocks not a multiple of 256), 1 computed but trivial for every panel
// (every launch as without them), 2 in use.  *n_vals = values per array (may exceed cap).
gmrf_status gmrf_test_envelope(gmrf_handle* h, int32_t* lo, int32_t* hi, int64_t cap, int64_t* n_vals, int32_t* state) {
    if (!h || !n_vals || !state) return bad_shape("null argument");
    const int64_t want = h->N * (h->bsp / 64);
    const bool have = h->bsp % 256 == 0 && (int64_t)h->env_lo.size() == want && h->analyzed;
    *n_vals = have ? want : 0;
    *state = !have ? 0 : (h->env_ok ? 2 : 1);
    for (int64_t i = 0; have && lo && hi && i < std::min(cap, want); ++i) { lo[i] = h->env_lo[(size_t)i]; hi[i] = h->env_hi[(size_t)i]; }
    return GMRF_OK;
}

// rows of 11 doubles per distinct GEMM launch shape seen while profiling was on: class, M, N, K, tri, lower_only, problems,
// per-tile K bounds?, launches, ms, work (flops as booked in kernel_work).  *n_rows = rows available (may exceed cap_rows).
gmrf_status gmrf_test_gemm_shapes(gmrf_handle* h, double* rows, int64_t cap_rows, int64_t* n_rows) {
    if (!h || !n_rows) return bad_shape("null argument");
    HIPCHK(hipStreamSynchronize(h->stream));
    prof_collect(h);
    *n_rows = (int64_t)h->gemm_shapes.size();
    for (int64_t i = 0; rows && i < std::min<int64_t>(cap_rows, *n_rows); ++i) {
        const auto& g = h->gemm_shapes[(size_t)i];
        for (int c = 0; c < 8; ++c) rows[i * 11 + c] = (double)g.key[c];
        rows[i * 11 + 8] = g.launches; rows[i * 11 + 9] = g.ms; rows[i * 11 + 10] = g.work;
    }
    return GMRF_OK;
}

// Shader clock under load: _start launches clock_probe_kernel on a stream of its own and returns; the caller
// runs the load under test on its streams; _finish waits for the probe and returns, per sample interval, the clock in GHz
// (median over the probe's 8 waves) and the interval's start in ms since the first sample.  ghz / t_ms: n - 1 values.
struct ClockProbe { int device; hipStream_t st; unsigned long long* d; int n; };
gmrf_status gmrf_test_clock_probe_start(int32_t device, int32_t n, int32_t sleeps, void** probe) {
    if (!probe || n < 2 || n > 100000 || sleeps < 1 || sleeps > 64) return bad_shape("clock probe: 2 <= n <= 100000, 1 <= sleeps <= 64");
    HIPCHK(hipSetDevice(device));
    ClockProbe* p = new ClockProbe{device, nullptr, nullptr, n};
    auto drop = [&](hipError_t e) {                 // (no probe, stream or buffer is left behind on an error path: ADVICE r4)
        if (p->d) (void)hipFree(p->d);
        if (p->st) (void)hipStreamDestroy(p->st);
        delete p;
        g_last_error = std::string("clock probe: ") + hipGetErrorString(e);
        return GMRF_ERR_HIP;
    };
    hipError_t e = hipStreamCreateWithFlags(&p->st, hipStreamNonBlocking);
    if (e == hipSuccess) e = hipMalloc(&p->d, sizeof(unsigned long long) * 2 * 8 * (size_t)n);
    if (e == hipSuccess) e = hipMemsetAsync(p->d, 0, sizeof(unsigned long long) * 2 * 8 * (size_t)n, p->st);
    if (e != hipSuccess) return drop(e);
    hipLaunchKernelGGL(clock_probe_kernel, dim3(8), dim3(64), 0, p->st, p->d, n, sleeps);
    if ((e = hipGetLastError()) != hipSuccess) return drop(e);
    *probe = p;
    return GMRF_OK;
}
gmrf_status gmrf_test_clock_probe_finish(void* probe, double* ghz, double* t_ms) {
    ClockProbe* p = static_cast<ClockProbe*>(probe);
    if (!p || !ghz) return bad_shape("null pointer");
    std::vector<unsigned long long> h((size_t)2 * 8 * p->n);
    hipError_t e = hipSetDevice(p->device);
    if (e == hipSuccess) e = hipStreamSynchronize(p->st);
    if (e == hipSuccess) e = hipMemcpy(h.data(), p->d, h.size() * sizeof(unsigned long long), hipMemcpyDeviceToHost);
    if (e != hipSuccess) {
        (void)hipFree(p->d); (void)hipStreamDestroy(p->st);
        delete p;
        g_last_error = std::string("clock probe: ") + hipGetErrorString(e);
        return GMRF_ERR_HIP;
    }
    for (int i = 0; i + 1 < p->n; ++i) {
        double v[8];
        for (int b = 0; b < 8; ++b) {
            const unsigned long long* a = &h[((size_t)b * p->n + i) * 2];
            const double dc = (double)(a[2] - a[0]), dr = (double)(a[3] - a[1]);
            v[b] = dr > 0 ? dc / dr * 0.1 : 0.0;
        }
        std::sort(v, v + 8);
        ghz[i] = 0.5 * (v[3] + v[4]);
        if (t_ms) t_ms[i] = (double)(h[(size_t)i * 2 + 1] - h[1]) * 1e-5;
    }
    (void)hipFree(p->d); (void)hipStreamDestroy(p->st);
    delete p;
    return GMRF_OK;
}

gmrf_status gmrf_test_gemm_rate(int32_t device, int64_t M, int64_t N, int64_t K, int32_t transB, int32_t tri_flags,
                                int32_t lower_only, int32_t batch, int32_t big, int32_t reps, double* ms_per_launch) {
    if (M % 64 || N % 64 || K % 16 || batch < 1 || reps < 1) return bad_shape("gemm rate sizes");
    HIPCHK(hipSetDevice(device));
    const int64_t ld = std::max(std::max(M, N), K);
    const int64_t pm = ld * ld;
    double *dA, *dB, *dC;
    HIPCHK(hipMalloc(&dA, sizeof(double) * pm * batch));
    HIPCHK(hipMalloc(&dB, sizeof(double) * pm * batch));
    HIPCHK(hipMalloc(&dC, sizeof(double) * pm * batch));
    const int64_t tot = pm * batch;
    hipLaunchKernelGGL(fill_normals_panel, dim3((unsigned)((tot + 255) / 256)), dim3(256), 0, nullptr, dA, tot, 1 << 30,
                       1 << 30, 1, 1, 1ull, 0, 0, nullptr, (int64_t)0);
    hipLaunchKernelGGL(fill_normals_panel, dim3((unsigned)((tot + 255) / 256)), dim3(256), 0, nullptr, dB, tot, 1 << 30,
                       1 << 30, 1, 1, 2ull, 0, 0, nullptr, (int64_t)0);
    HIPCHK(hipMemset(dC, 0, sizeof(double) * pm * batch));
    GemmArgs g;
    g.A = dA; g.B = dB; g.C = dC; g.lda = g.ldb = g.ldc = ld;
    g.strideA = g.strideB = g.strideC = 0;
    g.pA = g.pB = g.pC = pm; g.nb1 = 1;
    g.D = nullptr; g.ldd = 0; g.pD = 0;
    g.M = (int)M; g.N = (int)N; g.K = (int)K; g.tri = tri_flags; g.lower_only = lower_only;
    g.alpha = 1.0; g.beta = 0.0; g.stamps = nullptr;
    HIPCHK(gemm_init());
    HIPCHK(gemm_dma_init());
    const int saved = gemm_big_policy(), saved_dma = gemm_dma_policy(), saved_force = gemm_dma_force();
    gemm_big_policy() = big == 1 ? 1 : (big == 2 ? 0 : 2);       // big = 2: the model's choice
    // big = 3 / 4 / 5: the LDS-DMA kernel with 64 x 64 / 128 x 64 / 64 x 128 tiles; 6: the production choice (all policies at their defaults)
    gemm_dma_policy() = big >= 3 ? 2 : 0;
    gemm_dma_force() = (big >= 3 && big <= 5) ? big - 2 : 0;
    if (big == 6) gemm_big_policy() = 0;
    hipEvent_t e0, e1;
    HIPCHK(hipEventCreate(&e0)); HIPCHK(hipEventCreate(&e1));
    hipError_t le = hipSuccess;
    for (int r = 0; r < 3 && le == hipSuccess; ++r) le = launch_gemm(nullptr, false, transB == 0, g, batch);
    HIPCHK(hipEventRecord(e0, nullptr));
    for (int r = 0; r < reps && le == hipSuccess; ++r) le = launch_gemm(nullptr, false, transB == 0, g, batch);
    HIPCHK(hipEventRecord(e1, nullptr));
    gemm_big_policy() = saved; gemm_dma_policy() = saved_dma; gemm_dma_force() = saved_force;
    HIPCHK(le);
    HIPCHK(hipEventSynchronize(e1));
    float ms = 0.f;
    HIPCHK(hipEventElapsedTime(&ms, e0, e1));
    *ms_per_launch = ms / reps;
    hipEventDestroy(e0); hipEventDestroy(e1);
    hipFree(dA); hipFree(dB); hipFree(dC);
    return GMRF_OK;
}

gmrf_status gmrf_test_potrf_tile(int32_t device, double* tile64, double* inv64, int32_t* info) {
    HIPCHK(hipSetDevice(device));
    double *dS, *dL, *dX;
    int* dinfo;
    HIPCHK(hipMalloc(&dS, sizeof(double) * 4096));
    HIPCHK(hipMalloc(&dL, sizeof(double) * 4096));
    HIPCHK(hipMalloc(&dX, sizeof(double) * 4096));
    HIPCHK(hipMalloc(&dinfo, sizeof(int)));
    HIPCHK(hipMemset(dinfo, 0, sizeof(int)));
    HIPCHK(hipMemcpy(dS, tile64, sizeof(double) * 4096, hipMemcpyHostToDevice));
    auto kern = potrf_tile_kernel;
    const dim3 tpb(256);
    (void)hipFuncSetAttribute((const void*)kern, hipFuncAttributeMaxDynamicSharedMemorySize, (int)POTRF_TILE_LDS);
    unsigned long long* dstamps;
    HIPCHK(hipMalloc(&dstamps, 64 * sizeof(unsigned long long)));
    HIPCHK(hipMemset(dstamps, 0, 64 * sizeof(unsigned long long)));
    hipLaunchKernelGGL(kern, dim3(1), tpb, POTRF_TILE_LDS, nullptr, dS, dL, dX, dinfo, (unsigned long long*)nullptr);
    HIPCHK(hipDeviceSynchronize());
    {   // timing: 200 back-to-back launches without stamps, then one stamped launch
        hipEvent_t e0, e1; HIPCHK(hipEventCreate(&e0)); HIPCHK(hipEventCreate(&e1));
        HIPCHK(hipEventRecord(e0, nullptr));
        for (int i = 0; i < 200; ++i)
            hipLaunchKernelGGL(kern, dim3(1), tpb, POTRF_TILE_LDS, nullptr, dS, dL, dX, dinfo, (unsigned long long*)nullptr);
        HIPCHK(hipEventRecord(e1, nullptr)); HIPCHK(hipEventSynchronize(e1));
        float ms = 0.f; HIPCHK(hipEventElapsedTime(&ms, e0, e1));
        g_tile_us = ms * 1e3 / 200.0;
        hipEventDestroy(e0); hipEventDestroy(e1);
    }
    hipLaunchKernelGGL(kern, dim3(1), tpb, POTRF_TILE_LDS, nullptr, dS, dL, dX, dinfo, dstamps);
    HIPCHK(hipDeviceSynchronize());
    HIPCHK(hipMemcpy(g_tile_stamps, dstamps, 64 * sizeof(unsigned long long), hipMemcpyDeviceToHost));
    hipFree(dstamps);
    HIPCHK(hipGetLastError());
    HIPCHK(hipDeviceSynchronize());
    HIPCHK(hipMemcpy(tile64, dL, sizeof(double) * 4096, hipMemcpyDeviceToHost));
    HIPCHK(hipMemcpy(inv64, dX, sizeof(double) * 4096, hipMemcpyDeviceToHost));
    int hi = 0;
    HIPCHK(hipMemcpy(&hi, dinfo, sizeof(int), hipMemcpyDeviceToHost));
    if (info) *info = hi;
    hipFree(dS); hipFree(dL); hipFree(dX); hipFree(dinfo);
    return GMRF_OK;
}

// diagnostics of the last gmrf_test_potrf_tile: out[0] = us per launch, out[1..17] = s_memtime stamps (cycles, relative)
gmrf_status gmrf_test_tile_timing(double* out, int32_t n) {
    if (!out || n < 18) return bad_shape("need 18 outputs");
    out[0] = g_tile_us;
    for (int i = 0; i < 17; ++i) out[1 + i] = (double)(g_tile_stamps[i] - g_tile_stamps[15]);
    if (n >= 24) for (int i = 0; i < 3; ++i) out[18 + i] = (double)(g_tile_stamps[20 + i] - g_tile_stamps[15]);
    if (n >= 30) for (int i = 0; i < 6; ++i) out[24 + i] = (double)(g_tile_stamps[24 + i] - g_tile_stamps[24]);   // fused step phases (gmrf_test_potrf_block)
    // round 5: per panel p (up to 8) three stamps of its owner wave: its column chain begins / is done / its columns are stored
    if (n >= 62) for (int i = 0; i < 8; ++i) out[54 + i] = g_tile_stamps[56 + i] ? (double)(g_tile_stamps[56 + i] - g_tile_stamps[15]) : -1.0;   // panel i: its owner has applied every earlier column
    if (n >= 54) for (int i = 0; i < 24; ++i) out[30 + i] = g_tile_stamps[32 + i] ? (double)(g_tile_stamps[32 + i] - g_tile_stamps[15]) : -1.0;
    return GMRF_OK;
}

// s_memtime stamps of the chain workgroup of the last gmrf_test_potrf_block that ran the persistent form: out[0] = after tile 0,
// then per step j four stamps (flags seen, operands in LDS, tile updated, tile j + 1 published), relative to the first, in cycles
gmrf_status gmrf_test_persist_stamps(double* out, int32_t n) {
    if (!out || n < 1 || n > 128) return bad_shape("1 .. 128 outputs");
    // (slot 8 s + 5 holds a small number, not a time: the panel in which the next step's operands were seen ready)
    for (int i = 0; i < n; ++i)
        out[i] = g_persist_stamps[i] ? (g_persist_stamps[i] < 64 ? (double)g_persist_stamps[i] : (double)(g_persist_stamps[i] - g_persist_stamps[0])) : -1.0;
    return GMRF_OK;
}

// How often a factorisation of this handle saw the abort word of its persistent launches (a bounded wait gave up) and was
// repeated with the launch-per-step form (tests force it with GMRF_PERSIST_SPIN_MS=0).
// 1 if the current factor holds y = L^-1 b for the registered b (gmrf_bt_set_factor_rhs), else 0; y_out (optional, host, n x B
// column-major) receives that y
gmrf_status gmrf_test_factor_fwd(gmrf_handle* h, int32_t* state, double* y_out) {
    if (!h || !state) return bad_shape("null pointer");
    HIPCHK(hipSetDevice(h->device));
    *state = (h->fy_for && h->factored && h->fy_for == h->frhs) ? 1 : 0;
    if (y_out && *state) {
        GCHK(cols_out(h, h->d_fy, 1, nullptr, y_out, h->n, false));
        HIPCHK(hipStreamSynchronize(h->stream));
    }
    return GMRF_OK;
}

// The last gmrf_gn_run: its iterations, and how many of them took y = L^-1 rhs from the factorisation (the forward-in-factor route)
gmrf_status gmrf_test_gn_route(gmrf_gn* g, int32_t* iterations, int32_t* fwd_iterations) {
    if (!g || !iterations || !fwd_iterations) return bad_shape("null pointer");
    *iterations = g->iterations; *fwd_iterations = g->fwd_iterations;
    return GMRF_OK;
}

// The last gmrf_dc_run: 1 if its factorisation carried the forward sweep of the information vector (the forward-in-factor route)
gmrf_status gmrf_test_dc_route(gmrf_dc* g, int32_t* fwd_in_factor) {
    if (!g || !fwd_in_factor) return bad_shape("null pointer");
    *fwd_in_factor = g->fwd_in_factor;
    return GMRF_OK;
}

// The last gmrf_bic_run: 1 if its factorisation carried the forward sweep of Qx_prior (the forward-in-factor route)
gmrf_status gmrf_test_bic_route(gmrf_bic* g, int32_t* fwd_in_factor) {
    if (!g || !fwd_in_factor) return bad_shape("null pointer");
    *fwd_in_factor = g->fwd_in_factor;
    return GMRF_OK;
}

// The last batched sampled estimator of this handle (gmrf_bt_marginal_var_batch, gmrf_dc_run): problems per group of the stage
// and groups per chunk, as GMRF_VAR_STAGE_MB sized them
gmrf_status gmrf_test_var_groups(gmrf_handle* h, int32_t* group_size, int32_t* groups) {
    if (!h || !group_size || !groups) return bad_shape("null pointer");
    *group_size = h->var_group; *groups = h->var_groups;
    return GMRF_OK;
}

gmrf_status gmrf_test_persist_aborts(gmrf_handle* h, int32_t* n) {
    if (!h || !n) return bad_shape("null argument");
    *n = h->persist_aborts;
    return GMRF_OK;
}

// The budget of CUs for persistent launches on a device with `cus` CUs, host only: `n` handles claim demands[i] CUs one after
// the other; granted[i] = 1 if the claim fitted beside the earlier ones (gmrf_handle::persist_cus), 0 if it was refused.
gmrf_status gmrf_test_persist_budget(int32_t cus, int32_t n, const int32_t* demands, int32_t* granted) {
    if (n < 0 || (n > 0 && (!demands || !granted))) return bad_shape("null argument");
    std::map<const void*, int> claims;
    for (int i = 0; i < n; ++i) granted[i] = persist_budget_claim(claims, (const void*)(demands + i), demands[i], cus) ? 1 : 0;
    return GMRF_OK;
}

gmrf_status gmrf_test_potrf_block(int32_t device, int64_t bs, double* S, double* Linv, int32_t* info) {
    if (bs % 64 || next_pow2(bs / 64) != bs / 64) return bad_shape("bs must be 64 * 2^p");
    gmrf_handle* h = nullptr;
    GCHK(gmrf_bt_create(device, nullptr, &h));
    h->N = 1; h->n = bs; h->bs = bs; h->bsp = bs; h->n_pad = bs; h->B = 1;
    gmrf_status s = set_layout_dense(h);
    if (s == GMRF_OK) s = alloc_factor(h);
    unsigned long long* dst = nullptr;
    if (s == GMRF_OK && hipMalloc(&dst, 128 * sizeof(unsigned long long)) == hipSuccess) {
        (void)hipMemset(dst, 0, 128 * sizeof(unsigned long long));
        h->dbg_stamps = dst;
    }
    if (s == GMRF_OK) {
        hipError_t e = hipMemcpyAsync(h->d_S, S, sizeof(double) * bs * bs, hipMemcpyHostToDevice, h->stream);
        persist_plan(h);
        if (e == hipSuccess) s = potrf_block(h, h->d_S, h->d_L, h->d_Linv, h->d_T, 1);
        if (s == GMRF_OK) {
            int hi = 0;
            (void)hipMemcpyAsync(&hi, h->d_info, sizeof(int), hipMemcpyDeviceToHost, h->stream);
            (void)hipMemcpyAsync(S, h->d_L, sizeof(double) * bs * bs, hipMemcpyDeviceToHost, h->stream);
            (void)hipMemcpyAsync(Linv, h->d_Linv, sizeof(double) * bs * bs, hipMemcpyDeviceToHost, h->stream);
            if (hipStreamSynchronize(h->stream) != hipSuccess) s = GMRF_ERR_HIP;
            if (info) *info = hi;
            if (dst) (void)hipMemcpy(g_tile_stamps + 24, dst, 6 * sizeof(unsigned long long), hipMemcpyDeviceToHost);
            if (dst) (void)hipMemcpy(g_persist_stamps, dst, 128 * sizeof(unsigned long long), hipMemcpyDeviceToHost);
        }
    }
    if (dst) (void)hipFree(dst);
    gmrf_bt_destroy(h);
    return s;
}

// potrf_block once, on whichever route a handle of this shape takes: N = 1, `batch` problems, set_eager(switches), keep_l, a
// coupling window that starts at cmin (what planned_xsplit looks at).  S, L, Linv: host, [batch][bs][bs]; all three are uploaded
// whole (so the caller decides what the kernels find where they do not write) and L, Linv are read back whole.  info: the info
// word as the kernels left it (0, or 1 + problem).  route[4] = {potrf_route, stats.persist_route, xsplit, persistent waits that
// gave up}.  Launches what the factorisation launches and nothing else; no stamps, no forward solve.
gmrf_status gmrf_test_potrf_route(int32_t device, int64_t bs, int32_t batch, int32_t switches, int64_t cmin, int32_t keep_l,
                                  double* S, double* L, double* Linv, int32_t* info, int32_t* route) {
    if (!S || !L || !Linv || !info || !route) return bad_shape("null pointer");
    if (bs < 64 || bs % 64 || next_pow2(bs / 64) != bs / 64) return bad_shape("bs must be 64 * 2^p");
    if (batch < 1) return bad_shape("batch must be >= 1");
    if (cmin < 0 || cmin >= bs || cmin % 64) return bad_shape("cmin must be a multiple of 64 in [0, bs)");
    gmrf_handle* h = nullptr;
    GCHK(gmrf_bt_create(device, nullptr, &h));
    h->N = 1; h->n = bs; h->bs = bs; h->bsp = bs; h->n_pad = bs; h->B = batch;
    h->keep_l = keep_l != 0;
    gmrf_status s = gmrf_bt_set_eager(h, switches);
    if (s == GMRF_OK) s = set_layout(h, cmin, bs, std::vector<int64_t>((size_t)(bs / 64), cmin));
    if (s == GMRF_OK) s = alloc_factor(h);
    if (s == GMRF_OK) {
        const size_t bytes = sizeof(double) * (size_t)bs * (size_t)bs * (size_t)batch;
        h->xsplit = planned_xsplit(h);
        persist_plan(h);
        hipError_t e = hipMemcpyAsync(h->d_S, S, bytes, hipMemcpyHostToDevice, h->stream);
        if (e == hipSuccess) e = hipMemcpyAsync(h->d_L, L, bytes, hipMemcpyHostToDevice, h->stream);
        if (e == hipSuccess) e = hipMemcpyAsync(h->d_Linv, Linv, bytes, hipMemcpyHostToDevice, h->stream);
        if (e != hipSuccess) s = GMRF_ERR_HIP;
        if (s == GMRF_OK) s = potrf_block(h, h->d_S, h->d_L, h->d_Linv, h->d_T, 1);
        if (s == GMRF_OK) {
            int hi[2] = {0, 0};
            (void)hipMemcpyAsync(hi, h->d_info, 2 * sizeof(int), hipMemcpyDeviceToHost, h->stream);
            (void)hipMemcpyAsync(L, h->d_L, bytes, hipMemcpyDeviceToHost, h->stream);
            (void)hipMemcpyAsync(Linv, h->d_Linv, bytes, hipMemcpyDeviceToHost, h->stream);
            if (hipStreamSynchronize(h->stream) != hipSuccess) s = GMRF_ERR_HIP;
            if (s == GMRF_OK && hi[1] != 0) persist_give_up(h);          // (counted, not repeated: the caller sees it in route[3])
            *info = hi[0];
            route[0] = potrf_route(h); route[1] = h->stats.persist_route; route[2] = h->xsplit; route[3] = h->persist_aborts;
        }
    }
    gmrf_bt_destroy(h);
    return s;
}

gmrf_status gmrf_test_mfma_f64_rate(int32_t device, double* tflops) {
    HIPCHK(hipSetDevice(device));
    double* d;
    HIPCHK(hipMalloc(&d, 64));
    hipEvent_t a, b;
    HIPCHK(hipEventCreate(&a)); HIPCHK(hipEventCreate(&b));
    const int iters = 20000, blocks = 256 * 2;
    hipLaunchKernelGGL(mfma_f64_rate_kernel, dim3(blocks), dim3(256), 0, nullptr, d, 100);
    HIPCHK(hipDeviceSynchronize());
    HIPCHK(hipEventRecord(a, nullptr));
    hipLaunchKernelGGL(mfma_f64_rate_kernel, dim3(blocks), dim3(256), 0, nullptr, d, iters);
    HIPCHK(hipEventRecord(b, nullptr));
    HIPCHK(hipEventSynchronize(b));
    float ms = 0.f;
    HIPCHK(hipEventElapsedTime(&ms, a, b));
    const double flops = (double)blocks * 4 /*waves*/ * iters * 4.0 * 2048.0;
    *tflops = flops / (ms * 1e-3) / 1e12;
    hipFree(d); hipEventDestroy(a); hipEventDestroy(b);
    return GMRF_OK;
}


// Micro-benchmark battery; fills out[0..n) (see tools/microbench.py for the meaning).
// The host-only part of the symbolic phase of gmrf_bt_factor_csc (block split + band check, zero structure of the coupling
// blocks, row pointers, tile plan of the sparse C = B X^T) without a device: what the sanitizer build of the host side
// (make libgmrf_hip_asan.so, tests/test_host_logic.py) drives.  out[8] = {cmin, rmax, entries, most entries in a row of a
// lower block, sparse route?, tile plan?, LDS entry capacity of the plan, checksum of the plan's arrays}.
gmrf_status gmrf_test_symbolic_csc(int64_t n, int64_t n_blocks, const int64_t* colptr, const int64_t* rowval, int32_t index_base,
                                   int64_t* out8) {
    if (!colptr || !rowval || !out8) return bad_shape("null pointer");
    if (n <= 0 || n_blocks <= 0 || n % n_blocks != 0) return bad_shape("n must be a positive multiple of N_blocks");
    const int64_t bs = n / n_blocks, bsp = 64 * next_pow2((bs + 63) / 64);
    std::vector<std::vector<HostEntry>> dg, lo;
    GCHK(split_csc(n, n_blocks, bs, colptr, rowval, index_base, dg, lo));
    SymbolicPlan sp;
    build_symbolic(n_blocks, bsp, dg, lo, false, sp);
    uint64_t sum = 1469598103934665603ull;
    auto mix = [&sum](uint64_t v) { sum = (sum ^ v) * 1099511628211ull; };
    for (uint64_t k : sp.keys) mix(k);
    for (int64_t v : sp.src) mix((uint64_t)v);
    for (int v : sp.rowptr) mix((uint64_t)(uint32_t)v);
    for (int v : sp.uptr) mix((uint64_t)(uint32_t)v);
    for (int v : sp.gtiles) mix((uint64_t)(uint32_t)v);
    for (int v : sp.ucols) mix((uint64_t)(uint32_t)v);
    for (uint16_t v : sp.lidx) mix(v);
    for (int64_t v : sp.first) mix((uint64_t)v);
    out8[0] = sp.cmin; out8[1] = sp.rmax; out8[2] = (int64_t)sp.keys.size(); out8[3] = sp.max_row; out8[4] = sp.sparse_b;
    out8[5] = sp.bxt_ok; out8[6] = sp.ecap; out8[7] = (int64_t)(sum >> 1);
    return GMRF_OK;
}

// The envelope bounds of a pattern without a device (build_envelope / derive_envelope): lo, hi as gmrf_test_envelope returns them
// ([n_blocks][bsp / 64]), and units[n_blocks][bsp / 256][3]: the 64-wide K units of a panel's product without / with a tail row riding
// and of its rank-256 update, as the factorisation books them.  cap: values lo and hi can hold; *n_vals = n_blocks * bsp / 64, or 0
// where the blocks are no multiple of 256.
gmrf_status gmrf_test_envelope_csc(int64_t n, int64_t n_blocks, const int64_t* colptr, const int64_t* rowval, int32_t index_base,
                                   int32_t* lo, int32_t* hi, double* units, int64_t cap, int64_t* n_vals) {
    if (!colptr || !rowval || !n_vals) return bad_shape("null pointer");
    if (n <= 0 || n_blocks <= 0 || n % n_blocks != 0) return bad_shape("n must be a positive multiple of N_blocks");
    const int64_t bs = n / n_blocks, bsp = 64 * next_pow2((bs + 63) / 64);
    std::vector<std::vector<HostEntry>> dg, lw;
    GCHK(split_csc(n, n_blocks, bs, colptr, rowval, index_base, dg, lw));
    SymbolicPlan sp;
    build_symbolic(n_blocks, bsp, dg, lw, false, sp);
    const int nt = (int)(bsp / 64), np = nt / 4;
    *n_vals = bsp % 256 == 0 ? n_blocks * nt : 0;
    if (*n_vals == 0 || !lo || !hi || cap < *n_vals) return GMRF_OK;
    for (int64_t k = 0; k < *n_vals; ++k) { lo[k] = sp.env_lo[(size_t)k]; hi[k] = sp.env_hi[(size_t)k]; }
    if (units) {
        EnvHost eh;
        derive_envelope(n_blocks, bsp, sp, eh);
        for (int64_t i = 0; i < n_blocks; ++i)
            for (int p = 0; p < np; ++p) {
                const int* host = eh.host.data() + (size_t)((i * np + p) * 4) * nt;
                const int m3 = nt - 4 * p - 4;
                double* u = units + (i * np + p) * 3;
                u[0] = env_units_pp(host, nt, m3, 0); u[1] = env_units_pp(host, nt, m3, 2); u[2] = env_units_upd(host, m3);
            }
    }
    return GMRF_OK;
}

// The tile plan and the routes of Y = S X for a CSR pattern, without a device (spmm_plan_host, spmm_rows_route, spmm_cols_route).
// geom[8] = {k, ldx, ldy, X base 16-byte aligned?, Y base 16-byte aligned?, x_stride, y_stride, padded plan withheld?} (the leading
// dimensions are the node-major call's).  out[12] = {plan state, R, ucap, ecap, ecap_pad, umax, tiles, distinct columns listed,
// node-major kind (0 plain, 1 tiled, 2 padded), NG, column-major route at this k (0: csr_spmv_tiles, else G), tiles_ok}.
// tile_uptr [tiles + 1], ucols, lidx [nnz]: filled where all three are given and cap_uptr / cap_ucols suffice.
gmrf_status gmrf_test_spmm_plan(int64_t n_rows, int64_t n_cols, const int64_t* rowptr, const int64_t* colidx, int32_t index_base,
                                const int64_t* geom, int64_t* out, int64_t* tile_uptr, int32_t* ucols, uint16_t* lidx,
                                int64_t cap_uptr, int64_t cap_ucols) {
    if (!rowptr || !colidx || !geom || !out) return bad_shape("null pointer");
    if (n_rows <= 0 || n_cols <= 0 || geom[0] <= 0 || geom[0] > (1 << 20)) return bad_shape("bad CSR arguments");
    std::vector<int64_t> rp((size_t)n_rows + 1);
    for (int64_t i = 0; i <= n_rows; ++i) {
        rp[i] = rowptr[i] - index_base;
        if (i == 0 ? rp[0] != 0 : rp[i] < rp[i - 1]) return bad_shape("bad CSR row pointers");
    }
    const int64_t nnz = rp[n_rows];
    std::vector<int32_t> ci((size_t)std::max<int64_t>(nnz, 1));
    for (int64_t p = 0; p < nnz; ++p) {
        const int64_t c = colidx[p] - index_base;
        if (c < 0 || c >= n_cols) return bad_shape("column index out of range");
        ci[p] = (int32_t)c;
    }
    SpmmPlan pl;
    spmm_plan_host(n_rows, rp.data(), ci.data(), pl);
    const bool tiles_ok = spmv_tiles_ok(n_rows, rp.data());
    const SpmmRowsRoute rt = spmm_rows_route(pl.state, pl.ucap, pl.ecap_pad, n_cols, (int)geom[0], geom[1], geom[2], geom[3] != 0,
                                             geom[4] != 0, geom[5], geom[6], geom[7] != 0);
    out[0] = pl.state; out[1] = pl.R; out[2] = pl.ucap; out[3] = pl.ecap; out[4] = pl.ecap_pad; out[5] = pl.umax;
    out[6] = pl.state == 1 ? (int64_t)pl.tile_uptr.size() - 1 : 0; out[7] = (int64_t)pl.ucols.size();
    out[8] = rt.kind; out[9] = rt.ng; out[10] = spmm_cols_route(nnz, n_rows, (int)geom[0], tiles_ok); out[11] = tiles_ok;
    if (pl.state == 1 && tile_uptr && ucols && lidx && cap_uptr >= (int64_t)pl.tile_uptr.size() && cap_ucols >= (int64_t)pl.ucols.size()) {
        std::copy(pl.tile_uptr.begin(), pl.tile_uptr.end(), tile_uptr);
        std::copy(pl.ucols.begin(), pl.ucols.end(), ucols);
        std::copy(pl.lidx.begin(), pl.lidx.begin() + nnz, lidx);
    }
    return GMRF_OK;
}

// The routes of a live matrix for one call geometry: geom[8] as gmrf_test_spmm_plan with the two alignment flags taken from the
// addresses X and Y (only their values are read; device or host).  out[12] = {plan state, R, ucap, ecap, ecap_pad, umax, node-major
// kind, NG, column-major route, and the routes of the LAST products launched on S: node-major kind, NG, column-major route (-1: none)}.
gmrf_status gmrf_test_spmm_route(const gmrf_csr* S, const int64_t* geom, const void* X, const void* Y, int64_t* out) {
    if (!S || !geom || !out) return bad_shape("null pointer");
    if (geom[0] <= 0 || geom[0] > (1 << 20)) return bad_shape("bad k");
    HIPCHK(hipSetDevice(S->device));
    gmrf_csr* m = const_cast<gmrf_csr*>(S);
    GCHK(spmm_plan(m));
    const SpmmRowsRoute rt = spmm_rows_route(m->plan_state, m->plan_ucap, m->plan_ecap_pad, S->n_cols, (int)geom[0], geom[1], geom[2],
                                             ptr_aligned16(X), ptr_aligned16(Y), geom[5], geom[6], geom[7] != 0);
    const bool planned = m->plan_state == 1;
    out[0] = m->plan_state; out[1] = planned ? m->plan_rows : 0; out[2] = planned ? m->plan_ucap : 0; out[3] = planned ? m->plan_ecap : 0;
    out[4] = planned ? m->plan_ecap_pad : 0; out[5] = planned ? m->plan_umax : 0;
    out[6] = rt.kind; out[7] = rt.ng; out[8] = spmm_cols_route(S->nnz, S->n_rows, (int)geom[0], S->tiles_ok);
    out[9] = S->last_rows_kind; out[10] = S->last_rows_ng; out[11] = S->last_cols_g;
    return GMRF_OK;
}

// spmm_rows_device_batch with explicit device pointers: B problems on S's pattern, values vals[B][nnz] (fp64), node-major operands
// X + p x_stride (row stride ldx) and Y + p y_stride (ldy), k right-hand sides; no_pad withholds the padded plan for this call.
// B = 1 is the product with another problem's values.  Synchronises S's stream.
gmrf_status gmrf_test_spmm_rows_batch(const gmrf_csr* S, int64_t B, const double* vals, const double* X, int64_t ldx, int64_t x_stride,
                                      double* Y, int64_t ldy, int64_t y_stride, int64_t k, int32_t no_pad) {
    if (!S || !vals || !X || !Y) return bad_shape("null pointer");
    if (B <= 0 || B > 65535 || k <= 0 || k > (1 << 20) || ldx < k || ldy < k) return bad_shape("bad B / k / ld");
    if (B > 1 && (x_stride < (S->n_cols - 1) * ldx + k || y_stride < (S->n_rows - 1) * ldy + k)) return bad_shape("problems overlap");
    HIPCHK(hipSetDevice(S->device));
    if (!is_device_ptr(vals) || !is_device_ptr(X) || !is_device_ptr(Y)) return bad_shape("gmrf_test_spmm_rows_batch takes device pointers");
    GCHK(spmm_rows_device_batch(S, S->stream, B, vals, X, ldx, x_stride, Y, ldy, y_stride, (int)k, no_pad != 0));
    HIPCHK(hipStreamSynchronize(S->stream));
    return GMRF_OK;
}

// ---- the block sweep products (sweep.hpp) as a route value and as one product on explicit operands ---------------------------
// desc[17] = {trans, tri, kp, rows, kdim, nprob, narrow, kst set?, mend set?, ld, ldx, ldb, ldo, pMat, pXin, pBin, pOut}
struct SweepDesc {
    bool trans, tri, has_kst, has_mend;
    int kp, rows, kdim, nprob, narrow;
    int64_t ld, ldx, ldb, ldo, pMat, pXin, pBin, pOut;
};
static gmrf_status sweep_desc_read(const int64_t* desc, SweepDesc* d) {
    for (int i = 2; i < 7; ++i)
        if (desc[i] < -(1 << 24) || desc[i] > (1 << 24)) return bad_shape("sweep test: a size is beyond 2^24");
    for (int i = 9; i < 17; ++i)
        if (desc[i] < 0 || desc[i] > ((int64_t)1 << 40)) return bad_shape("sweep test: a leading dimension or stride is negative");
    d->trans = desc[0] != 0; d->tri = desc[1] != 0; d->kp = (int)desc[2]; d->rows = (int)desc[3]; d->kdim = (int)desc[4];
    d->nprob = (int)desc[5]; d->narrow = (int)desc[6]; d->has_kst = desc[7] != 0; d->has_mend = desc[8] != 0;
    d->ld = desc[9]; d->ldx = desc[10]; d->ldb = desc[11]; d->ldo = desc[12];
    d->pMat = desc[13]; d->pXin = desc[14]; d->pBin = desc[15]; d->pOut = desc[16];
    return GMRF_OK;
}

// Host only, no device: the kernel launch_sweep takes for the description and its grid.  out[4] = {id (0: refused), gx, gy, gz};
// the reason of a refusal is left in gmrf_last_error.
gmrf_status gmrf_test_sweep_route(const int64_t* desc, int64_t* out) {
    if (!desc || !out) return bad_shape("null pointer");
    SweepDesc d;
    GCHK(sweep_desc_read(desc, &d));
    const SweepRoute r = sweep_route(d.trans, d.tri, d.kp, d.rows, d.kdim, d.nprob, d.narrow, d.has_kst, d.has_mend);
    if (r.id == SWEEP_REFUSED) g_last_error = r.why;
    out[0] = r.id; out[1] = r.gx; out[2] = r.gy; out[3] = r.gz;
    return GMRF_OK;
}

// One sweep product on explicit operands.  Mat (nMat doubles) and the panel P (nP doubles) are host arrays, uploaded whole; P is
// read back whole, so the caller sees what was written and what was left.  Xin = P + x_off, Bin = P + b_off (b_off < 0: no addend,
// sub = 0; b_off == o_off: in place), Out = P + o_off.  force = 0: launch_sweep's own choice; force = id: that instantiation, if the
// shape meets the kernel's own preconditions (sweep_kernel_route).  *route_out = the id that ran.  Everything a kernel could read
// or write out of bounds with -- or read misaligned, or race on -- is refused before anything is uploaded:
//   * the route refuses, or kst / mend are given to a product that has no staircase, or disagree with desc[7], desc[8];
//   * kst / mend shorter than one entry per 64 rows, an entry odd or outside [0, kdim], or one that leaves a sweep_mm range that
//     is not a multiple of 8;
//   * ld (pMat) odd where the kernel loads 16-byte row pieces (all but the transposed sweep_mm, which loads single elements of the
//     block); x_off, ldx, pXin odd where it loads 16-byte pieces of the input (sweep_mm and the non-transposed gemv kernels);
//   * ld below the row length, or the furthest element of the block beyond nMat: (rows - 1) ld + kdim, transposed (kdim - 1) ld +
//     rows, per problem -- the triangular kernels' pieces right of the diagonal end at the next even column (four-row gemv) or at
//     the end of the diagonal 16-row / CW-column block, all of them inside the first `rows` columns of their rows;
//   * an input, addend or output cell beyond nP; an output cell that is also an input cell, another output's cell, or an addend
//     cell other than its own (cell by cell over the whole batch).
gmrf_status gmrf_test_sweep_product(int32_t device, int32_t force, const int64_t* desc, const double* Mat, int64_t nMat, double* P, int64_t nP,
                                    int64_t x_off, int64_t b_off, int64_t o_off, const int32_t* kst, int64_t n_kst,
                                    const int32_t* mend, int64_t n_mend, int32_t* route_out) {
    if (!desc || !Mat || !P || !route_out) return bad_shape("sweep test: null pointer");
    *route_out = 0;
    SweepDesc d;
    GCHK(sweep_desc_read(desc, &d));
    if (nMat <= 0 || nP <= 0 || nMat > ((int64_t)1 << 28) || nP > ((int64_t)1 << 28)) return bad_shape("sweep test: buffer sizes");
    if ((kst != nullptr) != d.has_kst || (mend != nullptr) != d.has_mend) return bad_shape("sweep test: kst / mend disagree with the description");
    if (kst && (d.trans || d.tri)) return bad_shape("sweep test: kst belongs to the non-transposed, non-triangular product");
    if (mend && (!d.trans || d.tri)) return bad_shape("sweep test: mend belongs to the transposed, non-triangular product");
    if (force < 0 || force > SWEEP_KERNELS) return bad_shape("sweep test: no such kernel");
    const SweepRoute r = force ? sweep_kernel_route(force, d.trans, d.tri, d.kp, d.rows, d.kdim, d.nprob, d.has_kst, d.has_mend)
                               : sweep_route(d.trans, d.tri, d.kp, d.rows, d.kdim, d.nprob, d.narrow, d.has_kst, d.has_mend);
    if (r.id == SWEEP_REFUSED) return bad_shape(r.why);
    const bool mm = r.id <= SWEEP_MM_T_TRI;
    const int ntile = (d.rows + 63) / 64;
    for (const int32_t* a : {kst, mend}) {
        if (!a) continue;
        if ((a == kst ? n_kst : n_mend) < ntile) return bad_shape("sweep test: kst / mend shorter than one entry per 64 rows");
        for (int t = 0; t < ntile; ++t) {
            if (a[t] < 0 || a[t] > d.kdim || a[t] % 2) return bad_shape("sweep test: a kst / mend entry is odd or out of range");
            if (mm && (a == kst ? d.kdim - a[t] : a[t]) % 8) return bad_shape("sweep test: a kst / mend entry leaves a K range that is not a multiple of 8");
        }
    }
    const bool mat16 = r.id != SWEEP_MM_T && r.id != SWEEP_MM_T_TRI, x16 = r.id <= SWEEP_GEMV_N4_TRI;
    if (mat16 && (d.ld % 2 || d.pMat % 2)) return bad_shape("sweep test: odd ld or pMat under 16-byte loads of the block");
    if (x16 && (x_off % 2 || d.pXin % 2 || (mm && d.ldx % 2))) return bad_shape("sweep test: odd x_off, ldx or pXin under 16-byte loads of the input");
    if (d.ld < (d.trans ? d.rows : d.kdim)) return bad_shape("sweep test: ld below the row length");
    const bool sub = b_off >= 0;
    if (mm && (d.ldx < d.kdim || d.ldo < d.rows || (sub && d.ldb < d.rows))) return bad_shape("sweep test: a panel's leading dimension is below its extent");
    const int64_t needMat = (int64_t)(d.nprob - 1) * d.pMat + (d.trans ? (int64_t)(d.kdim - 1) * d.ld + d.rows : (int64_t)(d.rows - 1) * d.ld + d.kdim);
    if (needMat > nMat) return bad_shape("sweep test: the block does not fit its buffer");
    if (x_off < 0 || o_off < 0) return bad_shape("sweep test: negative offset");
    const bool in_place = sub && b_off == o_off;
    if (in_place && (d.pBin != d.pOut || (mm && d.ldb != d.ldo))) return bad_shape("sweep test: in place needs the addend's strides to be the output's");
    {
        // cell by cell: 1 = input, 2 = output, 4 = addend
        std::vector<uint8_t> mark((size_t)nP, 0);
        auto runs = [&](int64_t off, int64_t ldr, int64_t pstride, int len, uint8_t bit, uint8_t clash) -> const char* {
            for (int p = 0; p < d.nprob; ++p)
                for (int q = 0; q < d.kp; ++q) {
                    const int64_t a = off + (int64_t)p * pstride + (int64_t)q * ldr;
                    if (a < 0 || a + len > nP) return "sweep test: a panel operand does not fit its buffer";
                    for (int64_t c = a; c < a + len; ++c) {
                        if (mark[(size_t)c] & clash) return "sweep test: operands overlap";
                        mark[(size_t)c] |= bit;
                    }
                }
            return nullptr;
        };
        const char* bad = runs(x_off, d.ldx, d.pXin, d.kdim, 1, 0);
        if (!bad) bad = runs(o_off, d.ldo, d.pOut, d.rows, 2, 1 | 2);
        if (!bad && sub && !in_place) bad = runs(b_off, d.ldb, d.pBin, d.rows, 4, 2);
        if (bad) return bad_shape(bad);
    }

    HIPCHK(hipSetDevice(device));
    std::vector<void*> owned;
    auto drop = [&]() { for (void* p : owned) (void)hipFree(p); owned.clear(); };
    hipError_t e = hipSuccess;
    auto up = [&](const void* host, int64_t count, size_t elem) -> void* {
        if (!host || e != hipSuccess) return nullptr;
        void* dv = nullptr;
        e = hipMalloc(&dv, std::max<size_t>((size_t)count * elem, 16));
        if (e != hipSuccess) return nullptr;
        owned.push_back(dv);
        e = hipMemcpy(dv, host, (size_t)count * elem, hipMemcpyHostToDevice);
        return dv;
    };
    const double* dMat = (const double*)up(Mat, nMat, 8);
    double* dP = (double*)up(P, nP, 8);
    SweepArgs s;
    s.kst = (const int*)up(kst, ntile, 4);
    s.mend = (const int*)up(mend, ntile, 4);
    if (e != hipSuccess) { drop(); HIPCHK(e); }
    s.Mat = dMat; s.ld = d.ld; s.Xin = dP + x_off; s.ldx = d.ldx; s.Bin = sub ? dP + b_off : nullptr; s.ldb = sub ? d.ldb : 0;
    s.Out = dP + o_off; s.ldo = d.ldo; s.rows = d.rows; s.kdim = d.kdim; s.sub = sub ? 1 : 0;
    s.pMat = d.pMat; s.pXin = d.pXin; s.pBin = sub ? d.pBin : 0; s.pOut = d.pOut;
    s.narrow = d.narrow;
    e = force ? launch_sweep_kernel(nullptr, r, s) : launch_sweep(nullptr, d.trans, d.tri, d.kp, s, d.nprob);
    if (e == hipSuccess) e = hipDeviceSynchronize();
    if (e == hipSuccess) e = hipMemcpy(P, dP, sizeof(double) * (size_t)nP, hipMemcpyDeviceToHost);
    drop();
    HIPCHK(e);
    *route_out = r.id;
    return GMRF_OK;
}

static void coupling_route_write(const CouplingRoute& r, int64_t* out) {
    out[0] = r.kind; out[1] = r.km; out[2] = r.cw; out[3] = r.nch; out[4] = r.ncg; out[5] = r.ng; out[6] = r.grid; out[7] = r.fill;
    out[8] = r.zwgs; out[9] = r.skip_dead;
}

// Host only, no device: what the symbolic phase plans for the coupling products of a CSC pattern, array by array, and the route
// coupling_route takes on it.  group_tiles: build_symbolic's parameter (a handle passes B >= 8).  scal[12] = {cmin, rmax, most
// entries in a row of a lower block, sparse_b, bxt_ok, ecap, nrt, then the lengths of kst, rowptr, gtiles, ucols, lidx}.  The arrays
// (each may be NULL) are filled where cap[7] -- capacities of kst, rowptr, ng, gtiles, uptr, ucols, lidx in elements -- suffices:
// kst [bsp / 64] as set_layout leaves it, rowptr [N][bsp + 1], and of a usable plan ng [N], gtiles [N][nrt][3], uptr [N][nrt + 1],
// ucols, lidx [entries].  query (or NULL) = {B, CUs, block i, switches}: route[10] = {kind, KM, cw, nch, ncg, ng, grid, fill, zwgs,
// skip_dead} of block i of a handle of B problems on a device of that many CUs.
gmrf_status gmrf_test_coupling_plan(int64_t n, int64_t n_blocks, const int64_t* colptr, const int64_t* rowval, int32_t index_base,
                                    int32_t group_tiles, int64_t* scal, int32_t* kst, int32_t* rowptr, int32_t* ng, int32_t* gtiles,
                                    int32_t* uptr, int32_t* ucols, uint16_t* lidx, const int64_t* cap, const int64_t* query, int64_t* route) {
    if (!colptr || !rowval || !scal || !cap) return bad_shape("null pointer");
    if (n <= 0 || n_blocks <= 0 || n % n_blocks != 0) return bad_shape("n must be a positive multiple of N_blocks");
    if (query && !route) return bad_shape("null pointer");
    const int64_t bs = n / n_blocks, bsp = 64 * next_pow2((bs + 63) / 64);
    if (query && (query[0] < 1 || query[0] > (1 << 20) || query[1] < 0 || query[2] < 1 || query[2] >= n_blocks))
        return bad_shape("coupling plan: bad query");
    std::vector<std::vector<HostEntry>> dg, lo;
    GCHK(split_csc(n, n_blocks, bs, colptr, rowval, index_base, dg, lo));
    SymbolicPlan sp;
    build_symbolic(n_blocks, bsp, dg, lo, false, sp, group_tiles != 0);
    std::vector<int> k;
    layout_kst(bsp, sp.cmin, sp.rmax, sp.first, k);
    scal[0] = sp.cmin; scal[1] = sp.rmax; scal[2] = sp.max_row; scal[3] = sp.sparse_b; scal[4] = sp.bxt_ok; scal[5] = sp.ecap;
    scal[6] = sp.nrt; scal[7] = (int64_t)k.size(); scal[8] = (int64_t)sp.rowptr.size();
    scal[9] = sp.bxt_ok ? (int64_t)sp.gtiles.size() : 0; scal[10] = sp.bxt_ok ? (int64_t)sp.ucols.size() : 0;
    scal[11] = sp.bxt_ok ? (int64_t)sp.lidx.size() : 0;
    auto put = [](auto* dst, int64_t capn, const auto& v) {
        if (dst && capn >= (int64_t)v.size()) for (size_t q = 0; q < v.size(); ++q) dst[q] = v[q];
    };
    put(kst, cap[0], k);
    put(rowptr, cap[1], sp.rowptr);
    if (sp.bxt_ok) {
        put(ng, cap[2], sp.ng); put(gtiles, cap[3], sp.gtiles); put(uptr, cap[4], sp.uptr); put(ucols, cap[5], sp.ucols);
        put(lidx, cap[6], sp.lidx);
    }
    if (query) {
        CouplingShape s;
        s.bsp = (int)bsp; s.bs = (int)bs; s.cm = (int)sp.cmin; s.rm = (int)sp.rmax; s.nb = (int)query[0]; s.cus = (int)query[1];
        s.sparse_b = sp.sparse_b; s.plan_ok = sp.bxt_ok && sp.nrt == (int)(sp.rmax / 64); s.has_drow = sp.keys.size() < ((size_t)1 << 31);
        s.max_row = (int)sp.max_row; s.ng = s.plan_ok ? sp.ng[(size_t)query[2]] : 0; s.switches = (int32_t)query[3];
        coupling_route_write(coupling_route(s), route);
    }
    return GMRF_OK;
}

// The next analysis of this handle plans the tile groups of spmm_bxt_tiles with group_tiles = mode (0: every tile alone, 1: grouped)
// instead of by its batch (-1: by the batch again).
gmrf_status gmrf_test_coupling_group_tiles(gmrf_handle* h, int32_t mode) {
    if (!h || mode < -1 || mode > 1) return bad_shape("coupling test: bad arguments");
    h->group_tiles_force = mode;
    return GMRF_OK;
}

// One coupling step (launch_coupling, once, then a synchronisation) of block i on a handle that gmrf_bt_factor_begin_csc has
// prepared: pattern analysed, values resident, factor storage allocated.  force = 0: coupling_route's own choice; 1: spmm_bxt;
// 2: spmm_bxt_tiles on the handle's plan; 3: the dense GEMM.  over[4] (or NULL), 0 = own choice: cw in {16, 32, 64}; nch, one of the
// launcher's list; skip_dead 1 = off, 2 = on; Schur fill 1 = nobody, 2 = the zero role, 3 = the scatter role.  X[B][bsp bsp] is
// uploaded as Linv_{i-1} of every problem, C[nC] as the handle's whole d_C (every problem, every block), S[B][bsp bsp] as the
// Schur work block; C and S are read back whole.  route_out[10] as gmrf_test_coupling_plan.  Refused with GMRF_ERR_BAD_SHAPE,
// nothing uploaded or launched: a buffer of the wrong size, a route or override that the shape's own preconditions do not admit.
gmrf_status gmrf_test_coupling_product(gmrf_handle* h, int64_t i, int32_t force, const int32_t* over, const double* X, int64_t nX,
                                       double* C, int64_t nC, double* S, int64_t nS, int64_t* route_out) {
    if (!h || !X || !C || !S || !route_out) return bad_shape("coupling test: null pointer");
    GCHK(tw_refuse(h, "gmrf_test_coupling_product"));
    if (!h->analyzed || !h->d_C || !h->d_S || !h->d_Linv || !h->d_B || h->alloc_B != h->B || h->vals_B != h->B || h->alloc_rm != h->rmax ||
        h->alloc_wc != c_ld(h) || h->alloc_N != h->N || h->alloc_bsp != h->bsp)
        return bad_shape("coupling test: the handle has not been through gmrf_bt_factor_begin_csc");
    if (i < 1 || i >= h->N) return bad_shape("coupling test: block out of range");
    if (force < 0 || force > 3) return bad_shape("coupling test: no such route");
    const int64_t bsp = h->bsp, be = bsp * bsp * h->B;
    if (nX != be || nS != be || nC != stride_pC(h) * h->B) return bad_shape("coupling test: a buffer has the wrong size");
    const CouplingShape s = coupling_shape(h, i);
    CouplingRoute r;
    if (force == 0) r = coupling_route(s);
    else {
        if (force == 1 && !s.sparse_b) return bad_shape("coupling test: spmm_bxt holds rows of at most 32 entries");
        if (force == 2 && !s.plan_ok) return bad_shape("coupling test: the handle has no usable tile plan");
        r = coupling_route_of(s, force == 1 ? COUPLING_BXT : (force == 2 ? COUPLING_TILES : COUPLING_DENSE));
    }
    const int W = s.bsp - s.cm;
    if (over) {
        if (over[0]) {
            if (r.kind != COUPLING_BXT || (over[0] != 16 && over[0] != 32 && over[0] != 64) || W % over[0]) return bad_shape("coupling test: bad cw");
            r.cw = over[0];
        }
        if (over[1]) {
            if (r.kind != COUPLING_TILES || std::find(std::begin(kBxtNch), std::end(kBxtNch), over[1]) == std::end(kBxtNch) || over[1] > W / 16)
                return bad_shape("coupling test: bad nch");
            r.nch = over[1];
        }
        if (over[2]) {
            if (r.kind != COUPLING_TILES || over[2] < 0 || over[2] > 2) return bad_shape("coupling test: bad skip_dead");
            r.skip_dead = over[2] - 1;
        }
        if (over[3] == 1) { r.fill = FILL_NONE; r.zwgs = 0; }
        else if (over[3] == 2) {
            if (r.kind != COUPLING_TILES || s.rm >= s.bsp) return bad_shape("coupling test: the zero role needs the tile route and rows below rmax");
            r.fill = FILL_ZERO_ROLE; r.zwgs = coupling_zero_wgs(s);
        } else if (over[3] == 3) {
            if (r.kind != COUPLING_TILES || s.nb != 1 || s.bsp != s.bs || !s.has_drow)
                return bad_shape("coupling test: the scatter role needs the tile route, one problem and unpadded blocks");
            r.fill = FILL_SCATTER_ROLE; r.zwgs = 64;
        } else if (over[3] != 0) return bad_shape("coupling test: bad fill");
        coupling_grid(s, r);
    }
    HIPCHK(hipSetDevice(h->device));
    const int64_t bstride = bsp * bsp;
    HIPCHK(hipStreamSynchronize(h->stream));
    for (int64_t p = 0; p < h->B; ++p)
        HIPCHK(hipMemcpyAsync(h->d_Linv + p * stride_pX(h) + (i - 1) * bstride, X + p * bstride, sizeof(double) * (size_t)bstride, hipMemcpyHostToDevice, h->stream));
    HIPCHK(hipMemcpyAsync(h->d_C, C, sizeof(double) * (size_t)nC, hipMemcpyHostToDevice, h->stream));
    HIPCHK(hipMemcpyAsync(h->d_S, S, sizeof(double) * (size_t)nS, hipMemcpyHostToDevice, h->stream));
    HIPCHK(hipStreamSynchronize(h->stream));
    h->factored = false; h->l_valid = false;
    GCHK(launch_coupling(h, i, r));
    HIPCHK(hipStreamSynchronize(h->stream));
    HIPCHK(hipMemcpy(C, h->d_C, sizeof(double) * (size_t)nC, hipMemcpyDeviceToHost));
    HIPCHK(hipMemcpy(S, h->d_S, sizeof(double) * (size_t)nS, hipMemcpyDeviceToHost));
    coupling_route_write(r, route_out);
    return GMRF_OK;
}

gmrf_status gmrf_test_microbench(int32_t device, double* out, int32_t n) {
    if (!out || n < 16) return bad_shape("need 16 outputs");
    HIPCHK(hipSetDevice(device));
    unsigned long long* d_t; double* d_s; int* d_i;
    HIPCHK(hipMalloc(&d_t, 64)); HIPCHK(hipMalloc(&d_s, 64)); HIPCHK(hipMalloc(&d_i, 64));
    hipEvent_t a, b;
    HIPCHK(hipEventCreate(&a)); HIPCHK(hipEventCreate(&b));
    unsigned long long ht[2];
    float ms = 0.f;
    auto timed = [&](auto launch, double flops, int idx) -> gmrf_status {
        launch(); HIPCHK(hipDeviceSynchronize());              // warm
        HIPCHK(hipEventRecord(a, nullptr)); launch(); HIPCHK(hipEventRecord(b, nullptr));
        HIPCHK(hipEventSynchronize(b)); HIPCHK(hipEventElapsedTime(&ms, a, b));
        HIPCHK(hipMemcpy(ht, d_t, 16, hipMemcpyDeviceToHost));
        out[idx] = flops / (ms * 1e-3) / 1e12;                 // TFLOP/s
        out[idx + 1] = (double)ht[0] / (double)ht[1] * 0.1;    // shader clock GHz inside the loop
        return GMRF_OK;
    };
    const int it = 20000;
    // 0,1: MFMA f64, 1 wave/SIMD (256 blocks), 4 accumulators
    GCHK(timed([&] { hipLaunchKernelGGL((mb_mfma_f64<4>), dim3(256), dim3(256), 0, nullptr, d_t, d_s, it); },
               256.0 * 4 * it * 4 * 2048.0, 0));
    // 2,3: MFMA f64, 2 waves/SIMD
    GCHK(timed([&] { hipLaunchKernelGGL((mb_mfma_f64<4>), dim3(512), dim3(256), 0, nullptr, d_t, d_s, it); },
               512.0 * 4 * it * 4 * 2048.0, 2));
    // 4,5: MFMA f64, 1 wave/SIMD, single dependent accumulator
    GCHK(timed([&] { hipLaunchKernelGGL((mb_mfma_f64<1>), dim3(256), dim3(256), 0, nullptr, d_t, d_s, it); },
               256.0 * 4 * it * 1 * 2048.0, 4));
    // 6,7: VALU f64 FMA, 2 waves/SIMD, 8 chains
    GCHK(timed([&] { hipLaunchKernelGGL(mb_valu_f64, dim3(512), dim3(256), 0, nullptr, d_t, d_s, it * 4); },
               512.0 * 256 * (it * 4.0) * 8 * 2.0, 6));
    // 8,9: one workgroup only (light load): MFMA loop -> cycles per MFMA and clock
    GCHK(timed([&] { hipLaunchKernelGGL((mb_mfma_f64<4>), dim3(1), dim3(64), 0, nullptr, d_t, d_s, it); },
               1.0 * it * 4 * 2048.0, 8));
    out[10] = (double)ht[0] / (it * 4.0);                       // shader cycles per MFMA, one wave
    // 11: empty-kernel launch cadence (us per launch, back to back on one stream)
    hipLaunchKernelGGL(mb_null, dim3(1), dim3(64), 0, nullptr, d_i);
    HIPCHK(hipDeviceSynchronize());
    HIPCHK(hipEventRecord(a, nullptr));
    for (int i = 0; i < 2000; ++i) hipLaunchKernelGGL(mb_null, dim3(1), dim3(64), 0, nullptr, d_i);
    HIPCHK(hipEventRecord(b, nullptr));
    HIPCHK(hipEventSynchronize(b)); HIPCHK(hipEventElapsedTime(&ms, a, b));
    out[11] = ms * 1e3 / 2000.0;
    // 12: same through a captured graph of 2000 nodes
    {
        hipStream_t st; HIPCHK(hipStreamCreateWithFlags(&st, hipStreamNonBlocking));
        hipGraph_t g; hipGraphExec_t ge;
        HIPCHK(hipStreamBeginCapture(st, hipStreamCaptureModeThreadLocal));
        for (int i = 0; i < 2000; ++i) hipLaunchKernelGGL(mb_null, dim3(1), dim3(64), 0, st, d_i);
        HIPCHK(hipStreamEndCapture(st, &g));
        HIPCHK(hipGraphInstantiate(&ge, g, nullptr, nullptr, 0));
        HIPCHK(hipGraphLaunch(ge, st)); HIPCHK(hipStreamSynchronize(st));
        HIPCHK(hipEventRecord(a, st)); HIPCHK(hipGraphLaunch(ge, st)); HIPCHK(hipEventRecord(b, st));
        HIPCHK(hipEventSynchronize(b)); HIPCHK(hipEventElapsedTime(&ms, a, b));
        out[12] = ms * 1e3 / 2000.0;
        (void)hipGraphExecDestroy(ge); (void)hipGraphDestroy(g); (void)hipStreamDestroy(st);
    }
    // 13,14: light kernel right after 200 ms of idling (clock ramp check)
    {
        struct timespec ts = {0, 200000000};
        nanosleep(&ts, nullptr);
        HIPCHK(hipEventRecord(a, nullptr));
        hipLaunchKernelGGL((mb_mfma_f64<4>), dim3(1), dim3(64), 0, nullptr, d_t, d_s, 2000);
        HIPCHK(hipEventRecord(b, nullptr));
        HIPCHK(hipEventSynchronize(b)); HIPCHK(hipEventElapsedTime(&ms, a, b));
        HIPCHK(hipMemcpy(ht, d_t, 16, hipMemcpyDeviceToHost));
        out[13] = (double)ht[0] / (double)ht[1] * 0.1;
        out[14] = ms * 1e3;
    }
    out[15] = 0;
    hipFree(d_t); hipFree(d_s); hipFree(d_i); hipEventDestroy(a); hipEventDestroy(b);
    return GMRF_OK;
}

gmrf_status gmrf_test_hbm_rate(int32_t device, int64_t bytes, double* gbps) {
    HIPCHK(hipSetDevice(device));
    double2* src;
    double* d;
    HIPCHK(hipMalloc(&src, bytes));
    HIPCHK(hipMalloc(&d, 64));
    HIPCHK(hipMemset(src, 0, bytes));
    hipEvent_t a, b;
    HIPCHK(hipEventCreate(&a)); HIPCHK(hipEventCreate(&b));
    const int64_t n16 = bytes / 16;
    hipLaunchKernelGGL(hbm_read_kernel, dim3(2048), dim3(256), 0, nullptr, src, n16, d);
    HIPCHK(hipDeviceSynchronize());
    HIPCHK(hipEventRecord(a, nullptr));
    for (int r = 0; r < 5; ++r) hipLaunchKernelGGL(hbm_read_kernel, dim3(2048), dim3(256), 0, nullptr, src, n16, d);
    HIPCHK(hipEventRecord(b, nullptr));
    HIPCHK(hipEventSynchronize(b));
    float ms = 0.f;
    HIPCHK(hipEventElapsedTime(&ms, a, b));
    *gbps = 5.0 * (double)bytes / (ms * 1e-3) / 1e9;
    hipFree(src); hipFree(d); hipEventDestroy(a); hipEventDestroy(b);
    return GMRF_OK;
}

}  // extern "C"
