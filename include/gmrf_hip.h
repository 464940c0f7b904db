/*
 * gmrf_hip.h -- C ABI of libgmrf_hip.so: MI355X (gfx950) block-tridiagonal Cholesky
 * factor / solve / sample path for GMRF posteriors.
 *
 * Drop-in boundary for ONE path of timweiland/DiffEqGMRFs.jl (all citations relative to
 * /root/reference):
 *     src/tridiagonal_cholesky.jl   tridiagonal_cholesky :65-82, forward_solve :43-52,
 *                                   backward_solve :24-33, ldiv!/ldiv :54-63,
 *                                   TridiagonalCholeskyFactor :5-9
 *     scripts/solve_burger.jl       extract_blocks :182-254 (block input form)
 *     SpMV call sites               scripts/solve_burger.jl:157-158,166,177 (Q * x)
 * The reference has no FFI of its own (pure Julia); these are the entry points a
 * `ccall` shim binds (julia/DiffEqGMRFsHIP.jl).
 *
 * Conventions
 *   - every function returns a gmrf_status (0 = OK, negative = error class);
 *   - no C++ types, no exceptions, no torch types cross this boundary;
 *   - data pointers (`double*`, `float*`) may be HOST or DEVICE pointers; the library asks
 *     the HIP runtime which (hipPointerGetAttributes) and stages host data itself;
 *   - matrices of right-hand sides are column-major n x k with leading dimension ld >= n
 *     (Julia Matrix{Float64} layout);
 *   - one handle = one GPU + one HIP stream; a handle is used by one host thread at a time;
 *   - calls are synchronous at return unless the name ends in _async.
 */
#ifndef GMRF_HIP_H
#define GMRF_HIP_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef int32_t gmrf_status;

enum {
    GMRF_OK = 0,
    GMRF_ERR_NOT_SPD = -1,     /* Julia PosDefException: *info = failing block (1-based)   */
    GMRF_ERR_BAD_SHAPE = -2,   /* n % N_blocks != 0, k <= 0, ld < n, null pointer ...       */
    GMRF_ERR_BAND = -3,        /* an entry lies outside the block tri-band of the partition */
    GMRF_ERR_HIP = -4,         /* a HIP runtime call failed (gmrf_last_error has the text)  */
    GMRF_ERR_NO_FACTOR = -5,   /* solve/sample before a successful factor                    */
    GMRF_ERR_NO_DEVICE = -6,   /* no gfx950 device visible                                   */
    GMRF_ERR_ALLOC = -7,
    GMRF_ERR_RCCL = -8         /* librccl missing or a collective failed (gmrf_last_error)  */
};

enum { GMRF_SOLVE_FULL = 0, GMRF_SOLVE_FORWARD = 1, GMRF_SOLVE_BACKWARD = 2 };
enum { GMRF_VAR_EXACT = 0, GMRF_VAR_RBMC = 1, GMRF_VAR_MC = 2 };
enum { GMRF_BLOCK_L = 0, GMRF_BLOCK_C = 1, GMRF_BLOCK_LINV = 2 };

typedef struct gmrf_handle gmrf_handle;   /* block-tridiagonal factor context  */
typedef struct gmrf_csr gmrf_csr;         /* device-resident CSR matrix (K6)   */
typedef struct gmrf_comm gmrf_comm;       /* RCCL communicator of this process */

/* One sparse block in compressed-sparse-row or -column form, as extract_blocks
 * (scripts/solve_burger.jl:240-247) returns them: `ptr` has dim+1 entries. */
typedef struct {
    int64_t nnz;
    const int64_t* ptr;
    const int64_t* idx;
    const double* val;
} gmrf_sparse_block;

/* Per-phase statistics of the last calls on a handle (gmrf_bt_stats). */
typedef struct {
    double factor_ms;          /* last gmrf_bt_factor_*                                     */
    double solve_ms;           /* last gmrf_bt_solve (device part)                          */
    double sample_ms;          /* last gmrf_bt_sample                                       */
    double factor_flops;       /* N bs^3/3 + (N-1) 2 bs^3 (LAPACK counts, logical bs)       */
    double sweep_bytes;        /* 8 [N bs(bs+1)/2 + (N-1) bs^2] + 16 n k of the last sweep (the reference's dense blocks) */
    double sweep_ms;           /* duration of the last single sweep                         */
    int64_t n, n_blocks, block_size, block_size_padded;
    int64_t factor_bytes;      /* device bytes held by L (if kept), C (stored window), Linv */
    /* per-kernel accounting, filled when profiling is on (gmrf_bt_set_profiling); one class per
     * kernel symbol so that a class compares with one row of a rocprofv3 kernel trace:
     *  0 / 11 / 12 gemm_f64_mfma<false,false> / <false,true> / <true,*> (64 x 64 tile GEMM: G2,
     *    rank-256 updates, GEMM sweeps / doubling assembly, GEMM sweeps / selected inversion)
     *  1 potrf_step<false> (tile Cholesky + inverse; fused with panel + update for one problem)
     *  2 sweep_mm (k >= 2 right-hand sides)     3 sweep_gemv_n / _t (k = 1)
     *  4 csr_spmm                                5 other (scatter, pack, Philox, ...)
     *  6 gemm_f64_big<false>                     7 gemm_f64_big<true>   (128 x 128 tile GEMM)
     *  8 potrf_panel                             9 potrf_update
     * 10 spmm_bxt (sparse C = B X^T)          13 gemm_f64_ll (32 x 32 tile GEMM of small launches)
     * 14 / 15 gemm_f64_dma<.., B [n][k]> / <.., B [k][n]> (LDS-DMA staged GEMM: the batches' products since round 3)
     *    (14 also books gemm_f64_dma_grouped, two products in one launch: ONE launch with both products' flops; round 13)
     * 16 potrf_diag128 (128 x 128 diagonal block of a batch: two tile Choleskys + the block's inverse)
     * 17 potrf_persist (one problem: the in-block Cholesky of a block / a 256-column panel in ONE persistent launch; small
     *    batches: the 256 x 256 diagonal block of a panel.  Round 4 booked these under class 1; class 17 was potrf_panel256, removed)
     * 18 gemm_f64_dma<.., A [k][m]> (the A^T B products of selected inversion: round 4)
     * 19 / 20 sweep_persist<k = 1> / <k >= 16> (one problem: a whole sweep in ONE persistent launch; round 5)
     * work = algorithmic flops (0-2, 6-9, 11-18, 20) or algorithmic bytes (3-5, 10, 19). */
#define GMRF_KERNEL_CLASSES 24
    double kernel_ms[GMRF_KERNEL_CLASSES];
    double kernel_work[GMRF_KERNEL_CLASSES];
    int64_t kernel_launches[GMRF_KERNEL_CLASSES];
    double sweep_bytes_streamed;  /* bytes the last sweep really read: Linv triangles + C inside the staircase + 16 n k */
    /* persistent launches (potrf_persist: one launch per block / per 256-column panel / per panel diagonal block; round 4),
     * made observable in round 5 (failure detection): */
    int32_t persist_route;        /* form the LAST factorisation launched: 0 none (launch per step / potrf_diag128 + GEMM), 1 one launch per
                                   * block (one problem, blocks of up to 16 tiles), 2 one per 256-column panel (one problem, larger
                                   * blocks), 3 one per 256 x 256 diagonal block of a panel (small batches) */
    int32_t persist_aborts;       /* times a bounded wait inside a persistent launch of this handle gave up: the range was repeated
                                   * with the launch-per-step form, which the handle keeps until it is destroyed */
    int32_t persist_cus;          /* CUs this handle holds of its device's budget for persistent launches (every workgroup of such a
                                   * launch must be resident; the claims of all handles of a device never exceed its CU count) */
    int32_t persist_refused;      /* 1: the budget refused this handle's claim (other handles hold the CUs): no persistent launches */
    int32_t sweep_persist;        /* 1: the last call that runs sweeps (gmrf_bt_solve, gmrf_bt_sample, gmrf_bt_posterior, the sampled
                                   * gmrf_bt_marginal_var, gmrf_bt_var_accumulate, gmrf_bt_marginal_var_batch) ran them as ONE persistent
                                   * launch each (one problem, blocks of 512 .. 1024, the handle holds the whole chip); a call whose inputs
                                   * overlap its outputs keeps a launch per product (0); a launch that gives up counts in persist_aborts
                                   * and the call is repeated with a launch per product */
    int32_t sweep_persist_launches;   /* such launches since the handle was created */
} gmrf_stats;

/* ------------------------------------------------------------------ life cycle */

/* device >= 0: HIP device ordinal.  stream: a hipStream_t to run on (e.g. the caller's
 * PyTorch stream) or NULL to let the handle create its own. */
gmrf_status gmrf_bt_create(int32_t device, void* stream, gmrf_handle** out);
gmrf_status gmrf_bt_destroy(gmrf_handle* h);
const char* gmrf_last_error(void);
int32_t gmrf_version(void);

/* ------------------------------------------------------------------ factor
 * tridiagonal_cholesky(A::SparseMatrixCSC, N_blocks)  (src/tridiagonal_cholesky.jl:65-82).
 * colptr/rowval/nzval are the SparseMatrixCSC fields (index_base = 1 from Julia, 0 from
 * SciPy).  Only entries in the lower blocks (i,i) and (i,i-1) are used, as in the
 * reference (:73,:76); the (i,i+1) blocks are ignored; anything further out is
 * GMRF_ERR_BAND.  The factor stays resident on the device inside `h`. */
gmrf_status gmrf_bt_factor_csc(gmrf_handle* h, int64_t n, int64_t n_blocks,
                               const int64_t* colptr, const int64_t* rowval,
                               const double* nzval, int32_t index_base, int32_t* info);

/* Same from the output of extract_blocks (scripts/solve_burger.jl:182-254): n_blocks
 * diagonal blocks and n_blocks-1 lower off-diagonal blocks, each block_size square, CSC
 * (compressed by column, like SparseMatrixCSC) when `compressed_by_column` != 0. */
gmrf_status gmrf_bt_factor_blocks(gmrf_handle* h, int64_t n, int64_t n_blocks,
                                  const gmrf_sparse_block* diag,
                                  const gmrf_sparse_block* lower,
                                  int32_t index_base, int32_t compressed_by_column,
                                  int32_t* info);

/* Re-run the factorisation with new values on the SAME sparsity pattern as the last
 * gmrf_bt_factor_csc (Gauss-Newton loop, scripts/solve_burger.jl:143-149). */
gmrf_status gmrf_bt_refactor_values(gmrf_handle* h, const double* nzval, int32_t* info);

/* ------------------------------------------------------------------ solves
 * mode FULL:     y = A^-1 b           ldiv!/ldiv      (:54-63)
 * mode FORWARD:  y = L^-1 b           forward_solve   (:43-52)
 * mode BACKWARD: y = L^-T b           backward_solve  (:24-33)
 * b, y: n x k column-major with leading dimensions ldb, ldy (a strided Julia view and a dense
 * result may differ); b == y (in place, as ldiv! allows) needs ldb == ldy.  Overlapping b and y (in place included) are
 * well defined for k <= 128 and take the launch-per-product sweeps (stats.sweep_persist). */
gmrf_status gmrf_bt_solve(gmrf_handle* h, const double* b, double* y, int64_t k,
                          int64_t ldb, int64_t ldy, int32_t mode);

/* k samples  x_s = mean + L^-T z_s  (rand(rng, x_cond), solve_darcy_gmrf-fem.jl:191).
 * z == NULL: z_s[dof] is Philox4x32-10(key = seed, counter = (dof, first_id + s)) through
 * Box-Muller, independent of GPU count and launch geometry.  z != NULL: n x k column-major
 * standard normals supplied by the caller (parity mode).  mean may be NULL (zero).  z overlapping out (k <= 128), or
 * mean == out with k = 1, is well defined and takes the launch-per-product sweeps. */
gmrf_status gmrf_bt_sample(gmrf_handle* h, uint64_t seed, int64_t first_id, int64_t k,
                           const double* mean, const double* z, double* out, int64_t ld);

/* mean = A^-1 b and k samples mean + L^-T z(id = first_id + s) in ONE call: what
 * scripts/darcy/solve_darcy_gmrf-fem.jl:190-191 asks of one factor (`mean`, then `rand`).  Results bitwise those of
 * gmrf_bt_solve(mode 0) followed by gmrf_bt_sample(mean = that mean, z = NULL); where the sweeps of a handle are persistent
 * launches (one problem, blocks of 512 .. 1024, device pointers, 2 <= k <= 128) the samples' sweep runs BESIDE the mean's two on a
 * second stream.  b, mean: n doubles; samples: n x k column-major, leading dimension ld.  stats.solve_ms = the whole call.
 * A batch (B > 1; b, mean: B x n, problem-major; samples: B groups of k columns, ids first_id + p k + s as gmrf_bt_sample draws
 * them) whose samples' sweep runs on the GEMM (k <= 128 padded to a multiple of 64, B * bsp / 64 * kp / 64 >= 128, device
 * pointers) makes ONE backward pass over the factor for both: the mean's backward sweep is the tail row of every product of the
 * samples' (kp + 1 panel rows); its samples' L^-T z are the same bits as gmrf_bt_sample's, its mean agrees with gmrf_bt_solve's to
 * rounding (summed by another kernel), stats.solve_ms = the whole call, stats.sample_ms = 0.  set_eager bit 18 (GMRF_SW_TWO_CALL_POSTERIOR) keeps the two calls.
 * If two of b, mean, samples overlap the call IS the two calls (each with its own guard against overlap). */
gmrf_status gmrf_bt_posterior(gmrf_handle* h, const double* b, uint64_t seed, int64_t first_id, int64_t k,
                              double* mean, double* samples, int64_t ld);

/* Registers the right-hand side of a batch's later gmrf_bt_posterior calls: b is a DEVICE pointer, n x B (problem-major, as
 * gmrf_bt_posterior takes it), and it is READ AT FACTOR TIME.  Later factorisations of a batch on the 256-column panel route
 * (gmrf_bt_factor_csc / refactor_values / factor_blocks) also solve L y = b inside the factor's own products and keep y beside
 * the factor; a fused gmrf_bt_posterior with this same pointer then skips its forward sweep (the mean agrees with the swept one
 * to rounding).  Whatever b holds when gmrf_bt_posterior runs, the mean is that of b as the factorisation read it.  Any other way
 * to a factor (ranges, adopt, import), a set_eager change, another b or b == NULL leaves no y: the forward sweep runs as before.
 * set_eager bit 19 (GMRF_SW_NO_FACTOR_FWD) switches the forward solve inside the factorisation off. */
gmrf_status gmrf_bt_set_factor_rhs(gmrf_handle* h, const double* b);

/* The N(0,1) draws gmrf_bt_sample would use (for tests and for callers that need z). */
gmrf_status gmrf_bt_normals(gmrf_handle* h, uint64_t seed, int64_t first_id, int64_t k,
                            double* z, int64_t ld);

/* Marginal variances diag(A^-1)  (std(x_cond), solve_darcy_gmrf-fem.jl:192).
 * EXACT: block-tridiagonal selected inversion (deterministic); serves a batch too, var_out is then
 *        [batch][n].
 * RBMC:  Rao-Blackwellised Monte Carlo over k Philox samples, needs Q (the factored matrix).
 * MC:    plain Monte Carlo over k samples.
 * var_out (here and in the batch call below): host or DEVICE memory -- a device pointer keeps the variances on the device (no
 * copy out; the call still returns after the handle's stream has finished). */
gmrf_status gmrf_bt_marginal_var(gmrf_handle* h, int32_t method, int64_t k, uint64_t seed,
                                 const gmrf_csr* Q, double* var_out);

/* RBMC / MC variances of every problem of a batch in one call (var_out is [batch][n]).  Q gives
 * the sparsity pattern only; q_vals[batch][nnz] are the problems' values in Q's CSR order (for
 * a symmetric matrix: the nzval arrays the factor was given).  Problem p draws the sample ids
 * p*k .. p*k+k-1. */
gmrf_status gmrf_bt_marginal_var_batch(gmrf_handle* h, int32_t method, int64_t k, uint64_t seed,
                                       const gmrf_csr* Q, const double* q_vals, double* var_out);

/* Selected inverse: the entries of Sigma = A^-1 at the stored positions of S (a gmrf_csr that gives the pattern only; its
 * values are ignored).  vals_out: [batch][nnz(S)] in S's CSR order, host or device memory (as gmrf_bt_marginal_var).
 * Every entry (r, c) of S must satisfy |blk(r) - blk(c)| <= 1 and, when the blocks differ, the index (r or c) that falls in
 * the LATER block must be < rmax within that block, rmax of the factored pattern (true for every entry of the matrix that
 * was factored and of any sub-pattern of it).  Otherwise GMRF_ERR_BAD_SHAPE, and gmrf_last_error names the first offending
 * entry.  The plan of a pattern is built on the first call and kept across refactor_values; a new analysis drops it.
 * Batches are served in lock step (one pattern for all problems).  No factor: GMRF_ERR_NO_FACTOR; a twisted handle:
 * GMRF_ERR_BAD_SHAPE. */
gmrf_status gmrf_bt_selinv(gmrf_handle* h, const gmrf_csr* S, double* vals_out);

/* out[p][j] = tr(A_p^-1 dA_{p,j}) = sum_e Sigma_p[e] * dvals[p][j][e]: dA_{p,j} has S's pattern, its values in S's CSR order
 * (both triangles, as a symmetric CSR holds them).  dvals [batch][m][nnz(S)], out [batch][m]; host or device each.
 * Sigma never leaves the device.  Deterministic: the same call gives the same bits.  Pattern rule and errors as
 * gmrf_bt_selinv; m outside [1, 65535]: GMRF_ERR_BAD_SHAPE. */
gmrf_status gmrf_bt_trace_inv(gmrf_handle* h, const gmrf_csr* S, const double* dvals, int64_t m, double* out);

/* Accumulators for sharded variance estimation: adds this rank's contribution of samples
 * [first_id, first_id + k) to acc (length n; RBMC: sum of squared off-diagonal terms,
 * MC: sum of squares).  The caller all-reduces acc and finishes with
 * var = 1/Q_ii + acc / K_total (RBMC) or acc / K_total (MC). */
gmrf_status gmrf_bt_var_accumulate(gmrf_handle* h, int32_t method, int64_t first_id,
                                   int64_t k, uint64_t seed, const gmrf_csr* Q,
                                   double* acc);

/* logdet(A) = 2 sum_i sum_j log (L_i)_jj. */
gmrf_status gmrf_bt_logdet(gmrf_handle* h, double* out);
/* logdet of EVERY problem of the handle in one call (the per-problem `logdet(x_final)` of the data-set loops,
 * scripts/burgers/solve_burgers_gmrf-collocation.jl:262): out [B], host or device.  Problem p gets the bits of gmrf_bt_logdet
 * after gmrf_bt_select_problem(h, p): the same per-block parts (from the resident L blocks, else what the factorisation left), added
 * in block order by one thread per problem and doubled.  One launch or two and one synchronisation instead of B round trips.
 * GMRF_ERR_BAD_SHAPE on a handle in the twisted order, GMRF_ERR_NO_FACTOR before a factorisation or for a factor adopted
 * without its L blocks. */
gmrf_status gmrf_bt_logdet_batch(gmrf_handle* h, double* out);

/* ------------------------------------------------------------------ factor access
 * Copy one dense block of the factor to `out` (block_size x block_size, column-major,
 * leading dimension ld):  kind L -> chos[i].L, kind C -> Cs[i] (= L_{i+2,i+1} in 1-based
 * block numbering; i in [0, n_blocks-1)), kind LINV -> inv(chos[i].L).  i is 0-based. */
gmrf_status gmrf_bt_get_block(gmrf_handle* h, int32_t kind, int64_t i, double* out,
                              int64_t ld);

/* Flat host image of the selected problem's factor (SURVEY 8b `gmrf_bt_export_factor` /
 * `_import_factor`; what a Julia caller materialises `F.chos` / `F.Cs` from in one call, and the
 * unit a checkpoint or a host-side broadcast moves).  Layout: int64 header[8] = {0x46524d47,
 * version 1, n, N, bs, 1, 0, 0}, then column-major bs x bs blocks L_1..L_N, C_1..C_{N-1},
 * Linv_1..Linv_N.  Import re-creates the device factor (no numeric work). */
gmrf_status gmrf_bt_export_size(gmrf_handle* h, int64_t* bytes);
gmrf_status gmrf_bt_export_factor(gmrf_handle* h, void* host_buf, int64_t bytes);
gmrf_status gmrf_bt_import_factor(gmrf_handle* h, const void* host_buf, int64_t bytes);

/* Storage of the factor on the device (all fp64, row-major blocks padded to bsp = 64 * 2^p):
 *   LINV  [batch][N][bsp][bsp]      Linv_i = inv(chos[i].L), lower triangular -- what the sweeps stream.
 *         SPLIT representation (batches whose coupling window starts at cmin >= 256; p = the largest power of two
 *         <= cmin): with a = [0, p), b = [p, bsp) the block holds X_aa, X_bb and, where X_ba = -X_bb L_ba X_aa would
 *         be, the factor's own L_ba -- nobody multiplies with X_ba (C_i = B_i Linv_{i-1}^T reads X_bb only), and the
 *         sweeps apply X_aa, L_ba, X_bb in turn (same bytes, same flops).  gmrf_bt_get_block(LINV), export and the
 *         exact variances convert the factor to the full inverse in place; the last entry of the layout record says
 *         which form a factor is in (0: full).
 *   C     [batch][N-1][rmax][bsp - cmin]   the non-zero WINDOW of Cs[i]: rows 0 .. rmax, columns cmin ..
 *         (a FEM coupling block is zero outside it; inside, row tile t is zero left of cmin + kst[t]).
 *         The layout record {cmin, rmax, n_row_tiles, kst[...], split p} comes from the symbolic phase
 *         (gmrf_bt_get_layout) and travels with a broadcast factor (gmrf_bt_adopt_layout).
 *   L     [batch][N][bsp][bsp]      chos[i].L -- only F.chos / export / logdet read it.  With
 *         gmrf_bt_set_keep_l(h, 0) L_i lives in a one-block work buffer (log-determinant parts are taken
 *         during the factorisation): darcy256 1.60 -> 0.84 GB per posterior; F.chos is then unavailable.
 * gmrf_bt_factor_buffer gives base pointer and byte count of one array; gmrf_bt_block_range the element
 * range (per problem, plus the problem stride) that holds blocks [i0, i1) -- the unit of a block-range
 * broadcast (for kind C: the coupling blocks i0-1 .. i1-2). */
gmrf_status gmrf_bt_factor_buffer(gmrf_handle* h, int32_t kind, void** dev_ptr,
                                  int64_t* bytes);
gmrf_status gmrf_bt_block_range(gmrf_handle* h, int32_t kind, int64_t i0, int64_t i1,
                                int64_t* first_elem, int64_t* n_elems, int64_t* problem_stride);
gmrf_status gmrf_bt_set_keep_l(gmrf_handle* h, int32_t keep);
gmrf_status gmrf_bt_get_layout(gmrf_handle* h, int64_t* out, int64_t cap, int64_t* count);

/* Packed transport image of the blocks [i0, i1) -- the unit that moves when a factor is shared (over xGMI by
 * gmrf_bt_bcast_blocks_async, or by a transport of the caller's own).  Per problem one segment of
 * gmrf_bt_packed_size doubles: the lower-triangular 64 x 64 tiles of Linv_i0 .. Linv_{i1-1} (tile (r, c), c <= r, of
 * block i at ((i - i0) * nt (nt + 1) / 2 + r (r + 1) / 2 + c) * 4096, row-major; nt = bsp / 64 -- the tiles above the
 * block diagonal are zero and never read, so they do not travel: 136 of 256 tiles at bsp = 1024), the stored windows
 * of the coupling blocks C_{i0-1} .. C_{i1-2}, a two-double representation tag {split column of the SENDER's block inverses
 * when it packed (0: full inverses), 1196249670.0}, and the blocks' log-determinant parts ((i1 - i0) doubles, rounded up to
 * an even count).  The tag is authoritative: gmrf_bt_adopt_commit follows it, not the layout record (which can be older
 * than the image: the sender converts to the full inverses for gmrf_bt_get_block(LINV) / export / exact variances and goes
 * back to the split form at its next factorisation); raw-buffer transfers carry no tag and follow the record.  darcy256: 0.56 GB per posterior instead of the 0.83 GB of the raw Linv / C buffers.  dev_buf:
 * device memory, [batch][segment].  pack reads the handle's factor storage, unpack fills it (a receiving rank:
 * gmrf_bt_adopt_layout first, gmrf_bt_adopt_commit after the last range; gmrf_bt_logdet then works there too).
 * Both are enqueued on the handle's stream and return.  (No reference counterpart: the reference is one process.) */
gmrf_status gmrf_bt_packed_size(gmrf_handle* h, int64_t i0, int64_t i1, int64_t* elems_per_problem);
gmrf_status gmrf_bt_pack_blocks_async(gmrf_handle* h, int64_t i0, int64_t i1, double* dev_buf);
gmrf_status gmrf_bt_unpack_blocks_async(gmrf_handle* h, int64_t i0, int64_t i1, const double* dev_buf);

/* Caller-owned factor storage (e.g. torch tensors that RCCL broadcasts): upper bounds of the sizes
 * for a shape and batch (C at its dense size), then the three device buffers (dev_L may be NULL after
 * gmrf_bt_set_keep_l(h, 0)).  `batch` must equal the handle's batch.  Must be set before the first
 * factor / adopt of that shape; the buffers must outlive the handle's use of them; whatever the
 * handle had factored before is dropped. */
gmrf_status gmrf_bt_storage_bytes(int64_t n, int64_t n_blocks, int64_t batch, int64_t* bytes_L,
                                  int64_t* bytes_C, int64_t* bytes_Linv);
gmrf_status gmrf_bt_set_storage(gmrf_handle* h, int64_t n, int64_t n_blocks, int64_t batch,
                                void* dev_L, void* dev_C, void* dev_Linv);

/* A rank that RECEIVES the factor (broadcast): shape plus the root's layout record (adopt_shape =
 * dense coupling blocks), storage allocated WITHOUT factoring; once the buffers have been filled
 * adopt_commit marks the factor valid (l_blocks_valid != 0: the L buffer was filled too); it waits for the handle's stream
 * (the ranges must have been unpacked on it, or ordered behind it by gmrf_comm_wait) and reads the representation tag. */
gmrf_status gmrf_bt_adopt_layout(gmrf_handle* h, int64_t n, int64_t n_blocks,
                                 const int64_t* layout, int64_t count);
gmrf_status gmrf_bt_adopt_shape(gmrf_handle* h, int64_t n, int64_t n_blocks);
gmrf_status gmrf_bt_adopt_commit(gmrf_handle* h, int32_t l_blocks_valid);

/* ------------------------------------------------------------------ multi-GPU (RCCL over xGMI)
 * One process per GPU.  The factor is shared, right-hand sides / samples are sharded:
 * rank 0 factors block ranges (gmrf_bt_factor_begin_csc / _step_async) and each finished range is
 * broadcast (R1) while the next one is being factored; every rank then solves / samples its own
 * sample ids; variance accumulators are summed with one all-reduce (R2).
 *   rank 0:  gmrf_comm_unique_id(id)  -> ship the 128 bytes to the other processes by any means
 *   all:     gmrf_comm_create(device, rank, world, id, &c)
 *   ranks>0: gmrf_bt_adopt_layout(h, n, N, layout)   (layout: gmrf_bt_get_layout on rank 0, moved with
 *            gmrf_comm_bcast_host)
 *   per job, for each block range:  rank 0: gmrf_bt_factor_step_async(h, i0, i1);
 *                                   all:    gmrf_bt_bcast_blocks_async(h, c, 0, i0, i1, 0)   (one packed image per
 *                                           range: gmrf_bt_pack_blocks_async -> ncclBroadcast -> _unpack_)
 *            then  all: gmrf_comm_wait(h, c);  rank 0: gmrf_bt_factor_end;  ranks>0: gmrf_bt_adopt_commit(h, 0)
 * librccl is opened with dlopen on first use (GMRF_RCCL_PATH overrides the search). */
gmrf_status gmrf_comm_unique_id(void* id128);
gmrf_status gmrf_comm_create(int32_t device, int32_t rank, int32_t world, const void* id128,
                             gmrf_comm** out);
gmrf_status gmrf_comm_destroy(gmrf_comm* c);
gmrf_status gmrf_comm_bcast_host(gmrf_comm* c, void* host_buf, int64_t bytes, int32_t root);
gmrf_status gmrf_comm_allreduce_sum(gmrf_comm* c, gmrf_handle* stream_of, double* dev_buf,
                                    int64_t count);
gmrf_status gmrf_bt_bcast_blocks_async(gmrf_handle* h, gmrf_comm* c, int32_t root, int64_t i0,
                                       int64_t i1, int32_t with_l);
gmrf_status gmrf_comm_wait(gmrf_handle* h, gmrf_comm* c);
/* The all-gather form of sharing a BATCH of factors (round 4): every rank factors its own share of the batch on `src`
 * (src batch b) and the packed images of the blocks [i0, i1) are all-gathered (ncclAllGather) into `dst`, a handle of the same
 * shape with batch world * b that adopted src's layout record: problem r * b + p of dst = problem p of rank r.  Every rank
 * then takes means / samples of ALL world * b posteriors on dst (its own sample ids).  Against the root broadcast the
 * factorisation is spread over the ranks and every xGMI link carries 1 / world of the images instead of the root's links
 * carrying all of them.
 *   per job, for each block range:  all: gmrf_bt_factor_step_async(src, i0, i1);
 *                                        gmrf_bt_allgather_blocks_async(src, dst, c, i0, i1)
 *            then  all: gmrf_bt_factor_end(src);  gmrf_comm_wait(dst, c);  gmrf_bt_adopt_commit(dst, 0)
 * (No reference counterpart: the reference is one process.) */
gmrf_status gmrf_bt_allgather_blocks_async(gmrf_handle* src, gmrf_handle* dst, gmrf_comm* c, int64_t i0, int64_t i1);
/* Factor bytes this communicator has broadcast so far (reset != 0 clears the counter afterwards). */
gmrf_status gmrf_comm_bytes(gmrf_comm* c, int32_t reset, double* bytes);

/* Streams for several handles driven side by side (one host thread and one stream per handle: the latency-bound
 * launches of one factorisation leave CUs to the others -- bench.py runs 4 handles x 32 problems).  The HIP runtime
 * multiplexes streams onto a few hardware queues (4 by default) and two streams that land on the same queue
 * SERIALISE: measured on MI355X, 4 handles on 4 streams of which two share a queue deliver 27.3 k solves/s, on four
 * distinct queues 32.2 k (tools/stream_pairs.py).  gmrf_streams_create makes candidate streams
 * (hipStreamNonBlocking), runs a 1 ms spin kernel on pairs of them to find out which overlap, keeps n mutually
 * overlapping ones (as far as there are: *n_distinct tells how many of the returned streams are on queues of their
 * own) and destroys the rest.  streams: n hipStream_t, to be passed to gmrf_bt_create / released with
 * gmrf_streams_destroy.  (No reference counterpart: the reference is single-threaded CPU code.) */
gmrf_status gmrf_streams_create(int32_t device, int32_t n, void** streams, int32_t* n_distinct);
gmrf_status gmrf_streams_destroy(int32_t device, int32_t n, void** streams);

/* Pipelined factorisation (factor block ranges so a broadcast of finished blocks can
 * overlap): begin uploads the matrix, step_async enqueues blocks [i0, i1) and returns,
 * end synchronises and reports SPD failures.  Exception: a range that held persistent launches
 * (stats.persist_route != 0) is waited for inside step_async, and repeated with a launch per step
 * if one of them gave up, so that what the caller shares next is the factor; on such handles
 * step_async returns only when its range is done. */
gmrf_status gmrf_bt_factor_begin_csc(gmrf_handle* h, int64_t n, int64_t n_blocks,
                                     const int64_t* colptr, const int64_t* rowval,
                                     const double* nzval, int32_t index_base);
gmrf_status gmrf_bt_factor_step_async(gmrf_handle* h, int64_t i0, int64_t i1);
gmrf_status gmrf_bt_factor_end(gmrf_handle* h, int32_t* info);

/* Batch of B independent problems that share ONE sparsity pattern (the reference's loop over
 * data-set problems, scripts/darcy/solve_darcy_gmrf-fem.jl:176-198): they are factored and
 * solved in lock step, problem = one more grid dimension of every kernel.  With B > 1:
 * nzval holds B value arrays one after the other; b / y / z / out hold B consecutive groups of
 * k columns (problem-major); mean holds B vectors; sample ids are first_id + p*k + s.
 * Accessors (get_block, logdet) address the problem chosen by gmrf_bt_select_problem. */
gmrf_status gmrf_bt_set_batch(gmrf_handle* h, int64_t batch);
gmrf_status gmrf_bt_select_problem(gmrf_handle* h, int64_t p);

/* Elimination order of one problem.  REFERENCE (default): L L^T, blocks 0 .. N-1 in turn, as the reference does.
 * TWISTED: Q = T T^T with two chains that run at the same time -- blocks 0 .. m-1 downward (L_i, G_i = T[i, i-1]), blocks N-1 ..
 * m+1 upward (upper-triangular U_i, H_i = T[i, i+1]) -- and meet in block m: L_m L_m^T = D_m - G_m G_m^T - H_m H_m^T.  The same
 * flops in about half the dependent steps.  Order-invariant: A^-1 b, marginal variances, logdet.  Order-specific: the blocks
 * (gmrf_bt_get_block: kind L -> L_i (i <= m) or U_i (i > m); kind C, index i -> G_{i+1} (i < m) or H_i (i >= m); kind LINV ->
 * T_ii^-1), the half-solves (FORWARD = T^-1 b, BACKWARD = T^-T b) and a sample mean + T^-T z for a given z (the Philox z of a
 * seed / id is the same in both orders).
 * meet = -1: automatic (balances the two chains; N < 3: m = N - 1, which is the reference order bitwise); otherwise m in
 * [0, N-1], checked at factor time.  Unknown order: GMRF_ERR_BAD_SHAPE.  The call drops the current factor and pattern.
 * A twisted handle needs batch 1 and supports factor_csc, refactor_values, solve, sample, posterior, normals, marginal_var,
 * var_accumulate, logdet, get_block, stats, synchronize, set_eager and set_profiling; every other gmrf_bt_* call on it returns
 * GMRF_ERR_BAD_SHAPE with a gmrf_last_error that names the twisted order.  NOT_SPD: *info = the failing block, original 1-based.
 * gmrf_bt_get_order returns the resolved m after a factorisation (N - 1 for the reference order). */
enum { GMRF_ORDER_REFERENCE = 0, GMRF_ORDER_TWISTED = 1 };
gmrf_status gmrf_bt_set_order(gmrf_handle* h, int32_t order, int64_t meet);
gmrf_status gmrf_bt_get_order(gmrf_handle* h, int32_t* order, int64_t* meet);
/* Statistics of one half of a twisted handle (half 0: blocks 0 .. m, half 1: blocks N-1 .. m+1; persist_route / persist_cus /
 * persist_aborts of that half's factorisation).  gmrf_bt_stats of a twisted handle sums both halves' persist_aborts. */
gmrf_status gmrf_bt_half_stats(gmrf_handle* h, int32_t half, gmrf_stats* out);

gmrf_status gmrf_bt_stats(gmrf_handle* h, gmrf_stats* out);
gmrf_status gmrf_bt_set_profiling(gmrf_handle* h, int32_t level);
/* The route switches of a handle: gmrf_bt_set_eager takes the OR of any of them (0: every default route).  The values are ABI. */
enum {
    GMRF_SW_EAGER              = 1 << 0,    /* plain stream launches instead of replaying captured HIP graphs */
    GMRF_SW_BATCH_ROUTES       = 1 << 1,    /* the three-launch panel step (the batches' in-block routes) also for batch 1 (experiment) */
    GMRF_SW_SWEEP_NO_GEMM      = 1 << 2,    /* keep 64-multiples of right-hand sides on sweep_mm */
    GMRF_SW_DENSE_COUPLING     = 1 << 3,    /* C = B X^T by the dense GEMM even when the lower blocks are sparse */
    GMRF_SW_FORK_GRAPH         = 1 << 4,    /* second branch in the captured factor graph: inverse assembly beside the panel chain (experiment) */
    GMRF_SW_NO_STAIRCASE       = 1 << 5,    /* ignore the staircase of the coupling blocks: dense window; takes effect at the next factor_csc */
    GMRF_SW_DOUBLING_INVERSE   = 1 << 7,    /* one problem assembles Linv by recursive doubling after the panel steps, not row by row inside them */
    GMRF_SW_NO_LOOKAHEAD       = 1 << 8,    /* one problem re-factors the diagonal tile in every workgroup of a step instead of the look-ahead chain */
    GMRF_SW_NO_XSPLIT          = 1 << 12,   /* batches always assemble the full block inverses: no split representation (comparison) */
    GMRF_SW_NO_PERSIST         = 1 << 13,   /* no persistent launches (potrf_persist, sweep_persist): the launch-per-step / per-product forms */
    GMRF_SW_NO_PERSIST_PANELS  = 1 << 15,   /* small batches keep potrf_diag128 + the 128^3 products instead of one persistent launch per panel diagonal block */
    GMRF_SW_NO_SWEEP_PERSIST   = 1 << 16,   /* one problem's sweeps keep one launch per product instead of ONE persistent launch per sweep (comparison) */
    GMRF_SW_NO_SCATTER_FOLD    = 1 << 17,   /* one problem keeps scatter_block (S += D_i) a launch of its own behind S = -C C^T, not folded into spmm_bxt_tiles (comparison; same bits) */
    GMRF_SW_TWO_CALL_POSTERIOR = 1 << 18,   /* a batch's gmrf_bt_posterior is gmrf_bt_solve + gmrf_bt_sample, not the fused pass (comparison; samples the same bits, mean to rounding) */
    GMRF_SW_NO_FACTOR_FWD      = 1 << 19,   /* factorisations do not solve for the right-hand side of gmrf_bt_set_factor_rhs: the posterior's forward sweep runs (comparison) */
    GMRF_SW_NO_GROUPED_GEMM    = 1 << 20,   /* a 256-column panel's two independent 128^3 products stay two launches, not ONE of gemm_f64_dma_grouped (comparison; same bits) */
    GMRF_SW_NO_ENVELOPE        = 1 << 21    /* batched panel products, rank-256 updates and the backward L_ba^T product run their whole K ranges, no envelope skip (comparison; same bits) */
};
/* (Bits 6, 9, 10, 11 and 14 selected comparison routes that were removed in round 5; they are retired and ignored.) */
gmrf_status gmrf_bt_set_eager(gmrf_handle* h, int32_t eager);
gmrf_status gmrf_bt_synchronize(gmrf_handle* h);

/* ------------------------------------------------------------------ K6: CSR SpMV / SpMM
 * Device-resident sparse matrix built from CSR arrays (rowptr has n_rows+1 entries) --
 * or, for a symmetric matrix, from the CSC arrays of the same matrix.  values_f32 != 0
 * stores the values in fp32 and accumulates in fp64 (BASELINE config 5). */
gmrf_status gmrf_csr_create(int32_t device, void* stream, int64_t n_rows, int64_t n_cols,
                            const int64_t* rowptr, const int64_t* colidx,
                            const double* vals, int32_t index_base, int32_t values_f32,
                            gmrf_csr** out);
gmrf_status gmrf_csr_destroy(gmrf_csr* m);
/* Y = S X ;  X: n_cols x k, Y: n_rows x k, column-major with leading dimensions ldx, ldy. */
gmrf_status gmrf_spmm(const gmrf_csr* S, const double* X, double* Y, int64_t k,
                      int64_t ldx, int64_t ldy);
/* The same product with NODE-MAJOR operands: X is n_cols x k with the k values of one column index
 * contiguous (row stride ldx >= k), Y likewise -- in Julia the k x n matrices permutedims(X),
 * permutedims(Y).  This is the layout of the LDS-tiled kernel (csr_spmm_tiles): one gathered column
 * index fetches k contiguous doubles, and the distinct rows of X a 64-row tile needs are staged in
 * LDS once (the RBMC estimator of `std(x)` runs on it: 50 samples x Q * x,
 * scripts/darcy/solve_darcy_gmrf-fem.jl:100,192). */
gmrf_status gmrf_spmm_rows(const gmrf_csr* S, const double* X, double* Y, int64_t k,
                           int64_t ldx, int64_t ldy);
/* Stream-ordered variants for DEVICE operands: the product is enqueued on the matrix's stream (gmrf_csr_create) and
 * the call returns without synchronising -- `Q * x` inside a device-resident loop. */
gmrf_status gmrf_spmm_async(const gmrf_csr* S, const double* X, double* Y, int64_t k, int64_t ldx, int64_t ldy);
gmrf_status gmrf_spmm_rows_async(const gmrf_csr* S, const double* X, double* Y, int64_t k, int64_t ldx, int64_t ldy);

/* ------------------------------------------------------------------ posterior assembly
 * The step before the factorisation in the reference's Gauss-Newton loop
 * (scripts/solve_burger.jl:143-149) and in `condition_on_observations`:
 *     A   = Q + noise * J' * J                       (gmrf_assemble_precision)
 *     rhs = base + noise * J' * (J * x + obs_diff)   (gmrf_assemble_rhs; base = Q * x_prior)
 * Patterns are fixed, values change per iteration.  create() does the symbolic work on the host
 * (Q: CSC n x n with ascending rows per column, both triangles; J: CSR m x n); the numeric calls
 * take host or device pointers, and the device output of gmrf_assemble_precision is the `nzval`
 * array of the pattern gmrf_assemble_pattern returns -- feed it to gmrf_bt_factor_csc once and to
 * gmrf_bt_refactor_values afterwards.  device = -1: symbolic only (pattern queries). */
typedef struct gmrf_assembler gmrf_assembler;
gmrf_status gmrf_assemble_create(int32_t device, void* stream, int64_t n, const int64_t* q_colptr,
                                 const int64_t* q_rowval, int64_t m, const int64_t* j_rowptr,
                                 const int64_t* j_colidx, int32_t index_base, gmrf_assembler** out);
gmrf_status gmrf_assemble_destroy(gmrf_assembler* as);
/* nnz of the result, number of J[k,i] * J[k,j] products, and (if not NULL) its CSC pattern. */
gmrf_status gmrf_assemble_pattern(const gmrf_assembler* as, int64_t* nnz_out, int64_t* n_products,
                                  int64_t* colptr, int64_t* rowval, int32_t index_base);
gmrf_status gmrf_assemble_precision(gmrf_assembler* as, const double* q_nzval, const double* j_vals,
                                    double noise, double* out_nzval);
/* obs_diff and base may be NULL (zero). */
gmrf_status gmrf_assemble_rhs(gmrf_assembler* as, const double* base, const double* j_vals,
                              const double* x, const double* obs_diff, double noise, double* out);

/* ------------------------------------------------------------------ FEM block assembly (first piece)
 * Darcy stiffness matrix  G[i][j] = int a grad(phi_i).grad(phi_j),  f[i] = beta int phi_i  with the
 * homogeneous Dirichlet rows / columns applied -- assemble_darcy_diff_matrix,
 * /root/reference/src/problems/darcy.jl:5-63 (cell loop :27-60, coefficient looked up at the quadrature
 * point by nearest grid point, src/datasets/darcy.jl:30-34; `apply!` :61) -- on the structured P1 mesh
 * of the BASELINE Darcy configs: nx x ny nodes on the unit square, x fastest, quads cut by the diagonal
 * n00 - n11, one quadrature point per cell.  The values come out in CSR order of the 7-point
 * pattern gmrf_darcy_p1_pattern returns, which is the `J` of gmrf_assemble_precision
 * (Q_post = Q + Q_eps G'G): per problem only the ng x ng coefficient table crosses the bus.
 * coeff_table[ix * ng + iy] = a at grid point (x = ix / (ng-1), y = iy / (ng-1)); host or device
 * pointers; device = -1: pattern only. */
typedef struct gmrf_darcy_p1 gmrf_darcy_p1;
gmrf_status gmrf_darcy_p1_create(int32_t device, void* stream, int64_t nx, int64_t ny, gmrf_darcy_p1** out);
/* The same assembler with the reference's own element (src/utils.jl:32-33): Lagrange{RefTriangle,2} and the 4-point rule of
 * QuadratureRule{RefTriangle}(3) on the nx x ny vertex mesh; dofs = the (2 nx - 1) x (2 ny - 1) lattice of vertices and edge
 * midpoints, x fastest; the coefficient is looked up at every quadrature point.  Same handle type: gmrf_darcy_p1_pattern /
 * _assemble / _destroy serve both (n = (2 nx - 1)(2 ny - 1) rows, up to 19 entries per row). */
gmrf_status gmrf_darcy_p2_create(int32_t device, void* stream, int64_t nx, int64_t ny, gmrf_darcy_p1** out);
gmrf_status gmrf_darcy_p1_destroy(gmrf_darcy_p1* d);
gmrf_status gmrf_darcy_p1_pattern(const gmrf_darcy_p1* d, int64_t* nnz_out, int64_t* rowptr, int64_t* colidx,
                                  int32_t index_base);
gmrf_status gmrf_darcy_p1_assemble(gmrf_darcy_p1* d, const double* coeff_table, int64_t ng, double beta,
                                   double* vals_out, double* f_out);

/* Residual and tangent of the implicit-Euler Burgers space-time system (FEM block assembly, second piece):
 *     J(w) = J_static + dt J_adv(w),     f(w) = J_static w + dt v_adv(w)
 * -- f_and_J / nonlinear_primal_tangent, /root/reference/scripts/burgers/solve_burgers_gmrf-fem.jl:118-149, with
 * J_static = M_{t+1} - M_t + dt nu G_{t+1} (:123-130; assemble_burgers_mass_diffusion_matrices,
 * src/problems/burgers.jl:60-98) and assemble_burgers_advection_matrix (src/problems/burgers.jl:5-59, cell loop
 * :22-51) per time slice -- on the periodic P1 line of the BASELINE Burgers configs: ns nodes on [0,1), nt time
 * slices, time-major index (t-1) ns + s, 3-point Gauss rule.  J has (nt-1) ns rows (slices 2 .. nt), nt ns columns
 * and 6 entries per row; the values come out in the CSR order of gmrf_burgers_p1_pattern, which is the `J` that
 * gmrf_assemble_precision / gmrf_assemble_rhs take: a Gauss-Newton iteration (scripts/solve_burger.jl:143-149)
 * moves only w across the bus, or nothing at all with device pointers.  w, vals_out ((nt-1) ns 6), f_out
 * ((nt-1) ns): host or device pointers.  device -1: pattern only. */
typedef struct gmrf_burgers_p1 gmrf_burgers_p1;
gmrf_status gmrf_burgers_p1_create(int32_t device, void* stream, int64_t ns, int64_t nt, double dt, double nu,
                                   gmrf_burgers_p1** out);
/* The same on the QUADRATIC periodic line, the element the reference's Burgers scripts run on
 * (periodic_unit_interval_discretization, /root/reference/src/utils.jl:42-49: QuadraticLine cells, Lagrange{RefLine,2},
 * 3-point Gauss rule): ns = 2 N_x dofs numbered by position, even = cell boundaries, odd = midpoints; vertex rows of J hold
 * 10 entries (columns i-2 .. i+2 of slices t-1 and t), midpoint rows 6.  The handle is a gmrf_burgers_p1: _pattern,
 * _tangent and _destroy serve both element orders. */
gmrf_status gmrf_burgers_p2_create(int32_t device, void* stream, int64_t ns, int64_t nt, double dt, double nu,
                                   gmrf_burgers_p1** out);
/* The common creator: the line tangent over three independent choices (all 8 combinations), behind the same handle --
 * _pattern, _tangent, _tangent_batch, _destroy and gmrf_gn_create / _run / _finalize serve every variant.
 *   order   1 or 2, the elements above.
 *   scheme  GMRF_BURGERS_EULER as above, or GMRF_BURGERS_CN, Crank-Nicolson (J_static_CN, nonlinear_primal_tangent_CN,
 *           f_and_J_CN of _research/burgers_chen24.jl:121-132, :195-226): for the row block of the step t-1 -> t
 *               J[:, t-1] = -M + (dt nu 0.5) G + (dt 0.5) A(w_{t-1}),    J[:, t] = M + (dt nu 0.5) G + (dt 0.5) A(w_t),
 *               f = (static part of the row) . w + dt 0.5 (v(w_{t-1}) + v(w_t))
 *           with A, v the advection tangent and residual of one slice.  The pattern is implicit Euler's (consistent mass).
 *   bc      GMRF_BURGERS_PERIODIC: nc cells on [0, length), order nc dofs, wrap-around columns, as above;
 *           GMRF_BURGERS_DIRICHLET: nc cells on an interval of that length with homogeneous Dirichlet ends
 *           (_research/burgers_chen24.jl:101-108): ns = order nc + 1 dofs numbered by position, dofs 0 and ns-1 prescribed and
 *           treated as src/problems/burgers.jl:53-57, :87-92 treats them: their rows and columns of J hold stored 0.0 and f
 *           is 0.0 there, so m = (nt-1) ns stays uniform (a prior pins them).  A row holds its in-range columns only.
 * Only `length` enters (the cell length is length / nc), not the interval's origin.  gmrf_burgers_p1_create(ns) is
 * (nc = ns, order 1, euler, periodic, 1.0), gmrf_burgers_p2_create(ns) is (nc = ns / 2, order 2, ...): same kernels, same bits.
 * GMRF_ERR_BAD_SHAPE: an unknown order, scheme or bc, length <= 0, nc < 3 (periodic) or < 2 (dirichlet), nt < 2. */
typedef enum { GMRF_BURGERS_EULER = 0, GMRF_BURGERS_CN = 1 } gmrf_burgers_scheme;
typedef enum { GMRF_BURGERS_PERIODIC = 0, GMRF_BURGERS_DIRICHLET = 1 } gmrf_burgers_bc;
gmrf_status gmrf_burgers_line_create(int32_t device, void* stream, int64_t nc, int64_t nt, double dt, double nu, int32_t order,
                                     int32_t scheme, int32_t bc, double length, gmrf_burgers_p1** out);
/* The same handle for the COLLOCATION form of the implicit-Euler step: residual and tangent evaluated at points instead of
 * tested against basis functions -- f_and_J of the reference's scripts/burgers/solve_burgers_gmrf-collocation.jl:186-192 with
 * J_static (:183) and the operators A_coll, du/dx, d2u/dx2 of :167-169 -- on the periodic quadratic line above: nc cells of
 * length / nc, ns = 2 nc dofs numbered by position, cell e with the dofs (left, right, middle) = (2e, (2e+2) mod ns, 2e+1).
 * `points` is a HOST array of npts coordinates in [0, length), in any order, several of them in one cell if need be.  Per point,
 * once at creation and in double precision: e = min(floor(x / h), nc - 1), xi = 2 (x - e h) / h - 1, shape values
 * a = (xi(xi-1)/2, xi(xi+1)/2, 1 - xi^2), first derivatives d = (xi - 1/2, xi + 1/2, -2 xi) 2/h, second derivatives
 * s = (1, 1, -2) 4/h^2.  Row r = (t-1) npts + c (t = 1 .. nt-1, 0-based slices; rows = (nt-1) npts), with u = sum a_k w_t[k],
 * u_x = sum d_k w_t[k], u_xx = sum s_k w_t[k], u- = sum a_k w_{t-1}[k] summed in the local order (left, right, middle):
 *     f_r = u - u- + dt u u_x - dt nu u_xx,    J[r, t-1, k] = -a_k,    J[r, t, k] = a_k + dt (u_x a_k + u d_k) - dt nu s_k.
 * Six stored entries per row (nnz = 6 rows): the cell's three dofs of slice t-1 in ascending column order, then of slice t; the
 * wrap cell's columns sort as (0, 2e, 2e+1).  An entry that is exactly 0.0 (a point on a vertex) is stored.  _pattern, _tangent,
 * _tangent_batch, _destroy and gmrf_gn_create / _run / _finalize serve the handle; device -1 gives the pattern only.
 * GMRF_BURGERS_COLLOCATION is the handle's scheme, and a value gmrf_burgers_line_create keeps rejecting.
 * GMRF_ERR_BAD_SHAPE: nc < 3, nt < 2, npts < 1, dt <= 0, nu < 0, length <= 0, or a point that is not finite or not in
 * [0, length) -- gmrf_last_error names it. */
enum { GMRF_BURGERS_COLLOCATION = 2 };
gmrf_status gmrf_burgers_colloc_create(int32_t device, void* stream, int64_t nc, int64_t nt, double dt, double nu,
                                       double length, int64_t npts, const double* points, gmrf_burgers_p1** out);
gmrf_status gmrf_burgers_p1_destroy(gmrf_burgers_p1* b);
gmrf_status gmrf_burgers_p1_pattern(const gmrf_burgers_p1* b, int64_t* nnz_out, int64_t* rowptr, int64_t* colidx,
                                    int32_t index_base);
gmrf_status gmrf_burgers_p1_tangent(gmrf_burgers_p1* b, const double* w, double* vals_out, double* f_out);

/* The prior of the Burgers space-time GMRF for a batch of problems (the "Prior" stage of the data-set loop, form_prior of
 * scripts/burgers/solve_burgers_gmrf-fem.jl:86-107, and the information vector of its "Initial condition" stage, :161) on the
 * periodic P1 line with lumped mass, ns nodes, nt slices, time-major index -- the mesh of gmrf_burgers_p1_create.  Every problem
 * brings its initial condition ic [ns]; the prior depends on it through bulk = mean(ic):
 *     Q_ic = Q_prior(bulk) + ic_noise A_ic' A_ic,      Qx_prior = Q_prior(bulk) (bulk 1) + ic_noise A_ic' ic
 * with A_ic the restriction to the first slice, so that Q_ic^-1 Qx_prior is the mean of the prior conditioned on the initial
 * condition.  The pattern is structural: symmetric CSC, both triangles, rows ascending, nt blocks of ns; diagonal blocks hold the
 * periodic offsets 0, +-1, +-2, the blocks beside them 0, +-1; nnz = (11 nt - 6) ns; fixed by (ns, nt), an entry whose value is
 * 0.0 is stored.  ns < 5 (the offsets fold onto each other), nt < 2, nu <= 0: GMRF_ERR_BAD_SHAPE.  The other lines of
 * gmrf_burgers_line_create have their prior in gmrf_burgers_line_prior_create below.
 * gmrf_burgers_prior_values_batch: ic [batch][ns] -> bulk_out [batch], q_values_out [batch][nnz] in the order of _pattern (the
 * q_nzval of gmrf_gn_run at q_stride = nnz), qx_out [batch][nt ns]; each output may be NULL, every pointer host or device memory;
 * batch in [1, 4096].  The means are fixed-shape sums without atomics, the values are bitwise symmetric, and problem p's bits do
 * not depend on the batch or on its place in it.  device -1: pattern only. */
typedef struct gmrf_burgers_prior gmrf_burgers_prior;
gmrf_status gmrf_burgers_prior_create(int32_t device, void* stream, int64_t ns, int64_t nt, double dt, double nu, double ic_noise,
                                      gmrf_burgers_prior** out);
gmrf_status gmrf_burgers_prior_destroy(gmrf_burgers_prior* p);
gmrf_status gmrf_burgers_prior_pattern(const gmrf_burgers_prior* p, int64_t* nnz_out, int64_t* colptr, int64_t* rowval,
                                       int32_t index_base);
gmrf_status gmrf_burgers_prior_values_batch(gmrf_burgers_prior* p, int64_t batch, const double* ic, double* bulk_out,
                                            double* q_values_out, double* qx_out);
/* The same prior on every line gmrf_burgers_line_create serves: the periodic QUADRATIC line that form_prior runs on in
 * /root/reference/scripts/burgers/solve_burgers_gmrf-fem.jl:71-72, :86-107 (element_order = 2), and the interval with pinned ends
 * of _research/burgers_chen24.jl:79-108 (prescribed_noise = 1e-8, i.e. pin = 1e8), with this project's restatement of the prior
 * (`workloads.burgers_line_prior_from_bulk`): nc cells of length / nc, ns = order nc (periodic) or order nc + 1 (dirichlet) dofs
 * numbered by position, l the lumped mass (row sums), S the stiffness, Adv[i][j] = int phi_i phi_j', c = 1 / nu, gamma = -c bulk,
 * tau = 0.1 sqrt(c), kappa^2 = 12 nc:
 *     K = kappa^2 diag(l) + S,  G = diag(l) + dt (nu c S + gamma Adv),  W = diag((1 / (dt tau^2)) / l)
 *     block (t, t) = G'WG (t > 0) or K diag(1 / l) K (t = 0), + diag(l) W diag(l) for t < nt-1;   block (t, t-1) = -G'W diag(l)
 *     dirichlet: + pin on the diagonal of dofs 0 and ns-1 of every slice (pin is ignored on the periodic line)
 *     Q_ic = Q_prior + ic_noise A_ic' A_ic,   Qx_prior = Q_prior(without the pins) (bulk 1) + ic_noise A_ic' ic
 * A_ic observes slice 0 at GMRF_BURGERS_IC_ALL, every dof that is not pinned, or GMRF_BURGERS_IC_VERTICES (order 2), the even ones
 * of them -- a data grid of one point per cell; bulk is the mean of ic over the observed dofs (ic is [ns] either way).  The pattern
 * is structural, symmetric CSC, both triangles, rows ascending: offsets 0 .. +-2 order in the diagonal blocks and 0 .. +-order
 * beside them, wrapped (periodic) or clipped to the slice (dirichlet); an entry whose value is 0.0 is stored;
 * nnz = ((4o+1) nt + 2 (2o+1) (nt-1)) ns (periodic), nt ((4o+1) ns - 2o (2o+1)) + 2 (nt-1) ((2o+1) ns - o (o+1)) (dirichlet).
 * The handle is a gmrf_burgers_prior: _pattern, _values_batch (same outputs, pointer kinds and guarantees), _destroy and
 * gmrf_bic_create / _run serve it.  (order 1, periodic, length 1, all) is the prior of gmrf_burgers_prior_create evaluated by
 * other kernels: the same pattern and bulk, values equal to rounding.  GMRF_ERR_BAD_SHAPE, the argument named: an unknown order, bc
 * or ic_obs, vertices at order 1, length <= 0, nu <= 0, dt <= 0, pin < 0, nt < 2, periodic with order nc < 4 order + 1 (the
 * offsets fold), dirichlet with nc < 2.  device -1: pattern only. */
typedef enum { GMRF_BURGERS_IC_ALL = 0, GMRF_BURGERS_IC_VERTICES = 1 } gmrf_burgers_ic_obs;
gmrf_status gmrf_burgers_line_prior_create(int32_t device, void* stream, int64_t nc, int64_t nt, double dt, double nu,
                                           double ic_noise, int32_t order, int32_t bc, double length, double pin, int32_t ic_obs,
                                           gmrf_burgers_prior** out);

/* A batch of Gauss-Newton loops on one mesh (the Burgers data-set loop, scripts/burgers/solve_burgers_gmrf-fem.jl:154-233 with the
 * loop body of scripts/solve_burger.jl:143-180).  All arrays are problem-major ([batch][...]), host or device pointers like the
 * one-problem calls; problem p of a batch call gets the bits of the one-problem call on its slice.  q_stride: 0 = one Q for
 * every problem, nnz(Q) = one value array per problem (the prior depends on the initial condition).
 *     obj[p] = (x_prior_p - x_p)' Q_p (x_prior_p - x_p) + noise |obs_diff_p|^2                  (gmrf_assemble_objective_batch)
 * is summed over a fixed partition without atomics: the same bits on every call and in every batch. */
gmrf_status gmrf_burgers_p1_tangent_batch(gmrf_burgers_p1* b, int64_t batch, const double* w, double* vals_out, double* f_out);
gmrf_status gmrf_assemble_precision_batch(gmrf_assembler* as, int64_t batch, const double* q_nzval, int64_t q_stride,
                                          const double* j_vals, double noise, double* out_nzval);
gmrf_status gmrf_assemble_rhs_batch(gmrf_assembler* as, int64_t batch, const double* base, const double* j_vals,
                                    const double* x, const double* obs_diff, double noise, double* out);
gmrf_status gmrf_assemble_objective_batch(gmrf_assembler* as, int64_t batch, const double* q_nzval, int64_t q_stride,
                                          const double* x_prior, const double* x, const double* obs_diff, double noise,
                                          double* obj_out);
/* out[p] = (z_p - x_p)' A_p (z_p - x_p): `sqmahal(x_final, z)` of scripts/burgers/solve_burgers_gmrf-collocation.jl:208-215 for a
 * batch, with A_p the symmetric matrix on the assembler's OUTPUT pattern (gmrf_assemble_pattern: nnz_out entries, both triangles,
 * in that order) and the values a_nzval[p] -- what gmrf_assemble_precision_batch wrote.  a_stride: 0 = one value array for every
 * problem, nnz_out = one per problem.  x, z [batch][n], out [batch]; every pointer host or device.  One pass over the values,
 * z - x formed as it is read; summed over a fixed partition of the columns (it depends on n only) without atomics: the same bits on
 * every call and in every batch.  Needs n < 2^31. */
gmrf_status gmrf_assemble_quadform_batch(gmrf_assembler* as, int64_t batch, const double* a_nzval, int64_t a_stride,
                                         const double* x, const double* z, double* out);
/* The driver binds a handle (reference order; its batch B is the number of problems), an assembler and a Burgers tangent that
 * live on ONE device and ONE stream (create the three with the same stream argument); anything else is GMRF_ERR_BAD_SHAPE.
 * gmrf_gn_run: the handle must have factored the assembler's pattern once (GMRF_ERR_NO_FACTOR before the first analysis,
 * GMRF_ERR_BAD_SHAPE for another pattern).  Per iteration, on the handle's stream and without a host round trip but the status
 * words: tangent -> A = Q + noise J'J and rhs -> gmrf_bt_refactor_values -> solve -> objective -> stop rule.  A problem is active
 * while |last - cur| / |cur| > rtol and steps < max_steps (the first `last` is +Inf); a problem that has stopped is frozen (its x,
 * history and count no longer change) and stays in the batch.  x [B][n]: in the start points, out the results; y [B][m] the
 * observations (NULL = 0); steps_out [B]; obj_hist_out [B][max_steps + 1] (slot 0: the start point; slots no step reached: NaN).
 * GMRF_ERR_NOT_SPD in any problem ends the run (`info`: the failing block, as gmrf_bt_refactor_values reports it); x then holds
 * the last complete iterate of every problem and steps_out says which.  The run's right-hand sides are registered with
 * gmrf_bt_set_factor_rhs for its duration (the caller's registration is put back); GMRF_SW_NO_FACTOR_FWD switches that route off.
 * gmrf_gn_finalize: tangent at the final x, assemble, re-factor -- the handle then holds the factor of
 * Q + noise J(x)' J(x) of every problem (x_final of solve_burgers_gmrf-fem.jl:184-193) for posterior / sample / variance calls. */
typedef struct gmrf_gn gmrf_gn;
gmrf_status gmrf_gn_create(gmrf_handle* h, gmrf_assembler* as, gmrf_burgers_p1* b, gmrf_gn** out);
gmrf_status gmrf_gn_destroy(gmrf_gn* g);
gmrf_status gmrf_gn_run(gmrf_gn* g, const double* q_nzval, int64_t q_stride, const double* qx_prior, const double* x_prior,
                        double* x, const double* y, double noise, double rtol, int32_t max_steps, int32_t* steps_out,
                        double* obj_hist_out, int32_t* info);
gmrf_status gmrf_gn_finalize(gmrf_gn* g, int32_t* info);
/* The posterior stage of the data-set loops on the final iterate (x_final of solve_burgers_gmrf-fem.jl:184-208, collocation
 * :248-263, the final GMRF of _research/elliptic_chen24.jl) for the batch of the last gmrf_gn_run (GMRF_ERR_NO_FACTOR without
 * one, as gmrf_gn_finalize), every tangent the driver serves.  One call, on the handle's stream:
 *     what gmrf_gn_finalize does (tangent at x, A = Q + noise J'J with the run's noise, gmrf_bt_refactor_values) ->
 *     k_samples samples x_p + L_p^-T z (gmrf_bt_sample with the iterate as the mean, the sample ids of a batch: problem p, sample
 *     s = p k_samples + s; k_samples in [0, 128]) ->
 *     variances (var_method -1: none; GMRF_VAR_EXACT; GMRF_VAR_RBMC / GMRF_VAR_MC with k_var samples, problem p drawing the ids
 *     p k_var .. p k_var + k_var - 1 like gmrf_bt_marginal_var_batch, on the values of A just assembled; the stage capped by
 *     GMRF_VAR_STAGE_MB as in gmrf_dc_run) -> std = sqrt(var) and |std_p|_2 ->
 *     logdet_p (gmrf_bt_logdet_batch), sqmahal_p = (z_p - x_p)' A_p (z_p - x_p) (gmrf_assemble_quadform_batch on the values of A),
 *     nll_p = 0.5 * ((n * log(2 pi) + sqmahal_p) - logdet_p), each operation rounded on its own (:208-215, :262-263) ->
 *     errors_p = (rel_err, rmse, max_err) of x_p against z_p over the elements [first, n) (gmrf_field_errors_batch; first = ns skips
 *     the first slice as the scripts' [2:end, :] does).
 * Every step is the public call named, on the driver's device buffers: the results are bitwise those of the calls made one after
 * the other.  z [B][n]: the reference solution's dofs, host or device, or NULL -- then sqmahal_out, nll_out and errors_out must be
 * NULL (GMRF_ERR_BAD_SHAPE).  Outputs, each NULL (not wanted), host or device: samples_out [B][k_samples][n], std_out [B][n],
 * std_norm_out [B], logdet_out [B], sqmahal_out [B], nll_out [B], errors_out [B][3].  GMRF_ERR_NOT_SPD ends the call with `info`
 * as gmrf_bt_refactor_values sets it and leaves every output untouched.  The handle is left holding the factor, as after
 * gmrf_gn_finalize; a later gmrf_gn_run does not see that the stage ran. */
gmrf_status gmrf_gn_posterior(gmrf_gn* g, const double* z, int64_t first, int64_t k_samples, uint64_t sample_seed, int32_t var_method,
                              int64_t k_var, uint64_t var_seed, double* samples_out, double* std_out, double* std_norm_out,
                              double* logdet_out, double* sqmahal_out, double* nll_out, double* errors_out, int32_t* info);

/* The "Prior" and "Initial condition" stages of the Burgers data-set loop (solve_burgers_gmrf-fem.jl:154-179) for a batch, on
 * the handle and the analysis gmrf_gn_run uses afterwards.  The driver binds a handle (reference order; its batch B is the
 * number of problems), an assembler whose Q pattern is the prior's (gmrf_burgers_prior_pattern) and that prior, all on ONE device
 * and ONE stream; anything else -- a twisted handle, a handle that analysed another pattern, another Q pattern -- is
 * GMRF_ERR_BAD_SHAPE, an assembler or prior created with device -1 GMRF_ERR_NO_DEVICE.  gmrf_bic_run: the handle must have
 * factored the assembler's pattern once (GMRF_ERR_NO_FACTOR before).  One call, on the handle's stream:
 *     ic [B][ns] -> bulk, Q_ic's values, Qx_prior -> Q_ic on the assembler's pattern (its J'J entries 0) -> Qx_prior registered with
 *     gmrf_bt_set_factor_rhs for the run (the caller's registration is put back) -> gmrf_bt_refactor_values -> x_ic = Q_ic^-1 Qx_prior
 *     (the backward sweep alone where the factorisation carried the forward one; GMRF_SW_NO_FACTOR_FWD switches that off).
 * x_ic [B][n] is mean(x_ic) of :172-179: prior mean and start point of gmrf_gn_run, with q_values_out as its q_nzval and qx_out
 * (= Q_ic x_ic) as its qx_prior.  ic, x_ic_out: host or device; q_values_out [B][nnz(Q)], qx_out [B][n], bulk_out [B]: NULL (not
 * wanted), host or device.  GMRF_ERR_NOT_SPD ends the call with `info` as gmrf_bt_refactor_values sets it and leaves the outputs
 * untouched.  The handle is left as any refactorisation leaves it: a later gmrf_gn_run does not see that the stage ran. */
typedef struct gmrf_bic gmrf_bic;
gmrf_status gmrf_bic_create(gmrf_handle* h, gmrf_assembler* as, gmrf_burgers_prior* prior, gmrf_bic** out);
gmrf_status gmrf_bic_destroy(gmrf_bic* g);
gmrf_status gmrf_bic_run(gmrf_bic* g, const double* ic, double* x_ic_out, double* q_values_out, double* qx_out, double* bulk_out,
                         int32_t* info);

/* Error metrics of a batch of fields against their truths (src/metrics.jl:3-13) over the elements [first, n) of every problem:
 * out [batch][3] = (rel_err, rmse, max_err) = (|d|_2 / |soln|_2, sqrt(mean(d^2)), max |d|) with d = pred - soln; first = ns skips
 * the first time slice as the scripts' [2:end, :] does.  pred, soln [batch][n], out: host or device; stream NULL: one of the
 * call's own.  Fixed-shape sums without atomics: the same bits on every call and in every batch.  A zero soln gives inf / nan. */
gmrf_status gmrf_field_errors_batch(int32_t device, void* stream, int64_t batch, int64_t n, int64_t first, const double* pred,
                                    const double* soln, double* out);

/* FEM fields at the points of a data grid: E = evaluation_matrix(disc, pred_coords) of the data-set loops
 * (scripts/darcy/solve_darcy_gmrf-fem.jl:82-89, scripts/burgers/solve_burgers_gmrf-fem.jl:75-83; A_ic of :114-115 is the same operator at
 * the initial condition's coordinates), pred = E f on the device, and the metrics of pred against a truth in the same pass.
 * The rows of E are computed once at creation, on the host, in double precision; points / xy are HOST arrays in any order
 * (duplicates, several points in a cell and cells without a point are fine).  device -1: a handle for gmrf_eval_rows only.
 *   Line (the meshes of gmrf_burgers_line_create): nc cells of h = length / nc, order 1 or 2, bc GMRF_BURGERS_PERIODIC (ns = order nc
 *     dofs, points in [0, length)) or GMRF_BURGERS_DIRICHLET (ns = order nc + 1, points in [0, length]), dofs numbered by position.
 *     e = min(floor(x / h), nc - 1), xi = 2 (x - e h) / h - 1 clamped to [-1, 1].  Order 1: ((1 - xi) / 2, (1 + xi) / 2) on the dofs
 *     (e, (e + 1) mod ns); order 2: (xi (xi - 1) / 2, xi (xi + 1) / 2, 1 - xi^2) on (2e, (2e + 2) mod ns, 2e + 1), the shape functions
 *     of gmrf_burgers_colloc_create.
 *   Triangles (the meshes of gmrf_darcy_p1_create / _p2_create, the elliptic and the shallow-water handles): nx x ny vertices on the
 *     unit square, x fastest, quads cut by the diagonal n00 - n11; points in [0, 1]^2 as xy [npts][2].  hx = 1 / (nx - 1),
 *     qx = min(floor(x / hx), nx - 2), s = (x - qx hx) / hx clamped to [0, 1]; qy and t likewise.  t <= s: the lower triangle
 *     (n00, n10, n11) with barycentrics (1 - s, s - t, t); otherwise the upper one (n00, n11, n01) with (1 - t, s, t - s).  Order 1:
 *     the barycentrics on the vertices i + nx j.  Order 2 (dofs: the (2 nx - 1) x (2 ny - 1) lattice, x fastest): l (2 l - 1) at the
 *     lattice point 2 V of vertex V and 4 la lb at Va + Vb of the edge between Va and Vb.
 * A row holds width = 2, 3, 3 or 6 entries in ASCENDING dof index; a weight that is exactly 0.0 (a point on a vertex or an edge) is
 * stored.  gmrf_eval_rows: ns, width, idx [npts][width] (0-based) and w [npts][width], each NULL (not wanted) or HOST memory.
 * GMRF_ERR_BAD_SHAPE for another order or bc, length <= 0, nc < 3 (periodic) / < 2 (dirichlet), nx or ny < 2, npts < 1, and for a
 * point that is not finite or outside the domain -- gmrf_last_error names its index.  Upper limits (32-bit dof indices on the
 * device): nc <= 2^24, nx, ny <= 16384, npts <= 2^28.
 * gmrf_eval_apply_batch: pred_out [rows][npts] = E fields [rows][ns], rows in [1, 2^24] spatial fields (means, samples, or the
 * slices of space-time fields: spatial_to_spatiotemporal without the nt times larger matrix).  ONE rounding sequence,
 *     pred = w0 f[idx0], then pred = fma(wk, f[idxk], pred) for k = 1 .. width - 1 in the stored order,
 * so a result is the same bits in every batch, for every `rows` and on every call.
 * gmrf_eval_errors_batch: fields [batch][nt][ns] against truth [batch][nt][npts] -> errors_out [batch][3] = (rel_err, rmse, max_err)
 * over the slices [first_slice, nt) (first_slice = 1: the scripts' [2:end, :]), bitwise what gmrf_eval_apply_batch followed by
 * gmrf_field_errors_batch(batch, n = nt npts, first = first_slice npts) gives; pred_out NULL or [batch][nt][npts], the bits of
 * gmrf_eval_apply_batch -- without it nothing of that size is written.  batch in [1, 4096], nt >= 1, 0 <= first_slice < nt,
 * nt npts < 2^31.  fields, truth, pred_out, errors_out: host or device.  Both calls run on the handle's stream and synchronise
 * before they return; GMRF_ERR_NO_DEVICE on a device -1 handle. */
typedef struct gmrf_eval gmrf_eval;
gmrf_status gmrf_eval_line_create(int32_t device, void* stream, int64_t nc, int32_t order, int32_t bc, double length, int64_t npts,
                                  const double* points, gmrf_eval** out);
gmrf_status gmrf_eval_tri_create(int32_t device, void* stream, int64_t nx, int64_t ny, int32_t order, int64_t npts, const double* xy,
                                 gmrf_eval** out);
gmrf_status gmrf_eval_destroy(gmrf_eval* e);
gmrf_status gmrf_eval_rows(const gmrf_eval* e, int64_t* ns_out, int64_t* width_out, int64_t* idx, double* w);
gmrf_status gmrf_eval_apply_batch(gmrf_eval* e, int64_t rows, const double* fields, double* pred_out);
gmrf_status gmrf_eval_errors_batch(gmrf_eval* e, int64_t batch, int64_t nt, int64_t first_slice, const double* fields,
                                   const double* truth, double* errors_out, double* pred_out);

/* Pointwise predictive variance and calibration at the points: var = diag(E Sigma E^T) with Sigma = A^-1 of a factored handle,
 * exactly (no sampling).  Row c of E has width dofs i_0 < ... < i_{width-1} of one element, so
 *     v_c = sum_ab w_a w_b Sigma[i_a, i_b]
 * over width (width + 1) / 2 distinct entries of Sigma, which gmrf_bt_selinv gives on the device.
 * gmrf_eval_pairs (works on a device -1 handle): the pair table, built at creation.  P is the ns x ns pattern -- symmetric, both
 *   triangles stored, sorted CSR -- of exactly the dof pairs some point uses, the diagonal of every dof used among them.  nnz_out,
 *   rowptr [ns + 1], colidx [nnz] (0-based) and pos [width (width + 1) / 2][npts] (32-bit), each NULL (not wanted) or HOST memory:
 *   pos[a (a + 1) / 2 + b][c], a >= b, is the place of the entry (i_a, i_b) of the lower triangle in P's CSR order.  The variance of
 *   a space-time field of nt slices needs Sigma on I_nt (x) P (slice t on the dofs t ns .. (t + 1) ns - 1), where that entry sits at
 *   t nnz(P) + pos.
 * gmrf_eval_var_batch: var_out [batch][nt][npts], host or device, for the batch of h, whose n must be nt ns.  The evaluator keeps one
 *   gmrf_csr of I_nt (x) P (rebuilt only when nt changes); the call runs h's selected-inverse path on it into h's own Sigma buffer --
 *   the plan is keyed by that matrix, so it holds across refactor_values -- and then ONE rounding sequence per (problem, slice, point):
 *       s_a = w_0 Sigma[a,0], then s_a = fma(w_b, Sigma[a,b], s_a) for b = 1 .. width - 1;
 *       v = w_0 s_0, then v = fma(w_a, s_a, v) for a = 1 .. width - 1,
 *   the same bits in every batch and on every call, no atomics.  |v - exact form of the Sigma read| <= (2 width + 2) eps
 *   sum_ab |w_a w_b Sigma_ab|; a variance that small against that sum can come out <= 0.
 * gmrf_eval_calibration_batch: fields [batch][nt][ns] (the prediction's dofs, e.g. the posterior means of the batch h factors)
 *   against truth [batch][nt][npts] under those variances -> out [batch][4] = (mean z^2, coverage, mean log predictive density,
 *   min variance) over the slices [first_slice, nt): z = (pred - truth) / sqrt(v), coverage the share of points with |z| <= zcrit
 *   (counted in integers), the density's term -(log(2 pi v) + z^2) / 2.  Fixed-shape sums on the partition of gmrf_eval_errors_batch:
 *   the same bits on every call.  pred_out / var_out: NULL or [batch][nt][npts], the bits of gmrf_eval_apply_batch /
 *   gmrf_eval_var_batch.  A point with v <= 0 makes the first three outputs inf or nan and shows in the fourth: look at it first.
 *   batch must be h's; zcrit >= 0; fields, truth, out, pred_out, var_out: host or device.
 * Errors: the selected inverse's own, with its message -- a twisted handle GMRF_ERR_BAD_SHAPE, no factor GMRF_ERR_NO_FACTOR, a pair
 *   across two blocks whose later index is not below rmax (or across more than neighbouring blocks) GMRF_ERR_BAD_SHAPE naming the
 *   entry -- and n != nt ns, nt npts or nt nnz(P) >= 2^31, another batch or a handle on another device: GMRF_ERR_BAD_SHAPE; a
 *   device -1 evaluator: GMRF_ERR_NO_DEVICE.  Both calls wait for h's stream, run on the evaluator's and synchronise before they
 *   return. */
gmrf_status gmrf_eval_pairs(const gmrf_eval* e, int64_t* nnz_out, int64_t* rowptr, int64_t* colidx, int32_t* pos);
gmrf_status gmrf_eval_var_batch(gmrf_eval* e, gmrf_handle* h, int64_t nt, double* var_out);
gmrf_status gmrf_eval_calibration_batch(gmrf_eval* e, gmrf_handle* h, int64_t batch, int64_t nt, int64_t first_slice, double zcrit,
                                        const double* fields, const double* truth, double* out, double* pred_out, double* var_out);

/* Tangent, residual and load of the nonlinear elliptic benchmark -Lap u + u^3 = f_src (FEM block assembly, fourth piece;
 * /root/reference/_research/elliptic_chen24.jl) as its Gauss-Newton loop evaluates them per iteration (f_and_J, :280-285):
 *     J(w) = J_static + J_cube(w),  J_static[i][j] = int grad(phi_i).grad(phi_j)   (assemble_J_diff_and_f, :179-228)
 *                                   J_cube[i][j]   = int 3 phi_i u_h^2 phi_j       (assemble_J_cube, :231-278)
 *     f(w) = J_static w + int phi_i u_h^3          b[i] = int phi_i f_src          (the load `fe` of :222)
 * on the structured P1 triangle mesh of the Darcy configs (nx x ny nodes, x fastest, quads cut by the diagonal n00 - n11; cell
 * numbering: all lower triangles, then all upper, as in the shallow-water handle) with the symmetric 3-point rule of order 2
 * (QuadratureRule{RefTriangle}(element_order + 1) of :122 for P1).  Prescribed dofs are the nodes on the four sides: their ROWS
 * are skipped and stay zero, columns are kept, no apply! is done (:210-212, :262-264).  f does not contain the load: b goes to
 * gmrf_gn_run as the observations y, obs_diff = y - f(x), which is the reference's J_static w + f_cube - f_static against zero
 * observations; the handle is stateless like the Burgers one.  The pattern is exactly gmrf_darcy_p1_pattern's for the same
 * nx, ny (explicit zeros included); the values come out in its CSR order, n = m = nx ny.  src_q [batch][cells][3]: the source at
 * the points of _qpoints (xy [cells][3][2] doubles in host memory).  w, vals_out, f_out, src_q, b_out: host or device pointers,
 * batch arrays problem-major with batch in [1, 4096]; problem p of a batch call gets the bits of the one-problem call on its
 * slice.  device -1: pattern and quadrature points only. */
typedef struct gmrf_elliptic_p1 gmrf_elliptic_p1;
gmrf_status gmrf_elliptic_p1_create(int32_t device, void* stream, int64_t nx, int64_t ny, gmrf_elliptic_p1** out);
gmrf_status gmrf_elliptic_p1_destroy(gmrf_elliptic_p1* e);
gmrf_status gmrf_elliptic_p1_pattern(const gmrf_elliptic_p1* e, int64_t* nnz_out, int64_t* rowptr, int64_t* colidx,
                                     int32_t index_base);
gmrf_status gmrf_elliptic_p1_qpoints(const gmrf_elliptic_p1* e, double* xy);
gmrf_status gmrf_elliptic_p1_tangent(gmrf_elliptic_p1* e, const double* w, double* vals_out, double* f_out);
gmrf_status gmrf_elliptic_p1_tangent_batch(gmrf_elliptic_p1* e, int64_t batch, const double* w, double* vals_out, double* f_out);
gmrf_status gmrf_elliptic_p1_load(gmrf_elliptic_p1* e, int64_t batch, const double* src_q, double* b_out);
/* The same tangent, residual and load with the reference's default element (element_order = 2 of gmrf_fem_solve, :118-122):
 * Lagrange{RefTriangle,2} under QuadratureRule{RefTriangle}(3).  Element, 4-point rule, lattice and local node order are those of
 * gmrf_darcy_p2_create (see its comment): dofs are the points of the (2 nx - 1) x (2 ny - 1) lattice, x fastest, n = m =
 * (2 nx - 1)(2 ny - 1), and the pattern is exactly gmrf_darcy_p2_create(nx, ny)'s (explicit zeros included).  Prescribed dofs are
 * the lattice points on the four sides.  The handle is the P1 type: _pattern / _qpoints / _tangent / _tangent_batch / _load /
 * _destroy and gmrf_gn_create_elliptic serve both orders, with xy [cells][4][2] and src_q [batch][cells][4] for this one
 * (cells = 2 (nx - 1)(ny - 1), numbered as for P1).  nx, ny <= 16384.  device -1: pattern and quadrature points only. */
gmrf_status gmrf_elliptic_p2_create(int32_t device, void* stream, int64_t nx, int64_t ny, gmrf_elliptic_p1** out);
/* The Gauss-Newton driver bound to the elliptic tangent (the loop of gmrf_fem_solve, :142-166): the same gmrf_gn type and the
 * same binding rules (one device, one stream, as->n == as->m == the tangent's n, as->nnz_j == the pattern's nnz; anything else is
 * GMRF_ERR_BAD_SHAPE); gmrf_gn_run / _finalize / _destroy serve both tangents.  The stop rule is the driver's relative
 * objective change, not the Newton decrement of :156-159. */
gmrf_status gmrf_gn_create_elliptic(gmrf_handle* h, gmrf_assembler* as, gmrf_elliptic_p1* e, gmrf_gn** out);

/* The Darcy data-set loop (scripts/darcy/solve_darcy_gmrf-fem.jl:176-198 per problem) for a batch of problems on one mesh.
 * gmrf_darcy_p1_assemble_batch: coeff_tables [batch][ng][ng] -> vals_out [batch][nnz], f_out [batch][n]; problem p gets the bits
 * of gmrf_darcy_p1_assemble on its table (both element orders); host or device pointers; batch in [1, 4096]. */
gmrf_status gmrf_darcy_p1_assemble_batch(gmrf_darcy_p1* d, int64_t batch, const double* coeff_tables, int64_t ng, double beta,
                                         double* vals_out, double* f_out);
/* The driver binds a handle (reference order; its batch B is the number of problems), an assembler whose J is the Darcy
 * assembler's pattern, and that Darcy assembler, all on ONE device and ONE stream (create the three with the same stream argument);
 * anything else -- a twisted handle, a handle that analysed another pattern -- is GMRF_ERR_BAD_SHAPE, an assembler created with
 * device -1 GMRF_ERR_NO_DEVICE.  gmrf_dc_run: the handle must have factored the assembler's pattern once (GMRF_ERR_NO_FACTOR
 * before).  One call, on the handle's stream:
 *     tables -> A, y (the element kernels) -> Q + q_eps A'A -> information vector q_mu + q_eps A'y, registered with
 *     gmrf_bt_set_factor_rhs for the run (the caller's registration is put back) -> gmrf_bt_refactor_values ->
 *     gmrf_bt_posterior (mean, k_samples samples with the sample ids of a batch: problem p, sample s = p k_samples + s) ->
 *     variances (var_method -1: none; GMRF_VAR_EXACT; GMRF_VAR_RBMC / GMRF_VAR_MC with k_var samples, problem p drawing the ids
 *     p k_var .. p k_var + k_var - 1 like gmrf_bt_marginal_var_batch, on the posterior values just assembled) ->
 *     std = sqrt(var) and |std_p|_2 (a fixed-shape sum without atomics: the same bits in every batch).
 * q_nzval: the prior's values, q_stride 0 = shared, nnz(Q) = per problem; q_mu [B][n] = Q mu or NULL (zero prior mean).
 * coeff_tables, q_nzval, q_mu: host or device.  Outputs, each NULL (not wanted), host or device: mean_out [B][n], samples_out
 * [B][k_samples][n] (k_samples in [0, 128]), std_out [B][n], std_norm_out [B].  GMRF_ERR_NOT_SPD ends the call with `info` as
 * gmrf_bt_refactor_values sets it and leaves the outputs untouched.  The stage of the sampled estimators is capped
 * (GMRF_VAR_STAGE_MB, default 512): the problems go through it in groups. */
typedef struct gmrf_dc gmrf_dc;
gmrf_status gmrf_dc_create(gmrf_handle* h, gmrf_assembler* as, gmrf_darcy_p1* d, gmrf_dc** out);
gmrf_status gmrf_dc_destroy(gmrf_dc* g);
gmrf_status gmrf_dc_run(gmrf_dc* g, const double* coeff_tables, int64_t ng, double beta, const double* q_nzval, int64_t q_stride,
                        const double* q_mu, double q_eps, int64_t k_samples, uint64_t sample_seed, int32_t var_method, int64_t k_var,
                        uint64_t var_seed, double* mean_out, double* samples_out, double* std_out, double* std_norm_out,
                        int32_t* info);

/* Linear shallow-water SPDE (FEM block assembly, third piece): the element loops of `assemble_system!`,
 * /root/reference/src/spdes/shallow_water.jl:17-122 -- coupling matrix K (h-u, h-v: -H grad(phi_i) phi_j; u-h, v-h:
 * -g grad(phi_i) phi_j; u-u, v-v: k phi_i phi_j; u-v / v-u: -+ f phi_i phi_j), element-lumped mass M (`lump_matrix`, :116),
 * stiffness S, `apply!` of the constraint handler to all three (:119-121) -- and the per-step operators `discretize` forms
 * from them (:170-217), on the structured P1 triangle mesh of the Darcy configs (nx x ny nodes, x fastest, quads cut by the
 * diagonal n00 - n11; cell numbering: all lower triangles (n00, n10, n11), then all upper (n00, n11, n01)) with
 *   dof = 3 * node + field, fields (h, u, v) = (0, 1, 2)        (Ferrite numbers dofs in cell-visit order: a permutation)
 *   the symmetric 3-point quadrature rule of order 2; H enters through H_q[cell][q] = H(x_q), x_q from _qpoints.
 * pattern 0: K, 3 nn rows with the full field coupling over the 7-point node stencil (create_sparsity_pattern(dh, ch),
 * :140; explicit zeros kept); pattern 1: S (and M~ / the Matern factor), block-diagonal coupling (:141-150).  M is lumped and
 * comes back as a vector.  prescribed: 3 nn bytes (non-zero = dof of the constraint handler) or NULL.
 * _operators, for one time step dt: G_vals = (M~ + dt K) with the constraints applied (K's pattern, :212-217), J_vals =
 * sqrt(ratio) M~^-1/2 (kappa^2 M~ + G) in S's pattern -- the transposed square root of the initial precision, Q_matern = J'J
 * (:178-189; feed J to gmrf_assemble_precision with a zero Q), M_tilde (:172-174), beta(dt) = sqrt(dt) tau (1e-2 on prescribed
 * dofs, :198-211).  Values: host or device pointers; device -1: patterns and quadrature points only. */
typedef struct gmrf_swe_p1 gmrf_swe_p1;
gmrf_status gmrf_shallow_water_p1_create(int32_t device, void* stream, int64_t nx, int64_t ny, gmrf_swe_p1** out);
gmrf_status gmrf_shallow_water_p1_destroy(gmrf_swe_p1* w);
gmrf_status gmrf_shallow_water_p1_pattern(const gmrf_swe_p1* w, int32_t which, int64_t* nnz_out, int64_t* rowptr, int64_t* colidx,
                                          int32_t index_base);
gmrf_status gmrf_shallow_water_p1_qpoints(const gmrf_swe_p1* w, double* xy);   /* xy: [cells][3][2] doubles in host memory */
gmrf_status gmrf_shallow_water_p1_assemble(gmrf_swe_p1* w, const double* H_q, double k, double f, double g, const uint8_t* prescribed,
                                           double* K_vals, double* M_lumped, double* S_vals);
gmrf_status gmrf_shallow_water_p1_operators(gmrf_swe_p1* w, const double* K_vals, const double* M_lumped, const double* S_vals,
                                            const uint8_t* prescribed, double kappa_matern, double tau, double dt, double* G_vals,
                                            double* J_vals, double* M_tilde, double* beta);

/* ------------------------------------------------------------------ test hooks
 * Direct access to the dense device kernels for the parity tests (row-major operands on
 * the HOST; not part of the drop-in surface). */
/* gmrf_test_gemm tri_flags: 2048 the 128 x 128 kernel, 4096 the 32 x 32 one, 8192 / 16384 / 32768 the LDS-DMA kernel with
 * 64 x 64 / 128 x 64 / 64 x 128 tiles; 65536 the 64 x 64 LDS-DMA kernel with the tail row (A and C hold M + 1 rows, row M is
 * summed on the VALU from the staged B tile; transA = transB = 0). */
gmrf_status gmrf_test_gemm(int32_t device, int64_t M, int64_t N, int64_t K, int32_t transA,
                           int32_t transB, int32_t tri_flags, int32_t lower_only,
                           double alpha, const double* A, int64_t lda, const double* B,
                           int64_t ldb, double beta, double* C, int64_t ldc);
/* Two products of `batch` problems each on the 64 x 64 LDS-DMA kernel (host arrays, contiguous per problem: A [M][K], B [K][N] if b_n
 * else [N][K], C [M][N], in and out): grouped != 0 as ONE launch of gemm_f64_dma_grouped, else as two launches.  desc: M, N, K, b_n,
 * tri, lower_only of product 0, then of product 1; ab: alpha_0, beta_0, alpha_1, beta_1. */
gmrf_status gmrf_test_gemm_pair(int32_t device, int32_t batch, int32_t grouped, const int64_t* desc, const double* ab,
                                const double* A0, const double* B0, double* C0, const double* A1, const double* B1, double* C1);
/* One launch of a general GEMM descriptor on one chosen route; host buffers with their element counts, copied whole both ways
 * (any of D, tA, tC, tD, the K bounds and samples / mean may be null).  desc (28 x int64): M, N, K, transA, b_n, tri, lower_only,
 * batch, nb1, lda, ldb, ldc, ldd, strideA, strideB, strideC, pA, pB, pC, pD, ptA, ptC, ptD, o_j0, o_n, o_cols, o_ld, o_k; abt: alpha,
 * beta, tbeta.  route: 0 register-staged 64 x 64, 1 128 x 128, 2 32 x 32, 3 / 4 / 5 LDS-DMA 64 x 64 / 128 x 64 / 64 x 128, 6 tail row
 * (row M of A / C / D unless tC is given; with the direct output if samples is given), 7 the launcher's own choice.  *family: 1 / 2
 * register-staged at BK 16 / 32 (+ 256 single stage), 3 128 x 128, 4 32 x 32, 5 / 6 / 7 LDS-DMA by tile shape, 8 tail row, 9 tail row
 * with direct output.  Buffers too small for the descriptor, or a forced route it does not qualify for: GMRF_ERR_BAD_SHAPE, nothing
 * launched. */
gmrf_status gmrf_test_gemm_desc(int32_t device, int32_t route, const int64_t* desc, const double* abt,
                                const double* A, int64_t nA, const double* B, int64_t nB, double* C, int64_t nC,
                                const double* D, int64_t nD, const double* tA, int64_t ntA, double* tC, int64_t ntC,
                                const double* tD, int64_t ntD, const int32_t* kb_m, int64_t n_kb_m, const int32_t* kb_n,
                                int64_t n_kb_n, const int32_t* ke_n, int64_t n_ke_n, double* samples, int64_t n_samples,
                                double* mean, int64_t n_mean, int32_t* family);
/* gmrf_test_gemm_desc with GemmArgs::ke_m (an upper K bound per 64-row tile of A, the LDS-DMA kernels' only: routes 3 .. 6) and
 * without the direct output.  grouped = 1 / 2 (route 3): the descriptor runs as the first / second product of ONE launch of
 * gemm_f64_dma_grouped, beside a copy of itself that writes a buffer of its own. */
gmrf_status gmrf_test_gemm_env(int32_t device, int32_t route, const int64_t* desc, const double* abt,
                               const double* A, int64_t nA, const double* B, int64_t nB, double* C, int64_t nC,
                               const double* D, int64_t nD, const double* tA, int64_t ntA, double* tC, int64_t ntC,
                               const double* tD, int64_t ntD, const int32_t* kb_m, int64_t n_kb_m, const int32_t* kb_n,
                               int64_t n_kb_n, const int32_t* ke_n, int64_t n_ke_n, const int32_t* ke_m, int64_t n_ke_m,
                               int32_t grouped, int32_t* family);
/* gmrf_test_gemm_env with GemmArgs::strict_lower (0 / 1; 1 needs lower_only = 1 and M == N): nothing strictly above the element
 * diagonal is needed.  The 64 x 64 LDS-DMA launches (route 3, grouped or not, and the tail route 6) then leave, in every diagonal
 * tile, the six 16 x 16 blocks above its block diagonal (B stored [n][k]) or the quadrant rows 0 .. 31 x columns 32 .. 63 (B stored
 * [k][n]) as C held them; the other routes take the field and write whole tiles. */
gmrf_status gmrf_test_gemm_sym(int32_t device, int32_t route, const int64_t* desc, const double* abt,
                               const double* A, int64_t nA, const double* B, int64_t nB, double* C, int64_t nC,
                               const double* D, int64_t nD, const double* tA, int64_t ntA, double* tC, int64_t ntC,
                               const double* tD, int64_t ntD, const int32_t* kb_m, int64_t n_kb_m, const int32_t* kb_n,
                               int64_t n_kb_n, const int32_t* ke_n, int64_t n_ke_n, const int32_t* ke_m, int64_t n_ke_m,
                               int32_t grouped, int32_t strict_lower, int32_t* family);
/* Process-wide switch for comparisons: enabled = 0 makes every GEMM launcher drop the strict-lower mode (whole diagonal tiles),
 * 1 (the default) honours it.  It is read when a launch is issued, which for a handle is when its factor graph is CAPTURED: set
 * it before the handle's first factorisation (or use a fresh handle) -- a captured graph replays the launches it was taken with. */
gmrf_status gmrf_test_strict_lower(int32_t enabled);
/* The envelope bounds the symbolic phase derived per block and 64-row tile ([n_blocks][bsp / 64] each, in-block columns; blocks that
 * are a multiple of 256): lo = first column of D_i in the rows S = D_i - C C^T leaves untouched, rounded down to 64 (0 elsewhere),
 * hi = end of D_i's columns inside lo's 256-column panel, rounded up to 64 (the panel's end for a tile inside that panel, bsp
 * elsewhere).  *state: 0 none, 1 trivial for every panel (the launches of before), 2 in use.  *n_vals: values per array. */
gmrf_status gmrf_test_envelope(gmrf_handle* h, int32_t* lo, int32_t* hi, int64_t cap, int64_t* n_vals, int32_t* state);
/* Device-resident timing of one GEMM shape (random operands): batch problems, big = 1 takes the
 * 128 x 128 kernel, 0 the 64 x 64 one, 2 the launcher's own choice. */
gmrf_status gmrf_test_gemm_rate(int32_t device, int64_t M, int64_t N, int64_t K, int32_t transB,
                                int32_t tri_flags, int32_t lower_only, int32_t batch,
                                int32_t big, int32_t reps, double* ms_per_launch);
/* GEMM launches of the profiled steps of a handle by shape (gmrf_bt_set_profiling on): rows of 11 doubles = class, M, N, K,
 * tri flags, lower_only, problems, per-tile K bounds?, launches, ms (the dispatches' own time stamps), flops as booked. */
gmrf_status gmrf_test_gemm_shapes(gmrf_handle* h, double* rows, int64_t cap_rows, int64_t* n_rows);
gmrf_status gmrf_test_potrf_tile(int32_t device, double* tile64 /* in: SPD, out: L */,
                                 double* inv64, int32_t* info);
gmrf_status gmrf_test_tile_timing(double* out, int32_t n);
gmrf_status gmrf_test_potrf_block(int32_t device, int64_t bs, double* S /* in/out: L */,
                                  double* Linv, int32_t* info);
/* The in-block Cholesky (potrf_block) once, on the route a handle of this shape takes: one block per problem, `batch` problems,
 * gmrf_bt_set_eager(switches), gmrf_bt_set_keep_l(keep_l), a coupling window that starts at column cmin (a multiple of 64 in
 * [0, bs): what decides the split inverse).  bs = 64 * 2^p.  S, L, Linv: host, [batch][bs][bs] row-major; all three are uploaded
 * whole and L, Linv read back whole, so the caller sees what the kernels wrote and what they left.  *info: 0, or 1 + the index of a
 * problem with a non-positive pivot.  route[4]: the route (1 fused, 2 big one-problem, 3 256-column panels, 4 steps),
 * gmrf_stats.persist_route of the launches (0 none, 1 block, 2 panel, 3 diagonal block of a batch), the split p of the inverse
 * (0: full), and the number of persistent waits that gave up.  Bad arguments: GMRF_ERR_BAD_SHAPE, nothing launched.
 * tests/potrf_ref.py states the contract of the three buffers. */
gmrf_status gmrf_test_potrf_route(int32_t device, int64_t bs, int32_t batch, int32_t switches, int64_t cmin, int32_t keep_l,
                                  double* S, double* L, double* Linv, int32_t* info, int32_t* route);
/* s_memtime stamps of the chain workgroup of the last gmrf_test_potrf_block that took the persistent form
 * (csrc/potrf_persist.hpp): out[0] = tile 0 done, then eight per step (tools/persist_stamps.py names them); cycles relative to out[0], -1 = not written. */
gmrf_status gmrf_test_persist_stamps(double* out, int32_t n);
/* block ranges of this handle that were repeated with the launch-per-step form because a bounded wait inside a persistent
 * launch gave up (GMRF_PERSIST_SPIN_MS: default 2000 for one problem, 200 for batches); also in gmrf_stats.persist_aborts */
gmrf_status gmrf_test_persist_aborts(gmrf_handle* h, int32_t* n);
/* *state = 1 if the current factor holds y = L^-1 b for the registered b (gmrf_bt_set_factor_rhs), else 0; y_out (optional, host,
 * n x B column-major) then receives y */
gmrf_status gmrf_test_factor_fwd(gmrf_handle* h, int32_t* state, double* y_out);
/* the last gmrf_gn_run: iterations, and those whose solve took y = L^-1 rhs from the factorisation */
gmrf_status gmrf_test_gn_route(gmrf_gn* g, int32_t* iterations, int32_t* fwd_iterations);
/* the last gmrf_dc_run: 1 if its factorisation took y = L^-1 rhs along (the forward-in-factor route) */
gmrf_status gmrf_test_dc_route(gmrf_dc* g, int32_t* fwd_in_factor);
/* the last gmrf_bic_run: 1 if its factorisation took y = L^-1 Qx_prior along (the forward-in-factor route) */
gmrf_status gmrf_test_bic_route(gmrf_bic* g, int32_t* fwd_in_factor);
/* the last batched sampled estimator of the handle: problems per group of the stage, groups per chunk (GMRF_VAR_STAGE_MB) */
gmrf_status gmrf_test_var_groups(gmrf_handle* h, int32_t* group_size, int32_t* groups);
/* The per-device budget of CUs for persistent launches, host only (no GPU needed): `n` handles ask for demands[i] CUs one after
 * the other on a device of `cus` CUs; granted[i] = 1 if the claim fitted beside the earlier ones, 0 if it was refused (the
 * handle would take the launch-per-step routes up front instead of meeting a bounded wait). */
gmrf_status gmrf_test_persist_budget(int32_t cus, int32_t n, const int32_t* demands, int32_t* granted);
gmrf_status gmrf_test_mfma_f64_rate(int32_t device, double* tflops);
/* Shader clock under load: _start launches a bounded probe (8 waves stamping s_memtime / s_memrealtime every ~3.4 us x sleeps,
 * n samples) on a stream of its own and returns; run the load under test; _finish waits and returns n - 1 interval clocks in GHz
 * (median over the 8 waves) and the intervals' start times in ms. */
gmrf_status gmrf_test_clock_probe_start(int32_t device, int32_t n, int32_t sleeps, void** probe);
gmrf_status gmrf_test_clock_probe_finish(void* probe, double* ghz, double* t_ms);
gmrf_status gmrf_test_hbm_rate(int32_t device, int64_t bytes, double* gbps);
gmrf_status gmrf_test_microbench(int32_t device, double* out, int32_t n);
/* Host-only part of the symbolic phase of gmrf_bt_factor_csc (needs no device): driven by the sanitizer build of the host
 * side.  out8 = {cmin, rmax, entries, longest lower-block row, sparse route?, tile plan?, plan capacity, checksum}. */
gmrf_status gmrf_test_symbolic_csc(int64_t n, int64_t n_blocks, const int64_t* colptr, const int64_t* rowval,
                                   int32_t index_base, int64_t* out8);

/* The envelope bounds of a pattern, host only (no device): lo / hi as gmrf_test_envelope ([n_blocks][bsp / 64]; cap = what they can
 * hold) and units[n_blocks][bsp / 256][3] = 64-wide K units of each panel's product without / with a tail row riding and of its
 * rank-256 update.  *n_vals = n_blocks * bsp / 64 (0: blocks no multiple of 256). */
gmrf_status gmrf_test_envelope_csc(int64_t n, int64_t n_blocks, const int64_t* colptr, const int64_t* rowval, int32_t index_base,
                                   int32_t* lo, int32_t* hi, double* units, int64_t cap, int64_t* n_vals);

/* The sparse products' routes as values.  geom[8] = {k, ldx, ldy, X base 16-byte aligned?, Y base 16-byte aligned?, x_stride,
 * y_stride, padded plan withheld?} describes one node-major call (one problem: strides 0); node-major kinds: 0 csr_spmm_rows /
 * csr_spmm_rows_batch, 1 csr_spmm_tiles, 2 csr_spmm_tiles_pad, with NG gather loads per thread (7 or 10); column-major route at
 * the same k: 0 csr_spmv_tiles, else the lane group G of csr_spmm.
 * gmrf_test_spmm_plan: host only (no device), the tile plan of a CSR pattern and its routes.  out[12] = {plan state (1 usable, -1
 * none), R, ucap, ecap, ecap_pad, umax, tiles, listed distinct columns, node-major kind, NG, column-major route, every 64-row tile
 * within csr_spmv_tiles' capacity?}; tile_uptr[tiles + 1], ucols, lidx[nnz] are filled where all three are given and the two
 * capacities suffice.
 * gmrf_test_spmm_route: the same for a live matrix, the alignment flags taken from the addresses X and Y.  out[12] = {plan state,
 * R, ucap, ecap, ecap_pad, umax, node-major kind, NG, column-major route, and of the LAST products launched on S: node-major kind,
 * NG, column-major route (-1: none yet)}.
 * gmrf_test_spmm_rows_batch: the batched node-major product on explicit DEVICE pointers -- B problems on S's pattern with the fp64
 * values vals[B][nnz], operands X + p x_stride, Y + p y_stride; no_pad withholds the padded plan for this call, so the unpadded
 * tiled kernels run on a matrix whose padded image fits.  B = 1: the product with another problem's values.  Synchronises. */
gmrf_status gmrf_test_spmm_plan(int64_t n_rows, int64_t n_cols, const int64_t* rowptr, const int64_t* colidx, int32_t index_base,
                                const int64_t* geom, int64_t* out, int64_t* tile_uptr, int32_t* ucols, uint16_t* lidx,
                                int64_t cap_uptr, int64_t cap_ucols);
gmrf_status gmrf_test_spmm_route(const gmrf_csr* S, const int64_t* geom, const void* X, const void* Y, int64_t* out);
gmrf_status gmrf_test_spmm_rows_batch(const gmrf_csr* S, int64_t B, const double* vals, const double* X, int64_t ldx,
                                      int64_t x_stride, double* Y, int64_t ldy, int64_t y_stride, int64_t k, int32_t no_pad);

/* The block sweep products (csrc/sweep.hpp: out = [b -] Mat x or Mat^T x, the step of every forward and backward sweep) as values.
 * desc[17] = {trans, tri, kp, rows, kdim, nprob, narrow, kst set?, mend set?, ld, ldx, ldb, ldo, pMat, pXin, pBin, pOut}: the
 * arguments of sweep_route, then the leading dimensions of the block, the input, the addend and the output, then the per-problem
 * strides.  Kernel ids: 1 .. 4 sweep_mm<trans, tri> = <0,0>, <0,1>, <1,0>, <1,1>; 5 / 6 sweep_gemv_n<0 / 1>; 7 / 8
 * sweep_gemv_n_short; 9 / 10 sweep_gemv_n4; 11 / 12 sweep_gemv_t<0 / 1, 8>; 13 / 14 sweep_gemv_t<., 16>; 15 / 16 sweep_gemv_t<., 32>;
 * 0 = refused (the kernel cannot compute the shape; gmrf_last_error says why).
 * gmrf_test_sweep_route: host only (no device).  out[4] = {id, grid x, y, z} of the kernel launch_sweep takes.
 * gmrf_test_sweep_product: one product on host arrays.  Mat[nMat] and the panel P[nP] are uploaded whole and P is read back whole,
 * so the caller sees what was written and what was left.  Xin = P + x_off, Bin = P + b_off (b_off < 0: no addend; b_off == o_off:
 * in place), Out = P + o_off; kst / mend (or NULL): one entry per 64 rows.  force = 0: launch_sweep's own choice; force = id: that
 * kernel, if the shape meets its own preconditions.  *route_out = the id that ran.  GMRF_ERR_BAD_SHAPE with nothing uploaded or
 * launched: a refused route, an operand that does not fit its buffer, an odd ld / offset / stride under 16-byte loads, a kst / mend
 * entry that is odd, out of range or leaves a sweep_mm K range that is no multiple of 8, outputs that overlap inputs, each other or
 * another output's addend. */
gmrf_status gmrf_test_sweep_route(const int64_t* desc, int64_t* out);
gmrf_status gmrf_test_sweep_product(int32_t device, int32_t force, const int64_t* desc, const double* Mat, int64_t nMat, double* P,
                                    int64_t nP, int64_t x_off, int64_t b_off, int64_t o_off, const int32_t* kst, int64_t n_kst,
                                    const int32_t* mend, int64_t n_mend, int32_t* route_out);

/* The coupling step of block i > 0 of a factorisation (C_i = B_i Linv_{i-1}^T into the stored window of C, and whoever clears the
 * Schur block before S = D_i - C_i C_i^T) as a value.  route[10] = {kind (0 dense GEMM, 1 spmm_bxt, 2 spmm_bxt_tiles), KM of
 * spmm_bxt, cw, nch, ncg, ng, workgroups of the product's launch (0: the GEMM's own), Schur fill (0 nobody, 1 zero_rows, 2 the zero
 * role of spmm_bxt_tiles, 3 its scatter role), zwgs, skip_dead}.
 * gmrf_test_coupling_plan: host only (no device).  The plan of the symbolic phase for a CSC pattern with build_symbolic's
 * group_tiles flag (a handle passes batch >= 8): scal[12] = {cmin, rmax, most entries in a row of a lower block, sparse_b, bxt_ok,
 * ecap, nrt, and the lengths of kst, rowptr, gtiles, ucols, lidx}; the arrays (each may be NULL) are filled where cap[7] = the
 * capacities of {kst, rowptr, ng, gtiles, uptr, ucols, lidx} suffice: kst[bsp / 64] as the layout keeps it (monotone envelope,
 * relative to cmin), rowptr[N][bsp + 1], and of a usable plan ng[N], gtiles[N][nrt][3], uptr[N][nrt + 1], ucols, lidx[entries].
 * query (or NULL) = {batch, CUs of the device, block i, switches}: route[10] of that block.
 * gmrf_test_coupling_group_tiles: the next analysis of the handle plans with group_tiles = mode (0 / 1; -1: by its batch again).
 * gmrf_test_coupling_product: one coupling step of block i on a handle that gmrf_bt_factor_begin_csc has prepared (no step taken).
 * force = 0: the library's own route; 1 spmm_bxt, 2 spmm_bxt_tiles on the handle's plan, 3 the dense GEMM.  over[4] (or NULL), 0 =
 * own choice: {cw in 16 / 32 / 64, nch of the launcher's list, skip_dead 1 off / 2 on, Schur fill 1 nobody / 2 zero role / 3 scatter
 * role}.  X[batch][bsp bsp] is uploaded as Linv_{i-1} of every problem, C[nC] as the handle's whole image of the coupling blocks
 * (every problem, every block), S[batch][bsp bsp] as the Schur work block; C and S are read back whole.  One launch_coupling and
 * a synchronisation, nothing else.  GMRF_ERR_BAD_SHAPE with nothing uploaded or launched: a buffer of the wrong size; a forced
 * route or override the shape does not admit (tiles without a usable plan, spmm_bxt with rows of more than 32 entries, cw that does
 * not divide the window, nch above its 16-column chunks, the zero role without rows below rmax, the scatter role with a batch or
 * padded blocks). */
gmrf_status gmrf_test_coupling_plan(int64_t n, int64_t n_blocks, const int64_t* colptr, const int64_t* rowval, int32_t index_base,
                                    int32_t group_tiles, int64_t* scal, int32_t* kst, int32_t* rowptr, int32_t* ng, int32_t* gtiles,
                                    int32_t* uptr, int32_t* ucols, uint16_t* lidx, const int64_t* cap, const int64_t* query,
                                    int64_t* route);
gmrf_status gmrf_test_coupling_group_tiles(gmrf_handle* h, int32_t mode);
gmrf_status gmrf_test_coupling_product(gmrf_handle* h, int64_t i, int32_t force, const int32_t* over, const double* X, int64_t nX,
                                       double* C, int64_t nC, double* S, int64_t nS, int64_t* route_out);

#ifdef __cplusplus
}
#endif
#endif /* GMRF_HIP_H */
