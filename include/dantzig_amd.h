/*
 * dantzig_amd.h -- C ABI of the MI355X-native parametric self-dual simplex core.
 *
 * This is the drop-in boundary for the hot path of matteosantama/dantzig
 * (src/simplex.rs + src/linalg.rs).  The reference has no C ABI: its seam is the
 * PyO3 function `dantzig.rust.solve` (src/lib.rs:16-27) and, inside Rust, the pair
 * `Simplex::new(..)` / `Simplex::solve()` (src/simplex.rs:123, :332).  A Rust host
 * binds this header with a plain `extern "C"` block (INTEGRATION.md shows the stub);
 * the Python package binds it with ctypes.
 *
 * Conventions
 *   - plain pointers and sizes only; every buffer is caller-allocated host memory
 *     unless a parameter says "device"; the library never frees caller memory;
 *   - no exceptions or unwinding cross this boundary: every entry point returns a
 *     dzg_status (>= 0: solver outcome, < 0: call failed);
 *   - one solve per handle at a time (thread-compatible, not thread-safe);
 *   - all arithmetic is IEEE-754 binary64; indices are int64 at the boundary.
 *
 * Level 1 (dzg_solver_*, dzg_core_solve) takes the state `Simplex::new` leaves
 * behind and replaces `Simplex::solve`.  Level 2 (dzg_model_solve) also replaces
 * `Simplex::new` and `PySolution::from`, i.e. the whole of `dantzig.rust.solve`.
 * The dzg_kernel_* entry points expose single reference functions for parity tests.
 */
#ifndef DANTZIG_AMD_H
#define DANTZIG_AMD_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define DZG_ABI_VERSION 4

/* Outcome codes.  0..2 mirror the reference: Ok / Error::Unbounded / Error::Infeasible
 * (src/error.rs:3-7, src/simplex.rs:313,325).  The rest do not exist in the
 * reference, which recurses without a cap and panics instead. */
typedef enum {
    DZG_OPTIMAL = 0,
    DZG_UNBOUNDED = 1,
    DZG_INFEASIBLE = 2,
    DZG_ITER_LIMIT = 3,   /* stopped by max_iter / the run budget, state is resumable */
    DZG_SINGULAR = 4,     /* fast numerics: basis inverse lost accuracy                */
    DZG_PANIC = 5,        /* a reference panic path: safe_divide assert (src/simplex.rs:466),
                             "unexpected code path" (:304), zero-row LP (n-1 underflow) */
    DZG_RUNNING = 6,      /* internal: not terminated yet                              */
    DZG_NEAR_TIE = 7,     /* fast numerics, opts.near_tie_action = STOP: stopped BEFORE a pivot
                             whose choice (status(), find_first_pivot, find_second_pivot,
                             src/simplex.rs:274-306,423-461) is within rounding of a tie, so the
                             reference's arithmetic may choose differently.  The state is that
                             of the last executed pivot; dzg_solver_run resumes (that decision is
                             then taken as FAST sees it and counted in near_ties)         */
    DZG_NODE_LIMIT = 8,   /* dzg_mip_solve: node_limit node LPs solved with the search still open;
                             the incumbent, if there is one, is returned                  */
    DZG_E_DEVICE = -1,    /* HIP error, or no usable GPU (the product has no CPU path) */
    DZG_E_ARG = -2,       /* malformed input                                           */
    DZG_E_NOMEM = -3
} dzg_status;

typedef enum { DZG_STEP_PRIMAL = 0, DZG_STEP_DUAL = 1 } dzg_step_kind;

/* How dx = B^-1 a_j and v = B^-T e_p are obtained each iteration.
 *  STRICT: exactly the reference's arithmetic -- gather B, dense LU with partial
 *          pivoting of B and, separately, of B^T, forward/back substitution in the
 *          reference's operation order (src/linalg.rs:88-128,282-299), unfused.
 *          Bit-identical to the CPU restatement; O(m^3) per iteration.
 *  FAST:   the basis inverse is kept resident in HBM and updated per pivot; FTRAN is
 *          one GEMV, BTRAN one row read.  Same pivot rule; results agree with STRICT
 *          up to rounding (pivot choices differ only on near-ties).
 *  AUTO:   STRICT when m <= auto_strict_rows, else FAST. */
typedef enum { DZG_NUMERICS_STRICT = 0, DZG_NUMERICS_FAST = 1, DZG_NUMERICS_AUTO = 2 } dzg_numerics;

/* Pricing kernel choice for dz = -N^T v (src/linalg.rs:199-207). */
typedef enum {
    DZG_PRICE_AUTO = 0,
    DZG_PRICE_SEQ = 1,   /* one lane per column through an LDS-transposed tile: sums in the
                            reference's ascending-row order, bit-identical to neg_t_dot     */
    DZG_PRICE_WAVE = 2,  /* one wave per column, lane-strided partial sums + shuffle tree   */
    DZG_PRICE_TREE = 3   /* several columns per wave, register accumulators + shuffle tree: the
                            streaming kernel of FAST numerics; sums depend only on m, so dz is
                            bit-identical across column shardings (AUTO picks it for FAST and
                            DZG_PRICE_SEQ for STRICT)                                         */
} dzg_price_kernel;

/* The LP in the state `Simplex::new` produces (src/simplex.rs:209-223):
 *      maximise  c.x + constant   subject to   [A_struct | slacks] x = rhs,  x >= 0
 * Variables are numbered 0..n-1 in the reference's first-appearance order
 * (src/simplex.rs:168-176).  Structural columns are stored dense column-major; slack
 * columns are unit vectors and are never stored. */
typedef struct {
    int64_t m;               /* rows                                                    */
    int64_t n;               /* all variables, structural + slack                       */
    int64_t n_struct;        /* structural columns held in `a`                          */
    const double *a;         /* column-major m x n_struct, leading dimension lda >= m   */
    int64_t lda;
    const int64_t *var_col;  /* n entries: >= 0 structural column of variable v;
                                < 0: v is the slack of row (-1 - var_col[v]).
                                NULL = benchmark convention: variable v <
                                n_struct is column v, variable n_struct + i is slack i */
    const double *c;         /* n objective coefficients (the core MAXIMISES)           */
    double constant;
    const int64_t *basis;    /* m   initial basic variable per position  (Simplex.b)    */
    const int64_t *nonbasis; /* n-m initial nonbasic variable per position (Simplex.n)  */
    const double *x;         /* m   initial x (= rhs)                                   */
    const double *z;         /* n-m initial z (= -c of the nonbasic variables)          */
    /* Sparse alternative to `a` (used when a == NULL): the structural block in CSC, exactly
     * the reference's CscMatrix (src/linalg.rs:161-168): rows ascending inside a column, no
     * explicit zeros.  Kept as CSC on the device (12 bytes per nonzero). */
    const int64_t *col_ptr;  /* n_struct + 1                                            */
    const int32_t *row_idx;  /* nnz                                                     */
    const double *val;       /* nnz                                                     */
    /* The perturbation vectors of the parametric method (Simplex.x_bar, Simplex.z_bar,
     * src/simplex.rs:84-112).  NULL = all ones, as Simplex::new sets them (src/simplex.rs:219-220).
     * Given together with a non-slack `basis`, its `x` and `z`, they RESUME a solve from the state
     * a dzg_result handed back (basis, nonbasis, x, xbar, z, zbar): the basis is factorised on the
     * device and the loop goes on where it stopped. */
    const double *xbar;      /* m    or NULL                                             */
    const double *zbar;      /* n-m  or NULL                                             */
} dzg_lp;

typedef struct {
    int32_t numerics;         /* dzg_numerics, default AUTO                             */
    int32_t price_kernel;     /* dzg_price_kernel, default AUTO                         */
    int32_t device;           /* HIP device ordinal, default 0                          */
    int32_t auto_strict_rows; /* AUTO threshold, default 192                            */
    int64_t max_iter;         /* default 10,000,000                                     */
    double epsilon;           /* optimality tolerance, default 1e-12 (src/simplex.rs:9) */
    int64_t log_capacity;     /* pivots kept in the device log, default min(max_iter, 2^22) */
    int32_t poll_interval;    /* FAST: iterations enqueued between host status polls, default 32 */
    int32_t profile;          /* bit mask, bit (1 << DZG_K_*) set: time that kernel class with
                                 HIP events (slower); 0 = no timing, -1 = every class.
                                 Bits 16..23: a sampling stride S > 1 -- only every S-th
                                 iteration of a batch is stamped (an event pair costs a few
                                 microseconds of idle GPU between two short kernels)     */
    /* Column sharding (one process per GPU).  This rank prices the structural columns
     * [col_begin, col_end); 0,0 = all.  See dzg_shard_* below. */
    int64_t col_begin, col_end;
    int32_t rank, world;
    void *stream;             /* hipStream_t to enqueue on; NULL = a private stream.  A host that
                                 interleaves its own collectives passes the stream they are
                                 ordered against (torch.cuda.current_stream().cuda_stream)     */
    int64_t refactor_interval; /* FAST: rebuild the basis inverse from scratch (blocked LU with
                                 partial pivoting, fp64-MFMA trailing updates) every this many
                                 pivots; 0 = never (the eta file is still folded in every 64)  */
    int32_t a_is_block;       /* column sharding, dense: 1 = lp->a holds ONLY this rank's columns
                                 [col_begin, col_end) (column col_begin first), so a rank never
                                 materialises the other ranks' part of the matrix; 0 = lp->a is
                                 the whole m x n_struct matrix and the block is taken from it   */
    int32_t near_tie_action;  /* FAST: dzg_near_tie_action, default COUNT                       */
    int32_t replicate_matrix; /* column sharding, dense: 1 = every rank keeps ALL structural columns in
                                 its HBM and only the PRICING is split by [col_begin, col_end): the
                                 entering column is read locally, so the exchange records shrink to
                                 their 64-byte headers, and a sharded solver can refactorise.  For
                                 matrices that fit one GPU (config 5: 17 GB of 288).  With a_is_block
                                 the other ranks' columns follow through dzg_solver_upload_columns.
                                 0 = partitioned: a rank holds its block only, columns travel in
                                 the records                                                     */
    int32_t auto_restart_rows; /* AUTO: largest LP (rows) that is re-solved in STRICT after FAST met a
                                 near tie / lost its footing; default DZG_AUTO_STRICT_RESTART_ROWS
                                 (2048: 57 ms per STRICT pivot); < 0: never re-solve            */
    double tie_tol;           /* FAST: a decision of the pivot rule is a "near tie" when winner and
                                 runner-up differ by less than max(tie_tol, 64 * max_pivot_error)
                                 relative, or rest on a denominator that is zero up to that
                                 tolerance.  Default 1e-11; < 0 switches the detector off       */
    int32_t seven_launches;   /* FAST, dense matrix resident on the device (one GPU, or a column-sharded
                                 rank with replicate_matrix): 0 (default) = an iteration is three
                                 launches (k_chain_pre, pricing, k_chain_post: device-wide barriers
                                 inside, csrc/k_chain.hip; sharded: the same two kernels between the
                                 exchanges); 1 = the seven launches a partitioned rank runs.  Same
                                 arithmetic, same pivots. */
    int32_t auto_strict_budget_s; /* AUTO: wall-clock seconds the STRICT re-solve may take (31-57 ms per
                                 pivot at 1024-2048 rows: an LP with tens of thousands of pivots
                                 would take an hour).  When it runs out the LP is solved in FAST
                                 numerics with near ties counted, and the result says so
                                 (near_ties > 0, numerics_used = FAST).  0 = default (600 s),
                                 < 0 = no limit */
    int32_t shard_rows;       /* column sharding, dense: 1 = the BASIS SIDE is sharded too -- rank r owns
                                 the rows [r S, (r+1) S), S = ceil4(ceil(m / world)), of x, xbar, dx, of
                                 the compact inverse Binv0 and of the eta columns U; FTRAN, the x-side
                                 ratio test, the eta flush and the update touch a rank's own rows only
                                 (8 m k / world bytes per FTRAN instead of 8 m k on every rank).  Row p of
                                 the inverse (BTRAN) lives on one rank: every x-side candidate travels
                                 with its row in the exchange records (layout below), still two exchanges
                                 per iteration.  x / xbar are complete on every rank whenever
                                 dzg_shard_run / dzg_shard_run_lockstep return.  FAST numerics, pricing
                                 AUTO or TREE.  0 (default): the basis side is replicated on every rank */
    int32_t reserved0;
} dzg_opts;

/* What FAST numerics does at a near tie (the pivot rule is a first-wins strict argmax,
 * src/simplex.rs:432-435,456-459: inside rounding distance of a tie, FAST's rounding and the
 * reference's can disagree, and only the reference's own arithmetic -- STRICT, from the first
 * pivot -- can say which way the reference goes). */
typedef enum {
    DZG_NEAR_TIE_COUNT = 0,   /* carry on; count such pivots in dzg_result.near_ties             */
    DZG_NEAR_TIE_STOP = 1     /* stop with DZG_NEAR_TIE before the pivot is executed             */
} dzg_near_tie_action;

typedef struct {
    int32_t kind;       /* dzg_step_kind           */
    int32_t reserved;
    int64_t entering;   /* variable index j        */
    int64_t leaving;    /* variable index i        */
    double mu;
} dzg_pivot;

/* Kernel classes for the time/byte counters. */
enum {
    DZG_K_STATUS = 0, DZG_K_FTRAN, DZG_K_RATIO, DZG_K_BTRAN, DZG_K_PRICE, DZG_K_UPDATE,
    DZG_K_BASIS_UPDATE, DZG_K_LU,
    /* column-sharded loop (dzg_shard_run): the two all-gathers, from the moment the stream
     * reaches them to their completion (so waiting for a slower rank is counted here).  In that
     * loop STATUS = proposing the first-pivot candidate, FTRAN = the basis kernels before
     * pricing, RATIO = proposing the second record, UPDATE = everything after exchange 2. */
    DZG_K_XCHG1, DZG_K_XCHG2,
    DZG_K_COUNT
};
/* Mirrors of dzg_result in other languages write this number out (the Rust
 * `[c_double; DZG_K_COUNT]`, dantzig_amd/_ffi.py): adding a class is an ABI change. */
#ifdef __cplusplus
static_assert(DZG_K_COUNT == 10, "dzg_result.kernel_ms / kernel_launches have 10 entries");
#else
_Static_assert(DZG_K_COUNT == 10, "dzg_result.kernel_ms / kernel_launches have 10 entries");
#endif

typedef struct {
    int32_t status;          /* dzg_status                                              */
    int32_t numerics_used;   /* STRICT or FAST                                          */
    int64_t iterations;      /* executed pivots                                         */
    double objective;        /* constant + sum c[basis[p]] * x[p]  (src/simplex.rs:345-352) */
    /* optional outputs: NULL = not wanted */
    int64_t *basis;          /* m                                                       */
    int64_t *nonbasis;       /* n-m                                                     */
    double *x, *xbar;        /* m                                                       */
    double *z, *zbar;        /* n-m                                                     */
    dzg_pivot *log;          /* log_cap entries, first min(iterations, log_cap) filled  */
    int64_t log_cap;
    /* counters, filled when opts.profile != 0 */
    double kernel_ms[DZG_K_COUNT];
    int64_t kernel_launches[DZG_K_COUNT];
    double price_bytes;      /* algorithmic bytes of the pricing kernel, summed */
    double solve_ms;         /* wall time inside dzg_solver_run, summed                  */
    double max_pivot_error;  /* FAST health monitor: max relative |dx_p + dz_r| over all pivots
                                (the pivot element computed by FTRAN vs by BTRAN + pricing)   */
    /* FAST near-tie arbitration: the pivot log is the reference's, decision by decision, up to
     * (not including) pivot `first_near_tie`; near_ties == 0 means the whole log is.            */
    int64_t near_ties;       /* executed pivots with a decision inside the tie tolerance        */
    int64_t first_near_tie;  /* iteration index of the first one, -1 if none                    */
    double min_margin;       /* smallest relative margin (winner - runner-up) of any decision   */
    double *margins;         /* optional, like `log`: per-pivot smallest margin, log_cap entries */
    /* FAST basis representation */
    int64_t dense_columns;   /* k: structural variables in the basis = dense columns of the inverse */
    int64_t refactors;       /* refactorisations performed so far                               */
    int64_t chain_fallbacks; /* three-launch iteration: device-wide barriers that failed (another
                                kernel held CUs or LDS of the device) and were recovered from by
                                running on without barriers; 0 on an undisturbed device            */
    int32_t price_pass_used; /* FAST, dense matrix: which pricing pass the executed pivots ran, a bit
                                mask: 1 = row-wise over the k + 1 rows v does not zero (k_price_rows),
                                2 = column-wise over every nonbasic column (k_price_tree / the kernel
                                opts.price_kernel names); 3 = both (k crossed the rule's threshold);
                                0 = no pivot executed, or STRICT / CSC input                       */
    int32_t price_rows_copy; /* 1: the row-major copy of the matrix the row-wise pass streams is
                                resident; 0: not kept -- an explicit price_kernel, CSC, STRICT,
                                DZG_PRICE_ROWS=0, or hipMalloc could not hold a second copy of the
                                matrix (the solve then prices column-wise throughout: same pivots,
                                more bytes early in the solve)                                     */
    double state_drift;      /* FAST: largest relative difference between the carried x, xbar, z, zbar and
                                their recomputation from the fresh inverse, measured at the last
                                refactorisation (0 if none): what the near-tie tolerance is widened
                                by (tau = max(tie_tol, 64 max_pivot_error, 4 state_drift))         */
} dzg_result;

typedef struct dzg_solver dzg_solver;

int dzg_abi_version(void);
const char *dzg_status_str(int status);
/* Last HIP / argument error message of the calling thread ("" if none). */
const char *dzg_last_error(void);
/* Number of visible HIP devices (0 if none): lets a host fail early and loudly. */
int dzg_device_count(void);
void dzg_opts_default(dzg_opts *opts);

/* ---- Level 1: replaces Simplex::solve (src/simplex.rs:332-343) -------------------- */

/* Validates the LP, uploads it to HBM and allocates the workspace.  Not timed by bench. */
int dzg_solver_create(const dzg_lp *lp, const dzg_opts *opts, dzg_solver **out);
/* Runs until Optimal / error or until `max_new_iters` more pivots were executed
 * (<= 0: no budget).  Returns the status; DZG_ITER_LIMIT means "budget spent, call again". */
int dzg_solver_run(dzg_solver *s, int64_t max_new_iters);
/* Copies state, pivot log and counters back to the host. */
int dzg_solver_result(dzg_solver *s, dzg_result *res);
void dzg_solver_destroy(dzg_solver *s);
/* opts.replicate_matrix with opts.a_is_block: hands over the structural columns
 * [col_begin, col_end) that the rank did not pass at creation (column col_begin first in `a`,
 * leading dimension lda >= m).  Every column must be present before the first run. */
int dzg_solver_upload_columns(dzg_solver *s, int64_t col_begin, int64_t col_end, const double *a,
                              int64_t lda);
/* FAST: rebuild the basis inverse from scratch now (needs opts.refactor_interval != 0 at
 * creation, which reserves the workspace). */
int dzg_solver_refactor(dzg_solver *s);
/* create + run + result + destroy.  With opts == NULL or numerics AUTO and more than
 * auto_strict_rows rows, FAST runs with near_tie_action = STOP.  Up to DZG_AUTO_STRICT_RESTART_ROWS
 * rows, a run that meets a near tie (or ends in DZG_SINGULAR / DZG_PANIC) is abandoned and the LP
 * is solved again from the first pivot with STRICT numerics -- the reference's arithmetic, the only
 * arbiter of a tie -- and that result is returned.  Above that size STRICT is out of reach
 * (seconds per pivot): FAST carries on and the result reports near_ties / first_near_tie, so the
 * caller knows from which pivot on the path is no longer certified to be the reference's. */
#define DZG_AUTO_STRICT_RESTART_ROWS 2048
int dzg_core_solve(const dzg_lp *lp, const dzg_opts *opts, dzg_result *res);

/* The same on the fields of the reference's `Simplex` exactly as Rust holds them
 * (src/simplex.rs:84-112), so that Simplex::solve (:332-343) becomes ONE call with no
 * reshaping on the Rust side:
 *   constraints: CscMatrix  ->  m = nrows, n = ncols, col_ptr[n+1], row_idx[nnz], val = data[nnz]
 *                               over ALL n columns, slack columns included (src/linalg.rs:161-168;
 *                               Vec<usize> is 64-bit on the reference's targets: pass .as_ptr())
 *   objective               ->  c = coefficients[n], constant
 *   b, n, x, z              ->  basis[m], nonbasis[n-m], x[m], z[n-m]   (x_bar = z_bar = 1, :203-204)
 * The library finds the unit slack columns itself (a column whose only stored entry is 1.0; one per
 * row, scanned from the last column down -- Simplex::new puts them last, :188-201) and keeps the
 * other columns dense or CSC on the device, whichever is smaller.  IN/OUT: on return (status >= 0)
 * basis / nonbasis / x / z hold the final state, as Simplex::solve leaves it in `self`; `res` is
 * filled like dzg_core_solve fills it (its optional buffers may be NULL).  Numerics: as
 * dzg_core_solve (opts == NULL: AUTO). */
int dzg_core_solve_full_csc(int64_t m, int64_t n, const int64_t *col_ptr, const int64_t *row_idx,
                            const double *val, const double *c, double constant, int64_t *basis,
                            int64_t *nonbasis, double *x, double *z, const dzg_opts *opts,
                            dzg_result *res);

/* ---- Level 2: replaces dantzig.rust.solve (src/lib.rs:16-27) ---------------------- */

/* A model as the PyO3 layer hands it over: objective AffExpr (maximised) and a list of
 * Inequality  coef.x <= b  over user variables with optional bounds
 * (src/pyobjs.rs:10-152).  Terms keep expression order: it defines column order and
 * therefore tie-breaks (src/simplex.rs:168-176). */
typedef struct {
    int64_t nvars;
    const int32_t *has_lb, *has_ub;  /* nvars */
    const double *lb, *ub;           /* nvars */
    int64_t obj_nterms;
    const int64_t *obj_var;          /* index into the variable table */
    const double *obj_coef;
    double obj_const;
    int64_t ncons;
    const int64_t *con_ptr;          /* ncons + 1 */
    const int64_t *con_var;
    const double *con_coef;
    const double *con_b;             /* ncons */
} dzg_model;

typedef struct {
    int32_t status;
    int32_t numerics_used;
    int64_t iterations;
    double objective;     /* PySolution.objective_value (core sense: maximised)         */
    double *values;       /* nvars: x+ - x- per user variable (src/simplex.rs:354-371)  */
    int64_t m, n;         /* size of the standard form that was solved                  */
    int64_t near_ties;    /* FAST on an LP too large for a STRICT re-solve: pivots decided inside
                             the tie tolerance (0: the path is the reference's), see dzg_result */
    int64_t first_near_tie;
} dzg_model_result;

int dzg_model_solve(const dzg_model *model, const dzg_opts *opts, dzg_model_result *res);

/* ---- Batches of small LPs: one workgroup per LP (csrc/k_batch.hip) ------------------ */

/* Largest LP (rows) the batched solver takes: its m x (m+1) factor buffer lives in LDS. */
#define DZG_BATCH_MAX_ROWS 128
/* Solves lps[0..count) in STRICT numerics, one workgroup per LP.  Dense `a` only, m <= 128;
 * var_col, constant, resume state (xbar / zbar) as in dzg_lp.  opts: max_iter (per LP), epsilon;
 * numerics STRICT or AUTO (= STRICT here); FAST is DZG_E_ARG.  pivots_per_launch 0 = default.
 * res[i] is filled like dzg_solver_result fills it (its optional buffers may be NULL, log / log_cap
 * per LP); res[i].status is LP i's outcome.  Returns 0 when every LP was processed, a negative
 * code (nothing run, dzg_last_error names the offending index) otherwise. */
int dzg_batch_solve(const dzg_lp *lps, int64_t count, const dzg_opts *opts,
                    int64_t pivots_per_launch, dzg_result *res);
/* The same as calling dzg_model_solve(&models[i], opts, &res[i]) for every i -- result for result,
 * bit for bit -- with every model that call would solve in STRICT on <= 128 dense rows solved in
 * one batch; the others go through dzg_model_solve one at a time. */
int dzg_model_solve_batch(const dzg_model *models, int64_t count, const dzg_opts *opts,
                          dzg_model_result *res);

/* ---- The same batches in FAST numerics (csrc/k_batch_fast.hip) ---------------------------- */

/* dzg_batch_solve's arguments and checks; one workgroup per LP keeps the explicit basis inverse in
 * LDS and follows the reference pivot for pivot, flagging every decision within rounding of a tie.
 * opts->numerics: FAST honours near_tie_action and tie_tol (max_iter, epsilon as dzg_batch_solve);
 * AUTO, and opts == NULL, runs FAST with near_tie_action = STOP, and every LP that ends
 * DZG_NEAR_TIE, DZG_SINGULAR or DZG_PANIC is solved again from its first pivot by dzg_batch_solve in
 * the same call (res[i].numerics_used says which numerics produced res[i]; auto_strict_rows is not
 * consulted); STRICT is dzg_batch_solve.  pivots_per_launch 0 = 128, refactor_every 0 = 64: the
 * inverse is rebuilt from the basis at the start of every launch and every refactor_every pivots
 * inside one (res[i].refactors counts the rebuilds of a basis that was not all slack); negative:
 * DZG_E_ARG.  res[i] also carries margins (optional, like log), max_pivot_error, near_ties,
 * first_near_tie and min_margin with dzg_solver_result's meaning; state_drift is not measured and
 * stays 0.  An LP's result does not depend on its place in the batch. */
int dzg_batch_solve_fast(const dzg_lp *lps, int64_t count, const dzg_opts *opts,
                         int64_t pivots_per_launch, int64_t refactor_every, dzg_result *res);
/* dzg_model_solve_batch's routing: the models that would share its STRICT batch share one
 * dzg_batch_solve_fast call with AUTO numerics; the others go through dzg_model_solve unchanged. */
int dzg_model_solve_batch_fast(const dzg_model *models, int64_t count, const dzg_opts *opts,
                               dzg_model_result *res);

/* ---- Dual values and reduced costs at the optimum (csrc/k_duals.hip) ------------------ */

/* In the core sense (maximise c.x + constant, [A | I] x = rhs, x >= 0), at an OPTIMAL basis B with
 * nonbasic set N:
 *   y = B^-T c_B                   the dual value of every row (m entries)
 *   d[j] = a_j . y - c[j]          the reduced cost of nonbasic variable j (for the slack of row i
 *                                  that is y[i]); exactly 0.0 for a basic variable (n entries)
 *   primal_obj                     the solver's objective
 *   dual_obj = constant + sum_i rhs0[i] * y[i]     (rhs0: the right-hand side of the rows.  That is
 *                                  the x the solve started with where every slack starts at the
 *                                  position of its own row; a solver handle started from any other
 *                                  basis forms rhs0 = B0 x0 when it is created.  The batch calls
 *                                  take the starting x as it is.)
 *   primal_infeas = max(0, -min x) over the carried x,   dual_infeas = max(0, -min_j d[j])
 *   z_diff = |z_carried - d_N|_inf / max(1, |d_N|_inf)
 * source DZG_DUALS_FRESH: y and d were recomputed on the device from the final basis -- STRICT: the
 * reference's LU::solve of B^T y = c_B and its neg_t_dot, bit for bit, dual_obj summed over ascending
 * rows; FAST: from a fresh refactorisation of the basis, deterministic, dual_obj summed in chunks.
 * source DZG_DUALS_CARRIED (CSC storage, column- or row-sharded solvers): no device work, y[i] is
 * the carried z of row i's slack where it is nonbasic and 0 otherwise, d the carried z by
 * variable, dual_obj follows from that y, z_diff = 0. */
#define DZG_DUALS_FRESH 1
#define DZG_DUALS_CARRIED 2
typedef struct {
    int32_t source;      /* DZG_DUALS_FRESH / DZG_DUALS_CARRIED; 0: none (the LP did not end OPTIMAL) */
    int32_t reserved;
    double *y;           /* m, optional: NULL = not wanted                                      */
    double *d;           /* n, optional                                                         */
    double primal_obj, dual_obj, primal_infeas, dual_infeas, z_diff;
} dzg_duals;

/* The solver's status must be DZG_OPTIMAL, else DZG_E_ARG.  A FAST solver (dense, one GPU)
 * refactorises its final basis for this, like dzg_solver_refactor (refactors and state_drift move
 * accordingly), and needs the workspace of opts.refactor_interval != 0, else DZG_E_ARG.  The carried
 * x, xbar, z, zbar, the basis, the objective and the pivot count are not touched; two calls on the
 * same state return the same bits. */
int dzg_solver_duals(dzg_solver *s, dzg_duals *out);
/* dzg_batch_solve, then k_duals_small over the LPs that ended OPTIMAL, in the same device
 * allocation; du[i].source = 0 for the others.  res[] is what dzg_batch_solve fills, bit for bit. */
int dzg_batch_solve_duals(const dzg_lp *lps, int64_t count, const dzg_opts *opts,
                          int64_t pivots_per_launch, dzg_result *res, dzg_duals *du);

/* The duals in terms of the user's model (still the core sense: the model is maximised, rows are
 * coef.x <= b):  con_dual[r] = y[r] of user row r;  ub_dual[u] / lb_dual[u] = y of the bound rows
 * Simplex::new appends after the user rows (ub before lb per variable, in order of first
 * appearance), 0 where the bound is absent;  var_rc[u] = c_u - sum_r a_{r,u} con_dual[r] over the
 * user rows in row order (c_u: the objective's coefficient, the last one if u is repeated). */
typedef struct {
    double *con_dual;                    /* ncons                                              */
    double *var_rc, *lb_dual, *ub_dual;  /* nvars, optional                                    */
    dzg_duals core;                      /* scalars and source; y / d optional, sized by res->m / res->n */
} dzg_model_duals;
/* dzg_model_solve / dzg_model_solve_batch with the duals of whichever solver produced the result
 * (res and the return value are exactly what those give); core.source = 0 unless the status is
 * DZG_OPTIMAL, and also when the duals of an OPTIMAL solve could not be computed (the final basis of
 * a FAST run did not refactorise: dzg_last_error says so) -- the solve's outcome stands. */
int dzg_model_solve_duals(const dzg_model *model, const dzg_opts *opts, dzg_model_result *res,
                          dzg_model_duals *du);
int dzg_model_solve_batch_duals(const dzg_model *models, int64_t count, const dzg_opts *opts,
                                dzg_model_result *res, dzg_model_duals *du);
/* Host only: fills con_dual and the optional var_rc / lb_dual / ub_dual of `out` from y[0..m), m the
 * rows of the model's standard form (DZG_E_ARG otherwise). */
int dzg_model_map_duals(const dzg_model *model, const double *y, int64_t m, dzg_model_duals *out);

/* ---- Sensitivity ranging at the optimum (csrc/k_ranging.hip) ---------------------------- */

/* How far the slopes of dzg_duals hold.  Core sense, at an OPTIMAL basis B with nonbasic set N; x is
 * the carried basic solution by position, d the FRESH reduced costs by variable, both clamped at
 * zero: xc_p = max(x_p, 0.0), dc_j = max(d_j, 0.0), so that 0 is inside every range.
 *   cost direction g (sparse over the n variables; the cost becomes c + t g):
 *     Y = B^-T g_B,  delta_k = a_j . Y - g_j  for the variable j at nonbasic position k
 *   right-hand-side direction h (sparse over the m rows; the right-hand side becomes rhs + t h):
 *     delta_p = (B^-1 h)_p  for basis position p
 *   a position is a candidate when |delta| > pivot_tol, with value r = -(clamped / delta): delta > 0
 *   gives r <= 0, a bound on lo; delta < 0 gives r >= 0, a bound on hi.  lo is the largest candidate
 *   for lo (-inf if none), hi the smallest for hi (+inf if none); ties go to the lowest position.
 *   *_var is the variable at the blocking position (the nonbasic one that would enter, the basic one
 *   that would leave), -1 if none.
 * For every t in [lo, hi] the basis stays optimal: the optimal value is objective + t (g . x) for a
 * cost direction and objective + t (y . h) for a right-hand-side direction.
 * Directions are in CSR form: direction i owns entries ptr[i] .. ptr[i+1]; the indices of one
 * direction are distinct and in range, else DZG_E_ARG.  pivot_tol: 0 selects 1e-9; negative or NaN
 * is DZG_E_ARG. */
typedef struct {
    int64_t ncost;
    const int64_t *cost_ptr;   /* ncost + 1                                   */
    const int64_t *cost_idx;   /* variables                                   */
    const double *cost_val;
    int64_t nrhs;
    const int64_t *rhs_ptr;    /* nrhs + 1                                    */
    const int64_t *rhs_idx;    /* rows                                        */
    const double *rhs_val;
    double pivot_tol;
} dzg_ranging_req;
typedef struct {               /* every pointer is optional: NULL = not wanted */
    double *cost_lo, *cost_hi;            /* ncost */
    int64_t *cost_lo_var, *cost_hi_var;   /* ncost */
    double *rhs_lo, *rhs_hi;              /* nrhs  */
    int64_t *rhs_lo_var, *rhs_hi_var;     /* nrhs  */
} dzg_ranging;

/* dzg_solver_duals first (same preconditions and side effects: status DZG_OPTIMAL, a FAST solver
 * refactorises its final basis and needs its refactorisation workspace), then the ranges of `req`;
 * `duals` (optional) is filled as dzg_solver_duals fills it.  STRICT: the reference's LU::solve per
 * direction, the batch's bits.  FAST (dense, one GPU): from the fresh inverse, cost directions as one
 * fp64-MFMA product per chunk of directions whose ratio test runs in the epilogue.  The carried
 * state is not touched; two calls on the same state return the same bits.  CSC storage and sharded
 * solvers: DZG_E_ARG, "ranging is not supported ..." -- a range cannot be read off the carried z. */
int dzg_solver_ranging(dzg_solver *s, const dzg_ranging_req *req, dzg_duals *duals, dzg_ranging *out);
/* dzg_batch_solve_duals, then one workgroup per (LP, direction) over the LPs that ended OPTIMAL.
 * req and rg hold `count` entries; res and du (optional) are what dzg_batch_solve_duals fills, bit
 * for bit.  An LP that did not end OPTIMAL gets NaN ranges and *_var = -1. */
int dzg_batch_solve_ranging(const dzg_lp *lps, int64_t count, const dzg_opts *opts,
                            int64_t pivots_per_launch, const dzg_ranging_req *req, dzg_result *res,
                            dzg_duals *du, dzg_ranging *rg);

/* Ranging in the user's terms.  Cost direction i moves the objective coefficient of user variable
 * var[i]: +1 on x+ and -1 on x- of the split Simplex::new makes.  Right-hand-side direction i is a
 * group of user rows with coefficients, CSR: rows row_idx[row_ptr[i] .. row_ptr[i+1]).  A variable
 * that appears nowhere in the model, an index out of range or repeated inside one group: DZG_E_ARG.
 * The results are in the core sense (the model is maximised, rows are coef.x <= b) and *_var are
 * variables of the standard form. */
typedef struct {
    int64_t nvar;
    const int64_t *var;        /* nvar user variables                         */
    int64_t nrow;
    const int64_t *row_ptr;    /* nrow + 1                                    */
    const int64_t *row_idx;    /* user rows                                   */
    const double *row_coef;
    double pivot_tol;
} dzg_model_ranging_req;
/* dzg_model_solve_duals / dzg_model_solve_batch_duals, then the ranges (rg->cost_* by requested
 * variable, rg->rhs_* by requested group).  NaN ranges unless the status is DZG_OPTIMAL and the
 * duals could be computed.  When dzg_solver_ranging itself fails after an OPTIMAL solve, the call
 * returns its code with its text in dzg_last_error: DZG_E_ARG for a route without ranging (CSC
 * storage), DZG_E_NOMEM, DZG_E_DEVICE (the final basis of a FAST run did not refactorise); res then
 * still holds the solve's outcome. */
int dzg_model_solve_ranging(const dzg_model *model, const dzg_opts *opts,
                            const dzg_model_ranging_req *req, dzg_model_result *res,
                            dzg_model_duals *du, dzg_ranging *rg);
int dzg_model_solve_batch_ranging(const dzg_model *models, int64_t count, const dzg_opts *opts,
                                  const dzg_model_ranging_req *req, dzg_model_result *res,
                                  dzg_model_duals *du, dzg_ranging *rg);

/* ---- Unboundedness and infeasibility rays (csrc/k_rays.hip) ------------------------------- */

/* What a solve that ended DZG_UNBOUNDED or DZG_INFEASIBLE can show for its verdict.  Core sense, the
 * state the solver stopped in (basis B, nonbasic set N, carried x, xbar, z, zbar; the failed pivot
 * was not executed), with find_first_pivot as the pivot rule has it.
 *   DZG_UNBOUNDED -> kind DZG_RAY_PRIMAL:  pos = find_first_pivot(z, zbar), var = j = N[pos],
 *     mu = -z[pos] / zbar[pos], dx = B^-1 a_j;  d[j] = 1, d[B[p]] = -dx[p], 0 for the other
 *     nonbasics, so that [A | I] d = 0;  value = c[j] - sum_p c[B[p]] dx[p] (p ascending, each
 *     product rounded, then subtracted);  violation = max_p max(dx[p], 0).  If d >= 0 and value > 0,
 *     every feasible point can move along d for ever and gains `value` per unit.
 *   DZG_INFEASIBLE -> kind DZG_RAY_FARKAS:  pos = find_first_pivot(x, xbar), var = i = B[pos],
 *     mu = -x[pos] / xbar[pos], y = B^-T e_pos, dz = -N^T y;  d[N[k]] = -dz[k], d[i] = 1, 0 for the
 *     other basics: d is the aggregated row y^T [A | I];  value = sum_i rhs0[i] y[i] (rows ascending,
 *     each product rounded);  violation = max_k max(dz[k], 0).  d . x = value for every solution of
 *     the equations, so d >= 0, x >= 0 and value < 0 cannot all hold.
 *   violation is NaN if the vector it is taken over holds a NaN.
 *   proven = violation == 0.0 and (value > 0 for PRIMAL, value < 0 for FARKAS): the sign conditions
 *   on the vectors as computed; the equalities hold to the accuracy of one solve.  The pivot rule is
 *   the reference's, quirks included: on degenerate data it can end UNBOUNDED or INFEASIBLE on an
 *   LP that is neither, and proven = 0 is how that shows. */
#define DZG_RAY_PRIMAL 1
#define DZG_RAY_FARKAS 2
typedef struct {
    int32_t kind;      /* 0: none (any other status, or a route without rays) */
    int32_t proven;
    int64_t var, pos;  /* j and its nonbasic position / i and its basis position */
    double mu, value, violation;
    double *d;         /* n, optional */
    double *y;         /* m, optional; FARKAS only, zeros for PRIMAL */
} dzg_ray;

/* The solver's status must be DZG_UNBOUNDED or DZG_INFEASIBLE, else DZG_E_ARG.  STRICT: the
 * reference's LU::solve and neg_t_dot, the batch's bits.  FAST (dense, one GPU): the final basis is
 * refactorised as for dzg_solver_duals (same workspace requirement, refactors and state_drift move
 * as they do there), dx / y come from the fresh inverse, dz from one pricing pass, value is summed in
 * fixed chunks.  The carried state, the status, the objective and the pivot count are not touched;
 * two calls on the same state return the same bits.  CSC storage and sharded solvers: DZG_E_ARG,
 * "rays are not supported ...". */
int dzg_solver_ray(dzg_solver *s, dzg_ray *out);
/* dzg_batch_solve (with `du`: dzg_batch_solve_duals), then k_rays_small over the LPs that ended
 * UNBOUNDED or INFEASIBLE, in the same device allocation; ry[i].kind = 0 for the others.  res and du
 * (optional) are what the existing calls fill, bit for bit. */
int dzg_batch_solve_rays(const dzg_lp *lps, int64_t count, const dzg_opts *opts,
                         int64_t pivots_per_launch, dzg_result *res, dzg_duals *du, dzg_ray *ry);

/* The ray in terms of the user's model (core sense: the model is maximised, rows are coef.x <= b).
 *   PRIMAL: var[u] = d[x+_u] - d[x-_u] (0 if u appears nowhere); con[r], ub[u], lb[u] = d of the
 *           slacks of user row r and of u's bound rows: how fast each row's slack grows along the ray.
 *   FARKAS: con[r], ub[u], lb[u] = y of those rows (the walk of dzg_model_map_duals): the
 *           multipliers of the contradiction;  var[u] = d[x+_u] - d[x-_u], the aggregated coefficient
 *           of u (zero for a proof).
 * ub / lb are 0 where the bound is absent. */
typedef struct {
    double *var;              /* nvars */
    double *con;              /* ncons */
    double *lb, *ub;          /* nvars */
    dzg_ray core;             /* scalars; d / y optional, sized by res->n / res->m */
} dzg_model_ray;
/* dzg_model_solve / dzg_model_solve_batch (with `du`: their _duals forms) with the ray of whichever
 * solver produced the result; res, du and the return value are exactly what those give.
 * core.kind = 0 unless the status is DZG_UNBOUNDED or DZG_INFEASIBLE, and also on a route without
 * rays (CSC storage) or when the final basis of a FAST run did not refactorise -- the solve's outcome
 * stands and dzg_last_error says why.  All four arrays are required (ncons / nvars > 0). */
int dzg_model_solve_rays(const dzg_model *model, const dzg_opts *opts, dzg_model_result *res,
                         dzg_model_duals *du, dzg_model_ray *ry);
int dzg_model_solve_batch_rays(const dzg_model *models, int64_t count, const dzg_opts *opts,
                               dzg_model_result *res, dzg_model_duals *du, dzg_model_ray *ry);
/* Host only: fills var / con / lb / ub of `out` from d[0..n) and y[0..m) (y may be NULL for
 * DZG_RAY_PRIMAL), m and n those of the model's standard form (DZG_E_ARG otherwise). */
int dzg_model_map_ray(const dzg_model *model, int32_t kind, const double *d, const double *y, int64_t m,
                      int64_t n, dzg_model_ray *out);

/* ---- Re-optimisation from the current basis after b or c change (csrc/k_restart.hip) -------- */

/* New data for the LP a live handle holds.  The matrix, var_col and the sizes stay. */
typedef struct {
    const double *rhs;     /* m, by constraint row; NULL = keep the current one      */
    const double *c;       /* n, by variable (core sense: maximised); NULL = keep    */
    double constant;       /* used when set_constant != 0                            */
    int32_t set_constant, reserved;
} dzg_reopt;

/* Changes rhs and / or c (and the constant) of the LP and recomputes the state of the CURRENT basis
 * B (nonbasic set N) for the new data; dzg_solver_run then carries on from that basis with the
 * parametric self-dual method, which starts from any basis once xbar = zbar = 1.
 *   Allowed: the solver's status is DZG_RUNNING (not run yet), DZG_OPTIMAL, DZG_UNBOUNDED,
 *   DZG_INFEASIBLE, DZG_ITER_LIMIT or DZG_NEAR_TIE -- in all of these the basis on the device is
 *   valid; a pivot that was pending at DZG_NEAR_TIE is dropped.  DZG_SINGULAR and DZG_PANIC: DZG_E_ARG.
 *   NULL `s` or `chg`, or both arrays NULL with set_constant == 0: DZG_E_ARG; a NaN or infinite entry:
 *   DZG_E_ARG, dzg_last_error names the index.  These checks run on the host before any device work.
 *   CSC storage, column- and row-sharded solvers: DZG_E_ARG, "reoptimize is not supported ...".
 *   A FAST solver needs its refactorisation workspace (opts.refactor_interval != 0 at creation), like
 *   dzg_solver_duals, else DZG_E_ARG.
 * The refactorisation of B comes first.  If B does not refactorise (a singular block) the status is
 * put back, nothing else has been touched and the call returns DZG_E_DEVICE: the call changes
 * everything or nothing.  Then
 *   the new data is stored on the host and the device (c, the constant, rhs0 of the dual objective
 *   and of Farkas rays: a later dzg_solver_duals, _ranging, _ray or dzg_solver_result speaks about
 *   the new LP);
 *   x = B^-1 rhs;   z_k = a_{N_k} . y - c[N_k] with y = B^-T c_B -- exactly the d of dzg_duals on the
 *   nonbasic positions;   xbar = zbar = 1.0;   status = DZG_RUNNING;
 *   every word of the control block that describes a pivot in flight (entering and leaving
 *   positions, the acknowledged near tie, the host's bounds on k) returns to what dzg_solver_create
 *   writes.
 * The pivot count, the pivot log, the margins, near_ties, first_near_tie, min_margin, refactors and
 * solve_ms keep accumulating; opts.max_iter bounds the total.
 * STRICT: x is the reference's LU::solve of B x = rhs, z comes from dzg_solver_duals' STRICT route
 * (LU::solve of B^T y = c_B, then neg_t_dot in the reference's order): bit for bit what the CPU
 * restatement gives.  FAST: both come from the fresh inverse, deterministic (no atomics): two calls
 * with the same data on the same state leave the same bits.
 * The drift measurement (state_drift, csrc/k_drift.hip) compares the carried state with a solve that
 * started on the slack basis with the OLD data; after this call it is switched off, as it is for
 * warm-started and resumed handles: state_drift reads 0, its share of the near-tie tolerance is 0 and
 * the tolerance returns to tie_tol.
 * The re-optimised path is not the reference's path from the slack basis: the promise is the
 * optimum (or the verdict), not the pivots. */
int dzg_solver_reoptimize(dzg_solver *s, const dzg_reopt *chg);

/* ---- Rows and columns added to a live LP, re-optimised from its basis (csrc/k_extend.hip) ---- */

/* p new constraint rows and r new structural columns for the LP a live handle holds. */
typedef struct {
    int64_t n_rows;        /* p >= 0 new constraint rows, appended below row m-1                     */
    int64_t n_cols;        /* r >= 0 new structural columns, appended after column n_struct-1        */
    const double *rows;    /* p x n_struct, ROW-major, leading dimension ld_rows >= n_struct:
                              the new rows' coefficients on the EXISTING structural columns          */
    int64_t ld_rows;
    const double *rhs;     /* p                                                                      */
    const double *cols;    /* (m+p) x r, COLUMN-major, ld_cols >= m+p: the new columns over all rows,
                              the new ones included                                                  */
    int64_t ld_cols;
    const double *c_cols;  /* r objective coefficients (core sense: maximised)                       */
} dzg_extend;

/* Appends the rows and columns of `ext` to the LP and leaves the handle in the state
 * dzg_solver_reoptimize leaves it in, on the extended LP and the extended basis B':
 * dzg_solver_run then carries on from B' with the parametric self-dual method.
 *   Numbering: no existing variable, row or column index changes.  With m, n, n_struct, q = n - m
 *   the sizes before the call, the new structural variables are n .. n+r-1 on the columns
 *   n_struct .. n_struct+r-1; the slacks of the new rows are n+r .. n+r+p-1 on the rows m .. m+p-1.
 *   A handle created with var_col == NULL holds an explicit var_col afterwards.  Basis positions
 *   0 .. m-1 keep their variables and positions m .. m+p-1 hold the new slacks; nonbasic positions
 *   0 .. q-1 keep theirs and positions q .. q+r-1 hold the new structural variables: the pivot log
 *   stays readable across the call.
 *   State: x = B'^-1 rhs', z_k = a_{N'_k} . y - c'[N'_k] with y = B'^-T c'_{B'}, xbar = zbar = 1,
 *   status DZG_RUNNING, no pivot in flight, the drift measurement switched off -- all as
 *   dzg_solver_reoptimize writes them, STRICT bit for bit the reference's LU::solve and neg_t_dot,
 *   FAST from a fresh refactorisation of B' and one step of iterative refinement of x and y against
 *   a double-double residual, the step dzg_solver_ray takes (deterministic, no atomics).  At the slack basis
 *   x = rhs' and z = -c' exactly.  The pivot count, the log, the margins, near_ties, first_near_tie,
 *   min_margin, refactors, solve_ms and max_pivot_error carry on; opts.max_iter bounds the total.
 *   The handle keeps the numerics it was created with, even if m + p crosses auto_strict_rows.
 *   A later dzg_solver_duals, _ranging, _ray, _reoptimize or _result speaks about the extended LP
 *   (dzg_solver_reoptimize then takes m + p and n + p + r entries; dzg_solver_dims reports them).
 *   Allowed in the states dzg_solver_reoptimize allows, before the first run included.
 *   DZG_E_ARG, on the host before any device work: NULL `s` or `ext`; p == r == 0; a negative count;
 *   ld_rows < n_struct or ld_cols < m + p; a needed array that is NULL; a NaN or infinite entry
 *   (dzg_last_error names the array and the index); CSC storage or a column- or row-sharded solver
 *   ("extend is not supported on CSC storage or sharded solvers"); a FAST handle without its
 *   refactorisation workspace (opts.refactor_interval == 0); status DZG_SINGULAR or DZG_PANIC.
 * All or nothing: the extended LP is built as a successor next to the live state and takes its place
 * only when everything has succeeded.  If device memory runs out (DZG_E_NOMEM) or B' does not
 * refactorise (DZG_E_DEVICE) the handle is exactly what it was.
 * Memory: until the swap BOTH matrices are resident -- lda x n_struct and lda' x (n_struct + r)
 * doubles, each with its row-major copy where one is kept -- next to both sets of state vectors and
 * FAST's two inverses; the old ones are freed before the call returns.  The resident m x n_struct
 * block is copied on the device; only p x n_struct + (m+p) x r new numbers cross to it.
 * -0.0 entries are stored as +0.0, as dzg_solver_create stores them. */
int dzg_solver_extend(dzg_solver *s, const dzg_extend *ext);
/* The sizes of the LP the handle holds now (any of the three may be NULL). */
int dzg_solver_dims(const dzg_solver *s, int64_t *m, int64_t *n, int64_t *n_struct);

/* ---- Rows and columns removed from a live LP, carried on from its basis (csrc/k_remove.hip) ---- */

/* Constraint rows and structural columns to drop from the LP a live handle holds. */
typedef struct {
    int64_t n_rows;  const int64_t *rows;   /* constraint rows to drop, each in [0, m)           */
    int64_t n_cols;  const int64_t *cols;   /* structural columns to drop, each in [0, n_struct) */
} dzg_remove;

/* Drops the listed rows together with their slack variables and the listed structural columns
 * together with their variables, and leaves the handle in the state dzg_solver_extend leaves it in, on
 * the reduced LP and the reduced basis B'.  Only what is free may go: a row whose slack is BASIC (its
 * dual value is 0; what is left of B is still a basis) and a structural column whose variable is
 * NONBASIC.  x on the surviving positions and every surviving z are then what they were, up to the
 * rounding of their recomputation: an optimal handle stays optimal and dzg_solver_run ends without a
 * pivot.
 *   Numbering: survivors are compressed in ascending order of their old index -- variables, rows and
 *   structural columns alike.  var_col is rewritten to match: a structural variable gets its new
 *   column, a slack -1 - (its new row).  The handle holds an explicit var_col afterwards.  Surviving
 *   basis positions keep their relative order, and so do the nonbasic positions.
 *   Maps (each may be NULL): var_map has the old n entries and row_map the old m entries, the new
 *   index or -1 for what was dropped.  They are written only when the call succeeds.
 *   The pivot log is carried over unchanged: its older entries speak in the numbering (variables and
 *   positions) of their time; compose the maps of the calls since to read them in today's.
 *   State: x = B'^-1 rhs', z_k = a_{N'_k} . y - c'[N'_k] with y = B'^-T c'_{B'}, xbar = zbar = 1,
 *   status DZG_RUNNING, no pivot in flight -- as dzg_solver_extend writes them: STRICT bit for bit the
 *   reference's LU::solve and neg_t_dot on B', FAST from the refactorisation dzg_solver_create runs on
 *   B' plus one step of iterative refinement.  The pivot count, the log, the margins, near_ties,
 *   first_near_tie, min_margin, refactors, solve_ms and max_pivot_error carry on.  The handle keeps
 *   its numerics, even if m' falls to auto_strict_rows or below.  Later calls speak about the reduced
 *   LP (dzg_solver_dims reports its sizes).
 *   Allowed in the states dzg_solver_extend allows, before the first run included (every row and
 *   every structural column is removable then).
 *   DZG_E_ARG, with the handle untouched: NULL `s` or `rem`, or a NULL list with a count > 0; both
 *   counts 0; a negative count; an index out of range or listed twice; a row whose slack is nonbasic
 *   (dzg_last_error says the row is binding and names it); a column whose variable is basic (named);
 *   fewer than one row or one structural column left; CSC storage or a column- or row-sharded
 *   solver ("remove is not supported on CSC storage or sharded solvers"); a FAST handle without its
 *   refactorisation workspace (opts.refactor_interval == 0); status DZG_SINGULAR or DZG_PANIC.
 * All or nothing: the reduced LP is built as a successor next to the live state, as in
 * dzg_solver_extend, and takes its place only when everything has succeeded (DZG_E_NOMEM,
 * DZG_E_DEVICE: the handle is exactly what it was).  Until the swap both matrices are resident.
 * The successor's matrix is lda' x n_struct', lda' by dzg_solver_create's rule for m' (it may drop);
 * it is gathered on the device from the resident one, only the two lists of survivors are uploaded.
 * Out of scope: dropping a binding row or a basic column (that needs a forced pivot first: pivot the
 * slack in or the column out, then call this); CSC storage and sharded solvers; rebuilding FAST's
 * compact inverse without a refactorisation (B'^-1 is B^-1 with rows and columns struck out, but the
 * call refactorises B'). */
int dzg_solver_remove(dzg_solver *s, const dzg_remove *rem, int64_t *var_map, int64_t *row_map);

/* ---- Batches re-optimised from their last bases (csrc/k_batch_restart.hip) ---------------- */

/* The basis an LP of a batch starts from: typically res[i].basis / res[i].nonbasis of an earlier
 * call on the same matrix. */
typedef struct {
    const int64_t *basis;     /* m,   NULL = start this LP cold */
    const int64_t *nonbasis;  /* n-m                            */
} dzg_batch_start;

/* dzg_batch_solve (du == NULL) or dzg_batch_solve_duals (du != NULL) with a start basis per LP.
 *   lps[i] is the LP to solve now, in the slack-basis form dzg_batch_solve takes: its basis is all
 *   slack, so lps[i].x[p] is the right-hand side of the row whose slack sits at position p; c and
 *   constant are the costs.  start[i] names the basis B (nonbasic set N) to start from.
 *   An entry with start[i].basis == NULL, and every entry when start == NULL, is solved exactly as
 *   dzg_batch_solve / dzg_batch_solve_duals solve it, bit for bit.  Cold and warm LPs mix freely;
 *   an LP's result does not depend on its place in the batch.
 * A warm LP gets dzg_solver_reoptimize's STRICT restart state before the first pivot, from one
 * launch of k_batch_restart per bucket:
 *   x = LU::solve(B, rhs);   z_k = a_{N_k} . y - c[N_k] with y = LU::solve(B^T, c_B), the d of
 *   dzg_duals on the nonbasic positions, in the reference's operation order;   xbar = zbar = 1.0;
 *   the pivot count and the log start at 0 for this call.
 * The pivots that follow are the reference's from that state, bit for bit.  They are not the
 * reference's pivots from the slack basis: the promise is the optimum (or the verdict), not the
 * path.
 * A start whose B or B^T meets a zero pivot anywhere in its factorisation (the last diagonal entry
 * included), or whose restart x or z holds a non-finite entry, ends DZG_SINGULAR without a pivot:
 * iterations = 0, basis / nonbasis as handed in.  The other LPs of the batch are not affected.
 * Numerics: STRICT, or AUTO (= STRICT here); FAST is DZG_E_ARG.  Every check of dzg_batch_solve
 * applies; beside them, on the host and before any device work, DZG_E_ARG with the LP's index in
 * dzg_last_error: a warm LP whose own basis is not all slack, nonbasis == NULL beside a basis, a
 * start that is not a partition of 0 .. n-1 into m and n-m distinct entries.
 * Nothing stays on the device between calls: the matrices go up again every time. */
int dzg_batch_solve_from(const dzg_lp *lps, const dzg_batch_start *start, int64_t count,
                         const dzg_opts *opts, int64_t pivots_per_launch, dzg_result *res,
                         dzg_duals *du);
/* Device time (ms, between two events on the call's stream) of the k_batch_restart launches of the
 * calling thread's last dzg_batch_solve_from; 0 when it had no warm LP. */
double dzg_debug_batch_restart_ms(void);

/* dzg_batch_solve_fast with a start basis per LP (csrc/k_batch_fast.hip, k_batch_fast_restart).
 *   lps[i] is the LP to solve now in slack-basis form and start[i] names the basis to start from, as
 *   for dzg_batch_solve_from.  An entry with start[i].basis == NULL, and every entry when start ==
 *   NULL, is solved exactly as dzg_batch_solve_fast solves it, bit for bit.  Cold and warm LPs mix
 *   freely; an LP's result does not depend on its place in the batch.
 * A warm LP gets dzg_solver_reoptimize's FAST restart state before the first pivot, from one launch
 * of k_batch_fast_restart per bucket, with W = B^-1 as a launch of the FAST batch builds it:
 *   x = W rhs;   z_k = a_{N_k} . y - c[N_k] with y = W^T c_B (stored entries only);   xbar = zbar =
 *   1.0;   no refinement step.  iterations and the log count from 0 for this call; refactors counts
 *   every inversion of a basis that is not all slack, the restart's included.
 * A start whose inversion meets a zero or non-finite pivot, or whose restart x or z holds a non-finite
 * entry, ends DZG_SINGULAR without a pivot: iterations = 0, basis / nonbasis as handed in.
 * opts->numerics: STRICT is dzg_batch_solve_from(lps, start, count, opts, pivots_per_launch, res,
 * NULL).  FAST honours near_tie_action and tie_tol.  AUTO, and opts == NULL, runs FAST with
 * near_tie_action = STOP, and every LP that ends DZG_NEAR_TIE, DZG_SINGULAR or DZG_PANIC is solved
 * again in the same call by dzg_batch_solve_from, from the same start (a cold entry cold), into the
 * same result slot, which is then bit for bit what dzg_batch_solve_from gives for that LP;
 * res[i].numerics_used says which numerics produced res[i].
 * Host checks, before any device work: every check of dzg_batch_solve_fast (refactor_every < 0
 * included) and every start check of dzg_batch_solve_from, with the same dzg_last_error texts.
 * Nothing stays on the device between calls. */
int dzg_batch_solve_fast_from(const dzg_lp *lps, const dzg_batch_start *start, int64_t count,
                              const dzg_opts *opts, int64_t pivots_per_launch,
                              int64_t refactor_every, dzg_result *res);
/* Device time (ms, between two events on the call's stream) of the k_batch_fast_restart launches of
 * the calling thread's last dzg_batch_solve_fast or dzg_batch_solve_fast_from; 0 when it had no warm
 * LP. */
double dzg_debug_batch_fast_restart_ms(void);

/* ---- Duals, ranging and rays behind a FAST batch (csrc/k_batch_post.hip) ------------------ */

/* What a batch call computes beside the solve, from the state every LP ended in: du, (req, rg) and
 * ry hold `count` entries each and mean what they mean for dzg_batch_solve_duals / _ranging / _rays.
 * Every pointer is optional and all four compose in one call; req needs rg and rg needs req; ranging
 * computes the duals whether du is given or not. */
typedef struct {
    dzg_duals *du;
    const dzg_ranging_req *req;
    dzg_ranging *rg;
    dzg_ray *ry;
} dzg_batch_post;
/* dzg_batch_solve_fast_from(lps, start, count, opts, pivots_per_launch, refactor_every, res) -- res
 * is bit for bit what that call fills, and post == NULL, or a post whose four pointers are NULL, is
 * exactly that call -- and then, after the rounds and after AUTO's second attempt, per LP by
 * res[i].numerics_used and res[i].status:
 *   a FAST result: k_batch_fast_post, one workgroup per LP.  W = B^-1 of the final basis as a launch
 *     of the FAST batch builds it (an all-slack basis is a permutation; no refinement step), then
 *     OPTIMAL:  y = W^T c_B, d[N_k] = -dz_k - c[N_k] with dz one pricing pass over y (stored entries
 *       only), d[B_p] = 0.0, dual_obj = constant + rhs0 . y, source DZG_DUALS_FRESH; with ranging, a
 *       right-hand-side direction h gives delta_p = sum_e W[p][r_e] h_e over its entries in the order
 *       given, a cost direction g gives Y = sum over its basic entries of g_e (row pos(e) of W) and
 *       delta_k = -dz_k(Y) - g[N_k] (no basic entry: Y = 0 and no pricing pass); candidates, clamping,
 *       pivot_tol, ties and *_var as dzg_ranging defines them.
 *     UNBOUNDED / INFEASIBLE:  pos = the first-pivot winner over (z, zbar) / (x, xbar) as the FAST
 *       iteration finds it; PRIMAL: dx = W a_j;  FARKAS: y = row pos of W, dz one pricing pass;
 *       d, value, violation and proven as dzg_ray defines them.
 *     Every sum's order depends on m alone (four interleaved partial sums, j ascending; pricing as in
 *     the solve), the reductions are min / max with the position as tie-break and there are no
 *     atomics: an LP's post-solve does not depend on its place in the batch, and asking twice gives
 *     the same bits.  rhs0 is the right-hand side by constraint row for an LP with a start basis and
 *     the starting x as it is for a cold one.  The carried state, the pivot count, refactors and the
 *     log are not touched.  If the final basis does not invert (a zero or non-finite pivot) the LP
 *     reports nothing -- source = 0, kind = 0, NaN ranges, *_var = -1 -- and its result stands.
 *   a STRICT result (opts->numerics STRICT, or an LP AUTO handed over): k_duals_small,
 *     k_ranging_small and k_rays_small on the final state of the STRICT batch.  For a cold LP that is
 *     bit for bit what dzg_batch_solve_duals / _ranging / _rays return; a warm LP gets the same
 *     kernels on its final state, so through this call a start basis composes with ranging and rays.
 *   any other status (DZG_NEAR_TIE, DZG_SINGULAR, DZG_PANIC or DZG_ITER_LIMIT under pure FAST): no
 *     post-solve, source = 0, kind = 0, NaN ranges.
 * Host checks, before any device work: every check of dzg_batch_solve_fast_from, req without rg or
 * rg without req, and the checks of dzg_ranging_req per LP (indices in range and distinct per
 * direction, pivot_tol negative or NaN); DZG_E_ARG with the LP's index in dzg_last_error. */
int dzg_batch_solve_post(const dzg_lp *lps, const dzg_batch_start *start, int64_t count,
                         const dzg_opts *opts, int64_t pivots_per_launch, int64_t refactor_every,
                         const dzg_batch_post *post, dzg_result *res);
/* Device time (ms, between two events on the call's stream) of the post-solve launches of post_pass
 * (csrc/batch_steps.h) in the calling thread's last dzg_batch_solve_post or dzg_batch_resolve_post:
 * k_batch_fast_post for the FAST results and, on a handle, k_duals_small / k_ranging_small /
 * k_rays_small for the STRICT ones, added up.  0 when the call launched none, and after
 * dzg_batch_solve_post with numerics = STRICT, whose post-solve is dzg_batch_solve_ranging's own and
 * is not timed. */
double dzg_debug_batch_post_ms(void);

/* ---- A batch kept resident on the device between solves (csrc/k_batch_resident.hip) ------- */

/* The batched sibling of dzg_solver_reoptimize: the matrices, var_col and the descriptors of `count`
 * small LPs go up once; every later solve uploads the right-hand sides and costs that changed and
 * nothing else.  The handle holds, per LP i: the matrix and var_col (fixed at create); the current
 * rhs_i, c_i and constant_i; and last_i, the basis its last solve ended on -- none before the first
 * solve and after a solve that ended DZG_SINGULAR or DZG_PANIC.  One call at a time per handle;
 * several handles may live at once.  While it lives a handle holds one device allocation the size of
 * a stateless call's (the log sections sized by log_cap) plus rhs, c and three copies of a basis.
 * A HIP failure inside any call leaves the handle failed: every later call returns DZG_E_DEVICE;
 * dzg_batch_destroy still frees everything.
 * On the handle too: duals, ranging and rays: dzg_batch_resolve_post (below).
 * Out of scope: adding or removing rows, columns or LPs; the node LPs of dzg_mip_solve;
 * folding the restart into the first launch. */
typedef struct dzg_batch dzg_batch;

/* lps[0..count): dense, m <= DZG_BATCH_MAX_ROWS, in slack-basis form (own basis all slack, one
 * per row; xbar == zbar == NULL).  opts->numerics: STRICT, FAST or AUTO, with the meaning
 * dzg_batch_solve_fast_from gives them (opts == NULL: AUTO).  pivots_per_launch / refactor_every
 * as there.  log_cap >= 0: pivots of log kept per LP and per solve (0: none).
 * Host checks (DZG_E_ARG, the LP's index in dzg_last_error, before any device work): every check of
 * dzg_batch_solve_fast_from, an own basis that is not all slack, xbar / zbar given, log_cap < 0,
 * out == NULL.  count == 0 is a valid, empty handle. */
int  dzg_batch_create(const dzg_lp *lps, int64_t count, const dzg_opts *opts,
                      int64_t pivots_per_launch, int64_t refactor_every, int64_t log_cap,
                      dzg_batch **out);
void dzg_batch_destroy(dzg_batch *b);

typedef struct {
    int64_t lp;            /* index in the batch                                   */
    const double *rhs;     /* m, by constraint row (as dzg_reopt); NULL = keep      */
    const double *c;       /* n, by variable, core sense; NULL = keep               */
    double constant;       /* used when set_constant != 0                           */
    int32_t set_constant, reserved;
} dzg_batch_change;
/* Updates accumulate until the LP is next solved; per array the last value wins.  DZG_E_ARG, the
 * handle unchanged: NULL arguments with nchg > 0, lp out of range or listed twice in one call, an
 * entry with rhs, c and set_constant all empty, a NaN or infinite entry (array and index named). */
int dzg_batch_update(dzg_batch *b, const dzg_batch_change *chg, int64_t nchg);

/* The basis LP `lp` starts its next solve from; basis == NULL: cold (the slack basis).
 * DZG_E_ARG: not a partition of 0 .. n-1 (dzg_batch_solve_from's check). */
int dzg_batch_set_start(dzg_batch *b, int64_t lp, const int64_t *basis, const int64_t *nonbasis);

/* Solves the LPs which[0..nwhich) (which == NULL: all, in index order); res[k] belongs to
 * which[k].  res is filled, result for result and bit for bit, as
 *   dzg_batch_solve_fast_from(lps', start', nwhich, &opts, pivots_per_launch, refactor_every, res)
 * fills it, where lps'[k] is LP which[k] in slack-basis form with its current data (basis and
 * nonbasis those of create, x[p] the current right-hand side of the row whose slack sits at
 * position p, z the array handed to create until c is first updated and -c[nonbasis[k]] after) and
 * start'[k] = last_{which[k]}; the log is capped at min(res[k].log_cap, log_cap).  That covers
 * numerics_used, AUTO's STRICT second attempt from the same start, a singular start ending
 * DZG_SINGULAR with 0 iterations and the basis as it was, refactors and margins; STRICT numerics
 * is dzg_batch_solve_from's result.  Afterwards last_i is updated for the LPs listed; the LPs not
 * listed are not touched: their state on the device, their pending updates and last_i stay.
 * DZG_E_ARG, nothing changed: res == NULL, an index out of range or listed twice, nwhich < 0. */
int dzg_batch_resolve(dzg_batch *b, const int64_t *which, int64_t nwhich, dzg_result *res);

/* dzg_batch_resolve(b, which, nwhich, res) -- res has that call's bits, last_i moves as there, and
 * post == NULL or a post whose four pointers are NULL is exactly that call -- and then the post-solve
 * dzg_batch_solve_post defines, on the handle's own arena, from the resident c and the resident
 * right-hand sides by constraint row: a FAST result through k_batch_fast_post, a STRICT result (a
 * STRICT handle, or an LP AUTO handed over) through k_duals_small / k_ranging_small / k_rays_small on
 * its final state.  post's arrays hold one entry per listed LP: entry k belongs to which[k].  The
 * outputs come down for the listed LPs only; the carried state is not touched, so the next solve is
 * what it would have been.  Host checks, DZG_E_ARG and nothing changed: those of dzg_batch_resolve,
 * req without rg or rg without req, a ranging request that dzg_ranging_req refuses (which[k] named).
 * The bytes join dzg_debug_batch_traffic's; dzg_debug_batch_post_ms gives the launches' time. */
int dzg_batch_resolve_post(dzg_batch *b, const int64_t *which, int64_t nwhich,
                           const dzg_batch_post *post, dzg_result *res);

/* Test and measurement hook: bytes[0] / bytes[1] = host-to-device / device-to-host bytes of the
 * handle's last dzg_batch_resolve (every copy it enqueued, staged updates included);
 * ms[0] = device time between two events around its stage + restart launches. */
int dzg_debug_batch_traffic(const dzg_batch *b, int64_t bytes[2], double ms[1]);

/* ---- Mixed-integer models: branch and bound over batched node LPs (csrc/mip.cpp, k_mip.hip) -- */

/* Search knobs.  dzg_mip_opts_default() fills the defaults; in a zeroed struct the counts mean
 * "default" (node_limit 100000, nodes_per_round 1024, pivots_per_launch 16) while the tolerances are
 * taken as given (0 = exact).  Negative counts or tolerances and NaN tolerances are DZG_E_ARG, and so
 * is a warm_start other than 0 or 1. */
typedef struct {
    int64_t node_limit;        /* node LPs solved at most, then DZG_NODE_LIMIT; 0 = 100000        */
    int32_t nodes_per_round;   /* open nodes solved together per round; 0 = 1024                  */
    int32_t warm_start;        /* 0 = off; 1 = warm-start children from the parent's basis (below) */
    int64_t pivots_per_launch; /* as in dzg_batch_solve; 0 = 16                                   */
    double int_tol;            /* v is integral if |v - rint(v)| <= int_tol (default 1e-6)        */
    double abs_gap;            /* prune when objective <= incumbent + max(abs_gap, rel_gap*|inc|) */
    double rel_gap;            /*   (defaults 1e-9 and 0)                                         */
} dzg_mip_opts;

/* One solved node LP.  The root has id 0, parent -1, branch_var -1, direction 0.  A child records
 * the user variable branched on, direction -1 (down: ub = floor v) or +1 (up: lb = floor v + 1)
 * and that new bound.  objective (core sense) is meaningful when status is DZG_OPTIMAL. */
typedef struct {
    int64_t id, parent, branch_var;
    int32_t direction, status;
    double bound;
    int64_t iterations;
    double objective;
} dzg_mip_node;

typedef struct {
    int32_t status;            /* OPTIMAL, INFEASIBLE, UNBOUNDED (root relaxation), NODE_LIMIT, or
                                  the status of the node LP that failed (see failed_node)        */
    int32_t has_incumbent;
    double objective;          /* the incumbent's, core sense (maximised)                          */
    double *values;            /* nvars, optional: the incumbent node LP's own values (not rounded) */
    double best_bound;         /* max of the incumbent and the open nodes' parent bounds           */
    int64_t nodes_solved, nodes_batched, nodes_sequential;
    int64_t nodes_fast;        /* sequential node LPs dzg_model_solve ran in FAST numerics (AUTO,
                                  m > auto_strict_rows): 0 means every node LP is STRICT           */
    int64_t nodes_pruned;      /* pruned by bound, after solving or when selected                  */
    int64_t nodes_dropped;     /* infeasible node LPs and children whose bounds cross (never created) */
    int64_t rounds, lp_iterations;
    int64_t incumbent_node, failed_node; /* -1 when none */
    dzg_mip_node *log;         /* optional caller-owned node log, log_cap entries, in solve order  */
    int64_t log_cap, log_count;
} dzg_mip_result;

/* A warm-started node LP is accepted only if it ends OPTIMAL with every carried x and z at or above
 * -DZG_MIP_WARM_TOL (the default abs_gap); otherwise the node is solved again from the slack basis. */
#define DZG_MIP_WARM_TOL 1e-9

/* What warm_start did in the calling thread's last dzg_mip_solve (all zero after a cold search). */
typedef struct {
    int64_t nodes_warm;         /* node LPs started from their parent's basis (attempts)          */
    int64_t nodes_restarted;    /* of those, the attempts discarded and solved again cold          */
    int64_t warm_iterations;    /* pivots of the warm attempts, kept or discarded                  */
    int64_t restart_iterations; /* pivots of the cold runs of the restarted nodes                  */
} dzg_mip_warm_stats;

void dzg_mip_opts_default(dzg_mip_opts *mo);
/* Maximises model's objective with is_integer[u] != 0 marking integer variables.  Every node LP is
 * the model with the integer variables' bounds replaced by the node's, solved exactly as
 * dzg_model_solve(node model, opts) solves it: nodes that call would run in STRICT on <= 128 dense
 * rows go through k_mip.hip in batched rounds, the others through dzg_model_solve one at a time.
 * The search (best bound first, most fractional branching, incumbent updated between rounds) is
 * deterministic for a given nodes_per_round.  opts / mip_opts NULL: defaults.  FAST numerics is
 * DZG_E_ARG, and so is a bound of an integer variable that is flagged (has_lb / has_ub) but not
 * finite: the search keys nodes on which integer bounds are finite.  Returns res->status (>= 0) or a negative code.
 *
 * mip_opts->warm_start = 1 (opt-in; the above holds bit for bit with 0) relaxes "node LP =
 * dzg_model_solve of the node model" for speed: a child solved by k_mip.hip whose parent was solved
 * there too, with the same set of finite integer bounds (a branch that adds no bound row), starts
 * from the parent's final basis, nonbasis and carried z, with x = B^-1 b for its own right-hand side
 * and both perturbation vectors at one, instead of from the slack basis.  The attempt is kept only
 * if it ends OPTIMAL and passes the DZG_MIP_WARM_TOL sign check; any other end restarts the node cold
 * in the same round, and status, objective, values and branching are then the cold run's.  A node's
 * logged iterations are the pivots of both runs.  The tree may differ from the cold tree (another
 * optimal vertex, last bits of an objective); the optimum found is the same.  Still independent of
 * pivots_per_launch and deterministic for a given nodes_per_round. */
int dzg_mip_solve(const dzg_model *model, const int32_t *is_integer, const dzg_opts *opts,
                  const dzg_mip_opts *mip_opts, dzg_mip_result *res);
void dzg_mip_last_warm_stats(dzg_mip_warm_stats *out);

/* ---- FAST node LPs (opt-in; DESIGN.md 7c "FAST node LPs") ------------------------------------
 * dzg_mip_solve_nodes is dzg_mip_solve with node options; dzg_mip_solve(...) is
 * dzg_mip_solve_nodes(..., NULL, ...), and NULL or numerics = DZG_NUMERICS_STRICT change nothing,
 * bit for bit.  With numerics = DZG_NUMERICS_FAST every node that k_mip.hip would batch (<= 128 dense
 * rows under the STRICT rule) gets an attempt in FAST numerics first, the loop of dzg_batch_solve_fast
 * on a control block of the node's own; opts->tie_tol and opts->near_tie_action apply as given
 * (default COUNT), opts->numerics keeps its meaning (STRICT or AUTO; FAST stays DZG_E_ARG).
 *   start    a node that warm_start would start warm (warm_start = 1, a parent solved by k_mip.hip,
 *            the same set of finite integer bounds) starts from the parent's final basis and nonbasis
 *            with the FAST restart state of dzg_batch_solve_fast_from (W = B^-1, x = W rhs,
 *            y = W^T c_B, z = -dz - c_N, both perturbation vectors at one; the parent's z is not
 *            used), and its first launch pivots on that W.  Every other node starts from the slack basis.
 *   accept   an attempt that ends DZG_OPTIMAL is certified from its final basis: the inverse is
 *            rebuilt, x and z are recomputed by the same formulas and replace the carried ones, and
 *            the node stands only if every one of them is >= -DZG_MIP_WARM_TOL (NaN fails).  An
 *            accepted node is primal and dual feasible at one basis of its own LP; objective,
 *            values, integrality and the branching choice come from the recomputed x.
 *   reject   every other end (INFEASIBLE, UNBOUNDED, NEAR_TIE, SINGULAR, PANIC, ITER_LIMIT, a failed
 *            sign check) discards the attempt: the node is solved in the same round by the STRICT
 *            kernel from the slack basis, and its status, objective, values and branching are then
 *            bit for bit dzg_model_solve's of the node model.  Its logged iterations are the pivots
 *            of both runs.  A root that FAST ends UNBOUNDED is thus confirmed by STRICT first.
 * Nodes on the sequential route (dzg_model_solve) are untouched.  The optimum is the cold search's;
 * the tree may differ, as with warm_start.  The search is deterministic for a given nodes_per_round,
 * pivots_per_launch and refactor_every of this struct -- and NOT independent of the last two: the
 * FAST kernel rebuilds the inverse at the start of every launch and every refactor_every pivots, so
 * they move last bits and, through ties, possibly the tree.  With FAST, dzg_mip_last_warm_stats counts
 * the accepted warm attempts only (nodes_restarted = 0); rejected attempts are in dzg_mip_fast_stats. */
typedef struct {
    int32_t numerics;          /* DZG_NUMERICS_STRICT (0-filled default) or DZG_NUMERICS_FAST */
    int32_t reserved;
    int64_t pivots_per_launch; /* FAST node launches; 0 = 128, the FAST batch's default */
    int64_t refactor_every;    /* 0 = 64, the FAST batch's default */
    int32_t *route;            /* optional, caller-owned, parallel to res->log: 0 STRICT batched,
                                  1 FAST accepted, 2 FAST rejected then STRICT, 3 sequential */
    int64_t route_cap;
} dzg_mip_node_opts;
void dzg_mip_node_opts_default(dzg_mip_node_opts *no);
/* numerics other than STRICT or FAST, negative counts, route_cap < 0 (or > 0 without route):
 * DZG_E_ARG with a "mip:" text, before any device work. */
int dzg_mip_solve_nodes(const dzg_model *model, const int32_t *is_integer, const dzg_opts *opts,
                        const dzg_mip_opts *mip_opts, const dzg_mip_node_opts *node_opts,
                        dzg_mip_result *res);
/* What the FAST attempts did in the calling thread's last search (zeros after any other search,
 * a failed call included). */
typedef struct {
    int64_t nodes_fast;        /* node LPs that got a FAST attempt                       */
    int64_t nodes_rejected;    /* of those, the attempts discarded and solved in STRICT  */
    int64_t fast_iterations;   /* pivots of the FAST attempts, kept or discarded         */
    int64_t strict_iterations; /* pivots of the STRICT runs of the rejected nodes        */
} dzg_mip_fast_stats;
void dzg_mip_last_fast_stats(dzg_mip_fast_stats *out);

/* Test hook (tests/test_gpu_mip_fast.py): one node LP of `model` through the FAST node kernel, as a
 * round of dzg_mip_solve_nodes with numerics = FAST solves it.  bnd: lb, ub per integer variable in
 * index order (+-inf: none).  start_basis (m variables of the standard form, or NULL for a cold
 * node): the basis a warm node would take from its parent; the nonbasis is every other variable in
 * ascending order.  cap_m / cap_q size basis, x / nonbasis, z, which receive the node's final state
 * (the STRICT run's if the attempt was rejected); *m_out and *q_out the sizes.  The attempt is always
 * FAST: node_opts->numerics is not consulted, only pivots_per_launch and refactor_every are.  The
 * STRICT run of a rejected attempt uses the defaults of dzg_mip_opts (pivots_per_launch 16) and the
 * epilogue int_tol = 1e-6; opts->epsilon, tie_tol and near_tie_action apply as in the search. */
typedef struct {
    int32_t status, route;     /* route: 1 FAST accepted, 2 FAST rejected then STRICT */
    int64_t iterations, fast_iterations;
    double objective;
} dzg_mip_debug_node;
int dzg_debug_mip_fast_node(const dzg_model *model, const int32_t *is_integer, const double *bnd,
                            const int32_t *start_basis, const dzg_opts *opts,
                            const dzg_mip_node_opts *node_opts, int64_t cap_m, int64_t cap_q,
                            int32_t *basis, int32_t *nonbasis, double *x, double *z, int64_t *m_out,
                            int64_t *q_out, dzg_mip_debug_node *out);

/* Host-only: the standard-form builder alone (Simplex::new, src/simplex.rs:123-224).
 * Two-call protocol: first call with out->a == NULL fills m, n, n_struct and lda;
 * the caller allocates a[lda*n_struct], var_col[n], c[n], basis[m], nonbasis[n-m],
 * x[m], z[n-m], pos_var[nvars], neg_var[nvars] and calls again. */
typedef struct {
    int64_t m, n, n_struct, lda;
    double *a;
    int64_t *var_col;
    double *c;
    double constant;
    int64_t *basis, *nonbasis;
    double *x, *z;
    int64_t *pos_var, *neg_var;  /* variable index of x+ / x- per user variable, -1 if unseen */
} dzg_stdform;

int dzg_build_standard_form(const dzg_model *model, dzg_stdform *out);

/* ---- single reference functions on the GPU, for parity tests ---------------------- */

/* lu_solve (src/linalg.rs:8-10): a is n*n ROW-major and is not modified; x_out[n].
 * lu_out (n*n, may be NULL) and p_out (n-1, may be NULL) receive the packed factors
 * exactly as Matrix::factorize leaves them (src/linalg.rs:88-128). */
int dzg_kernel_lu_solve(int64_t n, const double *a, const double *b, double *x_out,
                        double *lu_out, int64_t *p_out, int32_t device);

/* collect_columns(cols).neg_t_dot(v) (src/linalg.rs:188-207) on a dense column-major
 * matrix: out[k] = -sum_i a[i, cols[k]] * v[i]; cols[k] < 0 selects the unit column of
 * row (-1 - cols[k]).  kernel: dzg_price_kernel. */
int dzg_kernel_neg_t_dot(int64_t m, int64_t n_struct, const double *a, int64_t lda,
                         const int64_t *cols, int64_t ncols, const double *v, double *out,
                         int32_t kernel, int32_t device);

/* The same on a CSC matrix (the reference's own storage, src/linalg.rs:161-168: rows ascending
 * inside a column, no explicit zeros): out[k] = sum over the stored entries of column cols[k],
 * in stored order, of val * -v[row] -- exactly neg_t_dot's loop (src/linalg.rs:199-207). */
int dzg_kernel_neg_t_dot_csc(int64_t m, int64_t n_struct, const int64_t *col_ptr,
                             const int32_t *row_idx, const double *val, const int64_t *cols,
                             int64_t ncols, const double *v, double *out, int32_t device);

/* find_first_pivot (src/simplex.rs:423-437): position or -1. */
int dzg_kernel_first_pivot(int64_t len, const double *y, const double *ybar, int64_t *pos_out,
                           int32_t device);
/* find_second_pivot (src/simplex.rs:439-461): position or -1. */
int dzg_kernel_second_pivot(int64_t len, double mu, const double *y, const double *ybar,
                            const double *dy, int64_t *pos_out, int32_t device);

/* ---- synthetic LPs of SURVEY 8(d) (host code, SplitMix64; used by bench and tests) -- */

/* Generator G2 (sparse): `per_col` nonzeros per column at distinct rows (sorted ascending),
 * values 2u-1 (redrawn if 0), b = A x0 + rb, c = A^T y0 - rc as in G1.
 * col_ptr[n_struct+1], row_idx[n_struct*per_col], val[n_struct*per_col], b[m], c[n_struct]. */
int dzg_gen_sparse_lp(uint64_t seed, int64_t m, int64_t n_struct, int64_t per_col,
                      int64_t *col_ptr, int32_t *row_idx, double *val, double *b, double *c);

/* Generator G1: dense m x n_struct LP, primal- and dual-feasible by construction.
 * a[lda*n_struct] column-major, b[m], c[n_struct]. */
int dzg_gen_dense_lp(uint64_t seed, int64_t m, int64_t n_struct, double *a, int64_t lda,
                     double *b, double *c);

/* The same LP, bit for bit, but only columns [col_begin, col_end) of A are produced
 * (a_block[lda*(col_end-col_begin)]); b[m] and c[n_struct] are complete.  What one rank of a
 * column-sharded solve needs (pair with opts.a_is_block = 1). */
int dzg_gen_dense_lp_block(uint64_t seed, int64_t m, int64_t n_struct, int64_t col_begin,
                           int64_t col_end, double *a_block, int64_t lda, double *b, double *c);

/* ---- column sharding over several GPUs, one process per GPU ------------------------
 * The host (torch.distributed over RCCL, or any collective layer) moves the small
 * exchange records between ranks; the library only produces and consumes them.
 * See DESIGN.md "Multi-GPU". */
typedef struct {
    double ratio;       /* candidate ratio, -inf when this rank has none                 */
    int64_t pos;        /* GLOBAL nonbasic position of the candidate, INT64_MAX if none   */
    double y, ybar, dy; /* z, zbar, dz of the candidate (for the step lengths s, sbar)    */
} dzg_candidate;

/* A sharded solver is created with opts.world > 1, opts.rank and this rank's column block
 * [col_begin, col_end) (FAST numerics; `a` holds ALL structural columns, only the block is
 * uploaded).  One iteration = three enqueue-only phases with one all-gather of one record per
 * rank between them; record = dzg_shard_record_doubles() doubles:
 *   [0] ratio  [1] global nonbasic position (-1 = none)  [2] z  [3] zbar  [4] dz
 *   [5] column code  [6..7] reserved  [8 .. 8+m) the candidate's column of A
 * phase1: proposes this rank's first-pivot candidate on the z side (src/simplex.rs:275);
 * phase2: merges the proposals (largest ratio, lowest position), runs status() and the part
 *         of the step that precedes the second exchange (primal: FTRAN, x ratio test, BTRAN,
 *         pricing of the owned columns; dual: BTRAN, pricing) and proposes the z-side ratio
 *         candidate (dual) or publishes z, zbar, dz of the entering position (primal);
 * phase3: merges, finishes the step (dual: FTRAN), pivots and updates.
 * `send`/`recv` are DEVICE pointers owned by the host (recv holds world records in rank order).
 * The library never calls a collective itself. */
/* With opts.shard_rows the record is
 *   [0..7]   the z-side candidate as above ([7] reserved)
 *   [8] ratio  [9] basis position p (-1 = none)  [10] x_p  [11] xbar_p  [12] dx_p (second exchange of
 *            a primal step)  [13] reserved  [14] runner-up  [15] reserved      -- the x-side candidate
 *            of the rank's own rows: first pivot (exchange 1), ratio test of a primal step (exchange 2)
 *   [16 .. 80)          U_t[p] of the pending etas t < 64
 *   [80 .. 80 + mc)     the z-side candidate's column of A (mc = ceil16(m); partitioned storage only,
 *                       mc = 0 with replicate_matrix)
 *   [80 + mc .. )       row p of the compact inverse Binv0, as many entries as the record holds
 * dzg_shard_record_doubles is the largest record (room for a row of m entries); dzg_shard_run sends
 * what the current compact width needs.  A host that drives the phases itself keeps the records of
 * exchange 1 intact until phase 3 has been enqueued and run (phase 3 reads the leaving row of a dual
 * step and the entering column of a primal step from them): two receive buffers. */
int64_t dzg_shard_record_doubles(const dzg_solver *s);
int dzg_shard_phase1(dzg_solver *s, double *send_dev);
int dzg_shard_phase2(dzg_solver *s, const double *recv_dev, double *send_dev);
int dzg_shard_phase3(dzg_solver *s, const double *recv_dev);
/* The whole sharded loop in native code.  dzg_shard_comm_init joins this rank to an RCCL
 * communicator (librccl is loaded lazily with dlopen; `unique_id` is the 128-byte ncclUniqueId
 * produced by dzg_comm_unique_id on rank 0 and distributed by the host, e.g. over gloo);
 * dzg_shard_run then iterates phase1 -> ncclAllGather -> phase2 -> ncclAllGather -> phase3 on
 * the solver's stream (xGMI between the GPUs of a node) and polls the status word every
 * poll_interval iterations.  Returns the status like dzg_solver_run. */
int dzg_comm_unique_id(void *unique_id_128);
int dzg_shard_comm_init(dzg_solver *s, const void *unique_id_128);
int dzg_shard_run(dzg_solver *s, int64_t max_new_iters);
/* Ranks of the communicator as RCCL counts them (ncclCommCount), or < 0. */
int dzg_shard_comm_size(dzg_solver *s);
/* All ranks inside one process on one device (solvers[r] created with rank r and a common
 * opts.stream = dzg_solver_stream(solvers[0])): the exchange is a device-to-device copy.
 * This is how the sharded device path is exercised on a single-GPU box. */
int dzg_shard_run_lockstep(dzg_solver **solvers, int32_t world, int64_t max_new_iters);
void *dzg_solver_stream(dzg_solver *s);
/* Changes which kernel classes are timed (opts.profile mask) between runs; the solver must have
 * been created with opts.profile != 0. */
int dzg_solver_set_profile(dzg_solver *s, int32_t mask);
/* Synchronises the stream and reads the status word and the pivot count. */
int dzg_solver_poll(dzg_solver *s, int32_t *status, int64_t *iterations);
/* Sets the run budget like dzg_solver_run does, without running (sharded hosts drive the loop). */
int dzg_solver_set_budget(dzg_solver *s, int64_t max_new_iters);

/* Test hook (tests/test_gpu_parity.py, tools/): occupies `workgroups` CUs of `device` for about
 * `seconds` with a kernel that holds 128 KB of LDS per workgroup and watches the clock, on a
 * stream of its own; returns at once.  dzg_debug_hold_wait waits for it.  This is how the
 * three-launch iteration's recovery from a co-tenant on the device is exercised. */
int dzg_debug_hold_cus(int32_t device, int32_t workgroups, double seconds);
int dzg_debug_hold_wait(void);

/* Test hook: checks the live-entry lists the sparse-basis pricing pass walks (csrc/k_sparse.hip,
 * k_price_csc_rl) against their definition; returns the number of columns whose list is wrong
 * (0 = consistent), < 0 on error (no such lists: DZG_E_ARG); *entries = entries listed in all. */
int64_t dzg_debug_live_lists(dzg_solver *s, int64_t *entries);
/* Test hook: the constraint row whose entries k_sp_btran has listed ahead of a pivot that has not
 * been executed yet (a run that stopped between BTRAN and the pivot, DZG_NEAR_TIE in a dual step's
 * ratio test), -1 if none; < -1 on error.  dzg_debug_live_lists counts that row as listed. */
int64_t dzg_debug_rl_listed(dzg_solver *s);
/* Test hooks (tests/test_gpu_extend.py): the dense matrix as the kernels read it.
 * dzg_debug_matrix copies structural columns [col0, col1), m rows each, column-major into `out`
 * (ld_out >= m) and returns 0.  dzg_debug_matrix_rows copies rows [row0, row1) of the row-major copy
 * the row-wise pricing pass reads, n_struct entries each, row-major into `out` (ld_out >= n_struct)
 * and returns the number of rows copied: 0 where that copy is not kept.  < 0 on error (CSC storage,
 * a sharded solver, a range outside the matrix: DZG_E_ARG). */
int dzg_debug_matrix(dzg_solver *s, int64_t col0, int64_t col1, double *out, int64_t ld_out);
int64_t dzg_debug_matrix_rows(dzg_solver *s, int64_t row0, int64_t row1, double *out, int64_t ld_out);
/* Test and measurement hook (tools/extend_bench.py): how the last dzg_solver_extend on this handle
 * spent its time, in ms of host clock -- [0] the matrix re-laid on the device (the successor's
 * allocation, the resident block copied, the new rows and columns uploaded, the row-major copy),
 * [1] the refactorisation of B', [2] the restart state (x, z).  Zeros before the first call. */
int dzg_debug_extend_ms(const dzg_solver *s, double ms[3]);
/* Test hook (tests/test_gpu_inverse.py): rows [row0, row1) of the basis inverse a FAST solver keeps,
 * B^-1 = Binv0 - U W^T (dense) or its sparse-basis form, assembled on the host from device copies of
 * the buffers the kernels read.  Row i of `out` is basis position row0 + i, column r constraint row
 * r; row-major, (row1 - row0) x m.  info = {ncompact (k), pending etas, first and end row this
 * solver keeps (a row-sharded rank: its slice; rows outside it are DZG_E_ARG)}.  STRICT: DZG_E_ARG.
 * No solve path calls it. */
int dzg_debug_basis_inverse(dzg_solver *s, int64_t row0, int64_t row1, double *out, int64_t info[4]);
/* Test hook (tests/test_gpu_batch_fast_inverse.py): the inverse W = B^-1 a dzg_batch_solve_fast launch
 * keeps in LDS and loses when it ends.  For every LP, W is built from the LP's starting basis exactly
 * as a launch builds it at its first step; at most `pivots` (>= 0) pivots run in that one launch, the
 * production kernel body with an epilogue that copies W out; refactor_every as in
 * dzg_batch_solve_fast (0 = 64; above `pivots`: no rebuild inside the launch).  res[i] is filled as
 * dzg_batch_solve_fast fills it (DZG_ITER_LIMIT if the budget ended the LP; opts->max_iter is not
 * consulted), and the final W goes to w_out: LP after LP, dense row-major m x m, row p basis
 * position p, column r constraint row r (sum of m^2 doubles).  opts->numerics must be FAST; the host
 * checks of dzg_batch_solve_fast run first.  No solve path calls it. */
int dzg_debug_batch_fast_inverse(const dzg_lp *lps, int64_t count, const dzg_opts *opts, int64_t pivots,
                                 int64_t refactor_every, double *w_out, dzg_result *res);

/* Test hook (tests/test_gpu_cand_reduce.py): runs the straight-line argmax reduction of the small-k
 * three-launch iteration (csrc/common.h, dzg_wave_best2_flat) on `ncases` independent cases and
 * returns one (r, k, h) per case.  Case c reads `width` consecutive candidates (r, k, h; k < 0: none)
 * starting at index c * width of the input arrays:
 *   form 0, width  64: one wave, candidate i in lane i;
 *   form 1, width 256: one wave, the four-slot form (k_chain.hip, chain_spec_reduce): candidate i in
 *                      slot i / 64 of lane i % 64, only the first count[c] of them take part;
 *   form 2, width 512: a workgroup of eight waves, thread i holds candidate i: the two-stage block form.
 * count is read for form 1 only.  No solve path calls it. */
int dzg_debug_cand_reduce(int32_t device, int32_t form, int64_t ncases, const double *r, const int32_t *k,
                          const double *h, const int32_t *count, double *out_r, int32_t *out_k,
                          double *out_h);

/* Test hook (tests/test_gpu_chain_instances.py): which instantiation of the chain kernels
 * (csrc/k_chain.hip, chain_pick) the launchers choose for m rows on `grid` workgroups, the host's
 * bound `k_bound` on the compact width for the batch (0: unknown), the launch's `fold` and `nrz`, a
 * column-sharded rank (`shard`), and k_chain_pre (`post` = 0) or k_chain_post (1).  Returns the
 * register-held FTRAN passes of the chosen kernel in bits 0..7 (16: the generic kernel), bit 8: it
 * has the 16-lanes-per-row arms only (k <= 512), bit 9: it has neither the fold head nor the path
 * for more than 256 candidates.  Pure host code: no device is touched. */
int dzg_debug_chain_instance(int32_t m, int32_t grid, int32_t k_bound, int32_t fold, int32_t nrz,
                             int32_t shard, int32_t post);

/* Test hooks of the small-k pricing pass run in k_chain_pre's tail (csrc/k_chain.hip, PRICE;
 * tests/test_gpu_price_in_pre.py).
 * dzg_debug_chain_price_counts: counts[0] = chain iterations this solver has enqueued with the pass
 * in k_chain_pre's tail (two launches), counts[1] = with the pass as a launch of its own (three).
 * dzg_debug_wk_mismatch: info[0] = the number of entries in which the kept compact copy of the eta
 * rows differs BITWISE from a fresh gather of W (t < neta, c < k; gathered into scratch on the
 * solver's stream), info[1] = whether the host held the copy valid (kept it) as it stood; clear_valid != 0 then drops the
 * flag, so that the next chain batch gathers the copy again.  DZG_E_ARG when the solver keeps no copy.
 * Call it between run() calls only, never while a batch is in flight: the scratch is the eta flush's
 * (which gathers again before it reads it), and the gather is sized for the full width.
 * dzg_debug_chain_price_rule: the host's rule (1: the pass runs in the tail) for m rows on `grid`
 * chain workgroups, the host's bound k_hint on the compact width, `tiles` column tiles, q nonbasic
 * positions, `small` = the fused small-k pass would run, `timed` = this slot's pricing pass is being
 * timed on its own.  Pure host code: no device is touched. */
int dzg_debug_chain_price_counts(dzg_solver *s, int64_t counts[2]);
int dzg_debug_wk_mismatch(dzg_solver *s, int32_t clear_valid, int64_t info[2]);
int dzg_debug_chain_price_rule(int32_t m, int32_t grid, int32_t k_hint, int32_t tiles, int64_t q,
                               int32_t small, int32_t timed);

/* Deterministic max-loc merge: largest ratio wins, lowest global position on ties --
 * the sequential first-wins rule of src/simplex.rs:432-435,456-459.  Returns the index
 * of the winning record, or -1 when every record is empty. */
int64_t dzg_merge_candidates(const dzg_candidate *cands, int64_t count);

#ifdef __cplusplus
}
#endif
#endif /* DANTZIG_AMD_H */
