// engine.hip -- host orchestration of the simplex iteration and the Level-1 C ABI.
//
// Replaces Simplex::solve (src/simplex.rs:332-343).  The reference recurses once per
// pivot on one CPU thread; here the host only enqueues kernels on one HIP stream.  All
// decisions live in the device control block (DzgCtl), so in FAST numerics the host
// enqueues `poll_interval` iterations back to back and reads the status word once per
// batch.  STRICT numerics needs O(m) launches per iteration anyway and reads the step kind
// after the status kernel to launch only the solves that iteration uses.
#include <dlfcn.h>

#include <chrono>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <limits>
#include <string>
#include <utility>
#include <algorithm>
#include <vector>

#include "common.h"
#include "duals.h"
#include "opts.h"
#include "ranging.h"
#include "rays.h"

static thread_local std::string g_err;

static int fail(int code, const std::string &msg)
{
    g_err = msg;
    return code;
}

#define HIP_OK(expr)                                                                      \
    do {                                                                                  \
        hipError_t e_ = (expr);                                                           \
        if (e_ != hipSuccess)                                                             \
            return fail(DZG_E_DEVICE, std::string(#expr) + ": " + hipGetErrorString(e_)); \
    } while (0)

extern "C" int dzg_abi_version(void) { return DZG_ABI_VERSION; }

extern "C" const char *dzg_last_error(void) { return g_err.c_str(); }

extern "C" const char *dzg_status_str(int s)
{
    switch (s) {
    case DZG_OPTIMAL: return "optimal";
    case DZG_UNBOUNDED: return "unbounded";
    case DZG_INFEASIBLE: return "infeasible";
    case DZG_ITER_LIMIT: return "iter_limit";
    case DZG_SINGULAR: return "singular";
    case DZG_PANIC: return "panic";
    case DZG_RUNNING: return "running";
    case DZG_NEAR_TIE: return "near_tie";
    case DZG_NODE_LIMIT: return "node_limit";
    case DZG_E_DEVICE: return "device_error";
    case DZG_E_ARG: return "bad_argument";
    case DZG_E_NOMEM: return "out_of_memory";
    default: return "unknown";
    }
}

extern "C" int dzg_device_count(void)
{
    int n = 0;
    if (hipGetDeviceCount(&n) != hipSuccess) return 0;
    return n;
}

extern "C" void dzg_opts_default(dzg_opts *o)
{
    std::memset(o, 0, sizeof(*o));
    o->numerics = DZG_NUMERICS_AUTO;
    o->price_kernel = DZG_PRICE_AUTO;
    o->device = 0;
    o->auto_strict_rows = 192;
    o->max_iter = 10000000;
    o->epsilon = 1e-12;
    o->log_capacity = -1;
    o->poll_interval = 32;
    o->profile = 0;
    o->world = 1;
    o->near_tie_action = DZG_NEAR_TIE_COUNT;
    o->auto_restart_rows = DZG_AUTO_STRICT_RESTART_ROWS;
    o->tie_tol = 1e-11;
}

struct dzg_solver {
    DzgDev d{};
    dzg_opts opts{};
    int numerics = DZG_NUMERICS_FAST;
    hipStream_t st = nullptr;
    bool own_stream = true;
    DzgCtl *h_ctl = nullptr; // pinned
    std::vector<void *> allocs;
    std::vector<double> c_host;
    std::vector<double> x0_host;   // the x the solve started with (rhs0 of the dual objective)
    std::vector<int> var_col_host; // column code of every variable
    double constant = 0.0;
    double solve_ms = 0.0;
    int since_flush = 0; // iterations enqueued since the eta file was last folded into Binv0
    // refactorisation workspace (FAST, opts.refactor_interval != 0)
    double *rfG = nullptr, *rfX = nullptr, *rfPn = nullptr, *rfTri = nullptr; // (rfPn: one 64-column panel,
                                                                 // column-major; rfTri: L11^-1, U11^-1 per panel)
    long long rf_ld = 0, rf_rows = 0; // leading dimension and rows of rfG / rfX as allocated
    int *rf_piv = nullptr, *rf_spos = nullptr, *rf_scode = nullptr, *rf_lpos = nullptr,
        *rf_lrow = nullptr, *rf_counts = nullptr, *rf_lslot = nullptr;
    long long since_refactor = 0;
    bool pending_refactor = false; // a warm start whose basic columns are not all on this device yet
                                   // (partitioned shards; replicate_matrix before the last upload):
                                   // the starting basis is factorised by the first run instead
    bool in_lockstep = false;      // inside dzg_shard_run_lockstep (the harness sums over the ranks)
    // STRICT: the O(m) launches of one basis solve, captured once and replayed (hipGraph)
    hipGraphExec_t g_solve[2] = {nullptr, nullptr}; // [0] B dx = a_j, [1] B^T v = e_p
    bool graphs_tried = false;
    int prof_slot = -1; // phase path: event slot of the iteration being enqueued (-1: none)
    int64_t refactors = 0;
    double *A_alloc = nullptr;  // device matrix as allocated (d.A points at column col0 inside it)
    long long cols_present = 0; // structural columns uploaded so far (replicate_matrix + a_is_block)
    std::vector<std::pair<int64_t, int64_t>> col_blocks; // ... as disjoint intervals [begin, end)
    double drift_trigger = 1e-9; // FAST health: disagreement of the two pivot elements that
                                 // triggers a refactorisation
    double max_err_life = 0.0; // largest ctl->max_pivot_err ever read (the device value restarts
                               // at every refactorisation)
    double state_drift = 0.0;  // carried x, xbar, z, zbar against the fresh inverse, at the last refactorisation
    // k_drift.hip: the data the state is recomputed from (solves that start on the slack basis of a
    // dense matrix on one GPU; nullptr otherwise) and scratch
    double *dr_b0 = nullptr, *dr_xb0 = nullptr, *dr_c = nullptr, *dr_cb = nullptr, *dr_agb = nullptr,
           *dr_agx = nullptr,
           *dr_part = nullptr, *dr_y = nullptr, *dr_dzy = nullptr, *dr_out = nullptr;
    // dzg_solver_duals (k_duals.hip): buffers of its own, reserved by the first call
    double *du_c = nullptr, *du_rhs0 = nullptr, *du_part = nullptr, *du_y = nullptr, *du_dzy = nullptr,
           *du_d = nullptr, *du_out = nullptr;
    int *du_codes = nullptr;
    DzgCtl *du_ctl = nullptr; // STRICT: a control block that reads DZG_RUNNING for the LU kernels
    // dzg_solver_ray (k_rays.hip): dx or dz, d by variable, the finish kernel's partial records
    double *ry_vec = nullptr, *ry_d = nullptr, *ry_part = nullptr, *ry_h = nullptr, *ry_res = nullptr;
    // dzg_solver_reoptimize (k_restart.hip), FAST: the new right-hand side in compact numbering
    double *ro_ag = nullptr;
    // dzg_solver_extend, FAST: the residual of the restart state's refinement step
    double *ro_res = nullptr;
    // dzg_solver_extend: ms the last call spent on the matrix, the refactorisation, the restart state
    double extend_ms[3] = {0.0, 0.0, 0.0};
    // FAST, dense, one GPU: the three-launch chain (k_chain.hip)
    unsigned long long *chain_bar = nullptr; // barrier counters (cleared only by chain_recover)
    unsigned long long *chain_dbg = nullptr; // DZG_CHAIN_DEBUG=1: phase clocks of workgroup 0
    int chain_grid = 0;                      // one workgroup per CU
    long long chain_kcap = DZG_CHAIN_AGCAP;  // compact width beyond which a batch runs as seven
                                             // launches (DZG_CHAIN_KCAP lowers it: tests)
    bool batch_chain = false;                // the batch in flight runs the chain
    bool chain_fold = true;                  // k_chain_post finishes the row-wise pricing pass itself
    bool chain_instances = true;             // the chain launchers choose among the kernels' instantiations
    // pricing in k_chain_pre's tail (k_chain.hip, PRICE): DZG_CHAIN_PRICE_FUSED=0, read once at creation,
    // turns it off for A/B runs.  wk_buf: the memory of the kept compact copy of the eta rows.  d.wk is
    // EITHER wk_buf -- the copy is the gather of W as the device holds it, and the chain kernels keep it
    // so -- OR NULL: no copy is kept (set by run_fast's gather before a batch that can price in the tail,
    // cleared for every other batch and wherever W, drow or neta change outside the chain)
    bool chain_price_fused = true;
    double *wk_buf = nullptr;
    int64_t chain_fused = 0, chain_unfused = 0; // chain iterations enqueued in two / in three launches
                                             // (DZG_CHAIN_INSTANCES=0, the A/B switch: generic always)
                                             // (DZG_CHAIN_NO_FOLD=1 at creation: the separate launch)
    int64_t chain_fallbacks = 0;             // barrier failures recovered from (chain_recover)
    long long chain_retry_iter = 0;          // the chain stays off until this pivot count
    // column sharding
    void *comm = nullptr;                  // ncclComm_t
    double *xsend = nullptr, *xrecv1 = nullptr, *xrecv2 = nullptr;
    // opts.shard_rows (k_rowshard.hip)
    long long xstride_max = 0;             // largest record (room for a row of m entries); d.xstride is
                                           // what the batch in flight sends
    const double *rs_recv1 = nullptr;      // records of exchange 1 (phase 3 of a dual step reads the
                                           // leaving row from them)
    int rs_slice = 0;                      // rows per rank
    double *rs_gsend = nullptr, *rs_grecv = nullptr; // x / xbar slices on their way to every rank
    // profiling
    std::vector<hipEvent_t> ev; // [batch slot][class][2]
    double kernel_ms[DZG_K_COUNT] = {};
    int64_t kernel_launches[DZG_K_COUNT] = {};
};

template <typename T> static int dev_alloc(dzg_solver *s, T **p, size_t count)
{
    void *q = nullptr;
    size_t bytes = sizeof(T) * (count ? count : 1);
    if (hipMalloc(&q, bytes) != hipSuccess)
        return fail(DZG_E_NOMEM, "hipMalloc of " + std::to_string(bytes) + " bytes failed");
    s->allocs.push_back(q);
    *p = static_cast<T *>(q);
    return 0;
}

#define TRY(expr)            \
    do {                     \
        int rc_ = (expr);    \
        if (rc_ != 0) return rc_; \
    } while (0)

// matrix_on_device: the structural block is already resident (dzg_solver_extend builds its successor
// from it), lp->a and the CSC arrays are not looked at
static int validate(const dzg_lp *lp, std::string &why, bool matrix_on_device = false)
{
    if (!lp) { why = "lp is NULL"; return 0; }
    if (lp->m < 0 || lp->n < lp->m || lp->n_struct < 0 || lp->n_struct > lp->n) { why = "bad sizes"; return 0; }
    if (lp->n >= (1ll << 31) - 64 || lp->m >= (1ll << 31) - 64) { why = "index range"; return 0; }
    if (lp->n_struct > 0 && lp->a && lp->lda < lp->m) { why = "lda"; return 0; }
    if (lp->n_struct > 0 && !lp->a && !matrix_on_device) {
        if (!lp->col_ptr || lp->col_ptr[0] != 0) { why = "neither a nor col_ptr"; return 0; }
        for (int64_t j = 0; j < lp->n_struct; ++j) {
            if (lp->col_ptr[j + 1] < lp->col_ptr[j]) { why = "col_ptr not monotone"; return 0; }
            for (int64_t e = lp->col_ptr[j]; e < lp->col_ptr[j + 1]; ++e) {
                if (!lp->row_idx || !lp->val || lp->row_idx[e] < 0 || lp->row_idx[e] >= lp->m ||
                    (e > lp->col_ptr[j] && lp->row_idx[e] <= lp->row_idx[e - 1])) {
                    why = "row_idx must ascend strictly inside a column";
                    return 0;
                }
            }
        }
    }
    const int64_t q = lp->n - lp->m;
    if ((lp->m > 0 && (!lp->basis || !lp->x)) || (q > 0 && (!lp->nonbasis || !lp->z)) || (lp->n > 0 && !lp->c)) { why = "NULL state vector"; return 0; }
    if (!lp->var_col && lp->n != lp->n_struct + lp->m) { why = "var_col == NULL needs n == n_struct + m"; return 0; }
    std::vector<char> seen((size_t)lp->n, 0);
    for (int64_t k = 0; k < lp->n; ++k) {
        int64_t v = k < lp->m ? lp->basis[k] : lp->nonbasis[k - lp->m];
        if (v < 0 || v >= lp->n || seen[(size_t)v]) { why = "basis/nonbasis is not a partition of 0..n-1"; return 0; }
        seen[(size_t)v] = 1;
    }
    if (lp->var_col) {
        for (int64_t v = 0; v < lp->n; ++v) {
            int64_t c = lp->var_col[v];
            if (c >= lp->n_struct || c < -lp->m) { why = "var_col out of range"; return 0; }
        }
    }
    return 1;
}

// For the other translation units of the library (k_batch.hip, model.cpp): the same checks and
// the same error slot as the entry points here.
int dzg_set_error(int code, const std::string &msg) { return fail(code, msg); }
int dzg_lp_valid(const dzg_lp *lp, std::string &why) { return validate(lp, why); }

// ---- RCCL, loaded lazily: single-GPU users never need librccl ------------------------
namespace {
struct NcclUniqueId { char internal[128]; };
struct Rccl {
    void *handle = nullptr;
    int (*GetUniqueId)(NcclUniqueId *) = nullptr;
    int (*CommInitRank)(void **, int, NcclUniqueId, int) = nullptr;
    int (*AllGather)(const void *, void *, size_t, int, void *, hipStream_t) = nullptr;
    int (*AllReduce)(const void *, void *, size_t, int, int, void *, hipStream_t) = nullptr;
    int (*CommDestroy)(void *) = nullptr;
    int (*CommCount)(void *, int *) = nullptr;
    const char *(*GetErrorString)(int) = nullptr;
    bool ok = false;
};
Rccl &rccl()
{
    static Rccl r;
    if (r.handle || r.ok) return r;
    // ROCm's own librccl first, by path: it binds to the same libamdhip64 as this library.  A
    // bare soname could resolve to a copy bundled with a Python package (its own HIP runtime).
    const char *names[] = {"/opt/rocm/lib/librccl.so.1", "/opt/rocm/lib/librccl.so", "librccl.so.1",
                           "librccl.so"};
    for (const char *n : names) {
        r.handle = dlopen(n, RTLD_NOW | RTLD_LOCAL);
        if (r.handle) break;
    }
    if (!r.handle) return r;
    r.GetUniqueId = (int (*)(NcclUniqueId *))dlsym(r.handle, "ncclGetUniqueId");
    r.CommInitRank = (int (*)(void **, int, NcclUniqueId, int))dlsym(r.handle, "ncclCommInitRank");
    r.AllGather = (int (*)(const void *, void *, size_t, int, void *, hipStream_t))dlsym(r.handle, "ncclAllGather");
    r.AllReduce = (int (*)(const void *, void *, size_t, int, int, void *, hipStream_t))dlsym(r.handle, "ncclAllReduce");
    r.CommDestroy = (int (*)(void *))dlsym(r.handle, "ncclCommDestroy");
    r.CommCount = (int (*)(void *, int *))dlsym(r.handle, "ncclCommCount");
    r.GetErrorString = (const char *(*)(int))dlsym(r.handle, "ncclGetErrorString");
    r.ok = r.GetUniqueId && r.CommInitRank && r.AllGather && r.CommDestroy;
    return r;
}
const int kNcclFloat64 = 8;
const int kNcclSum = 0;
} // namespace

static void shard_comm_destroy(dzg_solver *s);
static int shard_buffers(dzg_solver *s);
static int refactor_now(dzg_solver *s, bool at_end = false);
static int refactor_workspace(dzg_solver *s);
static bool partitioned(const dzg_solver *s);

// DZG_CHAIN_DEBUG=1: where workgroup 0 of the chain kernels spent its time (stderr, at destroy)
static void chain_debug_report(dzg_solver *s)
{
    unsigned long long h[16 * DZG_STAMP_SLOTS];
    if (hipMemcpy(h, s->chain_dbg, sizeof(h), hipMemcpyDeviceToHost) != hipSuccess) return;
    // (the pricing kernel's stages: control block | row list | rows | finish)
    static const char *names[DZG_SITE_SLOT] = {"k_chain_pre  primal", "k_chain_pre  dual  ", "k_chain_post primal",
                                                 "k_chain_post dual  ", "k_price_rows_small "};
    for (int slot = 0; slot < DZG_SITE_SLOT; ++slot) {
        const double n = (double)h[16 * slot + 15];
        if (n <= 0) continue;
        std::fprintf(stderr, "[chain] %s x%-8.0f us per stage:", names[slot], n);
        double tot = 0;
        for (int st = 0; st < 15; ++st) {
            if (!h[16 * slot + st]) continue;
            const double us = (double)h[16 * slot + st] / n / 100.0; // 100 MHz clock
            tot += us;
            std::fprintf(stderr, " %d:%.2f", st, us);
        }
        std::fprintf(stderr, "  sum %.2f\n", tot);
    }
    // the reduction sites (ChainStamps::site): us per visit; the last two since the kernel's start
    static const char *sites[DZG_SITE_COUNT] = {"pre first-pivot reduce", "pre fast_status", "pre row chain_best",
                                                "pre reduce_sc1", "post ratio reduce", "post chain_best bx",
                                                "post chain_best bz", "price publish", "post dual books end",
                                                "post dual last stamp"};
    for (int i = 0; i < DZG_SITE_COUNT; ++i) {
        const double n = (double)h[16 * (DZG_SITE_SLOT + 1) + i];
        if (n <= 0) continue;
        std::fprintf(stderr, "[chain] site %-24s x%-8.0f %.2f us\n", sites[i], n,
                     (double)h[16 * DZG_SITE_SLOT + i] / n / 100.0);
    }
}

extern "C" void dzg_solver_destroy(dzg_solver *s)
{
    if (!s) return;
    if (s->chain_dbg) chain_debug_report(s);
    shard_comm_destroy(s);
    for (hipGraphExec_t g : s->g_solve)
        if (g) hipGraphExecDestroy(g);
    for (hipEvent_t e : s->ev) hipEventDestroy(e);
    for (void *p : s->allocs) hipFree(p);
    if (s->h_ctl) hipHostFree(s->h_ctl);
    if (s->st && s->own_stream) hipStreamDestroy(s->st);
    delete s;
}

// columns [c0, c1) of the structural block into their slots of a replicated device matrix;
// -0.0 entries become +0.0 like everywhere else (the reference's CSC drops exact zeros)
static int upload_columns(dzg_solver *s, int64_t c0, int64_t c1, const double *a, int64_t lda)
{
    const DzgDev &d = s->d;
    if (c1 <= c0 || d.m == 0) return 0;
    const int64_t cnt = c1 - c0;
    double *dst = s->A_alloc + (size_t)c0 * (size_t)d.lda;
    bool has_negzero = false;
    for (int64_t j = 0; j < cnt && !has_negzero; ++j)
        for (int64_t i = 0; i < d.m; ++i) {
            const double val = a[j * lda + i];
            if (val == 0.0 && std::signbit(val)) { has_negzero = true; break; }
        }
    if (!has_negzero) {
        HIP_OK(hipMemcpy2DAsync(dst, sizeof(double) * d.lda, a, sizeof(double) * lda,
                                sizeof(double) * d.m, (size_t)cnt, hipMemcpyHostToDevice, s->st));
    } else {
        std::vector<double> tmp((size_t)d.m * (size_t)cnt);
        for (int64_t j = 0; j < cnt; ++j)
            for (int64_t i = 0; i < d.m; ++i) {
                const double val = a[j * lda + i];
                tmp[(size_t)(j * d.m + i)] = (val == 0.0) ? 0.0 : val;
            }
        HIP_OK(hipMemcpy2DAsync(dst, sizeof(double) * d.lda, tmp.data(), sizeof(double) * d.m,
                                sizeof(double) * d.m, (size_t)cnt, hipMemcpyHostToDevice, s->st));
        HIP_OK(hipStreamSynchronize(s->st)); // (tmp is a local: the copy must have read it)
    }
    HIP_OK(hipStreamSynchronize(s->st)); // the caller may reuse its buffer
    s->cols_present += cnt;
    return 0;
}

extern "C" int dzg_solver_upload_columns(dzg_solver *s, int64_t col_begin, int64_t col_end,
                                         const double *a, int64_t lda)
{
    if (!s || !a || !s->d.repl) return fail(DZG_E_ARG, "upload_columns: a solver with replicate_matrix");
    if (col_begin < 0 || col_end > s->d.ns || col_begin > col_end || lda < s->d.m ||
        (col_begin < s->d.col1 && col_end > s->d.col0))
        return fail(DZG_E_ARG, "upload_columns: [col_begin, col_end) must lie outside the rank's own block");
    // every column exactly once: a block handed over twice would leave another one unset (zeros)
    // behind a column count that looks complete
    for (const auto &blk : s->col_blocks)
        if (col_begin < blk.second && col_end > blk.first)
            return fail(DZG_E_ARG, "upload_columns: columns [" + std::to_string(col_begin) + ", " +
                                       std::to_string(col_end) + ") overlap a block that is already present");
    HIP_OK(hipSetDevice(s->opts.device));
    TRY(upload_columns(s, col_begin, col_end, a, lda));
    if (col_end > col_begin) s->col_blocks.emplace_back(col_begin, col_end);
    return 0;
}

// dzg_solver_extend, dzg_solver_remove: the successor's matrix comes from the device (lp->a is NULL and
// is not a request for CSC storage; lp->x is the right-hand side by row).  With `ext`: the resident
// block of `old`, re-laid for the new leading dimension, and the rows and columns of `ext`.  With
// `keep_rows` / `keep_cols` (ascending; keep_rows NULL: every row): those rows and columns of the
// resident block, gathered.
struct SuccessorSrc {
    const dzg_solver *old;
    const dzg_extend *ext;
    const std::vector<int> *keep_rows;
    const std::vector<int> *keep_cols;
};
static int successor_fill_matrix(dzg_solver *s, const SuccessorSrc &src);

static double ms_since(std::chrono::steady_clock::time_point t0)
{
    return std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
}

static int solver_create(const dzg_lp *lp, const dzg_opts *opts_in, dzg_solver **out, const SuccessorSrc *src)
{
    if (!out) return fail(DZG_E_ARG, "out is NULL");
    *out = nullptr;
    std::string why;
    if (!validate(lp, why, src != nullptr)) return fail(DZG_E_ARG, "invalid dzg_lp: " + why);
    dzg_opts o = dzg_opts_resolved(opts_in);

    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || ndev <= 0)
        return fail(DZG_E_DEVICE, "no HIP device visible: dantzig_amd has no CPU path");
    if (o.device < 0 || o.device >= ndev) return fail(DZG_E_ARG, "opts.device out of range");
    HIP_OK(hipSetDevice(o.device));

    dzg_solver *s = new dzg_solver();
    s->opts = o;
    struct Guard { dzg_solver *s; ~Guard() { if (s) dzg_solver_destroy(s); } } guard{s};
    if (o.stream) {
        s->st = (hipStream_t)o.stream;
        s->own_stream = false;
    } else {
        HIP_OK(hipStreamCreate(&s->st));
    }
    HIP_OK(hipHostMalloc((void **)&s->h_ctl, sizeof(DzgCtl)));

    DzgDev &d = s->d;
    const int m = (int)lp->m, n = (int)lp->n, ns = (int)lp->n_struct, q = n - m;
    d.m = m; d.n = n; d.ns = ns; d.q = q;
    // 16-B aligned columns; on tall matrices a column stride that is not a multiple of a large
    // power of two spreads the 16 concurrent column streams of a wave over more HBM channels
    // (+1.5-2 % on the pricing pass, profiles/r01_price_microbench_*.txt)
    d.lda = ((long long)m + 15) / 16 * 16 + (m >= 2048 ? 272 : 0);
    if (d.lda == 0) d.lda = 16;
    d.eps = o.epsilon;
    // FTRAN's loads of Binv0's rows (k > 512): nontemporal, eight steps in flight -- 125.4 -> 102.9 us
    // for k_chain_pre at k = 7 700 -- from the width on at which the inverse outgrows 1.5 x the Infinity
    // Cache; below it plain loads are faster (profiles/r04_ftran_row_loads_ab.txt)
    {
        const double kk = 384e6 / (8.0 * (double)(lp->m > 0 ? lp->m : 1));
        d.ftran_nt_k = kk > 2e9 ? 2000000000 : (int)kk;
        if (d.ftran_nt_k < 513) d.ftran_nt_k = 513;
    }
    d.beta_split = 1;
    if (const char *bs = std::getenv("DZG_CHAIN_BETA_SPLIT")) d.beta_split = bs[0] != '0';
    d.world = o.world > 1 ? o.world : 1;
    d.rank = d.world > 1 ? o.rank : 0;
    d.col0 = 0;
    d.col1 = ns;
    if (d.world > 1) {
        if (o.rank < 0 || o.rank >= o.world || o.col_begin < 0 || o.col_end > ns ||
            o.col_begin > o.col_end)
            return fail(DZG_E_ARG, "opts.rank / col_begin / col_end");
        d.col0 = (int)o.col_begin;
        d.col1 = (int)o.col_end;
    }
    const int nloc = d.col1 - d.col0; // structural columns this rank prices
    // dense + replicate_matrix: all ns columns are resident, the exchange carries headers only
    d.repl = (d.world > 1 && o.replicate_matrix && lp->a) ? 1 : 0;
    d.xstride = d.repl ? 8 : 8 + ((long long)m + 7) / 8 * 8;
    const double *a_host = !lp->a ? nullptr
                           : (o.a_is_block && d.world > 1) ? lp->a
                                                           : lp->a + (size_t)d.col0 * (size_t)lp->lda;

    d.csc = (ns > 0 && !lp->a && !src) ? 1 : 0;
    // opts.shard_rows: the basis side sharded by rows as well (k_rowshard.hip)
    d.rs = 0;
    d.rs_r0 = 0;
    d.rs_r1 = m;
    d.rs_mcol = 0;
    if (o.shard_rows && d.world > 1) {
        if (d.csc) return fail(DZG_E_ARG, "opts.shard_rows needs a dense matrix");
        if (o.price_kernel != DZG_PRICE_AUTO && o.price_kernel != DZG_PRICE_TREE)
            return fail(DZG_E_ARG, "opts.shard_rows prices with the AUTO / TREE kernels (every rank "
                                   "re-derives dz of the entering column in their summation order)");
        d.rs = 1;
        s->rs_slice = (int)((((long long)m + d.world - 1) / d.world + 15) / 16 * 16);
        if (s->rs_slice < 16) s->rs_slice = 16;
        const long long r0 = (long long)d.rank * s->rs_slice;
        d.rs_r0 = (int)(r0 < m ? r0 : m);
        d.rs_r1 = (int)(r0 + s->rs_slice < m ? r0 + s->rs_slice : m);
        d.rs_mcol = d.repl ? 0 : ((long long)m + 15) / 16 * 16;
        s->xstride_max = DZG_RS_COL + d.rs_mcol + ((long long)m + 2 + 15) / 16 * 16;
        d.xstride = s->xstride_max;
    }
    if (d.csc) {
        // sparse mode: the owned columns stay CSC on the device (12 bytes per nonzero); explicit
        // zeros are dropped like the reference's From<&Matrix> for CscMatrix (src/linalg.rs:261)
        std::vector<long long> cp((size_t)nloc + 1, 0);
        std::vector<int> ri;
        std::vector<double> cv;
        for (int j = 0; j < nloc; ++j) {
            for (int64_t e = lp->col_ptr[d.col0 + j]; e < lp->col_ptr[d.col0 + j + 1]; ++e)
                if (lp->val[e] != 0.0) {
                    ri.push_back((int)lp->row_idx[e]);
                    cv.push_back(lp->val[e]);
                }
            cp[(size_t)j + 1] = (long long)ri.size();
        }
        long long *dcp; int *dri; double *dcv;
        TRY(dev_alloc(s, &dcp, cp.size())); TRY(dev_alloc(s, &dri, ri.size() + 1));
        TRY(dev_alloc(s, &dcv, cv.size() + 1));
        HIP_OK(hipMemcpy(dcp, cp.data(), sizeof(long long) * cp.size(), hipMemcpyHostToDevice));
        if (!ri.empty()) {
            HIP_OK(hipMemcpy(dri, ri.data(), sizeof(int) * ri.size(), hipMemcpyHostToDevice));
            HIP_OK(hipMemcpy(dcv, cv.data(), sizeof(double) * cv.size(), hipMemcpyHostToDevice));
        }
        d.cptr = dcp; d.ridx = dri; d.cval = dcv;
        // One GPU, FAST numerics: the basis lives on its k x k structural block (k_sparse.hip),
        // which needs row access to the matrix as well: a CSR copy, columns ascending in a row.
        if (d.world == 1 && dzg_opts_numerics(o, m) == DZG_NUMERICS_FAST && m <= (1 << 20)) {
            d.spb = 1;
            std::vector<long long> rp((size_t)m + 1, 0);
            for (int r : ri) rp[(size_t)r + 1] += 1;
            for (int r = 0; r < m; ++r) rp[(size_t)r + 1] += rp[(size_t)r];
            std::vector<int> ci(ri.size());
            std::vector<double> rv(ri.size());
            std::vector<long long> fill(rp.begin(), rp.end() - 1);
            for (int j = 0; j < nloc; ++j) // columns ascending => ascending inside every row
                for (long long e = cp[(size_t)j]; e < cp[(size_t)j + 1]; ++e) {
                    const long long at = fill[(size_t)ri[(size_t)e]]++;
                    ci[(size_t)at] = j;
                    rv[(size_t)at] = cv[(size_t)e];
                }
            long long *drp; int *dci; double *drv;
            TRY(dev_alloc(s, &drp, rp.size())); TRY(dev_alloc(s, &dci, ci.size() + 1));
            TRY(dev_alloc(s, &drv, rv.size() + 1));
            HIP_OK(hipMemcpy(drp, rp.data(), sizeof(long long) * rp.size(), hipMemcpyHostToDevice));
            if (!ci.empty()) {
                HIP_OK(hipMemcpy(dci, ci.data(), sizeof(int) * ci.size(), hipMemcpyHostToDevice));
                HIP_OK(hipMemcpy(drv, rv.data(), sizeof(double) * rv.size(), hipMemcpyHostToDevice));
            }
            d.rptr = drp; d.cidx = dci; d.rval = drv;
            TRY(dev_alloc(s, &d.bcnt, (size_t)(m ? m : 1)));
            TRY(dev_alloc(s, &d.bcol, ci.size() + 1));
            TRY(dev_alloc(s, &d.bval, rv.size() + 1));
            // live-entry lists of the columns (k_price_csc_rl); the reference-order kernel and the
            // A/B switch DZG_SP_PRICE_FULL=1 price over every stored entry instead
            const char *full = std::getenv("DZG_SP_PRICE_FULL");
            if (o.price_kernel != DZG_PRICE_SEQ && !(full && full[0] == '1')) {
                TRY(dev_alloc(s, &d.lcnt, (size_t)(ns ? ns : 1)));
                TRY(dev_alloc(s, &d.lent, ri.size() + 1));
                TRY(dev_alloc(s, &d.rl_work, (size_t)DZG_RL_WORK_SLOTS));
                HIP_OK(hipMemsetAsync(d.rl_work, 0, sizeof(unsigned long long) * DZG_RL_WORK_SLOTS, s->st));
            }
        }
    }
    // --- constraint matrix: column-major, zero-padded to lda rows (16-B aligned columns)
    double *A = nullptr;
    const int ndense = d.csc ? 0 : nloc;
    const int nmem = d.csc ? 0 : (d.repl ? ns : nloc);       // columns held in HBM
    const long long mem0 = d.repl ? 0 : d.col0;              // first of them
    double *A_alloc = nullptr;
    TRY(dev_alloc(s, &A_alloc, (size_t)d.lda * (size_t)(nmem ? nmem : 1)));
    HIP_OK(hipMemsetAsync(A_alloc, 0, sizeof(double) * (size_t)d.lda * (size_t)(nmem ? nmem : 1), s->st));
    A = A_alloc + (size_t)(d.col0 - mem0) * (size_t)d.lda;   // column col0: kernels index from it
    s->A_alloc = A_alloc;
    s->cols_present = d.repl ? nloc : ns;
    if (src) {
        TRY(successor_fill_matrix(s, *src));
    } else if (ndense > 0 && m > 0) {
        // the reference's CSC drops exact zeros (src/linalg.rs:261), so -0.0 entries act as +0.0
        bool has_negzero = false;
        for (int64_t j = 0; j < nloc && !has_negzero; ++j)
            for (int64_t i = 0; i < m; ++i) {
                const double val = a_host[j * lp->lda + i];
                if (val == 0.0 && std::signbit(val)) { has_negzero = true; break; }
            }
        if (!has_negzero) {
            HIP_OK(hipMemcpy2DAsync(A, sizeof(double) * d.lda, a_host, sizeof(double) * lp->lda,
                                    sizeof(double) * m, nloc, hipMemcpyHostToDevice, s->st));
        } else {
            std::vector<double> tmp((size_t)m * nloc);
            for (int64_t j = 0; j < nloc; ++j)
                for (int64_t i = 0; i < m; ++i) {
                    const double val = a_host[j * lp->lda + i];
                    tmp[(size_t)(j * m + i)] = (val == 0.0) ? 0.0 : val;
                }
            HIP_OK(hipMemcpy2DAsync(A, sizeof(double) * d.lda, tmp.data(), sizeof(double) * m,
                                    sizeof(double) * m, nloc, hipMemcpyHostToDevice, s->st));
            HIP_OK(hipStreamSynchronize(s->st));
        }
    }
    d.A = A;
    if (d.repl && !o.a_is_block && ns > nloc) {
        // lp->a is the whole matrix: the other ranks' columns come from it right away
        if (d.col0 > 0) {
            TRY(upload_columns(s, 0, d.col0, lp->a, lp->lda));
            s->col_blocks.emplace_back(0, d.col0);
        }
        if (d.col1 < ns) {
            TRY(upload_columns(s, d.col1, ns, lp->a + (size_t)d.col1 * (size_t)lp->lda, lp->lda));
            s->col_blocks.emplace_back(d.col1, ns);
        }
    }

    // --- index maps
    std::vector<int> var_col((size_t)(n ? n : 1));
    for (int v = 0; v < n; ++v)
        var_col[v] = lp->var_col ? (int)lp->var_col[v] : (v < ns ? v : -1 - (v - ns));
    std::vector<int> basis((size_t)(m ? m : 1)), nonbasis((size_t)(q ? q : 1));
    long long nb_struct = 0;
    for (int p = 0; p < m; ++p) basis[p] = (int)lp->basis[p];
    for (int k = 0; k < q; ++k) {
        nonbasis[k] = (int)lp->nonbasis[k];
        if (var_col[nonbasis[k]] >= 0) ++nb_struct;
    }
    int *d_var_col, *d_basis, *d_nonbasis;
    TRY(dev_alloc(s, &d_var_col, (size_t)n));
    TRY(dev_alloc(s, &d_basis, (size_t)m));
    TRY(dev_alloc(s, &d_nonbasis, (size_t)q));
    HIP_OK(hipMemcpyAsync(d_var_col, var_col.data(), sizeof(int) * (size_t)(n ? n : 1), hipMemcpyHostToDevice, s->st));
    HIP_OK(hipMemcpyAsync(d_basis, basis.data(), sizeof(int) * (size_t)(m ? m : 1), hipMemcpyHostToDevice, s->st));
    HIP_OK(hipMemcpyAsync(d_nonbasis, nonbasis.data(), sizeof(int) * (size_t)(q ? q : 1), hipMemcpyHostToDevice, s->st));
    d.var_col = d_var_col; d.basis = d_basis; d.nonbasis = d_nonbasis;

    // --- state vectors: x = rhs, z = -c_N, xbar = zbar = 1 (src/simplex.rs:190-205)
    TRY(dev_alloc(s, &d.x, (size_t)m)); TRY(dev_alloc(s, &d.xbar, (size_t)m));
    TRY(dev_alloc(s, &d.z, (size_t)q)); TRY(dev_alloc(s, &d.zbar, (size_t)q));
    TRY(dev_alloc(s, &d.dx, (size_t)m)); TRY(dev_alloc(s, &d.dz, (size_t)q));
    TRY(dev_alloc(s, &d.v, (size_t)m + 2)); TRY(dev_alloc(s, &d.acol, (size_t)m));
    std::vector<double> ones((size_t)((m > q ? m : q) + 1), 1.0);
    if (m > 0) {
        HIP_OK(hipMemcpyAsync(d.x, lp->x, sizeof(double) * m, hipMemcpyHostToDevice, s->st));
        HIP_OK(hipMemcpyAsync(d.xbar, lp->xbar ? lp->xbar : ones.data(), sizeof(double) * m,
                              hipMemcpyHostToDevice, s->st));
    }
    if (q > 0) {
        HIP_OK(hipMemcpyAsync(d.z, lp->z, sizeof(double) * q, hipMemcpyHostToDevice, s->st));
        HIP_OK(hipMemcpyAsync(d.zbar, lp->zbar ? lp->zbar : ones.data(), sizeof(double) * q,
                              hipMemcpyHostToDevice, s->st));
    }
    HIP_OK(hipMemsetAsync(d.v, 0, sizeof(double) * ((size_t)m + 2), s->st));
    s->c_host.assign(lp->c, lp->c + n);
    if (m > 0) {
        // rhs0, the right-hand side of [A | I] x = rhs0 (the dual objective, the value of a Farkas
        // ray): the starting x itself where every slack starts at the position of its own row
        // (Simplex::new); B0 x0 for any other start (warm start, resumed solve), where x0 is indexed
        // by position and says nothing about a row on its own.  A rank that holds only a block of
        // the columns cannot form it and keeps x0 (such solvers return carried duals and no rays).
        s->x0_host.assign(lp->x, lp->x + m);
        bool own_rows = true;
        for (int p = 0; p < m; ++p)
            if (var_col[basis[p]] != -1 - p) own_rows = false;
        if (!own_rows && !(o.a_is_block && d.world > 1) && !src) {
            std::vector<double> rhs((size_t)m, 0.0);
            for (int p = 0; p < m; ++p) {
                const int code = var_col[basis[p]];
                const double xp = lp->x[p];
                if (code < 0) {
                    rhs[(size_t)(-1 - code)] += xp;
                } else if (lp->a) {
                    const double *col = lp->a + (size_t)code * (size_t)lp->lda;
                    for (int r = 0; r < m; ++r) rhs[(size_t)r] = std::fma(col[r], xp, rhs[(size_t)r]);
                } else {
                    for (int64_t e = lp->col_ptr[code]; e < lp->col_ptr[code + 1]; ++e)
                        rhs[(size_t)lp->row_idx[e]] = std::fma(lp->val[e], xp, rhs[(size_t)lp->row_idx[e]]);
                }
            }
            s->x0_host.swap(rhs);
        }
    }
    s->var_col_host.assign(var_col.begin(), var_col.begin() + n);
    s->constant = lp->constant;

    // --- pivot log
    long long cap = o.log_capacity >= 0 ? o.log_capacity : (o.max_iter < (1ll << 22) ? o.max_iter : (1ll << 22));
    d.log_cap = cap;
    TRY(dev_alloc(s, &d.log_kind, (size_t)cap)); TRY(dev_alloc(s, &d.log_enter, (size_t)cap));
    TRY(dev_alloc(s, &d.log_leave, (size_t)cap)); TRY(dev_alloc(s, &d.log_mu, (size_t)cap));
    TRY(dev_alloc(s, &d.log_margin, (size_t)cap));

    // --- numerics
    s->numerics = dzg_opts_numerics(o, m);
    if (s->numerics != DZG_NUMERICS_STRICT && s->numerics != DZG_NUMERICS_FAST)
        return fail(DZG_E_ARG, "opts.numerics");
    if (d.world > 1 && s->numerics != DZG_NUMERICS_FAST)
        return fail(DZG_E_ARG, "column sharding needs FAST numerics");
    TRY(dev_alloc(s, &d.ctl, 1));
    DzgCtl c0;
    std::memset(&c0, 0, sizeof(c0));
    c0.status = DZG_RUNNING;
    c0.iter_stop = o.max_iter;
    c0.enter_pos = c0.leave_pos = -1;
    c0.del_ce = c0.del_last = -1;
    c0.rl_listed = -1;
    c0.nb_struct = nb_struct;
    c0.tie_tol = c0.tau = o.tie_tol;
    c0.margin = c0.min_margin = std::numeric_limits<double>::infinity();
    c0.first_near_tie = c0.tie_skip_iter = -1;
    c0.tie_mode = o.near_tie_action == DZG_NEAR_TIE_STOP ? 1 : 0;
    HIP_OK(hipMemcpyAsync(d.ctl, &c0, sizeof(c0), hipMemcpyHostToDevice, s->st));
    *s->h_ctl = c0;

    if (s->numerics == DZG_NUMERICS_FAST) {
        // the slack basis of Simplex::new needs no factorisation (Binv0 starts empty); any other
        // starting basis (warm start) is factorised on the device before the first iteration
        bool slack_basis = true;
        for (int p = 0; p < m; ++p)
            if (var_col[basis[p]] >= 0) slack_basis = false;
        if (!slack_basis) {
            // a column-sharded rank that does not hold every basic column yet (partitioned storage, or
            // replicate_matrix before dzg_solver_upload_columns has run) factorises the starting
            // basis at its first run, where the ranks can exchange their columns' shares
            if (d.world > 1 && !(d.repl && s->cols_present == ns)) s->pending_refactor = true;
            if (o.refactor_interval == 0) o.refactor_interval = -1; // reserve the workspace
            s->opts.refactor_interval = o.refactor_interval;
        }
        const bool needs_initial_refactor = !slack_basis && !s->pending_refactor;
        if (slack_basis && d.world == 1 && !d.csc && m > 0 && q > 0 && !src) {
            // the state a refactorisation can be checked against (k_drift.hip): b = the starting x,
            // xbar0 = the starting xbar, c, and cbar: the c whose reduced costs zbar is (-zbar0 on the
            // starting nonbasics, 0 on the slacks), as c is for z
            TRY(dev_alloc(s, &s->dr_b0, (size_t)m + 2)); TRY(dev_alloc(s, &s->dr_xb0, (size_t)m + 2));
            TRY(dev_alloc(s, &s->dr_c, (size_t)n)); TRY(dev_alloc(s, &s->dr_cb, (size_t)n));
            std::vector<double> cbar((size_t)n, 0.0);
            for (int k = 0; k < q; ++k) cbar[(size_t)nonbasis[k]] = -(lp->zbar ? lp->zbar[k] : 1.0);
            HIP_OK(hipMemcpyAsync(s->dr_b0, lp->x, sizeof(double) * m, hipMemcpyHostToDevice, s->st));
            HIP_OK(hipMemcpyAsync(s->dr_xb0, lp->xbar ? lp->xbar : ones.data(), sizeof(double) * m,
                                  hipMemcpyHostToDevice, s->st));
            HIP_OK(hipMemcpyAsync(s->dr_c, lp->c, sizeof(double) * n, hipMemcpyHostToDevice, s->st));
            HIP_OK(hipMemcpyAsync(s->dr_cb, cbar.data(), sizeof(double) * n, hipMemcpyHostToDevice, s->st));
            HIP_OK(hipStreamSynchronize(s->st)); // (cbar is a local)
        }
        // row stride: not a multiple of a large power of two, so that the first k columns of
        // consecutive rows do not all land on the same HBM channels
        // row stride of the compact inverse: 160 doubles past a multiple of 512 (1 280 bytes past a
        // multiple of 4 KB).  FTRAN streams 2 048 rows at once, one wave each; at k = 7 700 of m = 8 192
        // the launch takes 102.4 us with m + 32, 110.7 with m + 64, 97.7 with m + 160 (or + 288, + 544),
        // 101.0 with m + 1 056 (profiles/r04_ftran_row_loads_ab.txt); DZG_LDB_PAD=<doubles> for A/B
        {
            const long long base = ((long long)m + 15) / 16 * 16;
            long long pad = ((160 - base % 512) % 512 + 512) % 512;
            if (pad < 32) pad += 512;
            if (const char *e = std::getenv("DZG_LDB_PAD")) pad = std::atoi(e) / 16 * 16;
            d.ldb = base + pad;
        }
        d.ldw = ((long long)m + 15) / 16 * 16 + 64;
        {
            // a row-sharded basis side keeps its own rows of Binv0 only; the kernels address rows by
            // their global index, so d.binv points rs_r0 rows BEFORE the allocation (never
            // dereferenced outside [rs_r0, rs_r1): every kernel that touches Binv0 takes the range)
            const size_t rows_kept = d.rs ? (size_t)(d.rs_r1 - d.rs_r0) : (size_t)m;
            double *binv_alloc = nullptr;
            TRY(dev_alloc(s, &binv_alloc, (rows_kept ? rows_kept : 1) * (size_t)d.ldb));
            d.binv = binv_alloc - (d.rs ? (long long)d.rs_r0 * d.ldb : 0);
        }
        TRY(dev_alloc(s, &d.drow, (size_t)m)); TRY(dev_alloc(s, &d.dslot, (size_t)m));
        TRY(dev_alloc(s, &d.U, (size_t)d.ldw * DZG_RMAX));
        TRY(dev_alloc(s, &d.W, (size_t)d.ldw * DZG_RMAX));
        TRY(dev_alloc(s, &d.Wc, (size_t)d.ldw * DZG_RMAX));
        TRY(dev_alloc(s, &d.ag, (size_t)m + 2)); TRY(dev_alloc(s, &d.beta, (size_t)DZG_RMAX));
        TRY(dev_alloc(s, &d.beta_part, (size_t)4 * DZG_RMAX));
        TRY(dev_alloc(s, &d.plist, (size_t)q)); TRY(dev_alloc(s, &d.pslot, (size_t)q));
        TRY(dev_alloc(s, &d.bcode, (size_t)m)); TRY(dev_alloc(s, &d.nbcode, (size_t)q));
        TRY(dev_alloc(s, &d.pcode, (size_t)q));
        if (!d.csc) TRY(dev_alloc(s, &d.cpos, (size_t)(d.col1 > d.col0 ? d.col1 - d.col0 : 1)));
        const size_t np = 4096;
        TRY(dev_alloc(s, &d.fpx_r, np)); TRY(dev_alloc(s, &d.fpz_r, np));
        TRY(dev_alloc(s, &d.rx_r, np)); TRY(dev_alloc(s, &d.rz_r, np));
        TRY(dev_alloc(s, &d.fpx_k, np)); TRY(dev_alloc(s, &d.fpz_k, np));
        TRY(dev_alloc(s, &d.rx_k, np)); TRY(dev_alloc(s, &d.rz_k, np));
        TRY(dev_alloc(s, &d.fpx_h, np)); TRY(dev_alloc(s, &d.fpz_h, np));
        TRY(dev_alloc(s, &d.rx_h, np)); TRY(dev_alloc(s, &d.rz_h, np));
        if (o.refactor_interval != 0) TRY(refactor_workspace(s));
        // (the CU count: both barrier-synchronised iterations below fit their grids to it)
        hipDeviceProp_t prop;
        HIP_OK(hipGetDeviceProperties(&prop, o.device));
        const int cus = prop.multiProcessorCount > 0 ? prop.multiProcessorCount : 1;
        if (d.spb && !o.seven_launches) {
            // the four-launch iteration (k_sp_pre / k_sp_mid, k_sparse.hip) synchronises its phases with
            // device-wide barriers: every workgroup of its grid must be resident at once
            const char *off = std::getenv("DZG_SP_FUSED");
            if (!(off && off[0] == '0') && (long long)dzg_sp_fused_resident_per_cu() * cus >= dzg_sp_grid(m)) {
                TRY(dev_alloc(s, &s->chain_bar, (size_t)DZG_CHAIN_BAR_WORDS));
                HIP_OK(hipMemsetAsync(s->chain_bar, 0, sizeof(unsigned long long) * DZG_CHAIN_BAR_WORDS, s->st));
            }
        }
        if (d.spb) {
            TRY(dev_alloc(s, &d.sslot, (size_t)m)); TRY(dev_alloc(s, &d.spos, (size_t)m));
            TRY(dev_alloc(s, &d.bslot, (size_t)(ns ? ns : 1))); TRY(dev_alloc(s, &d.rowpos, (size_t)m));
            TRY(dev_alloc(s, &d.dxs, (size_t)m)); TRY(dev_alloc(s, &d.acol_code, 1));
            HIP_OK(hipMemsetAsync(d.acol, 0, sizeof(double) * (size_t)(m ? m : 1), s->st));
            HIP_OK(hipMemsetAsync(d.dxs, 0, sizeof(double) * (size_t)(m ? m : 1), s->st));
        }
        // dense matrix: one GPU, or a column-sharded rank (replicated or partitioned storage)
        if (!d.csc && !o.seven_launches && !d.rs) { // (a partitioned rank takes the column from the record)
            // the chain's barriers need every workgroup resident at once: one per CU, and the
            // runtime must agree that a workgroup of either kernel fits a CU at all (registers,
            // 136 KB of LDS); otherwise the barrier-free seven launches run
            int grid = cus;
            if (grid > 256) grid = 256; // (k_chain_pre reads <= 256 candidates)
            const int per_cu = dzg_chain_resident_per_cu();
            if (per_cu < 1) grid = 0;
            if (const char *g = std::getenv("DZG_CHAIN_GRID")) { // tests: a device with few CUs
                const int v = std::atoi(g);
                if (v >= 1 && v < grid) grid = v;
            }
            // a thread takes one row and one column of its workgroup's share (512 threads)
            const int gdiv = grid > 0 ? grid : 1;
            const long long rows_per = (((long long)m + gdiv - 1) / gdiv + 3) & ~3ll;
            const long long cols_per = ((long long)q + gdiv - 1) / gdiv;
            if (grid >= 1 && rows_per <= 512 && cols_per <= 512) {
                s->chain_grid = grid;
                if (const char *cap = std::getenv("DZG_CHAIN_KCAP")) {
                    const long long v = std::atoll(cap);
                    if (v >= 0 && v < s->chain_kcap) s->chain_kcap = v;
                }
                if (const char *dbg = std::getenv("DZG_CHAIN_DEBUG")) {
                    if (dbg[0] == '1') {
                        TRY(dev_alloc(s, &s->chain_dbg, (size_t)16 * DZG_STAMP_SLOTS));
                        HIP_OK(hipMemsetAsync(s->chain_dbg, 0, sizeof(unsigned long long) * 16 * DZG_STAMP_SLOTS, s->st));
                    }
                }
                if (const char *nf = std::getenv("DZG_CHAIN_NO_FOLD")) s->chain_fold = nf[0] != '1';
                if (const char *ci = std::getenv("DZG_CHAIN_INSTANCES")) s->chain_instances = ci[0] != '0';
                TRY(dev_alloc(s, &s->chain_bar, (size_t)DZG_CHAIN_BAR_WORDS));
                HIP_OK(hipMemsetAsync(s->chain_bar, 0, sizeof(unsigned long long) * DZG_CHAIN_BAR_WORDS, s->st));
            }
        }
        // Row-wise pricing (k_price_kernels.h): a row-major copy of the rank's own columns and the
        // partial sums of the row groups.  AUTO pricing only (an explicit kernel choice means that
        // kernel); DZG_PRICE_ROWS=0 is the A/B switch of the tools and tests.
        {
            const char *rows_env = std::getenv("DZG_PRICE_ROWS");
            const int nown = d.col1 - d.col0;
            if (!d.csc && o.price_kernel == DZG_PRICE_AUTO && m > 0 && nown > 0 && ns > 0 &&
                !(rows_env && rows_env[0] == '0')) {
                // (no padding: with a row stride that is not a multiple of 4 KB the pass at k = 4 049 takes
                // 93.9 us instead of 85.8, profiles/r04_ftran_row_loads_ab.txt)
                d.ldt = ((long long)nown + 3) / 4 * 4;
                // (the copy doubles the matrix: a device that cannot hold it prices column-wise)
                void *at_mem = nullptr;
                if (hipMalloc(&at_mem, sizeof(double) * (size_t)m * (size_t)d.ldt) != hipSuccess) {
                    (void)hipGetLastError();
                    at_mem = nullptr;
                }
                double *at = static_cast<double *>(at_mem);
                if (at) {
                    s->allocs.push_back(at_mem);
                    TRY(dev_alloc(s, &d.ppart, (size_t)dzg_price_rows_groups() * (size_t)d.ldt));
                    TRY(dev_alloc(s, &d.vc, (size_t)m));
                    HIP_OK(hipMemsetAsync(d.vc, 0, sizeof(double) * (size_t)m, s->st));
                    dzg_launch_transpose_to_rows(d.A, d.lda, m, nown, at, d.ldt, s->st);
                }
                d.At = at;
                // where 8 (k + 1) n_s bytes of rows meet 8 m (n_s - k) bytes of columns, less the
                // second launch: a function of the problem's shape alone (the same on every rank)
                // (0.93: tools/price_rows_bench.hip -- 0.0205 us per row of 16 384 columns + 6 us for the
                // finishing launch against 0.0099 us per column of 8192 rows: equal at k = 5 150 of 5 461)
                d.rows_T = (int)(0.93 * (double)m * (double)ns / ((double)ns + (double)m));
                if (const char *t = std::getenv("DZG_PRICE_ROWS_T")) d.rows_T = std::atoi(t);
                if (d.rows_T < 1) { d.At = nullptr; d.vc = nullptr; }
            }
        }
        // the eta rows in compact coordinates, kept current by the chain kernels: only where the fused
        // small-k pass can ever run (dzg_price_small) behind a chain
        if (s->chain_bar && s->chain_grid > 0 && !d.spb && d.At && d.vc && d.cpos && d.world <= 1 && !d.rs &&
            dzg_price_small_partials(d) <= s->chain_grid) {
            TRY(dev_alloc(s, &s->wk_buf, (size_t)d.ldw * DZG_RMAX));
            HIP_OK(hipMemsetAsync(s->wk_buf, 0, sizeof(double) * (size_t)d.ldw * DZG_RMAX, s->st));
            if (const char *pf = std::getenv("DZG_CHAIN_PRICE_FUSED")) s->chain_price_fused = pf[0] != '0';
        }
        dzg_launch_fast_init(d, s->st);
        if (d.spb) {
            dzg_launch_sp_init(d, 1, s->st);
            dzg_launch_sp_update(d, 1, s->st);
        } else {
            dzg_launch_fast_update(d, 1, s->st); // first-pivot partials of the initial state
        }
        if (needs_initial_refactor && src) { // (dzg_debug_extend_ms: the refactorisation on its own)
            HIP_OK(hipStreamSynchronize(s->st));
            const auto t0 = std::chrono::steady_clock::now();
            TRY(refactor_now(s));
            HIP_OK(hipStreamSynchronize(s->st));
            s->extend_ms[1] = ms_since(t0);
        } else if (needs_initial_refactor) {
            TRY(refactor_now(s));
        }
    } else {
        dzg_lu_layout(m, &d.lu);
        const size_t mm = (size_t)(m ? m : 1);
        TRY(dev_alloc(s, &d.lu.W, mm * (size_t)d.lu.ldw));
        TRY(dev_alloc(s, &d.lu.P0, mm * DZG_LU_LDP)); TRY(dev_alloc(s, &d.lu.P1, mm * DZG_LU_LDP));
        TRY(dev_alloc(s, &d.lu.piv, mm)); TRY(dev_alloc(s, &d.lu.pz, mm));
        TRY(dev_alloc(s, &d.lu.ptab, mm * DZG_LU_NB));
        TRY(dev_alloc(s, &d.lu.part_r, (size_t)2 * d.lu.nparts));
        TRY(dev_alloc(s, &d.lu.part_k, (size_t)2 * d.lu.nparts));
    }
    if (o.profile) {
        s->ev.resize((size_t)o.poll_interval * DZG_K_COUNT * 2);
        // (timing only, read after the stream has been waited for: without the system-scope fence a
        // default event carries -- 5.7 us of idle GPU per record between two 10-us kernels,
        // profiles/r04_chain_phase_clocks.txt)
        for (auto &e : s->ev) HIP_OK(hipEventCreateWithFlags(&e, hipEventDisableSystemFence));
    }
    HIP_OK(hipStreamSynchronize(s->st));
    HIP_OK(hipGetLastError());
    guard.s = nullptr;
    *out = s;
    return 0;
}

extern "C" int dzg_solver_create(const dzg_lp *lp, const dzg_opts *opts_in, dzg_solver **out)
{
    return solver_create(lp, opts_in, out, nullptr);
}

// ---- one iteration, enqueued ------------------------------------------------------
namespace {
// opts.profile: the classes to time (low 16 bits; any negative value: all of them) and, in bits
// 16..23, a sampling stride S > 1: only every S-th iteration of a batch is stamped
static inline bool prof_on(const dzg_solver *s, int cls, int slot)
{
    const int p = s->opts.profile;
    if (p == 0 || slot < 0) return false;
    if (p < 0) return true;
    const int stride = (p >> 16) & 0xff;
    // (the last of each S: the first iteration of a batch starts on an empty queue)
    return (p & (1 << cls)) && (stride <= 1 || slot % stride == stride - 1);
}

struct Prof {
    dzg_solver *s;
    int slot;
    void begin(int cls) const
    {
        if (prof_on(s, cls, slot))
            hipEventRecord(s->ev[((size_t)slot * DZG_K_COUNT + cls) * 2], s->st);
    }
    void end(int cls) const
    {
        if (prof_on(s, cls, slot))
            hipEventRecord(s->ev[((size_t)slot * DZG_K_COUNT + cls) * 2 + 1], s->st);
    }
};
} // namespace

static int price_kernel_for(const dzg_solver *s)
{
    // AUTO: FAST numerics streams with the register-accumulator kernel, whose sums depend only
    // on m (bit-identical dz on one GPU and on any column sharding); the reference-order kernel
    // (bit-identical to neg_t_dot) belongs to STRICT, whose v is the reference's v.
    if (s->d.csc) // CSC: the tree-order kernel unless the options insist on the reference's order
        return s->opts.price_kernel == DZG_PRICE_SEQ ? DZG_PRICE_SEQ : DZG_PRICE_CSC_KERNEL;
    if (s->opts.price_kernel != DZG_PRICE_AUTO) return s->opts.price_kernel;
    return DZG_PRICE_TREE;
}

// per-workgroup ratio partials the pricing pass leaves (every CSC kernel uses the same grid)
static int price_partials_for(const dzg_solver *s, int pk)
{
    return dzg_price_partials_dev(s->d, pk);
}

static void enqueue_fast_iteration(dzg_solver *s, int slot)
{
    const DzgDev &d = s->d;
    hipStream_t st = s->st;
    Prof pf{s, slot};
    const int pk = price_kernel_for(s);
    pf.begin(DZG_K_STATUS);
    dzg_launch_fast_select_prep(d, 0, 0, nullptr, st); // status() + FTRAN prep of a primal step
    pf.end(DZG_K_STATUS);
    pf.begin(DZG_K_FTRAN);
    dzg_launch_fast_gemv(d, DZG_STEP_PRIMAL, nullptr, st); // primal step: dx first (+ ratio partials)
    pf.end(DZG_K_FTRAN);
    pf.begin(DZG_K_BTRAN);
    dzg_launch_fast_btran(d, st); // (primal: finishes the ratio test) v = row p of Binv
    pf.end(DZG_K_BTRAN);
    pf.begin(DZG_K_PRICE);
    dzg_launch_price_fast(d, pk, st); // dz (+ dual ratio partials)
    pf.end(DZG_K_PRICE);
    pf.begin(DZG_K_RATIO);
    dzg_launch_fast_select_prep(d, 1, price_partials_for(s, pk), nullptr, st); // dual: ratio + prep
    dzg_launch_fast_gemv(d, DZG_STEP_DUAL, nullptr, st);                    // dual step: dx last
    pf.end(DZG_K_RATIO);
    pf.begin(DZG_K_UPDATE);
    dzg_launch_fast_update(d, 0, st); // (the pivot's books were kept by the launch before)
    pf.end(DZG_K_UPDATE);
    if (++s->since_flush >= DZG_RMAX) {
        pf.begin(DZG_K_BASIS_UPDATE);
        dzg_launch_fast_flush(d, st); // Binv0 -= U Wc on the fp64 matrix cores
        pf.end(DZG_K_BASIS_UPDATE);
        s->since_flush = 0;
    } else {
        pf.begin(DZG_K_BASIS_UPDATE);
        pf.end(DZG_K_BASIS_UPDATE);
    }
}

// Dense matrix on one GPU: the same iteration in three launches (k_chain.hip).
static void enqueue_chain_iteration(dzg_solver *s, int slot)
{
    const DzgDev &d = s->d;
    hipStream_t st = s->st;
    Prof pf{s, slot};
    const int pk = price_kernel_for(s);
    // k below ~480 for the whole batch: one fused kernel prices row-wise AND finishes (dz, ratio
    // candidates) per column tile -- no partial sums in memory, nothing to fold.  Otherwise, while
    // the batch prices row-wise for certain, k_chain_post finishes the pass itself (FOLD)
    const int small = dzg_price_small(d, pk);
    const int fold = !small && s->chain_fold && dzg_price_rows_certain(d, pk);
    // ... and where every tile has a chain workgroup, that pass is the TAIL of k_chain_pre: two launches
    // a pivot.  A slot whose pricing pass is timed keeps the three launches, so that its events
    // bracket k_price_rows_small alone (run_fast has gathered d.wk where the batch can want it).
    const int fused = s->chain_price_fused &&
                      dzg_chain_price_fused(d, s->chain_grid, small, prof_on(s, DZG_K_PRICE, slot));
    (fused ? s->chain_fused : s->chain_unfused) += 1;
    pf.begin(DZG_K_FTRAN);
    dzg_launch_chain_pre(d, s->chain_grid, s->chain_bar, s->chain_dbg, nullptr, st, // status, primal FTRAN + ratio, BTRAN row
                         s->chain_instances, fused);
    pf.end(DZG_K_FTRAN);
    pf.begin(DZG_K_PRICE);
    if (!fused) dzg_launch_price_fast(d, pk, st, -1, fold, small, small ? s->chain_dbg : nullptr);
    pf.end(DZG_K_PRICE);
    pf.begin(DZG_K_UPDATE);
    dzg_launch_chain_post(d, s->chain_grid, s->chain_bar, s->chain_dbg, 0,
                          small ? dzg_price_small_partials(d)
                                : (fold ? s->chain_grid : price_partials_for(s, pk)),
                          nullptr, st, fold, small, s->chain_instances);
    pf.end(DZG_K_UPDATE);
    pf.begin(DZG_K_BASIS_UPDATE);
    if (++s->since_flush >= DZG_RMAX) {
        dzg_launch_fast_flush(d, st);
        s->since_flush = 0;
    }
    pf.end(DZG_K_BASIS_UPDATE);
}

// CSC input on one GPU: the sparse-basis kernels (k_sparse.hip).  Same phases as above.
static void enqueue_sparse_iteration(dzg_solver *s, int slot)
{
    const DzgDev &d = s->d;
    hipStream_t st = s->st;
    Prof pf{s, slot};
    if (s->batch_chain) { // four launches: the phases of one side of the pricing pass share a launch
        const int pk = price_kernel_for(s);
        pf.begin(DZG_K_FTRAN);
        dzg_launch_sp_pre(d, s->chain_bar, st); // status, primal FTRAN (both halves) + ratio test, BTRAN row
        pf.end(DZG_K_FTRAN);
        pf.begin(DZG_K_PRICE);
        dzg_launch_price_fast(d, pk, st);
        pf.end(DZG_K_PRICE);
        pf.begin(DZG_K_RATIO);
        dzg_launch_sp_mid(d, s->chain_bar, price_partials_for(s, pk), st); // dual ratio + FTRAN; the books
        pf.end(DZG_K_RATIO);
        pf.begin(DZG_K_UPDATE);
        dzg_launch_sp_update(d, 0, st);
        pf.end(DZG_K_UPDATE);
        pf.begin(DZG_K_BASIS_UPDATE);
        if (++s->since_flush >= DZG_RMAX) {
            dzg_launch_sp_flush(d, st);
            s->since_flush = 0;
        }
        pf.end(DZG_K_BASIS_UPDATE);
        return;
    }
    pf.begin(DZG_K_FTRAN);
    dzg_launch_sp_ftran(d, DZG_STEP_PRIMAL, 0, st); // status() + primal FTRAN (a no-op in a dual step)
    pf.end(DZG_K_FTRAN);
    pf.begin(DZG_K_BTRAN);
    dzg_launch_sp_btran(d, st);
    pf.end(DZG_K_BTRAN);
    pf.begin(DZG_K_PRICE);
    dzg_launch_price_fast(d, price_kernel_for(s), st);
    pf.end(DZG_K_PRICE);
    pf.begin(DZG_K_RATIO);
    dzg_launch_sp_ftran(d, DZG_STEP_DUAL, price_partials_for(s, price_kernel_for(s)), st); // ratio + dual FTRAN
    pf.end(DZG_K_RATIO);
    pf.begin(DZG_K_UPDATE);
    dzg_launch_sp_pivot(d, st);
    dzg_launch_sp_update(d, 0, st);
    pf.end(DZG_K_UPDATE);
    pf.begin(DZG_K_BASIS_UPDATE);
    if (++s->since_flush >= DZG_RMAX) {
        dzg_launch_sp_flush(d, st); // X -= Ub^T Wc on the fp64 matrix cores
        s->since_flush = 0;
    }
    pf.end(DZG_K_BASIS_UPDATE);
}

static void collect_profile(dzg_solver *s, int slots_real)
{
    if (!s->opts.profile) return;
    for (int slot = 0; slot < slots_real; ++slot)
        for (int cls = 0; cls < DZG_K_COUNT; ++cls) {
            if (!prof_on(s, cls, slot)) continue;
            if (s->d.csc && !s->d.spb && s->d.world == 1 && !s->comm && cls != DZG_K_PRICE)
                continue; // the single-GPU record path of a CSC solver only stamps pricing
            if (s->batch_chain && s->d.world == 1 && !s->comm &&
                (cls == DZG_K_STATUS || cls == DZG_K_BTRAN || (cls == DZG_K_RATIO && !s->d.spb)))
                continue; // the chain has no launches of their own for these
            float ms = 0.f;
            size_t base = ((size_t)slot * DZG_K_COUNT + cls) * 2;
            if (hipEventElapsedTime(&ms, s->ev[base], s->ev[base + 1]) == hipSuccess) {
                s->kernel_ms[cls] += ms;
                s->kernel_launches[cls] += 1;
            }
        }
    (void)hipGetLastError(); // a class this numerics mode never stamps (e.g. DZG_K_LU in FAST)
}

static int read_ctl(dzg_solver *s)
{
    HIP_OK(hipMemcpyAsync(s->h_ctl, s->d.ctl, sizeof(DzgCtl), hipMemcpyDeviceToHost, s->st));
    HIP_OK(hipStreamSynchronize(s->st));
    if (s->h_ctl->max_pivot_err > s->max_err_life) s->max_err_life = s->h_ctl->max_pivot_err;
    return 0;
}

// Rebuild Binv0 from scratch for the current basis (k_refactor.hip).  One host sync to learn
// k; everything else is enqueued.
// The refactorisation workspace (two m x m panels and a few index lists) is reserved when the
// options ask for periodic refactorisation, and otherwise on first need: a solver that never
// drifts never pays for it, and one that does can still recover.
static int refactor_workspace(dzg_solver *s)
{
    if (s->rf_piv) return 0;
    const size_t m = (size_t)(s->d.m ? s->d.m : 1);
    s->rf_ld = ((long long)s->d.m + 15) / 16 * 16 + 16;
    TRY(dev_alloc(s, &s->rfPn, (size_t)64 * (size_t)s->rf_ld));
    TRY(dev_alloc(s, &s->rfTri, ((m + 63) / 64) * (size_t)(2 * 64 * 64)));
    TRY(dev_alloc(s, &s->rf_spos, m));
    TRY(dev_alloc(s, &s->rf_scode, m)); TRY(dev_alloc(s, &s->rf_lpos, m));
    TRY(dev_alloc(s, &s->rf_lrow, m)); TRY(dev_alloc(s, &s->rf_counts, 4));
    TRY(dev_alloc(s, &s->rf_lslot, m));
    TRY(dev_alloc(s, &s->rf_piv, m)); // set last: rf_piv != nullptr means "lists reserved"
    return 0;
}

// The two big panels G and X hold k x k (the structural block, its factors, the inverse) and then
// nl x k (the basic-slack rows A[L, S]): max(k, nl) rows of rf_ld doubles each -- half of m x m when
// the basis is half structural, which is what lets eight ranks of config 5 share one device in the
// lockstep harness.  They grow when a later basis needs more rows.
static int refactor_panels(dzg_solver *s, int k, int nl)
{
    const long long need = k > nl ? k : nl;
    if (s->rfG && s->rf_rows >= need) return 0;
    for (double **p : {&s->rfG, &s->rfX})
        if (*p) {
            auto it = std::find(s->allocs.begin(), s->allocs.end(), (void *)*p);
            if (it != s->allocs.end()) s->allocs.erase(it);
            HIP_OK(hipFree(*p));
            *p = nullptr;
        }
    long long rows = need + need / 8 + 64; // (head room: k moves by one per pivot)
    if (rows > s->d.m) rows = s->d.m;
    if (rows < 1) rows = 1;
    double *x = nullptr, *g = nullptr;
    TRY(dev_alloc(s, &x, (size_t)rows * (size_t)s->rf_ld));
    TRY(dev_alloc(s, &g, (size_t)rows * (size_t)s->rf_ld));
    s->rfX = x;
    s->rfG = g;
    s->rf_rows = rows;
    return 0;
}

// A rank of a PARTITIONED column-sharded solve holds its own structural columns only (a
// replicated one holds them all, like a single GPU).
static bool partitioned(const dzg_solver *s) { return s->d.world > 1 && !s->d.repl; }

// Stage A: the basis lists, one host sync to learn k and nl, the rank's share of G = A[R, S].
// *active = false: the solve has ended, nothing to refactorise (every rank alike).
static int refactor_stage_a(dzg_solver *s, int counts[2], bool *active, bool at_end = false)
{
    TRY(refactor_workspace(s));
    const DzgDev &d = s->d;
    dzg_launch_refactor_lists(d, s->rf_spos, s->rf_scode, s->rf_lpos, s->rf_lrow, s->rf_counts, s->st);
    counts[0] = counts[1] = 0;
    HIP_OK(hipMemcpyAsync(counts, s->rf_counts, sizeof(int) * 2, hipMemcpyDeviceToHost, s->st));
    TRY(read_ctl(s));
    *active = s->h_ctl->status == DZG_RUNNING || s->h_ctl->status == DZG_ITER_LIMIT ||
              s->h_ctl->status == DZG_NEAR_TIE;
    // (at_end: dzg_solver_duals wants the fresh inverse of the OPTIMAL basis, dzg_solver_ray that of
    // the basis an UNBOUNDED or INFEASIBLE solve stopped on)
    if (at_end && (s->h_ctl->status == DZG_OPTIMAL || s->h_ctl->status == DZG_UNBOUNDED ||
                   s->h_ctl->status == DZG_INFEASIBLE))
        *active = true;
    if (!*active) return 0;
    if (counts[0] != s->h_ctl->ncompact)
        return fail(DZG_E_DEVICE, "refactor: structural basics != dense columns");
    TRY(refactor_panels(s, counts[0], counts[1]));
    dzg_launch_refactor_a(d, counts[0], s->rfG, s->rfX, s->rf_ld, s->rf_scode, s->rf_counts + 2, s->st);
    return 0;
}

// Stage B: LU, the inverse, Binv0's rows of the structural positions, the rank's share of A[L, S]
// (*block, nl x rf_ld; nullptr: none).
static int refactor_stage_b(dzg_solver *s, const int counts[2], double **block)
{
    *block = dzg_launch_refactor_b(s->d, counts[0], counts[1], s->rfG, s->rfX, s->rfPn, s->rfTri, s->rf_ld,
                                   s->rf_piv, s->rf_spos, s->rf_scode, s->rf_lpos, s->rf_lrow, s->rf_lslot,
                                   s->rf_counts + 2, s->st);
    return 0;
}

// Stage C: Binv0's rows of the basic slacks, the eta file emptied, the monitor restarted.
static int refactor_stage_c(dzg_solver *s, const int counts[2])
{
    dzg_launch_refactor_c(s->d, counts[0], counts[1], s->rfG, s->rfX, s->rf_ld, s->rf_lpos,
                          s->rf_counts + 2, s->st);
    s->since_flush = 0;
    s->h_ctl->neta = 0; // the refactorisation empties the eta file (k_ref_done)
    s->since_refactor = 0;
    s->refactors += 1;
    s->pending_refactor = false;
    return 0;
}

// sum of a block over the ranks of the RCCL communicator, in place (a column has one owner: exact)
static int shard_sum(dzg_solver *s, double *buf, size_t count)
{
    if (count == 0) return 0;
    Rccl &r = rccl();
    if (!s->comm || !r.ok || !r.AllReduce)
        return fail(DZG_E_ARG, "refactorisation of a partitioned column-sharded solver needs its "
                               "ranks' columns: dzg_shard_comm_init first (or the lockstep loop)");
    if (r.AllReduce(buf, buf, count, kNcclFloat64, kNcclSum, s->comm, s->st) != 0)
        return fail(DZG_E_DEVICE, "ncclAllReduce (basic columns of a refactorisation)");
    return 0;
}

// The carried x, xbar, z, zbar against their recomputation from the inverse the refactorisation has just
// built (k_drift.hip); the result widens the near-tie tolerance and is reported as state_drift.
static int measure_drift(dzg_solver *s)
{
    if (!s->dr_b0 || s->d.world != 1 || s->d.spb) return 0;
    DzgDev &d = s->d;
    if (!s->dr_out) {
        TRY(dev_alloc(s, &s->dr_agb, (size_t)d.m + 2)); TRY(dev_alloc(s, &s->dr_agx, (size_t)d.m + 2));
        TRY(dev_alloc(s, &s->dr_part, (size_t)dzg_drift_chunks() * (size_t)d.ldw));
        TRY(dev_alloc(s, &s->dr_y, (size_t)d.m + 2)); TRY(dev_alloc(s, &s->dr_dzy, (size_t)d.q));
        TRY(dev_alloc(s, &s->dr_out, (size_t)8 * dzg_drift_blocks()));
    }
    dzg_launch_drift(d, s->dr_b0, s->dr_xb0, s->dr_c, s->dr_cb, s->dr_agb, s->dr_agx, s->dr_part, s->dr_y,
                     s->dr_dzy, s->dr_out, (int)s->h_ctl->ncompact, s->st);
    const int nb = dzg_drift_blocks();
    std::vector<double> out((size_t)8 * nb);
    HIP_OK(hipMemcpyAsync(out.data(), s->dr_out, sizeof(double) * out.size(), hipMemcpyDeviceToHost, s->st));
    HIP_OK(hipStreamSynchronize(s->st));
    // e = max |x - x^|, max |x^|, the same for xbar, z, zbar
    double e[8] = {0, 0, 0, 0, 0, 0, 0, 0};
    for (int b = 0; b < nb; ++b) {
        for (int j = 0; j < 4; ++j) e[j] = std::max(e[j], out[(size_t)4 * b + j]);
        for (int j = 0; j < 2; ++j) e[4 + j] = std::max(e[4 + j], out[(size_t)4 * nb + 2 * b + j]);
        for (int j = 0; j < 2; ++j) e[6 + j] = std::max(e[6 + j], out[(size_t)6 * nb + 2 * b + j]);
    }
    double drift = 0.0;
    for (int j = 0; j < 8; j += 2) {
        const double rel = e[j] / std::max(1.0, e[j + 1]);
        if (rel == rel && rel > drift) drift = rel;
    }
    s->state_drift = drift;
    DzgCtl *h = s->h_ctl;
    h->drift_tau = 4.0 * drift;
    HIP_OK(hipMemcpyAsync(&d.ctl->drift_tau, &h->drift_tau, sizeof(double), hipMemcpyHostToDevice, s->st));
    if (h->tie_tol >= 0.0) { // (the monitor restarted with the fresh inverse: max_pivot_err = 0)
        h->tau = std::max(h->tie_tol, h->drift_tau);
        HIP_OK(hipMemcpyAsync(&d.ctl->tau, &h->tau, sizeof(double), hipMemcpyHostToDevice, s->st));
    }
    HIP_OK(hipStreamSynchronize(s->st));
    return 0;
}

static int refactor_now(dzg_solver *s, bool at_end)
{
    s->d.wk = nullptr; // (a new Binv0, a new compact numbering, an empty eta file: gathered afresh)
    if (partitioned(s) && s->in_lockstep)
        return fail(DZG_E_ARG, "refactor: the lockstep loop refactorises its ranks together");
    int counts[2];
    bool active = false;
    TRY(refactor_stage_a(s, counts, &active, at_end));
    if (!active) return 0;
    // (every rank of a sharded solve gets here at the same pivot count with the same k and nl: the
    // triggers -- interval, health monitor, a pending warm start -- read replicated state only)
    if (partitioned(s)) TRY(shard_sum(s, s->rfG, (size_t)counts[0] * (size_t)s->rf_ld));
    double *block = nullptr;
    TRY(refactor_stage_b(s, counts, &block));
    if (partitioned(s) && block) TRY(shard_sum(s, block, (size_t)counts[1] * (size_t)s->rf_ld));
    TRY(refactor_stage_c(s, counts));
    return measure_drift(s);
}

// All ranks of a lockstep group (one process, one device, one stream) refactorise together; the
// sums over the ranks of a partitioned solve are one kernel each.
static int refactor_lockstep(dzg_solver **sv, int world)
{
    if (!partitioned(sv[0])) {
        for (int r = 0; r < world; ++r) TRY(refactor_now(sv[r]));
        return 0;
    }
    std::vector<int> counts((size_t)2 * world, 0);
    bool active = false;
    for (int r = 0; r < world; ++r) {
        bool a = false;
        TRY(refactor_stage_a(sv[r], &counts[(size_t)2 * r], &a));
        if (r > 0 && (a != active || counts[(size_t)2 * r] != counts[0] || counts[(size_t)2 * r + 1] != counts[1]))
            return fail(DZG_E_DEVICE, "lockstep refactor: ranks diverged");
        active = a;
    }
    if (!active) return 0;
    hipStream_t st = sv[0]->st;
    double **dptrs = nullptr;
    HIP_OK(hipMalloc(&dptrs, sizeof(double *) * (size_t)world));
    struct Free { double **p; ~Free() { hipFree(p); } } free_ptrs{dptrs};
    std::vector<double *> ptrs((size_t)world);
    for (int r = 0; r < world; ++r) ptrs[(size_t)r] = sv[r]->rfG;
    HIP_OK(hipMemcpyAsync(dptrs, ptrs.data(), sizeof(double *) * (size_t)world, hipMemcpyHostToDevice, st));
    dzg_launch_lockstep_sum(dptrs, world, (long long)counts[0] * sv[0]->rf_ld, st);
    HIP_OK(hipStreamSynchronize(st)); // (ptrs is rewritten below)
    bool any_block = false;
    for (int r = 0; r < world; ++r) {
        double *block = nullptr;
        TRY(refactor_stage_b(sv[r], &counts[(size_t)2 * r], &block));
        ptrs[(size_t)r] = block;
        any_block = any_block || block;
    }
    if (any_block) {
        HIP_OK(hipMemcpyAsync(dptrs, ptrs.data(), sizeof(double *) * (size_t)world, hipMemcpyHostToDevice, st));
        dzg_launch_lockstep_sum(dptrs, world, (long long)counts[1] * sv[0]->rf_ld, st);
        HIP_OK(hipStreamSynchronize(st));
    }
    for (int r = 0; r < world; ++r) TRY(refactor_stage_c(sv[r], &counts[(size_t)2 * r]));
    return 0;
}

extern "C" int dzg_solver_refactor(dzg_solver *s)
{
    if (!s || s->numerics != DZG_NUMERICS_FAST) return fail(DZG_E_ARG, "refactor: FAST solver");
    HIP_OK(hipSetDevice(s->opts.device));
    TRY(refactor_now(s));
    HIP_OK(hipStreamSynchronize(s->st));
    HIP_OK(hipGetLastError());
    return 0;
}

// iterations to enqueue before the next status poll: never past the run budget (an iteration
// enqueued beyond it would be a no-op, but it would still cost its launches and exchanges)
static int batch_size(const dzg_solver *s)
{
    const long long remaining = s->h_ctl->iter_stop - s->h_ctl->iter;
    const int poll = s->opts.poll_interval;
    return (int)(remaining < poll ? (remaining < 1 ? 1 : remaining) : poll);
}

// FAST health rule without a refactorisation workspace: the pivot element computed by FTRAN
// and by BTRAN + pricing disagree beyond repair -> stop with DZG_SINGULAR rather than wander.
static int health_stop(dzg_solver *s)
{
    if (s->h_ctl->max_pivot_err > 1e-4) {
        int st = DZG_SINGULAR;
        HIP_OK(hipMemcpy(&s->d.ctl->status, &st, sizeof(int), hipMemcpyHostToDevice));
        s->h_ctl->status = st;
    }
    return 0;
}

// FAST health between batches: the pivot element computed by FTRAN and by BTRAN + pricing must
// agree.  A drift is shed by a refactorisation (workspace reserved on first need; the ranks of a
// partitioned sharded solve exchange their basic columns for it); where that is impossible -- a
// partitioned solver whose host drives the phases itself, out of memory -- or does not help, the
// solve stops with DZG_SINGULAR.  Every rank of a sharded solve sees the same max_pivot_err
// (replicated dx_p, published dz_r) and therefore takes the same action.
enum HealthAction { HEALTH_OK = 0, HEALTH_REFACTOR, HEALTH_GIVE_UP };

static bool can_refactor(const dzg_solver *s)
{
    return !partitioned(s) || s->comm != nullptr || s->in_lockstep;
}

static HealthAction health_decide(dzg_solver *s)
{
    if (!can_refactor(s)) return s->h_ctl->max_pivot_err > 1e-4 ? HEALTH_GIVE_UP : HEALTH_OK;
    if (!(s->h_ctl->max_pivot_err > s->drift_trigger && s->since_refactor > 0)) return HEALTH_OK;
    // a basis whose fresh inverse drifts again at once is ill-conditioned, not stale: accept a
    // larger disagreement instead of refactorising every batch
    const bool fresh = s->refactors > 0 && s->since_refactor <= 2ll * s->opts.poll_interval;
    if (fresh) s->drift_trigger *= 100.0;
    if (fresh && s->h_ctl->max_pivot_err > 1e-4) return HEALTH_GIVE_UP;
    return HEALTH_REFACTOR;
}

static int health_give_up(dzg_solver *s, bool *stop)
{
    if (can_refactor(s)) s->h_ctl->max_pivot_err = 1.0;
    TRY(health_stop(s));
    *stop = s->h_ctl->status != DZG_RUNNING;
    return 0;
}

static int health_check(dzg_solver *s, bool *stop)
{
    *stop = false;
    switch (health_decide(s)) {
    case HEALTH_OK: return 0;
    case HEALTH_REFACTOR: {
        const int rrc = refactor_now(s);
        // (a refactorisation that FAILED as a call -- device error, out of memory -- is that error,
        // not a singular basis)
        if (rrc == DZG_E_DEVICE || rrc == DZG_E_NOMEM) return rrc;
        if (rrc != 0) return health_give_up(s, stop);
        return 0;
    }
    default: return health_give_up(s, stop);
    }
}

// Budget spent: the host ends the run itself instead of enqueueing an iteration that would only
// discover it (a no-op iteration would still advance the host's flush bookkeeping, and the eta
// flush must fall after the same pivots however a solve is cut into runs: results are
// reproducible bit for bit across budgets, poll intervals and near-tie stops).
static int budget_spent(dzg_solver *s, bool *spent)
{
    *spent = s->h_ctl->status == DZG_RUNNING && s->h_ctl->iter >= s->h_ctl->iter_stop;
    if (*spent) {
        int st = DZG_ITER_LIMIT;
        HIP_OK(hipMemcpy(&s->d.ctl->status, &st, sizeof(int), hipMemcpyHostToDevice));
        s->h_ctl->status = st;
    }
    return 0;
}

// A device-wide barrier of the three-launch iteration failed (its workgroups were not all resident:
// another kernel holds CUs or LDS of this device).  chain_barrier fails CONSISTENTLY -- every
// workgroup of the launch alike -- and both chain kernels write nothing but scratch (dx, v, beta_part,
// candidates, the decision fields of the control block) before their last barrier, and every
// later launch of the batch saw status != RUNNING: the solver state is that of the last completed
// pivot.  Clear the counters, carry on with the barrier-free seven launches (same arithmetic, same
// pivots) and give the chain another chance later; after three failures it stays off.
static int chain_recover(dzg_solver *s)
{
    DzgCtl *h = s->h_ctl;
    s->chain_fallbacks += 1;
    s->d.wk = nullptr; // (a launch that ended at a barrier may have stored a row of the copy and not pivoted)
    s->chain_retry_iter = s->chain_fallbacks >= 3 ? std::numeric_limits<long long>::max()
                                                  : h->iter + 64ll * s->opts.poll_interval;
    HIP_OK(hipMemsetAsync(s->chain_bar, 0, sizeof(unsigned long long) * DZG_CHAIN_BAR_WORDS, s->st));
    h->status = DZG_RUNNING;
    h->bar_timeout = 0;
    h->bar_gen = 0;
    HIP_OK(hipMemcpyAsync(&s->d.ctl->status, &h->status, sizeof(int), hipMemcpyHostToDevice, s->st));
    HIP_OK(hipMemcpyAsync(&s->d.ctl->bar_timeout, &h->bar_timeout, sizeof(int), hipMemcpyHostToDevice, s->st));
    HIP_OK(hipMemcpyAsync(&s->d.ctl->bar_gen, &h->bar_gen, sizeof(unsigned long long), hipMemcpyHostToDevice, s->st));
    HIP_OK(hipStreamSynchronize(s->st));
    return 0;
}

static int run_fast(dzg_solver *s)
{
    for (;;) {
        bool spent = false;
        TRY(budget_spent(s, &spent));
        if (spent) break;
        if (s->opts.refactor_interval > 0 && s->since_refactor >= s->opts.refactor_interval)
            TRY(refactor_now(s));
        const long long before = s->h_ctl->iter;
        const int batch = batch_size(s);
        s->since_flush = s->h_ctl->neta; // pending etas as the device counts them
        s->d.price_cols_hint = (int)s->h_ctl->nb_struct + batch; // (at most one more per pivot)
        // the eta flush's grid follows k as the host knows it (k grows by at most one per pivot).
        // Only around launches this loop enqueues itself: the phase entry points are also driven
        // from outside (sharded hosts), where nobody refreshes the bound
        const int k_bound = (int)s->h_ctl->ncompact + batch;
        const int k_low = (int)s->h_ctl->ncompact > batch ? (int)s->h_ctl->ncompact - batch : 0;
        if (s->d.spb) {
            s->d.k_hint = k_bound;
            s->batch_chain = s->chain_bar && s->h_ctl->iter >= s->chain_retry_iter;
            for (int b = 0; b < batch; ++b) enqueue_sparse_iteration(s, b);
            s->d.k_hint = 0;
        } else if (s->d.csc) { // sparse input: the record-based phases, exchanging with itself
            TRY(shard_buffers(s));
            const size_t nb = sizeof(double) * (size_t)s->d.xstride;
            for (int b = 0; b < batch; ++b) {
                s->prof_slot = s->opts.profile ? b : -1;
                TRY(dzg_shard_phase1(s, s->xsend));
                HIP_OK(hipMemcpyAsync(s->xrecv1, s->xsend, nb, hipMemcpyDeviceToDevice, s->st));
                TRY(dzg_shard_phase2(s, s->xrecv1, s->xsend));
                HIP_OK(hipMemcpyAsync(s->xrecv2, s->xsend, nb, hipMemcpyDeviceToDevice, s->st));
                TRY(dzg_shard_phase3(s, s->xrecv2));
            }
            s->prof_slot = -1;
        } else {
            // the chain keeps the gathered entering column in LDS: beyond that compact width
            // (k grows by at most one per pivot) the batch runs as seven launches
            s->batch_chain = s->chain_bar && s->h_ctl->iter >= s->chain_retry_iter &&
                             (long long)s->h_ctl->ncompact + batch <= s->chain_kcap;
            s->d.k_hint = k_bound;
            s->d.k_lo_hint = k_low;
            if (s->batch_chain) {
                // a batch that can price in k_chain_pre's tail needs d.wk current: gathered here when
                // something outside the chain has changed W, drow or neta since it last was
                // (a batch that cannot -- k beyond the cap, more tiles than workgroups, the switch off --
                // runs with d.wk = NULL: its kernels neither store nor renumber, and no copy is kept)
                if (!(s->wk_buf && s->chain_price_fused && s->chain_instances &&
                      dzg_chain_keeps_wk(s->d, s->chain_grid, dzg_price_small(s->d, price_kernel_for(s))))) {
                    s->d.wk = nullptr;
                } else if (!s->d.wk) {
                    dzg_launch_gather_wk(s->d, s->wk_buf, s->st);
                    s->d.wk = s->wk_buf;
                }
                for (int b = 0; b < batch; ++b) enqueue_chain_iteration(s, b);
            } else {
                s->d.wk = nullptr; // (the seven launches append to W and renumber without the copy)
                for (int b = 0; b < batch; ++b) enqueue_fast_iteration(s, b);
            }
            s->d.k_hint = s->d.k_lo_hint = 0;
        }
        s->since_refactor += batch;
        TRY(read_ctl(s));
        HIP_OK(hipGetLastError());
        if (s->h_ctl->bar_timeout) { // the batch ended at a failed barrier: carry on without barriers
            TRY(chain_recover(s));
            continue;
        }
        collect_profile(s, (int)(s->h_ctl->iter - before));
        if (s->h_ctl->status != DZG_RUNNING) break;
        bool stop = false;
        TRY(health_check(s, &stop));
        if (stop) break;
    }
    return 0;
}

// STRICT basis solve = gather + 2(m-1) elimination launches + one substitution launch, the same
// sequence with the same arguments every time (the kernels read the basis and the control
// block from memory): capture it once per orientation and replay it, so an iteration costs two
// graph launches instead of ~4m kernel launches on the host.
static void strict_solve(dzg_solver *s, int transposed)
{
    const DzgDev &d = s->d;
    hipStream_t st = s->st;
    if (!s->graphs_tried) {
        s->graphs_tried = true;
        const bool off = getenv("DZG_NO_GRAPH") != nullptr; // diagnostic switch
        for (int t = 0; t < 2 && !off; ++t) {
            hipGraph_t graph = nullptr;
            if (hipStreamBeginCapture(st, hipStreamCaptureModeThreadLocal) != hipSuccess) break;
            dzg_launch_strict_solve(d, t, st);
            if (hipStreamEndCapture(st, &graph) != hipSuccess || !graph) {
                (void)hipGetLastError();
                break;
            }
            if (hipGraphInstantiate(&s->g_solve[t], graph, nullptr, nullptr, 0) != hipSuccess) {
                s->g_solve[t] = nullptr;
                (void)hipGetLastError();
            }
            hipGraphDestroy(graph);
        }
    }
    if (s->g_solve[transposed] && hipGraphLaunch(s->g_solve[transposed], st) == hipSuccess) return;
    dzg_launch_strict_solve(d, transposed, st); // capture unavailable: plain launches
}

static int run_strict(dzg_solver *s)
{
    const DzgDev &d = s->d;
    hipStream_t st = s->st;
    for (;;) {
        dzg_launch_status(d, st);
        TRY(read_ctl(s));
        if (s->h_ctl->status != DZG_RUNNING) break;
        if (s->h_ctl->kind == DZG_STEP_PRIMAL) { // src/simplex.rs:308-318
            dzg_launch_load_column(d, -1, st);
            hipMemcpyAsync(d.dx, d.acol, sizeof(double) * (size_t)d.m, hipMemcpyDeviceToDevice, st);
            strict_solve(s, 0);
            dzg_launch_ratio(d, DZG_STEP_PRIMAL, st);
            dzg_launch_unit_rhs(d, st); // needs leave_pos: no-op if the ratio test found none
            strict_solve(s, 1);
            dzg_launch_price(d, DZG_PRICE_SEQ, st);
        } else { // :320-330
            dzg_launch_unit_rhs(d, st);
            strict_solve(s, 1);
            dzg_launch_price(d, DZG_PRICE_SEQ, st);
            dzg_launch_ratio(d, DZG_STEP_DUAL, st);
            dzg_launch_load_column(d, -1, st);
            hipMemcpyAsync(d.dx, d.acol, sizeof(double) * (size_t)d.m, hipMemcpyDeviceToDevice, st);
            strict_solve(s, 0);
        }
        dzg_launch_prepare(d, st);
        dzg_launch_update_vectors(d, st);
    }
    HIP_OK(hipGetLastError());
    return 0;
}

static int set_budget(dzg_solver *s, int64_t max_new_iters)
{
    if (s->d.repl && s->cols_present != s->d.ns)
        return fail(DZG_E_ARG, "replicate_matrix: " + std::to_string(s->d.ns - s->cols_present) +
                               " structural columns have not been uploaded (dzg_solver_upload_columns)");
    s->d.k_hint = s->d.k_lo_hint = 0; // (bounds of a batch that ended in an error are void)
    if (s->pending_refactor && !partitioned(s)) TRY(refactor_now(s)); // (replicated: all columns are here now)
    if (s->pending_refactor && !s->comm && !s->in_lockstep)
        return fail(DZG_E_ARG, "a non-slack starting basis of a partitioned column-sharded solver is "
                               "factorised by dzg_shard_run / dzg_shard_run_lockstep (the ranks exchange "
                               "their basic columns): a host that drives the phases itself starts from "
                               "the slack basis or uses replicate_matrix");
    TRY(read_ctl(s));
    DzgCtl *h = s->h_ctl;
    // pending etas as the device counts them: a host that drives the phase entry points itself and
    // enqueued past a stop has a flush counter ahead of the device's (the flush kernels fold a FULL
    // file only), and would otherwise let neta reach DZG_RMAX with no flush pending
    s->since_flush = h->neta;
    if (h->status != DZG_RUNNING && h->status != DZG_ITER_LIMIT && h->status != DZG_NEAR_TIE)
        return h->status;
    long long stop = s->opts.max_iter;
    if (max_new_iters > 0 && h->iter + max_new_iters < stop) stop = h->iter + max_new_iters;
    if (h->status == DZG_ITER_LIMIT && h->iter >= s->opts.max_iter) return h->status;
    if (h->status == DZG_NEAR_TIE) {
        // resuming acknowledges the tie: the pivot in question is decided as FAST sees it
        h->tie_skip_iter = h->iter;
        HIP_OK(hipMemcpyAsync(&s->d.ctl->tie_skip_iter, &h->tie_skip_iter, sizeof(long long),
                              hipMemcpyHostToDevice, s->st));
    }
    h->status = DZG_RUNNING;
    h->iter_stop = stop;
    // only these words change; kernels are idle between runs
    HIP_OK(hipMemcpyAsync(&s->d.ctl->status, &h->status, sizeof(int), hipMemcpyHostToDevice, s->st));
    HIP_OK(hipMemcpyAsync(&s->d.ctl->iter_stop, &h->iter_stop, sizeof(long long), hipMemcpyHostToDevice, s->st));
    HIP_OK(hipStreamSynchronize(s->st));
    return DZG_RUNNING;
}

extern "C" int dzg_solver_set_budget(dzg_solver *s, int64_t max_new_iters)
{
    if (!s) return fail(DZG_E_ARG, "solver is NULL");
    HIP_OK(hipSetDevice(s->opts.device));
    return set_budget(s, max_new_iters);
}

extern "C" int dzg_solver_set_profile(dzg_solver *s, int32_t mask)
{
    if (!s) return fail(DZG_E_ARG, "solver is NULL");
    if (mask != 0 && s->ev.empty())
        return fail(DZG_E_ARG, "kernel timing needs opts.profile != 0 at creation (it reserves the events)");
    s->opts.profile = mask;
    return 0;
}

extern "C" int dzg_solver_poll(dzg_solver *s, int32_t *status, int64_t *iterations)
{
    if (!s) return fail(DZG_E_ARG, "solver is NULL");
    HIP_OK(hipSetDevice(s->opts.device));
    TRY(read_ctl(s));
    HIP_OK(hipGetLastError());
    if (status) *status = s->h_ctl->status;
    if (iterations) *iterations = s->h_ctl->iter;
    return 0;
}

// ---- column sharding: three enqueue-only phases per iteration (dantzig_amd.h) ---------
extern "C" int64_t dzg_shard_record_doubles(const dzg_solver *s) { return s ? s->d.xstride : 0; }

// event stamps of the phase path: slot = s->prof_slot (< 0: none)
static void phase_stamp(dzg_solver *s, int cls, int end)
{
    if (prof_on(s, cls, s->prof_slot))
        hipEventRecord(s->ev[((size_t)s->prof_slot * DZG_K_COUNT + cls) * 2 + end], s->st);
}

extern "C" int dzg_shard_phase1(dzg_solver *s, double *send_dev)
{
    if (!s || !send_dev || s->numerics != DZG_NUMERICS_FAST) return fail(DZG_E_ARG, "phase1");
    phase_stamp(s, DZG_K_STATUS, 0);
    if (s->d.rs)
        dzg_launch_rs_propose(s->d, 0, 0, send_dev, s->st);
    else
        dzg_launch_shard_propose(s->d, 0, 0, send_dev, s->st);
    phase_stamp(s, DZG_K_STATUS, 1);
    return 0;
}

extern "C" int dzg_shard_phase2(dzg_solver *s, const double *recv_dev, double *send_dev)
{
    if (!s || !recv_dev || !send_dev || s->numerics != DZG_NUMERICS_FAST)
        return fail(DZG_E_ARG, "phase2");
    const DzgDev &d = s->d;
    hipStream_t st = s->st;
    const int pk = price_kernel_for(s);
    if (d.rs) { // the basis side is row-sharded: k_rowshard.hip
        s->rs_recv1 = recv_dev;
        phase_stamp(s, DZG_K_FTRAN, 0);
        dzg_launch_rs_select(d, 0, recv_dev, st);                       // merge + status() (+ prep / v)
        dzg_launch_rs_gemv(d, DZG_STEP_PRIMAL, recv_dev, nullptr, st); // primal: FTRAN, own rows
        phase_stamp(s, DZG_K_FTRAN, 1);
        phase_stamp(s, DZG_K_PRICE, 0);
        dzg_launch_price_fast(d, pk, st, DZG_STEP_DUAL);                // dual: pricing, own columns
        phase_stamp(s, DZG_K_PRICE, 1);
        phase_stamp(s, DZG_K_RATIO, 0);
        dzg_launch_rs_propose(d, 1, price_partials_for(s, pk), send_dev, st);
        phase_stamp(s, DZG_K_RATIO, 1);
        return 0;
    }
    phase_stamp(s, DZG_K_FTRAN, 0);
    if (s->batch_chain) { // the three kernels below in one launch, k_chain.hip
        dzg_launch_chain_pre(d, s->chain_grid, s->chain_bar, s->chain_dbg, recv_dev, st);
    } else {
        dzg_launch_fast_select_prep(d, 4, 0, recv_dev, st);    // merge + status() + primal FTRAN prep
        dzg_launch_fast_gemv(d, DZG_STEP_PRIMAL, recv_dev, st);
        dzg_launch_fast_btran(d, st);
    }
    phase_stamp(s, DZG_K_FTRAN, 1);
    phase_stamp(s, DZG_K_PRICE, 0);
    dzg_launch_price_fast(d, pk, st);                      // owned columns only
    phase_stamp(s, DZG_K_PRICE, 1);
    phase_stamp(s, DZG_K_RATIO, 0);
    dzg_launch_shard_propose(d, 1, price_partials_for(s, pk), send_dev, st);
    phase_stamp(s, DZG_K_RATIO, 1);
    return 0;
}

extern "C" int dzg_shard_phase3(dzg_solver *s, const double *recv_dev)
{
    if (!s || !recv_dev || s->numerics != DZG_NUMERICS_FAST) return fail(DZG_E_ARG, "phase3");
    s->d.wk = nullptr; // (the phases pivot without the kept compact copy of the eta rows)
    const DzgDev &d = s->d;
    hipStream_t st = s->st;
    phase_stamp(s, DZG_K_UPDATE, 0);
    if (d.rs) {
        if (!s->rs_recv1) return fail(DZG_E_ARG, "phase3 before phase2");
        if (s->rs_recv1 == recv_dev)
            return fail(DZG_E_ARG, "shard_rows: phase 3 still reads the records of exchange 1 (the leaving "
                                   "row of a dual step, the entering column of a primal one): the second "
                                   "exchange needs a receive buffer of its own");
        dzg_launch_rs_select(d, 1, recv_dev, st);                          // merge (+ prep / v)
        dzg_launch_price_fast(d, price_kernel_for(s), st, DZG_STEP_PRIMAL); // primal: pricing
        dzg_launch_rs_gemv(d, DZG_STEP_DUAL, s->rs_recv1, recv_dev, st);   // dual: FTRAN + dx_p
        dzg_launch_rs_books(d, s->rs_recv1, st);
        dzg_launch_fast_update(d, 0, st);
    } else if (s->batch_chain) {
        dzg_launch_chain_post(d, s->chain_grid, s->chain_bar, s->chain_dbg, 0, 0, recv_dev, st);
    } else {
        dzg_launch_fast_select_prep(d, 5, 0, recv_dev, st);    // merge + (dual) FTRAN prep
        dzg_launch_fast_gemv(d, DZG_STEP_DUAL, recv_dev, st); // + the pivot's books
        dzg_launch_fast_update(d, 0, st);
    }
    if (++s->since_flush >= DZG_RMAX) {
        dzg_launch_fast_flush(d, st);
        s->since_flush = 0;
    }
    phase_stamp(s, DZG_K_UPDATE, 1);
    return 0;
}

// Row-sharded ranks (opts.shard_rows): a record carries a row of the compact inverse, k entries
// wide; the batch being enqueued sends what its bound on k needs (k grows by at most one per
// pivot), not the room for m entries the buffers hold.  0: back to the largest record.
static void rs_batch_stride(dzg_solver *s, int k_bound)
{
    if (!s->d.rs) return;
    long long krow = ((long long)s->d.m + 2 + 15) / 16 * 16;
    if (k_bound > 0) {
        const long long need = ((long long)k_bound + 2 + 15) / 16 * 16;
        if (need < krow) krow = need;
    }
    s->d.xstride = DZG_RS_COL + s->d.rs_mcol + krow;
}

// x and xbar live on their rows' owners while a row-sharded solve runs: every rank gets all of them
// when a run returns (RCCL: one all-gather of the two slices)
static int rs_gather_state(dzg_solver *s)
{
    if (!s->d.rs) return 0;
    Rccl &r = rccl();
    dzg_launch_rs_pack(s->d, s->rs_slice, s->rs_gsend, s->st);
    if (r.AllGather(s->rs_gsend, s->rs_grecv, (size_t)2 * s->rs_slice, kNcclFloat64, s->comm, s->st) != 0)
        return fail(DZG_E_DEVICE, "ncclAllGather (x, xbar of a row-sharded solve)");
    dzg_launch_rs_unpack(s->d, s->rs_slice, s->rs_grecv, s->st);
    HIP_OK(hipStreamSynchronize(s->st));
    return 0;
}

static void shard_comm_destroy(dzg_solver *s)
{
    if (s->comm && rccl().ok) rccl().CommDestroy(s->comm);
    s->comm = nullptr;
}

extern "C" void *dzg_solver_stream(dzg_solver *s) { return s ? (void *)s->st : nullptr; }

extern "C" int dzg_comm_unique_id(void *unique_id_128)
{
    if (!unique_id_128) return fail(DZG_E_ARG, "unique_id is NULL");
    Rccl &r = rccl();
    if (!r.ok) return fail(DZG_E_DEVICE, "librccl could not be loaded");
    NcclUniqueId id;
    const int rc = r.GetUniqueId(&id);
    if (rc != 0) return fail(DZG_E_DEVICE, std::string("ncclGetUniqueId: ") + (r.GetErrorString ? r.GetErrorString(rc) : "?"));
    std::memcpy(unique_id_128, &id, sizeof(id));
    return 0;
}

static int shard_buffers(dzg_solver *s)
{
    if (s->xsend) return 0;
    const size_t n = (size_t)(s->xstride_max ? s->xstride_max : s->d.xstride);
    if (s->d.rs) {
        TRY(dev_alloc(s, &s->rs_gsend, (size_t)2 * s->rs_slice));
        TRY(dev_alloc(s, &s->rs_grecv, (size_t)2 * s->rs_slice * (size_t)s->d.world));
    }
    TRY(dev_alloc(s, &s->xsend, n));
    TRY(dev_alloc(s, &s->xrecv1, n * (size_t)s->d.world));
    TRY(dev_alloc(s, &s->xrecv2, n * (size_t)s->d.world));
    HIP_OK(hipMemsetAsync(s->xsend, 0, sizeof(double) * n, s->st));
    HIP_OK(hipMemsetAsync(s->xrecv1, 0, sizeof(double) * n * s->d.world, s->st));
    HIP_OK(hipMemsetAsync(s->xrecv2, 0, sizeof(double) * n * s->d.world, s->st));
    return 0;
}

extern "C" int dzg_shard_comm_init(dzg_solver *s, const void *unique_id_128)
{
    if (!s || !unique_id_128 || s->d.world < 1) return fail(DZG_E_ARG, "comm_init");
    HIP_OK(hipSetDevice(s->opts.device));
    Rccl &r = rccl();
    if (!r.ok) return fail(DZG_E_DEVICE, "librccl could not be loaded");
    NcclUniqueId id;
    std::memcpy(&id, unique_id_128, sizeof(id));
    const int rc = r.CommInitRank(&s->comm, s->d.world, id, s->d.rank);
    if (rc != 0) return fail(DZG_E_DEVICE, std::string("ncclCommInitRank: ") + (r.GetErrorString ? r.GetErrorString(rc) : "?"));
    return shard_buffers(s);
}

extern "C" int dzg_shard_comm_size(dzg_solver *s)
{
    if (!s || !s->comm) return fail(DZG_E_ARG, "dzg_shard_comm_init first");
    Rccl &r = rccl();
    int n = 0;
    if (!r.CommCount || r.CommCount(s->comm, &n) != 0) return fail(DZG_E_DEVICE, "ncclCommCount");
    return n;
}

extern "C" int dzg_shard_run(dzg_solver *s, int64_t max_new_iters)
{
    if (!s || !s->comm) return fail(DZG_E_ARG, "dzg_shard_comm_init first");
    HIP_OK(hipSetDevice(s->opts.device));
    {
        const int rc0 = set_budget(s, max_new_iters);
        if (rc0 != DZG_RUNNING) return rc0;
    }
    Rccl &r = rccl();
    size_t n = (size_t)s->d.xstride;
    auto t0 = std::chrono::steady_clock::now();
    if (s->pending_refactor) TRY(refactor_now(s)); // a warm start: the starting basis, all ranks together
    for (;;) {
        bool spent = false;
        TRY(budget_spent(s, &spent));
        if (spent) break;
        if (s->opts.refactor_interval > 0 && s->since_refactor >= s->opts.refactor_interval)
            TRY(refactor_now(s));
        const long long before = s->h_ctl->iter;
        const int batch = batch_size(s);
        s->since_flush = s->h_ctl->neta;
        s->since_refactor += batch;
        s->batch_chain = s->chain_bar && (long long)s->h_ctl->ncompact + batch <= s->chain_kcap;
        s->d.price_cols_hint = (int)s->h_ctl->nb_struct + batch;
        s->d.k_hint = (int)s->h_ctl->ncompact + batch; // bounds on k for the launches of this batch
        s->d.k_lo_hint = (int)s->h_ctl->ncompact > batch ? (int)s->h_ctl->ncompact - batch : 0;
        rs_batch_stride(s, s->d.k_hint);
        n = (size_t)s->d.xstride;
        for (int b = 0; b < batch; ++b) {
            s->prof_slot = s->opts.profile ? b : -1;
            TRY(dzg_shard_phase1(s, s->xsend));
            phase_stamp(s, DZG_K_XCHG1, 0);
            if (r.AllGather(s->xsend, s->xrecv1, n, kNcclFloat64, s->comm, s->st) != 0)
                return fail(DZG_E_DEVICE, "ncclAllGather (exchange 1)");
            phase_stamp(s, DZG_K_XCHG1, 1);
            TRY(dzg_shard_phase2(s, s->xrecv1, s->xsend));
            phase_stamp(s, DZG_K_XCHG2, 0);
            if (r.AllGather(s->xsend, s->xrecv2, n, kNcclFloat64, s->comm, s->st) != 0)
                return fail(DZG_E_DEVICE, "ncclAllGather (exchange 2)");
            phase_stamp(s, DZG_K_XCHG2, 1);
            TRY(dzg_shard_phase3(s, s->xrecv2));
        }
        s->prof_slot = -1;
        s->d.k_hint = s->d.k_lo_hint = 0;
        rs_batch_stride(s, 0);
        TRY(read_ctl(s));
        HIP_OK(hipGetLastError());
        if (s->h_ctl->bar_timeout)
            return fail(DZG_E_DEVICE, "a device-wide barrier of the fused phase kernels timed out: their "
                                      "workgroups were not all resident; opts.seven_launches = 1 runs "
                                      "without barriers");
        collect_profile(s, (int)(s->h_ctl->iter - before));
        if (s->h_ctl->status != DZG_RUNNING) break;
        bool stop = false;
        TRY(health_check(s, &stop));
        if (stop) break;
    }
    TRY(rs_gather_state(s));
    s->solve_ms += std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
    return s->h_ctl->status;
}

extern "C" int dzg_shard_run_lockstep(dzg_solver **sv, int32_t world, int64_t max_new_iters)
{
    if (!sv || world < 1) return fail(DZG_E_ARG, "lockstep");
    for (int r = 0; r < world; ++r) {
        if (!sv[r] || sv[r]->d.world != world || sv[r]->d.rank != r || sv[r]->st != sv[0]->st ||
            sv[r]->d.rs != sv[0]->d.rs)
            return fail(DZG_E_ARG, "lockstep: solvers must be ranks 0..world-1 on one stream");
        TRY(shard_buffers(sv[r]));
    }
    struct Flag { // (the ranks refactorise together inside this call, and only here)
        dzg_solver **sv; int world;
        ~Flag() { for (int r = 0; r < world; ++r) sv[r]->in_lockstep = false; }
    } flag{sv, world};
    for (int r = 0; r < world; ++r) sv[r]->in_lockstep = true;
    for (int r = 0; r < world; ++r) {
        const int rc0 = set_budget(sv[r], max_new_iters);
        if (rc0 != DZG_RUNNING) return rc0;
    }
    if (sv[0]->pending_refactor) TRY(refactor_lockstep(sv, world)); // a warm start: the starting basis
    hipStream_t st = sv[0]->st;
    // the all-gather of the lockstep harness: ONE kernel copies every rank's record into every
    // rank's receive buffer (world^2 device copies per exchange would cost more than the ranks'
    // own kernels and blur the per-rank compute this harness is profiled for)
    std::vector<double *> ptrs((size_t)3 * world);
    for (int r = 0; r < world; ++r) {
        ptrs[(size_t)r] = sv[r]->xsend;
        ptrs[(size_t)world + r] = sv[r]->xrecv1;
        ptrs[(size_t)2 * world + r] = sv[r]->xrecv2;
    }
    double **dptrs = nullptr;
    HIP_OK(hipMalloc(&dptrs, sizeof(double *) * ptrs.size()));
    struct Free { double **p; ~Free() { hipFree(p); } } free_ptrs{dptrs};
    HIP_OK(hipMemcpy(dptrs, ptrs.data(), sizeof(double *) * ptrs.size(), hipMemcpyHostToDevice));
    auto exchange = [&](bool second) -> int {
        dzg_launch_lockstep_allgather(dptrs, world, second ? 2 : 1, sv[0]->d.xstride, st);
        return 0;
    };
    for (;;) {
        bool spent = false;
        for (int r = 0; r < world; ++r) TRY(budget_spent(sv[r], &spent));
        if (spent) break;
        if (sv[0]->opts.refactor_interval > 0 && sv[0]->since_refactor >= sv[0]->opts.refactor_interval)
            TRY(refactor_lockstep(sv, world));
        const int batch = batch_size(sv[0]);
        for (int r = 0; r < world; ++r) {
            sv[r]->since_flush = sv[r]->h_ctl->neta;
            sv[r]->since_refactor += batch;
            sv[r]->batch_chain =
                sv[r]->chain_bar && (long long)sv[r]->h_ctl->ncompact + batch <= sv[r]->chain_kcap;
            sv[r]->d.price_cols_hint = (int)sv[r]->h_ctl->nb_struct + batch;
            sv[r]->d.k_hint = (int)sv[r]->h_ctl->ncompact + batch;
            sv[r]->d.k_lo_hint = (int)sv[r]->h_ctl->ncompact > batch ? (int)sv[r]->h_ctl->ncompact - batch : 0;
            rs_batch_stride(sv[r], sv[r]->d.k_hint);
        }
        for (int b = 0; b < batch; ++b) {
            for (int r = 0; r < world; ++r) TRY(dzg_shard_phase1(sv[r], sv[r]->xsend));
            TRY(exchange(false));
            for (int r = 0; r < world; ++r) TRY(dzg_shard_phase2(sv[r], sv[r]->xrecv1, sv[r]->xsend));
            TRY(exchange(true));
            for (int r = 0; r < world; ++r) TRY(dzg_shard_phase3(sv[r], sv[r]->xrecv2));
        }
        for (int r = 0; r < world; ++r) {
            sv[r]->d.k_hint = sv[r]->d.k_lo_hint = 0;
            rs_batch_stride(sv[r], 0);
        }
        for (int r = 0; r < world; ++r) TRY(read_ctl(sv[r]));
        HIP_OK(hipGetLastError());
        for (int r = 0; r < world; ++r)
            if (sv[r]->h_ctl->bar_timeout)
                return fail(DZG_E_DEVICE, "lockstep: a device-wide barrier timed out");
        for (int r = 1; r < world; ++r)
            if (sv[r]->h_ctl->status != sv[0]->h_ctl->status || sv[r]->h_ctl->iter != sv[0]->h_ctl->iter)
                return fail(DZG_E_DEVICE, "lockstep: ranks diverged");
        if (sv[0]->h_ctl->status != DZG_RUNNING) break;
        // the health rule reads replicated state: every rank decides alike, the group acts together
        HealthAction act = HEALTH_OK;
        for (int r = 0; r < world; ++r) {
            const HealthAction a = health_decide(sv[r]);
            if (r > 0 && a != act) return fail(DZG_E_DEVICE, "lockstep: ranks diverged (health rule)");
            act = a;
        }
        bool stop = false;
        if (act == HEALTH_REFACTOR) {
            const int rrc = refactor_lockstep(sv, world);
            if (rrc == DZG_E_DEVICE || rrc == DZG_E_NOMEM) return rrc;
            if (rrc != 0) act = HEALTH_GIVE_UP;
        }
        if (act == HEALTH_GIVE_UP)
            for (int r = 0; r < world; ++r) {
                bool one = false;
                TRY(health_give_up(sv[r], &one));
                stop = stop || one;
            }
        if (stop) break;
    }
    if (sv[0]->d.rs) { // x, xbar of every rank's rows into every rank's arrays
        std::vector<double *> xp((size_t)2 * world);
        for (int r = 0; r < world; ++r) {
            xp[(size_t)r] = sv[r]->d.x;
            xp[(size_t)world + r] = sv[r]->d.xbar;
        }
        double **dxp = nullptr;
        HIP_OK(hipMalloc(&dxp, sizeof(double *) * xp.size()));
        struct FreeX { double **p; ~FreeX() { hipFree(p); } } free_xp{dxp};
        HIP_OK(hipMemcpy(dxp, xp.data(), sizeof(double *) * xp.size(), hipMemcpyHostToDevice));
        dzg_launch_rs_lockstep_gather(dxp, world, sv[0]->d.m, sv[0]->rs_slice, st);
        HIP_OK(hipStreamSynchronize(st));
    }
    return sv[0]->h_ctl->status;
}

extern "C" int dzg_solver_run(dzg_solver *s, int64_t max_new_iters)
{
    if (!s) return fail(DZG_E_ARG, "solver is NULL");
    if (s->d.world > 1) return fail(DZG_E_ARG, "a sharded solver is driven through dzg_shard_run");
    HIP_OK(hipSetDevice(s->opts.device));
    {
        const int rc0 = set_budget(s, max_new_iters);
        if (rc0 != DZG_RUNNING) return rc0;
    }
    auto t0 = std::chrono::steady_clock::now();
    int rc = s->numerics == DZG_NUMERICS_FAST ? run_fast(s) : run_strict(s);
    auto t1 = std::chrono::steady_clock::now();
    s->solve_ms += std::chrono::duration<double, std::milli>(t1 - t0).count();
    if (rc != 0) return rc;
    return s->h_ctl->status;
}

// Test hook: the live-entry lists of a sparse-basis solver (k_price_csc_rl's input) against their
// definition -- column j lists exactly its stored entries whose row has a nonbasic slack
// (dslot >= 0), each once, with the stored value.
extern "C" int64_t dzg_debug_live_lists(dzg_solver *s, int64_t *entries)
{
    if (!s) return fail(DZG_E_ARG, "NULL argument");
    const DzgDev &d = s->d;
    if (!d.spb || !d.lcnt) return fail(DZG_E_ARG, "this solver keeps no live-entry lists");
    HIP_OK(hipSetDevice(s->opts.device));
    TRY(read_ctl(s));
    // a run that stopped between BTRAN and the pivot (DZG_NEAR_TIE) has that pivot's leaving slack
    // row listed already (ctl->rl_listed): by definition part of the lists until the pivot executes
    const int pending = s->h_ctl->rl_listed;
    const size_t ns = (size_t)d.ns, m = (size_t)d.m;
    std::vector<long long> cp(ns + 1);
    std::vector<int> dslot(m), lcnt(ns);
    HIP_OK(hipMemcpy(cp.data(), d.cptr, sizeof(long long) * (ns + 1), hipMemcpyDeviceToHost));
    HIP_OK(hipMemcpy(dslot.data(), d.dslot, sizeof(int) * m, hipMemcpyDeviceToHost));
    HIP_OK(hipMemcpy(lcnt.data(), d.lcnt, sizeof(int) * ns, hipMemcpyDeviceToHost));
    const size_t nnz = (size_t)cp[ns];
    std::vector<int> ri(nnz + 1);
    std::vector<double> cv(nnz + 1);
    std::vector<DzgLiveEntry> lent(nnz + 1);
    if (nnz) {
        HIP_OK(hipMemcpy(ri.data(), d.ridx, sizeof(int) * nnz, hipMemcpyDeviceToHost));
        HIP_OK(hipMemcpy(cv.data(), d.cval, sizeof(double) * nnz, hipMemcpyDeviceToHost));
        HIP_OK(hipMemcpy(lent.data(), d.lent, sizeof(DzgLiveEntry) * nnz, hipMemcpyDeviceToHost));
    }
    int64_t bad = 0, total = 0;
    std::vector<std::pair<int, double>> want, got;
    for (size_t j = 0; j < ns; ++j) {
        want.clear();
        got.clear();
        for (long long e = cp[j]; e < cp[j + 1]; ++e)
            if (dslot[(size_t)ri[(size_t)e]] >= 0 || ri[(size_t)e] == pending)
                want.emplace_back(ri[(size_t)e], cv[(size_t)e]);
        const long long span = cp[j + 1] - cp[j];
        if (lcnt[j] < 0 || lcnt[j] > span) {
            ++bad;
            continue;
        }
        for (int i = 0; i < lcnt[j]; ++i)
            got.emplace_back(lent[(size_t)cp[j] + (size_t)i].row, lent[(size_t)cp[j] + (size_t)i].val);
        std::sort(got.begin(), got.end());
        std::sort(want.begin(), want.end());
        if (got != want) ++bad;
        total += lcnt[j];
    }
    if (entries) *entries = total;
    return bad;
}

extern "C" int64_t dzg_debug_rl_listed(dzg_solver *s)
{
    if (!s) return fail(DZG_E_ARG, "NULL argument");
    if (!s->d.spb || !s->d.lcnt) return fail(DZG_E_ARG, "this solver keeps no live-entry lists");
    HIP_OK(hipSetDevice(s->opts.device));
    TRY(read_ctl(s));
    return s->h_ctl->rl_listed;
}

// Test hook: rows [row0, row1) of the basis inverse FAST keeps, assembled on the host from device
// copies of what the kernels read -- dense: Binv0 (compact columns drow / dslot, unit columns of the
// basic slacks by bcode) minus U W^T; sparse basis: X - Ub^T Wc on the structural positions and
// e_r - A[r, S] (X - Ub^T Wc) on the basic slack of row r (the device's lists bcnt / bcol / bval).
// Row p is basis position p, column r constraint row r; out is row-major (row1 - row0) x m.
extern "C" int dzg_debug_basis_inverse(dzg_solver *s, int64_t row0, int64_t row1, double *out,
                                       int64_t info[4])
{
    if (!s || !info || (row1 > row0 && !out)) return fail(DZG_E_ARG, "NULL argument");
    if (s->numerics != DZG_NUMERICS_FAST) return fail(DZG_E_ARG, "basis inverse: FAST numerics only");
    const DzgDev &d = s->d;
    const int m = d.m;
    const int lo = d.rs ? d.rs_r0 : 0, hi = d.rs ? d.rs_r1 : m;
    if (row0 < lo || row1 > hi || row0 > row1)
        return fail(DZG_E_ARG, "basis inverse: rows outside [" + std::to_string(lo) + ", " +
                                   std::to_string(hi) + ")");
    HIP_OK(hipSetDevice(s->opts.device));
    TRY(read_ctl(s));
    const int k = s->h_ctl->ncompact, neta = s->h_ctl->neta;
    info[0] = k;
    info[1] = neta;
    info[2] = lo;
    info[3] = hi;
    const size_t nr = (size_t)(row1 - row0), mm = (size_t)m;
    if (nr == 0) return 0;
    if (k < 0 || k > m || neta < 0 || neta > DZG_RMAX)
        return fail(DZG_E_DEVICE, "basis inverse: control block out of range");
    const size_t ldb = (size_t)d.ldb, ldw = (size_t)d.ldw;
    std::vector<int> drow(mm), dslot(mm);
    std::vector<double> U((size_t)neta * ldw + 1), W((size_t)neta * ldw + 1);
    HIP_OK(hipMemcpy(drow.data(), d.drow, sizeof(int) * mm, hipMemcpyDeviceToHost));
    HIP_OK(hipMemcpy(dslot.data(), d.dslot, sizeof(int) * mm, hipMemcpyDeviceToHost));
    for (int c = 0; c < k; ++c)
        if (drow[(size_t)c] < 0 || drow[(size_t)c] >= m) return fail(DZG_E_DEVICE, "basis inverse: drow out of range");
    if (neta) {
        HIP_OK(hipMemcpy(U.data(), d.U, sizeof(double) * (size_t)neta * ldw, hipMemcpyDeviceToHost));
        HIP_OK(hipMemcpy(W.data(), d.W, sizeof(double) * (size_t)neta * ldw, hipMemcpyDeviceToHost));
    }
    std::fill(out, out + nr * mm, 0.0);
    if (!d.spb) {
        std::vector<int> bcode(mm);
        HIP_OK(hipMemcpy(bcode.data(), d.bcode, sizeof(int) * mm, hipMemcpyDeviceToHost));
        // (a row-sharded rank's allocation starts at its first row: d.binv points rs_r0 rows before it)
        const double *base = d.binv + (d.rs ? (long long)d.rs_r0 * d.ldb : 0);
        std::vector<double> b0(nr * ldb);
        HIP_OK(hipMemcpy(b0.data(), base + (size_t)(row0 - lo) * ldb, sizeof(double) * nr * ldb,
                         hipMemcpyDeviceToHost));
        for (size_t i = 0; i < nr; ++i) {
            const size_t p = (size_t)row0 + i;
            double *o = out + i * mm;
            for (int c = 0; c < k; ++c) o[drow[(size_t)c]] = b0[i * ldb + (size_t)c];
            if (bcode[p] < 0) o[(size_t)(-1 - bcode[p])] = 1.0;
            for (size_t r = 0; r < mm; ++r) {
                double acc = 0.0;
                for (int t = 0; t < neta; ++t) acc += U[(size_t)t * ldw + p] * W[(size_t)t * ldw + r];
                o[r] -= acc;
            }
        }
        return 0;
    }
    // sparse basis: X (k x k, row b = basis position spos[b], column c = constraint row drow[c])
    std::vector<int> sslot(mm), rowpos(mm), bcnt(mm), bslot((size_t)(d.ns ? d.ns : 1));
    std::vector<long long> rptr(mm + 1);
    HIP_OK(hipMemcpy(sslot.data(), d.sslot, sizeof(int) * mm, hipMemcpyDeviceToHost));
    HIP_OK(hipMemcpy(rowpos.data(), d.rowpos, sizeof(int) * mm, hipMemcpyDeviceToHost));
    HIP_OK(hipMemcpy(bcnt.data(), d.bcnt, sizeof(int) * mm, hipMemcpyDeviceToHost));
    HIP_OK(hipMemcpy(bslot.data(), d.bslot, sizeof(int) * (size_t)(d.ns ? d.ns : 1), hipMemcpyDeviceToHost));
    HIP_OK(hipMemcpy(rptr.data(), d.rptr, sizeof(long long) * (mm + 1), hipMemcpyDeviceToHost));
    const size_t nnz = (size_t)rptr[mm];
    std::vector<int> bcol(nnz + 1);
    std::vector<double> bval(nnz + 1), X((size_t)k * ldb + 1);
    if (nnz) {
        HIP_OK(hipMemcpy(bcol.data(), d.bcol, sizeof(int) * nnz, hipMemcpyDeviceToHost));
        HIP_OK(hipMemcpy(bval.data(), d.bval, sizeof(double) * nnz, hipMemcpyDeviceToHost));
    }
    if (k) HIP_OK(hipMemcpy(X.data(), d.binv, sizeof(double) * (size_t)k * ldb, hipMemcpyDeviceToHost));
    // the effective X row by row, on first need
    std::vector<double> Xe((size_t)k * (size_t)k);
    std::vector<char> done((size_t)k, 0);
    auto xrow = [&](int b) -> const double * {
        double *e = Xe.data() + (size_t)b * (size_t)k;
        if (!done[(size_t)b]) {
            for (int c = 0; c < k; ++c) {
                double acc = 0.0;
                for (int t = 0; t < neta; ++t)
                    acc += U[(size_t)t * ldw + (size_t)b] * W[(size_t)t * ldw + (size_t)c];
                e[c] = X[(size_t)b * ldb + (size_t)c] - acc;
            }
            done[(size_t)b] = 1;
        }
        return e;
    };
    std::vector<int> slack_row(mm, -1); // basis position -> the constraint row of its basic slack
    for (size_t r = 0; r < mm; ++r)
        if (rowpos[r] >= 0 && rowpos[r] < m) slack_row[(size_t)rowpos[r]] = (int)r;
    for (size_t i = 0; i < nr; ++i) {
        const size_t p = (size_t)row0 + i;
        double *o = out + i * mm;
        const int b = sslot[p];
        if (b >= 0) {
            if (b >= k) return fail(DZG_E_DEVICE, "basis inverse: sslot out of range");
            const double *e = xrow(b);
            for (int c = 0; c < k; ++c) o[drow[(size_t)c]] = e[c];
            continue;
        }
        const int r = slack_row[p];
        if (r < 0) return fail(DZG_E_DEVICE, "basis inverse: position without a variable");
        o[(size_t)r] = 1.0;
        for (int j = 0; j < bcnt[(size_t)r]; ++j) {
            const size_t at = (size_t)rptr[(size_t)r] + (size_t)j;
            const int bb = bslot[(size_t)bcol[at]];
            if (bb < 0 || bb >= k) return fail(DZG_E_DEVICE, "basis inverse: bslot out of range");
            const double *e = xrow(bb);
            for (int c = 0; c < k; ++c) o[drow[(size_t)c]] -= bval[at] * e[c];
        }
    }
    return 0;
}

extern "C" int dzg_solver_result(dzg_solver *s, dzg_result *res)
{
    if (!s || !res) return fail(DZG_E_ARG, "NULL argument");
    HIP_OK(hipSetDevice(s->opts.device));
    TRY(read_ctl(s));
    const DzgDev &d = s->d;
    const int m = d.m, q = d.q;
    res->status = s->h_ctl->status;
    res->numerics_used = s->numerics;
    res->iterations = s->h_ctl->iter;
    std::vector<int> basis((size_t)(m ? m : 1)), nonbasis((size_t)(q ? q : 1));
    std::vector<double> x((size_t)(m ? m : 1));
    if (m) {
        HIP_OK(hipMemcpy(basis.data(), d.basis, sizeof(int) * m, hipMemcpyDeviceToHost));
        HIP_OK(hipMemcpy(x.data(), d.x, sizeof(double) * m, hipMemcpyDeviceToHost));
    }
    if (q) HIP_OK(hipMemcpy(nonbasis.data(), d.nonbasis, sizeof(int) * q, hipMemcpyDeviceToHost));
    // objective_value, src/simplex.rs:345-352, summed in basis-position order
    double sum = 0.0;
    for (int p = 0; p < m; ++p) {
        const double prod = s->c_host[(size_t)basis[p]] * x[p];
        sum = sum + prod;
    }
    res->objective = s->constant + sum;
    if (res->basis) for (int p = 0; p < m; ++p) res->basis[p] = basis[p];
    if (res->nonbasis) for (int k = 0; k < q; ++k) res->nonbasis[k] = nonbasis[k];
    if (res->x && m) std::memcpy(res->x, x.data(), sizeof(double) * m);
    if (res->xbar && m) HIP_OK(hipMemcpy(res->xbar, d.xbar, sizeof(double) * m, hipMemcpyDeviceToHost));
    if (res->z && q) HIP_OK(hipMemcpy(res->z, d.z, sizeof(double) * q, hipMemcpyDeviceToHost));
    if (res->zbar && q) HIP_OK(hipMemcpy(res->zbar, d.zbar, sizeof(double) * q, hipMemcpyDeviceToHost));
    if (res->log && res->log_cap > 0) {
        long long cnt = res->iterations < d.log_cap ? res->iterations : d.log_cap;
        if (cnt > res->log_cap) cnt = res->log_cap;
        if (cnt > 0) {
            std::vector<int> kind((size_t)cnt), en((size_t)cnt), le((size_t)cnt);
            std::vector<double> mu((size_t)cnt);
            HIP_OK(hipMemcpy(kind.data(), d.log_kind, sizeof(int) * cnt, hipMemcpyDeviceToHost));
            HIP_OK(hipMemcpy(en.data(), d.log_enter, sizeof(int) * cnt, hipMemcpyDeviceToHost));
            HIP_OK(hipMemcpy(le.data(), d.log_leave, sizeof(int) * cnt, hipMemcpyDeviceToHost));
            HIP_OK(hipMemcpy(mu.data(), d.log_mu, sizeof(double) * cnt, hipMemcpyDeviceToHost));
            for (long long i = 0; i < cnt; ++i) {
                res->log[i].kind = kind[(size_t)i];
                res->log[i].reserved = 0;
                res->log[i].entering = en[(size_t)i];
                res->log[i].leaving = le[(size_t)i];
                res->log[i].mu = mu[(size_t)i];
            }
        }
    }
    for (int c = 0; c < DZG_K_COUNT; ++c) {
        res->kernel_ms[c] = s->kernel_ms[c];
        res->kernel_launches[c] = s->kernel_launches[c];
    }
    res->price_bytes = s->h_ctl->price_bytes;
    if (s->d.rl_work) { // live-entry pricing counts the entries it walked itself: 16-byte records
        std::vector<unsigned long long> w(DZG_RL_WORK_SLOTS);
        HIP_OK(hipMemcpyAsync(w.data(), s->d.rl_work, sizeof(unsigned long long) * w.size(),
                              hipMemcpyDeviceToHost, s->st));
        HIP_OK(hipStreamSynchronize(s->st));
        unsigned long long walked = 0;
        for (unsigned long long x : w) walked += x;
        res->price_bytes += 16.0 * (double)walked;
    }
    res->solve_ms = s->solve_ms;
    res->max_pivot_error = s->max_err_life;
    res->near_ties = s->h_ctl->near_ties;
    res->first_near_tie = s->h_ctl->first_near_tie;
    res->min_margin = s->h_ctl->min_margin;
    res->dense_columns = s->numerics == DZG_NUMERICS_FAST ? s->h_ctl->ncompact : 0;
    res->refactors = s->refactors;
    res->chain_fallbacks = s->chain_fallbacks;
    res->price_pass_used = s->numerics == DZG_NUMERICS_FAST && !s->d.csc ? s->h_ctl->price_mask : 0;
    res->price_rows_copy = s->d.At ? 1 : 0;
    res->state_drift = s->state_drift;
    if (res->margins && res->log_cap > 0 && s->numerics == DZG_NUMERICS_FAST) {
        long long cnt = res->iterations < d.log_cap ? res->iterations : d.log_cap;
        if (cnt > res->log_cap) cnt = res->log_cap;
        if (cnt > 0)
            HIP_OK(hipMemcpy(res->margins, d.log_margin, sizeof(double) * cnt, hipMemcpyDeviceToHost));
    }
    return 0;
}

// ---- what the calls on a finished solver share ---------------------------
// s->du_c, s->du_rhs0, s->du_ctl and the zero pads of s->du_y mirror the handle's own data: filled once
// by duals_workspace, the first two refreshed by restart_state, read by every call.  Anything else in
// the scratch buffers a call uploads or computes itself before it reads it, but s->du_d, which
// dzg_solver_ranging takes from the dzg_solver_duals call it makes.
// The two refusals that depend on how the solver was created, placed by each caller where its order of
// checks has them.  `unsupported`: the whole sentence where it is not "<what> is not supported ...".
static int dense_one_gpu_only(const dzg_solver *s, const char *what, const char *unsupported = nullptr)
{
    if (s->d.csc || s->d.world > 1)
        return fail(DZG_E_ARG, unsupported ? std::string(unsupported)
                                           : std::string(what) + " is not supported on CSC storage or sharded solvers");
    return 0;
}

static int fast_needs_workspace(const dzg_solver *s, const char *what)
{
    if (s->numerics == DZG_NUMERICS_FAST && !s->rf_piv)
        return fail(DZG_E_ARG, std::string(what) + ": a FAST solver needs its refactorisation workspace: "
                                                   "create it with opts.refactor_interval != 0");
    return 0;
}

// a basis can be carried on from before a run and after any end but singular / panic
static int carry_on_status_ok(const char *what, int status)
{
    if (status == DZG_SINGULAR || status == DZG_PANIC || status < 0 || status > DZG_NEAR_TIE)
        return fail(DZG_E_ARG, std::string(what) + ": the solver's status is " + dzg_status_str(status) +
                                   ": its basis cannot be carried on from");
    return 0;
}

static int singular_block(const char *what, const char *which)
{
    return fail(DZG_E_DEVICE, std::string(what) + ": the " + which + " basis did not refactorise (singular block)");
}

// FAST: a fresh inverse of the current basis, the eta file emptied (s->h_ctl is current).  Where
// k_ref_done met a singular block the status is put back on both sides: the solve's outcome stays.
static int fresh_inverse(dzg_solver *s, const char *what, const char *which_basis)
{
    const int status = s->h_ctl->status;
    TRY(refactor_now(s, true));
    TRY(read_ctl(s));
    if (s->h_ctl->status != status) {
        HIP_OK(hipMemcpy(&s->d.ctl->status, &status, sizeof(int), hipMemcpyHostToDevice));
        s->h_ctl->status = status;
        return singular_block(what, which_basis);
    }
    return 0;
}

// the lists of the current basis on the host (one entry at least: data() is never NULL); codes: upload_codes
struct BasisLists {
    std::vector<int> basis, nonbasis, codes;
};

static int fetch_lists(dzg_solver *s, BasisLists &lists)
{
    const int m = s->d.m, q = s->d.q;
    lists.basis.assign((size_t)(m ? m : 1), 0);
    lists.nonbasis.assign((size_t)(q ? q : 1), 0);
    if (m) HIP_OK(hipMemcpyAsync(lists.basis.data(), s->d.basis, sizeof(int) * m, hipMemcpyDeviceToHost, s->st));
    if (q) HIP_OK(hipMemcpyAsync(lists.nonbasis.data(), s->d.nonbasis, sizeof(int) * q, hipMemcpyDeviceToHost, s->st));
    HIP_OK(hipStreamSynchronize(s->st));
    return 0;
}

// STRICT: the column codes of the nonbasic variables, queued for s->du_codes (the sequential pricing pass
// reads them) from lists.codes: the caller synchronises the stream before `lists` or that pass goes on
static int upload_codes(dzg_solver *s, BasisLists &lists)
{
    const int q = s->d.q;
    lists.codes.assign((size_t)(q ? q : 1), 0);
    for (int k = 0; k < q; ++k) lists.codes[(size_t)k] = s->var_col_host[(size_t)lists.nonbasis[(size_t)k]];
    if (q) HIP_OK(hipMemcpyAsync(s->du_codes, lists.codes.data(), sizeof(int) * q, hipMemcpyHostToDevice, s->st));
    return 0;
}

// STRICT: the copy of the device view that the LU kernels of every STRICT FTRAN / BTRAN run on here: its
// control block is the scratch one, which reads DZG_RUNNING (the solver's own is left alone), v is s->du_y
static DzgDev strict_view(const dzg_solver *s, double *dx)
{
    DzgDev dd = s->d;
    dd.ctl = s->du_ctl;
    dd.v = s->du_y;
    dd.dx = dx;
    return dd;
}

// init + sum (or - sum) of a[idx ? idx[i] : i] * b[i] in the reference's order: ascending, one rounded
// product and one rounded sum or difference per element
static double dot_reference_order(const std::vector<double> &a, const int *idx, const std::vector<double> &b,
                                  int count, double init = 0.0, bool subtract = false)
{
    double acc = init;
    for (int i = 0; i < count; ++i) {
        const double prod = a[(size_t)(idx ? idx[i] : i)] * b[(size_t)i];
        acc = subtract ? acc - prod : acc + prod;
    }
    return acc;
}

// (`count` runs of `len` entries, `ld` apart)
static int finite_block(const char *prefix, const char *name, const double *v, int64_t len, int64_t count, int64_t ld)
{
    for (int64_t j = 0; v && j < count; ++j)
        for (int64_t i = 0; i < len; ++i)
            if (!std::isfinite(v[j * ld + i]))
                return fail(DZG_E_ARG, std::string(prefix) + name + "[" + std::to_string(j * ld + i) +
                                           "] is not finite");
    return 0;
}

// ---- dual values and reduced costs at the optimum (k_duals.hip) -------------
static int duals_workspace(dzg_solver *s)
{
    if (s->du_out) return 0;
    const DzgDev &d = s->d;
    const size_t m = (size_t)d.m, q = (size_t)d.q, n = (size_t)d.n;
    TRY(dev_alloc(s, &s->du_c, n)); TRY(dev_alloc(s, &s->du_rhs0, m));
    TRY(dev_alloc(s, &s->du_y, m + 2)); TRY(dev_alloc(s, &s->du_dzy, q));
    TRY(dev_alloc(s, &s->du_d, n));
    if (s->numerics == DZG_NUMERICS_FAST) {
        TRY(dev_alloc(s, &s->du_part, (size_t)dzg_drift_chunks() * (size_t)d.ldw));
    } else {
        TRY(dev_alloc(s, &s->du_codes, q));
        TRY(dev_alloc(s, &s->du_ctl, 1));
        DzgCtl c0;
        std::memset(&c0, 0, sizeof(c0));
        c0.status = DZG_RUNNING; // the LU kernels are no-ops under any other status
        HIP_OK(hipMemcpyAsync(s->du_ctl, &c0, sizeof(c0), hipMemcpyHostToDevice, s->st));
        HIP_OK(hipStreamSynchronize(s->st)); // (c0 is a local)
    }
    if (n) HIP_OK(hipMemcpyAsync(s->du_c, s->c_host.data(), sizeof(double) * n, hipMemcpyHostToDevice, s->st));
    if (m) HIP_OK(hipMemcpyAsync(s->du_rhs0, s->x0_host.data(), sizeof(double) * m, hipMemcpyHostToDevice, s->st));
    HIP_OK(hipMemsetAsync(s->du_y, 0, sizeof(double) * (m + 2), s->st)); // (the two pads stay zero)
    TRY(dev_alloc(s, &s->du_out, (size_t)DZG_DUALS_BLOCKS * DZG_DUALS_PART)); // set last: "reserved"
    return 0;
}

extern "C" int dzg_solver_duals(dzg_solver *s, dzg_duals *out)
{
    if (!s || !out) return fail(DZG_E_ARG, "duals: NULL argument");
    HIP_OK(hipSetDevice(s->opts.device));
    TRY(read_ctl(s));
    if (s->h_ctl->status != DZG_OPTIMAL)
        return fail(DZG_E_ARG, "duals: the solver's status is not DZG_OPTIMAL");
    const DzgDev &d = s->d;
    const int m = d.m, q = d.q, n = d.n;
    hipStream_t st = s->st;
    BasisLists lists;
    TRY(fetch_lists(s, lists));
    const std::vector<int> &basis = lists.basis, &nonbasis = lists.nonbasis;
    std::vector<double> x((size_t)(m ? m : 1)), z((size_t)(q ? q : 1));
    if (m) HIP_OK(hipMemcpy(x.data(), d.x, sizeof(double) * m, hipMemcpyDeviceToHost));
    if (q) HIP_OK(hipMemcpy(z.data(), d.z, sizeof(double) * q, hipMemcpyDeviceToHost));
    out->reserved = 0;
    // objective_value as dzg_solver_result forms it
    out->primal_obj = s->constant + dot_reference_order(s->c_host, basis.data(), x, m);
    std::vector<double> y((size_t)(m ? m : 1), 0.0), dv((size_t)(n ? n : 1), 0.0);
    double dmin = std::numeric_limits<double>::infinity(), dabs = 0.0, zdiff = 0.0, xmin = dmin, dot = 0.0;
    const auto give = [&](int source) {
        out->source = source;
        out->dual_obj = s->constant + dot;
        out->primal_infeas = std::max(0.0, -xmin);
        out->dual_infeas = std::max(0.0, -dmin);
        out->z_diff = zdiff / std::max(1.0, dabs); // (carried: 0)
        if (out->y && m) std::memcpy(out->y, y.data(), sizeof(double) * m);
        if (out->d && n) std::memcpy(out->d, dv.data(), sizeof(double) * n);
        return 0;
    };

    if (d.csc || d.world > 1) {
        // carried: the slack entries of z are the dual vector, z the reduced costs
        for (int k = 0; k < q; ++k) {
            const int var = nonbasis[k], code = s->var_col_host[(size_t)var];
            dv[(size_t)var] = z[k];
            if (code < 0) y[(size_t)(-1 - code)] = z[k];
            dmin = std::min(dmin, z[k]);
        }
        for (int p = 0; p < m; ++p) xmin = std::min(xmin, x[p]);
        dot = dot_reference_order(s->x0_host, nullptr, y, m);
        return give(DZG_DUALS_CARRIED);
    }

    const bool fast = s->numerics == DZG_NUMERICS_FAST;
    TRY(fast_needs_workspace(s, "duals"));
    TRY(duals_workspace(s));
    if (fast) {
        // on the fresh inverse y by the two-stage scheme of the drift measurement on buffers of our
        // own, then one column-wise pricing pass with y as v
        TRY(fresh_inverse(s, "duals", "optimal"));
        dzg_launch_drift_y(d, s->du_c, s->du_part, s->du_y, (int)s->h_ctl->ncompact, st);
        dzg_launch_price_raw(DZG_PRICE_TREE, m, d.lda, d.A, d.nbcode, q, s->du_y, s->du_dzy, st);
    } else {
        // B^T y = c_B by the LU of every STRICT BTRAN, then neg_t_dot in the reference's order
        std::vector<double> cb((size_t)(m ? m : 1));
        for (int p = 0; p < m; ++p) cb[(size_t)p] = s->c_host[(size_t)basis[p]];
        if (m) HIP_OK(hipMemcpyAsync(s->du_y, cb.data(), sizeof(double) * m, hipMemcpyHostToDevice, st));
        TRY(upload_codes(s, lists));
        HIP_OK(hipStreamSynchronize(st)); // (cb is a local)
        const DzgDev dd = strict_view(s, d.dx);
        dzg_launch_strict_solve(dd, 1, st);
        dzg_launch_price_raw(DZG_PRICE_SEQ, m, d.lda, d.A, s->du_codes, q, s->du_y, s->du_dzy, st);
    }
    dzg_launch_duals_finish(m, q, d.basis, d.nonbasis, s->du_c, s->du_dzy, d.z, d.x, s->du_rhs0, s->du_y,
                            s->du_d, s->du_out, st);
    std::vector<double> part((size_t)DZG_DUALS_BLOCKS * DZG_DUALS_PART);
    HIP_OK(hipMemcpyAsync(part.data(), s->du_out, sizeof(double) * part.size(), hipMemcpyDeviceToHost, st));
    if (m) HIP_OK(hipMemcpyAsync(y.data(), s->du_y, sizeof(double) * m, hipMemcpyDeviceToHost, st));
    if (n) HIP_OK(hipMemcpyAsync(dv.data(), s->du_d, sizeof(double) * n, hipMemcpyDeviceToHost, st));
    HIP_OK(hipStreamSynchronize(st));
    HIP_OK(hipGetLastError());
    for (int b = 0; b < DZG_DUALS_BLOCKS; ++b) { // workgroup order
        const double *r = &part[(size_t)b * DZG_DUALS_PART];
        dmin = std::min(dmin, r[0]);
        dabs = std::max(dabs, r[1]);
        zdiff = std::max(zdiff, r[2]);
        xmin = std::min(xmin, r[3]);
        dot = dot + r[4];
    }
    if (!fast) dot = dot_reference_order(s->x0_host, nullptr, y, m); // not the workgroups' sum: rows ascending
    return give(DZG_DUALS_FRESH);
}

// "no duals": an LP that did not end OPTIMAL, or whose duals could not be computed (k_batch.hip and
// model.cpp use it too)
void dzg_duals_none(dzg_duals *du, double objective)
{
    du->source = 0;
    du->reserved = 0;
    du->primal_obj = objective;
    du->dual_obj = du->primal_infeas = du->dual_infeas = du->z_diff = 0.0;
}

// ---- sensitivity ranging at the optimum (k_ranging.hip) ----------------------
static bool ranging_side_valid(const char *name, int64_t count, const int64_t *ptr, const int64_t *idx,
                               const double *val, int64_t bound, std::vector<int64_t> &mark, std::string &why)
{
    const std::string at = std::string("ranging: ") + name;
    if (count < 0) { why = at + " count < 0"; return false; }
    if (count == 0) return true;
    if (count >= (1ll << 31) - 64) { why = at + " count out of range"; return false; }
    if (!ptr) { why = at + "_ptr is NULL"; return false; }
    if (ptr[0] != 0) { why = at + "_ptr[0] != 0"; return false; }
    for (int64_t i = 0; i < count; ++i)
        if (ptr[i + 1] < ptr[i]) { why = at + "_ptr decreases"; return false; }
    if (ptr[count] > 0 && (!idx || !val)) { why = at + "_idx or " + name + "_val is NULL"; return false; }
    mark.assign((size_t)(bound > 0 ? bound : 1), -1);
    for (int64_t i = 0; i < count; ++i)
        for (int64_t e = ptr[i]; e < ptr[i + 1]; ++e) {
            const int64_t j = idx[e];
            if (j < 0 || j >= bound) {
                why = at + " direction " + std::to_string(i) + ": index " + std::to_string(j) + " out of range";
                return false;
            }
            if (mark[(size_t)j] == i) {
                why = at + " direction " + std::to_string(i) + ": index " + std::to_string(j) + " is repeated";
                return false;
            }
            mark[(size_t)j] = i;
        }
    return true;
}

bool dzg_ranging_req_valid(const dzg_ranging_req *req, int64_t m, int64_t n, std::string &why)
{
    if (!req) { why = "ranging: req is NULL"; return false; }
    if (!(req->pivot_tol >= 0.0)) { why = "ranging: pivot_tol is negative or NaN"; return false; }
    std::vector<int64_t> mark;
    return ranging_side_valid("cost", req->ncost, req->cost_ptr, req->cost_idx, req->cost_val, n, mark, why) &&
           ranging_side_valid("rhs", req->nrhs, req->rhs_ptr, req->rhs_idx, req->rhs_val, m, mark, why);
}

void dzg_ranging_none(const dzg_ranging_req *req, dzg_ranging *rg)
{
    const double nan = std::numeric_limits<double>::quiet_NaN();
    for (int64_t i = 0; i < req->ncost; ++i) {
        if (rg->cost_lo) rg->cost_lo[i] = nan;
        if (rg->cost_hi) rg->cost_hi[i] = nan;
        if (rg->cost_lo_var) rg->cost_lo_var[i] = -1;
        if (rg->cost_hi_var) rg->cost_hi_var[i] = -1;
    }
    for (int64_t i = 0; i < req->nrhs; ++i) {
        if (rg->rhs_lo) rg->rhs_lo[i] = nan;
        if (rg->rhs_hi) rg->rhs_hi[i] = nan;
        if (rg->rhs_lo_var) rg->rhs_lo_var[i] = -1;
        if (rg->rhs_hi_var) rg->rhs_hi_var[i] = -1;
    }
}

namespace {
// device memory of one dzg_solver_ranging call
struct RangeArena {
    std::vector<void *> ptrs;
    ~RangeArena()
    {
        for (void *p : ptrs) (void)hipFree(p);
    }
    template <typename T> int get(T **p, size_t count)
    {
        void *q = nullptr;
        const size_t bytes = sizeof(T) * (count ? count : 1);
        if (hipMalloc(&q, bytes) != hipSuccess)
            return fail(DZG_E_NOMEM, "ranging: hipMalloc of " + std::to_string(bytes) + " bytes failed");
        ptrs.push_back(q);
        *p = static_cast<T *>(q);
        return 0;
    }
    template <typename T> int put(T **p, const std::vector<T> &h, hipStream_t st)
    {
        TRY(get(p, h.size()));
        if (!h.empty())
            HIP_OK(hipMemcpyAsync(*p, h.data(), sizeof(T) * h.size(), hipMemcpyHostToDevice, st));
        return 0;
    }
};
} // namespace

extern "C" int dzg_solver_ranging(dzg_solver *s, const dzg_ranging_req *req, dzg_duals *duals,
                                  dzg_ranging *out)
{
    if (!s || !req || !out) return fail(DZG_E_ARG, "ranging: NULL argument");
    HIP_OK(hipSetDevice(s->opts.device));
    const DzgDev &d = s->d;
    const int m = d.m, q = d.q, n = d.n;
    std::string why;
    if (!dzg_ranging_req_valid(req, m, n, why)) return fail(DZG_E_ARG, why);
    TRY(read_ctl(s));
    if (s->h_ctl->status != DZG_OPTIMAL)
        return fail(DZG_E_ARG, "ranging: the solver's status is not DZG_OPTIMAL");
    TRY(dense_one_gpu_only(s, "ranging",
                           "ranging is not supported on CSC storage or sharded solvers: a range cannot "
                           "be read off the carried z"));
    dzg_duals tmp;
    std::memset(&tmp, 0, sizeof(tmp));
    // (leaves the fresh d by variable in s->du_d and, FAST, the fresh inverse: all that is read of its scratch)
    TRY(dzg_solver_duals(s, duals ? duals : &tmp));
    const double tol = req->pivot_tol == 0.0 ? 1e-9 : req->pivot_tol;
    const int nc = (int)req->ncost, nr = (int)req->nrhs;
    hipStream_t st = s->st;

    BasisLists lists;
    TRY(fetch_lists(s, lists));
    const std::vector<int> &basis = lists.basis, &nonbasis = lists.nonbasis;
    std::vector<int> where((size_t)(n ? n : 1), 0); // variable -> basis position p, or -1 - nonbasic position
    for (int p = 0; p < m; ++p) where[(size_t)basis[p]] = p;
    for (int k = 0; k < q; ++k) where[(size_t)nonbasis[k]] = -1 - k;

    RangeArena mem;
    const int nd = nc + nr; // results: cost directions first, then right-hand-side directions
    double *o_lo = nullptr, *o_hi = nullptr;
    int *o_lok = nullptr, *o_hik = nullptr;
    DzgRangePart *part = nullptr;
    TRY(mem.get(&o_lo, (size_t)nd)); TRY(mem.get(&o_hi, (size_t)nd));
    TRY(mem.get(&o_lok, (size_t)nd)); TRY(mem.get(&o_hik, (size_t)nd));

    if (s->numerics == DZG_NUMERICS_FAST) {
        // the eta file is empty after the refactorisation of dzg_solver_duals: Binv = Binv0
        const int k = (int)s->h_ctl->ncompact;
        const int rt = dzg_range_row_tiles(m), ct = dzg_range_col_tiles(q), ldy = dzg_range_ldy(m);
        std::vector<long long> hptr((size_t)nr + 1, 0), bptr((size_t)nc + 1, 0), nptr((size_t)nc + 1, 0);
        std::vector<int> hidx, bidx, nidx;
        std::vector<double> hval, bval, nval;
        for (int i = 0; i < nr; ++i) {
            for (int64_t e = req->rhs_ptr[i]; e < req->rhs_ptr[i + 1]; ++e) {
                hidx.push_back((int)req->rhs_idx[e]);
                hval.push_back(req->rhs_val[e]);
            }
            hptr[(size_t)i + 1] = (long long)hidx.size();
        }
        for (int i = 0; i < nc; ++i) {
            for (int64_t e = req->cost_ptr[i]; e < req->cost_ptr[i + 1]; ++e) {
                const int w = where[(size_t)req->cost_idx[e]];
                if (w >= 0) {
                    bidx.push_back(w);
                    bval.push_back(req->cost_val[e]);
                } else {
                    nidx.push_back(-1 - w);
                    nval.push_back(req->cost_val[e]);
                }
            }
            bptr[(size_t)i + 1] = (long long)bidx.size();
            nptr[(size_t)i + 1] = (long long)nidx.size();
        }
        long long *d_hptr = nullptr, *d_bptr = nullptr, *d_nptr = nullptr;
        int *d_hidx = nullptr, *d_bidx = nullptr, *d_nidx = nullptr;
        double *d_hval = nullptr, *d_bval = nullptr, *d_nval = nullptr, *Y = nullptr, *GN = nullptr;
        TRY(mem.put(&d_hptr, hptr, st)); TRY(mem.put(&d_hidx, hidx, st)); TRY(mem.put(&d_hval, hval, st));
        TRY(mem.put(&d_bptr, bptr, st)); TRY(mem.put(&d_bidx, bidx, st)); TRY(mem.put(&d_bval, bval, st));
        TRY(mem.put(&d_nptr, nptr, st)); TRY(mem.put(&d_nidx, nidx, st)); TRY(mem.put(&d_nval, nval, st));
        const int chunk_c = std::min(nc, DZG_RANGE_CHUNK), chunk_r = std::min(nr, DZG_RANGE_CHUNK);
        TRY(mem.get(&part, std::max((size_t)chunk_c * (size_t)ct, (size_t)chunk_r * (size_t)rt)));
        TRY(mem.get(&Y, (size_t)chunk_c * (size_t)ldy));
        TRY(mem.get(&GN, (size_t)chunk_c * (size_t)q));
        const DzgRangeDirs H{d_hptr, d_hidx, d_hval}, GB{d_bptr, d_bidx, d_bval}, GNd{d_nptr, d_nidx, d_nval};
        for (int dir0 = 0; dir0 < nc; dir0 += DZG_RANGE_CHUNK) {
            const int cnt = std::min(DZG_RANGE_CHUNK, nc - dir0);
            if (q) HIP_OK(hipMemsetAsync(GN, 0, sizeof(double) * (size_t)cnt * (size_t)q, st));
            dzg_launch_range_cost_y(d, k, GB, GNd, dir0, cnt, Y, GN, st);
            dzg_launch_range_cost_mfma(d, s->du_d, Y, GN, cnt, tol, part, st);
            dzg_launch_range_finish(part, q > 0 ? ct : 0, cnt, o_lo + dir0, o_hi + dir0, o_lok + dir0,
                                    o_hik + dir0, st);
        }
        for (int dir0 = 0; dir0 < nr; dir0 += DZG_RANGE_CHUNK) {
            const int cnt = std::min(DZG_RANGE_CHUNK, nr - dir0);
            dzg_launch_range_rhs_fast(d, k, H, dir0, cnt, tol, part, st);
            dzg_launch_range_finish(part, rt, cnt, o_lo + nc + dir0, o_hi + nc + dir0, o_lok + nc + dir0,
                                    o_hik + nc + dir0, st);
        }
        HIP_OK(hipGetLastError());
        HIP_OK(hipStreamSynchronize(st)); // (the CSR vectors are locals)
    } else {
        // one LU solve of every STRICT FTRAN / BTRAN per direction; a cost direction also takes the
        // sequential pricing pass
        double *dxv = nullptr, *gn = nullptr;
        TRY(mem.get(&dxv, (size_t)m + 2)); TRY(mem.get(&gn, (size_t)q));
        TRY(mem.get(&part, (size_t)DZG_RANGE_BLOCKS));
        TRY(upload_codes(s, lists));
        HIP_OK(hipStreamSynchronize(st));
        const DzgDev dd = strict_view(s, dxv);
        std::vector<double> hv((size_t)(m ? m : 1)), gv((size_t)(q ? q : 1));
        for (int i = 0; i < nc; ++i) {
            std::fill(hv.begin(), hv.end(), 0.0);
            std::fill(gv.begin(), gv.end(), 0.0);
            for (int64_t e = req->cost_ptr[i]; e < req->cost_ptr[i + 1]; ++e) {
                const int w = where[(size_t)req->cost_idx[e]];
                if (w >= 0) hv[(size_t)w] = req->cost_val[e]; else gv[(size_t)(-1 - w)] = req->cost_val[e];
            }
            if (m) HIP_OK(hipMemcpyAsync(s->du_y, hv.data(), sizeof(double) * m, hipMemcpyHostToDevice, st));
            if (q) HIP_OK(hipMemcpyAsync(gn, gv.data(), sizeof(double) * q, hipMemcpyHostToDevice, st));
            if (m) dzg_launch_strict_solve(dd, 1, st);
            dzg_launch_price_raw(DZG_PRICE_SEQ, m, d.lda, d.A, s->du_codes, q, s->du_y, s->du_dzy, st);
            dzg_launch_range_ratio(q, s->du_dzy, gn, s->du_d, d.nonbasis, tol, part, st);
            dzg_launch_range_finish(part, DZG_RANGE_BLOCKS, 1, o_lo + i, o_hi + i, o_lok + i, o_hik + i, st);
            HIP_OK(hipStreamSynchronize(st)); // (hv and gv are reused)
        }
        for (int i = 0; i < nr; ++i) {
            std::fill(hv.begin(), hv.end(), 0.0);
            for (int64_t e = req->rhs_ptr[i]; e < req->rhs_ptr[i + 1]; ++e)
                hv[(size_t)req->rhs_idx[e]] = req->rhs_val[e];
            if (m) HIP_OK(hipMemcpyAsync(dxv, hv.data(), sizeof(double) * m, hipMemcpyHostToDevice, st));
            if (m) dzg_launch_strict_solve(dd, 0, st);
            dzg_launch_range_ratio(m, dxv, nullptr, d.x, nullptr, tol, part, st);
            dzg_launch_range_finish(part, DZG_RANGE_BLOCKS, 1, o_lo + nc + i, o_hi + nc + i, o_lok + nc + i,
                                    o_hik + nc + i, st);
            HIP_OK(hipStreamSynchronize(st));
        }
        HIP_OK(hipGetLastError());
    }

    std::vector<double> lo((size_t)(nd ? nd : 1)), hi((size_t)(nd ? nd : 1));
    std::vector<int> lok((size_t)(nd ? nd : 1)), hik((size_t)(nd ? nd : 1));
    if (nd) {
        HIP_OK(hipMemcpyAsync(lo.data(), o_lo, sizeof(double) * nd, hipMemcpyDeviceToHost, st));
        HIP_OK(hipMemcpyAsync(hi.data(), o_hi, sizeof(double) * nd, hipMemcpyDeviceToHost, st));
        HIP_OK(hipMemcpyAsync(lok.data(), o_lok, sizeof(int) * nd, hipMemcpyDeviceToHost, st));
        HIP_OK(hipMemcpyAsync(hik.data(), o_hik, sizeof(int) * nd, hipMemcpyDeviceToHost, st));
        HIP_OK(hipStreamSynchronize(st));
    }
    for (int i = 0; i < nc; ++i) {
        if (out->cost_lo) out->cost_lo[i] = lo[(size_t)i];
        if (out->cost_hi) out->cost_hi[i] = hi[(size_t)i];
        if (out->cost_lo_var) out->cost_lo_var[i] = lok[(size_t)i] < 0 ? -1 : nonbasis[(size_t)lok[(size_t)i]];
        if (out->cost_hi_var) out->cost_hi_var[i] = hik[(size_t)i] < 0 ? -1 : nonbasis[(size_t)hik[(size_t)i]];
    }
    for (int i = 0; i < nr; ++i) {
        const size_t j = (size_t)nc + (size_t)i;
        if (out->rhs_lo) out->rhs_lo[i] = lo[j];
        if (out->rhs_hi) out->rhs_hi[i] = hi[j];
        if (out->rhs_lo_var) out->rhs_lo_var[i] = lok[j] < 0 ? -1 : basis[(size_t)lok[j]];
        if (out->rhs_hi_var) out->rhs_hi_var[i] = hik[j] < 0 ? -1 : basis[(size_t)hik[j]];
    }
    return 0;
}

// ---- unboundedness and infeasibility rays (k_rays.hip) ------------------------
void dzg_ray_none(dzg_ray *ry)
{
    ry->kind = 0;
    ry->proven = 0;
    ry->var = ry->pos = -1;
    ry->mu = ry->value = ry->violation = 0.0;
}

// find_first_pivot (src/simplex.rs:423-437) on the host
static int first_pivot_host(const std::vector<double> &y, const std::vector<double> &ybar, int len)
{
    int best = -1;
    double best_ratio = 0.0;
    for (int k = 0; k < len; ++k) {
        if (!(ybar[(size_t)k] > 0.0)) continue;
        const double ratio = -y[(size_t)k] / ybar[(size_t)k];
        if (best < 0 || ratio > best_ratio) {
            best = k;
            best_ratio = ratio;
        }
    }
    return best;
}

extern "C" int dzg_solver_ray(dzg_solver *s, dzg_ray *out)
{
    if (!s || !out) return fail(DZG_E_ARG, "ray: NULL argument");
    HIP_OK(hipSetDevice(s->opts.device));
    TRY(read_ctl(s));
    const int status = s->h_ctl->status;
    if (status != DZG_UNBOUNDED && status != DZG_INFEASIBLE)
        return fail(DZG_E_ARG, "ray: the solver's status is neither DZG_UNBOUNDED nor DZG_INFEASIBLE");
    const DzgDev &d = s->d;
    TRY(dense_one_gpu_only(s, "ray", "rays are not supported on CSC storage or sharded solvers"));
    TRY(fast_needs_workspace(s, "ray"));
    const bool fast = s->numerics == DZG_NUMERICS_FAST;
    const int m = d.m, q = d.q, n = d.n;
    const bool primal = status == DZG_UNBOUNDED;
    hipStream_t st = s->st;
    BasisLists lists;
    TRY(fetch_lists(s, lists));
    const std::vector<int> &basis = lists.basis, &nonbasis = lists.nonbasis;
    const int len = primal ? q : m;
    std::vector<double> side((size_t)(len ? len : 1)), sidebar((size_t)(len ? len : 1));
    if (len) {
        HIP_OK(hipMemcpy(side.data(), primal ? d.z : d.x, sizeof(double) * len, hipMemcpyDeviceToHost));
        HIP_OK(hipMemcpy(sidebar.data(), primal ? d.zbar : d.xbar, sizeof(double) * len, hipMemcpyDeviceToHost));
    }
    const int pos = first_pivot_host(side, sidebar, len);
    if (pos < 0 || m == 0) return fail(DZG_E_DEVICE, "ray: the final state has no first pivot");
    const int var = primal ? nonbasis[(size_t)pos] : basis[(size_t)pos];

    TRY(duals_workspace(s));
    if (!s->ry_part) {
        TRY(dev_alloc(s, &s->ry_vec, (size_t)std::max(m, q) + 2));
        TRY(dev_alloc(s, &s->ry_d, (size_t)n));
        TRY(dev_alloc(s, &s->ry_h, (size_t)m + 2)); TRY(dev_alloc(s, &s->ry_res, (size_t)m + 2));
        TRY(dev_alloc(s, &s->ry_part, (size_t)DZG_RAY_BLOCKS * DZG_RAY_PART)); // set last: "reserved"
    }
    if (fast) {
        // on the fresh inverse: dx is a_j through its columns, y its row `pos` in row space, each
        // refined once against a double-double residual (the explicit inverse alone loses |M| |a| eps
        // where the entering column nearly cancels a basic one); dz one column-wise pricing pass with
        // y as v
        TRY(fresh_inverse(s, "ray", "final"));
        const int k = (int)s->h_ctl->ncompact;
        if (primal) {
            dzg_launch_ray_rhs(m, d.A, d.lda, s->var_col_host[(size_t)var], s->ry_h, st);
            dzg_launch_ray_dx_fast(d, k, s->ry_h, 0, s->ry_vec, st);
            dzg_launch_ray_resid_dx(d, s->ry_h, s->ry_vec, s->ry_res, st);
            dzg_launch_ray_dx_fast(d, k, s->ry_res, 1, s->ry_vec, st);
        } else {
            dzg_launch_ray_rhs(m, nullptr, 0, pos, s->ry_h, st);
            dzg_launch_ray_vt_fast(d, k, s->ry_h, 0, s->du_y, st);
            dzg_launch_ray_resid_v(d, pos, s->du_y, s->ry_res, st);
            dzg_launch_ray_vt_fast(d, k, s->ry_res, 1, s->du_y, st);
            dzg_launch_price_raw(DZG_PRICE_TREE, m, d.lda, d.A, d.nbcode, q, s->du_y, s->ry_vec, st);
        }
    } else {
        // the LU of every STRICT FTRAN / BTRAN, then (Farkas) neg_t_dot in the reference's order: only
        // that pass reads the column codes
        const DzgDev dd = strict_view(s, s->ry_vec);
        if (primal) {
            dzg_launch_ray_rhs(m, d.A, d.lda, s->var_col_host[(size_t)var], s->ry_vec, st);
            dzg_launch_strict_solve(dd, 0, st);
        } else {
            TRY(upload_codes(s, lists));
            HIP_OK(hipStreamSynchronize(st));
            dzg_launch_ray_rhs(m, nullptr, 0, pos, s->du_y, st);
            dzg_launch_strict_solve(dd, 1, st);
            dzg_launch_price_raw(DZG_PRICE_SEQ, m, d.lda, d.A, s->du_codes, q, s->du_y, s->ry_vec, st);
        }
    }
    dzg_launch_ray_finish(primal ? DZG_RAY_PRIMAL : DZG_RAY_FARKAS, m, q, pos, d.basis, d.nonbasis, s->ry_vec,
                          s->du_c, s->du_rhs0, s->du_y, s->ry_d, s->ry_part, st);
    std::vector<double> part((size_t)DZG_RAY_BLOCKS * DZG_RAY_PART), vec((size_t)(m ? m : 1), 0.0),
        dv((size_t)(n ? n : 1), 0.0);
    HIP_OK(hipMemcpyAsync(part.data(), s->ry_part, sizeof(double) * part.size(), hipMemcpyDeviceToHost, st));
    // (the vector the reference's value is summed over: dx, or y)
    HIP_OK(hipMemcpyAsync(vec.data(), primal ? s->ry_vec : s->du_y, sizeof(double) * m, hipMemcpyDeviceToHost, st));
    if (n) HIP_OK(hipMemcpyAsync(dv.data(), s->ry_d, sizeof(double) * n, hipMemcpyDeviceToHost, st));
    HIP_OK(hipStreamSynchronize(st));
    HIP_OK(hipGetLastError());
    double viol = 0.0, bad = 0.0, sum = 0.0;
    for (int b = 0; b < DZG_RAY_BLOCKS; ++b) { // workgroup order
        const double *r = &part[(size_t)b * DZG_RAY_PART];
        viol = std::max(viol, r[0]);
        bad = std::max(bad, r[1]);
        sum = sum + r[2];
    }
    double value;
    if (fast) {
        value = primal ? s->c_host[(size_t)var] - sum : sum;
    } else if (primal) { // the reference's order: c_j less the products c_B[p] dx[p], one by one
        value = dot_reference_order(s->c_host, basis.data(), vec, m, s->c_host[(size_t)var], true);
    } else {
        value = dot_reference_order(s->x0_host, nullptr, vec, m);
    }
    out->kind = primal ? DZG_RAY_PRIMAL : DZG_RAY_FARKAS;
    out->var = var;
    out->pos = pos;
    out->mu = -side[(size_t)pos] / sidebar[(size_t)pos];
    out->value = value;
    out->violation = bad != 0.0 ? std::numeric_limits<double>::quiet_NaN() : viol;
    out->proven = out->violation == 0.0 && (primal ? value > 0.0 : value < 0.0) ? 1 : 0;
    if (out->d && n) std::memcpy(out->d, dv.data(), sizeof(double) * n);
    if (out->y && m) {
        if (primal) std::memset(out->y, 0, sizeof(double) * m);
        else std::memcpy(out->y, vec.data(), sizeof(double) * m);
    }
    return 0;
}

// ---- re-optimisation from the current basis after b or c change (k_restart.hip) ----
static int restart_state(dzg_solver *s, const double *rhs, const double *c, const double *constant,
                         bool refine = false);

extern "C" int dzg_solver_reoptimize(dzg_solver *s, const dzg_reopt *chg)
{
    if (!s || !chg) return fail(DZG_E_ARG, "reoptimize: NULL argument");
    if (!chg->rhs && !chg->c && !chg->set_constant)
        return fail(DZG_E_ARG, "reoptimize: nothing to change (rhs and c are NULL, set_constant is 0)");
    const int m = s->d.m, n = s->d.n;
    TRY(finite_block("reoptimize: ", "rhs", chg->rhs, m, 1, m));
    TRY(finite_block("reoptimize: ", "c", chg->c, n, 1, n));
    if (chg->set_constant && !std::isfinite(chg->constant))
        return fail(DZG_E_ARG, "reoptimize: constant is not finite");
    TRY(dense_one_gpu_only(s, "reoptimize"));
    TRY(fast_needs_workspace(s, "reoptimize"));
    HIP_OK(hipSetDevice(s->opts.device));
    TRY(read_ctl(s));
    TRY(carry_on_status_ok("reoptimize", s->h_ctl->status));
    const double *constant = chg->set_constant ? &chg->constant : nullptr;
    if (s->numerics != DZG_NUMERICS_FAST) return restart_state(s, chg->rhs, chg->c, constant);
    // a fresh inverse first: if it cannot be had, nothing has changed.  The drift measurement is about a
    // solve from the slack basis with the old data: off from here on, put back where the call fails with
    // the data as they were: no inverse, or restart_state out of memory (it reserves before it writes;
    // that now comes after the refactorisation: the same basis, only its eta file is empty)
    double *const drift_ref = s->dr_b0;
    s->dr_b0 = nullptr;
    const int rrc = fresh_inverse(s, "reoptimize", "current");
    const int rc = rrc != 0 ? rrc : restart_state(s, chg->rhs, chg->c, constant);
    if (rrc != 0 || rc == DZG_E_NOMEM) s->dr_b0 = drift_ref;
    return rc;
}

// The state of the current basis for new data (NULL: what the handle holds), written; FAST: the inverse
// is fresh (the caller has just refactorised), s->h_ctl is current.  The body dzg_solver_reoptimize and
// dzg_solver_extend share.  refine (FAST): x and y take one step of iterative refinement against a
// double-double residual, the step dzg_solver_ray takes (k_rays.hip): what the explicit inverse loses
// to cancellation comes back.  dzg_solver_reoptimize keeps the bits it has always given.
static int restart_state(dzg_solver *s, const double *rhs, const double *c, const double *constant, bool refine)
{
    DzgDev &d = s->d;
    const int m = d.m, q = d.q, n = d.n;
    const bool fast = s->numerics == DZG_NUMERICS_FAST;
    DzgCtl *h = s->h_ctl;
    hipStream_t st = s->st;
    TRY(duals_workspace(s));
    if (fast && !s->ro_ag) TRY(dev_alloc(s, &s->ro_ag, (size_t)m + 2));
    if (fast && refine && !s->ro_res) TRY(dev_alloc(s, &s->ro_res, (size_t)m));
    // the new data, on the host and in the device copies every post-solve call reads
    if (c) s->c_host.assign(c, c + n);
    if (rhs) s->x0_host.assign(rhs, rhs + m);
    if (constant) s->constant = *constant;
    if (n) HIP_OK(hipMemcpyAsync(s->du_c, s->c_host.data(), sizeof(double) * n, hipMemcpyHostToDevice, st));
    if (m) HIP_OK(hipMemcpyAsync(s->du_rhs0, s->x0_host.data(), sizeof(double) * m, hipMemcpyHostToDevice, st));
    if (fast) {
        const int k = (int)h->ncompact;
        dzg_launch_restart_x(d, s->du_rhs0, s->ro_ag, k, st);
        // y by the two-stage scheme of the drift measurement, dzy = -N^T y by one column-wise pricing pass
        dzg_launch_drift_y(d, s->du_c, s->du_part, s->du_y, k, st);
        if (refine && m) {
            dzg_launch_ray_resid_dx(d, s->du_rhs0, d.x, s->ro_res, st);      // rhs - B x, by row
            dzg_launch_ray_dx_fast(d, k, s->ro_res, 1, d.x, st);
            dzg_launch_ray_resid_v(d, -1, s->du_y, s->ro_res, st, s->du_c);  // c_B - B^T y, by position
            dzg_launch_ray_vt_fast(d, k, s->ro_res, 1, s->du_y, st);
        }
        if (q) dzg_launch_price_raw(DZG_PRICE_TREE, m, d.lda, d.A, d.nbcode, q, s->du_y, s->du_dzy, st);
    } else {
        // the LU of every STRICT FTRAN / BTRAN: B x = rhs in place in x, B^T y = c_B as
        // dzg_solver_duals solves it, then neg_t_dot in the reference's order
        BasisLists lists;
        TRY(fetch_lists(s, lists));
        std::vector<double> cb((size_t)(m ? m : 1)), ones((size_t)(m ? m : 1), 1.0);
        for (int p = 0; p < m; ++p) cb[(size_t)p] = s->c_host[(size_t)lists.basis[(size_t)p]];
        if (m) {
            HIP_OK(hipMemcpyAsync(d.x, s->x0_host.data(), sizeof(double) * m, hipMemcpyHostToDevice, st));
            HIP_OK(hipMemcpyAsync(d.xbar, ones.data(), sizeof(double) * m, hipMemcpyHostToDevice, st));
            HIP_OK(hipMemcpyAsync(s->du_y, cb.data(), sizeof(double) * m, hipMemcpyHostToDevice, st));
        }
        TRY(upload_codes(s, lists));
        HIP_OK(hipStreamSynchronize(st)); // (cb and ones are locals)
        const DzgDev dd = strict_view(s, d.x);
        if (m) {
            dzg_launch_strict_solve(dd, 0, st);
            dzg_launch_strict_solve(dd, 1, st);
        }
        if (q) dzg_launch_price_raw(DZG_PRICE_SEQ, m, d.lda, d.A, s->du_codes, q, s->du_y, s->du_dzy, st);
    }
    dzg_launch_restart_z(d, s->du_c, s->du_dzy, st);
    // the control block: no pivot is in flight, the run goes on; everything that counts stays
    h->status = DZG_RUNNING;
    h->enter_pos = h->leave_pos = -1;
    h->tie_skip_iter = -1;
    h->drift_tau = 0.0;
    h->tau = h->tie_tol;
    HIP_OK(hipMemcpyAsync(d.ctl, h, sizeof(DzgCtl), hipMemcpyHostToDevice, st));
    d.k_hint = d.k_lo_hint = 0;
    s->state_drift = 0.0;
    if (fast) dzg_launch_fast_update(d, 1, st); // first-pivot partials of the new state
    HIP_OK(hipStreamSynchronize(st));
    HIP_OK(hipGetLastError());
    return 0;
}

// ---- rows and columns added to a live LP, re-optimised from its basis (k_extend.hip) ----
// The successor's matrix (zeroed, lda' x n_struct'): the resident block re-laid, the new rows transposed
// in from a staging block, the new columns by the path of dzg_solver_upload_columns.
static int remove_fill_matrix(dzg_solver *s, const SuccessorSrc &src);
static int successor_fill_matrix(dzg_solver *s, const SuccessorSrc &src)
{
    if (!src.ext) return remove_fill_matrix(s, src);
    const dzg_solver *old = src.old;
    const dzg_extend *e = src.ext;
    const DzgDev &d = s->d;
    const int m0 = old->d.m, ns0 = old->d.ns, p = (int)e->n_rows, r = (int)e->n_cols;
    hipStream_t st = s->st;
    dzg_launch_extend_restride(old->A_alloc, old->d.lda, s->A_alloc, d.lda, m0, ns0, st);
    if (p > 0 && ns0 > 0) {
        void *stage = nullptr;
        const size_t bytes = sizeof(double) * (size_t)p * (size_t)ns0;
        if (hipMalloc(&stage, bytes) != hipSuccess) {
            (void)hipGetLastError();
            return fail(DZG_E_NOMEM, "hipMalloc of " + std::to_string(bytes) + " bytes failed");
        }
        struct Free { void *p; ~Free() { hipFree(p); } } free_stage{stage};
        HIP_OK(hipMemcpy2DAsync(stage, sizeof(double) * (size_t)ns0, e->rows, sizeof(double) * (size_t)e->ld_rows,
                                sizeof(double) * (size_t)ns0, (size_t)p, hipMemcpyHostToDevice, st));
        dzg_launch_extend_rows(static_cast<const double *>(stage), ns0, p, ns0, s->A_alloc, d.lda, m0, st);
        HIP_OK(hipStreamSynchronize(st)); // (the staging block goes away)
    }
    if (r > 0) {
        TRY(upload_columns(s, ns0, (int64_t)ns0 + r, e->cols, e->ld_cols));
        s->cols_present -= r; // (counted at creation already)
    }
    return 0;
}

static int successor_begin(dzg_solver *s, const char *what, DzgCtl *h0, BasisLists &lists0);
static int successor_swap(dzg_solver *s, const dzg_lp &lp, const SuccessorSrc &src, const DzgCtl &h0,
                          const char *what);

extern "C" int dzg_solver_extend(dzg_solver *s, const dzg_extend *ext)
{
    if (!s || !ext) return fail(DZG_E_ARG, "extend: NULL argument");
    const int64_t p = ext->n_rows, r = ext->n_cols;
    if (p < 0 || r < 0) return fail(DZG_E_ARG, "extend: n_rows and n_cols must not be negative");
    if (p == 0 && r == 0) return fail(DZG_E_ARG, "extend: nothing to add (n_rows and n_cols are 0)");
    const int64_t m = s->d.m, n = s->d.n, ns = s->d.ns, q = s->d.q;
    const int64_t m2 = m + p, n2 = n + p + r, ns2 = ns + r, q2 = q + r;
    TRY(dense_one_gpu_only(s, "extend"));
    if (n2 >= (1ll << 31) - 64) return fail(DZG_E_ARG, "extend: index range");
    if (p > 0 && (!ext->rhs || (ns > 0 && !ext->rows)))
        return fail(DZG_E_ARG, "extend: n_rows > 0 needs rows and rhs");
    if (p > 0 && ns > 0 && ext->ld_rows < ns) return fail(DZG_E_ARG, "extend: ld_rows < n_struct");
    if (r > 0 && (!ext->c_cols || (m2 > 0 && !ext->cols)))
        return fail(DZG_E_ARG, "extend: n_cols > 0 needs cols and c_cols");
    if (r > 0 && ext->ld_cols < m2) return fail(DZG_E_ARG, "extend: ld_cols < m + n_rows");
    if (p > 0) TRY(finite_block("extend: ", "rows", ext->rows, ns, p, ext->ld_rows));
    if (p > 0) TRY(finite_block("extend: ", "rhs", ext->rhs, p, 1, p));
    if (r > 0) TRY(finite_block("extend: ", "cols", ext->cols, m2, r, ext->ld_cols));
    if (r > 0) TRY(finite_block("extend: ", "c_cols", ext->c_cols, r, 1, r));
    DzgCtl h0;
    BasisLists lists0;
    TRY(successor_begin(s, "extend", &h0, lists0));
    const std::vector<int> &basis0 = lists0.basis, &nonbasis0 = lists0.nonbasis;

    // the extended LP on the host: everything but the matrix
    std::vector<int64_t> basis((size_t)(m2 ? m2 : 1)), nonbasis((size_t)(q2 ? q2 : 1)), var_col((size_t)(n2 ? n2 : 1));
    std::vector<double> c2((size_t)(n2 ? n2 : 1), 0.0), rhs2((size_t)(m2 ? m2 : 1), 0.0), z2((size_t)(q2 ? q2 : 1), 0.0);
    for (int64_t i = 0; i < m; ++i) basis[(size_t)i] = basis0[(size_t)i];
    for (int64_t i = 0; i < p; ++i) basis[(size_t)(m + i)] = n + r + i;
    for (int64_t k = 0; k < q; ++k) nonbasis[(size_t)k] = nonbasis0[(size_t)k];
    for (int64_t j = 0; j < r; ++j) nonbasis[(size_t)(q + j)] = n + j;
    for (int64_t v = 0; v < n; ++v) {
        var_col[(size_t)v] = s->var_col_host[(size_t)v];
        c2[(size_t)v] = s->c_host[(size_t)v];
    }
    for (int64_t j = 0; j < r; ++j) {
        var_col[(size_t)(n + j)] = ns + j;
        c2[(size_t)(n + j)] = ext->c_cols[j];
    }
    for (int64_t i = 0; i < p; ++i) var_col[(size_t)(n + r + i)] = -1 - (m + i);
    for (int64_t i = 0; i < m; ++i) rhs2[(size_t)i] = s->x0_host[(size_t)i];
    for (int64_t i = 0; i < p; ++i) rhs2[(size_t)(m + i)] = ext->rhs[i];
    dzg_lp lp;
    std::memset(&lp, 0, sizeof(lp));
    lp.m = m2; lp.n = n2; lp.n_struct = ns2;
    lp.var_col = var_col.data();
    lp.c = c2.data();
    lp.constant = s->constant;
    lp.basis = basis.data(); lp.nonbasis = nonbasis.data();
    lp.x = rhs2.data(); lp.z = z2.data(); // (the right-hand side by row; the state is written below)
    const SuccessorSrc src{s, ext, nullptr, nullptr};
    return successor_swap(s, lp, src, h0, "extend");
}

// What dzg_solver_extend and dzg_solver_remove share.  successor_begin: the refusals that depend on the
// handle's state, then its control block and its two lists on the host.  successor_swap: the LP `lp`
// (everything but the matrix, which `src` names) built as a successor next to the live state, left in
// restart_state's state with the counters and the log carried over, and swapped into the caller's
// handle; any failure leaves `s` as it was.
static int successor_begin(dzg_solver *s, const char *what, DzgCtl *h0, BasisLists &lists0)
{
    TRY(fast_needs_workspace(s, what));
    HIP_OK(hipSetDevice(s->opts.device));
    TRY(read_ctl(s));
    *h0 = *s->h_ctl;
    TRY(carry_on_status_ok(what, h0->status));
    return fetch_lists(s, lists0);
}

static int successor_swap(dzg_solver *s, const dzg_lp &lp, const SuccessorSrc &src, const DzgCtl &h0,
                          const char *what)
{
    const bool fast = s->numerics == DZG_NUMERICS_FAST;
    hipStream_t st = s->st;
    // the successor, on the same stream with the same options and the numerics the handle runs in
    dzg_opts o = s->opts;
    o.stream = (void *)st;
    o.numerics = s->numerics;
    dzg_solver *t = nullptr;
    const auto t0 = std::chrono::steady_clock::now();
    TRY(solver_create(&lp, &o, &t, &src));
    struct Guard { dzg_solver *t; ~Guard() { if (t) dzg_solver_destroy(t); } } guard{t};
    if (fast && t->refactors == 0) {
        // the slack basis, which creation does not factorise: the restart kernels read the lists a
        // refactorisation leaves, as they do in dzg_solver_reoptimize before a first run
        const auto tr = std::chrono::steady_clock::now();
        TRY(refactor_now(t, true));
        HIP_OK(hipStreamSynchronize(st));
        t->extend_ms[1] = ms_since(tr);
    }
    TRY(read_ctl(t));
    if (t->h_ctl->status != DZG_RUNNING) return singular_block(what, "new"); // (t goes: nothing to put back)
    t->extend_ms[0] = ms_since(t0) - t->extend_ms[1];
    // what carries on: the pivot count and everything counted per pivot, the log
    DzgCtl *h = t->h_ctl;
    h->iter = h0.iter;
    h->price_bytes = h0.price_bytes;
    h->price_mask = h0.price_mask;
    h->min_margin = h0.min_margin;
    h->near_ties = h0.near_ties;
    h->first_near_tie = h0.first_near_tie;
    const auto t1 = std::chrono::steady_clock::now();
    TRY(restart_state(t, nullptr, nullptr, nullptr, true));
    t->extend_ms[2] = ms_since(t1);
    const long long cnt = h0.iter < s->d.log_cap ? h0.iter : s->d.log_cap;
    if (cnt > 0 && cnt <= t->d.log_cap) {
        HIP_OK(hipMemcpyAsync(t->d.log_kind, s->d.log_kind, sizeof(int) * cnt, hipMemcpyDeviceToDevice, st));
        HIP_OK(hipMemcpyAsync(t->d.log_enter, s->d.log_enter, sizeof(int) * cnt, hipMemcpyDeviceToDevice, st));
        HIP_OK(hipMemcpyAsync(t->d.log_leave, s->d.log_leave, sizeof(int) * cnt, hipMemcpyDeviceToDevice, st));
        HIP_OK(hipMemcpyAsync(t->d.log_mu, s->d.log_mu, sizeof(double) * cnt, hipMemcpyDeviceToDevice, st));
        HIP_OK(hipMemcpyAsync(t->d.log_margin, s->d.log_margin, sizeof(double) * cnt, hipMemcpyDeviceToDevice, st));
    }
    HIP_OK(hipStreamSynchronize(st));
    HIP_OK(hipGetLastError());
    t->solve_ms = s->solve_ms;
    t->refactors += s->refactors;
    t->max_err_life = s->max_err_life;
    t->chain_fallbacks = s->chain_fallbacks;
    for (int c = 0; c < DZG_K_COUNT; ++c) {
        t->kernel_ms[c] = s->kernel_ms[c];
        t->kernel_launches[c] = s->kernel_launches[c];
    }
    // the successor takes the handle's place (the caller's pointer stays valid); the old state goes
    std::swap(*s, *t);
    s->opts = t->opts;
    s->own_stream = t->own_stream;
    t->own_stream = false;
    guard.t = nullptr;
    dzg_solver_destroy(t);
    return 0;
}

// ---- rows and columns removed from a live LP, carried on from its basis (k_remove.hip) ----
// The successor's matrix (zeroed, lda' x n_struct'): the kept rows and columns of the resident one,
// gathered on the device; the two lists are all that is uploaded.
static int remove_fill_matrix(dzg_solver *s, const SuccessorSrc &src)
{
    const dzg_solver *old = src.old;
    const DzgDev &d = s->d;
    const std::vector<int> *kr = src.keep_rows;
    const std::vector<int> &kc = *src.keep_cols;
    const size_t nr = kr ? kr->size() : 0, nc = kc.size();
    if (d.m <= 0 || nc == 0) return 0;
    hipStream_t st = s->st;
    void *lists = nullptr;
    const size_t bytes = sizeof(int) * (nr + nc);
    if (hipMalloc(&lists, bytes) != hipSuccess) {
        (void)hipGetLastError();
        return fail(DZG_E_NOMEM, "hipMalloc of " + std::to_string(bytes) + " bytes failed");
    }
    struct Free { void *p; ~Free() { hipFree(p); } } free_lists{lists};
    int *d_cols = static_cast<int *>(lists), *d_rows = d_cols + nc;
    HIP_OK(hipMemcpyAsync(d_cols, kc.data(), sizeof(int) * nc, hipMemcpyHostToDevice, st));
    if (nr) HIP_OK(hipMemcpyAsync(d_rows, kr->data(), sizeof(int) * nr, hipMemcpyHostToDevice, st));
    dzg_launch_remove_gather(old->A_alloc, old->d.lda, s->A_alloc, d.lda, old->d.m, kr ? d_rows : nullptr, d.m,
                             d_cols, (int)nc, st);
    HIP_OK(hipStreamSynchronize(st)); // (the lists go away)
    return 0;
}

// `idx[0..count)` marked in `drop` (sized for the range); DZG_E_ARG for one outside it or listed twice
static int remove_mark(const char *name, const int64_t *idx, int64_t count, std::vector<char> &drop)
{
    for (int64_t k = 0; k < count; ++k) {
        const int64_t i = idx[k];
        if (i < 0 || i >= (int64_t)drop.size())
            return fail(DZG_E_ARG, std::string("remove: ") + name + "[" + std::to_string(k) + "] = " +
                                       std::to_string(i) + " is out of range");
        if (drop[(size_t)i])
            return fail(DZG_E_ARG, std::string("remove: ") + name + "[" + std::to_string(k) + "] = " +
                                       std::to_string(i) + " is listed twice");
        drop[(size_t)i] = 1;
    }
    return 0;
}

extern "C" int dzg_solver_remove(dzg_solver *s, const dzg_remove *rem, int64_t *var_map, int64_t *row_map)
{
    if (!s || !rem) return fail(DZG_E_ARG, "remove: NULL argument");
    const int64_t p = rem->n_rows, r = rem->n_cols;
    if (p < 0 || r < 0) return fail(DZG_E_ARG, "remove: n_rows and n_cols must not be negative");
    if (p == 0 && r == 0) return fail(DZG_E_ARG, "remove: nothing to remove (n_rows and n_cols are 0)");
    if ((p > 0 && !rem->rows) || (r > 0 && !rem->cols))
        return fail(DZG_E_ARG, "remove: a count > 0 needs its list (NULL argument)");
    TRY(dense_one_gpu_only(s, "remove"));
    const int64_t m = s->d.m, n = s->d.n, ns = s->d.ns, q = s->d.q;
    std::vector<char> drop_row((size_t)m, 0), drop_col((size_t)ns, 0);
    TRY(remove_mark("rows", rem->rows, p, drop_row));
    TRY(remove_mark("cols", rem->cols, r, drop_col));
    const int64_t m2 = m - p, n2 = n - p - r, ns2 = ns - r, q2 = q - r;
    if (m2 < 1 || ns2 < 1)
        return fail(DZG_E_ARG, "remove: at least one row and one structural column must stay");
    DzgCtl h0;
    BasisLists lists0;
    TRY(successor_begin(s, "remove", &h0, lists0));
    const std::vector<int> &basis0 = lists0.basis, &nonbasis0 = lists0.nonbasis;

    // what may go: a row whose slack is basic, a structural column whose variable is nonbasic
    const std::vector<int> &code0 = s->var_col_host;
    for (int64_t k = 0; k < q; ++k) {
        const int v = nonbasis0[(size_t)k], code = code0[(size_t)v];
        if (code < 0 && drop_row[(size_t)(-1 - code)])
            return fail(DZG_E_ARG, "remove: row " + std::to_string(-1 - code) + " is binding (its slack, variable " +
                                       std::to_string(v) + ", is nonbasic): dropping it needs a pivot first");
    }
    for (int64_t i = 0; i < m; ++i) {
        const int v = basis0[(size_t)i], code = code0[(size_t)v];
        if (code >= 0 && drop_col[(size_t)code])
            return fail(DZG_E_ARG, "remove: column " + std::to_string(code) + " is basic (variable " +
                                       std::to_string(v) + " at basis position " + std::to_string(i) +
                                       "): dropping it needs a pivot first");
    }

    // the reduced LP on the host, everything but the matrix: survivors compressed in ascending order
    std::vector<int> keep_rows, keep_cols;
    std::vector<int64_t> new_row((size_t)m, -1), new_col((size_t)ns, -1), new_var((size_t)n, -1);
    for (int64_t i = 0; i < m; ++i)
        if (!drop_row[(size_t)i]) {
            new_row[(size_t)i] = (int64_t)keep_rows.size();
            keep_rows.push_back((int)i);
        }
    for (int64_t j = 0; j < ns; ++j)
        if (!drop_col[(size_t)j]) {
            new_col[(size_t)j] = (int64_t)keep_cols.size();
            keep_cols.push_back((int)j);
        }
    std::vector<int64_t> basis, nonbasis, var_col;
    std::vector<double> c2, rhs2((size_t)m2, 0.0), z2((size_t)(q2 ? q2 : 1), 0.0);
    for (int64_t v = 0; v < n; ++v) {
        const int code = code0[(size_t)v];
        const int64_t to = code >= 0 ? new_col[(size_t)code] : new_row[(size_t)(-1 - code)];
        if (to < 0) continue;
        new_var[(size_t)v] = (int64_t)var_col.size();
        var_col.push_back(code >= 0 ? to : -1 - to);
        c2.push_back(s->c_host[(size_t)v]);
    }
    for (int64_t i = 0; i < m; ++i)
        if (new_var[(size_t)basis0[(size_t)i]] >= 0) basis.push_back(new_var[(size_t)basis0[(size_t)i]]);
    for (int64_t k = 0; k < q; ++k)
        if (new_var[(size_t)nonbasis0[(size_t)k]] >= 0) nonbasis.push_back(new_var[(size_t)nonbasis0[(size_t)k]]);
    if ((int64_t)var_col.size() != n2 || (int64_t)basis.size() != m2 || (int64_t)nonbasis.size() != q2)
        return fail(DZG_E_ARG, "remove: the handle's lists do not partition its variables");
    for (int64_t i = 0; i < m2; ++i) rhs2[(size_t)i] = s->x0_host[(size_t)keep_rows[(size_t)i]];
    if (nonbasis.empty()) nonbasis.push_back(0); // (q' == 0: never read)
    dzg_lp lp;
    std::memset(&lp, 0, sizeof(lp));
    lp.m = m2; lp.n = n2; lp.n_struct = ns2;
    lp.var_col = var_col.data();
    lp.c = c2.data();
    lp.constant = s->constant;
    lp.basis = basis.data(); lp.nonbasis = nonbasis.data();
    lp.x = rhs2.data(); lp.z = z2.data(); // (the right-hand side by row; the state is written by the swap)
    const SuccessorSrc src{s, nullptr, p > 0 ? &keep_rows : nullptr, &keep_cols};
    TRY(successor_swap(s, lp, src, h0, "remove"));
    if (var_map) std::copy(new_var.begin(), new_var.end(), var_map);
    if (row_map) std::copy(new_row.begin(), new_row.end(), row_map);
    return 0;
}

extern "C" int dzg_solver_dims(const dzg_solver *s, int64_t *m, int64_t *n, int64_t *n_struct)
{
    if (!s) return fail(DZG_E_ARG, "dims: solver is NULL");
    if (m) *m = s->d.m;
    if (n) *n = s->d.n;
    if (n_struct) *n_struct = s->d.ns;
    return 0;
}

extern "C" int dzg_debug_extend_ms(const dzg_solver *s, double ms[3])
{
    if (!s || !ms) return fail(DZG_E_ARG, "extend_ms: NULL argument");
    for (int i = 0; i < 3; ++i) ms[i] = s->extend_ms[i];
    return 0;
}

extern "C" int dzg_debug_matrix(dzg_solver *s, int64_t col0, int64_t col1, double *out, int64_t ld_out)
{
    if (!s || (col1 > col0 && !out)) return fail(DZG_E_ARG, "matrix: NULL argument");
    const DzgDev &d = s->d;
    if (d.csc || d.world > 1) return fail(DZG_E_ARG, "matrix: a dense matrix on one GPU");
    if (col0 < 0 || col1 > d.ns || col0 > col1 || ld_out < d.m)
        return fail(DZG_E_ARG, "matrix: columns outside [0, n_struct) or ld_out < m");
    if (col1 == col0 || d.m == 0) return 0;
    HIP_OK(hipSetDevice(s->opts.device));
    HIP_OK(hipStreamSynchronize(s->st));
    HIP_OK(hipMemcpy2D(out, sizeof(double) * (size_t)ld_out, s->A_alloc + (size_t)col0 * (size_t)d.lda,
                       sizeof(double) * (size_t)d.lda, sizeof(double) * (size_t)d.m, (size_t)(col1 - col0),
                       hipMemcpyDeviceToHost));
    return 0;
}

extern "C" int64_t dzg_debug_matrix_rows(dzg_solver *s, int64_t row0, int64_t row1, double *out, int64_t ld_out)
{
    if (!s || (row1 > row0 && !out)) return fail(DZG_E_ARG, "matrix_rows: NULL argument");
    const DzgDev &d = s->d;
    if (d.csc || d.world > 1) return fail(DZG_E_ARG, "matrix_rows: a dense matrix on one GPU");
    if (row0 < 0 || row1 > d.m || row0 > row1 || ld_out < d.ns)
        return fail(DZG_E_ARG, "matrix_rows: rows outside [0, m) or ld_out < n_struct");
    if (!d.At || row1 == row0 || d.ns == 0) return 0;
    HIP_OK(hipSetDevice(s->opts.device));
    HIP_OK(hipStreamSynchronize(s->st));
    HIP_OK(hipMemcpy2D(out, sizeof(double) * (size_t)ld_out, d.At + (size_t)row0 * (size_t)d.ldt,
                       sizeof(double) * (size_t)d.ldt, sizeof(double) * (size_t)d.ns, (size_t)(row1 - row0),
                       hipMemcpyDeviceToHost));
    return row1 - row0;
}

// What a one-call solve wants beyond the result: the duals and, with `req`, the ranges of the solver
// that produced it.  rg_rc: what dzg_solver_ranging returned for an OPTIMAL solve (0 otherwise).
struct SolveExtras {
    dzg_duals *du = nullptr;
    const dzg_ranging_req *req = nullptr;
    dzg_ranging *rg = nullptr;
    int rg_rc = 0;
    dzg_ray *ry = nullptr; // the ray of a solve that ended UNBOUNDED or INFEASIBLE (kind 0 otherwise)
};

// (status, result and, when asked for and the LP ended OPTIMAL, the duals and ranges of this solver)
static int finish_solver(dzg_solver *s, int rc, dzg_result *res, SolveExtras &ex)
{
    const int rc2 = dzg_solver_result(s, res);
    if (rc2 == 0 && ex.rg) {
        dzg_duals tmp;
        std::memset(&tmp, 0, sizeof(tmp));
        dzg_duals *du = ex.du ? ex.du : &tmp;
        ex.rg_rc = 0;
        if (res->status == DZG_OPTIMAL) ex.rg_rc = dzg_solver_ranging(s, ex.req, du, ex.rg);
        if (res->status != DZG_OPTIMAL || ex.rg_rc != 0) {
            dzg_duals_none(du, res->objective);
            dzg_ranging_none(ex.req, ex.rg);
        }
    } else if (rc2 == 0 && ex.du) {
        // the solve's outcome is what dzg_core_solve returns, whatever becomes of the duals: a call
        // that fails (the final basis of a FAST run did not refactorise) leaves source = 0 and its
        // message in dzg_last_error
        if (res->status != DZG_OPTIMAL || dzg_solver_duals(s, ex.du) != 0) dzg_duals_none(ex.du, res->objective);
    }
    if (rc2 == 0 && ex.ry) {
        // as with the duals, the solve's outcome stands whatever becomes of the ray: a route without
        // rays or a final basis that did not refactorise leaves kind = 0 and its message in
        // dzg_last_error
        const bool ended = res->status == DZG_UNBOUNDED || res->status == DZG_INFEASIBLE;
        if (!ended || dzg_solver_ray(s, ex.ry) != 0) dzg_ray_none(ex.ry);
    }
    dzg_solver_destroy(s);
    return rc2 != 0 ? rc2 : rc;
}

static int solve_once(const dzg_lp *lp, const dzg_opts *o, dzg_result *res, SolveExtras &ex)
{
    dzg_solver *s = nullptr;
    int rc = dzg_solver_create(lp, o, &s);
    if (rc != 0) return rc;
    rc = dzg_solver_run(s, 0);
    if (rc < 0) {
        dzg_solver_destroy(s);
        return rc;
    }
    return finish_solver(s, rc, res, ex);
}

// dzg_core_solve; with ex.du / ex.rg also the duals / ranges of whichever solver produced the result
static int core_solve(const dzg_lp *lp, const dzg_opts *opts, dzg_result *res, SolveExtras &ex)
{
    const bool fresh = ex.du || ex.rg || ex.ry; // the final basis will be refactorised
    if (!res) return fail(DZG_E_ARG, "res is NULL");
    if (!lp) return fail(DZG_E_ARG, "lp is NULL");
    dzg_opts o;
    if (opts) o = *opts; else dzg_opts_default(&o);
    // (duals of a FAST run: reserve the refactorisation workspace, as a non-slack start does)
    if (fresh && o.refactor_interval == 0) o.refactor_interval = -1;
    const bool automatic = o.numerics == DZG_NUMERICS_AUTO;
    // AUTO above auto_strict_rows = FAST that must prove it followed the reference: up to
    // DZG_AUTO_STRICT_RESTART_ROWS rows it stops at the first decision that is within rounding of
    // a tie (and when it loses its footing: DZG_SINGULAR, DZG_PANIC -- degenerate or badly scaled
    // data), and the LP is solved again from the first pivot in the reference's own arithmetic;
    // the state vectors of a FAST run carry FAST's rounding, so no later point can be handed over
    // bit-exactly.  Above that size STRICT is out of reach and FAST reports what it met.
    const int restart_rows = o.auto_restart_rows != 0 ? o.auto_restart_rows : DZG_AUTO_STRICT_RESTART_ROWS;
    const bool can_restart = automatic && dzg_opts_numerics(o, lp->m) == DZG_NUMERICS_FAST && lp->m <= restart_rows;
    if (can_restart && o.tie_tol >= 0.0) o.near_tie_action = DZG_NEAR_TIE_STOP;
    int rc = solve_once(lp, &o, res, ex);
    if (rc < 0) return rc;
    if (can_restart && res->numerics_used == DZG_NUMERICS_FAST &&
        (rc == DZG_NEAR_TIE || rc == DZG_SINGULAR || rc == DZG_PANIC)) {
        dzg_opts strict = o;
        strict.numerics = DZG_NUMERICS_STRICT;
        strict.refactor_interval = 0;
        strict.near_tie_action = DZG_NEAR_TIE_COUNT;
        // The re-solve costs 3-57 ms per pivot: it runs against a wall-clock budget (an
        // integer model with many thousands of pivots would otherwise sit here for an hour without
        // a sign of life).  Out of budget: FAST from the first pivot with near ties COUNTED -- the
        // caller sees numerics_used = FAST and near_ties / first_near_tie, i.e. from which pivot on
        // the path is no longer certified to be the reference's.
        const double budget_s = o.auto_strict_budget_s < 0 ? -1.0
                                : (o.auto_strict_budget_s == 0 ? 600.0 : (double)o.auto_strict_budget_s);
        dzg_solver *ss = nullptr;
        rc = dzg_solver_create(lp, &strict, &ss);
        if (rc != 0) return rc;
        const auto t0 = std::chrono::steady_clock::now();
        bool out_of_time = false;
        for (;;) {
            rc = dzg_solver_run(ss, 256);
            // (the solver's own limit: dzg_solver_create normalised max_iter <= 0 in ITS copy only,
            // and a zero-filled dzg_opts from a C host must not read as "limit reached")
            if (rc != DZG_ITER_LIMIT || ss->h_ctl->iter >= ss->opts.max_iter) break;
            const double el = std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count();
            if (budget_s >= 0.0 && el > budget_s) { out_of_time = true; break; }
        }
        if (rc < 0) {
            dzg_solver_destroy(ss);
            return rc;
        }
        if (!out_of_time) return finish_solver(ss, rc, res, ex);
        dzg_solver_destroy(ss);
        dzg_opts fast = o;
        fast.numerics = DZG_NUMERICS_FAST;
        fast.near_tie_action = DZG_NEAR_TIE_COUNT;
        rc = solve_once(lp, &fast, res, ex);
    }
    return rc;
}

// (model.cpp)
int dzg_core_solve_with_duals(const dzg_lp *lp, const dzg_opts *opts, dzg_result *res, dzg_duals *du)
{
    SolveExtras ex;
    ex.du = du;
    return core_solve(lp, opts, res, ex);
}

// (model.cpp) the request was validated by the caller; *rg_rc: dzg_solver_ranging's own return value
int dzg_core_solve_with_ranging(const dzg_lp *lp, const dzg_opts *opts, dzg_result *res, dzg_duals *du,
                                const dzg_ranging_req *req, dzg_ranging *rg, int *rg_rc)
{
    SolveExtras ex;
    ex.du = du;
    ex.req = req;
    ex.rg = rg;
    const int rc = core_solve(lp, opts, res, ex);
    if (rg_rc) *rg_rc = ex.rg_rc;
    return rc;
}

// (model.cpp) du is optional
int dzg_core_solve_with_rays(const dzg_lp *lp, const dzg_opts *opts, dzg_result *res, dzg_duals *du,
                             dzg_ray *ry)
{
    SolveExtras ex;
    ex.du = du;
    ex.ry = ry;
    return core_solve(lp, opts, res, ex);
}

extern "C" int dzg_core_solve(const dzg_lp *lp, const dzg_opts *opts, dzg_result *res)
{
    SolveExtras ex;
    return core_solve(lp, opts, res, ex);
}

// Level 1 on the fields of the reference's `Simplex` AS THEY ARE (src/simplex.rs:84-112): one
// CscMatrix over all n columns, slack columns included (src/linalg.rs:161-168; usize indices),
// b / n / x / z, the objective's coefficients and constant.  Simplex::solve becomes this one call.
// The unit columns that the device never stores are found here: a column with exactly one stored
// entry, equal to 1.0, is the slack of its row (scanned from the last column down, one per row --
// Simplex::new puts the slacks last; any further unit column of a row stays an ordinary column).
// The remaining columns go to the device dense or as CSC, whichever is smaller.
extern "C" int dzg_core_solve_full_csc(int64_t m, int64_t n, const int64_t *col_ptr,
                                       const int64_t *row_idx, const double *val, const double *c,
                                       double constant, int64_t *basis, int64_t *nonbasis, double *x,
                                       double *z, const dzg_opts *opts, dzg_result *res)
{
    if (!res) return fail(DZG_E_ARG, "res is NULL");
    if (m < 0 || n < m || !col_ptr || (n > 0 && !c) || (m > 0 && (!basis || !x)) ||
        (n > m && (!nonbasis || !z)))
        return fail(DZG_E_ARG, "full_csc: sizes / NULL argument");
    if (n >= (1ll << 31) - 64) return fail(DZG_E_ARG, "full_csc: index range");
    if (col_ptr[0] != 0) return fail(DZG_E_ARG, "full_csc: col_ptr[0] != 0");
    for (int64_t j = 0; j < n; ++j) {
        if (col_ptr[j + 1] < col_ptr[j]) return fail(DZG_E_ARG, "full_csc: col_ptr not monotone");
        for (int64_t e = col_ptr[j]; e < col_ptr[j + 1]; ++e)
            if (!row_idx || !val || row_idx[e] < 0 || row_idx[e] >= m ||
                (e > col_ptr[j] && row_idx[e] <= row_idx[e - 1]))
                return fail(DZG_E_ARG, "full_csc: row_idx must ascend strictly inside a column");
    }
    std::vector<int64_t> var_col((size_t)(n ? n : 1), 0);
    std::vector<char> row_has_slack((size_t)(m ? m : 1), 0), is_slack((size_t)(n ? n : 1), 0);
    for (int64_t j = n - 1; j >= 0; --j) {
        const int64_t e = col_ptr[j];
        if (col_ptr[j + 1] - e == 1 && val[e] == 1.0 && !row_has_slack[(size_t)row_idx[e]]) {
            row_has_slack[(size_t)row_idx[e]] = 1;
            is_slack[(size_t)j] = 1;
            var_col[(size_t)j] = -1 - row_idx[e];
        }
    }
    int64_t ns = 0, nnz = 0;
    for (int64_t j = 0; j < n; ++j)
        if (!is_slack[(size_t)j]) {
            var_col[(size_t)j] = ns++;
            for (int64_t e = col_ptr[j]; e < col_ptr[j + 1]; ++e) nnz += val[e] != 0.0;
        }
    dzg_lp lp;
    std::memset(&lp, 0, sizeof(lp));
    lp.m = m; lp.n = n; lp.n_struct = ns;
    lp.var_col = var_col.data();
    lp.c = c; lp.constant = constant;
    lp.basis = basis; lp.nonbasis = nonbasis; lp.x = x; lp.z = z;
    // dense (8 m ns bytes) or CSC (12 bytes per entry + the CSR copy of the sparse-basis path)
    const bool dense = ns > 0 && (double)nnz * 24.0 >= (double)m * (double)ns * 8.0;
    std::vector<double> a, sval;
    std::vector<int64_t> scp;
    std::vector<int32_t> sri;
    if (dense) {
        a.assign((size_t)m * (size_t)ns, 0.0);
        for (int64_t j = 0; j < n; ++j)
            if (!is_slack[(size_t)j])
                for (int64_t e = col_ptr[j]; e < col_ptr[j + 1]; ++e)
                    a[(size_t)var_col[(size_t)j] * (size_t)m + (size_t)row_idx[e]] = val[e];
        lp.a = a.data();
        lp.lda = m;
    } else if (ns > 0) {
        scp.assign((size_t)ns + 1, 0);
        sri.reserve((size_t)nnz);
        sval.reserve((size_t)nnz);
        for (int64_t j = 0; j < n; ++j)
            if (!is_slack[(size_t)j]) {
                for (int64_t e = col_ptr[j]; e < col_ptr[j + 1]; ++e)
                    if (val[e] != 0.0) { // (the reference's CSC holds no explicit zeros, src/linalg.rs:261)
                        sri.push_back((int32_t)row_idx[e]);
                        sval.push_back(val[e]);
                    }
                scp[(size_t)var_col[(size_t)j] + 1] = (int64_t)sri.size();
            }
        if (sri.empty()) { sri.push_back(0); sval.push_back(0.0); }
        lp.col_ptr = scp.data();
        lp.row_idx = sri.data();
        lp.val = sval.data();
    }
    // the final state lands in the caller's b / n / x / z, as Simplex::solve leaves it in `self`
    const int64_t q = n - m;
    std::vector<int64_t> ob, on;
    std::vector<double> ox, oz;
    dzg_result r = *res;
    if (!r.basis) { ob.resize((size_t)(m ? m : 1)); r.basis = ob.data(); }
    if (!r.nonbasis) { on.resize((size_t)(q ? q : 1)); r.nonbasis = on.data(); }
    if (!r.x) { ox.resize((size_t)(m ? m : 1)); r.x = ox.data(); }
    if (!r.z) { oz.resize((size_t)(q ? q : 1)); r.z = oz.data(); }
    const int rc = dzg_core_solve(&lp, opts, &r);
    if (rc < 0) return rc;
    for (int64_t p = 0; p < m; ++p) { basis[p] = r.basis[p]; x[p] = r.x[p]; }
    for (int64_t k = 0; k < q; ++k) { nonbasis[k] = r.nonbasis[k]; z[k] = r.z[k]; }
    if (!res->basis) r.basis = nullptr;
    if (!res->nonbasis) r.nonbasis = nullptr;
    if (!res->x) r.x = nullptr;
    if (!res->z) r.z = nullptr;
    *res = r;
    return rc;
}

// ---- single-function entry points for parity tests -------------------------------
extern "C" int dzg_kernel_lu_solve(int64_t n, const double *a, const double *b, double *x_out,
                                   double *lu_out, int64_t *p_out, int32_t device)
{
    if (n <= 0 || !a || !b || !x_out) return fail(DZG_E_ARG, "bad argument");
    if (dzg_device_count() <= 0) return fail(DZG_E_DEVICE, "no HIP device visible");
    HIP_OK(hipSetDevice(device));
    DzgLu w{};
    dzg_lu_layout((int)n, &w);
    double *xo;
    DzgCtl *ctl;
    HIP_OK(hipMalloc(&w.W, sizeof(double) * (size_t)n * (size_t)w.ldw));
    HIP_OK(hipMalloc(&w.P0, sizeof(double) * (size_t)n * DZG_LU_LDP));
    HIP_OK(hipMalloc(&w.P1, sizeof(double) * (size_t)n * DZG_LU_LDP));
    HIP_OK(hipMalloc(&w.piv, sizeof(int) * n));
    HIP_OK(hipMalloc(&w.pz, sizeof(int) * n));
    HIP_OK(hipMalloc(&w.ptab, sizeof(int) * (size_t)n * DZG_LU_NB));
    HIP_OK(hipMalloc(&w.part_r, sizeof(double) * 2 * (size_t)w.nparts));
    HIP_OK(hipMalloc(&w.part_k, sizeof(int) * 2 * (size_t)w.nparts));
    HIP_OK(hipMalloc(&xo, sizeof(double) * n));
    HIP_OK(hipMalloc(&ctl, sizeof(DzgCtl)));
    DzgCtl c0;
    std::memset(&c0, 0, sizeof(c0));
    c0.status = DZG_RUNNING;
    HIP_OK(hipMemcpy(ctl, &c0, sizeof(c0), hipMemcpyHostToDevice));
    const size_t pitch = sizeof(double) * (size_t)w.ldw, rowb = sizeof(double) * (size_t)n;
    HIP_OK(hipMemcpy2D(w.W, pitch, a, rowb, rowb, (size_t)n, hipMemcpyHostToDevice));
    HIP_OK(hipMemcpy2D(w.W + n, pitch, b, sizeof(double), sizeof(double), (size_t)n,
                       hipMemcpyHostToDevice)); // the right-hand side is column n
    HIP_OK(hipMemset(w.piv, 0, sizeof(int) * n));
    dzg_launch_lu_raw(w, ctl, xo, 0);
    HIP_OK(hipDeviceSynchronize());
    HIP_OK(hipGetLastError());
    HIP_OK(hipMemcpy(x_out, xo, sizeof(double) * n, hipMemcpyDeviceToHost));
    if (lu_out) HIP_OK(hipMemcpy2D(lu_out, rowb, w.W, pitch, rowb, (size_t)n, hipMemcpyDeviceToHost));
    if (p_out && n > 1) {
        std::vector<int> p((size_t)n);
        HIP_OK(hipMemcpy(p.data(), w.piv, sizeof(int) * n, hipMemcpyDeviceToHost));
        for (int64_t k = 0; k + 1 < n; ++k) p_out[k] = p[(size_t)k];
    }
    hipFree(w.W); hipFree(w.P0); hipFree(w.P1); hipFree(w.piv); hipFree(w.pz); hipFree(w.ptab);
    hipFree(w.part_r); hipFree(w.part_k); hipFree(xo); hipFree(ctl);
    return 0;
}

extern "C" int dzg_kernel_neg_t_dot(int64_t m, int64_t n_struct, const double *a, int64_t lda,
                                    const int64_t *cols, int64_t ncols, const double *v,
                                    double *out, int32_t kernel, int32_t device)
{
    if (m <= 0 || n_struct < 0 || ncols < 0 || !v || !out || (ncols > 0 && !cols) ||
        (n_struct > 0 && (!a || lda < m)))
        return fail(DZG_E_ARG, "bad argument");
    if (dzg_device_count() <= 0) return fail(DZG_E_DEVICE, "no HIP device visible");
    HIP_OK(hipSetDevice(device));
    const long long ldd = (m + 15) / 16 * 16;
    const size_t abytes = sizeof(double) * (size_t)ldd * (size_t)(n_struct ? n_struct : 1);
    double *dA, *dv, *dout;
    int *dcols;
    HIP_OK(hipMalloc(&dA, abytes));
    HIP_OK(hipMalloc(&dv, sizeof(double) * ((size_t)m + 2)));
    HIP_OK(hipMalloc(&dout, sizeof(double) * (size_t)(ncols ? ncols : 1)));
    HIP_OK(hipMalloc(&dcols, sizeof(int) * (size_t)(ncols ? ncols : 1)));
    HIP_OK(hipMemset(dA, 0, abytes));
    HIP_OK(hipMemset(dv, 0, sizeof(double) * ((size_t)m + 2)));
    if (n_struct > 0)
        HIP_OK(hipMemcpy2D(dA, sizeof(double) * ldd, a, sizeof(double) * lda, sizeof(double) * m,
                           n_struct, hipMemcpyHostToDevice));
    HIP_OK(hipMemcpy(dv, v, sizeof(double) * m, hipMemcpyHostToDevice));
    std::vector<int> c32((size_t)(ncols ? ncols : 1));
    for (int64_t k = 0; k < ncols; ++k) {
        if (cols[k] >= n_struct || cols[k] < -m) return fail(DZG_E_ARG, "cols out of range");
        c32[(size_t)k] = (int)cols[k];
    }
    HIP_OK(hipMemcpy(dcols, c32.data(), sizeof(int) * (size_t)(ncols ? ncols : 1), hipMemcpyHostToDevice));
    dzg_launch_price_raw(kernel, (int)m, ldd, dA, dcols, (int)ncols, dv, dout, 0);
    HIP_OK(hipDeviceSynchronize());
    HIP_OK(hipGetLastError());
    if (ncols > 0) HIP_OK(hipMemcpy(out, dout, sizeof(double) * ncols, hipMemcpyDeviceToHost));
    hipFree(dA); hipFree(dv); hipFree(dout); hipFree(dcols);
    return 0;
}

extern "C" int dzg_kernel_neg_t_dot_csc(int64_t m, int64_t n_struct, const int64_t *col_ptr,
                                        const int32_t *row_idx, const double *val,
                                        const int64_t *cols, int64_t ncols, const double *v,
                                        double *out, int32_t device)
{
    if (m <= 0 || n_struct < 0 || ncols < 0 || !v || !out || (ncols > 0 && !cols) || !col_ptr ||
        col_ptr[0] != 0 || (n_struct > 0 && col_ptr[n_struct] > 0 && (!row_idx || !val)))
        return fail(DZG_E_ARG, "bad argument");
    if (dzg_device_count() <= 0) return fail(DZG_E_DEVICE, "no HIP device visible");
    HIP_OK(hipSetDevice(device));
    const size_t nnz = (size_t)col_ptr[n_struct];
    for (int64_t j = 0; j < n_struct; ++j)
        for (int64_t e = col_ptr[j]; e < col_ptr[j + 1]; ++e)
            if (row_idx[e] < 0 || row_idx[e] >= m) return fail(DZG_E_ARG, "row_idx out of range");
    std::vector<long long> cp((size_t)n_struct + 1);
    for (int64_t j = 0; j <= n_struct; ++j) cp[(size_t)j] = col_ptr[j];
    std::vector<int> c32((size_t)(ncols ? ncols : 1));
    for (int64_t k = 0; k < ncols; ++k) {
        if (cols[k] >= n_struct || cols[k] < -m) return fail(DZG_E_ARG, "cols out of range");
        c32[(size_t)k] = (int)cols[k];
    }
    long long *dcp; int *dri, *dcols; double *dcv, *dv, *dout;
    HIP_OK(hipMalloc(&dcp, sizeof(long long) * cp.size()));
    HIP_OK(hipMalloc(&dri, sizeof(int) * (nnz + 1)));
    HIP_OK(hipMalloc(&dcv, sizeof(double) * (nnz + 1)));
    HIP_OK(hipMalloc(&dv, sizeof(double) * ((size_t)m + 2)));
    HIP_OK(hipMalloc(&dout, sizeof(double) * c32.size()));
    HIP_OK(hipMalloc(&dcols, sizeof(int) * c32.size()));
    HIP_OK(hipMemcpy(dcp, cp.data(), sizeof(long long) * cp.size(), hipMemcpyHostToDevice));
    if (nnz) {
        HIP_OK(hipMemcpy(dri, row_idx, sizeof(int) * nnz, hipMemcpyHostToDevice));
        HIP_OK(hipMemcpy(dcv, val, sizeof(double) * nnz, hipMemcpyHostToDevice));
    }
    HIP_OK(hipMemset(dv, 0, sizeof(double) * ((size_t)m + 2)));
    HIP_OK(hipMemcpy(dv, v, sizeof(double) * m, hipMemcpyHostToDevice));
    HIP_OK(hipMemcpy(dcols, c32.data(), sizeof(int) * c32.size(), hipMemcpyHostToDevice));
    dzg_launch_price_csc_raw(dcp, dri, dcv, dcols, (int)ncols, dv, dout, 0);
    HIP_OK(hipDeviceSynchronize());
    HIP_OK(hipGetLastError());
    if (ncols > 0) HIP_OK(hipMemcpy(out, dout, sizeof(double) * ncols, hipMemcpyDeviceToHost));
    hipFree(dcp); hipFree(dri); hipFree(dcv); hipFree(dv); hipFree(dout); hipFree(dcols);
    return 0;
}

extern "C" int dzg_kernel_first_pivot(int64_t len, const double *y, const double *ybar,
                                      int64_t *pos_out, int32_t device)
{
    if (len < 0 || !pos_out) return fail(DZG_E_ARG, "bad argument");
    if (dzg_device_count() <= 0) return fail(DZG_E_DEVICE, "no HIP device visible");
    HIP_OK(hipSetDevice(device));
    return dzg_run_first_pivot(len, y, ybar, pos_out);
}

extern "C" int dzg_kernel_second_pivot(int64_t len, double mu, const double *y, const double *ybar,
                                       const double *dy, int64_t *pos_out, int32_t device)
{
    if (len < 0 || !pos_out) return fail(DZG_E_ARG, "bad argument");
    if (dzg_device_count() <= 0) return fail(DZG_E_DEVICE, "no HIP device visible");
    HIP_OK(hipSetDevice(device));
    return dzg_run_second_pivot(len, mu, y, ybar, dy, pos_out);
}

// ---- test hooks of the pricing tail of k_chain_pre (include/dantzig_amd.h) ----------------------
extern "C" int dzg_debug_chain_price_counts(dzg_solver *s, int64_t counts[2])
{
    if (!s || !counts) return fail(DZG_E_ARG, "NULL argument");
    counts[0] = s->chain_fused;
    counts[1] = s->chain_unfused;
    return 0;
}

extern "C" int dzg_debug_chain_price_rule(int32_t m, int32_t grid, int32_t k_hint, int32_t tiles, int64_t q,
                                          int32_t small, int32_t timed)
{
    return dzg_chain_price_rule(m, grid, k_hint, tiles, q, small, timed);
}

extern "C" int dzg_debug_wk_mismatch(dzg_solver *s, int32_t clear_valid, int64_t info[2])
{
    if (!s || !info) return fail(DZG_E_ARG, "NULL argument");
    const DzgDev &d = s->d;
    if (!s->wk_buf) return fail(DZG_E_ARG, "wk mismatch: this solver keeps no compact copy of the eta rows");
    HIP_OK(hipSetDevice(s->opts.device));
    TRY(read_ctl(s));
    const int k = s->h_ctl->ncompact, neta = s->h_ctl->neta;
    if (k < 0 || k > d.m || neta < 0 || neta > DZG_RMAX)
        return fail(DZG_E_DEVICE, "wk mismatch: control block out of range");
    info[1] = s->d.wk ? 1 : 0;
    // a fresh gather of W into the flush's scratch (the flush gathers it again before it reads it)
    dzg_launch_gather_wk(d, d.Wc, s->st);
    const size_t n = (size_t)d.ldw * DZG_RMAX;
    std::vector<double> kept(n), fresh(n);
    HIP_OK(hipMemcpyAsync(kept.data(), s->wk_buf, sizeof(double) * n, hipMemcpyDeviceToHost, s->st));
    HIP_OK(hipMemcpyAsync(fresh.data(), d.Wc, sizeof(double) * n, hipMemcpyDeviceToHost, s->st));
    HIP_OK(hipStreamSynchronize(s->st));
    HIP_OK(hipGetLastError());
    int64_t bad = 0;
    for (int t = 0; t < neta; ++t)
        for (int c = 0; c < k; ++c)
            bad += std::memcmp(&kept[(size_t)t * d.ldw + c], &fresh[(size_t)t * d.ldw + c], sizeof(double)) != 0;
    info[0] = bad;
    if (clear_valid) s->d.wk = nullptr;
    return 0;
}
