// k_batch_fast.hip -- many small LPs at once in FAST numerics: one workgroup owns one LP, keeps the
// explicit basis inverse W = B^-1 (m x m doubles) in LDS and follows the reference's loop
// (src/simplex.rs:274-343) pivot for pivot, every decision through fast_decide.h on a control block
// of the LP's own: margins, near_ties, first_near_tie, min_margin and the STOP / COUNT actions mean
// what they mean in the single-LP FAST solver.  dzg_batch_solve_fast with AUTO numerics runs STOP and
// hands every LP that ends DZG_NEAR_TIE, DZG_SINGULAR or DZG_PANIC to the STRICT batch (k_batch.hip).
// dzg_batch_solve_fast_from starts the LPs that come with a basis from that basis: k_batch_fast_restart
// (below) gives each of them its restart state before the first round.  dzg_batch_solve_post adds, behind
// the rounds, the duals, ranges and rays of the states the LPs ended in (k_batch_post.hip).
//
//   layout      W[p * ld + r] = (B^-1)[basis position p][constraint row r], ld = m | 1.  BTRAN reads
//               row p with lanes along r (contiguous); FTRAN gives every thread a row and walks the
//               columns, so at a fixed column the lanes are ld doubles apart: with ld odd the 32 lanes
//               of a ds_read_b64 group fall on 32 different 8-byte bank pairs.  128 rows: 128 x 129 x 8
//               = 132 096 B of the CU's 160 KiB; then acol[m], dx[m], piv[m] and the control block.
//   refactor    at the start of every launch and every `refactor_every` pivots inside one: an all-slack
//               basis is a permutation (W[p][r] = 1 where basis[p] is row r's slack); otherwise B is
//               gathered into W and inverted in place by Gauss-Jordan with partial pivoting (first
//               maximum of |.|, lowest row on ties), the row swaps undone as column swaps at the end.
//               A zero or non-finite pivot ends the LP with DZG_SINGULAR.  The health monitor
//               (max_pivot_err, hence tau) restarts with the fresh inverse, as in k_refactor.hip.  The
//               carried x, xbar, z, zbar are NOT replaced (k_drift.hip explains why); state_drift is not
//               computed here and stays 0.
//   iteration   first-pivot scans (dzg_first_pivot_entry, runner-up carried) -> fast_status ->
//               primal: FTRAN + ratio test on x -> BTRAN + pricing;  dual: BTRAN + pricing + ratio test
//               on z -> FTRAN;  step lengths (dzg_safe_divide), x / xbar / z / zbar, swap, then
//               row p <- row p / dx_p, row i <- row i - dx_i * row p.
//   FTRAN       dx_i = sum_j W[i][j] a_q[j], j ascending in four interleaved partial sums, or column c
//               of W for the slack of row c.
//   pricing     dz_k = -a_k . v, v = row p of W: a slack column is one negation; a structural column is
//               read by PL = 16 / 32 / 64 lanes along its rows (m <= 16 / <= 32 / above), each lane
//               summing its rows in ascending order, then an xor tree.  Stored entries only.
// Every sum's order depends on m alone, every decision is taken by all threads from the same data:
// an LP's result is bit-identical wherever it sits in a batch.
//
// Launches are bounded as in k_batch.hip: at most `ppl` pivots per LP, then the state is in global
// memory and the workgroup appends its LP to the next round's list if it is still running.  Nothing
// waits on another workgroup.  The host driver (checks, packing, rounds, results) is batch_host.h's,
// the one k_batch.hip runs.  The iteration itself (the inversion, FTRAN, pricing, the step loop and the
// restart arithmetic) is batch_fast.h's, which the branch-and-bound node kernel of k_mip.hip runs too.
#include <algorithm>
#include <cstring>
#include <string>
#include <vector>

#include "batch_fast.h"
#include "batch_host.h"
#include "batch_steps.h"
#include "batch_strict.h"
#include "common.h"
#include "fast_decide.h"
#include "opts.h"
#include "ranging.h" // dzg_ranging_req_valid

namespace {

using dzg_bf::FState;
using dzg_bf::fast_lds_bytes;

struct FArgs {
    const DzgBatchLp *lp;
    const double *A;
    const int *var_col;
    int *basis, *nonbasis;
    double *x, *xbar, *z, *zbar, *dz;
    FState *state;
    int *log_kind, *log_enter, *log_leave;
    double *log_mu, *log_margin;
    double eps;
    int ppl;            // pivots per launch
    int refactor_every; // pivots between two inversions inside a launch
    int mmax;           // largest m of the bucket: sizes the LDS carve-up
};

// LP L of the batch as batch_fast.h's loop reads it
__device__ __forceinline__ dzg_bf::FastLp lp_of(const FArgs &g, const DzgBatchLp &L)
{
    dzg_bf::FastLp P;
    P.A = g.A + L.a_off;
    P.var_col = g.var_col + L.vc_off;
    P.basis = g.basis + L.m_off;
    P.nonbasis = g.nonbasis + L.q_off;
    P.x = g.x + L.m_off;
    P.xbar = g.xbar + L.m_off;
    P.z = g.z + L.q_off;
    P.zbar = g.zbar + L.q_off;
    P.dz = g.dz + L.q_off;
    P.m = L.m;
    P.q = L.n - L.m;
    P.log_kind = g.log_kind;
    P.log_enter = g.log_enter;
    P.log_leave = g.log_leave;
    P.log_mu = g.log_mu;
    P.log_margin = g.log_margin;
    P.log_off = L.log_off;
    P.log_cap = L.log_cap;
    return P;
}

// DUMP (the test hook's instantiations) adds an epilogue that copies LP id's final W to
// w_out[w_off[id] + p * m + r]; nothing else depends on it or reads the two pointers.
template <int BLOCK, int PL, bool DUMP>
__global__ __launch_bounds__(BLOCK) void k_batch_fast(FArgs g, const int *__restrict__ list,
                                                      int *__restrict__ next_list,
                                                      int *__restrict__ next_count,
                                                      double *__restrict__ w_out,
                                                      const long long *__restrict__ w_off)
{
    extern __shared__ __attribute__((aligned(16))) double s_mem[];
    const int id = list[blockIdx.x];
    const DzgBatchLp L = g.lp[id];
    const dzg_bf::FastLp P = lp_of(g, L);
    const dzg_bf::FastLds S = dzg_bf::carve(s_mem, g.mmax, L.m);
    DzgCtl *sc = S.sc;
    FState *gs = g.state + id;

    for (int i = threadIdx.x; i < (int)(sizeof(DzgCtl) / sizeof(int)); i += BLOCK)
        ((int *)sc)[i] = ((const int *)&gs->ctl)[i];
    double max_err_life = gs->max_err_life;
    long long refactors = gs->refactors;
    __syncthreads();

    const int status = dzg_bf::fast_steps<BLOCK, PL>(P, S, g.eps, g.ppl, g.refactor_every, false, max_err_life,
                                                     refactors);
    for (int i = threadIdx.x; i < (int)(sizeof(DzgCtl) / sizeof(int)); i += BLOCK)
        ((int *)&gs->ctl)[i] = ((const int *)sc)[i];
    if (threadIdx.x == 0) {
        gs->max_err_life = max_err_life;
        gs->refactors = refactors;
        if (status == DZG_RUNNING) next_list[atomicAdd(next_count, 1)] = id;
    }
    if (DUMP) { // every path out of the loop has passed a barrier since W was last written
        const int m = L.m;
        double *out = w_out + w_off[id];
        for (int e = threadIdx.x; e < m * m; e += BLOCK) {
            const int p = e / m, r = e - p * m;
            out[e] = S.W[p * S.ld + r];
        }
    }
}

// The restart state of a warm LP (dzg_batch_solve_fast_from): what
// dzg_solver_reoptimize leaves in FAST numerics, from the inverse k_batch_fast builds at step 0:
// W = build_inverse(B) of the start's basis as it lies in global memory, then batch_fast.h's
// restart_state with the right-hand side that fill_upload left in x.
//
// One workgroup per warm LP, once, before the first round; k_batch_fast's LDS carve-up.  A zero or
// non-finite pivot of the inversion, or a non-finite entry of x or z, ends the LP: DZG_SINGULAR in
// its control block and in status[id], the array the host reads back before the first round (a
// control block is 50 times an int).
template <int BLOCK, int PL>
__global__ __launch_bounds__(BLOCK) void k_batch_fast_restart(FArgs g, const double *__restrict__ cost,
                                                              int *__restrict__ status,
                                                              const int *__restrict__ list)
{
    extern __shared__ __attribute__((aligned(16))) double s_mem[];
    const int id = list[blockIdx.x];
    const DzgBatchLp L = g.lp[id];
    const dzg_bf::FastLp P = lp_of(g, L);
    const dzg_bf::FastLds S = dzg_bf::carve(s_mem, g.mmax, L.m); // the control block is not used here
    int *s_flag = S.s_flag; // [0], [1]: build_inverse's; [2]: a non-finite entry of x or z
    FState *gs = g.state + id;
    const bool lead = threadIdx.x == 0;

    if (lead) s_flag[2] = 0;
    int inverted = 0;
    const int bad = P.m > 0 ? dzg_bf::build_inverse<BLOCK, PL>(S.W, S.ld, P.m, P.A, P.var_col, P.basis, S.acol,
                                                               S.piv, s_flag, inverted)
                            : 0;
    if (lead) gs->refactors = inverted;
    if (bad) {
        if (lead) gs->ctl.status = status[id] = DZG_SINGULAR;
        return;
    }
    const double *x = P.x;
    dzg_bf::restart_state<BLOCK, PL>(P, S, cost + L.vc_off, [x](int i) { return x[i]; });
    if (lead && s_flag[2]) gs->ctl.status = status[id] = DZG_SINGULAR;
}

namespace bh = dzg_bh;

// The warm LPs list[0..n) of row bucket b, one workgroup each: launch_bucket's instantiations and LDS
void launch_restart_bucket(int b, const FArgs &g, const double *cost, int *status, const int *list, int n,
                           hipStream_t st)
{
    const size_t lds = fast_lds_bytes(g.mmax);
    if (b == 3) { // more than 64 KiB of dynamic LDS, as in launch_bucket
        static const hipError_t attr =
            hipFuncSetAttribute(reinterpret_cast<const void *>(k_batch_fast_restart<256, 64>),
                                hipFuncAttributeMaxDynamicSharedMemorySize, (int)fast_lds_bytes(DZG_BATCH_MAX_ROWS));
        (void)attr;
    }
    bh::for_each_chunk(b, n, [&](int c0, int grid) {
        const dim3 block(bh::kBlock[b]);
        if (b == 0)
            hipLaunchKernelGGL((k_batch_fast_restart<64, 16>), dim3(grid), block, lds, st, g, cost, status,
                               list + c0);
        else if (b == 1)
            hipLaunchKernelGGL((k_batch_fast_restart<64, 32>), dim3(grid), block, lds, st, g, cost, status,
                               list + c0);
        else if (b == 2)
            hipLaunchKernelGGL((k_batch_fast_restart<128, 64>), dim3(grid), block, lds, st, g, cost, status,
                               list + c0);
        else
            hipLaunchKernelGGL((k_batch_fast_restart<256, 64>), dim3(grid), block, lds, st, g, cost, status,
                               list + c0);
    });
}

thread_local double t_restart_ms = 0.0; // dzg_debug_batch_fast_restart_ms

// ---- the restart state of the warm LPs: c goes up, one workgroup each, bucket by bucket, before the
// first round.  A singular start leaves the first round's lists; `live` follows.
int restart_pass(const dzg_lp *lps, const dzg_batch_start *start, const bh::Packed &P, const dzg_steps::FastRun &R,
                 unsigned char *host, std::array<int, bh::kBuckets> &live)
{
    const bh::Layout &L = *R.L;
    unsigned char *dev = R.dev;
    hipStream_t st = R.st;
    const size_t s_c = R.c, s_status = R.rst;
    const int N = L.N;
    std::vector<double> cost((size_t)P.nvc);
    for (int i = 0; i < N; ++i)
        std::copy(lps[i].c, lps[i].c + lps[i].n, cost.begin() + P.desc[(size_t)i].vc_off);
    DZG_HIP(hipMemcpyAsync(dev + s_c, cost.data(), sizeof(double) * cost.size(), hipMemcpyHostToDevice, st));
    const bh::StatusLists warm = bh::warm_lists(lps, start, N);
    // the next round's list is free until the first round appends to it
    int *wlist = (int *)(dev + L.list2);
    DZG_HIP(hipMemcpyAsync(wlist, warm.list.data(), sizeof(int) * warm.list.size(), hipMemcpyHostToDevice, st));
    bh::Events ev;
    DZG_HIP(hipEventCreate(&ev.e0));
    DZG_HIP(hipEventCreate(&ev.e1));
    DZG_HIP(hipEventRecord(ev.e0, st));
    if (const int rc = dzg_steps::fast_restart(R, wlist, warm.seg, P.mmax)) return rc;
    DZG_HIP(hipEventRecord(ev.e1, st));
    int *status = (int *)(host + s_status);
    DZG_HIP(hipMemcpyAsync(status, dev + s_status, sizeof(int) * N, hipMemcpyDeviceToHost, st));
    DZG_HIP(hipStreamSynchronize(st)); // (cost and the lists are uploaded: they may go)
    float ms = 0.0f;
    DZG_HIP(hipEventElapsedTime(&ms, ev.e0, ev.e1));
    t_restart_ms = ms;
    if (std::all_of(status, status + N, [](int s) { return s == DZG_RUNNING; })) return 0;
    return bh::drop_from_first_round(host, dev, L, P, live, st, [&](int i) { return status[i] != DZG_RUNNING; });
}

template <bool DUMP>
void launch_bucket(int b, const FArgs &g, const int *list, int n, int *next_list, int *next_count,
                   hipStream_t st, double *w_out = nullptr, const long long *w_off = nullptr)
{
    const size_t lds = fast_lds_bytes(g.mmax);
    if (b == 3) { // more than 64 KiB of dynamic LDS: say so once (a runtime that needs no telling ignores it)
        static const hipError_t attr =
            hipFuncSetAttribute(reinterpret_cast<const void *>(k_batch_fast<256, 64, DUMP>),
                                hipFuncAttributeMaxDynamicSharedMemorySize, (int)fast_lds_bytes(DZG_BATCH_MAX_ROWS));
        (void)attr;
    }
    bh::for_each_chunk(b, n, [&](int c0, int grid) {
        const dim3 block(bh::kBlock[b]);
        // the pricing lanes per column follow the bucket's rows: 16, 32, then the whole wave
        if (b == 0)
            hipLaunchKernelGGL((k_batch_fast<64, 16, DUMP>), dim3(grid), block, lds, st, g, list + c0, next_list,
                               next_count, w_out, w_off);
        else if (b == 1)
            hipLaunchKernelGGL((k_batch_fast<64, 32, DUMP>), dim3(grid), block, lds, st, g, list + c0, next_list,
                               next_count, w_out, w_off);
        else if (b == 2)
            hipLaunchKernelGGL((k_batch_fast<128, 64, DUMP>), dim3(grid), block, lds, st, g, list + c0, next_list,
                               next_count, w_out, w_off);
        else
            hipLaunchKernelGGL((k_batch_fast<256, 64, DUMP>), dim3(grid), block, lds, st, g, list + c0, next_list,
                               next_count, w_out, w_off);
    });
}

// The control block a FAST LP starts with, as dzg_solver_create starts a FAST solver's.
void start_ctl(DzgCtl &c0, const dzg_opts &o, long long max_iter)
{
    c0.status = DZG_RUNNING;
    c0.iter_stop = max_iter;
    c0.enter_pos = c0.leave_pos = -1;
    c0.del_ce = c0.del_last = -1;
    c0.rl_listed = -1;
    c0.tie_tol = c0.tau = o.tie_tol;
    c0.margin = c0.min_margin = __builtin_inf();
    c0.first_near_tie = c0.tie_skip_iter = -1;
    c0.tie_mode = o.near_tie_action == DZG_NEAR_TIE_STOP ? 1 : 0;
}

// What FAST reports beyond unpack_common: its counters, the margins and the structural columns of
// the final basis.
void write_fast(const dzg_lp &lp, const DzgBatchLp &d, const FState &fs, const int *basis, const double *lmg,
                dzg_result &r)
{
    const DzgCtl &c = fs.ctl;
    int64_t dense = 0;
    for (int64_t p = 0; p < lp.m; ++p) {
        const int var = basis[d.m_off + p];
        const int64_t code = lp.var_col ? lp.var_col[var] : (var < lp.n_struct ? var : -1);
        if (code >= 0) ++dense;
    }
    const long long cnt = std::min<long long>(r.iterations, d.log_cap);
    if (r.margins)
        for (long long k = 0; k < cnt; ++k) r.margins[k] = lmg[d.log_off + k];
    r.max_pivot_error = fs.max_err_life;
    r.near_ties = c.near_ties;
    r.first_near_tie = c.first_near_tie;
    r.min_margin = c.min_margin;
    r.dense_columns = dense;
    r.refactors = fs.refactors;
}

// The kernel arguments of a solve that lies as R says (mmax is the launch's own).
FArgs fast_args(const dzg_steps::FastRun &R)
{
    FArgs g;
    bh::wire(g, R.dev, *R.L);
    g.state = (FState *)(R.dev + R.state);
    g.log_margin = (double *)(R.dev + R.margin);
    g.eps = R.eps;
    g.ppl = R.ppl;
    g.refactor_every = R.refactor_every;
    g.mmax = 0;
    return g;
}

} // namespace

#define DZG_BATCH_FAST_DEFAULT_PPL 128
#define DZG_BATCH_FAST_DEFAULT_REFACTOR 64

// ---- the steps of batch_steps.h
int dzg_steps::fast_ppl(int64_t pivots_per_launch)
{
    return (int)(pivots_per_launch > 0 ? std::min<int64_t>(pivots_per_launch, 1 << 30) : DZG_BATCH_FAST_DEFAULT_PPL);
}

int dzg_steps::fast_refactor_every(int64_t refactor_every)
{
    return (int)(refactor_every > 0 ? std::min<int64_t>(refactor_every, 1 << 30) : DZG_BATCH_FAST_DEFAULT_REFACTOR);
}

size_t dzg_steps::fast_state_bytes() { return sizeof(FState); }

void dzg_steps::fast_state_init(void *block, const dzg_opts &o, long long max_iter)
{
    std::memset(block, 0, sizeof(FState));
    start_ctl(((FState *)block)->ctl, o, max_iter);
}

int dzg_steps::fast_restart(const FastRun &R, const int *wlist, const bh::Segments &wseg, const int *mmax)
{
    const FArgs g = fast_args(R);
    for (int b = 0; b < bh::kBuckets; ++b) {
        const int cnt = wseg[(size_t)b + 1] - wseg[(size_t)b];
        if (cnt == 0) continue;
        FArgs gb = g;
        gb.mmax = mmax[b];
        launch_restart_bucket(b, gb, (const double *)(R.dev + R.c), (int *)(R.dev + R.rst),
                              wlist + wseg[(size_t)b], cnt, R.st);
        DZG_HIP(hipGetLastError());
    }
    return 0;
}

int dzg_steps::fast_rounds(const FastRun &R, int *cur, int *nxt, const bh::Segments &seg,
                           const std::array<int, bh::kBuckets> &live, const int *mmax, double *w_out,
                           const long long *w_off, int *rounds)
{
    const FArgs g = fast_args(R);
    return bh::run_rounds(cur, nxt, (int *)(R.dev + R.L->count), seg, live, R.st,
                          [&](int b, const int *list, int n, int *next_list, int *next_count) {
                              FArgs gb = g;
                              gb.mmax = mmax[b];
                              if (w_out)
                                  launch_bucket<true>(b, gb, list, n, next_list, next_count, R.st, w_out, w_off);
                              else
                                  launch_bucket<false>(b, gb, list, n, next_list, next_count, R.st);
                          }, rounds);
}

void dzg_steps::fast_unpack(const dzg_lp &lp, const DzgBatchLp &d, const bh::HostView &view, const void *block,
                            const double *margins, dzg_result &r)
{
    const FState &fs = *(const FState *)block;
    r.status = fs.ctl.status;
    r.numerics_used = DZG_NUMERICS_FAST;
    r.iterations = fs.ctl.iter;
    bh::unpack_common(lp, d, view, r);
    write_fast(lp, d, fs, view.basis, margins, r);
}

long long dzg_steps::fast_state_iter(const void *block) { return ((const FState *)block)->ctl.iter; }

// The FAST batch itself: `o.near_tie_action` and `o.tie_tol` as given.  The driver is batch_host.h's,
// as in k_batch.hip; the state block and the margins are FAST's own sections.
// With w_out (dzg_debug_batch_fast_inverse) the budget is `pivots_per_launch` pivots in one launch of
// the DUMP instantiations: iter_stop is that budget and the launch has one step more, so that
// fast_status ends it -- after W was built, also when the budget is 0 -- and W comes down with the state.
// An LP with a start basis (dzg_batch_solve_fast_from) is laid out by fill_upload as k_batch_fast_restart
// reads it and gets its restart state from one launch per bucket between the upload and the first round;
// c (by variable) goes up behind the solve's sections, for those launches alone.
static int batch_solve_fast(const dzg_lp *lps, const dzg_batch_start *start, int64_t count, const dzg_opts &o,
                            int64_t pivots_per_launch, int64_t refactor_every_arg, dzg_result *res,
                            double *w_out = nullptr, const dzg_batch_post *post = nullptr)
{
    const bool dump = w_out != nullptr;
    const bool warm = bh::any_warm(start, (int)count);
    const long long max_iter = dump ? std::min<int64_t>(pivots_per_launch, 1 << 30)
                                    : dzg_opts_resolved(&o).max_iter;
    if (const int rc = bh::use_device(o.device)) return rc;

    const int N = (int)count;
    const bh::Packed P = bh::pack(lps, res, N, max_iter);
    bh::Layout L(P);
    const size_t s_state = L.ar.add(sizeof(FState) * N);
    const size_t s_woff = L.ar.add(dump ? sizeof(long long) * N : 0);
    const size_t s_rst = L.ar.add(warm ? sizeof(int) * N : 0); // the restart's statuses: DZG_RUNNING
    L.end_upload();
    const size_t s_lmg = L.ar.add(sizeof(double) * P.nlog);
    std::vector<long long> w_off((size_t)N + 1, 0);
    for (int i = 0; i < N; ++i) w_off[(size_t)i + 1] = w_off[(size_t)i] + (long long)lps[i].m * lps[i].m;
    const size_t s_w = L.ar.add(dump ? sizeof(double) * (size_t)w_off[(size_t)N] : 0);
    L.end_download();
    const size_t s_c = L.ar.add(warm ? sizeof(double) * (size_t)P.nvc : 0);
    dzg_steps::PostSections PSec; // the post-solve's sections, behind everything the solve has
    if (post) dzg_steps::post_layout(L.ar, PSec, P.nvc, P.nm, P.nq, N);

    std::vector<unsigned char> host(L.download_end, 0);
    bh::fill_upload(host.data(), L, P, lps, start);
    FState *fs = (FState *)(host.data() + s_state);
    for (int i = 0; i < N; ++i) dzg_steps::fast_state_init(&fs[i], o, max_iter);
    if (warm) std::fill_n((int *)(host.data() + s_rst), N, (int)DZG_RUNNING);
    if (dump) std::memcpy(host.data() + s_woff, w_off.data(), sizeof(long long) * N);
    bh::Device D;
    if (const int rc = bh::upload(D, L, host.data())) return rc;
    unsigned char *dev = D.arena;

    dzg_steps::FastRun R;
    R.dev = dev;
    R.L = &L;
    R.state = s_state;
    R.margin = s_lmg;
    R.rst = s_rst;
    R.c = s_c;
    R.eps = dzg_opts_resolved(&o).epsilon;
    R.ppl = dump ? (int)max_iter + 1 : dzg_steps::fast_ppl(pivots_per_launch);
    R.refactor_every = dzg_steps::fast_refactor_every(refactor_every_arg);
    R.st = D.st;
    std::array<int, bh::kBuckets> live = bh::live_of(P.bucket_n);
    if (warm)
        if (const int rc = restart_pass(lps, start, P, R, host.data(), live)) return rc;
    const int rc_rounds = dzg_steps::fast_rounds(
        R, (int *)(dev + L.list), (int *)(dev + L.list2), bh::segments(P.bucket_n), live, P.mmax,
        dump ? (double *)(dev + s_w) : nullptr, dump ? (const long long *)(dev + s_woff) : nullptr);
    if (rc_rounds) return rc_rounds;
    if (const int rc = bh::download(D, L, host.data())) return rc;

    const bh::HostView view(host.data(), L);
    for (int i = 0; i < N; ++i) {
        dzg_steps::fast_unpack(lps[i], P.desc[(size_t)i], view, &fs[i], (const double *)(host.data() + s_lmg),
                               res[i]);
    }
    if (dump) std::memcpy(w_out, host.data() + s_w, sizeof(double) * (size_t)w_off[(size_t)N]);
    if (!post) return 0;
    // ---- what the LPs can say about where they ended: c and the right-hand sides go up, then
    // batch_steps.h's pass.  A warm LP's right-hand side goes by constraint row, as fill_upload sent
    // it; a cold LP's starting x is taken as it is (dzg_duals: "the batch calls take the starting x")
    std::vector<double> cr((size_t)(P.nvc + P.nm), 0.0);
    for (int i = 0; i < N; ++i) {
        const dzg_lp &lp = lps[i];
        const DzgBatchLp &d = P.desc[(size_t)i];
        std::copy(lp.c, lp.c + lp.n, cr.begin() + d.vc_off);
        const bool by_row = start && start[i].basis;
        for (int64_t k = 0; k < lp.m; ++k)
            cr[(size_t)(P.nvc + d.m_off + (by_row ? -1 - bh::var_code(lp, lp.basis[k]) : k))] = lp.x[k];
    }
    DZG_HIP(hipMemcpyAsync(dev + PSec.c, cr.data(), sizeof(double) * (size_t)P.nvc, hipMemcpyHostToDevice, D.st));
    DZG_HIP(hipMemcpyAsync(dev + PSec.rhs0, cr.data() + P.nvc, sizeof(double) * (size_t)P.nm, hipMemcpyHostToDevice,
                           D.st));
    dzg_steps::PostRun PR;
    PR.dev = dev;
    PR.L = &L;
    PR.state = s_state;
    PR.S = PSec;
    PR.st = D.st;
    double ms = 0.0;
    const int rc_post = dzg_steps::post_pass(PR, false, P, N, nullptr, res, *post, nullptr, nullptr, &ms);
    dzg_steps::post_ms() = ms;
    return rc_post;
}

// dzg_batch_solve_fast_from, and behind it what `post` (NULL or empty: nothing) asks for.
static int solve_fast_from(const dzg_lp *lps, const dzg_batch_start *start, int64_t count, const dzg_opts *opts,
                           int64_t pivots_per_launch, int64_t refactor_every, const dzg_batch_post *post,
                           dzg_result *res)
{
    t_restart_ms = 0.0;
    dzg_steps::post_ms() = 0.0;
    if (post && !post->du && !post->req && !post->rg && !post->ry) post = nullptr;
    // ---- host checks first: malformed input is DZG_E_ARG on any machine
    if (const int rc = bh::check_batch(lps, count, res, pivots_per_launch)) return rc;
    if (refactor_every < 0) return dzg_set_error(DZG_E_ARG, "batch: refactor_every < 0");
    if (count > 0 && post && (post->req != nullptr) != (post->rg != nullptr))
        return dzg_set_error(DZG_E_ARG, "batch: req and rg go together (one of them is NULL)");
    dzg_opts o;
    if (opts) o = *opts; else dzg_opts_default(&o);
    if (o.numerics != DZG_NUMERICS_STRICT && o.numerics != DZG_NUMERICS_FAST && o.numerics != DZG_NUMERICS_AUTO)
        return dzg_set_error(DZG_E_ARG, "batch: opts.numerics");
    if (o.numerics == DZG_NUMERICS_STRICT) {
        if (!post) return dzg_batch_solve_from(lps, start, count, &o, pivots_per_launch, res, nullptr);
        return dzg_steps::strict_post(lps, start, count, &o, pivots_per_launch, res, post->du, post->req, post->rg,
                                      post->ry);
    }
    const int rc_lps = bh::check_batch(lps, count, [&](int64_t i, std::string &why) {
        if (start && !bh::start_valid(lps[i], start[i], why)) return false;
        return !post || !post->req || dzg_ranging_req_valid(&post->req[i], lps[i].m, lps[i].n, why);
    });
    if (rc_lps) return rc_lps;
    if (count == 0) return 0;
    const bool is_auto = o.numerics == DZG_NUMERICS_AUTO;
    if (is_auto) o.near_tie_action = DZG_NEAR_TIE_STOP;
    const int rc = batch_solve_fast(lps, start, count, o, pivots_per_launch, refactor_every, res, nullptr, post);
    if (rc < 0 || !is_auto) return rc;
    // ---- AUTO: only the reference's own arithmetic can arbitrate a tie -- the LPs FAST gave up on
    // are solved again by the STRICT batch, each from the start it had here (a cold one from its
    // first pivot), into the same result slots; their post-solve is the STRICT batch's too
    std::vector<int64_t> redo;
    for (int64_t i = 0; i < count; ++i)
        if (res[i].status == DZG_NEAR_TIE || res[i].status == DZG_SINGULAR || res[i].status == DZG_PANIC)
            redo.push_back(i);
    if (redo.empty()) return 0;
    std::vector<dzg_lp> lps2(redo.size());
    std::vector<dzg_result> res2(redo.size());
    std::vector<dzg_batch_start> start2(redo.size(), dzg_batch_start{nullptr, nullptr});
    std::vector<dzg_duals> du2;
    std::vector<dzg_ranging_req> req2;
    std::vector<dzg_ranging> rg2;
    std::vector<dzg_ray> ry2;
    for (size_t k = 0; k < redo.size(); ++k) {
        lps2[k] = lps[redo[k]];
        res2[k] = res[redo[k]];
        if (start) start2[k] = start[redo[k]];
        if (post && post->du) du2.push_back(post->du[redo[k]]); // (the caller's arrays are written in place)
        if (post && post->req) req2.push_back(post->req[redo[k]]);
        if (post && post->req) rg2.push_back(post->rg[redo[k]]);
        if (post && post->ry) ry2.push_back(post->ry[redo[k]]);
    }
    dzg_opts os = o;
    os.numerics = DZG_NUMERICS_STRICT;
    const int rc2 =
        post ? dzg_steps::strict_post(lps2.data(), start2.data(), (int64_t)redo.size(), &os, 0, res2.data(),
                                      du2.empty() ? nullptr : du2.data(), req2.empty() ? nullptr : req2.data(),
                                      rg2.empty() ? nullptr : rg2.data(), ry2.empty() ? nullptr : ry2.data())
             : dzg_batch_solve_from(lps2.data(), start2.data(), (int64_t)redo.size(), &os, 0, res2.data(), nullptr);
    if (rc2 < 0) return rc2;
    for (size_t k = 0; k < redo.size(); ++k) {
        res[redo[k]] = res2[k];
        if (!du2.empty()) post->du[redo[k]] = du2[k];
        if (!ry2.empty()) post->ry[redo[k]] = ry2[k];
    }
    return 0;
}

extern "C" int dzg_batch_solve_fast_from(const dzg_lp *lps, const dzg_batch_start *start, int64_t count,
                                         const dzg_opts *opts, int64_t pivots_per_launch,
                                         int64_t refactor_every, dzg_result *res)
{
    return solve_fast_from(lps, start, count, opts, pivots_per_launch, refactor_every, nullptr, res);
}

extern "C" int dzg_batch_solve_post(const dzg_lp *lps, const dzg_batch_start *start, int64_t count,
                                    const dzg_opts *opts, int64_t pivots_per_launch, int64_t refactor_every,
                                    const dzg_batch_post *post, dzg_result *res)
{
    return solve_fast_from(lps, start, count, opts, pivots_per_launch, refactor_every, post, res);
}

extern "C" int dzg_batch_solve_fast(const dzg_lp *lps, int64_t count, const dzg_opts *opts,
                                    int64_t pivots_per_launch, int64_t refactor_every, dzg_result *res)
{
    return dzg_batch_solve_fast_from(lps, nullptr, count, opts, pivots_per_launch, refactor_every, res);
}

extern "C" double dzg_debug_batch_fast_restart_ms(void) { return t_restart_ms; }

// Test hook (tests/test_gpu_batch_fast_inverse.py): the W = B^-1 a FAST batch launch keeps in LDS.
// Every LP's W is built from its starting basis as a launch builds it at step 0, at most `pivots`
// pivots run in that one launch (refactor_every as in dzg_batch_solve_fast), res[i] is filled as
// dzg_batch_solve_fast fills it, and the final W goes to w_out: LP after LP, m x m row-major, row p
// basis position p, column r constraint row r.  opts->max_iter is not consulted: `pivots` is the budget.
extern "C" int dzg_debug_batch_fast_inverse(const dzg_lp *lps, int64_t count, const dzg_opts *opts, int64_t pivots,
                                            int64_t refactor_every, double *w_out, dzg_result *res)
{
    if (const int rc = bh::check_batch(lps, count, res, pivots, w_out ? nullptr : "w_out")) return rc;
    if (refactor_every < 0) return dzg_set_error(DZG_E_ARG, "batch: refactor_every < 0");
    dzg_opts o;
    if (opts) o = *opts; else dzg_opts_default(&o);
    if (!opts || o.numerics != DZG_NUMERICS_FAST)
        return dzg_set_error(DZG_E_ARG, "dzg_debug_batch_fast_inverse: FAST numerics only");
    if (const int rc = bh::check_batch(lps, count)) return rc;
    if (count == 0) return 0;
    return batch_solve_fast(lps, nullptr, count, o, pivots, refactor_every, res, w_out);
}
