// k_batch.hip -- many small LPs at once in STRICT numerics: one workgroup owns one LP and runs the
// reference's loop (src/simplex.rs:274-343) for it, with no communication between workgroups.
//
//   status()            scan_first over z / zbar and x / xbar (common.h), the decision of
//                       src/simplex.rs:274-306 taken redundantly by every thread
//   solve_for_dx / _dz  a fresh LU of B (B^T) in LDS: one m x (m+1) buffer, the right-hand side
//                       riding along as column m (the forward substitution of LU::solve is the
//                       same sequence of operations on that column), then the back substitution
//   neg_t_dot           one thread per nonbasic column, stored entries only, rows ascending
//                       (oracle/dzg_oracle.c price(): a dense zero is skipped, a slack column
//                       contributes 1.0 * -v)
//   find_second_pivot   scan_second (common.h)
//   pivot x4 + swap     src/simplex.rs:253-268, :410-421, :239-251
//
// The arithmetic is k_strict.hip's: LINPACK LU with partial pivoting (first maximum of |.| under
// strict '>', swaps on columns >= k, unpermuted L, zero pivot skipped), one rounded product and one
// rounded subtraction per element and step in ascending k, never fused (-ffp-contract=off), every
// division through dzg_div / dzg_safe_divide.  Which thread applies an element's update is the only
// freedom taken.
//
// Per elimination step: wave 0 searches the pivot (a shuffle argmax), swaps the two rows on columns
// >= k and forms the multipliers; one barrier; every thread updates the trailing block; one barrier.
// The back substitution is a serial chain of m(m-1)/2 dependent subtractions: wave 0 forms a row's
// products in parallel and chains them in order through readlane.
//
// Launches are bounded: at most `ppl` pivots per LP, then the state is in global memory and the
// workgroup appends its LP to the next round's list if it is still running.  Nothing waits on
// another workgroup.
#include <algorithm>
#include <cstring>
#include <string>
#include <vector>

#include "batch_host.h"
#include "batch_restart.h"
#include "batch_steps.h"
#include "batch_strict.h"
#include "common.h"
#include "duals.h"
#include "opts.h"
#include "ranging.h"
#include "rays.h"

namespace {

struct BArgs {
    const DzgBatchLp *lp;
    const double *A;
    const int *var_col;
    int *basis, *nonbasis;
    double *x, *xbar, *z, *zbar, *dz;
    int *status;
    long long *iter;
    int *log_kind, *log_enter, *log_leave;
    double *log_mu;
    long long max_iter;
    double eps;
    int ppl;   // pivots per launch
    int mmax;  // largest m of the bucket: sizes the LDS carve-up
};

template <int BLOCK>
__global__ __launch_bounds__(BLOCK) void k_batch_strict(BArgs g, const int *__restrict__ list,
                                                        int *__restrict__ next_list,
                                                        int *__restrict__ next_count)
{
    extern __shared__ __attribute__((aligned(16))) double s_mem[];
    const int id = list[blockIdx.x];
    const DzgBatchLp L = g.lp[id];
    dzg_bs::LpState S;
    S.A = g.A + L.a_off;
    S.var_col = g.var_col + L.vc_off;
    S.m = L.m;
    S.q = L.n - L.m;
    S.basis = g.basis + L.m_off;
    S.nonbasis = g.nonbasis + L.q_off;
    S.x = g.x + L.m_off;
    S.xbar = g.xbar + L.m_off;
    S.z = g.z + L.q_off;
    S.zbar = g.zbar + L.q_off;
    S.dz = g.dz + L.q_off;
    S.log_kind = g.log_kind + L.log_off;
    S.log_enter = g.log_enter + L.log_off;
    S.log_leave = g.log_leave + L.log_off;
    S.log_mu = g.log_mu + L.log_off;
    S.log_cap = L.log_cap;
    long long it = g.iter[id];
    const int status = dzg_bs::strict_steps<BLOCK>(S, s_mem, g.mmax, it, g.max_iter, g.eps, g.ppl);
    if (threadIdx.x == 0) {
        g.status[id] = status;
        g.iter[id] = it;
        if (status == DZG_RUNNING) next_list[atomicAdd(next_count, 1)] = id;
    }
}

namespace bh = dzg_bh;
using bh::kBuckets;
using dzg_bs::lds_bytes;

void launch_bucket(int b, const BArgs &g, const int *list, int n, int *next_list, int *next_count,
                   hipStream_t st)
{
    const size_t lds = lds_bytes(g.mmax);
    bh::for_each_chunk(b, n, [&](int c0, int grid) {
        bh::with_block(b, [&](auto block) {
            constexpr int BLOCK = decltype(block)::value;
            hipLaunchKernelGGL(k_batch_strict<BLOCK>, dim3(grid), dim3(BLOCK), lds, st, g, list + c0,
                               next_list, next_count);
        });
    });
}

// The kernel arguments of a solve that lies as R says (mmax is the launch's own).
BArgs strict_args(const dzg_steps::StrictRun &R)
{
    BArgs g;
    bh::wire(g, R.dev, *R.L);
    g.status = (int *)(R.dev + R.status);
    g.iter = (long long *)(R.dev + R.iter);
    g.max_iter = R.max_iter;
    g.eps = R.eps;
    g.ppl = R.ppl;
    g.mmax = 0;
    return g;
}

// What a call asks for beside the solve, and where it goes.
struct BatchExtras {
    bool duals = false, ranging = false, rays = false;
    dzg_duals *du = nullptr;              // duals: of the LPs that end OPTIMAL
    const dzg_ranging_req *req = nullptr; // ranging: of the OPTIMAL LPs, after their duals
    dzg_ranging *rg = nullptr;
    dzg_ray *ry = nullptr;                // rays: of the LPs that end UNBOUNDED or INFEASIBLE
};

// One call of batch_solve.  The post-solve passes read the descriptors (P), the device pointers of
// the final state (g), P.mmax, the downloaded statuses and the stream (D.st); each keeps what it
// brought down in the buffers named after it.
struct Ctx {
    const dzg_lp *lps;
    const dzg_batch_start *start; // dzg_batch_solve_from: the LPs with a start basis are warm
    bool warm = false;            // any of them
    int N;
    dzg_result *res;
    BatchExtras ex;
    bh::Packed P;
    bh::Layout L;
    size_t status = 0, iter = 0; // the STRICT state sections
    // sections behind the solve's: duals (c and the starting x go up; y, d and the scalars come
    // down), then rays (d, y and the scalars come down)
    // (c alone goes up as well whenever an LP is warm: the restart prices with it)
    size_t c = 0, x0 = 0, dlist = 0, y = 0, d = 0, scal = 0, duals_end = 0;
    size_t rlist = 0, rd = 0, ry = 0, rscal = 0;
    std::vector<unsigned char> host;
    bh::Device D;
    dzg_steps::StrictRun R; // where the solve lies; max_iter, eps and ppl are batch_solve's to set
    BArgs g;
    std::vector<unsigned char> cx0;    // c .. x0 as uploaded
    std::vector<unsigned char> dhost;  // y .. scal as downloaded
    std::vector<unsigned char> ryhost; // rd .. rscal as downloaded
    std::vector<unsigned char> rhost;  // the ranging pass's arena (D.arena2) as uploaded and downloaded
    std::vector<long long> rg_out;     // LP i's ranges: rg_out[i] .., cost directions first
    size_t r_lo = 0, r_hi = 0, r_lov = 0, r_hiv = 0;

    Ctx(const dzg_lp *lps_, const dzg_batch_start *start_, int n, dzg_result *res_, const BatchExtras &ex_,
        long long max_iter)
        : lps(lps_), start(start_), N(n), res(res_), ex(ex_), P(bh::pack(lps_, res_, n, max_iter)), L(P)
    {
        for (int i = 0; start && i < n; ++i) warm = warm || start[i].basis;
    }
    bool is_warm(int i) const { return start && start[i].basis; }
    const int *stat() const { return (const int *)(host.data() + status); } // after the download
};

// The arena's sections and the upload buffer, the device's copy of it, the kernel arguments.
int pack_and_upload(Ctx &C)
{
    const int N = C.N;
    bh::Layout &L = C.L;
    C.status = L.ar.add(sizeof(int) * N);
    C.iter = L.ar.add(sizeof(long long) * N);
    L.end_upload();
    L.end_download();
    const bool post = C.ex.duals || C.ex.rays;
    if (post || C.warm) C.c = L.ar.add(sizeof(double) * C.P.nvc);
    if (post) {
        C.x0 = L.ar.add(sizeof(double) * C.P.nm);
        C.dlist = L.ar.add(sizeof(int) * N);
        C.y = L.ar.add(sizeof(double) * C.P.nm);
        C.d = L.ar.add(sizeof(double) * C.P.nvc);
        C.scal = L.ar.add(sizeof(double) * DZG_DUALS_SCAL * N);
    }
    C.duals_end = L.ar.top;
    if (C.ex.rays) {
        C.rlist = L.ar.add(sizeof(int) * N);
        C.rd = L.ar.add(sizeof(double) * C.P.nvc);
        C.ry = L.ar.add(sizeof(double) * C.P.nm);
        C.rscal = L.ar.add(sizeof(double) * DZG_RAY_SCAL * N);
    }
    C.host.assign(L.download_end, 0);
    bh::fill_upload(C.host.data(), L, C.P, C.lps, C.start);
    int *st = (int *)(C.host.data() + C.status);
    for (int i = 0; i < N; ++i) st[i] = DZG_RUNNING;
    if (const int rc = bh::upload(C.D, L, C.host.data())) return rc;
    unsigned char *dev = C.D.arena;
    if (post || C.warm) { // c and the starting x, for the restart and the passes behind the solve
        C.cx0.assign(post ? C.dlist - C.c : sizeof(double) * (size_t)C.P.nvc, 0);
        double *cc = (double *)C.cx0.data(), *x0 = post ? (double *)(C.cx0.data() + (C.x0 - C.c)) : nullptr;
        for (int i = 0; i < N; ++i) {
            const dzg_lp &lp = C.lps[i];
            const DzgBatchLp &d = C.P.desc[(size_t)i];
            for (int64_t v = 0; v < lp.n; ++v) cc[d.vc_off + v] = lp.c[v];
            for (int64_t k = 0; post && k < lp.m; ++k) x0[d.m_off + k] = lp.x[k];
        }
        DZG_HIP(hipMemcpyAsync(dev + C.c, C.cx0.data(), C.cx0.size(), hipMemcpyHostToDevice, C.D.st));
    }
    C.R.dev = dev;
    C.R.L = &C.L;
    C.R.status = C.status;
    C.R.iter = C.iter;
    C.R.c = C.c;
    C.R.st = C.D.st;
    C.g = strict_args(C.R);
    return 0;
}

thread_local double t_restart_ms = 0.0; // dzg_debug_batch_restart_ms

// ---- the restart state of the warm LPs: one workgroup each, bucket by bucket, before the first
// round.  A singular start leaves the first round's lists; `live` follows.
int restart_pass(Ctx &C, std::array<int, kBuckets> &live)
{
    unsigned char *dev = C.D.arena;
    hipStream_t st = C.D.st;
    const bh::StatusLists warm = bh::warm_lists(C.lps, C.start, C.N);
    const bh::Segments &wseg = warm.seg;
    // the next round's list is free until the first round appends to it
    int *wlist = (int *)(dev + C.L.list2);
    DZG_HIP(hipMemcpyAsync(wlist, warm.list.data(), sizeof(int) * warm.list.size(), hipMemcpyHostToDevice, st));
    bh::Events ev;
    DZG_HIP(hipEventCreate(&ev.e0));
    DZG_HIP(hipEventCreate(&ev.e1));
    DZG_HIP(hipEventRecord(ev.e0, st));
    if (const int rc = dzg_steps::strict_restart(C.R, wlist, wseg, C.P.mmax)) return rc;
    DZG_HIP(hipEventRecord(ev.e1, st));
    std::vector<int> status((size_t)C.N);
    DZG_HIP(hipMemcpyAsync(status.data(), dev + C.status, sizeof(int) * C.N, hipMemcpyDeviceToHost, st));
    DZG_HIP(hipStreamSynchronize(st));
    float ms = 0.0f;
    DZG_HIP(hipEventElapsedTime(&ms, ev.e0, ev.e1));
    t_restart_ms = ms;
    if (std::all_of(status.begin(), status.end(), [](int s) { return s == DZG_RUNNING; })) return 0;
    // the first round's lists without the singular starts
    return bh::drop_from_first_round(C.host.data(), dev, C.L, C.P, live, st,
                                     [&](int i) { return status[(size_t)i] != DZG_RUNNING; });
}

// ---- duals of the LPs that ended OPTIMAL: one workgroup each, bucket by bucket
int duals_pass(Ctx &C)
{
    unsigned char *dev = C.D.arena;
    hipStream_t st = C.D.st;
    C.dhost.assign(C.duals_end - C.y, 0);
    const bh::StatusLists opt =
        bh::lists_by_status(C.stat(), C.lps, C.N, [](int s) { return s == DZG_OPTIMAL; });
    if (opt.list.empty()) return 0;
    DZG_HIP(hipMemcpyAsync(dev + C.dlist, opt.list.data(), sizeof(int) * opt.list.size(),
                           hipMemcpyHostToDevice, st));
    DzgDualsArgs a;
    a.lp = C.g.lp;
    a.A = C.g.A;
    a.var_col = C.g.var_col;
    a.basis = C.g.basis;
    a.nonbasis = C.g.nonbasis;
    a.x = C.g.x;
    a.z = C.g.z;
    a.c = (const double *)(dev + C.c);
    a.rhs0 = (const double *)(dev + C.x0);
    a.y = (double *)(dev + C.y);
    a.d = (double *)(dev + C.d);
    a.scal = (double *)(dev + C.scal);
    for (int b = 0; b < kBuckets; ++b) {
        const int cnt = opt.seg[(size_t)b + 1] - opt.seg[(size_t)b];
        if (cnt == 0) continue;
        a.mmax = C.P.mmax[b];
        dzg_launch_duals_small(b, a, (const int *)(dev + C.dlist) + opt.seg[(size_t)b], cnt, st);
        DZG_HIP(hipGetLastError());
    }
    DZG_HIP(hipMemcpyAsync(C.dhost.data(), dev + C.y, C.duals_end - C.y, hipMemcpyDeviceToHost, st));
    DZG_HIP(hipStreamSynchronize(st));
    return 0;
}

void write_duals(const Ctx &C, int i)
{
    dzg_duals &u = C.ex.du[i];
    const dzg_result &r = C.res[i];
    if (r.status != DZG_OPTIMAL) {
        dzg_duals_none(&u, r.objective);
        return;
    }
    const dzg_lp &lp = C.lps[i];
    const DzgBatchLp &d = C.P.desc[(size_t)i];
    const double *sc = (const double *)(C.dhost.data() + (C.scal - C.y)) + (size_t)DZG_DUALS_SCAL * i;
    u.reserved = 0;
    u.primal_obj = r.objective;
    u.source = DZG_DUALS_FRESH;
    u.dual_obj = sc[0];
    u.primal_infeas = sc[1];
    u.dual_infeas = sc[2];
    u.z_diff = sc[3] / std::max(1.0, sc[4]);
    if (u.y && lp.m) std::memcpy(u.y, (const double *)C.dhost.data() + d.m_off, sizeof(double) * (size_t)lp.m);
    if (u.d && lp.n)
        std::memcpy(u.d, (const double *)(C.dhost.data() + (C.d - C.y)) + d.vc_off, sizeof(double) * (size_t)lp.n);
}

// ---- rays of the LPs that ended UNBOUNDED or INFEASIBLE: one workgroup each, bucket by bucket, on
// the final state as it lies on the device (g.dz is the solve's scratch)
int rays_pass(Ctx &C)
{
    unsigned char *dev = C.D.arena;
    hipStream_t st = C.D.st;
    C.ryhost.assign(C.L.ar.top - C.rd, 0);
    const bh::StatusLists ends = bh::lists_by_status(
        C.stat(), C.lps, C.N, [](int s) { return s == DZG_UNBOUNDED || s == DZG_INFEASIBLE; });
    if (ends.list.empty()) return 0;
    DZG_HIP(hipMemcpyAsync(dev + C.rlist, ends.list.data(), sizeof(int) * ends.list.size(),
                           hipMemcpyHostToDevice, st));
    DzgRaysArgs a;
    a.lp = C.g.lp;
    a.A = C.g.A;
    a.var_col = C.g.var_col;
    a.basis = C.g.basis;
    a.nonbasis = C.g.nonbasis;
    a.x = C.g.x;
    a.xbar = C.g.xbar;
    a.z = C.g.z;
    a.zbar = C.g.zbar;
    a.status = C.g.status;
    a.c = (const double *)(dev + C.c);
    a.rhs0 = (const double *)(dev + C.x0);
    a.dz = C.g.dz;
    a.d = (double *)(dev + C.rd);
    a.y = (double *)(dev + C.ry);
    a.scal = (double *)(dev + C.rscal);
    for (int b = 0; b < kBuckets; ++b) {
        const int cnt = ends.seg[(size_t)b + 1] - ends.seg[(size_t)b];
        if (cnt == 0) continue;
        a.mmax = C.P.mmax[b];
        dzg_launch_rays_small(b, a, (const int *)(dev + C.rlist) + ends.seg[(size_t)b], cnt, st);
        DZG_HIP(hipGetLastError());
    }
    DZG_HIP(hipMemcpyAsync(C.ryhost.data(), dev + C.rd, C.ryhost.size(), hipMemcpyDeviceToHost, st));
    DZG_HIP(hipStreamSynchronize(st));
    return 0;
}

void write_ray(const Ctx &C, int i)
{
    dzg_ray &u = C.ex.ry[i];
    const dzg_result &r = C.res[i];
    const double *sc = (const double *)(C.ryhost.data() + (C.rscal - C.rd)) + (size_t)DZG_RAY_SCAL * i;
    if ((r.status != DZG_UNBOUNDED && r.status != DZG_INFEASIBLE) || sc[0] < 0.0) {
        dzg_ray_none(&u);
        return;
    }
    const dzg_lp &lp = C.lps[i];
    const DzgBatchLp &d = C.P.desc[(size_t)i];
    const bool primal = r.status == DZG_UNBOUNDED;
    u.kind = primal ? DZG_RAY_PRIMAL : DZG_RAY_FARKAS;
    u.var = (int64_t)sc[0];
    u.pos = (int64_t)sc[1];
    u.mu = sc[2];
    u.value = sc[3];
    u.violation = sc[4];
    u.proven = u.violation == 0.0 && (primal ? u.value > 0.0 : u.value < 0.0) ? 1 : 0;
    if (u.d && lp.n) std::memcpy(u.d, (const double *)C.ryhost.data() + d.vc_off, sizeof(double) * (size_t)lp.n);
    if (u.y && lp.m)
        std::memcpy(u.y, (const double *)(C.ryhost.data() + (C.ry - C.rd)) + d.m_off, sizeof(double) * (size_t)lp.m);
}

// ---- ranges of the LPs that ended OPTIMAL: one workgroup per (LP, direction), bucket by bucket, in
// an arena of their own; the fresh d of the duals pass is still on the device
int ranging_pass(Ctx &C)
{
    const int N = C.N;
    const dzg_ranging_req *req = C.ex.req;
    hipStream_t st = C.D.st;
    C.rg_out.assign((size_t)N + 1, 0);
    for (int i = 0; i < N; ++i) C.rg_out[(size_t)i + 1] = C.rg_out[(size_t)i] + req[i].ncost + req[i].nrhs;
    const size_t nout = (size_t)C.rg_out[(size_t)N];
    std::vector<int> e_idx;
    std::vector<double> e_val, tol((size_t)N, 0.0);
    std::vector<long long> e_base((size_t)N, 0); // LP i's entries: cost side, then rhs side
    for (int i = 0; i < N; ++i) {
        const dzg_ranging_req &rq = req[i];
        tol[(size_t)i] = rq.pivot_tol == 0.0 ? 1e-9 : rq.pivot_tol;
        e_base[(size_t)i] = (long long)e_idx.size();
        const int64_t ce = rq.ncost ? rq.cost_ptr[rq.ncost] : 0, re = rq.nrhs ? rq.rhs_ptr[rq.nrhs] : 0;
        e_idx.insert(e_idx.end(), rq.cost_idx, rq.cost_idx + ce);
        e_val.insert(e_val.end(), rq.cost_val, rq.cost_val + ce);
        e_idx.insert(e_idx.end(), rq.rhs_idx, rq.rhs_idx + re);
        e_val.insert(e_val.end(), rq.rhs_val, rq.rhs_val + re);
    }
    const bh::StatusLists opt =
        bh::lists_by_status(C.stat(), C.lps, N, [](int s) { return s == DZG_OPTIMAL; });
    std::vector<DzgRangeItem> items;
    bh::Segments iseg{};
    for (int b = 0; b < kBuckets; ++b) {
        for (int k = opt.seg[(size_t)b]; k < opt.seg[(size_t)b + 1]; ++k) {
            const int i = opt.list[(size_t)k];
            const dzg_ranging_req &rq = req[i];
            const long long cbase = e_base[(size_t)i], rbase = cbase + (rq.ncost ? rq.cost_ptr[rq.ncost] : 0);
            for (int64_t j = 0; j < rq.ncost; ++j)
                items.push_back({cbase + rq.cost_ptr[j], cbase + rq.cost_ptr[j + 1], C.rg_out[(size_t)i] + j, i, 1});
            for (int64_t j = 0; j < rq.nrhs; ++j)
                items.push_back({rbase + rq.rhs_ptr[j], rbase + rq.rhs_ptr[j + 1],
                                 C.rg_out[(size_t)i] + rq.ncost + j, i, 0});
        }
        if (items.size() >= ((size_t)1 << 31)) return dzg_set_error(DZG_E_ARG, "batch: too many directions");
        iseg[(size_t)b + 1] = (int)items.size();
    }
    if (items.empty()) return 0;
    bh::Arena ar;
    const size_t r_items = ar.add(sizeof(DzgRangeItem) * items.size()), r_eidx = ar.add(sizeof(int) * e_idx.size()),
                 r_eval = ar.add(sizeof(double) * e_val.size()), r_tol = ar.add(sizeof(double) * N);
    const size_t r_up = ar.top;
    C.r_lo = ar.add(sizeof(double) * nout);
    C.r_hi = ar.add(sizeof(double) * nout);
    C.r_lov = ar.add(sizeof(int) * nout);
    C.r_hiv = ar.add(sizeof(int) * nout);
    C.rhost.assign(ar.top, 0);
    std::memcpy(C.rhost.data() + r_items, items.data(), sizeof(DzgRangeItem) * items.size());
    if (!e_idx.empty()) {
        std::memcpy(C.rhost.data() + r_eidx, e_idx.data(), sizeof(int) * e_idx.size());
        std::memcpy(C.rhost.data() + r_eval, e_val.data(), sizeof(double) * e_val.size());
    }
    std::memcpy(C.rhost.data() + r_tol, tol.data(), sizeof(double) * N);
    DZG_HIP(hipMalloc((void **)&C.D.arena2, ar.top));
    unsigned char *rdev = C.D.arena2;
    DZG_HIP(hipMemcpyAsync(rdev, C.rhost.data(), r_up, hipMemcpyHostToDevice, st));
    DzgRangingArgs a;
    a.lp = C.g.lp;
    a.A = C.g.A;
    a.var_col = C.g.var_col;
    a.basis = C.g.basis;
    a.nonbasis = C.g.nonbasis;
    a.x = C.g.x;
    a.d = (const double *)(C.D.arena + C.d);
    a.tol = (const double *)(rdev + r_tol);
    a.item = (const DzgRangeItem *)(rdev + r_items);
    a.e_idx = (const int *)(rdev + r_eidx);
    a.e_val = (const double *)(rdev + r_eval);
    a.lo = (double *)(rdev + C.r_lo);
    a.hi = (double *)(rdev + C.r_hi);
    a.lo_var = (int *)(rdev + C.r_lov);
    a.hi_var = (int *)(rdev + C.r_hiv);
    for (int b = 0; b < kBuckets; ++b) {
        const int cnt = iseg[(size_t)b + 1] - iseg[(size_t)b];
        if (cnt == 0) continue;
        a.mmax = C.P.mmax[b];
        dzg_launch_ranging_small(b, a, a.item + iseg[(size_t)b], cnt, st);
        DZG_HIP(hipGetLastError());
    }
    DZG_HIP(hipMemcpyAsync(C.rhost.data() + C.r_lo, rdev + C.r_lo, ar.top - C.r_lo, hipMemcpyDeviceToHost, st));
    DZG_HIP(hipStreamSynchronize(st));
    return 0;
}

void write_ranging(const Ctx &C, int i)
{
    const dzg_ranging_req &rq = C.ex.req[i];
    dzg_ranging &o = C.ex.rg[i];
    if (C.res[i].status != DZG_OPTIMAL) {
        dzg_ranging_none(&rq, &o);
        return;
    }
    const size_t at = (size_t)C.rg_out[(size_t)i];
    const double *lo = (const double *)(C.rhost.data() + C.r_lo) + at;
    const double *hi = (const double *)(C.rhost.data() + C.r_hi) + at;
    const int *lov = (const int *)(C.rhost.data() + C.r_lov) + at;
    const int *hiv = (const int *)(C.rhost.data() + C.r_hiv) + at;
    for (int64_t j = 0; j < rq.ncost; ++j) {
        if (o.cost_lo) o.cost_lo[j] = lo[j];
        if (o.cost_hi) o.cost_hi[j] = hi[j];
        if (o.cost_lo_var) o.cost_lo_var[j] = lov[j];
        if (o.cost_hi_var) o.cost_hi_var[j] = hiv[j];
    }
    for (int64_t j = 0; j < rq.nrhs; ++j) {
        if (o.rhs_lo) o.rhs_lo[j] = lo[rq.ncost + j];
        if (o.rhs_hi) o.rhs_hi[j] = hi[rq.ncost + j];
        if (o.rhs_lo_var) o.rhs_lo_var[j] = lov[rq.ncost + j];
        if (o.rhs_hi_var) o.rhs_hi_var[j] = hiv[rq.ncost + j];
    }
}

void write_results(const Ctx &C)
{
    const bh::HostView view(C.host.data(), C.L);
    const long long *iters = (const long long *)(C.host.data() + C.iter);
    for (int i = 0; i < C.N; ++i) {
        dzg_result &r = C.res[i];
        dzg_steps::strict_unpack(C.lps[i], C.P.desc[(size_t)i], view, C.stat()[i], iters[i], r);
        if (C.ex.rays) write_ray(C, i);
        if (C.ex.ranging) write_ranging(C, i);
        if (C.ex.duals) write_duals(C, i);
    }
}

} // namespace

#define DZG_BATCH_DEFAULT_PPL 16

// ---- the steps of batch_steps.h
int dzg_steps::strict_ppl(int64_t pivots_per_launch)
{
    return (int)(pivots_per_launch > 0 ? std::min<int64_t>(pivots_per_launch, 1 << 30) : DZG_BATCH_DEFAULT_PPL);
}

int dzg_steps::strict_restart(const StrictRun &R, const int *wlist, const bh::Segments &wseg, const int *mmax)
{
    const BArgs g = strict_args(R);
    DzgBatchRestartArgs a;
    a.lp = g.lp;
    a.A = g.A;
    a.var_col = g.var_col;
    a.basis = g.basis;
    a.nonbasis = g.nonbasis;
    a.x = g.x;
    a.xbar = g.xbar;
    a.z = g.z;
    a.zbar = g.zbar;
    a.c = (const double *)(R.dev + R.c);
    a.status = g.status;
    for (int b = 0; b < kBuckets; ++b) {
        const int cnt = wseg[(size_t)b + 1] - wseg[(size_t)b];
        if (cnt == 0) continue;
        a.mmax = mmax[b];
        dzg_launch_batch_restart(b, a, wlist + wseg[(size_t)b], cnt, R.st);
        DZG_HIP(hipGetLastError());
    }
    return 0;
}

int dzg_steps::strict_rounds(const StrictRun &R, int *cur, int *nxt, const bh::Segments &seg,
                             const std::array<int, bh::kBuckets> &live, const int *mmax, int *rounds)
{
    const BArgs g = strict_args(R);
    return bh::run_rounds(cur, nxt, (int *)(R.dev + R.L->count), seg, live, R.st,
                          [&](int b, const int *list, int n, int *next_list, int *next_count) {
                              BArgs gb = g;
                              gb.mmax = mmax[b];
                              launch_bucket(b, gb, list, n, next_list, next_count, R.st);
                          }, rounds);
}

void dzg_steps::strict_unpack(const dzg_lp &lp, const DzgBatchLp &d, const bh::HostView &view, int status,
                              long long iter, dzg_result &r)
{
    r.status = status;
    r.numerics_used = DZG_NUMERICS_STRICT;
    r.iterations = iter;
    bh::unpack_common(lp, d, view, r);
}

// dzg_batch_solve and, behind the solve and on sections of their own (the solve's layout does not
// move), what `ex` asks for: the duals of the LPs that end OPTIMAL (k_duals.hip), their ranges
// (k_ranging.hip, which reads the duals' fresh d), the rays of the LPs that end UNBOUNDED or
// INFEASIBLE (k_rays.hip).
static int batch_solve(const dzg_lp *lps, int64_t count, const dzg_opts *opts, int64_t pivots_per_launch,
                       dzg_result *res, BatchExtras ex, const dzg_batch_start *start = nullptr)
{
    t_restart_ms = 0.0;
    std::vector<dzg_duals> du_own; // ranging needs the fresh d on the device; the caller may not want it
    if (ex.ranging && !ex.du && count > 0 && count < (1ll << 31)) {
        dzg_duals none;
        std::memset(&none, 0, sizeof(none));
        du_own.assign((size_t)count, none);
        ex.du = du_own.data();
    }
    // ---- host checks first: malformed input is DZG_E_ARG on any machine
    if (const int rc = bh::check_batch(lps, count, res, pivots_per_launch, ex.duals && !ex.du ? "du" : nullptr))
        return rc;
    if (count > 0 && ex.ranging && (!ex.req || !ex.rg)) return dzg_set_error(DZG_E_ARG, "batch: req or rg is NULL");
    if (count > 0 && ex.rays && !ex.ry) return dzg_set_error(DZG_E_ARG, "batch: ry is NULL");
    dzg_opts o;
    if (opts) o = *opts; else dzg_opts_default(&o);
    if (o.numerics != DZG_NUMERICS_STRICT && o.numerics != DZG_NUMERICS_AUTO)
        return dzg_set_error(DZG_E_ARG, "batch: STRICT numerics only (FAST is not batched)");
    const long long max_iter = dzg_opts_resolved(&o).max_iter;
    const int rc_lps = bh::check_batch(lps, count, [&](int64_t i, std::string &why) {
        if (start && !bh::start_valid(lps[i], start[i], why)) return false;
        return !ex.ranging || dzg_ranging_req_valid(&ex.req[i], lps[i].m, lps[i].n, why);
    });
    if (rc_lps) return rc_lps;
    if (count == 0) return 0;
    if (const int rc = bh::use_device(o.device)) return rc;

    Ctx C(lps, start, (int)count, res, ex, max_iter);
    C.R.max_iter = max_iter;
    C.R.eps = dzg_opts_resolved(&o).epsilon;
    C.R.ppl = dzg_steps::strict_ppl(pivots_per_launch);
    if (const int rc = pack_and_upload(C)) return rc;
    unsigned char *dev = C.D.arena;
    std::array<int, kBuckets> live = bh::live_of(C.P.bucket_n);
    if (C.warm)
        if (const int rc = restart_pass(C, live)) return rc;
    const int rc_rounds = dzg_steps::strict_rounds(C.R, (int *)(dev + C.L.list), (int *)(dev + C.L.list2),
                                                   bh::segments(C.P.bucket_n), live, C.P.mmax);
    if (rc_rounds) return rc_rounds;
    if (const int rc = bh::download(C.D, C.L, C.host.data())) return rc;
    if (ex.duals)
        if (const int rc = duals_pass(C)) return rc;
    if (ex.rays)
        if (const int rc = rays_pass(C)) return rc;
    if (ex.ranging)
        if (const int rc = ranging_pass(C)) return rc;
    write_results(C);
    return 0;
}

extern "C" int dzg_batch_solve(const dzg_lp *lps, int64_t count, const dzg_opts *opts,
                               int64_t pivots_per_launch, dzg_result *res)
{
    return batch_solve(lps, count, opts, pivots_per_launch, res, BatchExtras());
}

extern "C" int dzg_batch_solve_duals(const dzg_lp *lps, int64_t count, const dzg_opts *opts,
                                     int64_t pivots_per_launch, dzg_result *res, dzg_duals *du)
{
    BatchExtras ex;
    ex.duals = true;
    ex.du = du;
    return batch_solve(lps, count, opts, pivots_per_launch, res, ex);
}

extern "C" int dzg_batch_solve_ranging(const dzg_lp *lps, int64_t count, const dzg_opts *opts,
                                       int64_t pivots_per_launch, const dzg_ranging_req *req, dzg_result *res,
                                       dzg_duals *du, dzg_ranging *rg)
{
    BatchExtras ex;
    ex.duals = ex.ranging = true;
    ex.du = du;
    ex.req = req;
    ex.rg = rg;
    return batch_solve(lps, count, opts, pivots_per_launch, res, ex);
}

extern "C" int dzg_batch_solve_rays(const dzg_lp *lps, int64_t count, const dzg_opts *opts,
                                    int64_t pivots_per_launch, dzg_result *res, dzg_duals *du, dzg_ray *ry)
{
    if (count > 0 && !ry) return dzg_set_error(DZG_E_ARG, "batch: ry is NULL");
    BatchExtras ex;
    ex.duals = du != nullptr;
    ex.rays = true;
    ex.du = du;
    ex.ry = ry;
    return batch_solve(lps, count, opts, pivots_per_launch, res, ex);
}

extern "C" int dzg_batch_solve_from(const dzg_lp *lps, const dzg_batch_start *start, int64_t count,
                                    const dzg_opts *opts, int64_t pivots_per_launch, dzg_result *res,
                                    dzg_duals *du)
{
    BatchExtras ex;
    ex.duals = du != nullptr;
    ex.du = du;
    return batch_solve(lps, count, opts, pivots_per_launch, res, ex, start);
}

int dzg_steps::strict_post(const dzg_lp *lps, const dzg_batch_start *start, int64_t count, const dzg_opts *opts,
                           int64_t pivots_per_launch, dzg_result *res, dzg_duals *du, const dzg_ranging_req *req,
                           dzg_ranging *rg, dzg_ray *ry)
{
    BatchExtras ex;
    ex.ranging = req != nullptr;
    ex.duals = du != nullptr || ex.ranging;
    ex.rays = ry != nullptr;
    ex.du = du;
    ex.req = req;
    ex.rg = rg;
    ex.ry = ry;
    return batch_solve(lps, count, opts, pivots_per_launch, res, ex, start);
}

extern "C" double dzg_debug_batch_restart_ms(void) { return t_restart_ms; }
