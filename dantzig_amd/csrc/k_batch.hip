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

#include "batch_strict.h"
#include "common.h"
#include "duals.h"
#include "ranging.h"
#include "rays.h"

int dzg_set_error(int code, const std::string &msg); // engine.hip
int dzg_lp_valid(const dzg_lp *lp, std::string &why);

namespace {

// One LP of the batch: sizes and its offsets into the packed arrays (elements, not bytes).
struct BLp {
    long long a_off;   // A: m x ns column-major, lda = m
    long long vc_off;  // var_col: n
    long long m_off;   // basis, x, xbar: m
    long long q_off;   // nonbasis, z, zbar, dz: n - m
    long long log_off; // pivot log: log_cap
    long long log_cap;
    int m, n, ns, pad;
};

struct BArgs {
    const BLp *lp;
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
    const BLp L = g.lp[id];
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

using dzg_bs::bucket_of;
using dzg_bs::kBucketRows;
using dzg_bs::kBuckets;
using dzg_bs::kMaxGrid;
using dzg_bs::lds_bytes;

void launch_bucket(int b, const BArgs &g, const int *list, int n, int *next_list, int *next_count,
                   hipStream_t st)
{
    const size_t lds = lds_bytes(g.mmax);
    for (int c0 = 0; c0 < n; c0 += kMaxGrid[b]) {
        const int grid = std::min(kMaxGrid[b], n - c0);
        // one wave per LP up to 32 rows (no barrier has a second wave to wait for), then 2 and 4
        if (b <= 1)
            hipLaunchKernelGGL(k_batch_strict<64>, dim3(grid), dim3(64), lds, st, g, list + c0,
                               next_list, next_count);
        else if (b == 2)
            hipLaunchKernelGGL(k_batch_strict<128>, dim3(grid), dim3(128), lds, st, g, list + c0,
                               next_list, next_count);
        else
            hipLaunchKernelGGL(k_batch_strict<256>, dim3(grid), dim3(256), lds, st, g, list + c0,
                               next_list, next_count);
    }
}

#define BHIP(expr)                                                                              \
    do {                                                                                        \
        hipError_t e_ = (expr);                                                                 \
        if (e_ != hipSuccess)                                                                   \
            return dzg_set_error(DZG_E_DEVICE, std::string(#expr) + ": " + hipGetErrorString(e_)); \
    } while (0)

struct Section {
    size_t off = 0, bytes = 0;
};

} // namespace

#define DZG_BATCH_DEFAULT_PPL 16

// dzg_batch_solve; with `du` the duals of the LPs that end OPTIMAL follow in the same allocation
// (k_duals.hip), after the solve and on sections of their own: the solve's layout does not move
// With `req` / `rg` the ranges of the OPTIMAL LPs follow the duals (k_ranging.hip), in an allocation
// of their own.  With `ry` the rays of the LPs that end UNBOUNDED or INFEASIBLE follow (k_rays.hip), on
// sections behind those of the duals.
static int batch_solve(const dzg_lp *lps, int64_t count, const dzg_opts *opts, int64_t pivots_per_launch,
                       dzg_result *res, dzg_duals *du, bool want_duals, const dzg_ranging_req *req = nullptr,
                       dzg_ranging *rg = nullptr, bool want_ranging = false, dzg_ray *ry = nullptr,
                       bool want_rays = false)
{
    std::vector<dzg_duals> du_own; // ranging needs the fresh d on the device; the caller may not want it
    if (want_ranging && !du && count > 0 && count < (1ll << 31)) {
        dzg_duals none;
        std::memset(&none, 0, sizeof(none));
        du_own.assign((size_t)count, none);
        du = du_own.data();
    }
    // ---- host checks first: malformed input is DZG_E_ARG on any machine
    if (count < 0) return dzg_set_error(DZG_E_ARG, "batch: count < 0");
    if (count > 0 && (!lps || !res)) return dzg_set_error(DZG_E_ARG, "batch: lps or res is NULL");
    if (count > 0 && want_duals && !du) return dzg_set_error(DZG_E_ARG, "batch: du is NULL");
    if (count >= (1ll << 31)) return dzg_set_error(DZG_E_ARG, "batch: count out of range");
    if (pivots_per_launch < 0) return dzg_set_error(DZG_E_ARG, "batch: pivots_per_launch < 0");
    if (count > 0 && want_ranging && (!req || !rg)) return dzg_set_error(DZG_E_ARG, "batch: req or rg is NULL");
    if (count > 0 && want_rays && !ry) return dzg_set_error(DZG_E_ARG, "batch: ry is NULL");
    dzg_opts o;
    if (opts) o = *opts; else dzg_opts_default(&o);
    if (o.numerics != DZG_NUMERICS_STRICT && o.numerics != DZG_NUMERICS_AUTO)
        return dzg_set_error(DZG_E_ARG, "batch: STRICT numerics only (FAST is not batched)");
    const long long max_iter = o.max_iter > 0 ? o.max_iter : 10000000;
    const double eps = o.epsilon != 0.0 ? o.epsilon : 1e-12;
    const int ppl = (int)(pivots_per_launch > 0 ? std::min<int64_t>(pivots_per_launch, 1 << 30)
                                                : DZG_BATCH_DEFAULT_PPL);
    for (int64_t i = 0; i < count; ++i) {
        const dzg_lp *lp = &lps[i];
        std::string why;
        const std::string at = "batch: lps[" + std::to_string(i) + "]: ";
        if (!dzg_lp_valid(lp, why)) return dzg_set_error(DZG_E_ARG, at + why);
        if (lp->m > DZG_BATCH_MAX_ROWS)
            return dzg_set_error(DZG_E_ARG, at + "m > DZG_BATCH_MAX_ROWS (" +
                                                std::to_string(DZG_BATCH_MAX_ROWS) + ")");
        if (lp->n_struct > 0 && !lp->a) return dzg_set_error(DZG_E_ARG, at + "CSC input is not batched");
        if (lp->n - lp->m > (1ll << 30)) return dzg_set_error(DZG_E_ARG, at + "too many columns");
        if (want_ranging && !dzg_ranging_req_valid(&req[i], lp->m, lp->n, why))
            return dzg_set_error(DZG_E_ARG, at + why);
    }
    if (count == 0) return 0;
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || ndev <= 0)
        return dzg_set_error(DZG_E_DEVICE, "no HIP device visible: dantzig_amd has no CPU path");
    if (o.device < 0 || o.device >= ndev) return dzg_set_error(DZG_E_ARG, "opts.device out of range");
    BHIP(hipSetDevice(o.device));

    // ---- packed layout: one arena, sections 16-B aligned
    const int N = (int)count;
    std::vector<BLp> desc((size_t)N);
    long long na = 0, nvc = 0, nm = 0, nq = 0, nlog = 0;
    int mmax[kBuckets] = {0, 0, 0, 0};
    std::vector<int> bucket_n(kBuckets, 0);
    for (int i = 0; i < N; ++i) {
        const dzg_lp &lp = lps[i];
        BLp &d = desc[(size_t)i];
        d.m = (int)lp.m;
        d.n = (int)lp.n;
        d.ns = (int)lp.n_struct;
        d.pad = 0;
        d.a_off = na;
        d.vc_off = nvc;
        d.m_off = nm;
        d.q_off = nq;
        d.log_off = nlog;
        d.log_cap = res[i].log && res[i].log_cap > 0 ? std::min<long long>(res[i].log_cap, max_iter) : 0;
        na += (long long)lp.m * lp.n_struct;
        nvc += lp.n;
        nm += lp.m;
        nq += lp.n - lp.m;
        nlog += d.log_cap;
        const int b = bucket_of(lp.m);
        mmax[b] = std::max(mmax[b], (int)lp.m);
        bucket_n[(size_t)b]++;
    }
    size_t top = 0;
    auto section = [&](size_t bytes) {
        Section s;
        s.off = top;
        s.bytes = bytes;
        top += (bytes + 15) / 16 * 16;
        return s;
    };
    // upload-only, then state (uploaded and downloaded), then log (downloaded), then scratch
    const Section s_desc = section(sizeof(BLp) * N), s_a = section(sizeof(double) * na),
                  s_vc = section(sizeof(int) * nvc), s_list = section(sizeof(int) * N);
    const size_t state0 = top;
    const Section s_basis = section(sizeof(int) * nm), s_nonbasis = section(sizeof(int) * nq),
                  s_x = section(sizeof(double) * nm), s_xbar = section(sizeof(double) * nm),
                  s_z = section(sizeof(double) * nq), s_zbar = section(sizeof(double) * nq),
                  s_status = section(sizeof(int) * N), s_iter = section(sizeof(long long) * N);
    const size_t upload_end = top;
    const Section s_lk = section(sizeof(int) * nlog), s_le = section(sizeof(int) * nlog),
                  s_ll = section(sizeof(int) * nlog), s_lmu = section(sizeof(double) * nlog);
    const size_t download_end = top;
    const Section s_dz = section(sizeof(double) * nq), s_list2 = section(sizeof(int) * N),
                  s_count = section(sizeof(int) * kBuckets);
    // duals: c and the starting x go up, the OPTIMAL LPs' list goes up after the solve, y, d and the
    // scalars come down
    // (the rays read the same descriptors, c and starting x)
    Section s_dlp, s_c, s_x0, s_dlist, s_y, s_d, s_scal;
    if (want_duals || want_rays) {
        s_dlp = section(sizeof(DzgDualsLp) * N);
        s_c = section(sizeof(double) * nvc);
        s_x0 = section(sizeof(double) * nm);
        s_dlist = section(sizeof(int) * N);
        s_y = section(sizeof(double) * nm);
        s_d = section(sizeof(double) * nvc);
        s_scal = section(sizeof(double) * DZG_DUALS_SCAL * N);
    }
    const size_t duals_end = top;
    // rays: the list of the LPs that ended UNBOUNDED or INFEASIBLE goes up after the solve, d, y and the
    // scalars come down
    Section s_rlist, s_rd, s_ry, s_rscal;
    if (want_rays) {
        s_rlist = section(sizeof(int) * N);
        s_rd = section(sizeof(double) * nvc);
        s_ry = section(sizeof(double) * nm);
        s_rscal = section(sizeof(double) * DZG_RAY_SCAL * N);
    }

    std::vector<unsigned char> host(download_end, 0);
    auto hp = [&](const Section &s) { return host.data() + s.off; };
    std::memcpy(hp(s_desc), desc.data(), sizeof(BLp) * N);
    {
        double *a = (double *)hp(s_a);
        int *vc = (int *)hp(s_vc), *bs = (int *)hp(s_basis), *nb = (int *)hp(s_nonbasis);
        double *x = (double *)hp(s_x), *xb = (double *)hp(s_xbar), *z = (double *)hp(s_z),
               *zb = (double *)hp(s_zbar);
        int *st = (int *)hp(s_status);
        for (int i = 0; i < N; ++i) {
            const dzg_lp &lp = lps[i];
            const BLp &d = desc[(size_t)i];
            const int64_t m = lp.m, q = lp.n - lp.m;
            for (int64_t j = 0; j < lp.n_struct; ++j)
                std::memcpy(a + d.a_off + j * m, lp.a + j * lp.lda, sizeof(double) * (size_t)m);
            for (int64_t v = 0; v < lp.n; ++v)
                vc[d.vc_off + v] = lp.var_col ? (int)lp.var_col[v]
                                              : (v < lp.n_struct ? (int)v : (int)(-1 - (v - lp.n_struct)));
            for (int64_t k = 0; k < m; ++k) {
                bs[d.m_off + k] = (int)lp.basis[k];
                x[d.m_off + k] = lp.x[k];
                xb[d.m_off + k] = lp.xbar ? lp.xbar[k] : 1.0; // Simplex::new, src/simplex.rs:219-220
            }
            for (int64_t k = 0; k < q; ++k) {
                nb[d.q_off + k] = (int)lp.nonbasis[k];
                z[d.q_off + k] = lp.z[k];
                zb[d.q_off + k] = lp.zbar ? lp.zbar[k] : 1.0;
            }
            st[i] = DZG_RUNNING;
        }
        // the first round's lists: LP indices grouped by bucket
        int *list = (int *)hp(s_list);
        std::vector<int> fill(kBuckets, 0);
        for (int b = 1; b < kBuckets; ++b) fill[(size_t)b] = fill[(size_t)b - 1] + bucket_n[(size_t)b - 1];
        for (int i = 0; i < N; ++i) list[fill[(size_t)bucket_of(lps[i].m)]++] = i;
    }

    unsigned char *dev = nullptr;
    hipStream_t st = nullptr;
    unsigned char *rdev = nullptr; // the ranging pass's arena
    struct Guard {
        unsigned char **dev, **rdev;
        hipStream_t *st;
        ~Guard()
        {
            if (*dev) (void)hipFree(*dev);
            if (*rdev) (void)hipFree(*rdev);
            if (*st) (void)hipStreamDestroy(*st);
        }
    } guard{&dev, &rdev, &st};
    BHIP(hipStreamCreateWithFlags(&st, hipStreamNonBlocking));
    BHIP(hipMalloc((void **)&dev, top));
    BHIP(hipMemcpyAsync(dev, host.data(), upload_end, hipMemcpyHostToDevice, st));
    std::vector<unsigned char> dhost; // s_dlp .. s_x0 as uploaded, then s_y .. s_scal as downloaded
    if (want_duals || want_rays) {
        dhost.assign(duals_end - s_dlp.off, 0);
        DzgDualsLp *dl = (DzgDualsLp *)dhost.data();
        double *cc = (double *)(dhost.data() + (s_c.off - s_dlp.off));
        double *x0 = (double *)(dhost.data() + (s_x0.off - s_dlp.off));
        for (int i = 0; i < N; ++i) {
            const dzg_lp &lp = lps[i];
            const BLp &d = desc[(size_t)i];
            dl[i].a_off = d.a_off;
            dl[i].vc_off = d.vc_off;
            dl[i].m_off = d.m_off;
            dl[i].q_off = d.q_off;
            dl[i].constant = lp.constant;
            dl[i].m = d.m;
            dl[i].n = d.n;
            for (int64_t v = 0; v < lp.n; ++v) cc[d.vc_off + v] = lp.c[v];
            for (int64_t k = 0; k < lp.m; ++k) x0[d.m_off + k] = lp.x[k];
        }
        BHIP(hipMemcpyAsync(dev + s_dlp.off, dhost.data(), s_dlist.off - s_dlp.off, hipMemcpyHostToDevice,
                            st));
    }

    BArgs g;
    g.lp = (const BLp *)(dev + s_desc.off);
    g.A = (const double *)(dev + s_a.off);
    g.var_col = (const int *)(dev + s_vc.off);
    g.basis = (int *)(dev + s_basis.off);
    g.nonbasis = (int *)(dev + s_nonbasis.off);
    g.x = (double *)(dev + s_x.off);
    g.xbar = (double *)(dev + s_xbar.off);
    g.z = (double *)(dev + s_z.off);
    g.zbar = (double *)(dev + s_zbar.off);
    g.dz = (double *)(dev + s_dz.off);
    g.status = (int *)(dev + s_status.off);
    g.iter = (long long *)(dev + s_iter.off);
    g.log_kind = (int *)(dev + s_lk.off);
    g.log_enter = (int *)(dev + s_le.off);
    g.log_leave = (int *)(dev + s_ll.off);
    g.log_mu = (double *)(dev + s_lmu.off);
    g.max_iter = max_iter;
    g.eps = eps;
    g.ppl = ppl;

    // ---- rounds: every bucket's running LPs, then one readback of the bucket counters
    int *cur = (int *)(dev + s_list.off), *nxt = (int *)(dev + s_list2.off);
    int *counts = (int *)(dev + s_count.off);
    std::vector<int> seg(kBuckets, 0);
    for (int b = 1; b < kBuckets; ++b) seg[(size_t)b] = seg[(size_t)b - 1] + bucket_n[(size_t)b - 1];
    std::vector<int> live(bucket_n);
    for (;;) {
        bool any = false;
        BHIP(hipMemsetAsync(counts, 0, sizeof(int) * kBuckets, st));
        for (int b = 0; b < kBuckets; ++b) {
            if (live[(size_t)b] == 0) continue;
            any = true;
            BArgs gb = g;
            gb.mmax = mmax[b];
            launch_bucket(b, gb, cur + seg[(size_t)b], live[(size_t)b], nxt + seg[(size_t)b],
                          counts + b, st);
            BHIP(hipGetLastError());
        }
        if (!any) break;
        int h_counts[kBuckets];
        BHIP(hipMemcpyAsync(h_counts, counts, sizeof(h_counts), hipMemcpyDeviceToHost, st));
        BHIP(hipStreamSynchronize(st));
        for (int b = 0; b < kBuckets; ++b) live[(size_t)b] = h_counts[b];
        std::swap(cur, nxt);
    }
    BHIP(hipMemcpyAsync(host.data() + state0, dev + state0, download_end - state0,
                        hipMemcpyDeviceToHost, st));
    BHIP(hipStreamSynchronize(st));

    // ---- duals of the LPs that ended OPTIMAL: one workgroup each, bucket by bucket
    if (want_duals) {
        const int *stat = (const int *)hp(s_status);
        std::vector<int> dlist;
        std::vector<int> dseg(kBuckets + 1, 0);
        for (int b = 0; b < kBuckets; ++b) {
            for (int i = 0; i < N; ++i)
                if (stat[i] == DZG_OPTIMAL && bucket_of(lps[i].m) == b) dlist.push_back(i);
            dseg[(size_t)b + 1] = (int)dlist.size();
        }
        if (!dlist.empty()) {
            BHIP(hipMemcpyAsync(dev + s_dlist.off, dlist.data(), sizeof(int) * dlist.size(),
                                hipMemcpyHostToDevice, st));
            DzgDualsArgs a;
            a.lp = (const DzgDualsLp *)(dev + s_dlp.off);
            a.A = g.A;
            a.var_col = g.var_col;
            a.basis = g.basis;
            a.nonbasis = g.nonbasis;
            a.x = g.x;
            a.z = g.z;
            a.c = (const double *)(dev + s_c.off);
            a.rhs0 = (const double *)(dev + s_x0.off);
            a.y = (double *)(dev + s_y.off);
            a.d = (double *)(dev + s_d.off);
            a.scal = (double *)(dev + s_scal.off);
            for (int b = 0; b < kBuckets; ++b) {
                const int cnt = dseg[(size_t)b + 1] - dseg[(size_t)b];
                if (cnt == 0) continue;
                a.mmax = mmax[b];
                dzg_launch_duals_small(b, a, (const int *)(dev + s_dlist.off) + dseg[(size_t)b], cnt, st);
                BHIP(hipGetLastError());
            }
            BHIP(hipMemcpyAsync(dhost.data() + (s_y.off - s_dlp.off), dev + s_y.off, duals_end - s_y.off,
                                hipMemcpyDeviceToHost, st));
            BHIP(hipStreamSynchronize(st));
        }
    }

    // ---- rays of the LPs that ended UNBOUNDED or INFEASIBLE: one workgroup each, bucket by bucket, on
    // the final state as it lies on the device (g.dz is the solve's scratch)
    std::vector<unsigned char> ryhost; // s_rd .. s_rscal as downloaded
    if (want_rays) {
        const int *stat = (const int *)hp(s_status);
        std::vector<int> rlist;
        std::vector<int> rseg(kBuckets + 1, 0);
        for (int b = 0; b < kBuckets; ++b) {
            for (int i = 0; i < N; ++i)
                if ((stat[i] == DZG_UNBOUNDED || stat[i] == DZG_INFEASIBLE) && bucket_of(lps[i].m) == b)
                    rlist.push_back(i);
            rseg[(size_t)b + 1] = (int)rlist.size();
        }
        ryhost.assign(top - s_rd.off, 0);
        if (!rlist.empty()) {
            BHIP(hipMemcpyAsync(dev + s_rlist.off, rlist.data(), sizeof(int) * rlist.size(),
                                hipMemcpyHostToDevice, st));
            DzgRaysArgs a;
            a.lp = (const DzgDualsLp *)(dev + s_dlp.off);
            a.A = g.A;
            a.var_col = g.var_col;
            a.basis = g.basis;
            a.nonbasis = g.nonbasis;
            a.x = g.x;
            a.xbar = g.xbar;
            a.z = g.z;
            a.zbar = g.zbar;
            a.status = g.status;
            a.c = (const double *)(dev + s_c.off);
            a.rhs0 = (const double *)(dev + s_x0.off);
            a.dz = g.dz;
            a.d = (double *)(dev + s_rd.off);
            a.y = (double *)(dev + s_ry.off);
            a.scal = (double *)(dev + s_rscal.off);
            for (int b = 0; b < kBuckets; ++b) {
                const int cnt = rseg[(size_t)b + 1] - rseg[(size_t)b];
                if (cnt == 0) continue;
                a.mmax = mmax[b];
                dzg_launch_rays_small(b, a, (const int *)(dev + s_rlist.off) + rseg[(size_t)b], cnt, st);
                BHIP(hipGetLastError());
            }
            BHIP(hipMemcpyAsync(ryhost.data(), dev + s_rd.off, top - s_rd.off, hipMemcpyDeviceToHost, st));
            BHIP(hipStreamSynchronize(st));
        }
    }

    // ---- ranges of the LPs that ended OPTIMAL: one workgroup per (LP, direction), bucket by bucket;
    // the fresh d of the duals pass is still on the device
    std::vector<unsigned char> rhost;
    std::vector<long long> rg_out((size_t)N + 1, 0); // LP i's results: rg_out[i] .. , cost directions first
    size_t r_lo = 0, r_hi = 0, r_lov = 0, r_hiv = 0;
    if (want_ranging) {
        const int *stat = (const int *)hp(s_status);
        for (int i = 0; i < N; ++i) rg_out[(size_t)i + 1] = rg_out[(size_t)i] + req[i].ncost + req[i].nrhs;
        const long long nout = rg_out[(size_t)N];
        std::vector<DzgRangeItem> items;
        std::vector<int> e_idx;
        std::vector<double> e_val, tol((size_t)N, 0.0);
        std::vector<int> iseg(kBuckets + 1, 0);
        std::vector<long long> e_base((size_t)N + 1, 0); // LP i's entries: cost side, then rhs side
        for (int i = 0; i < N; ++i) {
            const dzg_ranging_req &rq = req[i];
            tol[(size_t)i] = rq.pivot_tol == 0.0 ? 1e-9 : rq.pivot_tol;
            e_base[(size_t)i] = (long long)e_idx.size();
            const int64_t ce = rq.ncost ? rq.cost_ptr[rq.ncost] : 0, re = rq.nrhs ? rq.rhs_ptr[rq.nrhs] : 0;
            for (int64_t e = 0; e < ce; ++e) {
                e_idx.push_back((int)rq.cost_idx[e]);
                e_val.push_back(rq.cost_val[e]);
            }
            for (int64_t e = 0; e < re; ++e) {
                e_idx.push_back((int)rq.rhs_idx[e]);
                e_val.push_back(rq.rhs_val[e]);
            }
        }
        for (int b = 0; b < kBuckets; ++b) {
            for (int i = 0; i < N; ++i) {
                if (stat[i] != DZG_OPTIMAL || bucket_of(lps[i].m) != b) continue;
                const dzg_ranging_req &rq = req[i];
                const long long cbase = e_base[(size_t)i], rbase = cbase + (rq.ncost ? rq.cost_ptr[rq.ncost] : 0);
                for (int64_t j = 0; j < rq.ncost; ++j) {
                    DzgRangeItem it;
                    it.e0 = cbase + rq.cost_ptr[j];
                    it.e1 = cbase + rq.cost_ptr[j + 1];
                    it.out = rg_out[(size_t)i] + j;
                    it.lp = i;
                    it.kind = 1;
                    items.push_back(it);
                }
                for (int64_t j = 0; j < rq.nrhs; ++j) {
                    DzgRangeItem it;
                    it.e0 = rbase + rq.rhs_ptr[j];
                    it.e1 = rbase + rq.rhs_ptr[j + 1];
                    it.out = rg_out[(size_t)i] + rq.ncost + j;
                    it.lp = i;
                    it.kind = 0;
                    items.push_back(it);
                }
            }
            if (items.size() >= ((size_t)1 << 31)) return dzg_set_error(DZG_E_ARG, "batch: too many directions");
            iseg[(size_t)b + 1] = (int)items.size();
        }
        if (!items.empty()) {
            size_t rtop = 0;
            auto rsection = [&](size_t bytes) {
                const size_t off = rtop;
                rtop += (bytes + 15) / 16 * 16;
                return off;
            };
            const size_t r_items = rsection(sizeof(DzgRangeItem) * items.size()),
                         r_eidx = rsection(sizeof(int) * e_idx.size()),
                         r_eval = rsection(sizeof(double) * e_val.size()), r_tol = rsection(sizeof(double) * N);
            const size_t r_up = rtop;
            r_lo = rsection(sizeof(double) * (size_t)nout);
            r_hi = rsection(sizeof(double) * (size_t)nout);
            r_lov = rsection(sizeof(int) * (size_t)nout);
            r_hiv = rsection(sizeof(int) * (size_t)nout);
            rhost.assign(rtop, 0);
            std::memcpy(rhost.data() + r_items, items.data(), sizeof(DzgRangeItem) * items.size());
            if (!e_idx.empty()) {
                std::memcpy(rhost.data() + r_eidx, e_idx.data(), sizeof(int) * e_idx.size());
                std::memcpy(rhost.data() + r_eval, e_val.data(), sizeof(double) * e_val.size());
            }
            std::memcpy(rhost.data() + r_tol, tol.data(), sizeof(double) * N);
            BHIP(hipMalloc((void **)&rdev, rtop));
            BHIP(hipMemcpyAsync(rdev, rhost.data(), r_up, hipMemcpyHostToDevice, st));
            DzgRangingArgs a;
            a.lp = (const DzgDualsLp *)(dev + s_dlp.off);
            a.A = g.A;
            a.var_col = g.var_col;
            a.basis = g.basis;
            a.nonbasis = g.nonbasis;
            a.x = g.x;
            a.d = (const double *)(dev + s_d.off);
            a.tol = (const double *)(rdev + r_tol);
            a.item = (const DzgRangeItem *)(rdev + r_items);
            a.e_idx = (const int *)(rdev + r_eidx);
            a.e_val = (const double *)(rdev + r_eval);
            a.lo = (double *)(rdev + r_lo);
            a.hi = (double *)(rdev + r_hi);
            a.lo_var = (int *)(rdev + r_lov);
            a.hi_var = (int *)(rdev + r_hiv);
            for (int b = 0; b < kBuckets; ++b) {
                const int cnt = iseg[(size_t)b + 1] - iseg[(size_t)b];
                if (cnt == 0) continue;
                a.mmax = mmax[b];
                dzg_launch_ranging_small(b, a, a.item + iseg[(size_t)b], cnt, st);
                BHIP(hipGetLastError());
            }
            BHIP(hipMemcpyAsync(rhost.data() + r_lo, rdev + r_lo, rtop - r_lo, hipMemcpyDeviceToHost, st));
            BHIP(hipStreamSynchronize(st));
        }
    }

    // ---- results
    const int *bs = (const int *)hp(s_basis), *nb = (const int *)hp(s_nonbasis);
    const double *x = (const double *)hp(s_x), *xb = (const double *)hp(s_xbar),
                 *z = (const double *)hp(s_z), *zb = (const double *)hp(s_zbar);
    const int *stat = (const int *)hp(s_status);
    const long long *iters = (const long long *)hp(s_iter);
    const int *lk = (const int *)hp(s_lk), *le = (const int *)hp(s_le), *ll = (const int *)hp(s_ll);
    const double *lmu = (const double *)hp(s_lmu);
    for (int i = 0; i < N; ++i) {
        const dzg_lp &lp = lps[i];
        const BLp &d = desc[(size_t)i];
        dzg_result &r = res[i];
        const int64_t m = lp.m, q = lp.n - lp.m;
        r.status = stat[i];
        r.numerics_used = DZG_NUMERICS_STRICT;
        r.iterations = iters[i];
        double sum = 0.0; // objective_value, src/simplex.rs:345-352, basis-position order
        for (int64_t p = 0; p < m; ++p) {
            const double prod = lp.c[bs[d.m_off + p]] * x[d.m_off + p];
            sum = sum + prod;
        }
        r.objective = lp.constant + sum;
        for (int64_t k = 0; k < m; ++k) {
            if (r.basis) r.basis[k] = bs[d.m_off + k];
            if (r.x) r.x[k] = x[d.m_off + k];
            if (r.xbar) r.xbar[k] = xb[d.m_off + k];
        }
        for (int64_t k = 0; k < q; ++k) {
            if (r.nonbasis) r.nonbasis[k] = nb[d.q_off + k];
            if (r.z) r.z[k] = z[d.q_off + k];
            if (r.zbar) r.zbar[k] = zb[d.q_off + k];
        }
        const long long cnt = std::min<long long>(r.iterations, d.log_cap);
        for (long long k = 0; k < cnt; ++k) {
            r.log[k].kind = lk[d.log_off + k];
            r.log[k].reserved = 0;
            r.log[k].entering = le[d.log_off + k];
            r.log[k].leaving = ll[d.log_off + k];
            r.log[k].mu = lmu[d.log_off + k];
        }
        for (int c = 0; c < DZG_K_COUNT; ++c) {
            r.kernel_ms[c] = 0.0;
            r.kernel_launches[c] = 0;
        }
        r.price_bytes = 0.0;
        r.solve_ms = 0.0;
        r.max_pivot_error = 0.0;
        r.near_ties = 0;
        r.first_near_tie = -1;
        r.min_margin = __builtin_inf();
        r.dense_columns = 0;
        r.refactors = 0;
        r.chain_fallbacks = 0;
        r.price_pass_used = 0;
        r.price_rows_copy = 0;
        r.state_drift = 0.0;
        if (want_rays) {
            dzg_ray &u = ry[i];
            const double *sc = (const double *)(ryhost.data() + (s_rscal.off - s_rd.off)) + (size_t)DZG_RAY_SCAL * i;
            if ((r.status != DZG_UNBOUNDED && r.status != DZG_INFEASIBLE) || sc[0] < 0.0) {
                dzg_ray_none(&u);
            } else {
                const bool primal = r.status == DZG_UNBOUNDED;
                u.kind = primal ? DZG_RAY_PRIMAL : DZG_RAY_FARKAS;
                u.var = (int64_t)sc[0];
                u.pos = (int64_t)sc[1];
                u.mu = sc[2];
                u.value = sc[3];
                u.violation = sc[4];
                u.proven = u.violation == 0.0 && (primal ? u.value > 0.0 : u.value < 0.0) ? 1 : 0;
                if (u.d && lp.n)
                    std::memcpy(u.d, (const double *)ryhost.data() + d.vc_off, sizeof(double) * (size_t)lp.n);
                if (u.y && m)
                    std::memcpy(u.y, (const double *)(ryhost.data() + (s_ry.off - s_rd.off)) + d.m_off,
                                sizeof(double) * (size_t)m);
            }
        }
        if (want_ranging) {
            if (r.status != DZG_OPTIMAL) {
                dzg_ranging_none(&req[i], &rg[i]);
            } else {
                const dzg_ranging_req &rq = req[i];
                const dzg_ranging &o_ = rg[i];
                const double *lo = (const double *)(rhost.data() + r_lo) + rg_out[(size_t)i];
                const double *hi = (const double *)(rhost.data() + r_hi) + rg_out[(size_t)i];
                const int *lov = (const int *)(rhost.data() + r_lov) + rg_out[(size_t)i];
                const int *hiv = (const int *)(rhost.data() + r_hiv) + rg_out[(size_t)i];
                for (int64_t j = 0; j < rq.ncost; ++j) {
                    if (o_.cost_lo) o_.cost_lo[j] = lo[j];
                    if (o_.cost_hi) o_.cost_hi[j] = hi[j];
                    if (o_.cost_lo_var) o_.cost_lo_var[j] = lov[j];
                    if (o_.cost_hi_var) o_.cost_hi_var[j] = hiv[j];
                }
                for (int64_t j = 0; j < rq.nrhs; ++j) {
                    if (o_.rhs_lo) o_.rhs_lo[j] = lo[rq.ncost + j];
                    if (o_.rhs_hi) o_.rhs_hi[j] = hi[rq.ncost + j];
                    if (o_.rhs_lo_var) o_.rhs_lo_var[j] = lov[rq.ncost + j];
                    if (o_.rhs_hi_var) o_.rhs_hi_var[j] = hiv[rq.ncost + j];
                }
            }
        }
        if (want_duals) {
            dzg_duals &u = du[i];
            if (r.status != DZG_OPTIMAL) {
                dzg_duals_none(&u, r.objective);
                continue;
            }
            u.reserved = 0;
            u.primal_obj = r.objective;
            const double *yv = (const double *)(dhost.data() + (s_y.off - s_dlp.off)) + d.m_off;
            const double *dv = (const double *)(dhost.data() + (s_d.off - s_dlp.off)) + d.vc_off;
            const double *sc = (const double *)(dhost.data() + (s_scal.off - s_dlp.off)) +
                               (size_t)DZG_DUALS_SCAL * i;
            u.source = DZG_DUALS_FRESH;
            u.dual_obj = sc[0];
            u.primal_infeas = sc[1];
            u.dual_infeas = sc[2];
            u.z_diff = sc[3] / std::max(1.0, sc[4]);
            if (u.y && m) std::memcpy(u.y, yv, sizeof(double) * (size_t)m);
            if (u.d && lp.n) std::memcpy(u.d, dv, sizeof(double) * (size_t)lp.n);
        }
    }
    return 0;
}

extern "C" int dzg_batch_solve(const dzg_lp *lps, int64_t count, const dzg_opts *opts,
                               int64_t pivots_per_launch, dzg_result *res)
{
    return batch_solve(lps, count, opts, pivots_per_launch, res, nullptr, false);
}

extern "C" int dzg_batch_solve_duals(const dzg_lp *lps, int64_t count, const dzg_opts *opts,
                                     int64_t pivots_per_launch, dzg_result *res, dzg_duals *du)
{
    return batch_solve(lps, count, opts, pivots_per_launch, res, du, true);
}

extern "C" int dzg_batch_solve_ranging(const dzg_lp *lps, int64_t count, const dzg_opts *opts,
                                       int64_t pivots_per_launch, const dzg_ranging_req *req, dzg_result *res,
                                       dzg_duals *du, dzg_ranging *rg)
{
    return batch_solve(lps, count, opts, pivots_per_launch, res, du, true, req, rg, true);
}

extern "C" int dzg_batch_solve_rays(const dzg_lp *lps, int64_t count, const dzg_opts *opts,
                                    int64_t pivots_per_launch, dzg_result *res, dzg_duals *du, dzg_ray *ry)
{
    if (count > 0 && !ry) return dzg_set_error(DZG_E_ARG, "batch: ry is NULL");
    return batch_solve(lps, count, opts, pivots_per_launch, res, du, du != nullptr, nullptr, nullptr, false, ry,
                       true);
}
