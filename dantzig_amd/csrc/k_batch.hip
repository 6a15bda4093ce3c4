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

#include "common.h"

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

// B (transposed == 0: W[r][c] = A[r, basis[c]]) or B^T (W[r][c] = A[c, basis[r]]) into LDS, row
// stride ld = m + 1, the right-hand side into column m: the entering column (transposed == 0) or
// unit(pos).  Stored entries only: the reference's basis matrix is a CSC densified into zeros, so an
// explicit -0.0 of A arrives as +0.0 (oracle gather_basis / column_of).
template <int BLOCK>
__device__ void gather(double *W, int m, const double *A, const int *basis, const int *var_col,
                       int transposed, int enter_var, int pos)
{
    const int ld = m + 1;
    for (int e = threadIdx.x; e < m * m; e += BLOCK) {
        const int c = e / m, r = e - c * m; // basis position c, constraint row r
        const int code = var_col[basis[c]];
        double v;
        if (code >= 0) {
            v = A[(long long)code * m + r];
            v = v != 0.0 ? v : 0.0;
        } else {
            v = (-1 - code) == r ? 1.0 : 0.0;
        }
        if (transposed)
            W[c * ld + r] = v;
        else
            W[r * ld + c] = v;
    }
    for (int r = threadIdx.x; r < m; r += BLOCK) {
        double v;
        if (transposed) {
            v = r == pos ? 1.0 : 0.0;
        } else {
            const int code = var_col[enter_var];
            if (code >= 0) {
                v = A[(long long)code * m + r];
                v = v != 0.0 ? v : 0.0;
            } else {
                v = (-1 - code) == r ? 1.0 : 0.0;
            }
        }
        W[r * ld + m] = v;
    }
}

// first maximum of |.|: larger value wins, lower row on ties; NaN never wins (x > NaN is false)
__device__ __forceinline__ DzgCand abs_cand(double value, int row)
{
    DzgCand c;
    c.r = fabs(value);
    c.k = (c.r == c.r) ? row : -1;
    return c;
}

// Matrix::factorize + LU::solve (src/linalg.rs:88-128, 282-299) of the gathered system in place;
// the solution ends in column m.  Starts and ends with the buffer consistent for every thread.
template <int BLOCK>
__device__ void lu_solve_lds(double *W, int m, int *s_flag)
{
    const int ld = m + 1;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    __syncthreads(); // the gather is complete
    for (int k = 0; k + 1 < m; ++k) {
        if (wave == 0) {
            DzgCand best;
            best.r = 0.0;
            best.k = -1;
            for (int r = k + lane; r < m; r += 64) best = dzg_better(best, abs_cand(W[r * ld + k], r));
            best = dzg_wave_best(best);
            const double akk = W[k * ld + k];
            // `x > NaN` is never true: a NaN at (k,k) keeps mu = k (src/linalg.rs:98-105)
            const int mu = (fabs(akk) != fabs(akk) || best.k < 0) ? k : best.k;
            if (mu != k) { // swap rows k and mu on columns >= k, the right-hand side included
                for (int j = k + lane; j <= m; j += 64) {
                    const double a = W[k * ld + j];
                    W[k * ld + j] = W[mu * ld + j];
                    W[mu * ld + j] = a;
                }
            }
            __builtin_amdgcn_wave_barrier();
            const double pivot = W[k * ld + k];
            const bool zero = !(pivot != 0.0); // src/linalg.rs:117 (NaN is "nonzero")
            // zero pivot: no scaling, no update of the matrix; LU::solve still runs
            // b[i] -= b[k] * a(i,k) with the stored entry (src/linalg.rs:288-290)
            if (!zero)
                for (int r = k + 1 + lane; r < m; r += 64) W[r * ld + k] = dzg_div(W[r * ld + k], pivot);
            if (lane == 0) *s_flag = zero ? 1 : 0;
        }
        __syncthreads();
        const bool zero = *s_flag != 0;
        const int ncols = m - k; // columns k+1 .. m (m: the right-hand side)
        const int total = (m - 1 - k) * ncols;
        for (int e = threadIdx.x; e < total; e += BLOCK) {
            const int i = k + 1 + e / ncols;
            const int j = k + 1 + e % ncols;
            if (zero && j < m) continue;
            const double adjustment = W[i * ld + k] * W[k * ld + j];
            W[i * ld + j] = W[i * ld + j] - adjustment;
        }
        __syncthreads();
    }
    if (wave == 0) { // back substitution, src/linalg.rs:292-297: j ascending inside each row
        for (int i = m - 1; i >= 0; --i) {
            const int j0 = i + 1 + lane, j1 = j0 + 64;
            const double p0 = j0 < m ? W[i * ld + j0] * W[j0 * ld + m] : 0.0;
            const double p1 = j1 < m ? W[i * ld + j1] * W[j1 * ld + m] : 0.0;
            double t = W[i * ld + m];
            const int nj = m - 1 - i;
            for (int s = 0; s < nj; ++s) {
                const double prod = s < 64 ? dzg_readlane_f64(p0, s) : dzg_readlane_f64(p1, s - 64);
                t = t - prod;
            }
            t = dzg_div(t, W[i * ld + i]);
            if (lane == 0) W[i * ld + m] = t;
            __builtin_amdgcn_wave_barrier();
        }
    }
    __syncthreads();
}

template <int BLOCK>
__device__ void solve_dx(const BArgs &g, const BLp &L, double *W, double *dx, int *s_flag,
                         const int *basis, int enter_var)
{
    gather<BLOCK>(W, L.m, g.A + L.a_off, basis, g.var_col + L.vc_off, 0, enter_var, -1);
    lu_solve_lds<BLOCK>(W, L.m, s_flag);
    for (int r = threadIdx.x; r < L.m; r += BLOCK) dx[r] = W[r * (L.m + 1) + L.m];
    __syncthreads();
}

// v = B^-T e_pos, then dz = collect_columns(nonbasis).neg_t_dot(v) into global memory
template <int BLOCK>
__device__ void solve_dz(const BArgs &g, const BLp &L, double *W, double *v, int *s_flag,
                         const int *basis, const int *nonbasis, double *dz, int pos)
{
    const int m = L.m, q = L.n - L.m;
    const int *var_col = g.var_col + L.vc_off;
    const double *A = g.A + L.a_off;
    gather<BLOCK>(W, m, A, basis, var_col, 1, -1, pos);
    lu_solve_lds<BLOCK>(W, m, s_flag);
    for (int r = threadIdx.x; r < m; r += BLOCK) v[r] = W[r * (m + 1) + m];
    __syncthreads();
    for (int k = threadIdx.x; k < q; k += BLOCK) {
        const int code = var_col[nonbasis[k]];
        double acc = 0.0; // Iterator::sum identity
        if (code < 0) {   // a slack column's one stored entry
            const double prod = 1.0 * -v[-1 - code];
            acc = acc + prod;
        } else {
            const double *col = A + (long long)code * m;
            for (int r = 0; r < m; ++r) {
                const double a = col[r];
                if (a == 0.0) continue; // not a stored entry
                const double prod = a * -v[r];
                acc = acc + prod;
            }
        }
        dz[k] = acc;
    }
    __syncthreads();
}

template <int BLOCK>
__global__ __launch_bounds__(BLOCK) void k_batch_strict(BArgs g, const int *__restrict__ list,
                                                        int *__restrict__ next_list,
                                                        int *__restrict__ next_count)
{
    extern __shared__ __attribute__((aligned(16))) double s_mem[];
    const int id = list[blockIdx.x];
    const BLp L = g.lp[id];
    const int m = L.m, q = L.n - L.m;
    double *W = s_mem;                                  // mmax x (mmax + 1)
    double *dx = s_mem + (long long)g.mmax * (g.mmax + 1); // mmax
    double *v = dx + g.mmax;                            // mmax
    int *s_flag = (int *)(v + g.mmax);
    int *basis = g.basis + L.m_off, *nonbasis = g.nonbasis + L.q_off;
    double *x = g.x + L.m_off, *xbar = g.xbar + L.m_off;
    double *z = g.z + L.q_off, *zbar = g.zbar + L.q_off, *dz = g.dz + L.q_off;
    long long it = g.iter[id];
    int status = DZG_RUNNING;

    for (int step = 0; step < g.ppl; ++step) {
        // ---- status(), src/simplex.rs:274-306
        const DzgCand cj = scan_first(z, zbar, q);
        const DzgCand ci = scan_first(x, xbar, m);
        int kind;
        double mu;
        if (cj.k >= 0 && ci.k >= 0) {
            const double primal = ci.r, dual = cj.r; // :280-281
            if (primal <= g.eps && dual <= g.eps) {
                status = DZG_OPTIMAL;
                break;
            }
            if (primal < dual) {
                kind = DZG_STEP_PRIMAL;
                mu = dual;
            } else {
                kind = DZG_STEP_DUAL;
                mu = primal;
            }
        } else if (cj.k >= 0) { // :294-298, no optimality test
            kind = DZG_STEP_PRIMAL;
            mu = cj.r;
        } else if (ci.k >= 0) { // :299-303
            kind = DZG_STEP_DUAL;
            mu = ci.r;
        } else {
            status = DZG_PANIC; // :304
            break;
        }
        if (it >= g.max_iter) {
            status = DZG_ITER_LIMIT;
            break;
        }
        if (m == 0) { // n - 1 underflow in Matrix::factorize: a reference panic path
            status = DZG_PANIC;
            break;
        }
        int p, r;
        if (kind == DZG_STEP_PRIMAL) { // :308-318
            r = cj.k;
            solve_dx<BLOCK>(g, L, W, dx, s_flag, basis, nonbasis[r]);
            p = scan_second(mu, x, xbar, dx, m).k;
            if (p < 0) {
                status = DZG_UNBOUNDED;
                break;
            }
            solve_dz<BLOCK>(g, L, W, v, s_flag, basis, nonbasis, dz, p);
        } else { // :320-330
            p = ci.k;
            solve_dz<BLOCK>(g, L, W, v, s_flag, basis, nonbasis, dz, p);
            r = scan_second(mu, z, zbar, dz, q).k;
            if (r < 0) {
                status = DZG_INFEASIBLE;
                break;
            }
            solve_dx<BLOCK>(g, L, W, dx, s_flag, basis, nonbasis[r]);
        }
        // ---- pivot, src/simplex.rs:253-268: step lengths, finiteness assert (:466)
        int ok = 1;
        const double t = dzg_safe_divide(x[p], dx[p], &ok);
        const double s = dzg_safe_divide(z[r], dz[r], &ok);
        const double tbar = dzg_safe_divide(xbar[p], dx[p], &ok);
        const double sbar = dzg_safe_divide(zbar[r], dz[r], &ok);
        if (!ok) {
            status = DZG_PANIC; // the pivot was chosen, not executed
            break;
        }
        const int i_var = basis[p], j_var = nonbasis[r];
        __syncthreads(); // every thread has read x[p], z[r], basis[p], nonbasis[r]
        if (threadIdx.x == 0) {
            if (it < L.log_cap) {
                g.log_kind[L.log_off + it] = kind;
                g.log_enter[L.log_off + it] = j_var;
                g.log_leave[L.log_off + it] = i_var;
                g.log_mu[L.log_off + it] = mu;
            }
            basis[p] = j_var; // swap, :243-247
            nonbasis[r] = i_var;
        }
        for (int i = threadIdx.x; i < m; i += BLOCK) {
            const double d = dx[i];
            const double a = t * d, b = tbar * d;
            x[i] = (i == p) ? t : x[i] - a;
            xbar[i] = (i == p) ? tbar : xbar[i] - b;
        }
        for (int k = threadIdx.x; k < q; k += BLOCK) {
            const double d = dz[k];
            const double a = s * d, b = sbar * d;
            z[k] = (k == r) ? s : z[k] - a;
            zbar[k] = (k == r) ? sbar : zbar[k] - b;
        }
        ++it;
        __syncthreads(); // the next status() reads the updated vectors
    }
    if (threadIdx.x == 0) {
        g.status[id] = status;
        g.iter[id] = it;
        if (status == DZG_RUNNING) next_list[atomicAdd(next_count, 1)] = id;
    }
}

// Row buckets: one launch each, LDS and workgroup size sized for the bucket.
const int kBucketRows[] = {16, 32, 64, DZG_BATCH_MAX_ROWS};
const int kBuckets = 4;
// Workgroups per launch at most: what one launch's pivots_per_launch pivots may cost is bounded by
// how many workgroups must take turns on a CU.  128 rows: 134 KB of LDS, one workgroup per CU, 256
// per launch (16 pivots x 2.3 ms measured = 37 ms per launch); 64 rows: four per CU.
const int kMaxGrid[] = {4096, 4096, 2048, 256};

int bucket_of(int64_t m)
{
    for (int b = 0; b < kBuckets; ++b)
        if (m <= kBucketRows[b]) return b;
    return -1;
}

size_t lds_bytes(int mmax)
{
    return sizeof(double) * ((size_t)mmax * (mmax + 1) + 2 * (size_t)mmax) + 16;
}

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

extern "C" int dzg_batch_solve(const dzg_lp *lps, int64_t count, const dzg_opts *opts,
                               int64_t pivots_per_launch, dzg_result *res)
{
    // ---- host checks first: malformed input is DZG_E_ARG on any machine
    if (count < 0) return dzg_set_error(DZG_E_ARG, "batch: count < 0");
    if (count > 0 && (!lps || !res)) return dzg_set_error(DZG_E_ARG, "batch: lps or res is NULL");
    if (count >= (1ll << 31)) return dzg_set_error(DZG_E_ARG, "batch: count out of range");
    if (pivots_per_launch < 0) return dzg_set_error(DZG_E_ARG, "batch: pivots_per_launch < 0");
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
    struct Guard {
        unsigned char **dev;
        hipStream_t *st;
        ~Guard()
        {
            if (*dev) (void)hipFree(*dev);
            if (*st) (void)hipStreamDestroy(*st);
        }
    } guard{&dev, &st};
    BHIP(hipStreamCreateWithFlags(&st, hipStreamNonBlocking));
    BHIP(hipMalloc((void **)&dev, top));
    BHIP(hipMemcpyAsync(dev, host.data(), upload_end, hipMemcpyHostToDevice, st));

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
    }
    return 0;
}
