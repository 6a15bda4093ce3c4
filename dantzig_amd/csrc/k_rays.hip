// k_rays.hip -- what a solve that ended UNBOUNDED or INFEASIBLE can show for it, recomputed from
// the final basis.
//
//      UNBOUNDED:   r = find_first_pivot(z, zbar), j = N[r], dx = B^-1 a_j
//                   d[j] = 1, d[B[p]] = -dx[p];  value = c[j] - sum_p c[B[p]] dx[p];  violation over dx
//      INFEASIBLE:  p = find_first_pivot(x, xbar), y = B^-T e_p, dz = -N^T y
//                   d[N[k]] = -dz[k], d[B[p]] = 1;  value = sum_i rhs0[i] y[i];     violation over dz
//
// k_rays_small: one workgroup per LP of a batch (m <= DZG_BATCH_MAX_ROWS), in the reference's
// arithmetic: scan_first, then solve_dx or solve_dz of batch_strict.h exactly as the failed step
// ran them; value is summed sequentially, each product rounded.
//
// k_ray_rhs / k_ray_dx_fast / k_ray_vt_fast / k_ray_resid_* / k_ray_finish: the solver handle's path.
// STRICT takes dx or y from dzg_launch_strict_solve and dz from a sequential pricing pass; FAST forms
// both with the fresh compact inverse (column of row r: Binv0[.][dslot[r]] where the row's slack is
// nonbasic, the unit vector of the slack's position otherwise) and refines them once against a
// double-double residual.  k_ray_finish scatters d by variable and leaves per-workgroup partials,
// which the host finishes in workgroup order.  No atomics anywhere: two calls on one state give the
// same bits.
#include "batch_strict.h"
#include "rays.h"

namespace {

// max over the wave: order-independent, exact
__device__ __forceinline__ double wave_max(double v)
{
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) v = fmax(v, __shfl_xor(v, off, DZG_WAVE));
    return v;
}

template <int BLOCK>
__global__ __launch_bounds__(BLOCK) void k_rays_small(DzgRaysArgs g, const int *__restrict__ list)
{
    extern __shared__ __attribute__((aligned(16))) double s_mem[];
    __shared__ double s_red[4][2];
    const int id = list[blockIdx.x];
    const DzgBatchLp L = g.lp[id];
    const int m = L.m, q = L.n - L.m;
    const double *A = g.A + L.a_off;
    const int *var_col = g.var_col + L.vc_off;
    const int *basis = g.basis + L.m_off, *nonbasis = g.nonbasis + L.q_off;
    const double *c = g.c + L.vc_off, *rhs0 = g.rhs0 + L.m_off;
    double *d = g.d + L.vc_off, *y = g.y + L.m_off, *dz = g.dz + L.q_off;
    double *out = g.scal + (long long)id * DZG_RAY_SCAL;
    const bool primal = g.status[id] == DZG_UNBOUNDED;
    // the carve-up of strict_steps: W, dx, v, one int
    double *W = s_mem;
    double *dx = s_mem + (long long)g.mmax * (g.mmax + 1);
    double *v = dx + g.mmax;
    int *s_flag = (int *)(v + g.mmax);

    const DzgCand cand = primal ? scan_first(g.z + L.q_off, g.zbar + L.q_off, q)
                                : scan_first(g.x + L.m_off, g.xbar + L.m_off, m);
    const int pos = cand.k;
    if (pos < 0 || m == 0) { // (no such state ends UNBOUNDED or INFEASIBLE)
        if (threadIdx.x == 0) out[0] = -1.0;
        return;
    }
    double viol = 0.0, bad = 0.0;
    if (primal) {
        dzg_bs::solve_dx<BLOCK>(A, var_col, m, W, dx, s_flag, basis, nonbasis[pos]);
        for (int k = threadIdx.x; k < q; k += BLOCK) d[nonbasis[k]] = k == pos ? 1.0 : 0.0;
        for (int p = threadIdx.x; p < m; p += BLOCK) {
            const double e = dx[p];
            d[basis[p]] = -e;
            y[p] = 0.0;
            viol = fmax(viol, fmax(e, 0.0));
            if (e != e) bad = 1.0;
        }
    } else {
        dzg_bs::solve_dz<BLOCK>(A, var_col, m, q, W, v, s_flag, basis, nonbasis, dz, pos);
        for (int k = threadIdx.x; k < q; k += BLOCK) {
            const double e = dz[k];
            d[nonbasis[k]] = -e;
            viol = fmax(viol, fmax(e, 0.0));
            if (e != e) bad = 1.0;
        }
        for (int p = threadIdx.x; p < m; p += BLOCK) {
            d[basis[p]] = p == pos ? 1.0 : 0.0;
            y[p] = v[p];
        }
    }
    viol = wave_max(viol);
    bad = wave_max(bad);
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    if (lane == 0) {
        s_red[wave][0] = viol;
        s_red[wave][1] = bad;
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        for (int w = 1; w < BLOCK / 64; ++w) {
            viol = fmax(viol, s_red[w][0]);
            bad = fmax(bad, s_red[w][1]);
        }
        double value; // one rounded product and one rounded sum or difference each, ascending
        if (primal) {
            value = c[nonbasis[pos]];
            for (int p = 0; p < m; ++p) {
                const double prod = c[basis[p]] * dx[p];
                value = value - prod;
            }
        } else {
            value = 0.0;
            for (int i = 0; i < m; ++i) {
                const double prod = rhs0[i] * v[i];
                value = value + prod;
            }
        }
        out[0] = (double)(primal ? nonbasis[pos] : basis[pos]);
        out[1] = (double)pos;
        out[2] = cand.r;
        out[3] = value;
        out[4] = bad != 0.0 ? __builtin_nan("") : viol;
    }
}

__global__ __launch_bounds__(256) void k_ray_rhs(int m, const double *__restrict__ A, long long lda,
                                                 int code, double *__restrict__ out)
{
    const int r = blockIdx.x * 256 + threadIdx.x;
    if (r >= m) return;
    double v;
    if (A && code >= 0) {
        v = A[(long long)code * lda + r];
        v = v != 0.0 ? v : 0.0; // an explicit -0.0 is not a stored entry
    } else {
        v = (A ? -1 - code : code) == r ? 1.0 : 0.0;
    }
    out[r] = v;
}

// ---- FAST: products with the fresh compact inverse M (m positions x m rows):
//      M[p][r] = Binv0[p][dslot[r]] where row r's slack is nonbasic (dslot[r] in [0, k)),
//                1 where row r's slack sits at position p, 0 otherwise
// and one step of iterative refinement whose residual is accumulated in double-double (two_prod by
// fma, two_sum), so that what the explicit inverse loses to cancellation comes back: the result is
// as good as a backward-stable solve of the same basis, not as good as |M| |a| allows.
__device__ __forceinline__ void dd_add(double &hi, double &lo, double x)
{
    const double s = hi + x;
    const double bb = s - hi;
    lo = lo + ((hi - (s - bb)) + (x - bb));
    hi = s;
}

__device__ __forceinline__ void dd_add_prod(double &hi, double &lo, double a, double b)
{
    const double p = a * b;
    const double e = fma(a, b, -p);
    dd_add(hi, lo, p);
    lo = lo + e;
}

// dx[p] (+)= (M h)_p.  One wave per basis position p: the entries of h over the rows in lane order,
// a fixed tree.
__global__ __launch_bounds__(256) void k_ray_dx_fast(const DzgDev d, int k, const double *__restrict__ h,
                                                     int accumulate, double *__restrict__ dx)
{
    const int lane = threadIdx.x & 63;
    const int p = blockIdx.x * 4 + (threadIdx.x >> 6);
    if (p >= d.m) return; // (whole waves)
    const int bc = d.bcode[p];
    const double *row = d.binv + (long long)p * d.ldb;
    double acc = 0.0, unit = 0.0;
    for (int r = lane; r < d.m; r += 64) {
        const double a = h[r];
        const int c = d.dslot[r];
        if (c >= 0 && c < k) acc = fma(a, row[c], acc);
        if (bc == -1 - r) unit = a;
    }
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) {
        acc = acc + __shfl_xor(acc, off, DZG_WAVE);
        unit = unit + __shfl_xor(unit, off, DZG_WAVE); // (one lane at most holds a nonzero)
    }
    acc = acc + unit;
    if (lane == 0) dx[p] = accumulate ? dx[p] + acc : acc;
}

// v[r] (+)= (M^T w)_r, one thread per row
__global__ __launch_bounds__(256) void k_ray_vt_fast(const DzgDev d, int k, const double *__restrict__ w,
                                                     int accumulate, double *__restrict__ v)
{
    const int r = blockIdx.x * 256 + threadIdx.x;
    if (r >= d.m) return;
    const int c = d.dslot[r];
    double acc = 0.0;
    if (c >= 0 && c < k) {
        for (int p = 0; p < d.m; ++p) acc = fma(w[p], d.binv[(long long)p * d.ldb + c], acc);
    } else {
        for (int p = 0; p < d.m; ++p)
            if (d.bcode[p] == -1 - r) acc = w[p];
    }
    v[r] = accumulate ? v[r] + acc : acc;
}

// res[r] = h[r] - (B dx)_r, one thread per row (a row of B is read across the basis columns)
__global__ __launch_bounds__(256) void k_ray_resid_dx(const DzgDev d, const double *__restrict__ h,
                                                      const double *__restrict__ dx, double *__restrict__ res)
{
    const int r = blockIdx.x * 256 + threadIdx.x;
    if (r >= d.m) return;
    double hi = h[r], lo = 0.0;
    for (int p = 0; p < d.m; ++p) {
        const int bc = d.bcode[p];
        if (bc >= 0)
            dd_add_prod(hi, lo, -d.A[(long long)bc * d.lda + r], dx[p]);
        else if (r == -1 - bc)
            dd_add(hi, lo, -dx[p]);
    }
    res[r] = hi + lo;
}

// res[p] = t[p] - (B^T y)_p with t = unit(pos), or t[p] = cvar[basis[p]] where cvar is given (c_B: the
// residual of the dual vector); one wave per basis position p (its column of B in lane order)
__global__ __launch_bounds__(256) void k_ray_resid_v(const DzgDev d, int pos, const double *__restrict__ cvar,
                                                     const double *__restrict__ y, double *__restrict__ res)
{
    const int lane = threadIdx.x & 63;
    const int p = blockIdx.x * 4 + (threadIdx.x >> 6);
    if (p >= d.m) return; // (whole waves)
    const int bc = d.bcode[p];
    double hi = lane != 0 ? 0.0 : cvar ? cvar[d.basis[p]] : (p == pos ? 1.0 : 0.0), lo = 0.0;
    if (bc >= 0) {
        const double *col = d.A + (long long)bc * d.lda;
        for (int r = lane; r < d.m; r += 64) dd_add_prod(hi, lo, -col[r], y[r]);
    } else if (lane == 0) {
        dd_add(hi, lo, -y[-1 - bc]);
    }
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) { // a fixed tree of double-double sums
        const double ohi = __shfl_xor(hi, off, DZG_WAVE), olo = __shfl_xor(lo, off, DZG_WAVE);
        dd_add(hi, lo, ohi);
        lo = lo + olo;
    }
    if (lane == 0) res[p] = hi + lo;
}

__global__ __launch_bounds__(256) void k_ray_finish(int kind, int m, int q, int pos,
                                                    const int *__restrict__ basis,
                                                    const int *__restrict__ nonbasis,
                                                    const double *__restrict__ vec,
                                                    const double *__restrict__ c,
                                                    const double *__restrict__ rhs0,
                                                    const double *__restrict__ y, double *__restrict__ d,
                                                    double *__restrict__ part)
{
    __shared__ double s_red[4][3];
    const int gid = blockIdx.x * blockDim.x + threadIdx.x, stride = gridDim.x * blockDim.x;
    double viol = 0.0, bad = 0.0, sum = 0.0;
    if (kind == DZG_RAY_PRIMAL) {
        for (int k = gid; k < q; k += stride) d[nonbasis[k]] = k == pos ? 1.0 : 0.0;
        for (int p = gid; p < m; p += stride) {
            const int var = basis[p];
            const double e = vec[p];
            d[var] = -e;
            viol = fmax(viol, fmax(e, 0.0));
            if (e != e) bad = 1.0;
            const double prod = c[var] * e;
            sum = sum + prod;
        }
    } else {
        for (int k = gid; k < q; k += stride) {
            const double e = vec[k];
            d[nonbasis[k]] = -e;
            viol = fmax(viol, fmax(e, 0.0));
            if (e != e) bad = 1.0;
        }
        for (int p = gid; p < m; p += stride) {
            d[basis[p]] = p == pos ? 1.0 : 0.0;
            const double prod = rhs0[p] * y[p];
            sum = sum + prod;
        }
    }
    viol = wave_max(viol);
    bad = wave_max(bad);
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) sum = sum + __shfl_xor(sum, off, DZG_WAVE); // a fixed tree
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    if (lane == 0) {
        s_red[wave][0] = viol;
        s_red[wave][1] = bad;
        s_red[wave][2] = sum;
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        for (int w = 1; w < 4; ++w) { // wave order
            viol = fmax(viol, s_red[w][0]);
            bad = fmax(bad, s_red[w][1]);
            sum = sum + s_red[w][2];
        }
        double *out = part + (long long)blockIdx.x * DZG_RAY_PART;
        out[0] = viol;
        out[1] = bad;
        out[2] = sum;
        out[3] = 0.0;
    }
}

} // namespace

void dzg_launch_rays_small(int bucket, const DzgRaysArgs &g, const int *list, int n, hipStream_t st)
{
    const size_t lds = dzg_bs::lds_bytes(g.mmax);
    dzg_bh::for_each_chunk(bucket, n, [&](int c0, int grid) {
        dzg_bh::with_block(bucket, [&](auto block) {
            constexpr int BLOCK = decltype(block)::value;
            hipLaunchKernelGGL(k_rays_small<BLOCK>, dim3(grid), dim3(BLOCK), lds, st, g, list + c0);
        });
    });
}

void dzg_launch_ray_rhs(int m, const double *A, long long lda, int code, double *out, hipStream_t st)
{
    if (m <= 0) return;
    hipLaunchKernelGGL(k_ray_rhs, dim3((m + 255) / 256), dim3(256), 0, st, m, A, lda, code, out);
}

void dzg_launch_ray_dx_fast(const DzgDev &d, int k, const double *h, int accumulate, double *dx, hipStream_t st)
{
    if (d.m <= 0) return;
    hipLaunchKernelGGL(k_ray_dx_fast, dim3((d.m + 3) / 4), dim3(256), 0, st, d, k, h, accumulate, dx);
}

void dzg_launch_ray_vt_fast(const DzgDev &d, int k, const double *w, int accumulate, double *v, hipStream_t st)
{
    if (d.m <= 0) return;
    hipLaunchKernelGGL(k_ray_vt_fast, dim3((d.m + 255) / 256), dim3(256), 0, st, d, k, w, accumulate, v);
}

void dzg_launch_ray_resid_dx(const DzgDev &d, const double *h, const double *dx, double *res, hipStream_t st)
{
    if (d.m <= 0) return;
    hipLaunchKernelGGL(k_ray_resid_dx, dim3((d.m + 255) / 256), dim3(256), 0, st, d, h, dx, res);
}

void dzg_launch_ray_resid_v(const DzgDev &d, int pos, const double *y, double *res, hipStream_t st,
                            const double *cvar)
{
    if (d.m <= 0) return;
    hipLaunchKernelGGL(k_ray_resid_v, dim3((d.m + 3) / 4), dim3(256), 0, st, d, pos, cvar, y, res);
}

void dzg_launch_ray_finish(int kind, int m, int q, int pos, const int *basis, const int *nonbasis,
                           const double *vec, const double *c, const double *rhs0, const double *y,
                           double *d, double *part, hipStream_t st)
{
    hipLaunchKernelGGL(k_ray_finish, dim3(DZG_RAY_BLOCKS), dim3(256), 0, st, kind, m, q, pos, basis,
                       nonbasis, vec, c, rhs0, y, d, part);
}
