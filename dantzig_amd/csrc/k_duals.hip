// k_duals.hip -- dual values and reduced costs at an OPTIMAL basis, recomputed from the basis
// instead of read off the carried z.
//
//      y   = B^-T c_B                                   one entry per row
//      d_j = a_j . y - c_j  for nonbasic j,  0 for basic j   one entry per variable
//
// k_duals_small: one workgroup per LP of a batch (m <= DZG_BATCH_MAX_ROWS), in the reference's
// arithmetic: B^T is gathered as every BTRAN of batch_strict.h gathers it, with c_B in the place of
// the unit vector; lu_solve_lds leaves y in column m; d is solve_dz's neg_t_dot loop with y as v,
// then  -dot - c.  dual_obj is summed sequentially over ascending rows, each product rounded.
//
// k_duals_finish: the tail of the solver handle's path, where y came from dzg_launch_strict_solve
// (STRICT) or from the fresh compact inverse (FAST) and  dzy = -N^T y  from a pricing pass: scatters
// d by variable and leaves per-workgroup partials of the certificate's reductions, which the host
// finishes in workgroup order.  No atomics anywhere: two calls on one state give the same bits.
#include "batch_strict.h"
#include "duals.h"

namespace {

// min / max over the wave: order-independent, exact
__device__ __forceinline__ double wave_min(double v)
{
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) v = fmin(v, __shfl_xor(v, off, DZG_WAVE));
    return v;
}

__device__ __forceinline__ double wave_max(double v)
{
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) v = fmax(v, __shfl_xor(v, off, DZG_WAVE));
    return v;
}

template <int BLOCK>
__global__ __launch_bounds__(BLOCK) void k_duals_small(DzgDualsArgs g, const int *__restrict__ list)
{
    extern __shared__ __attribute__((aligned(16))) double s_mem[];
    __shared__ double s_red[4][4];
    const int id = list[blockIdx.x];
    const DzgBatchLp L = g.lp[id];
    const int m = L.m, q = L.n - L.m, ld = m + 1;
    const double *A = g.A + L.a_off;
    const int *var_col = g.var_col + L.vc_off;
    const int *basis = g.basis + L.m_off, *nonbasis = g.nonbasis + L.q_off;
    const double *c = g.c + L.vc_off;
    const double *x = g.x + L.m_off, *z = g.z + L.q_off, *rhs0 = g.rhs0 + L.m_off;
    double *y = g.y + L.m_off, *d = g.d + L.vc_off;
    // the carve-up of strict_steps: W, dx, v, one int
    double *W = s_mem;
    double *v = s_mem + (long long)g.mmax * (g.mmax + 1) + g.mmax;
    int *s_flag = (int *)(v + g.mmax);

    // ---- B^T y = c_B: the gather wrote zeros into column m; the thread that wrote an entry
    // overwrites it (same row -> thread map as the gather's)
    dzg_bs::gather<BLOCK>(W, m, A, basis, var_col, 1, -1, -1);
    for (int r = threadIdx.x; r < m; r += BLOCK) W[r * ld + m] = c[basis[r]];
    dzg_bs::lu_solve_lds<BLOCK>(W, m, s_flag);
    for (int r = threadIdx.x; r < m; r += BLOCK) {
        const double yr = W[r * ld + m];
        v[r] = yr;
        y[r] = yr;
    }
    __syncthreads();

    // ---- d_N = -neg_t_dot(nonbasis, y) - c_N (solve_dz's loop), zeros for the basics
    double dmin = __builtin_inf(), dabs = 0.0, zdiff = 0.0, xmin = __builtin_inf();
    for (int p = threadIdx.x; p < m; p += BLOCK) {
        d[basis[p]] = 0.0;
        xmin = fmin(xmin, x[p]);
    }
    for (int k = threadIdx.x; k < q; k += BLOCK) {
        const int var = nonbasis[k];
        const int code = var_col[var];
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
        const double dk = -acc - c[var];
        d[var] = dk;
        dmin = fmin(dmin, dk);
        dabs = fmax(dabs, fabs(dk));
        zdiff = fmax(zdiff, fabs(z[k] - dk));
    }
    dmin = wave_min(dmin);
    dabs = wave_max(dabs);
    zdiff = wave_max(zdiff);
    xmin = wave_min(xmin);
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    if (lane == 0) {
        s_red[wave][0] = dmin;
        s_red[wave][1] = dabs;
        s_red[wave][2] = zdiff;
        s_red[wave][3] = xmin;
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        for (int w = 1; w < BLOCK / 64; ++w) {
            dmin = fmin(dmin, s_red[w][0]);
            dabs = fmax(dabs, s_red[w][1]);
            zdiff = fmax(zdiff, s_red[w][2]);
            xmin = fmin(xmin, s_red[w][3]);
        }
        double sum = 0.0; // rows ascending, one rounded product and one rounded sum each
        for (int i = 0; i < m; ++i) {
            const double prod = rhs0[i] * v[i];
            sum = sum + prod;
        }
        double *out = g.scal + (long long)id * DZG_DUALS_SCAL;
        out[0] = L.constant + sum;
        out[1] = fmax(0.0, -xmin);
        out[2] = fmax(0.0, -dmin);
        out[3] = zdiff; // the host divides: max |z - d_N| / max(1, max |d_N|)
        out[4] = dabs;
    }
}

__global__ __launch_bounds__(256) void k_duals_finish(int m, int q, const int *__restrict__ basis,
                                                      const int *__restrict__ nonbasis,
                                                      const double *__restrict__ c,
                                                      const double *__restrict__ dzy,
                                                      const double *__restrict__ z,
                                                      const double *__restrict__ x,
                                                      const double *__restrict__ rhs0,
                                                      const double *__restrict__ y, double *__restrict__ d,
                                                      double *__restrict__ part)
{
    __shared__ double s_red[4][5];
    const int gid = blockIdx.x * blockDim.x + threadIdx.x, stride = gridDim.x * blockDim.x;
    double dmin = __builtin_inf(), dabs = 0.0, zdiff = 0.0, xmin = __builtin_inf(), dot = 0.0;
    for (int k = gid; k < q; k += stride) {
        const int var = nonbasis[k];
        const double dk = -dzy[k] - c[var];
        d[var] = dk;
        dmin = fmin(dmin, dk);
        dabs = fmax(dabs, fabs(dk));
        zdiff = fmax(zdiff, fabs(z[k] - dk));
    }
    for (int p = gid; p < m; p += stride) {
        d[basis[p]] = 0.0;
        xmin = fmin(xmin, x[p]);
        const double prod = rhs0[p] * y[p];
        dot = dot + prod;
    }
    dmin = wave_min(dmin);
    dabs = wave_max(dabs);
    zdiff = wave_max(zdiff);
    xmin = wave_min(xmin);
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) dot = dot + __shfl_xor(dot, off, DZG_WAVE); // a fixed tree
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    if (lane == 0) {
        s_red[wave][0] = dmin;
        s_red[wave][1] = dabs;
        s_red[wave][2] = zdiff;
        s_red[wave][3] = xmin;
        s_red[wave][4] = dot;
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        for (int w = 1; w < 4; ++w) { // wave order
            dmin = fmin(dmin, s_red[w][0]);
            dabs = fmax(dabs, s_red[w][1]);
            zdiff = fmax(zdiff, s_red[w][2]);
            xmin = fmin(xmin, s_red[w][3]);
            dot = dot + s_red[w][4];
        }
        double *out = part + (long long)blockIdx.x * DZG_DUALS_PART;
        out[0] = dmin;
        out[1] = dabs;
        out[2] = zdiff;
        out[3] = xmin;
        out[4] = dot;
        out[5] = out[6] = out[7] = 0.0;
    }
}

} // namespace

void dzg_launch_duals_small(int bucket, const DzgDualsArgs &g, const int *list, int n, hipStream_t st)
{
    const size_t lds = dzg_bs::lds_bytes(g.mmax);
    dzg_bh::for_each_chunk(bucket, n, [&](int c0, int grid) {
        dzg_bh::with_block(bucket, [&](auto block) {
            constexpr int BLOCK = decltype(block)::value;
            hipLaunchKernelGGL(k_duals_small<BLOCK>, dim3(grid), dim3(BLOCK), lds, st, g, list + c0);
        });
    });
}

void dzg_launch_duals_finish(int m, int q, const int *basis, const int *nonbasis, const double *c,
                             const double *dzy, const double *z, const double *x, const double *rhs0,
                             const double *y, double *d, double *part, hipStream_t st)
{
    hipLaunchKernelGGL(k_duals_finish, dim3(DZG_DUALS_BLOCKS), dim3(256), 0, st, m, q, basis, nonbasis, c,
                       dzy, z, x, rhs0, y, d, part);
}
