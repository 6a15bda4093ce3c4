// k_batch_restart.hip -- the restart state of a batched LP that starts from a handed-in basis B with
// nonbasic set N (dzg_batch_solve_from): what dzg_solver_reoptimize leaves in
// STRICT numerics, in the reference's arithmetic.
//
//      x   = LU::solve(B, rhs)                          rhs by constraint row
//      y   = LU::solve(B^T, c_B)
//      z_k = -neg_t_dot(N_k, y) - c[N_k]                k_duals_small's d on the nonbasic positions
//      xbar = zbar = 1
//
// One workgroup per LP, once, before the first round of k_batch_strict.  Both solves are
// batch_strict.h's gather + lu_solve_lds with the right-hand side written over column m, the way
// k_duals_small writes c_B there; the reduced costs are solve_dz's loop (stored entries only, rows
// ascending, each product rounded and then added, a slack column contributing 1.0 * -y[row]).  No
// product is fused with its sum (-ffp-contract=off).  The LDS carve-up is strict_steps':
// W, dx, v, then 16 bytes of flags.
//
// A start is singular when either factorisation met a zero pivot or the state holds a non-finite
// entry.  lu_solve_lds skips a zero pivot and leaves it where it found it: row k of the factored
// buffer is final after step k, so the diagonal read after the solve is the sticky flag over all
// steps, the last entry included, which the elimination loop never visits.
#include "batch_restart.h"
#include "batch_strict.h"

namespace {

template <int BLOCK>
__global__ __launch_bounds__(BLOCK) void k_batch_restart(DzgBatchRestartArgs g, const int *__restrict__ list)
{
    extern __shared__ __attribute__((aligned(16))) double s_mem[];
    const int id = list[blockIdx.x];
    const DzgBatchLp L = g.lp[id];
    const int m = L.m, q = L.n - L.m, ld = m + 1;
    const double *A = g.A + L.a_off;
    const int *var_col = g.var_col + L.vc_off;
    const int *basis = g.basis + L.m_off, *nonbasis = g.nonbasis + L.q_off;
    const double *c = g.c + L.vc_off;
    double *x = g.x + L.m_off, *xbar = g.xbar + L.m_off;
    double *z = g.z + L.q_off, *zbar = g.zbar + L.q_off;
    // the carve-up of strict_steps: W, dx, v, one int; the int behind it is this kernel's
    double *W = s_mem;
    double *v = s_mem + (long long)g.mmax * (g.mmax + 1) + g.mmax;
    int *s_flag = (int *)(v + g.mmax);
    int *s_bad = s_flag + 1;
    if (threadIdx.x == 0) *s_bad = 0;
    __syncthreads();
    int bad = 0;

    if (m > 0) {
        // ---- B x = rhs: the gather wrote a column of B into column m; the thread that wrote an
        // entry overwrites it (same row -> thread map as the gather's)
        dzg_bs::gather<BLOCK>(W, m, A, basis, var_col, 0, basis[0], -1);
        for (int r = threadIdx.x; r < m; r += BLOCK) W[r * ld + m] = x[r];
        dzg_bs::lu_solve_lds<BLOCK>(W, m, s_flag);
        for (int r = threadIdx.x; r < m; r += BLOCK) {
            const double xr = W[r * ld + m];
            x[r] = xr;
            xbar[r] = 1.0;
            if (!(W[r * ld + r] != 0.0) || !isfinite(xr)) bad = 1;
        }
        __syncthreads(); // the buffer is read; the next gather overwrites it

        // ---- B^T y = c_B, as k_duals_small
        dzg_bs::gather<BLOCK>(W, m, A, basis, var_col, 1, -1, -1);
        for (int r = threadIdx.x; r < m; r += BLOCK) W[r * ld + m] = c[basis[r]];
        dzg_bs::lu_solve_lds<BLOCK>(W, m, s_flag);
        for (int r = threadIdx.x; r < m; r += BLOCK) {
            v[r] = W[r * ld + m];
            if (!(W[r * ld + r] != 0.0)) bad = 1;
        }
        __syncthreads();
    }

    // ---- z = -neg_t_dot(nonbasis, y) - c_N (solve_dz's loop)
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
        const double zk = -acc - c[var];
        z[k] = zk;
        zbar[k] = 1.0;
        if (!isfinite(zk)) bad = 1;
    }
    if (bad) atomicOr(s_bad, 1);
    __syncthreads();
    if (threadIdx.x == 0 && *s_bad) g.status[id] = DZG_SINGULAR;
}

} // namespace

void dzg_launch_batch_restart(int bucket, const DzgBatchRestartArgs &g, const int *list, int n, hipStream_t st)
{
    const size_t lds = dzg_bs::lds_bytes(g.mmax);
    dzg_bh::for_each_chunk(bucket, n, [&](int c0, int grid) {
        dzg_bh::with_block(bucket, [&](auto block) {
            constexpr int BLOCK = decltype(block)::value;
            hipLaunchKernelGGL(k_batch_restart<BLOCK>, dim3(grid), dim3(BLOCK), lds, st, g, list + c0);
        });
    });
}
