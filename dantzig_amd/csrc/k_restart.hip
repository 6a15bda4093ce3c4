// k_restart.hip -- the state of the CURRENT basis of a FAST solve for new data (dzg_solver_reoptimize).
//
// k_drift.hip recomputes x^ = B^-1 b and z^_N = N^T (B^-T c_B) - c_N right after a refactorisation to
// MEASURE how far the carried state is from them, and throws them away.  Here the same values, for a
// changed right-hand side and / or a changed objective, are WRITTEN: they become the state the
// parametric self-dual method carries on from, with both perturbation vectors at one
// (src/simplex.rs:203-204 sets them so for the slack basis; any basis will do).
//
//      x = B^-1 rhs             FTRAN's row function with rhs as the column (fast_rows.h)
//      z_k = -dzy_k - c[N_k]    dzy = -N^T y, y = B^-T c_B (dzg_launch_drift_y, then the column-wise
//                               pricing pass with y as v, both on the duals scratch: engine.hip)
//      xbar = zbar = 1
//
// The eta file is empty (the caller has just refactorised), so Binv0 is the whole inverse.  No atomics:
// every entry is written by one lane from sums of a fixed order, the call is reproducible bit for bit.
// One GPU, dense matrix.  tests/test_gpu_reopt.py checks the result against the state the basis
// defines, computed in long double (tests/state_check.py).
#include "common.h"
#include "fast_rows.h"

// rhs gathered to compact numbering (FTRAN's `ag`), zero-padded to even length
__global__ __launch_bounds__(256) void k_restart_gather(const DzgDev d, const double *__restrict__ rhs,
                                                        double *__restrict__ ag)
{
    const int k = d.ctl->ncompact, k2 = (k + 1) & ~1;
    for (int c = blockIdx.x * blockDim.x + threadIdx.x; c < k2; c += gridDim.x * blockDim.x)
        ag[c] = c < k ? rhs[d.drow[c]] : 0.0;
}

// x[i] = (row i of Binv0) . ag  (+ rhs of its own row where a slack is basic at i);  xbar[i] = 1
template <int LPR>
__global__ __launch_bounds__(256) void k_restart_x(const DzgDev d, const double *__restrict__ rhs,
                                                   const double *__restrict__ ag)
{
    constexpr int RPW = 64 / LPR;
    const int lane = threadIdx.x & 63;
    const int sub = lane % LPR, grp = lane / LPR;
    const int wave_global = (blockIdx.x * blockDim.x + threadIdx.x) >> 6;
    const int nwaves = (gridDim.x * blockDim.x) >> 6;
    const int k = d.ctl->ncompact, k2 = (k + 1) & ~1, m = d.m;
    for (int i0 = wave_global * RPW; i0 < m; i0 += nwaves * RPW) {
        const int i = i0 + grp;
        // (the eta file is empty right after a refactorisation: neta = 0)
        double xi = fast_gemv_row<LPR>(i, m, k2, 0, d.binv, d.ldb, ag, d.U, d.ldw, d.beta, sub);
        if (i < m && sub == 0) {
            const int bc = d.bcode[i];
            if (bc < 0) xi += rhs[-1 - bc]; // a basic slack: its column of the inverse is e_i
            d.x[i] = xi;
            d.xbar[i] = 1.0;
        }
    }
}

// z[k] = -dzy[k] - c[nonbasis[k]]  (dzy = -N^T y: the d of dzg_duals on the nonbasic positions);  zbar[k] = 1
__global__ __launch_bounds__(256) void k_restart_z(int q, const int *__restrict__ nonbasis,
                                                   const double *__restrict__ cdev,
                                                   const double *__restrict__ dzy, double *__restrict__ z,
                                                   double *__restrict__ zbar)
{
    for (int kpos = blockIdx.x * blockDim.x + threadIdx.x; kpos < q; kpos += gridDim.x * blockDim.x) {
        z[kpos] = -dzy[kpos] - cdev[nonbasis[kpos]];
        zbar[kpos] = 1.0;
    }
}

#define RS_BLOCKS 256

// ag: [m + 2] scratch.  The 16-lane instantiation up to k = 512, the 64-lane one above, as
// dzg_launch_drift chooses; k = 0 (the basis is all slack): x = rhs.
void dzg_launch_restart_x(const DzgDev &d, const double *rhs, double *ag, int k_bound, hipStream_t st)
{
    const int kb = k_bound > 0 ? k_bound : 1;
    hipLaunchKernelGGL(k_restart_gather, dim3((kb + 1 + 255) / 256), dim3(256), 0, st, d, rhs, ag);
    if (kb > 512)
        hipLaunchKernelGGL((k_restart_x<64>), dim3(RS_BLOCKS), dim3(256), 0, st, d, rhs, ag);
    else
        hipLaunchKernelGGL((k_restart_x<16>), dim3(RS_BLOCKS), dim3(256), 0, st, d, rhs, ag);
}

void dzg_launch_restart_z(const DzgDev &d, const double *cdev, const double *dzy, hipStream_t st)
{
    if (d.q <= 0) return;
    int blocks = (d.q + 255) / 256;
    if (blocks > RS_BLOCKS) blocks = RS_BLOCKS;
    hipLaunchKernelGGL(k_restart_z, dim3(blocks), dim3(256), 0, st, d.q, d.nonbasis, cdev, dzy, d.z, d.zbar);
}
