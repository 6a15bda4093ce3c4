// k_remove.hip -- the constraint matrix of a live solver shrunk on the device (dzg_solver_remove).
//
// dzg_solver_remove drops constraint rows and structural columns from the LP a handle holds.  The
// successor's matrix is filled device to device from the resident one; only the two lists of what is
// kept cross PCIe.  Both lists are ascending, so
//
//      dst[j' * lda' + i'] = src[keep_col[j'] * lda + keep_row[i']]
//
// writes every column of the successor contiguously (lane i' next to lane i' + 1) and reads the source
// column in runs: keep_row is monotone, a wave's 64 reads fall into 64 + (rows dropped among them)
// consecutive doubles.  No LDS: nothing is transposed and nothing is read twice.
//
//      k_remove_gather     rows and columns: one double a lane, rows by the list
//      k_remove_columns    no row dropped (m' = m, lda' = lda): whole columns by the list, 16 bytes a
//                          lane, the body of k_extend_restride (k_extend.hip)
//
// One writer per entry, no atomics.  The source holds no -0.0 (creation and dzg_solver_extend store
// +0.0), a copy keeps it that way.  Rows m'..lda'-1 of the successor are zero from its allocation.
#include "common.h"

// grid (row chunks, columns), block 256.  keep_row: mk ascending rows in [0, m); keep_col: nk ascending
// columns in [0, ns).
__global__ __launch_bounds__(256) void k_remove_gather(const double *__restrict__ src, long long lda,
                                                       double *__restrict__ dst, long long ldn,
                                                       const int *__restrict__ keep_row, int mk,
                                                       const int *__restrict__ keep_col, int nk)
{
    for (int j = blockIdx.y; j < nk; j += gridDim.y) {
        const double *s = src + (long long)keep_col[j] * lda;
        double *t = dst + (long long)j * ldn;
        for (int i = blockIdx.x * blockDim.x + threadIdx.x; i < mk; i += gridDim.x * blockDim.x)
            t[i] = s[keep_row[i]];
    }
}

// Columns are 16-byte aligned on both sides (lda is a multiple of 16 doubles, column 0 starts an
// allocation): two rows per lane and trip, the last row of an odd m on its own.
// grid (row chunks, columns), block 256.
__global__ __launch_bounds__(256) void k_remove_columns(const double *__restrict__ src, long long lda,
                                                        double *__restrict__ dst, long long ldn, int m,
                                                        const int *__restrict__ keep_col, int nk)
{
    const int pairs = m >> 1;
    for (int j = blockIdx.y; j < nk; j += gridDim.y) {
        const double *s = src + (long long)keep_col[j] * lda;
        double *t = dst + (long long)j * ldn;
        const double2 *s2 = reinterpret_cast<const double2 *>(s);
        double2 *t2 = reinterpret_cast<double2 *>(t);
        for (int i = blockIdx.x * blockDim.x + threadIdx.x; i < pairs; i += gridDim.x * blockDim.x) t2[i] = s2[i];
        if ((m & 1) && blockIdx.x == 0 && threadIdx.x == 0) t[m - 1] = s[m - 1];
    }
}

// keep_row == nullptr: every one of the m rows is kept (mk == m)
void dzg_launch_remove_gather(const double *src, long long lda, double *dst, long long ldn, int m,
                              const int *keep_row, int mk, const int *keep_col, int nk, hipStream_t st)
{
    if (mk <= 0 || nk <= 0) return;
    const int by = nk < 65535 ? nk : 65535;
    if (!keep_row) {
        int bx = ((m >> 1) + 255) / 256;
        if (bx < 1) bx = 1;
        if (bx > 64) bx = 64;
        hipLaunchKernelGGL(k_remove_columns, dim3((unsigned)bx, (unsigned)by), dim3(256), 0, st, src, lda, dst, ldn,
                           m, keep_col, nk);
        return;
    }
    int bx = (mk + 255) / 256;
    if (bx > 64) bx = 64;
    hipLaunchKernelGGL(k_remove_gather, dim3((unsigned)bx, (unsigned)by), dim3(256), 0, st, src, lda, dst, ldn,
                       keep_row, mk, keep_col, nk);
}
