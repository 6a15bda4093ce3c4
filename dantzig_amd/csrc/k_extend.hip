// k_extend.hip -- the constraint matrix of a live solver grown on the device (dzg_solver_extend).
//
// dzg_solver_extend appends p rows and r structural columns to the LP a handle holds.  The m x n_s
// block that is already resident never crosses PCIe again: it is copied device to device into the
// successor's matrix, whose leading dimension follows dzg_solver_create's rule for m' = m + p rows and
// may therefore differ from the old one.  Only the new numbers travel: the p x n_s row block (staged
// row-major, as the caller holds it) and the m' x r column block (dzg_solver_upload_columns' path).
//
//      k_extend_restride   old block, column-major lda -> column-major lda'; rows m..m'-1 of those
//                          columns are left to the next kernel (the allocation starts zeroed)
//      k_extend_rows       staged p x n_s row-major block -> rows m..m'-1 of the column-major matrix:
//                          the transpose of k_transpose_to_rows (k_price_kernels.h) run the other way,
//                          32 x 32 tiles through LDS; -0.0 is stored as +0.0 like every other entry of
//                          the matrix
//
// No atomics, one writer per entry.
#include "common.h"

// Columns are 16-byte aligned on both sides (lda and lda' are multiples of 16 doubles, column 0 starts
// an allocation): two rows per lane and trip, the last row of an odd m on its own.
// grid (row chunks, columns), block 256.
__global__ __launch_bounds__(256) void k_extend_restride(const double *__restrict__ src, long long lda,
                                                         double *__restrict__ dst, long long ldn, int m,
                                                         int ncols)
{
    const int pairs = m >> 1;
    for (int j = blockIdx.y; j < ncols; j += gridDim.y) {
        const double *s = src + (long long)j * lda;
        double *t = dst + (long long)j * ldn;
        const double2 *s2 = reinterpret_cast<const double2 *>(s);
        double2 *t2 = reinterpret_cast<double2 *>(t);
        for (int i = blockIdx.x * blockDim.x + threadIdx.x; i < pairs; i += gridDim.x * blockDim.x) t2[i] = s2[i];
        if ((m & 1) && blockIdx.x == 0 && threadIdx.x == 0) t[m - 1] = s[m - 1];
    }
}

// rows: p x ns row-major (ldr); A: column-major (lda), the block lands in rows row0..row0+p-1.
// grid (ceil(ns / 32), ceil(p / 32)), block (32, 8).  The tile is padded by one double: the
// transposed read walks it with a stride of 33 doubles, two lanes per pair of banks.
__global__ __launch_bounds__(256) void k_extend_rows(const double *__restrict__ rows, long long ldr, int p,
                                                     int ns, double *__restrict__ A, long long lda, int row0)
{
    __shared__ double tile[32][33];
    const int j0 = blockIdx.x * 32, i0 = blockIdx.y * 32;
    for (int ii = threadIdx.y; ii < 32; ii += 8) {
        const int i = i0 + ii, j = j0 + threadIdx.x;
        double v = 0.0;
        if (i < p && j < ns) v = rows[(long long)i * ldr + j];
        tile[ii][threadIdx.x] = v == 0.0 ? 0.0 : v; // (-0.0 -> +0.0)
    }
    __syncthreads();
    for (int jj = threadIdx.y; jj < 32; jj += 8) {
        const int j = j0 + jj, i = i0 + threadIdx.x;
        if (j < ns && i < p) A[(long long)j * lda + row0 + i] = tile[threadIdx.x][jj];
    }
}

void dzg_launch_extend_restride(const double *src, long long lda, double *dst, long long ldn, int m, int ncols,
                                hipStream_t st)
{
    if (m <= 0 || ncols <= 0) return;
    int bx = ((m >> 1) + 255) / 256;
    if (bx < 1) bx = 1;
    if (bx > 64) bx = 64;
    const int by = ncols < 65535 ? ncols : 65535;
    hipLaunchKernelGGL(k_extend_restride, dim3((unsigned)bx, (unsigned)by), dim3(256), 0, st, src, lda, dst, ldn,
                       m, ncols);
}

void dzg_launch_extend_rows(const double *rows, long long ldr, int p, int ns, double *A, long long lda, int row0,
                            hipStream_t st)
{
    if (p <= 0 || ns <= 0) return;
    hipLaunchKernelGGL(k_extend_rows, dim3((unsigned)((ns + 31) / 32), (unsigned)((p + 31) / 32)), dim3(32, 8), 0,
                       st, rows, ldr, p, ns, A, lda, row0);
}
