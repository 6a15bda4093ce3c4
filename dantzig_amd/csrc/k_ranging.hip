// k_ranging.hip -- sensitivity ranging at an OPTIMAL basis: how far a cost direction g or a
// right-hand-side direction h can be followed before the basis stops being optimal (DESIGN.md
// section 7e).
//
//      cost:  Y = B^-T g_B,   delta_k = a_j . Y - g_j   (j at nonbasic position k),  against dc_j
//      rhs:   delta_p = (B^-1 h)_p                      (basis position p),          against xc_p
//      candidate when |delta| > pivot_tol:  r = -(clamped / delta);  delta > 0 bounds lo (largest
//      r wins), delta < 0 bounds hi (smallest r wins), the lowest position on ties.
//
// k_ranging_small: one workgroup per (LP, direction) of a batch, in the reference's arithmetic: the
// gather and LU of batch_strict.h with the direction in the place of the right-hand side, for a
// cost direction solve_dz's neg_t_dot loop as k_duals_small has it.
// k_range_ratio / k_range_finish: the tail of the STRICT handle's path, where delta came from
// dzg_launch_strict_solve (and a sequential pricing pass); the same arithmetic per element, so the
// two routes agree bit for bit.
// k_range_rhs_fast, k_range_cost_y, k_range_cost_mfma: a FAST handle right after the
// refactorisation of its final basis.  The cost directions of a chunk are one product
// delta_D = Y A_N - G_N on the fp64 matrix cores whose result is never stored: the epilogue runs the
// ratio test on the accumulators and leaves one partial record per (direction, column tile).
//
// The order (value, position) is total over the positions, so every grouping of the reduction ends
// on the same record; partial records are still finished in tile order, and there are no atomics:
// two calls on one state give the same bits.
#include "batch_strict.h"
#include "ranging.h"

typedef double double4_t __attribute__((ext_vector_type(4)));

namespace {

using namespace dzg_rg; // ranging.h: the candidate rule and its reductions

template <int BLOCK>
__global__ __launch_bounds__(BLOCK) void k_ranging_small(DzgRangingArgs g, const DzgRangeItem *__restrict__ items)
{
    extern __shared__ __attribute__((aligned(16))) double s_mem[];
    __shared__ DzgRangePart s_red[4];
    const DzgRangeItem it = items[blockIdx.x];
    const DzgBatchLp L = g.lp[it.lp];
    const int m = L.m, q = L.n - L.m, ld = m + 1;
    const double *A = g.A + L.a_off;
    const int *var_col = g.var_col + L.vc_off;
    const int *basis = g.basis + L.m_off, *nonbasis = g.nonbasis + L.q_off;
    const double *x = g.x + L.m_off, *d = g.d + L.vc_off;
    const double tol = g.tol[it.lp];
    // the carve-up of strict_steps: W, dx, v, one int
    double *W = s_mem;
    double *v = s_mem + (long long)g.mmax * (g.mmax + 1) + g.mmax;
    int *s_flag = (int *)(v + g.mmax);

    DzgRangePart me = range_none();
    if (it.kind == 0) {
        // ---- B delta_x = h: the gather's right-hand side is overwritten with the dense h by the
        // thread that wrote it (same row -> thread map)
        dzg_bs::gather<BLOCK>(W, m, A, basis, var_col, 0, m > 0 ? basis[0] : 0, -1);
        for (int r = threadIdx.x; r < m; r += BLOCK) W[r * ld + m] = dir_value(g.e_idx, g.e_val, it.e0, it.e1, r);
        dzg_bs::lu_solve_lds<BLOCK>(W, m, s_flag);
        for (int p = threadIdx.x; p < m; p += BLOCK) range_elem(me, fmax(x[p], 0.0), W[p * ld + m], tol, p);
    } else {
        // ---- B^T Y = g_B, then delta_k = -neg_t_dot(nonbasis, Y)_k - g[nonbasis[k]] (solve_dz's loop)
        dzg_bs::gather<BLOCK>(W, m, A, basis, var_col, 1, -1, -1);
        for (int r = threadIdx.x; r < m; r += BLOCK)
            W[r * ld + m] = dir_value(g.e_idx, g.e_val, it.e0, it.e1, basis[r]);
        dzg_bs::lu_solve_lds<BLOCK>(W, m, s_flag);
        for (int r = threadIdx.x; r < m; r += BLOCK) v[r] = W[r * ld + m];
        __syncthreads();
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
            const double delta = -acc - dir_value(g.e_idx, g.e_val, it.e0, it.e1, var);
            range_elem(me, fmax(d[var], 0.0), delta, tol, k);
        }
    }
    me = range_block<BLOCK>(me, s_red);
    if (threadIdx.x == 0) {
        const int *at = it.kind == 0 ? basis : nonbasis;
        g.lo[it.out] = me.lo;
        g.hi[it.out] = me.hi;
        g.lo_var[it.out] = me.lo_k == DZG_RANGE_NONE ? -1 : at[me.lo_k];
        g.hi_var[it.out] = me.hi_k == DZG_RANGE_NONE ? -1 : at[me.hi_k];
    }
}

__global__ __launch_bounds__(256) void k_range_ratio(int n, const double *__restrict__ src,
                                                     const double *__restrict__ sub,
                                                     const double *__restrict__ val,
                                                     const int *__restrict__ idx, double tol,
                                                     DzgRangePart *__restrict__ part)
{
    __shared__ DzgRangePart s_red[4];
    DzgRangePart me = range_none();
    for (int k = blockIdx.x * blockDim.x + threadIdx.x; k < n; k += gridDim.x * blockDim.x) {
        const double delta = sub ? -src[k] - sub[k] : src[k];
        range_elem(me, fmax(idx ? val[idx[k]] : val[k], 0.0), delta, tol, k);
    }
    me = range_block<256>(me, s_red);
    if (threadIdx.x == 0) part[blockIdx.x] = me;
}

// one wave per direction: its partial records in tile order
__global__ __launch_bounds__(64) void k_range_finish(const DzgRangePart *__restrict__ part, int ntiles,
                                                     int ndirs, double *__restrict__ lo,
                                                     double *__restrict__ hi, int *__restrict__ lo_k,
                                                     int *__restrict__ hi_k)
{
    const int dir = blockIdx.x;
    if (dir >= ndirs) return;
    DzgRangePart me = range_none();
    for (int t = threadIdx.x; t < ntiles; t += 64) range_merge(me, part[(long long)dir * ntiles + t]);
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) {
        const DzgRangePart o = range_shfl_xor(me, off);
        range_merge(me, o);
    }
    if (threadIdx.x == 0) {
        lo[dir] = me.lo;
        hi[dir] = me.hi;
        lo_k[dir] = me.lo_k == DZG_RANGE_NONE ? -1 : me.lo_k;
        hi_k[dir] = me.hi_k == DZG_RANGE_NONE ? -1 : me.hi_k;
    }
}

// ---- FAST ---------------------------------------------------------------------------------
// delta_x[p] = sum over the direction's rows r in R of h_r Binv0[p][dslot[r]], entries in order,
// plus h at the row whose slack sits at position p (that column of the inverse is e_p).
// grid (row tiles of 256, directions)
__global__ __launch_bounds__(256) void k_range_rhs_fast(const DzgDev d, int k, DzgRangeDirs h, int dir0,
                                                        double tol, DzgRangePart *__restrict__ part)
{
    __shared__ DzgRangePart s_red[4];
    const int p = blockIdx.x * 256 + threadIdx.x;
    const int dl = blockIdx.y;
    const long long e0 = h.ptr[dir0 + dl], e1 = h.ptr[dir0 + dl + 1];
    DzgRangePart me = range_none();
    if (p < d.m) {
        const double *row = d.binv + (long long)p * d.ldb;
        const int bc = d.bcode[p];
        double acc = 0.0, unit = 0.0;
        for (long long e = e0; e < e1; ++e) {
            const int r = h.idx[e];
            const int c = d.dslot[r];
            if (c >= 0 && c < k) acc = fma(h.val[e], row[c], acc);
            if (bc == -1 - r) unit = h.val[e];
        }
        range_elem(me, fmax(d.x[p], 0.0), acc + unit, tol, p);
    }
    me = range_block<256>(me, s_red);
    if (threadIdx.x == 0) part[(long long)dl * gridDim.x + blockIdx.x] = me;
}

// Y[dl][r] = sum over the direction's basic entries (position p, value) of value Binv0[p][dslot[r]]
// for a row of R, the value at the position of row r's slack otherwise; zero for r >= m.  The
// threads of the first workgroup of a direction scatter its nonbasic entries into GN (zeroed by
// the caller).  grid (ldy / 256 rounded up, directions)
__global__ __launch_bounds__(256) void k_range_cost_y(const DzgDev d, int k, DzgRangeDirs gb, DzgRangeDirs gn,
                                                      int dir0, int ldy, double *__restrict__ Y,
                                                      double *__restrict__ GN)
{
    const int r = blockIdx.x * 256 + threadIdx.x;
    const int dl = blockIdx.y;
    if (blockIdx.x == 0)
        for (long long e = gn.ptr[dir0 + dl] + threadIdx.x; e < gn.ptr[dir0 + dl + 1]; e += 256)
            GN[(long long)dl * d.q + gn.idx[e]] = gn.val[e];
    if (r >= ldy) return;
    double acc = 0.0;
    if (r < d.m) {
        const long long e0 = gb.ptr[dir0 + dl], e1 = gb.ptr[dir0 + dl + 1];
        const int c = d.dslot[r];
        if (c >= 0 && c < k) {
            for (long long e = e0; e < e1; ++e)
                acc = fma(gb.val[e], d.binv[(long long)gb.idx[e] * d.ldb + c], acc);
        } else {
            for (long long e = e0; e < e1; ++e)
                if (d.bcode[gb.idx[e]] == -1 - r) acc = gb.val[e];
        }
    }
    Y[(long long)dl * ldy + r] = acc;
}

// delta_D = Y A_N - G_N, one workgroup per (64 nonbasic positions, 32 directions), and the ratio
// test in the epilogue.  Wave w owns positions c0 + 16 w .. + 15 for all 32 directions: two
// 16 x 16 MFMA tiles (8 accumulator VGPR pairs).  K runs over the constraint rows in tiles of 64:
// Y's tile goes through LDS once for the four waves, A's column is K-contiguous in memory (column
// major), so a lane reads 16 consecutive rows of its column per tile: within a tile lane group lk
// takes rows 16 lk .. 16 lk + 15, one per MFMA step -- both operands use the same assignment of
// rows to the instruction's k slots, which is all the product needs.
// Lane maps as at k_ref_gemm_lds (k_refactor.hip): A[i = l&15][k = l>>4], B[k = l>>4][j = l&15],
// D[row = (l>>4) + 4 reg][col = l&15]; here i = direction, j = nonbasic position.
// A slack at a nonbasic position has no column in A: its delta is Y[dir][row] - g, read beside the
// product.  Rows m .. ldy-1 of Y are zero and rows >= m of A are not read.
#define RC_DIRS 32
#define RC_KT 64
#define RC_LD (RC_KT + 2)
__global__ __launch_bounds__(256) void k_range_cost_mfma(int m, int q, int ldy, long long lda,
                                                         const double *__restrict__ A,
                                                         const int *__restrict__ nbcode,
                                                         const int *__restrict__ nonbasis,
                                                         const double *__restrict__ dvar,
                                                         const double *__restrict__ Y,
                                                         const double *__restrict__ GN, int ndirs,
                                                         double tol, DzgRangePart *__restrict__ part)
{
    __shared__ double s_y[RC_DIRS][RC_LD];
    __shared__ DzgRangePart s_part[4][RC_DIRS];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int li = lane & 15, lk = lane >> 4;
    const int d0 = blockIdx.y * RC_DIRS;
    const int kpos = blockIdx.x * 64 + 16 * wave + li;
    const int code = kpos < q ? nbcode[kpos] : -1;
    const bool dense = kpos < q && code >= 0;
    const double *col = A + (long long)(dense ? code : 0) * lda;
    double4_t acc[2];
#pragma unroll
    for (int t = 0; t < 2; ++t)
#pragma unroll
        for (int g = 0; g < 4; ++g) acc[t][g] = 0.0;

    for (int k0 = 0; k0 < ldy; k0 += RC_KT) {
        __syncthreads(); // the previous tile has been consumed
        for (int e = threadIdx.x; e < RC_DIRS * RC_KT; e += 256) {
            const int dr = e / RC_KT, kk = e % RC_KT;
            s_y[dr][kk] = d0 + dr < ndirs ? Y[(long long)(d0 + dr) * ldy + k0 + kk] : 0.0;
        }
        __syncthreads();
        const int r0 = k0 + 16 * lk;
        // (the branch is uniform over the workgroup: an MFMA takes its operands from every lane of
        // the wave whatever EXEC says, so it must never sit in divergent control flow)
        if (k0 + RC_KT <= m) { // whole tile inside the matrix: no per-row test
#pragma unroll
            for (int s = 0; s < 16; ++s) {
                const double b = dense ? col[r0 + s] : 0.0;
                acc[0] = __builtin_amdgcn_mfma_f64_16x16x4f64(s_y[li][16 * lk + s], b, acc[0], 0, 0, 0);
                acc[1] = __builtin_amdgcn_mfma_f64_16x16x4f64(s_y[16 + li][16 * lk + s], b, acc[1], 0, 0, 0);
            }
        } else {
#pragma unroll
            for (int s = 0; s < 16; ++s) {
                const double b = (dense && r0 + s < m) ? col[r0 + s] : 0.0;
                acc[0] = __builtin_amdgcn_mfma_f64_16x16x4f64(s_y[li][16 * lk + s], b, acc[0], 0, 0, 0);
                acc[1] = __builtin_amdgcn_mfma_f64_16x16x4f64(s_y[16 + li][16 * lk + s], b, acc[1], 0, 0, 0);
            }
        }
    }

    // ---- epilogue: this lane holds delta for direction d0 + 16 t + lk + 4 g at position kpos
    const double dc = kpos < q ? fmax(dvar[nonbasis[kpos]], 0.0) : 0.0;
#pragma unroll
    for (int t = 0; t < 2; ++t) {
#pragma unroll
        for (int g = 0; g < 4; ++g) {
            const int dl = 16 * t + lk + 4 * g;
            DzgRangePart me = range_none();
            if (d0 + dl < ndirs && kpos < q) {
                const double ay = dense ? acc[t][g] : Y[(long long)(d0 + dl) * ldy + (-1 - code)];
                const double delta = ay - GN[(long long)(d0 + dl) * q + kpos];
                range_elem(me, dc, delta, tol, kpos);
            }
#pragma unroll
            for (int off = 8; off > 0; off >>= 1) { // the 16 lanes that share lk
                const DzgRangePart o = range_shfl_xor(me, off);
                range_merge(me, o);
            }
            if (li == 0) s_part[wave][dl] = me;
        }
    }
    __syncthreads();
    if (threadIdx.x < RC_DIRS && d0 + (int)threadIdx.x < ndirs) {
        DzgRangePart me = s_part[0][threadIdx.x];
        for (int w = 1; w < 4; ++w) range_merge(me, s_part[w][threadIdx.x]); // wave order
        part[(long long)(d0 + threadIdx.x) * gridDim.x + blockIdx.x] = me;
    }
}

} // namespace

void dzg_launch_ranging_small(int bucket, const DzgRangingArgs &g, const DzgRangeItem *items, int n,
                              hipStream_t st)
{
    const size_t lds = dzg_bs::lds_bytes(g.mmax);
    dzg_bh::for_each_chunk(bucket, n, [&](int c0, int grid) {
        dzg_bh::with_block(bucket, [&](auto block) {
            constexpr int BLOCK = decltype(block)::value;
            hipLaunchKernelGGL(k_ranging_small<BLOCK>, dim3(grid), dim3(BLOCK), lds, st, g, items + c0);
        });
    });
}

void dzg_launch_range_ratio(int n, const double *src, const double *sub, const double *val, const int *idx,
                            double tol, DzgRangePart *part, hipStream_t st)
{
    hipLaunchKernelGGL(k_range_ratio, dim3(DZG_RANGE_BLOCKS), dim3(256), 0, st, n, src, sub, val, idx, tol,
                       part);
}

void dzg_launch_range_finish(const DzgRangePart *part, int ntiles, int ndirs, double *lo, double *hi,
                             int *lo_k, int *hi_k, hipStream_t st)
{
    if (ndirs <= 0) return;
    hipLaunchKernelGGL(k_range_finish, dim3(ndirs), dim3(64), 0, st, part, ntiles, ndirs, lo, hi, lo_k, hi_k);
}

void dzg_launch_range_rhs_fast(const DzgDev &d, int k, DzgRangeDirs h, int dir0, int ndirs, double tol,
                               DzgRangePart *part, hipStream_t st)
{
    if (ndirs <= 0 || d.m <= 0) return;
    hipLaunchKernelGGL(k_range_rhs_fast, dim3(dzg_range_row_tiles(d.m), ndirs), dim3(256), 0, st, d, k, h,
                       dir0, tol, part);
}

void dzg_launch_range_cost_y(const DzgDev &d, int k, DzgRangeDirs gb, DzgRangeDirs gn, int dir0, int ndirs,
                             double *Y, double *GN, hipStream_t st)
{
    if (ndirs <= 0) return;
    const int ldy = dzg_range_ldy(d.m);
    const int gx = ldy > 0 ? (ldy + 255) / 256 : 1;
    hipLaunchKernelGGL(k_range_cost_y, dim3(gx, ndirs), dim3(256), 0, st, d, k, gb, gn, dir0, ldy, Y, GN);
}

void dzg_launch_range_cost_mfma(const DzgDev &d, const double *dvar, const double *Y, const double *GN,
                                int ndirs, double tol, DzgRangePart *part, hipStream_t st)
{
    if (ndirs <= 0 || d.q <= 0) return;
    hipLaunchKernelGGL(k_range_cost_mfma, dim3(dzg_range_col_tiles(d.q), (ndirs + RC_DIRS - 1) / RC_DIRS),
                       dim3(256), 0, st, d.m, d.q, dzg_range_ldy(d.m), d.lda, d.A, d.nbcode, d.nonbasis, dvar,
                       Y, GN, ndirs, tol, part);
}
