// ranging.h -- sensitivity ranging at an optimal basis (k_ranging.hip), shared by the batch
// (k_batch.hip) and the solver handle (engine.hip).  Definitions: DESIGN.md section 7e.
#pragma once

#include <string>

#include "common.h"
#include "duals.h"

// One side's partial result over a share of the positions: the best candidate for lo (largest
// value, lowest position on ties) and for hi (smallest value, lowest position on ties).  A side
// without candidate has position DZG_RANGE_NONE; its value is then -inf / +inf.
struct DzgRangePart {
    double lo, hi;
    int lo_k, hi_k;
};
#define DZG_RANGE_NONE 0x7fffffff

// ---- batch route: one workgroup per (LP, direction)
struct DzgRangeItem {
    long long e0, e1; // the direction's entries in e_idx / e_val
    long long out;    // where its result goes in lo / hi / lo_var / hi_var
    int lp;
    int kind;         // 0: right-hand-side direction (e_idx: rows), 1: cost direction (variables)
};

struct DzgRangingArgs {
    const DzgBatchLp *lp;
    const double *A;
    const int *var_col;
    const int *basis, *nonbasis; // the final state of the batch
    const double *x;             // carried, by position
    const double *d;             // fresh reduced costs by variable (k_duals_small)
    const double *tol;           // per LP
    const DzgRangeItem *item;
    const int *e_idx;
    const double *e_val;
    double *lo, *hi;
    int *lo_var, *hi_var;
    int mmax; // largest m of the bucket: the LDS carve-up of batch_strict.h
};

// items[0..n) of row bucket `bucket`, one workgroup each
void dzg_launch_ranging_small(int bucket, const DzgRangingArgs &g, const DzgRangeItem *items, int n,
                              hipStream_t st);

#ifdef __HIPCC__
// ---- device: the candidate rule and its reductions, for every kernel that ranges (k_ranging.hip,
// k_batch_post.hip)

namespace dzg_rg {

__device__ __forceinline__ DzgRangePart range_none()
{
    DzgRangePart a;
    a.lo = -__builtin_inf();
    a.hi = __builtin_inf();
    a.lo_k = DZG_RANGE_NONE;
    a.hi_k = DZG_RANGE_NONE;
    return a;
}

__device__ __forceinline__ void range_take_lo(DzgRangePart &a, double r, int k)
{
    if (k == DZG_RANGE_NONE) return;
    if (a.lo_k == DZG_RANGE_NONE || r > a.lo || (r == a.lo && k < a.lo_k)) {
        a.lo = r;
        a.lo_k = k;
    }
}

__device__ __forceinline__ void range_take_hi(DzgRangePart &a, double r, int k)
{
    if (k == DZG_RANGE_NONE) return;
    if (a.hi_k == DZG_RANGE_NONE || r < a.hi || (r == a.hi && k < a.hi_k)) {
        a.hi = r;
        a.hi_k = k;
    }
}

__device__ __forceinline__ void range_merge(DzgRangePart &a, const DzgRangePart &b)
{
    range_take_lo(a, b.lo, b.lo_k);
    range_take_hi(a, b.hi, b.hi_k);
}

// the candidate rule for one position: one division, one negation
__device__ __forceinline__ void range_elem(DzgRangePart &a, double clamped, double delta, double tol, int k)
{
    if (!(fabs(delta) > tol)) return; // (a NaN delta is no candidate)
    const double r = -dzg_div(clamped, delta);
    if (delta > 0.0)
        range_take_lo(a, r, k);
    else
        range_take_hi(a, r, k);
}

__device__ __forceinline__ DzgRangePart range_shfl_xor(const DzgRangePart &a, int off)
{
    DzgRangePart o;
    o.lo = __shfl_xor(a.lo, off, DZG_WAVE);
    o.hi = __shfl_xor(a.hi, off, DZG_WAVE);
    o.lo_k = __shfl_xor(a.lo_k, off, DZG_WAVE);
    o.hi_k = __shfl_xor(a.hi_k, off, DZG_WAVE);
    return o;
}

// over the whole workgroup: a wave shuffle of (value, position), then across waves in wave order;
// thread 0 holds the result.  Every thread of the workgroup calls it.
template <int BLOCK>
__device__ DzgRangePart range_block(DzgRangePart a, DzgRangePart *s_red)
{
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) {
        const DzgRangePart o = range_shfl_xor(a, off);
        range_merge(a, o);
    }
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    if (lane == 0) s_red[wave] = a;
    __syncthreads();
    if (threadIdx.x == 0)
        for (int w = 1; w < BLOCK / 64; ++w) range_merge(a, s_red[w]);
    return a;
}

// the value direction [e0, e1) holds for index `want`, 0.0 if it has none (indices are distinct)
__device__ __forceinline__ double dir_value(const int *e_idx, const double *e_val, long long e0, long long e1,
                                            int want)
{
    double v = 0.0;
    for (long long e = e0; e < e1; ++e)
        if (e_idx[e] == want) v = e_val[e];
    return v;
}

} // namespace dzg_rg
#endif // __HIPCC__

// ---- STRICT handle: the ratio test over one vector of deltas, DZG_RANGE_BLOCKS partial records
#define DZG_RANGE_BLOCKS 64
// delta_k = sub ? -src[k] - sub[k] : src[k];  clamped_k = max(idx ? val[idx[k]] : val[k], 0.0)
void dzg_launch_range_ratio(int n, const double *src, const double *sub, const double *val, const int *idx,
                            double tol, DzgRangePart *part, hipStream_t st);
// ndirs results from ndirs x ntiles partial records, tiles in order; positions, not variables
// (no candidate: -1, lo = -inf, hi = +inf)
void dzg_launch_range_finish(const DzgRangePart *part, int ntiles, int ndirs, double *lo, double *hi,
                             int *lo_k, int *hi_k, hipStream_t st);

// ---- FAST handle (dense, one GPU, the eta file empty: Binv = Binv0)
// Directions of one launch at most, and what the scratch buffers are sized by
#define DZG_RANGE_CHUNK 256
// Directions in CSR over device arrays.  Right-hand-side directions: rows.  Cost directions come
// split by the host: the basic entries as basis positions, the nonbasic ones as nonbasic positions.
struct DzgRangeDirs {
    const long long *ptr;
    const int *idx;
    const double *val;
};
inline int dzg_range_row_tiles(int m) { return (m + 255) / 256; }
inline int dzg_range_col_tiles(int q) { return (q + 63) / 64; }
inline int dzg_range_ldy(int m) { return (m + 63) / 64 * 64; }
// delta_x = B^-1 h for directions [dir0, dir0 + ndirs) and the ratio test against the carried x:
// part[ndirs x dzg_range_row_tiles(m)]
void dzg_launch_range_rhs_fast(const DzgDev &d, int k, DzgRangeDirs h, int dir0, int ndirs, double tol,
                               DzgRangePart *part, hipStream_t st);
// Y[ndirs x ldy] = rows of B^-T g_B, zero padded; GN[ndirs x q] = g by nonbasic position
void dzg_launch_range_cost_y(const DzgDev &d, int k, DzgRangeDirs gb, DzgRangeDirs gn, int dir0, int ndirs,
                             double *Y, double *GN, hipStream_t st);
// delta_D = Y A_N - GN on the fp64 matrix cores, the ratio test against max(dvar[nonbasis[k]], 0)
// in the epilogue: part[ndirs x dzg_range_col_tiles(q)]
void dzg_launch_range_cost_mfma(const DzgDev &d, const double *dvar, const double *Y, const double *GN,
                                int ndirs, double tol, DzgRangePart *part, hipStream_t st);

// ---- host (engine.hip)
// A well-formed request for an LP of m rows and n variables?  (why: what is wrong)
bool dzg_ranging_req_valid(const dzg_ranging_req *req, int64_t m, int64_t n, std::string &why);
// NaN ranges, *_var = -1
void dzg_ranging_none(const dzg_ranging_req *req, dzg_ranging *rg);
