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
