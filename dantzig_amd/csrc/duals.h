// duals.h -- dual values and reduced costs at an optimal basis (k_duals.hip), shared by the batch
// (k_batch.hip) and the solver handle (engine.hip).  Definitions: DESIGN.md section 7d.
#pragma once

#include "batch_host.h"
#include "common.h"

// k_duals_small reads the batch's own descriptors (DzgBatchLp, batch_host.h): c, d are indexed by
// variable (n entries, at vc_off like var_col); rhs0, y by row (at m_off).

// per LP: dual_obj, primal_infeas, dual_infeas, max |z - d_N|, max |d_N|
#define DZG_DUALS_SCAL 5

struct DzgDualsArgs {
    const DzgBatchLp *lp;
    const double *A;
    const int *var_col;
    const int *basis, *nonbasis; // the final state of the batch
    const double *x, *z;
    const double *c;    // objective coefficients by variable
    const double *rhs0; // the x every LP started with
    double *y, *d, *scal;
    int mmax; // largest m of the bucket: the LDS carve-up of batch_strict.h
};

// LPs list[0..n) of row bucket `bucket`, one workgroup each
void dzg_launch_duals_small(int bucket, const DzgDualsArgs &g, const int *list, int n, hipStream_t st);

// Workgroups of k_duals_finish = partial records it leaves; a record is DZG_DUALS_PART doubles:
// min d_N, max |d_N|, max |z - d_N|, min x, the block's share of rhs0 . y
#define DZG_DUALS_BLOCKS 64
#define DZG_DUALS_PART 8
// d[nonbasis[k]] = -dzy[k] - c[nonbasis[k]], d[basis[p]] = 0, and the partial records
void dzg_launch_duals_finish(int m, int q, const int *basis, const int *nonbasis, const double *c,
                             const double *dzy, const double *z, const double *x, const double *rhs0,
                             const double *y, double *d, double *part, hipStream_t st);

// k_drift.hip: y = B^-T c_B from the compact inverse of a FAST solver whose eta file is empty, in
// the two deterministic stages of the drift measurement.  part [chunks x ldw], y [m + 2].
void dzg_launch_drift_y(const DzgDev &d, const double *cdev, double *part, double *y, int k_bound,
                        hipStream_t st);

// engine.hip: source = 0, primal_obj = objective, the other scalars 0 (y / d are left alone)
void dzg_duals_none(dzg_duals *du, double objective);
