// batch_restart.h -- the restart state of the LPs of a batch that start from a handed-in basis
// (k_batch_restart.hip), launched by k_batch.hip before the first round.  Semantics: DESIGN.md
// section 7k.
#pragma once

#include "batch_host.h"
#include "common.h"

// k_batch_restart reads the batch's own descriptors (DzgBatchLp, batch_host.h).  On entry basis /
// nonbasis hold the start's and x holds the right-hand side by constraint row; on exit x = B^-1 rhs,
// z = the fresh reduced costs of the nonbasic positions, xbar = zbar = 1.  status[id] is written only
// for an LP whose start is singular (DZG_SINGULAR).
struct DzgBatchRestartArgs {
    const DzgBatchLp *lp;
    const double *A;
    const int *var_col;
    const int *basis, *nonbasis;
    double *x, *xbar, *z, *zbar;
    const double *c; // objective coefficients by variable (at vc_off)
    int *status;
    int mmax; // largest m of the bucket: the LDS carve-up of batch_strict.h
};

// LPs list[0..n) of row bucket `bucket`, one workgroup each
void dzg_launch_batch_restart(int bucket, const DzgBatchRestartArgs &g, const int *list, int n, hipStream_t st);
