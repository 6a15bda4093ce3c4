// rays.h -- unboundedness and infeasibility rays from the final basis (k_rays.hip), shared by the
// batch (k_batch.hip) and the solver handle (engine.hip).  Definitions: DESIGN.md section 7f.
#pragma once

#include "common.h"
#include "duals.h"

// per LP: var, pos (exact in a double), mu, value, violation; var = -1: find_first_pivot found none
#define DZG_RAY_SCAL 5

struct DzgRaysArgs {
    const DzgBatchLp *lp;
    const double *A;
    const int *var_col;
    const int *basis, *nonbasis; // the final state of the batch
    const double *x, *xbar, *z, *zbar;
    const int *status;  // DZG_UNBOUNDED: primal ray, anything else: Farkas ray
    const double *c;    // objective coefficients by variable
    const double *rhs0; // the x every LP started with
    double *dz;         // the solve's scratch, q per LP
    double *d, *y, *scal;
    int mmax; // largest m of the bucket: the LDS carve-up of batch_strict.h
};

// LPs list[0..n) of row bucket `bucket`, one workgroup each
void dzg_launch_rays_small(int bucket, const DzgRaysArgs &g, const int *list, int n, hipStream_t st);

// out[r] = the right-hand side of the handle's solve, r < m: column `code` of A as the reference
// gathers it (stored entries only; code < 0: the unit column of row -1 - code), or, with A = nullptr,
// the unit vector of position `code`
void dzg_launch_ray_rhs(int m, const double *A, long long lda, int code, double *out, hipStream_t st);

// FAST, dense, one GPU, the eta file empty (Binv = Binv0), k = ncompact; M is the inverse as it is
// kept (m positions x m rows).  accumulate != 0 adds to the output instead of overwriting it.
// dx[p] (+)= (M h)_p
void dzg_launch_ray_dx_fast(const DzgDev &d, int k, const double *h, int accumulate, double *dx, hipStream_t st);
// v[r] (+)= (M^T w)_r
void dzg_launch_ray_vt_fast(const DzgDev &d, int k, const double *w, int accumulate, double *v, hipStream_t st);
// the residuals of one refinement step, accumulated in double-double:
// res[r] = h[r] - (B dx)_r   and   res[p] = unit(pos)[p] - (B^T y)_p  (with cvar, c by variable:
// res[p] = cvar[basis[p]] - (B^T y)_p, the residual of y = B^-T c_B; pos is not looked at)
void dzg_launch_ray_resid_dx(const DzgDev &d, const double *h, const double *dx, double *res, hipStream_t st);
void dzg_launch_ray_resid_v(const DzgDev &d, int pos, const double *y, double *res, hipStream_t st,
                            const double *cvar = nullptr);

// Workgroups of k_ray_finish = partial records it leaves; a record is DZG_RAY_PART doubles:
// max of max(vec, 0), 1.0 if the block met a NaN else 0.0, the block's share of the value's sum
#define DZG_RAY_BLOCKS 64
#define DZG_RAY_PART 4
// kind DZG_RAY_PRIMAL: vec = dx [m]; d[nonbasis[k]] = (k == pos), d[basis[p]] = -dx[p], sum of
//   c[basis[p]] * dx[p].   kind DZG_RAY_FARKAS: vec = dz [q]; d[nonbasis[k]] = -dz[k],
//   d[basis[p]] = (p == pos), sum of rhs0[p] * y[p].
void dzg_launch_ray_finish(int kind, int m, int q, int pos, const int *basis, const int *nonbasis,
                           const double *vec, const double *c, const double *rhs0, const double *y,
                           double *d, double *part, hipStream_t st);

// engine.hip: kind = 0, the scalars cleared (d / y are left alone)
void dzg_ray_none(dzg_ray *ry);
