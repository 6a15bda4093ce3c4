// batch_strict.h -- the STRICT simplex loop of one LP run by one workgroup, shared by k_batch.hip
// (a batch of independent LPs) and k_mip.hip (branch-and-bound node LPs).  The arithmetic and the
// operation order are described at the top of k_batch.hip; both kernels run exactly this code, so
// a node LP gives what the same LP gives through dzg_batch_solve, bit for bit.
//
// The host side of both (buckets, launches, rounds) is batch_host.h.
//
// LDS carve-up (lds_bytes(mmax)): W = mmax x (mmax + 1) doubles, then dx[mmax], v[mmax], one int.
#pragma once

#include "common.h"

namespace dzg_bs {

// B (transposed == 0: W[r][c] = A[r, basis[c]]) or B^T (W[r][c] = A[c, basis[r]]) into LDS, row
// stride ld = m + 1, the right-hand side into column m: the entering column (transposed == 0) or
// unit(pos).  Stored entries only: the reference's basis matrix is a CSC densified into zeros, so an
// explicit -0.0 of A arrives as +0.0 (oracle gather_basis / column_of).
template <int BLOCK>
__device__ void gather(double *W, int m, const double *A, const int *basis, const int *var_col,
                       int transposed, int enter_var, int pos)
{
    const int ld = m + 1;
    for (int e = threadIdx.x; e < m * m; e += BLOCK) {
        const int c = e / m, r = e - c * m; // basis position c, constraint row r
        const int code = var_col[basis[c]];
        double v;
        if (code >= 0) {
            v = A[(long long)code * m + r];
            v = v != 0.0 ? v : 0.0;
        } else {
            v = (-1 - code) == r ? 1.0 : 0.0;
        }
        if (transposed)
            W[c * ld + r] = v;
        else
            W[r * ld + c] = v;
    }
    for (int r = threadIdx.x; r < m; r += BLOCK) {
        double v;
        if (transposed) {
            v = r == pos ? 1.0 : 0.0;
        } else {
            const int code = var_col[enter_var];
            if (code >= 0) {
                v = A[(long long)code * m + r];
                v = v != 0.0 ? v : 0.0;
            } else {
                v = (-1 - code) == r ? 1.0 : 0.0;
            }
        }
        W[r * ld + m] = v;
    }
}

// first maximum of |.|: larger value wins, lower row on ties; NaN never wins (x > NaN is false)
__device__ __forceinline__ DzgCand abs_cand(double value, int row)
{
    DzgCand c;
    c.r = fabs(value);
    c.k = (c.r == c.r) ? row : -1;
    return c;
}

// Matrix::factorize + LU::solve (src/linalg.rs:88-128, 282-299) of the gathered system in place;
// the solution ends in column m.  Starts and ends with the buffer consistent for every thread.
template <int BLOCK>
__device__ void lu_solve_lds(double *W, int m, int *s_flag)
{
    const int ld = m + 1;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    __syncthreads(); // the gather is complete
    for (int k = 0; k + 1 < m; ++k) {
        if (wave == 0) {
            DzgCand best;
            best.r = 0.0;
            best.k = -1;
            for (int r = k + lane; r < m; r += 64) best = dzg_better(best, abs_cand(W[r * ld + k], r));
            best = dzg_wave_best(best);
            const double akk = W[k * ld + k];
            // `x > NaN` is never true: a NaN at (k,k) keeps mu = k (src/linalg.rs:98-105)
            const int mu = (fabs(akk) != fabs(akk) || best.k < 0) ? k : best.k;
            if (mu != k) { // swap rows k and mu on columns >= k, the right-hand side included
                for (int j = k + lane; j <= m; j += 64) {
                    const double a = W[k * ld + j];
                    W[k * ld + j] = W[mu * ld + j];
                    W[mu * ld + j] = a;
                }
            }
            __builtin_amdgcn_wave_barrier();
            const double pivot = W[k * ld + k];
            const bool zero = !(pivot != 0.0); // src/linalg.rs:117 (NaN is "nonzero")
            // zero pivot: no scaling, no update of the matrix; LU::solve still runs
            // b[i] -= b[k] * a(i,k) with the stored entry (src/linalg.rs:288-290)
            if (!zero)
                for (int r = k + 1 + lane; r < m; r += 64) W[r * ld + k] = dzg_div(W[r * ld + k], pivot);
            if (lane == 0) *s_flag = zero ? 1 : 0;
        }
        __syncthreads();
        const bool zero = *s_flag != 0;
        const int ncols = m - k; // columns k+1 .. m (m: the right-hand side)
        const int total = (m - 1 - k) * ncols;
        for (int e = threadIdx.x; e < total; e += BLOCK) {
            const int i = k + 1 + e / ncols;
            const int j = k + 1 + e % ncols;
            if (zero && j < m) continue;
            const double adjustment = W[i * ld + k] * W[k * ld + j];
            W[i * ld + j] = W[i * ld + j] - adjustment;
        }
        __syncthreads();
    }
    if (wave == 0) { // back substitution, src/linalg.rs:292-297: j ascending inside each row
        for (int i = m - 1; i >= 0; --i) {
            const int j0 = i + 1 + lane, j1 = j0 + 64;
            const double p0 = j0 < m ? W[i * ld + j0] * W[j0 * ld + m] : 0.0;
            const double p1 = j1 < m ? W[i * ld + j1] * W[j1 * ld + m] : 0.0;
            double t = W[i * ld + m];
            const int nj = m - 1 - i;
            for (int s = 0; s < nj; ++s) {
                const double prod = s < 64 ? dzg_readlane_f64(p0, s) : dzg_readlane_f64(p1, s - 64);
                t = t - prod;
            }
            t = dzg_div(t, W[i * ld + i]);
            if (lane == 0) W[i * ld + m] = t;
            __builtin_amdgcn_wave_barrier();
        }
    }
    __syncthreads();
}

template <int BLOCK>
__device__ void solve_dx(const double *A, const int *var_col, int m, double *W, double *dx,
                         int *s_flag, const int *basis, int enter_var)
{
    gather<BLOCK>(W, m, A, basis, var_col, 0, enter_var, -1);
    lu_solve_lds<BLOCK>(W, m, s_flag);
    for (int r = threadIdx.x; r < m; r += BLOCK) dx[r] = W[r * (m + 1) + m];
    __syncthreads();
}

// v = B^-T e_pos, then dz = collect_columns(nonbasis).neg_t_dot(v) into global memory
template <int BLOCK>
__device__ void solve_dz(const double *A, const int *var_col, int m, int q, double *W, double *v,
                         int *s_flag, const int *basis, const int *nonbasis, double *dz, int pos)
{
    gather<BLOCK>(W, m, A, basis, var_col, 1, -1, pos);
    lu_solve_lds<BLOCK>(W, m, s_flag);
    for (int r = threadIdx.x; r < m; r += BLOCK) v[r] = W[r * (m + 1) + m];
    __syncthreads();
    for (int k = threadIdx.x; k < q; k += BLOCK) {
        const int code = var_col[nonbasis[k]];
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
        dz[k] = acc;
    }
    __syncthreads();
}

// One LP's state in global memory (basis, x, xbar: m; nonbasis, z, zbar, dz: q = n - m) and its
// optional pivot log (log_cap entries, indexed by iteration).
struct LpState {
    const double *A;    // m x ns column-major, lda = m
    const int *var_col; // n
    int m, q;
    int *basis, *nonbasis;
    double *x, *xbar, *z, *zbar, *dz;
    int *log_kind, *log_enter, *log_leave;
    double *log_mu;
    long long log_cap;
};

// At most `ppl` iterations of Simplex::solve (src/simplex.rs:332-343) from the state in S; `it`
// counts iterations across calls.  Returns the LP's status, DZG_RUNNING if the budget ran out.
// Every thread of the workgroup calls it and gets the same result.
template <int BLOCK>
__device__ int strict_steps(const LpState &S, double *s_mem, int mmax, long long &it,
                            long long max_iter, double eps, int ppl)
{
    const int m = S.m, q = S.q;
    double *W = s_mem;                                  // mmax x (mmax + 1)
    double *dx = s_mem + (long long)mmax * (mmax + 1);  // mmax
    double *v = dx + mmax;                              // mmax
    int *s_flag = (int *)(v + mmax);
    int *basis = S.basis, *nonbasis = S.nonbasis;
    double *x = S.x, *xbar = S.xbar, *z = S.z, *zbar = S.zbar, *dz = S.dz;
    int status = DZG_RUNNING;

    for (int step = 0; step < ppl; ++step) {
        // ---- status(), src/simplex.rs:274-306
        const DzgCand cj = scan_first(z, zbar, q);
        const DzgCand ci = scan_first(x, xbar, m);
        int kind;
        double mu;
        if (cj.k >= 0 && ci.k >= 0) {
            const double primal = ci.r, dual = cj.r; // :280-281
            if (primal <= eps && dual <= eps) {
                status = DZG_OPTIMAL;
                break;
            }
            if (primal < dual) {
                kind = DZG_STEP_PRIMAL;
                mu = dual;
            } else {
                kind = DZG_STEP_DUAL;
                mu = primal;
            }
        } else if (cj.k >= 0) { // :294-298, no optimality test
            kind = DZG_STEP_PRIMAL;
            mu = cj.r;
        } else if (ci.k >= 0) { // :299-303
            kind = DZG_STEP_DUAL;
            mu = ci.r;
        } else {
            status = DZG_PANIC; // :304
            break;
        }
        if (it >= max_iter) {
            status = DZG_ITER_LIMIT;
            break;
        }
        if (m == 0) { // n - 1 underflow in Matrix::factorize: a reference panic path
            status = DZG_PANIC;
            break;
        }
        int p, r;
        if (kind == DZG_STEP_PRIMAL) { // :308-318
            r = cj.k;
            solve_dx<BLOCK>(S.A, S.var_col, m, W, dx, s_flag, basis, nonbasis[r]);
            p = scan_second(mu, x, xbar, dx, m).k;
            if (p < 0) {
                status = DZG_UNBOUNDED;
                break;
            }
            solve_dz<BLOCK>(S.A, S.var_col, m, q, W, v, s_flag, basis, nonbasis, dz, p);
        } else { // :320-330
            p = ci.k;
            solve_dz<BLOCK>(S.A, S.var_col, m, q, W, v, s_flag, basis, nonbasis, dz, p);
            r = scan_second(mu, z, zbar, dz, q).k;
            if (r < 0) {
                status = DZG_INFEASIBLE;
                break;
            }
            solve_dx<BLOCK>(S.A, S.var_col, m, W, dx, s_flag, basis, nonbasis[r]);
        }
        // ---- pivot, src/simplex.rs:253-268: step lengths, finiteness assert (:466)
        int ok = 1;
        const double t = dzg_safe_divide(x[p], dx[p], &ok);
        const double s = dzg_safe_divide(z[r], dz[r], &ok);
        const double tbar = dzg_safe_divide(xbar[p], dx[p], &ok);
        const double sbar = dzg_safe_divide(zbar[r], dz[r], &ok);
        if (!ok) {
            status = DZG_PANIC; // the pivot was chosen, not executed
            break;
        }
        const int i_var = basis[p], j_var = nonbasis[r];
        __syncthreads(); // every thread has read x[p], z[r], basis[p], nonbasis[r]
        if (threadIdx.x == 0) {
            if (it < S.log_cap) {
                S.log_kind[it] = kind;
                S.log_enter[it] = j_var;
                S.log_leave[it] = i_var;
                S.log_mu[it] = mu;
            }
            basis[p] = j_var; // swap, :243-247
            nonbasis[r] = i_var;
        }
        for (int i = threadIdx.x; i < m; i += BLOCK) {
            const double d = dx[i];
            const double a = t * d, b = tbar * d;
            x[i] = (i == p) ? t : x[i] - a;
            xbar[i] = (i == p) ? tbar : xbar[i] - b;
        }
        for (int k = threadIdx.x; k < q; k += BLOCK) {
            const double d = dz[k];
            const double a = s * d, b = sbar * d;
            z[k] = (k == r) ? s : z[k] - a;
            zbar[k] = (k == r) ? sbar : zbar[k] - b;
        }
        ++it;
        __syncthreads(); // the next status() reads the updated vectors
    }
    return status;
}

// The row buckets, their grid caps and block sizes are in batch_host.h.
inline size_t lds_bytes(int mmax)
{
    return sizeof(double) * ((size_t)mmax * (mmax + 1) + 2 * (size_t)mmax) + 16;
}

} // namespace dzg_bs
