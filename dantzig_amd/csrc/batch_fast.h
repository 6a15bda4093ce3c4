// batch_fast.h -- the FAST iteration of one small LP whose basis inverse lies in LDS, written once
// for the kernels that run it: k_batch_fast, its DUMP twin and k_batch_fast_restart
// (k_batch_fast.hip, which documents the layout, the refactorisation, FTRAN and pricing) and the
// branch-and-bound node kernel k_mip_node_fast (k_mip.hip).  Device code only; the kernels own
// their arguments, their state in global memory and what follows the loop.
//
//   fast_steps     up to `ppl` pivots of src/simplex.rs:274-343 on a control block in LDS
//   restart_state  the restart state of a basis: x = W rhs, y = W^T c_B,
//                  z = -dz - c_N, both perturbation vectors at one
// Every sum's order depends on m alone.
#pragma once

#include "batch_strict.h"
#include "common.h"
#include "fast_decide.h"

namespace dzg_bf {

// What an LP carries from launch to launch beside its vectors.
struct FState {
    DzgCtl ctl;
    double max_err_life;  // largest max_pivot_err ever seen (the control block's restarts at a refactorisation)
    long long refactors;  // inversions of a basis that was not all slack
};

constexpr int kCtlBytes = (int)((sizeof(DzgCtl) + 15) / 16 * 16);

inline size_t fast_lds_bytes(int mmax)
{
    // W, acol, dx | control block | piv, flags
    return sizeof(double) * ((size_t)mmax * (mmax + 1) + 2 * (size_t)mmax) + kCtlBytes +
           (sizeof(int) * ((size_t)mmax + 4) + 15) / 16 * 16;
}

// One LP as the loop sees it: its matrix, its vectors in global memory and its pivot log
// (log_cap 0: none).
struct FastLp {
    const double *A;
    const int *var_col;
    int *basis, *nonbasis;
    double *x, *xbar, *z, *zbar, *dz;
    int m, q;
    int *log_kind, *log_enter, *log_leave;
    double *log_mu, *log_margin;
    long long log_off, log_cap;
};

// The LDS carve-up of fast_lds_bytes(mmax) for an LP of m rows.
struct FastLds {
    double *W;    // m x ld, inside mmax x (mmax + 1)
    double *acol; // mmax
    double *dxs;  // mmax
    DzgCtl *sc;
    int *piv;     // mmax
    int *s_flag;  // 4
    int ld;
};

__device__ __forceinline__ FastLds carve(double *s_mem, int mmax, int m)
{
    FastLds S;
    S.W = s_mem;
    S.acol = s_mem + (long long)mmax * (mmax + 1);
    S.dxs = S.acol + mmax;
    S.sc = (DzgCtl *)(S.dxs + mmax);
    S.piv = (int *)((char *)S.sc + kCtlBytes);
    S.s_flag = S.piv + mmax;
    S.ld = m | 1;
    return S;
}

__device__ __forceinline__ double shfl_xor_f64(double v, int off)
{
    const int lo = __shfl_xor(__double2loint(v), off, DZG_WAVE);
    const int hi = __shfl_xor(__double2hiint(v), off, DZG_WAVE);
    return __hiloint2double(hi, lo);
}

// W := B^-1 of the basis in global memory.  Returns 0, or 1 when a pivot was zero or not finite;
// `inverted` says whether an elimination ran (0: all-slack basis).  Every thread gets the same values.
template <int BLOCK, int PL>
__device__ int build_inverse(double *W, int ld, int m, const double *A, const int *var_col,
                             const int *basis, double *colk, int *piv, int *s_flag, int &inverted)
{
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    if (threadIdx.x == 0) {
        s_flag[0] = 0; // a structural column is basic
        s_flag[1] = 0; // singular
    }
    __syncthreads();
    for (int p = threadIdx.x; p < m; p += BLOCK)
        if (var_col[basis[p]] >= 0) s_flag[0] = 1;
    __syncthreads();
    inverted = s_flag[0];
    if (!inverted) { // B is a permutation matrix: its inverse is its transpose
        for (int e = threadIdx.x; e < m * m; e += BLOCK) {
            const int p = e / m, r = e - p * m;
            W[p * ld + r] = (-1 - var_col[basis[p]]) == r ? 1.0 : 0.0;
        }
        __syncthreads();
        return 0;
    }
    // stored entries only, as dzg_bs::gather: an explicit -0.0 of A arrives as +0.0
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
        W[r * ld + c] = v;
    }
    __syncthreads();
    for (int k = 0; k < m; ++k) {
        if (wave == 0) {
            DzgCand best;
            best.r = 0.0;
            best.k = -1;
            for (int r = k + lane; r < m; r += 64) best = dzg_better(best, dzg_bs::abs_cand(W[r * ld + k], r));
            best = dzg_wave_best(best);
            const int pr = best.k < 0 ? k : best.k;
            if (lane == 0) piv[k] = pr;
            if (pr != k) {
                for (int j = lane; j < m; j += 64) {
                    const double a = W[k * ld + j];
                    W[k * ld + j] = W[pr * ld + j];
                    W[pr * ld + j] = a;
                }
            }
            __builtin_amdgcn_wave_barrier();
            const double pivot = W[k * ld + k];
            const bool bad = !(pivot != 0.0) || isinf(pivot) || isnan(pivot);
            if (bad) {
                if (lane == 0) s_flag[1] = 1;
            } else {
                for (int i = lane; i < m; i += 64) { // column k leaves the matrix: the multipliers
                    colk[i] = W[i * ld + k];
                    W[i * ld + k] = i == k ? 1.0 : 0.0;
                }
                __builtin_amdgcn_wave_barrier();
                for (int j = lane; j < m; j += 64) W[k * ld + j] = W[k * ld + j] / pivot;
            }
        }
        __syncthreads();
        if (s_flag[1]) return 1;
        for (int i = threadIdx.x / PL; i < m; i += BLOCK / PL) { // PL lanes along a row
            if (i == k) continue;
            const double f = colk[i];
            for (int j = threadIdx.x % PL; j < m; j += PL) {
                const double adj = f * W[k * ld + j];
                W[i * ld + j] = W[i * ld + j] - adj;
            }
        }
        __syncthreads();
    }
    // P B = L U was inverted: B^-1 = (P B)^-1 P, the row swaps applied to the columns, last first
    for (int i = threadIdx.x; i < m; i += BLOCK) {
        for (int k = m - 1; k >= 0; --k) {
            const int pr = piv[k];
            if (pr == k) continue;
            const double a = W[i * ld + k];
            W[i * ld + k] = W[i * ld + pr];
            W[i * ld + pr] = a;
        }
    }
    __syncthreads();
    return 0;
}

// dx = W a_q into dxs (LDS); with RATIO the primal ratio test's candidates (src/simplex.rs:439-461)
template <int BLOCK, bool RATIO>
__device__ __forceinline__ void ftran(const double *W, int ld, int m, const double *A, int code,
                                      double *acol, double *dxs, const double *x, const double *xbar,
                                      double mu, double tau, DzgCand2 &best)
{
    if (code >= 0) {
        for (int i = threadIdx.x; i < m; i += BLOCK) acol[i] = A[(long long)code * m + i];
        __syncthreads();
    }
    for (int i = threadIdx.x; i < m; i += BLOCK) {
        double acc;
        if (code >= 0) {
            const double *row = W + i * ld;
            double s0 = 0.0, s1 = 0.0, s2 = 0.0, s3 = 0.0;
            int j = 0;
            for (; j + 3 < m; j += 4) {
                s0 = s0 + row[j] * acol[j];
                s1 = s1 + row[j + 1] * acol[j + 1];
                s2 = s2 + row[j + 2] * acol[j + 2];
                s3 = s3 + row[j + 3] * acol[j + 3];
            }
            if (j < m) s0 = s0 + row[j] * acol[j];
            if (j + 1 < m) s1 = s1 + row[j + 1] * acol[j + 1];
            if (j + 2 < m) s2 = s2 + row[j + 2] * acol[j + 2];
            acc = (s0 + s1) + (s2 + s3);
        } else {
            acc = W[i * ld + (-1 - code)];
        }
        dxs[i] = acc;
        if (RATIO) {
            const double xi = x[i], scaled = mu * xbar[i];
            const double den = xi + scaled;
            DzgCand2 cnd;
            cnd.r = dzg_div(acc, den);
            cnd.k = i;
            cnd.h = -__builtin_inf();
            if (cnd.r > 0.0) best = dzg_better2(best, cnd);
            if (dzg_noise_zero(den, xi, scaled, tau)) best.h = __builtin_inf();
        }
    }
}

// ratio-test candidate of one nonbasic position (src/simplex.rs:449-455), as k_price_kernels.h forms it
__device__ __forceinline__ void price_candidate_v(DzgCand2 &best, double dzk, int pos, double mu, double tau,
                                                  double zk, double zbk)
{
    const double scaled = mu * zbk;
    const double den = zk + scaled;
    DzgCand2 c;
    c.r = dzg_div(dzk, den);
    c.k = pos;
    c.h = -__builtin_inf();
    if (c.r > 0.0) best = dzg_better2(best, c);
    if (dzg_noise_zero(den, zk, scaled, tau)) best.h = __builtin_inf();
}

// dz = collect_columns(nonbasis).neg_t_dot(v) into global memory, v = row p of W; with RATIO the dual
// ratio test's candidates
template <int BLOCK, int PL, bool RATIO>
__device__ __forceinline__ void price(const double *v, int m, int q, const double *A, const int *var_col,
                                      const int *nonbasis, double *dz, const double *z, const double *zbar,
                                      double mu, double tau, DzgCand2 &best)
{
    const int sub = threadIdx.x % PL, grp = threadIdx.x / PL;
    constexpr int NG = BLOCK / PL;
    // every lane of a wave runs the same number of rounds: the xor tree needs all PL lanes of a group
    for (int k0 = 0; k0 < q; k0 += NG) {
        const int k = k0 + grp;
        double acc = 0.0;
        if (k < q) {
            const int code = var_col[nonbasis[k]];
            if (code < 0) {
                acc = -v[-1 - code]; // every lane of the group: the tree is skipped below
            } else {
                const double *col = A + (long long)code * m;
                for (int r = sub; r < m; r += PL) {
                    const double a = col[r];
                    if (a != 0.0) acc = acc + a * -v[r];
                }
#pragma unroll
                for (int off = PL / 2; off > 0; off >>= 1) acc = acc + shfl_xor_f64(acc, off);
            }
            if (sub == 0) {
                dz[k] = acc;
                if (RATIO) price_candidate_v(best, acc, k, mu, tau, z[k], zbar[k]);
            }
        }
    }
}

// Up to `ppl` pivots of LP `P` on the control block S.sc (LDS, loaded by the caller, who also stores
// it afterwards).  W is rebuilt from the basis in global memory at step 0 -- unless `w_built` says
// that S.W already holds the inverse of exactly that basis, with no pivot run on it -- and every
// `refactor_every` pivots after.  Returns DZG_RUNNING when the budget ran out, else the LP's final
// status (which S.sc->status holds too).  max_err_life and refactors are the caller's FState fields.
// Every path out has passed a barrier since W, the vectors and the control block were last written.
template <int BLOCK, int PL>
__device__ __forceinline__ int fast_steps(const FastLp &P, const FastLds &S, double eps, int ppl,
                                          int refactor_every, bool w_built, double &max_err_life,
                                          long long &refactors)
{
    const int m = P.m, q = P.q, ld = S.ld;
    double *W = S.W, *acol = S.acol, *dxs = S.dxs;
    DzgCtl *sc = S.sc;
    const double *A = P.A;
    const int *var_col = P.var_col;
    int *basis = P.basis, *nonbasis = P.nonbasis;
    double *x = P.x, *xbar = P.xbar, *z = P.z, *zbar = P.zbar, *dz = P.dz;
    const bool lead = threadIdx.x == 0;
    long long since = 0;

    int status = DZG_RUNNING;
    bool fresh = false; // W was built and no pivot has run on it yet
    for (int step = 0; step < ppl; ++step) {
        if (step == 0 || (refactor_every > 0 && since >= refactor_every)) {
            int inverted = 0;
            const int bad = m > 0 && !(step == 0 && w_built)
                                ? build_inverse<BLOCK, PL>(W, ld, m, A, var_col, basis, acol, S.piv, S.s_flag, inverted)
                                : 0;
            refactors += inverted;
            since = 0;
            fresh = true;
            if (lead) { // the monitor restarts with the fresh inverse
                sc->max_pivot_err = 0.0;
                if (sc->tie_tol >= 0.0) sc->tau = sc->tie_tol;
                if (bad) sc->status = DZG_SINGULAR;
            }
            __syncthreads();
            if (bad) {
                status = DZG_SINGULAR;
                break;
            }
        }
        DzgCtl c = *sc;
        const double tau = c.tau;
        // ---- status(), src/simplex.rs:274-306
        DzgCand2 bz = dzg_cand2_none(), bx = dzg_cand2_none();
        for (int k = threadIdx.x; k < q; k += BLOCK) dzg_first_pivot_entry(bz, z[k], zbar[k], k, tau);
        for (int i = threadIdx.x; i < m; i += BLOCK) dzg_first_pivot_entry(bx, x[i], xbar[i], i, tau);
        const DzgCand2 cj = dzg_block_best2(bz);
        const DzgCand2 ci = dzg_block_best2(bx);
        int kind = -1;
        double mu = 0.0;
        if (!fast_status(sc, c, lead, cj, ci, eps, m, false, kind, &mu)) {
            __syncthreads();
            status = sc->status;
            break;
        }
        int p, r;
        DzgCand2 best = dzg_cand2_none();
        if (kind == DZG_STEP_PRIMAL) { // :308-318
            r = cj.k;
            ftran<BLOCK, true>(W, ld, m, A, var_col[nonbasis[r]], acol, dxs, x, xbar, mu, tau, best);
            const DzgCand2 cw = dzg_block_best2(best);
            if (!fast_ratio_outcome(sc, c, lead, cw, DZG_UNBOUNDED)) {
                __syncthreads();
                status = sc->status;
                break;
            }
            p = cw.k;
            price<BLOCK, PL, false>(W + p * ld, m, q, A, var_col, nonbasis, dz, z, zbar, mu, tau, best);
        } else { // :320-330
            p = ci.k;
            price<BLOCK, PL, true>(W + p * ld, m, q, A, var_col, nonbasis, dz, z, zbar, mu, tau, best);
            const DzgCand2 cw = dzg_block_best2(best);
            if (!fast_ratio_outcome(sc, c, lead, cw, DZG_INFEASIBLE)) {
                __syncthreads();
                status = sc->status;
                break;
            }
            r = cw.k;
            DzgCand2 unused = dzg_cand2_none();
            ftran<BLOCK, false>(W, ld, m, A, var_col[nonbasis[r]], acol, dxs, x, xbar, mu, tau, unused);
        }
        __syncthreads(); // dxs (LDS) and dz (global) are complete
        // ---- pivot, src/simplex.rs:253-268: step lengths, finiteness assert (:466)
        const double dxp = dxs[p], dzr = dz[r];
        int ok = 1;
        const double t = dzg_safe_divide(x[p], dxp, &ok);
        const double s = dzg_safe_divide(z[r], dzr, &ok);
        const double tbar = dzg_safe_divide(xbar[p], dxp, &ok);
        const double sbar = dzg_safe_divide(zbar[r], dzr, &ok);
        if (!ok) { // the pivot was chosen, not executed
            if (lead) sc->status = DZG_PANIC;
            status = DZG_PANIC;
            break;
        }
        // the pivot element is known twice: dx_p from FTRAN, -dz_r from BTRAN + pricing
        double max_err = c.max_pivot_err;
        {
            const double a1 = fabs(dxp), a2 = fabs(dzr);
            const double den = a1 > a2 ? a1 : a2;
            const double err = den > 0.0 ? fabs(dxp + dzr) / den : 0.0;
            if (err > max_err) max_err = err;
        }
        if (max_err > max_err_life) max_err_life = max_err;
        const int i_var = basis[p], j_var = nonbasis[r];
        // row p of the new inverse, into acol (the entering column is spent)
        for (int j = threadIdx.x; j < m; j += BLOCK) acol[j] = W[p * ld + j] / dxp;
        __syncthreads(); // every thread has read x[p], z[r], basis[p], nonbasis[r], row p
        if (lead) {
            const long long it = c.iter;
            if (it < P.log_cap) {
                P.log_kind[P.log_off + it] = kind;
                P.log_enter[P.log_off + it] = j_var;
                P.log_leave[P.log_off + it] = i_var;
                P.log_mu[P.log_off + it] = mu;
                P.log_margin[P.log_off + it] = c.margin;
            }
            basis[p] = j_var; // swap, :243-247
            nonbasis[r] = i_var;
            sc->enter_pos = r;
            sc->leave_pos = p;
            sc->enter_var = j_var;
            sc->leave_var = i_var;
            sc->t = t;
            sc->s = s;
            sc->tbar = tbar;
            sc->sbar = sbar;
            sc->max_pivot_err = max_err;
            // near-tie record of this pivot; the tolerance follows the health monitor
            if (c.margin < c.min_margin) sc->min_margin = c.margin;
            if (c.tie_seen) {
                sc->near_ties = c.near_ties + 1;
                if (c.first_near_tie < 0) sc->first_near_tie = it;
            }
            if (c.tie_tol >= 0.0) {
                const double adaptive = 64.0 * max_err;
                sc->tau = adaptive > c.tie_tol ? adaptive : c.tie_tol;
            }
            sc->iter = it + 1;
        }
        for (int i = threadIdx.x; i < m; i += BLOCK) {
            const double d = dxs[i];
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
        for (int i = threadIdx.x / PL; i < m; i += BLOCK / PL) { // PL lanes along a row
            const double f = dxs[i];
            for (int j = threadIdx.x % PL; j < m; j += PL) {
                const double adj = f * acol[j];
                W[i * ld + j] = (i == p) ? acol[j] : W[i * ld + j] - adj;
            }
        }
        ++since;
        __syncthreads(); // the next status() reads the updated vectors and control block
        // FAST health: the two values of the pivot element disagree beyond repair.  A stale inverse
        // is rebuilt; one that drifts on its first pivot is ill-conditioned: DZG_SINGULAR
        if (max_err > 1e-4) {
            if (fresh) {
                if (lead) sc->status = DZG_SINGULAR;
                status = DZG_SINGULAR;
                break;
            }
            since = refactor_every > 0 ? refactor_every : since;
        }
        fresh = false;
    }
    __syncthreads();
    return status;
}

// sum_j a[j * stride] * b[j] in ftran's order: four interleaved partial sums, j ascending, then
// (s0 + s1) + (s2 + s3); every product rounded before it is added
__device__ __forceinline__ double dot4(const double *a, int stride, const double *b, int m)
{
    double s0 = 0.0, s1 = 0.0, s2 = 0.0, s3 = 0.0;
    int j = 0;
    for (; j + 3 < m; j += 4) {
        s0 = s0 + a[j * stride] * b[j];
        s1 = s1 + a[(j + 1) * stride] * b[j + 1];
        s2 = s2 + a[(j + 2) * stride] * b[j + 2];
        s3 = s3 + a[(j + 3) * stride] * b[j + 3];
    }
    if (j < m) s0 = s0 + a[j * stride] * b[j];
    if (j + 1 < m) s1 = s1 + a[(j + 1) * stride] * b[j + 1];
    if (j + 2 < m) s2 = s2 + a[(j + 2) * stride] * b[j + 2];
    return (s0 + s1) + (s2 + s3);
}

// The restart state of LP `P` from S.W = the inverse of its basis:
//
//      x_i = sum_j W[i][j] rhs(j)                       rhs by constraint row
//      y_r = sum_p W[p][r] c[basis[p]]                  one thread per r: a wave reads a row of W
//      z_k = -dz_k - c[N_k],  dz = price(v = y)         stored entries only; a slack is one negation
//      xbar = zbar = 1
//
// y lies in dxs, rhs and then c_B in acol.  Both sums run in dot4's order, which depends on m alone.
// No refinement step.  S.s_flag[2] (zeroed by the caller before a barrier) is set when an entry of x
// or z is not finite; it may be read after the return.  `c` is the cost by variable.
template <int BLOCK, int PL, class Rhs>
__device__ __forceinline__ void restart_state(const FastLp &P, const FastLds &S, const double *c, Rhs rhs)
{
    const int m = P.m, q = P.q, ld = S.ld;
    double *W = S.W, *acol = S.acol, *ys = S.dxs;
    for (int i = threadIdx.x; i < m; i += BLOCK) acol[i] = rhs(i);
    __syncthreads();
    for (int i = threadIdx.x; i < m; i += BLOCK) {
        const double xi = dot4(W + i * ld, 1, acol, m);
        P.x[i] = xi;
        P.xbar[i] = 1.0;
        if (isinf(xi) || isnan(xi)) S.s_flag[2] = 1;
    }
    __syncthreads(); // rhs is read
    for (int p = threadIdx.x; p < m; p += BLOCK) acol[p] = c[P.basis[p]];
    __syncthreads();
    for (int r = threadIdx.x; r < m; r += BLOCK) ys[r] = dot4(W + r, ld, acol, m);
    __syncthreads();
    DzgCand2 unused = dzg_cand2_none();
    price<BLOCK, PL, false>(ys, m, q, P.A, P.var_col, P.nonbasis, P.dz, P.z, P.zbar, 0.0, 0.0, unused);
    __syncthreads(); // dz (global) is complete
    for (int k = threadIdx.x; k < q; k += BLOCK) {
        const double zk = -P.dz[k] - c[P.nonbasis[k]];
        P.z[k] = zk;
        P.zbar[k] = 1.0;
        if (isinf(zk) || isnan(zk)) S.s_flag[2] = 1;
    }
    __syncthreads();
}

} // namespace dzg_bf
