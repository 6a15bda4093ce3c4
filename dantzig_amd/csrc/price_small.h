// price_small.h -- what the fused small-k row pass is made of (k_price_rows_small, k_price_kernels.h),
// for the two kernels that run it: the stand-alone launch and the pricing tail of k_chain_pre
// (k_chain.hip).  Device functions only: the arithmetic, the order of every sum and the issue path of
// the rows stage are written once.
#pragma once
#include "common.h"

typedef double double2_t __attribute__((ext_vector_type(2)));

#define PR_GMAX DZG_PR_GMAX
#define PR_BATCH DZG_PR_BATCH // rows per group at least (G = ceil(rows / PR_BATCH), capped at PR_GMAX)

// ratio-test candidate of one position (src/simplex.rs:449-455): dz / (z + mu*zbar) if > 0
// (FAST numerics only: the candidate carries its competition for the near-tie arbitration, and
// a denominator that is zero up to rounding marks the whole test untrustworthy -- the reference
// may have +inf, which wins, NaN or a negative ratio there)
__device__ __forceinline__ void price_candidate(DzgCand2 &best, double dzk, int pos, double mu,
                                                double tau, const double *__restrict__ z,
                                                const double *__restrict__ zbar)
{
    const double zk = z[pos], scaled = mu * zbar[pos];
    const double den = zk + scaled;
    DzgCand2 c;
    c.r = dzg_div(dzk, den);
    c.k = pos;
    c.h = -__builtin_inf();
    if (c.r > 0.0) best = dzg_better2(best, c);
    if (dzg_noise_zero(den, zk, scaled, tau)) best.h = __builtin_inf();
}

// the same with z[pos], zbar[pos] already in registers
__device__ __forceinline__ void price_candidate_v(DzgCand2 &best, double dzk, int pos, double mu,
                                                  double tau, double zk, double zbk)
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

// k_price_rows_small's publish step (512 threads): the straight-line wave reduction of common.h,
// then the eight wave results in the three steps of one half row -- one workgroup barrier instead of
// two, no 64-lane butterfly for eight values.  The same candidate, bit for bit (common.h).
// Only for a launch of exactly 512 threads, all of which arrive here (k_price_rows_small:
// __launch_bounds__(512), launched with 512; its early exits are taken by the whole workgroup): the
// half-row stage holds eight wave results, no more.
__device__ __forceinline__ void price_publish_small(DzgCand2 best, double *__restrict__ rz_r,
                                                    int *__restrict__ rz_k, double *__restrict__ rz_h)
{
    best = dzg_block_best2_flat<8>(best, false);
    if (rz_r && threadIdx.x == 0) {
        rz_r[blockIdx.x] = best.r;
        rz_k[blockIdx.x] = best.k;
        rz_h[blockIdx.x] = best.h;
    }
}

#define PRS_TILE 64
#define PRS_ROWS 512
#define PRS_STAMP_SLOT 4
// The two stages k_price_rows_small runs once its row list is in LDS (s_off[c] = row * ldt, s_coef[c],
// entry k the leaving slack's own row with 1.0), as device functions: the stand-alone kernel calls
// them, and so does the pricing tail of k_chain_pre (k_chain.hip, PRICE), whose workgroup b prices
// tile b.  Every thread of a 512-thread workgroup calls both, with a workgroup barrier in between.
//
// The rows stage: the partial sums of this workgroup's row groups, into s_part.  Returns G.
template <int VEC, int NG, int RPT>
__device__ __forceinline__ int price_small_rows(const double *__restrict__ At, long long ldt, int tile, int k,
                                                int lcode, const long long *s_off, const double *s_coef,
                                                double (*s_part)[PRS_TILE])
{
    constexpr int LPG = 64 / VEC; // lanes of a group slot
    constexpr int NS = 512 / LPG; // group slots of the workgroup
    static_assert(VEC == 1 || VEC == 2, "8- or 16-byte loads");
    static_assert(PR_BATCH % RPT == 0 && PR_GMAX * PR_BATCH >= PRS_ROWS, "a group has at most PR_BATCH rows");
    const int tid = threadIdx.x;
    const int nrows = k + (lcode < 0 ? 1 : 0);
    int G = (k + 1 + PR_BATCH - 1) / PR_BATCH; // (as k_price_rows)
    G = G > PR_GMAX ? PR_GMAX : G;
    const int slot = tid / LPG, h = tid % LPG;
    const long long jc = (long long)tile * PRS_TILE + h * VEC; // (ldt is even when VEC = 2)
    const double *col = At + (jc < ldt ? jc : 0);
    for (int g0 = slot; g0 < G; g0 += NS * NG) {
        double acc[NG][VEC];
#pragma unroll
        for (int t = 0; t < NG; ++t)
#pragma unroll
            for (int e = 0; e < VEC; ++e) acc[t][e] = 0.0;
        for (int r0 = 0; r0 < PR_BATCH; r0 += RPT) {
            if (RPT < PR_BATCH && g0 + r0 * G >= nrows) break; // (groups ascend with t: none has a row left)
            // entry (t, u): c = g + (r0 + u) G of group g = g0 + NS t; it exists when g < G and
            // c < nrows (the LDS reads are unconditional: one that does not exist reads entry 0)
#define PRS_ENTRY(T, U)                                                                              \
    const int c = g0 + NS * (T) + (r0 + (U)) * G;                                                    \
    const bool ok = g0 + NS * (T) < G && c < nrows
            long long off[NG][RPT]; // one batch of LDS reads, waited for once
#pragma unroll
            for (int t = 0; t < NG; ++t)
#pragma unroll
                for (int u = 0; u < RPT; ++u) {
                    PRS_ENTRY(t, u);
                    off[t][u] = s_off[ok ? c : 0];
                }
            // the rows, all in flight; the coefficients behind them
            double x[NG][RPT][VEC], cf[NG][RPT];
#pragma unroll
            for (int t = 0; t < NG; ++t)
#pragma unroll
                for (int u = 0; u < RPT; ++u) {
                    PRS_ENTRY(t, u);
                    const double *src = col + (ok ? off[t][u] : 0);
                    if constexpr (VEC == 2) {
                        const double2_t w = __builtin_nontemporal_load(reinterpret_cast<const double2_t *>(src));
                        x[t][u][0] = w.x;
                        x[t][u][1] = w.y;
                    } else {
                        x[t][u][0] = __builtin_nontemporal_load(src);
                    }
                }
            // (the scheduler otherwise holds back two of sixteen loads until the first sums are done,
            // a second trip, and mixes the coefficients' LDS reads among the loads)
            __builtin_amdgcn_sched_barrier(0);
#pragma unroll
            for (int t = 0; t < NG; ++t)
#pragma unroll
                for (int u = 0; u < RPT; ++u) {
                    PRS_ENTRY(t, u);
                    cf[t][u] = s_coef[ok ? c : 0];
                }
#pragma unroll
            for (int t = 0; t < NG; ++t)
#pragma unroll
                for (int u = 0; u < RPT; ++u) {
                    PRS_ENTRY(t, u);
#pragma unroll
                    for (int e = 0; e < VEC; ++e)
                        acc[t][e] = ok ? fma(cf[t][u], x[t][u][e], acc[t][e]) : acc[t][e];
                }
#undef PRS_ENTRY
        }
#pragma unroll
        for (int t = 0; t < NG; ++t)
            if (g0 + NS * t < G) {
#pragma unroll
                for (int e = 0; e < VEC; ++e) s_part[g0 + NS * t][h * VEC + e] = acc[t][e];
            }
    }
    return G;
}

// The finish: wave 0 adds a column's G partial sums in group order, writes dz and forms the z-side
// ratio candidate (pos = the lane's column's nonbasic position, < 0: none; zc, zbc = z, zbar there);
// every thread prices its unit-column position (scode < 0: position spos, sv = v of the slack's row,
// sz, szb = z, zbar there); the workgroup's best candidate goes to rz_*[blockIdx.x].
// STRIDED: positions beyond nwg * 512 are walked too (nwg = the workgroups that price; the chain
// tail's host rule keeps q <= nwg * 512, and v is being written by that launch).
template <bool STRIDED>
__device__ __forceinline__ void price_small_finish(ChainStamps &ts, int G, const double (*s_part)[PRS_TILE],
                                                   int pos, double zc, double zbc, int scode, int spos,
                                                   double sv, double sz, double szb, int nwg, int q,
                                                   const int *__restrict__ nbcode, const double *__restrict__ v,
                                                   double *__restrict__ dz, const double *__restrict__ z,
                                                   const double *__restrict__ zbar, double mu, double tau,
                                                   double *__restrict__ rz_r, int *__restrict__ rz_k,
                                                   double *__restrict__ rz_h)
{
    const int lane = threadIdx.x & 63;
    DzgCand2 best = dzg_cand2_none();
    if (pos >= 0) { // (wave 0) the finishing launch's sum: the groups in order
        double sum = 0.0;
        for (int g = 0; g < G; ++g) sum = sum + s_part[g][lane];
        dz[pos] = -sum;
        price_candidate_v(best, -sum, pos, mu, tau, zc, zbc);
    }
    // ---- unit columns (the arithmetic of price_slack_positions)
    if (scode < 0) {
        const double p = 1.0 * -sv;
        const double d = 0.0 + p;
        dz[spos] = d;
        price_candidate_v(best, d, spos, mu, tau, sz, szb);
    }
    for (int ps = spos + nwg * 512; STRIDED && ps < q; ps += nwg * 512) { // (never: 8 threads per column)
        const int code = nbcode[ps];
        if (code < 0) {
            const double p = 1.0 * -v[-1 - code];
            const double d = 0.0 + p;
            dz[ps] = d;
            price_candidate(best, d, ps, mu, tau, z, zbar);
        }
    }
    ts.pin(best);
    const unsigned long long t_publish = ts.now();
    price_publish_small(best, rz_r, rz_k, rz_h);
    ts.site(DZG_SITE_PUBLISH, t_publish);
}

