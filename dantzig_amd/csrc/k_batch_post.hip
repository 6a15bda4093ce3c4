// k_batch_post.hip -- what a FAST batch can say about the state its LPs ended in (DESIGN.md section
// 7n): dual values, reduced costs and the certificate's scalars of an LP that ended OPTIMAL, the ray
// of one that ended UNBOUNDED or INFEASIBLE.  The definitions are dzg_duals' and dzg_ray's
// (include/dantzig_amd.h); the arithmetic is the FAST batch's own (batch_fast.h).
//
// k_batch_fast_post: one workgroup per listed LP, once, after the rounds; k_batch_fast_restart's
// buckets, block sizes, chunks and LDS carve-up.  It reads the final state in global memory (basis,
// nonbasis, x, xbar, z, zbar), the status and tau of the LP's control block, c by variable and the
// right-hand side by constraint row, and writes to sections of its own: y (by row), d (by variable),
// PS doubles of scalars, one int of post status and a pricing scratch.  The carried state, the
// control block, refactors and the log are not touched.
//
//   step 0      W = build_inverse(final basis): an all-slack basis is a permutation, anything else a
//               Gauss-Jordan inversion, no refinement step -- as restart_state.  A zero or non-finite
//               pivot: post status DZG_POST_SINGULAR, nothing else is written for that LP.
//   OPTIMAL     y_r = sum_p W[p][r] c[B_p] (one thread per row, dot4 over positions), dz = price(y),
//               d[N_k] = -dz_k - c[N_k], d[B_p] = 0.0, dual_obj = constant + dot4(rhs0, y);
//               min x, min d_N, max |d_N|, max |z - d_N| reduced with min / max alone.
//   UNBOUNDED   pos = the first-pivot winner over (z, zbar) as fast_steps finds it (dzg_first_pivot_entry
//               at the control block's tau), j = N[pos], dx = ftran(W, a_j): d[j] = 1, d[B_p] = -dx_p,
//               value = c[j] - dot4(c_B, dx), violation = max_p max(dx_p, 0).
//   INFEASIBLE  pos over (x, xbar), y = row pos of W, dz = price(y): d[N_k] = -dz_k, d[B_pos] = 1,
//               value = dot4(rhs0, y), violation = max_k max(dz_k, 0).
// Every sum's order depends on m alone and there are no atomics: an LP's post-solve is bit-identical
// wherever it sits in a batch and when it is asked twice.
#include <algorithm>
#include <cstring>
#include <vector>

#include "batch_fast.h"
#include "batch_host.h"
#include "batch_steps.h"
#include "common.h"
#include "duals.h"
#include "ranging.h"
#include "rays.h"

namespace {

using namespace dzg_rg; // ranging.h: the candidate rule and its reductions

using dzg_bf::FState;
using dzg_bf::fast_lds_bytes;
namespace bh = dzg_bh;

constexpr int PS = DZG_POST_SCAL;

struct PArgs {
    const DzgBatchLp *lp;
    const double *A;
    const int *var_col;
    const int *basis, *nonbasis;
    const double *x, *xbar, *z, *zbar;
    const FState *state;
    const double *c;    // by variable
    const double *rhs0; // by constraint row
    double *dz;         // pricing scratch of the post-solve's own, q per LP
    double *y, *d, *scal;
    int *pstat;
    // ranging: per LP its tolerance and its directions item[irange[2 id] .. irange[2 id + 1]), as
    // DzgRangingArgs has them; posmap (one int per variable, at vc_off) is the kernel's to fill
    const double *tol;
    const int *irange;
    const DzgRangeItem *item;
    const int *e_idx;
    const double *e_val;
    int *posmap;
    double *lo, *hi;
    int *lo_var, *hi_var;
    int duals, ranging, rays; // what is asked for
    int mmax;        // largest m of the bucket: sizes the LDS carve-up
};

// min / max over the wave: order-independent, exact
__device__ __forceinline__ double wave_min(double v)
{
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) v = fmin(v, dzg_bf::shfl_xor_f64(v, off));
    return v;
}

__device__ __forceinline__ double wave_max(double v)
{
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) v = fmax(v, dzg_bf::shfl_xor_f64(v, off));
    return v;
}

// The four reductions of a pass over the whole workgroup: v[0], v[1] by min, v[2], v[3] by max;
// thread 0 holds the result.  Every thread of the workgroup calls it.
template <int BLOCK>
__device__ __forceinline__ void block_minmax(double (&v)[4], double (*s_red)[4])
{
    v[0] = wave_min(v[0]);
    v[1] = wave_min(v[1]);
    v[2] = wave_max(v[2]);
    v[3] = wave_max(v[3]);
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    if (lane == 0)
        for (int e = 0; e < 4; ++e) s_red[wave][e] = v[e];
    __syncthreads();
    if (threadIdx.x == 0) {
        for (int w = 1; w < BLOCK / 64; ++w) {
            v[0] = fmin(v[0], s_red[w][0]);
            v[1] = fmin(v[1], s_red[w][1]);
            v[2] = fmax(v[2], s_red[w][2]);
            v[3] = fmax(v[3], s_red[w][3]);
        }
    }
}

template <int BLOCK, int PL>
__global__ __launch_bounds__(BLOCK) void k_batch_fast_post(PArgs g, const int *__restrict__ list)
{
    extern __shared__ __attribute__((aligned(16))) double s_mem[];
    __shared__ double s_red[4][4];
    __shared__ DzgRangePart s_part[4];
    const int id = list[blockIdx.x];
    const DzgBatchLp L = g.lp[id];
    const int m = L.m, q = L.n - L.m;
    const dzg_bf::FastLds S = dzg_bf::carve(s_mem, g.mmax, m); // the control block is not used here
    const int ld = S.ld;
    double *W = S.W, *acol = S.acol, *vs = S.dxs;
    const double *A = g.A + L.a_off;
    const int *var_col = g.var_col + L.vc_off;
    const int *basis = g.basis + L.m_off, *nonbasis = g.nonbasis + L.q_off;
    const double *x = g.x + L.m_off, *xbar = g.xbar + L.m_off;
    const double *z = g.z + L.q_off, *zbar = g.zbar + L.q_off;
    const double *c = g.c + L.vc_off, *rhs0 = g.rhs0 + L.m_off;
    double *dz = g.dz + L.q_off, *y = g.y + L.m_off, *d = g.d + L.vc_off;
    double *out = g.scal + (long long)id * PS;
    const bool lead = threadIdx.x == 0;
    const int status = g.state[id].ctl.status;
    const double tau = g.state[id].ctl.tau;
    const bool optimal = status == DZG_OPTIMAL;
    const bool ray = status == DZG_UNBOUNDED || status == DZG_INFEASIBLE;
    if (m == 0 || !((optimal && g.duals) || (ray && g.rays))) { // (the host lists no such LP)
        if (lead) g.pstat[id] = DZG_POST_NONE;
        return;
    }

    // ---- step 0: the inverse of the final basis
    int inverted = 0;
    if (dzg_bf::build_inverse<BLOCK, PL>(W, ld, m, A, var_col, basis, acol, S.piv, S.s_flag, inverted)) {
        if (lead) g.pstat[id] = DZG_POST_SINGULAR;
        return;
    }
    DzgCand2 unused = dzg_cand2_none();

    if (optimal) {
        for (int p = threadIdx.x; p < m; p += BLOCK) acol[p] = c[basis[p]];
        __syncthreads();
        for (int r = threadIdx.x; r < m; r += BLOCK) {
            const double yr = dzg_bf::dot4(W + r, ld, acol, m);
            vs[r] = yr;
            y[r] = yr;
        }
        __syncthreads();
        dzg_bf::price<BLOCK, PL, false>(vs, m, q, A, var_col, nonbasis, dz, z, zbar, 0.0, 0.0, unused);
        __syncthreads(); // dz (global) is complete
        double v[4] = {__builtin_inf(), __builtin_inf(), 0.0, 0.0}; // min x, min d_N, max |d_N|, max |z - d_N|
        for (int p = threadIdx.x; p < m; p += BLOCK) {
            d[basis[p]] = 0.0;
            v[0] = fmin(v[0], x[p]);
        }
        for (int k = threadIdx.x; k < q; k += BLOCK) {
            const int var = nonbasis[k];
            const double dk = -dz[k] - c[var];
            d[var] = dk;
            v[1] = fmin(v[1], dk);
            v[2] = fmax(v[2], fabs(dk));
            v[3] = fmax(v[3], fabs(z[k] - dk));
        }
        block_minmax<BLOCK>(v, s_red);
        if (lead) {
            out[0] = L.constant + dzg_bf::dot4(rhs0, 1, vs, m);
            out[1] = fmax(0.0, -v[0]);
            out[2] = fmax(0.0, -v[1]);
            out[3] = v[3]; // the host divides: max |z - d_N| / max(1, max |d_N|)
            out[4] = v[2];
            g.pstat[id] = DZG_POST_DONE;
        }
        if (!g.ranging) return;
        // ---- the LP's directions, one after another.  The position of every variable first:
        // p for the basic one at position p, -1 - k for the nonbasic one at position k
        int *posmap = g.posmap + L.vc_off;
        for (int p = threadIdx.x; p < m; p += BLOCK) posmap[basis[p]] = p;
        for (int k = threadIdx.x; k < q; k += BLOCK) posmap[nonbasis[k]] = -1 - k;
        __syncthreads(); // posmap and d (global) are complete
        const double tol = g.tol[id];
        const int it1 = g.irange[2 * id + 1];
        for (int ii = g.irange[2 * id]; ii < it1; ++ii) {
            const DzgRangeItem it = g.item[ii];
            DzgRangePart me = range_none();
            if (it.kind == 0) { // delta_p = sum_e W[p][r_e] h_e, entries in the order given
                for (int p = threadIdx.x; p < m; p += BLOCK) {
                    double acc = 0.0;
                    for (long long e = it.e0; e < it.e1; ++e) {
                        const double prod = W[p * ld + g.e_idx[e]] * g.e_val[e];
                        acc = acc + prod;
                    }
                    range_elem(me, fmax(x[p], 0.0), acc, tol, p);
                }
            } else { // Y_r = sum over the basic entries of g_e W[pos(e)][r], delta_k = -dz_k(Y) - g_{N_k}
                int nbasic = 0;
                for (long long e = it.e0; e < it.e1; ++e) nbasic += posmap[g.e_idx[e]] >= 0 ? 1 : 0;
                if (nbasic > 0) { // (the same for every thread)
                    for (int r = threadIdx.x; r < m; r += BLOCK) {
                        double acc = 0.0;
                        for (long long e = it.e0; e < it.e1; ++e) {
                            const int p = posmap[g.e_idx[e]];
                            if (p < 0) continue;
                            const double prod = g.e_val[e] * W[p * ld + r];
                            acc = acc + prod;
                        }
                        vs[r] = acc;
                    }
                    __syncthreads();
                    dzg_bf::price<BLOCK, PL, false>(vs, m, q, A, var_col, nonbasis, dz, z, zbar, 0.0, 0.0, unused);
                    __syncthreads(); // dz (global) is complete
                }
                for (int k = threadIdx.x; k < q; k += BLOCK) {
                    const int var = nonbasis[k];
                    const double gk = dir_value(g.e_idx, g.e_val, it.e0, it.e1, var);
                    const double delta = (nbasic > 0 ? -dz[k] : 0.0) - gk; // no basic entry: Y = 0
                    range_elem(me, fmax(d[var], 0.0), delta, tol, k);
                }
            }
            me = range_block<BLOCK>(me, s_part);
            if (lead) {
                const int *at = it.kind == 0 ? basis : nonbasis;
                g.lo[it.out] = me.lo;
                g.hi[it.out] = me.hi;
                g.lo_var[it.out] = me.lo_k == DZG_RANGE_NONE ? -1 : at[me.lo_k];
                g.hi_var[it.out] = me.hi_k == DZG_RANGE_NONE ? -1 : at[me.hi_k];
            }
            __syncthreads(); // s_part, vs and dz are free for the next direction
        }
        return;
    }

    // ---- a ray: the position the failed step stopped at, as fast_steps' status() finds it
    const bool primal = status == DZG_UNBOUNDED;
    DzgCand2 b = dzg_cand2_none();
    if (primal)
        for (int k = threadIdx.x; k < q; k += BLOCK) dzg_first_pivot_entry(b, z[k], zbar[k], k, tau);
    else
        for (int i = threadIdx.x; i < m; i += BLOCK) dzg_first_pivot_entry(b, x[i], xbar[i], i, tau);
    const DzgCand2 cand = dzg_block_best2(b);
    const int pos = cand.k;
    if (pos < 0 || cand.r == -__builtin_inf()) { // (no such state ends UNBOUNDED or INFEASIBLE)
        if (lead) {
            out[0] = -1.0;
            g.pstat[id] = DZG_POST_DONE;
        }
        return;
    }
    double v[4] = {0.0, 0.0, 0.0, 0.0}; // [2]: violation, [3]: a NaN was met
    double value;
    if (primal) {
        dzg_bf::ftran<BLOCK, false>(W, ld, m, A, var_col[nonbasis[pos]], acol, vs, x, xbar, 0.0, 0.0, unused);
        __syncthreads(); // dx (LDS) is complete, the column in acol is spent
        for (int k = threadIdx.x; k < q; k += BLOCK) d[nonbasis[k]] = k == pos ? 1.0 : 0.0;
        for (int p = threadIdx.x; p < m; p += BLOCK) {
            const double e = vs[p];
            d[basis[p]] = -e;
            y[p] = 0.0;
            acol[p] = c[basis[p]];
            v[2] = fmax(v[2], fmax(e, 0.0));
            if (e != e) v[3] = 1.0;
        }
        block_minmax<BLOCK>(v, s_red); // (its barrier: acol is complete)
        value = lead ? c[nonbasis[pos]] - dzg_bf::dot4(acol, 1, vs, m) : 0.0;
    } else {
        const double *row = W + pos * ld;
        dzg_bf::price<BLOCK, PL, false>(row, m, q, A, var_col, nonbasis, dz, z, zbar, 0.0, 0.0, unused);
        __syncthreads(); // dz (global) is complete
        for (int k = threadIdx.x; k < q; k += BLOCK) {
            const double e = dz[k];
            d[nonbasis[k]] = -e;
            v[2] = fmax(v[2], fmax(e, 0.0));
            if (e != e) v[3] = 1.0;
        }
        for (int p = threadIdx.x; p < m; p += BLOCK) {
            d[basis[p]] = p == pos ? 1.0 : 0.0;
            y[p] = row[p];
        }
        block_minmax<BLOCK>(v, s_red);
        value = lead ? dzg_bf::dot4(rhs0, 1, row, m) : 0.0;
    }
    if (lead) {
        out[0] = (double)(primal ? nonbasis[pos] : basis[pos]);
        out[1] = (double)pos;
        out[2] = cand.r;
        out[3] = value;
        out[4] = v[3] != 0.0 ? __builtin_nan("") : v[2];
        g.pstat[id] = DZG_POST_DONE;
    }
}

// The LPs list[0..n) of row bucket b, one workgroup each: k_batch_fast_restart's instantiations and LDS
void launch_post_bucket(int b, const PArgs &g, const int *list, int n, hipStream_t st)
{
    const size_t lds = fast_lds_bytes(g.mmax);
    if (b == 3) { // more than 64 KiB of dynamic LDS, as in k_batch_fast.hip's launch_bucket
        static const hipError_t attr =
            hipFuncSetAttribute(reinterpret_cast<const void *>(k_batch_fast_post<256, 64>),
                                hipFuncAttributeMaxDynamicSharedMemorySize, (int)fast_lds_bytes(DZG_BATCH_MAX_ROWS));
        (void)attr;
    }
    bh::for_each_chunk(b, n, [&](int c0, int grid) {
        const dim3 block(bh::kBlock[b]);
        if (b == 0)
            hipLaunchKernelGGL((k_batch_fast_post<64, 16>), dim3(grid), block, lds, st, g, list + c0);
        else if (b == 1)
            hipLaunchKernelGGL((k_batch_fast_post<64, 32>), dim3(grid), block, lds, st, g, list + c0);
        else if (b == 2)
            hipLaunchKernelGGL((k_batch_fast_post<128, 64>), dim3(grid), block, lds, st, g, list + c0);
        else
            hipLaunchKernelGGL((k_batch_fast_post<256, 64>), dim3(grid), block, lds, st, g, list + c0);
    });
}

} // namespace

// ---- the steps of batch_steps.h
void dzg_steps::post_layout(bh::Arena &ar, PostSections &S, long long nvc, long long nm, long long nq, int N)
{
    S.c = ar.add(sizeof(double) * nvc);
    S.rhs0 = ar.add(sizeof(double) * nm);
    post_layout_out(ar, S, nvc, nm, nq, N);
}

void dzg_steps::post_layout_out(bh::Arena &ar, PostSections &S, long long nvc, long long nm, long long nq, int N)
{
    S.list = ar.add(sizeof(int) * N);
    S.dz = ar.add(sizeof(double) * nq);
    S.y = ar.add(sizeof(double) * nm);
    S.d = ar.add(sizeof(double) * nvc);
    S.scal = ar.add(sizeof(double) * PS * N);
    S.pstat = ar.add(sizeof(int) * N);
    S.end = ar.top;
}

int dzg_steps::post_ranging_pack(PostRanging &G, const dzg_ranging_req *req, int n, const int64_t *ids,
                                 const unsigned char *listed, const bh::Packed &P)
{
    const int N = (int)P.desc.size();
    const long long nvc = P.nvc;
    G.out0.assign((size_t)n + 1, 0);
    for (int k = 0; k < n; ++k) G.out0[(size_t)k + 1] = G.out0[(size_t)k] + req[k].ncost + req[k].nrhs;
    const size_t nout = (size_t)G.out0[(size_t)n];
    std::vector<int> e_idx, irange((size_t)2 * N, 0);
    std::vector<double> e_val, tol((size_t)N, 0.0);
    std::vector<DzgRangeItem> items;
    G.iseg = bh::Segments{};
    for (int bk = 0; bk < bh::kBuckets; ++bk) { // by bucket, in call order within one
        for (int k = 0; k < n; ++k) {
            const int id = ids ? (int)ids[k] : k;
            if (!listed[k] || bh::bucket_of(P.desc[(size_t)id].m) != bk) continue;
            const dzg_ranging_req &rq = req[k];
            tol[(size_t)id] = rq.pivot_tol == 0.0 ? 1e-9 : rq.pivot_tol;
            const long long cbase = (long long)e_idx.size();
            const int64_t ce = rq.ncost ? rq.cost_ptr[rq.ncost] : 0, re = rq.nrhs ? rq.rhs_ptr[rq.nrhs] : 0;
            const long long rbase = cbase + ce;
            e_idx.insert(e_idx.end(), rq.cost_idx, rq.cost_idx + ce);
            e_val.insert(e_val.end(), rq.cost_val, rq.cost_val + ce);
            e_idx.insert(e_idx.end(), rq.rhs_idx, rq.rhs_idx + re);
            e_val.insert(e_val.end(), rq.rhs_val, rq.rhs_val + re);
            irange[(size_t)2 * id] = (int)items.size();
            for (int64_t j = 0; j < rq.ncost; ++j)
                items.push_back({cbase + rq.cost_ptr[j], cbase + rq.cost_ptr[j + 1], G.out0[(size_t)k] + j, id, 1});
            for (int64_t j = 0; j < rq.nrhs; ++j)
                items.push_back({rbase + rq.rhs_ptr[j], rbase + rq.rhs_ptr[j + 1], G.out0[(size_t)k] + rq.ncost + j, id, 0});
            if (items.size() >= ((size_t)1 << 31) || e_idx.size() >= ((size_t)1 << 31))
                return dzg_set_error(DZG_E_ARG, "batch: too many directions");
            irange[(size_t)2 * id + 1] = (int)items.size();
        }
        G.iseg[(size_t)bk + 1] = (int)items.size();
    }
    G.any = !items.empty();
    if (!G.any) return 0;
    bh::Arena ar;
    G.tol = ar.add(sizeof(double) * N);
    G.irange = ar.add(sizeof(int) * 2 * N);
    G.item = ar.add(sizeof(DzgRangeItem) * items.size());
    G.eidx = ar.add(sizeof(int) * e_idx.size());
    G.eval = ar.add(sizeof(double) * e_val.size());
    G.up_end = ar.top;
    G.posmap = ar.add(sizeof(int) * (size_t)nvc);
    G.lo = ar.add(sizeof(double) * nout);
    G.hi = ar.add(sizeof(double) * nout);
    G.lov = ar.add(sizeof(int) * nout);
    G.hiv = ar.add(sizeof(int) * nout);
    G.top = ar.top;
    G.host.assign(G.top, 0);
    std::memcpy(G.host.data() + G.tol, tol.data(), sizeof(double) * N);
    std::memcpy(G.host.data() + G.irange, irange.data(), sizeof(int) * 2 * N);
    std::memcpy(G.host.data() + G.item, items.data(), sizeof(DzgRangeItem) * items.size());
    if (!e_idx.empty()) {
        std::memcpy(G.host.data() + G.eidx, e_idx.data(), sizeof(int) * e_idx.size());
        std::memcpy(G.host.data() + G.eval, e_val.data(), sizeof(double) * e_val.size());
    }
    return 0;
}

void dzg_steps::post_unpack_ranging(const PostRanging &G, int k, const dzg_ranging_req &rq, dzg_ranging &o, bool ok)
{
    if (!ok || !G.any) {
        dzg_ranging_none(&rq, &o);
        return;
    }
    const size_t at = (size_t)G.out0[(size_t)k];
    const double *lo = (const double *)(G.host.data() + G.lo) + at, *hi = (const double *)(G.host.data() + G.hi) + at;
    const int *lov = (const int *)(G.host.data() + G.lov) + at, *hiv = (const int *)(G.host.data() + G.hiv) + at;
    for (int64_t j = 0; j < rq.ncost; ++j) {
        if (o.cost_lo) o.cost_lo[j] = lo[j];
        if (o.cost_hi) o.cost_hi[j] = hi[j];
        if (o.cost_lo_var) o.cost_lo_var[j] = lov[j];
        if (o.cost_hi_var) o.cost_hi_var[j] = hiv[j];
    }
    for (int64_t j = 0; j < rq.nrhs; ++j) {
        if (o.rhs_lo) o.rhs_lo[j] = lo[rq.ncost + j];
        if (o.rhs_hi) o.rhs_hi[j] = hi[rq.ncost + j];
        if (o.rhs_lo_var) o.rhs_lo_var[j] = lov[rq.ncost + j];
        if (o.rhs_hi_var) o.rhs_hi_var[j] = hiv[rq.ncost + j];
    }
}

int dzg_steps::fast_post(const PostRun &R, const int *list, const bh::Segments &seg, const int *mmax)
{
    PArgs g;
    const bh::Layout &L = *R.L;
    unsigned char *dev = R.dev;
    g.lp = (const DzgBatchLp *)(dev + L.desc);
    g.A = (const double *)(dev + L.a);
    g.var_col = (const int *)(dev + L.vc);
    g.basis = (const int *)(dev + L.basis);
    g.nonbasis = (const int *)(dev + L.nonbasis);
    g.x = (const double *)(dev + L.x);
    g.xbar = (const double *)(dev + L.xbar);
    g.z = (const double *)(dev + L.z);
    g.zbar = (const double *)(dev + L.zbar);
    g.state = (const FState *)(dev + R.state);
    g.c = (const double *)(dev + R.S.c);
    g.rhs0 = (const double *)(dev + R.S.rhs0);
    g.dz = (double *)(dev + R.S.dz);
    g.y = (double *)(dev + R.S.y);
    g.d = (double *)(dev + R.S.d);
    g.scal = (double *)(dev + R.S.scal);
    g.pstat = (int *)(dev + R.S.pstat);
    g.duals = R.duals ? 1 : 0;
    g.rays = R.rays ? 1 : 0;
    g.ranging = R.rg && R.rg->any ? 1 : 0;
    if (g.ranging) {
        const PostRanging &G = *R.rg;
        g.tol = (const double *)(R.rdev + G.tol);
        g.irange = (const int *)(R.rdev + G.irange);
        g.item = (const DzgRangeItem *)(R.rdev + G.item);
        g.e_idx = (const int *)(R.rdev + G.eidx);
        g.e_val = (const double *)(R.rdev + G.eval);
        g.posmap = (int *)(R.rdev + G.posmap);
        g.lo = (double *)(R.rdev + G.lo);
        g.hi = (double *)(R.rdev + G.hi);
        g.lo_var = (int *)(R.rdev + G.lov);
        g.hi_var = (int *)(R.rdev + G.hiv);
    } else {
        g.tol = nullptr;
        g.irange = nullptr;
        g.item = nullptr;
        g.e_idx = nullptr;
        g.e_val = nullptr;
        g.posmap = nullptr;
        g.lo = g.hi = nullptr;
        g.lo_var = g.hi_var = nullptr;
    }
    for (int b = 0; b < bh::kBuckets; ++b) {
        const int cnt = seg[(size_t)b + 1] - seg[(size_t)b];
        if (cnt == 0) continue;
        g.mmax = mmax[b];
        launch_post_bucket(b, g, list + seg[(size_t)b], cnt, R.st);
        DZG_HIP(hipGetLastError());
    }
    return 0;
}

void dzg_steps::post_unpack(const DzgBatchLp &d, const PostDown &D, int i,
                            const dzg_result &r, dzg_duals *du, dzg_ray *ry)
{
    const struct { int m, n; } lp = {d.m, d.n};
    const int pstat = D.pstat()[i - D.i0];
    const double *sc = D.scal() + (size_t)PS * (size_t)(i - D.i0);
    const double *y = D.y() + (d.m_off - D.m0), *dd = D.d() + (d.vc_off - D.v0);
    if (du) {
        if (r.status != DZG_OPTIMAL || pstat != DZG_POST_DONE) {
            dzg_duals_none(du, r.objective);
        } else {
            du->reserved = 0;
            du->primal_obj = r.objective;
            du->source = DZG_DUALS_FRESH;
            du->dual_obj = sc[0];
            du->primal_infeas = sc[1];
            du->dual_infeas = sc[2];
            du->z_diff = sc[3] / std::max(1.0, sc[4]);
            if (du->y && lp.m) std::memcpy(du->y, y, sizeof(double) * (size_t)lp.m);
            if (du->d && lp.n) std::memcpy(du->d, dd, sizeof(double) * (size_t)lp.n);
        }
    }
    if (ry) {
        const bool ends = r.status == DZG_UNBOUNDED || r.status == DZG_INFEASIBLE;
        if (!ends || pstat != DZG_POST_DONE || sc[0] < 0.0) {
            dzg_ray_none(ry);
        } else {
            const bool primal = r.status == DZG_UNBOUNDED;
            ry->kind = primal ? DZG_RAY_PRIMAL : DZG_RAY_FARKAS;
            ry->var = (int64_t)sc[0];
            ry->pos = (int64_t)sc[1];
            ry->mu = sc[2];
            ry->value = sc[3];
            ry->violation = sc[4];
            ry->proven = ry->violation == 0.0 && (primal ? ry->value > 0.0 : ry->value < 0.0) ? 1 : 0;
            if (ry->d && lp.n) std::memcpy(ry->d, dd, sizeof(double) * (size_t)lp.n);
            if (ry->y && lp.m) std::memcpy(ry->y, y, sizeof(double) * (size_t)lp.m);
        }
    }
}

// STRICT's three launchers on the arena R describes: duals of the OPTIMAL LPs, their ranges (which read
// the fresh d), rays of the others.  list / seg: the listed LPs by bucket, as the host has them.
static int strict_launches(const dzg_steps::PostRun &R, const bh::Packed &P, const std::vector<int> &list,
                           const bh::Segments &seg, const int *mmax, const std::vector<int> &status_of)
{
    using namespace dzg_steps;
    const bh::Layout &L = *R.L;
    unsigned char *dev = R.dev;
    // the kernels take one list per launch: OPTIMAL first, then the rest, bucket by bucket
    std::vector<int> order;
    bh::Segments oseg{}, rseg{};
    for (int pass = 0; pass < 2; ++pass) {
        for (int b = 0; b < bh::kBuckets; ++b) {
            for (int k = seg[(size_t)b]; k < seg[(size_t)b + 1]; ++k)
                if ((status_of[(size_t)k] == DZG_OPTIMAL) == (pass == 0)) order.push_back(list[(size_t)k]);
            (pass == 0 ? oseg : rseg)[(size_t)b + 1] = (int)order.size();
        }
        if (pass == 0) rseg[0] = (int)order.size();
    }
    for (int b = 1; b <= bh::kBuckets; ++b) rseg[(size_t)b] = std::max(rseg[(size_t)b], rseg[0]);
    DZG_HIP(hipMemcpyAsync(dev + R.S.list, order.data(), sizeof(int) * order.size(), hipMemcpyHostToDevice, R.st));
    DZG_HIP(hipStreamSynchronize(R.st)); // (order may go)
    const int *dlist = (const int *)(dev + R.S.list);
    DzgDualsArgs a;
    a.lp = (const DzgBatchLp *)(dev + L.desc);
    a.A = (const double *)(dev + L.a);
    a.var_col = (const int *)(dev + L.vc);
    a.basis = (const int *)(dev + L.basis);
    a.nonbasis = (const int *)(dev + L.nonbasis);
    a.x = (const double *)(dev + L.x);
    a.z = (const double *)(dev + L.z);
    a.c = (const double *)(dev + R.S.c);
    a.rhs0 = (const double *)(dev + R.S.rhs0);
    a.y = (double *)(dev + R.S.y);
    a.d = (double *)(dev + R.S.d);
    a.scal = (double *)(dev + R.S.scal);
    if (R.duals)
        for (int b = 0; b < bh::kBuckets; ++b) {
            const int cnt = oseg[(size_t)b + 1] - oseg[(size_t)b];
            if (cnt == 0) continue;
            a.mmax = mmax[b];
            dzg_launch_duals_small(b, a, dlist + oseg[(size_t)b], cnt, R.st);
            DZG_HIP(hipGetLastError());
        }
    if (R.rg && R.rg->any) {
        const PostRanging &G = *R.rg;
        DzgRangingArgs g;
        g.lp = a.lp;
        g.A = a.A;
        g.var_col = a.var_col;
        g.basis = a.basis;
        g.nonbasis = a.nonbasis;
        g.x = a.x;
        g.d = a.d;
        g.tol = (const double *)(R.rdev + G.tol);
        g.item = (const DzgRangeItem *)(R.rdev + G.item);
        g.e_idx = (const int *)(R.rdev + G.eidx);
        g.e_val = (const double *)(R.rdev + G.eval);
        g.lo = (double *)(R.rdev + G.lo);
        g.hi = (double *)(R.rdev + G.hi);
        g.lo_var = (int *)(R.rdev + G.lov);
        g.hi_var = (int *)(R.rdev + G.hiv);
        for (int b = 0; b < bh::kBuckets; ++b) {
            const int cnt = G.iseg[(size_t)b + 1] - G.iseg[(size_t)b];
            if (cnt == 0) continue;
            g.mmax = mmax[b];
            dzg_launch_ranging_small(b, g, g.item + G.iseg[(size_t)b], cnt, R.st);
            DZG_HIP(hipGetLastError());
        }
    }
    if (R.rays) {
        DzgRaysArgs r;
        r.lp = a.lp;
        r.A = a.A;
        r.var_col = a.var_col;
        r.basis = a.basis;
        r.nonbasis = a.nonbasis;
        r.x = a.x;
        r.xbar = (const double *)(dev + L.xbar);
        r.z = a.z;
        r.zbar = (const double *)(dev + L.zbar);
        r.status = (const int *)(dev + R.status);
        r.c = a.c;
        r.rhs0 = a.rhs0;
        r.dz = (double *)(dev + R.S.dz);
        r.d = a.d;
        r.y = a.y;
        r.scal = a.scal;
        for (int b = 0; b < bh::kBuckets; ++b) {
            const int cnt = rseg[(size_t)b + 1] - rseg[(size_t)b];
            if (cnt == 0) continue;
            r.mmax = mmax[b];
            dzg_launch_rays_small(b, r, dlist + rseg[(size_t)b], cnt, R.st);
            DZG_HIP(hipGetLastError());
        }
    }
    return 0;
}

static thread_local double t_post_ms = 0.0;
double &dzg_steps::post_ms() { return t_post_ms; }
extern "C" double dzg_debug_batch_post_ms(void) { return t_post_ms; }

int dzg_steps::post_pass(PostRun R, bool strict, const bh::Packed &P, int n, const int64_t *ids,
                         const dzg_result *res, const dzg_batch_post &post, int64_t *h2d, int64_t *d2h, double *ms)
{
    const int want_numerics = strict ? DZG_NUMERICS_STRICT : DZG_NUMERICS_FAST;
    auto fast_result = [&](int k) { return res[k].numerics_used == want_numerics; }; // (this pass's results)
    auto wants = [&](int k) {
        const int s = res[k].status;
        if (s == DZG_OPTIMAL) return post.du != nullptr || post.req != nullptr;
        return (s == DZG_UNBOUNDED || s == DZG_INFEASIBLE) && post.ry != nullptr;
    };
    // ---- the lists by bucket, in call order within a bucket
    std::vector<unsigned char> listed((size_t)n, 0), ranged((size_t)n, 0);
    std::vector<int> list, status_of;
    bh::Segments seg{};
    int mmax[bh::kBuckets] = {0, 0, 0, 0};
    for (int b = 0; b < bh::kBuckets; ++b) {
        for (int k = 0; k < n; ++k) {
            const int id = ids ? (int)ids[k] : k;
            const int m = P.desc[(size_t)id].m;
            if (bh::bucket_of(m) != b || m == 0 || !fast_result(k) || !wants(k)) continue;
            listed[(size_t)k] = 1;
            ranged[(size_t)k] = post.req && res[k].status == DZG_OPTIMAL;
            list.push_back(id);
            status_of.push_back(res[k].status);
            mmax[b] = std::max(mmax[b], m);
        }
        seg[(size_t)b + 1] = (int)list.size();
    }
    PostRanging G;
    bh::Events ev;
    struct Free {
        unsigned char *p = nullptr;
        ~Free() { if (p) (void)hipFree(p); }
    } rdev;
    PostDown down;
    if (!list.empty()) {
        if (post.req)
            if (const int rc = post_ranging_pack(G, post.req, n, ids, ranged.data(), P)) return rc;
        DZG_HIP(hipMemcpyAsync(R.dev + R.S.list, list.data(), sizeof(int) * list.size(), hipMemcpyHostToDevice, R.st));
        if (h2d) *h2d += (int64_t)(sizeof(int) * list.size());
        if (G.any) {
            if (R.rkeep) { // the caller's own allocation, kept between calls: grown, never shrunk
                if (*R.rkeep_bytes < G.top) {
                    if (*R.rkeep) (void)hipFree(*R.rkeep);
                    *R.rkeep = nullptr;
                    *R.rkeep_bytes = 0;
                    DZG_HIP(hipMalloc((void **)R.rkeep, G.top));
                    *R.rkeep_bytes = G.top;
                }
            } else {
                DZG_HIP(hipMalloc((void **)&rdev.p, G.top));
            }
            unsigned char *const rd = R.rkeep ? *R.rkeep : rdev.p;
            DZG_HIP(hipMemcpyAsync(rd, G.host.data(), G.up_end, hipMemcpyHostToDevice, R.st));
            if (h2d) *h2d += (int64_t)G.up_end;
            R.rg = &G;
            R.rdev = rd;
        }
        R.duals = post.du != nullptr || post.req != nullptr;
        R.rays = post.ry != nullptr;
        DZG_HIP(hipEventCreate(&ev.e0));
        DZG_HIP(hipEventCreate(&ev.e1));
        DZG_HIP(hipEventRecord(ev.e0, R.st));
        if (strict) {
            if (const int rc = strict_launches(R, P, list, seg, mmax, status_of)) return rc;
        } else if (const int rc = fast_post(R, (const int *)(R.dev + R.S.list), seg, mmax)) {
            return rc;
        }
        DZG_HIP(hipEventRecord(ev.e1, R.st));
        // ---- per section the span from the first to the last listed LP comes down
        const int lo = *std::min_element(list.begin(), list.end()), hi = *std::max_element(list.begin(), list.end());
        const DzgBatchLp &dl = P.desc[(size_t)lo], &dh = P.desc[(size_t)hi];
        // (the host buffer holds those spans alone: y, d, the scalars, the post statuses)
        down.m0 = dl.m_off;
        down.v0 = dl.vc_off;
        down.i0 = lo;
        const size_t ny = (size_t)(dh.m_off + dh.m - dl.m_off), nd = (size_t)(dh.vc_off + dh.n - dl.vc_off),
                     ni = (size_t)(hi - lo + 1);
        down.o_d = sizeof(double) * ny;
        down.o_scal = down.o_d + sizeof(double) * nd;
        down.o_pstat = down.o_scal + sizeof(double) * PS * ni;
        down.buf.resize(down.o_pstat + sizeof(int) * ni);
        auto span = [&](size_t at, size_t sec, size_t bytes) {
            if (d2h) *d2h += (int64_t)bytes;
            return hipMemcpyAsync(down.buf.data() + at, R.dev + sec, bytes, hipMemcpyDeviceToHost, R.st);
        };
        DZG_HIP(span(0, R.S.y + sizeof(double) * (size_t)dl.m_off, sizeof(double) * ny));
        DZG_HIP(span(down.o_d, R.S.d + sizeof(double) * (size_t)dl.vc_off, sizeof(double) * nd));
        DZG_HIP(span(down.o_scal, R.S.scal + sizeof(double) * PS * (size_t)lo, sizeof(double) * PS * ni));
        DZG_HIP(span(down.o_pstat, R.S.pstat + sizeof(int) * (size_t)lo, sizeof(int) * ni));
        if (G.any) {
            DZG_HIP(hipMemcpyAsync(G.host.data() + G.lo, R.rdev + G.lo, G.top - G.lo, hipMemcpyDeviceToHost, R.st));
            if (d2h) *d2h += (int64_t)(G.top - G.lo);
        }
        DZG_HIP(hipStreamSynchronize(R.st));
        float t = 0.0f;
        DZG_HIP(hipEventElapsedTime(&t, ev.e0, ev.e1));
        if (ms) *ms += t;
    }
    // ---- this pass's results' outputs; the other numerics' are its own pass's to fill
    int *pstat = down.buf.empty() ? nullptr : (int *)(down.buf.data() + down.o_pstat);
    if (strict && pstat) // (STRICT's kernels keep no post status: what was listed is done)
        for (int id : list) pstat[id - down.i0] = DZG_POST_DONE;
    for (int k = 0; k < n; ++k) {
        if (!fast_result(k)) continue;
        const int id = ids ? (int)ids[k] : k;
        if (!listed[(size_t)k]) {
            if (post.du) dzg_duals_none(&post.du[k], res[k].objective);
            if (post.ry) dzg_ray_none(&post.ry[k]);
            if (post.req) dzg_ranging_none(&post.req[k], &post.rg[k]);
            continue;
        }
        post_unpack(P.desc[(size_t)id], down, id, res[k], post.du ? &post.du[k] : nullptr,
                    post.ry ? &post.ry[k] : nullptr);
        if (post.req) post_unpack_ranging(G, k, post.req[k], post.rg[k], ranged[(size_t)k] && pstat[id - down.i0] == DZG_POST_DONE);
    }
    return 0;
}
