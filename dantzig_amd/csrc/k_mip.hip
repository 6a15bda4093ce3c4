// k_mip.hip -- the node LPs of a branch-and-bound round, one workgroup per node, STRICT numerics.
//
// The simplex loop is k_batch.hip's (batch_strict.h) and the round loop, row buckets and chunked
// launches are the batch's own (batch_host.h): the same LDS carve-up and pivots_per_launch slicing,
// so a node LP ends exactly where dzg_batch_solve (and hence dzg_model_solve) would end it.  What is
// new here:
//
//   * shared structures.  A node's standard form differs from its structure's only in the
//     right-hand side of the bound rows of integer variables (model.cpp: a finite bound is a row
//     x+ - x- <= ub / -x+ + x- <= -lb, so tightening it moves b only).  A, var_col, c, the initial
//     nonbasis, z0 = -c and the row table live once per structure in one device arena; every node of
//     the structure reads that copy.
//   * device-side initialisation.  Per node the host uploads a structure id and two doubles per
//     integer variable.  On its first slice (iter < 0) the workgroup builds x = rhs from the row
//     table, x̄ = z̄ = 1, the slack basis and the structure's nonbasis and z0.
//   * device epilogue on OPTIMAL.  The objective is one sequential sum in basis-position order
//     (unpack_common's host loop in batch_host.h, unfused); the user values are x+ - x- found
//     through a copy of the basis in LDS; the integrality test and the branching choice are mip_branch_choice
//     (mip_internal.h), the host's own code.  The node's compact record is written; values stay on
//     the device unless the node is integral.
//   * warm starts (dzg_mip_opts.warm_start).  A node with a parent-state slot takes
//     the parent's final basis, nonbasis and z from the slot pool on its first slice, sets both
//     perturbation vectors to one and solves B x = b in LDS for its own right-hand side; the loop
//     then runs from iteration 0 as for any node.  The attempt stands only if it ends OPTIMAL with
//     every carried x and z >= -DZG_MIP_WARM_TOL; otherwise the workgroup marks the node restarted
//     and re-queues it, and its next slice initialises it cold.  k_mip_save copies the final state
//     of the nodes the host branches on from the round arena into their slots.
//   * FAST node LPs (dzg_mip_node_opts.numerics, DESIGN.md 7c "FAST node LPs").  k_mip_node_fast
//     runs batch_fast.h's iteration, k_batch_fast's, on a control block of the node's own: cold
//     from the slack basis, or warm from the parent's basis and nonbasis with the restart state of
//     DESIGN.md 7l (W = B^-1, x = W rhs, y = W^T c_B, z = -dz - c_N; the slot's z is not used), the
//     first launch pivoting on that same W.  An attempt that ends OPTIMAL is certified from its
//     final basis: W is rebuilt, x and z are recomputed by the restart formulas and written over
//     the carried ones, and the node stands only if all of them are >= -DZG_MIP_WARM_TOL.  Every
//     other end puts the node on the strict list, which k_mip_node then solves cold in the same
//     round.  Both kernels end in one epilogue (node_epilogue).
#include <algorithm>
#include <cstring>
#include <string>
#include <vector>

#include "batch_fast.h"
#include "batch_host.h"
#include "batch_steps.h"
#include "batch_strict.h"
#include "common.h"
#include "fast_decide.h"
#include "mip_internal.h"

using dzg_internal::MipNodeRecord;
using dzg_internal::MipStructure;

namespace {

namespace bh = dzg_bh;
using bh::bucket_of;
using bh::kBuckets;
using dzg_bs::lds_bytes;

// One structure: offsets into the double / int pools (elements).
struct SDesc {
    long long a_off, b0_off, c_off, z0_off;          // dpool
    long long vc_off, ri_off, bs_off, nb_off, pv_off; // ipool (pv: pos_var then neg_var)
    int m, n;
    double constant;
};

// One node of the round: its structure and its state offsets (elements).
struct NDesc {
    long long m_off, q_off;
    int sid;
    int pslot; // the parent's slot in the state pool, -1: a cold node
};

struct MArgs {
    const SDesc *sd;
    const double *dpool;
    const int *ipool;
    const int *int_vars;
    int nint, nvars;
    const NDesc *nd;
    const double *bnd; // 2 * nint per node
    int *basis, *nonbasis;
    double *x, *xbar, *z, *zbar, *dz;
    long long *iter; // < 0: not initialised yet
    int *status;
    MipNodeRecord *rec;
    double *values; // nvars per node
    long long max_iter;
    double eps, int_tol;
    int ppl, mmax;
    // the parent-state pool: per slot pool_si ints (basis, then nonbasis) and pool_sz doubles (z)
    const int *pool_i;
    const double *pool_z;
    long long pool_si, pool_sz;
};

constexpr int kWarmRestarted = 2; // MipNodeRecord::warm
constexpr int kFastAccepted = 1, kFastRejected = 2; // MipNodeRecord::fast

// Row r's right-hand side of node `id` (mip_internal.h, MipStructure)
__device__ __forceinline__ double node_rhs(const double *b0, const int *ri, const double *bnd, int r)
{
    const int code = ri[r];
    return code < 0 ? b0[r] : ((code & 1) ? bnd[code] : -bnd[code]);
}

// What follows an OPTIMAL node LP, from its final basis and x in global memory: the user values, the
// objective, the integrality test and the branching choice into rec.  s_mem: m ints of LDS that
// nothing else needs any more.  Every thread calls it; thread 0's rec is the one that counts.
template <int BLOCK>
__device__ __forceinline__ void node_epilogue(const MArgs &g, const SDesc &D, int id, int m, const int *basis,
                                              const double *x, double *s_mem, MipNodeRecord &rec)
{
    const double *c = g.dpool + D.c_off;
    const int *pv = g.ipool + D.pv_off, *nv = pv + g.nvars;
    double *vals = g.values + (long long)id * g.nvars;
    int *sb = (int *)s_mem; // the final basis, m entries
    __syncthreads();
    for (int p = threadIdx.x; p < m; p += BLOCK) sb[p] = basis[p];
    __syncthreads();
    // Simplex::solution (model.cpp solution_values): x+ - x-, 0.0 for a nonbasic part
    for (int u = threadIdx.x; u < g.nvars; u += BLOCK) {
        double val = 0.0;
        const int jp = pv[u], jn = nv[u];
        if (jp >= 0) {
            double pos = 0.0, neg = 0.0;
            for (int p = 0; p < m; ++p) {
                if (sb[p] == jp) pos = x[p];
                if (sb[p] == jn) neg = x[p];
            }
            val = pos - neg;
        }
        vals[u] = val;
    }
    __syncthreads(); // vals is read by thread 0 below
    if (threadIdx.x == 0) {
        double sum = 0.0; // objective_value, src/simplex.rs:345-352, basis-position order
        for (int p = 0; p < m; ++p) {
            const double prod = c[sb[p]] * x[p];
            sum = sum + prod;
        }
        rec.objective = D.constant + sum;
        dzg_internal::mip_branch_choice(vals, g.int_vars, g.nint, g.int_tol, &rec.branch, &rec.value,
                                        &rec.integral);
    }
}

template <int BLOCK>
__global__ __launch_bounds__(BLOCK) void k_mip_node(MArgs g, const int *__restrict__ list,
                                                    int *__restrict__ next_list,
                                                    int *__restrict__ next_count)
{
    extern __shared__ __attribute__((aligned(16))) double s_mem[];
    const int id = list[blockIdx.x];
    const NDesc N = g.nd[id];
    const SDesc D = g.sd[N.sid];
    const int m = D.m, q = D.n - D.m;
    dzg_bs::LpState S;
    S.A = g.dpool + D.a_off;
    S.var_col = g.ipool + D.vc_off;
    S.m = m;
    S.q = q;
    S.basis = g.basis + N.m_off;
    S.nonbasis = g.nonbasis + N.q_off;
    S.x = g.x + N.m_off;
    S.xbar = g.xbar + N.m_off;
    S.z = g.z + N.q_off;
    S.zbar = g.zbar + N.q_off;
    S.dz = g.dz + N.q_off;
    S.log_kind = S.log_enter = S.log_leave = nullptr;
    S.log_mu = nullptr;
    S.log_cap = 0;
    long long it = g.iter[id];
    // a warm attempt until it is rejected; the rejection is recorded in the node's record
    const bool warm_try = N.pslot >= 0 && g.rec[id].warm != kWarmRestarted;
    if (it < 0 && warm_try) { // first slice of a warm node: the parent's final state, x = B^-1 b
        const double *b0 = g.dpool + D.b0_off, *bnd = g.bnd + (long long)id * 2 * g.nint;
        const int *ri = g.ipool + D.ri_off;
        const int *pi = g.pool_i + N.pslot * g.pool_si;
        const double *pz = g.pool_z + N.pslot * g.pool_sz;
        for (int r = threadIdx.x; r < m; r += BLOCK) {
            S.basis[r] = pi[r];
            S.xbar[r] = 1.0;
        }
        for (int k = threadIdx.x; k < q; k += BLOCK) {
            S.nonbasis[k] = pi[m + k];
            S.z[k] = pz[k];
            S.zbar[k] = 1.0;
        }
        __syncthreads(); // the gather reads the basis
        if (m > 0) {
            double *W = s_mem; // strict_steps' carve-up: W, dx[mmax], v[mmax], one int
            int *s_flag = (int *)(s_mem + (long long)g.mmax * (g.mmax + 1) + 2 * g.mmax);
            dzg_bs::gather<BLOCK>(W, m, S.A, S.basis, S.var_col, 0, S.basis[0], -1);
            // column m: the node's right-hand side in place of an entering column (the same
            // thread wrote the entry it overwrites)
            for (int r = threadIdx.x; r < m; r += BLOCK) {
                const int code = ri[r];
                W[r * (m + 1) + m] = code < 0 ? b0[r] : ((code & 1) ? bnd[code] : -bnd[code]);
            }
            dzg_bs::lu_solve_lds<BLOCK>(W, m, s_flag);
            for (int r = threadIdx.x; r < m; r += BLOCK) S.x[r] = W[r * (m + 1) + m];
        }
        it = 0;
        __syncthreads();
    } else if (it < 0) { // first slice: the node's initial state (model.cpp build(), Simplex::new)
        const double *b0 = g.dpool + D.b0_off, *bnd = g.bnd + (long long)id * 2 * g.nint;
        const int *ri = g.ipool + D.ri_off, *bs = g.ipool + D.bs_off, *nb = g.ipool + D.nb_off;
        const double *z0 = g.dpool + D.z0_off;
        for (int r = threadIdx.x; r < m; r += BLOCK) {
            const int code = ri[r];
            S.x[r] = code < 0 ? b0[r] : ((code & 1) ? bnd[code] : -bnd[code]);
            S.xbar[r] = 1.0;
            S.basis[r] = bs[r];
        }
        for (int k = threadIdx.x; k < q; k += BLOCK) {
            S.nonbasis[k] = nb[k];
            S.z[k] = z0[k];
            S.zbar[k] = 1.0;
        }
        it = 0;
        __syncthreads();
    }
    const int status = dzg_bs::strict_steps<BLOCK>(S, s_mem, g.mmax, it, g.max_iter, g.eps, g.ppl);
    if (status == DZG_RUNNING) {
        if (threadIdx.x == 0) {
            g.iter[id] = it;
            next_list[atomicAdd(next_count, 1)] = id;
        }
        return;
    }
    long long warm_it = 0;
    int warm = 0;
    if (warm_try) {
        int reject = status != DZG_OPTIMAL;
        if (!reject) { // the signs of the carried x and z themselves, bars ignored; NaN fails
            int *s_bad = (int *)s_mem; // W is free after the loop
            __syncthreads();
            if (threadIdx.x == 0) *s_bad = 0;
            __syncthreads();
            int bad = 0;
            for (int p = threadIdx.x; p < m; p += BLOCK) bad |= !(S.x[p] >= -DZG_MIP_WARM_TOL);
            for (int k = threadIdx.x; k < q; k += BLOCK) bad |= !(S.z[k] >= -DZG_MIP_WARM_TOL);
            if (bad) *s_bad = 1; // every writer stores the same value
            __syncthreads();
            reject = *s_bad;
        }
        if (reject) { // restart cold inside the round: the next slice sees the mark
            if (threadIdx.x == 0) {
                g.rec[id].warm = kWarmRestarted;
                g.rec[id].warm_iterations = it;
                g.iter[id] = -1;
                next_list[atomicAdd(next_count, 1)] = id;
            }
            return;
        }
        warm = 1;
        warm_it = it;
    } else if (N.pslot >= 0) { // the cold run of a restarted node
        warm = kWarmRestarted;
        warm_it = g.rec[id].warm_iterations;
        it += warm_it;
    }
    MipNodeRecord rec;
    rec.status = status;
    rec.iterations = it;
    rec.warm = warm;
    rec.warm_iterations = warm_it;
    rec.branch = -1;
    rec.objective = 0.0;
    rec.value = 0.0;
    rec.integral = 0;
    rec.fast = 0;
    rec.fast_iterations = 0;
    if (status == DZG_OPTIMAL) node_epilogue<BLOCK>(g, D, id, m, S.basis, S.x, s_mem, rec); // W is free after the loop
    if (threadIdx.x == 0) {
        // a node that k_mip_node_fast gave up on: its mark stays, its pivots are added
        rec.fast = g.rec[id].fast;
        rec.fast_iterations = g.rec[id].fast_iterations;
        rec.iterations = rec.iterations + rec.fast_iterations;
        g.rec[id] = rec;
        g.status[id] = status;
        g.iter[id] = it;
    }
}

// What k_mip_node_fast needs beside MArgs.
struct FNode {
    dzg_bf::FState *state;      // one block per node of the round, written on the node's first slice
    const dzg_bf::FState *tmpl; // the block every node starts from (the host's start_ctl)
    NDesc *nd;                  // the round's descriptors again: a rejected node gives up its parent slot
    int ppl, refactor_every;    // FAST pivots per launch; pivots between two inversions inside one
};

// One node LP in FAST numerics (the header of this file).  LDS is k_batch_fast's
// carve-up, fast_lds_bytes(mmax).  A node that is still running goes to next_list as in k_mip_node; a
// node whose attempt is discarded goes to strict_list with rec.fast = kFastRejected, iter = -1 and no
// parent slot, so that k_mip_node solves it cold.  Every sum's order depends on m alone.
template <int BLOCK, int PL>
__global__ __launch_bounds__(BLOCK) void k_mip_node_fast(MArgs g, FNode f, const int *__restrict__ list,
                                                         int *__restrict__ next_list,
                                                         int *__restrict__ next_count,
                                                         int *__restrict__ strict_list,
                                                         int *__restrict__ strict_count)
{
    extern __shared__ __attribute__((aligned(16))) double s_mem[];
    const int id = list[blockIdx.x];
    const NDesc N = g.nd[id];
    const SDesc D = g.sd[N.sid];
    const int m = D.m, q = D.n - D.m;
    dzg_bf::FastLp P;
    P.A = g.dpool + D.a_off;
    P.var_col = g.ipool + D.vc_off;
    P.basis = g.basis + N.m_off;
    P.nonbasis = g.nonbasis + N.q_off;
    P.x = g.x + N.m_off;
    P.xbar = g.xbar + N.m_off;
    P.z = g.z + N.q_off;
    P.zbar = g.zbar + N.q_off;
    P.dz = g.dz + N.q_off;
    P.m = m;
    P.q = q;
    P.log_kind = P.log_enter = P.log_leave = nullptr;
    P.log_mu = P.log_margin = nullptr;
    P.log_off = P.log_cap = 0;
    const dzg_bf::FastLds S = dzg_bf::carve(s_mem, g.mmax, m);
    DzgCtl *sc = S.sc;
    int *s_flag = S.s_flag; // [0], [1]: build_inverse's; [2]: a non-finite x or z; [3]: a failed sign check
    const double *b0 = g.dpool + D.b0_off, *bnd = g.bnd + (long long)id * 2 * g.nint;
    const double *c = g.dpool + D.c_off;
    const int *ri = g.ipool + D.ri_off;
    const auto rhs = [b0, ri, bnd](int r) { return node_rhs(b0, ri, bnd, r); };
    dzg_bf::FState *gs = f.state + id;
    const bool lead = threadIdx.x == 0;
    const bool first = g.iter[id] < 0, warm = N.pslot >= 0;

    const dzg_bf::FState *src = first ? f.tmpl : gs;
    for (int i = threadIdx.x; i < (int)(sizeof(DzgCtl) / sizeof(int)); i += BLOCK)
        ((int *)sc)[i] = ((const int *)&src->ctl)[i];
    double max_err_life = src->max_err_life;
    long long refactors = src->refactors;
    if (lead) s_flag[2] = s_flag[3] = 0;
    __syncthreads();

    int status = DZG_RUNNING;
    bool w_built = false;
    if (first && warm) { // the parent's final basis and nonbasis; the restart state of that basis
        const int *pi = g.pool_i + N.pslot * g.pool_si;
        for (int r = threadIdx.x; r < m; r += BLOCK) P.basis[r] = pi[r];
        for (int k = threadIdx.x; k < q; k += BLOCK) P.nonbasis[k] = pi[m + k];
        __syncthreads(); // the inversion reads the basis
        int inverted = 0;
        const int bad = m > 0 ? dzg_bf::build_inverse<BLOCK, PL>(S.W, S.ld, m, P.A, P.var_col, P.basis, S.acol,
                                                                 S.piv, s_flag, inverted)
                              : 0;
        refactors += inverted;
        if (!bad) dzg_bf::restart_state<BLOCK, PL>(P, S, c, rhs);
        if (bad || s_flag[2]) {
            status = DZG_SINGULAR;
            if (lead) sc->status = DZG_SINGULAR;
            __syncthreads();
        }
        w_built = true; // the first launch pivots on this W
    } else if (first) { // k_mip_node's cold state (model.cpp build(), Simplex::new)
        const int *bs = g.ipool + D.bs_off, *nb = g.ipool + D.nb_off;
        const double *z0 = g.dpool + D.z0_off;
        for (int r = threadIdx.x; r < m; r += BLOCK) {
            P.x[r] = rhs(r);
            P.xbar[r] = 1.0;
            P.basis[r] = bs[r];
        }
        for (int k = threadIdx.x; k < q; k += BLOCK) {
            P.nonbasis[k] = nb[k];
            P.z[k] = z0[k];
            P.zbar[k] = 1.0;
        }
        __syncthreads();
    }
    if (status == DZG_RUNNING)
        status = dzg_bf::fast_steps<BLOCK, PL>(P, S, g.eps, f.ppl, f.refactor_every, w_built, max_err_life,
                                               refactors);
    const long long it = sc->iter; // every path here has passed a barrier since the last write
    if (status == DZG_RUNNING) {
        for (int i = threadIdx.x; i < (int)(sizeof(DzgCtl) / sizeof(int)); i += BLOCK)
            ((int *)&gs->ctl)[i] = ((const int *)sc)[i];
        if (lead) {
            gs->max_err_life = max_err_life;
            gs->refactors = refactors;
            g.iter[id] = it;
            next_list[atomicAdd(next_count, 1)] = id;
        }
        return;
    }
    // ---- the certificate: x and z of the final basis, recomputed; their signs, bars ignored, NaN fails
    int accept = 0;
    if (status == DZG_OPTIMAL) {
        int inverted = 0;
        const int bad = m > 0 ? dzg_bf::build_inverse<BLOCK, PL>(S.W, S.ld, m, P.A, P.var_col, P.basis, S.acol,
                                                                 S.piv, s_flag, inverted)
                              : 0;
        if (!bad) {
            dzg_bf::restart_state<BLOCK, PL>(P, S, c, rhs);
            int neg = 0;
            for (int p = threadIdx.x; p < m; p += BLOCK) neg |= !(P.x[p] >= -DZG_MIP_WARM_TOL);
            for (int k = threadIdx.x; k < q; k += BLOCK) neg |= !(P.z[k] >= -DZG_MIP_WARM_TOL);
            if (neg) s_flag[3] = 1; // every writer stores the same value
            __syncthreads();
            accept = !s_flag[2] && !s_flag[3];
        }
    }
    if (!accept) {
        if (lead) {
            g.rec[id].fast = kFastRejected;
            g.rec[id].fast_iterations = it;
            g.iter[id] = -1;
            f.nd[id].pslot = -1;
            strict_list[atomicAdd(strict_count, 1)] = id;
        }
        return;
    }
    MipNodeRecord rec;
    rec.status = status;
    rec.iterations = it;
    rec.warm = warm ? 1 : 0;
    rec.warm_iterations = warm ? it : 0;
    rec.branch = -1;
    rec.objective = 0.0;
    rec.value = 0.0;
    rec.integral = 0;
    rec.fast = kFastAccepted;
    rec.fast_iterations = it;
    node_epilogue<BLOCK>(g, D, id, m, P.basis, P.x, s_mem, rec); // W is spent
    if (lead) {
        g.rec[id] = rec;
        g.status[id] = status;
        g.iter[id] = it;
    }
}

// The final basis, nonbasis and z of round node pairs[2 i] into pool slot pairs[2 i + 1].
__global__ __launch_bounds__(64) void k_mip_save(MArgs g, const int *__restrict__ pairs,
                                                 int *__restrict__ pool_i,
                                                 double *__restrict__ pool_z)
{
    const int id = pairs[2 * blockIdx.x], slot = pairs[2 * blockIdx.x + 1];
    const NDesc N = g.nd[id];
    const SDesc D = g.sd[N.sid];
    const int m = D.m, q = D.n - D.m;
    int *pi = pool_i + slot * g.pool_si;
    double *pz = pool_z + slot * g.pool_sz;
    for (int r = threadIdx.x; r < m; r += 64) pi[r] = g.basis[N.m_off + r];
    for (int k = threadIdx.x; k < q; k += 64) {
        pi[m + k] = g.nonbasis[N.q_off + k];
        pz[k] = g.z[N.q_off + k];
    }
}

void launch_bucket(int b, const MArgs &g, const int *list, int n, int *next_list, int *next_count,
                   hipStream_t st)
{
    const size_t lds = lds_bytes(g.mmax);
    bh::for_each_chunk(b, n, [&](int c0, int grid) {
        bh::with_block(b, [&](auto block) {
            constexpr int BLOCK = decltype(block)::value;
            hipLaunchKernelGGL(k_mip_node<BLOCK>, dim3(grid), dim3(BLOCK), lds, st, g, list + c0, next_list,
                               next_count);
        });
    });
}

// The FAST attempts list[0..n) of row bucket b: k_batch_fast's instantiations and LDS.
void launch_bucket_fast(int b, const MArgs &g, const FNode &f, const int *list, int n, int *next_list,
                        int *next_count, int *strict_list, int *strict_count, hipStream_t st)
{
    const size_t lds = dzg_bf::fast_lds_bytes(g.mmax);
    if (b == 3) { // more than 64 KiB of dynamic LDS: say so once (a runtime that needs no telling ignores it)
        static const hipError_t attr =
            hipFuncSetAttribute(reinterpret_cast<const void *>(k_mip_node_fast<256, 64>),
                                hipFuncAttributeMaxDynamicSharedMemorySize,
                                (int)dzg_bf::fast_lds_bytes(DZG_BATCH_MAX_ROWS));
        (void)attr;
    }
    bh::for_each_chunk(b, n, [&](int c0, int grid) {
        const dim3 block(bh::kBlock[b]);
        // the pricing lanes per column follow the bucket's rows: 16, 32, then the whole wave
        if (b == 0)
            hipLaunchKernelGGL((k_mip_node_fast<64, 16>), dim3(grid), block, lds, st, g, f, list + c0, next_list,
                               next_count, strict_list, strict_count);
        else if (b == 1)
            hipLaunchKernelGGL((k_mip_node_fast<64, 32>), dim3(grid), block, lds, st, g, f, list + c0, next_list,
                               next_count, strict_list, strict_count);
        else if (b == 2)
            hipLaunchKernelGGL((k_mip_node_fast<128, 64>), dim3(grid), block, lds, st, g, f, list + c0, next_list,
                               next_count, strict_list, strict_count);
        else
            hipLaunchKernelGGL((k_mip_node_fast<256, 64>), dim3(grid), block, lds, st, g, f, list + c0, next_list,
                               next_count, strict_list, strict_count);
    });
}

} // namespace

namespace dzg_internal {

struct MipGpu {
    int device = 0, nvars = 0, nint = 0;
    hipStream_t st = nullptr;
    // structures: host copies, and the device arena [SDesc | int_vars | ipool | dpool]
    std::vector<MipStructure> structs;
    bool dirty = true;
    unsigned char *sdev = nullptr;
    MArgs base{};
    // the round arena, grown on demand and reused
    unsigned char *rdev = nullptr;
    size_t rcap = 0;
    std::vector<int> int_vars;
    // warm starts: the parent-state pool.  Slot strides are fixed by the first structure (every
    // structure of one model has the same q = 2 x its variables; m <= DZG_BATCH_MAX_ROWS).  Slots
    // are handed out on the host (free list first); the arrays grow when a save needs more.
    int pool_q = -1;
    int *pool_i = nullptr;
    double *pool_z = nullptr;
    int pool_cap = 0, pool_used = 0;
    std::vector<int> pool_free;
    int *pairs_dev = nullptr;
    int pairs_cap = 0;
    MArgs last{};      // the last round's arguments: where k_mip_save finds the final states
    int last_count = 0;
};

int mip_gpu_create(MipGpu **out, int device, int nvars, const std::vector<int> &int_vars)
{
    *out = nullptr;
    if (const int rc = bh::use_device(device)) return rc;
    MipGpu *g = new MipGpu;
    g->device = device;
    g->nvars = nvars;
    g->nint = (int)int_vars.size();
    g->int_vars = int_vars;
    hipError_t e = hipStreamCreateWithFlags(&g->st, hipStreamNonBlocking);
    if (e != hipSuccess) {
        delete g;
        return dzg_set_error(DZG_E_DEVICE, std::string("hipStreamCreateWithFlags: ") + hipGetErrorString(e));
    }
    *out = g;
    return 0;
}

void mip_gpu_destroy(MipGpu *g)
{
    if (!g) return;
    if (g->sdev) (void)hipFree(g->sdev);
    if (g->rdev) (void)hipFree(g->rdev);
    if (g->pool_i) (void)hipFree(g->pool_i);
    if (g->pool_z) (void)hipFree(g->pool_z);
    if (g->pairs_dev) (void)hipFree(g->pairs_dev);
    if (g->st) (void)hipStreamDestroy(g->st);
    delete g;
}

int mip_gpu_add_structure(MipGpu *g, MipStructure &&s)
{
    if (g->pool_q < 0) g->pool_q = s.n - s.m;
    g->structs.push_back(std::move(s));
    g->dirty = true;
    return (int)g->structs.size() - 1;
}

static int upload_structures(MipGpu *g)
{
    const size_t ns = g->structs.size();
    std::vector<SDesc> sd(ns);
    std::vector<double> dpool;
    std::vector<int> ipool;
    for (size_t i = 0; i < ns; ++i) {
        const MipStructure &s = g->structs[i];
        SDesc &d = sd[i];
        d.m = s.m;
        d.n = s.n;
        d.constant = s.constant;
        auto put_d = [&](const std::vector<double> &v) {
            const long long off = (long long)dpool.size();
            dpool.insert(dpool.end(), v.begin(), v.end());
            return off;
        };
        auto put_i = [&](const std::vector<int> &v) {
            const long long off = (long long)ipool.size();
            ipool.insert(ipool.end(), v.begin(), v.end());
            return off;
        };
        d.a_off = put_d(s.a);
        d.b0_off = put_d(s.b0);
        d.c_off = put_d(s.c);
        d.z0_off = put_d(s.z0);
        d.vc_off = put_i(s.var_col);
        d.ri_off = put_i(s.row_int);
        d.bs_off = put_i(s.basis0);
        d.nb_off = put_i(s.nonbasis0);
        d.pv_off = put_i(s.pos_var);
        put_i(s.neg_var); // directly after pos_var
    }
    bh::Arena ar;
    const size_t o_sd = ar.add(sizeof(SDesc) * ns), o_iv = ar.add(sizeof(int) * (g->int_vars.size() + 1)),
                 o_ip = ar.add(sizeof(int) * (ipool.size() + 1)), o_dp = ar.add(sizeof(double) * (dpool.size() + 1)),
                 total = ar.top;
    std::vector<unsigned char> host(total, 0);
    std::memcpy(host.data() + o_sd, sd.data(), sizeof(SDesc) * ns);
    if (!g->int_vars.empty())
        std::memcpy(host.data() + o_iv, g->int_vars.data(), sizeof(int) * g->int_vars.size());
    if (!ipool.empty()) std::memcpy(host.data() + o_ip, ipool.data(), sizeof(int) * ipool.size());
    if (!dpool.empty()) std::memcpy(host.data() + o_dp, dpool.data(), sizeof(double) * dpool.size());
    if (g->sdev) {
        DZG_HIP(hipStreamSynchronize(g->st));
        DZG_HIP(hipFree(g->sdev));
        g->sdev = nullptr;
    }
    DZG_HIP(hipMalloc((void **)&g->sdev, total));
    DZG_HIP(hipMemcpyAsync(g->sdev, host.data(), total, hipMemcpyHostToDevice, g->st));
    DZG_HIP(hipStreamSynchronize(g->st));
    g->base.sd = (const SDesc *)(g->sdev + o_sd);
    g->base.int_vars = (const int *)(g->sdev + o_iv);
    g->base.ipool = (const int *)(g->sdev + o_ip);
    g->base.dpool = (const double *)(g->sdev + o_dp);
    g->base.nint = g->nint;
    g->base.nvars = g->nvars;
    g->dirty = false;
    return 0;
}

int mip_gpu_slot_alloc(MipGpu *g, int sid)
{
    const MipStructure &s = g->structs[(size_t)sid];
    if (s.n - s.m != g->pool_q || s.m > DZG_BATCH_MAX_ROWS) return -1;
    if (!g->pool_free.empty()) {
        const int slot = g->pool_free.back();
        g->pool_free.pop_back();
        return slot;
    }
    return g->pool_used++;
}

void mip_gpu_slot_free(MipGpu *g, int slot) { g->pool_free.push_back(slot); }

int mip_gpu_save_states(MipGpu *g, const int *pairs, int count)
{
    if (count <= 0) return 0;
    DZG_HIP(hipSetDevice(g->device));
    const long long si = DZG_BATCH_MAX_ROWS + g->pool_q, sz = g->pool_q > 0 ? g->pool_q : 1;
    for (int i = 0; i < count; ++i)
        if (pairs[2 * i] < 0 || pairs[2 * i] >= g->last_count || pairs[2 * i + 1] < 0 ||
            pairs[2 * i + 1] >= g->pool_used)
            return dzg_set_error(DZG_E_ARG, "mip: a parent-state slot or round index out of range");
    if (g->pool_used > g->pool_cap) { // grow: by half again, the live slots copied across
        const int cap = std::max(64, g->pool_used + g->pool_used / 2);
        int *ni = nullptr;
        double *nz = nullptr;
        DZG_HIP(hipMalloc((void **)&ni, sizeof(int) * si * cap));
        DZG_HIP(hipMalloc((void **)&nz, sizeof(double) * sz * cap));
        if (g->pool_cap > 0) {
            DZG_HIP(hipMemcpyAsync(ni, g->pool_i, sizeof(int) * si * g->pool_cap, hipMemcpyDeviceToDevice, g->st));
            DZG_HIP(hipMemcpyAsync(nz, g->pool_z, sizeof(double) * sz * g->pool_cap, hipMemcpyDeviceToDevice, g->st));
            DZG_HIP(hipStreamSynchronize(g->st));
            DZG_HIP(hipFree(g->pool_i));
            DZG_HIP(hipFree(g->pool_z));
        }
        g->pool_i = ni;
        g->pool_z = nz;
        g->pool_cap = cap;
    }
    if (count > g->pairs_cap) {
        if (g->pairs_dev) {
            DZG_HIP(hipStreamSynchronize(g->st));
            DZG_HIP(hipFree(g->pairs_dev));
            g->pairs_dev = nullptr;
        }
        const int cap = std::max(256, count + count / 2);
        DZG_HIP(hipMalloc((void **)&g->pairs_dev, sizeof(int) * 2 * cap));
        g->pairs_cap = cap;
    }
    DZG_HIP(hipMemcpyAsync(g->pairs_dev, pairs, sizeof(int) * 2 * count, hipMemcpyHostToDevice, g->st));
    MArgs a = g->last;
    a.pool_si = si;
    a.pool_sz = sz;
    hipLaunchKernelGGL(k_mip_save, dim3(count), dim3(64), 0, g->st, a, g->pairs_dev, g->pool_i, g->pool_z);
    DZG_HIP(hipGetLastError());
    DZG_HIP(hipStreamSynchronize(g->st)); // `pairs` is the caller's; the next round reads the slots
    return 0;
}

int mip_gpu_plant_slot(MipGpu *g, int sid, const int *basis, const int *nonbasis)
{
    const MipStructure &s = g->structs[(size_t)sid];
    const int slot = mip_gpu_slot_alloc(g, sid);
    if (slot < 0) return dzg_set_error(DZG_E_ARG, "mip: this structure cannot use the parent-state pool");
    DZG_HIP(hipSetDevice(g->device));
    const long long si = DZG_BATCH_MAX_ROWS + g->pool_q, sz = g->pool_q > 0 ? g->pool_q : 1;
    if (slot >= g->pool_cap) {
        if (g->pool_cap > 0) return dzg_set_error(DZG_E_ARG, "mip: planted slots come before saved ones");
        const int cap = 64;
        DZG_HIP(hipMalloc((void **)&g->pool_i, sizeof(int) * si * cap));
        DZG_HIP(hipMalloc((void **)&g->pool_z, sizeof(double) * sz * cap));
        DZG_HIP(hipMemsetAsync(g->pool_z, 0, sizeof(double) * sz * cap, g->st));
        g->pool_cap = cap;
    }
    DZG_HIP(hipMemcpyAsync(g->pool_i + slot * si, basis, sizeof(int) * s.m, hipMemcpyHostToDevice, g->st));
    DZG_HIP(hipMemcpyAsync(g->pool_i + slot * si + s.m, nonbasis, sizeof(int) * (s.n - s.m), hipMemcpyHostToDevice,
                           g->st));
    DZG_HIP(hipStreamSynchronize(g->st)); // the arrays are the caller's
    return slot;
}

int mip_gpu_read_state(MipGpu *g, int idx, int sid, int *basis, int *nonbasis, double *x, double *z)
{
    if (idx < 0 || idx >= g->last_count) return dzg_set_error(DZG_E_ARG, "mip: round index out of range");
    DZG_HIP(hipSetDevice(g->device));
    const MipStructure &s = g->structs[(size_t)sid];
    NDesc N;
    DZG_HIP(hipMemcpyAsync(&N, g->last.nd + idx, sizeof(NDesc), hipMemcpyDeviceToHost, g->st));
    DZG_HIP(hipStreamSynchronize(g->st));
    DZG_HIP(hipMemcpyAsync(basis, g->last.basis + N.m_off, sizeof(int) * s.m, hipMemcpyDeviceToHost, g->st));
    DZG_HIP(hipMemcpyAsync(nonbasis, g->last.nonbasis + N.q_off, sizeof(int) * (s.n - s.m), hipMemcpyDeviceToHost,
                           g->st));
    DZG_HIP(hipMemcpyAsync(x, g->last.x + N.m_off, sizeof(double) * s.m, hipMemcpyDeviceToHost, g->st));
    DZG_HIP(hipMemcpyAsync(z, g->last.z + N.q_off, sizeof(double) * (s.n - s.m), hipMemcpyDeviceToHost, g->st));
    DZG_HIP(hipStreamSynchronize(g->st));
    return 0;
}

int mip_gpu_solve_round(MipGpu *g, const int *sid, const int *pslot, const double *bnd, int count,
                        long long max_iter, double eps, int ppl, double int_tol, MipNodeRecord *rec,
                        double *values, const MipFastRun *fast)
{
    if (count <= 0) return 0;
    DZG_HIP(hipSetDevice(g->device));
    if (g->dirty) {
        const int rc = upload_structures(g);
        if (rc < 0) return rc;
    }
    // ---- layout of the round arena
    std::vector<NDesc> nd((size_t)count);
    long long nm = 0, nq = 0;
    int mmax[kBuckets] = {0, 0, 0, 0};
    int bucket_n[kBuckets] = {0, 0, 0, 0};
    for (int i = 0; i < count; ++i) {
        const MipStructure &s = g->structs[(size_t)sid[i]];
        nd[(size_t)i].sid = sid[i];
        nd[(size_t)i].pslot = pslot ? pslot[i] : -1;
        if (nd[(size_t)i].pslot >= g->pool_cap || (nd[(size_t)i].pslot >= 0 && s.n - s.m != g->pool_q))
            return dzg_set_error(DZG_E_ARG, "mip: a node names a parent-state slot that was never saved");
        nd[(size_t)i].m_off = nm;
        nd[(size_t)i].q_off = nq;
        nm += s.m;
        nq += s.n - s.m;
        const int b = bucket_of(s.m);
        mmax[b] = std::max(mmax[b], s.m);
        bucket_n[b]++;
    }
    const size_t nb2 = (size_t)count * 2 * (size_t)g->nint;
    bh::Arena ar;
    // uploaded: descriptors, bounds, the first list; then device-only state and results
    const size_t o_nd = ar.add(sizeof(NDesc) * count), o_bnd = ar.add(sizeof(double) * (nb2 + 1)),
                 o_list = ar.add(sizeof(int) * count),
                 o_tmpl = ar.add(fast ? sizeof(dzg_bf::FState) : 0); // FAST: the block every node starts from
    const size_t upload_end = ar.top;
    const size_t o_iter = ar.add(sizeof(long long) * count), o_rec = ar.add(sizeof(MipNodeRecord) * count),
                 o_status = ar.add(sizeof(int) * count), o_list2 = ar.add(sizeof(int) * count),
                 // the running counters, then (FAST) the strict list's, read back together
                 o_counts = ar.add(sizeof(int) * 2 * kBuckets), o_basis = ar.add(sizeof(int) * (nm + 1)),
                 o_nonbasis = ar.add(sizeof(int) * (nq + 1)), o_x = ar.add(sizeof(double) * (nm + 1)),
                 o_xbar = ar.add(sizeof(double) * (nm + 1)), o_z = ar.add(sizeof(double) * (nq + 1)),
                 o_zbar = ar.add(sizeof(double) * (nq + 1)), o_dz = ar.add(sizeof(double) * (nq + 1)),
                 o_vals = ar.add(sizeof(double) * ((size_t)count * g->nvars + 1)),
                 o_fstate = ar.add(fast ? sizeof(dzg_bf::FState) * count : 0),
                 o_slist = ar.add(fast ? sizeof(int) * count : 0); // FAST: the rejected nodes, by bucket
    if (const size_t top = ar.top; top > g->rcap) { // one allocation, grown by half again so that few rounds reallocate
        if (g->rdev) {
            DZG_HIP(hipStreamSynchronize(g->st));
            DZG_HIP(hipFree(g->rdev));
            g->rdev = nullptr;
            g->rcap = 0;
        }
        const size_t cap = top + top / 2;
        DZG_HIP(hipMalloc((void **)&g->rdev, cap));
        g->rcap = cap;
    }
    std::vector<unsigned char> host(upload_end, 0);
    std::memcpy(host.data() + o_nd, nd.data(), sizeof(NDesc) * count);
    if (nb2) std::memcpy(host.data() + o_bnd, bnd, sizeof(double) * nb2);
    if (fast) dzg_steps::fast_state_init(host.data() + o_tmpl, *fast->opts, max_iter);
    const bh::Segments seg = bh::segments(bucket_n);
    {
        int *list = (int *)(host.data() + o_list);
        bh::Segments fill = seg;
        for (int i = 0; i < count; ++i) list[fill[(size_t)bucket_of(g->structs[(size_t)sid[i]].m)]++] = i;
    }
    unsigned char *dev = g->rdev;
    hipStream_t st = g->st;
    DZG_HIP(hipMemcpyAsync(dev, host.data(), upload_end, hipMemcpyHostToDevice, st));
    DZG_HIP(hipMemsetAsync(dev + o_iter, 0xff, sizeof(long long) * count, st)); // -1: not initialised
    DZG_HIP(hipMemsetAsync(dev + o_rec, 0, sizeof(MipNodeRecord) * count, st)); // warm = 0: no restart yet

    MArgs a = g->base;
    a.nd = (const NDesc *)(dev + o_nd);
    a.bnd = (const double *)(dev + o_bnd);
    a.basis = (int *)(dev + o_basis);
    a.nonbasis = (int *)(dev + o_nonbasis);
    a.x = (double *)(dev + o_x);
    a.xbar = (double *)(dev + o_xbar);
    a.z = (double *)(dev + o_z);
    a.zbar = (double *)(dev + o_zbar);
    a.dz = (double *)(dev + o_dz);
    a.iter = (long long *)(dev + o_iter);
    a.status = (int *)(dev + o_status);
    a.rec = (MipNodeRecord *)(dev + o_rec);
    a.values = (double *)(dev + o_vals);
    a.max_iter = max_iter;
    a.eps = eps;
    a.int_tol = int_tol;
    a.ppl = ppl;
    a.pool_i = g->pool_i;
    a.pool_z = g->pool_z;
    a.pool_si = DZG_BATCH_MAX_ROWS + g->pool_q;
    a.pool_sz = g->pool_q > 0 ? g->pool_q : 1;
    g->last = a;
    g->last_count = count;

    const auto strict_launch = [&](int b, const int *list, int n, int *next_list, int *next_count) {
        MArgs ab = a;
        ab.mmax = mmax[b];
        launch_bucket(b, ab, list, n, next_list, next_count, st);
    };
    int *const list1 = (int *)(dev + o_list), *const list2 = (int *)(dev + o_list2);
    int *const counts = (int *)(dev + o_counts);
    if (!fast) {
        const int rc = bh::run_rounds(list1, list2, counts, seg, bh::live_of(bucket_n), st, strict_launch);
        if (rc) return rc;
    } else {
        // FAST slices until the lists drain; the rejected nodes collect in slist, whose counters come
        // down with every round's.  Then k_mip_node on that list, cold (both round lists are free).
        FNode f;
        f.state = (dzg_bf::FState *)(dev + o_fstate);
        f.tmpl = (const dzg_bf::FState *)(dev + o_tmpl);
        f.nd = (NDesc *)(dev + o_nd);
        f.ppl = dzg_steps::fast_ppl(fast->pivots_per_launch);
        f.refactor_every = dzg_steps::fast_refactor_every(fast->refactor_every);
        int *const slist = (int *)(dev + o_slist);
        DZG_HIP(hipMemsetAsync(counts + kBuckets, 0, sizeof(int) * kBuckets, st));
        std::array<int, kBuckets> rejected{};
        const int rc = bh::run_rounds(list1, list2, counts, seg, bh::live_of(bucket_n), st,
                                      [&](int b, const int *list, int n, int *next_list, int *next_count) {
                                          MArgs ab = a;
                                          ab.mmax = mmax[b];
                                          launch_bucket_fast(b, ab, f, list, n, next_list, next_count,
                                                             slist + seg[(size_t)b], counts + kBuckets + b, st);
                                      }, nullptr, rejected.data());
        if (rc) return rc;
        const int rc2 = bh::run_rounds(slist, list1, counts, seg, rejected, st, strict_launch);
        if (rc2) return rc2;
    }
    DZG_HIP(hipMemcpyAsync(rec, dev + o_rec, sizeof(MipNodeRecord) * count, hipMemcpyDeviceToHost, st));
    DZG_HIP(hipStreamSynchronize(st));
    if (g->nvars > 0)
        for (int i = 0; i < count; ++i)
            if (rec[i].status == DZG_OPTIMAL && rec[i].integral)
                DZG_HIP(hipMemcpyAsync(values + (size_t)i * g->nvars,
                                    dev + o_vals + sizeof(double) * (size_t)i * g->nvars,
                                    sizeof(double) * g->nvars, hipMemcpyDeviceToHost, st));
    DZG_HIP(hipStreamSynchronize(st));
    return 0;
}

} // namespace dzg_internal
