// k_chain.hip -- the FAST iteration of the dense inverse in THREE launches on one GPU:
//
//      k_chain_pre   status(); a primal step: beta, FTRAN, ratio test;   then BTRAN's row
//      pricing       (k_price.hip: the only code that touches the matrix; while k is small it is the TAIL
//                    of k_chain_pre -- PRICE below -- and the iteration is two launches)
//      k_chain_post  a dual step: ratio test, beta, FTRAN;   the pivot's books;   the update
//
// The seven-launch form of the same iteration (k_fast.hip) pays a kernel boundary for every
// dependent phase.  Here the phases of one side of the pricing pass share a launch of one
// workgroup per CU, and two things keep the number of device-wide synchronisations below the number
// of phases:
//
//   * Every decision is taken by EVERY workgroup from the same partial results (a few KB), so a
//     decision needs no broadcast; the lead lane of workgroup 0 only records it in the control
//     block for the launches that follow.
//   * A workgroup owns the same rows in FTRAN, BTRAN and the update and the same columns of z, and
//     nothing it reads inside a launch is rewritten by another workgroup of that launch: the six
//     values the step lengths need are read before any writer can have got there (a dual step) or
//     were left in the control block by k_chain_pre (a primal step); dx_p is computed by every
//     workgroup itself, with the owner's arithmetic; Binv0's rows are read BEFORE the barrier beta
//     is waited for (the eta file's share is added after it), so the column a deleting pivot moves
//     is no longer read by anybody.  The update therefore starts without waiting for anybody, and
//     the pivot's books are kept by ONE WAVE of workgroup 0 beside it.
//
//   What remains: the eta file's beta = W^T a_j must be complete before the eta share of FTRAN's
//   rows (1 barrier), a primal step's ratio test needs every row of dx (1 more).
//   Barriers per iteration: 2 (primal step: both in k_chain_pre), 1 (dual step: in k_chain_post).
//
// The barrier itself is fence-free (profiles/r02_gridsync_vs_kernel_boundary.txt): an agent-scope
// release would write back the XCD's whole L2.  What crosses a barrier -- beta's 4 x 64 wave sums,
// one candidate record per workgroup -- is published with agent-scope (sc1, write-through) stores by
// lane 0 (of the wave that computed it) and read with sc1 loads; everything else a phase reads was
// written by an earlier launch or by the reading workgroup itself.  Arrivals are counted on eight counters (one per residue of the
// workgroup index mod 8, so that 256 atomics do not queue on one address), the last arrival of a
// residue class bumps the top counter everybody polls.  The counters only grow; the number of
// barriers passed so far lives in the control block (bar_gen).  A poll loop gives up after ~2.4 s (2^24 polls), marks
// the control block (status DZG_PANIC, bar_timeout) and the host returns DZG_E_DEVICE: every wave
// reaches its exit whatever happens (a barrier can only fail when the launch's workgroups are not
// all resident, i.e. when something else occupies CUs or LDS of this device).
//
// Arithmetic: the row, dot-product, book-keeping and update formulas are the functions the
// seven-launch kernels call (fast_rows.h), and argmax reductions do not depend on how candidates are
// grouped, so a solve is bit-identical whichever form runs an iteration; the host may switch between
// them at any poll (it does when the compact width outgrows the LDS copy of the gathered column).
#include <chrono>
#include "common.h"
#include "fast_decide.h"
#include "fast_rows.h"
#include "price_small.h"

#include "chain_barrier.h"

// (the stage clocks of DZG_CHAIN_DEBUG=1: ChainStamps, common.h)

// ---------------------------------------------------------------------------------
// Work split.  Workgroup b owns rows [r0, r1) -- thread t the row r0 + t -- in FTRAN, BTRAN and the
// update, and columns [q0, q1) of z -- thread t the column q0 + t.  (The host runs the chain only
// when a workgroup's share is at most one row and one column per thread.)  A thread loads what it
// needs of its row / column as the first thing the kernel does, together with the control block:
// after a kernel boundary every first touch of a line costs a trip to memory (1-2 us), and these
// trips are taken side by side instead of one behind the other.
// ---------------------------------------------------------------------------------
#define CH_NW (CH_THREADS / 64)
#define CH_MAXP 16 // FTRAN passes (rows per lane group) whose partial sums wait in registers: the generic kernels'

// ---------------------------------------------------------------------------------
// Instantiations.  The two chain kernels are compiled once in full -- CH_MAXP passes, both lane
// widths of FTRAN's rows, the FOLD head and both candidate paths chosen at run time: the GENERIC
// kernels, which run any launch -- and a few times with only what a launch can need, chosen by the
// host per batch (dzg_chain_pick below) from what it knows before the batch starts:
//   MAXP    register-held passes of chain_dot_head / chain_dot_tail.  Any value computes any share:
//           passes beyond MAXP take chain_dot_tail's trailing loop (whole rows, the same sums).
//   NARROW  the batch's bound on the compact width is known and <= 512: 16 lanes per row only.
//   NOFOLD  (k_chain_post) fold == 0 and nrz <= 256: neither the FOLD head nor the many-candidates
//           path exists.
// No formula, order of a sum, barrier or LDS buffer depends on the instantiation.
// ---------------------------------------------------------------------------------
template <bool NARROW>
__device__ __forceinline__ bool chain_wide(int k)
{
    if constexpr (NARROW)
        return false;
    else
        return k > 512;
}
template <bool NOFOLD>
__device__ __forceinline__ int chain_fold_on(int fold)
{
    if constexpr (NOFOLD)
        return 0;
    else
        return fold;
}
template <bool NOFOLD>
__device__ __forceinline__ bool chain_one_wave(int nrz)
{
    if constexpr (NOFOLD)
        return true;
    else
        return nrz <= 256;
}

__device__ __forceinline__ void chain_rows(int m, int &r0, int &r1)
{
    const int per = ((m + (int)gridDim.x - 1) / (int)gridDim.x + 3) & ~3;
    r0 = (int)blockIdx.x * per;
    if (r0 > m) r0 = m;
    r1 = r0 + per < m ? r0 + per : m;
}

__device__ __forceinline__ void chain_cols(int q, int &q0, int &q1)
{
    const int per = (q + (int)gridDim.x - 1) / (int)gridDim.x;
    q0 = (int)blockIdx.x * per;
    if (q0 > q) q0 = q;
    q1 = q0 + per < q ? q0 + per : q;
}

// The argmax reductions ONE wave runs while its workgroup waits: the straight-line form of common.h
// (dzg_wave_best2_flat; bit for bit the fold of dzg_better2, see there; profiles/cand_reduce.txt).
// All 64 lanes of the calling wave are active at every call below.
__device__ __forceinline__ DzgCand2 chain_wave_best2(DzgCand2 c)
{
    return dzg_wave_best2_flat<64>(c);
}
__device__ __forceinline__ DzgCand2 chain_block_best2(DzgCand2 c)
{
    static_assert(CH_THREADS == 512, "eight wave results: one half row");
    return dzg_block_best2_flat<8>(c, true);
}

// up to 4 x 64 partial candidates in the registers of one wave, loaded before their count is known
struct ChainSpec {
    double r[4], h[4];
    int k[4];
};
__device__ __forceinline__ void chain_spec_load(ChainSpec &s, const double *__restrict__ pr,
                                                const int *__restrict__ pk,
                                                const double *__restrict__ ph, int lane)
{
#pragma unroll
    for (int j = 0; j < 4; ++j) { // (the arrays hold 4096 entries: reading past `count` is harmless)
        s.r[j] = pr[lane + 64 * j];
        s.k[j] = pk[lane + 64 * j];
        s.h[j] = ph[lane + 64 * j];
    }
}
__device__ __forceinline__ DzgCand2 chain_spec_reduce(const ChainSpec &s, int count, int lane);
// (DZG_CHAIN_DEBUG=1: a reduction site's clock starts once its operands have arrived)
__device__ __forceinline__ void chain_spec_pin(const ChainStamps &ts, ChainSpec &s)
{
    if (ts.on)
        asm volatile("" : "+v"(s.r[0]), "+v"(s.r[1]), "+v"(s.r[2]), "+v"(s.r[3]), "+v"(s.k[0]), "+v"(s.k[1]),
                          "+v"(s.k[2]), "+v"(s.k[3]), "+v"(s.h[0]), "+v"(s.h[1]), "+v"(s.h[2]), "+v"(s.h[3]));
}
// the same for candidates that crossed a barrier of this launch (agent-scope loads): the four
// slots of a lane leave together -- one trip, where a loop over i = lane, lane + 64, ... waits for
// each turn's loads before it issues the next
__device__ __forceinline__ void chain_spec_load_sc1(ChainSpec &s, const double *pr, const int *pk,
                                                    const double *ph, int lane)
{
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        s.r[j] = ld_sc1(pr + lane + 64 * j);
        s.k[j] = ld_sc1(pk + lane + 64 * j);
        s.h[j] = ld_sc1(ph + lane + 64 * j);
    }
}
// the workgroups' candidates of a barrier-crossing ratio test, reduced by wave 0 (candidates
// i = lane, lane + 64, ... in ascending order, then the wave: the same order either way)
__device__ __forceinline__ DzgCand2 chain_reduce_sc1(const double *pr, const int *pk, const double *ph,
                                                     int n, int lane)
{
    if (n <= 256) {
        ChainSpec sx;
        chain_spec_load_sc1(sx, pr, pk, ph, lane);
        return chain_spec_reduce(sx, n, lane);
    }
    DzgCand2 w = dzg_cand2_none();
    for (int i = lane; i < n; i += 64) {
        DzgCand2 o;
        o.r = ld_sc1(pr + i);
        o.k = ld_sc1(pk + i);
        o.h = ld_sc1(ph + i);
        w = dzg_better2(w, o);
    }
    return chain_wave_best2(w);
}
__device__ __forceinline__ DzgCand2 chain_spec_reduce(const ChainSpec &s, int count, int lane)
{
    DzgCand2 best = dzg_cand2_none();
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        DzgCand2 o;
        o.r = s.r[j];
        o.k = s.k[j];
        o.h = s.h[j];
        if (lane + 64 * j < count) best = dzg_better2(best, o);
    }
    return chain_wave_best2(best);
}

// two argmax candidates through LDS: written by lane 0 of waves 0 and 1, read by everybody
struct ChainSlots {
    double r[2], h[2];
    int k[2];
};
__device__ __forceinline__ void chain_put(ChainSlots &s, int slot, const DzgCand2 &c)
{
    s.r[slot] = c.r;
    s.k[slot] = c.k;
    s.h[slot] = c.h;
}
__device__ __forceinline__ DzgCand2 chain_get(const ChainSlots &s, int slot)
{
    DzgCand2 c;
    c.r = s.r[slot];
    c.k = s.k[slot];
    c.h = s.h[slot];
    return c;
}

// best of the candidates threads 0 .. n-1 hold; valid in wave 0 (n <= 64: no workgroup barrier)
__device__ __forceinline__ DzgCand2 chain_best(DzgCand2 c, int n)
{
    if (n <= 64) return (threadIdx.x < 64) ? chain_wave_best2(c) : c;
    return chain_block_best2(c);
}
// two independent ones side by side: in wave 0 the two straight-line reductions are one instruction
// stream, and each one's waits (DPP, readlane, ballot) are filled with the other's work
__device__ __forceinline__ void chain_best_pair(DzgCand2 &a, int na, DzgCand2 &b, int nb)
{
    if (na <= 64 && nb <= 64) {
        if (threadIdx.x < 64) {
            const DzgCand2 wa = chain_wave_best2(a), wb = chain_wave_best2(b);
            a = wa;
            b = wb;
        }
        return;
    }
    a = chain_best(a, na);
    b = chain_best(b, nb);
}

// The entering column gathered to compact coordinates, in LDS (zero-padded to an even length).
// dr0, dr1 = drow[tid], drow[tid + CH_THREADS], loaded early.
__device__ __forceinline__ void chain_stage_ag(double *s_ag, int k, int code,
                                               const double *__restrict__ a,
                                               const int *__restrict__ drow, int dr0, int dr1)
{
    const int k2 = (k + 1) & ~1, tid = threadIdx.x;
    const int rr = -1 - code; // (entering slack: the unit vector of its row)
    if (tid < k2) s_ag[tid] = tid < k ? (code < 0 ? (dr0 == rr ? 1.0 : 0.0) : a[dr0]) : 0.0;
    if (tid + CH_THREADS < k2)
        s_ag[tid + CH_THREADS] = tid + CH_THREADS < k ? (code < 0 ? (dr1 == rr ? 1.0 : 0.0) : a[dr1]) : 0.0;
    for (int c = tid + 2 * CH_THREADS; c < k2; c += CH_THREADS)
        s_ag[c] = c < k ? (code < 0 ? (drow[c] == rr ? 1.0 : 0.0) : a[drow[c]]) : 0.0;
}

// The entering column: the device's own matrix (one GPU, or a sharded rank that keeps every column),
// or -- a PARTITIONED rank, whose HBM holds its own block only -- the copy that travels in the
// winner's exchange record (8 header doubles, then the column; include/dantzig_amd.h).
template <bool SHARD>
__device__ __forceinline__ const double *chain_col(const DzgDev &d, int code,
                                                   const double *__restrict__ xrecv, int w_rec)
{
    if (code < 0) return nullptr;
    if (SHARD && d.xstride > 8) return xrecv + (long long)w_rec * d.xstride + 8;
    return d.A + (long long)(code - d.col0) * d.lda;
}

// beta_t = W_t . a_j, published for everybody as the FOUR WAVE SUMS fast_beta_dot adds up
// (fast_rows.h): a wave sum depends on a quarter of W_t and a_j only, so the work items are the pairs
// (t, w), item = 4 t + w, one wave each -- at the usual grid of one workgroup per CU at most one item
// per workgroup, 16 + 16 KB of m = 8192 through a CU instead of 64 + 64 KB through the CUs of the
// first neta workgroups while the others wait for them at the barrier.  The wave that runs an item is
// one that has no share of the gather (threads < k2) and does not carry row p or the books (the
// last wave): wave CH_BETA_WAVE, then the waves after it.  Lane 0 publishes the sum in
// beta_part[item]; chain_beta_fetch adds the four up after the barrier, in block_sum's order.
// An entering slack (code < 0): beta_t = W_t[row] is one load and takes no part in any sum
// (0.0 + -0.0 would lose the sign): item (t, 0) publishes it, slot 4 t is taken verbatim.
// d.beta_split == 0 (DZG_CHAIN_BETA_SPLIT=0, the A/B switch): workgroup t runs the four items of
// eta t on its first four waves, as fast_beta_dot spreads them; same slots, same bits.
#define CH_BETA_WAVE 3
__device__ __forceinline__ void chain_beta_item(const DzgDev &d, int item, int code,
                                                const double *__restrict__ a)
{
    const int t = item >> 2, w = item & 3;
    const double *wt = d.W + (long long)t * d.ldw;
    double s;
    if (code < 0) {
        if (w != 0) return;
        s = wt[-1 - code];
    } else {
        s = fast_beta_wave(wt, a, d.m, w);
    }
    if ((threadIdx.x & 63) == 0) st_sc1(d.beta_part + item, s);
}
__device__ __forceinline__ void chain_beta(const DzgDev &d, int neta, int code,
                                           const double *__restrict__ a)
{
    const int wave = threadIdx.x >> 6;
    if (!d.beta_split) {
        for (int b = blockIdx.x; b < neta; b += gridDim.x)
            if (wave < 4) chain_beta_item(d, 4 * b + wave, code, a);
        return;
    }
    // (block-uniform loop: a grid of fewer workgroups than items -- a CU-masked or partitioned
    // device -- takes several per workgroup, on different waves while there are any; an item's bits
    // depend on the item only)
    int turn = CH_BETA_WAVE;
    for (int item = blockIdx.x; item < 4 * neta; item += gridDim.x) {
        if (wave == turn) chain_beta_item(d, item, code, a);
        turn = turn + 1 < CH_NW ? turn + 1 : 0;
    }
}
// What crosses a barrier is published by the lane that arrives at it (chain_barrier.h); the lanes
// that published wave sums are others, so every wave sees its own stores out of the CU before the
// workgroup barrier that chain_barrier begins with.  (By then the stores are long acknowledged.)
__device__ __forceinline__ void chain_beta_published()
{
    __builtin_amdgcn_s_waitcnt(0);
}
// After the barrier: beta into LDS.  Threads < 4 R_ load one slot each -- one trip, as the 64 loads
// were -- lane 4 j of a wave gathers the four slots of its eta by shuffle and adds them up.  The
// caller's __syncthreads makes s_beta visible.
__device__ __forceinline__ void chain_beta_fetch(const DzgDev &d, int neta, int code, double *s_beta)
{
    const int tid = threadIdx.x;
    if (tid < 4 * R_) { // (whole waves: 4 R_ is a multiple of 64)
        const double s0 = tid < 4 * neta ? ld_sc1(d.beta_part + tid) : 0.0;
        const double s1 = __shfl_down(s0, 1, DZG_WAVE);
        const double s2 = __shfl_down(s0, 2, DZG_WAVE);
        const double s3 = __shfl_down(s0, 3, DZG_WAVE);
        const int t = tid >> 2;
        if ((tid & 3) == 0) s_beta[t] = t < neta ? (code < 0 ? s0 : fast_beta_fold(s0, s1, s2, s3)) : 0.0;
    }
}

// FTRAN on this workgroup's rows, first half (needs the gathered column only): lane group `grp` of
// wave `wave` takes row r0 + (pass * CH_NW + wave) * RPW + grp; the partial sums of the first
// MAXP passes stay in registers across the barrier beta is waited for.  (A pass beyond the
// workgroup's share is masked off lane by lane in fast_gemv_row_head; a block-uniform branch over it,
// as chain_dot_tail has, was measured and withdrawn: profiles/chain_instances.txt.)
template <int LPR, int MAXP>
__device__ __forceinline__ void chain_dot_head(const DzgDev &d, int r0, int r1, int k,
                                               const double *s_ag, double (&accs)[MAXP])
{
    constexpr int RPW = 64 / LPR;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int sub = lane % LPR, grp = lane / LPR;
    const int k2 = (k + 1) & ~1;
    // (block-uniform) how the rows are loaded: an inverse that outgrows the 256-MB Infinity Cache
    // streams past the caches (nontemporal loads, eight steps in flight: 125.4 -> 102.9 us per FTRAN
    // at k = 7 700 of config 3), a smaller one is re-read from it pivot after pivot and plain loads
    // are faster (55.4 against 60.4 us at k = 4 049): profiles/r04_ftran_row_loads_ab.txt
    if (LPR == 64 && k >= d.ftran_nt_k) {
#pragma unroll
        for (int pass = 0; pass < MAXP; ++pass) {
            const int i = r0 + (pass * CH_NW + wave) * RPW + grp;
            accs[pass] = fast_gemv_row_head<LPR, true>(i < r1 ? i : d.m, d.m, k2, d.binv, d.ldb, s_ag, sub);
        }
        return;
    }
#pragma unroll
    for (int pass = 0; pass < MAXP; ++pass) {
        const int i = r0 + (pass * CH_NW + wave) * RPW + grp;
        accs[pass] = fast_gemv_row_head<LPR>(i < r1 ? i : d.m, d.m, k2, d.binv, d.ldb, s_ag, sub);
    }
}

// second half: the eta file's share and the sum over the lanes; row sums land in s_dx[row - r0]
template <int LPR, int MAXP>
__device__ __forceinline__ void chain_dot_tail(const DzgDev &d, int r0, int r1, int k, int neta,
                                               const double *s_ag, const double *s_beta,
                                               const double (&accs)[MAXP], double *s_dx)
{
    constexpr int RPW = 64 / LPR;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int sub = lane % LPR, grp = lane / LPR;
    const int k2 = (k + 1) & ~1;
    const int npass = (r1 - r0 + CH_NW * RPW - 1) / (CH_NW * RPW);
#pragma unroll
    for (int pass = 0; pass < MAXP; ++pass) {
        if (pass < npass) { // (block-uniform)
            const int i = r0 + (pass * CH_NW + wave) * RPW + grp;
            const int ii = i < r1 ? i : d.m;
            const double acc = fast_gemv_row_tail<LPR>(accs[pass], ii, d.m, neta, d.U, d.ldw, s_beta, sub);
            if (ii < d.m && sub == 0) s_dx[i - r0] = acc;
        }
    }
    for (int pass = MAXP; pass < npass; ++pass) { // shares taller than MAXP passes: the whole row now
        const int i = r0 + (pass * CH_NW + wave) * RPW + grp;
        const int ii = i < r1 ? i : d.m;
        const double acc = fast_gemv_row<LPR>(ii, d.m, k2, neta, d.binv, d.ldb, s_ag, d.U, d.ldw, s_beta, sub);
        if (ii < d.m && sub == 0) s_dx[i - r0] = acc;
    }
}

// ---------------------------------------------------------------------------------
// k_chain_pre: src/simplex.rs:274-306 (status), :226-229 + :439-461 (a primal step's FTRAN and
// ratio test), then v = row p of the inverse (:231-236's solve).  grid = one workgroup per CU.
// ---------------------------------------------------------------------------------
// SHARD (column sharding with the matrix replicated, one process per GPU): the z-side first pivot
// comes from the merge of every rank's proposal (xrecv: the first exchange's records) -- all ranks
// see the same records in the same order and apply the same rule, so they take the same decision.
//
// PRICE (one GPU, NARROW, one pass; 0: none, NG: the small-k row pass <2, NG, 16> of price_small.h in
// this kernel's tail).  BTRAN's row is computed piecewise, each workgroup on its own rows, and the
// pricing pass of every column tile needs all k + 1 compact entries of it: that is the only reason for
// the kernel boundary in between.  But a compact entry depends on nothing this launch writes --
// vc[c] = Binv0[p][c] - sum_t U[t][p] W[t][drow[c]], all left by earlier launches -- so every
// workgroup forms all of vc[0..k) itself once p is known: compact column c on thread CHP_COL0 + c
// (the rows sit on threads < CHP_COL0; k < 480 fills the workgroup exactly; no thread holds two eta
// columns' registers), in the SAME trip as BTRAN's own loads, the eta rows from d.wk (common.h: W in
// compact coordinates, contiguous, kept current by both chain kernels), with the owner's expression
// and operands and therefore its bits.  Workgroup b then prices tile b as k_price_rows_small does:
// row list and coefficients into LDS (the gathered column's buffer, free after FTRAN), one workgroup
// barrier, the rows stage, the finish.  A unit column's v is its row's compact entry (a nonbasic
// slack's row is a compact row by definition): s_coef[dslot[row]], no gather over v.  No barrier and
// no launch is added; the owners still store v, vc and wk[neta] for k_chain_post and the other kernels.
#define CHP_COL0 32
// `d` of the running chain kernel, read again from the kernel-argument segment at the point of the
// call, behind a barrier the compiler cannot hoist the loads across.  A stage that takes a dozen of
// d's pointers from the by-value argument keeps them in scalar registers from the kernel's start; the
// chain kernels sit at the scalar-register limit, and those pointers cost the stages before it 44-76
// registers spilled through vector lanes and a microsecond (profiles/price_in_pre.txt).
// ONLY VALID IN A KERNEL WHOSE FIRST ARGUMENT IS `const DzgDev d`, BY VALUE (offset 0 of the segment):
// k_chain_pre below says so at its signature, and its PRICE tail checks one field of the copy against
// the argument itself (ctl) and ends the solve with DZG_PANIC if they differ.
typedef const __attribute__((address_space(4))) DzgDev ChainDevArg;
__device__ __forceinline__ ChainDevArg *chain_dev_reloaded()
{
    ChainDevArg *kd = (ChainDevArg *)__builtin_amdgcn_kernarg_segment_ptr();
    asm volatile("" : "+s"(kd));
    return kd;
}
template <bool SHARD, int MAXP, bool NARROW, int PRICE = 0>
// (`d` MUST STAY THE FIRST ARGUMENT, BY VALUE: the PRICE tail reads it again through chain_dev_reloaded)
__global__ __launch_bounds__(CH_THREADS) void k_chain_pre(const DzgDev d, unsigned long long *bar,
                                                          unsigned long long *dbg,
                                                          const double *__restrict__ xrecv)
{
    static_assert(PRICE == 0 || (!SHARD && NARROW && MAXP == 1 && PRICE <= 2), "the pricing tail: P1, narrow");
    static_assert(CH_THREADS == 512 && CH_AGCAP >= 2 * PRS_ROWS + PR_GMAX * PRS_TILE, "the tail's LDS");
    // the kept compact copy of the eta rows (d.wk) exists only in the one-pass narrow kernels: the host
    // sets d.wk only for batches that run them (dzg_chain_keeps_wk); every other instantiation is the
    // code it was without the copy
    constexpr bool WK = !SHARD && NARROW && MAXP == 1;
    __shared__ __attribute__((aligned(16))) double s_ag[CH_AGCAP];
    __shared__ double s_beta[R_], s_dx[CH_THREADS], s_up[R_];
    __shared__ ChainSlots s_c;
    ChainStamps ts;
    ts.start(dbg);
    DzgCtl *ctl = d.ctl;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int m = d.m, nwg = (int)gridDim.x;
    const bool lead = blockIdx.x == 0 && tid == 0;
    // ---- first touches, side by side: candidates of the last update, this thread's row
    ChainSpec sp;
    if (wave == 0 && !SHARD)
        chain_spec_load(sp, d.fpz_r, d.fpz_k, d.fpz_h, lane);
    else if (wave == 1)
        chain_spec_load(sp, d.fpx_r, d.fpx_k, d.fpx_h, lane);
    DzgCand2 cj_rec = dzg_cand2_none();
    int w_rec = -1;
    if (SHARD) w_rec = shard_merge(xrecv, d.xstride, d.world, cj_rec);
    int r0, r1;
    chain_rows(m, r0, r1);
    const int row = r0 + tid;
    const bool has_row = row < r1;
    int dslot_i = -1, bcode_i = 0;
    double x_i = 0.0, xbar_i = 0.0;
    if (has_row) {
        dslot_i = d.dslot[row];
        bcode_i = d.bcode[row];
        x_i = d.x[row];
        xbar_i = d.xbar[row];
    }
    // (PRICE) the tail's first touches: this thread's unit-column position with its z, zbar, this
    // lane's column of the tile and where it sits, the row of this thread's compact column (fetched
    // before k is known: entries from k on are stale and never used; the list has m entries)
    const int tiles = PRICE ? (int)((d.ldt + PRS_TILE - 1) / PRS_TILE) : 0;
    const int spos = (int)blockIdx.x * CH_THREADS + tid, cc = tid - CHP_COL0;
    int scode = 0, pos = -1, lrow_c = 0;
    double sz = 0.0, szb = 0.0;
    const bool tile_on = PRICE != 0 && (int)blockIdx.x < tiles; // (block-uniform: this workgroup prices a tile)
    if (tile_on) {
        if (spos < d.q) {
            scode = d.nbcode[spos];
            sz = d.z[spos];
            szb = d.zbar[spos];
        }
        const long long j = (long long)blockIdx.x * PRS_TILE + lane;
        if (wave == 0 && j < d.col1 - d.col0) pos = d.cpos[j];
        if (cc >= 0) lrow_c = d.drow[cc < m ? cc : m - 1];
    }
    DzgCtl c = *ctl; // one snapshot; nothing the lead lane writes below is read from it
    if (c.status != DZG_RUNNING) return;
    unsigned long long gen = c.bar_gen;
    const int neta = c.neta, k = c.ncompact;
    const int dr0 = tid < k ? d.drow[tid] : -1;
    const int dr1 = tid + CH_THREADS < k ? d.drow[tid + CH_THREADS] : -1;
    if (wave < 2 && !(SHARD && wave == 0)) {
        chain_spec_pin(ts, sp);
        const unsigned long long t_site = ts.now();
        DzgCand2 w = chain_spec_reduce(sp, c.fp_count, lane);
        ts.pin(w);
        ts.site(DZG_SITE_PRE_FIRST, t_site);
        if (lane == 0) chain_put(s_c, wave, w);
    }
    __syncthreads();
    const DzgCand2 cj = SHARD ? cj_rec : chain_get(s_c, 0), ci = chain_get(s_c, 1);
    int kind;
    double mu;
    const unsigned long long t_status = ts.now();
    if (!fast_status(ctl, c, lead, cj, ci, d.eps, m, SHARD, kind, &mu)) return;
    ts.pin(mu);
    ts.site(DZG_SITE_PRE_STATUS, t_status);
    const int slot = kind == DZG_STEP_PRIMAL ? 0 : 1;
    ts.mark(slot); // 0: first touches + status
    // the host runs the seven launches -- and picks no NARROW kernel -- before this can happen
    if (k > CH_AGCAP || c.fp_count > 256 || (NARROW && k > 512)) {
        if (lead) ctl->status = DZG_PANIC;
        return;
    }
    // (PRICE: k_price_rows_small's guard, and what the tail's layout takes for granted: a thread per
    // compact entry, a row per thread < CHP_COL0, every nonbasic position under a pricing workgroup)
    if (PRICE != 0 && (k >= d.rows_T || k >= CH_THREADS - CHP_COL0 || r1 - r0 > CHP_COL0 ||
                       tiles > nwg || (long long)tiles * CH_THREADS < d.q || !d.wk)) {
        if (lead) ctl->status = DZG_PANIC;
        return;
    }
    if (lead) {
        ctl->neta_cur = neta;
        ctl->k_cur = k;
    }
    int p;
    if (kind == DZG_STEP_PRIMAL) {
        const int epos = cj.k;
        const int code = d.nbcode[epos];
        double zr = 0.0, zbr = 0.0;
        if (lead) {
            zr = d.z[epos];
            zbr = d.zbar[epos];
        }
        const double *a = chain_col<SHARD>(d, code, xrecv, w_rec);
        // this row's unit-column share of dx (fast_gemv_unit's term), loaded beside the gather
        const bool has_unit = has_row && bcode_i < 0;
        double unit_i = 0.0;
        if (has_unit) unit_i = code >= 0 ? a[-1 - bcode_i] : (code == bcode_i ? 1.0 : 0.0);
        int edslot = -1;
        if (lead && code < 0) edslot = d.dslot[-1 - code];
        chain_stage_ag(s_ag, k, code, a, d.drow, dr0, dr1);
        chain_beta(d, neta, code, a);
        ts.mark(slot); // 1: code, column, gather, (this workgroup's wave sum of) beta
        if (lead) {
            ctl->enter_code = code;
            ctl->zr = zr; // (SHARD: z is kept by the column's owner; k_chain_post takes it from
            ctl->zbar_r = zbr; //  the second exchange's records instead)
            ctl->enter_dslot = edslot;
            if (SHARD) ctl->enter_src = w_rec;
        }
        __syncthreads(); // the gathered column is complete
        double accs[MAXP];
        if (chain_wide<NARROW>(k)) // (block-uniform; NARROW: compile-time false)
            chain_dot_head<64>(d, r0, r1, k, s_ag, accs);
        else
            chain_dot_head<16>(d, r0, r1, k, s_ag, accs);
        chain_beta_published();
        ts.mark(slot); // 2: Binv0 rows
        if (!chain_barrier(ctl, bar, gen)) return;
        ts.mark(slot); // 3: barrier
        chain_beta_fetch(d, neta, code, s_beta);
        __syncthreads();
        if (chain_wide<NARROW>(k))
            chain_dot_tail<64>(d, r0, r1, k, neta, s_ag, s_beta, accs, s_dx);
        else
            chain_dot_tail<16>(d, r0, r1, k, neta, s_ag, s_beta, accs, s_dx);
        __syncthreads();
        // ratio test on this thread's row (src/simplex.rs:439-461)
        DzgCand2 best = dzg_cand2_none();
        if (has_row) {
            double dxi = s_dx[tid];
            if (has_unit) dxi += unit_i;
            d.dx[row] = dxi;
            const double scaled = mu * xbar_i;
            const double den = x_i + scaled;
            DzgCand2 cnd;
            cnd.r = dzg_div(dxi, den);
            cnd.k = row;
            cnd.h = -__builtin_inf();
            if (cnd.r > 0.0) best = dzg_better2(best, cnd);
            if (dzg_noise_zero(den, x_i, scaled, c.tau)) best.h = __builtin_inf();
        }
        ts.pin(best);
        const unsigned long long t_rowbest = ts.now();
        best = chain_best(best, r1 - r0);
        ts.pin(best);
        ts.site(DZG_SITE_PRE_ROWBEST, t_rowbest);
        if (tid == 0) {
            st_sc1(d.rx_r + blockIdx.x, best.r);
            st_sc1(d.rx_k + blockIdx.x, best.k);
            st_sc1(d.rx_h + blockIdx.x, best.h);
        }
        ts.mark(slot); // 4: eta share, candidates
        if (!chain_barrier(ctl, bar, gen)) return;
        ts.mark(slot); // 5: barrier
        const unsigned long long t_sc1 = ts.now();
        if (wave == 0) {
            const DzgCand2 w = chain_reduce_sc1(d.rx_r, d.rx_k, d.rx_h, nwg, lane);
            if (lane == 0) chain_put(s_c, 0, w);
        }
        __syncthreads();
        DzgCand2 cw = chain_get(s_c, 0);
        ts.pin(cw);
        ts.site(DZG_SITE_PRE_SC1, t_sc1);
        if (!fast_ratio_outcome(ctl, c, lead, cw, DZG_UNBOUNDED)) { // :313
            if (lead) ctl->bar_gen = gen;
            return;
        }
        p = cw.k;
        if (lead) ctl->leave_pos = p;
        ts.mark(slot); // 6: ratio test
    } else {
        p = ci.k;
    }
    // ---- BTRAN: v = row p of Binv on this thread's row; ONE trip: the leaving variable's code and
    // values, the row of Binv0, U's 64 entries of row p (wave 0, through LDS) and every entry of the
    // pending eta rows leave together, and nothing below waits for another load
    const int lcode = d.bcode[p];
    double xp = 0.0, xbp = 0.0;
    if (lead) { // (into registers first: a store to the control block between them would order the loads)
        xp = d.x[p];
        xbp = d.xbar[p];
    }
    double up = 0.0, base = 0.0, w[R_];
    if (tid < R_ && tid < neta) up = d.U[(long long)tid * d.ldw + p];
    int sd = -1;
    double zc = 0.0, zbc = 0.0, vr = 0.0;
    if constexpr (PRICE == 0) {
        if (has_row) {
            if (dslot_i >= 0) base = d.binv[(long long)p * d.ldb + dslot_i];
            fast_btran_eta_load(w, neta, d.W, d.ldw, row);
        }
        if (tid < R_) s_up[tid] = up;
        __syncthreads();
        if (has_row) {
            if (dslot_i < 0) base = lcode == -1 - row ? 1.0 : 0.0;
            vr = base - fast_btran_eta_fma(w, neta, s_up);
            d.v[row] = vr;
            if (dslot_i >= 0 && d.vc) d.vc[dslot_i] = vr; // (compact copy: the row-wise pricing pass's coefficients)
            // (and eta row neta of the kept compact copy, which k_chain_post renumbers with the pivot)
            if constexpr (WK)
                if (dslot_i >= 0 && d.wk && neta < R_) d.wk[(long long)neta * d.ldw + dslot_i] = vr;
        }
    } else {
        // in the same trip: this thread's compact column of row p and of the pending eta rows, the
        // compact slot of this thread's slack position, z and zbar where this lane's column sits
        const bool is_col = tile_on && cc >= 0 && cc < k; // (never a thread that has a row: r1 - r0 <= CHP_COL0)
        if (scode < 0) sd = d.dslot[-1 - scode];
        if (pos >= 0) {
            zc = d.z[pos];
            zbc = d.zbar[pos];
        }
        if (is_col) base = d.binv[(long long)p * d.ldb + cc];
        if (has_row && dslot_i >= 0) base = d.binv[(long long)p * d.ldb + dslot_i];
        if (has_row || is_col) // (ONE set of eta registers: the row's W, or the compact column's wk)
            fast_btran_eta_load(w, neta, is_col ? d.wk : d.W, d.ldw, is_col ? cc : row);
        if (tid < R_) s_up[tid] = up;
        __syncthreads();
        if (has_row || is_col) {
            if (has_row && dslot_i < 0) base = lcode == -1 - row ? 1.0 : 0.0;
            vr = base - fast_btran_eta_fma(w, neta, s_up);
        }
        if (has_row) {
            d.v[row] = vr;
            if (dslot_i >= 0 && d.vc) d.vc[dslot_i] = vr;
            if (dslot_i >= 0 && neta < R_) d.wk[(long long)neta * d.ldw + dslot_i] = vr; // (as above)
        }
    }
    if (lead) {
        ctl->xp = xp;
        ctl->xbp = xbp;
        ctl->leave_code = lcode;
        if (gen != c.bar_gen) ctl->bar_gen = gen;
    }
    ts.mark(slot); // primal 7 / dual 1: BTRAN row
    ts.done(slot);
    if constexpr (PRICE != 0) {
        // ---- the pricing pass of tile blockIdx.x (k_price_rows_small from its row list on; its stage
        // clocks, slot 4, under the stand-alone kernel's stage numbers: 1 list | 2 rows | 3 finish)
        if ((int)blockIdx.x >= tiles) return; // (no tile, and no position: tiles * 512 >= q)
        const auto *kd = chain_dev_reloaded(); // (`d` again, read here: see there)
        if (kd->ctl != ctl) { // (the segment does not start with `d`: see chain_dev_reloaded)
            if (lead) ctl->status = DZG_PANIC;
            return;
        }
        const long long ldt = kd->ldt;
        ts.stage = 1;
        long long *s_off = reinterpret_cast<long long *>(s_ag);
        double *s_coef = s_ag + PRS_ROWS;
        double(*s_part)[PRS_TILE] = reinterpret_cast<double(*)[PRS_TILE]>(s_ag + 2 * PRS_ROWS);
        if (cc >= 0) { // entry c < k: row drow[c] with vc[c]; entry k: the leaving slack's own row with 1.0
            const bool own = cc == k && lcode < 0;
            s_off[cc] = (long long)(own ? -1 - lcode : lrow_c) * ldt;
            s_coef[cc] = own ? 1.0 : vr;
        }
        __syncthreads();
        ts.mark(PRS_STAMP_SLOT); // 1: row list
        const double sv = sd >= 0 && sd < k ? s_coef[sd] : 0.0; // v of this thread's slack's row
        const int G = price_small_rows<2, PRICE, PR_BATCH>(kd->At, ldt, (int)blockIdx.x, k, lcode, s_off, s_coef,
                                                           s_part);
        __syncthreads();
        ts.mark(PRS_STAMP_SLOT); // 2: rows
        price_small_finish<false>(ts, G, s_part, pos, zc, zbc, scode, spos, sv, sz, szb, tiles, kd->q, kd->nbcode,
                                  kd->v, kd->dz, kd->z, kd->zbar, mu, c.tau, kd->rz_r, kd->rz_k, kd->rz_h);
        ts.mark(PRS_STAMP_SLOT); // 3: finish
        ts.done(PRS_STAMP_SLOT);
    }
}

// dz of ONE nonbasic position as the finishing launch of the row-wise pricing pass computes it
// (k_price_rows_finish, k_price_kernels.h): the G partial sums of the row groups in group order for
// a structural column, the unit column's single product otherwise.
__device__ __forceinline__ double chain_fold_dz(const DzgDev &d, int code, int G)
{
    if (code < 0) {
        const double p = 1.0 * -d.v[-1 - code];
        return 0.0 + p; // Iterator::sum identity + the single stored entry
    }
    const double *src = d.ppart + (code - d.col0);
    double sum = 0.0;
    int gg = 0;
    for (; gg + 8 <= G; gg += 8) { // eight partials side by side, added in group order
        double t[8];
#pragma unroll
        for (int e = 0; e < 8; ++e) t[e] = src[(long long)(gg + e) * d.ldt];
#pragma unroll
        for (int e = 0; e < 8; ++e) sum = sum + t[e];
    }
    for (; gg < G; ++gg) sum = sum + src[(long long)gg * d.ldt];
    return -sum;
}

// ---------------------------------------------------------------------------------
// k_chain_post: a dual step's ratio test and FTRAN (src/simplex.rs:324-325, :226-229), the pivot's
// books (fast_rows.h; the last wave of workgroup 0, beside everybody's update), pivot() x4
// (:262-265, :410-421) with the eta append, and the first-pivot candidates of the next iteration
// (:423-437).  only_partials != 0: the candidates only.
// ---------------------------------------------------------------------------------
// SHARD: the ratio test of a dual step is the merge of the ranks' proposals (xrecv: the second
// exchange's records), z, zbar, dz of the entering position come from its owner's record, and z is
// only kept -- and offered as a first-pivot candidate -- for slack positions and owned columns.
// FOLD (one GPU, the row-wise pricing pass, round 4): the pass's FINISHING launch is this kernel's
// head -- a workgroup owns its columns of z anyway: thread t adds the row groups' partial sums of
// position q0 + t itself (the finishing launch's arithmetic, chain_fold_dz), a dual step's ratio
// candidates are reduced per workgroup and cross one more device-wide barrier (a primal step needs
// none), and dz_r of the entering position is re-derived by every workgroup.  One launch and its
// cold first touches less per pivot; the same sums and candidates, bit for bit.
template <bool SHARD, int MAXP, bool NARROW, bool NOFOLD>
__global__ __launch_bounds__(CH_THREADS) void k_chain_post(const DzgDev d, unsigned long long *bar,
                                                           const DzgPivotArgs pa, int only_partials,
                                                           int nrz, unsigned long long *dbg,
                                                           const double *__restrict__ xrecv, int fold_arg)
{
    const int fold = chain_fold_on<NOFOLD>(fold_arg); // (block-uniform; NOFOLD: compile-time 0)
    __shared__ double s_ag[CH_AGCAP];
    __shared__ double s_beta[R_], s_dx[CH_THREADS];
    __shared__ double s_dxp;
    __shared__ ChainSlots s_c;
    ChainStamps ts;
    ts.start(only_partials ? nullptr : dbg);
    const unsigned long long t_books = (dbg && !only_partials && blockIdx.x == 0 && threadIdx.x == CH_THREADS - 64)
                                           ? __builtin_amdgcn_s_memrealtime()
                                           : 0ull;
    int slot = 2;
    DzgCtl *ctl = d.ctl;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int m = d.m, q = d.q;
    const bool lead = blockIdx.x == 0 && tid == 0;
    // ---- first touches, side by side: the pricing pass's candidates, this thread's row and column
    DzgCand2 mine = dzg_cand2_none();
    ChainSpec sp;
    const bool one_wave = chain_one_wave<NOFOLD>(nrz); // (block-uniform) the candidates fit one wave's registers
    if (SHARD || fold) {
        // (the candidates travel in the exchange records / are formed below)
    } else if (!only_partials && one_wave) {
        if (wave == 0) chain_spec_load(sp, d.rz_r, d.rz_k, d.rz_h, lane);
    } else if (!only_partials) {
#pragma unroll
        for (int j = 0; j < 4; ++j) { // (4096 entries: harmless past nrz; a primal step ignores them)
            const int i = tid + CH_THREADS * j;
            DzgCand2 o;
            o.r = d.rz_r[i];
            o.k = d.rz_k[i];
            o.h = d.rz_h[i];
            if (i < nrz) mine = dzg_better2(mine, o);
        }
        for (int i = tid + 4 * CH_THREADS; i < nrz; i += CH_THREADS) {
            DzgCand2 o;
            o.r = d.rz_r[i];
            o.k = d.rz_k[i];
            o.h = d.rz_h[i];
            mine = dzg_better2(mine, o);
        }
    }
    int r0, r1, q0, q1;
    chain_rows(m, r0, r1);
    chain_cols(q, q0, q1);
    const int row = r0 + tid, col = q0 + tid;
    const bool has_row = row < r1, has_col = col < q1;
    double x_i = 0.0, xbar_i = 0.0, v_i = 0.0, dx_i = 0.0, z_k = 0.0, zbar_k = 0.0, dz_k = 0.0;
    int bcode_i = 0, nbcode_k = -1;
    if (has_row) {
        x_i = d.x[row];
        xbar_i = d.xbar[row];
        if (!only_partials) {
            v_i = d.v[row];
            dx_i = d.dx[row]; // (a dual step computes its own below)
            bcode_i = d.bcode[row];
        }
    }
    if (has_col) {
        z_k = d.z[col];
        zbar_k = d.zbar[col];
        if (!only_partials && !fold) dz_k = d.dz[col];
        if (SHARD || fold) nbcode_k = d.nbcode[col]; // (before the books of this launch rewrite position r's)
    }
    DzgCtl c = *ctl;
    if (c.status != DZG_RUNNING) return;
    unsigned long long gen = c.bar_gen;
    // what the update needs (all block-uniform)
    int p = 0, r = 0, teta = 0, wzero = -1, del_ce = -1, del_last = -1, app_col = -1, new_code_r = -1;
    double t = 0.0, s = 0.0, tbar = 0.0, sbar = 0.0, rdxp = 0.0, tau = c.tau;
    if (!only_partials) {
        const int neta = c.neta_cur, k = c.k_cur, kind = c.kind;
        const int ci = c.leave_code;
        const double xp = c.xp, xbp = c.xbp;
        p = c.leave_pos;
        int cj, edslot;
        double zr, zbr, dzr, dxp;
        int G = (k + 1 + DZG_PR_BATCH - 1) / DZG_PR_BATCH; // row groups of the pricing pass (FOLD)
        G = G > DZG_PR_GMAX ? DZG_PR_GMAX : G;
        if (!SHARD && fold) {
            // this workgroup's (position, row group) partial sums, fetched by ALL its threads in one
            // trip through LDS (the gathered column's buffer is free until FTRAN); the owner of a
            // position then adds its G values in group order -- chain_fold_dz's sum, without 32
            // loads queuing behind one thread
            const int ncols = q1 - q0;
            int *s_code = reinterpret_cast<int *>(s_dx); // (CH_THREADS doubles: room for 512 codes)
            if (has_col) s_code[tid] = nbcode_k;
            __syncthreads();
            if ((long long)ncols * G <= CH_AGCAP) {
                for (int idx = tid; idx < ncols * G; idx += CH_THREADS) {
                    const int g = idx / ncols, pl = idx - g * ncols;
                    const int code = s_code[pl];
                    s_ag[idx] = code >= 0 ? d.ppart[(long long)g * d.ldt + (code - d.col0)] : 0.0;
                }
                __syncthreads();
                if (has_col) {
                    if (nbcode_k < 0) {
                        dz_k = chain_fold_dz(d, nbcode_k, G);
                    } else {
                        double sum = 0.0;
                        for (int g = 0; g < G; ++g) sum = sum + s_ag[g * ncols + tid];
                        dz_k = -sum;
                    }
                }
                __syncthreads(); // (s_ag and s_dx are about to be reused)
            } else if (has_col) {
                dz_k = chain_fold_dz(d, nbcode_k, G);
            }
        }
        if (kind == DZG_STEP_DUAL) {
            const int dr0 = tid < k ? d.drow[tid] : -1;
            const int dr1 = tid + CH_THREADS < k ? d.drow[tid + CH_THREADS] : -1;
            DzgCand2 cw;
            int w_rec = -1;
            if (SHARD) {
                w_rec = shard_merge(xrecv, d.xstride, d.world, cw);
            } else if (fold) {
                // the ratio test of the z side (src/simplex.rs:449-460) on this workgroup's columns;
                // the workgroups' winners cross a barrier, everybody reduces them
                DzgCand2 cnd = dzg_cand2_none();
                if (has_col) {
                    const double scaled = c.mu * zbar_k, den = z_k + scaled;
                    DzgCand2 o;
                    o.r = dzg_div(dz_k, den);
                    o.k = col;
                    o.h = -__builtin_inf();
                    if (o.r > 0.0) cnd = dzg_better2(cnd, o);
                    if (dzg_noise_zero(den, z_k, scaled, c.tau)) cnd.h = __builtin_inf();
                }
                cnd = chain_best(cnd, q1 - q0);
                if (tid == 0) {
                    st_sc1(d.rz_r + blockIdx.x, cnd.r);
                    st_sc1(d.rz_k + blockIdx.x, cnd.k);
                    st_sc1(d.rz_h + blockIdx.x, cnd.h);
                }
                if (!chain_barrier(ctl, bar, gen)) return;
                if (wave == 0) {
                    const DzgCand2 w = chain_reduce_sc1(d.rz_r, d.rz_k, d.rz_h, (int)gridDim.x, lane);
                    if (lane == 0) chain_put(s_c, 0, w);
                }
                __syncthreads();
                cw = chain_get(s_c, 0);
            } else if (one_wave) {
                if (wave == 0) {
                    chain_spec_pin(ts, sp);
                    const unsigned long long t_site = ts.now();
                    DzgCand2 w = chain_spec_reduce(sp, nrz, lane);
                    ts.pin(w);
                    ts.site(DZG_SITE_POST_RATIO, t_site);
                    if (lane == 0) chain_put(s_c, 0, w);
                }
                __syncthreads();
                cw = chain_get(s_c, 0);
            } else {
                cw = dzg_block_best2(mine);
            }
            if (!fast_ratio_outcome(ctl, c, lead, cw, DZG_INFEASIBLE)) { // :325
                if (lead && gen != c.bar_gen) ctl->bar_gen = gen;
                return;
            }
            slot = 3;
            ts.mark(slot); // 0: first touches + ratio test
            r = cw.k;
            if (SHARD) { // the entering column's code and z, zbar, dz travel in the winner's record
                const double *rec = xrecv + (long long)w_rec * d.xstride;
                cj = (int)rec[5];
                zr = rec[2];
                zbr = rec[3];
                dzr = rec[4];
                if (lead) {
                    ctl->enter_src = w_rec;
                    ctl->zr = zr;
                    ctl->zbar_r = zbr;
                    ctl->dz_r = dzr;
                    ctl->use_record = 1;
                }
            } else {
                cj = d.nbcode[r];
                zr = d.z[r];
                zbr = d.zbar[r];
                dzr = fold ? chain_fold_dz(d, cj, G) : d.dz[r];
            }
            const double *a = chain_col<SHARD>(d, cj, xrecv, w_rec);
            edslot = cj < 0 ? d.dslot[-1 - cj] : -1;
            const bool has_unit = has_row && bcode_i < 0;
            double unit_i = 0.0, unit_p = 0.0;
            if (has_unit) unit_i = cj >= 0 ? a[-1 - bcode_i] : (cj == bcode_i ? 1.0 : 0.0);
            if (ci < 0) unit_p = cj >= 0 ? a[-1 - ci] : (cj == ci ? 1.0 : 0.0);
            chain_stage_ag(s_ag, k, cj, a, d.drow, dr0, dr1);
            chain_beta(d, neta, cj, a);
            ts.mark(slot); // 1: loads, code, column, gather, (this workgroup's wave sum of) beta
            if (lead) {
                ctl->enter_pos = r;
                ctl->enter_code = cj;
            }
            c.enter_pos = r;
            c.enter_code = cj;
            __syncthreads(); // the gathered column is complete
            // Binv0's share of this workgroup's rows, and of row p: every workgroup computes dx_p
            // itself (the arithmetic of the row's owner, so the same bits) and then needs nobody
            // else's result for the step lengths
            const int k2 = (k + 1) & ~1;
            double accs[MAXP], accp;
            if (chain_wide<NARROW>(k)) { // (block-uniform; NARROW: compile-time false)
                chain_dot_head<64>(d, r0, r1, k, s_ag, accs);
                accp = fast_gemv_row_head<64>(wave == CH_NW - 1 ? p : m, m, k2, d.binv, d.ldb, s_ag, lane);
            } else {
                chain_dot_head<16>(d, r0, r1, k, s_ag, accs);
                accp = fast_gemv_row_head<16>(wave == CH_NW - 1 && lane < 16 ? p : m, m, k2, d.binv, d.ldb, s_ag,
                                              lane % 16);
            }
            chain_beta_published();
            ts.mark(slot); // 2: Binv0 rows
            if (!chain_barrier(ctl, bar, gen)) return;
            ts.mark(slot); // 3: barrier
            chain_beta_fetch(d, neta, cj, s_beta);
            __syncthreads();
            if (chain_wide<NARROW>(k)) {
                chain_dot_tail<64>(d, r0, r1, k, neta, s_ag, s_beta, accs, s_dx);
                if (wave == CH_NW - 1) {
                    const double acc = fast_gemv_row_tail<64>(accp, p, m, neta, d.U, d.ldw, s_beta, lane);
                    if (lane == 0) s_dxp = ci < 0 ? acc + unit_p : acc;
                }
            } else {
                chain_dot_tail<16>(d, r0, r1, k, neta, s_ag, s_beta, accs, s_dx);
                if (wave == CH_NW - 1) {
                    const double acc = fast_gemv_row_tail<16>(accp, lane < 16 ? p : m, m, neta, d.U, d.ldw,
                                                              s_beta, lane % 16);
                    if (lane == 0) s_dxp = ci < 0 ? acc + unit_p : acc;
                }
            }
            __syncthreads();
            dxp = s_dxp;
            if (has_row) {
                dx_i = s_dx[tid];
                if (has_unit) dx_i += unit_i;
                d.dx[row] = dx_i;
            }
            ts.mark(slot); // 4: eta share
        } else {
            r = c.enter_pos;
            cj = c.enter_code;
            zr = c.zr;
            zbr = c.zbar_r;
            dzr = (!SHARD && fold) ? chain_fold_dz(d, cj, G) : d.dz[r];
            if (SHARD) { // the owner of the entering position has published z, zbar, dz
                int w_rec = -1;
                for (int rk = 0; rk < d.world && w_rec < 0; ++rk)
                    if ((int)xrecv[(long long)rk * d.xstride + 1] == r) w_rec = rk;
                if (w_rec < 0) { // no rank owns the entering position: cannot happen
                    if (lead) ctl->status = DZG_PANIC;
                    return;
                }
                const double *rec = xrecv + (long long)w_rec * d.xstride;
                zr = rec[2];
                zbr = rec[3];
                dzr = rec[4];
                if (lead) {
                    ctl->zr = zr;
                    ctl->zbar_r = zbr;
                    ctl->dz_r = dzr;
                    ctl->use_record = 1;
                }
            }
            edslot = c.enter_dslot;
            dxp = d.dx[p];
            ts.mark(slot); // 0: first touches
        }
        const DzgPivotScalars ps = fast_pivot_scalars(xp, xbp, dxp, zr, zbr, dzr, neta, c.max_pivot_err);
        const bool appended = ci < 0, deleted = cj < 0;
        new_code_r = ci; // the leaving variable takes nonbasic position r
        if (blockIdx.x == 0 && wave == CH_NW - 1) { // one wave keeps the books
            c.neta = neta;
            c.ncompact = k;
            fast_pivot_books_s(ctl, c, pa, ps, 1);
            if (t_books && kind == DZG_STEP_DUAL && lane == 0) { // (the books lane's own clock)
                __builtin_amdgcn_s_waitcnt(0);
                dbg[16 * DZG_SITE_SLOT + DZG_SITE_BOOKS] += __builtin_amdgcn_s_memrealtime() - t_books;
                dbg[16 * (DZG_SITE_SLOT + 1) + DZG_SITE_BOOKS] += 1;
            }
        }
        if (!ps.ok) { // (the books have set DZG_PANIC, src/simplex.rs:466)
            if (lead && gen != c.bar_gen) ctl->bar_gen = gen;
            return;
        }
        if (deleted) {
            del_last = k + (appended ? 1 : 0) - 1;
            del_ce = edslot;
        }
        if (appended) app_col = k;
        if (lead && gen != c.bar_gen) ctl->bar_gen = gen;
        t = ps.t;
        s = ps.s;
        tbar = ps.tbar;
        sbar = ps.sbar;
        teta = neta; // index of the eta appended now
        wzero = cj < 0 ? -1 - cj : -1;
        rdxp = 1.0 / dxp;
        if (c.tie_tol >= 0.0) { // the tolerance the books are setting
            double adaptive = 64.0 * ps.max_err;
            if (c.drift_tau > adaptive) adaptive = c.drift_tau;
            tau = adaptive > c.tie_tol ? adaptive : c.tie_tol;
        }
        ts.mark(slot); // primal 1 / dual 5: step lengths
    }
    // The kept compact copy of the eta rows (d.wk, common.h) is renumbered as the pivot renumbers the
    // compact columns, by ONE wave, lane t for eta row t <= teta: not the books' wave of workgroup 0, not
    // wave 0 (rows, columns, the reductions) and none that runs a beta item or row p.  An appending
    // pivot: column k := W (v for the eta appended now) at the leaving slack's constraint row; a deleting
    // one: the last column -- the appended one when both happen -- takes the deleted one's place.
    // Loads and stores sit HERE, beside everybody's update: fetched with the kernel's first touches the
    // operands stayed live through the whole kernel and cost every workgroup scalar-register spills
    // (k_chain_post 12.85 -> 13.66 us, profiles/price_in_pre.txt).  Nothing else in the launch reads
    // or writes wk; the books zero W at an ENTERING slack's row only, another row.
    // Compiled into the one-pass narrow kernel only, the one a batch with d.wk set runs (dzg_chain_keeps_wk).
    if constexpr (!SHARD && NARROW && MAXP == 1 && NOFOLD)
    if (d.wk && !only_partials && (int)blockIdx.x == ((int)gridDim.x > 1 ? 1 : 0) && wave == 2 &&
        lane <= teta && (app_col >= 0 || del_last >= 0)) {
        double *wrow = d.wk + (long long)lane * d.ldw;
        double wk_app = 0.0;
        if (app_col >= 0) {
            const int rl = -1 - new_code_r; // (new_code_r = the leaving variable's code: a slack's here)
            wk_app = lane < teta ? d.W[(long long)lane * d.ldw + rl] : d.v[rl];
        }
        if (del_last >= 0) {
            if (del_ce != del_last) wrow[del_ce] = app_col == del_last ? wk_app : wrow[del_last];
        } else {
            wrow[app_col] = wk_app;
        }
    }
    // ---- update of this thread's row and column; candidates on the updated values
    DzgCand2 bx = dzg_cand2_none(), bz = dzg_cand2_none();
    if (has_row) {
        double xi = x_i, xb = xbar_i;
        if (!only_partials) {
            const double a = t * dx_i, b = tbar * dx_i;
            xi = (row == p) ? t : xi - a;
            xb = (row == p) ? tbar : xb - b;
            d.x[row] = xi;
            d.xbar[row] = xb;
            d.U[(long long)teta * d.ldw + row] = (row == p ? dx_i - 1.0 : dx_i) * rdxp;
            d.W[(long long)teta * d.ldw + row] = (row == wzero) ? 0.0 : v_i;
            // Binv0's columns: a leaving slack appends e_p, an entering slack deletes its column
            // (the last one takes its place).  Nobody reads Binv0 any more in this launch.
            double *brow = d.binv + (long long)row * d.ldb;
            if (del_last >= 0) {
                const double last_val = (app_col == del_last) ? (row == p ? 1.0 : 0.0) : brow[del_last];
                if (del_ce != del_last) brow[del_ce] = last_val;
                brow[del_last] = 0.0;
            } else if (app_col >= 0 && row == p) {
                brow[app_col] = 1.0;
            }
        }
        dzg_first_pivot_entry(bx, xi, xb, row, tau);
    }
    if (has_col) {
        double zk = z_k, zb = zbar_k;
        if (!only_partials) {
            const double a = s * dz_k, b = sbar * dz_k;
            zk = (col == r) ? s : zk - a;
            zb = (col == r) ? sbar : zb - b;
            d.z[col] = zk;
            d.zbar[col] = zb;
        }
        bool mine = true; // SHARD: z is only kept for slack positions and owned columns
        if (SHARD) {
            const int code = (!only_partials && col == r) ? new_code_r : nbcode_k;
            mine = code < 0 || (code >= d.col0 && code < d.col1);
        }
        if (mine) dzg_first_pivot_entry(bz, zk, zb, col, tau);
    }
    ts.pin(bx);
    ts.pin(bz);
    const unsigned long long t_best = ts.now();
    chain_best_pair(bx, r1 - r0, bz, q1 - q0);
    ts.pin(bx);
    ts.pin(bz);
    ts.site(DZG_SITE_POST_BX, t_best);
    if (tid == 0) {
        d.fpx_r[blockIdx.x] = bx.r;
        d.fpx_k[blockIdx.x] = bx.k;
        d.fpx_h[blockIdx.x] = bx.h;
        d.fpz_r[blockIdx.x] = bz.r;
        d.fpz_k[blockIdx.x] = bz.k;
        d.fpz_h[blockIdx.x] = bz.h;
        if (blockIdx.x == 0) ctl->fp_count = (int)gridDim.x;
    }
    ts.mark(slot); // primal 2 / dual 6: update + candidates
    if (slot == 3) ts.since_start(DZG_SITE_POST_END);
    ts.done(slot);
}

static_assert(CH_BAR_WORDS == DZG_CHAIN_BAR_WORDS, "barrier counter block");

// ---------------------------------------------------------------------------------
// Which instantiation runs a launch: the ONE rule both launchers and the test entry point share.
// Returned: DZG_CHAIN_* of common.h.  Everything the rule reads is known to the host before the
// batch is enqueued and is handed to the kernel unchanged, so a kernel never meets what it lacks:
//   passes  a workgroup's share is chain_rows' `per` rows, a pass covers 8 * 64 / LPR of them, and
//           LPR is 16 only when the whole batch stays at k <= 512; MAXP too small would still be
//           right (chain_dot_tail's trailing loop), only slower, so the rule takes the smallest
//           instantiation that covers the share and the generic kernel when none does.
//   narrow  the host's bound on k for the batch (d.k_hint = ncompact + batch, the bound
//           dzg_price_small relies on) is known and <= 512.  0 = nobody refreshed the bound (the
//           phases are driven from outside): generic.  (k_chain_pre ends a NARROW launch that
//           meets k > 512 with DZG_PANIC rather than computing with it.)
//   nofold  fold == 0 and nrz <= 256, the values the kernel is launched with.
// A column-sharded rank (shard != 0) runs the generic kernels: it has instantiations of its own
// (SHARD) and no specialised twins.
// ---------------------------------------------------------------------------------
static int chain_pick(int m, int grid, int k_bound, int fold, int nrz, int shard, int post)
{
    if (shard || grid < 1 || m < 0 || k_bound <= 0) return DZG_CHAIN_GENERIC;
    const int per = ((m + grid - 1) / grid + 3) & ~3; // chain_rows
    const bool narrow = k_bound <= 512;
    const int rows_per_pass = CH_NW * (narrow ? 64 / 16 : 64 / 64);
    const int need = (per + rows_per_pass - 1) / rows_per_pass;
    const bool nofold = fold == 0 && nrz <= 256;
    if (narrow) {
        if (need <= 1 && (!post || nofold)) return DZG_CHAIN_P1_NARROW;
        if (need <= 4) return DZG_CHAIN_P4_NARROW;
        return DZG_CHAIN_GENERIC;
    }
    return need <= 4 ? DZG_CHAIN_P4_WIDE : DZG_CHAIN_GENERIC;
}

// Test hook (include/dantzig_amd.h): the rule above, as properties.  Pure host code.
extern "C" int dzg_debug_chain_instance(int32_t m, int32_t grid, int32_t k_bound, int32_t fold, int32_t nrz,
                                        int32_t shard, int32_t post)
{
    switch (chain_pick(m, grid, k_bound, fold, nrz, shard, post)) {
    case DZG_CHAIN_P1_NARROW: return 1 | 0x100 | (post ? 0x200 : 0);
    case DZG_CHAIN_P4_NARROW: return 4 | 0x100;
    case DZG_CHAIN_P4_WIDE: return 4;
    default: return CH_MAXP;
    }
}

// Residency of the chain kernels as the runtime computes it (registers, LDS, 512 threads): the
// smallest count over every instantiation a launcher can choose; 0 = some kernel does not fit a CU
// at all.  (The barrier needs every workgroup of a launch resident, whichever kernel runs it.)
int dzg_chain_resident_per_cu(void)
{
    const void *kernels[] = {
        reinterpret_cast<const void *>(k_chain_pre<false, CH_MAXP, false>),
        reinterpret_cast<const void *>(k_chain_pre<true, CH_MAXP, false>),
        reinterpret_cast<const void *>(k_chain_pre<false, 1, true>),
        reinterpret_cast<const void *>(k_chain_pre<false, 4, true>),
        reinterpret_cast<const void *>(k_chain_pre<false, 4, false>),
        reinterpret_cast<const void *>(k_chain_pre<false, 1, true, 1>),
        reinterpret_cast<const void *>(k_chain_pre<false, 1, true, 2>),
        reinterpret_cast<const void *>(k_chain_post<false, CH_MAXP, false, false>),
        reinterpret_cast<const void *>(k_chain_post<true, CH_MAXP, false, false>),
        reinterpret_cast<const void *>(k_chain_post<false, 1, true, true>),
        reinterpret_cast<const void *>(k_chain_post<false, 4, true, false>),
        reinterpret_cast<const void *>(k_chain_post<false, 4, false, false>),
    };
    int least = 1 << 20, n = 0;
    for (const void *kern : kernels) {
        if (hipOccupancyMaxActiveBlocksPerMultiprocessor(&n, kern, CH_THREADS, 0) != hipSuccess) return 0;
        least = n < least ? n : least;
    }
    return least;
}

// xrecv != nullptr: a column-sharded rank (replicated matrix), records of the exchange just done.
// instances == 0 (DZG_CHAIN_INSTANCES=0, the A/B switch): the generic kernels always.
// The host's rule for the pricing tail of k_chain_pre (PRICE): the fused small-k pass would run
// (small = dzg_price_small), the chain pick is the one-pass narrow kernel (rows on threads < 32, a
// thread per compact entry), every tile and every nonbasic position has a workgroup, and this slot's
// pricing pass is not being timed on its own (a timed slot runs the three launches, so that the
// events bracket k_price_rows_small alone).  More tiles than workgroups stays unfused: a workgroup
// looping over four tiles would serialise four row trips.
int dzg_chain_price_rule(int m, int grid, int k_hint, int tiles, long long q, int small, int timed)
{
    if (!small || timed || tiles < 1 || tiles > grid || (long long)tiles * CH_THREADS < q) return 0;
    if (k_hint <= 0 || k_hint >= CH_THREADS - CHP_COL0) return 0;
    return chain_pick(m, grid, k_hint, 0, 0, 0, 0) == DZG_CHAIN_P1_NARROW;
}
int dzg_chain_price_fused(const DzgDev &d, int grid, int small, int timed)
{
    return d.wk && d.At && dzg_chain_price_rule(d.m, grid, d.k_hint, dzg_price_small_partials(d), d.q, small, timed);
}
// 1: a chain batch enqueued now may run with d.wk set -- some slot of it can price in the tail, and every
// launch of it, timed slots included, picks the one-pass narrow kernels, the only ones that keep the copy
int dzg_chain_keeps_wk(const DzgDev &d, int grid, int small)
{
    const int tiles = dzg_price_small_partials(d);
    return d.At && dzg_chain_price_rule(d.m, grid, d.k_hint, tiles, d.q, small, 0) &&
           chain_pick(d.m, grid, d.k_hint, 0, tiles, 0, 1) == DZG_CHAIN_P1_NARROW;
}

void dzg_launch_chain_pre(const DzgDev &d, int grid, unsigned long long *bar,
                          unsigned long long *dbg, const double *xrecv, hipStream_t st, int instances, int price)
{
    const int which = instances ? chain_pick(d.m, grid, d.k_hint, 0, 0, xrecv != nullptr, 0) : DZG_CHAIN_GENERIC;
    if (price && !xrecv) { // (the rule above held: P1_NARROW whatever `instances` says)
        // (k < 255 for the whole batch: at most sixteen row groups, one per half-wave; else two)
        if (d.k_hint < 16 * DZG_PR_BATCH - 1)
            hipLaunchKernelGGL((k_chain_pre<false, 1, true, 1>), dim3(grid), dim3(CH_THREADS), 0, st, d, bar, dbg, xrecv);
        else
            hipLaunchKernelGGL((k_chain_pre<false, 1, true, 2>), dim3(grid), dim3(CH_THREADS), 0, st, d, bar, dbg, xrecv);
        return;
    }
    if (xrecv)
        hipLaunchKernelGGL((k_chain_pre<true, CH_MAXP, false>), dim3(grid), dim3(CH_THREADS), 0, st, d, bar, dbg, xrecv);
    else if (which == DZG_CHAIN_P1_NARROW)
        hipLaunchKernelGGL((k_chain_pre<false, 1, true>), dim3(grid), dim3(CH_THREADS), 0, st, d, bar, dbg, xrecv);
    else if (which == DZG_CHAIN_P4_NARROW)
        hipLaunchKernelGGL((k_chain_pre<false, 4, true>), dim3(grid), dim3(CH_THREADS), 0, st, d, bar, dbg, xrecv);
    else if (which == DZG_CHAIN_P4_WIDE)
        hipLaunchKernelGGL((k_chain_pre<false, 4, false>), dim3(grid), dim3(CH_THREADS), 0, st, d, bar, dbg, xrecv);
    else
        hipLaunchKernelGGL((k_chain_pre<false, CH_MAXP, false>), dim3(grid), dim3(CH_THREADS), 0, st, d, bar, dbg, xrecv);
}

void dzg_launch_chain_post(const DzgDev &d, int grid, unsigned long long *bar,
                           unsigned long long *dbg, int only_partials, int nrz, const double *xrecv,
                           hipStream_t st, int fold, int price_small, int instances)
{
    DzgPivotArgs pa = dzg_pivot_args(d);
    pa.price_small = price_small;
    const int which = instances ? chain_pick(d.m, grid, d.k_hint, fold, nrz, xrecv != nullptr, 1) : DZG_CHAIN_GENERIC;
    if (xrecv)
        hipLaunchKernelGGL((k_chain_post<true, CH_MAXP, false, false>), dim3(grid), dim3(CH_THREADS), 0, st, d, bar,
                           pa, only_partials, nrz, dbg, xrecv, 0);
    else if (which == DZG_CHAIN_P1_NARROW)
        hipLaunchKernelGGL((k_chain_post<false, 1, true, true>), dim3(grid), dim3(CH_THREADS), 0, st, d, bar,
                           pa, only_partials, nrz, dbg, xrecv, fold);
    else if (which == DZG_CHAIN_P4_NARROW)
        hipLaunchKernelGGL((k_chain_post<false, 4, true, false>), dim3(grid), dim3(CH_THREADS), 0, st, d, bar,
                           pa, only_partials, nrz, dbg, xrecv, fold);
    else if (which == DZG_CHAIN_P4_WIDE)
        hipLaunchKernelGGL((k_chain_post<false, 4, false, false>), dim3(grid), dim3(CH_THREADS), 0, st, d, bar,
                           pa, only_partials, nrz, dbg, xrecv, fold);
    else
        hipLaunchKernelGGL((k_chain_post<false, CH_MAXP, false, false>), dim3(grid), dim3(CH_THREADS), 0, st, d, bar,
                           pa, only_partials, nrz, dbg, xrecv, fold);
}

// ---------------------------------------------------------------------------------
// Test hook: a co-tenant on the device.  Each workgroup keeps 128 KB of LDS (so that no chain
// workgroup -- 136 KB -- fits beside it on the CU) and watches the 100 MHz clock until the time is
// up: an exit every wave reaches.  Launched on a stream of its own.
// ---------------------------------------------------------------------------------
__global__ __launch_bounds__(64) void k_debug_hold(unsigned long long ticks, int *sink, int *started)
{
    extern __shared__ double s_hold[];
    s_hold[threadIdx.x] = 1.0;
    // (host-visible: the host waits until every workgroup of the co-tenant holds its CU)
    if (threadIdx.x == 0) __hip_atomic_fetch_add(started, 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
    const unsigned long long t0 = __builtin_amdgcn_s_memrealtime();
    unsigned long long spins = 0;
    while (__builtin_amdgcn_s_memrealtime() - t0 < ticks && spins < (1ull << 34)) {
        __builtin_amdgcn_s_sleep(64);
        ++spins;
    }
    if (s_hold[threadIdx.x] == 2.0) *sink = 1; // (keeps the allocation alive)
}

static hipStream_t g_hold_stream = nullptr;
static int *g_hold_sink = nullptr;
static int *g_hold_started = nullptr; // pinned host memory

// Returns once every workgroup of the co-tenant is resident (or DZG_E_DEVICE after two seconds):
// whether it gets in the way must not depend on how the two streams' first launches race.
extern "C" int dzg_debug_hold_cus(int32_t device, int32_t workgroups, double seconds)
{
    if (workgroups < 1 || workgroups > 256 || !(seconds > 0.0) || seconds > 30.0) return DZG_E_ARG;
    if (hipSetDevice(device) != hipSuccess) return DZG_E_DEVICE;
    const int lds = 128 * 1024;
    if (hipFuncSetAttribute(reinterpret_cast<const void *>(k_debug_hold),
                            hipFuncAttributeMaxDynamicSharedMemorySize, lds) != hipSuccess)
        return DZG_E_DEVICE;
    if (!g_hold_stream && hipStreamCreateWithFlags(&g_hold_stream, hipStreamNonBlocking) != hipSuccess)
        return DZG_E_DEVICE;
    if (!g_hold_sink && hipMalloc(&g_hold_sink, sizeof(int)) != hipSuccess) return DZG_E_NOMEM;
    if (!g_hold_started && hipHostMalloc(&g_hold_started, sizeof(int), hipHostMallocCoherent) != hipSuccess)
        return DZG_E_NOMEM;
    *(volatile int *)g_hold_started = 0;
    hipLaunchKernelGGL(k_debug_hold, dim3(workgroups), dim3(64), lds, g_hold_stream,
                       (unsigned long long)(seconds * 1e8), g_hold_sink, g_hold_started);
    if (hipGetLastError() != hipSuccess) return DZG_E_DEVICE;
    const auto t0 = std::chrono::steady_clock::now();
    while (*(volatile int *)g_hold_started < workgroups) {
        if (std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count() > 2.0) return DZG_E_DEVICE;
    }
    return 0;
}

extern "C" int dzg_debug_hold_wait(void)
{
    if (!g_hold_stream) return 0;
    return hipStreamSynchronize(g_hold_stream) == hipSuccess ? 0 : DZG_E_DEVICE;
}

// ---------------------------------------------------------------------------------
// Test hook: the straight-line argmax reduction on arrays of cases (include/dantzig_amd.h).
// One wave (forms 0, 1) or one workgroup of 512 threads (form 2) per case; every lane is active.
// ---------------------------------------------------------------------------------
__global__ __launch_bounds__(CH_THREADS) void k_debug_cand_reduce(int form, const double *__restrict__ r,
                                                                  const int *__restrict__ k,
                                                                  const double *__restrict__ h,
                                                                  const int *__restrict__ count,
                                                                  double *out_r, int *out_k, double *out_h)
{
    const long long cs = blockIdx.x;
    const int tid = threadIdx.x;
    DzgCand2 w;
    if (form == 0) {
        DzgCand2 c;
        c.r = r[cs * 64 + tid];
        c.k = k[cs * 64 + tid];
        c.h = h[cs * 64 + tid];
        w = dzg_wave_best2_flat<64>(c);
    } else if (form == 1) {
        ChainSpec sp;
        chain_spec_load(sp, r + cs * 256, k + cs * 256, h + cs * 256, tid);
        w = chain_spec_reduce(sp, count[cs], tid);
    } else {
        DzgCand2 c;
        c.r = r[cs * CH_THREADS + tid];
        c.k = k[cs * CH_THREADS + tid];
        c.h = h[cs * CH_THREADS + tid];
        w = dzg_block_best2_flat<8>(c, false);
    }
    if (tid == 0) {
        out_r[cs] = w.r;
        out_k[cs] = w.k;
        out_h[cs] = w.h;
    }
}

extern "C" int dzg_debug_cand_reduce(int32_t device, int32_t form, int64_t ncases, const double *r,
                                     const int32_t *k, const double *h, const int32_t *count, double *out_r,
                                     int32_t *out_k, double *out_h)
{
    if (form < 0 || form > 2 || ncases < 1 || ncases > (1 << 20) || !r || !k || !h || !out_r || !out_k ||
        !out_h || (form == 1 && !count))
        return DZG_E_ARG;
    if (hipSetDevice(device) != hipSuccess) return DZG_E_DEVICE;
    const size_t width = form == 0 ? 64 : (form == 1 ? 256 : CH_THREADS), n = (size_t)ncases * width;
    double *d_r = nullptr, *d_h = nullptr, *d_or = nullptr, *d_oh = nullptr;
    int *d_k = nullptr, *d_cnt = nullptr, *d_ok = nullptr;
    int rc = DZG_E_NOMEM;
    if (hipMalloc(&d_r, n * 8) == hipSuccess && hipMalloc(&d_h, n * 8) == hipSuccess &&
        hipMalloc(&d_k, n * 4) == hipSuccess && hipMalloc(&d_cnt, (size_t)ncases * 4) == hipSuccess &&
        hipMalloc(&d_or, (size_t)ncases * 8) == hipSuccess && hipMalloc(&d_oh, (size_t)ncases * 8) == hipSuccess &&
        hipMalloc(&d_ok, (size_t)ncases * 4) == hipSuccess) {
        rc = DZG_E_DEVICE;
        bool ok = hipMemcpy(d_r, r, n * 8, hipMemcpyHostToDevice) == hipSuccess &&
                  hipMemcpy(d_h, h, n * 8, hipMemcpyHostToDevice) == hipSuccess &&
                  hipMemcpy(d_k, k, n * 4, hipMemcpyHostToDevice) == hipSuccess &&
                  (form != 1 || hipMemcpy(d_cnt, count, (size_t)ncases * 4, hipMemcpyHostToDevice) == hipSuccess);
        if (ok) {
            hipLaunchKernelGGL(k_debug_cand_reduce, dim3((unsigned)ncases), dim3(form == 2 ? CH_THREADS : 64), 0,
                               nullptr, form, d_r, d_k, d_h, d_cnt, d_or, d_ok, d_oh);
            ok = hipGetLastError() == hipSuccess && hipDeviceSynchronize() == hipSuccess &&
                 hipMemcpy(out_r, d_or, (size_t)ncases * 8, hipMemcpyDeviceToHost) == hipSuccess &&
                 hipMemcpy(out_k, d_ok, (size_t)ncases * 4, hipMemcpyDeviceToHost) == hipSuccess &&
                 hipMemcpy(out_h, d_oh, (size_t)ncases * 8, hipMemcpyDeviceToHost) == hipSuccess;
        }
        if (ok) rc = 0;
    }
    hipFree(d_r);
    hipFree(d_h);
    hipFree(d_k);
    hipFree(d_cnt);
    hipFree(d_or);
    hipFree(d_oh);
    hipFree(d_ok);
    return rc;
}
