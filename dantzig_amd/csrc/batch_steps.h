// batch_steps.h -- the batched solvers' solve, cut into the steps a caller with an arena of its own
// can run one by one: wire the kernel arguments to the arena's sections, give a list of warm LPs
// their restart state, run the rounds over the first round's lists, unpack one LP's result.
// k_batch.hip (STRICT) and k_batch_fast.hip (FAST) define them and go through them themselves, so
// there is one implementation of each; k_batch_resident.hip runs them on the arena a dzg_batch
// handle keeps.  What follows the rounds -- duals, ranging and rays of the state the LPs ended in
// (dzg_batch_solve_post) -- is cut the same way: k_batch_post.hip defines the FAST pass on an arena the
// caller describes, k_batch.hip the STRICT one.  Host code only.
#pragma once

#include <array>
#include <vector>

#include "batch_host.h"
#include "common.h"

namespace dzg_steps {

namespace bh = dzg_bh;

// ---- STRICT (k_batch.hip)

// Where a STRICT solve lies: the arena, its Layout (log and scratch sections placed), the numerics'
// own sections (byte offsets) and the knobs every launch gets.
struct StrictRun {
    unsigned char *dev = nullptr;
    const bh::Layout *L = nullptr;
    size_t status = 0; // int per LP: DZG_RUNNING before the first round
    size_t iter = 0;   // long long per LP: 0 before the first round
    size_t c = 0;      // double per variable (at vc_off): read by the restart alone
    long long max_iter = 0;
    double eps = 0.0;
    int ppl = 0;
    hipStream_t st = nullptr;
};

int strict_ppl(int64_t pivots_per_launch); // 0: the default
// The warm LPs wlist[wseg[b] .. wseg[b + 1]) of every bucket b (a device list), one workgroup each;
// mmax[b]: the largest m among them at least.  Launches only: the caller reads status[] back.
int strict_restart(const StrictRun &R, const int *wlist, const bh::Segments &wseg, const int *mmax);
// bh::run_rounds over the lists cur / nxt laid out by seg, counters at L->count; rounds as there.
int strict_rounds(const StrictRun &R, int *cur, int *nxt, const bh::Segments &seg,
                  const std::array<int, bh::kBuckets> &live, const int *mmax, int *rounds = nullptr);
// r from the downloaded state; lp gives m, n, c and constant, d the offsets and the log's cap.
void strict_unpack(const dzg_lp &lp, const DzgBatchLp &d, const bh::HostView &view, int status, long long iter,
                   dzg_result &r);

// ---- FAST (k_batch_fast.hip)

struct FastRun {
    unsigned char *dev = nullptr;
    const bh::Layout *L = nullptr;
    size_t state = 0;  // fast_state_bytes() per LP: fast_state_init's block before the first round
    size_t margin = 0; // double per log entry
    size_t rst = 0;    // int per LP: the restart's statuses, DZG_RUNNING before it
    size_t c = 0;      // double per variable: read by the restart alone
    double eps = 0.0;
    int ppl = 0, refactor_every = 0;
    hipStream_t st = nullptr;
};

int fast_ppl(int64_t pivots_per_launch);         // 0: the default
int fast_refactor_every(int64_t refactor_every); // 0: the default
size_t fast_state_bytes();
// The state block a FAST LP starts a solve with (zeros but for the control block's start).
void fast_state_init(void *block, const dzg_opts &o, long long max_iter);
int fast_restart(const FastRun &R, const int *wlist, const bh::Segments &wseg, const int *mmax);
// w_out / w_off (device): the DUMP instantiations of dzg_debug_batch_fast_inverse.
int fast_rounds(const FastRun &R, int *cur, int *nxt, const bh::Segments &seg,
                const std::array<int, bh::kBuckets> &live, const int *mmax, double *w_out = nullptr,
                const long long *w_off = nullptr, int *rounds = nullptr);
// r from the downloaded state; `block` is the LP's own state block, `margins` the whole section.
void fast_unpack(const dzg_lp &lp, const DzgBatchLp &d, const bh::HostView &view, const void *block,
                 const double *margins, dzg_result &r);
long long fast_state_iter(const void *block); // the pivots a downloaded state block counts

// ---- what follows the rounds: duals of the LPs that ended OPTIMAL, rays of
// those that ended UNBOUNDED or INFEASIBLE.  A FAST result goes through fast_post
// (k_batch_post.hip), a STRICT one through strict_post (k_batch.hip).

// Per LP: DZG_POST_SCAL doubles -- OPTIMAL: dual_obj, primal_infeas, dual_infeas, max |z - d_N|,
// max |d_N|; a ray: var (-1: find_first_pivot found none), pos, mu, value, violation -- and one int:
#define DZG_POST_SCAL 5
#define DZG_POST_NONE 0     // nothing was asked of this LP's status
#define DZG_POST_DONE 1
#define DZG_POST_SINGULAR 2 // the final basis did not invert: the LP reports nothing, its result stands

// The post-solve's own sections of an arena (byte offsets): c and rhs0 go up with the list, the
// pricing scratch stays, [y, end) comes down.  An LP has either duals or a ray, so both share y and d.
struct PostSections {
    size_t c = 0, rhs0 = 0, list = 0, dz = 0; // c by variable (vc_off), rhs0 by constraint row (m_off)
    size_t y = 0, d = 0, scal = 0, pstat = 0, end = 0;
};
void post_layout(bh::Arena &ar, PostSections &S, long long nvc, long long nm, long long nq, int N);
// ... for an arena that holds c and rhs0 already (the caller sets S.c and S.rhs0): the rest.
void post_layout_out(bh::Arena &ar, PostSections &S, long long nvc, long long nm, long long nq, int N);

// The directions of the LPs a ranging request counts for, packed for the device: an arena of its own,
// [0, up_end) goes up, [lo, top) comes down into `host`.
struct PostRanging {
    std::vector<unsigned char> host;
    size_t tol = 0, irange = 0, item = 0, eidx = 0, eval = 0, up_end = 0;
    size_t posmap = 0, lo = 0, hi = 0, lov = 0, hiv = 0, top = 0;
    std::vector<long long> out0; // call entry k's first result slot, cost directions first
    bh::Segments iseg{};         // bucket b's items: [iseg[b], iseg[b + 1])
    bool any = false;            // a listed LP has a direction: there is an arena at all
};
// req[k], k < n, belongs to LP ids[k] of the arena (ids == NULL: k) and counts where listed[k] != 0;
// P describes the arena's LPs.  Items lie by bucket (iseg), in call order within one.  The requests
// are checked already.
int post_ranging_pack(PostRanging &G, const dzg_ranging_req *req, int n, const int64_t *ids,
                      const unsigned char *listed, const bh::Packed &P);
// Entry k's ranges from G.host as downloaded; !ok: NaN ranges, *_var = -1.
void post_unpack_ranging(const PostRanging &G, int k, const dzg_ranging_req &rq, dzg_ranging &o, bool ok);

struct PostRun {
    unsigned char *dev = nullptr;
    const bh::Layout *L = nullptr;
    size_t state = 0;  // FAST's state blocks, as FastRun::state
    size_t status = 0; // STRICT's statuses, as StrictRun::status (the STRICT pass alone)
    PostSections S;
    bool duals = false, rays = false;
    const PostRanging *rg = nullptr; // with rdev, its arena on the device: ranges of the OPTIMAL LPs
    unsigned char *rdev = nullptr;
    // optional: a device allocation of the caller's for the ranging arena (and its size), kept between
    // calls so that a handle does not allocate per solve; NULL: the pass allocates and frees its own
    unsigned char **rkeep = nullptr;
    size_t *rkeep_bytes = nullptr;
    hipStream_t st = nullptr;
};
// The LPs list[seg[b] .. seg[b + 1]) of every bucket b (a device list), one workgroup each; mmax[b]:
// the largest m among them at least.  Launches only.
int fast_post(const PostRun &R, const int *list, const bh::Segments &seg, const int *mmax);
// What a pass brought down: per section the span from the first to the last listed LP and nothing
// else -- y from row m0 on, d from variable v0 on, the scalars and post statuses from LP i0 on.
struct PostDown {
    std::vector<unsigned char> buf;
    size_t o_d = 0, o_scal = 0, o_pstat = 0;
    long long m0 = 0, v0 = 0;
    int i0 = 0;
    const double *y() const { return (const double *)buf.data(); }
    const double *d() const { return (const double *)(buf.data() + o_d); }
    const double *scal() const { return (const double *)(buf.data() + o_scal); }
    const int *pstat() const { return (const int *)(buf.data() + o_pstat); }
};
// LP i's du / ry (either may be NULL) from what came down (i inside its spans); r is the LP's result.
void post_unpack(const DzgBatchLp &d, const PostDown &D, int i, const dzg_result &r, dzg_duals *du, dzg_ray *ry);
// The whole pass behind a solve whose arena lies as R says (S.c and S.rhs0 hold the costs and the
// right-hand sides by row already; duals, rays, rg and rdev are set here).  Call entry k < n is LP
// ids[k] of the arena (ids == NULL: k) with result res[k].  strict = false: the entries whose result is
// FAST's go through k_batch_fast_post; strict = true: those whose result is STRICT's go through
// k_duals_small / k_ranging_small / k_rays_small.  Entries of this pass whose status asks for something
// are listed, run and written to post's arrays at k; one that asks for nothing, or whose final basis
// did not invert, gets source = 0, kind = 0, NaN ranges.  The other numerics' entries are not touched.
// Only the listed LPs' outputs come down.  h2d / d2h / ms (optional) are added to: bytes copied, and
// the device time between two events around the launches.
int post_pass(PostRun R, bool strict, const bh::Packed &P, int n, const int64_t *ids, const dzg_result *res,
              const dzg_batch_post &post, int64_t *h2d = nullptr, int64_t *d2h = nullptr, double *ms = nullptr);
double &post_ms(); // dzg_debug_batch_post_ms: the calling thread's last post-solve launches
// The STRICT batch with a start per LP (NULL: all cold) and every post-solve it has behind it, on the
// final state, by k_duals_small / k_ranging_small / k_rays_small: du, (req, rg) and ry are optional.
int strict_post(const dzg_lp *lps, const dzg_batch_start *start, int64_t count, const dzg_opts *opts,
                int64_t pivots_per_launch, dzg_result *res, dzg_duals *du, const dzg_ranging_req *req,
                dzg_ranging *rg, dzg_ray *ry);

} // namespace dzg_steps
