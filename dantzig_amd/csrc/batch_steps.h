// batch_steps.h -- the batched solvers' solve, cut into the steps a caller with an arena of its own
// can run one by one: wire the kernel arguments to the arena's sections, give a list of warm LPs
// their restart state, run the rounds over the first round's lists, unpack one LP's result.
// k_batch.hip (STRICT) and k_batch_fast.hip (FAST) define them and go through them themselves, so
// there is one implementation of each; k_batch_resident.hip runs them on the arena a dzg_batch
// handle keeps.  Host code only.
#pragma once

#include <array>

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

} // namespace dzg_steps
