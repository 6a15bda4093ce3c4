// k_batch_resident.hip -- a batch of small LPs kept on the device between solves (dzg_batch, DESIGN.md
// section 7m): the batched sibling of dzg_solver_reoptimize.  The matrices, var_col and the
// descriptors go up once, at dzg_batch_create; a dzg_batch_resolve uploads the changed right-hand
// sides and costs of the LPs it lists and nothing else, and is, result for result and bit for bit,
// the stateless dzg_batch_solve_fast_from on the same data from each LP's last basis.
//
// The arithmetic is not here: the handle runs k_batch_restart / k_batch_strict and k_batch_fast_restart
// / k_batch_fast through the steps of batch_steps.h, on an arena of its own that lives as long as the
// handle.  What is here is k_batch_stage, which does on the device what bh::fill_upload does on the
// host of a stateless call: one workgroup per listed LP, before the restart pass,
//   - scatters the LP's pending rhs / c from the compact staging buffer into the resident sections
//     (and, with a new c, the cold z = -c[nonbasis] of the create-time nonbasis);
//   - a warm LP: copies the basis it starts from (the one its last solve left in place, one handed in
//     through dzg_batch_set_start, or the saved one for AUTO's second attempt) to the start copy and to
//     the state, x[r] = rhs[r] by constraint row, xbar = zbar = 1, z = 0: what the restart kernels read;
//   - a cold LP: the create-time basis and nonbasis, x[p] = rhs[row of position p], the cold z,
//     xbar = zbar = 1;
//   - resets the per-solve state: STRICT's status / iter, the restart status, FAST's state block.
// Copies and one negation: plain stores, no atomics, nothing that rounds.
#include <algorithm>
#include <cmath>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include "batch_host.h"
#include "batch_steps.h"
#include "common.h"
#include "opts.h"
#include "ranging.h" // dzg_ranging_req_valid

namespace {

namespace bh = dzg_bh;
namespace steps = dzg_steps;

enum StageMode : int {
    STAGE_WARM = 0,   // from the basis the last solve left in the state sections
    STAGE_COLD = 1,   // from the create-time slack basis
    STAGE_HANDED = 2, // from a basis in the staging buffer (dzg_batch_set_start)
    STAGE_SAVED = 3,  // from the start copy (AUTO's second attempt)
};

// One listed LP of a solve.  Offsets into the staging buffer's doubles / ints, -1: nothing pending.
struct StageItem {
    long long rhs_off, c_off, start_off;
    int id, mode;
};

struct StageArgs {
    const DzgBatchLp *lp;
    const int *var_col;
    int *basis, *nonbasis;
    double *x, *xbar, *z, *zbar;
    double *rhs, *c;                  // resident: by constraint row (at m_off), by variable (at vc_off)
    const int *basis0, *nonbasis0;    // the create-time basis: the cold start and the position -> row map
    double *z0;                       // the cold z
    int *sbasis, *snonbasis;          // the basis the current solve started from
    int *status;                      // STRICT
    long long *iter;
    int *rst;                         // FAST: the restart's status
    int *fstate;                      // FAST: state blocks of fstate_words ints each
    const int *fstate0;               // ... and the block a solve starts with
    int fstate_words;
    const double *stg_d;
    const int *stg_i;
};

constexpr int kStageBlock = 256;

__global__ __launch_bounds__(kStageBlock) void k_batch_stage(StageArgs g, const StageItem *__restrict__ items)
{
    const StageItem it = items[blockIdx.x];
    const DzgBatchLp L = g.lp[it.id];
    const int m = L.m, n = L.n, q = L.n - L.m;
    const int tid = threadIdx.x;
    const int *var_col = g.var_col + L.vc_off;
    const int *basis0 = g.basis0 + L.m_off, *nonbasis0 = g.nonbasis0 + L.q_off;
    double *rhs = g.rhs + L.m_off, *c = g.c + L.vc_off, *z0 = g.z0 + L.q_off;
    int *basis = g.basis + L.m_off, *nonbasis = g.nonbasis + L.q_off;
    int *sbasis = g.sbasis + L.m_off, *snonbasis = g.snonbasis + L.q_off;
    double *x = g.x + L.m_off, *xbar = g.xbar + L.m_off, *z = g.z + L.q_off, *zbar = g.zbar + L.q_off;
    const double *new_rhs = it.rhs_off >= 0 ? g.stg_d + it.rhs_off : nullptr;
    const double *new_c = it.c_off >= 0 ? g.stg_d + it.c_off : nullptr;
    // what this solve reads is read from where it was written by the host, not from the section a
    // neighbouring thread is filling
    const double *rhs_now = new_rhs ? new_rhs : rhs;

    if (new_rhs)
        for (int r = tid; r < m; r += kStageBlock) rhs[r] = new_rhs[r];
    if (new_c) {
        for (int v = tid; v < n; v += kStageBlock) c[v] = new_c[v];
        for (int k = tid; k < q; k += kStageBlock) z0[k] = -new_c[nonbasis0[k]];
    }
    if (it.mode == STAGE_COLD) {
        for (int p = tid; p < m; p += kStageBlock) {
            const int v = basis0[p];
            basis[p] = v;
            x[p] = rhs_now[-1 - var_col[v]];
            xbar[p] = 1.0;
        }
        for (int k = tid; k < q; k += kStageBlock) {
            const int v = nonbasis0[k];
            nonbasis[k] = v;
            z[k] = new_c ? -new_c[v] : z0[k];
            zbar[k] = 1.0;
        }
    } else {
        const int *from_b = it.mode == STAGE_HANDED ? g.stg_i + it.start_off : it.mode == STAGE_SAVED ? sbasis : basis;
        const int *from_n = it.mode == STAGE_HANDED ? g.stg_i + it.start_off + m
                          : it.mode == STAGE_SAVED  ? snonbasis
                                                    : nonbasis;
        for (int p = tid; p < m; p += kStageBlock) {
            const int v = from_b[p];
            sbasis[p] = v;
            basis[p] = v;
            x[p] = rhs_now[p];
            xbar[p] = 1.0;
        }
        for (int k = tid; k < q; k += kStageBlock) {
            const int v = from_n[k];
            snonbasis[k] = v;
            nonbasis[k] = v;
            z[k] = 0.0; // the restart kernel's to write
            zbar[k] = 1.0;
        }
    }
    if (tid == 0) {
        g.status[it.id] = DZG_RUNNING;
        g.iter[it.id] = 0;
        g.rst[it.id] = DZG_RUNNING;
    }
    int *fs = g.fstate + (long long)it.id * g.fstate_words;
    for (int w = tid; w < g.fstate_words; w += kStageBlock) fs[w] = g.fstate0[w];
}

} // namespace

struct dzg_batch {
    int N = 0;
    int device = 0;
    bool failed = false;
    dzg_opts o;             // as given (near_tie_action forced to STOP under AUTO)
    bool strict = false, is_auto = false;
    long long max_iter = 0;
    int64_t ppl_arg = 0, refactor_arg = 0;

    // ---- host: each LP's data now, and where it starts its next solve
    bh::Packed P;
    std::vector<dzg_lp> lp;                // m, n, n_struct, c, constant, var_col, basis, nonbasis: own storage
    std::vector<double> c, rhs;            // by variable (vc_off), by constraint row (m_off)
    std::vector<int64_t> var_col, basis0, nonbasis0;
    std::vector<int> start_b, start_n;     // a handed-in start (m_off, q_off), valid where handed[i]
    std::vector<char> cold, handed, dirty_rhs, dirty_c;

    // ---- device
    hipStream_t st = nullptr;
    hipEvent_t e0 = nullptr, e1 = nullptr;
    unsigned char *arena = nullptr;
    bh::Layout *L = nullptr;
    size_t s_status = 0, s_iter = 0, s_fstate = 0, s_rst = 0, s_lmg = 0;
    size_t s_c = 0, s_rhs = 0, s_basis0 = 0, s_nonbasis0 = 0, s_z0 = 0, s_sbasis = 0, s_snonbasis = 0, s_fstate0 = 0;
    size_t s_items = 0, s_list = 0, s_wlist = 0, s_sd = 0, s_si = 0, s_end = 0; // the staging buffer
    size_t fstate_bytes = 0;
    dzg_steps::PostSections post; // dzg_batch_resolve_post: c and rhs0 are the resident sections
    unsigned char *rarena = nullptr; // ... and its ranging arena, made at the first use, grown when needed
    size_t rarena_bytes = 0;
    unsigned char *stage = nullptr;  // pinned: the staging buffer as it goes up, offsets from s_items
    unsigned char *mirror = nullptr; // pinned: the state sections [state0, upload_end) as they come down
    int *h_lk = nullptr, *h_le = nullptr, *h_ll = nullptr; // the log as it comes down (made at the first use)
    double *h_lmu = nullptr, *h_lmg = nullptr;

    // ---- dzg_debug_batch_traffic
    int64_t h2d = 0, d2h = 0;
    double ms = 0.0;

    ~dzg_batch()
    {
        if (arena || st || rarena) (void)hipSetDevice(device);
        if (arena) (void)hipFree(arena);
        if (rarena) (void)hipFree(rarena);
        if (stage) (void)hipHostFree(stage);
        if (mirror) (void)hipHostFree(mirror);
        if (e0) (void)hipEventDestroy(e0);
        if (e1) (void)hipEventDestroy(e1);
        if (st) (void)hipStreamDestroy(st);
        std::free(h_lk);
        std::free(h_le);
        std::free(h_ll);
        std::free(h_lmu);
        std::free(h_lmg);
        delete L;
    }
};

namespace {

int up(dzg_batch *b, size_t dst, const void *src, size_t bytes)
{
    if (bytes == 0) return 0;
    DZG_HIP(hipMemcpyAsync(b->arena + dst, src, bytes, hipMemcpyHostToDevice, b->st));
    b->h2d += (int64_t)bytes;
    return 0;
}

int down(dzg_batch *b, void *dst, size_t src, size_t bytes)
{
    if (bytes == 0) return 0;
    DZG_HIP(hipMemcpyAsync(dst, b->arena + src, bytes, hipMemcpyDeviceToHost, b->st));
    b->d2h += (int64_t)bytes;
    return 0;
}

// The host's view of the downloaded state: the mirror holds [state0, upload_end) at its own offsets.
unsigned char *mirror_base(const dzg_batch *b) { return b->mirror - b->L->state0; }

int create_device(dzg_batch *b, const dzg_lp *lps)
{
    const int N = b->N;
    const bh::Packed &P = b->P;
    bh::Layout &L = *b->L;
    b->fstate_bytes = steps::fast_state_bytes();
    b->s_status = L.ar.add(sizeof(int) * N);
    b->s_iter = L.ar.add(sizeof(long long) * N);
    b->s_fstate = L.ar.add(b->fstate_bytes * N);
    b->s_rst = L.ar.add(sizeof(int) * N);
    L.end_upload();
    b->s_lmg = L.ar.add(sizeof(double) * P.nlog);
    L.end_download();
    b->s_c = L.ar.add(sizeof(double) * P.nvc);
    b->s_rhs = L.ar.add(sizeof(double) * P.nm);
    b->s_basis0 = L.ar.add(sizeof(int) * P.nm);
    b->s_nonbasis0 = L.ar.add(sizeof(int) * P.nq);
    b->s_z0 = L.ar.add(sizeof(double) * P.nq);
    b->s_sbasis = L.ar.add(sizeof(int) * P.nm);
    b->s_snonbasis = L.ar.add(sizeof(int) * P.nq);
    b->s_fstate0 = L.ar.add(b->fstate_bytes);
    b->s_items = L.ar.add(sizeof(StageItem) * N);
    b->s_list = L.ar.add(sizeof(int) * N);
    b->s_wlist = L.ar.add(sizeof(int) * N);
    b->s_sd = L.ar.add(sizeof(double) * (P.nm + P.nvc));
    b->s_si = L.ar.add(sizeof(int) * (P.nm + P.nq));
    b->s_end = L.ar.top;
    b->post.c = b->s_c;
    b->post.rhs0 = b->s_rhs;
    steps::post_layout_out(L.ar, b->post, P.nvc, P.nm, P.nq, N);

    DZG_HIP(hipStreamCreateWithFlags(&b->st, hipStreamNonBlocking));
    DZG_HIP(hipEventCreate(&b->e0));
    DZG_HIP(hipEventCreate(&b->e1));
    DZG_HIP(hipMalloc((void **)&b->arena, L.ar.top));
    DZG_HIP(hipHostMalloc((void **)&b->stage, b->s_end - b->s_items, hipHostMallocDefault));
    DZG_HIP(hipHostMalloc((void **)&b->mirror, std::max<size_t>(L.upload_end - L.state0, 16), hipHostMallocDefault));

    // once: the descriptors, A, var_col (and the cold state, which every solve stages afresh)
    std::vector<unsigned char> host(L.upload_end, 0);
    bh::fill_upload(host.data(), L, P, lps);
    DZG_HIP(hipMemcpyAsync(b->arena, host.data(), L.upload_end, hipMemcpyHostToDevice, b->st));
    // ... and the resident data behind the solve's sections
    std::vector<unsigned char> more(b->s_items - b->s_c, 0);
    auto at = [&](size_t s) { return more.data() + (s - b->s_c); };
    std::memcpy(at(b->s_c), b->c.data(), sizeof(double) * b->c.size());
    std::memcpy(at(b->s_rhs), b->rhs.data(), sizeof(double) * b->rhs.size());
    int *b0 = (int *)at(b->s_basis0), *n0 = (int *)at(b->s_nonbasis0);
    double *z0 = (double *)at(b->s_z0);
    for (size_t k = 0; k < b->basis0.size(); ++k) b0[k] = (int)b->basis0[k];
    for (size_t k = 0; k < b->nonbasis0.size(); ++k) n0[k] = (int)b->nonbasis0[k];
    for (int i = 0; i < N; ++i)
        for (int64_t k = 0; k < lps[i].n - lps[i].m; ++k) z0[P.desc[(size_t)i].q_off + k] = lps[i].z[k];
    steps::fast_state_init(at(b->s_fstate0), b->o, b->max_iter);
    DZG_HIP(hipMemcpyAsync(b->arena + b->s_c, more.data(), more.size(), hipMemcpyHostToDevice, b->st));
    DZG_HIP(hipStreamSynchronize(b->st));
    return 0;
}

StageArgs stage_args(const dzg_batch *b)
{
    unsigned char *dev = b->arena;
    const bh::Layout &L = *b->L;
    StageArgs g;
    g.lp = (const DzgBatchLp *)(dev + L.desc);
    g.var_col = (const int *)(dev + L.vc);
    g.basis = (int *)(dev + L.basis);
    g.nonbasis = (int *)(dev + L.nonbasis);
    g.x = (double *)(dev + L.x);
    g.xbar = (double *)(dev + L.xbar);
    g.z = (double *)(dev + L.z);
    g.zbar = (double *)(dev + L.zbar);
    g.rhs = (double *)(dev + b->s_rhs);
    g.c = (double *)(dev + b->s_c);
    g.basis0 = (const int *)(dev + b->s_basis0);
    g.nonbasis0 = (const int *)(dev + b->s_nonbasis0);
    g.z0 = (double *)(dev + b->s_z0);
    g.sbasis = (int *)(dev + b->s_sbasis);
    g.snonbasis = (int *)(dev + b->s_snonbasis);
    g.status = (int *)(dev + b->s_status);
    g.iter = (long long *)(dev + b->s_iter);
    g.rst = (int *)(dev + b->s_rst);
    g.fstate = (int *)(dev + b->s_fstate);
    g.fstate0 = (const int *)(dev + b->s_fstate0);
    g.fstate_words = (int)(b->fstate_bytes / sizeof(int));
    g.stg_d = (const double *)(dev + b->s_sd);
    g.stg_i = (const int *)(dev + b->s_si);
    return g;
}

steps::StrictRun strict_run(const dzg_batch *b, int64_t ppl_arg)
{
    steps::StrictRun R;
    R.dev = b->arena;
    R.L = b->L;
    R.status = b->s_status;
    R.iter = b->s_iter;
    R.c = b->s_c;
    R.max_iter = b->max_iter;
    R.eps = dzg_opts_resolved(&b->o).epsilon;
    R.ppl = steps::strict_ppl(ppl_arg);
    R.st = b->st;
    return R;
}

steps::FastRun fast_run(const dzg_batch *b)
{
    steps::FastRun R;
    R.dev = b->arena;
    R.L = b->L;
    R.state = b->s_fstate;
    R.margin = b->s_lmg;
    R.rst = b->s_rst;
    R.c = b->s_c;
    R.eps = dzg_opts_resolved(&b->o).epsilon;
    R.ppl = steps::fast_ppl(b->ppl_arg);
    R.refactor_every = steps::fast_refactor_every(b->refactor_arg);
    R.st = b->st;
    return R;
}

// The log's cap for res: the stateless call's rule (pack) under the handle's own cap.
long long log_cap_of(const DzgBatchLp &d, const dzg_result &r)
{
    return r.log && r.log_cap > 0 ? std::min<long long>(r.log_cap, d.log_cap) : 0;
}

// The log entries [0, cnt) of the LPs ids[k] come down: neighbouring ranges in one copy per section.
int download_logs(dzg_batch *b, const std::vector<int> &ids, const std::vector<long long> &cnt, bool fast)
{
    const bh::Layout &L = *b->L;
    std::vector<std::pair<long long, long long>> ranges; // [first, last) in log entries
    std::vector<size_t> order(ids.size());
    for (size_t k = 0; k < ids.size(); ++k) order[k] = k;
    std::sort(order.begin(), order.end(), [&](size_t a, size_t c) { return ids[a] < ids[c]; });
    const long long kGap = 4096; // entries between two ranges that are cheaper to copy than to skip
    for (size_t k : order) {
        if (cnt[k] <= 0) continue;
        const long long lo = b->P.desc[(size_t)ids[k]].log_off, hi = lo + cnt[k];
        if (!ranges.empty() && lo - ranges.back().second <= kGap) ranges.back().second = hi;
        else ranges.push_back({lo, hi});
    }
    if (ranges.empty()) return 0;
    if (!b->h_lk) {
        const size_t nlog = (size_t)std::max<long long>(b->P.nlog, 1);
        b->h_lk = (int *)std::calloc(nlog, sizeof(int));
        b->h_le = (int *)std::calloc(nlog, sizeof(int));
        b->h_ll = (int *)std::calloc(nlog, sizeof(int));
        b->h_lmu = (double *)std::calloc(nlog, sizeof(double));
        b->h_lmg = (double *)std::calloc(nlog, sizeof(double));
        if (!b->h_lk || !b->h_le || !b->h_ll || !b->h_lmu || !b->h_lmg)
            return dzg_set_error(DZG_E_DEVICE, "batch: out of host memory for the log");
    }
    for (const auto &r : ranges) {
        const size_t at = (size_t)r.first, len = (size_t)(r.second - r.first);
        if (const int rc = down(b, b->h_lk + at, L.lk + sizeof(int) * at, sizeof(int) * len)) return rc;
        if (const int rc = down(b, b->h_le + at, L.le + sizeof(int) * at, sizeof(int) * len)) return rc;
        if (const int rc = down(b, b->h_ll + at, L.ll + sizeof(int) * at, sizeof(int) * len)) return rc;
        if (const int rc = down(b, b->h_lmu + at, L.lmu + sizeof(double) * at, sizeof(double) * len)) return rc;
        if (fast)
            if (const int rc = down(b, b->h_lmg + at, b->s_lmg + sizeof(double) * at, sizeof(double) * len)) return rc;
    }
    DZG_HIP(hipStreamSynchronize(b->st));
    return 0;
}

// One pass over the LPs ids[k] (distinct, in range), each staged as mode[k] says: stage, restart,
// rounds, download, res[slot[k]].  with_updates: the pending rhs / c of these LPs go up.
int run_pass(dzg_batch *b, const std::vector<int> &ids, const std::vector<int> &mode, const std::vector<int64_t> &slot,
             bool with_updates, bool fast, int64_t strict_ppl_arg, dzg_result *res)
{
    const int n = (int)ids.size();
    const bh::Layout &L = *b->L;
    const bh::Packed &P = b->P;
    unsigned char *dev = b->arena;
    StageItem *items = (StageItem *)b->stage;
    int *list = (int *)(b->stage + (b->s_list - b->s_items));
    int *wlist = (int *)(b->stage + (b->s_wlist - b->s_items));
    double *sd = (double *)(b->stage + (b->s_sd - b->s_items));
    int *si = (int *)(b->stage + (b->s_si - b->s_items));

    // ---- the staging buffer: items, the first round's lists and the warm lists by bucket, the data
    int bucket_n[bh::kBuckets] = {0, 0, 0, 0}, warm_n[bh::kBuckets] = {0, 0, 0, 0};
    int mmax[bh::kBuckets] = {0, 0, 0, 0};
    long long nd = 0, ni = 0;
    for (int k = 0; k < n; ++k) {
        const int i = ids[k];
        const DzgBatchLp &d = P.desc[(size_t)i];
        const int bk = bh::bucket_of(d.m);
        bucket_n[bk]++;
        if (mode[k] != STAGE_COLD) warm_n[bk]++;
        mmax[bk] = std::max(mmax[bk], d.m);
        StageItem &it = items[k];
        it.id = i;
        it.mode = mode[k];
        it.rhs_off = it.c_off = it.start_off = -1;
        if (with_updates && b->dirty_rhs[(size_t)i]) {
            it.rhs_off = nd;
            std::memcpy(sd + nd, b->rhs.data() + d.m_off, sizeof(double) * (size_t)d.m);
            nd += d.m;
        }
        if (with_updates && b->dirty_c[(size_t)i]) {
            it.c_off = nd;
            std::memcpy(sd + nd, b->c.data() + d.vc_off, sizeof(double) * (size_t)d.n);
            nd += d.n;
        }
        if (mode[k] == STAGE_HANDED) {
            it.start_off = ni;
            std::memcpy(si + ni, b->start_b.data() + d.m_off, sizeof(int) * (size_t)d.m);
            std::memcpy(si + ni + d.m, b->start_n.data() + d.q_off, sizeof(int) * (size_t)(d.n - d.m));
            ni += d.n;
        }
    }
    const bh::Segments seg = bh::segments(bucket_n), wseg = bh::segments(warm_n);
    bh::Segments fill = seg, wfill = wseg;
    for (int k = 0; k < n; ++k) {
        const int bk = bh::bucket_of(P.desc[(size_t)ids[k]].m);
        list[fill[(size_t)bk]++] = ids[k];
        if (mode[k] != STAGE_COLD) wlist[wfill[(size_t)bk]++] = ids[k];
    }
    const int nwarm = wseg[bh::kBuckets];
    if (const int rc = up(b, b->s_items, items, sizeof(StageItem) * (size_t)n)) return rc;
    if (const int rc = up(b, b->s_list, list, sizeof(int) * (size_t)n)) return rc;
    if (const int rc = up(b, b->s_wlist, wlist, sizeof(int) * (size_t)nwarm)) return rc;
    if (const int rc = up(b, b->s_sd, sd, sizeof(double) * (size_t)nd)) return rc;
    if (const int rc = up(b, b->s_si, si, sizeof(int) * (size_t)ni)) return rc;

    // ---- stage, then the restart state of the warm LPs
    const steps::StrictRun RS = strict_run(b, strict_ppl_arg);
    const steps::FastRun RF = fast_run(b);
    DZG_HIP(hipEventRecord(b->e0, b->st));
    hipLaunchKernelGGL(k_batch_stage, dim3(n), dim3(kStageBlock), 0, b->st, stage_args(b),
                       (const StageItem *)(dev + b->s_items));
    DZG_HIP(hipGetLastError());
    if (nwarm > 0) {
        const int *dw = (const int *)(dev + b->s_wlist);
        if (const int rc = fast ? steps::fast_restart(RF, dw, wseg, mmax) : steps::strict_restart(RS, dw, wseg, mmax))
            return rc;
    }
    DZG_HIP(hipEventRecord(b->e1, b->st));
    const int lo = *std::min_element(ids.begin(), ids.end()), hi = *std::max_element(ids.begin(), ids.end());
    unsigned char *mb = mirror_base(b);
    std::array<int, bh::kBuckets> live = bh::live_of(bucket_n);
    if (nwarm > 0) { // a singular start leaves the first round's lists
        const size_t s_st = fast ? b->s_rst : b->s_status;
        if (const int rc = down(b, mb + s_st + sizeof(int) * (size_t)lo, s_st + sizeof(int) * (size_t)lo,
                                sizeof(int) * (size_t)(hi - lo + 1)))
            return rc;
        DZG_HIP(hipStreamSynchronize(b->st));
        const int *status = (const int *)(mb + s_st);
        bool gone = false;
        for (int k = 0; k < nwarm; ++k) gone = gone || status[wlist[k]] != DZG_RUNNING;
        if (gone) {
            for (int bk = 0; bk < bh::kBuckets; ++bk) {
                int kept = 0;
                for (int k = seg[(size_t)bk]; k < seg[(size_t)bk + 1]; ++k)
                    if (status[list[k]] == DZG_RUNNING) list[seg[(size_t)bk] + kept++] = list[k];
                live[(size_t)bk] = kept;
            }
            if (const int rc = up(b, b->s_list, list, sizeof(int) * (size_t)n)) return rc;
        }
    }

    // ---- the rounds
    int rounds = 0;
    int *cur = (int *)(dev + b->s_list), *nxt = (int *)(dev + L.list2);
    const int rc_rounds = fast ? steps::fast_rounds(RF, cur, nxt, seg, live, mmax, nullptr, nullptr, &rounds)
                               : steps::strict_rounds(RS, cur, nxt, seg, live, mmax, &rounds);
    if (rc_rounds) return rc_rounds;
    b->d2h += (int64_t)sizeof(int) * bh::kBuckets * rounds;

    // ---- the listed LPs' state comes down: per section the span from the first to the last of them
    const DzgBatchLp &dl = P.desc[(size_t)lo], &dh = P.desc[(size_t)hi];
    const size_t m0 = (size_t)dl.m_off, m1 = (size_t)(dh.m_off + dh.m), q0 = (size_t)dl.q_off,
                 q1 = (size_t)(dh.q_off + dh.n - dh.m), i0 = (size_t)lo, i1 = (size_t)hi + 1;
    auto span = [&](size_t sec, size_t elem, size_t first, size_t last) {
        return down(b, mb + sec + elem * first, sec + elem * first, elem * (last - first));
    };
    if (const int rc = span(L.basis, sizeof(int), m0, m1)) return rc;
    if (const int rc = span(L.nonbasis, sizeof(int), q0, q1)) return rc;
    if (const int rc = span(L.x, sizeof(double), m0, m1)) return rc;
    if (const int rc = span(L.xbar, sizeof(double), m0, m1)) return rc;
    if (const int rc = span(L.z, sizeof(double), q0, q1)) return rc;
    if (const int rc = span(L.zbar, sizeof(double), q0, q1)) return rc;
    if (fast) {
        if (const int rc = span(b->s_fstate, b->fstate_bytes, i0, i1)) return rc;
    } else {
        if (const int rc = span(b->s_status, sizeof(int), i0, i1)) return rc;
        if (const int rc = span(b->s_iter, sizeof(long long), i0, i1)) return rc;
    }
    DZG_HIP(hipStreamSynchronize(b->st));
    float ms = 0.0f;
    DZG_HIP(hipEventElapsedTime(&ms, b->e0, b->e1));
    b->ms += ms;

    // ---- the log of the pivots each of them took, as far as its result has room
    const int *st_h = (const int *)(mb + b->s_status);
    const long long *it_h = (const long long *)(mb + b->s_iter);
    const unsigned char *fs_h = mb + b->s_fstate;
    std::vector<long long> cnt((size_t)n);
    for (int k = 0; k < n; ++k) {
        const int i = ids[k];
        const long long iters = fast ? steps::fast_state_iter(fs_h + b->fstate_bytes * (size_t)i) : it_h[i];
        cnt[(size_t)k] = std::min(iters, log_cap_of(P.desc[(size_t)i], res[slot[(size_t)k]]));
    }
    if (const int rc = download_logs(b, ids, cnt, fast)) return rc;

    // ---- results
    bh::HostView view(mb, L);
    view.lk = b->h_lk;
    view.le = b->h_le;
    view.ll = b->h_ll;
    view.lmu = b->h_lmu;
    for (int k = 0; k < n; ++k) {
        const int i = ids[k];
        dzg_result &r = res[slot[(size_t)k]];
        DzgBatchLp d = P.desc[(size_t)i];
        d.log_cap = log_cap_of(d, r);
        if (fast)
            steps::fast_unpack(b->lp[(size_t)i], d, view, fs_h + b->fstate_bytes * (size_t)i, b->h_lmg, r);
        else
            steps::strict_unpack(b->lp[(size_t)i], d, view, st_h[i], it_h[i], r);
    }
    return 0;
}

int resolve(dzg_batch *b, const std::vector<int> &ids, dzg_result *res)
{
    const int n = (int)ids.size();
    DZG_HIP(hipSetDevice(b->device));
    std::vector<int> mode((size_t)n);
    std::vector<int64_t> slot((size_t)n);
    for (int k = 0; k < n; ++k) {
        const size_t i = (size_t)ids[k];
        mode[(size_t)k] = b->cold[i] ? STAGE_COLD : b->handed[i] ? STAGE_HANDED : STAGE_WARM;
        slot[(size_t)k] = k;
    }
    if (const int rc = run_pass(b, ids, mode, slot, true, !b->strict, b->ppl_arg, res)) return rc;
    for (int i : ids) b->dirty_rhs[(size_t)i] = b->dirty_c[(size_t)i] = 0; // they are resident now
    if (b->is_auto) {
        // only the reference's own arithmetic can arbitrate a tie: the LPs FAST gave up on run again
        // in STRICT numerics on the same arena, each from the start it had (a cold one cold)
        std::vector<int> ids2, mode2;
        std::vector<int64_t> slot2;
        for (int k = 0; k < n; ++k) {
            const int s = res[k].status;
            if (s != DZG_NEAR_TIE && s != DZG_SINGULAR && s != DZG_PANIC) continue;
            ids2.push_back(ids[k]);
            mode2.push_back(mode[(size_t)k] == STAGE_COLD ? STAGE_COLD : STAGE_SAVED);
            slot2.push_back(k);
        }
        if (!ids2.empty())
            if (const int rc = run_pass(b, ids2, mode2, slot2, false, false, 0, res)) return rc;
    }
    for (int k = 0; k < n; ++k) { // where each of them starts its next solve
        const size_t i = (size_t)ids[k];
        b->cold[i] = res[k].status == DZG_SINGULAR || res[k].status == DZG_PANIC;
        b->handed[i] = 0;
    }
    return 0;
}

int fail_if_device(dzg_batch *b, int rc)
{
    if (rc == DZG_E_DEVICE) b->failed = true;
    return rc;
}

int usable(const dzg_batch *b, const char *call)
{
    if (!b) return dzg_set_error(DZG_E_ARG, std::string(call) + ": the handle is NULL");
    if (b->failed)
        return dzg_set_error(DZG_E_DEVICE, std::string(call) + ": the handle failed in an earlier call (destroy it)");
    return 0;
}

} // namespace

extern "C" int dzg_batch_create(const dzg_lp *lps, int64_t count, const dzg_opts *opts, int64_t pivots_per_launch,
                                int64_t refactor_every, int64_t log_cap, dzg_batch **out)
{
    // ---- host checks first: malformed input is DZG_E_ARG on any machine
    if (!out) return dzg_set_error(DZG_E_ARG, "batch: out is NULL");
    *out = nullptr;
    if (count < 0) return dzg_set_error(DZG_E_ARG, "batch: count < 0");
    if (count > 0 && !lps) return dzg_set_error(DZG_E_ARG, "batch: lps is NULL");
    if (count >= (1ll << 31)) return dzg_set_error(DZG_E_ARG, "batch: count out of range");
    if (pivots_per_launch < 0) return dzg_set_error(DZG_E_ARG, "batch: pivots_per_launch < 0");
    if (refactor_every < 0) return dzg_set_error(DZG_E_ARG, "batch: refactor_every < 0");
    if (log_cap < 0) return dzg_set_error(DZG_E_ARG, "batch: log_cap < 0");
    dzg_opts o;
    if (opts) o = *opts; else dzg_opts_default(&o);
    if (o.numerics != DZG_NUMERICS_STRICT && o.numerics != DZG_NUMERICS_FAST && o.numerics != DZG_NUMERICS_AUTO)
        return dzg_set_error(DZG_E_ARG, "batch: opts.numerics");
    const int rc_lps = bh::check_batch(lps, count, [&](int64_t i, std::string &why) {
        const dzg_lp &lp = lps[i];
        if (lp.xbar || lp.zbar) {
            why = "xbar / zbar given: a resident LP is handed over in slack-basis form";
            return false;
        }
        const dzg_batch_start own = {lp.basis, lp.nonbasis};
        return bh::start_valid(lp, own, why);
    });
    if (rc_lps) return rc_lps;

    dzg_batch *b = new dzg_batch();
    b->N = (int)count;
    b->device = o.device;
    b->strict = o.numerics == DZG_NUMERICS_STRICT;
    b->is_auto = o.numerics == DZG_NUMERICS_AUTO;
    if (b->is_auto) o.near_tie_action = DZG_NEAR_TIE_STOP;
    b->o = o;
    b->max_iter = dzg_opts_resolved(&o).max_iter;
    b->ppl_arg = pivots_per_launch;
    b->refactor_arg = refactor_every;
    const int N = b->N;
    std::vector<dzg_result> caps((size_t)N); // pack reads the log's cap from a result
    dzg_pivot some;
    for (dzg_result &r : caps) {
        std::memset(&r, 0, sizeof(r));
        r.log = &some;
        r.log_cap = log_cap;
    }
    b->P = bh::pack(lps, caps.data(), N, b->max_iter);
    const bh::Packed &P = b->P;
    b->c.assign((size_t)P.nvc, 0.0);
    b->rhs.assign((size_t)P.nm, 0.0);
    b->var_col.assign((size_t)P.nvc, 0);
    b->basis0.assign((size_t)P.nm, 0);
    b->nonbasis0.assign((size_t)P.nq, 0);
    b->start_b.assign((size_t)P.nm, 0);
    b->start_n.assign((size_t)P.nq, 0);
    b->cold.assign((size_t)N, 1);
    b->handed.assign((size_t)N, 0);
    b->dirty_rhs.assign((size_t)N, 0);
    b->dirty_c.assign((size_t)N, 0);
    b->lp.resize((size_t)N);
    for (int i = 0; i < N; ++i) {
        const dzg_lp &lp = lps[i];
        const DzgBatchLp &d = P.desc[(size_t)i];
        for (int64_t v = 0; v < lp.n; ++v) {
            b->c[(size_t)(d.vc_off + v)] = lp.c[v];
            b->var_col[(size_t)(d.vc_off + v)] = bh::var_code(lp, v);
        }
        for (int64_t p = 0; p < lp.m; ++p) {
            b->basis0[(size_t)(d.m_off + p)] = lp.basis[p];
            b->rhs[(size_t)(d.m_off + (-1 - bh::var_code(lp, lp.basis[p])))] = lp.x[p];
        }
        for (int64_t k = 0; k < lp.n - lp.m; ++k) b->nonbasis0[(size_t)(d.q_off + k)] = lp.nonbasis[k];
        dzg_lp &own = b->lp[(size_t)i];
        std::memset(&own, 0, sizeof(own));
        own.m = lp.m;
        own.n = lp.n;
        own.n_struct = lp.n_struct;
        own.lda = lp.lda;
        own.constant = lp.constant;
        own.c = b->c.data() + d.vc_off;
        own.var_col = b->var_col.data() + d.vc_off;
        own.basis = b->basis0.data() + d.m_off;
        own.nonbasis = b->nonbasis0.data() + d.q_off;
    }
    b->L = new bh::Layout(P);
    if (N > 0) {
        int rc = bh::use_device(o.device);
        if (rc == 0) rc = create_device(b, lps);
        if (rc) {
            delete b;
            return rc;
        }
    }
    *out = b;
    return 0;
}

extern "C" void dzg_batch_destroy(dzg_batch *b) { delete b; }

extern "C" int dzg_batch_update(dzg_batch *b, const dzg_batch_change *chg, int64_t nchg)
{
    if (const int rc = usable(b, "dzg_batch_update")) return rc;
    if (nchg < 0) return dzg_set_error(DZG_E_ARG, "dzg_batch_update: nchg < 0");
    if (nchg > 0 && !chg) return dzg_set_error(DZG_E_ARG, "dzg_batch_update: chg is NULL");
    std::vector<char> seen((size_t)b->N, 0);
    for (int64_t k = 0; k < nchg; ++k) {
        const dzg_batch_change &ch = chg[k];
        const std::string at = "dzg_batch_update: chg[" + std::to_string(k) + "]: ";
        if (ch.lp < 0 || ch.lp >= b->N)
            return dzg_set_error(DZG_E_ARG, at + "lp " + std::to_string(ch.lp) + " out of range");
        if (seen[(size_t)ch.lp]) return dzg_set_error(DZG_E_ARG, at + "lp " + std::to_string(ch.lp) + " listed twice");
        seen[(size_t)ch.lp] = 1;
        if (!ch.rhs && !ch.c && !ch.set_constant) return dzg_set_error(DZG_E_ARG, at + "no rhs, no c, no constant");
        const dzg_lp &lp = b->lp[(size_t)ch.lp];
        for (int64_t r = 0; ch.rhs && r < lp.m; ++r)
            if (!std::isfinite(ch.rhs[r]))
                return dzg_set_error(DZG_E_ARG, at + "rhs[" + std::to_string(r) + "] is not finite");
        for (int64_t v = 0; ch.c && v < lp.n; ++v)
            if (!std::isfinite(ch.c[v])) return dzg_set_error(DZG_E_ARG, at + "c[" + std::to_string(v) + "] is not finite");
        if (ch.set_constant && !std::isfinite(ch.constant)) return dzg_set_error(DZG_E_ARG, at + "constant is not finite");
    }
    for (int64_t k = 0; k < nchg; ++k) {
        const dzg_batch_change &ch = chg[k];
        const size_t i = (size_t)ch.lp;
        const DzgBatchLp &d = b->P.desc[i];
        if (ch.rhs) {
            std::memcpy(b->rhs.data() + d.m_off, ch.rhs, sizeof(double) * (size_t)d.m);
            b->dirty_rhs[i] = 1;
        }
        if (ch.c) {
            std::memcpy(b->c.data() + d.vc_off, ch.c, sizeof(double) * (size_t)d.n);
            b->dirty_c[i] = 1;
        }
        if (ch.set_constant) b->lp[i].constant = ch.constant;
    }
    return 0;
}

extern "C" int dzg_batch_set_start(dzg_batch *b, int64_t lp, const int64_t *basis, const int64_t *nonbasis)
{
    if (const int rc = usable(b, "dzg_batch_set_start")) return rc;
    if (lp < 0 || lp >= b->N)
        return dzg_set_error(DZG_E_ARG, "dzg_batch_set_start: lp " + std::to_string(lp) + " out of range");
    const size_t i = (size_t)lp;
    if (!basis) {
        b->cold[i] = 1;
        b->handed[i] = 0;
        return 0;
    }
    std::string why;
    const dzg_batch_start s = {basis, nonbasis};
    if (!bh::start_valid(b->lp[i], s, why))
        return dzg_set_error(DZG_E_ARG, "dzg_batch_set_start: lp " + std::to_string(lp) + ": " + why);
    const DzgBatchLp &d = b->P.desc[i];
    for (int p = 0; p < d.m; ++p) b->start_b[(size_t)(d.m_off + p)] = (int)basis[p];
    for (int k = 0; k < d.n - d.m; ++k) b->start_n[(size_t)(d.q_off + k)] = (int)nonbasis[k];
    b->cold[i] = 0;
    b->handed[i] = 1;
    return 0;
}

// dzg_batch_resolve, and behind it what `post` (NULL or empty: nothing) asks for.
static int resolve_post(dzg_batch *b, const int64_t *which, int64_t nwhich, const dzg_batch_post *post,
                        dzg_result *res)
{
    if (const int rc = usable(b, "dzg_batch_resolve")) return rc;
    if (post && !post->du && !post->req && !post->rg && !post->ry) post = nullptr;
    if (which && nwhich < 0) return dzg_set_error(DZG_E_ARG, "dzg_batch_resolve: nwhich < 0");
    const int64_t n = which ? nwhich : b->N;
    if (n > 0 && !res) return dzg_set_error(DZG_E_ARG, "dzg_batch_resolve: res is NULL");
    std::vector<int> ids;
    std::vector<char> seen((size_t)b->N, 0);
    for (int64_t k = 0; k < n; ++k) {
        const int64_t i = which ? which[k] : k;
        const std::string at = "dzg_batch_resolve: which[" + std::to_string(k) + "]: ";
        if (i < 0 || i >= b->N) return dzg_set_error(DZG_E_ARG, at + "lp " + std::to_string(i) + " out of range");
        if (seen[(size_t)i]) return dzg_set_error(DZG_E_ARG, at + "lp " + std::to_string(i) + " listed twice");
        seen[(size_t)i] = 1;
        ids.push_back((int)i);
    }
    if (n > 0 && post && (post->req != nullptr) != (post->rg != nullptr))
        return dzg_set_error(DZG_E_ARG, "dzg_batch_resolve: req and rg go together (one of them is NULL)");
    for (int64_t k = 0; post && post->req && k < n; ++k) {
        std::string why;
        const dzg_lp &lp = b->lp[(size_t)ids[(size_t)k]];
        if (!dzg_ranging_req_valid(&post->req[k], lp.m, lp.n, why))
            return dzg_set_error(DZG_E_ARG, "dzg_batch_resolve: which[" + std::to_string(k) + "]: lp " +
                                                std::to_string(ids[(size_t)k]) + ": " + why);
    }
    b->h2d = b->d2h = 0;
    b->ms = 0.0;
    steps::post_ms() = 0.0;
    if (ids.empty()) return 0;
    if (const int rc = fail_if_device(b, resolve(b, ids, res))) return rc;
    if (!post) return 0;
    // ---- what the listed LPs can say about where they ended, on the handle's own arena: a FAST
    // result through k_batch_fast_post, a STRICT one through the STRICT batch's kernels
    steps::PostRun R;
    R.dev = b->arena;
    R.L = b->L;
    R.state = b->s_fstate;
    R.status = b->s_status;
    R.S = b->post;
    R.rkeep = &b->rarena;
    R.rkeep_bytes = &b->rarena_bytes;
    R.st = b->st;
    std::vector<int64_t> ids64(ids.begin(), ids.end());
    double ms = 0.0;
    for (int strict = b->strict ? 1 : 0; strict <= (b->strict || b->is_auto ? 1 : 0); ++strict)
        if (const int rc = fail_if_device(b, steps::post_pass(R, strict != 0, b->P, (int)n, ids64.data(), res, *post,
                                                              &b->h2d, &b->d2h, &ms)))
            return rc;
    steps::post_ms() = ms;
    return 0;
}

extern "C" int dzg_batch_resolve(dzg_batch *b, const int64_t *which, int64_t nwhich, dzg_result *res)
{
    return resolve_post(b, which, nwhich, nullptr, res);
}

extern "C" int dzg_batch_resolve_post(dzg_batch *b, const int64_t *which, int64_t nwhich,
                                      const dzg_batch_post *post, dzg_result *res)
{
    return resolve_post(b, which, nwhich, post, res);
}

extern "C" int dzg_debug_batch_traffic(const dzg_batch *b, int64_t bytes[2], double ms[1])
{
    if (!b || !bytes || !ms) return dzg_set_error(DZG_E_ARG, "dzg_debug_batch_traffic: NULL argument");
    bytes[0] = b->h2d;
    bytes[1] = b->d2h;
    ms[0] = b->ms;
    return 0;
}
