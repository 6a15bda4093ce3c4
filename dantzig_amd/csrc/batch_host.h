// batch_host.h -- the host half of the batched solvers, written once: k_batch.hip (STRICT, with the
// duals, rays and ranging passes behind it), k_batch_fast.hip (FAST / AUTO) and k_mip.hip (the node
// LPs of a branch-and-bound round) drive their kernels through it.  Host code only; every file still
// launches its own kernel templates, so this header has no translation unit.
//
//   buckets      LPs are grouped by row count; a bucket runs one launch per kMaxGrid workgroups at
//                the block size of kBlock (for_each_chunk, with_block)
//   packing      pack() lays the LPs of a batch end to end and describes each by a DzgBatchLp;
//                Layout places the packed arrays in one device arena; fill_upload() writes the part
//                of the upload buffer that does not depend on the numerics
//   rounds       run_rounds(): every live bucket, one readback of the bucket counters, swap the lists
//   warm starts  start_valid(), warm_lists(), drop_from_first_round(): what the restart pass of
//                either numerics needs around its own kernel
//   results      HostView + unpack_common(): what both numerics report alike
#pragma once

#include <algorithm>
#include <array>
#include <cstring>
#include <string>
#include <type_traits>
#include <vector>

#include "common.h"

int dzg_set_error(int code, const std::string &msg); // engine.hip
int dzg_lp_valid(const dzg_lp *lp, std::string &why);

// A failed HIP call ends the enclosing function with DZG_E_DEVICE and the call's text.
#define DZG_HIP(expr)                                                                           \
    do {                                                                                        \
        hipError_t e_ = (expr);                                                                 \
        if (e_ != hipSuccess)                                                                   \
            return dzg_set_error(DZG_E_DEVICE, std::string(#expr) + ": " + hipGetErrorString(e_)); \
    } while (0)

// One LP of a batch: sizes and its offsets into the packed arrays (elements, not bytes).  Every
// batch kernel reads this one descriptor.  Padded to a power of two (128 B), so that g.lp[id] stays
// the shift it was for the 64-byte descriptors this one replaced: with a multiply in the kernels'
// prologue the STRICT batch measured 0.1 % slower (profiles/batch_host_refactor_bench.jsonl).
struct alignas(64) DzgBatchLp {
    long long a_off;   // A: m x ns column-major, lda = m
    long long vc_off;  // var_col, c, d: n
    long long m_off;   // basis, x, xbar, y, the starting x: m
    long long q_off;   // nonbasis, z, zbar, dz: n - m
    long long log_off; // pivot log (and FAST's margins): log_cap
    long long log_cap;
    double constant;
    int m, n, ns;
};

namespace dzg_bh {

// Row buckets: one launch each, LDS and workgroup size sized for the bucket.
constexpr int kBucketRows[] = {16, 32, 64, DZG_BATCH_MAX_ROWS};
constexpr int kBuckets = 4;
// Workgroups per launch at most: what one launch's pivots_per_launch pivots may cost is bounded by
// how many workgroups must take turns on a CU.  128 rows: 134 KB of LDS, one workgroup per CU, 256
// per launch (16 pivots x 2.3 ms measured = 37 ms per launch); 64 rows: four per CU.
constexpr int kMaxGrid[] = {4096, 4096, 2048, 256};
// Threads per workgroup: one wave per LP up to 32 rows (no barrier has a second wave to wait for),
// then 2 and 4.
constexpr int kBlock[] = {64, 64, 128, 256};

inline int bucket_of(int64_t m)
{
    for (int b = 0; b < kBuckets; ++b)
        if (m <= kBucketRows[b]) return b;
    return -1;
}

// f(first, grid) for every launch of a bucket's list of n entries
template <class F>
void for_each_chunk(int bucket, int n, F f)
{
    for (int c0 = 0; c0 < n; c0 += kMaxGrid[bucket]) f(c0, std::min(kMaxGrid[bucket], n - c0));
}

// f(std::integral_constant<int, BLOCK>) with the bucket's block size, for kernels templated on it
template <class F>
void with_block(int bucket, F f)
{
    switch (kBlock[bucket]) {
    case 64: f(std::integral_constant<int, 64>()); break;
    case 128: f(std::integral_constant<int, 128>()); break;
    default: f(std::integral_constant<int, 256>()); break;
    }
}

using Segments = std::array<int, kBuckets + 1>; // bucket b's entries of a list: [seg[b], seg[b + 1])

inline Segments segments(const int *bucket_n)
{
    Segments seg{};
    for (int b = 0; b < kBuckets; ++b) seg[(size_t)b + 1] = seg[(size_t)b] + bucket_n[b];
    return seg;
}

// Sections of one allocation, 16-B aligned; add() returns the section's byte offset.
struct Arena {
    size_t top = 0;
    size_t add(size_t bytes)
    {
        const size_t off = top;
        top += (bytes + 15) / 16 * 16;
        return off;
    }
};

// The stream and the device allocations of one call.
struct Device {
    hipStream_t st = nullptr;
    unsigned char *arena = nullptr, *arena2 = nullptr;
    Device() = default;
    Device(const Device &) = delete;
    Device &operator=(const Device &) = delete;
    ~Device()
    {
        if (arena) (void)hipFree(arena);
        if (arena2) (void)hipFree(arena2);
        if (st) (void)hipStreamDestroy(st);
    }
};

inline int use_device(int device)
{
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || ndev <= 0)
        return dzg_set_error(DZG_E_DEVICE, "no HIP device visible: dantzig_amd has no CPU path");
    if (device < 0 || device >= ndev) return dzg_set_error(DZG_E_ARG, "opts.device out of range");
    DZG_HIP(hipSetDevice(device));
    return 0;
}

// ---- host checks: malformed input is DZG_E_ARG on any machine, before the first HIP call

// The arguments of a batch entry point; `missing` names an output array of the caller's that is
// NULL though asked for (nullptr: none).
inline int check_batch(const dzg_lp *lps, int64_t count, const dzg_result *res, int64_t pivots_per_launch,
                       const char *missing = nullptr)
{
    if (count < 0) return dzg_set_error(DZG_E_ARG, "batch: count < 0");
    if (count > 0 && (!lps || !res)) return dzg_set_error(DZG_E_ARG, "batch: lps or res is NULL");
    if (count > 0 && missing) return dzg_set_error(DZG_E_ARG, std::string("batch: ") + missing + " is NULL");
    if (count >= (1ll << 31)) return dzg_set_error(DZG_E_ARG, "batch: count out of range");
    if (pivots_per_launch < 0) return dzg_set_error(DZG_E_ARG, "batch: pivots_per_launch < 0");
    return 0;
}

// Every LP of the batch; own(i, why) is the caller's own per-LP check (false: `why` says what is wrong).
template <class Own>
int check_batch(const dzg_lp *lps, int64_t count, Own own)
{
    for (int64_t i = 0; i < count; ++i) {
        const dzg_lp *lp = &lps[i];
        std::string why;
        const std::string at = "batch: lps[" + std::to_string(i) + "]: ";
        if (!dzg_lp_valid(lp, why)) return dzg_set_error(DZG_E_ARG, at + why);
        if (lp->m > DZG_BATCH_MAX_ROWS)
            return dzg_set_error(DZG_E_ARG, at + "m > DZG_BATCH_MAX_ROWS (" +
                                                std::to_string(DZG_BATCH_MAX_ROWS) + ")");
        if (lp->n_struct > 0 && !lp->a) return dzg_set_error(DZG_E_ARG, at + "CSC input is not batched");
        if (lp->n - lp->m > (1ll << 30)) return dzg_set_error(DZG_E_ARG, at + "too many columns");
        if (!own(i, why)) return dzg_set_error(DZG_E_ARG, at + why);
    }
    return 0;
}

inline int check_batch(const dzg_lp *lps, int64_t count)
{
    return check_batch(lps, count, [](int64_t, std::string &) { return true; });
}

// ---- packing

struct Packed {
    std::vector<DzgBatchLp> desc;
    long long na = 0, nvc = 0, nm = 0, nq = 0, nlog = 0; // elements of the packed arrays
    int mmax[kBuckets] = {0, 0, 0, 0};                   // largest m of each bucket
    int bucket_n[kBuckets] = {0, 0, 0, 0};
};

inline Packed pack(const dzg_lp *lps, const dzg_result *res, int count, long long max_iter)
{
    Packed P;
    P.desc.resize((size_t)count);
    for (int i = 0; i < count; ++i) {
        const dzg_lp &lp = lps[i];
        DzgBatchLp &d = P.desc[(size_t)i];
        d.m = (int)lp.m;
        d.n = (int)lp.n;
        d.ns = (int)lp.n_struct;
        d.constant = lp.constant;
        d.a_off = P.na;
        d.vc_off = P.nvc;
        d.m_off = P.nm;
        d.q_off = P.nq;
        d.log_off = P.nlog;
        d.log_cap = res[i].log && res[i].log_cap > 0 ? std::min<long long>(res[i].log_cap, max_iter) : 0;
        P.na += (long long)lp.m * lp.n_struct;
        P.nvc += lp.n;
        P.nm += lp.m;
        P.nq += lp.n - lp.m;
        P.nlog += d.log_cap;
        const int b = bucket_of(lp.m);
        P.mmax[b] = std::max(P.mmax[b], (int)lp.m);
        P.bucket_n[b]++;
    }
    return P;
}

// The solve's arena: upload-only, then state (uploaded and downloaded), then log (downloaded), then
// scratch.  The caller adds its own state sections after the constructor, its own log sections
// after end_upload(), and whatever follows the solve after end_download().
struct Layout {
    Arena ar;
    size_t desc, a, vc, list, state0, basis, nonbasis, x, xbar, z, zbar;
    size_t upload_end = 0, lk = 0, le = 0, ll = 0, lmu = 0;
    size_t download_end = 0, dz = 0, list2 = 0, count = 0;
    long long nlog, nq;
    int N;

    explicit Layout(const Packed &P) : nlog(P.nlog), nq(P.nq), N((int)P.desc.size())
    {
        desc = ar.add(sizeof(DzgBatchLp) * N);
        a = ar.add(sizeof(double) * P.na);
        vc = ar.add(sizeof(int) * P.nvc);
        list = ar.add(sizeof(int) * N);
        state0 = ar.top;
        basis = ar.add(sizeof(int) * P.nm);
        nonbasis = ar.add(sizeof(int) * P.nq);
        x = ar.add(sizeof(double) * P.nm);
        xbar = ar.add(sizeof(double) * P.nm);
        z = ar.add(sizeof(double) * P.nq);
        zbar = ar.add(sizeof(double) * P.nq);
    }
    void end_upload()
    {
        upload_end = ar.top;
        lk = ar.add(sizeof(int) * nlog);
        le = ar.add(sizeof(int) * nlog);
        ll = ar.add(sizeof(int) * nlog);
        lmu = ar.add(sizeof(double) * nlog);
    }
    void end_download()
    {
        download_end = ar.top;
        dz = ar.add(sizeof(double) * nq);
        list2 = ar.add(sizeof(int) * N);
        count = ar.add(sizeof(int) * kBuckets);
    }
};

// The constraint row of a slack variable as var_col codes it (-1 - row), the column of a structural
inline int64_t var_code(const dzg_lp &lp, int64_t v)
{
    return lp.var_col ? lp.var_col[v] : (v < lp.n_struct ? v : -1 - (v - lp.n_struct));
}

// A warm LP's own basis is all slack, one per row; its start is a partition of 0 .. n-1.
inline bool start_valid(const dzg_lp &lp, const dzg_batch_start &s, std::string &why)
{
    if (!s.basis) return true;
    const int64_t m = lp.m, n = lp.n;
    if (n > m && !s.nonbasis) {
        why = "start: nonbasis is NULL beside a basis";
        return false;
    }
    std::vector<char> seen((size_t)m, 0);
    for (int64_t p = 0; p < m; ++p) {
        const int64_t code = var_code(lp, lp.basis[p]);
        if (code >= 0 || seen[(size_t)(-1 - code)]) {
            why = "start: the LP's own basis is not all slack (basis[" + std::to_string(p) + "])";
            return false;
        }
        seen[(size_t)(-1 - code)] = 1;
    }
    seen.assign((size_t)n, 0);
    for (int64_t k = 0; k < n; ++k) {
        const int64_t v = k < m ? s.basis[k] : s.nonbasis[k - m];
        if (v < 0 || v >= n || seen[(size_t)v]) {
            why = "start: basis/nonbasis is not a partition of 0..n-1";
            return false;
        }
        seen[(size_t)v] = 1;
    }
    return true;
}

inline bool any_warm(const dzg_batch_start *start, int count)
{
    for (int i = 0; start && i < count; ++i)
        if (start[i].basis) return true;
    return false;
}

// The descriptors, A, var_col, the starting state and the first round's lists (LP indices grouped by
// bucket) into the upload buffer.  An LP with a start basis (start[i].basis != NULL, dzg_batch_solve_from)
// goes up as k_batch_restart reads it: the start's basis and nonbasis, the right-hand side by
// constraint row in x (lp.x[p] belongs to the row whose slack sits at position p), xbar = zbar = 1.
inline void fill_upload(unsigned char *host, const Layout &L, const Packed &P, const dzg_lp *lps,
                        const dzg_batch_start *start = nullptr)
{
    std::memcpy(host + L.desc, P.desc.data(), sizeof(DzgBatchLp) * P.desc.size());
    double *a = (double *)(host + L.a);
    int *vc = (int *)(host + L.vc), *bs = (int *)(host + L.basis), *nb = (int *)(host + L.nonbasis);
    double *x = (double *)(host + L.x), *xb = (double *)(host + L.xbar), *z = (double *)(host + L.z),
           *zb = (double *)(host + L.zbar);
    int *list = (int *)(host + L.list);
    Segments fill = segments(P.bucket_n);
    for (int i = 0; i < L.N; ++i) {
        const dzg_lp &lp = lps[i];
        const DzgBatchLp &d = P.desc[(size_t)i];
        const int64_t m = lp.m, q = lp.n - lp.m;
        for (int64_t j = 0; j < lp.n_struct; ++j)
            std::memcpy(a + d.a_off + j * m, lp.a + j * lp.lda, sizeof(double) * (size_t)m);
        for (int64_t v = 0; v < lp.n; ++v)
            vc[d.vc_off + v] = lp.var_col ? (int)lp.var_col[v]
                                          : (v < lp.n_struct ? (int)v : (int)(-1 - (v - lp.n_struct)));
        list[fill[(size_t)bucket_of(lp.m)]++] = i;
        if (start && start[i].basis) {
            for (int64_t k = 0; k < m; ++k) {
                bs[d.m_off + k] = (int)start[i].basis[k];
                x[d.m_off + (-1 - var_code(lp, lp.basis[k]))] = lp.x[k];
                xb[d.m_off + k] = 1.0;
            }
            for (int64_t k = 0; k < q; ++k) {
                nb[d.q_off + k] = (int)start[i].nonbasis[k];
                z[d.q_off + k] = 0.0; // the kernel's to write
                zb[d.q_off + k] = 1.0;
            }
            continue;
        }
        for (int64_t k = 0; k < m; ++k) {
            bs[d.m_off + k] = (int)lp.basis[k];
            x[d.m_off + k] = lp.x[k];
            xb[d.m_off + k] = lp.xbar ? lp.xbar[k] : 1.0; // Simplex::new, src/simplex.rs:219-220
        }
        for (int64_t k = 0; k < q; ++k) {
            nb[d.q_off + k] = (int)lp.nonbasis[k];
            z[d.q_off + k] = lp.z[k];
            zb[d.q_off + k] = lp.zbar ? lp.zbar[k] : 1.0;
        }
    }
}

// The device pointers that STRICT's and FAST's kernel arguments have in common.
template <class Args>
void wire(Args &g, unsigned char *dev, const Layout &L)
{
    g.lp = (const DzgBatchLp *)(dev + L.desc);
    g.A = (const double *)(dev + L.a);
    g.var_col = (const int *)(dev + L.vc);
    g.basis = (int *)(dev + L.basis);
    g.nonbasis = (int *)(dev + L.nonbasis);
    g.x = (double *)(dev + L.x);
    g.xbar = (double *)(dev + L.xbar);
    g.z = (double *)(dev + L.z);
    g.zbar = (double *)(dev + L.zbar);
    g.dz = (double *)(dev + L.dz);
    g.log_kind = (int *)(dev + L.lk);
    g.log_enter = (int *)(dev + L.le);
    g.log_leave = (int *)(dev + L.ll);
    g.log_mu = (double *)(dev + L.lmu);
}

// Stream, arena, upload: everything up to L.upload_end goes up.
inline int upload(Device &D, const Layout &L, const unsigned char *host)
{
    DZG_HIP(hipStreamCreateWithFlags(&D.st, hipStreamNonBlocking));
    DZG_HIP(hipMalloc((void **)&D.arena, L.ar.top));
    DZG_HIP(hipMemcpyAsync(D.arena, host, L.upload_end, hipMemcpyHostToDevice, D.st));
    return 0;
}

// The state and the log come down.
inline int download(Device &D, const Layout &L, unsigned char *host)
{
    DZG_HIP(hipMemcpyAsync(host + L.state0, D.arena + L.state0, L.download_end - L.state0,
                           hipMemcpyDeviceToHost, D.st));
    DZG_HIP(hipStreamSynchronize(D.st));
    return 0;
}

// ---- rounds: every bucket's running entries, then one readback of the bucket counters.
// launch(bucket, list, n, next_list, next_count) runs entries list[0..n) of a bucket; a kernel
// appends the entries that are still running to next_list through atomicAdd(next_count, 1).
// cur / nxt: two device lists laid out by `seg`; counts: kBuckets device ints; live: entries per bucket.
// rounds (optional): counts the readbacks, kBuckets ints each.
// tail (optional): kBuckets more device ints lie directly behind `counts`; they are never reset here
// and come down with every readback, into tail[0..kBuckets).
template <class Launch>
int run_rounds(int *cur, int *nxt, int *counts, const Segments &seg, std::array<int, kBuckets> live,
               hipStream_t st, Launch launch, int *rounds = nullptr, int *tail = nullptr)
{
    int back[2 * kBuckets];
    for (;;) {
        bool any = false;
        DZG_HIP(hipMemsetAsync(counts, 0, sizeof(int) * kBuckets, st));
        for (int b = 0; b < kBuckets; ++b) {
            if (live[(size_t)b] == 0) continue;
            any = true;
            launch(b, cur + seg[(size_t)b], live[(size_t)b], nxt + seg[(size_t)b], counts + b);
            DZG_HIP(hipGetLastError());
        }
        if (!any) return 0;
        DZG_HIP(hipMemcpyAsync(back, counts, sizeof(int) * kBuckets * (tail ? 2 : 1), hipMemcpyDeviceToHost, st));
        DZG_HIP(hipStreamSynchronize(st));
        std::copy(back, back + kBuckets, live.begin());
        if (tail) std::copy(back + kBuckets, back + 2 * kBuckets, tail);
        if (rounds) ++*rounds;
        std::swap(cur, nxt);
    }
}

inline std::array<int, kBuckets> live_of(const int *bucket_n)
{
    return {bucket_n[0], bucket_n[1], bucket_n[2], bucket_n[3]};
}

// The LPs whose status satisfies pred, grouped by bucket, in batch order within a bucket.
struct StatusLists {
    std::vector<int> list;
    Segments seg{};
};

template <class Pred>
StatusLists lists_by_status(const int *status, const dzg_lp *lps, int count, Pred pred)
{
    StatusLists out;
    for (int b = 0; b < kBuckets; ++b) {
        for (int i = 0; i < count; ++i)
            if (pred(status[i]) && bucket_of(lps[i].m) == b) out.list.push_back(i);
        out.seg[(size_t)b + 1] = (int)out.list.size();
    }
    return out;
}

// ---- the restart pass of a warm batch (k_batch.hip and k_batch_fast.hip run one before the first
// round): its lists and its clock

// The LPs with a start basis, grouped by bucket, in batch order within a bucket.
inline StatusLists warm_lists(const dzg_lp *lps, const dzg_batch_start *start, int count)
{
    StatusLists out;
    for (int b = 0; b < kBuckets; ++b) {
        for (int i = 0; i < count; ++i)
            if (start[i].basis && bucket_of(lps[i].m) == b) out.list.push_back(i);
        out.seg[(size_t)b + 1] = (int)out.list.size();
    }
    return out;
}

// Two events around the restart launches.
struct Events {
    hipEvent_t e0 = nullptr, e1 = nullptr;
    Events() = default;
    Events(const Events &) = delete;
    Events &operator=(const Events &) = delete;
    ~Events()
    {
        if (e0) (void)hipEventDestroy(e0);
        if (e1) (void)hipEventDestroy(e1);
    }
};

// The first round's lists (the host's copy, as fill_upload wrote it) without the LPs that gone(i)
// names, in the order they had; `live` follows and the lists go up again.
template <class Gone>
int drop_from_first_round(unsigned char *host, unsigned char *dev, const Layout &L, const Packed &P,
                          std::array<int, kBuckets> &live, hipStream_t st, Gone gone)
{
    int *list = (int *)(host + L.list);
    const Segments seg = segments(P.bucket_n);
    for (int b = 0; b < kBuckets; ++b) {
        int n = 0;
        for (int k = seg[(size_t)b]; k < seg[(size_t)b + 1]; ++k)
            if (!gone(list[k])) list[seg[(size_t)b] + n++] = list[k];
        live[(size_t)b] = n;
    }
    DZG_HIP(hipMemcpyAsync(dev + L.list, list, sizeof(int) * L.N, hipMemcpyHostToDevice, st));
    return 0;
}

// ---- results

// The downloaded state and log, as packed.
struct HostView {
    const int *basis, *nonbasis;
    const double *x, *xbar, *z, *zbar;
    const int *lk, *le, *ll;
    const double *lmu;
    HostView(const unsigned char *host, const Layout &L)
        : basis((const int *)(host + L.basis)), nonbasis((const int *)(host + L.nonbasis)),
          x((const double *)(host + L.x)), xbar((const double *)(host + L.xbar)),
          z((const double *)(host + L.z)), zbar((const double *)(host + L.zbar)),
          lk((const int *)(host + L.lk)), le((const int *)(host + L.le)), ll((const int *)(host + L.ll)),
          lmu((const double *)(host + L.lmu))
    {
    }
};

// What both numerics report alike: the objective, the state vectors, the pivot log (r.iterations is
// set already) and the profile fields a batch does not measure.
inline void unpack_common(const dzg_lp &lp, const DzgBatchLp &d, const HostView &h, dzg_result &r)
{
    const int64_t m = lp.m, q = lp.n - lp.m;
    double sum = 0.0; // objective_value, src/simplex.rs:345-352, basis-position order
    for (int64_t p = 0; p < m; ++p) {
        const double prod = lp.c[h.basis[d.m_off + p]] * h.x[d.m_off + p];
        sum = sum + prod;
    }
    r.objective = lp.constant + sum;
    for (int64_t k = 0; k < m; ++k) {
        if (r.basis) r.basis[k] = h.basis[d.m_off + k];
        if (r.x) r.x[k] = h.x[d.m_off + k];
        if (r.xbar) r.xbar[k] = h.xbar[d.m_off + k];
    }
    for (int64_t k = 0; k < q; ++k) {
        if (r.nonbasis) r.nonbasis[k] = h.nonbasis[d.q_off + k];
        if (r.z) r.z[k] = h.z[d.q_off + k];
        if (r.zbar) r.zbar[k] = h.zbar[d.q_off + k];
    }
    const long long cnt = std::min<long long>(r.iterations, d.log_cap);
    for (long long k = 0; k < cnt; ++k) {
        r.log[k].kind = h.lk[d.log_off + k];
        r.log[k].reserved = 0;
        r.log[k].entering = h.le[d.log_off + k];
        r.log[k].leaving = h.ll[d.log_off + k];
        r.log[k].mu = h.lmu[d.log_off + k];
    }
    for (int c = 0; c < DZG_K_COUNT; ++c) {
        r.kernel_ms[c] = 0.0;
        r.kernel_launches[c] = 0;
    }
    r.price_bytes = 0.0;
    r.solve_ms = 0.0;
    r.max_pivot_error = 0.0;
    r.near_ties = 0;
    r.first_near_tie = -1;
    r.min_margin = __builtin_inf();
    r.dense_columns = 0;
    r.refactors = 0;
    r.chain_fallbacks = 0;
    r.price_pass_used = 0;
    r.price_rows_copy = 0;
    r.state_drift = 0.0; // not measured by the batched solvers
}

} // namespace dzg_bh
