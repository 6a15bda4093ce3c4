// mip.cpp -- dzg_mip_solve: branch and bound over node LPs (include/dantzig_amd.h).
//
// A node LP is the user's model with each integer variable's lb / ub replaced by the node's; its
// result is what dzg_model_solve returns for that model.  Nodes whose integer variables have the same
// set of finite bounds share one standard form (a "structure", keyed by that mask): bound values only
// move right-hand sides (model.cpp).  Structures are built once, with model.cpp's builder, the first
// time a mask is seen.  Nodes that dzg_model_solve would run in STRICT on <= 128 dense rows are solved
// in rounds on the GPU (k_mip.hip); the rest go through dzg_model_solve one at a time.
//
// Search: each round takes up to nodes_per_round open nodes, best parent bound first (ties: lower
// id), pruning on selection those whose bound is <= incumbent + tol.  The round's results are then
// processed in ascending node id: infeasible -> dropped; objective <= incumbent + tol -> pruned;
// integral -> new incumbent; otherwise branched on the most fractional integer variable (down child
// first).  A child whose bounds cross is never created.  Node ids follow creation order.
//
// Warm starts (opt-in, mip_opts.warm_start): a GPU node that is branched keeps its final basis,
// nonbasis and z in a slot of a device pool while it has open children of its own structure (the
// branch tightened a bound that was already finite); such a child names the slot in its round and
// k_mip.hip starts it from there, restarting it cold if the attempt is not accepted.  A slot is
// taken back once every child that names it is solved or pruned, so the pool never holds more
// slots than there are open nodes.
//
// FAST node LPs (opt-in, dzg_mip_solve_nodes with node_opts.numerics = FAST): every GPU node gets an
// attempt in FAST numerics first (k_mip_node_fast), warm from its parent's slot or cold; the attempts
// that are not certified are solved by the STRICT kernel in the same round.  The search itself does
// not change; a node's record says which way it went, and dzg_mip_last_fast_stats counts.
#include <algorithm>
#include <cmath>
#include <cstring>
#include <map>
#include <set>
#include <string>
#include <vector>

#include "../../include/dantzig_amd.h"
#include "mip_internal.h"
#include "opts.h"

int dzg_set_error(int code, const std::string &msg); // engine.hip

using namespace dzg_internal;

namespace {

struct Node {
    int64_t id, parent, branch_var;
    int32_t direction;
    double bound;              // the new bound of branch_var
    double parent_obj;         // +inf at the root
    std::vector<double> bnd;   // lb_k, ub_k per integer variable (+-inf: no bound)
    int pslot = -1;            // warm starts: the parent's slot in the device state pool
};

struct OpenKey {
    double bound;
    int64_t id;
    bool operator<(const OpenKey &o) const
    {
        if (bound != o.bound) return bound > o.bound; // best (largest) bound first
        return id < o.id;
    }
};

struct StructInfo {
    int gpu_id = -1; // -1: solved through dzg_model_solve
    int64_t m = 0;
};

// Node model: md with the integer variables' bounds replaced.
struct NodeModel {
    std::vector<int32_t> has_lb, has_ub;
    std::vector<double> lb, ub;
    dzg_model md;
    NodeModel(const dzg_model *base, const std::vector<int> &ints, const std::vector<double> &bnd)
        : has_lb(base->has_lb, base->has_lb + base->nvars), has_ub(base->has_ub, base->has_ub + base->nvars),
          lb(base->lb, base->lb + base->nvars), ub(base->ub, base->ub + base->nvars)
    {
        for (size_t k = 0; k < ints.size(); ++k) {
            const int u = ints[k];
            const double l = bnd[2 * k], h = bnd[2 * k + 1];
            has_lb[(size_t)u] = std::isinf(l) ? 0 : 1;
            lb[(size_t)u] = std::isinf(l) ? 0.0 : l;
            has_ub[(size_t)u] = std::isinf(h) ? 0 : 1;
            ub[(size_t)u] = std::isinf(h) ? 0.0 : h;
        }
        md = *base;
        if (base->nvars > 0) {
            md.has_lb = has_lb.data();
            md.has_ub = has_ub.data();
            md.lb = lb.data();
            md.ub = ub.data();
        }
    }
};

bool bad_tol(double t) { return !(t >= 0.0); } // NaN or negative

// The structure k_mip.hip keeps of a built node model; ints: the integer variables in index order.
MipStructure make_structure(const Built &b, int nvars, const std::vector<int> &ints)
{
    const int nint = (int)ints.size();
    std::vector<int> k_of((size_t)(nvars ? nvars : 1), -1);
    for (int k = 0; k < nint; ++k) k_of[(size_t)ints[(size_t)k]] = k;
    MipStructure s;
    s.m = (int)b.m;
    s.n = (int)b.n;
    s.ns = (int)b.ns;
    s.constant = b.constant;
    s.a = b.a;
    s.b0 = b.x;
    s.c = b.c;
    s.z0 = b.z;
    s.var_col.assign(b.var_col.begin(), b.var_col.end());
    s.basis0.assign(b.basis.begin(), b.basis.end());
    s.nonbasis0.assign(b.nonbasis.begin(), b.nonbasis.end());
    s.pos_var.assign(b.pos_var.begin(), b.pos_var.end());
    s.neg_var.assign(b.neg_var.begin(), b.neg_var.end());
    s.row_int.assign((size_t)b.m, -1);
    for (int64_t r = 0; r < b.m; ++r) {
        const int64_t tag = b.row_tag[(size_t)r];
        if (tag < 0) continue;
        const int k = k_of[(size_t)(tag / 2)];
        if (k < 0) continue;                       // a continuous variable's bound row
        s.row_int[(size_t)r] = (tag & 1) ? 2 * k : 2 * k + 1; // lb row -> lb_k, ub row -> ub_k
    }
    return s;
}

thread_local dzg_mip_warm_stats g_warm_stats = {0, 0, 0, 0};
thread_local dzg_mip_fast_stats g_fast_stats = {0, 0, 0, 0};

} // namespace

extern "C" void dzg_mip_opts_default(dzg_mip_opts *mo)
{
    if (!mo) return;
    std::memset(mo, 0, sizeof(*mo));
    mo->int_tol = 1e-6;
    mo->abs_gap = 1e-9;
    mo->rel_gap = 0.0;
}

extern "C" void dzg_mip_last_warm_stats(dzg_mip_warm_stats *out)
{
    if (out) *out = g_warm_stats;
}

extern "C" void dzg_mip_node_opts_default(dzg_mip_node_opts *no)
{
    if (no) std::memset(no, 0, sizeof(*no)); // STRICT, the FAST batch's defaults, no route array
}

extern "C" void dzg_mip_last_fast_stats(dzg_mip_fast_stats *out)
{
    if (out) *out = g_fast_stats;
}

extern "C" int dzg_mip_solve(const dzg_model *model, const int32_t *is_integer, const dzg_opts *opts,
                             const dzg_mip_opts *mip_opts, dzg_mip_result *res)
{
    return dzg_mip_solve_nodes(model, is_integer, opts, mip_opts, nullptr, res);
}

extern "C" int dzg_mip_solve_nodes(const dzg_model *model, const int32_t *is_integer, const dzg_opts *opts,
                                   const dzg_mip_opts *mip_opts, const dzg_mip_node_opts *node_opts,
                                   dzg_mip_result *res)
{
    g_warm_stats = dzg_mip_warm_stats{0, 0, 0, 0};
    g_fast_stats = dzg_mip_fast_stats{0, 0, 0, 0};
    dzg_mip_node_opts no;
    if (node_opts) no = *node_opts; else dzg_mip_node_opts_default(&no);
    if (no.numerics != DZG_NUMERICS_STRICT && no.numerics != DZG_NUMERICS_FAST)
        return dzg_set_error(DZG_E_ARG, "mip: node_opts.numerics must be STRICT or FAST");
    if (no.pivots_per_launch < 0) return dzg_set_error(DZG_E_ARG, "mip: node_opts.pivots_per_launch < 0");
    if (no.refactor_every < 0) return dzg_set_error(DZG_E_ARG, "mip: node_opts.refactor_every < 0");
    if (no.route_cap < 0 || (no.route_cap > 0 && !no.route))
        return dzg_set_error(DZG_E_ARG, "mip: node_opts.route_cap > 0 needs a route buffer (and must not be < 0)");
    const bool fast_on = no.numerics == DZG_NUMERICS_FAST;
    // ---- argument checks, before any device work
    if (!model || !res) return dzg_set_error(DZG_E_ARG, "mip: model or res is NULL");
    if (model->nvars > 0 && !is_integer) return dzg_set_error(DZG_E_ARG, "mip: is_integer is NULL");
    if (!valid(model)) return dzg_set_error(DZG_E_ARG, "mip: the model is malformed");
    if (model->nvars >= (1ll << 31)) return dzg_set_error(DZG_E_ARG, "mip: too many variables");
    dzg_opts o;
    if (opts) o = *opts; else dzg_opts_default(&o);
    if (o.numerics != DZG_NUMERICS_STRICT && o.numerics != DZG_NUMERICS_AUTO)
        return dzg_set_error(DZG_E_ARG, "mip: FAST numerics is not supported for node LPs");
    dzg_mip_opts mo;
    if (mip_opts) mo = *mip_opts; else dzg_mip_opts_default(&mo);
    if (mo.node_limit < 0) return dzg_set_error(DZG_E_ARG, "mip: node_limit < 0");
    if (mo.nodes_per_round < 0) return dzg_set_error(DZG_E_ARG, "mip: nodes_per_round < 0");
    if (mo.pivots_per_launch < 0) return dzg_set_error(DZG_E_ARG, "mip: pivots_per_launch < 0");
    if (mo.warm_start != 0 && mo.warm_start != 1)
        return dzg_set_error(DZG_E_ARG, "mip: warm_start must be 0 or 1");
    if (bad_tol(mo.int_tol) || bad_tol(mo.abs_gap) || bad_tol(mo.rel_gap))
        return dzg_set_error(DZG_E_ARG, "mip: int_tol, abs_gap and rel_gap must be >= 0 (not NaN)");
    if (res->log_cap < 0 || (res->log_cap > 0 && !res->log))
        return dzg_set_error(DZG_E_ARG, "mip: log_cap > 0 needs a log buffer");

    const int64_t node_limit = mo.node_limit > 0 ? mo.node_limit : 100000;
    const int npr = mo.nodes_per_round > 0 ? mo.nodes_per_round : 1024;
    const int ppl = (int)(mo.pivots_per_launch > 0 ? std::min<int64_t>(mo.pivots_per_launch, 1 << 30) : 16);
    const long long max_iter = dzg_opts_resolved(&o).max_iter;
    const double eps = dzg_opts_resolved(&o).epsilon;
    const int nvars = (int)model->nvars;

    std::vector<int> ints;
    for (int u = 0; u < nvars; ++u) {
        if (!is_integer[u]) continue;
        if ((model->has_lb[u] && !std::isfinite(model->lb[u])) || (model->has_ub[u] && !std::isfinite(model->ub[u])))
            return dzg_set_error(DZG_E_ARG, "mip: integer variable " + std::to_string(u) +
                                                " has a flagged bound that is not finite");
        ints.push_back(u);
    }
    const int nint = (int)ints.size();

    res->status = DZG_INFEASIBLE;
    res->has_incumbent = 0;
    res->objective = 0.0;
    res->best_bound = -__builtin_inf();
    res->nodes_solved = res->nodes_batched = res->nodes_sequential = res->nodes_fast = 0;
    res->nodes_pruned = res->nodes_dropped = res->rounds = res->lp_iterations = 0;
    res->incumbent_node = res->failed_node = -1;
    res->log_count = 0;

    MipGpu *gpu = nullptr;
    struct Guard {
        MipGpu **g;
        ~Guard() { mip_gpu_destroy(*g); }
    } guard{&gpu};
    {
        const int rc = mip_gpu_create(&gpu, o.device, nvars, ints);
        if (rc < 0) return rc;
    }

    std::map<std::vector<char>, StructInfo> structs; // mask (has_lb, has_ub per integer) -> structure
    auto structure_of = [&](const std::vector<double> &bnd, const dzg_model *node_md) -> StructInfo {
        std::vector<char> mask((size_t)2 * nint);
        for (size_t j = 0; j < mask.size(); ++j) mask[j] = std::isinf(bnd[j]) ? 0 : 1;
        auto it = structs.find(mask);
        if (it != structs.end()) return it->second;
        Built b;
        build(node_md, b, true);
        StructInfo info;
        info.m = b.m;
        const bool strict = dzg_opts_numerics(o, b.m) == DZG_NUMERICS_STRICT;
        if (strict && !b.sparse && b.m <= DZG_BATCH_MAX_ROWS)
            info.gpu_id = mip_gpu_add_structure(gpu, make_structure(b, nvars, ints));
        structs.emplace(mask, info);
        return info;
    };

    // ---- the root
    std::vector<Node> nodes;
    {
        Node root;
        root.id = 0;
        root.parent = -1;
        root.branch_var = -1;
        root.direction = 0;
        root.bound = 0.0;
        root.parent_obj = __builtin_inf();
        root.bnd.resize((size_t)2 * nint);
        for (int k = 0; k < nint; ++k) {
            const int u = ints[(size_t)k];
            root.bnd[(size_t)2 * k] = model->has_lb[u] ? model->lb[u] : -__builtin_inf();
            root.bnd[(size_t)2 * k + 1] = model->has_ub[u] ? model->ub[u] : __builtin_inf();
        }
        nodes.push_back(std::move(root));
    }
    std::set<OpenKey> open;
    open.insert({__builtin_inf(), 0});

    bool has_inc = false;
    double inc = 0.0;
    std::vector<double> inc_values((size_t)(nvars ? nvars : 1), 0.0);
    auto tol = [&]() { return std::max(mo.abs_gap, mo.rel_gap * std::fabs(inc)); };
    int final_status = -1;

    std::vector<int64_t> round;
    std::vector<int> sid, pslot, slot_refs, round_slot, save_pairs;
    const bool warm_on = mo.warm_start == 1;
    auto release = [&](Node &nd) { // one child fewer names its parent's slot
        if (nd.pslot < 0) return;
        if (--slot_refs[(size_t)nd.pslot] == 0) mip_gpu_slot_free(gpu, nd.pslot);
        nd.pslot = -1;
    };
    std::vector<double> bnd;
    std::vector<MipNodeRecord> rec;
    std::vector<double> vals;
    while (!open.empty()) {
        // ---- select
        round.clear();
        while (!open.empty() && (int)round.size() < npr) {
            const OpenKey key = *open.begin();
            if (has_inc && key.bound <= inc + tol()) {
                open.erase(open.begin());
                res->nodes_pruned++;
                release(nodes[(size_t)key.id]);
                continue;
            }
            if (res->nodes_solved + (int64_t)round.size() >= node_limit) break;
            open.erase(open.begin());
            round.push_back(key.id);
        }
        if (round.empty()) {
            if (!open.empty()) final_status = DZG_NODE_LIMIT;
            break;
        }
        std::sort(round.begin(), round.end());
        res->rounds++;
        const int cnt = (int)round.size();
        rec.assign((size_t)cnt, MipNodeRecord{});
        vals.assign((size_t)cnt * (size_t)nvars + 1, 0.0);
        // ---- GPU nodes in one call, the others through dzg_model_solve
        std::vector<int> gpu_idx;
        sid.clear();
        pslot.clear();
        bnd.clear();
        round_slot.assign((size_t)cnt, -1); // round index -> index in the GPU call
        save_pairs.clear();
        for (int i = 0; i < cnt; ++i) {
            const Node &nd = nodes[(size_t)round[(size_t)i]];
            NodeModel nm(model, ints, nd.bnd);
            const StructInfo info = structure_of(nd.bnd, &nm.md);
            if (info.gpu_id >= 0) {
                round_slot[(size_t)i] = (int)gpu_idx.size();
                gpu_idx.push_back(i);
                sid.push_back(info.gpu_id);
                pslot.push_back(nd.pslot);
                bnd.insert(bnd.end(), nd.bnd.begin(), nd.bnd.end());
                continue;
            }
            dzg_model_result mr;
            std::memset(&mr, 0, sizeof(mr));
            mr.values = vals.data() + (size_t)i * nvars;
            const int rc = dzg_model_solve(&nm.md, &o, &mr);
            if (rc < 0) return rc;
            MipNodeRecord &r = rec[(size_t)i];
            r.status = mr.status;
            r.iterations = mr.iterations;
            r.objective = mr.objective;
            r.branch = -1;
            r.value = 0.0;
            r.integral = 0;
            if (mr.status == DZG_OPTIMAL)
                mip_branch_choice(mr.values, ints.data(), nint, mo.int_tol, &r.branch, &r.value, &r.integral);
            res->nodes_sequential++;
            if (mr.numerics_used == DZG_NUMERICS_FAST) res->nodes_fast++;
        }
        if (!gpu_idx.empty()) {
            const int g = (int)gpu_idx.size();
            std::vector<MipNodeRecord> grec((size_t)g);
            std::vector<double> gvals((size_t)g * nvars + 1, 0.0);
            const MipFastRun fr{&o, no.pivots_per_launch, no.refactor_every};
            const int rc = mip_gpu_solve_round(gpu, sid.data(), warm_on ? pslot.data() : nullptr,
                                               bnd.data(), g, max_iter, eps, ppl, mo.int_tol,
                                               grec.data(), gvals.data(), fast_on ? &fr : nullptr);
            if (rc < 0) return rc;
            for (int j = 0; j < g; ++j) {
                const int i = gpu_idx[(size_t)j];
                rec[(size_t)i] = grec[(size_t)j];
                std::copy(gvals.begin() + (size_t)j * nvars, gvals.begin() + (size_t)(j + 1) * nvars,
                          vals.begin() + (size_t)i * nvars);
            }
            res->nodes_batched += g;
        }
        res->nodes_solved += cnt;
        for (int i = 0; i < cnt; ++i) release(nodes[(size_t)round[(size_t)i]]);
        // ---- process in ascending node id
        for (int i = 0; i < cnt && final_status < 0; ++i) {
            const int64_t id = round[(size_t)i];
            const MipNodeRecord &r = rec[(size_t)i];
            res->lp_iterations += r.iterations;
            if (r.warm) {
                g_warm_stats.nodes_warm++;
                g_warm_stats.warm_iterations += r.warm_iterations;
                if (r.warm == 2) {
                    g_warm_stats.nodes_restarted++;
                    g_warm_stats.restart_iterations += r.iterations - r.warm_iterations;
                }
            }
            if (r.fast) {
                g_fast_stats.nodes_fast++;
                g_fast_stats.fast_iterations += r.fast_iterations;
                if (r.fast == 2) {
                    g_fast_stats.nodes_rejected++;
                    g_fast_stats.strict_iterations += r.iterations - r.fast_iterations;
                }
            }
            if (res->log_count < res->log_cap) {
                if (res->log_count < no.route_cap)
                    no.route[res->log_count] = round_slot[(size_t)i] >= 0 ? r.fast : 3;
                const Node &nd = nodes[(size_t)id];
                dzg_mip_node &e = res->log[res->log_count++];
                e.id = id;
                e.parent = nd.parent;
                e.branch_var = nd.branch_var;
                e.direction = nd.direction;
                e.status = r.status;
                e.bound = nd.bound;
                e.iterations = r.iterations;
                e.objective = r.objective;
            }
            if (r.status == DZG_INFEASIBLE) {
                res->nodes_dropped++;
                continue;
            }
            if (r.status != DZG_OPTIMAL) { // the root's UNBOUNDED included: the search stops
                final_status = r.status;
                res->failed_node = id;
                break;
            }
            if (has_inc && r.objective <= inc + tol()) {
                res->nodes_pruned++;
                continue;
            }
            if (r.integral || r.branch < 0) {
                if (!r.integral) { // no branching candidate (NaN values): nothing to branch on
                    res->nodes_dropped++;
                    continue;
                }
                has_inc = true;
                inc = r.objective;
                res->incumbent_node = id;
                std::copy(vals.begin() + (size_t)i * nvars, vals.begin() + (size_t)(i + 1) * nvars,
                          inc_values.begin());
                continue;
            }
            const int k = r.branch;
            const double fl = std::floor(r.value);
            int my_slot = -1; // this node's state slot, taken when its first warm child is made
            for (int dir = -1; dir <= 1; dir += 2) {
                std::vector<double> cb = nodes[(size_t)id].bnd;
                // the child keeps this node's structure iff the bound it tightens is finite already
                const bool same_structure = !std::isinf(cb[(size_t)2 * k + (dir < 0 ? 1 : 0)]);
                double nb;
                if (dir < 0) {
                    nb = std::min(cb[(size_t)2 * k + 1], fl);
                    cb[(size_t)2 * k + 1] = nb;
                } else {
                    nb = std::max(cb[(size_t)2 * k], fl + 1.0);
                    cb[(size_t)2 * k] = nb;
                }
                if (cb[(size_t)2 * k] > cb[(size_t)2 * k + 1]) {
                    res->nodes_dropped++;
                    continue;
                }
                Node child;
                child.id = (int64_t)nodes.size();
                child.parent = id;
                child.branch_var = ints[(size_t)k];
                child.direction = dir;
                child.bound = nb;
                child.parent_obj = r.objective;
                child.bnd = std::move(cb);
                if (warm_on && same_structure && round_slot[(size_t)i] >= 0) {
                    if (my_slot < 0) {
                        my_slot = mip_gpu_slot_alloc(gpu, sid[(size_t)round_slot[(size_t)i]]);
                        if (my_slot >= 0) {
                            if ((size_t)my_slot >= slot_refs.size()) slot_refs.resize((size_t)my_slot + 1, 0);
                            slot_refs[(size_t)my_slot] = 0;
                            save_pairs.push_back(round_slot[(size_t)i]);
                            save_pairs.push_back(my_slot);
                        }
                    }
                    if (my_slot >= 0) {
                        child.pslot = my_slot;
                        slot_refs[(size_t)my_slot]++;
                    }
                }
                open.insert({child.parent_obj, child.id});
                nodes.push_back(std::move(child));
            }
        }
        if (final_status >= 0) break;
        if (!save_pairs.empty()) {
            const int rc = mip_gpu_save_states(gpu, save_pairs.data(), (int)save_pairs.size() / 2);
            if (rc < 0) return rc;
        }
    }
    if (final_status < 0) final_status = has_inc ? DZG_OPTIMAL : DZG_INFEASIBLE;
    res->status = final_status;
    res->has_incumbent = has_inc ? 1 : 0;
    if (has_inc) {
        res->objective = inc;
        if (res->values && nvars > 0) std::copy(inc_values.begin(), inc_values.begin() + nvars, res->values);
    }
    double bb = has_inc ? inc : -__builtin_inf();
    if (final_status == DZG_NODE_LIMIT)
        for (const OpenKey &key : open) bb = std::max(bb, key.bound);
    res->best_bound = bb;
    return final_status;
}

// Test hook: one node LP through a FAST round (include/dantzig_amd.h).
extern "C" int dzg_debug_mip_fast_node(const dzg_model *model, const int32_t *is_integer, const double *bnd,
                                       const int32_t *start_basis, const dzg_opts *opts,
                                       const dzg_mip_node_opts *node_opts, int64_t cap_m, int64_t cap_q,
                                       int32_t *basis, int32_t *nonbasis, double *x, double *z, int64_t *m_out,
                                       int64_t *q_out, dzg_mip_debug_node *out)
{
    if (!model || !out || !m_out || !q_out || !basis || !nonbasis || !x || !z)
        return dzg_set_error(DZG_E_ARG, "mip: dzg_debug_mip_fast_node: a NULL argument");
    if (model->nvars > 0 && !is_integer) return dzg_set_error(DZG_E_ARG, "mip: is_integer is NULL");
    if (!valid(model)) return dzg_set_error(DZG_E_ARG, "mip: the model is malformed");
    dzg_opts o;
    if (opts) o = *opts; else dzg_opts_default(&o);
    if (o.numerics != DZG_NUMERICS_STRICT && o.numerics != DZG_NUMERICS_AUTO)
        return dzg_set_error(DZG_E_ARG, "mip: FAST numerics is not supported for node LPs");
    dzg_mip_node_opts no;
    if (node_opts) no = *node_opts; else dzg_mip_node_opts_default(&no);
    if (no.pivots_per_launch < 0 || no.refactor_every < 0)
        return dzg_set_error(DZG_E_ARG, "mip: node_opts: a negative count");
    const int nvars = (int)model->nvars;
    std::vector<int> ints;
    for (int u = 0; u < nvars; ++u)
        if (is_integer[u]) ints.push_back(u);
    if (!ints.empty() && !bnd) return dzg_set_error(DZG_E_ARG, "mip: bnd is NULL");
    const std::vector<double> nb(bnd, bnd + 2 * ints.size());
    NodeModel nm(model, ints, nb);
    Built b;
    build(&nm.md, b, true);
    if (b.sparse || b.m > DZG_BATCH_MAX_ROWS || dzg_opts_numerics(o, b.m) != DZG_NUMERICS_STRICT)
        return dzg_set_error(DZG_E_ARG, "mip: this node LP is not one k_mip.hip batches");
    *m_out = b.m;
    *q_out = b.n - b.m;
    if (cap_m < b.m || cap_q < b.n - b.m) return dzg_set_error(DZG_E_ARG, "mip: cap_m or cap_q too small");
    MipGpu *gpu = nullptr;
    struct Guard {
        MipGpu **g;
        ~Guard() { mip_gpu_destroy(*g); }
    } guard{&gpu};
    if (const int rc = mip_gpu_create(&gpu, o.device, nvars, ints); rc < 0) return rc;
    const int sid = mip_gpu_add_structure(gpu, make_structure(b, nvars, ints));
    int pslot = -1;
    if (start_basis) {
        std::vector<char> in((size_t)b.n, 0);
        std::vector<int> sb((size_t)b.m), sn;
        for (int64_t p = 0; p < b.m; ++p) {
            if (start_basis[p] < 0 || start_basis[p] >= b.n)
                return dzg_set_error(DZG_E_ARG, "mip: start_basis names a variable out of range");
            sb[(size_t)p] = start_basis[p];
            in[(size_t)start_basis[p]] = 1;
        }
        for (int64_t j = 0; j < b.n && (int64_t)sn.size() < b.n - b.m; ++j)
            if (!in[(size_t)j]) sn.push_back((int)j);
        sn.resize((size_t)(b.n - b.m), 0);
        pslot = mip_gpu_plant_slot(gpu, sid, sb.data(), sn.data());
        if (pslot < 0) return pslot;
    }
    const MipFastRun fr{&o, no.pivots_per_launch, no.refactor_every};
    MipNodeRecord rec{};
    std::vector<double> vals((size_t)nvars + 1, 0.0);
    const int rc = mip_gpu_solve_round(gpu, &sid, start_basis ? &pslot : nullptr, nb.data(), 1,
                                       dzg_opts_resolved(&o).max_iter, dzg_opts_resolved(&o).epsilon, 16, 1e-6, &rec,
                                       vals.data(), &fr);
    if (rc < 0) return rc;
    std::vector<int> fb((size_t)b.m + 1), fn((size_t)(b.n - b.m) + 1);
    if (const int rc2 = mip_gpu_read_state(gpu, 0, sid, fb.data(), fn.data(), x, z); rc2 < 0) return rc2;
    std::copy(fb.begin(), fb.begin() + b.m, basis);
    std::copy(fn.begin(), fn.begin() + (b.n - b.m), nonbasis);
    out->status = rec.status;
    out->route = rec.fast;
    out->iterations = rec.iterations;
    out->fast_iterations = rec.fast_iterations;
    out->objective = rec.objective;
    return 0;
}
