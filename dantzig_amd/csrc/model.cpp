// model.cpp -- Level 2 of the C ABI: the standard-form builder and the whole of
// `dantzig.rust.solve` (src/lib.rs:16-27) = Simplex::new + Simplex::solve + PySolution::from.
//
// Builder semantics follow Simplex::new (src/simplex.rs:123-224): every user variable is
// split x = x+ - x- in order of first appearance (objective first, then the rows); a finite
// ub adds the row x+ - x- <= ub and a finite lb the row -x+ + x- <= -lb, ub before lb,
// appended after the user rows; every row gets a slack; variables are numbered by first
// appearance over objective then rows (slack last in its row); slacks start basic with
// x = rhs, everything else nonbasic with z = -c.  Coefficients are scattered by assignment
// (the last duplicate wins, src/linalg.rs:34-36, src/simplex.rs:41-43).
//
// Unlike the reference (COO -> dense m x n row-major -> CSC, src/simplex.rs:62-81) the
// structural block is written straight into the column-major layout the GPU consumes and
// slack columns are never materialised.
#include <cmath>
#include <cstring>
#include <string>
#include <vector>

#include "../../include/dantzig_amd.h"
#include "mip_internal.h"
#include "opts.h"

namespace {

struct Row {
    std::vector<int64_t> id; // internal ids: 2*ord = x+, 2*ord+1 = x-, slack0 + r = slack
    std::vector<double> coef;
    double b = 0.0;
    int64_t tag = -1;        // Built::row_tag
};

} // namespace

namespace dzg_internal {

bool valid(const dzg_model *md)
{
    if (!md || md->nvars < 0 || md->obj_nterms < 0 || md->ncons < 0) return false;
    if (md->nvars > 0 && (!md->has_lb || !md->has_ub || !md->lb || !md->ub)) return false;
    if (md->obj_nterms > 0 && (!md->obj_var || !md->obj_coef)) return false;
    if (md->ncons > 0 && (!md->con_ptr || !md->con_b)) return false;
    for (int64_t t = 0; t < md->obj_nterms; ++t)
        if (md->obj_var[t] < 0 || md->obj_var[t] >= md->nvars) return false;
    if (md->ncons > 0) {
        if (md->con_ptr[0] != 0) return false;
        for (int64_t r = 0; r < md->ncons; ++r)
            if (md->con_ptr[r + 1] < md->con_ptr[r]) return false;
        const int64_t nt = md->con_ptr[md->ncons];
        if (nt > 0 && (!md->con_var || !md->con_coef)) return false;
        for (int64_t e = 0; e < nt; ++e)
            if (md->con_var[e] < 0 || md->con_var[e] >= md->nvars) return false;
    }
    return true;
}

void build(const dzg_model *md, Built &out, bool allow_sparse)
{
    const int64_t V = md->nvars;
    std::vector<int64_t> ord((size_t)V, -1);
    int64_t nseen = 0;
    std::vector<Row> bound_rows;
    auto see = [&](int64_t u) {
        if (ord[(size_t)u] >= 0) return;
        ord[(size_t)u] = nseen++;
        const int64_t pos = 2 * ord[(size_t)u], neg = pos + 1;
        if (md->has_ub[u]) { // src/simplex.rs:141-144
            Row r;
            r.id = {pos, neg};
            r.coef = {1.0, -1.0};
            r.b = md->ub[u];
            r.tag = 2 * u;
            bound_rows.push_back(std::move(r));
        }
        if (md->has_lb[u]) { // :145-148
            Row r;
            r.id = {pos, neg};
            r.coef = {-1.0, 1.0};
            r.b = -md->lb[u];
            r.tag = 2 * u + 1;
            bound_rows.push_back(std::move(r));
        }
    };
    for (int64_t t = 0; t < md->obj_nterms; ++t) see(md->obj_var[t]);
    const int64_t nterms = md->ncons ? md->con_ptr[md->ncons] : 0;
    for (int64_t e = 0; e < nterms; ++e) see(md->con_var[e]);

    std::vector<Row> rows((size_t)md->ncons);
    for (int64_t r = 0; r < md->ncons; ++r) {
        Row &row = rows[(size_t)r];
        for (int64_t e = md->con_ptr[r]; e < md->con_ptr[r + 1]; ++e) {
            const int64_t o = ord[(size_t)md->con_var[e]];
            row.id.push_back(2 * o);
            row.coef.push_back(md->con_coef[e]);
            row.id.push_back(2 * o + 1);
            row.coef.push_back(-md->con_coef[e]);
        }
        row.b = md->con_b[r];
    }
    for (Row &r : bound_rows) rows.push_back(std::move(r));

    const int64_t m = (int64_t)rows.size();
    const int64_t ns = 2 * nseen, slack0 = ns, n = ns + m;
    for (int64_t r = 0; r < m; ++r) { // slack injected last, src/simplex.rs:19-31
        rows[(size_t)r].id.push_back(slack0 + r);
        rows[(size_t)r].coef.push_back(1.0);
    }

    // variable index = order of first appearance, src/simplex.rs:168-176
    std::vector<int64_t> index_of((size_t)n, -1), id_of((size_t)n, -1);
    int64_t next = 0;
    auto touch = [&](int64_t id) {
        if (index_of[(size_t)id] < 0) {
            index_of[(size_t)id] = next;
            id_of[(size_t)next++] = id;
        }
    };
    for (int64_t t = 0; t < md->obj_nterms; ++t) {
        const int64_t o = ord[(size_t)md->obj_var[t]];
        touch(2 * o);
        touch(2 * o + 1);
    }
    for (const Row &r : rows)
        for (int64_t id : r.id) touch(id);

    out.m = m;
    out.n = n;
    out.ns = ns;
    out.row_tag.resize((size_t)m);
    for (int64_t r = 0; r < m; ++r) out.row_tag[(size_t)r] = rows[(size_t)r].tag;
    out.constant = md->obj_const;
    out.c.assign((size_t)n, 0.0);
    for (int64_t t = 0; t < md->obj_nterms; ++t) { // Objective::new, assignment
        const int64_t o = ord[(size_t)md->obj_var[t]];
        out.c[(size_t)index_of[(size_t)(2 * o)]] = md->obj_coef[t];
        out.c[(size_t)index_of[(size_t)(2 * o + 1)]] = -md->obj_coef[t];
    }
    out.var_col.resize((size_t)n);
    for (int64_t i = 0; i < n; ++i) {
        const int64_t id = id_of[(size_t)i];
        if (id >= slack0) {
            out.var_col[(size_t)i] = -1 - (id - slack0);
            out.basis.push_back(i);
            out.x.push_back(rows[(size_t)(id - slack0)].b);
        } else {
            out.var_col[(size_t)i] = id; // structural column = internal id
            out.nonbasis.push_back(i);
            out.z.push_back(-out.c[(size_t)i]);
        }
    }
    // dense when small or dense; CSC when the m x ns block would be large and mostly zero
    // (the reference densifies to m x n regardless, src/simplex.rs:62-81)
    int64_t nterms_total = 0;
    for (const Row &row : rows) nterms_total += (int64_t)row.id.size() - 1;
    out.sparse = allow_sparse && m * ns >= (int64_t)1 << 22 && nterms_total * 4 < m * ns;
    if (!out.sparse) {
        out.a.assign((size_t)(m * ns > 0 ? m * ns : 1), 0.0);
        for (int64_t r = 0; r < m; ++r) {
            const Row &row = rows[(size_t)r];
            for (size_t e = 0; e + 1 < row.id.size(); ++e) // all but the slack
                out.a[(size_t)(row.id[e] * m + r)] = row.coef[e];
        }
    } else {
        // rows are visited in ascending order, so every column's entries come out row-ascending;
        // a variable repeated inside one row keeps its LAST coefficient (assignment semantics)
        std::vector<int64_t> cnt((size_t)ns + 1, 0);
        std::vector<int64_t> last_row((size_t)ns, -1);
        for (int64_t r = 0; r < m; ++r) {
            const Row &row = rows[(size_t)r];
            for (size_t e = 0; e + 1 < row.id.size(); ++e)
                if (last_row[(size_t)row.id[e]] != r) {
                    last_row[(size_t)row.id[e]] = r;
                    ++cnt[(size_t)row.id[e] + 1];
                }
        }
        for (int64_t j = 0; j < ns; ++j) cnt[(size_t)j + 1] += cnt[(size_t)j];
        out.col_ptr = cnt;
        out.row_idx.assign((size_t)cnt[(size_t)ns] + 1, 0);
        out.val.assign((size_t)cnt[(size_t)ns] + 1, 0.0);
        std::vector<int64_t> fill(cnt.begin(), cnt.end() - 1);
        std::fill(last_row.begin(), last_row.end(), -1);
        std::vector<int64_t> slot_of((size_t)ns, -1);
        for (int64_t r = 0; r < m; ++r) {
            const Row &row = rows[(size_t)r];
            for (size_t e = 0; e + 1 < row.id.size(); ++e) {
                const int64_t j = row.id[e];
                if (last_row[(size_t)j] != r) {
                    last_row[(size_t)j] = r;
                    slot_of[(size_t)j] = fill[(size_t)j]++;
                    out.row_idx[(size_t)slot_of[(size_t)j]] = (int32_t)r;
                }
                out.val[(size_t)slot_of[(size_t)j]] = row.coef[e];
            }
        }
    }
    out.pos_var.assign((size_t)V, -1);
    out.neg_var.assign((size_t)V, -1);
    for (int64_t u = 0; u < V; ++u)
        if (ord[(size_t)u] >= 0) {
            out.pos_var[(size_t)u] = index_of[(size_t)(2 * ord[(size_t)u])];
            out.neg_var[(size_t)u] = index_of[(size_t)(2 * ord[(size_t)u] + 1)];
        }
}

// Simplex::solution, src/simplex.rs:354-371: x+ - x- per user variable from the final basis
void solution_values(const dzg_model *md, const Built &b, const int64_t *basis, const double *x,
                     double *values)
{
    std::vector<int64_t> pos_of((size_t)(b.n ? b.n : 1), -1);
    for (int64_t p = 0; p < b.m; ++p) pos_of[(size_t)basis[p]] = p;
    for (int64_t u = 0; u < md->nvars; ++u) {
        if (b.pos_var[(size_t)u] < 0) {
            values[u] = 0.0; // unknown variable, src/pyobjs.rs:163-165
            continue;
        }
        const int64_t pp = pos_of[(size_t)b.pos_var[(size_t)u]];
        const int64_t pn = pos_of[(size_t)b.neg_var[(size_t)u]];
        const double pos = pp >= 0 ? x[(size_t)pp] : 0.0;
        const double neg = pn >= 0 ? x[(size_t)pn] : 0.0;
        values[u] = pos - neg;
    }
}

} // namespace dzg_internal

using dzg_internal::Built;
using dzg_internal::build;
using dzg_internal::solution_values;
using dzg_internal::valid;

extern "C" int dzg_build_standard_form(const dzg_model *md, dzg_stdform *out)
{
    if (!out || !valid(md)) return DZG_E_ARG;
    Built b;
    build(md, b, false);
    if (!out->a && !out->var_col && !out->c) { // sizing call
        out->m = b.m;
        out->n = b.n;
        out->n_struct = b.ns;
        out->lda = b.m > 0 ? b.m : 1;
        out->constant = b.constant;
        return 0;
    }
    if (out->m != b.m || out->n != b.n || out->n_struct != b.ns || out->lda < b.m) return DZG_E_ARG;
    for (int64_t j = 0; j < b.ns; ++j)
        for (int64_t i = 0; i < b.m; ++i) out->a[j * out->lda + i] = b.a[(size_t)(j * b.m + i)];
    std::memcpy(out->var_col, b.var_col.data(), sizeof(int64_t) * (size_t)b.n);
    std::memcpy(out->c, b.c.data(), sizeof(double) * (size_t)b.n);
    out->constant = b.constant;
    if (b.m) {
        std::memcpy(out->basis, b.basis.data(), sizeof(int64_t) * (size_t)b.m);
        std::memcpy(out->x, b.x.data(), sizeof(double) * (size_t)b.m);
    }
    if (b.n - b.m) {
        std::memcpy(out->nonbasis, b.nonbasis.data(), sizeof(int64_t) * (size_t)(b.n - b.m));
        std::memcpy(out->z, b.z.data(), sizeof(double) * (size_t)(b.n - b.m));
    }
    if (md->nvars) {
        std::memcpy(out->pos_var, b.pos_var.data(), sizeof(int64_t) * (size_t)md->nvars);
        std::memcpy(out->neg_var, b.neg_var.data(), sizeof(int64_t) * (size_t)md->nvars);
    }
    return 0;
}

int dzg_set_error(int code, const std::string &msg); // engine.hip
int dzg_core_solve_with_duals(const dzg_lp *lp, const dzg_opts *opts, dzg_result *res, dzg_duals *du);

// The one place that maps the standard form's dual vector to the user's model: user rows first,
// then the bound rows by their tag (Built::row_tag).
static void map_duals(const dzg_model *md, const Built &b, const double *y, dzg_model_duals *out)
{
    for (int64_t r = 0; r < md->ncons; ++r) out->con_dual[r] = y[r];
    for (int64_t u = 0; u < md->nvars; ++u) {
        if (out->lb_dual) out->lb_dual[u] = 0.0;
        if (out->ub_dual) out->ub_dual[u] = 0.0;
    }
    for (int64_t r = md->ncons; r < b.m; ++r) {
        const int64_t tag = b.row_tag[(size_t)r];
        if (tag < 0) continue;
        double *dst = (tag & 1) ? out->lb_dual : out->ub_dual;
        if (dst) dst[tag / 2] = y[r];
    }
    if (!out->var_rc) return;
    // var_rc[u] = c_u - sum_r a_{r,u} con_dual[r], rows ascending; a repeated variable keeps its
    // last coefficient, in the objective and inside a row (assignment semantics of the builder)
    std::vector<double> acc((size_t)(md->nvars ? md->nvars : 1), 0.0);
    std::vector<int64_t> last((size_t)(md->nvars ? md->nvars : 1), -1);
    for (int64_t r = 0; r < md->ncons; ++r) {
        for (int64_t e = md->con_ptr[r]; e < md->con_ptr[r + 1]; ++e) last[(size_t)md->con_var[e]] = e;
        for (int64_t e = md->con_ptr[r]; e < md->con_ptr[r + 1]; ++e) {
            const int64_t u = md->con_var[e];
            if (last[(size_t)u] != e) continue;
            const double prod = md->con_coef[e] * y[r];
            acc[(size_t)u] = acc[(size_t)u] + prod;
        }
    }
    for (int64_t u = 0; u < md->nvars; ++u) {
        const double cu = b.pos_var[(size_t)u] >= 0 ? b.c[(size_t)b.pos_var[(size_t)u]] : 0.0;
        out->var_rc[u] = cu - acc[(size_t)u];
    }
}

extern "C" int dzg_model_map_duals(const dzg_model *md, const double *y, int64_t m, dzg_model_duals *out)
{
    if (!out || !valid(md)) return dzg_set_error(DZG_E_ARG, "map duals: out is NULL or the model is malformed");
    if (md->ncons > 0 && !out->con_dual) return dzg_set_error(DZG_E_ARG, "map duals: con_dual is NULL");
    Built b;
    build(md, b, true);
    if (m != b.m || (m > 0 && !y))
        return dzg_set_error(DZG_E_ARG, "map duals: y must hold the " + std::to_string(b.m) +
                                            " rows of the model's standard form");
    map_duals(md, b, y, out);
    return 0;
}

void dzg_duals_none(dzg_duals *du, double objective); // engine.hip

// What a solve's core duals (scalars, and y in `yv`) become in the caller's dzg_model_duals; the
// caller's y / d pointers stay the caller's (d was filled in place).
static void adopt_duals(const dzg_model *md, const Built &b, int status, double objective,
                        const dzg_duals &core, const double *yv, dzg_model_duals *du)
{
    if (status != DZG_OPTIMAL || core.source == 0) {
        dzg_duals_none(&du->core, objective);
        return;
    }
    double *uy = du->core.y, *ud = du->core.d;
    du->core = core;
    du->core.y = uy;
    du->core.d = ud;
    if (uy && b.m) std::memcpy(uy, yv, sizeof(double) * (size_t)b.m);
    map_duals(md, b, yv, du);
}

// engine.hip
bool dzg_ranging_req_valid(const dzg_ranging_req *req, int64_t m, int64_t n, std::string &why);
void dzg_ranging_none(const dzg_ranging_req *req, dzg_ranging *rg);
int dzg_core_solve_with_ranging(const dzg_lp *lp, const dzg_opts *opts, dzg_result *res, dzg_duals *du,
                                const dzg_ranging_req *req, dzg_ranging *rg, int *rg_rc);

// A model's ranging request as core directions over the standard form `b`.
struct CoreRanging {
    std::vector<int64_t> cost_ptr, cost_idx, rhs_ptr, rhs_idx;
    std::vector<double> cost_val, rhs_val;
    dzg_ranging_req req;
};

// The one place that maps a request in the user's terms to core directions (Built's numbering):
// user variable u -> +1 on x+ and -1 on x-; a group of user rows -> the same rows of the standard
// form, which lists the user rows first.  false: `why` says what is wrong.
static bool map_ranging_req(const dzg_model *md, const Built &b, const dzg_model_ranging_req *mr,
                            CoreRanging &out, std::string &why)
{
    if (!mr) { why = "model ranging: req is NULL"; return false; }
    if (mr->nvar < 0 || mr->nrow < 0) { why = "model ranging: negative count"; return false; }
    if (mr->nvar > 0 && !mr->var) { why = "model ranging: var is NULL"; return false; }
    if (mr->nrow > 0 && !mr->row_ptr) { why = "model ranging: row_ptr is NULL"; return false; }
    out.cost_ptr.assign(1, 0);
    for (int64_t i = 0; i < mr->nvar; ++i) {
        const int64_t u = mr->var[i];
        if (u < 0 || u >= md->nvars) {
            why = "model ranging: variable " + std::to_string(u) + " out of range";
            return false;
        }
        if (b.pos_var[(size_t)u] < 0) {
            why = "model ranging: variable " + std::to_string(u) + " appears nowhere in the model";
            return false;
        }
        out.cost_idx.push_back(b.pos_var[(size_t)u]);
        out.cost_val.push_back(1.0);
        out.cost_idx.push_back(b.neg_var[(size_t)u]);
        out.cost_val.push_back(-1.0);
        out.cost_ptr.push_back((int64_t)out.cost_idx.size());
    }
    out.rhs_ptr.assign(1, 0);
    if (mr->nrow > 0) {
        if (mr->row_ptr[0] != 0) { why = "model ranging: row_ptr[0] != 0"; return false; }
        for (int64_t i = 0; i < mr->nrow; ++i)
            if (mr->row_ptr[i + 1] < mr->row_ptr[i]) { why = "model ranging: row_ptr decreases"; return false; }
        if (mr->row_ptr[mr->nrow] > 0 && (!mr->row_idx || !mr->row_coef)) {
            why = "model ranging: row_idx or row_coef is NULL";
            return false;
        }
    }
    for (int64_t i = 0; i < mr->nrow; ++i) {
        for (int64_t e = mr->row_ptr[i]; e < mr->row_ptr[i + 1]; ++e) {
            if (mr->row_idx[e] < 0 || mr->row_idx[e] >= md->ncons) {
                why = "model ranging: row " + std::to_string(mr->row_idx[e]) + " out of range";
                return false;
            }
            out.rhs_idx.push_back(mr->row_idx[e]); // user rows come first in the standard form
            out.rhs_val.push_back(mr->row_coef[e]);
        }
        out.rhs_ptr.push_back((int64_t)out.rhs_idx.size());
    }
    out.req.ncost = mr->nvar;
    out.req.cost_ptr = out.cost_ptr.data();
    out.req.cost_idx = out.cost_idx.data();
    out.req.cost_val = out.cost_val.data();
    out.req.nrhs = mr->nrow;
    out.req.rhs_ptr = out.rhs_ptr.data();
    out.req.rhs_idx = out.rhs_idx.data();
    out.req.rhs_val = out.rhs_val.data();
    out.req.pivot_tol = mr->pivot_tol;
    return dzg_ranging_req_valid(&out.req, b.m, b.n, why); // duplicates inside a group, pivot_tol
}

// engine.hip
void dzg_ray_none(dzg_ray *ry);
int dzg_core_solve_with_rays(const dzg_lp *lp, const dzg_opts *opts, dzg_result *res, dzg_duals *du,
                             dzg_ray *ry);

// The one place that maps a core ray to the user's model.  Rows as map_duals walks them (user rows
// first, then the bound rows by their tag); a row's entry is the d of its slack for a primal ray and
// its y for a Farkas ray.
static void map_ray(const dzg_model *md, const Built &b, int kind, const double *d, const double *y,
                    dzg_model_ray *out)
{
    std::vector<int64_t> slack_var((size_t)(b.m ? b.m : 1), -1);
    for (int64_t i = 0; i < b.n; ++i)
        if (b.var_col[(size_t)i] < 0) slack_var[(size_t)(-1 - b.var_col[(size_t)i])] = i;
    auto row = [&](int64_t r) { return kind == DZG_RAY_PRIMAL ? d[slack_var[(size_t)r]] : y[r]; };
    for (int64_t r = 0; r < md->ncons; ++r) out->con[r] = row(r);
    for (int64_t u = 0; u < md->nvars; ++u) {
        out->lb[u] = 0.0;
        out->ub[u] = 0.0;
        out->var[u] = b.pos_var[(size_t)u] >= 0 ? d[b.pos_var[(size_t)u]] - d[b.neg_var[(size_t)u]] : 0.0;
    }
    for (int64_t r = md->ncons; r < b.m; ++r) {
        const int64_t tag = b.row_tag[(size_t)r];
        if (tag < 0) continue;
        double *dst = (tag & 1) ? out->lb : out->ub;
        dst[tag / 2] = row(r);
    }
}

static bool ray_arrays_ok(const dzg_model *md, const dzg_model_ray *ry)
{
    return ry && (md->ncons == 0 || ry->con) && (md->nvars == 0 || (ry->var && ry->lb && ry->ub));
}

extern "C" int dzg_model_map_ray(const dzg_model *md, int32_t kind, const double *d, const double *y,
                                 int64_t m, int64_t n, dzg_model_ray *out)
{
    if (!out || !valid(md)) return dzg_set_error(DZG_E_ARG, "map ray: out is NULL or the model is malformed");
    if (kind != DZG_RAY_PRIMAL && kind != DZG_RAY_FARKAS)
        return dzg_set_error(DZG_E_ARG, "map ray: kind is neither DZG_RAY_PRIMAL nor DZG_RAY_FARKAS");
    if (!ray_arrays_ok(md, out)) return dzg_set_error(DZG_E_ARG, "map ray: var, con, lb or ub is NULL");
    Built b;
    build(md, b, true);
    if (m != b.m || n != b.n || (n > 0 && !d) || (kind == DZG_RAY_FARKAS && m > 0 && !y))
        return dzg_set_error(DZG_E_ARG, "map ray: d and y must hold the " + std::to_string(b.n) +
                                            " variables and " + std::to_string(b.m) +
                                            " rows of the model's standard form");
    map_ray(md, b, kind, d, y, out);
    return 0;
}

// What a solve's core ray (scalars; d in `dv`, y in `yv`) becomes in the caller's dzg_model_ray; the
// caller's d / y pointers stay the caller's.
static void adopt_ray(const dzg_model *md, const Built &b, const dzg_ray &core, const double *dv,
                      const double *yv, dzg_model_ray *ry)
{
    double *ud = ry->core.d, *uy = ry->core.y;
    if (core.kind == 0) {
        dzg_ray_none(&ry->core);
        return;
    }
    ry->core = core;
    ry->core.d = ud;
    ry->core.y = uy;
    if (ud && b.n) std::memcpy(ud, dv, sizeof(double) * (size_t)b.n);
    if (uy && b.m) std::memcpy(uy, yv, sizeof(double) * (size_t)b.m);
    map_ray(md, b, core.kind, dv, yv, ry);
}

static int model_solve(const dzg_model *md, const dzg_opts *opts, dzg_model_result *res,
                       dzg_model_duals *du, bool want_duals, const dzg_model_ranging_req *mreq = nullptr,
                       dzg_ranging *rg = nullptr, dzg_model_ray *ry = nullptr)
{
    if (!res || !valid(md)) return DZG_E_ARG;
    if (want_duals && (!du || (md->ncons > 0 && !du->con_dual))) return DZG_E_ARG;
    if (ry && !ray_arrays_ok(md, ry)) return DZG_E_ARG;
    Built b;
    build(md, b, true);
    CoreRanging cr;
    if (rg) {
        std::string why;
        if (!map_ranging_req(md, b, mreq, cr, why)) return dzg_set_error(DZG_E_ARG, why);
    }
    res->m = b.m;
    res->n = b.n;
    dzg_lp lp;
    std::memset(&lp, 0, sizeof(lp));
    lp.m = b.m;
    lp.n = b.n;
    lp.n_struct = b.ns;
    lp.a = b.sparse ? nullptr : b.a.data();
    lp.lda = b.m > 0 ? b.m : 1;
    if (b.sparse) {
        lp.col_ptr = b.col_ptr.data();
        lp.row_idx = b.row_idx.data();
        lp.val = b.val.data();
    }
    lp.var_col = b.var_col.data();
    lp.c = b.c.data();
    lp.constant = b.constant;
    lp.basis = b.basis.data();
    lp.nonbasis = b.nonbasis.data();
    lp.x = b.x.data();
    lp.z = b.z.data();
    std::vector<int64_t> basis((size_t)(b.m ? b.m : 1));
    std::vector<double> x((size_t)(b.m ? b.m : 1));
    dzg_result r;
    std::memset(&r, 0, sizeof(r));
    r.basis = basis.data();
    r.x = x.data();
    // AUTO: falls back to STRICT if FAST gives up; the duals are those of the solver whose result this is
    std::vector<double> yv((size_t)(b.m ? b.m : 1), 0.0);
    dzg_duals core;
    std::memset(&core, 0, sizeof(core));
    if (want_duals) {
        core.y = yv.data();
        core.d = du->core.d;
    }
    std::vector<double> ray_d((size_t)(ry && b.n ? b.n : 1), 0.0), ray_y((size_t)(ry && b.m ? b.m : 1), 0.0);
    dzg_ray ray_core;
    std::memset(&ray_core, 0, sizeof(ray_core));
    ray_core.d = ray_d.data();
    ray_core.y = ray_y.data();
    int rg_rc = 0;
    const int rc = rg ? dzg_core_solve_with_ranging(&lp, opts, &r, &core, &cr.req, rg, &rg_rc)
                 : ry ? dzg_core_solve_with_rays(&lp, opts, &r, want_duals ? &core : nullptr, &ray_core)
                      : dzg_core_solve_with_duals(&lp, opts, &r, want_duals ? &core : nullptr);
    res->status = rc < 0 ? rc : r.status;
    res->numerics_used = r.numerics_used;
    res->iterations = r.iterations;
    res->objective = r.objective;
    res->near_ties = r.near_ties;
    res->first_near_tie = r.first_near_tie;
    if (rc < 0) return rc;
    if (res->values) solution_values(md, b, basis.data(), x.data(), res->values);
    if (want_duals) adopt_duals(md, b, r.status, r.objective, core, yv.data(), du);
    if (ry) adopt_ray(md, b, ray_core, ray_d.data(), ray_y.data(), ry);
    // (ranging failed after an OPTIMAL solve -- a route without ranging, no memory, a final basis
    // that did not refactorise: the call fails with that code, dzg_last_error holds
    // dzg_solver_ranging's text; res keeps the solve's outcome)
    if (rg && r.status == DZG_OPTIMAL && rg_rc < 0) return rg_rc;
    return r.status;
}

extern "C" int dzg_model_solve(const dzg_model *md, const dzg_opts *opts, dzg_model_result *res)
{
    return model_solve(md, opts, res, nullptr, false);
}

extern "C" int dzg_model_solve_duals(const dzg_model *md, const dzg_opts *opts, dzg_model_result *res,
                                     dzg_model_duals *du)
{
    if (!du) return dzg_set_error(DZG_E_ARG, "model duals: du is NULL");
    if (!res || !valid(md)) return dzg_set_error(DZG_E_ARG, "model duals: res is NULL or the model is malformed");
    if (md->ncons > 0 && !du->con_dual) return dzg_set_error(DZG_E_ARG, "model duals: con_dual is NULL");
    return model_solve(md, opts, res, du, true);
}

// The batch form of dzg_model_solve.  The routing rule lives here and only here: a model that
// dzg_model_solve would solve in STRICT numerics (STRICT asked for, or AUTO at m <= auto_strict_rows)
// on a dense block of at most DZG_BATCH_MAX_ROWS rows goes into one dzg_batch_solve call; every
// other model goes through dzg_model_solve by itself.  The standard form and the values are
// extracted exactly as dzg_model_solve extracts them.
static int model_solve_batch(const dzg_model *models, int64_t count, const dzg_opts *opts,
                             dzg_model_result *res, dzg_model_duals *du, bool want_duals,
                             const dzg_model_ranging_req *mreq = nullptr, dzg_ranging *rg = nullptr,
                             dzg_model_ray *ry = nullptr, bool fast = false)
{
    if (count > 0 && want_duals && rg && !mreq) return dzg_set_error(DZG_E_ARG, "model batch: req is NULL");
    if (count < 0) return dzg_set_error(DZG_E_ARG, "model batch: count < 0");
    if (count > 0 && (!models || !res)) return dzg_set_error(DZG_E_ARG, "model batch: models or res is NULL");
    if (count > 0 && want_duals && !du) return dzg_set_error(DZG_E_ARG, "model batch: du is NULL");
    for (int64_t i = 0; want_duals && i < count; ++i)
        if (models[i].ncons > 0 && !du[i].con_dual)
            return dzg_set_error(DZG_E_ARG, "model batch: du[" + std::to_string(i) + "].con_dual is NULL");
    for (int64_t i = 0; i < count; ++i)
        if (!valid(&models[i]))
            return dzg_set_error(DZG_E_ARG, "model batch: models[" + std::to_string(i) + "] is malformed");
    for (int64_t i = 0; ry && i < count; ++i)
        if (!ray_arrays_ok(&models[i], &ry[i]))
            return dzg_set_error(DZG_E_ARG, "model batch: ry[" + std::to_string(i) + "]: var, con, lb or ub is NULL");
    dzg_opts o;
    if (opts) o = *opts; else dzg_opts_default(&o);
    std::vector<Built> built((size_t)count);
    std::vector<int64_t> batched;
    for (int64_t i = 0; i < count; ++i) {
        Built &b = built[(size_t)i];
        build(&models[i], b, true);
        const bool strict = dzg_opts_numerics(o, b.m) == DZG_NUMERICS_STRICT;
        if (strict && !b.sparse && b.m <= DZG_BATCH_MAX_ROWS) batched.push_back(i);
    }
    std::vector<CoreRanging> crs((size_t)(rg ? count : 0));
    for (int64_t i = 0; rg && i < count; ++i) {
        std::string why;
        if (!map_ranging_req(&models[i], built[(size_t)i], &mreq[i], crs[(size_t)i], why))
            return dzg_set_error(DZG_E_ARG, "model batch: models[" + std::to_string(i) + "]: " + why);
    }
    const size_t nb = batched.size();
    std::vector<dzg_ranging_req> breq(rg ? nb : 0);
    std::vector<dzg_ranging> brg(rg ? nb : 0);
    std::vector<dzg_lp> lps(nb);
    std::vector<dzg_result> rs(nb);
    std::vector<std::vector<int64_t>> basis(nb);
    std::vector<std::vector<double>> x(nb);
    std::vector<std::vector<double>> yv(want_duals ? nb : 0);
    std::vector<dzg_duals> cores(want_duals ? nb : 0);
    std::vector<std::vector<double>> ray_d(ry ? nb : 0), ray_y(ry ? nb : 0);
    std::vector<dzg_ray> rays(ry ? nb : 0);
    for (size_t k = 0; k < nb; ++k) {
        const Built &b = built[(size_t)batched[k]];
        dzg_lp &lp = lps[k];
        std::memset(&lp, 0, sizeof(lp));
        lp.m = b.m;
        lp.n = b.n;
        lp.n_struct = b.ns;
        lp.a = b.a.data();
        lp.lda = b.m > 0 ? b.m : 1;
        lp.var_col = b.var_col.data();
        lp.c = b.c.data();
        lp.constant = b.constant;
        lp.basis = b.basis.data();
        lp.nonbasis = b.nonbasis.data();
        lp.x = b.x.data();
        lp.z = b.z.data();
        basis[k].assign((size_t)(b.m ? b.m : 1), 0);
        x[k].assign((size_t)(b.m ? b.m : 1), 0.0);
        std::memset(&rs[k], 0, sizeof(dzg_result));
        rs[k].basis = basis[k].data();
        rs[k].x = x[k].data();
        if (want_duals) {
            yv[k].assign((size_t)(b.m ? b.m : 1), 0.0);
            std::memset(&cores[k], 0, sizeof(dzg_duals));
            cores[k].y = yv[k].data();
            cores[k].d = du[batched[k]].core.d;
        }
        if (rg) {
            breq[k] = crs[(size_t)batched[k]].req;
            brg[k] = rg[batched[k]];
        }
        if (ry) {
            ray_d[k].assign((size_t)(b.n ? b.n : 1), 0.0);
            ray_y[k].assign((size_t)(b.m ? b.m : 1), 0.0);
            std::memset(&rays[k], 0, sizeof(dzg_ray));
            rays[k].d = ray_d[k].data();
            rays[k].y = ray_y[k].data();
        }
    }
    if (nb > 0 && fast) { // (plain solves only) the shared batch in FAST numerics under the AUTO policy
        dzg_opts of = o;
        of.numerics = DZG_NUMERICS_AUTO;
        const int rc = dzg_batch_solve_fast(lps.data(), (int64_t)nb, &of, 0, 0, rs.data());
        if (rc < 0) return rc;
    } else if (nb > 0) {
        const int rc = ry ? dzg_batch_solve_rays(lps.data(), (int64_t)nb, &o, 0, rs.data(),
                                                 want_duals ? cores.data() : nullptr, rays.data())
                     : rg ? dzg_batch_solve_ranging(lps.data(), (int64_t)nb, &o, 0, breq.data(), rs.data(),
                                                    cores.data(), brg.data())
                     : want_duals ? dzg_batch_solve_duals(lps.data(), (int64_t)nb, &o, 0, rs.data(), cores.data())
                                  : dzg_batch_solve(lps.data(), (int64_t)nb, &o, 0, rs.data());
        if (rc < 0) return rc;
    }
    size_t k = 0;
    for (int64_t i = 0; i < count; ++i) {
        dzg_model_result &out = res[i];
        if (k < nb && batched[k] == i) {
            const Built &b = built[(size_t)i];
            const dzg_result &r = rs[k];
            out.status = r.status;
            out.numerics_used = r.numerics_used;
            out.iterations = r.iterations;
            out.objective = r.objective;
            out.m = b.m;
            out.n = b.n;
            out.near_ties = r.near_ties;
            out.first_near_tie = r.first_near_tie;
            if (out.values) solution_values(&models[i], b, basis[k].data(), x[k].data(), out.values);
            if (want_duals)
                adopt_duals(&models[i], b, r.status, r.objective, cores[k], yv[k].data(), &du[i]);
            if (ry) adopt_ray(&models[i], b, rays[k], ray_d[k].data(), ray_y[k].data(), &ry[i]);
            ++k;
            continue;
        }
        const int rc = model_solve(&models[i], opts, &out, want_duals ? &du[i] : nullptr, want_duals,
                                   rg ? &mreq[i] : nullptr, rg ? &rg[i] : nullptr, ry ? &ry[i] : nullptr);
        if (rc < 0) return rc;
    }
    return 0;
}

extern "C" int dzg_model_solve_batch(const dzg_model *models, int64_t count, const dzg_opts *opts,
                                     dzg_model_result *res)
{
    return model_solve_batch(models, count, opts, res, nullptr, false);
}

extern "C" int dzg_model_solve_batch_fast(const dzg_model *models, int64_t count, const dzg_opts *opts,
                                          dzg_model_result *res)
{
    return model_solve_batch(models, count, opts, res, nullptr, false, nullptr, nullptr, nullptr, true);
}

extern "C" int dzg_model_solve_batch_duals(const dzg_model *models, int64_t count, const dzg_opts *opts,
                                           dzg_model_result *res, dzg_model_duals *du)
{
    return model_solve_batch(models, count, opts, res, du, true);
}

extern "C" int dzg_model_solve_ranging(const dzg_model *md, const dzg_opts *opts,
                                       const dzg_model_ranging_req *req, dzg_model_result *res,
                                       dzg_model_duals *du, dzg_ranging *rg)
{
    if (!du || !req || !rg) return dzg_set_error(DZG_E_ARG, "model ranging: req, du or rg is NULL");
    if (!res || !valid(md)) return dzg_set_error(DZG_E_ARG, "model ranging: res is NULL or the model is malformed");
    if (md->ncons > 0 && !du->con_dual) return dzg_set_error(DZG_E_ARG, "model ranging: con_dual is NULL");
    return model_solve(md, opts, res, du, true, req, rg);
}

extern "C" int dzg_model_solve_batch_ranging(const dzg_model *models, int64_t count, const dzg_opts *opts,
                                             const dzg_model_ranging_req *req, dzg_model_result *res,
                                             dzg_model_duals *du, dzg_ranging *rg)
{
    if (count > 0 && (!req || !rg)) return dzg_set_error(DZG_E_ARG, "model batch: req or rg is NULL");
    return model_solve_batch(models, count, opts, res, du, true, req, rg);
}

extern "C" int dzg_model_solve_rays(const dzg_model *md, const dzg_opts *opts, dzg_model_result *res,
                                    dzg_model_duals *du, dzg_model_ray *ry)
{
    if (!ry) return dzg_set_error(DZG_E_ARG, "model rays: ry is NULL");
    if (!res || !valid(md)) return dzg_set_error(DZG_E_ARG, "model rays: res is NULL or the model is malformed");
    if (du && md->ncons > 0 && !du->con_dual) return dzg_set_error(DZG_E_ARG, "model rays: con_dual is NULL");
    if (!ray_arrays_ok(md, ry)) return dzg_set_error(DZG_E_ARG, "model rays: var, con, lb or ub is NULL");
    return model_solve(md, opts, res, du, du != nullptr, nullptr, nullptr, ry);
}

extern "C" int dzg_model_solve_batch_rays(const dzg_model *models, int64_t count, const dzg_opts *opts,
                                          dzg_model_result *res, dzg_model_duals *du, dzg_model_ray *ry)
{
    if (count > 0 && !ry) return dzg_set_error(DZG_E_ARG, "model batch: ry is NULL");
    return model_solve_batch(models, count, opts, res, du, du != nullptr, nullptr, nullptr, ry);
}
