// mip_internal.h -- library-internal seams of the MILP search (not part of the C ABI):
//   * the standard-form builder of model.cpp (Simplex::new), used by mip.cpp to make a structure;
//   * the node-LP solver of k_mip.hip, called by mip.cpp once per round.
#pragma once

#include <cmath>
#include <cstdint>
#include <vector>

#include "../../include/dantzig_amd.h"

namespace dzg_internal {

struct Built {
    int64_t m = 0, n = 0, ns = 0;
    std::vector<double> a; // column-major m x ns, lda = m (dense mode)
    bool sparse = false;   // large, sparse models: structural block kept CSC, never densified
    std::vector<int64_t> col_ptr;
    std::vector<int32_t> row_idx;
    std::vector<double> val;
    std::vector<int64_t> var_col, basis, nonbasis, pos_var, neg_var;
    std::vector<double> c, x, z;
    double constant = 0.0;
    // per row: -1 for a user row, 2u for the ub row of user variable u, 2u + 1 for its lb row
    std::vector<int64_t> row_tag;
};

bool valid(const dzg_model *md);
void build(const dzg_model *md, Built &out, bool allow_sparse);
void solution_values(const dzg_model *md, const Built &b, const int64_t *basis, const double *x,
                     double *values);

// ---- k_mip.hip

// A structure: the standard form shared by every node whose integer variables have the same set
// of finite bounds.  Row r's right-hand side is b0[r] when row_int[r] < 0; otherwise it is read
// from the node's bounds, bnd[row_int[r]] (an ub row, odd code) or -bnd[row_int[r]] (an lb row,
// even code), with bnd = {lb_0, ub_0, lb_1, ub_1, ...} over the integer variables.
struct MipStructure {
    int m = 0, n = 0, ns = 0;
    double constant = 0.0;
    std::vector<double> a, b0, c, z0;                  // a: m x ns column-major
    std::vector<int> var_col, row_int, basis0, nonbasis0;
    std::vector<int> pos_var, neg_var;                 // nvars each, -1 if unseen
};

// The kernel's record of one node LP.  branch < 0 when the node is integral (or not OPTIMAL).
struct MipNodeRecord {
    int status;
    int branch;        // index into the integer-variable list, -1: none
    long long iterations;
    double objective;  // constant + sum c[basis[p]] x[p], basis-position order
    double value;      // the branching variable's value
    int integral;
    int warm;                  // 0: cold; 1: warm attempt accepted; 2: rejected and restarted cold
    long long warm_iterations; // the warm attempt's pivots (iterations holds both runs' sum)
    int fast;                  // 0: STRICT only; 1: FAST attempt accepted; 2: FAST rejected, then STRICT
    long long fast_iterations; // the FAST attempt's pivots (iterations holds both runs' sum)
};

// FAST node LPs (dzg_mip_node_opts): the options the control block starts from (tie_tol,
// near_tie_action), pivots per FAST launch and pivots between two inversions inside a launch
// (0: the FAST batch's defaults).
struct MipFastRun {
    const dzg_opts *opts;
    int64_t pivots_per_launch, refactor_every;
};

struct MipGpu; // device arenas, reused across rounds

int mip_gpu_create(MipGpu **out, int device, int nvars, const std::vector<int> &int_vars);
void mip_gpu_destroy(MipGpu *g);
// Registers a structure (uploaded before the next round); returns its id.
int mip_gpu_add_structure(MipGpu *g, MipStructure &&s);
// Solves `count` node LPs: node i uses structure sid[i] and bounds bnd[i * 2 * nint ...].
// pslot (NULL: every node cold): node i's parent-state slot, -1 for a cold node; a node with a
// slot is warm-started from it and restarted cold if the attempt is not accepted.
// rec[i] is filled for every node; values[i * nvars ...] for the integral OPTIMAL ones only.
// fast (NULL: STRICT only): every node gets a FAST attempt first -- warm from its slot's basis and
// nonbasis, else cold -- and the attempts that are not accepted are then solved by the STRICT kernel,
// cold, in the same call.
int mip_gpu_solve_round(MipGpu *g, const int *sid, const int *pslot, const double *bnd, int count,
                        long long max_iter, double eps, int ppl, double int_tol, MipNodeRecord *rec,
                        double *values, const MipFastRun *fast);
// Test hooks (dzg_debug_mip_fast_node): a slot that holds a given basis and nonbasis of structure sid
// (returns the slot; before any save_states), and the final basis, nonbasis, x and z of node idx of
// the last round.
int mip_gpu_plant_slot(MipGpu *g, int sid, const int *basis, const int *nonbasis);
int mip_gpu_read_state(MipGpu *g, int idx, int sid, int *basis, int *nonbasis, double *x, double *z);
// The parent-state pool (warm starts).  A slot holds the final basis, nonbasis and z of one node of
// structure sid; alloc returns -1 if that structure cannot use the pool.  Slots are handed out and
// taken back on the host; save_states copies the final states of nodes of the last round into
// their slots: pairs = {index in that round, slot} x count.
int mip_gpu_slot_alloc(MipGpu *g, int sid);
void mip_gpu_slot_free(MipGpu *g, int slot);
int mip_gpu_save_states(MipGpu *g, const int *pairs, int count);

// The integrality test and the branching rule, shared by the host (sequential route) and the
// device epilogue so that both take the same decision on the same values.
#if defined(__HIPCC__)
__host__ __device__
#endif
inline void mip_branch_choice(const double *values, const int *int_vars, int nint, double int_tol,
                              int *branch, double *value, int *integral)
{
    int best = -1;
    double best_score = -1.0;
    int all = 1;
    for (int k = 0; k < nint; ++k) {
        const double v = values[int_vars[k]];
        if (!(fabs(v - rint(v)) <= int_tol)) all = 0;
        const double f = v - floor(v);
        const double score = fmin(f, 1.0 - f);
        if (score > best_score) {
            best_score = score;
            best = k;
        }
    }
    *integral = all;
    *branch = all ? -1 : best;
    *value = all || best < 0 ? 0.0 : values[int_vars[best]];
}

} // namespace dzg_internal
