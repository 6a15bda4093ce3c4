// opts.h -- what a dzg_opts means, for every entry point of the library (.hip and host-compiled alike).
// The defaults themselves are dzg_opts_default's (engine.hip) and are written nowhere else.
#pragma once

#include "../../include/dantzig_amd.h"

// `opts` (NULL: the defaults) with every field that reads as "unset" at its default.  A C host may hand
// over a zero-filled struct: zero -- for the counts anything <= 0 -- is "unset" in these five fields.
// (dzg_solver_create keeps the outcome as the solver's own options; the entry points that pass the
// caller's options on pass them on as they came and read single fields through this.)
inline dzg_opts dzg_opts_resolved(const dzg_opts *opts)
{
    dzg_opts def;
    dzg_opts_default(&def);
    if (!opts) return def;
    dzg_opts o = *opts;
    if (o.max_iter <= 0) o.max_iter = def.max_iter;
    if (o.poll_interval <= 0) o.poll_interval = def.poll_interval;
    if (o.epsilon == 0.0) o.epsilon = def.epsilon;
    if (o.auto_strict_rows <= 0) o.auto_strict_rows = def.auto_strict_rows;
    if (o.tie_tol == 0.0) o.tie_tol = def.tie_tol;
    return o;
}

// The numerics a solve of `m` rows runs under `o` (resolved or not): AUTO is STRICT up to
// auto_strict_rows rows and FAST above.
inline int dzg_opts_numerics(const dzg_opts &o, int64_t m)
{
    if (o.numerics != DZG_NUMERICS_AUTO) return o.numerics;
    return m <= dzg_opts_resolved(&o).auto_strict_rows ? DZG_NUMERICS_STRICT : DZG_NUMERICS_FAST;
}
