"""Shared pieces of the re-optimisation tests (tests/test_reopt_host.py, tests/test_gpu_reopt.py):
the constant the FAST restart state is held to, and the changed LPs that stay solvable.

Generator G1 gives b = A x0 + rb and c = A^T y0 - rc with rb, rc >= 0, so b' = b + d with d >= 0 and
c' = c - e with e >= 0 keep the LP feasible and bounded (x0 stays feasible, y0 stays dual feasible).

The restart state of dzg_solver_reoptimize in FAST numerics is x = B^-1 b' and z = N^T B^-T c'_B - c'_N
from a fresh inverse.  It is compared with the state the basis defines for the CHANGED LP, in long
double (state_check.exact_state with the slack start of (a, b', c')), in Exact.drift's metric over x
and z: D = max over the two of ||v - v^||_inf / max(1, ||v^||_inf).  C_RESTART is 10x the worst D an
MI355X showed over the shapes of test_gpu_reopt.py (C_RESTART_OBSERVED; pytest -s prints them):
state_check.py's rule for C_STATE."""
from __future__ import annotations

import numpy as np

C_RESTART_OBSERVED = {"37x53 odd k": 1.631e-16, "37x53 even k": 1.857e-16, "37x53 slack basis": 0.0,
                      "300x500 three launches": 6.399e-14, "300x500 seven launches": 6.399e-14,
                      "640x1280": 3.418e-13}
C_RESTART = 3.5e-12


def restart_drift(exact, state) -> dict:
    """Exact.drift over x and z only (xbar and zbar are exactly one after a reoptimise)."""
    d = exact.drift(state)
    return {"x": d["x"], "z": d["z"], "D": max(d["x"], d["z"])}


def moved(seed: int, b, c, rows=None, cols=None, scale: float = 1.0):
    """(b + d, c - e) with d, e uniform in [0, scale) on `rows` / `cols` (None: all) and 0 elsewhere."""
    rng = np.random.default_rng(seed)
    b, c = np.asarray(b, dtype=np.float64), np.asarray(c, dtype=np.float64)
    d, e = np.zeros(len(b)), np.zeros(len(c))
    rows = np.arange(len(b)) if rows is None else np.asarray(rows, dtype=np.int64)
    cols = np.arange(len(c)) if cols is None else np.asarray(cols, dtype=np.int64)
    d[rows] = scale * rng.random(len(rows))
    e[cols] = scale * rng.random(len(cols))
    return b + d, c - e


def slack_start(a, b, c) -> dict:
    """The slack start of CoreLP.from_inequality_form(a, b, c) as a mapping (no GPU needed)."""
    m, ns = np.asarray(a).shape
    return dict(basis=np.arange(ns, ns + m), nonbasis=np.arange(ns), x=np.asarray(b, dtype=np.float64),
                xbar=None, z=-np.asarray(c, dtype=np.float64), zbar=None)
