"""The CPU oracle's carried state (basis, nonbasis, x, xbar, z, zbar) at a few stops of the
512 x 1024 seed-2001 solve, written to tests/golden/oracle_states_2001_512x1024.npz.

The state is what the reference's own rounding leaves after P pivots; tests/test_state_check.py
measures how far it is from the state its basis defines (tests/state_check.py) and
tests/test_gpu_state.py compares that with FAST's state at the same pivots.  The blocked twin of
the oracle (bit-equal to the literal one) runs the solve from stop to stop: the oracle keeps
nothing between iterations but this state, so resuming from it continues the same solve -- the
pivots of every leg are checked against the committed pivot log of that solve.

Run: python tests/golden/make_oracle_states.py
"""
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
from dantzig_amd import core  # noqa: E402  (host-side generator only, no GPU needed)
from oracle import oracle as ora  # noqa: E402

SEED, M, NS = 2001, 512, 1024
STOPS = (1000, 4000, 7692)

if __name__ == "__main__":
    a, b, c = core.gen_dense_lp(seed=SEED, m=M, n_struct=NS)
    log = np.load(os.path.join(ROOT, "tests", "golden", f"oracle_pivots_{SEED}_{M}x{NS}.npz"))
    sf = ora.stdform_from_dense(a, b, c)
    xbar = zbar = None
    done, out = 0, {}
    for stop in STOPS:
        t = time.time()
        res = ora.simplex_solve(sf, max_iter=stop - done, blocked=True, xbar=xbar, zbar=zbar)
        got = np.array([p[:3] for p in res.pivots], dtype=np.int64).reshape(-1, 3)
        want = np.stack([log["kind"], log["entering"], log["leaving"]], axis=1)[done:stop]
        assert np.array_equal(got, want), f"leg to {stop} left the oracle's pivot log"
        done += res.iterations
        assert done == stop, (done, stop)
        sf.basis, sf.nonbasis, sf.x, sf.z = res.basis, res.nonbasis, res.x, res.z
        xbar, zbar = res.xbar, res.zbar
        for name in ("basis", "nonbasis"):
            out[f"{name}_{stop}"] = np.asarray(getattr(res, name), dtype=np.int16)
        for name in ("x", "xbar", "z", "zbar"):
            out[f"{name}_{stop}"] = np.asarray(getattr(res, name), dtype=np.float64)
        print(f"pivot {stop}: {res.status}, {time.time() - t:.0f} s", flush=True)
    path = os.path.join(ROOT, "tests", "golden", f"oracle_states_{SEED}_{M}x{NS}.npz")
    np.savez_compressed(path, seed=SEED, m=M, n_struct=NS, stops=np.array(STOPS), **out)
    print(path, os.path.getsize(path), "bytes")
