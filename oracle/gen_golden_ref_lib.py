"""oracle/gen_golden_ref_lib.py -- generates tests/golden/ot_ref_library.npz FROM THE REFERENCE'S COMPILED LIBRARY.

Runs only where oracle/_ref/libot_ref.so was built (`make -C oracle`, which needs the reference tree).  It records the
inputs and outputs of the library's update_k_double + update_process_double on seeded random problems, so that
tests/test_oracle_ot.py::test_against_compiled_reference_library can check the oracle against them anywhere.  The
fixture is data (inputs + expected outputs); no reference source is written anywhere.

    python oracle/gen_golden_ref_lib.py
"""
import ctypes
import os
import sys

import numpy as np

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")
sys.path.insert(0, ROOT)
from oracle import ot_oracle  # noqa: E402

OUT = os.path.join(ROOT, "tests", "golden", "ot_ref_library.npz")
SHAPES = [(5, 9), (64, 33), (130, 257)]
# eps, lambda1, lambda2, tau (tau = 3 forces an absorb on these inputs)
PARAMS = (0.2, 0.1, 5.0, 3.0)


def problems(seed=7):
    rng = np.random.default_rng(seed)
    for (m, n) in SHAPES:
        C = rng.uniform(0, 4, size=(m, n)); u = rng.normal(size=m) * .2; v = rng.normal(size=n) * .2
        p = rng.uniform(.5, 2, size=m)
        yield m, n, C, u, v, p


def run_reference(L, C, u, v, p):
    m, n = C.shape
    eps, l1, l2, tau = PARAMS
    D = ctypes.POINTER(ctypes.c_double)
    P = lambda x: x.ctypes.data_as(D)
    cd = ctypes.c_double
    al1, al2 = l1 / (l1 + eps), l2 / (l2 + eps)
    dx, dy = np.ones(m) / m, np.ones(n) / n
    q = np.ones(n) * p.mean()
    K = np.zeros((m, n)); Kb = np.zeros((m, n)); R = np.zeros((m, n))
    a, b, oa, ob = np.ones(m), np.ones(n), np.ones(m), np.ones(n)
    uu, vv = u.copy(), v.copy()
    L.update_k_double(P(K), P(Kb), P(C), P(uu), P(vv), cd(eps), m, n)
    gap = L.update_process_double(P(R), P(a), P(b), P(oa), P(ob), P(K), P(Kb), P(C), P(dx), P(dy), P(p), P(q), P(uu),
                                  P(vv), 5, 5, 5, cd(eps), cd(1e-8), cd(tau), cd(l1), cd(l2), cd(al1), cd(al2), 0, 10 ** 7,
                                  m, n)
    return dict(K=K, R=R, a=a, b=b, u_out=uu, v_out=vv, gap=np.float64(gap))


def main():
    L = ot_oracle.ref_lib()
    if L is None:
        raise SystemExit("oracle/_ref/libot_ref.so is not built: run `make -C oracle` where the reference tree is present")
    rec = {"shapes": np.array(SHAPES, dtype=np.int64), "params": np.array(PARAMS)}
    for m, n, C, u, v, p in problems():
        tag = f"{m}x{n}"
        rec.update({f"{tag}_C": C, f"{tag}_u": u, f"{tag}_v": v, f"{tag}_p": p})
        rec.update({f"{tag}_{k}": x for k, x in run_reference(L, C, u, v, p).items()})
    np.savez_compressed(OUT, **rec)
    print("wrote", os.path.relpath(OUT, ROOT), sum(x.nbytes for x in rec.values()), "bytes of arrays")


if __name__ == "__main__":
    main()
