"""One Sinkhorn scaling iteration and the tau-absorb, restated in plain numpy from the formulas (ot_func.cpp:610-668, :792-814):

    a'_i = (p_i / sum_j K_ij b_j dy_j)^(l1/(l1+eps)) * exp(-u_i/(l1+eps))
    b'_j = (q_j / sum_i K_ij a'_i dx_i)^(l2/(l2+eps)) * exp(-v_j/(l2+eps))
    absorb (when max(a', b') > tau):  u += eps ln a ; v += eps ln b ; a = b = 1 ; K_ij = exp((u_i + v_j - C_ij)/eps)

Sums, powers and exponentials are carried in np.longdouble (64-bit mantissa on x86: a sum of n positive terms is off by at most
n * 2^-64) and rounded to fp64 once.  Nothing here calls the library; tests/test_ot_pass_ref_cpu.py ties it to the C oracle."""
import numpy as np

LD = np.longdouble
ROW_BLOCK = 128         # rows widened to longdouble at a time (bounds the temporary to ROW_BLOCK x J x 16 bytes)


def ref_iteration(a, b, K, dx, dy, p, q, u, v, l1, l2, eps, w_fp32=False, a_col=None, columns_only=False):
    """Returns a', b', old_a', old_b', max(a'), max(b').  w_fp32: w = b.dy is rounded to fp32 before the row sums (what the two
    widest fp32 geometries document).  a_col: the a' that enters the column sums (default: this function's own a'), so that
    a test can give the device's a' and judge b' on its own; with columns_only the row sums are skipped and a' = a_col."""
    I, J = K.shape
    al1, al2 = LD(l1) / (LD(l1) + LD(eps)), LD(l2) / (LD(l2) + LD(eps))
    w = np.asarray(b, np.float64) * np.asarray(dy, np.float64)
    if w_fp32:
        w = w.astype(np.float32)
    w = w.astype(LD)
    pL, uL, dxL = np.asarray(p).astype(LD), np.asarray(u).astype(LD), np.asarray(dx).astype(LD)
    a_new = np.empty(I, np.float64)
    t = np.zeros(J, LD)
    for r0 in range(0, I, ROW_BLOCK):
        r1 = min(I, r0 + ROW_BLOCK)
        Kb = K[r0:r1].astype(LD)
        if columns_only:
            a_new[r0:r1] = a_col[r0:r1]
        else:
            s = Kb @ w
            an = (pL[r0:r1] / s) ** al1 * np.exp(-uL[r0:r1] / (LD(l1) + LD(eps)))
            a_new[r0:r1] = an.astype(np.float64)
        ac = a_new[r0:r1] if a_col is None else np.asarray(a_col[r0:r1], np.float64)
        t += (ac.astype(LD) * dxL[r0:r1]) @ Kb
    bn = (np.asarray(q).astype(LD) / t) ** al2 * np.exp(-np.asarray(v).astype(LD) / (LD(l2) + LD(eps)))
    b_new = bn.astype(np.float64)
    return a_new, b_new, np.array(a, np.float64), np.array(b, np.float64), float(a_new.max()), float(b_new.max())


def ref_absorb(a, b, u, v, C, eps):
    """Returns u', v', a' = 1, b' = 1, K' of the absorb."""
    u2 = (np.asarray(u).astype(LD) + LD(eps) * np.log(np.asarray(a).astype(LD))).astype(np.float64)
    v2 = (np.asarray(v).astype(LD) + LD(eps) * np.log(np.asarray(b).astype(LD))).astype(np.float64)
    K = np.empty(C.shape, np.float64)
    for r0 in range(0, C.shape[0], ROW_BLOCK):
        r1 = min(C.shape[0], r0 + ROW_BLOCK)
        # the argument in longdouble, rounded once (|arg| < 64: 7e-15 absolute, so 7e-15 relative on K), then one fp64 exp
        arg = (u2[r0:r1, None].astype(LD) + v2[None, :].astype(LD) - C[r0:r1].astype(LD)) / LD(eps)
        K[r0:r1] = np.exp(arg.astype(np.float64))
    return u2, v2, np.ones(len(a)), np.ones(len(b)), K


def ref_step(a, b, K, C, dx, dy, p, q, u, v, l1, l2, eps, tau, iters):
    """`iters` iterations, each followed by the absorb when a scaling exceeds tau (ot_func.cpp:689-828).  Returns a dict of the
    state (a, b, old_a, old_b, K, u, v), the number of absorbs and, per iteration, (max a', max b') before any absorb."""
    a, b, u, v, K = (np.array(x, np.float64) for x in (a, b, u, v, K))
    old_a, old_b, absorbs, maxima = a.copy(), b.copy(), 0, []
    for _ in range(iters):
        a, b, old_a, old_b, ma, mb = ref_iteration(a, b, K, dx, dy, p, q, u, v, l1, l2, eps)
        maxima.append((ma, mb))
        if max(ma, mb) > tau:
            u, v, a, b, K = ref_absorb(a, b, u, v, C, eps)
            absorbs += 1
    return dict(a=a, b=b, old_a=old_a, old_b=old_b, K=K, u=u, v=v, absorbs=absorbs, maxima=maxima)


def two_largest(*vectors):
    """The two largest entries of the vectors together, largest first."""
    x = np.concatenate([np.ravel(v) for v in vectors])
    if x.size == 1:
        return float(x[0]), float(x[0])
    top = np.partition(x, x.size - 2)[-2:]
    return float(top[1]), float(top[0])
