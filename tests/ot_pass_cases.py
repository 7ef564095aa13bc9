"""Shapes and inputs for the Sinkhorn pass tests: every register-tile width of the fused pass, the band shapes its row loop
distinguishes, one band longer than the workgroup, and the two-sweep kernels' loop tails.

`fused_geometry_expected` restates the rule of choose_fused (csrc/ot_sinkhorn.hip) and `chunks_expected` that of
choose_chunks; every GPU case asserts OTSolver.fused_geometry() against the former before it looks at a value, so a case cannot
test another band shape than it names.  I depends on the number of compute units (the pass runs one workgroup per CU): the GPU
tests read it from the device, tests/test_ot_pass_ref_cpu.py uses CPU_CUS."""
import numpy as np

CPU_CUS = 256
THREADS = 512                       # workgroup of the fused pass
LDS_LIMIT = 160 * 1024
VEC = {"f32": 4, "f64": 2}          # elements of a 16-byte vector
ELT = {"f32": 4, "f64": 8}
MAX_VPT = {"f32": 10, "f64": 12}
TWO_ROW_MAX = {"f32": 5, "f64": 6}  # widest vpt with two rows per group
# The passes from an arbitrary state (make_state).  One pass, tau = 1e9: with one row or one column nothing averages, a
# kernel entry near e^-21 meets the scaling alone and (p / s)^alpha stays below tau only for moderate alpha: 0.6 and 0.5 give
# at most 1.6e6 over the table.  The absorb and the exact stage: alpha1 = 0.96 keeps the factor 50 on p of the last row
# (50^alpha1 = 43) above b', whose scale is (q / sum_i K a' dx)^alpha2 ~ 2 e^(-v/eps), and makes the stage take 40 iterations.
EPS, L1, L2 = 0.2, 0.3, 0.2
ABSORB_L1, ABSORB_L2 = 5.0, 2.0
TAU_OFF = 1e9

ZERO_GEOMETRY = dict(vpt=0, rows_per_group=0, workgroups=0, rows_per_workgroup=0)


def round_up(x, m):
    return (x + m - 1) // m * m


def rows_per_group(storage, vpt):
    return 2 if vpt <= TWO_ROW_MAX[storage] else 1


def fused_geometry_expected(I, J, storage, cus, no_fused=False):
    """What OTSolver(I, J, storage).fused_geometry() must report on a device with `cus` compute units, plus 'lds' (bytes of
    dynamic LDS of the pass) and 'ld'.  All zeros when the two-sweep kernels are used."""
    ld = round_up(J, 64)
    out = dict(ZERO_GEOMETRY, lds=0, ld=ld)
    if no_fused:
        return out
    V = VEC[storage]
    vpt = (ld + V * THREADS - 1) // (V * THREADS)
    if vpt > MAX_VPT[storage]:
        return out
    wbytes = 4 if (storage == "f32" and vpt > 8) else 8
    R = rows_per_group(storage, vpt)
    lds = wbytes * vpt * THREADS * V + 8 * (2 * (THREADS // 64) * R) + 8
    if lds + 4096 > LDS_LIMIT:
        return out
    blocks = max(1, min(cus, (I + 2 * R - 1) // (2 * R)))
    rpb = round_up((I + blocks - 1) // blocks, R)
    blocks = (I + rpb - 1) // rpb
    lds += 8 * 4 * rpb
    if lds > LDS_LIMIT:
        return out
    return dict(vpt=vpt, rows_per_group=R, workgroups=blocks, rows_per_workgroup=rpb, lds=lds, ld=ld)


def public_geometry(g):
    """The four entries OTSolver.fused_geometry() returns."""
    return {k: g[k] for k in ZERO_GEOMETRY}


def chunks_expected(I, J, storage):
    """(rows per chunk, chunks) of the two-sweep column pass."""
    V = VEC[storage]
    gx = (round_up(J, 64) + 256 * V - 1) // (256 * V)
    want = min(max(1, 2048 // gx), max(1, I // 16))
    rpc = (I + want - 1) // want
    return rpc, (I + rpc - 1) // rpc


def band_groups(g, I):
    """Groups in the full bands and in the last band, and rows in the last group of the last band."""
    R, rpb = g["rows_per_group"], g["rows_per_workgroup"]
    last = I - (g["workgroups"] - 1) * rpb
    return rpb // R, (last + R - 1) // R, last - ((last + R - 1) // R - 1) * R


def loop_rounds_and_tail(n):
    """A band of n groups in k_fused_pass / k_fused_rowdot: (rounds of the two-group double-buffer loop, groups in the tail).
    The loop runs while more than three groups are left."""
    rounds = 0
    while n > 3:
        n -= 2
        rounds += 1
    return rounds, n


# ------------------------------------------------------------------------------------------------ the case table
# A case is a dict: name, storage, I, J, no_fused, kind.  Specs (what pytest parametrises over) carry no I; `resolve` makes
# the case for a CU count.

def width_J(storage, vpt, which):
    """'lo': one 64-column block into tile `vpt` (every vector slot of the last tile but one block clamped, 63 pad columns);
    'hi': the full tile, whose last 64-block holds one real column."""
    V = VEC[storage]
    return (vpt - 1) * V * THREADS + 1 if which == "lo" else vpt * V * THREADS - 63


WIDTH_SPECS = [("width", st, vpt, which) for st in ("f64", "f32") for vpt in range(1, MAX_VPT[st] + 1) for which in ("lo", "hi")]
# band shapes: groups per band 1, 2, 3, 4, 6; I = 1, 2R, 2R + 1
BAND_VPT = {"f64": (1, 7), "f32": (1, 6)}
BAND_SHAPES = ("g1", "g2", "g3", "g4", "g6", "i1", "i2r", "i2r1")
BAND_SPECS = [("band", st, vpt, sh) for st in ("f64", "f32") for vpt in BAND_VPT[st] for sh in BAND_SHAPES]
LONG_SPEC = ("long", "f64", 1, "513")
# two-sweep: (I, J, forced).  ld / (64 V) below 1, odd, even, odd with a loop trip, fractional; rows_per_chunk % 4 = 1, 3, 2, 0
# with a short last chunk; I < 16 = one chunk; the natural fall-back past the widest tile.
TWO_SWEEP = {"f64": [(33, 128, True), (37, 256, True), (35, 384, True), (47, 130, True), (9, 40, True), (37, 12289, False)],
             "f32": [(33, 256, True), (37, 512, True), (35, 768, True), (47, 300, True), (9, 40, True), (37, 20481, False)]}
TWO_SWEEP_SPECS = [("sweep", st, k, "forced" if c[2] else "natural") for st in ("f64", "f32") for k, c in enumerate(TWO_SWEEP[st])]


def spec_id(spec):
    return "-".join(str(x) for x in spec)


def resolve(spec, cus):
    kind, st, x, y = spec
    no_fused = False
    if kind == "width":
        R = rows_per_group(st, x)
        I, J = cus * 4 * R + 3, width_J(st, x, y)       # five groups a band (one steady round + a tail of three); short last band
    elif kind == "band":
        R = rows_per_group(st, x)
        J = width_J(st, x, "lo") if x > 1 else 100      # vpt 1: two 64-blocks, most vector slots clamped
        if y[0] == "g":
            g = int(y[1:])
            # g == 1 needs a single band (a band holds at least two groups otherwise); else every band g groups and the last
            # one row short: an odd row in a two-row group, a short band of one-row groups
            I = R if g == 1 else cus * g * R - 1
        else:
            I = {"i1": 1, "i2r": 2 * R, "i2r1": 2 * R + 1}[y]
    elif kind == "long":
        I, J = cus * 513 + 1, 64
    else:
        I, J, forced = TWO_SWEEP[st][x]
        no_fused = forced
    return dict(name=spec_id(spec), kind=kind, storage=st, I=I, J=J, no_fused=no_fused, vpt=x if kind in ("width", "band", "long") else 0)


def make_state(I, J, seed, boost_last=False):
    """Test 1's arbitrary state: a, b in (0.5, 2), u, v ~ 0.2 N(0, 1), p in (0.5, 2), q = mean p, C uniform in (0, 4),
    K = exp((u + v - C)/eps) at eps = EPS.  boost_last multiplies p of the last row by 50."""
    rng = np.random.default_rng(seed)
    a, b = rng.uniform(0.5, 2.0, I), rng.uniform(0.5, 2.0, J)
    u, v = 0.2 * rng.normal(size=I), 0.2 * rng.normal(size=J)
    p = rng.uniform(0.5, 2.0, I)
    if boost_last:
        # a'_i ~ (p_i / S)^alpha1 e^(-u_i/eps) with S nearly the same for every row (K carries e^(u_i/eps)): the factor 50 on p
        # alone does not lift the last row above the e^(-u/eps) spread of a thousand rows, so the last row also takes the
        # sample's smallest u (a swap: the sample stays what it was)
        k = int(np.argmin(u))
        u[k], u[-1] = u[-1], u[k]
        p[-1] *= 50.0
    q = np.full(J, p.mean())
    C = rng.uniform(0.0, 4.0, (I, J))
    K = np.exp((u[:, None] + v[None, :] - C) / EPS)
    return dict(a=a, b=b, u=u, v=v, p=p, q=q, C=C, K=K, dx=np.full(I, 1.0 / I), dy=np.full(J, 1.0 / J))


def seed_of(case):
    return 1000 * (case["I"] % 9973) + case["J"]
