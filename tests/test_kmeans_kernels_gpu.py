"""The K-means kernels (spadot_lloyd_step, spadot_kmeanspp_seed, spadot_kmeans_assign) and their driver against the host
reference of tests/kmeans_ref.py, on the inputs of tests/kmeans_inputs.py whose preconditions tests/test_kmeans_ref_cpu.py
proves.  Lattice inputs are compared bit for bit; general inputs within the forward bounds of kmeans_ref.lloyd_step and with
equal labels, rows, flags and counts.  No point, draw or step is excluded anywhere.

Every launch is prepared the hostile way: work spaces, outputs, the padding rows of C and the unused draws are NaN (or a
sentinel integer) beforehand and the data sets are separated by NaN guard rows that no (xoff, npts) covers.

What they are known to catch (each one-line change built once and run against this file on an MI355X; the suite before this
file caught only the third): `d2 <= best` in k_lloyd_assign (the lattice step); an empty cluster set to 0 instead of kept
(lattice step, the 30-dimensional trajectories); k_lloyd_update summing one chunk too few (lattice step, trajectories, flags,
fit); done raised at `sh < tol` (lattice step: tol 0 with a shift of exactly 0); kpp_trials stepping at K >= 22 (lattice and
blob seeding); `run > rv` in the seeding walk (lattice seeding, first at a zero potential).
The lattice centres equal the exact quotients bit for bit: the device's fp64 division is correctly rounded."""
import functools
import warnings

import numpy as np
import pytest
import torch

import kmeans_inputs as ki
import kmeans_ref as ref

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
NAN_BITS = np.array([np.nan]).view(np.int64)[0]
SENTINEL = -77


def _dev(a, dt):
    return torch.as_tensor(np.ascontiguousarray(a), dtype=dt, device=DEV)


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.int64)


def _pack(sets):
    """X = guard, set 0, guard, set 1, ..., guard (NaN guard rows); returns (X device, its host copy, xoff, npts)."""
    d = sets[0].shape[1]
    guard = np.full((1, d), np.nan)
    rows, xoff, at = [guard], [], 1
    for s in sets:
        xoff.append(at)
        rows += [s, guard]
        at += s.shape[0] + 1
    X = np.concatenate(rows)
    return _dev(X, torch.float64), X, _dev(xoff, torch.int32), _dev([s.shape[0] for s in sets], torch.int32)


class Lloyd:
    """One launch configuration of spadot_lloyd_step with hostile buffers; step() runs one iteration, checks what must not
    have been touched and returns host copies of C, inertia and done."""

    def __init__(self, sets, restarts, K_max, tols, done=None):
        from spadot_amd.ops import lloyd_steps
        self.fn = lloyd_steps
        self.X, self.Xh, self.xoff, self.npts = _pack(sets)
        R, d = len(restarts), sets[0].shape[1]
        C = np.full((R, K_max, d), np.nan)
        self.pad = np.ones((R, K_max), dtype=bool)
        for r, (_, C0) in enumerate(restarts):
            C[r, :C0.shape[0]] = C0
            self.pad[r, :C0.shape[0]] = False
        self.C = _dev(C, torch.float64)
        self.rg = _dev([g for g, _ in restarts], torch.int32)
        self.Kr = _dev([C0.shape[0] for _, C0 in restarts], torch.int32)
        self.tol = _dev(tols, torch.float64)
        self.done = _dev(np.zeros(R) if done is None else done, torch.int32)
        self.inertia = _dev(np.full(R, np.nan), torch.float64)
        self.n_max = max(s.shape[0] for s in sets)
        self.part = torch.empty(R * ((self.n_max + 255) // 256) * (K_max * (d + 1) + 1), dtype=torch.float64, device=DEV)

    def step(self, skip_done):
        self.part.fill_(float("nan"))
        self.fn(self.X, self.C, self.xoff, self.npts, self.n_max, self.rg, self.Kr, self.tol, self.done, self.inertia,
                self.part, 1, skip_done=skip_done)
        torch.cuda.synchronize()
        C = self.C.cpu().numpy()
        assert (_bits(C)[self.pad] == NAN_BITS).all(), "padding rows of C were written"
        assert np.isfinite(C[~self.pad]).all()
        assert np.array_equal(_bits(self.X.cpu().numpy()), _bits(self.Xh)), "the data were written"
        return C, self.inertia.cpu().numpy(), self.done.cpu().numpy()


def _seed_launch(sets, probs, K_max, n_max):
    """spadot_kmeanspp_seed on hostile buffers: (idx [P, K_max], centers [P, K_max, d]) on the host."""
    from spadot_amd.ops import kmeanspp_seed
    X, Xh, xoff, npts = _pack(sets)
    U, puoff, at = [np.full(3, np.nan)], [], 3                  # NaN before, between and after the problems' draws
    for p in probs:
        puoff.append(at)
        U += [np.asarray(p["U"], dtype=np.float64), np.full(2, np.nan)]
        at += len(p["U"]) + 2
    P, d = len(probs), sets[0].shape[1]
    idx = torch.full((P, K_max), SENTINEL, dtype=torch.int32, device=DEV)
    centers = torch.full((P, K_max, d), float("nan"), dtype=torch.float64, device=DEV)
    closest = torch.full((P, n_max), float("nan"), dtype=torch.float64, device=DEV)
    i32 = lambda key: _dev([p[key] for p in probs], torch.int32)
    kmeanspp_seed(X, xoff, npts, n_max, i32("g"), i32("k"), i32("first"), _dev(puoff, torch.int32),
                  _dev(np.concatenate(U), torch.float64), K_max, out=(idx, centers, closest))
    torch.cuda.synchronize()
    assert np.array_equal(_bits(X.cpu().numpy()), _bits(Xh)), "the data were written"
    return idx.cpu().numpy(), centers.cpu().numpy()


def _check_seeded(sets, probs, idx, centers, valid=None):
    for j, p in enumerate(probs):
        k, X = p["k"], sets[p["g"]]
        if valid is not None and not valid[j]:
            assert (idx[j] == -1).all() and (_bits(centers[j]) == 0).all(), (j, p["k"], p["first"])
            continue
        rows = ref.seed_rows(X, k, p["first"], p["U"])[0]
        assert idx[j, :k].tolist() == rows.tolist(), (j, p.get("tag"), X.shape, k)
        assert (idx[j, k:] == -1).all() and (_bits(centers[j, k:]) == 0).all()
        assert np.array_equal(_bits(centers[j, :k]), _bits(X[rows])), (j, p.get("tag"))


# ------------------------------------------------------------------------------------------------------ a. one step, exact
@pytest.mark.parametrize("d", ki.LLOYD_DIMS)
def test_lloyd_step_on_the_lattice_is_the_reference_bit_for_bit(d):
    """Centres (member sums exact, one correctly rounded division), inertia (exact) and done, bitwise, for sets of 1 .. 2300
    points x Kr in {1, 2, 7, 20, 32} under one K_max (8 in 30 dimensions), >= 70 restarts in the launch."""
    sets, restarts, K_max = ki.lattice_lloyd(d)
    tols = ki.exact_tols(sets, restarts)
    C, inertia, done = Lloyd(sets, restarts, K_max, tols).step(False)
    for r, (g, C0) in enumerate(restarts):
        _, C_new, want_inertia, shift, want_done, _, _ = ref.lloyd_step(sets[g], C0, tols[g])
        k = C0.shape[0]
        assert np.array_equal(_bits(C[r, :k]), _bits(C_new)), (r, g, k, np.abs(C[r, :k] - C_new).max())
        assert inertia[r] == want_inertia and done[r] == int(want_done), (r, g, k, inertia[r], want_inertia, shift, tols[g])


def test_lloyd_step_of_one_restart():
    sets, restarts, _ = ki.lattice_lloyd(3)
    g, C0 = next((g, C) for g, C in restarts if sets[g].shape[0] == 257 and C.shape[0] == 7)
    C, inertia, done = Lloyd([sets[g]], [(0, C0)], 7, [0.0]).step(True)
    _, C_new, want_inertia, shift, want_done, _, _ = ref.lloyd_step(sets[g], C0, 0.0)
    assert np.array_equal(_bits(C[0]), _bits(C_new)) and inertia[0] == want_inertia and done[0] == int(want_done)


# ------------------------------------------------------------------------------------------------------ b. trajectories
@pytest.mark.parametrize("skip_done", [False, True])
@pytest.mark.parametrize("name", [c[0] for c in ki.GENERAL])
def test_lloyd_trajectory_follows_the_reference_step_by_step(name, skip_done):
    """Every step of every restart: the reference applied to the DEVICE's centres of the step before gives the device's
    centres within `bound`, its inertia (of the centres the step started from) within its bound and the same done flag;
    the iteration count is kmeans_ref.fit's.  A decoy set sits in front so that the set under test has an offset."""
    Xc, tol, C0 = ki.general_case(name)
    R, k, d = C0.shape
    n = Xc.shape[0]
    decoy = np.random.default_rng(9).normal(size=(5, d))
    restarts = [(0, decoy[:2].copy())] + [(1, C0[r]) for r in range(R)]
    L = Lloyd([decoy, Xc], restarts, k, [1e300, tol])
    prev = [C0[r].copy() for r in range(R)]
    was_done = np.zeros(R, dtype=bool)
    n_iter = np.zeros(R, dtype=int)
    last_inertia = np.full(R, np.nan)
    for it in range(1, 301):
        C, inertia, done = L.step(skip_done)
        C, inertia, done = C[1:], inertia[1:], done[1:]
        for r in range(R):
            if was_done[r]:
                assert done[r] == 1 and np.array_equal(_bits(C[r]), _bits(prev[r])), (name, it, r)
                if skip_done:
                    assert _bits(inertia[r]) == _bits(last_inertia[r])
                else:
                    want = float(ref._sum0(ref.assign(Xc, prev[r])[1]))
                    assert abs(inertia[r] - want) <= ref.inertia_bound(n, d, want), (name, it, r)
                continue
            _, C_new, want_inertia, shift, want_done, gap, bound = ref.lloyd_step(Xc, prev[r], tol)
            # (the CPU test's conditions, on the device's own trajectory)
            assert gap.min() >= ki.COND / 2 and abs(shift - tol) >= ki.COND / 2 * tol
            err = np.abs(C[r] - C_new)
            assert (err <= bound).all(), (name, it, r, float((err / np.maximum(bound, 1e-300)).max()))
            assert abs(inertia[r] - want_inertia) <= ref.inertia_bound(n, d, want_inertia), (name, it, r, inertia[r], want_inertia)
            assert done[r] == int(want_done), (name, it, r, shift, tol)
            prev[r], last_inertia[r] = C[r].copy(), inertia[r]
            if want_done:
                was_done[r], n_iter[r] = True, it
        if was_done.all():
            break
    assert was_done.all()
    for r in range(R):
        assert n_iter[r] == ref.fit(Xc, C0[r], tol)[3], (name, r)


# ------------------------------------------------------------------------------------------------------ c. the flags
def test_lloyd_flags_contract():
    """Two copies of one data set, tol 0 and tol huge, one restart each from the same centres (tol is taken per set)."""
    Xc, _, C0 = ki.general_case("separated")
    n, d = Xc.shape
    L = Lloyd([Xc, Xc.copy()], [(0, C0[0]), (1, C0[0])], C0.shape[1], [0.0, 1e300])
    _, C1, inertia0, _, _, _, bound1 = ref.lloyd_step(Xc, C0[0], 0.0)
    ok_inertia = lambda got, want: abs(got - want) <= ref.inertia_bound(n, d, want)

    C, inertia, done = L.step(True)
    assert done.tolist() == [0, 1]
    # the step that raises done still writes its centres; inertia is that of the centres the step STARTED from
    assert (np.abs(C[1] - C1) <= bound1).all() and np.array_equal(_bits(C[0]), _bits(C[1]))
    assert ok_inertia(inertia[0], inertia0) and _bits(inertia[0]) == _bits(inertia[1])
    inertia1 = float(ref._sum0(ref.assign(Xc, C[1])[1]))
    assert inertia1 < inertia0 * (1 - 1e-6) and not ok_inertia(inertia[1], inertia1)
    frozen_C, frozen_inertia = C[1].copy(), inertia[1]

    C2, inertia2, done = L.step(True)                            # skip_done = 1: the done restart keeps centres AND inertia
    assert done.tolist() == [0, 1]
    assert np.array_equal(_bits(C2[1]), _bits(frozen_C)) and _bits(inertia2[1]) == _bits(frozen_inertia)
    assert ok_inertia(inertia2[0], inertia1) and not np.array_equal(C2[0], C[0])      # the live one moved on from C1

    C3, inertia3, done = L.step(False)                           # skip_done = 0: centres kept, inertia of the FINAL centres
    assert done.tolist() == [0, 1]
    assert np.array_equal(_bits(C3[1]), _bits(frozen_C)) and ok_inertia(inertia3[1], inertia1)
    assert ok_inertia(inertia3[0], float(ref._sum0(ref.assign(Xc, C2[0])[1])))

    L.done.fill_(1)                                              # every flag preset, skip_done = 0: no centre changes
    C4, inertia4, done = L.step(False)
    assert done.tolist() == [1, 1] and np.array_equal(_bits(C4), _bits(C3))
    assert ok_inertia(inertia4[0], float(ref._sum0(ref.assign(Xc, C3[0])[1]))) and ok_inertia(inertia4[1], inertia1)


# ------------------------------------------------------------------------------------------------------ d. seeding, exact
@pytest.mark.parametrize("d", ki.SEED_DIMS)
def test_seeding_on_the_lattice_is_the_reference_bit_for_bit(d):
    sets, probs = ki.lattice_seeding(d)
    idx, centers = _seed_launch(sets, probs, 32, max(s.shape[0] for s in sets))
    _check_seeded(sets, probs, idx, centers)


def test_seeding_refuses_invalid_problems_and_leaves_their_neighbours_alone():
    sets, n_max, K_max, probs = ki.invalid_seeding()
    idx, centers = _seed_launch(sets, probs, K_max, n_max)
    _check_seeded(sets, probs, idx, centers, valid=[p["valid"] for p in probs])
    good = [p for p in probs if p["valid"]]
    idx2, centers2 = _seed_launch(sets[:1], good, K_max, n_max)                       # the valid ones on their own
    keep = [j for j, p in enumerate(probs) if p["valid"]]
    assert np.array_equal(idx[keep], idx2) and np.array_equal(_bits(centers[keep]), _bits(centers2))


# ------------------------------------------------------------------------------------------------------ e. seeding, general
def test_seeding_on_blobs_chooses_the_reference_rows():
    sets = ki.seed_general_sets()
    probs = ki.seed_general_problems(sets)
    idx, centers = _seed_launch(sets, probs, 32, max(s.shape[0] for s in sets))
    _check_seeded(sets, probs, idx, centers)


# ------------------------------------------------------------------------------------------------------ f. the whole fit
@functools.lru_cache(maxsize=None)
def _fit_reference():
    """Per (set, k, restart): the host fit from the host seeding on the device-centred data, and sklearn from the same
    seeded centres on the original data."""
    from sklearn.cluster import KMeans
    from spadot_amd.kmeans import sweep_draws
    out = {}
    for t, X in enumerate(ki.fit_sets()):
        x = _dev(X, torch.float64)
        mean = x.mean(0)
        Xc = (x - mean).cpu().numpy()                           # the bits _Plan._seed works on
        tol = ki.tol_of(Xc)
        for k in ki.FIT_KS:
            first, U = sweep_draws(X.shape[0], k, ki.FIT_SEED, ki.FIT_RESTARTS)
            for r in range(ki.FIT_RESTARTS):
                rows = ref.seed_rows(Xc, k, int(first[r]), U[r])[0]
                C, labels, inertia, n_iter, _, _, emptied, bound = ref.fit(Xc, Xc[rows], tol)
                assert n_iter < 300
                with warnings.catch_warnings():
                    warnings.simplefilter("ignore")
                    sk = KMeans(k, init=X[rows], n_init=1, algorithm="lloyd").fit(X)
                out[t, k, r] = dict(C=C, labels=labels, inertia=inertia, n_iter=n_iter, emptied=emptied, sk=sk, bound=bound,
                                    mean=mean.cpu().numpy())
    return out


@pytest.mark.parametrize("path", ["kernel", "torch"])
@pytest.mark.parametrize("check_every", [1, 8])
def test_fit_sweep_is_the_reference_fit_after_the_draws(check_every, path):
    """Everything after the random draws is pinned: every restart's centres and inertia to the host fit, the winner's labels,
    the iteration count, and sklearn started from the same seeded centres (where no cluster emptied: sklearn relocates)."""
    from spadot_amd import kmeans
    want = _fit_reference()
    Xh = ki.fit_sets()
    Xs = [_dev(x, torch.float64) for x in Xh]
    R, T = ki.FIT_RESTARTS, len(Xh)
    plans = [[list(ki.FIT_KS)] * T] if path == "kernel" else [[[k]] * T for k in ki.FIT_KS]
    compared_sklearn = 0
    for ks in plans:
        plan = kmeans._plan(Xs, ks, ki.FIT_SEED, R, 300, 1e-4, check_every, True)      # (fit_sweep's own two lines)
        assert plan.torch_seed == (path == "torch")
        res = plan.run(Xs)
        C_dev = plan.C.cpu().numpy()
        inertia_dev = plan.inertia.cpu().numpy().reshape(len(plan.pairs), R)
        for q, (t, k) in enumerate(plan.pairs):
            n, d = Xh[t].shape
            w = [want[t, k, r] for r in range(R)]
            for r in range(R):
                err = np.abs(C_dev[q * R + r, :k] - w[r]["C"])      # (bound: of the step that wrote the final centres)
                assert (err <= w[r]["bound"]).all(), (t, k, r, float((err / np.maximum(w[r]["bound"], 1e-300)).max()))
                assert abs(inertia_dev[q, r] - w[r]["inertia"]) <= ref.inertia_bound(n, d, w[r]["inertia"]), (t, k, r)
                if not w[r]["emptied"]:
                    assert abs(inertia_dev[q, r] - w[r]["sk"].inertia_) <= 1e-12 * w[r]["sk"].inertia_, (t, k, r)
                    compared_sklearn += 1
            best = int(np.argmin(inertia_dev[q]))                                       # first minimum wins
            ref_in = np.array([x["inertia"] for x in w])
            if np.sort(ref_in)[min(1, R - 1)] - ref_in.min() > 2 * ref.inertia_bound(n, d, ref_in.min()) or R == 1:
                assert best == int(np.argmin(ref_in)), (t, k)
            else:                                                                       # equal optima: the first of them
                assert abs(ref_in[best] - ref_in.min()) <= 2 * ref.inertia_bound(n, d, ref_in.min()), (t, k)
            km = res[t][k]
            assert km.inertia_ == inertia_dev[q, best]
            assert np.array_equal(km.cluster_centers_, C_dev[q * R + best, :k] + w[best]["mean"])
            np.testing.assert_array_equal(km.labels_, w[best]["labels"])
            if not w[best]["emptied"]:
                np.testing.assert_array_equal(km.labels_, w[best]["sk"].labels_)
            slowest = max(x["n_iter"] for x in w)
            assert km.n_iter_ == min(-(-slowest // check_every) * check_every, 300), (t, k, km.n_iter_, slowest)
    assert compared_sklearn >= len(ki.FIT_KS) * T * R // 2


# ------------------------------------------------------------------------------------------------------ g. assign
@pytest.mark.parametrize("dtype", [torch.float32, torch.float64])
def test_kmeans_assign_matches_the_reference(dtype):
    from spadot_amd.ops import kmeans_assign
    npdt = np.float32 if dtype == torch.float32 else np.float64
    for n, k, d in ki.assign_shapes():
        for lattice in (True, False):
            X, C = ki.assign_case(n, k, d, lattice)
            X, C = X.astype(npdt), C.astype(npdt)                # (the reference sees the rounded inputs too)
            got = kmeans_assign(_dev(X, dtype), _dev(C, dtype)).cpu().numpy()
            want = ref.assign(X, C)[0]
            assert got.dtype == np.int32 and np.array_equal(got, want), (n, k, d, lattice, int((got != want).sum()))


# ------------------------------------------------------------------------------------------------------ h. refusals
def _lloyd_args(R, K, d, n=4):
    f = lambda shape, dt, v: torch.full(shape, v, dtype=dt, device=DEV)
    return dict(X=f((n, d), torch.float64, 1.0), C=f((R, K, d), torch.float64, float("nan")),
                xoff=f((1,), torch.int32, 0), npts=f((1,), torch.int32, n), n_max=n, rgroup=f((R,), torch.int32, 0),
                Kr=f((R,), torch.int32, K), tol=f((1,), torch.float64, 0.0), done=f((R,), torch.int32, SENTINEL),
                inertia=f((R,), torch.float64, float("nan")), part=f((R * (K * (d + 1) + 1),), torch.float64, float("nan")))


def _lloyd_refused(a):
    from spadot_amd.ops import lloyd_steps
    with pytest.raises(RuntimeError, match="-22"):
        lloyd_steps(a["X"], a["C"], a["xoff"], a["npts"], a["n_max"], a["rgroup"], a["Kr"], a["tol"], a["done"], a["inertia"],
                    a["part"], 1)
    torch.cuda.synchronize()
    assert bool(torch.isnan(a["C"]).all()) and bool(torch.isnan(a["inertia"]).all()) and bool((a["done"] == SENTINEL).all())


def test_lloyd_step_refuses_what_it_cannot_hold():
    from spadot_amd.ops import lloyd_steps
    a = _lloyd_args(2, 8, 30)                                    # (8 + 256) * 30 = 7920 <= 7936: runs
    a["C"].fill_(0.5)
    a["done"].zero_()
    lloyd_steps(a["X"], a["C"], a["xoff"], a["npts"], a["n_max"], a["rgroup"], a["Kr"], a["tol"], a["done"], a["inertia"],
                a["part"], 1)
    torch.cuda.synchronize()
    assert bool(torch.isfinite(a["inertia"]).all()) and a["inertia"].tolist() == [4 * 30 * 0.25] * 2
    _lloyd_refused(_lloyd_args(2, 9, 30))                        # (9 + 256) * 30 = 7950
    _lloyd_refused(_lloyd_args(2, 1, 31))                        # 257 * 31 = 7967: no 31st dimension
    _lloyd_refused(_lloyd_args(2, 1, 33))
    _lloyd_refused(_lloyd_args(2, 33, 1))
    _lloyd_refused(_lloyd_args(65536, 1, 1))
    for missing in ("tol", "part", "xoff", "Kr"):                # a null pointer
        _lloyd_refused(dict(_lloyd_args(2, 2, 2), **{missing: None}))


def test_seeding_refuses_what_it_cannot_hold():
    from spadot_amd.ops import kmeanspp_seed

    def refused(d=3, K_max=4, P=2, n_max=6, **none):
        i32 = lambda v: torch.full((P,), v, dtype=torch.int32, device=DEV)
        a = dict(X=torch.ones((6, d), dtype=torch.float64, device=DEV), xoff=i32(0)[:1], npts=i32(6)[:1], n_max=n_max,
                 pset=i32(0), pK=i32(2), pfirst=i32(0), puoff=i32(0), U=torch.full((8,), 0.5, dtype=torch.float64, device=DEV))
        a.update(none)
        idx = torch.full((max(P, 1), K_max), SENTINEL, dtype=torch.int32, device=DEV)
        cen = torch.full((max(P, 1), K_max, d), float("nan"), dtype=torch.float64, device=DEV)
        closest = torch.full((max(P, 1), max(n_max, 1)), float("nan"), dtype=torch.float64, device=DEV)
        with pytest.raises(RuntimeError, match="-22"):
            kmeanspp_seed(a["X"], a["xoff"], a["npts"], a["n_max"], a["pset"], a["pK"], a["pfirst"], a["puoff"], a["U"], K_max,
                          out=(idx, cen, closest))
        torch.cuda.synchronize()
        assert bool((idx == SENTINEL).all()) and bool(torch.isnan(cen).all()) and bool(torch.isnan(closest).all())

    refused(d=33)
    refused(K_max=33)
    refused(P=0)
    refused(n_max=0)
    refused(U=None)
    refused(pfirst=None)
    # d = 32, K_max = 32 is within the seeding entry's limits (the Lloyd step stops at 30): it runs
    X = _dev(np.arange(64.0).reshape(2, 32), torch.float64)
    one = lambda v: torch.tensor([v], dtype=torch.int32, device=DEV)
    idx, cen = kmeanspp_seed(X, one(0), one(2), 2, one(0), one(2), one(1), one(0), _dev([0.5, 0.5], torch.float64), 32)
    assert idx[0, :2].tolist() == [1, 0] and bool((idx[0, 2:] == -1).all())


def test_fit_sweep_raises_for_the_same_shapes():
    from spadot_amd.kmeans import check_sweep_shape, fit_sweep
    x = lambda n, d: torch.ones((n, d), dtype=torch.float64, device=DEV)
    check_sweep_shape(30, 8)
    for d, k in ((30, 9), (31, 1), (32, 1), (33, 1), (1, 33), (20, 0)):
        with pytest.raises(ValueError):
            check_sweep_shape(d, k)
    for X, k, kw in ((x(40, 30), 9, {}), (x(40, 31), 1, {}), (x(40, 33), 1, {}), (x(40, 2), 33, {}), (x(5, 2), 6, {}),
                     (x(5, 1), 1, dict(n_init=65536))):
        with pytest.raises(ValueError):
            fit_sweep([X], [[k]], **kw)
