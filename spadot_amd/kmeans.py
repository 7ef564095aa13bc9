"""K-means on the device: the per-epoch `_update_Kmeans` of the reference fits
sklearn.cluster.KMeans(n_clusters, random_state=seed, n_init=10) on the host for every time point
(/root/reference/SpaDOT/utils/_train_utils.py:255-269) -- at cfg3 that costs more wall time per epoch than
the 100 training steps -- and its analyze stage fits k = 4 .. 20 the same way (_analyze_utils.py:42-105).  This module runs
the same algorithm (k-means++ seeding with sklearn's candidate rule, Lloyd iterations for all n_init restarts at once,
tol = 1e-4 * mean feature variance, best inertia wins) on the MI355X; random draws come from a host numpy RandomState
seeded like sklearn's, everything that touches the data stays in HBM.

One driver (_Plan) fits a list of (data set, k, restart) problems: one seeding launch (spadot_kmeanspp_seed) and one Lloyd
launch pair per iteration (spadot_lloyd_step) for all of them.  Every problem's arithmetic is independent of the others in
the list, so a set fitted on its own and the same set fitted in a batch give the same bits.  Entry points:
KMeansDevice(k).fit(X) (one set, one k), fit_many(Xs, k) (the per-epoch refit of every time point: the plan is cached and
replayed as hipGraphs) and fit_sweep(Xs, ks) (the analyze stage's sweep over k: DESIGN 7b).

Parity: sklearn's random draws are not reproduced (it draws the first centre with p=weights), so single restarts start
elsewhere; everything AFTER the draws is pinned by tests/test_kmeans_kernels_gpu.py to a host reference and through it to
sklearn.cluster.KMeans(init=<the seeded centres>, n_init=1): inertia, labels and iteration count, except where a cluster
empties (it keeps its centre here, sklearn relocates it).  Labels are produced by the spadot_kmeans_assign kernel (nearest
centre, first minimum wins), the same rule sklearn's predict applies.
Selected by model_config['kmeans_backend']: 'device' (default) | 'sklearn' (the reference's host fit, the parity option).
"""
import numpy as np
import torch

from .ops import kmeans_assign, kmeanspp_seed, lloyd_steps

SWEEP_LDS_DOUBLES = 7936         # the Lloyd kernels keep K_max * D centres and 256 * D points in LDS
# Seeding: the kernel runs one workgroup per problem, so its time hardly grows with the problem count; the batched torch
# rounds grow with it but win on few problems (DESIGN 7b, 10 000 x 20, k = 10: 3.1 against 5.3 ms at 50 problems, 5.1 against
# 5.6 ms at 100, 7.6 against 5.9 ms at 150).  A plan of one k for every problem and at most this many problems seeds with the
# torch rounds.
SEED_TORCH_MAX_PROBLEMS = 100


def check_sweep_shape(d, k_max):
    """ValueError unless the device K-means can fit k_max clusters in d dimensions: K <= 32 and the Lloyd launch's LDS budget
    (k_max + 256) * d <= 7936, which admits d <= 30 (the seeding kernel alone would take 32)."""
    if not 1 <= d <= 30:
        raise ValueError(f"the device K-means supports data of 1 to 30 dimensions (got {d})")
    if not 1 <= k_max <= 32:
        raise ValueError(f"the device K-means supports 1 to 32 clusters (got {k_max})")
    if (k_max + 256) * d > SWEEP_LDS_DOUBLES:
        raise ValueError(f"{k_max} clusters in {d} dimensions exceed the device K-means' LDS budget "
                         f"((k + 256) * d <= {SWEEP_LDS_DOUBLES})")


def sweep_draws(n, k, random_state, n_init):
    """The random draws of KMeans(k, random_state, n_init) on n points (sklearn's order): per restart the first centre's row
    and the (k - 1) * (2 + int(log k)) uniforms of the selection rounds, round-major.  Returns (first int64 [n_init], U fp64
    [n_init, (k - 1) * trials])."""
    trials = 2 + int(np.log(k))
    seeds = np.random.RandomState(int(random_state)).randint(np.iinfo(np.int32).max, size=int(n_init))
    first = np.empty(int(n_init), dtype=np.int64)
    U = np.empty((int(n_init), (k - 1) * trials), dtype=np.float64)
    for r, sd in enumerate(seeds):
        g = np.random.RandomState(int(sd))
        first[r] = int(g.choice(n))
        U[r] = g.uniform(size=(k - 1) * trials)       # the same stream as k - 1 calls of size `trials`
    return first, U


class KMeansResult:
    """What sklearn's fitted estimator exposes and _update_Kmeans reads: cluster_centers_, labels_, inertia_, n_iter_."""

    def __init__(self, centers, labels, inertia, n_iter):
        self.cluster_centers_, self.labels_, self.inertia_, self.n_iter_ = centers, labels, inertia, n_iter


class _Plan:
    """Buffers, constants and random draws of every (set t, k in ks[t], restart) problem, and the three phases that fit them:
    (a) centring and tol per set, k-means++ seeding of every problem; (b) `steps` Lloyd iterations (converged restarts
    skipped); (c) the final inertia of every restart, the best of n_init per (set, k) (first minimum wins) and labels for the
    pairs in `want` by the exact nearest-centre kernel on the original coordinates.  The phases are functions of the plan's
    fixed-address buffers only (no host synchronisation, no host-side tensor creation), so fit_many can capture them."""

    def __init__(self, dev, ns, d, ks, n_init, seed, max_iter, tol, check_every, in_dtype, want):
        f64, i32 = torch.float64, torch.int32
        self.ns, self.d, self.R = list(ns), d, int(n_init)
        self.max_iter, self.tol, self.check_every = int(max_iter), float(tol), int(check_every)
        self.pairs = [(t, k) for t, kt in enumerate(ks) for k in kt]
        self.K_max, self.n_max = max(k for _, k in self.pairs), max(ns)
        self.offs = np.concatenate([[0], np.cumsum(ns)]).astype(np.int64)
        self.Xin = torch.zeros((sum(ns), d), dtype=in_dtype, device=dev)        # the caller's data, copied in per call
        # problems in (set, k, restart) order; the host draws every restart's random numbers up front
        pset, pK, pfirst, puoff, Us = [], [], [], [], []
        uoff = 0
        for t, k in self.pairs:
            first, U = sweep_draws(ns[t], k, seed, self.R)
            for r in range(self.R):
                pset.append(t); pK.append(k); pfirst.append(int(first[r])); puoff.append(uoff)
                Us.append(U[r])
                uoff += U.shape[1]
        if uoff >= np.iinfo(np.int32).max:
            raise ValueError("too many random draws for one K-means plan")
        as_dev = lambda a, dt: torch.as_tensor(np.asarray(a), dtype=dt, device=dev)
        self.pset, self.pK, self.pfirst, self.puoff = (as_dev(a, i32) for a in (pset, pK, pfirst, puoff))
        self.U = as_dev(np.concatenate(Us) if uoff else np.zeros(1), f64)
        self.xoff, self.npts = as_dev(self.offs[:-1], i32), as_dev(ns, i32)
        self.qset = as_dev([t for t, _ in self.pairs], torch.int64)
        P, Q, k = len(pset), len(self.pairs), self.K_max
        self.torch_seed = len({k for _, k in self.pairs}) == 1 and P <= SEED_TORCH_MAX_PROBLEMS
        if self.torch_seed:             # the rounds' constants: [Q, R] first rows, [Q, R, k - 1, trials] uniforms, padding
            self.first = self.pfirst.view(Q, self.R).long()
            self.Ut = self.U.view(Q, self.R, k - 1, -1) if k > 1 else None
            self.valid = torch.zeros((Q, self.n_max), dtype=f64, device=dev)
            for q, (t, _) in enumerate(self.pairs):
                self.valid[q, :ns[t]] = 1.0
            self.nlast = as_dev([ns[t] - 1 for t, _ in self.pairs], torch.int64).view(Q, 1, 1)
            self.Xp = torch.zeros((Q, self.n_max, d), dtype=f64, device=dev)
            self.qi = torch.arange(Q, device=dev)[:, None].expand(Q, self.R)
            self.ri = torch.arange(self.R, device=dev)[None, :].expand(Q, self.R)
        else:                           # the kernel's outputs and work space
            self.idx = torch.zeros((P, k), dtype=i32, device=dev)
            self.closest = torch.zeros((P, self.n_max), dtype=f64, device=dev)
        # state the phases share
        self.Xall = torch.zeros((sum(ns), d), dtype=f64, device=dev)            # centred data, all sets back to back
        self.means = torch.zeros((len(ns), d), dtype=f64, device=dev)
        self.tolv = torch.zeros(len(ns), dtype=f64, device=dev)
        self.nd = as_dev([n * d for n in ns], f64)
        self.C = torch.zeros((P, k, d), dtype=f64, device=dev)
        self.done = torch.zeros(P, dtype=i32, device=dev)
        self.ones = torch.ones(P, dtype=i32, device=dev)
        self.inertia = torch.zeros(P, dtype=f64, device=dev)
        self.part = torch.empty(P * ((self.n_max + 255) // 256) * (k * (d + 1) + 1), dtype=f64, device=dev)
        self.ar = torch.arange(Q, device=dev)
        self.cen = torch.zeros((Q, k, d), dtype=f64, device=dev)
        self.best_inertia = torch.zeros(Q, dtype=f64, device=dev)
        self.want = [q for q, pair in enumerate(self.pairs) if pair in want]
        self.loff = np.concatenate([[0], np.cumsum([ns[self.pairs[q][0]] for q in self.want])]).astype(np.int64)
        self.labels = torch.zeros(int(self.loff[-1]), dtype=i32, device=dev)
        self.calls, self.graphs = 0, None

    def _seed(self):
        ms, sq = [], []
        for t in range(len(self.ns)):
            # a fresh tensor per set: its mean and tol do not depend on where the set sits in the plan's buffers
            x = self.Xin[self.offs[t]:self.offs[t + 1]].to(torch.float64, copy=True)
            ms.append(x.mean(0))                            # sklearn centres the data for accuracy
            xc = torch.sub(x, ms[-1], out=self.Xall[self.offs[t]:self.offs[t + 1]])
            sq.append((xc * xc).sum(1).sum())
        torch.stack(ms, out=self.means)
        torch.mul(torch.stack(sq) / self.nd, self.tol, out=self.tolv)             # tol * mean feature variance
        if self.torch_seed:
            self._seed_torch()
        else:
            kmeanspp_seed(self.Xall, self.xoff, self.npts, self.n_max, self.pset, self.pK, self.pfirst, self.puoff, self.U,
                          self.K_max, out=(self.idx, self.C, self.closest))
        self.done.zero_()

    def _seed_torch(self):
        """The k - 1 selection rounds of every problem batched on [Q, R, n_max] tensors (shorter sets are padded with rows
        that can never be drawn and weigh nothing): the rule and the draws of spadot_kmeanspp_seed.  Its prefix sums, distance
        products and potentials round in another order than the kernel's, and with the padding and product shapes of the
        batch, so a chosen row can differ only where a draw lies within rounding distance of a prefix boundary or two
        candidates' potentials tie to rounding.  (Chosen rows are exact data rows: everything after them is per problem.)"""
        Q, R, k, d = len(self.pairs), self.R, self.K_max, self.d
        Xp, valid = self.Xp, self.valid
        for q, (t, _) in enumerate(self.pairs):
            Xp[q, :self.ns[t]] = self.Xall[self.offs[t]:self.offs[t + 1]]
        xsq = (Xp * Xp).sum(2)                                                    # [Q, n_max]
        centers = self.C.view(Q, R, k, d)
        c0 = Xp[self.qi, self.first]                                              # [Q, R, d]
        centers[:, :, 0] = c0
        closest = (xsq[:, None, :] - 2.0 * torch.matmul(c0, Xp.transpose(1, 2)) + (c0 * c0).sum(2)[:, :, None]).clamp_(min=0)
        closest = closest * valid[:, None, :]                                     # [Q, R, n_max]; padding weighs nothing
        pot = closest.sum(2)
        for c in range(1, k):
            rv = self.Ut[:, :, c - 1] * pot[:, :, None]                           # [Q, R, trials]
            cand = torch.minimum(torch.searchsorted(torch.cumsum(closest, 2), rv), self.nlast)
            Xcand = Xp[self.qi[:, :, None], cand]                                 # [Q, R, trials, d]
            dist = (xsq[:, None, None, :] - 2.0 * torch.matmul(Xcand, Xp[:, None].transpose(2, 3))
                    + (Xcand * Xcand).sum(3)[..., None]).clamp_(min=0)
            dist = torch.minimum(dist * valid[:, None, None, :], closest[:, :, None, :])       # [Q, R, trials, n_max]
            pots = dist.sum(3)
            best = torch.argmin(pots, dim=2)                                      # [Q, R]
            centers[:, :, c] = Xcand[self.qi, self.ri, best]
            closest = dist[self.qi, self.ri, best]
            pot = pots[self.qi, self.ri, best]

    def _lloyd(self, steps):
        lloyd_steps(self.Xall, self.C, self.xoff, self.npts, self.n_max, self.pset, self.pK, self.tolv, self.done,
                    self.inertia, self.part, steps, skip_done=True)

    def _finish(self):
        # inertia of the FINAL centres: one assignment pass with every restart frozen (frozen centres are not written)
        lloyd_steps(self.Xall, self.C, self.xoff, self.npts, self.n_max, self.pset, self.pK, self.tolv, self.ones,
                    self.inertia, self.part, 1)
        inert = self.inertia.view(len(self.pairs), self.R)
        best = torch.argmin(inert, dim=1)                                         # first minimum wins
        self.best_inertia.copy_(inert[self.ar, best])
        self.cen.copy_(self.C.view(len(self.pairs), self.R, self.K_max, self.d)[self.ar, best] + self.means[self.qset][:, None, :])
        for j, q in enumerate(self.want):       # the exact nearest-centre rule on the ORIGINAL coordinates (HIP kernel)
            t, k = self.pairs[q]
            x = self.Xin[self.offs[t]:self.offs[t + 1]].to(torch.float64)
            self.labels[self.loff[j]:self.loff[j + 1]] = kmeans_assign(x, self.cen[q, :k])

    def _capture(self):
        torch.cuda.synchronize()
        pool = torch.cuda.graph_pool_handle()
        graphs = []
        for fn in (self._seed, lambda: self._lloyd(self.check_every), self._finish):
            g = torch.cuda.CUDAGraph()
            with torch.cuda.graph(g, pool=pool, capture_error_mode="thread_local"):
                fn()
            graphs.append(g)
        self.graphs = graphs

    def run(self, Xs, graphs=False):
        """Fits the problems on Xs; graphs: capture the phases at the second call and replay them from then on.  Returns
        [ {k: KMeansResult} per set ]; labels_ is None outside `want`; n_iter_ is the iteration count at the check where all
        restarts of that (set, k) had converged."""
        for t, x in enumerate(Xs):
            self.Xin[self.offs[t]:self.offs[t + 1]].copy_(x)
        self.calls += 1
        if graphs and self.graphs is None and self.calls >= 2 and not torch.cuda.is_current_stream_capturing():
            self._capture()                      # (first call: eager -- library handles, allocator warm-up)
        seed, finish = (self.graphs[0].replay, self.graphs[2].replay) if self.graphs else (self._seed, self._finish)
        seed()
        Q, R = len(self.pairs), self.R
        n_iter = np.zeros(Q, dtype=np.int64)
        it = 0
        while it < self.max_iter:
            steps = min(self.check_every, self.max_iter - it)
            if self.graphs and steps == self.check_every:
                self.graphs[1].replay()
            else:
                self._lloyd(steps)
            it += steps
            pair_done = self.done.view(Q, R).all(1).cpu().numpy()      # one host sync per `check_every` iterations
            n_iter[(n_iter == 0) & pair_done] = it
            if pair_done.all():
                break
        n_iter[n_iter == 0] = it
        finish()
        cen = self.cen.cpu().numpy()             # (synchronises)
        inert = self.best_inertia.cpu().numpy()
        lab = self.labels.cpu().numpy()
        labels = {q: lab[self.loff[j]:self.loff[j + 1]].copy() for j, q in enumerate(self.want)}
        out = [dict() for _ in self.ns]
        for q, (t, k) in enumerate(self.pairs):
            out[t][k] = KMeansResult(cen[q, :k].copy(), labels.get(q), float(inert[q]), int(n_iter[q]))
        return out


def _plan(Xs, ks, random_state, n_init, max_iter, tol, check_every, labels_for):
    """Checks the inputs and builds the plan of fit_sweep's arguments; None when there is nothing to fit."""
    T = len(Xs)
    if len(ks) != T:
        raise ValueError("the device K-means needs one list of k values per data set")
    if T == 0:
        return None
    if not all(x.is_cuda and x.dim() == 2 and x.shape[1] == Xs[0].shape[1] and x.dtype == Xs[0].dtype for x in Xs):
        raise ValueError("the device K-means runs on the MI355X, on data sets of one dimension and dtype")
    ns = [int(x.shape[0]) for x in Xs]
    d = int(Xs[0].shape[1])
    k_max = max((k for kt in ks for k in kt), default=0)
    if k_max == 0:
        return None
    check_sweep_shape(d, k_max)
    for t, kt in enumerate(ks):
        for k in kt:
            if not 1 <= k <= ns[t]:
                raise ValueError(f"k = {k} clusters on data set {t} of {ns[t]} points")
    pairs = [(t, k) for t, kt in enumerate(ks) for k in kt]
    if not 1 <= len(pairs) * int(n_init) <= 65535:
        raise ValueError(f"{len(pairs)} (data set, k) pairs x {n_init} restarts: one Lloyd launch holds 1 to 65535 restarts")
    want = set(pairs) if labels_for is True else set((int(t), int(k)) for t, k in (labels_for or ()))
    return _Plan(Xs[0].device, ns, d, ks, n_init, random_state, max_iter, tol, check_every, Xs[0].dtype, want)


def fit_sweep(Xs, ks, random_state=1993, n_init=10, max_iter=300, tol=1e-4, check_every=8, labels_for=None):
    """KMeansDevice(k, random_state, n_init).fit(Xs[t]) for every t and every k in ks[t], all at once (see _Plan._seed_torch
    for the one place where a plan's composition can move a result).

    Xs: list of [n_t, d] device tensors (one dimension and dtype); ks[t]: the k values to fit on set t.  Every k draws from
    RandomState(random_state), as the reference creates every KMeans with random_state=1993.  One host sync per
    `check_every` Lloyd iterations; max_iter is honoured exactly.  labels_for: (t, k) pairs whose labels are wanted (True:
    all).  Returns [ {k: KMeansResult} per set ]; labels_ is None where not asked for; n_iter_ is the iteration count at the
    check where all restarts of that (set, k) had converged."""
    ks = [[int(k) for k in kt] for kt in ks]
    plan = _plan(Xs, ks, random_state, n_init, max_iter, tol, check_every, labels_for)
    return plan.run(Xs) if plan is not None else [{} for _ in Xs]


class KMeansDevice:
    """sklearn.cluster.KMeans-shaped estimator: fit(X) on one [n, d] device tensor sets cluster_centers_ (numpy [k, d]),
    labels_ (numpy int32 [n]), inertia_ (float) and n_iter_; the one-set, one-k case of fit_sweep."""

    def __init__(self, n_clusters, random_state=1993, n_init=10, max_iter=300, tol=1e-4, check_every=8):
        self.k, self.seed, self.n_init, self.max_iter, self.tol, self.check_every = \
            int(n_clusters), int(random_state), int(n_init), int(max_iter), float(tol), int(check_every)

    def fit(self, X):
        r = fit_sweep([X], [[self.k]], self.seed, self.n_init, self.max_iter, self.tol, self.check_every, labels_for=True)[0][self.k]
        self.cluster_centers_, self.labels_, self.inertia_, self.n_iter_ = r.cluster_centers_, r.labels_, r.inertia_, r.n_iter_
        return self


_PLANS = {}


def fit_many(Xs, n_clusters, random_state=1993, n_init=10, max_iter=300, tol=1e-4, check_every=8):
    """KMeansDevice(...).fit(X) for SEVERAL data sets (the latents of all time points, refitted every epoch:
    _train_utils.py:255-269) as one plan.  The refit repeats its shape every epoch and was HOST-bound (~420
    launches, 11 ms of launch overhead for ~4 ms of device work), so the plan is kept per shape (a few at most) and from its
    second call on its three phases are replayed hipGraphs; the only host synchronisations left are the convergence checks
    between Lloyd groups and the final copy.  Returns a list of KMeansResult."""
    if len(Xs) == 0:
        return []
    ks = [[int(n_clusters)]] * len(Xs)
    key = (str(Xs[0].device), tuple(int(x.shape[0]) for x in Xs), tuple(Xs[0].shape[1:]), int(n_clusters), int(n_init),
           int(random_state), int(max_iter), float(tol), int(check_every), Xs[0].dtype)
    plan = _PLANS.get(key)
    if plan is None:
        plan = _plan(Xs, ks, random_state, n_init, max_iter, tol, check_every, True)
        if len(_PLANS) >= 8:                     # a few shapes at most are alive in a run; do not hoard buffers
            _PLANS.clear()
        _PLANS[key] = plan
    return [r[int(n_clusters)] for r in plan.run(Xs, graphs=True)]
