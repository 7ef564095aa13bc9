"""Full-covariance Gaussian mixtures on the device: elongated domains, a membership probability per spot and a likelihood-based
rule (BIC) for the number of domains (csrc/gmm.hip).  The reference has no such stage; the definition is sklearn 1.7's
GaussianMixture(covariance_type='full', reg_covar=1e-6, tol=1e-3, max_iter=100, n_init=1) started from a hard labeling.

    fit_sweep(Xs, labelings, n_components)   every (data set t, labeling l) problem of the call in one launch group per iteration
    estep_many(Xs, models)                   one E-step with fitted (or given) parameters: score_samples, labels, memberships
    m_step_many(Xs, resps)                   one M-step from given responsibilities (the fit's first step; the kernel tests)
    GaussianMixtureDevice(K).fit(X)          sklearn-shaped, started from KMeansDevice(K, random_state)'s labels

A problem is X [n, d], K and labels in 0 .. K-1.  The data of a set are centred by its fp64 column mean m (as kmeans._Plan._seed
does); means are reported as mu + m.  For a component that holds points this is sklearn's result (translation invariance); an
initial label value without points has nk = 10 eps and its mean is then m, where sklearn gives the origin: the one deviation.
    M-step   nk = sum_i r_ik + 10 eps, mu_k = sum_i r_ik x_i / nk, Sigma_k = sum_i r_ik (x_i - mu_k)(x_i - mu_k)^T / nk + reg I
             (formed from moments about the mean the iteration started from, so that a collapsed component keeps reg I to
             full precision: DESIGN 7g), w_k = nk / n, P_k = L_k^-T with Sigma_k = L_k L_k^T
    E-step   lp_ik = -(d log 2pi + |(x_i - mu_k) P_k|^2) / 2 + sum_j log P_k,jj + log w_k, norm_i = logsumexp_k lp_ik,
             log r_ik = lp_ik - norm_i
    fit      r = one-hot(labels), M-step; then per iteration E-step, lb = mean norm, M-step, stop (converged) when |lb - lb_prev|
             < tol, at most max_iter times; one last E-step gives resp, labels (argmax, first maximum), log_likelihood = sum norm,
             bic = -2 ll + (K d (d + 1) / 2 + K d + K - 1) log n and aic = -2 ll + 2 (...).
n_iter and the stop flags are kept per problem on the device; the host reads them once per `check_every` iterations.  A Sigma
that is not positive definite (sklearn raises) gives NaN parameters here and a fit that does not converge.
Limits: 1 <= d <= 32, 1 <= K <= 32, at most 65535 problems per call, and the LDS rule of check_shape."""
import numpy as np

MAX_DIM = 32
MAX_COMPONENTS = 32
MAX_PROBLEMS = 65535
MAX_POINTS = 2147483391
LDS_BYTES = 163840


def _dims(d):
    """DP (d padded to a multiple of 4), T (packed triangle), S (doubles per component in par), M (moments per component)."""
    DP = (d + 3) // 4 * 4
    T = DP * (DP + 1) // 2
    return DP, T, DP + T + 2, 1 + DP + T


def lds_bytes(d, K):
    DP, _, S, _ = _dims(d)
    return 8 * (max(K * S, (K + 256) * DP) + 256 * (K | 1)) + 2048


def check_shape(d, K):
    """ValueError unless the kernels take K components in d dimensions: the parameters of the problem (K S doubles, S = DP +
    DP (DP + 1) / 2 + 2, DP = 4 ceil(d / 4)) or its means and the block's 256 points ((K + 256) DP), and the 256 x (K | 1) tile of
    responsibilities, share one compute unit's LDS."""
    from .stage_ops import GMM_LIMITS
    if not (1 <= d <= MAX_DIM and 1 <= K <= MAX_COMPONENTS and lds_bytes(d, K) <= LDS_BYTES):
        raise ValueError(f"{K} components in {d} dimensions are outside the limits of the device Gaussian mixture: {GMM_LIMITS}")


def n_parameters(K, d):
    return K * d * (d + 1) // 2 + K * d + K - 1


class GMMResult:
    """One fitted mixture, named as sklearn's: weights_ [K], means_ [K, d], covariances_ [K, d, d], precisions_cholesky_ [K, d, d]
    (upper), lower_bound_, n_iter_, converged_, log_likelihood_ (sum over the points), bic_, aic_, labels_ (int32 [n]) and resp_
    ([n, K], None unless asked for); center_ [d] is the set's mean and means_centred_ = the means relative to it."""

    def __init__(self, **kw):
        self.resp_ = None
        self.__dict__.update(kw)

    @property
    def n_components(self):
        return int(self.weights_.shape[0])


def _as_sets(Xs):
    import torch
    Xs = [x if isinstance(x, torch.Tensor) else torch.as_tensor(np.asarray(x)) for x in Xs]
    if not Xs:
        raise ValueError("the device Gaussian mixture needs at least one data set")
    for x in Xs:
        if not x.is_cuda:
            raise RuntimeError("spadot_amd fits Gaussian mixtures on the MI355X only (got a CPU tensor); there is no CPU path")
        if x.dim() != 2 or x.dtype not in (torch.float32, torch.float64):
            raise ValueError(f"a data set must be an [n, d] fp32 or fp64 tensor (got {tuple(x.shape)} {x.dtype})")
    x0 = Xs[0]
    if any(int(x.shape[1]) != int(x0.shape[1]) or x.dtype != x0.dtype or x.device != x0.device for x in Xs):
        raise ValueError("the data sets of one call must share their dimension, their dtype and their device")
    for t, x in enumerate(Xs):
        if not 1 <= int(x.shape[0]) <= MAX_POINTS:
            raise ValueError(f"data set {t} has {int(x.shape[0])} points: the device Gaussian mixture takes 1 to {MAX_POINTS}")
    return Xs


class _Batch:
    """The problems of one call on the device: the centred data of all sets back to back, the problem table, the parameter
    blocks and the work space.  sets[p]: the data set of problem p; Ks[p]: its component count; centers: the mean to take from
    every set (None: its own column mean)."""

    def __init__(self, Xs, sets, Ks, centers=None, work=True):
        import torch
        f64 = torch.float64
        dev, d = Xs[0].device, int(Xs[0].shape[1])
        P, K_max = len(sets), max(Ks)
        if not 1 <= P <= MAX_PROBLEMS:
            raise ValueError(f"one call takes 1 to {MAX_PROBLEMS} mixtures (got {P})")
        check_shape(d, K_max)
        self.dev, self.d, self.P, self.K_max, self.sets, self.Ks = dev, d, P, K_max, list(sets), list(Ks)
        self.DP, self.T, self.S, self.M = _dims(d)
        ns = [int(x.shape[0]) for x in Xs]
        self.sizes = [ns[t] for t in sets]
        self.n_max = max(self.sizes)
        xoff = np.concatenate([[0], np.cumsum(ns)[:-1]]).astype(np.int64)
        self.roff = np.concatenate([[0], np.cumsum(self.sizes)]).astype(np.int64)
        self.total = int(self.roff[-1])
        with torch.cuda.device(dev):
            ms, xc = [], []
            for t, x in enumerate(Xs):                    # a fresh tensor per set: its mean does not depend on the batch
                x64 = x.to(f64, copy=True)
                m = x64.mean(0) if centers is None else torch.as_tensor(np.asarray(centers[t], dtype=np.float64), device=dev)
                ms.append(m)
                xc.append(x64.sub_(m))
            self.X = torch.cat(xc).contiguous()
            self.means = torch.stack(ms).cpu().numpy()
            prob = np.stack([xoff[np.asarray(sets)], self.roff[:-1], np.asarray(self.sizes, dtype=np.int64),
                             np.asarray(Ks, dtype=np.int64)], axis=1)
            self.prob = torch.as_tensor(np.ascontiguousarray(prob), device=dev)
            self.par = torch.zeros((P, K_max, self.S), dtype=f64, device=dev)
            if work:
                nblk = (self.n_max + 255) // 256
                self.w = torch.zeros((P, K_max), dtype=f64, device=dev)
                self.cov = torch.zeros((P, K_max, d, d), dtype=f64, device=dev)
                self.mom = torch.zeros((P, K_max, self.M), dtype=f64, device=dev)
                self.part = torch.empty(P * nblk * (K_max * self.M + 1), dtype=f64, device=dev)
                self.done = torch.zeros(P, dtype=torch.int32, device=dev)
                self.n_iter = torch.zeros(P, dtype=torch.int32, device=dev)
                self.lb = torch.full((P,), -np.inf, dtype=f64, device=dev)

    def em(self, steps, reg_covar, tol, resp_init=None):
        import torch
        from .stage_ops import gmm_em_steps
        with torch.cuda.device(self.dev):
            gmm_em_steps(self.X, self.prob, self.n_max, self.par, self.w, self.cov, self.part, self.done, self.n_iter, self.lb,
                         reg_covar, tol, steps, resp_init=resp_init, mom=self.mom)

    def estep(self, labels=True, resp=False, lp=False):
        """(norm [total], labels [total] | None, resp [total, K_max] | None, lp | None), device tensors."""
        import torch
        from .stage_ops import gmm_estep
        f64 = torch.float64
        with torch.cuda.device(self.dev):
            norm = torch.empty(self.total, dtype=f64, device=self.dev)
            lab = torch.empty(self.total, dtype=torch.int32, device=self.dev) if labels else None
            r = torch.empty((self.total, self.K_max), dtype=f64, device=self.dev) if resp else None
            l = torch.empty((self.total, self.K_max), dtype=f64, device=self.dev) if lp else None
            gmm_estep(self.X, self.prob, self.n_max, self.par, norm, lab, r, l)
        return norm, lab, r, l

    def unpack(self, par):
        """par [P, K_max, S] (numpy; per problem the K_max padded means, then per component the packed factor, its log
        determinant and log w) -> (centred means [P, K_max, d], precision Cholesky factors [P, K_max, d, d])."""
        d, DP, T, K_max = self.d, self.DP, self.T, self.K_max
        flat = par.reshape(par.shape[0], -1)
        mu = flat[:, :K_max * DP].reshape(-1, K_max, DP)[:, :, :d].copy()
        rest = flat[:, K_max * DP:].reshape(-1, K_max, T + 2)
        pc = np.zeros((par.shape[0], K_max, d, d))
        for j in range(d):
            pc[:, :, :j + 1, j] = rest[:, :, j * (j + 1) // 2: j * (j + 1) // 2 + j + 1]
        return mu, pc

    def pack(self, weights, means_c, pchol):
        """The parameters of one problem as its block of a host image of par ([K_max, S])."""
        d, DP, T, K_max = self.d, self.DP, self.T, self.K_max
        K = weights.shape[0]
        mu = np.zeros((K_max, DP))
        mu[:K, :d] = means_c
        rest = np.zeros((K_max, T + 2))
        for j in range(DP):
            if j < d:
                rest[:K, j * (j + 1) // 2: j * (j + 1) // 2 + j + 1] = pchol[:, :j + 1, j]
            else:
                rest[:, j * (j + 1) // 2 + j] = 1.0
        with np.errstate(divide="ignore"):
            rest[:K, T] = np.sum(np.log(np.diagonal(pchol, axis1=1, axis2=2)), axis=1)
            rest[:K, T + 1] = np.log(weights)
        return np.concatenate([mu.ravel(), rest.ravel()]).reshape(K_max, self.S)


def _flatten(Xs, per_set):
    if len(per_set) != len(Xs):
        raise ValueError(f"one list per data set is needed ({len(Xs)} sets, {len(per_set)} lists)")
    sets = [t for t, ls in enumerate(per_set) for _ in ls]
    return sets, [len(ls) for ls in per_set]


def _nest(flat, shape):
    out, p = [], 0
    for m in shape:
        out.append(flat[p:p + m])
        p += m
    return out


def _labels_on_device(Xs, labelings, n_components):
    """Validates the labelings (ValueError before any launch) and returns (sets, shape, Ks, labels int64 [total] on the device)."""
    import torch
    sets, shape = _flatten(Xs, labelings)
    dev = Xs[0].device
    labs = []
    for t, ls in enumerate(labelings):
        n = int(Xs[t].shape[0])
        for lab in ls:
            lab = lab if isinstance(lab, torch.Tensor) else torch.as_tensor(np.asarray(lab))
            if lab.dim() != 1 or lab.shape[0] != n:
                raise ValueError(f"a labeling of data set {t} must hold one label per point ({n}), not {tuple(lab.shape)}")
            if lab.dtype.is_floating_point or lab.dtype == torch.bool or lab.dtype.is_complex:
                raise ValueError(f"labels must be integers (got {lab.dtype})")
            labs.append(lab.to(device=dev, dtype=torch.int64))
    if not labs:
        raise ValueError("the device Gaussian mixture needs at least one labeling")
    with torch.cuda.device(dev):
        lo = torch.stack([l.min() for l in labs]).cpu().numpy()
        hi = torch.stack([l.max() for l in labs]).cpu().numpy()
    if n_components is None:
        Ks = (hi + 1).tolist()
    else:
        Ks = [int(k) for kt in n_components for k in kt]
        if len(Ks) != len(labs):
            raise ValueError(f"n_components holds {len(Ks)} component counts for {len(labs)} labelings")
    for p, K in enumerate(Ks):
        if not 1 <= K <= MAX_COMPONENTS:
            raise ValueError(f"labeling {p} has {K} components: the device Gaussian mixture takes 1 to {MAX_COMPONENTS}")
        if lo[p] < 0 or hi[p] >= K:
            raise ValueError(f"labeling {p} holds labels {int(lo[p])} .. {int(hi[p])}: labels must lie in 0 .. {K - 1}")
    return sets, shape, Ks, torch.cat(labs)


def fit_sweep(Xs, labelings, n_components=None, reg_covar=1e-6, tol=1e-3, max_iter=100, check_every=4, resp_for=None):
    """Xs: [n_t, d] device tensors (fp32 or fp64, converted to fp64: exact); labelings[t]: the integer label vectors (numpy or
    torch) that start one mixture each on set t; n_components[t][l]: the K of each (default: its largest label + 1).  All
    problems advance together, `check_every` iterations per host round trip; a converged problem is frozen.  resp_for: True or
    the (t, l) pairs whose responsibilities are wanted.  Returns [t][l] -> GMMResult.  A problem's result does not depend on what
    else the call holds, nor on check_every."""
    import torch
    Xs = _as_sets(Xs)
    sets, shape, Ks, labels = _labels_on_device(Xs, labelings, n_components)
    if int(max_iter) < 1 or int(check_every) < 1:
        raise ValueError("max_iter and check_every must be at least 1")
    pairs = [(t, l) for t, m in enumerate(shape) for l in range(m)]
    want = set(pairs) if resp_for is True else set((int(t), int(l)) for t, l in (resp_for or ()))
    b = _Batch(Xs, sets, Ks)
    with torch.cuda.device(b.dev):
        onehot = torch.zeros((b.total, b.K_max), dtype=torch.float64, device=b.dev)
        onehot.scatter_(1, labels[:, None], 1.0)
        it = 0
        while it < max_iter:
            steps = min(int(check_every), int(max_iter) - it)
            b.em(steps, reg_covar, tol, resp_init=onehot if it == 0 else None)
            it += steps
            if bool(b.done.all()):                        # the one host sync per `check_every` iterations
                break
        del onehot
        norm, lab, _, _ = b.estep(labels=True)
        norm, lab = norm.cpu().numpy(), lab.cpu().numpy()
        par, w, cov = b.par.cpu().numpy(), b.w.cpu().numpy(), b.cov.cpu().numpy()
        done, n_iter, lb = b.done.cpu().numpy(), b.n_iter.cpu().numpy(), b.lb.cpu().numpy()
    mu, pc = b.unpack(par)
    flat = []
    for p, (t, K) in enumerate(zip(sets, Ks)):
        lo, hi = int(b.roff[p]), int(b.roff[p + 1])
        n = hi - lo
        ll = float(np.sum(norm[lo:hi]))
        npar = n_parameters(K, b.d)
        flat.append(GMMResult(weights_=w[p, :K].copy(), means_=mu[p, :K] + b.means[t], means_centred_=mu[p, :K].copy(),
                              center_=b.means[t].copy(), covariances_=cov[p, :K].copy(), precisions_cholesky_=pc[p, :K].copy(),
                              lower_bound_=float(lb[p]), n_iter_=int(n_iter[p]), converged_=bool(done[p]), log_likelihood_=ll,
                              bic_=-2.0 * ll + npar * np.log(n), aic_=-2.0 * ll + 2.0 * npar, labels_=lab[lo:hi].copy()))
    res = _nest(flat, shape)
    if want:
        if any(not (0 <= t < len(shape) and 0 <= l < shape[t]) for t, l in want):
            raise ValueError("resp_for names a (data set, labeling) pair that the call does not hold")
        ps = [p for p, pair in enumerate(pairs) if pair in want]
        sub = _Batch(Xs, [sets[p] for p in ps], [Ks[p] for p in ps], work=False)       # the same centring, the same bits
        with torch.cuda.device(b.dev):
            idx = torch.as_tensor(ps, device=b.dev)
            src = b.par.view(b.P, -1)[idx]
            dst = sub.par.view(sub.P, -1)
            dst[:, :sub.K_max * b.DP] = src[:, :sub.K_max * b.DP]
            dst[:, sub.K_max * b.DP:] = src[:, b.K_max * b.DP: b.K_max * b.DP + sub.K_max * (b.T + 2)]
            r = sub.estep(labels=False, resp=True)[2].cpu().numpy()
        for i, p in enumerate(ps):
            flat[p].resp_ = r[int(sub.roff[i]):int(sub.roff[i + 1]), :Ks[p]].copy()
    return res


def estep_many(Xs, models, resp=False, lp=False):
    """One E-step of every models[t][l] (GMMResult, or anything with weights_, means_centred_, center_ and precisions_cholesky_)
    on Xs[t]: returns [t][l] -> {'norm' (score_samples), 'labels', and where asked 'resp', 'lp'}.  The data are centred by the
    model's center_, so the training data give exactly the fit's own last E-step."""
    import torch
    Xs = _as_sets(Xs)
    sets, shape = _flatten(Xs, models)
    flat = [m for ms in models for m in ms]
    if not flat:
        return [[] for _ in Xs]
    # the sets of one launch are centred once, so models of one set with different centres go into separate launches
    groups, seen = {}, {}
    for p, (t, m) in enumerate(zip(sets, flat)):
        if int(m.means_centred_.shape[1]) != int(Xs[t].shape[1]):
            raise ValueError(f"a mixture of {m.means_centred_.shape[1]} dimensions cannot score data of {int(Xs[t].shape[1])}")
        cs = seen.setdefault(t, [])
        key = next((i for i, c in enumerate(cs) if np.array_equal(c, m.center_)), len(cs))
        if key == len(cs):
            cs.append(np.asarray(m.center_))
        groups.setdefault(key, []).append(p)
    results = [None] * len(flat)
    for ps in groups.values():
        ts = sorted({sets[p] for p in ps})
        remap = {t: i for i, t in enumerate(ts)}
        centers = {remap[sets[p]]: flat[p].center_ for p in ps}
        b = _Batch([Xs[t] for t in ts], [remap[sets[p]] for p in ps], [flat[p].n_components for p in ps],
                   centers=[centers[i] for i in range(len(ts))], work=False)
        host = np.stack([b.pack(flat[p].weights_, flat[p].means_centred_, flat[p].precisions_cholesky_)
                         for p in ps])
        with torch.cuda.device(b.dev):
            b.par.copy_(torch.as_tensor(host, device=b.dev))
            norm, lab, r, l = b.estep(labels=True, resp=resp, lp=lp)
            norm, lab = norm.cpu().numpy(), lab.cpu().numpy()
            r = r.cpu().numpy() if r is not None else None
            l = l.cpu().numpy() if l is not None else None
        for i, p in enumerate(ps):
            lo, hi, K = int(b.roff[i]), int(b.roff[i + 1]), flat[p].n_components
            o = {"norm": norm[lo:hi].copy(), "labels": lab[lo:hi].copy()}
            if r is not None:
                o["resp"] = r[lo:hi, :K].copy()
            if l is not None:
                o["lp"] = l[lo:hi, :K].copy()
            results[p] = o
    return _nest(results, shape)


def m_step_many(Xs, resps, reg_covar=1e-6, centers=None):
    """One M-step from given responsibilities: resps[t] is a list of [n_t, K] arrays.  Returns [t][l] -> dict(weights, means_c
    (centred), covariances, precisions_cholesky, s0 [K], s1 [K, d], s2 [K, d, d] (the summed moments of the centred data), center).
    centers: the mean to take from every set (default: its own column mean)."""
    import torch
    Xs = _as_sets(Xs)
    sets, shape = _flatten(Xs, resps)
    flat = [np.asarray(r, dtype=np.float64) for rs in resps for r in rs]
    for p, (t, r) in enumerate(zip(sets, flat)):
        if r.ndim != 2 or r.shape[0] != int(Xs[t].shape[0]):
            raise ValueError(f"responsibilities {p} must be [n, K] with n = {int(Xs[t].shape[0])} (got {r.shape})")
    b = _Batch(Xs, sets, [r.shape[1] for r in flat], centers=centers)
    host = np.zeros((b.total, b.K_max))
    for p, r in enumerate(flat):
        host[int(b.roff[p]):int(b.roff[p + 1]), :r.shape[1]] = r
    with torch.cuda.device(b.dev):
        b.em(0, reg_covar, 0.0, resp_init=torch.as_tensor(host, device=b.dev))
        par, w, cov, mom = b.par.cpu().numpy(), b.w.cpu().numpy(), b.cov.cpu().numpy(), b.mom.cpu().numpy()
    mu, pc = b.unpack(par)
    d, DP = b.d, b.DP
    out = []
    for p, (t, K) in enumerate(zip(sets, b.Ks)):
        s2 = np.zeros((K, d, d))
        for j in range(d):
            s2[:, :j + 1, j] = mom[p, :K, 1 + DP + j * (j + 1) // 2: 1 + DP + j * (j + 1) // 2 + j + 1]
            s2[:, j, :j + 1] = s2[:, :j + 1, j]
        out.append(dict(weights=w[p, :K].copy(), means_c=mu[p, :K].copy(), covariances=cov[p, :K].copy(),
                        precisions_cholesky=pc[p, :K].copy(), s0=mom[p, :K, 0].copy(), s1=mom[p, :K, 1:1 + d].copy(), s2=s2,
                        center=b.means[t].copy()))
    return _nest(out, shape)


class GaussianMixtureDevice:
    """sklearn.mixture.GaussianMixture-shaped estimator (covariance_type='full', one start) for [n, d] device tensors.  fit(X)
    starts from the labels of KMeansDevice(n_components, random_state) -- sklearn's own K-means draws are not reproduced, as
    kmeans.py says of itself -- and sets weights_, means_, covariances_, precisions_cholesky_, lower_bound_, n_iter_, converged_.
    predict, predict_proba, score_samples, score, bic and aic follow sklearn's definitions."""

    def __init__(self, n_components, random_state=1993, reg_covar=1e-6, tol=1e-3, max_iter=100, check_every=4):
        self.n_components, self.random_state = int(n_components), int(random_state)
        self.reg_covar, self.tol, self.max_iter, self.check_every = float(reg_covar), float(tol), int(max_iter), int(check_every)
        self.result_ = None

    def fit(self, X, labels=None):
        """labels: a starting labeling in 0 .. n_components - 1 instead of the K-means one."""
        X = _as_sets([X])[0]
        check_shape(int(X.shape[1]), self.n_components)
        if labels is None:
            from .kmeans import KMeansDevice
            labels = KMeansDevice(self.n_components, random_state=self.random_state).fit(X).labels_
        r = fit_sweep([X], [[labels]], [[self.n_components]], self.reg_covar, self.tol, self.max_iter, self.check_every)[0][0]
        self.result_ = r
        for name in ("weights_", "means_", "covariances_", "precisions_cholesky_", "lower_bound_", "n_iter_", "converged_",
                     "labels_"):
            setattr(self, name, getattr(r, name))
        return self

    def fit_predict(self, X, labels=None):
        return self.fit(X, labels).labels_

    def _estep(self, X, **kw):
        if self.result_ is None:
            raise RuntimeError("this GaussianMixtureDevice is not fitted yet")
        return estep_many([X], [[self.result_]], **kw)[0][0]

    def predict(self, X):
        return self._estep(X)["labels"]

    def predict_proba(self, X):
        return self._estep(X, resp=True)["resp"]

    def score_samples(self, X):
        return self._estep(X)["norm"]

    def score(self, X):
        return float(np.mean(self.score_samples(X)))

    def bic(self, X):
        n, d = int(X.shape[0]), int(X.shape[1])
        return -2.0 * self.score(X) * n + n_parameters(self.n_components, d) * np.log(n)

    def aic(self, X):
        n, d = int(X.shape[0]), int(X.shape[1])
        return -2.0 * self.score(X) * n + 2.0 * n_parameters(self.n_components, d)
