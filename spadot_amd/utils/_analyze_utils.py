"""Host-side parts of the analyze stage: mirror of the reference's SpaDOT/utils/_analyze_utils.py.  The clustering itself
runs on the device (spadot_amd.kmeans.fit_sweep); here are the elbow rule of Adaptive_clustering (:73-88) as a pure
function, the silhouette rule of `--criterion silhouette` and the BIC rule of `--method gmm --criterion bic` (no counterparts in the reference), the WSS table, and the plots (WSS curve :89-99, domains :140-164, transition dotplot :166-209), drawn with
matplotlib's object API on an Agg canvas (no pyplot: global plotting state is left alone; seaborn is not needed)."""
import numpy as np

MIN_CLUSTERS, MAX_CLUSTERS, WSS_THRESHOLD = 4, 20, 0.1       # Adaptive_clustering's defaults


def _curve(wss):
    """(wss, d, ratio) as fp64 arrays: d[i] = wss[i-1] - wss[i] (NaN at i = 0), ratio[i] = d[i] / d[i+1] with numpy float
    semantics (x / 0 -> +-inf, 0 / 0 -> NaN), NaN at the first and the last row."""
    w = np.asarray(wss, dtype=np.float64).ravel()
    n = w.size
    d = np.full(n, np.nan)
    ratio = np.full(n, np.nan)
    if n > 1:
        d[1:] = -np.diff(w)
    if n > 2:
        with np.errstate(divide="ignore", invalid="ignore"):
            ratio[1:n - 1] = d[1:n - 1] / d[2:n]
    return w, d, ratio


def select_k(wss, min_clusters=MIN_CLUSTERS, max_clusters=MAX_CLUSTERS, wss_threshold=WSS_THRESHOLD, timepoint=None):
    """The elbow rule of the reference's Adaptive_clustering (_analyze_utils.py:73-88).

    wss[i] is the inertia of k = min_clusters + i, for k up to max_clusters.  With d_i = wss[i-1] - wss[i] and
    ratio_i = d_i / d_{i+1} (undefined for the first and the last k; x / 0 = +-inf and 0 / 0 = NaN as in numpy), the rows
    with d_i > wss_threshold * (max wss - min wss) are kept, and among them the k with the largest ratio wins; on ties the
    first (pandas idxmax), NaN ratios are skipped.  When no kept row has a defined ratio the reference fails (idxmax gives
    NaN, then a KeyError); here that is a ValueError naming the time point and showing the curve."""
    w, d, ratio = _curve(wss)
    if w.size != max_clusters - min_clusters + 1:
        raise ValueError(f"select_k needs one WSS value per k = {min_clusters} .. {max_clusters} (got {w.size})")
    thr = wss_threshold * (w.max() - w.min())
    with np.errstate(invalid="ignore"):
        ok = (d > thr) & ~np.isnan(ratio)
    if not ok.any():
        where = f" at time point {timepoint}" if timepoint is not None else ""
        curve = ", ".join(f"{min_clusters + i}: {v:.6g}" for i, v in enumerate(w.tolist()))
        raise ValueError(f"the WSS curve{where} has no elbow the adaptive rule can pick (WSS per k: {curve}); "
                         f"give the number of clusters per time point with --n_clusters")
    idx = np.flatnonzero(ok)
    best = idx[int(np.argmax(ratio[idx]))]                # first maximum (inf included)
    return int(min_clusters + best)


def wss_table(wss, selected, min_clusters=MIN_CLUSTERS):
    """The WSS table of one time point: columns clusters, wss, wss_diff, wss_diff_ratio, selected (a pandas DataFrame)."""
    import pandas as pd
    w, d, ratio = _curve(wss)
    ks = np.arange(min_clusters, min_clusters + w.size)
    return pd.DataFrame({"clusters": ks, "wss": w, "wss_diff": d, "wss_diff_ratio": ratio, "selected": ks == int(selected)})


def select_k_silhouette(scores, min_clusters=MIN_CLUSTERS, max_clusters=MAX_CLUSTERS, timepoint=None):
    """The silhouette rule of `analyze --criterion silhouette`: scores[i] is the silhouette score of the fit with
    k = min_clusters + i; the k with the largest score wins, on ties the first, NaN (an undefined labeling) is skipped.
    ValueError naming the time point when no score is defined."""
    s = np.asarray(scores, dtype=np.float64).ravel()
    if s.size != max_clusters - min_clusters + 1:
        raise ValueError(f"select_k_silhouette needs one score per k = {min_clusters} .. {max_clusters} (got {s.size})")
    ok = ~np.isnan(s)
    if not ok.any():
        where = f" at time point {timepoint}" if timepoint is not None else ""
        raise ValueError(f"no fit{where} has a defined silhouette score (k = {min_clusters} .. {max_clusters}); give the "
                         f"number of clusters per time point with --n_clusters")
    idx = np.flatnonzero(ok)
    return int(min_clusters + idx[int(np.argmax(s[idx]))])            # first maximum


def silhouette_table(scores, selected, min_clusters=MIN_CLUSTERS):
    """The silhouette table of one time point: columns clusters, silhouette, selected (a pandas DataFrame)."""
    import pandas as pd
    s = np.asarray(scores, dtype=np.float64).ravel()
    ks = np.arange(min_clusters, min_clusters + s.size)
    return pd.DataFrame({"clusters": ks, "silhouette": s, "selected": ks == int(selected)})


def select_k_bic(bics, min_clusters=MIN_CLUSTERS, max_clusters=MAX_CLUSTERS, timepoint=None):
    """The BIC rule of `analyze --method gmm --criterion bic`: bics[i] is the BIC of the mixture with k = min_clusters + i; the k
    with the smallest BIC wins, on ties the first, NaN (a fit that broke down) is skipped.  ValueError naming the time point when
    no BIC is defined."""
    b = np.asarray(bics, dtype=np.float64).ravel()
    if b.size != max_clusters - min_clusters + 1:
        raise ValueError(f"select_k_bic needs one BIC per k = {min_clusters} .. {max_clusters} (got {b.size})")
    ok = ~np.isnan(b)
    if not ok.any():
        where = f" at time point {timepoint}" if timepoint is not None else ""
        raise ValueError(f"no mixture{where} has a defined BIC (k = {min_clusters} .. {max_clusters}); give the number of "
                         f"clusters per time point with --n_clusters")
    idx = np.flatnonzero(ok)
    return int(min_clusters + idx[int(np.argmin(b[idx]))])            # first minimum


def bic_table(fits, selected, min_clusters=MIN_CLUSTERS):
    """The BIC table of one time point from its fitted mixtures (k ascending): columns clusters, bic, aic, log_likelihood, n_iter,
    converged, selected (a pandas DataFrame)."""
    import pandas as pd
    ks = np.arange(min_clusters, min_clusters + len(fits))
    return pd.DataFrame({"clusters": ks, "bic": [f.bic_ for f in fits], "aic": [f.aic_ for f in fits],
                         "log_likelihood": [f.log_likelihood_ for f in fits], "n_iter": [f.n_iter_ for f in fits],
                         "converged": [bool(f.converged_) for f in fits], "selected": ks == int(selected)})


def have_matplotlib():
    try:
        import matplotlib  # noqa: F401
        return True
    except ImportError:
        return False


def _figure(figsize):
    from matplotlib.backends.backend_agg import FigureCanvasAgg
    from matplotlib.figure import Figure
    fig = Figure(figsize=figsize)
    FigureCanvasAgg(fig)
    return fig


def plot_wss(path, clusters, wss, k_selected):
    """{prefix}{tp}_WSS_vs_Clusters.png (_analyze_utils.py:89-99)."""
    clusters, wss = list(clusters), list(wss)
    fig = _figure((10, 6))
    ax = fig.add_subplot(1, 1, 1)
    ax.plot(clusters, wss, marker="o")
    ax.scatter(k_selected, wss[clusters.index(k_selected)], color="red", s=100, label="Selected Cluster")
    ax.set_title("WSS vs Number of Clusters")
    ax.set_xlabel("Number of Clusters")
    ax.set_ylabel("WSS")
    ax.set_xticks(clusters)
    ax.grid()
    fig.savefig(path)


def plot_silhouette(path, clusters, scores, k_selected):
    """{prefix}{tp}_silhouette_vs_Clusters.png: the silhouette score of every k, the chosen one marked (as plot_wss)."""
    clusters, scores = list(clusters), list(scores)
    fig = _figure((10, 6))
    ax = fig.add_subplot(1, 1, 1)
    ax.plot(clusters, scores, marker="o")
    ax.scatter(k_selected, scores[clusters.index(k_selected)], color="red", s=100, label="Selected Cluster")
    ax.set_title("Silhouette score vs Number of Clusters")
    ax.set_xlabel("Number of Clusters")
    ax.set_ylabel("Silhouette score")
    ax.set_xticks(clusters)
    ax.grid()
    fig.savefig(path)


def plot_bic(path, clusters, bics, k_selected):
    """{prefix}{tp}_BIC_vs_Clusters.png: the BIC of every k, the chosen one marked (as plot_wss)."""
    clusters, bics = list(clusters), list(bics)
    fig = _figure((10, 6))
    ax = fig.add_subplot(1, 1, 1)
    ax.plot(clusters, bics, marker="o")
    ax.scatter(k_selected, bics[clusters.index(k_selected)], color="red", s=100, label="Selected Cluster")
    ax.set_title("BIC vs Number of Clusters")
    ax.set_xlabel("Number of Clusters")
    ax.set_ylabel("BIC")
    ax.set_xticks(clusters)
    ax.grid()
    fig.savefig(path)


def plot_domains(path, pixel_x, pixel_y, labels, timepoint):
    """{prefix}{tp}_domains.png: the spots coloured by K-means domain (_analyze_utils.py:140-164, there a seaborn scatter
    with the tab10 palette)."""
    import matplotlib
    fig = _figure((5, 5))
    ax = fig.add_subplot(1, 1, 1)
    cmap = matplotlib.colormaps["tab10"]
    labels = np.asarray(labels)
    for i, c in enumerate(np.unique(labels).tolist()):
        m = labels == c
        ax.scatter(np.asarray(pixel_x)[m], np.asarray(pixel_y)[m], s=10, color=cmap(i % 10), label=str(c), linewidths=0)
    ax.set_xlabel("pixel_x")
    ax.set_ylabel("pixel_y")
    ax.legend(title="kmeans", bbox_to_anchor=(1.05, 1), loc=2, borderaxespad=0.)
    ax.set_title("Time point: {}".format(timepoint))
    fig.tight_layout()
    fig.savefig(path)


def plot_territories(path, pixel_x, pixel_y, labels, small, timepoint, min_size):
    """{prefix}{tp}_territories.png: the spots coloured by domain as plot_domains draws them, the spots of territories of fewer
    than min_size spots ringed in black."""
    import matplotlib
    fig = _figure((5, 5))
    ax = fig.add_subplot(1, 1, 1)
    cmap = matplotlib.colormaps["tab10"]
    x, y, labels, small = np.asarray(pixel_x), np.asarray(pixel_y), np.asarray(labels), np.asarray(small, dtype=bool)
    for i, c in enumerate(np.unique(labels).tolist()):
        m = labels == c
        ax.scatter(x[m], y[m], s=10, color=cmap(i % 10), label=str(c), linewidths=0)
    ax.scatter(x[small], y[small], s=24, facecolors="none", edgecolors="black", linewidths=0.6,
               label=f"< {int(min_size)} spots")
    ax.set_xlabel("pixel_x")
    ax.set_ylabel("pixel_y")
    ax.legend(title="kmeans", bbox_to_anchor=(1.05, 1), loc=2, borderaxespad=0.)
    ax.set_title("Territories, time point: {}".format(timepoint))
    fig.tight_layout()
    fig.savefig(path)


def plot_depth(path, pixel_x, pixel_y, depth, timepoint):
    """{prefix}{tp}_centrality.png: the spots coloured by depth, the number of hops to the nearest spot of another domain (1: on
    a border); a spot that reaches no other domain (depth -1) is drawn grey."""
    fig = _figure((5.5, 5))
    ax = fig.add_subplot(1, 1, 1)
    x, y, depth = np.asarray(pixel_x), np.asarray(pixel_y), np.asarray(depth)
    far = depth < 0
    ax.scatter(x[far], y[far], s=10, color="lightgrey", linewidths=0)
    sc = ax.scatter(x[~far], y[~far], s=10, c=depth[~far], cmap="viridis", vmin=1, vmax=max(int(depth.max()), 2), linewidths=0)
    fig.colorbar(sc, ax=ax, label="hops to another domain")
    ax.set_xlabel("pixel_x")
    ax.set_ylabel("pixel_y")
    ax.set_title("Depth, time point: {}".format(timepoint))
    fig.tight_layout()
    fig.savefig(path)


def plot_nhood(path, zscore, timepoint):
    """{prefix}{tp}_nhood.png: the neighbourhood-enrichment z-scores of one time point as a heat map (domain by neighbor), on
    a diverging scale centred at 0; a cell without a z-score (no variance under permutation) stays blank."""
    z = np.asarray(zscore, dtype=np.float64)
    K = z.shape[0]
    finite = z[np.isfinite(z)]
    lim = float(np.abs(finite).max()) if finite.size and np.abs(finite).max() > 0 else 1.0
    fig = _figure((max(4.0, 0.5 * K + 2.0), max(3.5, 0.5 * K + 1.5)))
    ax = fig.add_subplot(1, 1, 1)
    im = ax.imshow(np.ma.masked_invalid(z), cmap="RdBu_r", vmin=-lim, vmax=lim)
    ax.set_xticks(range(K))
    ax.set_yticks(range(K))
    ax.set_xlabel("neighbor")
    ax.set_ylabel("domain")
    ax.set_title("Neighbourhood enrichment, time point: {}".format(timepoint))
    fig.colorbar(im, label="z-score", ax=ax)
    fig.tight_layout()
    fig.savefig(path)


def plot_cooccurrence(path, radii, ratio, timepoint, ring=False):
    """{prefix}{tp}_cooccurrence.png: one panel per domain, the co-occurrence ratio against the radius, one curve per
    neighbor, a line at 1 (no association); a ratio that is not defined leaves a gap."""
    import matplotlib
    r = np.asarray(radii, dtype=np.float64)
    v = np.asarray(ratio, dtype=np.float64)
    K = v.shape[0]
    cols = min(K, 4)
    rows = (K + cols - 1) // cols
    fig = _figure((3.6 * cols + 1.2, 2.8 * rows + 0.6))
    cmap = matplotlib.colormaps["tab20"]
    for a in range(K):
        ax = fig.add_subplot(rows, cols, a + 1)
        for b in range(K):
            ax.plot(r, v[a, b], color=cmap(b % 20), linewidth=2.0 if a == b else 1.0, label=str(b))
        ax.axhline(1.0, color="black", linewidth=0.8, linestyle="--")
        ax.set_title("domain {}".format(a))
        ax.set_xlabel("radius")
        ax.set_ylabel("ratio")
    handles, names = fig.axes[0].get_legend_handles_labels()
    fig.legend(handles, names, title="neighbor", loc="center right")
    fig.suptitle("Co-occurrence{}, time point: {}".format(" (rings)" if ring else "", timepoint))
    fig.tight_layout(rect=(0, 0, 1 - 1.0 / (3.6 * cols + 1.2), 0.96))
    fig.savefig(path)


def plot_cooccurrence_null(path, radii, ratio, ratio_sim_min, ratio_sim_max, timepoint, ring=False, relation=None):
    """{prefix}{tp}_cooccurrence_null.png: the curves of plot_cooccurrence, each over the envelope of its ratio under the
    relabelings as a band of its own colour; a pair whose verdict is not 'independent' is drawn solid, the others dotted."""
    import matplotlib
    r = np.asarray(radii, dtype=np.float64)
    v, lo, hi = (np.asarray(x, dtype=np.float64) for x in (ratio, ratio_sim_min, ratio_sim_max))
    K = v.shape[0]
    cols = min(K, 4)
    rows = (K + cols - 1) // cols
    fig = _figure((3.6 * cols + 1.2, 2.8 * rows + 0.6))
    cmap = matplotlib.colormaps["tab20"]
    for a in range(K):
        ax = fig.add_subplot(rows, cols, a + 1)
        for b in range(K):
            found = relation is None or str(relation[a][b]) != "independent"
            ax.fill_between(r, lo[a, b], hi[a, b], color=cmap(b % 20), alpha=0.2, linewidth=0)
            ax.plot(r, v[a, b], color=cmap(b % 20), linewidth=2.0 if a == b else 1.0, linestyle="-" if found else ":",
                    label=str(b))
        ax.axhline(1.0, color="black", linewidth=0.8, linestyle="--")
        ax.set_title("domain {}".format(a))
        ax.set_xlabel("radius")
        ax.set_ylabel("ratio")
    handles, names = fig.axes[0].get_legend_handles_labels()
    fig.legend(handles, names, title="neighbor", loc="center right")
    fig.suptitle("Co-occurrence{} against random labelling, time point: {}".format(" (rings)" if ring else "", timepoint))
    fig.tight_layout(rect=(0, 0, 1 - 1.0 / (3.6 * cols + 1.2), 0.96))
    fig.savefig(path)


def plot_ripley(path, radii, observed, sim_mean, sim_min, sim_max, timepoint, pattern=None):
    """{prefix}{tp}_ripley.png: one row per statistic (L, G, F), one panel per domain: the envelope of the simulations as a band,
    their mean dashed, the observed curve on top; a statistic that is not defined leaves its panel empty."""
    r = np.asarray(radii, dtype=np.float64)
    obs = np.asarray(observed, dtype=np.float64)
    K = obs.shape[1]
    fig = _figure((2.6 * K + 0.8, 7.2))
    for i, name in enumerate(("L", "G", "F")):
        for c in range(K):
            ax = fig.add_subplot(3, K, i * K + c + 1)
            if not np.all(np.isnan(obs[i, c])):
                ax.fill_between(r, np.asarray(sim_min)[i, c], np.asarray(sim_max)[i, c], color="0.8", linewidth=0)
                ax.plot(r, np.asarray(sim_mean)[i, c], color="0.4", linewidth=0.8, linestyle="--")
                ax.plot(r, obs[i, c], color="tab:red", linewidth=1.6)
            if i == 0:
                ax.set_title("domain {}{}".format(c, "" if pattern is None else "\n" + str(pattern[c])), fontsize=9)
            if i == 2:
                ax.set_xlabel("radius")
            if c == 0:
                ax.set_ylabel(name)
    fig.suptitle("Ripley's L, G and F, time point: {}".format(timepoint))
    fig.tight_layout(rect=(0, 0, 1, 0.96))
    fig.savefig(path)


def plot_correlogram(path, mids, I, expected, names, timepoint):
    """{prefix}{tp}_correlogram.png: Moran's I of the leading genes (the rows of I [genes, bands]) against the middle of the
    distance band, with its expectation under no autocorrelation as a dashed line."""
    fig = _figure((7.5, 5))
    ax = fig.add_subplot(1, 1, 1)
    for row, name in zip(np.asarray(I, dtype=np.float64), names):
        ax.plot(mids, row, marker="o", markersize=3, linewidth=1.2, label=str(name))
    ax.axhline(expected, color="0.4", linewidth=0.8, linestyle="--")
    ax.set_xlabel("distance")
    ax.set_ylabel("Moran's I")
    ax.set_title("Correlogram, time point: {}".format(timepoint))
    if len(names):
        ax.legend(fontsize=7, ncol=2)
    fig.tight_layout()
    fig.savefig(path)


def plot_embedding(path, Y, timepoint, labels=None):
    """{prefix}embedding.png: the t-SNE map of the latents in two panels, coloured by time point and by domain (the second panel
    says so where no domains table was given)."""
    import matplotlib
    fig = _figure((11, 5))
    cmap = matplotlib.colormaps["tab10"]
    Y = np.asarray(Y, dtype=np.float64)
    for pos, (title, values) in enumerate((("time point", timepoint), ("kmeans", labels))):
        ax = fig.add_subplot(1, 2, pos + 1)
        if values is None:
            ax.scatter(Y[:, 0], Y[:, 1], s=4, color="0.6", linewidths=0)
            ax.set_title("no domains table given")
        else:
            values = np.asarray(values)
            for i, c in enumerate(sorted(set(values.tolist()))):
                m = values == c
                ax.scatter(Y[m, 0], Y[m, 1], s=4, color=cmap(i % 10), label=str(c), linewidths=0)
            ax.legend(title=title, fontsize=7, markerscale=2)
            ax.set_title("by {}".format(title))
        ax.set_xlabel("tsne_1")
        ax.set_ylabel("tsne_2")
    fig.tight_layout()
    fig.savefig(path)


def transition_min_prob(table):
    """Element-wise minimum of the column-normalised and the row-normalised transition table (_analyze_utils.py:184-194)."""
    t = np.asarray(table, dtype=np.float64)
    with np.errstate(divide="ignore", invalid="ignore"):
        return np.minimum(t / t.sum(axis=0, keepdims=True), t / t.sum(axis=1, keepdims=True))


def plot_transition_dotplot(path, table, obs_names, var_names, prev_day, next_day):
    """{prefix}transition_dotplot_{d}_{d+1}.png (_analyze_utils.py:166-209): dot size and colour = transition_min_prob,
    grey below 0.2."""
    import matplotlib
    from matplotlib.cm import ScalarMappable
    v = transition_min_prob(table)
    reds = matplotlib.colormaps["Reds"]
    fig = _figure((v.shape[1] * 0.8, v.shape[0] * 0.8))
    ax = fig.add_subplot(1, 1, 1)
    for i in range(v.shape[0]):
        for j in range(v.shape[1]):
            value = v[i, j]
            color = "grey" if value < 0.2 else reds(value)
            ax.scatter(j, i, s=value * 500, c=[color], edgecolors="black", alpha=0.8)
    ax.set_xticks(range(v.shape[1]))
    ax.set_xticklabels(list(var_names), rotation=45, ha="right")
    ax.set_yticks(range(v.shape[0]))
    ax.set_yticklabels(list(obs_names))
    ax.set_xlabel("{} Domains".format(next_day))
    ax.set_ylabel("{} Domains".format(prev_day))
    ax.set_title("Transition Probability Dotplot")
    fig.colorbar(ScalarMappable(cmap="Reds"), label="Transition Probability", ax=ax)
    fig.tight_layout()
    fig.savefig(path)
