"""`analyze(args)`: mirror of the reference's SpaDOT/analyze.py -- the stage after `train`: K-means domains per time
point (a fixed k per time point, or the adaptive elbow rule over k = 4 .. 20), the spot-level optimal transport between
consecutive time points and its domain transition tables, and the plots.

Arguments (the reference's): data, output_dir (default: the data file's directory), prefix ('adaptive_' when n_clusters is
None and the prefix is empty), n_clusters (one k per time point, or None); added: device ('cuda:0'), write_tmaps (False),
lineage (False), criterion ('elbow' | 'silhouette' | 'bic': how the adaptive mode picks k; 'silhouette' scores all 17 fits of
every time point in one spadot_amd.silhouette.silhouette_many call and takes the k with the largest score), method
('kmeans' | 'gmm': with 'gmm' every labeling of the K-means sweep starts one full-covariance Gaussian mixture, all of them in
one spadot_amd.gmm.fit_sweep call; the domains are the mixtures' labels and every spot gets a membership probability per
domain; the adaptive mode then picks k by 'bic' (the smallest BIC) or 'silhouette' (of the mixtures' labels)).

Input: the latent.npz `train` always writes (X, rows, timepoint, spatial), latent.h5ad where `anndata` is importable, or an
in-memory object with .X, .obs['timepoint'], .obsm['spatial'].  Time points are taken sorted; days are their positions.

Outputs in output_dir:
  {prefix}domains.csv                          one row per input spot, in input order: row, timepoint, kmeans, pixel_x, pixel_y
  {prefix}{tp}_WSS.csv                         (adaptive) clusters, wss, wss_diff, wss_diff_ratio, selected
  {prefix}{tp}_silhouette.csv                  (adaptive, criterion silhouette) clusters, silhouette, selected; the WSS table's
                                               `selected` then marks the k the silhouette rule chose
  {prefix}transition_table_{d}_{d+1}.csv/.npz  analyze_ot.write_transition_tables (also OT_g.txt, OT/tmap_*.npz on request);
                                               .h5ad with the reference's names where anndata is importable
  {prefix}{tp}_WSS_vs_Clusters.png, {prefix}{tp}_domains.png, {prefix}transition_dotplot_{d}_{d+1}.png   (with matplotlib)
  {prefix}{tp}_silhouette_vs_Clusters.png      (criterion silhouette, with matplotlib)
With method gmm (`kmeans` in domains.csv then holds the mixture's label: markers, score and trends read that name):
  {prefix}{tp}_BIC.csv                         (adaptive) clusters, bic, aic, log_likelihood, n_iter, converged, selected
  {prefix}{tp}_BIC_vs_Clusters.png             (adaptive, with matplotlib)
  {prefix}memberships.npz                      X [N, sum_t K_t], rows, timepoint, names, in the layout of trajectories.npz: column
                                               '<tp>_<domain>' holds the responsibilities of that time point's spots, 0 elsewhere
                                               (`trends --trajectories` reads it: mean expression per soft domain)
  {prefix}gmm.npz                              per time point tp: weights_{tp}, means_{tp}, covariances_{tp}; timepoints
With lineage (spadot_amd.lineage: the plans of all pairs stay on the device and are chained, none is formed or solved twice):
  {prefix}transition_table_{d}_{e}.csv/.npz    for every e > d + 1: the long-range table, in the layout of the consecutive ones
                                               (.h5ad and transition_dotplot_{d}_{e}.png under the same conditions)
  {prefix}trajectories.npz                     X [N, sum_t K_t] in input row order, rows, timepoint, names ('<tp>_<domain>' per
                                               column: time points sorted, domains ascending): per domain, the distribution of
                                               its ancestors / descendants over the spots of every time point
  {prefix}fates.npz                            X [N, K_last], rows, timepoint, names: per spot, the share of its mass that ends in
                                               each domain of the last time point (the last time point's rows: their own domain)

The whole K-means work of the stage (17 k x 10 restarts per time point in adaptive mode) is ONE kmeans.fit_sweep call on the
MI355X; the reference refits the chosen k with the same seed, which reproduces the sweep's own fit for that k, so the labels
are taken from the sweep.
"""
import os
import time

import numpy as np

from .utils import _analyze_utils, _utils
from .utils._stage_utils import cuda_device, open_output, timepoint_masks

ADAPTIVE_KS = list(range(_analyze_utils.MIN_CLUSTERS, _analyze_utils.MAX_CLUSTERS + 1))


def _dense(X):
    return np.asarray(X.toarray() if hasattr(X, "toarray") else X)


def _rows(adata, n):
    obs = adata.obs
    if isinstance(obs, dict):
        return np.asarray(obs["row"]) if "row" in obs else np.arange(n)
    return np.asarray(obs.index)                      # AnnData: obs_names


def validate(n_clusters, counts, d):
    """Checks of the outside input, before any device work.  counts: spots per (sorted) time point; d: latent dimension.
    Returns the k values to fit per time point."""
    from .kmeans import check_sweep_shape
    T = len(counts)
    if n_clusters is None:
        for tp, n in counts.items():
            if n < ADAPTIVE_KS[-1]:
                raise ValueError(f"adaptive clustering fits k = {ADAPTIVE_KS[0]} .. {ADAPTIVE_KS[-1]}: time point {tp} has "
                                 f"only {n} spots; give --n_clusters")
        ks = [list(ADAPTIVE_KS) for _ in range(T)]
    else:
        n_clusters = [int(k) for k in n_clusters]
        if len(n_clusters) != T:
            raise ValueError(f"n_clusters has {len(n_clusters)} entries for {T} time points ({list(counts)}): give one k "
                             f"per time point")
        for (tp, n), k in zip(counts.items(), n_clusters):
            if not 1 <= k <= min(n, 32):
                raise ValueError(f"n_clusters = {k} for time point {tp} of {n} spots: k must be between 1 and "
                                 f"min(spots, 32) = {min(n, 32)}")
        ks = [[k] for k in n_clusters]
    if d > 32:
        raise ValueError(f"the latent has {d} dimensions; the device K-means supports at most 32")
    check_sweep_shape(d, max(k for kt in ks for k in kt))
    return ks


def analyze(args):
    criterion = getattr(args, "criterion", "elbow") or "elbow"
    method = getattr(args, "method", "kmeans") or "kmeans"
    if criterion not in ("elbow", "silhouette", "bic"):
        raise ValueError(f"criterion must be 'elbow', 'silhouette' or 'bic', not {criterion!r}")
    if method not in ("kmeans", "gmm"):
        raise ValueError(f"method must be 'kmeans' or 'gmm', not {method!r}")
    if criterion in ("silhouette", "bic") and getattr(args, "n_clusters", None) is not None:
        raise ValueError(f"--criterion {criterion} chooses the number of clusters: it cannot be combined with --n_clusters")
    if criterion == "bic" and method != "gmm":
        raise ValueError("--criterion bic is the BIC of Gaussian mixtures: it needs --method gmm")
    if method == "gmm" and criterion == "elbow" and getattr(args, "n_clusters", None) is None:
        raise ValueError("adaptive --method gmm needs --criterion bic or silhouette: the elbow rule reads the WSS curve of "
                         "K-means, and a mixture has no WSS")
    print("Loading latent representations...")
    adata, path = _utils.load_data(args.data)
    open_output(args, path)                               # the prefix of this stage depends on what follows
    if getattr(args, "prefix", None) is None:
        args.prefix = ""
    n_clusters = getattr(args, "n_clusters", None)
    if n_clusters is None and args.prefix == "":
        args.prefix = "adaptive_"
    prefix, out = args.prefix, args.output_dir
    device = getattr(args, "device", None) or "cuda:0"
    write_tmaps = bool(getattr(args, "write_tmaps", False))
    want_lineage = bool(getattr(args, "lineage", False))

    X = _dense(adata.X)
    tp_all = np.asarray(adata.obs["timepoint"])
    spatial = np.asarray(adata.obsm["spatial"])
    rows = _rows(adata, X.shape[0])
    tps, masks = timepoint_masks(tp_all)
    ks = validate(n_clusters, {tp: int(m.sum()) for tp, m in zip(tps, masks)}, int(X.shape[1]))
    if method == "gmm":
        from .gmm import check_shape
        check_shape(int(X.shape[1]), max(k for kt in ks for k in kt))

    import torch
    from . import analyze_ot, kmeans
    from .ops import kmeans_assign
    dev = cuda_device(args, "analyzes")
    timings = {}
    t0 = time.perf_counter()
    print("Clustering...")
    latents = [np.ascontiguousarray(X[m]) for m in masks]
    Xs = [torch.as_tensor(x, device=dev) for x in latents]
    adaptive = n_clusters is None
    by_silhouette = adaptive and criterion == "silhouette"
    use_gmm = method == "gmm"
    res = kmeans.fit_sweep(Xs, ks, random_state=1993, n_init=10,
                           labels_for=None if adaptive and not by_silhouette and not use_gmm else True)
    mix = None
    if use_gmm:                                           # every labeling of the sweep starts one mixture: one call
        from . import gmm
        t1 = time.perf_counter()
        mix = gmm.fit_sweep(Xs, [[res[t][k].labels_ for k in ks[t]] for t in range(len(tps))], n_components=ks,
                            resp_for=None if adaptive else True)
        timings["gmm"] = time.perf_counter() - t1
    sil_scores = None
    if by_silhouette:                                     # all T x 17 labelings of the sweep: one launch
        from .silhouette import silhouette_many
        t1 = time.perf_counter()
        sil_labels = [[(mix[t][i].labels_ if use_gmm else res[t][k].labels_) for i, k in enumerate(ADAPTIVE_KS)]
                      for t in range(len(tps))]
        sil = silhouette_many(Xs, sil_labels, n_clusters=[list(ADAPTIVE_KS) for _ in tps])
        sil_scores = [[r.score for r in st] for st in sil]
        timings["silhouette"] = time.perf_counter() - t1      # the results are on the host: the launch has finished
    chosen, labels, wss_tables, sil_tables, bic_tables, models = [], [], [], [], [], []
    for t, tp in enumerate(tps):
        if use_gmm:
            if not adaptive:
                k, i = ks[t][0], 0
            elif by_silhouette:
                k = _analyze_utils.select_k_silhouette(sil_scores[t], timepoint=tp)
                sil_tables.append(_analyze_utils.silhouette_table(sil_scores[t], k))
                i = ADAPTIVE_KS.index(k)
            else:
                k = _analyze_utils.select_k_bic([m.bic_ for m in mix[t]], timepoint=tp)
                i = ADAPTIVE_KS.index(k)
            if adaptive:
                bic_tables.append(_analyze_utils.bic_table(mix[t], k))
            models.append(mix[t][i])
            lab = mix[t][i].labels_
        elif by_silhouette:
            wss = [res[t][k].inertia_ for k in ADAPTIVE_KS]
            k = _analyze_utils.select_k_silhouette(sil_scores[t], timepoint=tp)
            wss_tables.append(_analyze_utils.wss_table(wss, k))
            sil_tables.append(_analyze_utils.silhouette_table(sil_scores[t], k))
            lab = res[t][k].labels_
        elif adaptive:
            wss = [res[t][k].inertia_ for k in ADAPTIVE_KS]
            k = _analyze_utils.select_k(wss, timepoint=tp)
            wss_tables.append(_analyze_utils.wss_table(wss, k))
            cen = torch.as_tensor(res[t][k].cluster_centers_, device=dev)
            lab = kmeans_assign(Xs[t].to(torch.float64), cen).cpu().numpy()   # the labels the sweep's fit of k gives
        else:
            k = ks[t][0]
            lab = res[t][k].labels_
        chosen.append(int(k))
        labels.append(np.asarray(lab, dtype=np.int64))
    memberships = None
    if use_gmm:
        if adaptive:                                      # the responsibilities of the chosen mixtures: one E-step launch
            from .gmm import estep_many
            resp = [o[0]["resp"] for o in estep_many(Xs, [[m] for m in models], resp=True)]
        else:
            resp = [m.resp_ for m in models]
        memberships = np.zeros((X.shape[0], int(sum(chosen))), dtype=np.float64)
        c0 = 0
        for m, r in zip(masks, resp):
            memberships[m, c0:c0 + r.shape[1]] = r
            c0 += r.shape[1]
        member_names = np.array([f"{tp}_{c}" for tp, k in zip(tps, chosen) for c in range(k)])
    torch.cuda.synchronize(dev)
    timings["clustering"] = time.perf_counter() - t0

    t0 = time.perf_counter()
    print("Optimal transport...")
    lin = None
    if not want_lineage:
        tables = analyze_ot.write_transition_tables(out, latents, labels, tps, prefix=prefix, device=device,
                                                    write_tmaps=write_tmaps)
        torch.cuda.synchronize(dev)
        timings["ot"] = time.perf_counter() - t0
    else:
        from . import lineage
        with lineage.TransportChain(latents, device=device) as chain:        # the same solves, kept
            tables = analyze_ot.write_transition_tables(out, latents, labels, tps, prefix=prefix, device=device,
                                                        write_tmaps=write_tmaps, chain=chain)
            torch.cuda.synchronize(dev)
            timings["ot"] = time.perf_counter() - t0
            t0 = time.perf_counter()
            print("Lineages...")
            lin = lineage.write_lineage(out, chain, labels, tps, masks, rows, tp_all, prefix=prefix)
            torch.cuda.synchronize(dev)
            timings["lineage"] = time.perf_counter() - t0

    t0 = time.perf_counter()
    import pandas as pd
    kcol = np.empty(X.shape[0], dtype=np.int64)
    for m, lab in zip(masks, labels):
        kcol[m] = lab
    pd.DataFrame({"row": rows, "timepoint": tp_all, "kmeans": kcol, "pixel_x": spatial[:, 0],
                  "pixel_y": spatial[:, 1]}).to_csv(os.path.join(out, prefix + "domains.csv"), index=False)
    for tp, tab in zip(tps, wss_tables):
        tab.to_csv(os.path.join(out, prefix + str(tp) + "_WSS.csv"), index=False)
    for tp, tab in zip(tps, sil_tables):
        tab.to_csv(os.path.join(out, prefix + str(tp) + "_silhouette.csv"), index=False)
    for tp, tab in zip(tps, bic_tables):
        tab.to_csv(os.path.join(out, prefix + str(tp) + "_BIC.csv"), index=False)
    if use_gmm:
        np.savez_compressed(os.path.join(out, prefix + "memberships.npz"), X=memberships, rows=np.asarray(rows),
                            timepoint=np.asarray(tp_all), names=member_names)
        arrays = {"timepoints": np.asarray([str(tp) for tp in tps])}
        for tp, m in zip(tps, models):
            arrays.update({f"weights_{tp}": m.weights_, f"means_{tp}": m.means_, f"covariances_{tp}": m.covariances_})
        np.savez_compressed(os.path.join(out, prefix + "gmm.npz"), **arrays)
    pairs = [(d, d + 1, tab) for d, tab in enumerate(tables)]
    if lin is not None:
        pairs += [(d, e, tab) for (d, e), tab in sorted(lin["long_tables"].items())]
    names = [([f"{tps[d]}_{c}" for c in range(tab.shape[0])], [f"{tps[e]}_{c}" for c in range(tab.shape[1])])
             for d, e, tab in pairs]
    try:
        import anndata
        for (d, e, tab), (obs, var) in zip(pairs, names):              # the reference's files (tools/npz_to_h5ad.py's mapping)
            anndata.AnnData(np.asarray(tab), obs=pd.DataFrame(index=obs), var=pd.DataFrame(index=var)).write_h5ad(
                os.path.join(out, f"{prefix}transition_table_{d}_{e}.h5ad"))
    except ImportError:
        pass
    if _analyze_utils.have_matplotlib():
        for t, tp in enumerate(tps):
            if use_gmm and adaptive:
                _analyze_utils.plot_bic(os.path.join(out, f"{prefix}{tp}_BIC_vs_Clusters.png"), ADAPTIVE_KS,
                                        bic_tables[t]["bic"].tolist(), chosen[t])
            if adaptive and not use_gmm:
                _analyze_utils.plot_wss(os.path.join(out, f"{prefix}{tp}_WSS_vs_Clusters.png"), ADAPTIVE_KS,
                                        wss_tables[t]["wss"].tolist(), chosen[t])
            if by_silhouette:
                _analyze_utils.plot_silhouette(os.path.join(out, f"{prefix}{tp}_silhouette_vs_Clusters.png"), ADAPTIVE_KS,
                                               sil_scores[t], chosen[t])
            _analyze_utils.plot_domains(os.path.join(out, f"{prefix}{tp}_domains.png"), spatial[masks[t], 0],
                                        spatial[masks[t], 1], labels[t], tp)
        for (d, e, tab), (obs, var) in zip(pairs, names):
            _analyze_utils.plot_transition_dotplot(os.path.join(out, f"{prefix}transition_dotplot_{d}_{e}.png"), tab, obs,
                                                   var, d, e)
    else:
        print("matplotlib not installed: no plots")
    timings["writing"] = time.perf_counter() - t0
    print("Results written to %s" % out)
    res = {"timepoints": tps, "labels": dict(zip(tps, labels)), "n_clusters": chosen, "tables": tables, "timings": timings}
    if by_silhouette:
        res["silhouette"] = dict(zip(tps, sil_scores))
        res["criterion"] = criterion
    if use_gmm:
        res["method"] = method
        res["bic"] = dict(zip(tps, ([m.bic_ for m in mt] for mt in mix)))
        res["memberships"] = {"X": memberships, "names": member_names, "rows": rows, "timepoint": tp_all}
        if adaptive and not by_silhouette:
            res["criterion"] = criterion
    if lin is not None:
        res["lineage"] = dict(lin, rows=rows, timepoint=tp_all)
    return res
