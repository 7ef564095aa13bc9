"""What the analysis stages share on the host.  What only the three Moran stages share is in spadot_amd/moran.py,
what only the two pair-counting stages share in spadot_amd/pairs.py.

The frame of a stage driver, as small functions that every driver calls in its own order (the order in which a driver refuses
its arguments is part of its behaviour):
    load_marker_counts(data), read_domains(domains, timepoint)     the counts and the domain labels of the stages that read them
    align_rows(rows, said, timepoint, ...)                         the rows of a table against the rows of the data
    need_domains(args, stage), read_domains_table(args, stage)     the domains table of the stages that read nothing else
    timepoint_masks(timepoint)                                     the sorted time points and the rows of each
    top_setting(args, default, least), open_output(args, beside), cuda_device(args, what)
    write_timepoints(path, stem, tps, results, table, fields)      one csv and the '{tp}_{field}' arrays per time point
    plot_timepoints(tps, results, plot)                            the plots, or the line that says why there are none
    Stage, open_stage(..), timings(..)                             the opening of a stage that reads counts and builds graphs
and labeling_runs, edge_pair and savez_pinned."""
import collections
import os
import time
import zipfile

import numpy as np

MAX_EDGES = 2147483647


def labeling_runs(n_perms, observed, first, per, budget):
    """The labelings of a call -- the observed one, if any, then the permutations first .. first + n_perms - 1 -- in runs that
    share one buffer of `budget` units at `per` units a labeling: [(observed in the run, its first permutation, its
    permutations)].  One run where everything fits; otherwise max(1, budget // per) labelings a run, the observed one in the
    first."""
    observed, n_perms, first = int(bool(observed)), int(n_perms), int(first)
    L = observed + n_perms
    step = L if per * L <= budget else max(1, budget // per)
    runs = []
    for l in range(0, L, step):                                  # l: the labelings ahead of the run, the observed one included
        obs = observed if l == 0 else 0
        runs.append((bool(obs), first + l - (observed - obs), min(step, L - l) - obs))
    return runs


def edge_pair(e, dev, g):
    """The (src, dst) of graph g as 1-d integer device tensors on `dev` (None: wherever they are)."""
    import torch
    src, dst = e
    src = src if isinstance(src, torch.Tensor) else torch.as_tensor(np.asarray(src))
    dst = dst if isinstance(dst, torch.Tensor) else torch.as_tensor(np.asarray(dst))
    for t in (src, dst):
        if not t.is_cuda:
            raise RuntimeError("spadot_amd counts neighbourhoods on the MI355X only (got a CPU tensor); there is no CPU path")
        if t.dim() != 1 or t.dtype.is_floating_point or t.dtype == torch.bool or t.dtype.is_complex:
            raise ValueError(f"the edges of graph {g} must be two 1-d integer tensors (got {tuple(t.shape)} {t.dtype})")
    if src.shape != dst.shape or src.device != dst.device or (dev is not None and src.device != dev):
        raise ValueError(f"the sources and targets of graph {g} must have one length and all graphs one device")
    if src.shape[0] > MAX_EDGES:
        raise ValueError(f"graph {g} has {src.shape[0]} edges: the device takes at most {MAX_EDGES} per graph")
    return src, dst


def savez_pinned(path, arrays):
    """np.savez with the archive's time stamps pinned, so that two runs write the same bytes (np.load reads it as any npz)."""
    with zipfile.ZipFile(path, "w", zipfile.ZIP_STORED, allowZip64=True) as z:
        for name, v in arrays.items():
            info = zipfile.ZipInfo(name + ".npy", date_time=(1980, 1, 1, 0, 0, 0))
            with z.open(info, "w", force_zip64=True) as f:
                np.lib.format.write_array(f, np.asanyarray(v), allow_pickle=False)


def load_marker_counts(data):
    """The counts the stages read: the .npz `preprocess` writes (its X holds scaled values; the raw counts of the selected genes
    are its counts_data / counts_indices / counts_indptr / counts_shape), or anything load_counts reads.  Returns (RawCounts,
    absolute path or None)."""
    from ._preprocess_utils import RawCounts, _to_csr, load_counts
    if isinstance(data, (str, os.PathLike)) and str(data).endswith(".npz"):
        path = os.path.abspath(data)
        z = np.load(path, allow_pickle=False)
        if "counts_data" in z.files:
            import scipy.sparse as sp
            for key in ("timepoint", "spatial"):
                if key not in z.files:
                    raise ValueError(f"{path} has no `{key}` array")
            shape = tuple(int(v) for v in z["counts_shape"])
            X = sp.csr_matrix((z["counts_data"], z["counts_indices"], z["counts_indptr"]), shape=shape)
            genes = z["genes"] if "genes" in z.files else np.arange(shape[1]).astype(str)
            if len(z["timepoint"]) != shape[0] or len(genes) != shape[1]:
                raise ValueError(f"{path}: counts of shape {shape} against {len(z['timepoint'])} time point entries and "
                                 f"{len(genes)} gene names")
            return RawCounts(_to_csr(X), z["timepoint"], np.asarray(z["spatial"], dtype=np.float64), genes), path
    return load_counts(data)


def align_rows(rows, said, timepoint, column, table, twice, missing, show=repr):
    """The row numbers `rows` of a table against the data's time point per row: integers in 0 .. n-1, every row of the data
    exactly once, and `said`, the table's time point per entry, equal to the data's (as strings).  Returns the rows as int64;
    ValueError otherwise, in the words of the caller: `column` holds the rows, `table` names them, a row `twice` or of the data
    `missing`, and show() writes a time point."""
    tp = np.asarray(timepoint)
    n = tp.shape[0]
    row = np.asarray(rows)
    if row.dtype.kind not in "iu":
        raise ValueError(f"{column} must hold integer row numbers of the data")
    row = row.astype(np.int64)
    if row.size and (row.min() < 0 or row.max() >= n):
        raise ValueError(f"{table} names row {int(row.max() if row.max() >= n else row.min())}: the data has rows 0 .. {n - 1}")
    seen = np.bincount(row, minlength=n)
    if np.any(seen > 1):
        raise ValueError(f"row {int(np.flatnonzero(seen > 1)[0])} {twice} ({int((seen > 1).sum())} duplicate rows)")
    if np.any(seen == 0):
        raise ValueError(f"row {int(np.flatnonzero(seen == 0)[0])} of the data {missing} ({int((seen == 0).sum())} missing rows)")
    said = np.asarray(said)
    bad = np.flatnonzero(said.astype(str) != tp[row].astype(str))
    if bad.size:
        r = int(row[bad[0]])
        raise ValueError(f"time point mismatch at row {r}: {table} says {show(said[bad[0]])}, the data says {show(tp[r])} "
                         f"({bad.size} rows differ)")
    return row


def read_domains(domains, timepoint):
    """Domain label of every row of the data from the domains table of analyze (columns row, timepoint, kmeans; a path or a
    DataFrame).  `timepoint`: the data's time point per row.  Every row must be labelled exactly once, with the data's time
    point, and no time point may have more than 32 domains: ValueError otherwise."""
    import pandas as pd
    from ..markers import check_labels
    df = pd.read_csv(domains) if isinstance(domains, (str, os.PathLike)) else domains
    for col in ("row", "timepoint", "kmeans"):
        if col not in df.columns:
            raise ValueError(f"the domains table has no `{col}` column (expected the domains.csv that analyze writes)")
    row = align_rows(df["row"], df["timepoint"], timepoint, "the `row` column of the domains table", "the domains table",
                     "is labelled more than once in the domains table", "has no label in the domains table")
    labels = np.empty(row.shape[0], dtype=np.int64)
    labels[row] = np.asarray(df["kmeans"])
    return check_labels(labels, np.asarray(timepoint))[0]


def need_domains(args, stage):
    """args.domains, a path or a DataFrame; ValueError in the name of the stage without one."""
    domains = getattr(args, "domains", None)
    if domains is None or (isinstance(domains, str) and not domains):
        raise ValueError(f"the {stage} stage needs the domains table of analyze (--domains)")
    return domains


def timepoint_masks(timepoint):
    """(the time points sorted, per time point the bool mask of its rows)."""
    tps = sorted(set(timepoint.tolist()))
    return tps, [timepoint == tp for tp in tps]


DomainsTable = collections.namedtuple("DomainsTable", "n tp_all row_ids labels coords tps masks Ks beside")


def read_domains_table(args, stage):
    """The domains table of a stage that reads nothing else (neighbors, cooccurrence, ripley), in the table's own order: n rows,
    tp_all and row_ids per row, labels int64 (K <= 32 per time point), coords fp64 [n, 2], the time points sorted with their
    masks and domain counts Ks, and `beside`: what open_output takes for the default output directory.  ValueError, in this
    order, for no --domains, a missing column, an empty table, rows that read_domains refuses and coordinates that are not
    finite."""
    import pandas as pd
    domains = need_domains(args, stage)
    df = pd.read_csv(domains) if isinstance(domains, (str, os.PathLike)) else domains
    for col in ("pixel_x", "pixel_y", "timepoint", "kmeans"):
        if col not in df.columns:
            raise ValueError(f"the domains table has no `{col}` column (expected the domains.csv that analyze writes)")
    n = len(df)
    if n == 0:
        raise ValueError("the domains table is empty")
    tp_all = np.asarray(df["timepoint"])
    row_ids = np.asarray(df["row"]) if "row" in df.columns else np.arange(n)
    labels = read_domains(df.assign(row=np.arange(n)), tp_all).astype(np.int64)
    coords = np.stack([np.asarray(df["pixel_x"], dtype=np.float64), np.asarray(df["pixel_y"], dtype=np.float64)], axis=1)
    if not np.all(np.isfinite(coords)):
        raise ValueError("the domains table holds spots without finite pixel_x / pixel_y")
    tps, masks = timepoint_masks(tp_all)
    return DomainsTable(n, tp_all, row_ids, labels, coords, tps, masks, [int(labels[m].max()) + 1 for m in masks], domains)


def top_setting(args, default, least=None):
    """args.top as an int (`default` where it is absent or None); with `least`, ValueError for a smaller one."""
    top = getattr(args, "top", default)
    top = default if top is None else int(top)
    if least is not None and top < least:
        raise ValueError(f"top must be 0 (all genes) or a positive count, not {top}")
    return top


def open_output(args, beside):
    """args.output_dir, by default the directory of the input `beside` (a path; anything else: the working directory), is
    created.  Returns path(name): the file {output_dir}/{args.prefix}{name}."""
    if not getattr(args, "output_dir", None):
        args.output_dir = os.path.dirname(os.path.abspath(beside)) if isinstance(beside, (str, os.PathLike)) else os.getcwd()
    os.makedirs(args.output_dir, exist_ok=True)
    out_dir, prefix = args.output_dir, getattr(args, "prefix", "") or ""
    return lambda name: os.path.join(out_dir, prefix + name)


def cuda_device(args, what):
    """torch.device(args.device or 'cuda:0'), asked for when this is called and not before; RuntimeError ("spadot_amd {what}
    on the MI355X only") for one that is not cuda."""
    import torch
    dev = torch.device(getattr(args, "device", None) or "cuda:0")
    if dev.type != "cuda":
        raise RuntimeError(f"spadot_amd {what} on the MI355X only (device 'cuda:N'); there is no CPU path")
    return dev


def write_timepoints(path, stem, tps, results, table, fields, arrays=None, more=None):
    """Per time point tp with result r, number t: table(t, r) goes to path('{stem}_{tp}.csv') and getattr(r, field) of every
    field, then the entries of more(t, r), to arrays['{tp}_{field}'] (arrays: what the archive holds ahead of them).  Returns
    (tables by time point, arrays)."""
    tables, arrays = {}, {} if arrays is None else arrays
    for t, (tp, r) in enumerate(zip(tps, results)):
        tables[tp] = table(t, r)
        tables[tp].to_csv(path(f"{stem}_{tp}.csv"), index=False)
        for name in fields:
            arrays[f"{tp}_{name}"] = getattr(r, name)
        for name, v in (more(t, r) if more else {}).items():
            arrays[f"{tp}_{name}"] = v
    return tables, arrays


def plot_timepoints(tps, results, plot):
    """plot(tp, r) for every time point where matplotlib is installed; a line on stdout where it is not."""
    from . import _analyze_utils
    if _analyze_utils.have_matplotlib():
        for tp, r in zip(tps, results):
            plot(tp, r)
    else:
        print("matplotlib not installed: no plots")


class Stage:
    """What open_stage hands to a stage: dev, dc (the DeviceCounts), tps, off (dc.tp_off_host), edges (spatial_edges per time
    point), path (of open_output), extras (what the stage's own `resolve` returned) and the clock marks t_start, t_read,
    t_graph."""

    def rows(self, t):
        """The rows of time point t in the order of the DeviceCounts."""
        return slice(int(self.off[t]), int(self.off[t + 1]))


def open_stage(args, k, what, t_start, resolve=None):
    """The opening of a stage on the counts and their spatial graphs: the device must be cuda ("spadot_amd takes {what} on the
    MI355X only"), the counts of args.data are read (load_marker_counts), resolve(raw) takes what the stage reads of its other
    arguments -- before anything is written, so that an unknown name raises first --, args.output_dir defaults to the directory
    of the data and is created, the counts go to the device, the coordinates must be finite and every time point gets its
    spatial_edges(.., k)."""
    import torch
    from ..neighbors import spatial_edges
    from ..preprocess import DeviceCounts
    st = Stage()
    st.t_start = t_start
    st.dev = cuda_device(args, f"takes {what}")
    raw, path = load_marker_counts(args.data)
    st.extras = resolve(raw) if resolve else None
    st.path = open_output(args, path)
    st.dc = DeviceCounts(raw, st.dev)
    if not np.all(np.isfinite(st.dc.spatial)):
        raise ValueError("the data holds spots without finite spatial coordinates")
    st.tps, st.off = [str(t) for t in st.dc.tps], st.dc.tp_off_host
    st.t_read = time.perf_counter()
    st.edges = [spatial_edges(st.dc.spatial[st.rows(t)], k, st.dev) for t in range(st.dc.T)]
    torch.cuda.synchronize(st.dev)
    st.t_graph = time.perf_counter()
    return st


def timings(t_start, t_read, t_dev, t_end, t_graph=None):
    """The `timings` of a stage's result from its clock marks: t_read after the input is read, t_graph (where the stage builds
    graphs) after they are built, t_dev after the device part, t_end after the files are written."""
    out = dict(read_s=t_read - t_start)
    if t_graph is not None:
        out["graph_s"] = t_graph - t_read
    out.update(device_s=t_dev - (t_read if t_graph is None else t_graph), write_s=t_end - t_dev, total_s=t_end - t_start)
    return out
