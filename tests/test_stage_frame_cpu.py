"""The frame the eleven stage drivers share (spadot_amd/utils/_stage_utils.py), without a device: which refusal
every driver gives, which of two faults wins, whether the output directory exists after it, and that a well-formed input gets as
far as the device and no further.  The expectations are what the drivers did when each carried its own copy of the frame.  Then
the helpers on their own: the row alignment against the two copies it replaced, the per-time-point writer and the timings."""
import argparse
import os

import numpy as np
import pytest

TPS = ("E10", "E12")
SIZES = (12, 18)
N, G = sum(SIZES), 8


class Inputs:
    """2 time points of 12 and 18 rows, 3 domains, 8 genes: counts.npz, latent.npz, the domains table (a DataFrame and a csv),
    interactions.csv, trajectories.npz, and `out`, a directory that does not exist yet."""

    def __init__(self, root):
        import pandas as pd
        rng = np.random.default_rng(5)
        self.root, self.out = str(root), str(root / "out")
        tp = np.repeat(np.asarray(TPS), SIZES)
        xy = rng.random((N, 2)) * 100.0
        genes = np.asarray([f"g{i}" for i in range(G)])
        self.counts = str(root / "counts.npz")
        np.savez(self.counts, X=rng.poisson(2.0, (N, G)).astype(np.float32), timepoint=tp, spatial=xy, genes=genes)
        self.latent = str(root / "latent.npz")
        np.savez(self.latent, X=rng.standard_normal((N, 4)).astype(np.float32), rows=np.arange(N), timepoint=tp, spatial=xy)
        self.table = pd.DataFrame({"row": np.arange(N), "timepoint": tp, "kmeans": np.arange(N) % 3, "pixel_x": xy[:, 0],
                                   "pixel_y": xy[:, 1]})
        self.domains = str(root / "domains.csv")
        self.table.to_csv(self.domains, index=False)
        self.pairs = str(root / "interactions.csv")
        pd.DataFrame({"source": ["g0", "g1", "g2"], "target": ["g3", "g4", "g5"]}).to_csv(self.pairs, index=False)
        self.strangers = str(root / "strangers.csv")
        pd.DataFrame({"source": ["x0"], "target": ["x1"]}).to_csv(self.strangers, index=False)
        self.traj = str(root / "trajectories.npz")
        np.savez(self.traj, X=rng.random((N, 2)), rows=np.arange(N), timepoint=tp, names=np.asarray(["a", "b"]))
        self.traj_twice = str(root / "twice.npz")
        np.savez(self.traj_twice, X=rng.random((N, 2)), rows=np.r_[0, np.arange(N - 1)], timepoint=np.r_[tp[:1], tp[:-1]],
                 names=np.asarray(["a", "b"]))
        self.missing = str(root / "nowhere.npz")

    def twice(self):
        import pandas as pd
        return pd.concat([self.table, self.table.iloc[:1]], ignore_index=True)

    def twice_csv(self):
        """markers, hotspots and interactions take the table as a path only."""
        path = os.path.join(self.root, "twice.csv")
        self.twice().to_csv(path, index=False)
        return path


def _driver(name):
    import importlib
    module, fn = {"markers": ("markers", "markers"), "score": ("silhouette", "score"), "trends": ("trends", "trends"),
                  "neighbors": ("neighbors", "neighbors"), "cooccur": ("cooccurrence", "cooccur"),
                  "ripley_stage": ("ripley", "ripley_stage"), "autocorr": ("autocorr", "autocorr"),
                  "hotspots": ("hotspots", "hotspots"), "modules": ("modules", "modules"),
                  "interactions": ("ligrec", "interactions"), "analyze": ("analyze", "analyze")}[name]
    return getattr(importlib.import_module("spadot_amd." + module), fn)


def _base(name, inp):
    """A well-formed argument set of the driver."""
    if name in ("neighbors", "cooccur", "ripley_stage"):
        return dict(domains=inp.table)
    if name == "score":
        return dict(data=inp.latent, domains=inp.table)
    if name == "analyze":
        return dict(data=inp.latent, n_clusters=[2, 2])
    if name == "trends":
        return dict(data=inp.counts, trajectories=inp.traj)
    if name == "interactions":
        return dict(data=inp.counts, domains=inp.domains, interactions=inp.pairs)
    if name == "markers":
        return dict(data=inp.counts, domains=inp.domains)
    return dict(data=inp.counts)


DEVICE = "the device was asked for"          # what the torch.device of these tests raises: an AssertionError

# (driver, case, what the case changes of the well-formed arguments (a callable: of the Inputs), the exception, a fragment of its
#  message, whether the output directory exists afterwards).  Every case runs with torch.device replaced by a function that
#  raises, so a case that expects another exception also says that the device was not asked for before it.
CASES = [
    ("markers", "no domains", dict(domains=None), ValueError, "the markers stage needs the domains table of analyze (--domains)", False),
    ("markers", "a row twice", lambda i: dict(domains=i.twice_csv()), ValueError, "row 0 is labelled more than once in the domains table (1 duplicate rows)", False),
    ("markers", "bad top and no data file", lambda i: dict(top=-1, data=i.missing), FileNotFoundError, "nowhere.npz", False),
    ("markers", "bad top", dict(top=-1), ValueError, "top must be 0 (all genes) or a positive count, not -1", True),
    ("markers", "well-formed", {}, AssertionError, DEVICE, True),
    ("score", "no domains", dict(domains=None), ValueError, "the score stage needs the domains table of analyze (--domains)", False),
    ("score", "a row twice", lambda i: dict(domains=i.twice()), ValueError, "is labelled more than once in the domains table", False),
    ("score", "a row missing", lambda i: dict(domains=i.table.iloc[1:]), ValueError, "row 0 of the data has no label in the domains table (1 missing rows)", False),
    ("score", "well-formed", {}, AssertionError, DEVICE, True),
    ("trends", "no lineage", dict(trajectories=None), ValueError, "the trends stage needs trajectories.npz and / or fates.npz", False),
    ("trends", "bad top and no data file", lambda i: dict(top=-1, data=i.missing), ValueError, "top must be 0 (all genes) or a positive count, not -1", False),
    ("trends", "no data file", lambda i: dict(data=i.missing), FileNotFoundError, "nowhere.npz", False),
    ("trends", "a row twice", lambda i: dict(trajectories=i.traj_twice), ValueError, "row 0 appears more than once in", False),
    ("trends", "well-formed", {}, AssertionError, DEVICE, True),
    ("neighbors", "bad device and no domains", dict(device="cpu", domains=None), ValueError, "the neighbors stage needs the domains table of analyze (--domains)", False),
    ("neighbors", "an empty path", dict(domains=""), ValueError, "the neighbors stage needs the domains table", False),
    ("neighbors", "no pixel_x", lambda i: dict(domains=i.table.drop(columns="pixel_x")), ValueError, "the domains table has no `pixel_x` column (expected the domains.csv that analyze writes)", False),
    ("neighbors", "an empty table", lambda i: dict(domains=i.table.iloc[:0]), ValueError, "the domains table is empty", False),
    ("neighbors", "a NaN coordinate", lambda i: dict(domains=i.table.assign(pixel_y=np.nan)), ValueError, "the domains table holds spots without finite pixel_x / pixel_y", False),
    ("neighbors", "33 domains", lambda i: dict(domains=i.table.assign(kmeans=np.r_[np.arange(12) % 3, [40] * 18])), ValueError, "at most 32 per time point", False),
    ("neighbors", "bad k", dict(k=0), ValueError, "the neighbors stage takes k >= 1 and n_perms >= 1 (got k = 0, n_perms = 1000)", False),
    ("neighbors", "well-formed", {}, AssertionError, DEVICE, True),
    ("cooccur", "too many relabelings and no domains", dict(n_perms=10000, domains=None), ValueError, "the cooccurrence stage takes 0 to 9999 relabelings (got n_perms = 10000)", False),
    ("cooccur", "no domains", dict(domains=None), ValueError, "the cooccurrence stage needs the domains table of analyze (--domains)", False),
    ("cooccur", "no kmeans", lambda i: dict(domains=i.table.drop(columns="kmeans")), ValueError, "the domains table has no `kmeans` column", False),
    ("cooccur", "an empty table", lambda i: dict(domains=i.table.iloc[:0]), ValueError, "the domains table is empty", False),
    ("cooccur", "an infinite coordinate", lambda i: dict(domains=i.table.assign(pixel_x=np.inf)), ValueError, "without finite pixel_x / pixel_y", False),
    ("cooccur", "bad bins and a bad device", dict(bins=0, device="cpu"), ValueError, "the cooccurrence stage takes 1 to 64 radii (got bins = 0)", False),
    ("cooccur", "well-formed", {}, AssertionError, DEVICE, True),
    ("ripley_stage", "no domains", dict(domains=None), ValueError, "the ripley stage needs the domains table of analyze (--domains)", False),
    ("ripley_stage", "no timepoint", lambda i: dict(domains=i.table.drop(columns="timepoint")), ValueError, "the domains table has no `timepoint` column", False),
    ("ripley_stage", "an empty table", lambda i: dict(domains=i.table.iloc[:0]), ValueError, "the domains table is empty", False),
    ("ripley_stage", "a NaN coordinate", lambda i: dict(domains=i.table.assign(pixel_x=np.nan)), ValueError, "without finite pixel_x / pixel_y", False),
    ("ripley_stage", "bad bins and a bad device", dict(bins=65, device="cpu"), ValueError, "the ripley stage takes 1 to 64 radii (got bins = 65)", False),
    ("ripley_stage", "bad mode", dict(mode="L,X"), ValueError, "modes are taken from L, G and F", False),
    ("ripley_stage", "bad window", dict(window="disc"), ValueError, "the ripley stage takes the window 'hull' or 'box' (got 'disc')", False),
    ("ripley_stage", "well-formed", {}, AssertionError, DEVICE, True),
    ("autocorr", "bad top", dict(top=-1), ValueError, "the autocorr stage takes top >= 0, k >= 1 and n_perms >= 0 (got top = -1, k = 6, n_perms = 100)", False),
    ("autocorr", "bad k and no data file", lambda i: dict(k=0, data=i.missing), ValueError, "the autocorr stage takes top >= 0, k >= 1", False),
    ("autocorr", "well-formed: the device before the data", lambda i: dict(data=i.missing), AssertionError, DEVICE, False),
    ("hotspots", "bad top", dict(top=0), ValueError, "the hotspots stage takes top >= 1, k >= 1, n_perms >= 1 and 0 < alpha <= 1 (got top = 0, k = 6, n_perms = 999, alpha = 0.05)", False),
    ("hotspots", "well-formed: the device before the genes", dict(genes="g1,nope"), AssertionError, DEVICE, False),
    ("modules", "bad top", dict(top=0), ValueError, "the modules stage takes top >= 1, k >= 1, n_perms >= 1, min_sim <= 1, min_genes >= 1, 0 < alpha <= 1 and top_pairs >= 0 (got top = 0,", False),
    ("modules", "well-formed: the device before the genes", dict(genes="g1,nope"), AssertionError, DEVICE, False),
    ("interactions", "bad threshold", dict(threshold=2.0), ValueError, "the ligrec stage takes top >= 0, n_perms >= 0 and 0 <= threshold <= 1 (got top = 100, n_perms = 1000, threshold = 2.0)", False),
    ("interactions", "well-formed: the device before the domains", dict(domains=None), AssertionError, DEVICE, False),
    ("analyze", "bad criterion", dict(criterion="aic"), ValueError, "criterion must be 'elbow', 'silhouette' or 'bic', not 'aic'", False),
    ("analyze", "one k for two time points", dict(n_clusters=[2]), ValueError, "n_clusters has 1 entries for 2 time points", True),
    ("analyze", "well-formed", {}, AssertionError, DEVICE, True),
]

# The same, with torch.device as it is: what a device that is not cuda meets, and what is refused after a cuda device was named
# (naming one needs no GPU).
CASES_WITH_DEVICE = [
    ("score", "bad device", dict(device="cpu"), RuntimeError, "spadot_amd scores silhouettes on the MI355X only (device 'cuda:N'); there is no CPU path", True),
    ("neighbors", "bad device", dict(device="cpu"), RuntimeError, "spadot_amd counts neighbourhoods on the MI355X only (device 'cuda:N'); there is no CPU path", True),
    ("cooccur", "bad device", dict(device="cpu"), RuntimeError, "spadot_amd counts co-occurrences on the MI355X only (device 'cuda:N'); there is no CPU path", True),
    ("ripley_stage", "bad device", dict(device="cpu"), RuntimeError, "spadot_amd counts Ripley's functions on the MI355X only (device 'cuda:N'); there is no CPU path", True),
    ("analyze", "bad device", dict(device="cpu"), RuntimeError, "spadot_amd analyzes on the MI355X only (device 'cuda:N'); there is no CPU path", True),
    ("markers", "bad device", dict(device="cpu"), ValueError, "the markers stage runs on the MI355X (a cuda device), not on 'cpu'", True),
    ("trends", "bad device", dict(device="cpu"), ValueError, "the trends stage runs on the MI355X (a cuda device), not on 'cpu'", True),
    ("autocorr", "bad device and no data file", lambda i: dict(device="cpu", data=i.missing), RuntimeError, "spadot_amd takes the autocorrelation on the MI355X only (device 'cuda:N'); there is no CPU path", False),
    ("autocorr", "no data file", lambda i: dict(data=i.missing), FileNotFoundError, "nowhere.npz", False),
    ("hotspots", "an unknown gene and a bad device", dict(genes="g1,nope", device="cpu"), RuntimeError, "spadot_amd takes the local autocorrelation on the MI355X only (device 'cuda:N'); there is no CPU path", False),
    ("hotspots", "an unknown gene", dict(genes="g1,nope"), ValueError, "--genes names 1 genes that the data does not hold: nope", False),
    ("hotspots", "a row twice", lambda i: dict(genes="g1", domains=i.twice_csv()), ValueError, "is labelled more than once in the domains table", False),
    ("modules", "an unknown gene and a bad device", dict(genes="g1,nope", device="cpu"), RuntimeError, "spadot_amd takes the gene modules on the MI355X only (device 'cuda:N'); there is no CPU path", False),
    ("modules", "an unknown gene", dict(genes="g1,nope"), ValueError, "--genes names 1 genes that the data does not hold: nope", False),
    ("interactions", "a bad device and no domains", dict(device="cpu", domains=None), RuntimeError, "spadot_amd takes the ligand-receptor test on the MI355X only (device 'cuda:N'); there is no CPU path", False),
    ("interactions", "no domains", dict(domains=None), ValueError, "the ligrec stage needs the domains table of analyze (--domains)", False),
    ("interactions", "no interactions", dict(interactions=None), ValueError, "the ligrec stage needs a csv of ligand-receptor pairs with the header source,target (--interactions)", False),
    ("interactions", "a row twice", lambda i: dict(domains=i.twice_csv()), ValueError, "is labelled more than once in the domains table", False),
    ("interactions", "no pair of the data's genes", lambda i: dict(interactions=i.strangers), ValueError, "no interaction is left: none of the 1 pairs names two genes of the data", False),
]


def _ids(cases):
    return [f"{c[0]}: {c[1]}" for c in cases]


def _refused(tmp_path, name, change, exc, fragment, made):
    inp = Inputs(tmp_path)
    kw = dict(_base(name, inp), output_dir=inp.out, device="cuda:0")
    kw.update(change(inp) if callable(change) else change)
    with pytest.raises(exc) as e:
        _driver(name)(argparse.Namespace(**kw))
    assert type(e.value) is exc and fragment in str(e.value), str(e.value)
    assert os.path.isdir(inp.out) == made
    if made:
        assert not [f for f in os.listdir(inp.out) if f.endswith((".csv", ".npz"))]           # refused before anything is written


@pytest.mark.parametrize("name,case,change,exc,fragment,made", CASES, ids=_ids(CASES))
def test_a_driver_refuses_before_it_asks_for_the_device(tmp_path, monkeypatch, name, case, change, exc, fragment, made):
    import torch

    def no_device(*a, **k):
        raise AssertionError(DEVICE)
    monkeypatch.setattr(torch, "device", no_device)
    _refused(tmp_path, name, change, exc, fragment, made)


@pytest.mark.parametrize("name,case,change,exc,fragment,made", CASES_WITH_DEVICE, ids=_ids(CASES_WITH_DEVICE))
def test_a_driver_refuses_with_a_device_named(tmp_path, name, case, change, exc, fragment, made):
    _refused(tmp_path, name, change, exc, fragment, made)


def test_every_driver_has_its_cases():
    drivers = ["markers", "score", "trends", "neighbors", "cooccur", "ripley_stage", "autocorr", "hotspots", "modules",
               "interactions", "analyze"]
    for d in drivers:
        mine = [c for c in CASES + CASES_WITH_DEVICE if c[0] == d]
        assert len(mine) >= 3 and {c[5] for c in mine} <= {True, False}, d
        assert any(c[4] == DEVICE for c in mine), d                                             # how far a well-formed input gets
    assert {c[0] for c in CASES + CASES_WITH_DEVICE} == set(drivers)


# ------------------------------------------------------------------------------------------------------------- the helpers
def _old_read_domains(domains, timepoint):
    """markers.read_domains as it stood, up to the labels it handed to check_labels."""
    df = domains
    tp = np.asarray(timepoint)
    n = tp.shape[0]
    row = np.asarray(df["row"])
    if row.dtype.kind not in "iu":
        raise ValueError("the `row` column of the domains table must hold integer row numbers of the data")
    if row.size and (row.min() < 0 or row.max() >= n):
        raise ValueError(f"the domains table names row {int(row.max() if row.max() >= n else row.min())}: the data has rows "
                         f"0 .. {n - 1}")
    seen = np.bincount(row, minlength=n)
    if np.any(seen > 1):
        raise ValueError(f"row {int(np.flatnonzero(seen > 1)[0])} is labelled more than once in the domains table "
                         f"({int((seen > 1).sum())} duplicate rows)")
    if np.any(seen == 0):
        raise ValueError(f"row {int(np.flatnonzero(seen == 0)[0])} of the data has no label in the domains table "
                         f"({int((seen == 0).sum())} missing rows)")
    bad = np.flatnonzero(np.asarray(df["timepoint"]).astype(str) != tp[row].astype(str))
    if bad.size:
        r = int(row[bad[0]])
        raise ValueError(f"time point mismatch at row {r}: the domains table says {df['timepoint'].iloc[int(bad[0])]!r}, the "
                         f"data says {tp[r]!r} ({bad.size} rows differ)")
    labels = np.empty(n, dtype=np.int64)
    labels[row] = np.asarray(df["kmeans"])
    return labels


def _old_read_lineage(path, timepoint):
    """trends.read_lineage as it stood."""
    z = np.load(path, allow_pickle=False)
    for key in ("X", "rows", "timepoint", "names"):
        if key not in z.files:
            raise ValueError(f"{path} has no `{key}` array (expected a trajectories.npz or fates.npz of analyze --lineage)")
    tp = np.asarray(timepoint)
    n = tp.shape[0]
    X, row, ztp = np.asarray(z["X"]), np.asarray(z["rows"]), np.asarray(z["timepoint"])
    if row.dtype.kind not in "iu":
        raise ValueError(f"the `rows` of {path} must hold integer row numbers of the data")
    if X.ndim != 2 or X.shape[0] != row.shape[0] or ztp.shape[0] != row.shape[0] or len(z["names"]) != X.shape[1]:
        raise ValueError(f"{path}: X of shape {X.shape} against {row.shape[0]} rows, {ztp.shape[0]} time point entries and "
                         f"{len(z['names'])} names")
    row = row.astype(np.int64)
    if row.size and (row.min() < 0 or row.max() >= n):
        raise ValueError(f"{path} names row {int(row.max() if row.max() >= n else row.min())}: the data has rows 0 .. {n - 1}")
    seen = np.bincount(row, minlength=n)
    if np.any(seen > 1):
        raise ValueError(f"row {int(np.flatnonzero(seen > 1)[0])} appears more than once in {path} "
                         f"({int((seen > 1).sum())} duplicate rows)")
    if np.any(seen == 0):
        raise ValueError(f"row {int(np.flatnonzero(seen == 0)[0])} of the data is missing from {path} "
                         f"({int((seen == 0).sum())} missing rows)")
    bad = np.flatnonzero(ztp.astype(str) != tp[row].astype(str))
    if bad.size:
        r = int(row[bad[0]])
        raise ValueError(f"time point mismatch at row {r}: {path} says {str(ztp[bad[0]])!r}, the data says {str(tp[r])!r} "
                         f"({bad.size} rows differ)")
    out = np.empty((n, X.shape[1]), dtype=np.float64)
    out[row] = X
    return out, np.asarray(z["names"]).astype(str)


def _outcome(fn, *args):
    try:
        return ("returned", fn(*args))
    except Exception as e:                                                # noqa: BLE001  (the type is part of what is compared)
        return (type(e), str(e))


def _alignment_faults(n):
    """(what, rows, a function of the rows' time points): every way a table can miss the data's rows, and a clean one."""
    order = np.random.default_rng(11).permutation(n)
    return [("shuffled", order, None), ("in order", np.arange(n), None),
            ("a row twice", np.r_[order, order[:1]], None), ("two rows twice", np.r_[order, order[:2], order[:1]], None),
            ("a row missing", order[order != 4], None), ("a row too large", np.r_[order[1:], n], None),
            ("a negative row", np.r_[order[1:], -2], None), ("rows that are no integers", order.astype(np.float64), None),
            ("rows as strings", order.astype(str), None), ("unsigned rows", order.astype(np.uint16), None),
            ("a time point mismatch", order, lambda t: np.where(np.arange(n) == 3, "E99", t)),
            ("two mismatches", order, lambda t: np.where(np.arange(n) < 2, "E99", t)),
            ("no rows", order[:0], None)]


@pytest.mark.parametrize("numbers", [False, True], ids=["time points as strings", "time points as numbers"])
def test_the_row_alignment_is_that_of_the_two_readers_it_replaced(tmp_path, numbers):
    import pandas as pd
    from spadot_amd.markers import read_domains
    from spadot_amd.trends import read_lineage
    tp = np.repeat(np.asarray([10, 12]) if numbers else np.asarray(TPS), SIZES)
    rng = np.random.default_rng(3)
    for what, rows, alter in _alignment_faults(N):
        inside = np.clip(np.asarray(rows if rows.dtype.kind in "iu" else np.arange(rows.shape[0]) % N, dtype=np.int64), 0, N - 1)
        said = tp[inside] if alter is None else alter(tp[inside].astype(str))
        df = pd.DataFrame({"row": rows, "timepoint": said, "kmeans": np.arange(rows.shape[0]) % 3})
        old, new = _outcome(_old_read_domains, df, tp), _outcome(read_domains, df, tp)
        assert old[0] == new[0], (what, old, new)
        if old[0] == "returned":
            assert what in ("shuffled", "in order", "unsigned rows"), what
            assert new[1].dtype == np.int32 and new[1].tolist() == old[1].tolist(), what
        else:
            assert old[0] is ValueError and old[1] == new[1], (what, old, new)
        path = str(tmp_path / f"{what.replace(' ', '_')}_{int(numbers)}.npz")
        np.savez(path, X=rng.random((rows.shape[0], 2)), rows=rows, timepoint=said, names=np.asarray(["a", "b"]))
        old, new = _outcome(_old_read_lineage, path, tp), _outcome(read_lineage, path, tp)
        assert old[0] == new[0], (what, old, new)
        if old[0] == "returned":
            np.testing.assert_array_equal(old[1][0], new[1][0])
            assert new[1][0].dtype == np.float64 and old[1][1].tolist() == new[1][1].tolist() == ["a", "b"]
        else:
            assert old[0] is ValueError and old[1] == new[1] and path in new[1], (what, old, new)
    # a table of another length than its rows is the lineage reader's own refusal, and comes after the integer rows
    path = str(tmp_path / "short.npz")
    np.savez(path, X=rng.random((N, 2)), rows=np.arange(N), timepoint=tp[:-1], names=np.asarray(["a", "b"]))
    assert _outcome(_old_read_lineage, path, tp) == _outcome(read_lineage, path, tp)
    np.savez(path, X=rng.random((N, 2)), rows=np.arange(N).astype(np.float32), timepoint=tp[:-1], names=np.asarray(["a", "b"]))
    assert _outcome(_old_read_lineage, path, tp) == _outcome(read_lineage, path, tp)
    assert "must hold integer row numbers" in _outcome(read_lineage, path, tp)[1]


def test_the_moved_names_are_handed_on():
    from spadot_amd import markers, moran
    from spadot_amd.utils import _stage_utils as su
    assert markers.load_marker_counts is su.load_marker_counts and markers.read_domains is su.read_domains
    assert moran.Stage is su.Stage and moran.open_stage is su.open_stage and moran.timings is su.timings


class _Result:
    def __init__(self, seed):
        self.first, self.second, self.unused = np.arange(3) + seed, np.float64(seed) / 2, "never written"


def test_the_writer_of_a_time_point_each(tmp_path):
    import pandas as pd
    from spadot_amd.utils._stage_utils import write_timepoints
    res = [_Result(1), _Result(2)]
    seen = []

    def table(t, r):
        seen.append(t)
        return pd.DataFrame({"b": r.first, "a": r.first * 2}, columns=["b", "a"])

    def path(name):
        return str(tmp_path / ("p_" + name))
    head = {"timepoints": np.asarray(TPS)}
    tables, arrays = write_timepoints(path, "thing", TPS, res, table, ("first", "second"), arrays=head,
                                      more=lambda t, r: {"extra": np.int64(t)})
    assert seen == [0, 1] and list(tables) == list(TPS) and arrays is head
    assert list(arrays) == ["timepoints", "E10_first", "E10_second", "E10_extra", "E12_first", "E12_second", "E12_extra"]
    assert arrays["E12_first"].tolist() == [2, 3, 4] and arrays["E10_second"] == 0.5 and arrays["E12_extra"] == 1
    assert sorted(os.listdir(tmp_path)) == ["p_thing_E10.csv", "p_thing_E12.csv"]
    for tp in TPS:
        back = pd.read_csv(path(f"thing_{tp}.csv"))
        assert list(back.columns) == ["b", "a"] and back.equals(tables[tp])
        assert open(path(f"thing_{tp}.csv")).read() == tables[tp].to_csv(index=False)
    tables, arrays = write_timepoints(path, "bare", TPS, res, table, ("second",))
    assert list(arrays) == ["E10_second", "E12_second"] and list(tables) == list(TPS)


def test_timings_with_and_without_a_graph_mark():
    from spadot_amd.moran import timings
    with_graph = timings(1.0, 1.5, 4.0, 4.25, t_graph=2.5)
    assert list(with_graph) == ["read_s", "graph_s", "device_s", "write_s", "total_s"]
    assert with_graph == dict(read_s=0.5, graph_s=1.0, device_s=1.5, write_s=0.25, total_s=3.25)
    without = timings(1.0, 1.5, 4.0, 4.25)
    assert list(without) == ["read_s", "device_s", "write_s", "total_s"]
    assert without == dict(read_s=0.5, device_s=2.5, write_s=0.25, total_s=3.25)


def test_the_settings_helpers(tmp_path, monkeypatch):
    import torch
    from spadot_amd.utils._stage_utils import cuda_device, open_output, top_setting
    ns = argparse.Namespace
    assert top_setting(ns(), 100) == 100 and top_setting(ns(top=None), 50) == 50 and top_setting(ns(top="7"), 50) == 7
    assert top_setting(ns(top=-3), 100) == -3 and top_setting(ns(top=0), 100, least=0) == 0
    with pytest.raises(ValueError, match=r"top must be 0 \(all genes\) or a positive count, not -3"):
        top_setting(ns(top=-3), 100, least=0)
    args = ns(output_dir=None, prefix=None)
    path = open_output(args, str(tmp_path / "deep" / "table.csv"))
    assert args.output_dir == str(tmp_path / "deep") and os.path.isdir(args.output_dir)
    assert path("x.npz") == str(tmp_path / "deep" / "x.npz")
    args = ns(output_dir=str(tmp_path / "given"), prefix="s_")
    assert open_output(args, None)("x.npz") == str(tmp_path / "given" / "s_x.npz") and os.path.isdir(tmp_path / "given")
    monkeypatch.chdir(tmp_path)
    args = ns()
    assert open_output(args, None)("y") == str(tmp_path / "y") and args.output_dir == str(tmp_path)
    assert cuda_device(ns(), "does things").type == "cuda" and cuda_device(ns(device="cuda:3"), "does things").index == 3
    with pytest.raises(RuntimeError, match=r"spadot_amd does things on the MI355X only \(device 'cuda:N'\); there is no CPU path"):
        cuda_device(ns(device="cpu"), "does things")
    monkeypatch.setattr(torch, "device", lambda *a: (_ for _ in ()).throw(AssertionError(DEVICE)))   # asked for at call time
    with pytest.raises(AssertionError, match=DEVICE):
        cuda_device(ns(), "does things")
