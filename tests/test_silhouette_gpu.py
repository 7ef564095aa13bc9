"""The silhouette kernel on the MI355X against the numpy restatement of its definition (tests/silhouette_ref.py, pinned to sklearn
by tests/test_silhouette_cpu.py): the edge call, the 256-point tile's edges, bitwise repeatability (fp32 against fp64 input, alone
against in a batch, run against run), the refusals, the score stage and `analyze --criterion silhouette`.

Tolerances.  Every sum of at most n terms carries at most (n - 1) 2^-53 relative error in any order and a distance a few ulps
more, so |delta s| <= 2 (n + d + 4) 2^-53 < 5e-13 for n <= 2000: samples and score atol 1e-12, a and b rtol 1e-12.  `nearest` is
compared exactly after asserting ON THE REFERENCE that the two smallest cluster means of every spot differ by more than 1e-9
relative (a condition on the input); the degenerate sets are compared exactly as they are."""
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import silhouette_cases as cases
import silhouette_ref as ref

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _dev(x, dtype=torch.float64):
    return torch.as_tensor(x, dtype=dtype, device=DEV)


def _compare(got, want, random=True):
    print(f"max |ds| {np.nanmax(np.abs(got.samples - want['samples'])):.3e}  |dscore| {abs(got.score - want['score']):.3e}  "
          f"min gap {ref.min_gap(want['means']).min():.3e}")
    np.testing.assert_allclose(got.samples, want["samples"], rtol=0, atol=1e-12)
    np.testing.assert_allclose(got.a, want["a"], rtol=1e-12, atol=0)
    np.testing.assert_allclose(got.b, want["b"], rtol=1e-12, atol=0)
    if random:
        assert ref.min_gap(want["means"]).min() > 1e-9             # on the reference: no spot sits on a tie between clusters
    np.testing.assert_array_equal(got.nearest, want["nearest"])
    assert got.nearest.dtype == np.int32 and got.samples.dtype == np.float64
    np.testing.assert_array_equal(got.sizes, want["sizes"])
    assert abs(got.score - want["score"]) <= 1e-12


def _same_bits(r, q):
    return all(np.array_equal(getattr(r, f), getattr(q, f), equal_nan=True) for f in ("a", "b", "nearest", "samples")) \
        and (r.score == q.score or (np.isnan(r.score) and np.isnan(q.score)))


@pytest.fixture(scope="module")
def edge():
    """The edge call, scored once: (sets, labelings, random flags, results, references)."""
    from spadot_amd.silhouette import silhouette_many
    sets, labelings, random = cases.edge_call()
    res = silhouette_many([_dev(x) for x in sets], labelings)
    want = [[ref.silhouette(x, lab) for lab in ls] for x, ls in zip(sets, labelings)]
    return sets, labelings, random, res, want


def test_edge_call_matches_the_restatement(edge):
    sets, labelings, random, res, want = edge
    assert [len(r) for r in res] == [3, 3, 3, 3]
    for t in range(4):
        for l in range(3):
            _compare(res[t][l], want[t][l], random[t])
    assert res[0][1].sizes[2] == 1 and res[0][1].samples[36] == 0.0                 # the singleton
    assert res[0][2].sizes[2] == 0 and not np.any(res[0][2].nearest == 2)           # the label value without points
    for l in range(3):
        assert not res[2][l].a.any() and not res[2][l].b.any() and not res[2][l].samples.any()      # all points equal
        assert np.all(res[3][l].samples == 1.0) and res[3][l].score == 1.0                          # two point masses


@pytest.mark.parametrize("name", [c[0] for c in cases.TILE_CASES])
def test_tile_edges_match_the_restatement(name):
    from spadot_amd.silhouette import silhouette_many, silhouette_samples, silhouette_score
    X, lab = cases.tile_case(name)
    want = ref.silhouette(X, lab)
    got = silhouette_many([_dev(X)], [[lab]])[0][0]
    _compare(got, want)
    if name == "n257":                                                              # the one-problem forms, shaped like sklearn's
        np.testing.assert_array_equal(silhouette_samples(_dev(X), lab), got.samples)
        assert silhouette_score(_dev(X), torch.as_tensor(lab, device=DEV)) == got.score


def test_fp32_input_gives_the_bits_of_fp64_input(edge):
    from spadot_amd.silhouette import silhouette_many
    sets, labelings, _, res, _ = edge
    res32 = silhouette_many([_dev(x, torch.float32) for x in sets], labelings)
    for t in range(4):
        for l in range(3):
            assert _same_bits(res32[t][l], res[t][l]), (t, l)


def test_a_problem_alone_gives_the_bits_it_gives_in_a_batch(edge):
    from spadot_amd.silhouette import silhouette_many
    sets, labelings, _, res, _ = edge
    for t, l in ((1, 2), (0, 1), (3, 0)):
        alone = silhouette_many([_dev(sets[t])], [[labelings[t][l]]])[0][0]
        assert _same_bits(alone, res[t][l]), (t, l)


def test_two_runs_are_bitwise_identical(edge):
    from spadot_amd.silhouette import silhouette_many
    sets, labelings, _, res, _ = edge
    again = silhouette_many([_dev(x) for x in sets], labelings)
    for t in range(4):
        for l in range(3):
            assert _same_bits(again[t][l], res[t][l]), (t, l)


def test_an_undefined_labeling_scores_nan_in_a_batch_and_raises_alone():
    from spadot_amd.silhouette import silhouette_many, silhouette_samples
    X, lab = cases.tile_case("n255")
    one = np.zeros(255, dtype=np.int64)
    r = silhouette_many([_dev(X)], [[one, lab, np.arange(255) % 32]], n_clusters=[[4, 3, 32]])[0]
    assert np.isnan(r[0].score) and not r[0].defined and np.all(r[0].nearest == -1)
    _compare(r[1], ref.silhouette(X, lab))                                          # its neighbours are untouched by it
    assert np.isfinite(r[2].score)
    with pytest.raises(ValueError, match="Number of labels is 1"):
        silhouette_samples(_dev(X), np.ones(255, dtype=np.int64))                   # K = 2 with cluster 0 empty


def test_refusals_come_before_any_launch(monkeypatch):
    from spadot_amd import stage_ops as ops
    from spadot_amd.silhouette import silhouette_many, silhouette_samples
    X = _dev(np.zeros((40, 3)))
    valid = (X, torch.tensor([[0, 0, 40, 2]], dtype=torch.int64, device=DEV), torch.arange(40, dtype=torch.int32, device=DEV),
             torch.tensor([[0, 20] + [40] * 31], dtype=torch.int32, device=DEV))
    out = tuple(torch.full((40,), 7, dtype=dt, device=DEV) for dt in (torch.float64, torch.float64, torch.int32, torch.float64))
    # the library's own refusals (-7 -> ValueError): nothing is launched, the outputs keep their fill
    for args, kw in (((_dev(np.zeros((40, 33))),) + valid[1:], dict(k_min=2, k_max=2)), (valid, dict(k_min=2, k_max=33)),
                     (valid, dict(k_min=1, k_max=2))):
        with pytest.raises(ValueError, match="outside its limits"):
            ops.silhouette_launch(*args, 40, kw["k_min"], kw["k_max"], out=out)
    torch.cuda.synchronize()
    assert all(bool((o == 7).all()) for o in out)

    def no_launch(*a, **k):
        raise AssertionError("launched")
    monkeypatch.setattr(ops, "silhouette_launch", no_launch)
    with pytest.raises(ValueError, match="1 to 32 dimensions"):
        silhouette_many([_dev(np.zeros((40, 33)))], [[np.arange(40) % 2]])
    with pytest.raises(ValueError, match="33 label values"):
        silhouette_samples(X, np.arange(40) % 33)
    with pytest.raises(ValueError, match="1 label values"):
        silhouette_samples(X, np.zeros(40, dtype=np.int64))
    with pytest.raises(ValueError, match="labels must lie in 0 .. 1"):
        silhouette_samples(X, np.where(np.arange(40) == 7, -1, np.arange(40) % 2))
    with pytest.raises(ValueError, match="labels must lie in 0 .. 2"):
        silhouette_many([X], [[np.arange(40) % 4]], n_clusters=[[3]])
    with pytest.raises(ValueError, match="labels must be integers"):
        silhouette_samples(X, np.zeros(40))
    with pytest.raises(ValueError, match="one label per point"):
        silhouette_samples(X, np.arange(39) % 2)
    with pytest.raises(RuntimeError, match="MI355X only"):
        silhouette_samples(X.cpu(), np.arange(40) % 2)
    with pytest.raises(AssertionError, match="launched"):                           # the patch is what a valid call would reach
        silhouette_samples(X, np.arange(40) % 2)


# ---------------------------------------------------------------------------------------------------------------- the stage
class _Args:
    def __init__(self, **kw):
        self.__dict__.update(dict(output_dir=None, prefix="", n_clusters=None, device=DEV, write_tmaps=False), **kw)


def _planted(counts=(500, 600, 700), k0s=(5, 6, 7)):
    """Three time points of planted blobs, d = 20: centres normal * 4, unit noise.  With sklearn's K-means on the host the planted
    k has the largest silhouette score in every time point by a wide margin (0.706 / 0.619, 0.720 / 0.659, 0.728 / 0.649 against
    the runner-up), so the selection is far from a tie."""
    rng = np.random.default_rng(1993)
    X, truth = [], []
    for n, k0 in zip(counts, k0s):
        cen = rng.normal(size=(k0, 20)) * 4
        which = rng.integers(0, k0, n)
        X.append((cen[which] + rng.normal(size=(n, 20))).astype(np.float32))
        truth.append(which)
    return X, truth


def _write_latent(path, X, seed=3):
    rng = np.random.default_rng(seed)
    n = sum(x.shape[0] for x in X)
    tp = np.repeat(np.array(["E1", "E2", "E3"]), [x.shape[0] for x in X])
    rows = rng.permutation(n) + 1000
    np.savez_compressed(path, X=np.concatenate(X), rows=rows, timepoint=tp, spatial=rng.uniform(0, 100, size=(n, 2)))
    return tp, rows


def test_score_stage_end_to_end_and_command_line(tmp_path):
    import pandas as pd
    from spadot_amd.silhouette import score
    X, truth = _planted((300, 257, 120), (3, 4, 2))
    f = tmp_path / "latent.npz"
    tp, rows = _write_latent(f, X)
    lab = np.concatenate(truth)
    shuffle = np.random.default_rng(4).permutation(lab.shape[0])                    # the table need not be in row order
    csv = tmp_path / "domains.csv"
    pd.DataFrame({"row": rows[shuffle], "timepoint": tp[shuffle], "kmeans": lab[shuffle], "pixel_x": 0.0,
                  "pixel_y": 0.0}).to_csv(csv, index=False)
    a = _Args(data=str(f), domains=str(csv), prefix="p_")
    out = score(a)
    assert a.output_dir == str(tmp_path) and out["timepoints"] == ["E1", "E2", "E3"]
    s = pd.read_csv(tmp_path / "p_silhouette.csv", float_precision="round_trip")
    m = pd.read_csv(tmp_path / "p_silhouette_summary.csv", float_precision="round_trip")
    assert list(s.columns) == ["row", "timepoint", "kmeans", "a", "b", "nearest", "silhouette"]
    assert list(m.columns) == ["timepoint", "domain", "n", "silhouette"]
    np.testing.assert_array_equal(s["row"].to_numpy(), rows)                        # input order
    np.testing.assert_array_equal(s["timepoint"].to_numpy().astype(str), tp)
    np.testing.assert_array_equal(s["kmeans"].to_numpy(), lab)
    np.testing.assert_array_equal(out["samples"]["silhouette"].to_numpy(), s["silhouette"].to_numpy())   # repr round trip
    rowsum = []
    for t, x, lt in zip(("E1", "E2", "E3"), X, truth):
        want = ref.silhouette(x, lt)
        got = s[s["timepoint"] == t]
        np.testing.assert_allclose(got["silhouette"].to_numpy(), want["samples"], rtol=0, atol=1e-12)
        np.testing.assert_allclose(got["a"].to_numpy(), want["a"], rtol=1e-12, atol=0)
        np.testing.assert_allclose(got["b"].to_numpy(), want["b"], rtol=1e-12, atol=0)
        np.testing.assert_array_equal(got["nearest"].to_numpy(), want["nearest"])
        assert abs(out["scores"][t] - want["score"]) <= 1e-12
        mt = m[m["timepoint"] == t]
        assert mt["domain"].astype(str).tolist() == [str(k) for k in range(int(lt.max()) + 1)] + ["all"]
        for k in range(int(lt.max()) + 1):                                          # the means follow from the samples
            r = mt[mt["domain"].astype(str) == str(k)].iloc[0]
            assert r["n"] == int((lt == k).sum())
            assert r["silhouette"] == pytest.approx(float(np.mean(got["silhouette"].to_numpy()[lt == k])), rel=1e-15, abs=1e-16)
        r = mt[mt["domain"].astype(str) == "all"].iloc[0]
        assert r["n"] == x.shape[0] and r["silhouette"] == pytest.approx(float(np.mean(got["silhouette"])), rel=1e-15, abs=1e-16)
        rowsum.append(int(r["n"]))
    assert rowsum == [300, 257, 120] and set(out["timings"]) == {"read_s", "device_s", "write_s", "total_s"}
    # the subcommand writes the same two files
    env = dict(os.environ)
    env["PYTHONPATH"] = ROOT + os.pathsep + env.get("PYTHONPATH", "")
    p = subprocess.run([sys.executable, "-m", "spadot_amd", "score", "-i", str(f), "--domains", str(csv), "-o",
                        str(tmp_path / "cli")], cwd=ROOT, env=env, capture_output=True, text=True, timeout=600)
    assert p.returncode == 0, p.stdout[-2000:] + p.stderr[-2000:]
    assert sorted(os.listdir(tmp_path / "cli")) == ["silhouette.csv", "silhouette_summary.csv"]
    for name in ("silhouette.csv", "silhouette_summary.csv"):
        assert (tmp_path / "cli" / name).read_bytes() == (tmp_path / ("p_" + name)).read_bytes()


def test_analyze_picks_the_planted_k_by_silhouette_and_leaves_the_default_alone(tmp_path):
    import pandas as pd
    from spadot_amd import analyze
    from spadot_amd.utils._analyze_utils import have_matplotlib
    X, _ = _planted()
    f = tmp_path / "latent.npz"
    _write_latent(f, X)
    tps = ["E1", "E2", "E3"]
    sil_dir, def_dir = tmp_path / "sil", tmp_path / "elbow"
    out = analyze(_Args(data=str(f), output_dir=str(sil_dir), criterion="silhouette"))
    assert out["n_clusters"] == [5, 6, 7] and out["criterion"] == "silhouette"
    for t, (tp, x) in enumerate(zip(tps, X)):
        tab = pd.read_csv(sil_dir / f"adaptive_{tp}_silhouette.csv", float_precision="round_trip")
        assert list(tab.columns) == ["clusters", "silhouette", "selected"] and tab["clusters"].tolist() == list(range(4, 21))
        assert tab["clusters"][tab["selected"]].tolist() == [5 + t]
        np.testing.assert_array_equal(tab["silhouette"].to_numpy(), np.asarray(out["silhouette"][tp]))
        best = int(np.argmax(out["silhouette"][tp]))
        assert best == 1 + t                                                        # k = 5, 6, 7 at index 1, 2, 3
        want = ref.silhouette(x, out["labels"][tp], K=5 + t)["score"]               # on the labels of res
        assert abs(tab["silhouette"][best] - want) <= 1e-12
        wss = pd.read_csv(sil_dir / f"adaptive_{tp}_WSS.csv")
        assert list(wss.columns) == ["clusters", "wss", "wss_diff", "wss_diff_ratio", "selected"]
        assert wss["clusters"][wss["selected"]].tolist() == [5 + t]                 # marks the k actually chosen
    # the default criterion: the files it wrote before, none of the silhouette ones
    a = _Args(data=str(f), output_dir=str(def_dir))
    res = analyze(a)
    files, sil_files = set(os.listdir(def_dir)), set(os.listdir(sil_dir))
    want = {"adaptive_domains.csv", "OT_g.txt"} | {f"adaptive_transition_table_{d}_{d + 1}.{e}" for d in (0, 1) for e in ("csv", "npz")}
    want |= {f"adaptive_{t}_WSS.csv" for t in tps}
    extra = {f"adaptive_{t}_silhouette.csv" for t in tps}
    if have_matplotlib():
        want |= {f"adaptive_{t}_domains.png" for t in tps} | {f"adaptive_transition_dotplot_{d}_{d + 1}.png" for d in (0, 1)}
        want |= {f"adaptive_{t}_WSS_vs_Clusters.png" for t in tps}
        extra |= {f"adaptive_{t}_silhouette_vs_Clusters.png" for t in tps}
    assert want <= files and not any("silhouette" in name for name in files)
    assert sil_files - files == extra and files <= sil_files
    assert "silhouette" not in res and "criterion" not in res and not hasattr(a, "criterion")
