"""CPU: the numpy restatement of the ripley stage (tests/ripley_ref.py) and the host code of spadot_amd.ripley against their own
conditions: the generator, the window, the agreement with the co-occurrence restatement, the host statistics, the refusals that
need no device, the command line, and the planted verdicts that the GPU test asserts again on the device."""
import argparse
from fractions import Fraction

import numpy as np
import pytest

import cooccur_cases
import cooccur_ref
import nhood_cases
import ripley_cases as cases
import ripley_ref as ref
import spadot_amd.ripley  # noqa: F401  (the stage under test)


def _inside(v, pts):
    """Every point on or left of every edge of the counter-clockwise polygon v, in exact rational arithmetic."""
    V = [(Fraction(x), Fraction(y)) for x, y in v.tolist()]
    for x, y in pts.tolist():
        px, py = Fraction(x), Fraction(y)
        for (ax, ay), (bx, by) in zip(V, V[1:] + V[:1]):
            if (bx - ax) * (py - ay) - (by - ay) * (px - ax) < 0:
                return False
    return True


@pytest.mark.parametrize("name", sorted(cases.windows()))
def test_generated_points_lie_inside_the_window(name):
    v = cases.windows()[name]
    cum, area = ref.fan(v)
    assert area > 0 and cum[-1] == pytest.approx(area, rel=1e-12)
    for stream in (0, 5):
        pts = ref.points(v, cum, cases.SEED, 3, stream, 400)
        assert pts.shape == (400, 2) and _inside(v, pts)
    a, b = ref.points(v, cum, cases.SEED, 3, 0, 300), ref.points(v, cum, cases.SEED, 3, 0, 400)
    np.testing.assert_array_equal(a, b[:300])                                  # a pure function of the index
    assert not np.array_equal(b, ref.points(v, cum, cases.SEED, 3, 1, 400))    # of the stream,
    assert not np.array_equal(b, ref.points(v, cum, cases.SEED, 4, 0, 400))    # of the problem
    assert not np.array_equal(b, ref.points(v, cum, cases.SEED + 1, 3, 0, 400))  # and of the seed


# the 0.999 quantiles of chi-square with 34 and 10 degrees of freedom (the fan triangles of the windows below, less one)
CHI2_999 = {"gon37": 65.247, "jittered": 29.588}


@pytest.mark.parametrize("name", sorted(CHI2_999))
def test_generated_points_fill_the_fan_triangles_in_proportion_to_area(name):
    v = cases.windows()[name]
    cum, _ = ref.fan(v)
    T, n = cum.shape[0], 40000
    pts = ref.points(v, cum, 11, 0, 2, n)
    d = v[1:] - v[0]
    q = pts - v[0]
    left = d[None, :, 0] * q[:, None, 1] - d[None, :, 1] * q[:, None, 0] >= 0      # left of the ray V0 -> V_{k+1}
    k = np.clip(left.sum(axis=1) - 1, 0, T - 1)                                   # the sector of the fan, from the geometry
    got = np.bincount(k, minlength=T)
    want = n * np.diff(cum, prepend=0.0) / cum[-1]
    chi2 = float(np.sum((got - want) ** 2 / want))
    print(f"{name}: {T} triangles, smallest expectation {want.min():.1f}, chi-square {chi2:.2f}, 0.999 quantile {CHI2_999[name]}")
    assert T - 1 == {"gon37": 34, "jittered": 10}[name] and want.min() > 5
    assert chi2 < CHI2_999[name]


@pytest.mark.parametrize("name,prob", [("tile257_labels", lambda: cases.tile_case(257)), ("lattice_csr", lambda: cases.lattice("csr")),
                                       ("edge2", lambda: cases.edge_call()[2])])
def test_the_observed_pair_counts_are_the_diagonal_of_the_cooccurrence_restatement(name, prob):
    p = prob()
    N = cooccur_ref.counts(p["xy"], p["lab"], p["r2"], p["K"])
    np.testing.assert_array_equal(cases.want(name)[:, 0, 0, :], N[np.arange(p["K"]), np.arange(p["K"]), :])


def test_a_contracted_distance_would_lose_nearest_neighbours_on_their_threshold():
    p, pairs = cases.on_threshold()
    lost = cooccur_cases.fused_misses(p["xy"], p["r2"], pairs)
    print("on-threshold nearest-neighbour pairs that a fused distance would lose:", lost, "of", len(pairs))
    assert lost >= 1
    G = cases.want("on_threshold")[:, 0, 1, :].sum(axis=0)
    assert np.all(np.diff(G) >= 1) and G[0] >= 1                               # every threshold gains the spot that lies on it


def test_edge_problems_of_the_restatement():
    w = [cases.want(f"edge{i}") for i in range(4)]
    assert not w[0][:, :, :2].any()                                            # n = 1: no pair, G never counts
    np.testing.assert_array_equal(w[1][0, 0, 0], np.full(16, 2))               # two coincident spots: a pair at threshold 0
    np.testing.assert_array_equal(w[1][0, 0, 1], np.full(16, 2))
    assert not w[2][1].any() and w[2][0].any() and w[2][2].any()               # the label value without spots
    assert [x.shape for x in w] == [(1, 2, 3, 1), (1, 20, 3, 16), (3, 20, 3, 17), (32, 2, 3, 64)]


def test_convex_window_equals_the_restatement():
    from spadot_amd.ripley import convex_window
    rng = np.random.default_rng(8)
    lattice = np.stack(np.meshgrid(np.arange(9.0), np.arange(7.0)), -1).reshape(-1, 2)
    grid = nhood_cases.planted(45)[0]
    sets = {"collinear": np.stack([np.arange(6.0), 2 * np.arange(6.0) + 1], axis=1),
            "one": np.array([[3.5, -2.0]]), "two": np.array([[0.0, 0.0], [1.0, 2.0]]),
            "duplicated": np.repeat(rng.uniform(0, 5, (9, 2)), 3, axis=0),
            "three": np.array([[0.0, 0.0], [0.0, 3.0], [4.0, 0.0]]),
            "lattice": lattice[rng.permutation(63)], "jittered": grid, "random": rng.normal(size=(500, 2))}
    for name, xy in sets.items():
        v, cum, area = convex_window(xy)
        want = ref.hull(xy)
        np.testing.assert_array_equal(v, want, err_msg=name)
        np.testing.assert_array_equal(cum, ref.fan(want)[0], err_msg=name)
        assert area == ref.fan(want)[1] and v.shape[0] >= 3, name
        bv, bc, ba = convex_window(xy, "box")
        np.testing.assert_array_equal(bv, ref.box(xy), err_msg=name)
        assert ba == ref.fan(ref.box(xy))[1]
    assert convex_window(sets["collinear"])[2] == 0 and convex_window(sets["one"])[2] == 0
    np.testing.assert_array_equal(convex_window(sets["lattice"])[0], [[0, 0], [8, 0], [8, 6], [0, 6]])
    np.testing.assert_array_equal(convex_window(sets["three"])[0], [[0, 0], [4, 0], [0, 3]])
    for name, poly in cases.windows().items():                                 # a caller's polygon comes back as it is
        v, cum, area = convex_window(None, poly)
        np.testing.assert_array_equal(v, poly)
        np.testing.assert_array_equal(cum, ref.fan(poly)[0])


@pytest.mark.parametrize("name,prob", [("edge0", lambda: cases.edge_call()[0]), ("edge1", lambda: cases.edge_call()[1]),
                                       ("edge2", lambda: cases.edge_call()[2]), ("lattice_labels", lambda: cases.lattice()),
                                       ("planted_csr", lambda: cases.planted("csr"))])
def test_ripley_stats_equals_the_restatement(name, prob):
    from spadot_amd.ripley import convex_window, ripley_stats
    p = prob()
    N = cases.want(name)
    want = cases.stats_of(p, N)
    got = ripley_stats(N, np.bincount(p["lab"], minlength=p["K"]), convex_window(p["xy"])[2], p["M"])
    assert set(got) == set(want)
    for key, w in want.items():
        if key == "pattern":
            assert got[key].tolist() == w.tolist()
            continue
        assert got[key].shape == w.shape, key
        np.testing.assert_array_equal(np.isnan(got[key]), np.isnan(w), err_msg=key)
        np.testing.assert_allclose(got[key], w, rtol=1e-12, atol=0, equal_nan=True, err_msg=key)
    if name == "edge2":                                                        # the empty label value: NaN throughout
        assert np.all(np.isnan(got["observed"][:, 1])) and np.all(np.isnan(got["p_global"][:, 1])) and got["pattern"][1] == "random"
    if name == "edge0":                                                        # one spot: L and G undefined, F defined
        assert np.all(np.isnan(got["value"][:2])) and not np.any(np.isnan(got["value"][2]))


def test_refusals_that_need_no_device():
    import torch
    from spadot_amd import ripley as rp
    from spadot_amd import stage_ops as ops
    square = cases.windows()["square"]
    with pytest.raises(ValueError, match="'hull', 'box' or a convex polygon"):
        rp.convex_window(square, "disc")
    with pytest.raises(ValueError, match="counter-clockwise"):
        rp.convex_window(None, square[::-1])                                   # clockwise
    with pytest.raises(ValueError, match="counter-clockwise"):
        rp.convex_window(None, np.array([[0.0, 0], [4, 0], [1, 1], [0, 4]]))   # a reflex vertex
    with pytest.raises(ValueError, match="counter-clockwise"):
        rp.convex_window(None, np.array([[0.0, 0], [2, 0], [4, 0], [0, 4]]))   # three vertices on a line
    star = np.stack([np.cos(4 * np.pi * np.arange(5) / 5), np.sin(4 * np.pi * np.arange(5) / 5)], axis=1)
    with pytest.raises(ValueError, match="goes round more than once"):
        rp.convex_window(None, star)                                           # left turns all the way, twice round
    ang = 2 * np.pi * np.arange(300) / 300
    ring = np.stack([np.cos(ang), np.sin(ang)], axis=1)
    for call in (lambda: rp.convex_window(ring), lambda: rp.convex_window(None, ring)):
        with pytest.raises(ValueError, match='at most 256.*window="box"'):
            call()
    assert rp.convex_window(ring, "box")[0].shape == (4, 2)
    with pytest.raises(ValueError, match="not finite|must be finite"):
        rp.convex_window(np.array([[0.0, 0], [1, np.nan], [0, 1]]))
    with pytest.raises(ValueError, match=r"\[K, 1 \+ S, 3, B\]"):
        rp.ripley_stats(np.zeros((3, 1, 3, 5), np.int64), [1, 1, 1], 1.0, 10)
    with pytest.raises(ValueError, match="sizes holds"):
        rp.ripley_stats(np.zeros((3, 2, 3, 5), np.int64), [1, 1], 1.0, 10)
    with pytest.raises(ValueError, match="taken from L, G and F"):
        rp._mode_mask("L,K")
    xy, lab, r2 = torch.zeros((5, 2), dtype=torch.float64), np.zeros(5, np.int64), [1.0, 2.0]
    with pytest.raises(ValueError, match="exactly one of radii and radii_sq"):
        rp.ripley_counts([xy], [lab])
    for kw, what in ((dict(n_sim=0), "1 to 9999"), (dict(n_sim=10000), "1 to 9999"), (dict(n_probes=0), "1 to 1048576"),
                     (dict(n_probes=1048577), "1 to 1048576"), (dict(null="poisson"), "'labels' or 'csr'"),
                     (dict(modes=("L", "X")), "taken from L, G and F"), (dict(n_sim=[3, 4]), "2 values for 1 problems")):
        with pytest.raises(ValueError, match=what):
            rp.ripley_counts([xy], [lab], radii_sq=[r2], **kw)
    with pytest.raises(ValueError, match="1 to 64"):
        rp.ripley_counts([xy], [lab], radii_sq=[np.arange(65.0)])
    with pytest.raises(ValueError, match="finite, >= 0 and strictly increasing"):
        rp.ripley_counts([xy], [lab], radii=[[2.0, 1.0]])
    with pytest.raises(RuntimeError, match="MI355X only.*no CPU path"):
        rp.ripley_counts([xy], [lab], radii_sq=[r2])
    with pytest.raises(RuntimeError, match="MI355X only.*no CPU path"):
        rp.ripley([xy], [lab])
    with pytest.raises(RuntimeError, match="MI355X only"):
        ops.ripley_counts(xy, np.zeros((1, 48), np.int64), [r2], [(square, ref.fan(square)[0])], 1, 1, 2)
    with pytest.raises(RuntimeError, match="MI355X only"):
        ops.ripley_points(square, ref.fan(square)[0], 0, 0, 0, 10, device="cpu")
    with pytest.raises(RuntimeError, match="MI355X only.*no CPU path"):
        rp.ripley_stage(argparse.Namespace(domains=nhood_cases.stage_table(), output_dir=None, device="cpu"))
    with pytest.raises(ValueError, match="needs the domains table"):
        rp.ripley_stage(argparse.Namespace(domains=None))
    with pytest.raises(ValueError, match="no `pixel_x` column"):
        rp.ripley_stage(argparse.Namespace(domains=nhood_cases.stage_table().drop(columns="pixel_x")))


def test_the_command_line_takes_the_documented_flags():
    from spadot_amd import cli
    a = cli.build_parser().parse_args(["ripley", "--domains", "d.csv"])
    assert (a.cmd_choice, a.domains, a.output_dir, a.prefix, a.bins, a.radius, a.n_sim, a.n_probes, a.null, a.mode, a.window,
            a.alpha, a.seed, a.device) == ("ripley", "d.csv", None, "", 50, None, 99, 1000, "labels", "L,G,F", "hull", 0.05, 0,
                                           "cuda:0")
    a = cli.build_parser().parse_args(["ripley", "--domains", "d.csv", "-o", "out", "--prefix", "p_", "--bins", "20", "--radius",
                                       "3.5", "--n_sim", "19", "--n_probes", "64", "--null", "csr", "--mode", "L,F", "--window",
                                       "box", "--alpha", "0.01", "--seed", "9", "--device", "cuda:1"])
    assert (a.output_dir, a.prefix, a.bins, a.radius, a.n_sim, a.n_probes, a.null, a.mode, a.window, a.alpha, a.seed,
            a.device) == ("out", "p_", 20, 3.5, 19, 64, "csr", "L,F", "box", 0.01, 9, "cuda:1")
    for bad in (["--null", "poisson"], ["--window", "disc"]):
        with pytest.raises(SystemExit):
            cli.build_parser().parse_args(["ripley", "--domains", "d.csv"] + bad)
    assert "python -m spadot_amd ripley --domains CSV" in cli.__doc__ and "DESIGN 7n" in cli.__doc__


@pytest.mark.parametrize("null", ["labels", "csr"])
def test_planted_domains_read_clustered_in_the_restatement(null):
    """The 45 x 45 planted set: under either null every Voronoi domain is farther from its envelope than every simulation,
    p_global = 1 / (S + 1) for L, which Benjamini-Hochberg over the 7 domains leaves at 0.025 <= 0.05."""
    st = cases.stats_of(cases.planted(null), cases.want("planted_" + null))
    print(null, "p_global of L", st["p_global"][0], "pattern", st["pattern"])
    np.testing.assert_array_equal(st["p_global"][0], np.full(7, 1.0 / (cases.PLANTED_S + 1)))
    assert st["pattern"].tolist() == ["clustered"] * 7


def test_a_domain_relabelled_at_random_reads_random_in_the_restatement():
    """300 spots drawn at random are a draw from the labels null itself: the domain they form reads random (p_global of L 0.6 in
    the restatement), the seven planted domains beside it still read clustered."""
    st = cases.stats_of(cases.planted("labels", True), cases.want("scattered"))
    print("p_global of L", st["p_global"][0], "padj", st["padj"][0], "pattern", st["pattern"])
    assert st["pattern"].tolist() == ["clustered"] * 7 + ["random"]
    assert st["padj"][0, 7] > 0.05


def _lattice_spots(rng, trial):
    """A square or hexagonal lattice of spots, a tenth of them dropped, mapped to pixel coordinates by a scale, a rotation within
    0.1 rad and an offset: how the full-resolution coordinates of a slide look.  Its hull holds vertices that are collinear up to
    rounding."""
    side, hexa = int(rng.integers(20, 61)), trial % 2
    i, j = np.meshgrid(np.arange(side), np.arange(side))
    xy = np.stack([i + 0.5 * (j % 2) * hexa, j * (np.sqrt(3) / 2 if hexa else 1.0)], -1).reshape(-1, 2)
    xy = xy[rng.uniform(size=xy.shape[0]) > 0.1]
    th = rng.uniform(-0.1, 0.1)
    R = np.array([[np.cos(th), -np.sin(th)], [np.sin(th), np.cos(th)]])
    return rng.uniform(50, 500) * xy @ R.T + rng.uniform(0, 20000, 2)


def test_the_hull_of_a_rotated_lattice_passes_the_window_check_and_holds_every_spot():
    """The monotone chain and the window check test two forms of the cross product, which disagree on vertices that are
    collinear up to rounding: without the finishing pass of _hull about 8 % of these sets are refused.  A spot may lie outside
    the finished hull by rounding alone: coordinates of size s carry eps s / 2 each, the differences and products of the
    predicates a few times that, so the bound is 8 eps s."""
    from spadot_amd.ripley import convex_window
    from spadot_amd.stage_ops import ripley_window
    rng = np.random.default_rng(0)
    worst = 0.0
    for trial in range(100):
        xy = _lattice_spots(rng, trial)
        v, cum, area = convex_window(xy)                                       # refuses what the device's check would refuse
        ripley_window(v, cum)
        want = ref.hull(xy)
        np.testing.assert_array_equal(v, want, err_msg=f"set {trial}")
        np.testing.assert_array_equal(cum, ref.fan(want)[0], err_msg=f"set {trial}")
        assert area > 0 and np.all(np.diff(cum) >= 0) and cum[0] >= 0 and abs(cum[-1] - area) <= 1e-12 * area
        e = np.roll(v, -1, axis=0) - v
        assert not np.any(e[:, 0] * np.roll(e, -1, axis=0)[:, 1] < e[:, 1] * np.roll(e, -1, axis=0)[:, 0])
        assert not any(ref._right_turn(want[k - 2], want[k - 1], want[k]) for k in range(len(want)))
        for a, d in zip(v, e):
            out = (d[0] * (xy[:, 1] - a[1]) - d[1] * (xy[:, 0] - a[0])) / np.hypot(d[0], d[1])
            worst = min(worst, float(out.min()) / np.abs(xy).max())
    print("farthest spot outside its hull, in units of the largest coordinate:", worst)
    assert worst >= -8 * np.finfo(np.float64).eps


def test_a_statistic_that_was_not_counted_is_not_reported():
    from spadot_amd.ripley import convex_window, ripley_stats
    p = cases.lattice()
    N = cases.counts_of(p, modes=("G", "F"))
    sizes, area = np.bincount(p["lab"], minlength=p["K"]), convex_window(p["xy"]).area
    got, want = ripley_stats(N, sizes, area, p["M"], modes="G,F"), ref.stats(N, sizes, area, p["M"], modes=("G", "F"))
    full = ripley_stats(cases.want("lattice_labels"), sizes, area, p["M"])
    for key in ("value", "observed", "sim_mean", "sim_min", "sim_max", "p_lo", "p_hi", "p_global", "padj"):
        assert np.all(np.isnan(got[key][0])), key                              # L: no zeros passed off as data
        np.testing.assert_array_equal(got[key][1:], full[key][1:], err_msg=key)
        np.testing.assert_allclose(got[key], want[key], rtol=1e-12, atol=0, equal_nan=True, err_msg=key)
    assert got["pattern"].tolist() == want["pattern"].tolist() == [""] * 3      # no verdict without L
    only = ripley_stats(cases.counts_of(p, modes=("L",)), sizes, area, p["M"], modes=("L",))
    assert np.all(np.isnan(only["value"][1:])) and np.all(np.isnan(only["p_global"][1:]))
    np.testing.assert_array_equal(only["value"][0], full["value"][0])
    assert only["pattern"].tolist() == full["pattern"].tolist()


def test_a_polygon_is_one_window_however_it_is_written():
    from spadot_amd.ripley import Window, _per_window, convex_window
    tri = [(0.0, 0.0), (7.0, 1.0), (2.0, 5.0)]
    win = convex_window(None, tri)
    assert isinstance(win, Window) and win.vertices.shape == (3, 2)
    for poly in (tri, tuple(tri), [list(q) for q in tri], np.array(tri)):       # a list or a tuple of pairs is ONE polygon
        assert all(w is poly for w in _per_window(poly, 2))
    assert _per_window("box", 2) == ["box", "box"] and _per_window(win, 3) == [win] * 3
    assert _per_window(["hull", np.array(tri)], 2)[0] == "hull" and _per_window((win, "box"), 2) == [win, "box"]
    assert [np.shape(w) for w in _per_window([tri, tri], 2)] == [(3, 2), (3, 2)]  # two polygons, one per problem
    with pytest.raises(ValueError, match="window holds 3 values for 2 problems"):
        _per_window(["hull", "box", "hull"], 2)
