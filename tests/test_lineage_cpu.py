"""Lineage analyses, host side (no GPU): the three definitions on tiny dense plans worked out by hand as exact fractions, for
the test-side reference (tests/lineage_ref.py) and for spadot_amd.lineage.TransportChain driven by dense stand-in solvers;
properties of the reference on random plans; the command line flag; the input checks of analyze(lineage=True) that run
before any device work."""
from fractions import Fraction as Fr

import numpy as np
import pytest

import lineage_ref as ref
from lineage_ref import EPS

# Three time points of 2, 3 and 2 spots.  All entries small integers, so every expected value is a short fraction.
PI0 = np.array([[1, 1, 0], [0, 2, 2]], dtype=np.float64)
PI1 = np.array([[1, 0], [1, 1], [0, 4]], dtype=np.float64)
PI1_ZERO_ROW = np.array([[1, 0], [0, 0], [0, 4]], dtype=np.float64)        # spot 1 of the middle time point sends nothing
L0, L1, L2 = np.array([0, 1]), np.array([0, 0, 1]), np.array([0, 1])


def F(rows):
    return np.array([[float(Fr(x)) for x in r] for r in rows], dtype=np.float64)


def close(got, want):
    """Equal to a few roundings; a zero is exactly zero."""
    np.testing.assert_allclose(np.asarray(got, dtype=np.float64), want, rtol=8 * EPS, atol=0)


# ---- what the definitions give on PI0, PI1 (worked by hand) ----
TRAJ_FROM_0 = [F([[1, 0], [0, 1]]),
               F([["1/2", 0], ["1/2", "1/2"], [0, "1/2"]]),            # PI0^T columns (1,1,0) / 2 and (0,2,2) / 4
               F([["2/3", "1/6"], ["1/3", "5/6"]])]                    # PI1^T of those: (1, 1/2) / (3/2) and (1/2, 5/2) / 3
TRAJ_FROM_1 = [F([["1/2", 0], ["1/2", 1]]),                            # PI0 (1/2,1/2,0) = (1,1) / 2 ; PI0 (0,0,1) = (0,2) / 2
               F([["1/2", 0], ["1/2", 0], [0, 1]]),
               F([["2/3", 0], ["1/3", 1]])]                            # PI1^T (1/2,1/2,0) = (1,1/2) / (3/2) ; PI1^T (0,0,1) = (0,4) / 4
TRAJ_FROM_2 = [F([["1/2", "1/11"], ["1/2", "10/11"]]),                 # PI0 of the row below: (1,1) / 2 and (1/5, 2) / (11/5)
               F([["1/2", 0], ["1/2", "1/5"], [0, "4/5"]]),            # PI1 columns (1,1,0) / 2 and (0,1,4) / 5
               F([[1, 0], [0, 1]])]
FATES_0_TO_2 = F([["2/3", "1/3"], ["1/6", "5/6"]])                     # PI0 PI1 = [[2,1],[2,10]], rows / 3 and / 12
FATES_1_TO_2 = F([[1, 0], ["1/2", "1/2"], [0, 1]])
TABLE_0_2 = F([["3/2", "1/2"], [1, 3]])                                # PI0 diag(1,1/2,1/4) PI1
TABLE_0_2_ONE_DOMAIN = F([["5/2", "7/2"]])
TABLE_0_2_ZERO_ROW = F([[1, 0], [0, 2]])                               # PI0 diag(1,0,1/4) PI1_ZERO_ROW: the mass of spot 1 is lost


def test_reference_on_the_hand_worked_plans():
    plans = [PI0, PI1]
    for t, labels, want in ((0, L0, TRAJ_FROM_0), (1, L1, TRAJ_FROM_1), (2, L2, TRAJ_FROM_2)):
        got = ref.trajectories(plans, labels, t)
        assert len(got) == 3
        for u in range(3):
            close(got[u], want[u])
    close(ref.fates(plans, L2, 2, 0), FATES_0_TO_2)
    close(ref.fates(plans, L2, 2, 1), FATES_1_TO_2)
    close(ref.transition_table(plans, L0, L2, 0, 2), TABLE_0_2)
    close(ref.transition_table(plans, np.array([0, 0]), L2, 0, 2), TABLE_0_2_ONE_DOMAIN)
    close(ref.transition_table(plans, L0, L1, 0, 1), F([[2, 0], [2, 2]]))               # u = t + 1: the block sums
    close(ref.transition_table([PI0, PI1_ZERO_ROW], L0, L2, 0, 2), TABLE_0_2_ZERO_ROW)


def test_reference_zero_mass_stays_zero_without_nan():
    plans = [PI0, PI1_ZERO_ROW]
    own = np.array([0, 1, 2])                                   # every middle spot its own domain; domain 1 sends nothing
    tr = ref.trajectories(plans, own, 1)
    close(tr[2], F([[1, 0, 0], [0, 0, 1]]))                      # the column of domain 1 is zero, the others sum to 1
    close(tr[0], F([[1, "1/3", 0], [0, "2/3", 1]]))              # ancestors do not go through PI1: all three columns live
    f = ref.fates(plans, L2, 2, 1)
    close(f, F([[1, 0], [0, 0], [0, 1]]))                        # the row of the silent spot stays zero
    for a in tr + [f]:
        assert np.isfinite(np.asarray(a, dtype=np.float64)).all()


def _random_chain(rng, sizes, zero=False):
    plans = [rng.uniform(0.0, 1.0, size=(a, b)) * (rng.uniform(size=(a, b)) < 0.7) for a, b in zip(sizes[:-1], sizes[1:])]
    if zero:
        plans[1][3, :] = 0.0
        plans[0][:, 5] = 0.0
    labels = []
    for n in sizes:
        k = int(rng.integers(2, 6))
        lab = np.concatenate([np.arange(k), rng.integers(0, k, n - k)])
        labels.append(rng.permutation(lab))
    return plans, labels


@pytest.mark.parametrize("zero", [False, True])
def test_reference_properties_on_random_plans(zero):
    rng = np.random.default_rng(11 + zero)
    sizes = (17, 23, 19, 21)
    plans, labels = _random_chain(rng, sizes, zero)
    tol = 64 * EPS
    for t in range(4):
        tr = ref.trajectories(plans, labels[t], t)
        for u in range(4):
            a = np.asarray(tr[u], dtype=np.float64)
            assert a.shape == (sizes[u], labels[t].max() + 1) and np.isfinite(a).all() and (a >= 0).all()
            s = a.sum(0)
            assert np.all((np.abs(s - 1) <= tol) | (s == 0))
            if not zero:
                assert np.all(np.abs(s - 1) <= tol)
    for t in range(3):
        f = np.asarray(ref.fates(plans, labels[3], 3, t), dtype=np.float64)
        assert np.isfinite(f).all()
        s = f.sum(1)
        assert np.all((np.abs(s - 1) <= tol) | (s == 0))
        if not zero:
            assert np.all(np.abs(s - 1) <= tol)
    for t in range(3):
        np.testing.assert_allclose(np.asarray(ref.transition_table(plans, labels[t], labels[t + 1], t, t + 1), dtype=np.float64),
                                   np.asarray(ref.block_sums(plans[t], labels[t], labels[t + 1]), dtype=np.float64),
                                   rtol=tol, atol=0)
    for t, u in ((0, 2), (0, 3), (1, 3)):
        tab = np.asarray(ref.transition_table(plans, labels[t], labels[u], t, u), dtype=np.float64)
        assert np.isfinite(tab).all() and (tab >= 0).all()
        if not zero:                                             # no row sum is 0: every unit of mass of Pi_t is handed on
            assert abs(tab.sum() - plans[t].sum()) <= tol * plans[t].sum()
        else:                                                    # what a silent spot received is lost, nothing is invented
            assert tab.sum() <= plans[t].sum() * (1 + tol)
    if zero:
        own = np.arange(sizes[1])
        tr = ref.trajectories(plans, own, 1)
        assert np.all(np.asarray(tr[0], dtype=np.float64)[:, 5] == 0)      # the column of spot 5 in Pi_0 is zero: no ancestors
        assert np.all(np.asarray(tr[2], dtype=np.float64)[:, 3] == 0)      # the row of spot 3 in Pi_1 is zero: no descendants


# ---- spadot_amd.lineage on the host: the chain logic with dense stand-ins for the device solvers ----
class _DenseSolver:
    def __init__(self, plan):
        import torch
        self.plan_t = torch.as_tensor(plan, dtype=torch.float64)
        self.closed = False

    def apply(self, P, transpose=False):
        import torch
        P = torch.as_tensor(P, dtype=torch.float64)
        return (self.plan_t.T if transpose else self.plan_t) @ P

    def transition_table(self, row_labels, col_labels, n_row_groups=None, n_col_groups=None):
        import torch
        a = torch.as_tensor(np.asarray(ref.onehot(row_labels, n_row_groups), dtype=np.float64))
        b = torch.as_tensor(np.asarray(ref.onehot(col_labels, n_col_groups), dtype=np.float64))
        return a.T @ self.plan_t @ b

    def close(self):
        self.closed = True


def _dense_chain(monkeypatch, plans, fail_at=None):
    from spadot_amd import analyze_ot, lineage
    made = []

    def fake_spot_transport(latent_a, latent_b, config=None, growth=None, which="last", storage="f32", device="cuda:0"):
        if fail_at is not None and len(made) == fail_at:
            raise RuntimeError("solve failed")
        made.append(_DenseSolver(plans[len(made)]))
        return made[-1], []
    monkeypatch.setattr(analyze_ot, "spot_transport", fake_spot_transport)
    sizes = [p.shape[0] for p in plans] + [plans[-1].shape[1]]
    return lineage, [np.zeros((n, 2)) for n in sizes], made


def test_transport_chain_gives_the_hand_worked_values(monkeypatch):
    lineage, latents, made = _dense_chain(monkeypatch, [PI0, PI1])
    with lineage.TransportChain(latents, device="cpu") as chain:
        assert len(chain) == 3 and len(chain.solvers) == 2
        for t, labels, want in ((0, L0, TRAJ_FROM_0), (1, L1, TRAJ_FROM_1), (2, L2, TRAJ_FROM_2)):
            got = chain.trajectories(labels, t)
            for u in range(3):
                assert got[u].dtype == np.float64
                close(got[u], want[u])
        close(chain.fates(L2, 2, 0), FATES_0_TO_2)
        close(chain.fates(L2, 2, 1), FATES_1_TO_2)
        close(chain.transition_table(L0, L2, 0, 2), TABLE_0_2)
        close(chain.transition_table(np.array([0, 0]), L2, 0, 2), TABLE_0_2_ONE_DOMAIN)
        close(chain.transition_table(L0, L1, 0, 1), F([[2, 0], [2, 2]]))
        close(chain.push(np.array([1.0, -1.0]), 0, 2).cpu().numpy()[:, 0], np.array([0.0, -9.0]))   # PI1^T PI0^T (1,-1)
        close(chain.pull(np.eye(2), 2, 0).cpu().numpy(), np.array([[2.0, 1.0], [2.0, 10.0]]))
        with pytest.raises(ValueError):
            chain.push(np.ones(2), 1, 1)
        with pytest.raises(ValueError):
            chain.pull(np.ones(3), 2, 0)                   # three rows for a time point of two spots
    assert all(s.closed for s in made)
    with pytest.raises(RuntimeError, match="closed"):
        chain.pull(np.eye(2), 2, 0)


def test_transport_chain_zero_mass_and_arrays(monkeypatch):
    lineage, latents, _ = _dense_chain(monkeypatch, [PI0, PI1_ZERO_ROW])
    with lineage.TransportChain(latents, device="cpu") as chain:
        close(chain.transition_table(L0, L2, 0, 2), TABLE_0_2_ZERO_ROW)
        own = np.array([0, 1, 2])
        tr = chain.trajectories(own, 1)
        close(tr[2], F([[1, 0, 0], [0, 0, 1]]))
        close(chain.fates(L2, 2, 1), F([[1, 0], [0, 0], [0, 1]]))
        # the stage's arrays, rows interleaved: input row order is kept
        tp = np.array([2, 0, 1, 1, 0, 2, 1])
        masks = [tp == t for t in range(3)]
        res = lineage.lineage_arrays(chain, [L0, own, L2], ["a", "b", "c"], masks)
        assert res["trajectory_names"].tolist() == ["a_0", "a_1", "b_0", "b_1", "b_2", "c_0", "c_1"]
        assert res["fate_names"].tolist() == ["c_0", "c_1"]
        X = res["trajectories"]
        assert X.shape == (7, 7) and np.isfinite(X).all()
        close(X[masks[2]][:, 2:5], F([[1, 0, 0], [0, 0, 1]]))
        close(X[masks[1]][:, 2:5], np.eye(3))
        close(res["fates"][masks[1]], F([[1, 0], [0, 0], [0, 1]]))
        close(res["fates"][masks[2]], np.eye(2))
        assert sorted(res["long_tables"]) == [(0, 2)]
        close(res["long_tables"][(0, 2)], TABLE_0_2_ZERO_ROW)


def test_transport_chain_closes_its_solvers_when_a_solve_raises(monkeypatch):
    lineage, latents, made = _dense_chain(monkeypatch, [PI0, PI1], fail_at=1)
    with pytest.raises(RuntimeError, match="solve failed"):
        lineage.TransportChain(latents, device="cpu")
    assert len(made) == 1 and made[0].closed


# ---- surfaces ----
def test_cli_lineage_flag():
    from spadot_amd import cli
    p = cli.build_parser()
    a = p.parse_args(["analyze", "-i", "x.npz", "--n_clusters", "5,7,7,6"])
    assert a.lineage is False
    assert a.n_clusters == [5, 7, 7, 6] and a.data == "x.npz" and a.prefix == "" and a.device == "cuda:0"
    assert a.output_dir is None and a.write_tmaps is False
    a = p.parse_args(["analyze", "-i", "x.npz", "--lineage"])
    assert a.lineage is True and a.write_tmaps is False and a.n_clusters is None
    a = p.parse_args(["analyze", "-i", "x.npz", "-o", "out", "--prefix", "p_", "--device", "cuda:1", "--write_tmaps", "--lineage"])
    assert a.output_dir == "out" and a.prefix == "p_" and a.device == "cuda:1" and a.write_tmaps and a.lineage


class _Args:
    def __init__(self, **kw):
        self.__dict__.update(dict(output_dir=None, prefix="", n_clusters=None, device="cuda:0", lineage=True), **kw)


def test_analyze_with_lineage_checks_its_input_before_the_device(tmp_path, monkeypatch):
    import torch
    from spadot_amd import analyze_ot
    from spadot_amd.analyze import analyze

    def no_device(*a, **k):
        raise AssertionError("device touched before the input checks")
    monkeypatch.setattr(torch, "as_tensor", no_device)
    monkeypatch.setattr(analyze_ot, "spot_transport", no_device)
    rng = np.random.default_rng(0)
    counts = [30, 12, 25]
    n = sum(counts)
    f = tmp_path / "latent.npz"
    np.savez_compressed(f, X=rng.normal(size=(n, 20)).astype(np.float32), rows=np.arange(n),
                        timepoint=np.repeat(np.arange(3), counts), spatial=rng.uniform(size=(n, 2)))
    a = _Args(data=str(f))
    with pytest.raises(ValueError, match="time point 1 has only 12 spots"):
        analyze(a)
    assert a.prefix == "adaptive_" and a.output_dir == str(tmp_path)
    with pytest.raises(ValueError, match="2 entries for 3 time points"):
        analyze(_Args(data=str(f), n_clusters=[3, 3]))
    with pytest.raises(ValueError, match="n_clusters = 13 for time point 1 of 12 spots"):
        analyze(_Args(data=str(f), n_clusters=[3, 13, 3]))
    assert not [x for x in tmp_path.iterdir() if x.name != "latent.npz"]
