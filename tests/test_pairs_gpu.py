"""The dispatch over the padded threshold count that the three pair-counting entries share (csrc/pair_count.h) on the
MI355X: B = 17 and B = 33 run the 32- and 48-column kernels of spadot_cooccur_counts, spadot_cooccur_null and
spadot_ripley_counts, which the tests of the stages themselves reach only through ripley's planted set (32) or not at all (48).
Everything the device computes is an integer, so every comparison is assert_array_equal against the numpy restatements."""
import numpy as np
import pytest
import torch

import pairs_cases as cases

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


def _dev(x):
    return torch.as_tensor(np.asarray(x), device=DEV)


@pytest.mark.parametrize("B", cases.BINS)
def test_every_entry_matches_its_restatement_at_the_padded_widths_32_and_48(B):
    from spadot_amd import stage_ops as ops
    from spadot_amd.cooccurrence import cooccurrence_counts, cooccurrence_null_counts
    from spadot_amd.ripley import ripley_counts
    assert ops.cooccur_padded(B) == {17: 32, 33: 48}[B]
    xy, lab, r2, K = cases.cooccur_problem(B)
    plain = cooccurrence_counts([_dev(xy)], [lab], radii_sq=[r2], n_clusters=[K])[0]
    np.testing.assert_array_equal(plain, cases.want("cooccur", B))
    null = cooccurrence_null_counts([_dev(xy)], [lab], radii_sq=[r2], n_perms=cases.S, seed=cases.SEED, n_clusters=[K])[0]
    np.testing.assert_array_equal(null, cases.want("null", B))
    np.testing.assert_array_equal(null[0], plain)                                    # pattern 0 of the null is the plain count
    for kind in ("labels", "csr"):
        p = cases.ripley_problem(B, kind)
        got = ripley_counts([_dev(p["xy"])], [p["lab"]], radii_sq=[p["r2"]], n_sim=p["S"], n_probes=p["M"], null=kind,
                            seed=cases.SEED, n_clusters=[p["K"]], problem_ids=[p["g"]])[0]
        assert got.shape == (p["K"], 1 + cases.S, 3, B) and got.dtype == np.int64
        np.testing.assert_array_equal(got, cases.want(kind, B), err_msg=kind)
        co = cooccurrence_counts([_dev(p["xy"])], [p["lab"]], radii_sq=[p["r2"]], n_clusters=[p["K"]])[0]
        np.testing.assert_array_equal(got[:, 0, 0, :], co[np.arange(p["K"]), np.arange(p["K"]), :])      # observed Lc: the diagonal
