"""spadot_amd -- MI355X-native implementation of SpaDOT's preprocess, train and analyze stages.

`preprocess` mirrors SpaDOT.preprocess (SPARK-X gene selection and scaling on the device; the gene clusters of the balancing
rule come from K-means by default, or with gene_clusters='louvain' from the reference's SCTransform + Louvain), `train` mirrors SpaDOT.train and `analyze` mirrors
SpaDOT.analyze (reference SpaDOT/__init__.py:1-5); `python -m spadot_amd preprocess|train|analyze` is the command line
(reference cli.py).  Importing this package does not load the HIP libraries; the first numeric call does, and fails loudly
if they have not been built (python -m spadot_amd.csrc.build)."""
from .preprocess import preprocess  # noqa: F401  (binds the function over the submodule name, as the reference does)
from .train import train  # noqa: F401
from .analyze import analyze  # noqa: F401

__all__ = ["preprocess", "train", "analyze"]
