"""spadot_amd -- MI355X-native implementation of SpaDOT's train and analyze stages.

`train` mirrors SpaDOT.train and `analyze` mirrors SpaDOT.analyze (reference SpaDOT/__init__.py:1-5);
`python -m spadot_amd train|analyze` is the command line (reference cli.py).  The preprocess stage is out
of scope: use the reference's `SpaDOT preprocess`.  Importing this package does not load the HIP
libraries; the first numeric call does, and fails loudly if they have not been built
(python -m spadot_amd.csrc.build)."""
from .train import train  # noqa: F401  (binds the function over the submodule name, as the reference does)
from .analyze import analyze  # noqa: F401

__all__ = ["train", "analyze"]
