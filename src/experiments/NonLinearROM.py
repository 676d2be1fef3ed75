"""The sampling / PCA / index part of the reference's src/experiments/NonLinearROM.py under its import path (plots and
the LabPipeline driver are out of scope; see romhighcontrast_amd/nonlinear.py)."""
import os as _os
import sys as _sys

_root = _os.path.dirname(_os.path.dirname(_os.path.dirname(_os.path.abspath(__file__))))
if _root not in _sys.path:
    _sys.path.insert(0, _root)

from romhighcontrast_amd.nonlinear import (ZERO, Bounds, ForestMap, MLPMap, MWhere, PolynomialMap, TreeMap, do_pca, draw_parameters,  # noqa: E402,F401
                                           get_known_unknown_indexes, learn_eigenvalues, learn_eigenvalues_device,
                                           nonlinear_reconstruction, vn_family_sampler)
from romhighcontrast_amd.lib.ReducedBasis import TallPCA, pca_tall  # noqa: E402,F401
from romhighcontrast_amd.lib.SolutionsManagers import SolutionsManagerFEM  # noqa: E402,F401
