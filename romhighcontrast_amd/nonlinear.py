"""The device-independent parts of the reference's second experiment, src/experiments/NonLinearROM.py ("learn the higher
PCA coordinates of a solution from its leading ones"): the parameter sweep, the full PCA of the tall snapshot block and
the index bookkeeping of the regression experiments.  The sweep runs on the device (SolutionsManagerFEM) and the PCA is
``pca_tall`` (rom_pca_tall: 25,000 x 81 is M >> dim, the shape rom_pod was not designed for).  The plots and the
PerplexityLab LabPipeline driver of the reference are out of scope.
"""
from __future__ import annotations

from collections import namedtuple

import numpy as np

from .lib.ReducedBasis import pca_tall
from .lib.SolutionsManagers import SolutionsManagerFEM

__all__ = ["ZERO", "Bounds", "MWhere", "draw_parameters", "vn_family_sampler", "do_pca", "get_known_unknown_indexes",
           "learn_eigenvalues"]

ZERO = 1e-15
Bounds = namedtuple("Bounds", "lower upper")
MWhere = namedtuple("MWhere", "m start")   # the m known PCA coordinates start at index `start`


def draw_parameters(n_max, geometry, lower_bounds, upper_bounds):
    """The reference's draw (:25-28): seed 42, then one ``uniform(lo, hi, n_max)`` call per block in row-major block
    order; sample i takes entry i of every call.  Returns the list of n_max arrays of shape ``geometry``."""
    np.random.seed(42)
    per_block = [np.random.uniform(lower_bounds, upper_bounds, n_max) for _ in range(int(np.prod(geometry)))]
    return [np.reshape(coefs, geometry) for coefs in zip(*per_block)]


def vn_family_sampler(n_max, geometry, lower_bounds, upper_bounds, mesh):
    """(:24-31) n_max snapshots of the (geometry, N = mesh) problem for the parameters of ``draw_parameters``."""
    a = draw_parameters(n_max, geometry, lower_bounds, upper_bounds)
    sm = SolutionsManagerFEM(blocks_geometry=tuple(geometry), N=mesh, num_cores=1, method="lsq")
    solutions = sm.generate_solutions(a)
    return {"solution_manager": sm, "a": a, "solutions": solutions}


def do_pca(solutions, ctx=None):
    """(:34-41) the full PCA of the snapshot block, all min(M, dim) modes: the scores of the block, the variances and
    the singular values.  ``do_pca.last`` keeps the TallPCA of the call (components, mean, resolved_modes_)."""
    from . import _ffi
    ctx = _ffi.get_context() if ctx is None else ctx
    M, dim = np.shape(solutions)
    n = min(M, dim)
    pca = pca_tall(ctx, solutions, n=n, center=True, scores=True, download=True)
    do_pca.last = pca
    return {"pca_projections": pca.scores, "explained_variance": pca.explained_variance_,
            "singular_values": pca.singular_values_}


def get_known_unknown_indexes(mwhere, pca_projections, learn_higher_modes_only, only_j=None):
    """(:44-51) columns of the scores that are given (``mwhere.m`` of them from ``mwhere.start``) and columns to learn:
    those after the known ones -- the first ``only_j`` of them when given -- and, unless ``learn_higher_modes_only``, the
    ones before the known block as well (listed first)."""
    n_modes = np.shape(pca_projections)[1]
    idx = np.arange(n_modes, dtype=int)
    first_after = mwhere.start + mwhere.m
    known = idx[mwhere.start:first_after]
    stop = n_modes if only_j is None else first_after + only_j
    unknown = idx[first_after:stop]
    if not learn_higher_modes_only:
        unknown = np.append(idx[:mwhere.start], unknown)
    return known, unknown


def learn_eigenvalues(model):
    """(:54-70) an experiment function around a scikit-learn pipeline: fit unknown <- known coordinates on the rows
    [n_test, n_test + n_train), predict the first n_test rows (always the same test rows), return the errors.  Host
    scikit-learn on the (M, n) scores: not a hot path."""

    def experiment(n_train, n_test, pca_projections, mwhere: MWhere, only_j, learn_higher_modes_only=True):
        known, unknown = get_known_unknown_indexes(mwhere, pca_projections, learn_higher_modes_only, only_j)
        train = slice(n_test, n_test + n_train)
        model.fit(pca_projections[train, known], pca_projections[train, unknown])
        predictions = np.asarray(model.predict(pca_projections[:n_test, known]))
        return {"error": pca_projections[:n_test, unknown] - predictions.reshape((-1, len(unknown)))}

    experiment.__name__ = " ".join(step[0] for step in model.steps)
    return experiment
