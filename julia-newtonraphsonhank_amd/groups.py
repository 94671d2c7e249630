"""Weight arrays for the group outputs of the household block (`HouseholdBlock.set_group_outputs`): who moves.

A group is a weight vector over the grid, indexed like the distribution D (pt = e·n_a + ia, the column-major vec of the
(n_a, n_e) matrix), and fixed over time: the groups are defined at the steady state, by wealth LEVEL or by productivity state,
and the aggregates Y^k_t = Σ W_k f_t D_t (ForwardIteration.jl:303-307 with a weight) then follow the households on those grid
points along the transition. Every function returns W (G, K), one column per group."""
from __future__ import annotations

import numpy as np


def _rows(member, n_e):
    """member (n_a, K) row indicators -> W (G, K): every productivity column carries the same rows."""
    return np.ascontiguousarray(np.tile(np.asarray(member, dtype=np.float64), (n_e, 1)))


def wealth_groups(D_ss, n_a, n_e, edges):
    """groups by position in the steady-state wealth distribution: `edges` are increasing CDF points from 0 to 1 (e.g.
    [0, 0.5, 0.9, 1]: the bottom half, the next 40 %, the top decile). Wealth row ia belongs to group g when the CDF up to
    and including it lies in (edges[g], edges[g+1]], so the rows of a group are contiguous, the groups are a partition of
    unity, and the mass up to a group's last row is within one row's mass of its upper edge. -> W (G, len(edges) - 1)."""
    edges = np.asarray(edges, dtype=np.float64)
    if edges.ndim != 1 or edges.size < 2 or edges[0] != 0.0 or edges[-1] != 1.0 or np.any(np.diff(edges) <= 0):
        raise ValueError(f"edges must increase from 0 to 1, got {edges}")
    D = np.asarray(D_ss, dtype=np.float64).reshape((n_a, n_e), order="F")
    cdf = np.cumsum(D.sum(axis=1))
    cdf /= cdf[-1]
    g = np.searchsorted(edges[1:-1], cdf, side="left")          # inner edges strictly below the row's CDF
    member = g[:, None] == np.arange(edges.size - 1)[None, :]
    return _rows(member, n_e)


def productivity_groups(n_a, n_e):
    """one group per productivity state: W (G, n_e), column e the indicator of state e."""
    return np.ascontiguousarray(np.repeat(np.eye(n_e), n_a, axis=0))


def constrained(n_a, n_e):
    """the households at the first grid point (the borrowing limit's mass point): W (G, 1), row 0 of every column. With base
    GROUP_MASS its output is the mass of constrained households."""
    member = np.zeros((n_a, 1))
    member[0, 0] = 1.0
    return _rows(member, n_e)
