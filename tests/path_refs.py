"""The oracle loop and the algebra on top of it, stated once for every household-side path (beta_t, y_t[e], amin_t).
A new kind supplies three things, in a module of its own: its path and its economies; its backward step of period t (`Kind.step`);
and one `Kind` row, registered here — tests/path_checks.py and the suites read everything else from that row.

1. `forward_walk`: `Oracle.transition_step` forward with a dual D (ForwardIteration.jl:293), consumption from the budget, every
   output dotted with the dual post-transition D_t (ForwardIteration.jl:303-307), the group dots and the wealth grid's aggregate.
2. `oracle_path_sweeps`: the loop of the CPU oracle's household block with duals on the inputs, on the path and on the boundary — the
   directions in chunks of the oracle's widest instance, `Kind.step` backward from a dual `value_next` (BackwardIteration.jl:85),
   `forward_walk` forward. tests/sweep_refs.oracle_sweeps is this loop at the row `PLAIN`, which has no path.
3. the algebra: `unit_sweeps` (cached per session), the dense pair `jacobians`, the grid aggregate's `grid_jacobians`, their products
   `linear`, `grid_linear`, `linear_policies` and the transposed `path_bar`; `seeds`; `StubPathBlock`. All are written over the path's
   leading shape: () for beta_t and amin_t, (n_e,) for y_t[e]. Where a contraction differs between the two layouts its subscripts
   are selected by the layout — never reshaped into one flat contraction, which would move bits."""
from collections import namedtuple
from types import SimpleNamespace

import numpy as np

import cases
from oracle.oracle import SUPPORTED_N, pad_N


class Kind(namedtuple("Kind", "name table key model lead neutral step oracle budget floor also declares")):
    """a path kind: name ("shock", "income", "borrow": SteadyStateJacobian's `<name>_jacobian`); table: its key in hip._PATHS; key: the
    case key of its path; model: the case key of what the references take as the model (the Oracle, or HouseholdBlock's args);
    lead(orc): the path's leading shape — the path is (*lead, P), a seed (*lead, P, N); neutral(model, P): the path that changes
    nothing; step(w, Vn, xd, pd, t) -> (V_t, pol_t): the backward step of period t (`oracle_path_sweeps`); oracle(model): the
    Oracle that has the dimensions and makes the transition; budget: the path is additive income in consumption; floor: what every
    output's block of both unit sweeps must exceed (None: not asked); also(res): further keys of the sweeps' result; declares: a
    context of the suite declares the case's n_het outputs."""
    __slots__ = ()

    @property
    def binding(self):
        """the kind's row of hip._PATHS: the C symbols, the attribute of the path in force, the seed's name"""
        from hank_amd.hip import _PATHS
        return _PATHS[self.table]

    def method(self, which):
        """the binding's method of the entry `which` (set, jvp, vjp, fake_news): the C symbol without its prefix"""
        return getattr(self.binding, which).removeprefix("hank_")

    @property
    def bar(self):
        """the name of the path's cotangent: beta_bar, y_bar, amin_bar"""
        return self.binding.seed[1:] + "_bar"


KINDS = {}


def register(kind):
    KINDS[kind.name] = kind
    return kind


def _plain_step(w, Vn, xd, pd, t):
    st, V, pol = w.orc.value_function(Vn, xd[0, t], xd[1, t], w.Nc, xd[2, t] if w.n_hh > 2 else None)
    assert st == 0, (t, st)
    return V, pol


PLAIN = Kind("plain", None, None, "orc", lambda orc: (), lambda orc, P: np.zeros(P), _plain_step, lambda orc: orc, False, None, None, True)


# ---- 1. the forward walk ------------------------------------------------------------------------------------------------------
def forward_walk(orc, pol, val, xd, Dd, n, n_het, gamma=None, groups=None, income=None):
    """pol[t], val[t] (n_a, n_e, 1 + Nc): the recorded duals of the policy and of the value, t = 0 .. P - 1; xd (n_hh, P, 1 + Nc) the
    inputs' dual; Dd (n_a, n_e, 1 + Nc) the dual D_0, its tangent slots already seeded; n <= Nc the directions in use; gamma is
    needed for n_het = 4 only; groups = (W (G, K), base[K]) (hank_set_group_outputs' arguments) or None; income (n_e, P, 1 + Nc) or
    None: an additive per-state income dual, y_t[e]'s direct term in consumption.
    -> (dict, the final Dd): agg (P, n_het) and dagg (P, n_het, n) of (savings, consumption, Value[, UCE]) with the post-transition
    D_t — the shapes of hank_get_het_outputs; agg2 (P,), dagg2 (P, n) the wealth grid's aggregate; grp (P, K), dgrp (P, K, n) the
    weighted dots of 1 (base 0), a' (1) or c (2) with the same dual D_t; Dseq (P, n_a, n_e) the post-transition D_t."""
    n_hh, P, Nc = xd.shape[0], xd.shape[1], xd.shape[2] - 1
    n_a, n_e, a, z = orc.n_a, orc.n_e, orc.a, orc.z
    K = 0 if groups is None else np.asarray(groups[0]).shape[1]
    agg, agg2 = np.zeros((P, n_het)), np.zeros(P)
    dagg, dagg2 = np.zeros((P, n_het, n)), np.zeros((P, n))
    grp, dgrp = np.zeros((P, K)), np.zeros((P, K, n))
    Dseq = np.zeros((P, n_a, n_e))
    for t in range(P):
        Dd = orc.transition_step(pol[t], Dd, Nc)
        p0, dp, D0, dDt = pol[t][..., 0], pol[t][..., 1:1 + n], Dd[..., 0], Dd[..., 1:1 + n]
        tr, dtr = (xd[2, t, 0], xd[2, t, 1:1 + n]) if n_hh > 2 else (0.0, np.zeros(n))
        # consumption: the affine map of the policy dual, c = (1 + r) a + w z_e + tr [+ y_e] - a' (KrusellSmith.jl:79)
        c0_ = (1.0 + xd[0, t, 0]) * a[:, None] + xd[1, t, 0] * z[None, :] + tr
        dc = xd[0, t, 1:1 + n] * a[:, None, None] + xd[1, t, 1:1 + n] * z[None, :, None] + dtr
        if income is not None:
            c0_, dc = c0_ + income[None, :, t, 0], dc + income[None, :, t, 1:1 + n]
        c0_, dc = c0_ - p0, dc - dp
        fs = [(p0, dp), (c0_, dc), (val[t][..., 0], val[t][..., 1:1 + n])]
        if n_het > 3:
            fs.append((z[None, :] * c0_ ** (-gamma), (z[None, :] * (-gamma) * c0_ ** (-gamma - 1.0))[..., None] * dc))
        for o, (f0, df) in enumerate(fs[:n_het]):
            agg[t, o] = np.sum(f0 * D0)
            dagg[t, o] = np.einsum("aen,ae->n", df, D0) + np.einsum("ae,aen->n", f0, dDt)
        for k in range(K):
            Wk = np.asarray(groups[0])[:, k].reshape((n_a, n_e), order="F")
            f0, df = ((np.ones_like(p0), np.zeros_like(dp)), fs[0], fs[1])[int(groups[1][k])]
            grp[t, k] = np.sum(Wk * f0 * D0)
            dgrp[t, k] = np.einsum("aen,ae->n", df, Wk * D0) + np.einsum("ae,aen->n", Wk * f0, dDt)
        agg2[t] = np.sum(a[:, None] * D0)
        dagg2[t] = np.einsum("a,aen->n", a, dDt)
        Dseq[t] = D0
    return dict(agg=agg, dagg=dagg, agg2=agg2, dagg2=dagg2, grp=grp, dgrp=dgrp, Dseq=Dseq), Dd


# ---- 2. the sweep -------------------------------------------------------------------------------------------------------------
def _dual(level, seeds, c0, n, Nc):
    """(*shape, 1 + Nc): the level in slot 0, directions c0 .. c0 + n of seeds (*shape, N) (None: zeros) behind it"""
    d = np.zeros(np.shape(level) + (1 + Nc,))
    d[..., 0] = level
    if seeds is not None:
        d[..., 1:1 + n] = np.asarray(seeds)[..., c0:c0 + n]
    return d


def oracle_path_sweeps(kind, model, x, V, D, path=None, gamma=None, n_het=2, dx=None, dpath=None, groups=None, dV=None, dD=None):
    """kind: a `Kind` row; model: what the row's references take (`Kind.model`); x (n_hh, P), boundary V (n_a, n_e), D (G,), path
    (*lead, P) (None: the neutral one); seeds dx (n_hh, P, N), dpath (*lead, P, N), dV, dD (n_a, n_e, N), None = zeros (all None: the
    level alone, one zero direction); gamma and groups as in `forward_walk`.
    -> dict: `forward_walk`'s agg, dagg (P, n_het, N), agg2, dagg2, grp, dgrp, Dseq; pol (P, n_a, n_e), dpol (P, n_a, n_e, N); D
    (n_a, n_e) the last D_t; whatever the kind's step records in w.rec, stacked over t; and the keys of `Kind.also`.
    The step is handed w — model, orc, gamma, n_hh, seeded (dpath was given), the chunk's n and Nc, rec (name -> list over t) — the
    incoming dual value Vn, the duals xd (n_hh, P, 1 + Nc) and pd (*lead, P, 1 + Nc) of the inputs and of the path, and t."""
    x = np.asarray(x, dtype=np.float64)
    n_hh, P = x.shape
    orc = kind.oracle(model)
    n_a, n_e = orc.n_a, orc.n_e
    path = kind.neutral(model, P) if path is None else np.asarray(path, dtype=np.float64)
    assert path.shape == kind.lead(orc) + (P,), (kind.name, path.shape)
    N = next((np.asarray(v).shape[-1] for v in (dx, dpath, dV, dD) if v is not None), 1)
    w = SimpleNamespace(model=model, orc=orc, gamma=gamma, n_hh=n_hh, seeded=dpath is not None, rec={})
    out = {k: [] for k in ("dagg", "dagg2", "dpol", "dgrp")}
    for c0 in range(0, N, SUPPORTED_N[-1]):
        w.n = n = min(N, c0 + SUPPORTED_N[-1]) - c0
        w.Nc = Nc = pad_N(n)
        xd, pd, Vn = _dual(x, dx, c0, n, Nc), _dual(path, dpath, c0, n, Nc), _dual(V, dV, c0, n, Nc)
        Dd = _dual(np.asarray(D).reshape((n_a, n_e), order="F"), dD, c0, n, Nc)
        pol, val = [None] * P, [None] * P
        for t in range(P - 1, -1, -1):
            Vn, pol[t] = kind.step(w, Vn, xd, pd, t)
            val[t] = Vn
        f, Dd = forward_walk(orc, pol, val, xd, Dd, n, n_het, gamma, groups, pd if kind.budget else None)
        for k in ("dagg", "dagg2", "dgrp"):
            out[k].append(f[k])
        out["dpol"].append(np.stack([p[..., 1:1 + n] for p in pol]))
    res = {k: np.concatenate(v, axis=-1) for k, v in out.items()}
    res.update(agg=f["agg"], agg2=f["agg2"], grp=f["grp"], pol=np.stack([p[..., 0] for p in pol]), D=Dd[..., 0], Dseq=f["Dseq"])
    res.update({k: np.stack(v) for k, v in w.rec.items()})
    if kind.also is not None:
        res.update(kind.also(res))
    return res


# ---- 3. the algebra -----------------------------------------------------------------------------------------------------------
_JAC = {}


def _ident(model):
    """what the unit sweeps' cache keys a model on: an Oracle's identity; HouseholdBlock's args: the bytes of the first five"""
    if hasattr(model, "value_function"):
        return id(model)
    return (np.asarray(model[0]).tobytes(), np.asarray(model[1]).tobytes(), np.asarray(model[2]).tobytes(), float(model[3]), float(model[4]))


def unit_sweeps(kind, model, x, V, D, path=None, gamma=None, n_het=2):
    """-> (sx, sp): `oracle_path_sweeps` with cases.unit_tangents as dx, and with dpath = the prod(lead) P unit directions (the
    leading axes fastest), once per session and key (the kind, the model as `_ident` has it and the bits of every input); with
    `Kind.floor` every output's block of either must exceed it"""
    x, V, D = (np.ascontiguousarray(v, dtype=np.float64) for v in (x, V, D))
    n_hh, P = x.shape
    path = np.ascontiguousarray(kind.neutral(model, P) if path is None else path, dtype=np.float64)
    key = (kind.name, _ident(model), x.tobytes(), V.tobytes(), D.tobytes(), path.tobytes(), gamma, n_het)
    if key not in _JAC:
        sx = oracle_path_sweeps(kind, model, x, V, D, path, gamma, n_het, dx=cases.unit_tangents(n_hh, P))
        sp = oracle_path_sweeps(kind, model, x, V, D, path, gamma, n_het, dpath=np.eye(path.size).reshape(path.shape + (path.size,), order="F"))
        for o in range(n_het if kind.floor is not None else 0):
            assert np.abs(sx["dagg"][:, o, :]).max() > kind.floor and np.abs(sp["dagg"][:, o, :]).max() > kind.floor, (o, n_het, x.shape, V.shape)
        _JAC[key] = (sx, sp)
    return _JAC[key]


def _by_lead(d, lead, P):
    """unit columns d (..., prod(lead) P), the leading axes fastest -> (..., *lead, P); d itself where lead is ()"""
    if not lead:
        return d
    return np.ascontiguousarray(np.moveaxis(d.reshape(d.shape[:-1] + (P,) + lead), -1, -2))


def jacobians(kind, model, x, V, D, path=None, gamma=None, n_het=2):
    """the dense Jacobians of the first n_het heterogeneous outputs at the path, from the oracle's unit tangents: -> (Jx (n_het, P,
    n_hh, P), d output o at t / d input k at s — the layout cases.jt takes — and Jp (P, n_het, *lead, P), d output o at t / d
    path_s[lead] as [t, o, *lead, s]). The tangent map is linear, so the pair is the reference of every width:
        dagg = Jx dx + Jp dpath (`linear`), xhh_bar = cases.jt(Jx[:n_het], yb), path_bar[*lead, s, m] = sum_{t,o} Jp[t, o, *lead, s] yb[t, o, m]
    (`path_bar`). Cached per session (`unit_sweeps`)."""
    sx, sp = unit_sweeps(kind, model, x, V, D, path, gamma, n_het)
    n_hh, P = np.asarray(x).shape
    return np.ascontiguousarray(sx["dagg"].reshape(P, n_het, P, n_hh).transpose(1, 0, 3, 2)), _by_lead(sp["dagg"], kind.lead(kind.oracle(model)), P)


def grid_jacobians(kind, model, x, V, D, path=None, gamma=None, n_het=2):
    """the same pair for the grid-weighted aggregate of hank_get_grid_aggregates, from the same two sweeps:
    -> (J2x (P, n_hh, P) as [t, k, s], J2p (P, *lead, P) as [t, *lead, s])"""
    sx, sp = unit_sweeps(kind, model, x, V, D, path, gamma, n_het)
    n_hh, P = np.asarray(x).shape
    return np.ascontiguousarray(sx["dagg2"].reshape(P, P, n_hh).transpose(0, 2, 1)), _by_lead(sp["dagg2"], kind.lead(kind.oracle(model)), P)


def linear(J, dx, dp):
    """dagg (P, n_het, N) = Jx dx + Jp dpath of J = `jacobians`' pair; dx (n_hh, P, N) or None, dp (*lead, P, N) or None"""
    Jx, Jp = J
    N = next(v.shape[-1] for v in (dx, dp) if v is not None)
    out = np.zeros((Jp.shape[0], Jp.shape[1], N))
    if dx is not None:
        out += np.einsum("otks,ksn->ton", Jx, dx)
    if dp is not None:
        out += np.einsum("tos,sn->ton" if Jp.ndim == 3 else "toes,esn->ton", Jp, dp)
    return out


def grid_linear(J2, dx, dp):
    """dagg2 (P, N) = J2x dx + J2p dpath of J2 = `grid_jacobians`' pair; dx (n_hh, P, N) or None, dp (*lead, P, N) or None"""
    by_path = 0.0 if dp is None else J2[1] @ dp if J2[1].ndim == 2 else np.einsum("tes,esn->tn", J2[1], dp)
    return (0.0 if dx is None else np.einsum("tks,ksn->tn", J2[0], dx)) + by_path


def path_bar(Jp, yb):
    """path_bar (*lead, P, M): [*lead, s, m] = sum_{t,o} Jp[t, o, *lead, s] yb[t, o, m] over the outputs yb (P, n_het, M) holds"""
    return np.einsum("tos,tom->sm" if Jp.ndim == 3 else "toes,tom->esm", Jp[:, :yb.shape[1]], yb)


def linear_policies(kind, model, x, V, D, path=None, gamma=None, n_het=2, *, dx=None, dp=None):
    """dpol (P, n_a, n_e, N) of the directions dx (n_hh, P, N) or None and dp (*lead, P, N) or None, from the unit sweeps' policy
    partials (the map is linear)"""
    sx, sp = unit_sweeps(kind, model, x, V, D, path, gamma, n_het)
    n_hh, P = np.asarray(x).shape
    N = next(v.shape[-1] for v in (dx, dp) if v is not None)
    out = np.zeros(sx["dpol"].shape[:3] + (N,))
    if dx is not None:
        out += sx["dpol"] @ np.asarray(dx).reshape((n_hh * P, N), order="F")
    if dp is not None:
        dp = np.asarray(dp)
        out += sp["dpol"] @ (dp if dp.ndim == 2 else dp.reshape((-1, N), order="F"))
    return out


def seeds(kind, c, N, seed, t_only=None):
    """(dx (n_hh, P, N), dpath (*lead, P, N)): random directions of the inputs' and of the path's scale; t_only: dpath in that period
    alone"""
    rng = np.random.default_rng(seed)
    n_hh, P = c["x"].shape
    dx = rng.standard_normal((n_hh, P, N)) * 1e-2
    dp = rng.standard_normal(c[kind.key].shape + (N,)) * 1e-2
    if t_only is not None:
        keep = np.zeros((P, 1)); keep[t_only] = 1.0
        dp = dp * keep
    return dx, dp


class StubPathBlock:
    """stands in for the device context under SteadyStateJacobian's `<kind>_jacobian`: its `method_name` (fake_news_shock, ...) hands
    out the F and Dv it was made with"""

    def __init__(self, method_name, F, Dv):
        self.F, self.Dv, self.calls = F, Dv, 0
        setattr(self, method_name, self._fake_news)

    def _fake_news(self, n_het):
        self.calls += 1
        return self.F[..., :n_het].copy(), self.Dv[..., :n_het].copy()
