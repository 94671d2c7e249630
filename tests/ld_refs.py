"""A plain extended-precision restatement of the two granular steps, with a running error bound of the float64 kernels.

What it restates, from the reference's Julia text (nothing here is copied from it or reads it):
  `egm_step`      ValueFunction (KrusellSmith.jl:43-83): value and policy of one EGM step with N partials. The partials follow the
                  Dual rules of ForwardDiff's dual.jl — Dual^Real carries y v^(y-1) (:563-572), a quotient carries 1/v and -u/v^2
                  (:528-539), `max` passes or drops the partials (the DiffRules rule) — written as the linear coefficients
                  (kc, A, B, u, v) they amount to. Two families: the inputs (r, w), and (r, w, tr) with a lump-sum transfer in
                  the budget, as hh_tr (csrc/hank_device.h) and the C oracle take it;
  `forward_step`  make_endogenous_transition and transition_step (ForwardIteration.jl:37-99) followed by the exogenous mixing
                  kron(Pi', I) (:280-284), with partials, and the aggregate dot(policy, D_t) of :301-307. `D_prev` may be a
                  `Tracked` itself: pushing D_0 through a policy sequence compounds the bound period by period.

Every function takes a `dtype`: the same text runs in np.longdouble (the reference: 64 mantissa bits) and in np.float64 (a host
model of the kernels). The module skips where the long double is not the 80-bit x87 format.

Beside every value a `Tracked` carries a first-order RUNNING ERROR BOUND of the float64 kernel (Higham, Accuracy and Stability
of Numerical Algorithms, section 3.3), as float64 arrays, by these rules and no others:
  * an input (grids, Pi, V_next, policy, D_prev, prices, partials' seeds) is exact;
  * each float64 operation of the kernel adds 2^-53 |result| to what its operands' bounds propagate to at first order
    (|dz/dx| e_x + |dz/dy| e_y); a product with a power of two adds nothing;
  * a sum of n terms adds (n - 1) 2^-53 sum|terms|, whatever its order: the atomics, tree sums and block partials are covered;
  * fast_rcp, fast_rsqrt and fast_sqrt add U = 2 ulps (2 x 2^-52 |result|): csrc/hank_kernels.h's own claim;
  * the generic `pow` arm adds 2 ulps as well: the ROCm installation's documents carry no accuracy table of the device library's
    fp64 pow (searched under its share/ tree), so the fallback figure stands, not a documented one;
  * where the kernel's outcome is exact (a policy at the borrowing limit, flat extrapolation, the zero partials there, a whole
    mass moved by a clamp) the bound is zero.
The expressions are the KERNELS' where those round differently from the textbook form: diet_kc rebuilds cm as (s opr + wz) - a,
diet_v takes u sqrt(u), the lottery weight is w = (p - a_l) / gap with 1 - w formed afterwards, one reciprocal of the knot
distance serves both interpolation quotients, egm_Y_finish's `max` rule. `bound()` rounds the bound up by 1 + 1e-6 for its own
float64 arithmetic; there is no other margin: the bound is derived, not tuned. (The long double reference's own rounding,
2^-64 per operation, is 2^-11 of the bound and is not modelled.)

Ambiguous brackets are FLAGGED, not bounded: a first-order bound says nothing where a rounding error may change a branch. For the
EGM interpolation that is a grid point within the tracked error of a knot (or an interpolated policy within its error of the
borrowing limit); for the lottery a policy within one ulp of a grid point without being on it. An exact tie of the LOTTERY — a
policy on a grid point, both of them inputs — is no ambiguity: every side takes the same branch by the same comparison, and the
forward cases hold such ties and test them as ties. The EGM interpolation has no such tie to test: a knot is a RESULT, so a grid
point that equals a float64 knot equals a rounded value, the long double knot lies beside it, and the entry is flagged like any
other grid point within the knot's error. No case here constructs one, and none occurred."""
import numpy as np
import pytest

if np.finfo(np.longdouble).nmant != 63:
    pytest.skip(f"np.longdouble has {np.finfo(np.longdouble).nmant} mantissa bits here, not the 63 of the x87 extended format: "
                "no reference more precise than the kernels", allow_module_level=True)

U53 = 2.0 ** -53            # unit roundoff of one float64 operation
ULP = 2.0 ** -52            # an ulp, relative to the result, at most
U_FAST = 2                  # fast_rcp / fast_rsqrt / fast_sqrt: "within an ulp or two"
U_POW = 2                   # the device library's pow: no table on the machine, the fallback figure
ROUND_UP = 1.0 + 1e-6       # the bound's own float64 arithmetic


def _mag(v):
    return np.abs(v).astype(np.float64)


class Tracked:
    """a value (in the run's dtype) and the running error bound of the float64 kernel's value (float64), element by element"""
    __slots__ = ("v", "e")

    def __init__(self, v, e=0.0):
        self.v = np.asarray(v)
        self.e = np.broadcast_to(np.asarray(e, dtype=np.float64), self.v.shape)

    def _of(self, b):
        return b if isinstance(b, Tracked) else Tracked(np.asarray(b, dtype=self.v.dtype))

    def bound(self):
        return self.e * ROUND_UP

    # ---- the float64 operations: each adds 2^-53 |result|
    def __add__(self, b):
        b = self._of(b)
        v = self.v + b.v
        return Tracked(v, self.e + b.e + U53 * _mag(v))

    __radd__ = __add__

    def __sub__(self, b):
        b = self._of(b)
        v = self.v - b.v
        return Tracked(v, self.e + b.e + U53 * _mag(v))

    def __rsub__(self, b):
        return self._of(b) - self

    def __mul__(self, b):
        b = self._of(b)
        v = self.v * b.v
        return Tracked(v, _mag(b.v) * self.e + _mag(self.v) * b.e + U53 * _mag(v))

    __rmul__ = __mul__

    def __truediv__(self, b):
        """the IEEE quotient"""
        b = self._of(b)
        v = self.v / b.v
        return Tracked(v, (self.e + _mag(v) * b.e) / _mag(b.v) + U53 * _mag(v))

    def __rtruediv__(self, b):
        return self._of(b) / self

    # ---- exact in float64
    def __neg__(self):
        return Tracked(-self.v, self.e)

    def scaled(self, c):
        """times a power of two"""
        assert np.frexp(abs(float(c)))[0] == 0.5, c
        return Tracked(self.v * self.v.dtype.type(c), self.e * abs(float(c)))

    # ---- the kernels' functions: `ulps` of the result on top of the propagated bound
    def rcp(self, ulps=U_FAST):
        v = 1 / self.v
        return Tracked(v, self.e * _mag(v) ** 2 + ulps * ULP * _mag(v))

    def rsqrt(self, ulps=U_FAST):
        v = 1 / np.sqrt(self.v)
        return Tracked(v, 0.5 * _mag(v / self.v) * self.e + ulps * ULP * _mag(v))

    def sqrt(self, ulps=U_FAST):
        v = np.sqrt(self.v)
        return Tracked(v, 0.5 * _mag(v / self.v) * self.e + ulps * ULP * _mag(v))

    def pow(self, y, ulps=U_POW):
        """self ^ y for an exact float64 exponent"""
        y = np.float64(y)
        v = np.power(self.v, self.v.dtype.type(y))
        return Tracked(v, abs(y) * _mag(v / self.v) * self.e + ulps * ULP * _mag(v))

    # ---- sums, any order: (n - 1) 2^-53 sum |terms|
    def sum(self, axis=None):
        n = self.v.size if axis is None else self.v.shape[axis]
        return Tracked(np.sum(self.v, axis=axis), np.sum(self.e, axis=axis) + max(n - 1, 0) * U53 * np.sum(_mag(self.v), axis=axis))

    def scatter_sum(self, idx, size):
        """out[k] = the sum of this (flat) array's entries with idx == k"""
        v = np.zeros(size, dtype=self.v.dtype)
        e, m, n = np.zeros(size), np.zeros(size), np.zeros(size)
        np.add.at(v, idx, self.v); np.add.at(e, idx, self.e); np.add.at(m, idx, _mag(self.v)); np.add.at(n, idx, 1.0)
        return Tracked(v, e + np.maximum(n - 1.0, 0.0) * U53 * m)

    # ---- moving data: exact
    def __getitem__(self, k):
        return Tracked(self.v[k], self.e[k])

    def reshape(self, *shape):
        return Tracked(self.v.reshape(*shape), self.e.reshape(*shape))

    @staticmethod
    def where(cond, a, b):
        return Tracked(np.where(cond, a.v, b.v), np.where(cond, a.e, b.e))

    @staticmethod
    def concat(parts):
        return Tracked(np.concatenate([p.v for p in parts]), np.concatenate([p.e for p in parts]))


def pow_crra(x, y):
    """csrc/hank_kernels.h pow_crra: the exponents CRRA utility produces most often go through a reciprocal or a reciprocal
    square root, the others through the device library's pow"""
    if y == -0.5:
        return x.rsqrt()
    if y == -2.0:
        return (x * x).rcp()
    if y == -1.0:
        return x.rcp()
    return x.pow(y)


def lerp(f, omf, ai, aj):
    """g = (1 - f) ai + f aj on exact ai, aj, with omf = 1 - f formed by ONE subtraction: the error of f reaches omf with the
    opposite sign, so it moves g by (aj - ai) df — not by the (|ai| + |aj|) e_f that two independent operands would give, a
    hundred times more at the top of a wealth grid. What is added: omf's own rounding times |ai|, the two products', the sum's."""
    g = omf.v * ai + f.v * aj
    return Tracked(g, _mag(aj - ai) * f.e + U53 * (2.0 * _mag(omf.v * ai) + _mag(f.v * aj) + _mag(g)))


def egm_step(dtype, a, z, Pi, beta, gamma, bc, V_next, dV_next, x, dx, diet):
    """One EGM step (KrusellSmith.jl:43-83) at the inputs x = (r, w) or (r, w, tr), with the partials dV_next (n_a, n_e, N) and
    dx (len(x), N); Pi[e, e2] = P(e -> e2). `diet`: the record diet of the context (kc and v rebuilt by diet_kc / diet_v).
    -> dict of Tracked V, policy (n_a, n_e), dV, dpolicy (n_a, n_e, N), and the boolean (n_a, n_e) masks
       ambiguous (see the module's text), constrained (the borrowing limit binds), below / above (flat extrapolation); the
       intermediate s (knots), ds (their partials), kc (d s / d E) and v (the coefficient of d c in d V) for whoever models another
       operation order."""
    T = lambda q: Tracked(np.asarray(q, dtype=dtype))          # noqa: E731 — an exact input
    a, z, Pi = (np.asarray(q, dtype=np.float64) for q in (a, z, Pi))
    n_a, n_e = V_next.shape
    N = dx.shape[1]
    gamma, beta, bc = np.float64(gamma), np.float64(beta), np.float64(bc)
    r, w, tr = x[0], x[1], (x[2] if len(x) > 2 else None)
    dr, dw, dtr = T(dx[0]), T(dx[1]), (T(dx[2]) if len(x) > 2 else None)
    ac, zr = T(a[:, None]), T(z[None, :])

    # ---- the X half (:59-62): expected marginal value -> consumption and the endogenous knots s[a', e]
    E = (T(V_next[:, None, :]) * T(Pi[None, :, :])).sum(axis=2)                    # (V Pi')[a, e] = sum_e2 V[a, e2] Pi[e, e2]
    bE = E * beta
    ex = np.float64(-1.0) / gamma                                                  # (-1 / γ) is a Float64 in the reference too
    cm = pow_crra(bE, ex)
    opr = T(1.0) + r
    rho = 1.0 / opr
    wz = T(w) * zr
    wz_tr = wz if tr is None else wz + tr
    s = rho * ((cm - wz_tr) + ac)
    if diet:                                                                       # diet_kc: cm back out of s, then a product
        cmr = (s * opr + wz_tr) - ac
        k = rho * T(beta).scaled(-1.0 / gamma)
        kc = k * (cmr * cmr * cmr) if gamma == 2.0 else k * (cmr * cmr)
    else:                                                                          # Dual^Real: β y (βE)^(y-1) = β y cm / (βE)
        kc = rho * (T(beta) * ex * (cm / bE))
    dE = (T(dV_next[:, None, :, :]) * T(Pi[None, :, :, None])).sum(axis=2)         # (n_a, n_e, N)
    inc_d = zr[..., None] * dw if dtr is None else zr[..., None] * dw + dtr        # d (w z_e + tr)
    ds = kc[..., None] * dE - rho * (inc_d + s[..., None] * dr)

    # ---- the Y half (:66-80): Gridded(Linear()) + Flat() on the knots of column e, the borrowing constraint, the marginal value
    i = np.empty((n_a, n_e), dtype=np.int64)
    below, above, amb = (np.zeros((n_a, n_e), dtype=bool) for _ in range(3))
    sb = s.bound()
    for e in range(n_e):
        sv = s.v[:, e]
        assert np.all(np.diff(sv) > 0), "knots must be sorted and unique"
        av = a.astype(dtype)
        below[:, e], above[:, e] = av < sv[0], av > sv[-1]
        i[:, e] = np.clip(np.searchsorted(sv, av, side="right") - 1, 0, n_a - 2)   # the last knot <= x
        amb[:, e] = np.any(_mag(av[:, None] - sv[None, :]) <= sb[None, :, e], axis=1)
    cols = np.arange(n_e)[None, :]
    si, sj = s[i, cols], s[i + 1, cols]
    ai, aj = T(a[i]), T(a[i + 1])
    rh = (sj - si).rcp()                                                           # one reciprocal serves both quotients
    f = (ac - si) * rh
    omf = 1.0 - f
    g = lerp(f, omf, ai.v, aj.v)
    sl = (aj - ai) * rh
    A, B = (-sl) * omf, (-sl) * f
    zero = T(np.zeros((n_a, n_e)))
    flat = below | above
    g = Tracked.where(below, T(np.full((n_a, n_e), a[0])), Tracked.where(above, T(np.full((n_a, n_e), a[-1])), g))
    amb |= ~flat & (_mag(g.v - dtype(bc)) <= g.bound()) & (g.v != bc)
    drop = (bc > g.v) | (np.signbit(bc) < np.signbit(g.v))                         # the `max` rule: the partial does not pass
    binds = bc > g.v
    g = Tracked.where(binds | ((g.v == bc) & np.signbit(g.v)), T(np.full((n_a, n_e), bc)), g)
    constrained = binds | (below & (a[0] == bc))            # the limit holds the policy: by `max`, or as the flat end value
    A, B = Tracked.where(flat | drop, zero, A), Tracked.where(flat | drop, zero, B)
    cg = (opr * ac + wz_tr) - g
    assert np.all(cg.v > 0), "negative consumption"
    u = pow_crra(cg, -gamma)
    if diet:
        v = opr * (u * u.sqrt()).scaled(-2.0) if gamma == 2.0 else opr * (-(u * u))
    else:
        v = opr * ((u / cg) * (-gamma))
    Vout = opr * u
    dg = A[..., None] * ds[i, cols] + B[..., None] * ds[i + 1, cols]
    inc_y = zr[..., None] * dw if dtr is None else zr[..., None] * dw + dtr
    dVout = u[..., None] * dr + v[..., None] * ((ac[..., None] * dr + inc_y) - dg)
    return dict(V=Vout, policy=g, dV=dVout, dpolicy=dg, ambiguous=amb, constrained=constrained, below=below, above=above,
                s=s, ds=ds, kc=kc, v=v)


def forward_step(dtype, a, Pi, policy, dpolicy, D_prev, dD_prev):
    """transition_step with the exogenous mixing and the aggregate: policy (n_a, n_e) and dpolicy (n_a, n_e, N) exact; D_prev
    (n_a, n_e) and dD_prev (n_a, n_e, N) exact arrays or Tracked (a compounding bound); N may be 0.
    -> dict of Tracked D (n_a, n_e), dD (n_a, n_e, N), agg (), dagg (N,), total () = sum D; `mass` (n_a, n_e) float64, the unweighted
       mass of the sources that touch a row; `ambiguous` (n_a, n_e), the rows a policy within an ulp of a grid point feeds."""
    T = lambda q: q if isinstance(q, Tracked) else Tracked(np.asarray(q, dtype=dtype))          # noqa: E731
    a, Pi, policy, dpolicy = (np.asarray(q, dtype=np.float64) for q in (a, Pi, policy, dpolicy))
    n_a, n_e = policy.shape
    N = dpolicy.shape[2]
    D, dD = T(D_prev), T(dD_prev)
    hi = np.searchsorted(a, policy, side="left")                  # searchsortedfirst (:52): a[hi - 1] < p <= a[hi], on exact inputs
    low, top = hi == 0, hi >= n_a
    inner = ~(low | top)
    l = np.clip(hi - 1, 0, n_a - 2)
    h = l + 1
    gap = T(a[h]) - T(a[l])
    w = (T(policy) - T(a[l])) / gap                               # (:66); 1 - w afterwards (:69)
    omw = 1.0 - w
    dwt = T(dpolicy) / gap[..., None]
    one_target = np.where(low, 0, n_a - 1)                        # a clamp moves the whole mass, exactly
    col = np.arange(n_e)[None, :] * n_a
    parts, idx = [], []                                            # the scatter's terms, values and partials side by side (n, 1 + N)
    both = lambda t0, t1: Tracked(np.concatenate([t0.v[..., None], t1.v], axis=-1), np.concatenate([t0.e[..., None], t1.e], axis=-1))  # noqa: E731
    clamp = both(D, dD)
    lo_t = both(omw * D, omw[..., None] * dD - dwt * D[..., None])
    hi_t = both(w * D, w[..., None] * dD + dwt * D[..., None])
    parts.append(clamp[~inner]); idx.append((col + one_target)[~inner])
    parts.append(lo_t[inner]); idx.append((col + l)[inner])
    parts.append(hi_t[inner]); idx.append((col + h)[inner])
    terms, idx = Tracked.concat(parts), np.concatenate(idx)
    G, W = n_a * n_e, 1 + N
    flat_idx = (idx[:, None] * W + np.arange(W)[None, :]).ravel()
    mid = terms.reshape(-1).scatter_sum(flat_idx, G * W).reshape(n_e, n_a, W)                  # [e][a][slot]
    # the exogenous mixing: D_new[a, e2] = sum_e mid[a, e] Pi[e, e2]
    new = (mid.reshape(n_e, 1, n_a, W) * T(Pi[:, :, None, None])).sum(axis=0)                  # [e2][a][slot]
    new = Tracked(new.v.transpose(1, 0, 2), new.e.transpose(1, 0, 2))                          # (n_a, n_e, slot)
    Dn, dDn = new[..., 0], new[..., 1:]
    pol = T(policy)
    agg = (pol * Dn).sum()
    dagg = (pol[..., None] * dDn + T(dpolicy) * Dn[..., None]).reshape(G, N).sum(axis=0)
    # the unweighted mass behind a row, and the rows that a nearly-on-the-grid policy feeds
    Dm = _mag(D.v)
    msrc, near = np.zeros(G), np.zeros(G)
    np.add.at(msrc, (col + one_target)[~inner], Dm[~inner])
    np.add.at(msrc, (col + l)[inner], Dm[inner]); np.add.at(msrc, (col + h)[inner], Dm[inner])
    close_lo = inner & (policy - a[l] <= np.spacing(a[l]))
    close_hi = inner & (a[h] - policy <= np.spacing(a[h])) & (policy != a[h])
    for k, m in ((l, close_lo | close_hi), (h, close_lo | close_hi)):
        np.add.at(near, (col + k)[m], 1.0)
    msrc, near = msrc.reshape(n_e, n_a), near.reshape(n_e, n_a)
    touch = (Pi > 0).astype(np.float64)
    return dict(D=Dn, dD=dDn, agg=agg, dagg=dagg, total=Dn.sum(), mass=np.einsum("ea,ef->af", msrc, touch),
                ambiguous=np.einsum("ea,ef->af", near, touch) > 0)
