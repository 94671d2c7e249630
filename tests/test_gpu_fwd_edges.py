"""The forward sweeps — the per-period launches (k_dist_step, k_tan_fwd / k_fused_fwd), the persistent family (k_xunits_fwd,
k_xfwd, k_xstat) and the on-chip wide family (k_wide_fwd) — on the data-dependent edges of the raw-grid economies of
tests/cases.py, section 3, against the CPU oracle (oracle/hank_oracle.c) at rel 1e-10 + abs 1e-12 and against the launches at
1e-12 and bit equality. The calibrated grids of the other GPU modules clamp a row or two; here (measured on the oracle's policy
by tests/test_vjp_host.py: cases.forward_edges)

  deep-prefix  the clamped prefix of column 0 runs over members 0..3 of the persistent family (`clo > r0` for a member other than
               0) and into wave 1 of the wide family's workgroup (red[1]); a target row with 76..191 sources (a work unit of more
               than 64 lanes loops)
  swing        a period with every column clamped (anyopen == 0), then five without any clamp — the first after a clamped period
               (vnz set, anyclo clear: all virtual mass re-enters through row 0's lottery), the others after unclamped ones — and
               a clamp that returns; 121-122 sources clamped at the top of every column
  collapse     whole columns clamped (clo == n_a): all mass on row 0, the aggregate exactly 0 for two periods, then spread again

next to the three economies of the transposed sweeps (dense-bottom, short-top, both). Every context must report its own family
for every sweep, no fallback and its schedule: a unit overflow or a fallback would hide a persistent-sweep bug behind the
launches' numbers."""
import numpy as np
import pytest

from cases import (FAMILY, FWD_ECONOMIES, against_oracle_and_launches, close, oracle_dist_seq, raw_block, raw_economy)

pytestmark = pytest.mark.gpu

NS = (1, 5, 12, 40)          # with 8 groups: D = 1, 1, 2, and two passes (32 at D = 4, then 8)
NWIDE = 96                   # the default schedule sends it to the on-chip wide sweeps; the oracle covers its first 40 columns
CONTEXTS = [("launch", {}), ("xcd", {}), ("xcd", {"HANK_RECORD_DIET": 0}), ("wide", {"HANK_WIDE_R": 2}), ("wide", {"HANK_WIDE_R": 4}), (None, {})]
WIDTHS = {"launch": NS + (NWIDE,), "xcd": NS, "wide": NS, None: NS + (NWIDE,)}
THREE = ("launch", "xcd", "wide")


def _shape(name):
    ec = raw_economy(name)
    return ec["args"], ec["V"], ec["D"], ec["x"], ec["orc"]


@pytest.mark.parametrize("name", FWD_ECONOMIES)
def test_both_entry_points_of_every_family(hank, name):
    """aggregates, policy, partials and the distribution sequence of both entry points at N = 1, 5, 12, 40 (and 96 under the
    launches and the default schedule) in every context of CONTEXTS, each on its own schedule and without a fallback."""
    for sched, env, st, info in against_oracle_and_launches(hank, _shape(name), CONTEXTS, WIDTHS):
        # (these grids fit the persistent sweeps: a forced `wide` keeps them for the primal, schedule 2 like the default)
        assert st["schedule"] == {"launch": 0, "xcd": 1}.get(sched, 2) and st["fallbacks"] == 0, (name, sched, env, st)


_REF = {}


def _oracle_tangents(name, N, seed=31):
    """y (2, P, N) and the oracle's policy, partials, D_t and dD_t (P, n_a, n_e[, N]) of an economy: the household block, then
    the dual forward iteration on its policy sequence (once per session and width)."""
    if (name, N) not in _REF:
        from oracle.oracle import pad_N
        ec = raw_economy(name)
        orc, x = ec["orc"], ec["x"]
        y = np.random.default_rng(seed).standard_normal((2, x.shape[1], N))
        _, _, pol, dpol = orc.block(x, y, ec["V"], ec["D"])
        dD = []
        for c0 in range(0, N, 32):
            n = min(N, c0 + 32) - c0
            Nc = pad_N(n)
            pd = np.zeros(pol.shape + (1 + Nc,))
            pd[..., 0] = pol
            pd[..., 1:1 + n] = dpol[..., c0:c0 + n]
            dD.append(orc.forward_iteration(pd, ec["D"], Nc, return_D=True)[1][..., 1:1 + n])
        _REF[name, N] = (y, pol, dpol, oracle_dist_seq(orc, pol, ec["D"]), np.concatenate(dD, axis=-1))
    return _REF[name, N]


@pytest.mark.parametrize("sched", THREE)
@pytest.mark.parametrize("name", ["deep-prefix", "swing"])
def test_grid_aggregates(hank, name, sched):
    """hank_get_grid_aggregates after a tangent sweep of either entry point: sum a D_t and sum a dD_t of the oracle's (dual) forward
    iteration. The mass point carries a = grid[0] = 0 on these grids: what leaves it, or fails to, shows in the rows above."""
    ec = raw_economy(name)
    a = ec["grid"]
    hb = raw_block(hank, ec["args"], sched)
    hb.set_boundary(ec["V"], ec["D"])
    for entry, N in (("dual", 5), ("tan", 12)):
        y, _, _, D, dD = _oracle_tangents(name, N)
        if entry == "dual":
            hb.primal_jvp(ec["x"], y)
        else:
            hb.primal(ec["x"] * 1.01); hb.primal(ec["x"]); hb.jvp(y)
        assert hb.info()["last_tangent_family_name"] == FAMILY[sched]
        ad, dad = hb.grid_aggregates(N)
        what = f"{name} {sched} {entry} N={N}"
        close(ad, np.einsum("i,tie->t", a, D), what=what + " sum a D")
        close(dad, np.einsum("i,tien->tn", a, dD), what=what + " sum a dD")
    assert hb.stats()["fallbacks"] == 0
    hb.close()


_HET = {}


def _oracle_het(name, N, seed=37):
    if (name, N) not in _HET:
        ec = raw_economy(name)
        y = np.random.default_rng(seed).standard_normal((2, ec["x"].shape[1], N))
        parts = [ec["orc"].het_outputs(ec["x"], y[:, :, c0:c0 + 32], ec["V"], ec["D"], 3, ec["args"][4]) for c0 in range(0, N, 32)]
        _HET[name, N] = (y, parts[0][0], np.concatenate([p[1] for p in parts], axis=2))
    return _HET[name, N]


@pytest.mark.parametrize("sched", THREE)
@pytest.mark.parametrize("name", ["deep-prefix", "swing", "collapse"])
def test_nonaffine_outputs(hank, name, sched):
    """savings, consumption and Value = (1+r) c^-γ (pinned by the clamp on the prefix's rows; 1 + r >= 0.41 on these paths) after
    a Dual pass (N = 5) and after hank_primal + hank_jvp (N = 40), against Oracle.het_outputs."""
    ec = raw_economy(name)
    hb = raw_block(hank, ec["args"], sched)
    hb.set_boundary(ec["V"], ec["D"])
    hb.set_het_outputs(3)
    for entry, N in (("dual", 5), ("tan", 40)):
        y, oagg, odagg = _oracle_het(name, N)
        if entry == "dual":
            hb.primal_jvp(ec["x"], y)
        else:
            hb.primal(ec["x"] * 1.01); hb.primal(ec["x"]); hb.jvp(y)
        assert hb.info()["last_tangent_family_name"] == FAMILY[sched]
        agg, dagg = hb.het_outputs(3, y)
        for j in range(3):
            what = f"{name} {sched} {entry} N={N} output {j}"
            close(agg[:, j], oagg[j], what=what)
            close(dagg[:, j, :], odagg[j], what=what + " partials")
    assert hb.stats()["fallbacks"] == 0
    hb.close()


@pytest.mark.parametrize("sched", ["launch", "xcd"])
@pytest.mark.parametrize("name,t", [("swing", 1), ("deep-prefix", 0)])
def test_power_method_steps(hank, name, t, sched):
    """hank_stationary_dist (k_dist_iter; k_xstat) with tol = 0: exactly 60 steps from a uniform D, checked every 10, on the oracle's
    period-1 policy of `swing` (every column clamped) and period-0 policy of `deep-prefix` (a prefix over three members), against 60
    applications of the oracle's transition_step."""
    ec = raw_economy(name)
    orc = ec["orc"]
    pol = orc.block(ec["x"], None, ec["V"], ec["D"])[2][t]
    key = (name, "power")
    if key not in _REF:
        D = ec["D"].reshape(pol.shape, order="F")
        for _ in range(60):
            D = orc.transition_step(pol, D, 1)[..., 0]
        _REF[key] = D
    hb = raw_block(hank, ec["args"], sched)
    D_dev, steps = hb.stationary_dist(pol, tol=0.0, max_iter=60, check_every=10)
    st = hb.stats()
    hb.close()
    assert steps == 60 and st["fallbacks"] == 0 and st["schedule"] == (0 if sched == "launch" else 1), (steps, st)
    close(D_dev.reshape(pol.shape, order="F"), _REF[key], what=f"{name} period {t} {sched} D after 60 steps")
