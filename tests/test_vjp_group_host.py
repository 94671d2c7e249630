"""hank_vjp_group without a GPU: (1) the map of DESIGN.md section 3j — cotangents on group outputs Y^k_t = sum W_k f_b D_t enter
Sweep A through three point-wise fields q0, q1, q2 (the MASS, POLICY and CONS groups' W_k g[t,k]), Sweep B is untouched, and the
CONS sums reach the inputs directly — stated in numpy on the random records of tests/sweep_refs.py and compared with the dense
transpose of `tangent_map`, where a group is an extra output with f = W f_b, f_c = -sigma W and S from the record. This pins the
formula, not the device. (2) the binding."""
import numpy as np
import pytest

from sweep_refs import _cons, _random_record, cotangent_map, tangent_map

MASS, POLICY, CONS = 0, 1, 2
SIGMA = {MASS: 0.0, POLICY: 1.0, CONS: -1.0}


def _groups_as_extra_outputs(R, W, base):
    """X of tests/sweep_refs.py for K groups: f = W f_b, fc = -sigma_b W, S = (Sa, Sz, S1, Sr) = CONS: sum W D_t (a, z_e, 1), 0"""
    K, P, a, z = W.shape[0], R["P"], R["a"], R["z"]
    f, fc, S = np.zeros((K, P, R["n_a"], R["n_e"])), np.zeros((K, P, R["n_a"], R["n_e"])), np.zeros((K, P, 4))
    for k in range(K):
        for t in range(P):
            fb = {MASS: np.ones_like(W[k]), POLICY: R["pol"][t], CONS: _cons(R, t)}[int(base[k])]
            f[k, t], fc[k, t] = W[k] * fb, -SIGMA[int(base[k])] * W[k]
            if base[k] == CONS:
                WD = W[k] * R["D"][t + 1]
                S[k, t, :3] = [np.sum(WD * a[:, None]), np.sum(WD * z[None, :]), np.sum(WD)]
    return {"f": f, "fc": fc, "S": S}


def group_cotangent_map(R, yb, g, W, base, S):
    """section 3j: yb (2, P) on outputs 0 and 1, g (K, P) on the groups -> (xbar (3, P), pbar (P, n_a, n_e)). Sweep A with
    lam += (yb0 + q1) pol + (yb1 + q2) c + q0 and pbar = D_t ((yb0 + q1) - (yb1 + q2)) + the lottery part; Sweep B as it is
    (cotangent_map's, fed through a record whose outputs 0 and 1 carry nothing); then xbar += sum_k g[k,t] S[k,t]."""
    n_e, P, Pi = R["n_e"], R["P"], R["Pi"]
    cols = np.arange(n_e)[None, :]
    q = np.zeros((3, P) + W.shape[1:])
    for k in range(W.shape[0]):
        q[int(base[k])] += g[k][:, None, None] * W[k][None]
    pbar, lam = np.zeros((P,) + W.shape[1:]), np.zeros(W.shape[1:])
    for t in range(P - 1, -1, -1):
        lam = lam + (yb[0, t] + q[1, t]) * R["pol"][t] + (yb[1, t] + q[2, t]) * _cons(R, t) + q[0, t]
        U = lam @ Pi.T
        lo, w = R["lo"][t], R["w"][t]
        pbar[t] = R["D"][t + 1] * ((yb[0, t] + q[1, t]) - (yb[1, t] + q[2, t])) + R["ig"][t] * R["D"][t] * (U[lo + 1, cols] - U[lo, cols])
        lam = (1 - w) * U[lo, cols] + w * U[lo + 1, cols]
    xbar = _sweep_b(R, pbar)
    for t in range(P):                                           # consumption's direct term (k_adj_out)
        Dt = R["D"][t + 1]
        xbar[:, t] += yb[1, t] * np.array([np.sum(R["a"][:, None] * Dt), np.sum(R["z"][None, :] * Dt), np.sum(Dt)])
    for k in range(W.shape[0]):
        xbar += g[k][None, :] * S[k, :, :3].T
    return xbar, pbar


def _sweep_b(R, pbar):
    """Sweep B of cotangent_map alone (the inputs' cotangents that a policy cotangent sequence carries)"""
    n_a, n_e, P, a, z, Pi = R["n_a"], R["n_e"], R["P"], R["a"], R["z"], R["Pi"]
    cols = np.arange(n_e)[None, :]
    xbar, mu = np.zeros((3, P)), np.zeros((n_a, n_e))
    for t in range(P):
        rho = 1.0 / (1.0 + R["x"][0, t])
        gbar = pbar[t] - R["v"][t] * mu
        xbar[:, t] += [np.sum(mu * (R["u"][t] + R["v"][t] * a[:, None])), np.sum(mu * R["v"][t] * z[None, :]), np.sum(mu * R["v"][t])]
        sbar = np.zeros((n_a, n_e))
        cc = np.broadcast_to(cols, gbar.shape)
        np.add.at(sbar, (R["ib"][t], cc), R["A"][t] * gbar)
        np.add.at(sbar, (R["ib"][t] + 1, cc), R["B"][t] * gbar)
        xbar[:, t] -= rho * np.array([np.sum(sbar * R["s"][t]), np.sum(sbar * z[None, :]), np.sum(sbar)])
        mu = (R["kc"][t] * sbar) @ Pi
    return xbar


@pytest.mark.parametrize("seed", [0, 1, 2])
def test_the_group_cotangent_map_is_the_transpose_of_the_group_tangent_map(seed):
    rng = np.random.default_rng(seed)
    R = _random_record(rng)
    P, K = R["P"], 7
    W = rng.standard_normal((K, R["n_a"], R["n_e"]))
    base = np.arange(K) % 3
    X = _groups_as_extra_outputs(R, W, base)
    NO = 2 + K
    J = np.zeros((NO * P, 3 * P))                                # rows (output, t), columns (input, s)
    for i in range(3):
        for s in range(P):
            dx = np.zeros((3, P)); dx[i, s] = 1.0
            J[:, i * P + s] = tangent_map(R, dx, X)[0].reshape(-1)
    for k in range(K):
        assert np.abs(J[(2 + k) * P:(3 + k) * P]).max() > 1e-3, k
    scale = max(1.0, np.abs(J).max())
    for only in (None, "groups", 2, 3, 4, 2 + K - 1):            # everything; the groups alone; one group alone (a swapped base shows)
        yb = rng.standard_normal((NO, P))
        if only == "groups":
            yb[:2] = 0.0
        elif only is not None:
            yb[np.arange(NO) != only] = 0.0
        xbar, pbar = group_cotangent_map(R, yb[:2], yb[2:], W, base, X["S"])
        want = J.T @ yb.reshape(-1)
        err = np.max(np.abs(xbar.reshape(-1) - want))
        print(f"seed {seed}, cotangents on {only}: max err {err:.3e} at scale {np.abs(want).max():.3e}")
        assert err <= 1e-13 * max(scale, np.abs(want).max())
        # the same statement as extra outputs in Sweep A (sweep_refs.cotangent_map): equal up to the order of the sums
        xb2, pb2 = cotangent_map(R, yb, X)[:2]
        assert np.max(np.abs(xb2 - xbar)) <= 1e-13 * max(scale, np.abs(want).max())
        assert np.max(np.abs(pb2 - pbar)) <= 1e-13 * max(1.0, np.abs(pb2).max())


class _Lib:
    """stands in for the library: records what hank_vjp_group is handed"""
    def __init__(self):
        self.seen = None

    def hank_vjp_group(self, ctx, n_het, agg_bar, grp_bar, M, out, vb, db):
        self.seen = (n_het, agg_bar is not None, M, vb is not None, db is not None)
        return 0


def test_binding_lists_the_entries_and_reshapes_a_single_column(hank):
    from hank_amd import hip
    assert {"hank_vjp_group", "hank_vjp_group_dev"} <= set(hip.ABI_SYMBOLS)
    assert hasattr(hip.HouseholdBlock, "vjp_group") and hasattr(hip.HouseholdBlock, "vjp_group_dev")
    hb = hip.HouseholdBlock.__new__(hip.HouseholdBlock)          # no context: the argument handling alone
    hb.P, hb.n_hh, hb.n_a, hb.n_e, hb.n_groups, hb._ctx, hb._lib = 5, 2, 4, 3, 6, None, _Lib()
    hb._chk = lambda rc: None
    out = hb.vjp_group(np.ones((5, 6)))                          # (P, K): one column
    assert out.shape == (2, 5, 1) and hb._lib.seen == (0, False, 1, False, False)
    out, vb, db = hb.vjp_group(np.ones((5, 6, 3)), agg_bar=np.ones((5, 2, 3)), n_het=2, D_init=True)
    assert out.shape == (2, 5, 3) and vb is None and db.shape == (4, 3, 3) and hb._lib.seen == (2, True, 3, False, True)
    with pytest.raises(ValueError):
        hb.vjp_group(np.ones((5, 7, 3)))                         # K of another set
    with pytest.raises(ValueError):
        hb.vjp_group(np.ones((5, 6, 3)), agg_bar=np.ones((5, 2, 4)), n_het=2)
