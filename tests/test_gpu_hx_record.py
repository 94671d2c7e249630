"""The record of the outputs that are not affine in the policy (Value, UCE: f, f_c and the direction-independent sums S of
k_hx_record) has ONE owner in the context, held at the family's count SX of extra outputs and built by
whichever product asks first at a primal record: hank_get_het_outputs (the tangent side) or hank_vjp_het (the transposed side).
(a) a call with fewer extra outputs than the record holds (NX = 1 against SX = 2) reads it with the record's stride; (b) the bits do
not depend on who built it, nor on whether it was built or reused; (c) a new primal drops it for both readers and a new boundary
leaves neither anything to read; (d) the device-pointer forms. The economy is the smallest with SX = 2, the sticky-wage one-asset
HANK 80x3, T = 40 (Krusell-Smith 130x3 with SX = 1 in (d)), recorded by the launches; N = 3 directions and M = 5 cotangent columns,
both odd. Everything is compared bit for bit except hank_vjp_het against the CPU oracle's Jacobian, transposed (cases.close: rel
1e-10 + abs 1e-12 on the largest entry of the reference, the tolerance of tests/test_gpu_vjp_het.py)."""
import numpy as np
import pytest

import cases

pytestmark = pytest.mark.gpu

N, M = 3, 5
_CASE = {}


def _wages():
    """the economy, its inputs x, another path x2, N directions y and M cotangent columns yb — made once, never written to"""
    if "wages" not in _CASE:
        m, ss = cases.hank_economy(80, 3, 40, "one_asset_hank_wages.yaml")
        P = m.compspec.T - 1
        x = cases.hank_x(ss, P)
        rng = np.random.default_rng(7)
        _CASE["wages"] = (m, ss, x, np.ascontiguousarray(x * np.array([[1.1], [0.99], [1.0]])), rng.standard_normal((3, P, N)), rng.standard_normal((P, 4, M)))
    return _CASE["wages"]


def _fresh(hank, m, ss, n_het, x):
    hb = cases.block(hank, m, "launch")
    hb.set_boundary(ss.value, ss.D)
    hb.set_het_outputs(n_het)
    hb.primal(x)
    return hb


def _same(a, b, what):
    assert a.shape == b.shape and np.array_equal(a, b), what


def _same_het(a, b, what):
    _same(a[0], b[0], f"{what}: agg")
    _same(a[1], b[1], f"{what}: dagg")


# ---- (a) the stride ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("first", [3, 4])
def test_one_extra_output_reads_a_record_of_two(hank, oracle_mod, first):
    m, ss, x, _, y, yb = _wages()
    P = x.shape[1]
    hb = _fresh(hank, m, ss, 4, x)
    try:
        hb.jvp(y)
        got = {n_het: hb.het_outputs(n_het, y) for n_het in (first, 7 - first)}
        assert got[3][0].shape == (P, 3) and got[3][1].shape == (P, 3, N) and got[4][1].shape == (P, 4, N)
        _same_het(got[3], (got[4][0][:, :3], got[4][1][:, :3, :]), f"n_het = 3 against 4, {first} asked first")
        assert np.abs(got[4][0][:, 2]).min() > 0 and np.abs(got[4][1][:, 2:, :]).max() > 1e-3      # (nothing compares zeros)
        # the NX = 1 graph of Sweep A on the same two-output record: the oracle's Jacobian of three outputs, transposed
        J = cases.jacobian_het("wages", cases.oracle_of(m), ss.value, ss.D, x, 4, m.params.γ)[:3]      # (the reference of test_gpu_vjp_het.py)
        yb3 = np.ascontiguousarray(yb[:, :3, :])
        cases.close(hb.vjp_het(yb3, 3), cases.jt(J, yb3), what="vjp_het, n_het = 3 on a record of two extra outputs")
    finally:
        hb.close()


# ---- (b) whoever builds it first, (c) a stale record ------------------------------------------------------------------------
def test_the_record_is_the_same_whoever_builds_it_and_goes_with_the_primal(hank, oracle_mod):
    from hank_amd.hip import HANK_ERR_NOT_READY
    m, ss, x, x2, y, yb = _wages()
    A = _fresh(hank, m, ss, 4, x)
    B = _fresh(hank, m, ss, 4, x)
    C = _fresh(hank, m, ss, 4, x2)
    try:
        # A: the tangent side builds the record, the transposed side reuses it, the tangent side reuses it
        dagg_a = A.jvp(y)
        het_a = A.het_outputs(4, y)
        xb_a, pb_a = A.vjp_het(yb, 4), A.policy_cotangent_seq(M)
        _same_het(A.het_outputs(4, y), het_a, "A: het_outputs at a record it built against the record reused")
        # B: the transposed side builds it
        xb_b, pb_b = B.vjp_het(yb, 4), B.policy_cotangent_seq(M)
        dagg_b = B.jvp(y)
        het_b = B.het_outputs(4, y)
        _same(dagg_b, dagg_a, "jvp")
        _same_het(het_b, het_a, "het_outputs: built by hank_vjp_het against built by hank_get_het_outputs")
        _same(xb_b, xb_a, "vjp_het: built by itself against built by hank_get_het_outputs")
        _same(pb_b, pb_a, "policy_cotangent_seq")
        assert np.abs(xb_a).max() > 1e-3 and np.abs(pb_a).max() > 0
        # (c) another primal on A: both readers see the new record, as a context that only ever saw x2 does
        A.primal(x2)
        dagg_a2 = A.jvp(y)
        het_a2, xb_a2 = A.het_outputs(4, y), A.vjp_het(yb, 4)
        dagg_c = C.jvp(y)
        het_c, xb_c = C.het_outputs(4, y), C.vjp_het(yb, 4)
        _same(dagg_a2, dagg_c, "jvp after a primal at another path")
        _same_het(het_a2, het_c, "het_outputs after a primal at another path")
        _same(xb_a2, xb_c, "vjp_het after a primal at another path")
        assert np.abs(het_a2[0][:, 2:] - het_a[0][:, 2:]).max() > 1e-6 * np.abs(het_a[0][:, 2:]).max()      # (x2 is another record)
        assert np.abs(xb_a2 - xb_a).max() > 1e-6 * np.abs(xb_a).max()
        # a new boundary: no record, nothing to read
        A.set_boundary(ss.value * 1.0001, ss.D)
        for call in (lambda: A.het_outputs(4, y), lambda: A.het_outputs(4), lambda: A.vjp_het(yb, 4)):
            with pytest.raises(hank.HankHIPError) as e:
                call()
            assert e.value.code == HANK_ERR_NOT_READY
    finally:
        A.close()
        B.close()
        C.close()


# ---- (d) the device-pointer forms -------------------------------------------------------------------------------------------
def test_device_forms_on_a_record_the_transposed_side_built(hank, oracle_mod):
    import torch
    m, ss, x, _ = cases.economy("ks", 2.0)      # Krusell-Smith 130x3, T = 40: SX = 1
    P = x.shape[1]
    rng = np.random.default_rng(8)
    y, yb = rng.standard_normal((2, P, N)), rng.standard_normal((P, 3, M))
    H = _fresh(hank, m, ss, 3, x)
    D = _fresh(hank, m, ss, 3, x)
    try:
        H.jvp(y)
        xb, (agg, dagg) = H.vjp_het(yb, 3), H.het_outputs(3, y)
        dev = torch.device("cuda", 0)
        up = lambda a: torch.from_numpy(np.asfortranarray(a).reshape(-1, order="F").copy()).to(dev)
        d_y, d_yb = up(y), up(yb)
        d_xb, d_a, d_d = (torch.empty(n, dtype=torch.float64, device=dev) for n in (2 * P * M, 3 * P, 3 * P * N))
        torch.cuda.synchronize()
        D.jvp(y)
        D.vjp_het_dev(3, d_yb.data_ptr(), M, d_xb.data_ptr())
        D.het_outputs_dev(3, d_y.data_ptr(), N, d_a.data_ptr(), d_d.data_ptr())
        D.sync()
        _same(d_xb.cpu().numpy().reshape((2, P, M), order="F"), xb, "vjp_het_dev")
        _same(d_a.cpu().numpy().reshape((P, 3), order="F"), agg, "het_outputs_dev: agg")
        _same(d_d.cpu().numpy().reshape((P, 3, N), order="F"), dagg, "het_outputs_dev: dagg")
        assert np.abs(agg[:, 2]).min() > 0 and np.abs(dagg[:, 2, :]).max() > 1e-3
    finally:
        H.close()
        D.close()
