"""hank_fake_news / hank_fake_news_het on the MI355X, EVERY entry of both exports — F (P, P, n_hh[, n_het]) and Dv (P, n_hh[, n_het])
— against the dense reference of tests/fake_news_refs.py (the CPU oracle's operators at the polished stationary point, pinned by
tests/test_fake_news_ref_host.py 100 to 500 times inside the bound). The older modules (test_gpu_jacobian.py, test_gpu_fake_news_het.py)
look through the Toeplitz recursion at five columns and 1e-8; an entry F[u, j] with u - j > P/2 and j >= 2 reaches none of them.

Tolerance: `cases.close` (rel 1e-10 + abs 1e-12) once per (input, output) slab of F and of Dv, so the scale is that slab's largest
reference entry. The largest ENTRYWISE relative error per slab is printed and not bounded: min |F| / max |F| is 1e-3 to 1e-4.

The context is test_gpu_ss_diff._ctx's with T = P + 1: the polished (V, D) of ss_diff_cases.case as both boundaries, so that the
record is stationary to rounding, and `primal` at the constant path. The shapes, and what each reaches in the eight kernels of
csrc/hank_jacobian.h, are fake_news_refs.SHAPES; every case asserts its claims on fake_news_refs.geometry (tests/test_geom_host.py
holds that arithmetic and the source together). P = 1 (T = 2), a single lag, is covered by tests/test_gpu_short_horizons.py
(test_fake_news_matches_the_dense_reference), against the same reference at the same bound."""
import numpy as np
import pytest

import cases
import fake_news_refs as R
import ss_diff_cases as S

pytestmark = pytest.mark.gpu

_REF = {}


def _ref(name, P):
    """the dense (F, Dv) of every output of the family, once per session and shape"""
    if (name, P) not in _REF:
        c = S.case(name)
        _REF[name, P] = R.dense_fake_news(c, P, c["n_het"])
    return _REF[name, P]


def _ctx(hank, name, P, schedule=None):
    c = S.case(name)
    assert len(c["args"]) == 8 and c["args"][6] == S.T_SHORT
    hb = cases.raw_block(hank, c["args"][:6] + (P + 1,) + c["args"][7:], schedule)
    hb.set_boundary(c["V"], c["D"])
    hb.primal(R.constant_path(c, P))
    assert hb.P == P and hb.G == c["orc"].G and hb.n_hh == len(c["x"])
    return hb, c


def _slabs(got, ref, what):
    """`close` per (input, output) slab; got, ref (..., n_hh, n_het). Prints the largest entrywise relative error of each slab."""
    assert got.shape == ref.shape, (what, got.shape, ref.shape)
    for o in range(ref.shape[-1]):
        for k in range(ref.shape[-2]):
            g, r = got[..., k, o], ref[..., k, o]
            nz = r != 0.0
            assert nz.any(), (what, k, o)
            entry = np.max(np.abs(g - r)[nz] / np.abs(r)[nz])
            print(f"{what} input {k} output {o}: entrywise relative error {entry:.3e} at most (min |ref| / max |ref| = {np.abs(r)[nz].min() / np.abs(r).max():.1e})")
            cases.close(g, r, what=f"{what} input {k} output {o}")


def _parity(hb, c, name, P, tag=""):
    """fake_news_het(n) for every n the family allows, and fake_news(), against the dense reference over the whole arrays
    -> (F, Dv) of the widest call"""
    Fr, Dvr = _ref(name, P)
    for n in range(1, c["n_het"] + 1):
        F, Dv = hb.fake_news_het(n)
        _slabs(F, Fr[..., :n], f"{name} P={P}{tag} fake_news_het({n}) F")
        _slabs(Dv, Dvr[..., :n], f"{name} P={P}{tag} fake_news_het({n}) Dv")
    F0, Dv0 = hb.fake_news()
    _slabs(F0[..., None], Fr[..., :1], f"{name} P={P}{tag} fake_news() F")
    _slabs(Dv0[..., None], Dvr[..., :1], f"{name} P={P}{tag} fake_news() Dv")
    return F, Dv


@pytest.mark.parametrize("name,P", sorted(R.SHAPES))
def test_every_entry_matches_the_dense_reference(hank, oracle_mod, name, P):
    hb, c = _ctx(hank, name, P)
    try:
        g = R.check_shape(name, P, hb.G, hb.n_hh, c["n_het"])
        print(f"{name} P={P}: {g}")
        Pi = np.asarray(c["orc"].Pi)
        if Pi.shape[0] >= 3:
            # k_fn_impulse and fn_expect_at both index Pi (Pi[e + ne * e2]); a symmetric chain — every two-state one of these
            # economies is — cannot see it transposed, so the economies with three states and more must not be symmetric
            assert not np.allclose(Pi, Pi.T), name
        if name == "ks40x16":
            assert Pi.shape[0] == 16          # mid[16] of k_fn_impulse full
        _parity(hb, c, name, P)
    finally:
        hb.close()


@pytest.mark.parametrize("name,P", [("hank30x3", 33), ("clamp", 12)])
def test_both_schedules_match_the_reference(hank, oracle_mod, name, P):
    """the default schedule's record and tangent sweep (the persistent family's) and HANK_SCHEDULE=launch's, each against the dense
    reference. F is the same bits under both and that is asserted: the policy record and the backward tangent sweep are bit-equal
    across the families (pol, dpol), and the impulse weighs with ig D_0, D_0 being the boundary as given. Dv is NOT the same bits
    (measured: 89 of 396 entries on hank30x3, 7 of 72 on clamp, apart by 8.9e-16 at most on a scale of 2.4 and 5.2): its weights
    are D_1 = Dseq[G + pt], the post-transition distribution the primal's forward sweep computed, whose last bits differ between
    the two families' forward sweeps (dist_seq: 1329 of 2970 entries, by 1.7e-16 at most; the suite compares the families'
    aggregates under 1e-12, never by bits). Its distance is printed."""
    out = {}
    for sched in (None, "launch"):
        hb, c = _ctx(hank, name, P, schedule=sched)
        try:
            out[sched] = _parity(hb, c, name, P, tag=f" schedule {sched or 'default'}")
        finally:
            hb.close()
    (F, Dv), (Fl, Dvl) = out[None], out["launch"]
    print(f"{name} P={P}: default schedule against launch: F differs in {np.count_nonzero(F != Fl)} of {F.size} entries; "
          f"Dv in {np.count_nonzero(Dv != Dvl)} of {Dv.size}, apart by {np.max(np.abs(Dv - Dvl)):.3e} at most on a scale of {np.abs(Dvl).max():.3e}")
    assert np.array_equal(F, Fl)


STATE = ("hank30x3", 33)


def test_calls_repeat_their_bits_and_a_caller_s_batch_leaves_them_alone(hank, oracle_mod):
    """the same call twice returns the same bits; a hank_jvp of width 5 between two hank_fake_news_het calls — the tangent
    workspace of width n_hh is shared with callers' batches of that width, and a wider batch owns the sweep's record of who is
    current — does not change the second call's bits, nor does a batch of width n_hh itself"""
    name, P = STATE
    hb, c = _ctx(hank, name, P)
    try:
        n = c["n_het"]
        F0, Dv0 = hb.fake_news_het(n)
        F1, Dv1 = hb.fake_news_het(n)
        assert np.array_equal(F0, F1) and np.array_equal(Dv0, Dv1)
        rng = np.random.default_rng(5)
        for width in (5, hb.n_hh):
            dagg = hb.jvp(rng.standard_normal((hb.n_hh, P, width)) * 1e-2)
            assert np.all(np.isfinite(dagg))
            F2, Dv2 = hb.fake_news_het(n)
            assert np.array_equal(F0, F2) and np.array_equal(Dv0, Dv2), width
        Fa, Dva = hb.fake_news()
        assert np.array_equal(Fa, F0[..., 0]) and np.array_equal(Dva, Dv0[..., 0])
    finally:
        hb.close()
