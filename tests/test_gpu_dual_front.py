"""The front of the one-pass persistent Dual pass (k_xdual_front + k_xunits_pack in hank_xsweep.h) against the launches it stands for
(k_lottery_lq + k_xunits_fwd), one library being its own A/B through HANK_XDUAL_FRONT=0|1 (read at hank_create).

The lean front writes only what k_xfwd<D, true, ., true> reads — the packed record lq, clo and the work units — and leaves lo, lw, ig
and start to k_lottery, which the host runs before the first reader (ensure_lottery). So, on the shapes of tests/test_gpu_xfwd_lq.py
(n_a = 63, 64, 130: one, two and three members, one short; n_e = 2, 11; T = 6; N = 17, 32; the six raw-grid economies with both
clamps, virtual rows that carry mass, units of more than 64 sources and a mass point that vanishes mid-path), under the forced
persistent schedule:

  identity   the same hank_primal_jvp in both contexts: agg, dagg, the work units and their src words (hank_get_forward_units, a
             member's unused slots masked by its count), and lq, iga, lo, lw, ig (hank_get_lottery_record — through the gate) are
             byte-identical
  readers    with HANK_XDUAL_FRONT_POISON=1 the lean front fills what it leaves unwritten (lw, ig NaN; lo, start 0): hank_jvp, hank_vjp,
             hank_jvp_het with Value (and UCE, one-asset HANK), hank_fake_news and hank_get_dist_seq, each directly after a lean Dual
             pass, return the bytes they return after HANK_XDUAL_FRONT=0 — a reader that skipped the gate would compute from the poison
  overflow   a policy whose walk needs more units than the budget (dev knob HANK_XUCAP=3 on the deep-clamp economy of
             tests/test_gpu_fallback.py) fails with the same code and message and counts the same fallback"""
import numpy as np
import pytest

import cases
from cases import FAMILY, FWD_ECONOMIES, block, model_args, raw_block, raw_economy
from conftest import ks_paths, ks_setup

pytestmark = pytest.mark.gpu
T = 6
NS = (17, 32)


def _bytes(a):
    return np.ascontiguousarray(a).view(np.uint8)


def _same(a, b, what):
    assert a.shape == b.shape and a.dtype == b.dtype and np.array_equal(_bytes(a), _bytes(b)), what


def _ctx(hank, args, V, D, front, poison=None, **env):
    hb = raw_block(hank, args, "xcd", HANK_XDUAL_FRONT=front, HANK_XDUAL_FRONT_POISON=poison, **env)
    hb.set_boundary(V, D)
    return hb


def _units(hb):
    """(src, units with every slot behind a member's count zeroed)"""
    src, units = hb.forward_units()
    cnt = (src >> 18) & 0x7f
    units = np.where((np.arange(64)[None, None, :] < cnt[:, :, None])[..., None], units, 0)
    return src, units


def _identity(hank, args, V, D, x, what):
    n_hh, P = x.shape
    y = np.random.default_rng(29).standard_normal((n_hh, P, max(NS)))
    got = {}
    for front in (0, 1):
        hb = _ctx(hank, args, V, D, front)
        for N in NS:
            hb.primal(x * 1.01)
            agg, dagg = hb.primal_jvp(x, np.ascontiguousarray(y[:, :, :N]))
            info = hb.info()
            src, units = _units(hb)
            rec = hb.lottery_record()
            got[front, N] = dict(agg=agg, dagg=dagg, src=src, units=units, lq=rec["lq"], iga=rec["iga"], lo=rec["lo"], lw=rec["lw"], ig=rec["ig"])
            assert info["last_tangent_family_name"] == FAMILY["xcd"], (what, front, N, info)
        st = hb.stats()
        assert st["schedule"] == 1 and st["fallbacks"] == 0, (what, front, st)
        hb.close()
    for N in NS:
        assert np.any((got[0, N]["src"] >> 18) >= 1), (what, "no member has a unit")      # (a member all of whose sources are clamped has none: collapse, swing)
        for k, v in got[0, N].items():
            _same(got[1, N][k], v, (what, N, k))


@pytest.mark.parametrize("n_a", (63, 64, 130))
@pytest.mark.parametrize("n_e", (2, 11))
def test_calibrated_shapes(hank, n_e, n_a):
    m, V, D, x, _ = cases.shape(n_a, n_e, T)
    _identity(hank, model_args(m), V, D, x, (n_a, n_e))


@pytest.mark.parametrize("name", FWD_ECONOMIES)
def test_raw_grid_economies(hank, name):
    ec = raw_economy(name)
    _identity(hank, ec["args"], ec["V"], ec["D"], ec["x"], name)


def _readers(n_hh, P, n_het):
    """the readers of the record behind a Dual pass, each a function of the context -> an array"""
    rng = np.random.default_rng(31)
    y2, yb, ybh = rng.standard_normal((n_hh, P, 5)), rng.standard_normal((P, 2, 4)), rng.standard_normal((P, n_het, 3))
    return {
        "hank_jvp": lambda hb: hb.jvp(y2),
        "hank_vjp": lambda hb: hb.vjp(yb, 2),
        "hank_jvp_het": lambda hb: hb.jvp_het(y2, n_het=n_het),
        "hank_vjp_het": lambda hb: hb.vjp_het(ybh, n_het),
        "hank_get_dist_seq": lambda hb: hb.dist_seq(),
        "hank_get_lottery_record": lambda hb: np.concatenate([hb.lottery_record()[k].astype(np.float64).ravel() for k in ("lo", "lw", "ig")]),
    }


def _poisoned_readers(hank, args, V, D, x, n_het, what):
    n_hh, P = x.shape
    y = np.random.default_rng(29).standard_normal((n_hh, P, 32))
    readers = _readers(n_hh, P, n_het)
    got = {}
    for front, poison in ((0, None), (1, 1)):
        hb = _ctx(hank, args, V, D, front, poison)
        hb.set_het_outputs(n_het)
        for name, read in readers.items():      # each reader directly behind a Dual pass of its own: every gate is met with the record unmade
            hb.primal(x * 1.01)
            hb.primal_jvp(x, y)
            got[front, name] = read(hb)
        assert hb.stats()["fallbacks"] == 0, (what, front)
        hb.close()
    for name in readers:
        assert np.all(np.isfinite(got[0, name])), (what, name)
        _same(got[1, name], got[0, name], (what, name))


@pytest.mark.parametrize("name", ("calibrated-130x3", "deep-prefix", "swing"))
def test_readers_behind_a_lean_pass_see_the_lottery(hank, name):
    if name == "calibrated-130x3":
        m, V, D, x, _ = cases.shape(130, 3, T)
        _poisoned_readers(hank, model_args(m), V, D, x, 3, name)
    else:
        ec = raw_economy(name)
        _poisoned_readers(hank, ec["args"], ec["V"], ec["D"], ec["x"], 3, name)


def test_readers_with_uce_one_asset_hank(hank):
    m, ss = cases.hank_economy(80, 3, 40)
    _poisoned_readers(hank, model_args(m), ss.value, ss.D, cases.hank_x(ss, m.compspec.T - 1), 4, "one-asset HANK 80x3")


def test_fake_news_behind_a_lean_pass(hank):
    """hank_fake_news at a stationary record that a lean Dual pass wrote (the constant steady-state path, the steady state as both boundaries)"""
    m, ss, _ = ks_setup(130, 3, 20)
    x = np.ascontiguousarray(ks_paths(m, ss, "x1", 0.0)[0][2:4])
    assert np.all(x == x[:, :1])
    y = np.random.default_rng(3).standard_normal((2, x.shape[1], 32))
    got = {}
    for front, poison in ((0, None), (1, 1)):
        hb = _ctx(hank, model_args(m), ss.value, ss.D, front, poison)
        hb.primal_jvp(x, y)
        got[front] = hb.fake_news()
        hb.close()
    for a, b in zip(got[1], got[0]):
        assert np.all(np.isfinite(b))
        _same(a, b, "hank_fake_news")


def test_overflow_fails_as_before(hank, monkeypatch):
    m, ss, _ = ks_setup(130, 3, 20)
    x, _ = ks_paths(m, ss, "x1", 0.05)
    y = np.random.default_rng(2).standard_normal((2, 19, 5))
    monkeypatch.setenv("HANK_XUCAP", "3")
    seen = {}
    for front in (0, 1):
        monkeypatch.setenv("HANK_XDUAL_FRONT", str(front))
        hb = block(hank, m, "xcd")                  # a forced schedule fails loudly
        hb.set_boundary(ss.value, ss.D)
        with pytest.raises(hank.HankHIPError, match="work units") as ei:
            hb.primal_jvp(x[2:4], y)
        forced = (ei.value.code, str(ei.value), hb.stats()["fallbacks"])
        hb.close()
        hb = block(hank, m, None)                   # the default schedule returns the launches' numbers and counts the fallback
        hb.set_boundary(ss.value, ss.D)
        a, d = hb.primal_jvp(x[2:4], y)
        st = hb.stats()
        seen[front] = (forced, a, d, st["fallbacks"], st["schedule"])
        hb.close()
    assert seen[0][0][0] == hank.hip.HANK_ERR_SWEEP and seen[1][0] == seen[0][0], (seen[0][0], seen[1][0])
    _same(seen[1][1], seen[0][1], "agg")
    _same(seen[1][2], seen[0][2], "dagg")
    assert seen[1][3:] == seen[0][3:] == (1, 0), (seen[0][3:], seen[1][3:])
