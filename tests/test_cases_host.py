"""The owners of tests/cases.py without a GPU: `close`, the suite's only tolerance function, and `raw_block`, which creates a
context under HANK_* variables and restores every one of them."""
import os

import numpy as np
import pytest

from cases import close, raw_block


def test_close_passes_just_under_its_bound_and_fails_just_over_it():
    b = np.array([1.0, -4.0, 2.0])
    bound = 1e-12 + 1e-10 * 4.0
    close(b + np.array([0.0, 0.0, 0.99 * bound]), b)
    with pytest.raises(AssertionError):
        close(b + np.array([0.0, 0.0, 1.01 * bound]), b)
    close(b + 3.9e-6, b, 1e-6, ab=0.0)
    with pytest.raises(AssertionError):
        close(b + 4.1e-6, b, 1e-6, ab=0.0)
    with pytest.raises(AssertionError):                     # no floor on the scale: a zero reference takes the absolute part alone
        close(np.full(3, 1e-11), np.zeros(3))
    close(np.zeros(3), np.zeros(3), ab=0.0)


def test_close_refuses_shapes_that_would_broadcast():
    b = np.linspace(1.0, 2.0, 5)
    with pytest.raises(AssertionError):
        close(b[:, None], b)
    with pytest.raises(AssertionError):
        close(b, b[:, None])
    with pytest.raises(AssertionError):
        close(1.0, np.ones(5))


@pytest.mark.parametrize("side", [0, 1])
def test_close_fails_on_a_nan_on_either_side(side):
    pair = [np.ones(4), np.ones(4)]
    pair[side] = np.array([1.0, np.nan, 1.0, 1.0])
    with pytest.raises(AssertionError):
        close(*pair)


class _Recorder:
    """stands in for the hank module: HouseholdBlock records the HANK_* variables it is constructed under."""

    def __init__(self, fail=False):
        self.fail, self.seen = fail, None

    def HouseholdBlock(self, *args):
        self.seen = {k: v for k, v in os.environ.items() if k.startswith("HANK_")}
        if self.fail:
            raise RuntimeError("refused")
        return args


@pytest.mark.parametrize("fail", [False, True])
def test_raw_block_sets_its_variables_for_the_construction_and_restores_them(monkeypatch, fail):
    monkeypatch.setenv("HANK_SCHEDULE", "launch")           # the operator's: a whole run on one family
    monkeypatch.setenv("HANK_WIDE_R", "4")
    monkeypatch.delenv("HANK_XFAULT", raising=False)
    monkeypatch.delenv("HANK_PRIMAL_MEMO", raising=False)
    hank = _Recorder(fail)
    if fail:
        with pytest.raises(RuntimeError, match="refused"):
            raw_block(hank, (1, 2), "xcd", HANK_XFAULT="placement", HANK_PRIMAL_MEMO=0, HANK_WIDE_R=None)
    else:
        assert raw_block(hank, (1, 2), "xcd", HANK_XFAULT="placement", HANK_PRIMAL_MEMO=0, HANK_WIDE_R=None) == (1, 2)
    assert hank.seen == {"HANK_SCHEDULE": "xcd", "HANK_XFAULT": "placement", "HANK_PRIMAL_MEMO": "0"}
    assert os.environ["HANK_SCHEDULE"] == "launch" and os.environ["HANK_WIDE_R"] == "4"
    assert "HANK_XFAULT" not in os.environ and "HANK_PRIMAL_MEMO" not in os.environ
    hank.fail = False
    raw_block(hank, (), None)                               # None: the default schedule, whatever the operator set
    assert "HANK_SCHEDULE" not in hank.seen and os.environ["HANK_SCHEDULE"] == "launch"
