"""The host side of hank_ss_batch, no GPU: the step-halving rule on a batch of trials, the refusal of
find_ss(batch=True) without the device VFI, the two entries in the ABI table and in the header, and the example's option."""
import re
import subprocess
import sys

import numpy as np
import pytest

from conftest import ROOT


def test_first_acceptable_is_the_sequential_rules_choice():
    from hank_amd.SteadyState import first_acceptable
    inf, nan = np.inf, np.nan
    assert first_acceptable([0.5, 0.4, 0.3], 1.0) == 0                      # the full step is taken when it does not increase the norm
    assert first_acceptable([2.0, 1.5, 0.9, 0.1], 1.0) == 2                 # the first one at or below, not the smallest
    assert first_acceptable([2.0, 1.0], 1.0) == 1                           # equality is accepted (the loop halves only while > z_norm)
    assert first_acceptable([inf, nan, 3.0, 0.99, 0.5, 0.2], 1.0) == 3      # inf and nan entries are skipped
    assert first_acceptable([inf, nan, 3.0, 2.0, 1.5, 1.01], 1.0) is None
    assert first_acceptable([nan] * 6, 1.0) is None and first_acceptable([], 1.0) is None
    assert first_acceptable(np.array([inf, 0.0]), 0.0) == 1


def test_find_ss_batch_needs_the_device_vfi():
    import hank_amd as h
    from hank_amd.SteadyState import SSAssembler, find_ss
    ov = {"T": 9, "dimensions": {"wealth": {"n": 20}, "productivity": {"n": 2}}}
    m = h.build_model_from_yaml(str(ROOT / "examples" / "krusell_smith.yaml"), overrides=ov)
    with pytest.raises(ValueError, match="batch=True needs the device VFI.*vfi='host'"):
        find_ss(m, m.ss_initial, "initial", vfi="host", batch=True)
    asm = SSAssembler(m, m.ss_initial, None, "host")
    with pytest.raises(ValueError, match="device VFI"):
        asm.batch(np.zeros((asm.n_free, 2)))


def test_the_entries_are_in_the_abi_table_and_in_the_header():
    from hank_amd import hip
    header = (ROOT / "include" / "hank_hip.h").read_text()
    for name in ("hank_ss_batch", "hank_last_ss_batch_timings"):
        assert name in hip.ABI_SYMBOLS
        assert re.search(rf"^int {name}\(hank_ctx \*ctx", header, re.M), name
    assert "SteadyState.jl:132-141" in header[header.index("hank_ss_batch  =="):] and "ForwardIteration.jl:436-442" in header[header.index("hank_ss_batch  =="):]


def test_the_example_lists_the_curve():
    r = subprocess.run([sys.executable, str(ROOT / "examples" / "solve_transition.py"), "--help"], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr[-2000:]
    assert "--ss-curve VAR LO HI K" in r.stdout
