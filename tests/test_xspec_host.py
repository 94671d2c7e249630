"""The Dual pass's backward sweep has instances compiled for the model's constants (k_xdual_back<D, 768, NE, CRRA>, hank_xsweep.h).
x_spec (hank_xspec.h) is the ONE rule that chooses among them, and x_spec_mode reads the dev knob HANK_XSPEC that switches each half
off: plain integers in a header without device code, compiled alone by the host compiler here, no GPU and no library."""
import shutil
import subprocess
from pathlib import Path

import pytest

CSRC = Path(__file__).resolve().parent.parent / "julia-newtonraphsonhank_amd" / "csrc"
MAIN = """#include "hank_xspec.h"
#include <cstdio>
#include <cstdlib>
#include <cstring>
int main(int argc, char **argv) {      // per question: HANK_XSPEC ("-" = unset), n_e, gamma, diet; one answer "NE CRRA" per line
    for (int i = 1; i + 3 < argc; i += 4) {
        const int mode = hank::x_spec_mode(strcmp(argv[i], "-") == 0 ? nullptr : argv[i]);
        const hank::XSpec s = hank::x_spec(mode, atoi(argv[i + 1]), atof(argv[i + 2]), atoi(argv[i + 3]));
        printf("%d %d\\n", s.ne, s.crra);
    }
    return 0;
}
"""


@pytest.fixture(scope="module")
def spec(tmp_path_factory):
    """hank_xspec.h compiled ALONE by the host compiler into a program that answers."""
    cxx = next((c for c in (shutil.which("c++"), shutil.which("g++"), shutil.which("clang++"), "/opt/rocm/lib/llvm/bin/clang++") if c and Path(c).exists()), None)
    assert cxx, "no host C++ compiler"
    d = tmp_path_factory.mktemp("xspec")
    (d / "main.cpp").write_text(MAIN)
    subprocess.run([cxx, "-std=c++17", "-O1", "-Wall", "-Werror", "-I", str(CSRC), "-o", str(d / "xspec"), str(d / "main.cpp")], check=True, capture_output=True, timeout=120)

    def ask(n_e, gamma, diet, knob=None):
        out = subprocess.run([str(d / "xspec"), "-" if knob is None else knob, str(n_e), repr(float(gamma)), str(diet)], check=True, capture_output=True, text=True, timeout=30).stdout.split()
        assert len(out) == 2, out
        return int(out[0]), int(out[1])
    return ask


def test_ne_is_compiled_in_for_the_listed_grids_only(spec):
    for n_e in range(1, 17):
        assert spec(n_e, 2.0, 1, "1") == ((n_e if n_e in (4, 7, 11) else 0), 1), n_e
        assert spec(n_e, 2.0, 1) == (0, 1), n_e            # unset: the NE half is off (it measured no gain of its own)
    assert spec(0, 2.0, 1, "1")[0] == 0 and spec(44, 2.0, 1, "1")[0] == 0 and spec(-4, 2.0, 1, "1")[0] == 0


def test_crra_needs_gamma_two_and_the_record_diet(spec):
    assert spec(11, 2.0, 1, "1") == (11, 1)
    assert spec(11, 2.0, 0, "1") == (11, 0)                # HANK_RECORD_DIET=0
    for gamma in (1.0, 1.5, 3.0, 2.0000000000000004, 1.9999999999999998, -2.0):
        for diet in (0, 1):
            assert spec(4, gamma, diet, "1") == (4, 0), (gamma, diet)
            assert spec(4, gamma, diet) == (0, 0), (gamma, diet)
    assert spec(3, 2.0, 1, "1") == (0, 1) and spec(3, 1.5, 0, "1") == (0, 0)


def test_the_knob_switches_each_half(spec):
    for knob, (ne_on, crra_on) in {None: (0, 1), "1": (1, 1), "0": (0, 0), "ne": (1, 0), "crra": (0, 1)}.items():
        assert spec(11, 2.0, 1, knob) == (11 * ne_on, crra_on), knob
        assert spec(7, 2.0, 1, knob) == (7 * ne_on, crra_on), knob
        assert spec(5, 3.0, 1, knob) == (0, 0), knob       # nothing to switch on
        assert spec(4, 1.5, 0, knob) == (4 * ne_on, 0), knob
    for knob in ("off", "NE", "2", "crra ", "10"):         # not one of the four words: the default, never the costlier NE half
        assert spec(11, 2.0, 1, knob) == (0, 1), knob
