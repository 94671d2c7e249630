"""The lane geometry of the tangent kernels and of the transposed ones at a batch width has ONE definition, hank_geom.h (tan_geom,
adj_geom), which build_tanwork, build_cotwork, ss_jvp and ss_vjp (hank_hip.hip) all call. Plain integers in a header without device
code: compiled alone by the host compiler here, no GPU and no library, and compared with a Python mirror written from
build_tanwork's loop and with cases.adj_rows_per_block (what the GPU tests size their economies by)."""
import shutil
import subprocess
from pathlib import Path

import pytest

import cases

CSRC = Path(__file__).resolve().parent.parent / "julia-newtonraphsonhank_amd" / "csrc"
N_A = (30, 50, 63, 64, 65)
MAIN = """#include "hank_geom.h"
#include <cstdio>
#include <cstdlib>
int main(int argc, char **argv) {      // questions on the command line: t n_a N V | a n_a M; one line of integers per answer
    for (int i = 1; i < argc;) {
        if (argv[i][0] == 't' && i + 3 < argc) {
            const hank::TanGeom g = hank::tan_geom(atoi(argv[i + 1]), atoi(argv[i + 2]), atoi(argv[i + 3]));
            printf("%d %d %d %d %d\\n", g.N, g.NC, g.lgNC, g.nbx, g.ss);
            i += 4;
        } else if (argv[i][0] == 'a' && i + 2 < argc) {
            const hank::AdjGeom g = hank::adj_geom(atoi(argv[i + 1]), atoi(argv[i + 2]));
            printf("%d %d %d %d %d %d\\n", g.MV, g.NC, g.lgNC, g.R, g.nb, hank::adj_lane_width(atoi(argv[i + 2])));
            i += 3;
        } else {
            return 2;
        }
    }
    return 0;
}
"""


@pytest.fixture(scope="module")
def ask(tmp_path_factory):
    """hank_geom.h compiled ALONE by the host compiler (it is plain C++: no HIP, no library) into a program that answers."""
    cxx = next((c for c in (shutil.which("c++"), shutil.which("g++"), shutil.which("clang++"), "/opt/rocm/lib/llvm/bin/clang++") if c and Path(c).exists()), None)
    assert cxx, "no host C++ compiler"
    d = tmp_path_factory.mktemp("geom")
    (d / "main.cpp").write_text(MAIN)
    subprocess.run([cxx, "-std=c++17", "-O1", "-Wall", "-Werror", "-I", str(CSRC), "-o", str(d / "geom"), str(d / "main.cpp")], check=True, capture_output=True, timeout=120)

    def run(questions):
        """[(kind, ints...)] -> one list of ints per question"""
        args = [str(v) for q in questions for v in q]
        out = subprocess.run([str(d / "geom")] + args, check=True, capture_output=True, text=True, timeout=30).stdout.splitlines()
        assert len(out) == len(questions)
        return [[int(v) for v in l.split()] for l in out]
    return run


def tan_mirror(n_a, N, V):
    """build_tanwork's loop: N / V lanes of directions, NC of them (a power of two <= 64) across a wave, 64 / NC rows per instruction"""
    NV = N // V
    NC, lg = 1, 0
    while NC < NV and NC < 64:
        NC, lg = NC * 2, lg + 1
    RB = 64 // NC
    return [NV, NC, lg, (n_a + RB - 1) // RB, 0]


def test_tan_geom_matches_the_mirror_at_every_width(ask):
    qs = [("t", n_a, N, V) for n_a in N_A for V in (1, 2) for N in range(1, 71) if N % V == 0]
    assert len(qs) == len(N_A) * (70 + 35)
    for q, got in zip(qs, ask(qs)):
        assert got == tan_mirror(*q[1:]), q
        NV, NC, lg, nbx, _ = got
        assert NC == 1 << lg and (NC >= NV or NC == 64) and (NC == 1 or NC // 2 < NV)
        assert (nbx - 1) * (64 // NC) < q[1] <= nbx * (64 // NC)          # the row blocks cover n_a, none is empty


def test_adj_geom_rows_per_block_are_the_tests(ask):
    qs = [("a", n_a, M) for n_a in N_A for M in range(1, 71)]
    for q, (MV, NC, lg, R, nb, V) in zip(qs, ask(qs)):
        _, n_a, M = q
        assert R == cases.adj_rows_per_block(M), q
        assert V == (2 if M % 2 == 0 else 1) and MV * V == M
        assert NC == 1 << lg and NC <= 16 and (NC >= MV or NC == 16) and (NC == 1 or NC // 2 < MV)
        assert R == max(64 // NC, 8) and R + 2 <= 3 * (64 // NC)          # (ADJ_KS = 3 row slots per lane hold the tile)
        assert nb == (n_a + R - 1) // R


# what tests/test_gpu_ss_diff.py says its widths reach in hank_ss_jvp / hank_ss_vjp (rows per wave instruction RB = 64 / NC):
# JVP N -> (columns per lane V, NC, RB, blocks in y); the forward step is the source-stationary form where NC >= 16 (ss_jvp)
SS_JVP_TABLE = {2: (2, 1, 64, 1), 7: (1, 8, 8, 1), 16: (2, 8, 8, 1), 9: (1, 16, 4, 1), 18: (2, 16, 4, 1), 32: (2, 16, 4, 1), 34: (2, 32, 2, 1),
                65: (1, 64, 1, 2), 130: (2, 64, 1, 2)}
# VJP M -> (V, NC, RB, rows per block R, blocks in y)
SS_VJP_TABLE = {2: (2, 1, 64, 64, 1), 3: (1, 4, 16, 16, 1), 7: (1, 8, 8, 8, 1), 16: (2, 8, 8, 8, 1), 32: (2, 16, 4, 8, 1), 34: (2, 16, 4, 8, 2)}
SS_SOURCE_STATIONARY = {2: False, 7: False, 16: False, 9: True, 18: True, 32: True, 34: True, 65: True, 130: True}
SS_XCDMAP_FWD_MAXN = 32          # HANK_XCDMAP_FWD_MAXN: the forward step remaps its blocks while N * (columns per lane) stays below


def test_ss_diff_widths_reach_the_geometries_they_name(ask):
    """if the geometry rule moves, the GPU tests cannot silently stop reaching what they claim: every width of the two tables at
    the row counts of their economies (190, 30, 40)"""
    import re
    for n_a in (190, 30, 40):
        for N, (V, NC, RB, ny) in SS_JVP_TABLE.items():
            assert V == (2 if N % 2 == 0 else 1)                      # ss_jvp's choice of lanes
            (NV, gNC, lg, nbx, _), = ask([("t", n_a, N, V)])
            assert (gNC, 64 // gNC, (NV + gNC - 1) // gNC) == (NC, RB, ny), (n_a, N)
            assert nbx == (n_a + RB - 1) // RB and NV * V == N
            assert (gNC >= 16) == SS_SOURCE_STATIONARY[N], N         # gf.ss of ss_jvp
        for M, (V, NC, RB, R, ny) in SS_VJP_TABLE.items():
            (MV, gNC, lg, gR, nb, gV), = ask([("a", n_a, M)])
            assert (gV, gNC, 64 // gNC, gR, (MV + gNC - 1) // gNC) == (V, NC, RB, R, ny), (n_a, M)
            assert nb == (n_a + R - 1) // R
    # the widths' notes: lanes in use, the block map, the slot trips
    assert SS_JVP_TABLE[7][1] - 7 == 1 and 16 // 2 == SS_JVP_TABLE[16][1] and 18 // 2 == 9 < SS_JVP_TABLE[18][1] and 32 // 2 == SS_JVP_TABLE[32][1]
    src = (CSRC / "hank_device.h").read_text() + (CSRC / "hank_hip.hip").read_text()
    assert int(re.search(r"#define\s+HANK_XCDMAP_FWD_MAXN\s+(\d+)", src).group(1)) == SS_XCDMAP_FWD_MAXN
    assert re.search(r"gf\.ss = g\.NC >= 16 \? 1 : 0;", src), "ss_jvp no longer takes the source-stationary form at NC >= 16"
    on = {N: N <= SS_XCDMAP_FWD_MAXN for N in SS_JVP_TABLE}          # g.N * sizeof(VT) / 8 = N
    assert [N for N in SS_JVP_TABLE if on[N] and SS_SOURCE_STATIONARY[N]] == [9, 18, 32] and not on[34]
    # regular blocks of the block-mapped source-stationary step (RB = 4, two row groups per block) on the three economies: a
    # multiple of the 8 XCDs (`clamp`: 24) and two counts below 8 (4, 5); the gather form at RB = 16 (N = 3, 4) gives `clamp` 12
    assert [(((n_a + 3) // 4) + 1) // 2 for n_a in (190, 30, 40)] == [24, 4, 5] and (190 + 15) // 16 == 12
    R, RB = SS_VJP_TABLE[7][3], SS_VJP_TABLE[7][2]
    assert R + 2 == 10 and -(-(R + 2) // RB) == 2                     # M = 7: NS = 10 slots, two trips of RB = 8
    assert 65 - SS_JVP_TABLE[65][1] == 1 and 130 // 2 - SS_JVP_TABLE[130][1] == 1 and 34 // 2 - SS_VJP_TABLE[34][1] == 1   # one live lane in the second block


LAUNCH_LANES = {129: (1, 129), 256: (2, 128), 130: (2, 65)}      # tests/test_gpu_launch_lanes.py's widths -> (directions per lane, NV)
TAN_RG_BACK_4 = 128              # tan_rg: 4 backward row groups per wave from this many lanes of directions on


def test_launch_lane_widths_straddle_the_row_group_threshold(ask):
    """tests/test_gpu_launch_lanes.py's three widths give g.N = 129, 128 and 65 at its row counts, and tan_rg's threshold is still
    128: two widths at and above it (one per lane type), one below. If the threshold moves, move LANES there (and this table) so
    that an odd and an even width sit at or just above it and one even width below."""
    import re
    src = (CSRC / "hank_hip.hip").read_text()
    m = re.search(r"static inline int tan_rg\(int NV, int forward, int ss = 0\) \{.*?\n\}", src, re.S)
    assert m, "tan_rg has moved"
    assert re.search(r"return \(want == 2 && N % 2 == 0\) \? 2 : 1;", src), "tan_lane_width no longer takes two directions per lane for an even N"
    rule = re.search(r"return forward \? \(\(NV >= 32 \|\| ss\) \? 2 : 1\) : \(NV >= (\d+) \? 4 : 2\);", m.group(0))
    assert rule and int(rule.group(1)) == TAN_RG_BACK_4, "tan_rg's rule has moved: move tests/test_gpu_launch_lanes.py's widths with it"
    assert "tan_rg(w.g.N, 0)" in src and "tan_rg(w.gf.N, 1, w.gf.ss)" in src          # build_tanwork asks with g.N
    for n_a in (37, 50, 40):
        for N, (V, NV) in LAUNCH_LANES.items():
            assert V == (2 if N % 2 == 0 else 1)
            (gN, NC, lg, nbx, _), = ask([("t", n_a, N, V)])
            assert gN == NV and NC == 64 and nbx == n_a, (n_a, N, gN, NC, nbx)      # one row per wave instruction
    NVs = sorted(NV for _, NV in LAUNCH_LANES.values())
    assert NVs[0] < TAN_RG_BACK_4 <= NVs[1] and NVs[0] >= 32                          # (the control keeps 2 forward row groups as well)
    assert 37 % 4 != 0 and 37 % 2 != 0                                                # a ragged last block at 4 and at 2 row groups


def test_fake_news_shapes_reach_what_they_name():
    """tests/test_gpu_fake_news_dense.py's shapes against fake_news()'s launch arithmetic restated in fake_news_refs.geometry, and
    that restatement against the source: if a tile, the K split or a block size moves, the GPU module cannot silently stop reaching
    the edges its table names"""
    import re
    import fake_news_refs as R
    for name, P in R.SHAPES:
        R.check_shape(name, P)
    # the claims of the table that are sentences rather than entries
    g = R.geometry(90, 2, 3, 7)
    assert g["slices"][5] == 10 and g["kchunk"] == 16 and not any(g["slices"][6:])          # slice 5: 10 of 16 k
    g = R.geometry(380, 2, 3, 12)
    assert g["slices"][11] == 16 + 12 and g["slices"][11] < g["kchunk"]                      # one full 16-chunk plus 12
    g = R.geometry(640, 2, 3, 12)
    assert g["slices"].count(48) == 13 and g["slices"][13] == 16 and g["slices"].count(0) == 2
    g = R.geometry(256, 2, 3, 16)
    assert set(g["slices"]) == {R.GEMM_KSTEP} and g["expect"] == (1, R.BLOCK)
    assert R.geometry(100, 2, 3, 32)["gemm_n"][1] == R.GEMM_TILE and R.geometry(100, 2, 3, 32)["transpose_t"][1] == R.TRANSPOSE_TILE
    assert R.geometry(90, 3, 4, 100)["gemm_m"] == (7, 400 - 6 * 64)
    n_e = {n: e for n, (_, e, _, _) in R.ECONOMIES.items()}
    assert n_e["ks40x16"] == 16 and n_e["ks40x5"] == 5 and max(n_e.values()) == 16           # k_fn_impulse keeps double mid[16]
    # ... and the source
    host, jac = (CSRC / "hank_hip.hip").read_text(), (CSRC / "hank_jacobian.h").read_text()
    body = host[host.index("static int fake_news("):host.index("int hank_fake_news(")]
    assert re.search(r"NP = P \* N, S = 16,", body) and R.FN_SLICES == 16
    assert "const int kchunk = ((G + S - 1) / S + 15) / 16 * 16, MP = nh * P;" in body
    assert "(G + 31) / 32), (unsigned)((P + 31) / 32), (unsigned)N), dim3(256)" in body and "tile[32][33]" in jac
    assert body.count("(NP + 63) / 64)") == 2 and "(MP + 63) / 64)" in body and "(nh + 63) / 64)" in body
    assert "As[16][68], Bs[16][64]" in jac and "k0 += 16" in jac
    assert "dim3((unsigned)c.n_a, (unsigned)((NP + 255) / 256)), dim3(256)" in body and "blockIdx.y * 256 + threadIdx.x" in jac
    assert body.count("(G + 255) / 256)") == 2 and "double mid[16];" in jac
